// pt_bloom_layout and pt_bloom_planes: the bloom pyramid of every view in caller memory — source and first down step (k_bloom_down1), the
// large levels (k_bloom_down, k_bloom_up), the small ones (k_bloom_tail) and the composite (k_bloom_composite).  Part of pt_lib.hip.
#include "pt_bloom.h"

// The level at which k_bloom_tail takes over: the first level from 2 on that has at most this many texels in every view (none: the
// per-level kernels do it all).  One workgroup has one CU's vector cache behind it: a down texel costs it about 4 clocks of 64 bytes, an
// up texel a good one, so the tail pays for itself only where a level is smaller than a launch gap is long.  Measured at 1080p with 6
// levels (profiles/bloom.md: no tail, 1 Ki, 2 Ki, 16 Ki and 32 Ki side by side).  PT_BLOOM_TAIL_TEXELS overrides it for such a
// measurement (tools/bloom_bench.py) and for nothing else: the result does not depend on it.
#define BLOOM_TAIL_TEXELS 1024u
static uint32_t bloom_tail_texels() {
    const char* e = getenv("PT_BLOOM_TAIL_TEXELS");
    return e && *e ? (uint32_t)strtoul(e, nullptr, 10) : BLOOM_TAIL_TEXELS;
}

// The rectangles (each view's, or the frame) and their levels: tab is [nv][BLOOM_STRIDE], entries past `levels` zero.  Returns the
// pyramid's size in float4.
static uint64_t bloom_table(const pt_ctx* ctx, uint32_t levels, std::vector<BloomLevel>& tab) {
    const std::vector<PassRect> rects = pass_rects(ctx);
    tab.assign(rects.size() * BLOOM_STRIDE, BloomLevel{0u, 0u, 0u, 0u});
    uint64_t at = 0;
    for (size_t v = 0; v < rects.size(); ++v) {
        BloomLevel* t = tab.data() + v * BLOOM_STRIDE;
        t[0] = BloomLevel{rects[v].w, rects[v].h, 0u, pass_rect_org(rects[v])};
        for (uint32_t k = 1; k <= levels; ++k) {
            t[k] = BloomLevel{(t[k - 1].w + 1u) / 2u, (t[k - 1].h + 1u) / 2u, (uint32_t)at, 0u};
            at += (uint64_t)t[k].w * t[k].h;
        }
    }
    return at;
}

extern "C" int pt_bloom_layout(const pt_ctx* cctx, uint32_t levels, uint32_t* dims, size_t* bytes) {
    if (!cctx) return fail(nullptr, PT_ERR_INVALID, "pt_bloom_layout: null context");
    pt_ctx* ctx = const_cast<pt_ctx*>(cctx); // (the error text only)
    if (!bytes) return fail(ctx, PT_ERR_INVALID, "pt_bloom_layout: bytes is null");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_bloom_layout: no frame size yet (pt_resize)");
    if (levels < 1u || levels > PT_BLOOM_MAX_LEVELS) return fail(ctx, PT_ERR_INVALID, ("pt_bloom_layout: levels must be 1.." + std::to_string(PT_BLOOM_MAX_LEVELS) + ", not " + std::to_string(levels)).c_str());
    std::vector<BloomLevel> tab;
    const uint64_t texels = bloom_table(ctx, levels, tab);
    if (texels > 0xffffffffull) return fail(ctx, PT_ERR_UNSUPPORTED, "pt_bloom_layout: the pyramid has more than 2^32 - 1 texels");
    if (dims) {
        const uint32_t nv = pass_camera_count(ctx);
        for (uint32_t v = 0; v < nv; ++v)
            for (uint32_t k = 1; k <= PT_BLOOM_MAX_LEVELS; ++k) {
                const BloomLevel& L = tab[(size_t)v * BLOOM_STRIDE + k];
                uint32_t* d = dims + 4 * ((size_t)v * PT_BLOOM_MAX_LEVELS + (k - 1u));
                d[0] = L.w, d[1] = L.h, d[2] = L.off, d[3] = 0u;
            }
    }
    *bytes = (size_t)texels * 16;
    return PT_OK;
}

extern "C" int pt_bloom_planes(pt_ctx* ctx, const pt_bloom_desc* desc, pt_bloom_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_bloom_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_bloom_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_bloom_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_bloom_planes: ";
    if (desc->flags != 0u) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags)).c_str());
    if (desc->levels < 1u || desc->levels > PT_BLOOM_MAX_LEVELS)
        return fail(ctx, PT_ERR_INVALID, (fn + "levels must be 1.." + std::to_string(PT_BLOOM_MAX_LEVELS) + ", not " + std::to_string(desc->levels)).c_str());
    if (!std::isfinite(desc->exposure) || !(desc->exposure > 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "exposure must be finite and > 0").c_str());
    if (!std::isfinite(desc->threshold) || !(desc->threshold >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "threshold must be finite and >= 0").c_str());
    if (!std::isfinite(desc->knee) || !(desc->knee >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "knee must be finite and >= 0").c_str());
    if (!std::isfinite(desc->clamp) || !(desc->clamp > 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "clamp must be finite and > 0").c_str());
    if (!(desc->spread >= 0.f && desc->spread <= 1.f)) return fail(ctx, PT_ERR_INVALID, (fn + "spread must be in [0,1]").c_str());
    if (!std::isfinite(desc->intensity) || !(desc->intensity >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "intensity must be finite and >= 0").c_str());
    const uint32_t levels = desc->levels;
    std::vector<BloomLevel> tab;
    const uint64_t texels = bloom_table(ctx, levels, tab);
    if (texels > 0xffffffffull) return fail(ctx, PT_ERR_UNSUPPORTED, (fn + "the pyramid has more than 2^32 - 1 texels").c_str());
    const size_t npix = (size_t)ctx->width * ctx->height;
    const uint32_t nv = pass_camera_count(ctx);
    // exclusive: may overlap no other plane (the two written ones) — except that out may be exactly color: the pyramid is complete before
    // the composite writes its first pixel, and a pixel of the composite reads its own colour alone
    const PassPlane planes[4] = {{"color", desc->color, npix * 16, true, false},
                                 {"state", desc->state, (size_t)nv * 16, false, false},
                                 {"out", desc->out, npix * 16, true, true},
                                 {"scratch", desc->scratch, (size_t)texels * 16, true, true}};
    int rc = pass_planes_check(ctx, "pt_bloom_planes", planes, 4, 0, 2);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(desc->scratch) & 15u) return fail(ctx, PT_ERR_INVALID, (fn + "scratch is not 16-byte aligned").c_str());
    // n = 1; repeat levels - 1 times: n = n * spread + 1 — float32, one rounding per operation (the host's flags forbid contraction, too)
    float nsum = 1.0f;
    for (uint32_t k = 1; k < levels; ++k) nsum = nsum * desc->spread + 1.0f;
    const float a = desc->intensity * (1.0f / nsum);
    uint64_t sources = 0;
    uint32_t tiles = 0; // of k_bloom_down1, the largest view's
    for (uint32_t v = 0; v < nv; ++v) {
        const BloomLevel *L0 = &tab[(size_t)v * BLOOM_STRIDE], *L1 = L0 + 1;
        sources += (uint64_t)L0->w * L0->h;
        tiles = std::max(tiles, ((L1->w + BLOOM_TW - 1u) / BLOOM_TW) * ((L1->h + BLOOM_TH - 1u) / BLOOM_TH));
    }
    auto level_texels = [&](uint32_t k) { // the largest view's
        uint32_t m = 0;
        for (uint32_t v = 0; v < nv; ++v) m = std::max(m, tab[(size_t)v * BLOOM_STRIDE + k].w * tab[(size_t)v * BLOOM_STRIDE + k].h);
        return m;
    };
    const uint32_t cut = bloom_tail_texels();
    uint32_t first = levels + 1u; // the tail's first level; levels + 1: no tail
    for (uint32_t k = 2; k <= levels; ++k)
        if (level_texels(k) <= cut) {
            first = k;
            break;
        }
    PassRun run;
    rc = run.open(ctx, "pt_bloom_planes", PASS_SLOT_BYTES); // per slot: bright, nonfinite
    if (rc) return rc;
    BloomLevel* d_tab = nullptr;
    CK(run.tmp.alloc(&d_tab, tab.size()));
    CK(hipMemcpyAsync(d_tab, tab.data(), sizeof(BloomLevel) * tab.size(), hipMemcpyHostToDevice, ctx->stream)); // (tab lives until the call has waited)
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    float4* scratch = reinterpret_cast<float4*>(desc->scratch);
    const BloomSourceArgs sa{d_tab, ctx->width, desc->color, desc->state, scratch, desc->exposure, desc->threshold, desc->knee, desc->clamp, run.counts()};
    hipLaunchKernelGGL(k_bloom_down1, dim3(tiles, nv), dim3(256), 0, ctx->stream, sa);
    const uint32_t per_level_end = first <= levels ? first - 1u : levels; // the last level of the per-level kernels
    for (uint32_t k = 2; k <= per_level_end; ++k)
        hipLaunchKernelGGL(k_bloom_down, dim3((level_texels(k) + 255u) / 256u, nv), dim3(256), 0, ctx->stream, BloomLevelArgs{d_tab, scratch, k, desc->spread});
    if (first <= levels) hipLaunchKernelGGL(k_bloom_tail, dim3(nv), dim3(BLOOM_TAIL_THREADS), 0, ctx->stream, BloomTailArgs{d_tab, scratch, first, levels, desc->spread});
    // the up steps the tail did not do: levels - 1 .. 1 without it, first - 2 .. 1 behind it
    for (uint32_t k = (first <= levels ? first - 1u : levels) - 1u; k >= 1u; --k)
        hipLaunchKernelGGL(k_bloom_up, dim3((level_texels(k) + 255u) / 256u, nv), dim3(256), 0, ctx->stream, BloomLevelArgs{d_tab, scratch, k, desc->spread});
    if (n != 0) {
        const BloomCompositeArgs ca{run.pixels, n, ctx->width, ctx->height, desc->color, desc->out, d_tab, scratch, a};
        PASS_LAUNCH(run, (n + 255u) / 256u, 256, ca, k_bloom_composite);
    }
    unsigned long long sum[2] = {};
    rc = run.close_slots(sum, 2);
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->sources = sources;
        stats->bright = sum[0];
        stats->nonfinite = sum[1];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}
