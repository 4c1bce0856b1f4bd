// pt_ao_layout and pt_ao_planes: ambient occlusion from the G-buffer's hit and position planes over the context's current tree.  Per batch of
// the call's pixel list: k_ao_rays, the any-hit traversal exactly as pt_trace_device launches it, k_ao_reduce.  Part of pt_lib.hip.
#include "pt_ao.h"

// rays and max_rays_in_flight as both entry points refuse them; *batch_pixels: floor(M / rays), at most the frame's pixels
static int ao_batch(pt_ctx* ctx, const std::string& fn, uint32_t rays, uint32_t max_rays_in_flight, uint64_t* batch_pixels) {
    if (rays < 1u || rays > (uint32_t)PT_AO_MAX_RAYS) return fail(ctx, PT_ERR_INVALID, (fn + "rays must be 1.." + std::to_string(PT_AO_MAX_RAYS) + ", not " + std::to_string(rays)).c_str());
    if (max_rays_in_flight != 0u && max_rays_in_flight < rays)
        return fail(ctx, PT_ERR_INVALID, (fn + "max_rays_in_flight is " + std::to_string(max_rays_in_flight) + ", below rays (" + std::to_string(rays) + ")").c_str());
    const uint64_t M = max_rays_in_flight ? max_rays_in_flight : (uint64_t)PT_AO_DEFAULT_RAYS_IN_FLIGHT;
    *batch_pixels = std::min<uint64_t>(M / rays, (uint64_t)ctx->width * ctx->height);
    return PT_OK;
}

extern "C" int pt_ao_layout(const pt_ctx* cctx, uint32_t rays, uint32_t max_rays_in_flight, size_t* bytes) {
    if (!cctx) return fail(nullptr, PT_ERR_INVALID, "pt_ao_layout: null context");
    pt_ctx* ctx = const_cast<pt_ctx*>(cctx); // (the error text only)
    if (!bytes) return fail(ctx, PT_ERR_INVALID, "pt_ao_layout: bytes is null");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_ao_layout: no frame size yet (pt_resize)");
    uint64_t bp = 0;
    const int rc = ao_batch(ctx, "pt_ao_layout: ", rays, max_rays_in_flight, &bp);
    if (rc) return rc;
    *bytes = ao_scratch_bytes(bp, rays);
    return PT_OK;
}

extern "C" int pt_ao_planes(pt_ctx* ctx, const pt_ao_desc* desc, pt_ao_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_ao_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_ao_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_ao_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_ao_planes: ";
    if (desc->flags & ~(uint32_t)PT_AO_JITTER) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags & ~(uint32_t)PT_AO_JITTER)).c_str());
    uint64_t bp64 = 0;
    int rc = ao_batch(ctx, fn, desc->rays, desc->max_rays_in_flight, &bp64);
    if (rc) return rc;
    if (!std::isfinite(desc->radius) || !(desc->radius > 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "radius must be finite and > 0").c_str());
    if (!std::isfinite(desc->bias) || !(desc->bias >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "bias must be finite and >= 0").c_str());
    if (!desc->ao && !desc->out && !desc->bent) return fail(ctx, PT_ERR_INVALID, (fn + "no output asked for (ao, out and bent are all null)").c_str());
    if (desc->scratch && (reinterpret_cast<uintptr_t>(desc->scratch) & 15u)) return fail(ctx, PT_ERR_INVALID, (fn + "scratch is not 16-byte aligned").c_str());
    const uint32_t bp = (uint32_t)bp64, rays = desc->rays;
    const size_t npix = (size_t)ctx->width * ctx->height;
    const PassPlane planes[6] = {{"hit", desc->hit, npix * 32, true, false},     {"position", desc->position, npix * 16, true, false},
                                 {"ao", desc->ao, npix * 4, false, true},        {"out", desc->out, npix * 16, false, true},
                                 {"bent", desc->bent, npix * 16, false, true},   {"scratch", desc->scratch, ao_scratch_bytes(bp, rays), true, true}};
    rc = pass_planes_check(ctx, "pt_ao_planes", planes, 6);
    if (rc) return rc;
    AoTaps tt;
    pass_spiral(tt.D);
    const float frays = (float)rays;
    for (uint32_t k = 0; k < (uint32_t)PT_AO_MAX_RAYS; ++k) tt.rho[k] = k < rays ? sqrtf(((float)k + 0.5f) / frays) : 0.0f;
    PassRun run;
    rc = run.open(ctx, "pt_ao_planes", PASS_SLOT_BYTES); // per slot: skipped, nonfinite, invalid, occluded
    if (rc) return rc;
    const AoScratch sc = ao_scratch(desc->scratch, bp, rays);
    AoTaps* d_tt = nullptr;
    CK(run.tmp.alloc(&d_tt, 1));
    CK(hipMemcpyAsync(d_tt, &tt, sizeof(AoTaps), hipMemcpyHostToDevice, ctx->stream)); // (tt lives until the call has waited)
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    const uint32_t batches = n ? (n + bp - 1u) / bp : 0u;
    std::vector<hipEvent_t> ev(2 * (size_t)batches);
    for (hipEvent_t& e : ev) CK(run.tmp.event(&e));
    uint32_t h_fault = 0;
    if (n != 0) {
        CK(hipMemsetAsync(sc.count, 0, AO_HEAD_BYTES, ctx->stream)); // count, chunk counter and fault word; between batches k_ao_reduce clears the first two
        for (uint32_t b = 0; b < batches; ++b) {
            const uint32_t first = b * bp, nb = std::min(bp, n - first);
            const AoArgs aa{run.pixels + first, nb, ctx->width, ctx->height, reinterpret_cast<const float*>(desc->hit), desc->position, desc->ao, desc->out, desc->bent, sc, d_tt, ctx->eye, rays,
                            desc->radius, desc->bias, desc->seed, desc->flags & (uint32_t)PT_AO_JITTER, run.counts()};
            PASS_LAUNCH(run, (nb + AO_GROUP - 1u) / AO_GROUP, 256, aa, k_ao_rays);
            CK(hipEventRecord(ev[2 * b], ctx->stream));
            PathState st{};
            st.rayO = sc.rayO;
            st.rayD = sc.rayD;
            st.hit = sc.hit;
            Trace8Args ta{st, bvh_dev(ctx), QView{nullptr, sc.count, 0}, QView{}, sc.work, ctx->ovf, 0, nullptr, 0, ctx->lds_skip, ctx->ovf_depth, sc.fault, ctx->bvh.num_nodes8};
            hipLaunchKernelGGL((k_trace8<TR_ANY_QUERY>), dim3(ctx->trace_grid), dim3(64), 0, ctx->stream, ta);
            CK(hipEventRecord(ev[2 * b + 1], ctx->stream));
            hipLaunchKernelGGL(k_ao_reduce, dim3((nb + 255u) / 256u), dim3(256), 0, ctx->stream, aa); // (clears the count and the chunk counter for the next batch)
        }
        CK(hipMemcpyAsync(&h_fault, sc.fault, 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    unsigned long long sum[4] = {};
    rc = run.close_slots(sum, 4);
    if (rc) return rc;
    if (h_fault & 1u) return fail(ctx, PT_ERR_UNSUPPORTED, "pt_ao_planes: traversal stack overflow: the acceleration structure is deeper than the traversal stack");
    double trace_ms = 0.0;
    for (uint32_t b = 0; b < batches; ++b) {
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, ev[2 * b], ev[2 * b + 1]));
        trace_ms += ms;
    }
    if (stats) {
        stats->pixels = n;
        stats->skipped = sum[0];
        stats->nonfinite = sum[1];
        stats->traced = n - sum[0] - sum[1];
        stats->invalid = sum[2];
        stats->rays = stats->traced * rays - sum[2];
        stats->occluded = sum[3];
        stats->batches = batches;
        stats->kernel_ms = run.ms;
        stats->trace_ms = trace_ms;
    }
    return PT_OK;
}
