// pt_shadow_layout and pt_shadow_planes: shadows and direct light of up to four distant disc lights from the G-buffer's hit and position
// planes over the context's current tree.  Per batch of the call's pixel list: k_shadow_rays, the any-hit traversal exactly as
// pt_trace_device launches it, k_shadow_reduce.  Part of pt_lib.hip.
#include "pt_shadow.h"

// the lights' ray counts and max_rays_in_flight as both entry points refuse them; *R: the sum of the rays; *batch_pixels: floor(M / R), at
// most the frame's pixels
static int shadow_batch(pt_ctx* ctx, const std::string& fn, const pt_shadow_light* lights, uint32_t num_lights, uint32_t max_rays_in_flight, uint32_t* R, uint64_t* batch_pixels) {
    if (num_lights < 1u || num_lights > (uint32_t)PT_SHADOW_MAX_LIGHTS)
        return fail(ctx, PT_ERR_INVALID, (fn + "num_lights must be 1.." + std::to_string(PT_SHADOW_MAX_LIGHTS) + ", not " + std::to_string(num_lights)).c_str());
    if (!lights) return fail(ctx, PT_ERR_INVALID, (fn + "lights is null").c_str());
    uint64_t sum = 0;
    for (uint32_t i = 0; i < num_lights; ++i) {
        if (lights[i].rays == 0u) return fail(ctx, PT_ERR_INVALID, (fn + "light " + std::to_string(i) + ": rays must be >= 1").c_str());
        sum += lights[i].rays;
    }
    if (sum > (uint64_t)PT_SHADOW_MAX_RAYS)
        return fail(ctx, PT_ERR_INVALID, (fn + "the lights' rays add up to " + std::to_string(sum) + ", above " + std::to_string(PT_SHADOW_MAX_RAYS)).c_str());
    if (max_rays_in_flight != 0u && max_rays_in_flight < sum)
        return fail(ctx, PT_ERR_INVALID, (fn + "max_rays_in_flight is " + std::to_string(max_rays_in_flight) + ", below the lights' rays (" + std::to_string(sum) + ")").c_str());
    const uint64_t M = max_rays_in_flight ? max_rays_in_flight : (uint64_t)PT_SHADOW_DEFAULT_RAYS_IN_FLIGHT;
    *R = (uint32_t)sum;
    *batch_pixels = std::min<uint64_t>(M / sum, (uint64_t)ctx->width * ctx->height);
    return PT_OK;
}

// L = normalize3(dir) and pt_ao_planes's step-4 frame around it, in the header's float32 statements (the build does not contract them);
// false: dir has no direction
static bool shadow_light_dev(const pt_shadow_light& l, ShadowLightDev* out) {
    const float x = l.dir[0], y = l.dir[1], z = l.dir[2];
    const float xx = x * x, yy = y * y, zz = z * z;
    const float s = (xx + yy) + zz;
    const float inv = 1.0f / sqrtf(s);
    const float nx = x * inv, ny = y * inv, nz = z * inv;
    const float lx = nx * nx, ly = ny * ny, lz = nz * nz;
    const float ll = (lx + ly) + lz;
    if (!std::isfinite(nx) || !std::isfinite(ny) || !std::isfinite(nz) || !(ll > 0.5f)) return false;
    const float sg = nz >= 0.0f ? 1.0f : -1.0f;
    const float fa = -1.0f / (sg + nz);
    const float fb = (nx * ny) * fa;
    out->L = v3{nx, ny, nz};
    out->T = v3{1.0f + (sg * lx) * fa, sg * fb, (-sg) * nx};
    out->B = v3{fb, sg + ly * fa, -ny};
    out->spread = l.spread;
    out->rays = l.rays;
    return true;
}

extern "C" int pt_shadow_layout(const pt_ctx* cctx, const pt_shadow_light* lights, uint32_t num_lights, uint32_t max_rays_in_flight, size_t* bytes) {
    if (!cctx) return fail(nullptr, PT_ERR_INVALID, "pt_shadow_layout: null context");
    pt_ctx* ctx = const_cast<pt_ctx*>(cctx); // (the error text only)
    if (!bytes) return fail(ctx, PT_ERR_INVALID, "pt_shadow_layout: bytes is null");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_shadow_layout: no frame size yet (pt_resize)");
    uint32_t R = 0;
    uint64_t bp = 0;
    const int rc = shadow_batch(ctx, "pt_shadow_layout: ", lights, num_lights, max_rays_in_flight, &R, &bp);
    if (rc) return rc;
    *bytes = shadow_scratch_bytes(bp, R);
    return PT_OK;
}

extern "C" int pt_shadow_planes(pt_ctx* ctx, const pt_shadow_desc* desc, pt_shadow_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_shadow_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_shadow_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_shadow_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_shadow_planes: ";
    if (desc->flags & ~(uint32_t)PT_SHADOW_JITTER) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags & ~(uint32_t)PT_SHADOW_JITTER)).c_str());
    uint32_t R = 0;
    uint64_t bp64 = 0;
    int rc = shadow_batch(ctx, fn, desc->lights, desc->num_lights, desc->max_rays_in_flight, &R, &bp64);
    if (rc) return rc;
    const uint32_t nl = desc->num_lights;
    ShadowLightDev lights[PT_SHADOW_MAX_LIGHTS] = {};
    v3 radiance[PT_SHADOW_MAX_LIGHTS] = {};
    ShadowTaps tt = {};
    pass_spiral(tt.D);
    uint32_t at = 0;
    for (uint32_t i = 0; i < nl; ++i) {
        const pt_shadow_light& l = desc->lights[i];
        const std::string li = fn + "light " + std::to_string(i) + ": ";
        if (!std::isfinite(l.dir[0]) || !std::isfinite(l.dir[1]) || !std::isfinite(l.dir[2])) return fail(ctx, PT_ERR_INVALID, (li + "dir is not finite").c_str());
        if (!shadow_light_dev(l, &lights[i])) return fail(ctx, PT_ERR_INVALID, (li + "dir cannot be normalised").c_str());
        if (!std::isfinite(l.spread) || !(l.spread >= 0.f) || !(l.spread <= 1.f)) return fail(ctx, PT_ERR_INVALID, (li + "spread must be finite and in [0, 1]").c_str());
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(l.radiance[c]) || !(l.radiance[c] >= 0.f)) return fail(ctx, PT_ERR_INVALID, (li + "radiance must be finite and >= 0").c_str());
        radiance[i] = v3{l.radiance[0], l.radiance[1], l.radiance[2]};
        lights[i].rho0 = at;
        const float frays = (float)l.rays;
        for (uint32_t k = 0; k < l.rays; ++k) tt.rho[at + k] = sqrtf(((float)k + 0.5f) / frays);
        at += l.rays;
    }
    if (!std::isfinite(desc->max_distance) || !(desc->max_distance > 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "max_distance must be finite and > 0").c_str());
    if (!std::isfinite(desc->bias) || !(desc->bias >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "bias must be finite and >= 0").c_str());
    if (!desc->visibility && !desc->light) return fail(ctx, PT_ERR_INVALID, (fn + "no output asked for (visibility and light are both null)").c_str());
    if (desc->scratch && (reinterpret_cast<uintptr_t>(desc->scratch) & 15u)) return fail(ctx, PT_ERR_INVALID, (fn + "scratch is not 16-byte aligned").c_str());
    const uint32_t bp = (uint32_t)bp64;
    const size_t npix = (size_t)ctx->width * ctx->height;
    const PassPlane planes[6] = {{"hit", desc->hit, npix * 32, true, false},           {"position", desc->position, npix * 16, true, false},
                                 {"view_ray", desc->view_ray, npix * 32, false, false}, {"visibility", desc->visibility, npix * 16, false, true},
                                 {"light", desc->light, npix * 16, false, true},        {"scratch", desc->scratch, shadow_scratch_bytes(bp, R), true, true}};
    rc = pass_planes_check(ctx, "pt_shadow_planes", planes, 6);
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_shadow_planes", PASS_SLOT_BYTES); // per slot: skipped, nonfinite, invalid, backfacing, slots, occluded
    if (rc) return rc;
    const ShadowScratch sc = shadow_scratch(desc->scratch, bp, R);
    ShadowTaps* d_tt = nullptr;
    CK(run.tmp.alloc(&d_tt, 1));
    CK(hipMemcpyAsync(d_tt, &tt, sizeof(ShadowTaps), hipMemcpyHostToDevice, ctx->stream)); // (tt lives until the call has waited)
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    const uint32_t batches = n ? (n + bp - 1u) / bp : 0u;
    std::vector<hipEvent_t> ev(2 * (size_t)batches);
    for (hipEvent_t& e : ev) CK(run.tmp.event(&e));
    uint32_t h_fault = 0;
    if (n != 0) {
        CK(hipMemsetAsync(sc.count, 0, SH_HEAD_BYTES, ctx->stream)); // count, chunk counter and fault word; between batches k_shadow_reduce clears the first two
        ShadowArgs aa{};
        aa.width = ctx->width, aa.height = ctx->height;
        aa.hit = reinterpret_cast<const float*>(desc->hit), aa.position = desc->position, aa.view_ray = desc->view_ray;
        aa.visibility = desc->visibility, aa.light = desc->light;
        aa.s = sc, aa.tt = d_tt, aa.eye = ctx->eye;
        aa.num_lights = nl, aa.max_distance = desc->max_distance, aa.bias = desc->bias;
        aa.seed = desc->seed, aa.jitter = desc->flags & (uint32_t)PT_SHADOW_JITTER;
        for (uint32_t i = 0; i < (uint32_t)PT_SHADOW_MAX_LIGHTS; ++i) aa.lights[i] = lights[i], aa.radiance[i] = radiance[i];
        aa.counts = run.counts();
        for (uint32_t b = 0; b < batches; ++b) {
            const uint32_t first = b * bp, nb = std::min(bp, n - first);
            aa.pixels = run.pixels + first;
            aa.n = nb;
            PASS_LAUNCH(run, (nb + SH_GROUP - 1u) / SH_GROUP, 256, aa, k_shadow_rays);
            CK(hipEventRecord(ev[2 * b], ctx->stream));
            PathState st{};
            st.rayO = sc.rayO;
            st.rayD = sc.rayD;
            st.hit = sc.hit;
            Trace8Args ta{st, bvh_dev(ctx), QView{nullptr, sc.count, 0}, QView{}, sc.work, ctx->ovf, 0, nullptr, 0, ctx->lds_skip, ctx->ovf_depth, sc.fault, ctx->bvh.num_nodes8};
            hipLaunchKernelGGL((k_trace8<TR_ANY_QUERY>), dim3(ctx->trace_grid), dim3(64), 0, ctx->stream, ta);
            CK(hipEventRecord(ev[2 * b + 1], ctx->stream));
            PASS_LAUNCH(run, (nb + 255u) / 256u, 256, aa, k_shadow_reduce); // (clears the count and the chunk counter for the next batch)
        }
        CK(hipMemcpyAsync(&h_fault, sc.fault, 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    unsigned long long sum[6] = {};
    rc = run.close_slots(sum, 6);
    if (rc) return rc;
    if (h_fault & 1u) return fail(ctx, PT_ERR_UNSUPPORTED, "pt_shadow_planes: traversal stack overflow: the acceleration structure is deeper than the traversal stack");
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
        stats->backfacing = sum[3];
        stats->invalid = sum[2];
        stats->rays = sum[4] - sum[2];
        stats->occluded = sum[5];
        stats->batches = batches;
        stats->kernel_ms = run.ms;
        stats->trace_ms = trace_ms;
    }
    return PT_OK;
}
