// pt_reflect_layout and pt_reflect_planes: a second G-buffer along each pixel's mirror ray, from the G-buffer's hit and position planes over the
// context's current tree.  Per batch of the call's pixel list: k_reflect_rays, the closest-hit traversal exactly as pt_trace_device launches
// it, k_reflect_resolve.  Part of pt_lib.hip.
#include "pt_reflect.h"

// *batch_pixels: M, at most the frame's pixels
static uint64_t reflect_batch(const pt_ctx* ctx, uint32_t max_rays_in_flight) {
    const uint64_t M = max_rays_in_flight ? max_rays_in_flight : (uint64_t)PT_REFLECT_DEFAULT_RAYS_IN_FLIGHT;
    return std::min<uint64_t>(M, (uint64_t)ctx->width * ctx->height);
}

extern "C" int pt_reflect_layout(const pt_ctx* cctx, uint32_t max_rays_in_flight, size_t* bytes) {
    if (!cctx) return fail(nullptr, PT_ERR_INVALID, "pt_reflect_layout: null context");
    pt_ctx* ctx = const_cast<pt_ctx*>(cctx); // (the error text only)
    if (!bytes) return fail(ctx, PT_ERR_INVALID, "pt_reflect_layout: bytes is null");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_reflect_layout: no frame size yet (pt_resize)");
    *bytes = reflect_scratch_bytes(reflect_batch(ctx, max_rays_in_flight));
    return PT_OK;
}

extern "C" int pt_reflect_planes(pt_ctx* ctx, const pt_reflect_desc* desc, pt_reflect_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_reflect_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_reflect_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_reflect_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_reflect_planes: ";
    if (desc->flags) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags)).c_str());
    if (!std::isfinite(desc->bias) || !(desc->bias >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "bias must be finite and >= 0").c_str());
    if (!std::isfinite(desc->max_distance) || !(desc->max_distance > 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "max_distance must be finite and > 0").c_str());
    if (!desc->hit2 && !desc->position2 && !desc->ray && !desc->sky)
        return fail(ctx, PT_ERR_INVALID, (fn + "no output asked for (hit2, position2, ray and sky are all null)").c_str());
    if (desc->sky && !ctx->pr.dev.data) return fail(ctx, PT_ERR_INVALID, (fn + "sky: no probe set (setProbe)").c_str());
    if (desc->scratch && (reinterpret_cast<uintptr_t>(desc->scratch) & 15u)) return fail(ctx, PT_ERR_INVALID, (fn + "scratch is not 16-byte aligned").c_str());
    const uint32_t bp = (uint32_t)reflect_batch(ctx, desc->max_rays_in_flight);
    const size_t npix = (size_t)ctx->width * ctx->height;
    const PassPlane planes[7] = {{"hit", desc->hit, npix * 32, true, false},          {"position", desc->position, npix * 16, true, false},
                                 {"hit2", desc->hit2, npix * 32, false, true},        {"position2", desc->position2, npix * 16, false, true},
                                 {"ray", desc->ray, npix * 32, false, true},          {"sky", desc->sky, npix * 16, false, true},
                                 {"scratch", desc->scratch, reflect_scratch_bytes(bp), true, true}};
    int rc = pass_planes_check(ctx, "pt_reflect_planes", planes, 7);
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_reflect_planes", PASS_SLOT_BYTES); // per slot: skipped, nonfinite, invalid, hits, escaped
    if (rc) return rc;
    const ReflectScratch sc = reflect_scratch(desc->scratch, bp);
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    const uint32_t batches = n ? (n + bp - 1u) / bp : 0u;
    std::vector<hipEvent_t> ev(2 * (size_t)batches);
    for (hipEvent_t& e : ev) CK(run.tmp.event(&e));
    uint32_t h_fault = 0;
    if (n != 0) {
        CK(hipMemsetAsync(sc.count, 0, REFLECT_HEAD_BYTES, ctx->stream)); // count, chunk counter and fault word; between batches k_reflect_resolve clears the first two
        for (uint32_t b = 0; b < batches; ++b) {
            const uint32_t first = b * bp, nb = std::min(bp, n - first);
            const ReflectArgs aa{run.pixels + first, nb, ctx->width, ctx->height, reinterpret_cast<const float*>(desc->hit), desc->position, reinterpret_cast<float*>(desc->hit2),
                                 desc->position2, desc->ray, desc->sky, sc, ctx->eye, desc->bias, desc->max_distance, ctx->bvh.tris8, ctx->sc.d_tri_nrm, ctx->pr.dev, run.counts()};
            PASS_LAUNCH(run, (nb + REFLECT_GROUP - 1u) / REFLECT_GROUP, 256, aa, k_reflect_rays);
            CK(hipEventRecord(ev[2 * b], ctx->stream));
            PathState st{};
            st.rayO = sc.rayO;
            st.rayD = sc.rayD;
            st.hit = sc.hit;
            Trace8Args ta{st, bvh_dev(ctx), QView{nullptr, sc.count, 0}, QView{}, sc.work, ctx->ovf, 0, nullptr, 0, ctx->lds_skip, ctx->ovf_depth, sc.fault, ctx->bvh.num_nodes8};
            hipLaunchKernelGGL((k_trace8<TR_CLOSEST>), dim3(ctx->trace_grid), dim3(64), 0, ctx->stream, ta);
            CK(hipEventRecord(ev[2 * b + 1], ctx->stream));
            hipLaunchKernelGGL(k_reflect_resolve, dim3((nb + 255u) / 256u), dim3(256), 0, ctx->stream, aa); // (clears the count and the chunk counter for the next batch)
        }
        CK(hipMemcpyAsync(&h_fault, sc.fault, 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    unsigned long long sum[5] = {};
    rc = run.close_slots(sum, 5);
    if (rc) return rc;
    if (h_fault & 1u) return fail(ctx, PT_ERR_UNSUPPORTED, "pt_reflect_planes: traversal stack overflow: the acceleration structure is deeper than the traversal stack");
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
        stats->hits = sum[3];
        stats->escaped = sum[4];
        stats->batches = batches;
        stats->kernel_ms = run.ms;
        stats->trace_ms = trace_ms;
    }
    return PT_OK;
}
