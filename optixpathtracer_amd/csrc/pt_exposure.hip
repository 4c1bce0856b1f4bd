// pt_exposure_planes and pt_tonemap_planes: metering and adapting an exposure per view (k_meter, k_adapt) and the display operator under
// it (k_tonemap).  Part of pt_lib.hip.
#include "pt_exposure.h"

extern "C" int pt_exposure_planes(pt_ctx* ctx, const pt_exposure_desc* desc, pt_exposure_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_exposure_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_exposure_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_exposure_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_exposure_planes: ";
    const uint32_t known = PT_EXPOSURE_ACCUMULATE | PT_EXPOSURE_FROM_HISTOGRAM;
    if (desc->flags & ~known) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags & ~known)).c_str());
    const bool from_hist = (desc->flags & PT_EXPOSURE_FROM_HISTOGRAM) != 0u;
    if (from_hist && (desc->color || desc->hit || desc->block_mask))
        return fail(ctx, PT_ERR_INVALID, (fn + "PT_EXPOSURE_FROM_HISTOGRAM takes no color, hit or block_mask").c_str());
    if ((unsigned long long)desc->low_permille + desc->high_permille > 999ull) return fail(ctx, PT_ERR_INVALID, (fn + "low_permille + high_permille must be <= 999").c_str());
    if (!std::isfinite(desc->key_log2)) return fail(ctx, PT_ERR_INVALID, (fn + "key_log2 must be finite").c_str());
    if (!(desc->ev_min >= -24.f && desc->ev_min <= 24.f && desc->ev_max >= -24.f && desc->ev_max <= 24.f && desc->ev_min <= desc->ev_max))
        return fail(ctx, PT_ERR_INVALID, (fn + "ev_min and ev_max must be in [-24,24] with ev_min <= ev_max").c_str());
    if (!(desc->rate_up >= 0.f && desc->rate_up <= 1.f && desc->rate_down >= 0.f && desc->rate_down <= 1.f))
        return fail(ctx, PT_ERR_INVALID, (fn + "rate_up and rate_down must be in [0,1]").c_str());
    const size_t npix = (size_t)ctx->width * ctx->height;
    const uint32_t nv = pass_camera_count(ctx);
    // exclusive: may overlap no other plane (the two written ones) — except that state_out may be exactly state_in: a view reads its own
    // four words before it writes them
    const PassPlane planes[5] = {{"color", desc->color, npix * 16, !from_hist, false},
                                 {"hit", desc->hit, npix * sizeof(pt_hit), false, false},
                                 {"hist", desc->hist, (size_t)nv * EXPO_BINS * 4, true, true},
                                 {"state_in", desc->state_in, (size_t)nv * 16, false, false},
                                 {"state_out", desc->state_out, (size_t)nv * 16, true, true}};
    int rc = pass_planes_check(ctx, "pt_exposure_planes", planes, 5, 3, 4);
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_exposure_planes", PASS_SLOT_BYTES); // per slot: skipped, nonfinite, under, over
    if (rc) return rc;
    if (!(desc->flags & known)) CK(hipMemsetAsync(desc->hist, 0, (size_t)nv * EXPO_BINS * 4, ctx->stream));
    uint32_t n = 0;
    if (from_hist) {
        CK(hipEventRecord(run.ev0, ctx->stream)); // no pixel set: the timed span is the adaptation's
    } else {
        rc = run.select(desc->block_mask);
        if (rc) return rc;
        n = run.n;
    }
    if (n != 0) {
        int cus = 0;
        CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        const uint32_t ntiles = (n + EXPO_TILE - 1u) / EXPO_TILE;
        const uint32_t want = std::min(ntiles, (uint32_t)std::max(cus, 1) * 4u); // four workgroups a CU: one wave of each on every SIMD
        const uint32_t per = (ntiles + want - 1u) / want;
        const MeterArgs ma{run.pixels, n, per, ctx->width, ctx->height, desc->color, reinterpret_cast<const float*>(desc->hit), desc->hist, run.counts()};
        PASS_LAUNCH(run, (ntiles + per - 1u) / per, 256, ma, k_meter);
    }
    const AdaptArgs aa{desc->hist, desc->state_in, desc->state_out, nv, desc->low_permille, desc->high_permille, desc->key_log2, desc->ev_min, desc->ev_max,
                       desc->rate_up, desc->rate_down};
    hipLaunchKernelGGL(k_adapt, dim3(nv), dim3(64), 0, ctx->stream, aa);
    unsigned long long sum[4] = {};
    rc = run.close_slots(sum, 4);
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->skipped = sum[0];
        stats->nonfinite = sum[1];
        stats->under = sum[2];
        stats->over = sum[3];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}

extern "C" int pt_tonemap_planes(pt_ctx* ctx, const pt_tonemap_desc* desc, pt_tonemap_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_tonemap_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_tonemap_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_tonemap_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_tonemap_planes: ";
    if (desc->flags != 0u) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags)).c_str());
    if (desc->op > (uint32_t)PT_TONEMAP_ACES) return fail(ctx, PT_ERR_INVALID, (fn + "unknown operator " + std::to_string(desc->op)).c_str());
    if (!std::isfinite(desc->exposure) || !(desc->exposure > 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "exposure must be finite and > 0").c_str());
    if (!std::isfinite(desc->white) || !(desc->white > 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "white must be finite and > 0").c_str());
    if (!desc->out && !desc->frame_rgba8) return fail(ctx, PT_ERR_INVALID, (fn + "no output asked for (out and frame_rgba8 are both null)").c_str());
    const size_t npix = (size_t)ctx->width * ctx->height;
    const uint32_t nv = pass_camera_count(ctx);
    // exclusive: may overlap no other plane (the two written ones) — except that out may be exactly color: the pass is pixel-local
    const PassPlane planes[4] = {{"color", desc->color, npix * 16, true, false},
                                 {"state", desc->state, (size_t)nv * 16, false, false},
                                 {"out", desc->out, npix * 16, false, true},
                                 {"frame_rgba8", desc->frame_rgba8, npix * 4, false, true}};
    int rc = pass_planes_check(ctx, "pt_tonemap_planes", planes, 4, 0, 2); // color and out: in place
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_tonemap_planes", PASS_SLOT_BYTES); // per slot: clipped
    if (rc) return rc;
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    if (n != 0) {
        const TonemapArgs ta{run.pixels, n, ctx->width, ctx->height, desc->color, desc->state, desc->out, desc->frame_rgba8, desc->exposure, desc->white, desc->op,
                             run.counts()};
        PASS_LAUNCH(run, (n + 255u) / 256u, 256, ta, k_tonemap);
    }
    unsigned long long sum[1] = {};
    rc = run.close_slots(sum, 1);
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->clipped = sum[0];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}
