// pt_temporal_accumulate: reprojects last frame's history along the motion plane and blends this frame's colour in (k_temporal).  Part of
// pt_lib.hip.
#include "pt_temporal.h"

extern "C" int pt_temporal_accumulate(pt_ctx* ctx, const pt_temporal_desc* desc, pt_temporal_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_temporal_accumulate: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_temporal_accumulate: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_temporal_accumulate: no frame size yet (pt_resize)");
    const std::string fn = "pt_temporal_accumulate: ";
    if (desc->flags & ~(uint32_t)PT_TEMPORAL_CLEAR_COLOR) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags & ~(uint32_t)PT_TEMPORAL_CLEAR_COLOR)).c_str());
    if (!std::isfinite(desc->color_scale) || !(desc->color_scale > 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "color_scale must be finite and > 0").c_str());
    if (!(desc->normal_cos >= -1.f && desc->normal_cos <= 1.f)) return fail(ctx, PT_ERR_INVALID, (fn + "normal_cos must be in [-1,1]").c_str());
    if (!std::isfinite(desc->plane_eps) || !(desc->plane_eps >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "plane_eps must be finite and >= 0").c_str());
    if (!(desc->min_weight >= 0.f && desc->min_weight <= 1.f)) return fail(ctx, PT_ERR_INVALID, (fn + "min_weight must be in [0,1]").c_str());
    if (desc->max_history < 1u || desc->max_history > 65535u) return fail(ctx, PT_ERR_INVALID, (fn + "max_history must be in [1,65535]").c_str());
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (color is zeroed, the four outputs are written); the read-only planes may alias one another
    const PassPlane planes[12] = {{"color", desc->color, npix * 16, true, true},
                                  {"motion", desc->motion, npix * 8, true, false},
                                  {"hit", desc->hit, npix * sizeof(pt_hit), true, false},
                                  {"position", desc->position, npix * 16, true, false},
                                  {"prev_hit", desc->prev_hit, npix * sizeof(pt_hit), true, false},
                                  {"prev_position", desc->prev_position, npix * 16, true, false},
                                  {"history_in", desc->history_in, npix * 16, true, false},
                                  {"length_in", desc->length_in, npix * 4, true, false},
                                  {"history_out", desc->history_out, npix * 16, true, true},
                                  {"length_out", desc->length_out, npix * 4, true, true},
                                  {"frame_rgba8", desc->frame_rgba8, npix * 4, false, true},
                                  {"copy_out", desc->copy_out, npix * 16, false, true}};
    int rc = pass_planes_check(ctx, "pt_temporal_accumulate", planes, 12);
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_temporal_accumulate", sizeof(unsigned long long)); // one counter: the reprojected pixels
    if (rc) return rc;
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    if (n != 0) {
        const TemporalArgs ta{run.pixels, n,
                              {desc->motion, reinterpret_cast<const float*>(desc->hit), desc->position, reinterpret_cast<const float*>(desc->prev_hit), desc->prev_position,
                               desc->history_in, nullptr, desc->length_in, ctx->width, ctx->height, desc->normal_cos, desc->plane_eps, desc->min_weight},
                              desc->color, desc->history_out, desc->length_out, desc->frame_rgba8, desc->copy_out, desc->color_scale,
                              (float)(desc->max_history - 1u), desc->flags & (uint32_t)PT_TEMPORAL_CLEAR_COLOR, run.counts()};
        const unsigned grid = (n + 255u) / 256u;
        PASS_LAUNCH(run, grid, 256, ta, k_temporal);
    }
    unsigned long long h_count = 0;
    rc = run.close(hipSuccess, &h_count, sizeof(h_count));
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->reprojected = h_count;
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}
