// pt_sample_plan and pt_temporal_carry: which blocks of a frame need samples (k_plan), and the temporal stage of the others (k_carry).  Part of
// pt_lib.hip.
#include "pt_plan.h"

// the three parameters of the gather, as pt_temporal_moments checks them
static int plan_gather_check(pt_ctx* ctx, const std::string& fn, float normal_cos, float plane_eps, float min_weight) {
    if (!(normal_cos >= -1.f && normal_cos <= 1.f)) return fail(ctx, PT_ERR_INVALID, (fn + "normal_cos must be in [-1,1]").c_str());
    if (!std::isfinite(plane_eps) || !(plane_eps >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "plane_eps must be finite and >= 0").c_str());
    if (!(min_weight >= 0.f && min_weight <= 1.f)) return fail(ctx, PT_ERR_INVALID, (fn + "min_weight must be in [0,1]").c_str());
    return PT_OK;
}

extern "C" int pt_sample_plan(pt_ctx* ctx, const pt_plan_desc* desc, pt_plan_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_sample_plan: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_sample_plan: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_sample_plan: no frame size yet (pt_resize)");
    const std::string fn = "pt_sample_plan: ";
    if (!desc->block_mask_out) return fail(ctx, PT_ERR_INVALID, (fn + "block_mask_out is null").c_str());
    if (desc->flags != 0u) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags)).c_str());
    int rc = plan_gather_check(ctx, fn, desc->normal_cos, desc->plane_eps, desc->min_weight);
    if (rc) return rc;
    if (!std::isfinite(desc->threshold) || !(desc->threshold >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "threshold must be finite and >= 0").c_str());
    if (!std::isfinite(desc->dark_floor) || !(desc->dark_floor >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "dark_floor must be finite and >= 0").c_str());
    if (desc->min_length > 65535u) return fail(ctx, PT_ERR_INVALID, (fn + "min_length must be in [0,65535]").c_str());
    if (desc->min_pixels < 1u || desc->min_pixels > 64u) return fail(ctx, PT_ERR_INVALID, (fn + "min_pixels must be in [1,64]").c_str());
    if (desc->refresh_period > 65535u) return fail(ctx, PT_ERR_INVALID, (fn + "refresh_period must be in [0,65535]").c_str());
    const size_t npix = (size_t)ctx->width * ctx->height;
    // nothing on the device is written except the call's own temporaries: no plane is exclusive, all may alias one another
    const PassPlane planes[8] = {{"motion", desc->motion, npix * 8, true, false},
                                 {"hit", desc->hit, npix * sizeof(pt_hit), true, false},
                                 {"position", desc->position, npix * 16, true, false},
                                 {"prev_hit", desc->prev_hit, npix * sizeof(pt_hit), true, false},
                                 {"prev_position", desc->prev_position, npix * 16, true, false},
                                 {"history_in", desc->history_in, npix * 16, true, false},
                                 {"moments_in", desc->moments_in, npix * 8, true, false},
                                 {"length_in", desc->length_in, npix * 4, true, false}};
    rc = pass_planes_check(ctx, "pt_sample_plan", planes, 8);
    if (rc) return rc;
    std::vector<uint8_t> inset; // outlives the run: its upload is one of the run's copies
    PassRun run;
    rc = run.open(ctx, "pt_sample_plan", PLAN_COUNTERS * sizeof(unsigned long long));
    if (rc) return rc;
    const pt_ctx::Blocks& B = ctx->blk;
    // the call's block set (the mask is read here, before anything is written: block_mask_out may be the very same array), and the answer
    inset = pass_block_set(ctx, desc->block_mask);
    uint64_t blocks = 0;
    for (uint8_t f : inset) blocks += f;
    uint8_t *d_inset = nullptr, *d_out = nullptr;
    CK(run.tmp.alloc(&d_inset, (size_t)B.nblk));
    CK(run.tmp.alloc(&d_out, (size_t)B.nblk));
    CK(hipMemcpyAsync(d_inset, inset.data(), B.nblk, hipMemcpyHostToDevice, ctx->stream));
    rc = run.select(nullptr); // the kernel walks the block table itself: no pixel list, no compaction
    if (rc) return rc;
    const uint32_t period = desc->refresh_period;
    const PlanArgs pa{{desc->motion, reinterpret_cast<const float*>(desc->hit), desc->position, reinterpret_cast<const float*>(desc->prev_hit), desc->prev_position,
                       desc->history_in, desc->moments_in, desc->length_in, ctx->width, ctx->height, desc->normal_cos, desc->plane_eps, desc->min_weight},
                      d_inset, d_out, B.nblk, B.nbx, desc->threshold * desc->threshold, desc->dark_floor, (float)desc->min_length, desc->min_pixels,
                      period, period ? desc->frame_index % period : 0u, run.counts()};
    PASS_LAUNCH(run, (B.nblk + 3u) / 4u, 256, pa, k_plan);
    unsigned long long h_counts[PLAN_COUNTERS] = {};
    rc = run.close(hipGetLastError(), h_counts, sizeof(h_counts));
    if (rc) return rc;
    CK(hipMemcpy(desc->block_mask_out, d_out, B.nblk, hipMemcpyDeviceToHost)); // the stream is idle: close has waited
    if (stats) {
        stats->blocks = blocks;
        stats->sampled = h_counts[PLAN_SAMPLED];
        stats->by_lost = h_counts[PLAN_BY_LOST];
        stats->by_need = h_counts[PLAN_BY_NEED];
        stats->by_refresh = h_counts[PLAN_BY_REFRESH];
        stats->pixels = h_counts[PLAN_PIXELS];
        stats->lost = h_counts[PLAN_LOST];
        stats->needy = h_counts[PLAN_NEEDY];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}

extern "C" int pt_temporal_carry(pt_ctx* ctx, const pt_carry_desc* desc, pt_carry_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_temporal_carry: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_temporal_carry: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_temporal_carry: no frame size yet (pt_resize)");
    const std::string fn = "pt_temporal_carry: ";
    if (desc->flags != 0u) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags)).c_str());
    int rc = plan_gather_check(ctx, fn, desc->normal_cos, desc->plane_eps, desc->min_weight);
    if (rc) return rc;
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (the four outputs are written); the read-only planes may alias one another
    const PassPlane planes[12] = {{"motion", desc->motion, npix * 8, true, false},
                                  {"hit", desc->hit, npix * sizeof(pt_hit), true, false},
                                  {"position", desc->position, npix * 16, true, false},
                                  {"prev_hit", desc->prev_hit, npix * sizeof(pt_hit), true, false},
                                  {"prev_position", desc->prev_position, npix * 16, true, false},
                                  {"history_in", desc->history_in, npix * 16, true, false},
                                  {"moments_in", desc->moments_in, npix * 8, true, false},
                                  {"length_in", desc->length_in, npix * 4, true, false},
                                  {"history_out", desc->history_out, npix * 16, true, true},
                                  {"moments_out", desc->moments_out, npix * 8, true, true},
                                  {"length_out", desc->length_out, npix * 4, true, true},
                                  {"variance_out", desc->variance_out, npix * 4, false, true}};
    rc = pass_planes_check(ctx, "pt_temporal_carry", planes, 12);
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_temporal_carry", sizeof(unsigned long long)); // one counter: carried
    if (rc) return rc;
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    if (n != 0) {
        const CarryArgs ca{{desc->motion, reinterpret_cast<const float*>(desc->hit), desc->position, reinterpret_cast<const float*>(desc->prev_hit), desc->prev_position,
                            desc->history_in, desc->moments_in, desc->length_in, ctx->width, ctx->height, desc->normal_cos, desc->plane_eps, desc->min_weight},
                           run.pixels, n, desc->history_out, desc->moments_out, desc->length_out, desc->variance_out, run.counts()};
        PASS_LAUNCH(run, (n + 255u) / 256u, 256, ca, k_carry);
    }
    unsigned long long carried = 0;
    rc = run.close(hipGetLastError(), &carried, sizeof(carried));
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->carried = carried;
        stats->lost = n - carried;
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}
