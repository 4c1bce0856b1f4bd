// pt_temporal_moments and pt_modulate_planes: the fused SVGF temporal stage (k_tmom, k_clear4) and the end of the chain (k_modulate).  Part
// of pt_lib.hip.
#include "pt_moments.h"

extern "C" int pt_temporal_moments(pt_ctx* ctx, const pt_tmom_desc* desc, pt_tmom_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_temporal_moments: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_temporal_moments: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_temporal_moments: no frame size yet (pt_resize)");
    const std::string fn = "pt_temporal_moments: ";
    const uint32_t known = (uint32_t)PT_TMOM_CLEAR_COLOR | (uint32_t)PT_TMOM_CLAMP;
    if (desc->flags & ~known) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags & ~known)).c_str());
    const bool clamp = (desc->flags & (uint32_t)PT_TMOM_CLAMP) != 0u, clear = (desc->flags & (uint32_t)PT_TMOM_CLEAR_COLOR) != 0u;
    if (!std::isfinite(desc->color_scale) || !(desc->color_scale > 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "color_scale must be finite and > 0").c_str());
    if (!std::isfinite(desc->albedo_min) || !(desc->albedo_min >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "albedo_min must be finite and >= 0").c_str());
    if (!(desc->normal_cos >= -1.f && desc->normal_cos <= 1.f)) return fail(ctx, PT_ERR_INVALID, (fn + "normal_cos must be in [-1,1]").c_str());
    if (!std::isfinite(desc->plane_eps) || !(desc->plane_eps >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "plane_eps must be finite and >= 0").c_str());
    if (!(desc->min_weight >= 0.f && desc->min_weight <= 1.f)) return fail(ctx, PT_ERR_INVALID, (fn + "min_weight must be in [0,1]").c_str());
    if (clamp && (!std::isfinite(desc->clamp_k) || !(desc->clamp_k >= 0.f))) return fail(ctx, PT_ERR_INVALID, (fn + "clamp_k must be finite and >= 0").c_str());
    if (desc->max_history < 1u || desc->max_history > 65535u) return fail(ctx, PT_ERR_INVALID, (fn + "max_history must be in [1,65535]").c_str());
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (color may be zeroed, the four outputs are written); the read-only planes may alias one another
    const PassPlane planes[14] = {{"color", desc->color, npix * 16, true, true},
                                  {"albedo", desc->albedo, npix * 16, false, false},
                                  {"motion", desc->motion, npix * 8, true, false},
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
    int rc = pass_planes_check(ctx, "pt_temporal_moments", planes, 14);
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_temporal_moments", 2 * sizeof(unsigned long long)); // two counters: reprojected, clamped
    if (rc) return rc;
    const pt_ctx::Blocks& B = ctx->blk;
    std::vector<uint8_t> inset; // for the `block` test of the clamp window
    uint8_t* d_inset = nullptr;
    if (clamp) {
        inset = pass_block_set(ctx, desc->block_mask);
        CK(run.tmp.alloc(&d_inset, (size_t)B.nblk));
        CK(hipMemcpyAsync(d_inset, inset.data(), B.nblk, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    hipError_t e = hipSuccess;
    if (n != 0) {
        const TMomArgs ta{run.pixels, n,
                          {desc->motion, reinterpret_cast<const float*>(desc->hit), desc->position, reinterpret_cast<const float*>(desc->prev_hit), desc->prev_position,
                           desc->history_in, desc->moments_in, desc->length_in, ctx->width, ctx->height, desc->normal_cos, desc->plane_eps, desc->min_weight},
                          desc->color, desc->albedo, desc->history_out, desc->moments_out, desc->length_out, desc->variance_out, d_inset, B.nbx, desc->color_scale,
                          desc->albedo_min, clamp ? desc->clamp_k : 0.f, (float)(desc->max_history - 1u), run.counts()};
        const unsigned grid = (n + 255u) / 256u;
        if (clamp) PASS_LAUNCH(run, grid, 256, ta, k_tmom, true);
        else PASS_LAUNCH(run, grid, 256, ta, k_tmom, false);
        e = hipGetLastError();
        // the clear: behind every read of the call, on the same stream
        if (e == hipSuccess && clear) {
            hipLaunchKernelGGL(k_clear4, dim3(grid), dim3(256), 0, ctx->stream, run.pixels, n, ctx->width, desc->color);
            e = hipGetLastError();
        }
    }
    unsigned long long h_counts[2] = {0, 0};
    rc = run.close(e, h_counts, sizeof(h_counts));
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->reprojected = h_counts[0];
        stats->clamped = h_counts[1];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}

extern "C" int pt_modulate_planes(pt_ctx* ctx, const pt_modulate_desc* desc, pt_modulate_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_modulate_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_modulate_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_modulate_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_modulate_planes: ";
    if (desc->flags != 0u) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags)).c_str());
    if (!std::isfinite(desc->albedo_min) || !(desc->albedo_min >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "albedo_min must be finite and >= 0").c_str());
    if (!desc->out && !desc->frame_rgba8) return fail(ctx, PT_ERR_INVALID, (fn + "no output asked for (out and frame_rgba8 are both null)").c_str());
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (the two written ones) — except that out may be exactly color: the pass is pixel-local
    const PassPlane planes[4] = {{"color", desc->color, npix * 16, true, false},
                                 {"albedo", desc->albedo, npix * 16, false, false},
                                 {"out", desc->out, npix * 16, false, true},
                                 {"frame_rgba8", desc->frame_rgba8, npix * 4, false, true}};
    int rc = pass_planes_check(ctx, "pt_modulate_planes", planes, 4, 0, 2); // color and out: in place
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_modulate_planes", 0);
    if (rc) return rc;
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    if (n != 0) {
        const ModulateArgs ma{run.pixels, n, ctx->width, desc->color, desc->albedo, desc->out, desc->frame_rgba8, desc->albedo_min};
        hipLaunchKernelGGL(k_modulate, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, ma);
    }
    rc = run.close(hipSuccess);
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}
