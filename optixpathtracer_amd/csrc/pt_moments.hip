// The library's device translation unit: the C ABI of pt_api.hip, pt_render_gbuffer (pt_gbuffer.hip), pt_temporal_accumulate
// (pt_temporal.hip), pt_filter_planes (pt_filter.hip) and pt_motion_planes (pt_motion.hip), then pt_temporal_moments and pt_modulate_planes.
//
// pt_motion.hip is included, not edited, for the reason written at the top of pt_gbuffer.hip: the entry points need the context and the
// file-local helpers of pt_api.hip (the pointer checks, the block compaction of the mask, the drain of the frames in flight), add no field
// to the context and change no line of the frame path or of the four passes in front of them.  What the calls need beside the context —
// two counters, the byte table of the call's block set, two events — is allocated per call and freed on every exit path (DevScope), outside
// the timed span.
#include "pt_motion.hip"

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
    struct Plane { const char* name; const void* p; size_t bytes; bool required, exclusive; };
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (color may be zeroed, the four outputs are written); the read-only planes may alias one another
    const Plane planes[14] = {{"color", desc->color, npix * 16, true, true},
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
    CK(hipSetDevice(ctx->device));
    {
        std::string err;
        for (const Plane& pl : planes)
            if ((pl.p || pl.required) && query_pointer_validate(ctx, pl.p, pl.bytes, pl.name, err, "pt_temporal_moments", "a device copy") != PT_OK) return fail(ctx, PT_ERR_INVALID, err.c_str());
        for (int i = 0; i < 14; ++i)
            for (int j = i + 1; j < 14; ++j) {
                if (!planes[i].exclusive && !planes[j].exclusive) continue;
                const uintptr_t a = reinterpret_cast<uintptr_t>(planes[i].p), b = reinterpret_cast<uintptr_t>(planes[j].p);
                if (a && b && a < b + planes[j].bytes && b < a + planes[i].bytes) return fail(ctx, PT_ERR_INVALID, (fn + planes[i].name + " and " + planes[j].name + " overlap").c_str());
            }
    }
    int rc = subset_open(ctx, "pt_temporal_moments", false, 0); // frames in flight and queued queries finish first; the block table for the mask
    if (rc) return rc;
    pt_ctx::Blocks& B = ctx->blk;
    // the call's block set, for the `block` test of the clamp window: pt_filter_planes's table
    std::vector<uint8_t> inset;
    if (clamp) {
        inset.assign(B.owned_flags.begin(), B.owned_flags.begin() + B.nblk);
        if (desc->block_mask)
            for (uint32_t b = 0; b < B.nblk; ++b) inset[b] = (inset[b] && desc->block_mask[b]) ? 1 : 0;
    }
    DevScope tmp;
    unsigned long long* d_counts = nullptr;
    uint8_t* d_inset = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    CK(tmp.alloc(&d_counts, 2));
    if (clamp) CK(tmp.alloc(&d_inset, (size_t)B.nblk));
    CK(tmp.event(&ev0));
    CK(tmp.event(&ev1));
    // (uploads and clears stay outside the timed span)
    CK(hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), ctx->stream));
    if (clamp) CK(hipMemcpyAsync(d_inset, inset.data(), B.nblk, hipMemcpyHostToDevice, ctx->stream));
    if (desc->block_mask) CK(hipMemcpyAsync(B.d_flags, desc->block_mask, B.nblk, hipMemcpyHostToDevice, ctx->stream));
    CK(hipEventRecord(ev0, ctx->stream));
    const uint32_t* pixels = ctx->frame_pixels();
    uint32_t n = ctx->frame_owned();
    if (desc->block_mask) {
        rc = compact_enqueue(ctx, ctx->stream, B.d_flags, B.d_list, 1);
        if (rc) {
            hipStreamSynchronize(ctx->stream); // nothing of the call may still run when its temporaries go
            return rc;
        }
        CK(hipStreamSynchronize(ctx->stream)); // the launch is sized on the host: it needs the count
        pixels = B.d_list;
        n = B.h_counts[0];
    }
    hipError_t e = hipSuccess;
    if (n != 0) {
        const TMomArgs ta{pixels, n, ctx->width, ctx->height, desc->color, desc->albedo, desc->motion, reinterpret_cast<const float*>(desc->hit), desc->position,
                          reinterpret_cast<const float*>(desc->prev_hit), desc->prev_position, desc->history_in, desc->moments_in, desc->length_in,
                          desc->history_out, desc->moments_out, desc->length_out, desc->variance_out, d_inset, B.nbx, desc->color_scale, desc->albedo_min,
                          desc->normal_cos, desc->plane_eps, desc->min_weight, clamp ? desc->clamp_k : 0.f, (float)(desc->max_history - 1u), d_counts};
        const unsigned grid = (n + 255u) / 256u;
        const bool views = ctx->vw.n != 0;
        const ViewParams vp = views ? ViewParams{ctx->vw.d_vblock, ctx->vw.d_views, (uint32_t)(ctx->width + 7) / 8u} : ViewParams{};
        if (clamp) {
            if (views) hipLaunchKernelGGL((k_tmom<true, true>), dim3(grid), dim3(256), 0, ctx->stream, ta, vp);
            else hipLaunchKernelGGL((k_tmom<false, true>), dim3(grid), dim3(256), 0, ctx->stream, ta, vp);
        } else {
            if (views) hipLaunchKernelGGL((k_tmom<true, false>), dim3(grid), dim3(256), 0, ctx->stream, ta, vp);
            else hipLaunchKernelGGL((k_tmom<false, false>), dim3(grid), dim3(256), 0, ctx->stream, ta, vp);
        }
        e = hipGetLastError();
        // the clear: behind every read of the call, on the same stream
        if (e == hipSuccess && clear) {
            hipLaunchKernelGGL(k_clear4, dim3(grid), dim3(256), 0, ctx->stream, pixels, n, ctx->width, desc->color);
            e = hipGetLastError();
        }
    }
    // from here on the stream is waited for before the temporaries are freed, whatever fails
    unsigned long long h_counts[2] = {0, 0};
    if (e == hipSuccess) e = hipEventRecord(ev1, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_counts, d_counts, sizeof(h_counts), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    CK(e);
    CK(es);
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, ev0, ev1));
    if (stats) {
        stats->pixels = n;
        stats->reprojected = h_counts[0];
        stats->clamped = h_counts[1];
        stats->kernel_ms = ms;
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
    struct Plane { const char* name; const void* p; size_t bytes; bool required, exclusive; };
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (the two written ones) — except that out may be exactly color: the pass is pixel-local
    const Plane planes[4] = {{"color", desc->color, npix * 16, true, false},
                             {"albedo", desc->albedo, npix * 16, false, false},
                             {"out", desc->out, npix * 16, false, true},
                             {"frame_rgba8", desc->frame_rgba8, npix * 4, false, true}};
    CK(hipSetDevice(ctx->device));
    {
        std::string err;
        for (const Plane& pl : planes)
            if ((pl.p || pl.required) && query_pointer_validate(ctx, pl.p, pl.bytes, pl.name, err, "pt_modulate_planes", "a device copy") != PT_OK) return fail(ctx, PT_ERR_INVALID, err.c_str());
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j) {
                if (!planes[i].exclusive && !planes[j].exclusive) continue;
                const uintptr_t a = reinterpret_cast<uintptr_t>(planes[i].p), b = reinterpret_cast<uintptr_t>(planes[j].p);
                if (i == 0 && j == 2 && a == b) continue; // in place
                if (a && b && a < b + planes[j].bytes && b < a + planes[i].bytes) return fail(ctx, PT_ERR_INVALID, (fn + planes[i].name + " and " + planes[j].name + " overlap").c_str());
            }
    }
    int rc = subset_open(ctx, "pt_modulate_planes", false, 0); // frames in flight and queued queries finish first; the block table for the mask
    if (rc) return rc;
    DevScope tmp;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    CK(tmp.event(&ev0));
    CK(tmp.event(&ev1));
    pt_ctx::Blocks& B = ctx->blk;
    // (uploads stay outside the timed span)
    if (desc->block_mask) CK(hipMemcpyAsync(B.d_flags, desc->block_mask, B.nblk, hipMemcpyHostToDevice, ctx->stream));
    CK(hipEventRecord(ev0, ctx->stream));
    const uint32_t* pixels = ctx->frame_pixels();
    uint32_t n = ctx->frame_owned();
    if (desc->block_mask) {
        rc = compact_enqueue(ctx, ctx->stream, B.d_flags, B.d_list, 1);
        if (rc) {
            hipStreamSynchronize(ctx->stream); // nothing of the call may still run when its temporaries go
            return rc;
        }
        CK(hipStreamSynchronize(ctx->stream)); // the launch is sized on the host: it needs the count
        pixels = B.d_list;
        n = B.h_counts[0];
    }
    if (n != 0) {
        const ModulateArgs ma{pixels, n, ctx->width, desc->color, desc->albedo, desc->out, desc->frame_rgba8, desc->albedo_min};
        hipLaunchKernelGGL(k_modulate, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, ma);
    }
    // from here on the stream is waited for before the temporaries are freed, whatever fails
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ev1, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    CK(e);
    CK(es);
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, ev0, ev1));
    if (stats) {
        stats->pixels = n;
        stats->kernel_ms = ms;
    }
    return PT_OK;
}
