// The library's device translation unit: the C ABI of pt_api.hip and pt_render_gbuffer (pt_gbuffer.hip), then pt_temporal_accumulate.
//
// pt_gbuffer.hip is included, not edited, for the reason written at its top: the entry point needs the context and the file-local helpers of
// pt_api.hip (the pointer checks, the block compaction of the mask, the drain of the frames in flight), adds no field to the context and
// changes no line of the frame path or of the G-buffer pass.  What the call needs beside the context — one counter, two events — is
// allocated per call and freed on every exit path (DevScope), outside the timed span.
#include "pt_gbuffer.hip"

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
    struct Plane { const char* name; const void* p; size_t bytes; bool required, exclusive; };
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (color is zeroed, the four outputs are written); the read-only planes may alias one another
    const Plane planes[12] = {{"color", desc->color, npix * 16, true, true},
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
    CK(hipSetDevice(ctx->device));
    {
        std::string err;
        for (const Plane& pl : planes)
            if ((pl.p || pl.required) && query_pointer_validate(ctx, pl.p, pl.bytes, pl.name, err, "pt_temporal_accumulate", "a device copy") != PT_OK) return fail(ctx, PT_ERR_INVALID, err.c_str());
        for (int i = 0; i < 12; ++i)
            for (int j = i + 1; j < 12; ++j) {
                if (!planes[i].exclusive && !planes[j].exclusive) continue;
                const uintptr_t a = reinterpret_cast<uintptr_t>(planes[i].p), b = reinterpret_cast<uintptr_t>(planes[j].p);
                if (a && b && a < b + planes[j].bytes && b < a + planes[i].bytes) return fail(ctx, PT_ERR_INVALID, (fn + planes[i].name + " and " + planes[j].name + " overlap").c_str());
            }
    }
    int rc = subset_open(ctx, "pt_temporal_accumulate", false, 0); // frames in flight and queued queries finish first; the block table for the mask
    if (rc) return rc;
    DevScope tmp;
    unsigned long long* d_count = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    CK(tmp.alloc(&d_count, 1));
    CK(tmp.event(&ev0));
    CK(tmp.event(&ev1));
    pt_ctx::Blocks& B = ctx->blk;
    // (uploads and clears stay outside the timed span)
    CK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), ctx->stream));
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
        const TemporalArgs ta{pixels, n, ctx->width, ctx->height, desc->color, desc->motion, reinterpret_cast<const float*>(desc->hit), desc->position,
                              reinterpret_cast<const float*>(desc->prev_hit), desc->prev_position, desc->history_in, desc->length_in, desc->history_out, desc->length_out,
                              desc->frame_rgba8, desc->copy_out, desc->color_scale, desc->normal_cos, desc->plane_eps, desc->min_weight,
                              (float)(desc->max_history - 1u), desc->flags & (uint32_t)PT_TEMPORAL_CLEAR_COLOR, d_count};
        const unsigned grid = (n + 255u) / 256u;
        if (ctx->vw.n) {
            const ViewParams vp{ctx->vw.d_vblock, ctx->vw.d_views, (uint32_t)(ctx->width + 7) / 8u};
            hipLaunchKernelGGL((k_temporal<true>), dim3(grid), dim3(256), 0, ctx->stream, ta, vp);
        } else {
            hipLaunchKernelGGL((k_temporal<false>), dim3(grid), dim3(256), 0, ctx->stream, ta, ViewParams{});
        }
    }
    // from here on the stream is waited for before the temporaries are freed, whatever fails
    unsigned long long h_count = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ev1, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_count, d_count, sizeof(h_count), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    CK(e);
    CK(es);
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, ev0, ev1));
    if (stats) {
        stats->pixels = n;
        stats->reprojected = h_count;
        stats->kernel_ms = ms;
    }
    return PT_OK;
}
