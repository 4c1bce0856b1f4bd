// The library's device translation unit: the C ABI of pt_api.hip, pt_render_gbuffer (pt_gbuffer.hip) and pt_temporal_accumulate
// (pt_temporal.hip), then pt_filter_planes.
//
// pt_temporal.hip is included, not edited, for the reason written at the top of pt_gbuffer.hip: the entry point needs the context and the
// file-local helpers of pt_api.hip (the pointer checks, the block compaction of the mask, the drain of the frames in flight), adds no field
// to the context and changes no line of the frame path or of the two passes in front of it.  What the call needs beside the context — two
// counters, the byte table of the call's block set, two events — is allocated per call and freed on every exit path (DevScope), outside the
// timed span.
#include "pt_temporal.hip"

#include "pt_filter.h"

extern "C" int pt_filter_planes(pt_ctx* ctx, const pt_filter_desc* desc, pt_filter_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_filter_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_filter_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_filter_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_filter_planes: ";
    if (desc->flags != 0u) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags)).c_str());
    if (desc->iterations < 0 || desc->iterations > 6) return fail(ctx, PT_ERR_INVALID, (fn + "iterations must be in [0,6]").c_str());
    if (!std::isfinite(desc->sigma_lum) || !(desc->sigma_lum > 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "sigma_lum must be finite and > 0").c_str());
    if (!(desc->normal_cos >= -1.f && desc->normal_cos <= 1.f)) return fail(ctx, PT_ERR_INVALID, (fn + "normal_cos must be in [-1,1]").c_str());
    if (!std::isfinite(desc->plane_eps) || !(desc->plane_eps >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "plane_eps must be finite and >= 0").c_str());
    if (desc->min_length > 65535u) return fail(ctx, PT_ERR_INVALID, (fn + "min_length must be in [0,65535]").c_str());
    struct Plane { const char* name; const void* p; size_t bytes; bool required, exclusive; };
    const size_t npix = (size_t)ctx->width * ctx->height;
    const int iters = desc->iterations;
    // exclusive: may overlap no other plane (the three written ones); the read-only planes may alias one another
    const Plane planes[8] = {{"color", desc->color, npix * 16, true, false},
                             {"hit", desc->hit, npix * sizeof(pt_hit), true, false},
                             {"position", desc->position, npix * 16, true, false},
                             {"variance", desc->variance, npix * 4, false, false},
                             {"length", desc->length, npix * 4, false, false},
                             {"out", desc->out, npix * 16, true, true},
                             {"scratch", desc->scratch, npix * 16, iters >= 1, true},
                             {"frame_rgba8", desc->frame_rgba8, npix * 4, false, true}};
    CK(hipSetDevice(ctx->device));
    {
        std::string err;
        for (const Plane& pl : planes)
            if ((pl.p || pl.required) && query_pointer_validate(ctx, pl.p, pl.bytes, pl.name, err, "pt_filter_planes", "a device copy") != PT_OK) return fail(ctx, PT_ERR_INVALID, err.c_str());
        for (int i = 0; i < 8; ++i)
            for (int j = i + 1; j < 8; ++j) {
                if (!planes[i].exclusive && !planes[j].exclusive) continue;
                const uintptr_t a = reinterpret_cast<uintptr_t>(planes[i].p), b = reinterpret_cast<uintptr_t>(planes[j].p);
                if (a && b && a < b + planes[j].bytes && b < a + planes[i].bytes) return fail(ctx, PT_ERR_INVALID, (fn + planes[i].name + " and " + planes[j].name + " overlap").c_str());
            }
    }
    int rc = subset_open(ctx, "pt_filter_planes", false, 0); // frames in flight and queued queries finish first; the block table for the mask
    if (rc) return rc;
    pt_ctx::Blocks& B = ctx->blk;
    // the call's block set, for the `block` test of the taps: the rank's blocks (view blocks only while views are set) that the mask names
    std::vector<uint8_t> inset(B.owned_flags.begin(), B.owned_flags.begin() + B.nblk);
    if (desc->block_mask)
        for (uint32_t b = 0; b < B.nblk; ++b) inset[b] = (inset[b] && desc->block_mask[b]) ? 1 : 0;
    DevScope tmp;
    unsigned long long* d_counts = nullptr;
    uint8_t* d_inset = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    CK(tmp.alloc(&d_counts, 2));
    CK(tmp.alloc(&d_inset, (size_t)B.nblk));
    CK(tmp.event(&ev0));
    CK(tmp.event(&ev1));
    // (uploads and clears stay outside the timed span)
    CK(hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), ctx->stream));
    CK(hipMemcpyAsync(d_inset, inset.data(), B.nblk, hipMemcpyHostToDevice, ctx->stream));
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
        FilterArgs fa{pixels, n, ctx->width, ctx->height, desc->color, reinterpret_cast<const float*>(desc->hit), desc->position, desc->variance, desc->length,
                      nullptr, nullptr, nullptr, d_inset, B.nbx, desc->sigma_lum, desc->normal_cos, desc->plane_eps, (float)desc->min_length, 1, 0u, d_counts};
        const unsigned grid = (n + 255u) / 256u;
        const bool views = ctx->vw.n != 0;
        const ViewParams vp = views ? ViewParams{ctx->vw.d_vblock, ctx->vw.d_views, (uint32_t)(ctx->width + 7) / 8u} : ViewParams{};
        // stage k of iters + 1 writes `out` when the number of stages after it is even: the last one always does
        float* bufs[2] = {desc->out, desc->scratch};
        for (int k = 0; k <= iters && e == hipSuccess; ++k) {
            fa.src = k ? bufs[(iters - k + 1) & 1] : nullptr;
            fa.dst = bufs[(iters - k) & 1];
            fa.last = k == iters ? 1u : 0u;
            fa.frame = k == iters ? desc->frame_rgba8 : nullptr;
            fa.step = k ? 1 << (k - 1) : 1;
            if (k == 0) {
                if (views) hipLaunchKernelGGL((k_filter_prepare<true>), dim3(grid), dim3(256), 0, ctx->stream, fa, vp);
                else hipLaunchKernelGGL((k_filter_prepare<false>), dim3(grid), dim3(256), 0, ctx->stream, fa, vp);
            } else {
                if (views) hipLaunchKernelGGL((k_filter_pass<true>), dim3(grid), dim3(256), 0, ctx->stream, fa, vp);
                else hipLaunchKernelGGL((k_filter_pass<false>), dim3(grid), dim3(256), 0, ctx->stream, fa, vp);
            }
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
        stats->filtered = h_counts[0];
        stats->spatial = h_counts[1];
        stats->kernel_ms = ms;
    }
    return PT_OK;
}
