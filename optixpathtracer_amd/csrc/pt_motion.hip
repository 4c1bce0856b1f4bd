// The library's device translation unit: the C ABI of pt_api.hip, pt_render_gbuffer (pt_gbuffer.hip), pt_temporal_accumulate
// (pt_temporal.hip) and pt_filter_planes (pt_filter.hip), then pt_vertex_count, pt_copy_vertices_device and pt_motion_planes.
//
// pt_filter.hip is included, not edited, for the reason written at the top of pt_gbuffer.hip: the entry points need the context and the
// file-local helpers of pt_api.hip (the pointer checks, the block compaction of the mask, the drain of the frames in flight), add no field
// to the context and change no line of the frame path or of the three passes in front of them.  What pt_motion_planes needs beside the
// context — two counters, the previous cameras, two events — is allocated per call and freed on every exit path (DevScope), outside the
// timed span.
#include "pt_filter.hip"

#include "pt_motion.h"

extern "C" int pt_vertex_count(const pt_ctx* ctx, uint32_t* vertices, uint32_t* triangles) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_vertex_count: null context");
    if (vertices) *vertices = (uint32_t)ctx->nvert;
    if (triangles) *triangles = ctx->ntri;
    return PT_OK;
}

extern "C" int pt_copy_vertices_device(pt_ctx* ctx, float* dev_dst, size_t bytes) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_copy_vertices_device: null context");
    if (bytes != sizeof(float) * 3 * ctx->nvert)
        return fail(ctx, PT_ERR_INVALID, ("pt_copy_vertices_device: bytes must equal vertices * 12 = " + std::to_string(sizeof(float) * 3 * ctx->nvert)).c_str());
    CK(hipSetDevice(ctx->device));
    {
        std::string err;
        if (query_pointer_validate(ctx, dev_dst, bytes, "dev_dst", err, "pt_copy_vertices_device", "pt_download_vertices") != PT_OK) return fail(ctx, PT_ERR_INVALID, err.c_str());
    }
    int rc = drain(ctx); // frames in flight and queued queries finish first
    if (rc) return rc;
    CK(hipSetDevice(ctx->device));
    if (bytes) CK(hipMemcpyAsync(dev_dst, ctx->d_verts, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

extern "C" int pt_motion_planes(pt_ctx* ctx, const pt_motion_desc* desc, pt_motion_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_motion_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_motion_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_motion_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_motion_planes: ";
    if (desc->flags != 0u) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags)).c_str());
    if (!desc->motion && !desc->prev_point && !desc->prev_surface) return fail(ctx, PT_ERR_INVALID, (fn + "no plane asked for (motion, prev_point, prev_surface are all null)").c_str());
    struct Plane { const char* name; const void* p; size_t bytes; bool required, exclusive; };
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (the three written ones); hit and prev_vertices are only read
    const Plane planes[5] = {{"hit", desc->hit, npix * sizeof(pt_hit), true, false},
                             {"prev_vertices", desc->prev_vertices, sizeof(float) * 3 * ctx->nvert, true, false},
                             {"motion", desc->motion, npix * 8, false, true},
                             {"prev_point", desc->prev_point, npix * 16, false, true},
                             {"prev_surface", desc->prev_surface, npix * sizeof(pt_hit), false, true}};
    CK(hipSetDevice(ctx->device));
    {
        std::string err;
        for (const Plane& pl : planes)
            if ((pl.p || pl.required) && query_pointer_validate(ctx, pl.p, pl.bytes, pl.name, err, "pt_motion_planes", "a device copy") != PT_OK) return fail(ctx, PT_ERR_INVALID, err.c_str());
        for (int i = 0; i < 5; ++i)
            for (int j = i + 1; j < 5; ++j) {
                if (!planes[i].exclusive && !planes[j].exclusive) continue;
                const uintptr_t a = reinterpret_cast<uintptr_t>(planes[i].p), b = reinterpret_cast<uintptr_t>(planes[j].p);
                if (a && b && a < b + planes[j].bytes && b < a + planes[i].bytes) return fail(ctx, PT_ERR_INVALID, (fn + planes[i].name + " and " + planes[j].name + " overlap").c_str());
            }
    }
    const uint32_t ncams = std::max(1u, ctx->vw.n);
    if (desc->motion && !desc->prev_cameras) return fail(ctx, PT_ERR_INVALID, (fn + "motion needs prev_cameras").c_str());
    if (desc->prev_cameras) {
        if (desc->num_prev_cameras != ncams)
            return fail(ctx, PT_ERR_INVALID, (fn + "num_prev_cameras is " + std::to_string(desc->num_prev_cameras) + ", expected " + std::to_string(ncams) +
                                              (ctx->vw.n ? " (the view count)" : " (no views are set)")).c_str());
        for (size_t k = 0; k < (size_t)12 * ncams; ++k)
            if (!std::isfinite(desc->prev_cameras[k])) return fail(ctx, PT_ERR_INVALID, (fn + "prev_cameras: value " + std::to_string(k) + " is not finite").c_str());
    }
    int rc = subset_open(ctx, "pt_motion_planes", false, 0); // frames in flight and queued queries finish first; the block table for the mask
    if (rc) return rc;
    DevScope tmp;
    unsigned long long* d_counts = nullptr;
    float* d_prev = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    CK(tmp.alloc(&d_counts, 2));
    if (desc->motion) CK(tmp.alloc(&d_prev, (size_t)12 * ncams));
    CK(tmp.event(&ev0));
    CK(tmp.event(&ev1));
    pt_ctx::Blocks& B = ctx->blk;
    // (uploads and clears stay outside the timed span)
    CK(hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), ctx->stream));
    if (desc->motion) CK(hipMemcpyAsync(d_prev, desc->prev_cameras, sizeof(float) * 12 * ncams, hipMemcpyHostToDevice, ctx->stream));
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
        const MotionArgs ma{pixels, n, ctx->width, ctx->height, reinterpret_cast<const float*>(desc->hit), desc->prev_vertices, ctx->d_idx, ctx->ntri,
                            ctx->eye, ctx->U, ctx->V, ctx->W, d_prev, desc->motion, desc->prev_point, reinterpret_cast<float*>(desc->prev_surface), d_counts};
        const unsigned grid = (n + 255u) / 256u;
        if (ctx->vw.n) {
            const ViewParams vp{ctx->vw.d_vblock, ctx->vw.d_views, (uint32_t)(ctx->width + 7) / 8u};
            hipLaunchKernelGGL((k_motion<true>), dim3(grid), dim3(256), 0, ctx->stream, ma, vp);
        } else {
            hipLaunchKernelGGL((k_motion<false>), dim3(grid), dim3(256), 0, ctx->stream, ma, ViewParams{});
        }
    }
    // from here on the stream is waited for before the temporaries are freed, whatever fails
    unsigned long long h_counts[2] = {0, 0};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ev1, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_counts, d_counts, sizeof(h_counts), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    CK(e);
    CK(es);
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, ev0, ev1));
    if (stats) {
        stats->pixels = n;
        stats->hits = h_counts[0];
        stats->stale = h_counts[1];
        stats->kernel_ms = ms;
    }
    return PT_OK;
}
