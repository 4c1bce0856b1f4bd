// The library's device translation unit: the C ABI of pt_api.hip, then pt_render_gbuffer.
//
// pt_api.hip is included, not edited.  The entry point needs the context and the file-local helpers of pt_api.hip (the pointer checks of
// pt_trace_device, the block compaction of pt_render_mask, the drain of the frames in flight), so it lives in the same translation unit;
// but it adds no field to the context and changes no line of the frame path, and keeping that text as it is keeps what was measured on it
// attached to it (bench.py quotes counter figures only for the kernel sources they were collected on).  What the call needs beside the
// context — a counter block, the previous cameras, two events — is allocated per call and freed on every exit path (DevScope, as pt_trace
// does): a few small allocations of host time, outside the timed span.
#include "pt_api.hip"

#include "pt_gbuffer.h"

extern "C" int pt_render_gbuffer(pt_ctx* ctx, const pt_gbuffer_desc* desc, pt_gbuffer_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_render_gbuffer: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_render_gbuffer: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_render_gbuffer: no frame size yet (pt_resize)");
    struct Plane { const char* name; const void* p; size_t bytes; };
    const size_t npix = (size_t)ctx->width * ctx->height;
    const Plane planes[5] = {{"hit", desc->hit, npix * sizeof(pt_hit)}, {"depth", desc->depth, npix * 4}, {"position", desc->position, npix * 16},
                             {"motion", desc->motion, npix * 8}, {"ray", desc->ray, npix * 32}};
    if (!desc->hit && !desc->depth && !desc->position && !desc->motion && !desc->ray) return fail(ctx, PT_ERR_INVALID, "pt_render_gbuffer: no plane asked for (hit, depth, position, motion, ray are all null)");
    CK(hipSetDevice(ctx->device));
    {
        std::string err;
        for (const Plane& pl : planes)
            if (pl.p && query_pointer_validate(ctx, pl.p, pl.bytes, pl.name, err, "pt_render_gbuffer", "a device copy") != PT_OK) return fail(ctx, PT_ERR_INVALID, err.c_str());
        for (int i = 0; i < 5; ++i)
            for (int j = i + 1; j < 5; ++j) {
                const uintptr_t a = reinterpret_cast<uintptr_t>(planes[i].p), b = reinterpret_cast<uintptr_t>(planes[j].p);
                if (a && b && a < b + planes[j].bytes && b < a + planes[i].bytes)
                    return fail(ctx, PT_ERR_INVALID, (std::string("pt_render_gbuffer: ") + planes[i].name + " and " + planes[j].name + " overlap").c_str());
            }
    }
    const uint32_t ncams = std::max(1u, ctx->vw.n);
    if (desc->motion && !desc->prev_cameras) return fail(ctx, PT_ERR_INVALID, "pt_render_gbuffer: motion needs prev_cameras");
    if (desc->prev_cameras) {
        if (desc->num_prev_cameras != ncams)
            return fail(ctx, PT_ERR_INVALID, ("pt_render_gbuffer: num_prev_cameras is " + std::to_string(desc->num_prev_cameras) + ", expected " + std::to_string(ncams) +
                                              (ctx->vw.n ? " (the view count)" : " (no views are set)")).c_str());
        for (size_t k = 0; k < (size_t)12 * ncams; ++k)
            if (!std::isfinite(desc->prev_cameras[k])) return fail(ctx, PT_ERR_INVALID, ("pt_render_gbuffer: prev_cameras: value " + std::to_string(k) + " is not finite").c_str());
    }
    int rc = subset_open(ctx, "pt_render_gbuffer", false, 0); // frames in flight and queued queries finish first; the block table for the mask
    if (rc) return rc;
    // the call's own temporaries: QueryCounters (hits, fault) followed by 64 bytes for the packet counter, the previous cameras, two events
    DevScope tmp;
    uint8_t* block = nullptr;
    float* d_prev = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    CK(tmp.alloc(&block, sizeof(QueryCounters) + 64));
    if (desc->motion) CK(tmp.alloc(&d_prev, (size_t)12 * ncams));
    CK(tmp.event(&ev0));
    CK(tmp.event(&ev1));
    pt_ctx::Blocks& B = ctx->blk;
    QueryCounters* counters = reinterpret_cast<QueryCounters*>(block);
    uint32_t* work = reinterpret_cast<uint32_t*>(block + sizeof(QueryCounters));
    // (uploads and clears stay outside the timed span)
    CK(hipMemsetAsync(block, 0, sizeof(QueryCounters) + 64, ctx->stream));
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
        GBufferArgs ga{pixels, n, bvh_dev(ctx), ctx->d_tri_nrm, work, counters, ctx->width, ctx->height, ctx->eye, ctx->U, ctx->V, ctx->W,
                       d_prev, reinterpret_cast<float*>(desc->hit), desc->depth, desc->position, desc->motion, desc->ray};
        // the packet kernel at every size, its grid sized as launch_closest sizes k_trace8_cam's
        const unsigned tgrid = (unsigned)ctx->trace_grid;
        const unsigned grid = ctx->cam_grid > 0 ? (unsigned)ctx->cam_grid : std::max(1u, ctx->bvh.num_nodes8 < 256u ? tgrid * 2u / (unsigned)PT8_WAVES_PER_EU : tgrid);
        if (ctx->vw.n) {
            const ViewParams vp{ctx->vw.d_vblock, ctx->vw.d_views, (uint32_t)(ctx->width + 7) / 8u};
            hipLaunchKernelGGL((k_gbuffer<true>), dim3(grid), dim3(64), 0, ctx->stream, ga, vp);
        } else {
            hipLaunchKernelGGL((k_gbuffer<false>), dim3(grid), dim3(64), 0, ctx->stream, ga, ViewParams{});
        }
    }
    // from here on the stream is waited for before the temporaries are freed, whatever fails
    QueryCounters h_counters;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ev1, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_counters, block, sizeof(QueryCounters), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    CK(e);
    CK(es);
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, ev0, ev1));
    if (stats) {
        stats->pixels = n;
        stats->hits = 0;
        for (const QuerySlot& sl : h_counters.slot) stats->hits += sl.hits;
        stats->kernel_ms = ms;
    }
    if (h_counters.fault & 1u) return fail(ctx, PT_ERR_UNSUPPORTED, "pt_render_gbuffer: traversal stack overflow: the acceleration structure is deeper than the traversal stack");
    return PT_OK;
}
