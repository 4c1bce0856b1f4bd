// pt_vertex_count, pt_copy_vertices_device and pt_motion_planes: where each pixel's surface point was before the geometry moved
// (k_motion).  Part of pt_lib.hip.
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
    if (bytes) CK(hipMemcpyAsync(dev_dst, ctx->sc.d_verts, bytes, hipMemcpyDeviceToDevice, ctx->stream));
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
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (the three written ones); hit and prev_vertices are only read
    const PassPlane planes[5] = {{"hit", desc->hit, npix * sizeof(pt_hit), true, false},
                                 {"prev_vertices", desc->prev_vertices, sizeof(float) * 3 * ctx->nvert, true, false},
                                 {"motion", desc->motion, npix * 8, false, true},
                                 {"prev_point", desc->prev_point, npix * 16, false, true},
                                 {"prev_surface", desc->prev_surface, npix * sizeof(pt_hit), false, true}};
    int rc = pass_planes_check(ctx, "pt_motion_planes", planes, 5);
    if (rc) return rc;
    rc = pass_prev_cameras_check(ctx, "pt_motion_planes", desc->motion, desc->prev_cameras, desc->num_prev_cameras);
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_motion_planes", 2 * sizeof(unsigned long long)); // two counters: hits, stale
    if (rc) return rc;
    float* d_prev = nullptr;
    if (desc->motion) {
        const size_t nprev = (size_t)12 * pass_camera_count(ctx);
        CK(run.tmp.alloc(&d_prev, nprev));
        CK(hipMemcpyAsync(d_prev, desc->prev_cameras, sizeof(float) * nprev, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    if (n != 0) {
        const MotionArgs ma{run.pixels, n, ctx->width, ctx->height, reinterpret_cast<const float*>(desc->hit), desc->prev_vertices, ctx->sc.d_idx, ctx->ntri,
                            ctx->eye, ctx->U, ctx->V, ctx->W, d_prev, desc->motion, desc->prev_point, reinterpret_cast<float*>(desc->prev_surface), run.counts()};
        const unsigned grid = (n + 255u) / 256u;
        PASS_LAUNCH(run, grid, 256, ma, k_motion);
    }
    unsigned long long h_counts[2] = {0, 0};
    rc = run.close(hipSuccess, h_counts, sizeof(h_counts));
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->hits = h_counts[0];
        stats->stale = h_counts[1];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}
