// pt_render_gbuffer: the first hit under the centre of every pixel, written by one packet kernel (k_gbuffer).  Part of pt_lib.hip.
#include "pt_gbuffer.h"

extern "C" int pt_render_gbuffer(pt_ctx* ctx, const pt_gbuffer_desc* desc, pt_gbuffer_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_render_gbuffer: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_render_gbuffer: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_render_gbuffer: no frame size yet (pt_resize)");
    const size_t npix = (size_t)ctx->width * ctx->height;
    // all optional, all written
    const PassPlane planes[5] = {{"hit", desc->hit, npix * sizeof(pt_hit), false, true},
                                 {"depth", desc->depth, npix * 4, false, true},
                                 {"position", desc->position, npix * 16, false, true},
                                 {"motion", desc->motion, npix * 8, false, true},
                                 {"ray", desc->ray, npix * 32, false, true}};
    if (!desc->hit && !desc->depth && !desc->position && !desc->motion && !desc->ray) return fail(ctx, PT_ERR_INVALID, "pt_render_gbuffer: no plane asked for (hit, depth, position, motion, ray are all null)");
    int rc = pass_planes_check(ctx, "pt_render_gbuffer", planes, 5);
    if (rc) return rc;
    rc = pass_prev_cameras_check(ctx, "pt_render_gbuffer", desc->motion, desc->prev_cameras, desc->num_prev_cameras);
    if (rc) return rc;
    // the counters: QueryCounters (hits, fault) followed by 64 bytes for the packet counter
    PassRun run;
    rc = run.open(ctx, "pt_render_gbuffer", sizeof(QueryCounters) + 64);
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
        QueryCounters* counters = reinterpret_cast<QueryCounters*>(run.d_counters);
        uint32_t* work = reinterpret_cast<uint32_t*>(run.d_counters + sizeof(QueryCounters));
        GBufferArgs ga{run.pixels, n, bvh_dev(ctx), ctx->sc.d_tri_nrm, work, counters, ctx->width, ctx->height, ctx->eye, ctx->U, ctx->V, ctx->W,
                       d_prev, reinterpret_cast<float*>(desc->hit), desc->depth, desc->position, desc->motion, desc->ray};
        // the packet kernel at every size, its grid sized as launch_closest sizes k_trace8_cam's
        const unsigned tgrid = (unsigned)ctx->trace_grid;
        const unsigned grid = ctx->cam_grid > 0 ? (unsigned)ctx->cam_grid : std::max(1u, ctx->bvh.num_nodes8 < 256u ? tgrid * 2u / (unsigned)PT8_WAVES_PER_EU : tgrid);
        PASS_LAUNCH(run, grid, 64, ga, k_gbuffer);
    }
    QueryCounters h_counters;
    rc = run.close(hipSuccess, &h_counters, sizeof(h_counters));
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->hits = 0;
        for (const QuerySlot& sl : h_counters.slot) stats->hits += sl.hits;
        stats->kernel_ms = run.ms;
    }
    if (h_counters.fault & 1u) return fail(ctx, PT_ERR_UNSUPPORTED, "pt_render_gbuffer: traversal stack overflow: the acceleration structure is deeper than the traversal stack");
    return PT_OK;
}
