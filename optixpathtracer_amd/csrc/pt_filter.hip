// pt_filter_planes: the chain's variance-guided a-trous filter (k_filter_prepare, k_filter_pass).  Part of pt_lib.hip.
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
    const size_t npix = (size_t)ctx->width * ctx->height;
    const int iters = desc->iterations;
    // exclusive: may overlap no other plane (the three written ones); the read-only planes may alias one another
    const PassPlane planes[8] = {{"color", desc->color, npix * 16, true, false},
                                 {"hit", desc->hit, npix * sizeof(pt_hit), true, false},
                                 {"position", desc->position, npix * 16, true, false},
                                 {"variance", desc->variance, npix * 4, false, false},
                                 {"length", desc->length, npix * 4, false, false},
                                 {"out", desc->out, npix * 16, true, true},
                                 {"scratch", desc->scratch, npix * 16, iters >= 1, true},
                                 {"frame_rgba8", desc->frame_rgba8, npix * 4, false, true}};
    int rc = pass_planes_check(ctx, "pt_filter_planes", planes, 8);
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_filter_planes", 2 * sizeof(unsigned long long)); // two counters: filtered, spatial
    if (rc) return rc;
    const pt_ctx::Blocks& B = ctx->blk;
    const std::vector<uint8_t> inset = pass_block_set(ctx, desc->block_mask); // for the `block` test of the taps
    uint8_t* d_inset = nullptr;
    CK(run.tmp.alloc(&d_inset, (size_t)B.nblk));
    CK(hipMemcpyAsync(d_inset, inset.data(), B.nblk, hipMemcpyHostToDevice, ctx->stream));
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    hipError_t e = hipSuccess;
    if (n != 0) {
        FilterArgs fa{run.pixels, n, ctx->width, ctx->height, desc->color, reinterpret_cast<const float*>(desc->hit), desc->position, desc->variance, desc->length,
                      nullptr, nullptr, nullptr, d_inset, B.nbx, desc->sigma_lum, desc->normal_cos, desc->plane_eps, (float)desc->min_length, 1, 0u, run.counts()};
        const unsigned grid = (n + 255u) / 256u;
        // stage k of iters + 1 writes `out` when the number of stages after it is even: the last one always does
        float* bufs[2] = {desc->out, desc->scratch};
        for (int k = 0; k <= iters && e == hipSuccess; ++k) {
            fa.src = k ? bufs[(iters - k + 1) & 1] : nullptr;
            fa.dst = bufs[(iters - k) & 1];
            fa.last = k == iters ? 1u : 0u;
            fa.frame = k == iters ? desc->frame_rgba8 : nullptr;
            fa.step = k ? 1 << (k - 1) : 1;
            if (k == 0) PASS_LAUNCH(run, grid, 256, fa, k_filter_prepare);
            else PASS_LAUNCH(run, grid, 256, fa, k_filter_pass);
            e = hipGetLastError();
        }
    }
    unsigned long long h_counts[2] = {0, 0};
    rc = run.close(e, h_counts, sizeof(h_counts));
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->filtered = h_counts[0];
        stats->spatial = h_counts[1];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}
