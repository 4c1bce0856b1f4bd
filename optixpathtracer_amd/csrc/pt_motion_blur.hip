// pt_motion_blur_layout and pt_motion_blur_planes: the tile maxima (k_mblur_tile), the neighbourhood maxima (k_tile_neighbour<float2>) and
// the gather (k_mblur_gather) of every view, T and N in caller memory.  Part of pt_lib.hip.
#include "pt_motion_blur.h"

static_assert(PT_MOTION_BLUR_TILE == PASS_TILE, "pt_motion_blur_planes works on the tiled passes' tiles");

extern "C" int pt_motion_blur_layout(const pt_ctx* ctx, uint32_t* dims, size_t* bytes) { return pass_tile_layout(ctx, "pt_motion_blur_layout", 8, dims, bytes); }

extern "C" int pt_motion_blur_planes(pt_ctx* ctx, const pt_motion_blur_desc* desc, pt_motion_blur_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_motion_blur_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_motion_blur_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_motion_blur_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_motion_blur_planes: ";
    if (desc->flags & ~(uint32_t)PT_MOTION_BLUR_JITTER) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags & ~(uint32_t)PT_MOTION_BLUR_JITTER)).c_str());
    if (!std::isfinite(desc->shutter) || !(desc->shutter >= 0.f && desc->shutter <= 4.f)) return fail(ctx, PT_ERR_INVALID, (fn + "shutter must be finite and in [0,4]").c_str());
    if (!std::isfinite(desc->max_blur) || !(desc->max_blur >= 1.f && desc->max_blur <= (float)PT_MOTION_BLUR_TILE))
        return fail(ctx, PT_ERR_INVALID, (fn + "max_blur must be finite and in [1," + std::to_string(PT_MOTION_BLUR_TILE) + "]").c_str());
    if (!std::isfinite(desc->depth_soft) || !(desc->depth_soft > 0.f && desc->depth_soft <= 1.f)) return fail(ctx, PT_ERR_INVALID, (fn + "depth_soft must be finite and in (0,1]").c_str());
    if (desc->taps < 1u || desc->taps > 64u) return fail(ctx, PT_ERR_INVALID, (fn + "taps must be 1..64, not " + std::to_string(desc->taps)).c_str());
    std::vector<TileView> tab;
    const uint64_t texels = pass_tile_views(ctx, tab);
    const size_t npix = (size_t)ctx->width * ctx->height;
    const uint32_t nv = (uint32_t)tab.size();
    // exclusive: may overlap no other plane (the two written ones); out may not be color either: the gather reads neighbours
    const PassPlane planes[5] = {{"color", desc->color, npix * 16, true, false},
                                 {"motion", desc->motion, npix * 8, true, false},
                                 {"depth", desc->depth, npix * 4, true, false},
                                 {"out", desc->out, npix * 16, true, true},
                                 {"scratch", desc->scratch, (size_t)texels * 8, true, true}};
    int rc = pass_planes_check(ctx, "pt_motion_blur_planes", planes, 5);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(desc->scratch) & 7u) return fail(ctx, PT_ERR_INVALID, (fn + "scratch is not 8-byte aligned").c_str());
    const MblurParams k{0.5f * desc->shutter, desc->max_blur, desc->max_blur * desc->max_blur};
    const uint32_t tiles = pass_tile_max(tab);
    PassRun run;
    rc = run.open(ctx, "pt_motion_blur_planes", PASS_SLOT_BYTES); // per slot: sources, unknown, moving, taps, nonfinite
    if (rc) return rc;
    TileView* d_tab = nullptr;
    CK(run.tmp.alloc(&d_tab, tab.size()));
    CK(hipMemcpyAsync(d_tab, tab.data(), sizeof(TileView) * tab.size(), hipMemcpyHostToDevice, ctx->stream)); // (tab lives until the call has waited)
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    float2* scratch = reinterpret_cast<float2*>(desc->scratch);
    hipLaunchKernelGGL(k_mblur_tile, dim3((tiles + MBLUR_TILES_PER_BLOCK - 1u) / MBLUR_TILES_PER_BLOCK, nv), dim3(256), 0, ctx->stream, MblurTileArgs{d_tab, ctx->width, desc->motion, scratch, k, run.counts()});
    hipLaunchKernelGGL(k_tile_neighbour<float2>, dim3((tiles + 255u) / 256u, nv), dim3(256), 0, ctx->stream, TileNeighbourArgs<float2>{d_tab, scratch});
    if (n != 0) {
        const MblurGatherArgs ga{run.pixels, n, ctx->width, ctx->height, desc->color, desc->motion, desc->depth, desc->out, d_tab, scratch, k, desc->depth_soft,
                                 desc->taps, desc->seed, desc->flags & (uint32_t)PT_MOTION_BLUR_JITTER, run.counts()};
        PASS_LAUNCH(run, (n + 255u) / 256u, 256, ga, k_mblur_gather);
    }
    unsigned long long sum[5] = {};
    rc = run.close_slots(sum, 5);
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->sources = sum[0];
        stats->unknown = sum[1];
        stats->moving = sum[2];
        stats->taps = sum[3];
        stats->nonfinite = sum[4];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}
