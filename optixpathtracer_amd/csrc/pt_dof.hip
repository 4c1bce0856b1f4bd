// pt_dof_layout and pt_dof_planes: the tile maxima (k_dof_tile), the neighbourhood maxima (k_tile_neighbour<float>) and the gather
// (k_dof_gather) of every view, T and N in caller memory.  Part of pt_lib.hip.
#include "pt_dof.h"

static_assert(PT_DOF_TILE == PASS_TILE, "pt_dof_planes works on the tiled passes' tiles");

// The header's D (pass_spiral, pt_pass.h) and rho, operation for operation.
static void dof_taps(DofTaps& t, uint32_t taps) {
    pass_spiral(t.D);
    const float ftaps = (float)taps;
    for (uint32_t i = 0; i < 64u; ++i) t.rho[i] = i < taps ? sqrtf(((float)i + 0.5f) / ftaps) : 0.0f;
}

extern "C" int pt_dof_layout(const pt_ctx* ctx, uint32_t* dims, size_t* bytes) { return pass_tile_layout(ctx, "pt_dof_layout", 4, dims, bytes); }

extern "C" int pt_dof_planes(pt_ctx* ctx, const pt_dof_desc* desc, pt_dof_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_dof_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_dof_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_dof_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_dof_planes: ";
    if (desc->flags & ~(uint32_t)PT_DOF_JITTER) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags & ~(uint32_t)PT_DOF_JITTER)).c_str());
    const auto focus_ok = [](float f) { return std::isfinite(f) && f > 0.f && f <= 1e30f; };
    if (!focus_ok(desc->focus)) return fail(ctx, PT_ERR_INVALID, (fn + "focus must be finite and in (0,1e30]").c_str());
    if (!std::isfinite(desc->aperture) || !(desc->aperture >= 0.f && desc->aperture <= 4096.f)) return fail(ctx, PT_ERR_INVALID, (fn + "aperture must be finite and in [0,4096]").c_str());
    if (!std::isfinite(desc->max_radius) || !(desc->max_radius >= 1.f && desc->max_radius <= (float)PT_DOF_TILE))
        return fail(ctx, PT_ERR_INVALID, (fn + "max_radius must be finite and in [1," + std::to_string(PT_DOF_TILE) + "]").c_str());
    if (desc->taps < 1u || desc->taps > 64u) return fail(ctx, PT_ERR_INVALID, (fn + "taps must be 1..64, not " + std::to_string(desc->taps)).c_str());
    std::vector<TileView> tab;
    const uint64_t texels = pass_tile_views(ctx, tab);
    const uint32_t nv = (uint32_t)tab.size();
    for (uint32_t v = 0; v < nv; ++v) { // aux: Fv
        tab[v].aux = desc->view_focus ? desc->view_focus[v] : desc->focus;
        if (!focus_ok(tab[v].aux)) return fail(ctx, PT_ERR_INVALID, (fn + "view_focus[" + std::to_string(v) + "] must be finite and in (0,1e30]").c_str());
    }
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (the two written ones); out may not be color either: the gather reads neighbours
    const PassPlane planes[4] = {{"color", desc->color, npix * 16, true, false},
                                 {"depth", desc->depth, npix * 4, true, false},
                                 {"out", desc->out, npix * 16, true, true},
                                 {"scratch", desc->scratch, (size_t)texels * 4, true, true}};
    int rc = pass_planes_check(ctx, "pt_dof_planes", planes, 4);
    if (rc) return rc;
    const DofParams k{desc->aperture + 0.0f, desc->max_radius};
    const uint32_t tiles = pass_tile_max(tab);
    DofTaps tt;
    dof_taps(tt, desc->taps);
    PassRun run;
    rc = run.open(ctx, "pt_dof_planes", PASS_SLOT_BYTES); // per slot: sources, gathered, taps, nonfinite
    if (rc) return rc;
    TileView* d_tab = nullptr;
    DofTaps* d_tt = nullptr;
    CK(run.tmp.alloc(&d_tab, tab.size()));
    CK(run.tmp.alloc(&d_tt, 1));
    CK(hipMemcpyAsync(d_tab, tab.data(), sizeof(TileView) * tab.size(), hipMemcpyHostToDevice, ctx->stream)); // (tab and tt live until the call has waited)
    CK(hipMemcpyAsync(d_tt, &tt, sizeof(DofTaps), hipMemcpyHostToDevice, ctx->stream));
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    float* scratch = reinterpret_cast<float*>(desc->scratch);
    hipLaunchKernelGGL(k_dof_tile, dim3((tiles + DOF_TILES_PER_BLOCK - 1u) / DOF_TILES_PER_BLOCK, nv), dim3(256), 0, ctx->stream, DofTileArgs{d_tab, ctx->width, desc->depth, scratch, k, run.counts()});
    hipLaunchKernelGGL(k_tile_neighbour<float>, dim3((tiles + 255u) / 256u, nv), dim3(256), 0, ctx->stream, TileNeighbourArgs<float>{d_tab, scratch});
    if (n != 0) {
        const DofGatherArgs ga{run.pixels, n, ctx->width, ctx->height, desc->color, desc->depth, desc->out, d_tab, d_tt, scratch, k,
                               desc->taps, desc->seed, desc->flags & (uint32_t)PT_DOF_JITTER, run.counts()};
        PASS_LAUNCH(run, (n + 255u) / 256u, 256, ga, k_dof_gather);
    }
    unsigned long long sum[4] = {};
    rc = run.close_slots(sum, 4);
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->sources = sum[0];
        stats->gathered = sum[1];
        stats->taps = sum[2];
        stats->nonfinite = sum[3];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}
