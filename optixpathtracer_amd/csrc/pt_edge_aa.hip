// pt_edge_aa_planes: geometric edge antialiasing of the chain's final image from the hit plane (k_edge_aa).  Part of pt_lib.hip.
#include "pt_edge_aa.h"

extern "C" int pt_edge_aa_planes(pt_ctx* ctx, const pt_edge_aa_desc* desc, pt_edge_aa_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_edge_aa_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_edge_aa_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_edge_aa_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_edge_aa_planes: ";
    if (desc->flags != 0u) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags)).c_str());
    if (!(desc->normal_cos >= -1.f && desc->normal_cos <= 1.f)) return fail(ctx, PT_ERR_INVALID, (fn + "normal_cos must be in [-1,1]").c_str());
    if (!std::isfinite(desc->plane_eps) || !(desc->plane_eps >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "plane_eps must be finite and >= 0").c_str());
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (the three written ones: the kernel gathers neighbours of color, so out may not be color);
    // the read-only planes may alias one another
    const PassPlane planes[6] = {{"color", desc->color, npix * 16, true, false},
                                 {"hit", desc->hit, npix * sizeof(pt_hit), true, false},
                                 {"position", desc->position, npix * 16, true, false},
                                 {"out", desc->out, npix * 16, true, true},
                                 {"edge", desc->edge, npix * 8, false, true},
                                 {"frame_rgba8", desc->frame_rgba8, npix * 4, false, true}};
    int rc = pass_planes_check(ctx, "pt_edge_aa_planes", planes, 6);
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_edge_aa_planes", PASS_SLOT_BYTES); // per slot: hits, stale, boundary, blended
    if (rc) return rc;
    const pt_ctx::Blocks& B = ctx->blk;
    const std::vector<uint8_t> inset = pass_block_set(ctx, desc->block_mask); // for the `block` test of the neighbours
    uint8_t* d_inset = nullptr;
    CK(run.tmp.alloc(&d_inset, (size_t)B.nblk));
    CK(hipMemcpyAsync(d_inset, inset.data(), B.nblk, hipMemcpyHostToDevice, ctx->stream));
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    if (n != 0) {
        const EdgeAaArgs ea{run.pixels, n, ctx->width, ctx->height, desc->color, reinterpret_cast<const float*>(desc->hit), desc->position, ctx->sc.d_idx, ctx->sc.d_verts,
                            ctx->ntri, ctx->eye, ctx->U, ctx->V, ctx->W, desc->out, desc->edge, desc->frame_rgba8, d_inset, B.nbx, desc->normal_cos, desc->plane_eps,
                            run.counts()};
        PASS_LAUNCH(run, (n + 255u) / 256u, 256, ea, k_edge_aa);
    }
    unsigned long long sum[4] = {};
    rc = run.close_slots(sum, 4);
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->hits = sum[0];
        stats->stale = sum[1];
        stats->boundary = sum[2];
        stats->blended = sum[3];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}
