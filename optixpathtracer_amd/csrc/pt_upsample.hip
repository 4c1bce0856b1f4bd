// pt_upsample_planes: the guided upsample of a low-resolution colour plane to the context's resolution (k_upsample).  Part of pt_lib.hip.
#include "pt_upsample.h"

extern "C" int pt_upsample_planes(pt_ctx* ctx, const pt_upsample_desc* desc, pt_upsample_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_upsample_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_upsample_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_upsample_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_upsample_planes: ";
    if (desc->flags != 0u) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags)).c_str());
    if (desc->scale < 2u || desc->scale > 4u) return fail(ctx, PT_ERR_INVALID, (fn + "scale must be in [2,4]").c_str());
    const uint32_t s = desc->scale;
    if ((uint64_t)desc->lo_width * s != (uint64_t)ctx->width || (uint64_t)desc->lo_height * s != (uint64_t)ctx->height)
        return fail(ctx, PT_ERR_INVALID, (fn + "the low-resolution size " + std::to_string(desc->lo_width) + " x " + std::to_string(desc->lo_height) + " times scale " + std::to_string(s) +
                                          " is not the frame's " + std::to_string(ctx->width) + " x " + std::to_string(ctx->height)).c_str());
    if (!(desc->normal_cos >= -1.f && desc->normal_cos <= 1.f)) return fail(ctx, PT_ERR_INVALID, (fn + "normal_cos must be in [-1,1]").c_str());
    if (!std::isfinite(desc->plane_eps) || !(desc->plane_eps >= 0.f)) return fail(ctx, PT_ERR_INVALID, (fn + "plane_eps must be finite and >= 0").c_str());
    // a view's low-resolution rectangle is the view divided by scale: every bound must divide
    for (uint32_t k = 0; k < ctx->vw.n; ++k) {
        const pt_view& v = ctx->vw.host[k];
        if (v.x % (int)s || v.y % (int)s || v.width % (int)s || v.height % (int)s)
            return fail(ctx, PT_ERR_INVALID, (fn + "view " + std::to_string(k) + " (x " + std::to_string(v.x) + ", y " + std::to_string(v.y) + ", " + std::to_string(v.width) + " x " +
                                              std::to_string(v.height) + ") is not a multiple of scale " + std::to_string(s)).c_str());
    }
    const size_t npix = (size_t)ctx->width * ctx->height, nlo = (size_t)desc->lo_width * desc->lo_height;
    // exclusive: may overlap no other plane (the two written ones); the read-only planes may alias one another
    const PassPlane planes[7] = {{"lo_color", desc->lo_color, nlo * 16, true, false},
                                 {"lo_hit", desc->lo_hit, nlo * sizeof(pt_hit), true, false},
                                 {"lo_position", desc->lo_position, nlo * 16, true, false},
                                 {"hit", desc->hit, npix * sizeof(pt_hit), true, false},
                                 {"position", desc->position, npix * 16, true, false},
                                 {"out", desc->out, npix * 16, true, true},
                                 {"weight_out", desc->weight_out, npix * 4, false, true}};
    int rc = pass_planes_check(ctx, "pt_upsample_planes", planes, 7);
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_upsample_planes", PASS_SLOT_BYTES); // per slot: hits, full, rescued, orphans
    if (rc) return rc;
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    if (n != 0) {
        const UpsampleArgs ua{run.pixels, n, ctx->width, ctx->height, (int)desc->lo_width, (int)s, desc->lo_color, reinterpret_cast<const float*>(desc->lo_hit),
                              desc->lo_position, reinterpret_cast<const float*>(desc->hit), desc->position, desc->out, desc->weight_out, desc->normal_cos,
                              desc->plane_eps, run.counts()};
        PASS_LAUNCH(run, (n + 255u) / 256u, 256, ua, k_upsample);
    }
    unsigned long long sum[4];
    rc = run.close_slots(sum, 4);
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->hits = sum[0];
        stats->full = sum[1];
        stats->rescued = sum[2];
        stats->orphans = sum[3];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}
