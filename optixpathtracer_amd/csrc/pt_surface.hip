// pt_copy_texcoords_device and pt_surface_planes: the albedo and the texcoord under every pixel's centre, from the hit plane (k_surface).
// Part of pt_lib.hip.
#include "pt_surface.h"

// The per-primitive texcoords, back from the leaf-ordered records (pt_create frees its PrimUV array once they exist).  The builder emits
// one LeafTri per primitive (k_emit_tris: one per sorted Morton key) and the wide tree's leaves partition that array (k_collapse8 hands
// out counters[2] ranges that sum to n; no pad records, no spatial splits), so k_textris_to_uvs writes every primitive's six words
// exactly once — what pt_update_meshes(PT_UPDATE_REBUILD) already relies on.  num_tris8 == triangles is checked all the same.
extern "C" int pt_copy_texcoords_device(pt_ctx* ctx, float* dev_dst, size_t bytes) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_copy_texcoords_device: null context");
    if (bytes != sizeof(PrimUV) * (size_t)ctx->ntri)
        return fail(ctx, PT_ERR_INVALID, ("pt_copy_texcoords_device: bytes must equal triangles * 24 = " + std::to_string(sizeof(PrimUV) * (size_t)ctx->ntri)).c_str());
    CK(hipSetDevice(ctx->device));
    {
        std::string err;
        if (query_pointer_validate(ctx, dev_dst, bytes, "dev_dst", err, "pt_copy_texcoords_device", "a device copy") != PT_OK) return fail(ctx, PT_ERR_INVALID, err.c_str());
    }
    int rc = drain(ctx); // frames in flight and queued queries finish first
    if (rc) return rc;
    CK(hipSetDevice(ctx->device));
    if (!ctx->sc.d_textris) { // no textured mesh: no texcoord is ever read
        if (bytes) CK(hipMemsetAsync(dev_dst, 0, bytes, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        return PT_OK;
    }
    if (ctx->bvh.num_tris8 != ctx->ntri) return fail(ctx, PT_ERR_UNSUPPORTED, "pt_copy_texcoords_device: the tree does not hold one leaf record per primitive");
    DevOwner tmp;
    PrimUV* uvs = reinterpret_cast<PrimUV*>(dev_dst);
    const bool staged = (reinterpret_cast<uintptr_t>(dev_dst) & 7u) != 0; // the kernel stores 8-byte pairs: a 4-byte-aligned destination gets a copy
    if (staged) CK(tmp.alloc(&uvs, (size_t)ctx->ntri));
    hipLaunchKernelGGL(k_textris_to_uvs, dim3((ctx->ntri + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->bvh.tris8, ctx->sc.d_textris, ctx->ntri, uvs);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && staged) e = hipMemcpyAsync(dev_dst, uvs, bytes, hipMemcpyDeviceToDevice, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream); // before the temporary goes, on every path
    CK(e);
    CK(es);
    return PT_OK;
}

extern "C" int pt_surface_planes(pt_ctx* ctx, const pt_surface_desc* desc, pt_surface_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_surface_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_surface_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_surface_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_surface_planes: ";
    if (desc->flags != 0u) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags)).c_str());
    if (!desc->albedo && !desc->texcoord) return fail(ctx, PT_ERR_INVALID, (fn + "no plane asked for (albedo and texcoord are both null)").c_str());
    const bool tex = ctx->sc.d_textris != nullptr; // the scene has a textured mesh (d_mesh_tex exists with it)
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (the two written ones); hit and prim_texcoords are only read.  On an untextured scene
    // prim_texcoords is not looked at at all.
    const PassPlane planes[4] = {{"hit", desc->hit, npix * sizeof(pt_hit), true, false},
                                 {"prim_texcoords", tex ? desc->prim_texcoords : nullptr, sizeof(PrimUV) * (size_t)ctx->ntri, false, false},
                                 {"albedo", desc->albedo, npix * 16, false, true},
                                 {"texcoord", desc->texcoord, npix * 8, false, true}};
    int rc = pass_planes_check(ctx, "pt_surface_planes", planes, 4);
    if (rc) return rc;
    if (tex && !desc->prim_texcoords) return fail(ctx, PT_ERR_INVALID, (fn + "the scene has a textured mesh: prim_texcoords is required (pt_copy_texcoords_device)").c_str());
    PassRun run;
    rc = run.open(ctx, "pt_surface_planes", PASS_SLOT_BYTES); // per slot: hits, stale, textured
    if (rc) return rc;
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    if (n != 0) {
        const SurfaceArgs sa{run.pixels, n, ctx->width, reinterpret_cast<const float*>(desc->hit), ctx->sc.d_tri_mesh, ctx->ntri, ctx->sc.d_mats,
                             tex ? ctx->sc.d_mesh_tex : nullptr, tex ? desc->prim_texcoords : nullptr, tex ? ctx->sc.d_textures : nullptr,
                             desc->albedo, desc->texcoord, run.counts()};
        const unsigned grid = (n + 255u) / 256u;
        if (tex) hipLaunchKernelGGL(k_surface<true>, dim3(grid), dim3(256), 0, ctx->stream, sa);
        else hipLaunchKernelGGL(k_surface<false>, dim3(grid), dim3(256), 0, ctx->stream, sa);
    }
    unsigned long long sum[3];
    rc = run.close_slots(sum, 3);
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->hits = sum[0];
        stats->stale = sum[1];
        stats->textured = sum[2];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}
