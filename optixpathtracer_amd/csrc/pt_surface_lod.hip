// pt_texture_mips_layout, pt_copy_texture_mips_device, pt_surface_lod_planes and pt_surface_aniso_planes: the mip pyramid of the context's
// textures in caller memory (k_mip_from_tiles, k_mip_reduce) and the footprint-filtered albedo under every pixel's centre, with one lookup
// (k_surface_lod) or several along the footprint's longer axis (k_surface_aniso).  Part of pt_lib.hip.
#include "pt_surface_lod.h"

// The context keeps its texture records on the device only (DevTex: w, h next to the tiles' address); they never change after pt_create.
// Every size below comes from them, so no level address depends on anything the caller passes.  They are fetched on the context's stream:
// a blocking hipMemcpy runs on the null stream and made every call wait for whatever the caller had enqueued there.
static int lod_textures(pt_ctx* ctx, std::vector<DevTex>& tex) {
    tex.resize(ctx->sc.d_tex_pixels.size());
    if (tex.empty()) return PT_OK;
    CK(hipSetDevice(ctx->device));
    CK(hipMemcpyAsync(tex.data(), ctx->sc.d_textures, sizeof(DevTex) * tex.size(), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return PT_OK;
}
static int lod_layout_of(pt_ctx* ctx, const char* fn, std::vector<DevTex>& tex, std::vector<uint32_t>& dims, size_t* bytes) {
    const int rc = lod_textures(ctx, tex);
    if (rc) return rc;
    std::vector<int> wh(2 * tex.size());
    for (size_t t = 0; t < tex.size(); ++t) wh[2 * t] = tex[t].w, wh[2 * t + 1] = tex[t].h;
    dims.assign(4 * tex.size(), 0u);
    const uint64_t texels = lod_layout(wh.data(), (uint32_t)tex.size(), dims.data());
    if (texels > 0xffffffffull) return fail(ctx, PT_ERR_UNSUPPORTED, (std::string(fn) + ": the pyramid has more than 2^32 - 1 texels").c_str());
    *bytes = (size_t)texels * 16;
    return PT_OK;
}

extern "C" int pt_texture_mips_layout(const pt_ctx* cctx, uint32_t* textures, uint32_t* dims, size_t* bytes) {
    if (!cctx) return fail(nullptr, PT_ERR_INVALID, "pt_texture_mips_layout: null context");
    pt_ctx* ctx = const_cast<pt_ctx*>(cctx); // (the error text and the device selection only)
    std::vector<DevTex> tex;
    std::vector<uint32_t> d;
    size_t b = 0;
    const int rc = lod_layout_of(ctx, "pt_texture_mips_layout", tex, d, &b);
    if (rc) return rc;
    if (textures) *textures = (uint32_t)tex.size();
    if (dims && !d.empty()) memcpy(dims, d.data(), sizeof(uint32_t) * d.size());
    if (bytes) *bytes = b;
    return PT_OK;
}

extern "C" int pt_copy_texture_mips_device(pt_ctx* ctx, void* dev_dst, size_t bytes) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_copy_texture_mips_device: null context");
    std::vector<DevTex> tex;
    std::vector<uint32_t> dims;
    size_t want = 0;
    int rc = lod_layout_of(ctx, "pt_copy_texture_mips_device", tex, dims, &want);
    if (rc) return rc;
    if (bytes != want) return fail(ctx, PT_ERR_INVALID, ("pt_copy_texture_mips_device: bytes must equal pt_texture_mips_layout's " + std::to_string(want)).c_str());
    if (bytes == 0) return PT_OK; // no texture, or 1 x 1 textures only: there is no level above 0
    CK(hipSetDevice(ctx->device));
    {
        std::string err;
        if (query_pointer_validate(ctx, dev_dst, bytes, "dev_dst", err, "pt_copy_texture_mips_device", "a device copy") != PT_OK) return fail(ctx, PT_ERR_INVALID, err.c_str());
    }
    if (reinterpret_cast<uintptr_t>(dev_dst) & 15u) return fail(ctx, PT_ERR_INVALID, "pt_copy_texture_mips_device: dev_dst is not 16-byte aligned");
    rc = drain(ctx); // frames in flight and queued queries finish first
    if (rc) return rc;
    CK(hipSetDevice(ctx->device));
    float4* base = reinterpret_cast<float4*>(dev_dst);
    for (size_t t = 0; t < tex.size(); ++t) {
        const uint32_t w = dims[4 * t], h = dims[4 * t + 1], levels = dims[4 * t + 2];
        float4* dst = base + dims[4 * t + 3];
        const float4* src = nullptr;
        for (uint32_t k = 1; k < levels; ++k) { // one launch per level: level k is complete before level k + 1 reads it
            const uint32_t wd = lod_dim(w, k), hd = lod_dim(h, k);
            const unsigned grid = (unsigned)(((uint64_t)wd * hd + 255u) / 256u);
            if (k == 1) hipLaunchKernelGGL(k_mip_from_tiles, dim3(grid), dim3(256), 0, ctx->stream, tex[t], dst, wd, hd);
            else hipLaunchKernelGGL(k_mip_reduce, dim3(grid), dim3(256), 0, ctx->stream, src, lod_dim(w, k - 1), lod_dim(h, k - 1), dst, wd, hd);
            src = dst;
            dst += (size_t)wd * hd;
        }
    }
    const hipError_t e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    CK(e);
    CK(es);
    return PT_OK;
}

// What pt_surface_lod_planes and pt_surface_aniso_planes share on the host: every check behind the null tests, the level_first upload,
// the pixel set, the launch and the counters.  aniso = false is the isotropic pass (k_surface_lod, four counters, no taps plane, no max_aniso).
struct LodCall {
    const char* name;
    const void* hit;
    const float* prim_texcoords;
    const void* mips;
    size_t mips_bytes;
    float *albedo, *texcoord, *footprint, *lod, *taps;
    const uint8_t* block_mask;
    float footprint_scale;
    uint32_t flags, max_aniso;
    bool aniso;
};
static int lod_call(pt_ctx* ctx, const LodCall& d, unsigned long long (&sum)[6], uint32_t* pixels, double* ms) {
    const bool aniso = d.aniso;
    const std::string fn = std::string(d.name) + ": ";
    if (d.flags != 0u) return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(d.flags)).c_str());
    if (aniso && (d.max_aniso < 1u || d.max_aniso > 16u)) return fail(ctx, PT_ERR_INVALID, (fn + "max_aniso must be 1..16, not " + std::to_string(d.max_aniso)).c_str());
    if (!d.albedo && !d.texcoord && !d.footprint && !d.lod && !d.taps)
        return fail(ctx, PT_ERR_INVALID, (fn + "no plane asked for (albedo, texcoord, footprint, lod" + (aniso ? ", taps" : "") + " are all null)").c_str());
    if (!(std::isfinite(d.footprint_scale) && d.footprint_scale >= 0.0f)) return fail(ctx, PT_ERR_INVALID, (fn + "footprint_scale must be finite and >= 0").c_str());
    const bool tex = ctx->sc.d_textris != nullptr; // the scene has a textured mesh (d_mesh_tex exists with it)
    std::vector<DevTex> textures;
    std::vector<uint32_t> dims;
    size_t mips_bytes = 0;
    int rc = PT_OK;
    if (tex) rc = lod_layout_of(ctx, d.name, textures, dims, &mips_bytes);
    if (rc) return rc;
    const bool pyr = tex && mips_bytes != 0;
    if (pyr && d.mips && d.mips_bytes != mips_bytes)
        return fail(ctx, PT_ERR_INVALID, (fn + "mips_bytes must equal pt_texture_mips_layout's " + std::to_string(mips_bytes)).c_str());
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (the written ones); hit, prim_texcoords and mips are only read.  On an untextured scene
    // prim_texcoords and mips are not looked at at all, nor is mips where no texture has a level above 0.
    const PassPlane planes[8] = {{"hit", d.hit, npix * sizeof(pt_hit), true, false},
                                 {"prim_texcoords", tex ? d.prim_texcoords : nullptr, sizeof(PrimUV) * (size_t)ctx->ntri, false, false},
                                 {"mips", pyr ? d.mips : nullptr, mips_bytes, false, false},
                                 {"albedo", d.albedo, npix * 16, false, true},
                                 {"texcoord", d.texcoord, npix * 8, false, true},
                                 {"footprint", d.footprint, npix * 16, false, true},
                                 {"lod", d.lod, npix * 4, false, true},
                                 {"taps", d.taps, npix * 4, false, true}};
    rc = pass_planes_check(ctx, d.name, planes, aniso ? 8 : 7);
    if (rc) return rc;
    if (tex && !d.prim_texcoords) return fail(ctx, PT_ERR_INVALID, (fn + "the scene has a textured mesh: prim_texcoords is required (pt_copy_texcoords_device)").c_str());
    if (pyr && !d.mips) return fail(ctx, PT_ERR_INVALID, (fn + "the scene has a textured mesh: mips is required (pt_copy_texture_mips_device)").c_str());
    if (pyr && (reinterpret_cast<uintptr_t>(d.mips) & 15u)) return fail(ctx, PT_ERR_INVALID, (fn + "mips is not 16-byte aligned").c_str());
    // The first texel of every level >= 1, from the context's sizes: 128 bytes per texture behind the counter slots, in the call's one
    // temporary allocation.  `first` outlives the run (declared in front of it), so the upload needs no wait of its own.
    std::vector<uint32_t> first;
    if (tex) {
        first.assign(textures.size() * LOD_MAX_LEVELS, 0u);
        for (size_t t = 0; t < textures.size(); ++t) {
            uint32_t at = dims[4 * t + 3];
            for (uint32_t k = 1; k < dims[4 * t + 2]; ++k) {
                first[t * LOD_MAX_LEVELS + k] = at;
                at += lod_dim(dims[4 * t], k) * lod_dim(dims[4 * t + 1], k);
            }
        }
    }
    const size_t slot_bytes = PASS_SLOT_BYTES; // per slot: hits, stale, textured, minified (anisotropic, taps beyond the first)
    PassRun run;
    rc = run.open(ctx, d.name, slot_bytes + sizeof(uint32_t) * first.size());
    if (rc) return rc;
    const uint32_t* d_first = nullptr;
    if (tex) {
        d_first = reinterpret_cast<const uint32_t*>(run.d_counters + slot_bytes);
        CK(hipMemcpyAsync(run.d_counters + slot_bytes, first.data(), sizeof(uint32_t) * first.size(), hipMemcpyHostToDevice, ctx->stream));
    }
    rc = run.select(d.block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    if (n != 0) {
        const SurfaceLodArgs sa{run.pixels, n, ctx->width, ctx->height, reinterpret_cast<const float*>(d.hit), ctx->sc.d_tri_mesh, ctx->ntri, ctx->sc.d_mats,
                                tex ? ctx->sc.d_mesh_tex : nullptr, tex ? d.prim_texcoords : nullptr, tex ? ctx->sc.d_textures : nullptr,
                                tex ? ctx->sc.d_idx : nullptr, tex ? ctx->sc.d_verts : nullptr, pyr ? reinterpret_cast<const float4*>(d.mips) : nullptr, d_first,
                                ctx->eye, ctx->U, ctx->V, ctx->W, d.footprint_scale, d.albedo, d.texcoord, d.footprint, d.lod, run.counts()};
        const unsigned grid = (n + 255u) / 256u;
        if (aniso) {
            const SurfaceAnisoArgs aa{sa, d.taps, d.max_aniso};
            if (tex) PASS_LAUNCH(run, grid, 256, aa, k_surface_aniso, true);
            else PASS_LAUNCH(run, grid, 256, aa, k_surface_aniso, false);
        } else {
            if (tex) PASS_LAUNCH(run, grid, 256, sa, k_surface_lod, true);
            else PASS_LAUNCH(run, grid, 256, sa, k_surface_lod, false);
        }
    }
    rc = run.close_slots(sum, aniso ? 6 : 4);
    if (rc) return rc;
    *pixels = n;
    *ms = run.ms;
    return PT_OK;
}

extern "C" int pt_surface_lod_planes(pt_ctx* ctx, const pt_surface_lod_desc* desc, pt_surface_lod_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_surface_lod_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_surface_lod_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_surface_lod_planes: no frame size yet (pt_resize)");
    const LodCall d{"pt_surface_lod_planes", desc->hit, desc->prim_texcoords, desc->mips, desc->mips_bytes, desc->albedo, desc->texcoord, desc->footprint,
                    desc->lod, nullptr, desc->block_mask, desc->footprint_scale, desc->flags, 0u, false};
    unsigned long long sum[6] = {};
    uint32_t n = 0;
    double ms = 0.0;
    const int rc = lod_call(ctx, d, sum, &n, &ms);
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->hits = sum[0];
        stats->stale = sum[1];
        stats->textured = sum[2];
        stats->minified = sum[3];
        stats->kernel_ms = ms;
    }
    return PT_OK;
}

extern "C" int pt_surface_aniso_planes(pt_ctx* ctx, const pt_surface_aniso_desc* desc, pt_surface_aniso_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_surface_aniso_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_surface_aniso_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_surface_aniso_planes: no frame size yet (pt_resize)");
    const LodCall d{"pt_surface_aniso_planes", desc->hit, desc->prim_texcoords, desc->mips, desc->mips_bytes, desc->albedo, desc->texcoord, desc->footprint,
                    desc->lod, desc->taps, desc->block_mask, desc->footprint_scale, desc->flags, desc->max_aniso, true};
    unsigned long long sum[6] = {};
    uint32_t n = 0;
    double ms = 0.0;
    const int rc = lod_call(ctx, d, sum, &n, &ms);
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->hits = sum[0];
        stats->stale = sum[1];
        stats->textured = sum[2];
        stats->minified = sum[3];
        stats->anisotropic = sum[4];
        stats->taps = sum[2] + sum[5]; // one tap per textured pixel, and the taps beyond it
        stats->kernel_ms = ms;
    }
    return PT_OK;
}
