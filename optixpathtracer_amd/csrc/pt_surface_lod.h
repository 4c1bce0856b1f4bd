// pt_texture_mips_layout, pt_copy_texture_mips_device, pt_surface_lod_planes and pt_surface_aniso_planes (include/pt_amd.h): a box-filtered
// mip pyramid of the context's textures in caller memory, and the albedo under every pixel's centre filtered over the pixel's footprint in
// texture space — pt_surface_planes with a level of detail (k_surface_lod), and with several taps along the footprint's longer axis
// (k_surface_aniso).  Stateless, every plane the caller's.
//
// The first part is host only and needs no HIP header (tests/test_surface_lod_cabi.py compiles it with a host compiler alone).
#pragma once
#include <cstddef>
#include <cstdint>

#define LOD_MAX_LEVELS 32u // 1 + floor(log2(max(w, h))) of int sizes

static inline uint32_t lod_levels(uint32_t w, uint32_t h) {
    uint32_t m = w > h ? w : h, l = 1;
    while (m >>= 1) ++l;
    return l;
}
static inline uint32_t lod_dim(uint32_t w, uint32_t k) { return (w >> k) ? (w >> k) : 1u; }
// The pyramid of n textures (wh: n x 2, width then height): for textures in order, levels 1 .. levels-1, each row-major and contiguous.
// dims (n x 4, may be null): w, h, levels, the index of the first texel of level 1.  Returns the texels of the whole pyramid.
static inline uint64_t lod_layout(const int* wh, uint32_t n, uint32_t* dims) {
    uint64_t texels = 0;
    for (uint32_t t = 0; t < n; ++t) {
        const uint32_t w = (uint32_t)wh[2 * t], h = (uint32_t)wh[2 * t + 1], levels = lod_levels(w, h);
        if (dims) {
            dims[4 * t] = w;
            dims[4 * t + 1] = h;
            dims[4 * t + 2] = levels;
            dims[4 * t + 3] = (uint32_t)texels;
        }
        for (uint32_t k = 1; k < levels; ++k) texels += (uint64_t)lod_dim(w, k) * lod_dim(h, k);
    }
    return texels;
}

#ifdef __HIPCC__
#include "pt_pass_dev.h"

// ------------------------------------------------------------------ the pyramid
// One thread per texel of the level written, 256 per block, one launch per level: a kernel boundary is the only ordering needed.  Texel
// (i, j) of level k+1 is ((S(2i, 2j) + S(i1, 2j)) + (S(2i, j1) + S(i1, j1))) * 0.25f with i1 = min(2i + 1, w_k - 1), j1 = min(2j + 1,
// h_k - 1): every source index lies inside level k whatever the sizes are.  An odd dimension drops its last row or column.
__global__ void __launch_bounds__(256) k_mip_from_tiles(DevTex tx, float4* dst, uint32_t wd, uint32_t hd) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= wd * hd) return;
    const uint32_t i = q % wd, j = q / wd;
    const int i0 = (int)(2u * i), j0 = (int)(2u * j);
    const int i1 = min(i0 + 1, tx.w - 1), j1 = min(j0 + 1, tx.h - 1);
    const uint32_t t00 = tx.pixel[tex_tiled_index(i0, j0, tx.tiles_x)], t10 = tx.pixel[tex_tiled_index(i1, j0, tx.tiles_x)],
                   t01 = tx.pixel[tex_tiled_index(i0, j1, tx.tiles_x)], t11 = tx.pixel[tex_tiled_index(i1, j1, tx.tiles_x)];
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = ((texel_ch(t00, k) + texel_ch(t10, k)) + (texel_ch(t01, k) + texel_ch(t11, k))) * 0.25f;
    dst[q] = make_float4(o[0], o[1], o[2], o[3]);
#endif
}
__global__ void __launch_bounds__(256) k_mip_reduce(const float4* src, uint32_t ws, uint32_t hs, float4* dst, uint32_t wd, uint32_t hd) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= wd * hd) return;
    const uint32_t i = q % wd, j = q / wd;
    const uint32_t i0 = 2u * i, j0 = 2u * j;
    const uint32_t i1 = min(i0 + 1u, ws - 1u), j1 = min(j0 + 1u, hs - 1u);
    const float4 a = src[(size_t)j0 * ws + i0], b = src[(size_t)j0 * ws + i1], c = src[(size_t)j1 * ws + i0], d = src[(size_t)j1 * ws + i1];
    dst[q] = make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f, ((a.z + b.z) + (c.z + d.z)) * 0.25f,
                         ((a.w + b.w) + (c.w + d.w)) * 0.25f);
#endif
}

// ------------------------------------------------------------------ the pass
// One thread per entry of the frame's pixel list, 256 threads per block, no scratch: the shape of k_surface.  Loads go cheapest first and
// each one decides whether the next is needed: the first 16 bytes of the hit record, on a hit in range the primitive's mesh and the three
// colour words of its material, and only on a textured mesh the primitive's 24 bytes of texcoords, its three indices and nine floats of the
// context's CURRENT vertices, the view's camera, the texture's sizes and the texels of one or two levels: level 0 from the RGBA8 tiles
// through the 256 values (float)b / 255.0f in LDS (1 KiB), a level >= 1 by four 16-byte loads of the pyramid.  A miss stops after 16
// bytes; an untextured mesh reads no vertex.  It writes up to 16 + 8 + 16 + 4 bytes.
//
// The arithmetic is the header's, in the header's order, one float32 rounding per operation (-ffp-contract=off is part of the library's
// flags); the camera lookup is k_motion's, RESTATED.  The primitive word of the hit plane is caller memory: it is compared with the triangle
// count before any address is formed from it.  Every level address comes from level_first (built by the host from the context's own texture
// sizes) and the DevTex record, never from caller memory; the texel indices are clamped into the level before any texel is read.
struct SurfaceLodArgs {
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    int width, height;          // the frame: the planes are indexed Y * width + X
    const float* hit;           // this frame's hit plane
    const uint32_t* tri_mesh;   // [triangles] the context's mesh of every primitive
    uint32_t ntri;
    const pt_material* mats;    // [meshes]
    const int32_t* mesh_tex;    // [meshes] texture id or -1 (TEX only)
    const float* prim_uv;       // [triangles][6], the caller's table (TEX only)
    const DevTex* textures;     // (TEX only)
    const uint32_t* idx;        // [triangles][3] global vertex indices (TEX only)
    const float* verts;         // [vertices][3] the context's current vertices (TEX only)
    const float4* mips;         // the caller's pyramid (TEX only; null when every texture is 1 x 1)
    const uint32_t* level_first; // [textures][LOD_MAX_LEVELS] the first texel of level k >= 1 in the pyramid (TEX only)
    v3 eye, U, V, W;            // the frame's camera (unused with views)
    float scale;                // footprint_scale
    float *albedo, *texcoord, *footprint, *lod; // the planes, null = not asked for
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] hits, [1] stale, [2] textured, [3] minified of a slot (pass_slot); zero at launch
};

// the header's tex2D on level k >= 1: W x H float4 texels, row-major
PT_DEV float4 lod_tex2d(const float4* T, int W, int H, float s, float t) {
    const float x = (s - floorf(s)) * (float)W, y = (t - floorf(t)) * (float)H;
    const float xB = x - 0.5f, yB = y - 0.5f;
    const float fi = floorf(xB), fj = floorf(yB);
    const float alpha = floorf((xB - fi) * 256.0f + 0.5f) * (1.0f / 256.0f);
    const float beta = floorf((yB - fj) * 256.0f + 0.5f) * (1.0f / 256.0f);
    // wrap and clamp as tex2d_wrap_linear (pt_device.h): the same index for every finite coordinate, inside the level for every other
    int i0 = (int)fi, j0 = (int)fj;
    int i1 = i0 + 1, j1 = j0 + 1;
    i0 = i0 < 0 ? i0 + W : i0; i1 = i1 >= W ? i1 - W : i1;
    j0 = j0 < 0 ? j0 + H : j0; j1 = j1 >= H ? j1 - H : j1;
    i0 = (int)min((uint32_t)i0, (uint32_t)(W - 1)); i1 = (int)min((uint32_t)i1, (uint32_t)(W - 1));
    j0 = (int)min((uint32_t)j0, (uint32_t)(H - 1)); j1 = (int)min((uint32_t)j1, (uint32_t)(H - 1));
    const float4 t00 = T[(size_t)j0 * W + i0], t10 = T[(size_t)j0 * W + i1], t01 = T[(size_t)j1 * W + i0], t11 = T[(size_t)j1 * W + i1];
    const float w00 = (1.0f - alpha) * (1.0f - beta), w10 = alpha * (1.0f - beta), w01 = (1.0f - alpha) * beta, w11 = alpha * beta;
    return make_float4(w00 * t00.x + w10 * t10.x + w01 * t01.x + w11 * t11.x, w00 * t00.y + w10 * t10.y + w01 * t01.y + w11 * t11.y,
                       w00 * t00.z + w10 * t10.z + w01 * t01.z + w11 * t11.z, w00 * t00.w + w10 * t10.w + w01 * t01.w + w11 * t11.w);
}
// level k of a texture at (s, t): the tiles for k = 0, the pyramid above
PT_DEV float4 lod_level(const SurfaceLodArgs& a, const DevTex& tx, int tid, uint32_t k, float s, float t, const float* u8lut) {
    if (k == 0u) return tex2d_wrap_linear(tx, s, t, u8lut);
    const float4* T = a.mips + a.level_first[(uint32_t)tid * LOD_MAX_LEVELS + k];
    return lod_tex2d(T, max(1, tx.w >> k), max(1, tx.h >> k), s, t);
}

// The footprint of one textured hit, the header's text from w0 to rx, ry: what k_surface_lod and k_surface_aniso share.  prim is in range
// and tid >= 0 (the caller has tested both).
struct LodFoot {
    float s, t, ds_x, dt_x, ds_y, dt_y, rx, ry;
    bool ok;
    DevTex tx;
};
template <bool VIEWS>
PT_DEV LodFoot lod_footprint(const SurfaceLodArgs& a, const ViewParams& vp, uint32_t xy, int32_t prim, float u, float v, int tid) {
    float c[6]; // uv0.xy, uv1.xy, uv2.xy
    __builtin_memcpy(c, a.prim_uv + 6 * (size_t)prim, 24);
    const float w0 = (1.0f - u) - v;
    const float s = ((w0 * c[0]) + (u * c[2])) + (v * c[4]);
    const float t = ((w0 * c[1]) + (u * c[3])) + (v * c[5]);
    // the pixel's camera: its view's or the frame's.  Looked up here, where the few pixels that need it are
    const PassPixel px = pass_pixel<VIEWS>(vp, xy, a.width, a.height);
    const uint32_t x = px.X - (uint32_t)px.x0, y = px.Y - (uint32_t)px.y0;
    const int wr = px.wr, hr = px.hr;
    v3 eye = a.eye, eU = a.U, eV = a.V, eW = a.W;
    if (VIEWS) {
        const pt_view& vw = vp.views[px.view];
        eye = mk3(vw.eye[0], vw.eye[1], vw.eye[2]);
        eU = mk3(vw.U[0], vw.U[1], vw.U[2]);
        eV = mk3(vw.V[0], vw.V[1], vw.V[2]);
        eW = mk3(vw.W[0], vw.W[1], vw.W[2]);
    }
    const uint32_t i0 = a.idx[3u * (size_t)prim], i1 = a.idx[3u * (size_t)prim + 1], i2 = a.idx[3u * (size_t)prim + 2];
    const float *f0 = a.verts + 3 * (size_t)i0, *f1 = a.verts + 3 * (size_t)i1, *f2 = a.verts + 3 * (size_t)i2;
    const v3 p0 = mk3(f0[0], f0[1], f0[2]), p1 = mk3(f1[0], f1[1], f1[2]), p2 = mk3(f2[0], f2[1], f2[2]);
    const v3 e1 = sub3(p1, p0), e2 = sub3(p2, p0), nrm = cross3(e1, e2);
    const float nn = dot3(nrm, nrm), hgt = dot3(nrm, sub3(p0, eye));
    const float fx = (float)x, fy = (float)y, fw = (float)wr, fh = (float)hr;
    const v3 dc = lod_ray(eU, eV, eW, fx + 0.5f, fy + 0.5f, fw, fh), dx = lod_ray(eU, eV, eW, fx + 1.5f, fy + 0.5f, fw, fh),
             dy = lod_ray(eU, eV, eW, fx + 0.5f, fy + 1.5f, fw, fh);
    const float t_c = hgt / dot3(nrm, dc), t_x = hgt / dot3(nrm, dx), t_y = hgt / dot3(nrm, dy);
    const v3 Pc = add3(scl3(dc, t_c), eye), Px = add3(scl3(dx, t_x), eye), Py = add3(scl3(dy, t_y), eye);
    const bool ok = t_c > 0.0f && t_x > 0.0f && t_y > 0.0f;
    const float c20 = c[2] - c[0], c40 = c[4] - c[0], c31 = c[3] - c[1], c51 = c[5] - c[1];
    const v3 gx = sub3(Px, Pc), gy = sub3(Py, Pc);
    const float dux = dot3(cross3(gx, e2), nrm) / nn, dvx = dot3(cross3(e1, gx), nrm) / nn;
    const float duy = dot3(cross3(gy, e2), nrm) / nn, dvy = dot3(cross3(e1, gy), nrm) / nn;
    const float ds_x = dux * c20 + dvx * c40, dt_x = dux * c31 + dvx * c51;
    const float ds_y = duy * c20 + dvy * c40, dt_y = duy * c31 + dvy * c51;
    const DevTex tx = a.textures[tid];
    const float Wt = (float)tx.w, Ht = (float)tx.h;
    const float rx = (ds_x * Wt) * (ds_x * Wt) + (dt_x * Ht) * (dt_x * Ht);
    const float ry = (ds_y * Wt) * (ds_y * Wt) + (dt_y * Ht) * (dt_y * Ht);
    return LodFoot{s, t, ds_x, dt_x, ds_y, dt_y, rx, ry, ok, tx};
}

template <bool VIEWS, bool TEX>
__global__ void __launch_bounds__(256) k_surface_lod(SurfaceLodArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    __shared__ float s_u8[TEX ? 256 : 1];
    if (TEX) {
        s_u8[threadIdx.x] = (float)threadIdx.x / 255.0f;
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool is_hit = false, is_stale = false, is_tex = false, is_min = false;
    if (i < a.n) {
        const uint32_t xy = a.pixels[i];
        const size_t p = (size_t)pass_y(xy) * (size_t)a.width + pass_x(xy);
        const float4 ha = tp_load4(a.hit + 8 * p); // t, u, v, prim
        const int32_t prim = __float_as_int(ha.w);
        const bool miss = hit_is_miss(ha.w);
        is_hit = !miss && (uint32_t)prim < a.ntri;
        is_stale = !miss && !is_hit;
        float4 alb = make_float4(0.f, 0.f, 0.f, 1.0f), fp = make_float4(0.f, 0.f, 0.f, 0.f);
        float2 tc = make_float2(0.f, 0.f);
        float lod = 0.f;
        if (is_hit) {
            const uint32_t mesh = a.tri_mesh[prim];
            const float* col = a.mats[mesh].color;
            int tid = -1;
            if (TEX) tid = a.mesh_tex[mesh];
            if (TEX && tid >= 0) {
                is_tex = true;
                const LodFoot f = lod_footprint<VIEWS>(a, vp, xy, prim, ha.y, ha.z, tid);
                const float s = f.s, t = f.t, rx = f.rx, ry = f.ry;
                const bool ok = f.ok;
                const DevTex tx = f.tx;
                tc = make_float2(s, t);
                fp = make_float4(f.ds_x, f.dt_x, f.ds_y, f.dt_y);
                const float rho2 = ok ? (rx > ry ? rx : ry) : __uint_as_float(0x7f800000u);
                const float rho = sqrtf(rho2) * a.scale;
                float4 o;
                if (!(rho > 1.0f)) { // level 0; a NaN lands here
                    o = tex2d_wrap_linear(tx, s, t, s_u8);
                } else {
                    is_min = true;
                    const uint32_t Lm = 31u - (uint32_t)__clz(max(tx.w, tx.h)); // levels - 1 = floor(log2(max(w, h))); sizes are >= 1
                    if (!(rho < (float)(1u << Lm))) { // the coarsest level alone (+inf too)
                        o = lod_level(a, tx, tid, Lm, s, t, s_u8);
                        lod = (float)Lm;
                    } else { // 1 < rho < 2^Lm: k in [0, Lm - 1]
                        const uint32_t bits = __float_as_uint(rho);
                        const uint32_t k = min(((bits >> 23) & 0xffu) - 127u, Lm - 1u); // (the range above already bounds it)
                        const float frac = __uint_as_float((bits & 0x007fffffu) | 0x3f800000u) - 1.0f;
                        const float4 ck = lod_level(a, tx, tid, k, s, t, s_u8), cn = lod_level(a, tx, tid, k + 1u, s, t, s_u8);
                        o = make_float4(ck.x + (cn.x - ck.x) * frac, ck.y + (cn.y - ck.y) * frac, ck.z + (cn.z - ck.z) * frac, 1.0f);
                        lod = (float)k + frac;
                    }
                }
                alb = make_float4(o.x, o.y, o.z, 1.0f);
            } else {
                alb = make_float4(col[0], col[1], col[2], 1.0f);
            }
        }
        if (a.albedo) gb_store4(a.albedo + 4 * p, alb);
        if (a.texcoord) gb_store2(a.texcoord + 2 * p, tc);
        if (a.footprint) gb_store4(a.footprint + 4 * p, fp);
        if (a.lod) a.lod[p] = lod;
    }
    pass_tally(pass_slot(a.counts), {is_hit, is_stale, is_tex, is_min}); // is_tex, is_min: never without TEX
#endif
}
// ------------------------------------------------------------------ the anisotropic pass
// pt_surface_aniso_planes: k_surface_lod with N <= max_aniso <= 16 taps along the footprint's major axis, each the level choice of
// rho_maj / N.  Same thread layout, same order of loads, same LDS table; the pyramid, level_first, lod_level and lod_footprint are the
// sibling's.  The tap loop has a runtime trip count and stays a loop (no unroll): three accumulators, no array, no scratch.  A wave is one
// 8 x 8 block of pixels, so its lanes take similar N and their taps overlap in texture space: the reuse is left to L1/L2, as in k_filter
// and k_upsample, with no LDS window (profiles/surface_aniso.md has the measurement).  Every tap address is formed as the sibling forms
// its own: level k <= Lm of the context's texture tid through level_first, texel indices clamped into the level — the tap's texcoord is
// a caller-influenced float and may be anything.
struct SurfaceAnisoArgs {
    SurfaceLodArgs lod; // counts: [0] hits, [1] stale, [2] textured, [3] minified, [4] anisotropic, [5] the sum of N - 1 of a slot
    float* taps;        // null = not asked for
    uint32_t max_aniso; // 1..16
};

template <bool VIEWS, bool TEX>
__global__ void __launch_bounds__(256) k_surface_aniso(SurfaceAnisoArgs aa, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const SurfaceLodArgs& a = aa.lod;
    __shared__ float s_u8[TEX ? 256 : 1];
    if (TEX) {
        s_u8[threadIdx.x] = (float)threadIdx.x / 255.0f;
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool is_hit = false, is_stale = false, is_tex = false, is_min = false;
    uint32_t N = 0; // the taps of a textured pixel; 0 where no texture is read
    if (i < a.n) {
        const uint32_t xy = a.pixels[i];
        const size_t p = (size_t)pass_y(xy) * (size_t)a.width + pass_x(xy);
        const float4 ha = tp_load4(a.hit + 8 * p); // t, u, v, prim
        const int32_t prim = __float_as_int(ha.w);
        const bool miss = hit_is_miss(ha.w);
        is_hit = !miss && (uint32_t)prim < a.ntri;
        is_stale = !miss && !is_hit;
        float4 alb = make_float4(0.f, 0.f, 0.f, 1.0f), fp = make_float4(0.f, 0.f, 0.f, 0.f);
        float2 tc = make_float2(0.f, 0.f);
        float lod = 0.f;
        if (is_hit) {
            const uint32_t mesh = a.tri_mesh[prim];
            const float* col = a.mats[mesh].color;
            int tid = -1;
            if (TEX) tid = a.mesh_tex[mesh];
            if (TEX && tid >= 0) {
                is_tex = true;
                const LodFoot f = lod_footprint<VIEWS>(a, vp, xy, prim, ha.y, ha.z, tid);
                const float s = f.s, t = f.t;
                const DevTex tx = f.tx;
                tc = make_float2(s, t);
                fp = make_float4(f.ds_x, f.dt_x, f.ds_y, f.dt_y);
                const bool xm = f.rx > f.ry; // the sibling's own comparison: a tie takes y
                const float r_maj2 = xm ? f.rx : f.ry, r_min2 = xm ? f.ry : f.rx;
                const float a_s = xm ? f.ds_x : f.ds_y, a_t = xm ? f.dt_x : f.dt_y;
                const float rho_maj = (f.ok ? sqrtf(r_maj2) : __uint_as_float(0x7f800000u)) * a.scale;
                is_min = rho_maj > 1.0f;
                N = 1u;
                if (is_min && f.ok) {
                    const float rho_min = sqrtf(r_min2) * a.scale;
                    const float q = rho_maj / rho_min; // >= 1, +inf on a degenerate minor axis, NaN on a NaN one
                    N = (q <= (float)aa.max_aniso) ? (uint32_t)ceilf(q) : aa.max_aniso;
                }
                const float rho = N > 1u ? rho_maj / (float)N : rho_maj;
                // the level choice of rho, the sibling's three cases: level k alone, or k and k + 1 blended by frac
                uint32_t k = 0u;
                bool tri = false;
                float frac = 0.f;
                if (rho > 1.0f) { // (a NaN stays at level 0)
                    const uint32_t Lm = 31u - (uint32_t)__clz(max(tx.w, tx.h));
                    if (!(rho < (float)(1u << Lm))) { // the coarsest level alone (+inf too)
                        k = Lm;
                        lod = (float)Lm;
                    } else {
                        const uint32_t bits = __float_as_uint(rho);
                        k = min(((bits >> 23) & 0xffu) - 127u, Lm - 1u);
                        frac = __uint_as_float((bits & 0x007fffffu) | 0x3f800000u) - 1.0f;
                        tri = true;
                        lod = (float)k + frac;
                    }
                }
                const float two_n = (float)(2u * N);
                float ax = 0.f, ay = 0.f, az = 0.f;
#pragma nounroll
                for (uint32_t j = 0; j < N; ++j) {
                    float sj = s, tj = t; // N = 1: the tap is (s, t) itself, no arithmetic on the axis
                    if (N > 1u) {
                        const float o = (float)((int)(2u * j + 1u) - (int)N) / two_n;
                        const float os = o * a.scale;
                        sj = s + os * a_s;
                        tj = t + os * a_t;
                    }
                    float4 c = lod_level(a, tx, tid, k, sj, tj, s_u8);
                    if (tri) {
                        const float4 cn = lod_level(a, tx, tid, k + 1u, sj, tj, s_u8);
                        c = make_float4(c.x + (cn.x - c.x) * frac, c.y + (cn.y - c.y) * frac, c.z + (cn.z - c.z) * frac, 1.0f);
                    }
                    ax = j ? ax + c.x : c.x;
                    ay = j ? ay + c.y : c.y;
                    az = j ? az + c.z : c.z;
                }
                if (N > 1u) {
                    const float fn = (float)N;
                    ax = ax / fn, ay = ay / fn, az = az / fn;
                }
                alb = make_float4(ax, ay, az, 1.0f);
            } else {
                alb = make_float4(col[0], col[1], col[2], 1.0f);
            }
        }
        if (a.albedo) gb_store4(a.albedo + 4 * p, alb);
        if (a.texcoord) gb_store2(a.texcoord + 2 * p, tc);
        if (a.footprint) gb_store4(a.footprint + 4 * p, fp);
        if (a.lod) a.lod[p] = lod;
        if (aa.taps) aa.taps[p] = (float)N;
    }
    unsigned long long* slot = pass_slot(a.counts);
    pass_tally(slot, {is_hit, is_stale, is_tex, is_min, N > 1u}); // the last three: never without TEX
    if (TEX) { // the wave's taps beyond the first, the sum of N - 1 (<= 15: four bits), one ballot per bit; every lane arrives here.  The
               // host adds the textured pixels: a wave without an anisotropic pixel issues the sibling's atomics and no more
        const uint32_t extra = N > 1u ? N - 1u : 0u;
        unsigned long long sum = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) sum += (unsigned long long)__popcll(__ballot((extra >> b) & 1u)) << b;
        if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(slot + 5, sum);
    }
#endif
}
#endif // __HIPCC__
