// pt_pass_dev.h — what the image-space passes share on the device (pt_pass.h is the host's side): the 16-byte loads and stores, the decode of a
// pixel-list entry and its view, the surface key with the chain's two "same surface" predicates, the reprojection gather, the per-wave
// tally, and the scaffold of the tiled passes (motion blur, depth of field).  Every pass header includes this file and no other pass's
// kernel; nothing the frame path is compiled from includes it.
//
// Everything here is PT_DEV (forced inline) and written in the order the public header gives, one float32 rounding per operation
// (-ffp-contract=off is part of the library's flags), so a kernel built on these pieces keeps the bits its tests/*_ref.py reference pins.
#pragma once
#include <cstdint>

// The view table of a tiled pass, one entry per rectangle: the one structure here that the host fills (pass_tile_table, pt_pass.h) and the
// device reads, so it stands in front of the HIP headers, where a host compiler alone can see it.  T and N are planes of one texel per
// tile, PASS_TILE x PASS_TILE pixels, in the caller's scratch.
#define PASS_TILE 16u
struct TileView {
    uint32_t w, h, org;  // the rectangle; org = x0 | y0 << 16 in the frame
    uint32_t tw, th;     // its tile grid
    uint32_t offT, offN; // the first texel of T and of N in the scratch
    float aux;           // the pass's own word per view: depth of field's focus distance, 0 for motion blur
};

#ifdef __HIPCC__
#include <cfloat>

#include "pt_kernels.h"

// ------------------------------------------------------------------ loads and stores
// Four (two) words to or from a plane that is only known to be 4-byte aligned, as ONE access: a copy of known size with alignment 4 compiles
// to global_store_dwordx4 / global_load_dwordx4 (x2), which the hardware takes at any 4-byte address — a plane at a 16-byte address gets
// 16-byte-aligned accesses from the same instruction, so there is no second code path.  (Two paths chosen by a flag were tried first: the
// compiler merged them into dword stores, 23 per pixel for the G-buffer's five planes.)
PT_DEV void gb_store4(float* p, float4 v) { __builtin_memcpy(p, &v, 16); }
PT_DEV void gb_store2(float* p, float2 v) { __builtin_memcpy(p, &v, 8); }
PT_DEV float4 tp_load4(const float* p) {
    float4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
PT_DEV float2 tp_load2(const float* p) {
    float2 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
PT_DEV bool tp_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; } // exponent bits: no compiler mode can fold it away
PT_DEV float fl_lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }
PT_DEV float fl_max0(float v) { return v > 0.0f ? v : 0.0f; }

// ------------------------------------------------------------------ a pixel-list entry, its view and its rectangle
// An entry is x | y << 16 in frame coordinates.  The view of a pixel is found by its 8x8 block; the lists hold view pixels only, so the
// table's 0xffff never comes back.  Without views the rectangle is the frame and the index is 0 (the one previous camera).
PT_DEV uint32_t pass_x(uint32_t xy) { return xy & 0xffffu; }
PT_DEV uint32_t pass_y(uint32_t xy) { return xy >> 16; }
struct PassPixel {
    uint32_t X, Y, view;  // frame coordinates; the index of the view (and of its camera)
    int x0, y0, wr, hr;   // the rectangle [x0, x0 + wr) x [y0, y0 + hr) the pixel's neighbours may come from
};
template <bool VIEWS>
PT_DEV PassPixel pass_pixel_at(const ViewParams& vp, uint32_t X, uint32_t Y, int width, int height) {
    PassPixel p{X, Y, 0u, 0, 0, width, height};
    if (VIEWS) {
        p.view = vp.vblock[(Y >> 3) * vp.nbx + (X >> 3)];
        p.x0 = vp.views[p.view].x;
        p.y0 = vp.views[p.view].y;
        p.wr = vp.views[p.view].width;
        p.hr = vp.views[p.view].height;
    }
    return p;
}
template <bool VIEWS>
PT_DEV PassPixel pass_pixel(const ViewParams& vp, uint32_t xy, int width, int height) {
    return pass_pixel_at<VIEWS>(vp, pass_x(xy), pass_y(xy), width, height);
}
// rect and block: is (qx, qy) a pixel whose planes may be looked at — inside p's rectangle and in a block of the call's set (inset: one byte
// per block, nbx blocks a row)
PT_DEV bool pass_reachable(const PassPixel& p, const uint8_t* inset, uint32_t nbx, int qx, int qy) {
    if (qx < p.x0 || qx >= p.x0 + p.wr || qy < p.y0 || qy >= p.y0 + p.hr) return false;
    return inset[(uint32_t)(qy >> 3) * nbx + (uint32_t)(qx >> 3)] != 0;
}

// The header's d(a, b): the camera ray through the point (a, b), in pixels, of a rectangle wr x hr (k_surface_lod, k_surface_aniso, k_edge_aa)
PT_DEV v3 lod_ray(v3 U, v3 V, v3 W, float a, float b, float wr, float hr) {
    const float dx = 2.0f * (a / wr) - 1.0f, dy = 2.0f * (b / hr) - 1.0f;
    return add3(add3(scl3(U, dx), scl3(V, dy)), W);
}

// ------------------------------------------------------------------ the surface key and the chain's "same surface"
// A pt_hit is t, u, v, prim | mesh, ng.xyz: a negative primitive word is a miss.  The key is the pixel's side of the tests; a tap q of a
// hit is the same surface when same_facet and same_plane hold.  They are two functions so that a kernel orders its loads itself, cheapest
// word first; each makes one 16-byte load.  Both comparisons are written so that a NaN fails.  The plane test is a dot with a DIFFERENCE
// of positions: dot3(ng, Q - P) is not dot3(ng, Q) - dot3(ng, P) in float32, so the planes are read as they are.
PT_DEV bool hit_is_miss(float prim_word) { return __float_as_int(prim_word) < 0; }
struct SurfaceKey {
    bool miss;
    int mesh;
    v3 ng, P;
    float plane_max; // plane_eps * t
};
// hb: the record's second half; P: the pixel's position (anything under a miss: no test reads it)
PT_DEV SurfaceKey surface_key(bool miss, float t, float4 hb, float4 P, float plane_eps) {
    return SurfaceKey{miss, __float_as_int(hb.x), mk3(hb.y, hb.z, hb.w), mk3(P.x, P.y, P.z), plane_eps * t};
}
PT_DEV bool same_facet(const SurfaceKey& k, const float* hit, size_t q, float normal_cos) { // mesh, normal
    const float4 qb = tp_load4(hit + 8 * q + 4);
    return __float_as_int(qb.x) == k.mesh && dot3(k.ng, mk3(qb.y, qb.z, qb.w)) >= normal_cos;
}
PT_DEV bool same_plane(const SurfaceKey& k, const float* position, size_t q) {
    const float4 Q = tp_load4(position + 4 * q);
    return fabsf(dot3(k.ng, mk3(Q.x - k.P.x, Q.y - k.P.y, Q.z - k.P.z))) <= k.plane_max;
}

// ------------------------------------------------------------------ the reprojection gather
// The eight read-only planes of the gather (moments_in: MOMENTS only) and its three parameters.
struct GatherPlanes {
    const float *motion, *hit, *position, *prev_hit, *prev_position, *history_in, *moments_in, *length_in;
    int width, height; // the frame: the planes are indexed Y * width + X
    float normal_cos, plane_eps, min_weight;
};
// What the gather leaves for a pixel: the sums in tap order, the minimum history length of the counting taps, and valid.
struct Gather {
    float wsum, nprev, msx, msy;
    v3 hsum;
    bool valid;
};
// Steps 2, 3 and 4 of pt_temporal_accumulate (MOMENTS false) and of pt_temporal_moments (true): the previous position from the motion plane,
// the four bilinear taps, the sums.  A tap is read cheapest word first: the history length (4 bytes), the previous hit record's mesh and
// normal (16 bytes; the primitive word alone under a miss), prev_position (16 bytes), and only a tap that survived the geometry tests loads
// its moments (8 bytes, MOMENTS) and its history (16 bytes).  A caller that never uses hsum (k_plan) loses its products and sums as dead
// code; the history's loads stay, for the finite test.
template <bool MOMENTS>
PT_DEV Gather rp_gather(const GatherPlanes& a, const PassPixel& px) {
    const int x = (int)px.X - px.x0, y = (int)px.Y - px.y0;
    const size_t p = (size_t)px.Y * (size_t)a.width + px.X;
    // ---------------- 2. previous position
    const float2 mv = tp_load2(a.motion + 2 * p);
    const float fpx = (float)x + mv.x, fpy = (float)y + mv.y;
    Gather g;
    g.wsum = 0.0f;
    g.nprev = 0.0f;
    g.msx = 0.0f;
    g.msy = 0.0f;
    g.hsum = mk3(0.0f);
    bool any = false;
    if (fpx >= -1.0f && fpx <= (float)px.wr && fpy >= -1.0f && fpy <= (float)px.hr) { // a NaN fails
        const float flx = floorf(fpx), fly = floorf(fpy);
        const int ix = (int)flx, iy = (int)fly;
        const float fx = fpx - flx, fy = fpy - fly;
        const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
        const float4 ha = tp_load4(a.hit + 8 * p), hb = tp_load4(a.hit + 8 * p + 4);
        const SurfaceKey key = surface_key(hit_is_miss(ha.w), ha.x, hb, tp_load4(a.position + 4 * p), a.plane_eps);
        float wt[4], mx[4], my[4];
        v3 ht[4];
        // ---------------- 3. which taps count; order (0,0), (1,0), (0,1), (1,1)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ti = k & 1, tj = k >> 1;
            const int tx = ix + ti, ty = iy + tj;
            const float w = wx[ti] * wy[tj];
            wt[k] = 0.0f;
            mx[k] = 0.0f;
            my[k] = 0.0f;
            ht[k] = mk3(0.0f);
            if (tx >= 0 && tx < px.wr && ty >= 0 && ty < px.hr && w > 0.0f) {
                const size_t q = (size_t)(px.y0 + ty) * (size_t)a.width + (size_t)(px.x0 + tx);
                const float len = a.length_in[q];
                if (len >= 1.0f) {
                    bool alive;
                    if (key.miss) alive = hit_is_miss(a.prev_hit[8 * q + 3]);
                    else alive = same_facet(key, a.prev_hit, q, a.normal_cos) && same_plane(key, a.prev_position, q);
                    if (alive) {
                        float2 mq = make_float2(0.0f, 0.0f);
                        if (MOMENTS) mq = tp_load2(a.moments_in + 2 * q);
                        const float4 hq = tp_load4(a.history_in + 4 * q);
                        if (tp_finite(hq.x) && tp_finite(hq.y) && tp_finite(hq.z) && tp_finite(mq.x) && tp_finite(mq.y)) {
                            wt[k] = w;
                            ht[k] = mk3(w * hq.x, w * hq.y, w * hq.z);
                            mx[k] = w * mq.x;
                            my[k] = w * mq.y;
                            g.nprev = any ? fminf(g.nprev, len) : len;
                            any = true;
                        }
                    }
                }
            }
        }
        // ---------------- 4. sums, in tap order
        g.wsum = ((wt[0] + wt[1]) + wt[2]) + wt[3];
        g.hsum = mk3(((ht[0].x + ht[1].x) + ht[2].x) + ht[3].x, ((ht[0].y + ht[1].y) + ht[2].y) + ht[3].y, ((ht[0].z + ht[1].z) + ht[2].z) + ht[3].z);
        g.msx = ((mx[0] + mx[1]) + mx[2]) + mx[3];
        g.msy = ((my[0] + my[1]) + my[2]) + my[3];
    }
    g.valid = any && g.wsum >= a.min_weight;
    return g;
}

// ------------------------------------------------------------------ the per-wave tally
// Counts of the lanes for which flag[j] holds, added to words[j] by one 64-bit atomic per wave and non-zero count.  EVERY lane of the wave
// must reach the call (the ballots), so it stands outside a kernel's `i < n` branch.  Into ONE word the 32 400 waves of a 1080p frame
// serialise at about 10 ns an atomic: 0.32 ms per counter whatever the kernel reads, measured (profiles/surface.md).  A short kernel
// therefore tallies into pass_slot(counts), the wave's slot of PASS_SLOTS, 64 bytes apart (QuerySlot's layout, pt_kernels.h), and the host
// adds the slots up (PassRun::close_slots, pt_pass.h).
#define PASS_SLOTS 64u
template <int N>
PT_DEV void pass_tally(unsigned long long* words, const bool (&flag)[N]) {
    unsigned long long m[N];
#pragma unroll
    for (int j = 0; j < N; ++j) m[j] = __ballot(flag[j]);
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (m[j]) atomicAdd(words + j, (unsigned long long)__popcll(m[j]));
    }
}
// counts: [PASS_SLOTS][8], zero at launch; 256-thread blocks
PT_DEV unsigned long long* pass_slot(unsigned long long* counts) { return counts + 8u * ((blockIdx.x * 4u + (threadIdx.x >> 6)) & (PASS_SLOTS - 1u)); }

// ------------------------------------------------------------------ tiled passes
// What k_mblur_* and k_dof_* share: a pass reduces every PASS_TILE x PASS_TILE tile of every rectangle to one texel (T), takes the greatest T
// of the 3 x 3 tiles around each tile (N), and gathers along or around N over the call's pixel list.  One launch covers all views:
// blockIdx.y is the view, and a block past the end of its view's grid leaves at once.  Everything works in a rectangle's own coordinates,
// which is what keeps a tap and a tile neighbour from leaving it.  What differs stays in the pass's header: what a tile is reduced to and
// how (k_mblur_tile's 64-bit key, k_dof_tile's plain maximum), the tap rule, the weights.
PT_DEV float pass_depth(float d) { return (d > 1e-6f && d <= FLT_MAX) ? d : FLT_MAX; } // Z(depth) of the header
PT_DEV float pass_clamp01(float x) {
    x = x > 0.0f ? x : 0.0f;
    return x < 1.0f ? x : 1.0f;
}
PT_DEV uint32_t pass_hash(uint32_t x, uint32_t y, uint32_t seed) {
    uint32_t h = (x * 0x9E3779B1u) ^ (y * 0x85EBCA77u) ^ (seed * 0xC2B2AE3Du);
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}
PT_DEV uint32_t pass_wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// A tile kernel is one WAVE per tile: lane l takes the four pixels (l & 3) * 4 + k, k = 0 .. 3, of the tile's row l >> 2, so lane * 4 + k is
// the pixel's row-order index in the tile.  in: the pixel lies in the rectangle (a partial tile); p: its index in a plane of the frame
// (Y * width + X).  A pixel outside has the p of the rectangle's pixel (0, 0), to be loaded and dropped.  Pixel 0 of a tile is always inside.
struct TilePixel {
    bool in;
    size_t p;
};
PT_DEV TilePixel tile_pixel(const TileView& L, int width, uint32_t tile, uint32_t lane, uint32_t k) {
    const uint32_t x = (tile % L.tw) * PASS_TILE + (lane & 3u) * 4u + k, y = (tile / L.tw) * PASS_TILE + (lane >> 2);
    const bool in = x < L.w && y < L.h;
    const uint32_t sx = in ? x : 0u, sy = in ? y : 0u;
    return TilePixel{in, (size_t)((L.org >> 16) + sy) * (size_t)width + (size_t)((L.org & 0xffffu) + sx)};
}

// k_tile_neighbour<Texel>: N, the T of greatest key of the 3 x 3 tiles around a tile that exist.  One thread per tile, up to nine loads,
// row order, the first existing tile taken, then strict >: among equal keys the first in row order wins, which is what decides motion blur's
// N (float2, key l2).  Depth of field's (float, key the value itself) does not depend on it: every T is a radius K * |..| clamped to R with
// K = aperture + 0.0f, so it is >= +0, never NaN and never -0, and the first of several equal floats has the bits of all of them — the
// same bits as a maximum that starts from 0.  The launch is tiny and launch-bound; it is a kernel of its own because folded into the gather
// every wave would redo the nine loads for a value that 256 pixels share, and N has to reach the scratch either way.
PT_DEV float tile_key(float t) { return t; }
PT_DEV float tile_key(float2 t) { return t.x * t.x + t.y * t.y; }
template <typename Texel>
struct TileNeighbourArgs {
    const TileView* tab;
    Texel* scratch;
};
template <typename Texel>
__global__ void __launch_bounds__(256) k_tile_neighbour(TileNeighbourArgs<Texel> a) {
#if __HIP_DEVICE_COMPILE__
    const TileView L = a.tab[blockIdx.y];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= L.tw * L.th) return;
    const int ti = (int)(i % L.tw), tj = (int)(i / L.tw);
    Texel best{};
    float bestk = 0.0f;
    bool any = false;
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
        for (int di = -1; di <= 1; ++di) {
            const int u = ti + di, v = tj + dj;
            if (u < 0 || u >= (int)L.tw || v < 0 || v >= (int)L.th) continue;
            const Texel t = a.scratch[(size_t)L.offT + (size_t)v * L.tw + (size_t)u];
            const float key = tile_key(t);
            if (!any || key > bestk) {
                best = t;
                bestk = key;
                any = true;
            }
        }
    a.scratch[(size_t)L.offN + i] = best;
#endif
}

// A gather's tap: the position (fx, fy) in the rectangle's coordinates, as the pass's rule computed it, rounded to the nearest pixel,
// clamped to the rectangle; returns that pixel's index in a plane of the frame.
PT_DEV size_t pass_tap(const PassPixel& px, int width, float fx, float fy) {
    int qx = (int)floorf(fx + 0.5f), qy = (int)floorf(fy + 0.5f);
    qx = qx < 0 ? 0 : qx > px.wr - 1 ? px.wr - 1 : qx;
    qy = qy < 0 ? 0 : qy > px.hr - 1 ? px.hr - 1 : qy;
    return (size_t)(px.y0 + qy) * (size_t)width + (size_t)(px.x0 + qx);
}

// A gather's epilogue: per-lane counts (sums, not flags: pass_tally is for those), added up across the wave by shuffles and added to words
// first .. first + N - 1 of the wave's slot by one atomic per non-zero sum.  EVERY lane of the wave must reach the call.
template <int N>
PT_DEV void pass_tally_sums(unsigned long long* counts, uint32_t first, const uint32_t (&n)[N]) {
    uint32_t s[N];
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = pass_wave_sum(n[j]);
    if ((threadIdx.x & 63u) == 0u) {
        unsigned long long* slot = pass_slot(counts) + first;
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (s[j]) atomicAdd(slot + j, (unsigned long long)s[j]);
    }
}
#endif // __HIPCC__
