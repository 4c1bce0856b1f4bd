// pt_motion_blur_layout and pt_motion_blur_planes (include/pt_amd.h): motion blur after McGuire et al. 2012 over the chain's motion plane.
// Three kernels: k_mblur_tile reduces every 16 x 16 tile of every rectangle to its fastest velocity (T), k_tile_neighbour<float2> takes the
// fastest T of the 3 x 3 tiles around each tile (N), k_mblur_gather<VIEWS> runs over the call's pixel list and gathers `taps` pixels along
// N.  T and N are planes of 8-byte texels (V.x, V.y) in the caller's scratch; the view table (TileView, one per rectangle, aux unused) is a
// temporary of the call in device memory.
//
// The view table, a tile kernel's pixels, the neighbour kernel, the tap's address, the counters' way out, Z(depth), the hash and the
// clamp are the tiled passes' scaffold in pt_pass_dev.h, shared with depth of field.  What stands here is motion blur's own: the velocity
// rule, the tile's reduction, the line's taps and their weights.
#pragma once
#include "pt_pass_dev.h"

struct MblurParams {
    float hs, R, R2; // 0.5f * shutter, max_blur, max_blur * max_blur (the host's roundings)
};

// Step 1 of the header: V and l2 of a pixel from its motion words
struct MblurVel {
    float x, y, l2;
    bool unknown;
};
PT_DEV MblurVel mblur_velocity(float2 m, const MblurParams& k) {
    MblurVel v{0.0f, 0.0f, 0.0f, !(tp_finite(m.x) && tp_finite(m.y))};
    if (!v.unknown) {
        float x = m.x * k.hs, y = m.y * k.hs;
        x = x < -4096.0f ? -4096.0f : x;
        x = x > 4096.0f ? 4096.0f : x;
        y = y < -4096.0f ? -4096.0f : y;
        y = y > 4096.0f ? 4096.0f : y;
        float l2 = x * x + y * y;
        if (l2 > k.R2) {
            const float s = k.R / sqrtf(l2);
            x = x * s;
            y = y * s;
            l2 = x * x + y * y;
        }
        v.x = x;
        v.y = y;
        v.l2 = l2;
    }
    return v;
}
PT_DEV float mblur_len(float l2) {
    const float l = sqrtf(l2);
    return l > 0.5f ? l : 0.5f;
}
PT_DEV float mblur_cone(float d, float l) { return pass_clamp01(1.0f - d / l); }
PT_DEV float mblur_cyl(float d, float l) {
    const float u = pass_clamp01((d - 0.95f * l) / (1.05f * l - 0.95f * l));
    return 1.0f - (u * u) * (3.0f - 2.0f * u);
}

// ------------------------------------------------------------------ k_mblur_tile: T, the fastest velocity of each tile
// One WAVE per tile, four tiles to a workgroup of 256 threads: a lane's four pixels (tile_pixel, pt_pass_dev.h) are four 8-byte loads that
// are all in flight before the first is used.  (The first version was one workgroup per tile and one pixel per
// thread, with the four waves' maxima going through LDS and a barrier: correct, and 14.8 us for a 1080p frame whatever it read — 32 640
// waves of a few instructions each are bound by the rate at which waves are launched, as k_modulate's are.  A quarter of the waves, no LDS
// and no barrier: profiles/motion_blur.md has both.)  The winner must not depend on the order of the reduction, so what is reduced is the
// 64-bit key (bits of l2) << 32 | ~(row-order index in the tile): l2 >= 0 is never NaN, so its bits order as integers, and among equal l2
// the smallest index has the greatest key.  A pixel outside the rectangle (a partial tile) has key 0, below every real pixel's (pixel 0
// of a tile is always inside).  A lane keeps the greatest of its four keys with that pixel's V, six shuffle steps take the maximum across
// the wave, and the one lane whose own key is that maximum writes its V.  sources and unknown are added up in scalar registers from
// ballots, one per pixel slot, and leave through pass_slot with one atomic per wave and non-zero counter.
struct MblurTileArgs {
    const TileView* tab;
    int width; // of the frame: the planes are indexed Y * width + X
    const float* motion;
    float2* scratch;
    MblurParams k;
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] sources, [1] unknown ([2] moving, [3] taps, [4] nonfinite: k_mblur_gather)
};
#define MBLUR_TILES_PER_BLOCK 4u

__global__ void __launch_bounds__(256) k_mblur_tile(MblurTileArgs a) {
#if __HIP_DEVICE_COMPILE__
    const TileView L = a.tab[blockIdx.y];
    const uint32_t tile = blockIdx.x * MBLUR_TILES_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= L.tw * L.th) return; // the whole wave; the kernel has no barrier
    float2 m[4];
    bool in[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const TilePixel t = tile_pixel(L, a.width, tile, lane, k);
        in[k] = t.in;
        m[k] = tp_load2(a.motion + 2 * t.p);
    }
    unsigned long long own = 0ull;
    float2 mine = make_float2(0.0f, 0.0f);
    uint32_t nin = 0u, nunk = 0u; // wave-uniform
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const MblurVel v = mblur_velocity(m[k], a.k);
        const uint32_t idx = lane * 4u + k; // row order in the tile (tile_pixel)
        const unsigned long long key = in[k] ? ((unsigned long long)__float_as_uint(v.l2) << 32) | (unsigned long long)(~idx) : 0ull;
        if (key > own) {
            own = key;
            mine = make_float2(v.x, v.y);
        }
        nin += (uint32_t)__popcll(__ballot(in[k]));
        nunk += (uint32_t)__popcll(__ballot(in[k] && v.unknown));
    }
    unsigned long long best = own;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if (lane == 0u) {
        unsigned long long* slot = pass_slot(a.counts);
        if (nin) atomicAdd(slot + 0, (unsigned long long)nin);
        if (nunk) atomicAdd(slot + 1, (unsigned long long)nunk);
    }
    if (own == best && own != 0ull) a.scratch[(size_t)L.offT + tile] = mine;
#endif
}

// (N, the fastest T of the 3 x 3 tiles around a tile: k_tile_neighbour<float2>, pt_pass_dev.h)

// ------------------------------------------------------------------ k_mblur_gather: step 4, over the call's pixel list
// k_bloom_composite's shape: one thread per entry of the pixel list.  vN is uniform over a tile, so where the list hands a wave one 8 x 8
// block the early exit, the tap count and (without jitter) t are the same in every lane.  A tap costs 28 bytes — colour 16, motion 8,
// depth 4 — and its three loads are issued together, in front of the first use; the taps of neighbouring lanes land on neighbouring
// pixels, so reuse is left to the caches.  The three counters (taps and nonfinite are sums of per-lane counts, not ballots) leave through
// pass_tally_sums; every lane reaches it.
struct MblurGatherArgs {
    const uint32_t* pixels;
    uint32_t n;
    int width, height;
    const float *color, *motion, *depth;
    float* out;
    const TileView* tab;
    const float2* scratch;
    MblurParams k;
    float depth_soft;
    uint32_t taps, seed, jitter;
    unsigned long long* counts;
};

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_mblur_gather(MblurGatherArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t nmoving = 0u, ntaps = 0u, nnonfinite = 0u;
    if (i < a.n) {
        const PassPixel px = pass_pixel<VIEWS>(vp, a.pixels[i], a.width, a.height);
        const size_t p = (size_t)px.Y * (size_t)a.width + px.X;
        const int x = (int)px.X - px.x0, y = (int)px.Y - px.y0;
        const TileView L = a.tab[px.view];
        const float4 c = tp_load4(a.color + 4 * p);
        const float2 vN = a.scratch[(size_t)L.offN + (size_t)(y >> 4) * L.tw + (size_t)(x >> 4)];
        const float n2 = vN.x * vN.x + vN.y * vN.y;
        v3 o = mk3(c.x, c.y, c.z);
        if (n2 > 0.25f && tp_finite(c.x) && tp_finite(c.y) && tp_finite(c.z)) {
            nmoving = 1u;
            const float lN = sqrtf(n2);
            const float lp = mblur_len(mblur_velocity(tp_load2(a.motion + 2 * p), a.k).l2);
            const float wp = 1.0f / lp;
            const float zp = pass_depth(a.depth[p]);
            const float j = a.jitter ? (float)(pass_hash((uint32_t)x, (uint32_t)y, a.seed) >> 8) * 5.9604644775390625e-8f - 0.5f : 0.0f;
            const float ftaps = (float)a.taps;
            v3 sum = mk3(0.0f);
            float Wt = 0.0f;
            for (uint32_t k = 0; k < a.taps; ++k) {
                const float av = ((float)k + 0.5f) + j;
                const float t = (2.0f * av) / ftaps - 1.0f;
                const size_t q = pass_tap(px, a.width, (float)x + vN.x * t, (float)y + vN.y * t);
                const float4 cq = tp_load4(a.color + 4 * q); // the tap's three loads, in front of the first use
                const float2 mq = tp_load2(a.motion + 2 * q);
                const float dq = a.depth[q];
                if (!(tp_finite(cq.x) && tp_finite(cq.y) && tp_finite(cq.z))) {
                    ++nnonfinite;
                    continue;
                }
                const float d = fabsf(t) * lN;
                const float lq = mblur_len(mblur_velocity(mq, a.k).l2);
                const float zq = pass_depth(dq);
                const float e = a.depth_soft * (zp < zq ? zp : zq);
                const float fg = pass_clamp01(1.0f - (zq - zp) / e), bg = pass_clamp01(1.0f - (zp - zq) / e);
                const float w = (fg * mblur_cone(d, lq) + bg * mblur_cone(d, lp)) + (mblur_cyl(d, lq) * mblur_cyl(d, lp)) * 2.0f;
                sum = mk3(sum.x + cq.x * w, sum.y + cq.y * w, sum.z + cq.z * w);
                Wt = Wt + w;
                if (w > 0.0f) ++ntaps;
            }
            if (!(Wt == 0.0f)) {
                const float den = wp + Wt;
                o = mk3((c.x * wp + sum.x) / den, (c.y * wp + sum.y) / den, (c.z * wp + sum.z) / den);
            }
        }
        gb_store4(a.out + 4 * p, make_float4(o.x, o.y, o.z, 1.0f));
    }
    const uint32_t counted[3] = {nmoving, ntaps, nnonfinite};
    pass_tally_sums(a.counts, 2u, counted); // words 2 .. 4
#endif
}
