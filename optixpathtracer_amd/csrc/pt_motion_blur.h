// pt_motion_blur_layout and pt_motion_blur_planes (include/pt_amd.h): motion blur after McGuire et al. 2012 over the chain's motion plane.
// Three kernels: k_mblur_tile reduces every 16 x 16 tile of every rectangle to its fastest velocity (T), k_mblur_neighbour takes the
// fastest T of the 3 x 3 tiles around each tile (N), k_mblur_gather<VIEWS> runs over the call's pixel list and gathers `taps` pixels along
// N.  T and N are planes of 8-byte texels (V.x, V.y) in the caller's scratch; the view table (MblurView, one per rectangle) is a temporary
// of the call in device memory.  One launch covers all views: blockIdx.y is the view, and a block past the end of its view's grid leaves
// at once.  Everything works in a rectangle's own coordinates, which is what keeps a tap and a tile neighbour from leaving it.
#pragma once
#include <cfloat>

#include "pt_pass_dev.h"

struct MblurView {
    uint32_t w, h, org; // the rectangle; org = x0 | y0 << 16 in the frame
    uint32_t tw, th;    // its tile grid
    uint32_t offT, offN; // the first 8-byte texel of T and of N in the scratch
    uint32_t pad_;
};

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
PT_DEV float mblur_clamp01(float x) {
    x = x > 0.0f ? x : 0.0f;
    return x < 1.0f ? x : 1.0f;
}
PT_DEV float mblur_depth(float d) { return (d > 1e-6f && d <= FLT_MAX) ? d : FLT_MAX; }
PT_DEV float mblur_len(float l2) {
    const float l = sqrtf(l2);
    return l > 0.5f ? l : 0.5f;
}
PT_DEV float mblur_cone(float d, float l) { return mblur_clamp01(1.0f - d / l); }
PT_DEV float mblur_cyl(float d, float l) {
    const float u = mblur_clamp01((d - 0.95f * l) / (1.05f * l - 0.95f * l));
    return 1.0f - (u * u) * (3.0f - 2.0f * u);
}
PT_DEV uint32_t mblur_hash(uint32_t x, uint32_t y, uint32_t seed) {
    uint32_t h = (x * 0x9E3779B1u) ^ (y * 0x85EBCA77u) ^ (seed * 0xC2B2AE3Du);
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}

// ------------------------------------------------------------------ k_mblur_tile: T, the fastest velocity of each tile
// One WAVE per tile, four tiles to a workgroup of 256 threads: lane l takes the four pixels (l & 3) * 4 .. + 3 of the tile's row l >> 2,
// four 8-byte loads that are all in flight before the first is used.  (The first version was one workgroup per tile and one pixel per
// thread, with the four waves' maxima going through LDS and a barrier: correct, and 14.8 us for a 1080p frame whatever it read — 32 640
// waves of a few instructions each are bound by the rate at which waves are launched, as k_modulate's are.  A quarter of the waves, no LDS
// and no barrier: profiles/motion_blur.md has both.)  The winner must not depend on the order of the reduction, so what is reduced is the
// 64-bit key (bits of l2) << 32 | ~(row-order index in the tile): l2 >= 0 is never NaN, so its bits order as integers, and among equal l2
// the smallest index has the greatest key.  A pixel outside the rectangle (a partial tile) has key 0, below every real pixel's (pixel 0
// of a tile is always inside).  A lane keeps the greatest of its four keys with that pixel's V, six shuffle steps take the maximum across
// the wave, and the one lane whose own key is that maximum writes its V.  sources and unknown are added up in scalar registers from
// ballots, one per pixel slot, and leave through pass_slot with one atomic per wave and non-zero counter.
struct MblurTileArgs {
    const MblurView* tab;
    int width; // of the frame: the planes are indexed Y * width + X
    const float* motion;
    float2* scratch;
    MblurParams k;
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] sources, [1] unknown ([2] moving, [3] taps, [4] nonfinite: k_mblur_gather)
};
#define MBLUR_TILES_PER_BLOCK 4u

__global__ void __launch_bounds__(256) k_mblur_tile(MblurTileArgs a) {
#if __HIP_DEVICE_COMPILE__
    const MblurView L = a.tab[blockIdx.y];
    const uint32_t tile = blockIdx.x * MBLUR_TILES_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= L.tw * L.th) return; // the whole wave; the kernel has no barrier
    const uint32_t ti = tile % L.tw, tj = tile / L.tw;
    const uint32_t lx = (lane & 3u) * 4u, ly = lane >> 2;
    const uint32_t y = tj * 16u + ly;
    float2 m[4];
    bool in[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t x = ti * 16u + lx + k;
        in[k] = x < L.w && y < L.h;
        const uint32_t sx = in[k] ? x : 0u, sy = in[k] ? y : 0u; // (outside: the rectangle's pixel (0, 0), loaded and dropped)
        m[k] = tp_load2(a.motion + 2 * ((size_t)((L.org >> 16) + sy) * (size_t)a.width + (size_t)((L.org & 0xffffu) + sx)));
    }
    unsigned long long own = 0ull;
    float2 mine = make_float2(0.0f, 0.0f);
    uint32_t nin = 0u, nunk = 0u; // wave-uniform
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const MblurVel v = mblur_velocity(m[k], a.k);
        const uint32_t idx = ly * 16u + lx + k;
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

// ------------------------------------------------------------------ k_mblur_neighbour: N, the fastest T of the 3 x 3 tiles around a tile
// One thread per tile, up to nine 8-byte loads, row order, strict >.  The launch is tiny and launch-bound; it is kept as a kernel of its
// own: folded into the gather's prologue every wave would redo the nine loads for a value that 256 pixels share, and N has to reach the
// scratch either way.
struct MblurNeighbourArgs {
    const MblurView* tab;
    float2* scratch;
};

__global__ void __launch_bounds__(256) k_mblur_neighbour(MblurNeighbourArgs a) {
#if __HIP_DEVICE_COMPILE__
    const MblurView L = a.tab[blockIdx.y];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= L.tw * L.th) return;
    const int ti = (int)(i % L.tw), tj = (int)(i / L.tw);
    float2 best = make_float2(0.0f, 0.0f);
    float best2 = 0.0f;
    bool any = false;
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
        for (int di = -1; di <= 1; ++di) {
            const int u = ti + di, v = tj + dj;
            if (u < 0 || u >= (int)L.tw || v < 0 || v >= (int)L.th) continue;
            const float2 t = a.scratch[(size_t)L.offT + (size_t)v * L.tw + (size_t)u];
            const float l2 = t.x * t.x + t.y * t.y;
            if (!any || l2 > best2) {
                best = t;
                best2 = l2;
                any = true;
            }
        }
    a.scratch[(size_t)L.offN + i] = best;
#endif
}

// ------------------------------------------------------------------ k_mblur_gather: step 4, over the call's pixel list
// k_bloom_composite's shape: one thread per entry of the pixel list.  vN is uniform over a tile, so where the list hands a wave one 8 x 8
// block the early exit, the tap count and (without jitter) t are the same in every lane.  A tap costs 28 bytes — colour 16, motion 8,
// depth 4 — and its three loads are issued together, in front of the first use; the taps of neighbouring lanes land on neighbouring
// pixels, so reuse is left to the caches.  The three counters are added up across the wave by shuffles (taps and nonfinite are sums of
// per-lane counts, not ballots) and leave with one atomic per wave and non-zero counter; every lane reaches them.
struct MblurGatherArgs {
    const uint32_t* pixels;
    uint32_t n;
    int width, height;
    const float *color, *motion, *depth;
    float* out;
    const MblurView* tab;
    const float2* scratch;
    MblurParams k;
    float depth_soft;
    uint32_t taps, seed, jitter;
    unsigned long long* counts;
};

PT_DEV uint32_t mblur_wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_mblur_gather(MblurGatherArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t nmoving = 0u, ntaps = 0u, nnonfinite = 0u;
    if (i < a.n) {
        const PassPixel px = pass_pixel<VIEWS>(vp, a.pixels[i], a.width, a.height);
        const size_t p = (size_t)px.Y * (size_t)a.width + px.X;
        const int x = (int)px.X - px.x0, y = (int)px.Y - px.y0;
        const MblurView L = a.tab[px.view];
        const float4 c = tp_load4(a.color + 4 * p);
        const float2 vN = a.scratch[(size_t)L.offN + (size_t)(y >> 4) * L.tw + (size_t)(x >> 4)];
        const float n2 = vN.x * vN.x + vN.y * vN.y;
        v3 o = mk3(c.x, c.y, c.z);
        if (n2 > 0.25f && tp_finite(c.x) && tp_finite(c.y) && tp_finite(c.z)) {
            nmoving = 1u;
            const float lN = sqrtf(n2);
            const float lp = mblur_len(mblur_velocity(tp_load2(a.motion + 2 * p), a.k).l2);
            const float wp = 1.0f / lp;
            const float zp = mblur_depth(a.depth[p]);
            const float j = a.jitter ? (float)(mblur_hash((uint32_t)x, (uint32_t)y, a.seed) >> 8) * 5.9604644775390625e-8f - 0.5f : 0.0f;
            const float ftaps = (float)a.taps;
            v3 sum = mk3(0.0f);
            float Wt = 0.0f;
            for (uint32_t k = 0; k < a.taps; ++k) {
                const float av = ((float)k + 0.5f) + j;
                const float t = (2.0f * av) / ftaps - 1.0f;
                int qx = (int)floorf(((float)x + vN.x * t) + 0.5f), qy = (int)floorf(((float)y + vN.y * t) + 0.5f);
                qx = qx < 0 ? 0 : qx > px.wr - 1 ? px.wr - 1 : qx;
                qy = qy < 0 ? 0 : qy > px.hr - 1 ? px.hr - 1 : qy;
                const size_t q = (size_t)(px.y0 + qy) * (size_t)a.width + (size_t)(px.x0 + qx);
                const float4 cq = tp_load4(a.color + 4 * q); // the tap's three loads, in front of the first use
                const float2 mq = tp_load2(a.motion + 2 * q);
                const float dq = a.depth[q];
                if (!(tp_finite(cq.x) && tp_finite(cq.y) && tp_finite(cq.z))) {
                    ++nnonfinite;
                    continue;
                }
                const float d = fabsf(t) * lN;
                const float lq = mblur_len(mblur_velocity(mq, a.k).l2);
                const float zq = mblur_depth(dq);
                const float e = a.depth_soft * (zp < zq ? zp : zq);
                const float fg = mblur_clamp01(1.0f - (zq - zp) / e), bg = mblur_clamp01(1.0f - (zp - zq) / e);
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
    nmoving = mblur_wave_sum(nmoving);
    ntaps = mblur_wave_sum(ntaps);
    nnonfinite = mblur_wave_sum(nnonfinite);
    if ((threadIdx.x & 63u) == 0u) {
        unsigned long long* slot = pass_slot(a.counts);
        if (nmoving) atomicAdd(slot + 2, (unsigned long long)nmoving);
        if (ntaps) atomicAdd(slot + 3, (unsigned long long)ntaps);
        if (nnonfinite) atomicAdd(slot + 4, (unsigned long long)nnonfinite);
    }
#endif
}
