// pt_bloom_layout and pt_bloom_planes (include/pt_amd.h): bloom as a multi-resolution filter over a pyramid per view in caller memory.
// The bright-passed source and the first down step are one kernel (k_bloom_down1: it reads the frame once and writes a quarter of it), the
// further levels that are still large are one thread per texel (k_bloom_down, k_bloom_up), the small ones are one workgroup per view that
// walks down AND back up through the scratch (k_bloom_tail), and the last up step is fused into the composite (k_bloom_composite).
//
// A level is w x h float4 texels (xyz, w = 0), 16-byte aligned: every access of the pyramid is one 16-byte load or store.  The level table
// (BloomLevel, [views][BLOOM_STRIDE]) is a temporary of the call in device memory; entry 0 of a view is its rectangle (org = x0 | y0 << 16
// in the frame), entries 1 .. levels its levels (off: the level's first float4 in the scratch).  One launch covers all views of a level:
// blockIdx.y is the view, and a block past the end of its view's level leaves at once.  Only the composite needs the view of a PIXEL
// (ViewParams); everything above it works in a rectangle's own coordinates, which is what keeps a tap from leaving it.
#pragma once
#include "pt_pass_dev.h"

#define BLOOM_STRIDE (PT_BLOOM_MAX_LEVELS + 1u)
#define BLOOM_TW 32u                        // k_bloom_down1's output tile: 32 x 8 texels of level 1, one per thread
#define BLOOM_TH 8u
#define BLOOM_SW (2u * BLOOM_TW + 2u)       // its source window: 66 x 18 pixels (stride 2, four taps: one pixel of halo in front, one behind)
#define BLOOM_SH (2u * BLOOM_TH + 2u)
#define BLOOM_SN (BLOOM_SW * BLOOM_SH)
#define BLOOM_TAIL_THREADS 1024u

struct BloomLevel {
    uint32_t w, h, off, org;
};

PT_DEV int bloom_clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
PT_DEV v3 bloom_texel(const float4* lvl, uint32_t w, int x, int y) {
    const float4 t = lvl[(size_t)y * w + (size_t)x];
    return mk3(t.x, t.y, t.z);
}
PT_DEV float bloom_row(float s0, float s1, float s2, float s3) { return ((s0 + 3.0f * s1) + 3.0f * s2) + s3; }

// "Down" of the header: texel (i, j) of a level from the level ws x hs above it
PT_DEV v3 bloom_down(const float4* src, uint32_t ws, uint32_t hs, int i, int j) {
    int cx[4], cy[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        cx[t] = bloom_clampi(2 * i - 1 + t, (int)ws - 1);
        cy[t] = bloom_clampi(2 * j - 1 + t, (int)hs - 1);
    }
    v3 r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const v3 s0 = bloom_texel(src, ws, cx[0], cy[u]), s1 = bloom_texel(src, ws, cx[1], cy[u]), s2 = bloom_texel(src, ws, cx[2], cy[u]),
                 s3 = bloom_texel(src, ws, cx[3], cy[u]);
        r[u] = mk3(bloom_row(s0.x, s1.x, s2.x, s3.x), bloom_row(s0.y, s1.y, s2.y, s3.y), bloom_row(s0.z, s1.z, s2.z, s3.z));
    }
    const float k = 1.0f / 64.0f;
    return mk3(bloom_row(r[0].x, r[1].x, r[2].x, r[3].x) * k, bloom_row(r[0].y, r[1].y, r[2].y, r[3].y) * k, bloom_row(r[0].z, r[1].z, r[2].z, r[3].z) * k);
}

PT_DEV float bloom_up1(float a, float b, float c, float d) { return 0.75f * (0.75f * a + 0.25f * b) + 0.25f * (0.75f * c + 0.25f * d); }
// "up_k" of the header at texel (x, y) of level k, from the level wu x hu below it
PT_DEV v3 bloom_up(const float4* U, uint32_t wu, uint32_t hu, int x, int y) {
    const int i = x >> 1, j = y >> 1;
    const int i2 = (x & 1) ? (i + 1 < (int)wu ? i + 1 : (int)wu - 1) : (i > 0 ? i - 1 : 0);
    const int j2 = (y & 1) ? (j + 1 < (int)hu ? j + 1 : (int)hu - 1) : (j > 0 ? j - 1 : 0);
    const v3 a = bloom_texel(U, wu, i, j), b = bloom_texel(U, wu, i2, j), c = bloom_texel(U, wu, i, j2), d = bloom_texel(U, wu, i2, j2);
    return mk3(bloom_up1(a.x, b.x, c.x, d.x), bloom_up1(a.y, b.y, c.y, d.y), bloom_up1(a.z, b.z, c.z, d.z));
}

// ------------------------------------------------------------------ k_bloom_down1: the source and the first down step
// The kernel that moves the bytes: it reads every rectangle pixel once (plus the halo: 66 x 18 for 64 x 16, 16 % more) and writes a quarter.
// A workgroup bright-passes the 66 x 18 source window of its 32 x 8 output tile into LDS, component planes of 66 floats a row (14 256 bytes:
// eleven workgroups a CU by LDS, eight by waves), one 16-byte load per window pixel, five per thread, all in flight before the first is
// used.  A window pixel outside the rectangle is the clamped one: LDS holds what the tap would have read.  Each thread then takes its
// texel's 4 x 4 taps from LDS, rows first, then the column — the header's order.  (Neighbouring lanes read LDS two floats apart: a two-way
// bank conflict, 48 reads a thread; at eight tiles a CU for a 1080p frame that is microseconds less than the frame's bytes take.)
// A pixel is TALLIED by the tile that owns it — the 64 x 16 pixels under the tile's texels — not by the tiles that read it as halo: the
// counts are added up per wave in scalar registers from ballots and leave with one atomic per wave and non-zero counter.
struct BloomSourceArgs {
    const BloomLevel* tab;
    int width;          // of the frame: color is indexed Y * width + X
    const float* color;
    const float* state; // or null
    float4* scratch;
    float exposure, threshold, knee, clamp;
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] bright, [1] nonfinite
};

__global__ void __launch_bounds__(256) k_bloom_down1(BloomSourceArgs a) {
#if __HIP_DEVICE_COMPILE__
    __shared__ float s_b[3][BLOOM_SH][BLOOM_SW];
    const uint32_t view = blockIdx.y;
    const BloomLevel L0 = a.tab[view * BLOOM_STRIDE], L1 = a.tab[view * BLOOM_STRIDE + 1u];
    const uint32_t tiles_x = (L1.w + BLOOM_TW - 1u) / BLOOM_TW, tiles = tiles_x * ((L1.h + BLOOM_TH - 1u) / BLOOM_TH);
    if (blockIdx.x >= tiles) return; // the whole workgroup: no barrier is left behind
    const uint32_t ox0 = (blockIdx.x % tiles_x) * BLOOM_TW, oy0 = (blockIdx.x / tiles_x) * BLOOM_TH;
    const int x0 = (int)(L0.org & 0xffffu), y0 = (int)(L0.org >> 16), w0 = (int)L0.w, h0 = (int)L0.h;
    float E = a.state ? a.state[4 * (size_t)view + 1] : 1.0f;
    if (!(tp_finite(E) && E > 0.0f)) E = 1.0f;
    const float s = E * a.exposure;
    const float knee2 = 2.0f * a.knee, kden = 4.0f * a.knee + 1e-4f;
    constexpr uint32_t STEPS = (BLOOM_SN + 255u) / 256u;
    float4 c[STEPS];
    uint32_t lx[STEPS], ly[STEPS];
    bool in[STEPS], own[STEPS];
#pragma unroll
    for (uint32_t k = 0; k < STEPS; ++k) {
        const uint32_t e = k * 256u + threadIdx.x;
        in[k] = e < BLOOM_SN;
        lx[k] = in[k] ? e % BLOOM_SW : 0u;
        ly[k] = in[k] ? e / BLOOM_SW : 0u;
        const int ux = (int)(2u * ox0 + lx[k]) - 1, uy = (int)(2u * oy0 + ly[k]) - 1; // in the rectangle's coordinates, not yet clamped
        own[k] = in[k] && lx[k] >= 1u && lx[k] <= 2u * BLOOM_TW && ly[k] >= 1u && ly[k] <= 2u * BLOOM_TH && ux < w0 && uy < h0;
        const int sx = bloom_clampi(ux, w0 - 1), sy = bloom_clampi(uy, h0 - 1);
        c[k] = tp_load4(a.color + 4 * ((size_t)(y0 + sy) * (size_t)a.width + (size_t)(x0 + sx))); // (past the window: its pixel (0, 0), loaded and dropped)
    }
    uint32_t nbright = 0u, nnonfinite = 0u; // wave-uniform
#pragma unroll
    for (uint32_t k = 0; k < STEPS; ++k) {
        const bool nonfinite = !(tp_finite(c[k].x) && tp_finite(c[k].y) && tp_finite(c[k].z));
        v3 B = mk3(0.0f);
        float g = 0.0f;
        if (!nonfinite) {
            v3 x = mk3(fl_max0(c[k].x), fl_max0(c[k].y), fl_max0(c[k].z));
            x = mk3(x.x < a.clamp ? x.x : a.clamp, x.y < a.clamp ? x.y : a.clamp, x.z < a.clamp ? x.z : a.clamp);
            const float Y = fl_lum(x.x, x.y, x.z) * s, d = Y - a.threshold;
            float t = d + a.knee;
            t = t > 0.0f ? t : 0.0f;
            t = t < knee2 ? t : knee2;
            t = (t * t) / kden;
            float m = t > d ? t : d;
            m = m > 0.0f ? m : 0.0f;
            g = m / (Y > 1e-4f ? Y : 1e-4f);
            B = mk3(x.x * g, x.y * g, x.z * g);
        }
        if (in[k]) {
            s_b[0][ly[k]][lx[k]] = B.x;
            s_b[1][ly[k]][lx[k]] = B.y;
            s_b[2][ly[k]][lx[k]] = B.z;
        }
        nbright += (uint32_t)__popcll(__ballot(own[k] && g > 0.0f));
        nnonfinite += (uint32_t)__popcll(__ballot(own[k] && nonfinite));
    }
    if ((threadIdx.x & 63u) == 0u) {
        unsigned long long* slot = pass_slot(a.counts);
        if (nbright) atomicAdd(slot + 0, (unsigned long long)nbright);
        if (nnonfinite) atomicAdd(slot + 1, (unsigned long long)nnonfinite);
    }
    __syncthreads();
    const uint32_t tx = threadIdx.x % BLOOM_TW, ty = threadIdx.x / BLOOM_TW;
    const uint32_t ox = ox0 + tx, oy = oy0 + ty;
    if (ox < L1.w && oy < L1.h) {
        float v[3];
#pragma unroll
        for (uint32_t ch = 0; ch < 3u; ++ch) {
            float r[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                const float* row = &s_b[ch][2u * ty + u][2u * tx];
                r[u] = bloom_row(row[0], row[1], row[2], row[3]);
            }
            v[ch] = bloom_row(r[0], r[1], r[2], r[3]) * (1.0f / 64.0f);
        }
        a.scratch[(size_t)L1.off + (size_t)oy * L1.w + ox] = make_float4(v[0], v[1], v[2], 0.0f);
    }
#endif
}

// ------------------------------------------------------------------ k_bloom_down, k_bloom_up: one thread per texel of the level written
struct BloomLevelArgs {
    const BloomLevel* tab;
    float4* scratch;
    uint32_t level; // the level written
    float spread;   // k_bloom_up
};

__global__ void __launch_bounds__(256) k_bloom_down(BloomLevelArgs a) {
#if __HIP_DEVICE_COMPILE__
    const BloomLevel S = a.tab[blockIdx.y * BLOOM_STRIDE + a.level - 1u], D = a.tab[blockIdx.y * BLOOM_STRIDE + a.level];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= D.w * D.h) return;
    const v3 v = bloom_down(a.scratch + S.off, S.w, S.h, (int)(i % D.w), (int)(i / D.w));
    a.scratch[(size_t)D.off + i] = make_float4(v.x, v.y, v.z, 0.0f);
#endif
}

// U_k = D_k + spread * up_k(U_{k+1}), in place: a thread reads and writes its own texel of level k and reads four of level k + 1
PT_DEV void bloom_up_texel(float4* scratch, const BloomLevel& L, const BloomLevel& N, uint32_t i, float spread) {
    const v3 u = bloom_up(scratch + N.off, N.w, N.h, (int)(i % L.w), (int)(i / L.w));
    const float4 d = scratch[(size_t)L.off + i];
    scratch[(size_t)L.off + i] = make_float4(d.x + spread * u.x, d.y + spread * u.y, d.z + spread * u.z, 0.0f);
}

__global__ void __launch_bounds__(256) k_bloom_up(BloomLevelArgs a) {
#if __HIP_DEVICE_COMPILE__
    const BloomLevel L = a.tab[blockIdx.y * BLOOM_STRIDE + a.level], N = a.tab[blockIdx.y * BLOOM_STRIDE + a.level + 1u];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= L.w * L.h) return;
    bloom_up_texel(a.scratch, L, N, i, a.spread);
#endif
}

// ------------------------------------------------------------------ k_bloom_tail: the small levels, one workgroup per view
// Levels of a few thousand texels are launch-bound: a kernel each costs more in the gaps between them than in the work.  One workgroup of
// 1024 threads per view runs the down steps first .. levels and then the up steps levels - 1 .. first - 1 (the level it started from),
// through the scratch.  A level is complete before the next step reads it: the writers are waves of this workgroup, so a workgroup-scope
// release, the barrier and a workgroup-scope acquire order them (one CU, one vector cache).  No other workgroup touches a view's levels.
struct BloomTailArgs {
    const BloomLevel* tab;
    float4* scratch;
    uint32_t first, levels; // 2 <= first <= levels
    float spread;
};

PT_DEV void bloom_level_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ void __launch_bounds__(BLOOM_TAIL_THREADS) k_bloom_tail(BloomTailArgs a) {
#if __HIP_DEVICE_COMPILE__
    const BloomLevel* tab = a.tab + blockIdx.x * BLOOM_STRIDE;
    for (uint32_t k = a.first; k <= a.levels; ++k) {
        const BloomLevel S = tab[k - 1u], D = tab[k];
        const uint32_t n = D.w * D.h;
        for (uint32_t i = threadIdx.x; i < n; i += BLOOM_TAIL_THREADS) {
            const v3 v = bloom_down(a.scratch + S.off, S.w, S.h, (int)(i % D.w), (int)(i / D.w));
            a.scratch[(size_t)D.off + i] = make_float4(v.x, v.y, v.z, 0.0f);
        }
        bloom_level_barrier();
    }
    for (uint32_t k = a.levels - 1u; k + 1u >= a.first; --k) { // k = levels - 1 .. first - 1 (first - 1 >= 1)
        const BloomLevel L = tab[k], N = tab[k + 1u];
        const uint32_t n = L.w * L.h;
        for (uint32_t i = threadIdx.x; i < n; i += BLOOM_TAIL_THREADS) bloom_up_texel(a.scratch, L, N, i, a.spread);
        bloom_level_barrier();
    }
#endif
}

// ------------------------------------------------------------------ k_bloom_composite: the last up step and the composite
// k_tonemap's shape — one thread per entry of the call's pixel list, the colour streamed — plus four gathers of U_1 (a quarter of the
// frame: neighbouring pixels share them).  out may be color itself: a pixel reads its own colour before it writes.
struct BloomCompositeArgs {
    const uint32_t* pixels;
    uint32_t n;
    int width, height;
    const float* color;
    float* out;
    const BloomLevel* tab;
    const float4* scratch;
    float a; // intensity * (1 / n)
};

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_bloom_composite(BloomCompositeArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const PassPixel px = pass_pixel<VIEWS>(vp, a.pixels[i], a.width, a.height);
    const size_t p = (size_t)px.Y * (size_t)a.width + px.X;
    const float4 c = tp_load4(a.color + 4 * p);
    const BloomLevel L1 = a.tab[px.view * BLOOM_STRIDE + 1u];
    const v3 u = bloom_up(a.scratch + L1.off, L1.w, L1.h, (int)px.X - px.x0, (int)px.Y - px.y0);
    gb_store4(a.out + 4 * p, make_float4(c.x + a.a * u.x, c.y + a.a * u.y, c.z + a.a * u.z, 1.0f));
#endif
}
