// pt_lens_warp_planes (include/pt_amd.h): lens pre-distortion with per-channel coefficients and rotational late reprojection, the last pass
// of the chain — ONE gather kernel, stateless, every plane the caller's.  Each output pixel computes up to three source points (one per
// colour channel: a radial polynomial around the lens centre, then a 3x3 matrix in pixel coordinates) and resamples the colour there,
// bilinear (2 x 2 taps) or Catmull-Rom (4 x 4).
#pragma once
#include "pt_pass_dev.h"

// One thread per entry of the frame's pixel list, 256 per block, no scratch, no LDS: the shape of k_edge_aa.  The list is in 8x8-block
// order, so a wave is one block, and under a smooth warp its source points cover a patch of about a block's size: most of a tap's lines are
// shared inside the wave, the rest with the neighbouring waves.  The reuse is left to L1/L2 (profiles/lens_warp.md has what they make of it).
//
// The table is the caller's pt_lens_view array as it is (LW_WORDS floats a view, or the identity the host wrote for lenses == NULL), read
// through the view index: without views that index is 0 for every lane, and the loads are scalar.
//
// CHROMA false: the host found the three k rows of every view equal word for word, so steps 1 to 6 run once and a tap is one 16-byte
// load for three channels — 4 or 16 loads a pixel.  CHROMA true: the channel loop stays ROLLED (one body, 4-byte loads of the channel's own
// word, 12 or 48 loads a pixel), which keeps the bicubic variant's registers at one channel's worth.  Both give the bits of the header's
// rule: lw_source and the weights are the same code, and a sum of one channel never meets another channel's.
//
// The arithmetic is the header's, in the header's order, one float32 rounding per operation (-ffp-contract=off is part of the library's
// flags).  No float becomes an int and no address is formed before step 5 has placed the source point in [0, wr] x [0, hr]; from there
// ix, iy lie in [-1, wr - 1] x [-1, hr - 1], and every tap is clamped to the rectangle, which lies inside the frame.
#define LW_WORDS 24u // sizeof(pt_lens_view) / 4: center 0, inv_radius 2, k 4, warp 13, reserved 22
struct LensWarpArgs {
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    int width, height;      // the frame: the planes are indexed Y * width + X
    const float* color;
    float* out;             // or null
    uint32_t* frame;        // or null
    const float* lenses;    // [max(1, views)][LW_WORDS]
    float border[3];
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] outside, [1] nonfinite of a slot (pass_slot); zero at launch
};

// Steps 1 to 6 for one channel: where its source point lies.  in false: outside (ix, iy, tx, ty are then not to be used).
struct LwSource {
    bool in;
    int ix, iy;
    float tx, ty;
};
PT_DEV LwSource lw_source(const float* L, uint32_t ch, int x, int y, float fwr, float fhr) {
    const float cx = L[0], cy = L[1], irx = L[2], iry = L[3];
    const float k1 = L[4u + 3u * ch], k2 = L[5u + 3u * ch], k3 = L[6u + 3u * ch];
    const float* H = L + 13;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const float qx = px - cx, qy = py - cy;
    const float ax = qx * irx, ay = qy * iry;
    const float r2 = ax * ax + ay * ay;
    const float g = r2 * (k1 + r2 * (k2 + r2 * k3));
    const float ux = px + qx * g, uy = py + qy * g;
    const float a = (H[0] * ux + H[1] * uy) + H[2];
    const float b = (H[3] * ux + H[4] * uy) + H[5];
    const float c = (H[6] * ux + H[7] * uy) + H[8];
    LwSource s{false, 0, 0, 0.0f, 0.0f};
    if (!(c > 0.0f)) return s; // a NaN is outside
    const float sx = a / c, sy = b / c;
    if (!(sx >= 0.0f && sx <= fwr && sy >= 0.0f && sy <= fhr)) return s;
    const float fx = sx - 0.5f, fy = sy - 0.5f;
    const float flx = floorf(fx), fly = floorf(fy);
    s.in = true;
    s.ix = (int)flx;
    s.iy = (int)fly;
    s.tx = fx - flx;
    s.ty = fy - fly;
    return s;
}
PT_DEV int lw_clamp(int v, int n) { return v < 0 ? 0 : v > n - 1 ? n - 1 : v; }
// a colour word as a tap reads it: 0 where it is not finite, and counted
PT_DEV float lw_word(float v, uint32_t& bad) {
    if (tp_finite(v)) return v;
    ++bad;
    return 0.0f;
}
// Catmull-Rom weights of step 8
PT_DEV void lw_cubic(float t, float (&w)[4]) {
    w[0] = ((-0.5f * t + 1.0f) * t - 0.5f) * t;
    w[1] = ((1.5f * t - 2.5f) * t) * t + 1.0f;
    w[2] = ((-1.5f * t + 2.0f) * t + 0.5f) * t;
    w[3] = ((0.5f * t - 0.5f) * t) * t;
}

// Steps 7 and 8 over N = 1 (CHROMA: the word at color + ch) or 3 channels of one source point.  T: 2 or 4 taps a side, first tap at
// (ix + o, iy + o) with o = 0 or -1.
template <int T, int N>
PT_DEV void lw_resample(const float* color, const PassPixel& px, int width, const LwSource& s, float (&val)[N], uint32_t& bad) {
    float wx[T], wy[T];
    if constexpr (T == 2) {
        wx[0] = 1.0f - s.tx, wx[1] = s.tx;
        wy[0] = 1.0f - s.ty, wy[1] = s.ty;
    } else {
        float w4[4];
        lw_cubic(s.tx, w4);
#pragma unroll
        for (int i = 0; i < T; ++i) wx[i] = w4[i];
        lw_cubic(s.ty, w4);
#pragma unroll
        for (int i = 0; i < T; ++i) wy[i] = w4[i];
    }
    const int o = T == 2 ? 0 : -1;
    size_t col[T];
#pragma unroll
    for (int i = 0; i < T; ++i) col[i] = 4 * (size_t)(px.x0 + lw_clamp(s.ix + o + i, px.wr));
    if constexpr (T == 2) {
        // val = ((c00*w00 + c10*w10) + c01*w01) + c11*w11 with w_ij = wx[i] * wy[j]
        float c[4][N];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float* q = color + 4 * (size_t)(px.y0 + lw_clamp(s.iy + (k >> 1), px.hr)) * (size_t)width + col[k & 1];
            if constexpr (N == 3) {
                const float4 v = tp_load4(q);
                c[k][0] = lw_word(v.x, bad);
                c[k][1] = lw_word(v.y, bad);
                c[k][2] = lw_word(v.z, bad);
            } else {
                c[k][0] = lw_word(q[0], bad);
            }
        }
        const float w00 = wx[0] * wy[0], w10 = wx[1] * wy[0], w01 = wx[0] * wy[1], w11 = wx[1] * wy[1];
#pragma unroll
        for (int n = 0; n < N; ++n) val[n] = ((c[0][n] * w00 + c[1][n] * w10) + c[2][n] * w01) + c[3][n] * w11;
    } else {
        float row[4][N];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* r = color + 4 * (size_t)(px.y0 + lw_clamp(s.iy + o + j, px.hr)) * (size_t)width;
            float c[4][N];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (N == 3) {
                    const float4 v = tp_load4(r + col[i]);
                    c[i][0] = lw_word(v.x, bad);
                    c[i][1] = lw_word(v.y, bad);
                    c[i][2] = lw_word(v.z, bad);
                } else {
                    c[i][0] = lw_word(r[col[i]], bad);
                }
            }
#pragma unroll
            for (int n = 0; n < N; ++n) row[j][n] = ((c[0][n] * wx[0] + c[1][n] * wx[1]) + c[2][n] * wx[2]) + c[3][n] * wx[3];
        }
#pragma unroll
        for (int n = 0; n < N; ++n) val[n] = ((row[0][n] * wy[0] + row[1][n] * wy[1]) + row[2][n] * wy[2]) + row[3][n] * wy[3];
    }
}

template <bool VIEWS, bool CHROMA, bool BICUBIC>
__global__ void __launch_bounds__(256) k_lens_warp(LensWarpArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    constexpr int T = BICUBIC ? 4 : 2;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t tally[2] = {0u, 0u}; // outside (0 or 1), nonfinite words
    if (i < a.n) {
        const PassPixel px = pass_pixel<VIEWS>(vp, a.pixels[i], a.width, a.height);
        const size_t pi = (size_t)px.Y * (size_t)a.width + (size_t)px.X;
        const int x = (int)px.X - px.x0, y = (int)px.Y - px.y0;
        const float fwr = (float)px.wr, fhr = (float)px.hr;
        const float* L = a.lenses + (size_t)LW_WORDS * px.view;
        float r = a.border[0], g = a.border[1], b = a.border[2];
        bool all_in;
        if (CHROMA) {
            uint32_t inside = 0u;
#pragma unroll 1
            for (uint32_t ch = 0; ch < 3u; ++ch) {
                const LwSource s = lw_source(L, ch, x, y, fwr, fhr);
                if (s.in) {
                    float val[1];
                    lw_resample<T, 1>(a.color + ch, px, a.width, s, val, tally[1]);
                    r = ch == 0u ? val[0] : r;
                    g = ch == 1u ? val[0] : g;
                    b = ch == 2u ? val[0] : b;
                    ++inside;
                }
            }
            all_in = inside == 3u;
        } else {
            const LwSource s = lw_source(L, 0u, x, y, fwr, fhr);
            all_in = s.in;
            if (s.in) {
                float val[3];
                lw_resample<T, 3>(a.color, px, a.width, s, val, tally[1]);
                r = val[0], g = val[1], b = val[2];
            }
        }
        tally[0] = all_in ? 0u : 1u;
        if (a.out) gb_store4(a.out + 4 * pi, make_float4(r, g, b, all_in ? 1.0f : 0.0f));
        if (a.frame) a.frame[pi] = make_color(mk3(r, g, b));
    }
    pass_tally_sums(a.counts, 0u, tally);
#endif
}
