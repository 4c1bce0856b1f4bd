// pt_upsample_planes (include/pt_amd.h): a joint-bilateral upsample of a low-resolution colour plane to the context's resolution under the
// guidance of both G-buffers — ONE kernel, stateless, every plane the caller's.  The "same surface" tests are those of k_temporal and
// k_filter_pass (mesh, normal, plane distance), so the chain keeps its single notion of a surface across the change of resolution.
#pragma once
#include "pt_pass_dev.h"

// One thread per entry of the frame's pixel list, 256 per block, as k_filter_prepare.  The list is in 8x8-block order, so a wave is one
// full-resolution block and its taps fall into a window of at most (8 / s + 3)^2 low-resolution pixels: the reuse between the lanes of a wave
// (s^2 pixels share a low-res pixel) and between neighbouring waves is left to the L2, as in the filter.  No LDS: DESIGN.md §8o has the
// bytes and the measured time that decision rests on.
//
// Loads go cheapest first.  The pixel: its pt_hit as two 16-byte loads, its position as a third only for a hit.  A tap of a hit: the
// 16-byte second half of the low-res pt_hit (mesh, ng), then the prim word, then the 16-byte position, each only while the tap is still
// alive; a tap of a miss: the prim word alone; the 16-byte colour last.  The plane test is a dot with a DIFFERENCE of positions, as in the filter, so the guide planes are read as they are.  The
// rescue loop is entered only by the lanes whose bilinear stage found nothing.  The arithmetic is the header's, in the header's order, one
// float32 rounding per operation (-ffp-contract=off is part of the library's flags): tests/upsample_ref.py reproduces every output bit.
struct UpsampleArgs {
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    int width, height; // the frame: the full-resolution planes are indexed Y * width + X
    int lo_width;      // the low-resolution planes are indexed y * lo_width + x
    int scale;         // 2..4; lo_width * scale == width
    const float *lo_color, *lo_hit, *lo_position, *hit, *position;
    float* out;
    float* weight_out;          // or null
    float normal_cos, plane_eps;
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] hits, [1] full, [2] rescued, [3] orphans of a slot (pass_slot); zero at launch
};

// a / s for 0 <= a < 65536 and s in 2..4 without a division: 3 * 43691 = 2^17 + 1, so (a * 43691) >> 17 = floor(a / 3 + a / (3 * 2^17)),
// and the second term stays below 1/6 while the fraction of a / 3 is at most 2/3
PT_DEV int up_div(int a, int s) { return s == 2 ? a >> 1 : s == 4 ? a >> 2 : (int)(((uint32_t)a * 43691u) >> 17); }

// the pixel's low-resolution rectangle [lx0, lx1) x [ly0, ly1), and its side of the tap tests
struct UpsamplePixel {
    int lx0, ly0, lx1, ly1;
    SurfaceKey key;
};

// One axis of the header: the low-res pixel that holds the coordinate (c), the first tap (i) and the weight of the second tap (f).
PT_DEV void up_axis(int X, int x0, int s, int& c, int& i, float& f) {
    const int a = X - x0;
    const int d = up_div(a, s);
    const int r = a - d * s;
    c = up_div(x0, s) + d;
    const float t = (float)(2 * r + 1 - s) / (float)(2 * s);
    if (t < 0.0f) {
        i = c - 1;
        f = t + 1.0f;
    } else {
        i = c;
        f = t;
    }
}

// Does low-res pixel (qx, qy) count for the pixel?  Its colour is loaded only when everything before it held.
PT_DEV bool up_counts(const UpsampleArgs& a, const UpsamplePixel& p, int qx, int qy, float4& c) {
    if (qx < p.lx0 || qx >= p.lx1 || qy < p.ly0 || qy >= p.ly1) return false;
    const size_t q = (size_t)qy * (size_t)a.lo_width + (size_t)qx;
    if (p.key.miss) {
        if (!hit_is_miss(a.lo_hit[8 * q + 3])) return false;
    } else {
        if (!same_facet(p.key, a.lo_hit, q, a.normal_cos)) return false;
        if (hit_is_miss(a.lo_hit[8 * q + 3])) return false;
        if (!same_plane(p.key, a.lo_position, q)) return false;
    }
    c = tp_load4(a.lo_color + 4 * q);
    return tp_finite(c.x) && tp_finite(c.y) && tp_finite(c.z);
}

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_upsample(UpsampleArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    bool is_hit = false, is_full = false, is_rescued = false, is_orphan = false;
    if (idx < a.n) {
        const PassPixel px = pass_pixel<VIEWS>(vp, a.pixels[idx], a.width, a.height);
        const int X = (int)px.X, Y = (int)px.Y, x0 = px.x0, y0 = px.y0;
        const int s = a.scale;
        UpsamplePixel p;
        p.lx0 = up_div(x0, s);
        p.ly0 = up_div(y0, s);
        p.lx1 = up_div(x0 + px.wr, s);
        p.ly1 = up_div(y0 + px.hr, s);
        const size_t pi = (size_t)Y * (size_t)a.width + (size_t)X;
        const float4 ha = tp_load4(a.hit + 8 * pi), hb = tp_load4(a.hit + 8 * pi + 4); // t, u, v, prim | mesh, ng.xyz
        is_hit = !hit_is_miss(ha.w);
        p.key = surface_key(!is_hit, ha.x, hb, make_float4(0.0f, 0.0f, 0.0f, 0.0f), a.plane_eps);
        if (is_hit) { // the position only for a hit, and its three words only
            const float4 P = tp_load4(a.position + 4 * pi);
            p.key.P = mk3(P.x, P.y, P.z);
        }
        int cx, cy, i, j;
        float fx, fy;
        up_axis(X, x0, s, cx, i, fx);
        up_axis(Y, y0, s, cy, j, fy);
        // ---------------- the bilinear stage: taps (0,0), (1,0), (0,1), (1,1)
        float4 S = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float W = 0.0f;
        int counted = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int dx = k & 1, dy = k >> 1;
            const float wx = dx ? fx : 1.0f - fx, wy = dy ? fy : 1.0f - fy;
            const float w = wx * wy;
            float4 c;
            if (w != 0.0f && up_counts(a, p, i + dx, j + dy, c)) {
                S.x += c.x * w;
                S.y += c.y * w;
                S.z += c.z * w;
                S.w += c.w * w;
                W += w;
                ++counted;
            }
        }
        float4 o;
        float wo = W;
        if (W > 0.0f) {
            o = make_float4(S.x / W, S.y / W, S.z / W, S.w / W);
            is_full = counted == 4;
        } else {
            // ---------------- the rescue: the 16 low-res pixels around the taps, unweighted
            float N = 0.0f;
            S = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 1
            for (int dy = -1; dy <= 2; ++dy)
#pragma unroll 1
                for (int dx = -1; dx <= 2; ++dx) {
                    float4 c;
                    if (up_counts(a, p, i + dx, j + dy, c)) {
                        S.x += c.x;
                        S.y += c.y;
                        S.z += c.z;
                        S.w += c.w;
                        N += 1.0f;
                    }
                }
            if (N > 0.0f) {
                o = make_float4(S.x / N, S.y / N, S.z / N, S.w / N);
                wo = 0.0f;
                is_rescued = true;
            } else {
                // ---------------- the orphan: the low-res pixel that contains p, as it is
                o = tp_load4(a.lo_color + 4 * ((size_t)cy * (size_t)a.lo_width + (size_t)cx));
                wo = -1.0f;
                is_orphan = true;
            }
        }
        gb_store4(a.out + 4 * pi, o);
        if (a.weight_out) a.weight_out[pi] = wo;
    }
    pass_tally(pass_slot(a.counts), {is_hit, is_full, is_rescued, is_orphan});
#endif
}
