// pt_upsample_planes (include/pt_amd.h): a joint-bilateral upsample of a low-resolution colour plane to the context's resolution under the
// guidance of both G-buffers — ONE kernel, stateless, every plane the caller's.  The "same surface" tests are those of k_temporal and
// k_filter_pass (mesh, normal, plane distance), so the chain keeps its single notion of a surface across the change of resolution.
#pragma once
#include "pt_temporal.h"

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
    unsigned long long* counts; // [UPSAMPLE_SLOTS][8]: [0] hits, [1] full, [2] rescued, [3] orphans of a slot; zero at launch
};
// One 64-bit atomic per wave and non-zero count, into the wave's slot of 64 (64 bytes apart), as k_surface_lod.
#define UPSAMPLE_SLOTS 64u

// a / s for 0 <= a < 65536 and s in 2..4 without a division: 3 * 43691 = 2^17 + 1, so (a * 43691) >> 17 = floor(a / 3 + a / (3 * 2^17)),
// and the second term stays below 1/6 while the fraction of a / 3 is at most 2/3
PT_DEV int up_div(int a, int s) { return s == 2 ? a >> 1 : s == 4 ? a >> 2 : (int)(((uint32_t)a * 43691u) >> 17); }

// the pixel's side of the tap tests, and its low-resolution rectangle [lx0, lx1) x [ly0, ly1)
struct UpsamplePixel {
    int lx0, ly0, lx1, ly1;
    bool miss;
    int mesh;
    v3 ng, P;
    float plane_max;
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
    if (p.miss) {
        if (__float_as_int(a.lo_hit[8 * q + 3]) >= 0) return false;
    } else {
        const float4 qb = tp_load4(a.lo_hit + 8 * q + 4);
        if (__float_as_int(qb.x) != p.mesh || !(dot3(p.ng, mk3(qb.y, qb.z, qb.w)) >= a.normal_cos)) return false;
        if (__float_as_int(a.lo_hit[8 * q + 3]) < 0) return false;
        const float4 Q = tp_load4(a.lo_position + 4 * q);
        if (!(fabsf(dot3(p.ng, mk3(Q.x - p.P.x, Q.y - p.P.y, Q.z - p.P.z))) <= p.plane_max)) return false;
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
        const uint32_t xy = a.pixels[idx];
        const int X = (int)(xy & 0xffffu), Y = (int)(xy >> 16);
        int x0 = 0, y0 = 0, x1 = a.width, y1 = a.height;
        if (VIEWS) {
            const uint32_t vi = vp.vblock[(uint32_t)(Y >> 3) * vp.nbx + (uint32_t)(X >> 3)]; // the list holds view pixels only: never 0xffff
            x0 = vp.views[vi].x;
            y0 = vp.views[vi].y;
            x1 = x0 + vp.views[vi].width;
            y1 = y0 + vp.views[vi].height;
        }
        const int s = a.scale;
        UpsamplePixel p;
        p.lx0 = up_div(x0, s);
        p.ly0 = up_div(y0, s);
        p.lx1 = up_div(x1, s);
        p.ly1 = up_div(y1, s);
        const size_t pi = (size_t)Y * (size_t)a.width + (size_t)X;
        const float4 ha = tp_load4(a.hit + 8 * pi), hb = tp_load4(a.hit + 8 * pi + 4); // t, u, v, prim | mesh, ng.xyz
        p.miss = __float_as_int(ha.w) < 0;
        p.mesh = __float_as_int(hb.x);
        p.ng = mk3(hb.y, hb.z, hb.w);
        p.P = mk3(0.0f);
        p.plane_max = a.plane_eps * ha.x;
        is_hit = !p.miss;
        if (is_hit) {
            const float4 P = tp_load4(a.position + 4 * pi);
            p.P = mk3(P.x, P.y, P.z);
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
    const unsigned long long hm = __ballot(is_hit), fm = __ballot(is_full), rm = __ballot(is_rescued), om = __ballot(is_orphan);
    if ((threadIdx.x & 63u) == 0u) {
        unsigned long long* slot = a.counts + 8u * ((blockIdx.x * 4u + (threadIdx.x >> 6)) & (UPSAMPLE_SLOTS - 1u));
        if (hm) atomicAdd(slot, (unsigned long long)__popcll(hm));
        if (fm) atomicAdd(slot + 1, (unsigned long long)__popcll(fm));
        if (rm) atomicAdd(slot + 2, (unsigned long long)__popcll(rm));
        if (om) atomicAdd(slot + 3, (unsigned long long)__popcll(om));
    }
#endif
}
