// pt_filter_planes (include/pt_amd.h): a view-aware, variance-guided a-trous filter over the G-buffer's exact planes — TWO kernels, stateless,
// every plane the caller's.  k_filter_prepare makes the record (colour, variance) of every pixel of the set, k_filter_pass is one a-trous
// pass at tap spacing `step`; the passes ping-pong between the caller's `out` and `scratch`.
#pragma once
#include "pt_pass_dev.h"

// One thread per entry of the frame's pixel list, as k_temporal.  The list is in 8x8-block order, so a wave is one block, and the lanes' tap
// (dx, dy) is the same block displaced by step * (dx, dy): eight runs of eight neighbouring pixels, 128 contiguous bytes of each 16-byte
// plane per run.  A tap of the wave therefore moves whole 128-byte lines at every step, and the reuse between neighbouring blocks (each
// displaced block is some other wave's tap, too) is left to the L2.  No LDS: see DESIGN.md §8h for what a residue-class tile would save and
// why this first version does not stage one.
//
// What a tap costs: the 16-byte record, the 16-byte second half of the pt_hit (mesh, ng) and, only while it is still alive, the 16-byte
// position.  The guide planes are read as they are: the plane test is a dot with a DIFFERENCE of positions, and
// dot3(ng, Q - P) is not dot3(ng, Q) - dot3(ng, P) in float32, so a repacked plane offset could not keep the header's bits.
// Inert pixels are marked in the intermediate records (variance word FL_INERT = -1.0f, a value no stage can compute: a variance is a sum of
// products of non-negative numbers, or a NaN), so a pass needs neither the colour plane nor the first half of the hit record again; the
// last stage writes the 0.0f the header specifies instead.  The arithmetic is the header's, in the header's order, one float32 rounding per
// operation (-ffp-contract=off is part of the library's flags): tests/filter_ref.py reproduces every output bit.
struct FilterArgs {
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    int width, height;    // the frame: the planes are indexed Y * width + X
    const float *color, *hit, *position;
    const float *variance, *length; // or null
    const float* src;               // the previous stage's records (k_filter_pass)
    float* dst;                     // this stage's records
    uint32_t* frame;                // or null; the last stage only
    const uint8_t* inset;           // [nbx * nby] 1 = the block belongs to the call's set (owned by the rank, named by the mask)
    uint32_t nbx;
    float sigma_lum, normal_cos, plane_eps, min_length;
    int step;
    uint32_t last;                  // this stage's records are the call's output
    unsigned long long* counts;     // {filtered, spatial}, zero at launch; one atomic per wave (k_filter_prepare)
};

#define FL_INERT_BITS 0xbf800000u // -1.0f

PT_DEV float fl_min80(float v) { return v < 80.0f ? v : 80.0f; }

// the pixel's side of the tap tests (pt_pass_dev.h): the pixel and its rectangle; mesh, normal, position, plane bound
struct FilterPixel {
    PassPixel px;
    SurfaceKey key;
};
// An inert pixel never gets here, so the key is never a miss's; the first half of the hit record gives its t alone.
PT_DEV void fl_guides(const FilterArgs& a, FilterPixel& p, size_t pi) {
    p.key = surface_key(false, a.hit[8 * pi], tp_load4(a.hit + 8 * pi + 4), tp_load4(a.position + 4 * pi), a.plane_eps);
}
// rect and block: is (qx, qy) a pixel whose planes and record may be looked at
PT_DEV bool fl_reachable(const FilterArgs& a, const FilterPixel& p, int qx, int qy) { return pass_reachable(p.px, a.inset, a.nbx, qx, qy); }
// mesh, normal, plane
PT_DEV bool fl_same_surface(const FilterArgs& a, const FilterPixel& p, size_t q) {
    return same_facet(p.key, a.hit, q, a.normal_cos) && same_plane(p.key, a.position, q);
}
PT_DEV bool fl_inert_input(const FilterArgs& a, size_t q, float4 c) {
    return hit_is_miss(a.hit[8 * q + 3]) || !(tp_finite(c.x) && tp_finite(c.y) && tp_finite(c.z));
}
PT_DEV void fl_store(const FilterArgs& a, size_t pi, float4 rec, bool inert) {
    if (inert) rec.w = a.last ? 0.0f : __uint_as_float(FL_INERT_BITS);
    gb_store4(a.dst + 4 * pi, rec);
    if (a.frame) a.frame[pi] = make_color(mk3(rec.x, rec.y, rec.z));
}

// ---------------------------------------------------------------- stage 0: the record (colour, variance) of every pixel of the set
template <bool VIEWS>
__global__ void __launch_bounds__(256) k_filter_prepare(FilterArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool live = false, spatial = false;
    if (i < a.n) {
        FilterPixel p;
        p.px = pass_pixel<VIEWS>(vp, a.pixels[i], a.width, a.height);
        const size_t pi = (size_t)p.px.Y * (size_t)a.width + (size_t)p.px.X;
        const float4 c = tp_load4(a.color + 4 * pi);
        live = !fl_inert_input(a, pi, c);
        float v = 0.0f;
        if (live) {
            spatial = a.variance == nullptr || (a.length != nullptr && a.length[pi] < a.min_length);
            if (!spatial) {
                v = fl_max0(a.variance[pi]);
            } else {
                fl_guides(a, p, pi);
                float n = 0.0f, s1 = 0.0f, s2 = 0.0f;
                for (int dy = -3; dy <= 3; ++dy)
                    for (int dx = -3; dx <= 3; ++dx) {
                        const int qx = (int)p.px.X + dx, qy = (int)p.px.Y + dy;
                        bool counts = (dx | dy) == 0;
                        float4 cq = c;
                        if (!counts && fl_reachable(a, p, qx, qy)) {
                            const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
                            cq = tp_load4(a.color + 4 * q);
                            counts = !fl_inert_input(a, q, cq) && fl_same_surface(a, p, q);
                        }
                        if (counts) {
                            const float l = fl_lum(cq.x, cq.y, cq.z);
                            n += 1.0f;
                            s1 += l;
                            s2 += l * l;
                        }
                    }
                const float m = s1 / n;
                v = fl_max0(s2 / n - m * m);
            }
        }
        fl_store(a, pi, make_float4(c.x, c.y, c.z, v), !live);
    }
    pass_tally(a.counts, {live, spatial});
#endif
}

// ---------------------------------------------------------------- stage i: one a-trous pass at spacing `step`
template <bool VIEWS>
__global__ void __launch_bounds__(256) k_filter_pass(FilterArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    FilterPixel p;
    p.px = pass_pixel<VIEWS>(vp, a.pixels[i], a.width, a.height);
    const size_t pi = (size_t)p.px.Y * (size_t)a.width + (size_t)p.px.X;
    const float4 r = tp_load4(a.src + 4 * pi);
    if (__float_as_uint(r.w) == FL_INERT_BITS) {
        fl_store(a, pi, r, true);
        return;
    }
    fl_guides(a, p, pi);
    // 1. the variance, prefiltered over the 3x3 window at spacing 1
    float G = 0.0f, K = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const float kk = (dy ? 0.25f : 0.5f) * (dx ? 0.25f : 0.5f);
            float vq = r.w;
            bool counts = (dx | dy) == 0;
            const int qx = (int)p.px.X + dx, qy = (int)p.px.Y + dy;
            if (!counts && fl_reachable(a, p, qx, qy)) {
                const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
                vq = a.src[4 * q + 3];
                counts = __float_as_uint(vq) != FL_INERT_BITS && fl_same_surface(a, p, q);
            }
            if (counts) {
                G += kk * vq;
                K += kk;
            }
        }
    const float g = G / K;
    // 2.
    const float den = a.sigma_lum * sqrtf(g) + 1e-6f;
    const float lp = fl_lum(r.x, r.y, r.z);
    // 3. the 25 taps, row-major
    float Sx = 0.0f, Sy = 0.0f, Sz = 0.0f, V = 0.0f, W = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float ky = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
            const float kx = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
            const float kk = ky * kx;
            float4 rq = r;
            bool counts = (dx | dy) == 0;
            const int qx = (int)p.px.X + a.step * dx, qy = (int)p.px.Y + a.step * dy;
            if (!counts && fl_reachable(a, p, qx, qy)) {
                const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
                rq = tp_load4(a.src + 4 * q);
                counts = __float_as_uint(rq.w) != FL_INERT_BITS && fl_same_surface(a, p, q);
            }
            if (counts) {
                const float e = fl_min80(fabsf(lp - fl_lum(rq.x, rq.y, rq.z)) / den);
                const float w = pt_expf(-e) * kk;
                Sx += rq.x * w;
                Sy += rq.y * w;
                Sz += rq.z * w;
                V += (w * w) * rq.w;
                W += w;
            }
        }
    // 4.
    fl_store(a, pi, make_float4(Sx / W, Sy / W, Sz / W, V / (W * W)), false);
#endif
}
