// pt_temporal_moments and pt_modulate_planes (include/pt_amd.h): the SVGF temporal stage as ONE kernel — demodulate by the first-hit albedo,
// reproject colour AND luminance moments through one gather, clamp the history to the 3x3 neighbourhood of this frame's colour, blend, write the
// variance — and the remodulation pass that ends the chain behind pt_filter_planes.  Stateless, every plane the caller's.
#pragma once
#include "pt_pass_dev.h"

// k_tmom: one thread per entry of the frame's pixel list, the shape of k_temporal (pt_temporal.h): the list is in 8x8-block order, so a wave
// is one block and the four-tap footprints of its lanes fall into one displaced neighbourhood.  Steps 2 to 4 are rp_gather<true>
// (pt_pass_dev.h), k_temporal's gather with the moments plane: what three pt_temporal_accumulate calls gathered three times is gathered once.
//
// CLAMP is a template parameter: the 3x3 window of demodulated colours, its up to nine colour and nine albedo loads and its six sums exist
// only in that instantiation, behind the tap loop, when the taps' registers are dead; the other one does not pay a register for it.  The
// window reads neighbours' colours, so PT_TMOM_CLEAR_COLOR is k_clear4, a second launch behind this kernel on the same stream, never a store
// in here.  No LDS (the neighbourhood depends on the motion, as in k_temporal; the window's lines are the block's own and its neighbours',
// resident in L2 in block order), no scratch.  Two counters, one atomic per wave each.
//
// Eight waves per SIMD need at most 64 VGPRs AND at most 80 SGPRs (a CU admits 800 / (sgprs rounded up to 16, + 16) blocks of 256).  The
// fourteen plane pointers and the window's nested branches took the clamp instantiation without views to 84 SGPRs, so the kernel caps them:
// amdgpu_num_sgpr(80) makes the compiler keep the overflow (14 words there, 2 with views, none without the clamp) in lanes of a VGPR.
//
// The arithmetic is the header's, in the header's order, one float32 rounding per operation (-ffp-contract=off is part of the library's
// flags): float32 NumPy evaluating it reproduces every output bit (tests/moments_ref.py).
struct TMomArgs {
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    GatherPlanes g;
    const float* color;
    const float* albedo; // or null
    float *history_out, *moments_out, *length_out;
    float* variance_out;  // or null
    const uint8_t* inset; // [nbx * nby] 1 = the block belongs to the call's set (CLAMP only)
    uint32_t nbx;
    float color_scale, albedo_min, clamp_k;
    float max_n;                // (float)(max_history - 1)
    unsigned long long* counts; // {reprojected, clamped}, zero at launch; one atomic per wave each
};

// step 0: den(q).k, one word
PT_DEV float tm_den(float a, float albedo_min) { return a > albedo_min ? a : 1.0f; } // a NaN gives 1, a miss's zero gives 1
// step 0: d(q), the demodulated colour of frame pixel q
PT_DEV v3 tm_demod(const float* color, const float* albedo, size_t q, float color_scale, float albedo_min) {
    const float4 c = tp_load4(color + 4 * q);
    v3 den = mk3(1.0f);
    if (albedo) {
        const float4 al = tp_load4(albedo + 4 * q);
        den = mk3(tm_den(al.x, albedo_min), tm_den(al.y, albedo_min), tm_den(al.z, albedo_min));
    }
    return mk3((c.x * color_scale) / den.x, (c.y * color_scale) / den.y, (c.z * color_scale) / den.z);
}

template <bool VIEWS, bool CLAMP>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) k_tmom(TMomArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool valid = false, clamped = false;
    if (i < a.n) {
        // the pixel's rectangle: its view (found by block, as k_temporal finds it) or the whole frame
        const PassPixel px = pass_pixel<VIEWS>(vp, a.pixels[i], a.g.width, a.g.height);
        const size_t p = (size_t)px.Y * (size_t)a.g.width + px.X;
        // ---------------- 0, 1. this frame: demodulated colour, luminance, moments
        const v3 d = tm_demod(a.color, a.albedo, p, a.color_scale, a.albedo_min);
        const float l = fl_lum(d.x, d.y, d.z);
        const float m1 = l, m2 = l * l;
        // ---------------- 2, 3, 4. previous position, taps, sums
        const Gather g = rp_gather<true>(a.g, px);
        valid = g.valid;
        v3 out = d;
        float mo1 = m1, mo2 = m2, len = 1.0f;
        if (valid) {
            // ---------------- 5. the reprojected history
            v3 H = mk3(g.hsum.x / g.wsum, g.hsum.y / g.wsum, g.hsum.z / g.wsum);
            const float M1 = g.msx / g.wsum, M2 = g.msy / g.wsum;
            const float n = fminf(g.nprev, a.max_n);
            const float al = 1.0f / (n + 1.0f);
            if (CLAMP) {
                // ---------------- 5b. clamp to this frame's 3x3 neighbourhood, row-major
                float cnt = 0.0f;
                v3 s1 = mk3(0.0f), s2 = mk3(0.0f);
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int qx = (int)px.X + dx, qy = (int)px.Y + dy;
                        if (!pass_reachable(px, a.inset, a.nbx, qx, qy)) continue;
                        const v3 dq = (dx | dy) == 0 ? d : tm_demod(a.color, a.albedo, (size_t)qy * (size_t)a.g.width + (size_t)qx, a.color_scale, a.albedo_min);
                        if (tp_finite(dq.x) && tp_finite(dq.y) && tp_finite(dq.z)) {
                            cnt += 1.0f;
                            s1 = mk3(s1.x + dq.x, s1.y + dq.y, s1.z + dq.z);
                            s2 = mk3(s2.x + dq.x * dq.x, s2.y + dq.y * dq.y, s2.z + dq.z * dq.z);
                        }
                    }
                if (cnt >= 1.0f) {
                    const v3 mu = mk3(s1.x / cnt, s1.y / cnt, s1.z / cnt);
                    const v3 sd = mk3(sqrtf(fl_max0(s2.x / cnt - mu.x * mu.x)), sqrtf(fl_max0(s2.y / cnt - mu.y * mu.y)), sqrtf(fl_max0(s2.z / cnt - mu.z * mu.z)));
                    const v3 e = mk3(a.clamp_k * sd.x, a.clamp_k * sd.y, a.clamp_k * sd.z);
                    const v3 lo = mk3(mu.x - e.x, mu.y - e.y, mu.z - e.z), hi = mk3(mu.x + e.x, mu.y + e.y, mu.z + e.z);
                    clamped = H.x < lo.x || H.x > hi.x || H.y < lo.y || H.y > hi.y || H.z < lo.z || H.z > hi.z;
                    H = mk3(H.x < lo.x ? lo.x : (H.x > hi.x ? hi.x : H.x), H.y < lo.y ? lo.y : (H.y > hi.y ? hi.y : H.y), H.z < lo.z ? lo.z : (H.z > hi.z ? hi.z : H.z));
                }
            }
            // ---------------- 5c. blend
            out = mk3(H.x + (d.x - H.x) * al, H.y + (d.y - H.y) * al, H.z + (d.z - H.z) * al);
            mo1 = M1 + (m1 - M1) * al;
            mo2 = M2 + (m2 - M2) * al;
            len = n + 1.0f;
        }
        // ---------------- 6. outputs
        gb_store4(a.history_out + 4 * p, make_float4(out.x, out.y, out.z, 1.0f));
        gb_store2(a.moments_out + 2 * p, make_float2(mo1, mo2));
        a.length_out[p] = len;
        if (a.variance_out) a.variance_out[p] = fl_max0(mo2 - mo1 * mo1);
    }
    pass_tally(a.counts, {valid, clamped}); // clamped: never without CLAMP
#endif
}

// PT_TMOM_CLEAR_COLOR: the four colour words of every pixel of the list become 0, behind k_tmom on the same stream
__global__ void __launch_bounds__(256) k_clear4(const uint32_t* pixels, uint32_t n, int width, float* color) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t xy = pixels[i];
    const size_t p = (size_t)pass_y(xy) * (size_t)width + pass_x(xy);
    gb_store4(color + 4 * p, make_float4(0.f, 0.f, 0.f, 0.f));
#endif
}

// pt_modulate_planes: pixel-local and streaming — 16 bytes of colour and of albedo in, 16 bytes and / or 4 bytes out per pixel.  out may be
// color itself: every pixel reads its own record before it writes it and no other.
struct ModulateArgs {
    const uint32_t* pixels;
    uint32_t n;
    int width;
    const float* color;
    const float* albedo; // or null
    float* out;          // or null
    uint32_t* frame;     // or null
    float albedo_min;
};

__global__ void __launch_bounds__(256) k_modulate(ModulateArgs a) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t xy = a.pixels[i];
    const size_t p = (size_t)pass_y(xy) * (size_t)a.width + pass_x(xy);
    const float4 c = tp_load4(a.color + 4 * p);
    v3 r = mk3(c.x, c.y, c.z); // den = 1 without an albedo plane: x * 1.0f is x
    if (a.albedo) {
        const float4 al = tp_load4(a.albedo + 4 * p);
        r = mk3(c.x * tm_den(al.x, a.albedo_min), c.y * tm_den(al.y, a.albedo_min), c.z * tm_den(al.z, a.albedo_min));
    }
    if (a.out) gb_store4(a.out + 4 * p, make_float4(r.x, r.y, r.z, c.w));
    if (a.frame) a.frame[p] = make_color(r);
#endif
}
