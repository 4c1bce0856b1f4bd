// pt_temporal_accumulate (include/pt_amd.h): reproject last frame's accumulated colour along the G-buffer's motion plane, check that it is the
// same surface, blend with a per-pixel history length — ONE kernel, stateless, every plane the caller's.
#pragma once
#include "pt_gbuffer.h"

// One thread per entry of the frame's pixel list.  The list is in 8x8-block order, so a wave is one block and its four-tap footprints fall
// into one displaced neighbourhood of about 9x9 pixels: the taps of neighbouring lanes share cache lines, which is what brings the 368 bytes
// a pixel touches at worst down to about 164 bytes of unique traffic.  No LDS: the neighbourhood depends on the motion, so a tile would
// have to be gathered through the same addresses first.
//
// The arithmetic is the header's, in the header's order, one float32 rounding per operation (-ffp-contract=off is part of the library's
// flags): float32 NumPy evaluating it reproduces every output bit (tests/temporal_ref.py).  A tap is read cheapest word first — the history
// length (4 bytes), then the previous hit record's mesh and normal (16 bytes; the primitive word alone under a miss), and only for a tap
// that is still alive prev_position and history_in (16 bytes each).  Records move as 16-byte loads and stores at whatever 4-byte-aligned
// address the plane has (gb_store4 of pt_gbuffer.h, and its mirror for loads).
struct TemporalArgs {
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    int width, height; // the frame: the planes are indexed Y * width + X
    float* color;
    const float *motion, *hit, *position, *prev_hit, *prev_position, *history_in, *length_in;
    float *history_out, *length_out;
    uint32_t* frame; // or null
    float* copy_out; // or null
    float color_scale, normal_cos, plane_eps, min_weight;
    float max_n;    // (float)(max_history - 1)
    uint32_t clear; // PT_TEMPORAL_CLEAR_COLOR
    unsigned long long* reprojected; // zero at launch; one atomic per wave
};

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

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_temporal(TemporalArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool valid = false;
    if (i < a.n) {
        const uint32_t xy = a.pixels[i];
        const uint32_t X = xy & 0xffffu, Y = xy >> 16;
        // the pixel's rectangle: its view (found by block, as k_gbuffer<true> finds it) or the whole frame
        int x0 = 0, y0 = 0, wr = a.width, hr = a.height;
        if (VIEWS) {
            const uint32_t vi = vp.vblock[(Y >> 3) * vp.nbx + (X >> 3)]; // the list holds view pixels only: never 0xffff
            x0 = vp.views[vi].x;
            y0 = vp.views[vi].y;
            wr = vp.views[vi].width;
            hr = vp.views[vi].height;
        }
        const int x = (int)X - x0, y = (int)Y - y0;
        const size_t p = (size_t)Y * (size_t)a.width + X;
        // ---------------- 1. colour
        const float4 c4 = tp_load4(a.color + 4 * p);
        const v3 c = mk3(c4.x * a.color_scale, c4.y * a.color_scale, c4.z * a.color_scale);
        if (a.clear) gb_store4(a.color + 4 * p, make_float4(0.f, 0.f, 0.f, 0.f));
        // ---------------- 2. previous position
        const float2 mv = tp_load2(a.motion + 2 * p);
        const float px = (float)x + mv.x, py = (float)y + mv.y;
        float wsum = 0.0f, nprev = 0.0f;
        v3 hsum = mk3(0.0f);
        bool any = false;
        if (px >= -1.0f && px <= (float)wr && py >= -1.0f && py <= (float)hr) { // a NaN fails
            const float flx = floorf(px), fly = floorf(py);
            const int ix = (int)flx, iy = (int)fly;
            const float fx = px - flx, fy = py - fly;
            const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
            const float4 ha = tp_load4(a.hit + 8 * p), hb = tp_load4(a.hit + 8 * p + 4); // t, u, v, prim | mesh, ng.xyz
            const float4 P = tp_load4(a.position + 4 * p);
            const bool miss = __float_as_int(ha.w) < 0;
            const v3 ng = mk3(hb.y, hb.z, hb.w);
            const float plane_max = a.plane_eps * ha.x;
            float wt[4];
            v3 ht[4];
            // ---------------- 3. which taps count; order (0,0), (1,0), (0,1), (1,1)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ti = k & 1, tj = k >> 1;
                const int tx = ix + ti, ty = iy + tj;
                const float w = wx[ti] * wy[tj];
                wt[k] = 0.0f;
                ht[k] = mk3(0.0f);
                if (tx >= 0 && tx < wr && ty >= 0 && ty < hr && w > 0.0f) {
                    const size_t q = (size_t)(y0 + ty) * (size_t)a.width + (size_t)(x0 + tx);
                    const float len = a.length_in[q];
                    if (len >= 1.0f) {
                        bool alive;
                        if (miss) {
                            alive = __float_as_int(a.prev_hit[8 * q + 3]) < 0;
                        } else {
                            const float4 qb = tp_load4(a.prev_hit + 8 * q + 4);
                            alive = __float_as_int(qb.x) == __float_as_int(hb.x) && dot3(ng, mk3(qb.y, qb.z, qb.w)) >= a.normal_cos;
                            if (alive) {
                                const float4 Q = tp_load4(a.prev_position + 4 * q);
                                alive = fabsf(dot3(ng, mk3(Q.x - P.x, Q.y - P.y, Q.z - P.z))) <= plane_max;
                            }
                        }
                        if (alive) {
                            const float4 hq = tp_load4(a.history_in + 4 * q);
                            if (tp_finite(hq.x) && tp_finite(hq.y) && tp_finite(hq.z)) {
                                wt[k] = w;
                                ht[k] = mk3(w * hq.x, w * hq.y, w * hq.z);
                                nprev = any ? fminf(nprev, len) : len;
                                any = true;
                            }
                        }
                    }
                }
            }
            // ---------------- 4. sums, in tap order
            wsum = ((wt[0] + wt[1]) + wt[2]) + wt[3];
            hsum = mk3(((ht[0].x + ht[1].x) + ht[2].x) + ht[3].x, ((ht[0].y + ht[1].y) + ht[2].y) + ht[3].y, ((ht[0].z + ht[1].z) + ht[2].z) + ht[3].z);
        }
        valid = any && wsum >= a.min_weight;
        // ---------------- 5. blend
        v3 out = c;
        float len = 1.0f;
        if (valid) {
            const v3 H = mk3(hsum.x / wsum, hsum.y / wsum, hsum.z / wsum);
            const float n = fminf(nprev, a.max_n);
            const float al = 1.0f / (n + 1.0f);
            out = lerp3(H, c, al);
            len = n + 1.0f;
        }
        // ---------------- 6. outputs
        const float4 o4 = make_float4(out.x, out.y, out.z, 1.0f);
        gb_store4(a.history_out + 4 * p, o4);
        a.length_out[p] = len;
        if (a.frame) a.frame[p] = make_color(out);
        if (a.copy_out) gb_store4(a.copy_out + 4 * p, o4);
    }
    const unsigned long long vm = __ballot(valid);
    if ((threadIdx.x & 63u) == 0u && vm) atomicAdd(a.reprojected, (unsigned long long)__popcll(vm));
#endif
}
