// pt_temporal_accumulate (include/pt_amd.h): reproject last frame's accumulated colour along the G-buffer's motion plane, check that it is the
// same surface, blend with a per-pixel history length — ONE kernel, stateless, every plane the caller's.
#pragma once
#include "pt_pass_dev.h"

// One thread per entry of the frame's pixel list.  The list is in 8x8-block order, so a wave is one block and its four-tap footprints fall
// into one displaced neighbourhood of about 9x9 pixels: the taps of neighbouring lanes share cache lines, which is what brings the 368 bytes
// a pixel touches at worst down to about 164 bytes of unique traffic.  No LDS: the neighbourhood depends on the motion, so a tile would
// have to be gathered through the same addresses first.
//
// The arithmetic is the header's, in the header's order, one float32 rounding per operation (-ffp-contract=off is part of the library's
// flags): float32 NumPy evaluating it reproduces every output bit (tests/temporal_ref.py).  Steps 2 to 4 are rp_gather<false> (pt_pass_dev.h),
// the gather k_tmom, k_plan and k_carry share, without the moments plane.  Records move as 16-byte loads and stores at whatever
// 4-byte-aligned address the plane has (gb_store4, tp_load4).
struct TemporalArgs {
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    GatherPlanes g; // moments_in is null
    float* color;
    float *history_out, *length_out;
    uint32_t* frame; // or null
    float* copy_out; // or null
    float color_scale;
    float max_n;    // (float)(max_history - 1)
    uint32_t clear; // PT_TEMPORAL_CLEAR_COLOR
    unsigned long long* reprojected; // zero at launch; one atomic per wave
};

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_temporal(TemporalArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool valid = false;
    if (i < a.n) {
        // the pixel's rectangle: its view (found by block, as k_gbuffer<true> finds it) or the whole frame
        const PassPixel px = pass_pixel<VIEWS>(vp, a.pixels[i], a.g.width, a.g.height);
        const size_t p = (size_t)px.Y * (size_t)a.g.width + px.X;
        // ---------------- 1. colour
        const float4 c4 = tp_load4(a.color + 4 * p);
        const v3 c = mk3(c4.x * a.color_scale, c4.y * a.color_scale, c4.z * a.color_scale);
        if (a.clear) gb_store4(a.color + 4 * p, make_float4(0.f, 0.f, 0.f, 0.f));
        // ---------------- 2, 3, 4. previous position, taps, sums
        const Gather g = rp_gather<false>(a.g, px);
        valid = g.valid;
        // ---------------- 5. blend
        v3 out = c;
        float len = 1.0f;
        if (valid) {
            const v3 H = mk3(g.hsum.x / g.wsum, g.hsum.y / g.wsum, g.hsum.z / g.wsum);
            const float n = fminf(g.nprev, a.max_n);
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
    pass_tally(a.reprojected, {valid});
#endif
}
