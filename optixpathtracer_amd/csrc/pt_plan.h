// pt_sample_plan and pt_temporal_carry (include/pt_amd.h): adaptive sampling inside the reprojection chain.  The plan decides, before a frame
// is rendered, which 8x8 blocks need new samples — where the history was lost, where it is short, where the reprojected luminance moments say
// the estimate is still noisy (the stopping rule of pt_render_adaptive with the history length in place of the subframe count) —; the carry is
// the temporal stage of the blocks that were NOT rendered: it moves their history, moments and length along the motion plane unchanged, so
// that the ping-pong of the chain stays whole.  Both are stateless; every plane is the caller's; neither reads a colour plane.
#pragma once
#include "pt_pass_dev.h"

// Both kernels gather through rp_gather<true> (pt_pass_dev.h): pt_temporal_moments's steps 2, 3 and 4, the text k_tmom runs.  The plan never
// uses hsum: inlined there, the three products and sums per tap are dead and go; the history's loads stay, for the finite test.

// k_plan: one wave per 8x8 block of the frame's block table, the shape of k_adapt_decide: lane l stands for the pixel (8 bx + (l & 7),
// 8 by + (l >> 3)); lanes outside the image or outside the block's view are idle.  A block outside the call's set gets a 0 and nothing else.
// L and S are popcounts of ballots: integers, so no order of lanes or waves can show in the result.  One lane writes the block's byte
// (every byte of the table is written by exactly one wave) and adds the wave's non-zero counts, one atomic each.  No LDS, no scratch.
struct PlanArgs {
    GatherPlanes pl;
    const uint8_t* inset; // [nblk] 1 = the block belongs to the call's set (owned by the rank, named by the mask)
    uint8_t* out;         // [nblk] 1 = sample the block
    uint32_t nblk, nbx;
    float t2;         // threshold * threshold
    float dark_floor;
    float min_length; // as a float: exact, the range ends at 65535
    uint32_t min_pixels;
    uint32_t refresh_period, frame_mod; // frame_index % refresh_period (0 with no period)
    unsigned long long* counts;         // PLAN_* below, zero at launch
};
enum { PLAN_SAMPLED = 0, PLAN_BY_LOST, PLAN_BY_NEED, PLAN_BY_REFRESH, PLAN_PIXELS, PLAN_LOST, PLAN_NEEDY, PLAN_COUNTERS };

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_plan(PlanArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (b >= a.nblk) return;
    if (a.inset[b] == 0) {
        if (lane == 0u) a.out[b] = 0;
        return;
    }
    const uint32_t bx = b % a.nbx, by = b / a.nbx;
    const uint32_t X = bx * 8u + (lane & 7u), Y = by * 8u + (lane >> 3);
    const PassPixel px = pass_pixel_at<VIEWS>(vp, X, Y, a.pl.width, a.pl.height); // a block of the set has view pixels: its view is never 0xffff
    const bool inside = (int)X >= px.x0 && (int)X < px.x0 + px.wr && (int)Y >= px.y0 && (int)Y < px.y0 + px.hr && X < (uint32_t)a.pl.width && Y < (uint32_t)a.pl.height;
    bool lost = false, needy = false;
    if (inside) {
        const Gather g = rp_gather<true>(a.pl, px);
        lost = !g.valid;
        if (g.valid) {
            needy = g.nprev < a.min_length; // short
            if (!needy) {
                const float M1 = g.msx / g.wsum, M2 = g.msy / g.wsum;
                const float var = fl_max0(M2 - M1 * M1);
                const float B = M1 + a.dark_floor;
                float rhs = a.t2 * g.nprev;
                rhs = rhs * B;
                rhs = rhs * B;
                needy = !(var <= rhs); // noisy; a NaN on either side is noisy
            }
        }
    }
    const uint32_t P = (uint32_t)__popcll(__ballot(inside)), L = (uint32_t)__popcll(__ballot(lost)), S = (uint32_t)__popcll(__ballot(needy));
    if (lane != 0u) return;
    // ((uint64)bx + 3 * (uint64)by + frame_index) % period: both summands are reduced first, so 32 bits hold every intermediate
    const bool refresh = a.refresh_period > 0u && ((bx + 3u * by) % a.refresh_period + a.frame_mod) % a.refresh_period == 0u;
    const bool by_lost = L >= 1u, by_need = !by_lost && S >= a.min_pixels;
    const bool sampled = by_lost || by_need || refresh;
    a.out[b] = sampled ? 1 : 0;
    if (sampled) atomicAdd(a.counts + PLAN_SAMPLED, 1ull);
    if (by_lost) atomicAdd(a.counts + PLAN_BY_LOST, 1ull);
    if (by_need) atomicAdd(a.counts + PLAN_BY_NEED, 1ull);
    if (sampled && !by_lost && !by_need) atomicAdd(a.counts + PLAN_BY_REFRESH, 1ull);
    atomicAdd(a.counts + PLAN_PIXELS, (unsigned long long)P);
    if (L) atomicAdd(a.counts + PLAN_LOST, (unsigned long long)L);
    if (S) atomicAdd(a.counts + PLAN_NEEDY, (unsigned long long)S);
#endif
}

// k_carry: one thread per entry of the call's pixel list, the shape of k_tmom without its colour, clamp and blend parts: the gather, two
// divisions per word, the stores.  A pixel without a valid gather gets the record nothing downstream takes for a history: three NaN colour
// words (pt_filter_planes leaves such a pixel alone and takes it as no tap; the next frame's gather rejects it) and length 0.
struct CarryArgs {
    GatherPlanes pl;
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    float *history_out, *moments_out, *length_out;
    float* variance_out;        // or null
    unsigned long long* counts; // {carried}, zero at launch; one atomic per wave
};

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_carry(CarryArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool valid = false;
    if (i < a.n) {
        const PassPixel px = pass_pixel<VIEWS>(vp, a.pixels[i], a.pl.width, a.pl.height);
        const Gather g = rp_gather<true>(a.pl, px);
        valid = g.valid;
        const size_t p = (size_t)px.Y * (size_t)a.pl.width + px.X;
        const float nan = __int_as_float(0x7fc00000);
        float4 h = make_float4(nan, nan, nan, 1.0f);
        float2 m = make_float2(0.0f, 0.0f);
        float len = 0.0f, var = 0.0f;
        if (valid) {
            h = make_float4(g.hsum.x / g.wsum, g.hsum.y / g.wsum, g.hsum.z / g.wsum, 1.0f);
            m = make_float2(g.msx / g.wsum, g.msy / g.wsum);
            len = g.nprev;
            var = fl_max0(m.y - m.x * m.x);
        }
        gb_store4(a.history_out + 4 * p, h);
        gb_store2(a.moments_out + 2 * p, m);
        a.length_out[p] = len;
        if (a.variance_out) a.variance_out[p] = var;
    }
    pass_tally(a.counts, {valid});
#endif
}
