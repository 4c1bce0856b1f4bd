// pt_sample_plan and pt_temporal_carry (include/pt_amd.h): adaptive sampling inside the reprojection chain.  The plan decides, before a frame
// is rendered, which 8x8 blocks need new samples — where the history was lost, where it is short, where the reprojected luminance moments say
// the estimate is still noisy (the stopping rule of pt_render_adaptive with the history length in place of the subframe count) —; the carry is
// the temporal stage of the blocks that were NOT rendered: it moves their history, moments and length along the motion plane unchanged, so
// that the ping-pong of the chain stays whole.  Both are stateless; every plane is the caller's; neither reads a colour plane.
#pragma once
#include "pt_filter.h"

// The eight read-only planes both kernels gather from, and the three parameters of the gather.
struct PlanPlanes {
    const float *motion, *hit, *position, *prev_hit, *prev_position, *history_in, *moments_in, *length_in;
    int width, height; // the frame: the planes are indexed Y * width + X
    float normal_cos, plane_eps, min_weight;
};

// What step G leaves for a pixel: the sums in tap order, the minimum history length of the counting taps, and valid.
struct PlanGather {
    float wsum, nprev, msx, msy;
    v3 hsum;
    bool valid;
};

// Step G: pt_temporal_moments's steps 2, 3 and 4 (k_tmom's tap loop, restated once more: k_tmom and k_temporal keep their own text, so their
// listings do not move).  Frame pixel (X, Y) inside the rectangle (x0, y0, wr, hr).  A tap is read cheapest word first: the history length
// (4 bytes), the previous hit record's mesh and normal (16 bytes; the primitive word alone under a miss), prev_position (16 bytes), and only
// a tap that survived the geometry tests loads its moments (8 bytes) and its history (16 bytes).  The plan never uses hsum: inlined there,
// the three products and sums per tap are dead and go; the history's loads stay, for the finite test.
PT_DEV PlanGather pl_gather(const PlanPlanes& a, uint32_t X, uint32_t Y, int x0, int y0, int wr, int hr) {
    const int x = (int)X - x0, y = (int)Y - y0;
    const size_t p = (size_t)Y * (size_t)a.width + X;
    // ---------------- 2. previous position
    const float2 mv = tp_load2(a.motion + 2 * p);
    const float px = (float)x + mv.x, py = (float)y + mv.y;
    PlanGather g;
    g.wsum = 0.0f;
    g.nprev = 0.0f;
    g.msx = 0.0f;
    g.msy = 0.0f;
    g.hsum = mk3(0.0f);
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
        float wt[4], mx[4], my[4];
        v3 ht[4];
        // ---------------- 3. which taps count; order (0,0), (1,0), (0,1), (1,1)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ti = k & 1, tj = k >> 1;
            const int tx = ix + ti, ty = iy + tj;
            const float w = wx[ti] * wy[tj];
            wt[k] = 0.0f;
            mx[k] = 0.0f;
            my[k] = 0.0f;
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
                        const float2 mq = tp_load2(a.moments_in + 2 * q);
                        const float4 hq = tp_load4(a.history_in + 4 * q);
                        if (tp_finite(hq.x) && tp_finite(hq.y) && tp_finite(hq.z) && tp_finite(mq.x) && tp_finite(mq.y)) {
                            wt[k] = w;
                            ht[k] = mk3(w * hq.x, w * hq.y, w * hq.z);
                            mx[k] = w * mq.x;
                            my[k] = w * mq.y;
                            g.nprev = any ? fminf(g.nprev, len) : len;
                            any = true;
                        }
                    }
                }
            }
        }
        // ---------------- 4. sums, in tap order
        g.wsum = ((wt[0] + wt[1]) + wt[2]) + wt[3];
        g.hsum = mk3(((ht[0].x + ht[1].x) + ht[2].x) + ht[3].x, ((ht[0].y + ht[1].y) + ht[2].y) + ht[3].y, ((ht[0].z + ht[1].z) + ht[2].z) + ht[3].z);
        g.msx = ((mx[0] + mx[1]) + mx[2]) + mx[3];
        g.msy = ((my[0] + my[1]) + my[2]) + my[3];
    }
    g.valid = any && g.wsum >= a.min_weight;
    return g;
}

// k_plan: one wave per 8x8 block of the frame's block table, the shape of k_adapt_decide: lane l stands for the pixel (8 bx + (l & 7),
// 8 by + (l >> 3)); lanes outside the image or outside the block's view are idle.  A block outside the call's set gets a 0 and nothing else.
// L and S are popcounts of ballots: integers, so no order of lanes or waves can show in the result.  One lane writes the block's byte
// (every byte of the table is written by exactly one wave) and adds the wave's non-zero counts, one atomic each.  No LDS, no scratch.
struct PlanArgs {
    PlanPlanes pl;
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
    int x0 = 0, y0 = 0, wr = a.pl.width, hr = a.pl.height;
    if (VIEWS) {
        const uint32_t vi = vp.vblock[b]; // a block of the set has view pixels: never 0xffff
        x0 = vp.views[vi].x;
        y0 = vp.views[vi].y;
        wr = vp.views[vi].width;
        hr = vp.views[vi].height;
    }
    const bool inside = (int)X >= x0 && (int)X < x0 + wr && (int)Y >= y0 && (int)Y < y0 + hr && X < (uint32_t)a.pl.width && Y < (uint32_t)a.pl.height;
    bool lost = false, needy = false;
    if (inside) {
        const PlanGather g = pl_gather(a.pl, X, Y, x0, y0, wr, hr);
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
    PlanPlanes pl;
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
        const uint32_t xy = a.pixels[i];
        const uint32_t X = xy & 0xffffu, Y = xy >> 16;
        int x0 = 0, y0 = 0, wr = a.pl.width, hr = a.pl.height;
        if (VIEWS) {
            const uint32_t vi = vp.vblock[(Y >> 3) * vp.nbx + (X >> 3)]; // the list holds view pixels only: never 0xffff
            x0 = vp.views[vi].x;
            y0 = vp.views[vi].y;
            wr = vp.views[vi].width;
            hr = vp.views[vi].height;
        }
        const PlanGather g = pl_gather(a.pl, X, Y, x0, y0, wr, hr);
        valid = g.valid;
        const size_t p = (size_t)Y * (size_t)a.pl.width + X;
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
    const unsigned long long vm = __ballot(valid);
    if ((threadIdx.x & 63u) == 0u && vm) atomicAdd(a.counts, (unsigned long long)__popcll(vm));
#endif
}
