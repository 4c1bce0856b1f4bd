// pt_dof_layout and pt_dof_planes (include/pt_amd.h): a thin lens behind the pinhole frame path, as a post pass over colour and depth.
// Motion blur's family with a disc for the line.  Three kernels: k_dof_tile reduces every 16 x 16 tile of every rectangle to its largest
// blur radius (T), k_tile_neighbour<float> takes the largest T of the 3 x 3 tiles around each tile (N), k_dof_gather<VIEWS> runs over the
// call's pixel list and gathers `taps` pixels of a disc of radius N.  T and N are planes of floats in the caller's scratch; the view table
// (TileView, one per rectangle, aux = the view's focus distance) and the tap table (DofTaps) are temporaries of the call in device memory.
//
// The view table, a tile kernel's pixels, the neighbour kernel, the tap's address, the counters' way out, Z(depth), the hash and the
// clamp are the tiled passes' scaffold in pt_pass_dev.h, shared with motion blur.  What stands here is depth of field's own: the radius
// rule, the tile's reduction, the disc's taps and their weights.
#pragma once
#include "pt_pass_dev.h"

// The host's table of a call: the spiral's directions D[0 .. 127] by the header's recurrence, and rho[i] = sqrtf((i + 0.5f) / taps).  Both
// are the header's operations, done once on the host (built with -ffp-contract=off like the device code) instead of per lane and tap.
struct DofTaps {
    float2 D[128];
    float rho[64];
};

struct DofParams {
    float K, R; // aperture + 0.0f, max_radius
};

#define DOF_PI 3.14159274f

// Step 1 of the header, from Z(depth)
PT_DEV float dof_radius(float z, float focus, const DofParams& k) {
    const float r = k.K * fabsf(1.0f - focus / z);
    return r < k.R ? r : k.R;
}
PT_DEV float dof_area(float r) {
    const float a = (r * r) * DOF_PI;
    return a > 1.0f ? a : 1.0f;
}

// ------------------------------------------------------------------ k_dof_tile: T, the largest blur radius of each tile
// k_mblur_tile's shape as it was measured: one WAVE per tile, four tiles to a workgroup of 256 threads; a lane's four pixels (tile_pixel)
// are four 4-byte loads that are all in flight before the first is used.  r >= 0 is never NaN, so the maximum does not depend on the order
// of the reduction and needs no key: a pixel outside the rectangle (a partial tile) contributes 0, six shuffle steps take the maximum
// across the wave, and lane 0 writes it (pixel 0 of a tile is always inside).  No LDS, no barrier.  sources is added up in a scalar
// register from ballots and leaves through pass_slot with one atomic per wave.
struct DofTileArgs {
    const TileView* tab;
    int width; // of the frame: the planes are indexed Y * width + X
    const float* depth;
    float* scratch;
    DofParams k;
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] sources ([1] gathered, [2] taps, [3] nonfinite: k_dof_gather)
};
#define DOF_TILES_PER_BLOCK 4u

__global__ void __launch_bounds__(256) k_dof_tile(DofTileArgs a) {
#if __HIP_DEVICE_COMPILE__
    const TileView L = a.tab[blockIdx.y];
    const uint32_t tile = blockIdx.x * DOF_TILES_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= L.tw * L.th) return; // the whole wave; the kernel has no barrier
    float d[4];
    bool in[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const TilePixel t = tile_pixel(L, a.width, tile, lane, k);
        in[k] = t.in;
        d[k] = a.depth[t.p];
    }
    float best = 0.0f;
    uint32_t nin = 0u; // wave-uniform
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const float r = in[k] ? dof_radius(pass_depth(d[k]), L.aux, a.k) : 0.0f;
        best = r > best ? r : best;
        nin += (uint32_t)__popcll(__ballot(in[k]));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if (lane == 0u) {
        atomicAdd(pass_slot(a.counts) + 0, (unsigned long long)nin); // (nin >= 1: pixel 0 of a tile is inside)
        a.scratch[(size_t)L.offT + tile] = best;
    }
#endif
}

// ------------------------------------------------------------------ k_dof_gather: step 4, over the call's pixel list
// k_mblur_gather's shape: one thread per entry of the pixel list.  rN is uniform over a tile, so where the list hands a wave one 8 x 8
// block the early exit, d and (without jitter) the tap's offset are the same in every lane.  A tap loads the depth (4 bytes) first; the
// colour (16 bytes) is loaded only where the weight is positive, which the rule allows: a tap outside its own blur circle never looks at
// its colour.  (Issuing both loads together in front of the first use gives the same bits and, measured, the same time within the spread
// of the runs: profiles/dof.md.  The branch stays: it saves the 16 bytes wherever a tap does not count.)  The three counters leave through
// pass_tally_sums; every lane reaches it.
struct DofGatherArgs {
    const uint32_t* pixels;
    uint32_t n;
    int width, height;
    const float *color, *depth;
    float* out;
    const TileView* tab;
    const DofTaps* tt;
    const float* scratch;
    DofParams k;
    uint32_t taps, seed, jitter;
    unsigned long long* counts;
};

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_dof_gather(DofGatherArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t ngathered = 0u, ntaps = 0u, nnonfinite = 0u;
    if (i < a.n) {
        const PassPixel px = pass_pixel<VIEWS>(vp, a.pixels[i], a.width, a.height);
        const size_t p = (size_t)px.Y * (size_t)a.width + px.X;
        const int x = (int)px.X - px.x0, y = (int)px.Y - px.y0;
        const TileView L = a.tab[px.view];
        const float4 c = tp_load4(a.color + 4 * p);
        const float rN = a.scratch[(size_t)L.offN + (size_t)(y >> 4) * L.tw + (size_t)(x >> 4)];
        v3 o = mk3(c.x, c.y, c.z);
        if (rN > 0.5f && tp_finite(c.x) && tp_finite(c.y) && tp_finite(c.z)) {
            ngathered = 1u;
            const float zp = pass_depth(a.depth[p]);
            const float rp = dof_radius(zp, L.aux, a.k);
            const float wp = 1.0f / dof_area(rp);
            const float At = ((rN * rN) * DOF_PI) / (float)a.taps;
            const uint32_t k0 = a.jitter ? pass_hash((uint32_t)x, (uint32_t)y, a.seed) & 63u : 0u;
            const float fx = (float)x, fy = (float)y;
            v3 sum = mk3(0.0f);
            float Wt = 0.0f;
            for (uint32_t k = 0; k < a.taps; ++k) {
                const float d = rN * a.tt->rho[k];
                const float2 D = a.tt->D[k + k0];
                const size_t q = pass_tap(px, a.width, fx + d * D.x, fy + d * D.y);
                const float dq = a.depth[q];
                const float zq = pass_depth(dq);
                const float rq = dof_radius(zq, L.aux, a.k);
                const float re = zq > zp ? rp : rq;
                const float cov = pass_clamp01((re - d) + 0.5f);
                const float w = (cov * At) / dof_area(re);
                if (!(w > 0.0f)) continue;
                const float4 cq = tp_load4(a.color + 4 * q);
                if (!(tp_finite(cq.x) && tp_finite(cq.y) && tp_finite(cq.z))) {
                    ++nnonfinite;
                    continue;
                }
                sum = mk3(sum.x + cq.x * w, sum.y + cq.y * w, sum.z + cq.z * w);
                Wt = Wt + w;
                ++ntaps;
            }
            if (!(Wt == 0.0f)) {
                const float den = wp + Wt;
                o = mk3((c.x * wp + sum.x) / den, (c.y * wp + sum.y) / den, (c.z * wp + sum.z) / den);
            }
        }
        gb_store4(a.out + 4 * p, make_float4(o.x, o.y, o.z, 1.0f));
    }
    const uint32_t counted[3] = {ngathered, ntaps, nnonfinite};
    pass_tally_sums(a.counts, 1u, counted); // words 1 .. 3
#endif
}
