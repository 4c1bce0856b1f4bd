// pt_exposure_planes and pt_tonemap_planes (include/pt_amd.h): the end of the chain after the end of the chain — a per-view histogram of
// log2 luminance (k_meter), an exposure adapted from it in integers (k_adapt), and the display operator under that exposure (k_tonemap).
// The exposure goes from k_adapt to k_tonemap through the caller's state words in device memory.
#pragma once
#include "pt_pass_dev.h"

#define EXPO_BINS 256u
#define EXPO_UNROLL 4u                      // pixels per thread and step: four independent 16-byte loads in flight
#define EXPO_TILE (256u * EXPO_UNROLL)      // entries of the pixel list per workgroup and step

// k_meter is the first reduction of the chain.  Counting into the histogram words directly would put every pixel's atomic onto a handful
// of words (a frame's luminances fill a few dozen bins, and its black pixels one): the figure of pass_tally's comment, 10 ns an atomic onto
// one word, prices that.  So: a BOUNDED grid (the host sizes it from the CU count), each workgroup walking a CONTIGUOUS run of tiles of
// the pixel list, each of its four waves counting into a privatised histogram of its own, 256 words in LDS.  At its end the workgroup adds
// its four copies up and flushes once: one integer atomicAdd per NON-ZERO bin (thread b owns bin b).  Contiguous runs, not a grid stride:
// the list is in block-raster order, so under views a strided workgroup would meet another view at almost every step.
//
// Views: the choice is FLUSH ON A VIEW CHANGE, per wave.  A wave's copy serves ONE view, `cur`.  Of a tile a wave takes 256 consecutive
// entries, 64 at a step: one 8x8 block where the blocks are whole, so a step's pixels nearly always share a view.  A step's counted lanes
// are served view by view: those of the first pending lane's view count into LDS — after the wave has flushed its copy and moved `cur`, if
// that view is another — until none is pending.  Nothing goes to global memory except through a flush, which costs four LDS reads a lane
// and one atomic per non-zero bin, and no barrier: a wave's LDS operations complete in order.  (Sending such stragglers straight to global
// memory was tried first: with the 69 000 pixels beside the seam of two side-by-side 1080p views, four in ten of them black and so on
// the one word of bin 0, the call took 0.59 ms.)  No LDS is needed per view.  When the four waves end on one view (always, without
// views) the last flush is the merged one; otherwise each wave flushes its own.
//
// A step whose counted lanes all have the same bin (a flat region; the constant plane is the extreme) adds their count with ONE LDS
// atomic instead of up to 64 onto one word.  Integer adds commute, so none of this changes the result.
struct MeterArgs {
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    uint32_t tiles_per_group; // tiles of EXPO_TILE entries each workgroup walks
    int width, height;
    const float* color;
    const float* hit;       // or null
    uint32_t* hist;         // [views][256]
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] skipped, [1] nonfinite, [2] under, [3] over
};

// step 3 of the header: the bin of a luminance, from its bit pattern
PT_DEV uint32_t expo_bin(float Y) {
    if (!(Y > 0.0f)) return 0u;
    if (!tp_finite(Y)) return 255u;
    const int k = (int)(__float_as_uint(Y) >> 20) - 887;
    return k < 1 ? 0u : k > 254 ? 255u : (uint32_t)k;
}

// one wave's copy into its view's histogram, and cleared; every lane of the wave
PT_DEV void expo_wave_flush(uint32_t* s_wave, uint32_t* hist, uint32_t view) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t b = lane + 64u * k, v = s_wave[b];
        if (v) atomicAdd(hist + (size_t)view * EXPO_BINS + b, v);
        s_wave[b] = 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_meter(MeterArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    __shared__ uint32_t s_hist[4][EXPO_BINS];
    __shared__ uint32_t s_cur[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t* s_wave = s_hist[wave];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) s_hist[k][threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t ntiles = (a.n + EXPO_TILE - 1u) / EXPO_TILE;
    const uint32_t t0 = blockIdx.x * a.tiles_per_group;
    const uint32_t t1 = t0 + a.tiles_per_group < ntiles ? t0 + a.tiles_per_group : ntiles;
    uint32_t cur = 0u; // wave-uniform
    bool first = true;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const uint32_t base = tile * EXPO_TILE + wave * (64u * EXPO_UNROLL) + lane; // a wave: 256 consecutive entries, 64 at a step
        uint32_t xy[EXPO_UNROLL], view[EXPO_UNROLL];
        size_t pi[EXPO_UNROLL];
        float4 c[EXPO_UNROLL];
        int32_t prim[EXPO_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < EXPO_UNROLL; ++u) {
            const uint32_t i = base + 64u * u;
            xy[u] = i < a.n ? a.pixels[i] : 0u; // past the list's end: entry (0, 0), a pixel of the frame, loaded and dropped
        }
#pragma unroll
        for (uint32_t u = 0; u < EXPO_UNROLL; ++u) {
            view[u] = VIEWS ? vp.vblock[(pass_y(xy[u]) >> 3) * vp.nbx + (pass_x(xy[u]) >> 3)] : 0u;
            pi[u] = (size_t)pass_y(xy[u]) * (size_t)a.width + pass_x(xy[u]);
            c[u] = tp_load4(a.color + 4 * pi[u]);
            prim[u] = a.hit ? __float_as_int(a.hit[8 * pi[u] + 3]) : 0;
        }
#pragma unroll
        for (uint32_t u = 0; u < EXPO_UNROLL; ++u) {
            const bool in = base + 64u * u < a.n;
            const bool skipped = in && prim[u] < 0;
            const bool nonfinite = in && !skipped && !(tp_finite(c[u].x) && tp_finite(c[u].y) && tp_finite(c[u].z));
            const bool counted = in && !skipped && !nonfinite;
            const uint32_t bin = expo_bin(fl_lum(c[u].x, c[u].y, c[u].z));
            bool pending = counted;
            unsigned long long left = __ballot(pending);
            while (left) { // once, except where views meet inside the step
                const int lead = __ffsll((long long)left) - 1;
                bool mine = pending;
                if (VIEWS) {
                    const uint32_t v = __shfl(view[u], lead);
                    if (first) cur = v;
                    if (v != cur) {
                        expo_wave_flush(s_wave, a.hist, cur);
                        cur = v;
                    }
                    mine = pending && view[u] == v;
                }
                first = false;
                const unsigned long long m = __ballot(mine);
                const uint32_t b0 = __shfl(bin, lead);
                if (__ballot(mine && bin == b0) == m) {
                    if (lane == 0u) atomicAdd(s_wave + b0, (uint32_t)__popcll(m));
                } else if (mine) {
                    atomicAdd(s_wave + bin, 1u);
                }
                pending = pending && !mine;
                left = __ballot(pending);
            }
            pass_tally(pass_slot(a.counts), {skipped, nonfinite, counted && bin == 0u, counted && bin == 255u});
        }
    }
    if (lane == 0u) s_cur[wave] = first ? 0xffffffffu : cur; // a wave that counted nothing has an empty copy: any view serves
    __syncthreads();
    uint32_t common = 0xffffffffu;
    bool same = true;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t v = s_cur[k];
        if (v != 0xffffffffu) {
            same = same && (common == 0xffffffffu || common == v);
            common = v;
        }
    }
    if (same) {
        const uint32_t v = ((s_hist[0][threadIdx.x] + s_hist[1][threadIdx.x]) + s_hist[2][threadIdx.x]) + s_hist[3][threadIdx.x];
        if (v) atomicAdd(a.hist + (size_t)common * EXPO_BINS + threadIdx.x, v); // v != 0 implies some wave counted: common is a view
    } else if (!first) {
        expo_wave_flush(s_wave, a.hist, cur);
    }
#endif
}

// The adaptation: one wave per view.  Lane l holds bins 4l .. 4l + 3 as uint64; the two trims are prefix sums (what the walk up from bin
// 0 has left of `lo` when it reaches bin i is max(0, lo - sum of c[j < i]), and likewise down from bin 255 on what the first trim left), so
// the whole of it is two wave scans and two wave sums, integer, equal to the serial walk word for word.  Lane 0 ends in float32.  A view
// reads its own four state words before it writes them, and no other view's: state_out may be state_in.
struct AdaptArgs {
    const uint32_t* hist;
    const float* state_in; // or null
    float* state_out;
    uint32_t nv, low_permille, high_permille;
    float key_log2, ev_min, ev_max, rate_up, rate_down;
};

PT_DEV unsigned long long expo_shfl(unsigned long long v, int src) {
    return ((unsigned long long)(uint32_t)__shfl((int)(v >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src);
}
// inclusive prefix sum over the wave's lanes
PT_DEV unsigned long long expo_scan(unsigned long long v, uint32_t lane) {
#pragma unroll
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
        const unsigned long long t = expo_shfl(v, (int)(lane >= off ? lane - off : lane));
        if (lane >= off) v += t;
    }
    return v;
}

__global__ void __launch_bounds__(64) k_adapt(AdaptArgs a) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t v = blockIdx.x, lane = threadIdx.x;
    if (v >= a.nv) return;
    unsigned long long c[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) c[k] = a.hist[(size_t)v * EXPO_BINS + 4u * lane + k];
    // ---------------- 1, 2. the total, the two trims
    unsigned long long sum = (c[0] + c[1]) + (c[2] + c[3]);
    unsigned long long incl = expo_scan(sum, lane);
    const unsigned long long N = expo_shfl(incl, 63);
    const unsigned long long lo = N * a.low_permille / 1000ull, hi = N * a.high_permille / 1000ull;
    // ---------------- 3. up from bin 0
    unsigned long long before = incl - sum;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long rem = lo > before ? lo - before : 0ull, take = c[k] < rem ? c[k] : rem;
        before += c[k];
        c[k] -= take;
    }
    // down from bin 255, on what is left
    sum = (c[0] + c[1]) + (c[2] + c[3]);
    incl = expo_scan(sum, lane);
    unsigned long long after = expo_shfl(incl, 63) - incl;
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        const unsigned long long rem = hi > after ? hi - after : 0ull, take = c[k] < rem ? c[k] : rem;
        after += c[k];
        c[k] -= take;
    }
    // ---------------- 4. n and S over bins 1 .. 254
    unsigned long long n = 0, S = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t i = 4u * lane + k;
        if (i >= 1u && i <= 254u) {
            n += c[k];
            S += c[k] * (unsigned long long)(2u * i - 1u);
        }
    }
    n = expo_shfl(expo_scan(n, lane), 63);
    S = expo_shfl(expo_scan(S, lane), 63);
    if (lane != 0u) return;
    // ---------------- 5 .. 8.
    const bool have = a.state_in != nullptr;
    const float ev_prev = have ? a.state_in[4 * (size_t)v] : 0.0f;
    const bool prev_ok = have && tp_finite(ev_prev);
    float m, ev;
    if (n == 0) {
        m = have ? a.state_in[4 * (size_t)v + 2] : __uint_as_float(0x7fc00000u);
        ev = prev_ok ? ev_prev : 0.0f;
    } else {
        const unsigned long long q = (S << 12) / n;
        m = (float)q * (1.0f / 65536.0f) - 16.0f;
        float t = a.key_log2 - m;
        t = t < a.ev_min ? a.ev_min : t;
        t = t > a.ev_max ? a.ev_max : t;
        if (!prev_ok) {
            ev = t;
        } else {
            const float r = (t > ev_prev) ? a.rate_up : a.rate_down;
            ev = ev_prev + ((t - ev_prev) * r);
        }
    }
    const float E = pt_expf(ev * 0.69314718f);
    gb_store4(a.state_out + 4 * (size_t)v, make_float4(ev, E, m, (float)n));
#endif
}

// k_tonemap: one thread per entry of the pixel list, 256 per block, pixel-local and streaming — k_modulate's shape with the view's exposure
// word read from device memory (one word per view: it stays in cache).  out may be color itself.
struct TonemapArgs {
    const uint32_t* pixels;
    uint32_t n;
    int width, height;
    const float* color;
    const float* state; // or null
    float* out;         // or null
    uint32_t* frame;    // or null
    float exposure, white;
    uint32_t op;
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] clipped
};

PT_DEV float tm_clamp(float x) {
    x = x > 0.0f ? x : 0.0f;
    return x < 65504.0f ? x : 65504.0f;
}
PT_DEV float tm_aces(float x) {
    const float a = x * (2.51f * x + 0.03f), b = x * (2.43f * x + 0.59f) + 0.14f;
    return a / b;
}

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_tonemap(TonemapArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool clipped = false;
    if (i < a.n) {
        const PassPixel px = pass_pixel<VIEWS>(vp, a.pixels[i], a.width, a.height);
        const size_t p = (size_t)px.Y * (size_t)a.width + px.X;
        const float4 c = tp_load4(a.color + 4 * p);
        float E = a.state ? a.state[4 * (size_t)px.view + 1] : 1.0f;
        if (!(tp_finite(E) && E > 0.0f)) E = 1.0f;
        const float s = E * a.exposure;
        const v3 x = mk3(tm_clamp(c.x * s), tm_clamp(c.y * s), tm_clamp(c.z * s));
        v3 y = x;
        if (a.op == 1u) y = reinhard_tonemap(x, a.white);
        else if (a.op == 2u) y = mk3(tm_aces(x.x), tm_aces(x.y), tm_aces(x.z));
        clipped = y.x > 1.0f || y.y > 1.0f || y.z > 1.0f;
        if (a.out) gb_store4(a.out + 4 * p, make_float4(y.x, y.y, y.z, 1.0f));
        if (a.frame) a.frame[p] = make_color(y);
    }
    pass_tally(pass_slot(a.counts), {clipped});
#endif
}
