// pt_shadow_layout and pt_shadow_planes (include/pt_amd.h): shadows and direct light of up to four distant disc lights from the G-buffer,
// the third pass of the chain that asks the acceleration structure.  Two kernels around the existing any-hit traversal, per batch of the
// call's pixel list, as pt_ao.h's: k_shadow_rays<VIEWS> builds a pixel's rays from hit and position in registers and writes them where
// k_trace8<TR_ANY_QUERY> reads its rays; k_shadow_reduce<VIEWS> turns the traversal's records into visibility and light.
//
// What differs from ambient occlusion is the number of rays a pixel shoots: rays_i for every light above its horizon, none for the others.
// So the slot compaction of a workgroup is PER LIGHT.  A workgroup owns SH_GROUP consecutive entries of the pixel list; total_i of them
// shoot at light i.  One atomic on the count word gives it sum_i total_i * rays_i consecutive slots from `base`; light i's part starts at
// off_i = sum_{j<i} total_j * rays_j, and sample k of the pixel of rank r among that light's shooters (in list order) sits at
// base + off_i + k * total_i + r.  The store of one sample of one light is a coalesced run of 16-byte slots across the lanes, and the 64
// rays a traversal wave loads are the same sample, towards the same light, of neighbouring pixels.  The reduction finds the records of
// (pixel, light) through two words: first = base + off_i + r, stride = total_i; a light under the pixel's horizon has first = SH_NO_RAYS.
// A pixel of step 1 or 2 has (SH_NO_RAYS, SH_CONSTANT) in its first pair and gets its constant outputs from k_shadow_rays.  An invalid ray
// keeps its slot and is staged as the neutral ray, as in pt_ao.h.
#pragma once
#include "pt_pass_dev.h"

// A light as the kernels take it, by value in the kernel argument (uniform: scalar registers): L = normalize3(dir), T and B the frame of
// pt_ao_planes's step 4 around L, computed once on the host (shadow_light_dev, pt_shadow.hip)
struct ShadowLightDev {
    v3 L, T, B;
    float spread;
    uint32_t rays;
    uint32_t rho0; // where the light's rho table starts in ShadowTaps::rho
};
// The host's table of a call: the spiral's directions (pass_spiral) and, light after light, rho[rho0 + k] = sqrtf((k + 0.5f) / rays)
struct ShadowTaps {
    float2 D[128];
    float rho[PT_SHADOW_MAX_RAYS];
};

#define SH_NO_RAYS 0xffffffffu
#define SH_CONSTANT 1u // the stride word of a pixel of step 1 or 2: its outputs are written already
#define SH_HEAD_BYTES 256u // count at byte 0, the traversal's chunk counter at 64, the fault word at 128
#define SH_PER_THREAD 4u
#define SH_GROUP (256u * SH_PER_THREAD) // entries of the pixel list a workgroup of k_shadow_rays owns
#define SH_LIGHTS ((uint32_t)PT_SHADOW_MAX_LIGHTS)
// The scratch of a call, for batches of at most `pixels` pixels of R rays: the head, then rayO, rayD (16 bytes a slot), hit (8), pix (32 a pixel)
struct ShadowScratch {
    uint32_t *count, *work, *fault;
    float4 *rayO, *rayD;
    float2* hit;
    uint2* pix; // per batch pixel and light: first slot | stride between the samples
};
static inline size_t shadow_scratch_bytes(uint64_t pixels, uint32_t R) {
    const uint64_t slots = pixels * R;
    return (size_t)((SH_HEAD_BYTES + slots * 40u + pixels * 32u + 15u) & ~(uint64_t)15u);
}
static inline ShadowScratch shadow_scratch(void* p, uint64_t pixels, uint32_t R) {
    uint8_t* b = reinterpret_cast<uint8_t*>(p);
    const uint64_t slots = pixels * R;
    ShadowScratch s;
    s.count = reinterpret_cast<uint32_t*>(b);
    s.work = reinterpret_cast<uint32_t*>(b + 64);
    s.fault = reinterpret_cast<uint32_t*>(b + 128);
    s.rayO = reinterpret_cast<float4*>(b + SH_HEAD_BYTES);
    s.rayD = s.rayO + slots;
    s.hit = reinterpret_cast<float2*>(s.rayD + slots);
    s.pix = reinterpret_cast<uint2*>(s.hit + slots);
    return s;
}

struct ShadowArgs {
    const uint32_t* pixels; // the batch's part of the call's list
    uint32_t n;
    int width, height;
    const float *hit, *position, *view_ray;
    float *visibility, *light;
    ShadowScratch s;
    const ShadowTaps* tt;
    v3 eye; // the frame's camera (unused with views and with view_ray)
    uint32_t num_lights;
    float max_distance, bias;
    uint32_t seed, jitter;
    ShadowLightDev lights[PT_SHADOW_MAX_LIGHTS];
    v3 radiance[PT_SHADOW_MAX_LIGHTS];
    // [PASS_SLOTS][8]: [0] skipped, [1] nonfinite, [2] invalid, [3] backfacing, [4] slots (k_shadow_rays), [5] occluded (k_shadow_reduce)
    unsigned long long* counts;
};

// steps 1 and 2 over a pixel's loaded words: 0 shoots, 1 a miss, 2 nonfinite.  E4: view_ray's first four words (zeros without view_ray)
PT_DEV uint32_t shadow_class(float4 ha, float4 hb, float4 P4, float4 E4) {
    if (hit_is_miss(ha.w)) return 1u;
    const bool fin = tp_finite(P4.x) && tp_finite(P4.y) && tp_finite(P4.z) && tp_finite(hb.y) && tp_finite(hb.z) && tp_finite(hb.w) && tp_finite(ha.x) &&
                     tp_finite(E4.x) && tp_finite(E4.y) && tp_finite(E4.z);
    return fin && ha.x > 0.0f ? 0u : 2u;
}
// step 3: the normal turned towards E
PT_DEV v3 shadow_facing(float4 hb, float4 P4, v3 E) {
    const v3 P = mk3(P4.x, P4.y, P4.z), n0 = mk3(hb.y, hb.z, hb.w);
    const float s = dot3(n0, sub3(E, P));
    return s < 0.0f ? neg3(n0) : n0;
}
template <bool VIEWS>
PT_DEV v3 shadow_eye(const ShadowArgs& a, const ViewParams& vp, const PassPixel& px, float4 E4) {
    if (a.view_ray) return mk3(E4.x, E4.y, E4.z);
    if (VIEWS) {
        const pt_view& vw = vp.views[px.view];
        return mk3(vw.eye[0], vw.eye[1], vw.eye[2]);
    }
    return a.eye;
}
PT_DEV void shadow_write(const ShadowArgs& a, size_t p, float4 vis, v3 light) {
    if (a.visibility) gb_store4(a.visibility + 4 * p, vis);
    if (a.light) gb_store4(a.light + 4 * p, make_float4(light.x, light.y, light.z, 1.0f));
}

// ------------------------------------------------------------------ k_shadow_rays: steps 1 to 5
// 256 threads, SH_PER_THREAD pixels a thread: entry blockIdx.x * SH_GROUP + j * 256 + threadIdx.x for j = 0 .. 3, so every load of a plane
// runs over consecutive entries across the lanes, and all sixteen 16-byte loads of a thread are in flight before the first is used.
template <bool VIEWS>
__global__ void __launch_bounds__(256) k_shadow_rays(ShadowArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    __shared__ uint32_t s_cnt[SH_LIGHTS][SH_PER_THREAD * 4u]; // per light: shooting pixels of (j, wave), in list order
    __shared__ uint32_t s_first[SH_LIGHTS], s_total[SH_LIGHTS]; // per light: base + off_i, total_i
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t nl = a.num_lights;
    uint32_t nskipped = 0u, nnonfinite = 0u, ninvalid = 0u, nback = 0u, nslots = 0u;
    PassPixel px[SH_PER_THREAD];
    float4 ha[SH_PER_THREAD], hb[SH_PER_THREAD], P4[SH_PER_THREAD], E4[SH_PER_THREAD];
#pragma unroll
    for (uint32_t j = 0; j < SH_PER_THREAD; ++j) {
        const uint32_t i = blockIdx.x * SH_GROUP + j * 256u + threadIdx.x;
        px[j] = PassPixel{};
        ha[j] = hb[j] = P4[j] = E4[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < a.n) {
            px[j] = pass_pixel<VIEWS>(vp, a.pixels[i], a.width, a.height);
            const size_t p = (size_t)px[j].Y * (size_t)a.width + px[j].X;
            ha[j] = tp_load4(a.hit + 8 * p);
            hb[j] = tp_load4(a.hit + 8 * p + 4);
            P4[j] = tp_load4(a.position + 4 * p);
            if (a.view_ray) E4[j] = tp_load4(a.view_ray + 8 * p);
        }
    }
    v3 nrm[SH_PER_THREAD];
    unsigned long long m[SH_PER_THREAD][SH_LIGHTS]; // the ballots: uniform across the wave
    uint32_t cls[SH_PER_THREAD];                    // 0 shoots, 1 a miss, 2 nonfinite, 3 no entry
#pragma unroll
    for (uint32_t j = 0; j < SH_PER_THREAD; ++j) {
        const uint32_t i = blockIdx.x * SH_GROUP + j * 256u + threadIdx.x;
        cls[j] = 3u;
        nrm[j] = mk3(0.0f);
        if (i < a.n) {
            cls[j] = shadow_class(ha[j], hb[j], P4[j], E4[j]);
            if (cls[j] == 1u) ++nskipped;
            else if (cls[j] == 2u) ++nnonfinite;
            else nrm[j] = shadow_facing(hb[j], P4[j], shadow_eye<VIEWS>(a, vp, px[j], E4[j])); // step 3
        }
#pragma unroll
        for (uint32_t li = 0; li < SH_LIGHTS; ++li) {
            bool shoots = false;
            if (li < nl && cls[j] == 0u) {
                shoots = dot3(nrm[j], a.lights[li].L) > 0.0f; // step 4
                if (shoots) nslots += a.lights[li].rays;
                else ++nback;
            }
            m[j][li] = __ballot(shoots);
            if (lane == 0u) s_cnt[li][j * 4u + wave] = (uint32_t)__popcll(m[j][li]);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total[SH_LIGHTS], slots = 0u;
        for (uint32_t li = 0; li < SH_LIGHTS; ++li) {
            total[li] = 0u;
            for (uint32_t e = 0; e < SH_PER_THREAD * 4u; ++e) total[li] += s_cnt[li][e];
            slots += li < nl ? total[li] * a.lights[li].rays : 0u;
        }
        uint32_t at = slots ? atomicAdd(a.s.count, slots) : 0u; // the group's slots: [base, base + sum_i total_i * rays_i)
        for (uint32_t li = 0; li < SH_LIGHTS; ++li) {
            s_first[li] = at;
            s_total[li] = total[li];
            at += li < nl ? total[li] * a.lights[li].rays : 0u;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < SH_PER_THREAD; ++j) {
        const uint32_t i = blockIdx.x * SH_GROUP + j * 256u + threadIdx.x;
        if (i >= a.n) continue;
        uint2* pix = a.s.pix + (size_t)i * SH_LIGHTS;
        if (cls[j] != 0u) {
            const size_t p = (size_t)px[j].Y * (size_t)a.width + px[j].X;
            pix[0] = make_uint2(SH_NO_RAYS, SH_CONSTANT);
            shadow_write(a, p, make_float4(1.0f, 1.0f, 1.0f, 1.0f), mk3(0.0f));
            continue;
        }
        const v3 P = mk3(P4[j].x, P4[j].y, P4[j].z), n = nrm[j];
        const float lift = a.bias * ha[j].x;
        const v3 O = add3(P, scl3(n, lift));
        const bool o_ok = tp_finite(O.x) && tp_finite(O.y) && tp_finite(O.z);
        const int x = (int)px[j].X - px[j].x0, y = (int)px[j].Y - px[j].y0;
#pragma unroll
        for (uint32_t li = 0; li < SH_LIGHTS; ++li) { // (unrolled: m and a.lights are indexed by constants)
            if (li >= nl) break;
            const unsigned long long mm = m[j][li];
            if (!((mm >> lane) & 1ull)) {
                pix[li] = make_uint2(SH_NO_RAYS, 0u);
                continue;
            }
            const ShadowLightDev& lt = a.lights[li];
            const uint32_t total = s_total[li];
            uint32_t rank = (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
            for (uint32_t e = 0; e < j * 4u + wave; ++e) rank += s_cnt[li][e];
            const uint32_t first = s_first[li] + rank;
            const uint32_t k0 = a.jitter ? pass_hash((uint32_t)x, (uint32_t)y, a.seed + li) & 63u : 0u;
            // ---------------- 5. the rays of light li
            for (uint32_t k = 0; k < lt.rays; ++k) {
                const float rho = a.tt->rho[lt.rho0 + k];
                const float2 D = a.tt->D[(k + k0) & 127u];
                const float ak = (rho * D.x) * lt.spread, bk = (rho * D.y) * lt.spread;
                const v3 w = add3(add3(lt.L, scl3(lt.T, ak)), scl3(lt.B, bk));
                const v3 d = normalize3(w);
                // pt_trace_device's rule (k_stage_rays): eight finite words, dot3(d, d) and its reciprocal finite and not zero
                const float dd = dot3(d, d);
                const float inv = 1.0f / dd;
                const bool ok = o_ok && tp_finite(d.x) && tp_finite(d.y) && tp_finite(d.z) && tp_finite(dd) && query_nonzero(dd) && tp_finite(inv) && query_nonzero(inv);
                float4 o4 = make_float4(O.x, O.y, O.z, 0.0f), d4 = make_float4(d.x, d.y, d.z, a.max_distance);
                if (!ok) { // the neutral ray, as k_stage_rays leaves an invalid one: never traversed
                    o4 = make_float4(0.f, 0.f, 0.f, 1.f);
                    d4 = make_float4(0.f, 0.f, 1.f, -1.f);
                    ++ninvalid;
                }
                const size_t slot = (size_t)first + (size_t)k * total;
                a.s.rayO[slot] = o4;
                a.s.rayD[slot] = d4;
            }
            pix[li] = make_uint2(first, total);
        }
    }
    const uint32_t sums[5] = {nskipped, nnonfinite, ninvalid, nback, nslots};
    pass_tally_sums(a.counts, 0u, sums);
#endif
}

// ------------------------------------------------------------------ k_shadow_reduce: steps 6 and 7, one thread per pixel of the batch
// occ is the traversal's record (1 occluded / 0; 0 for the neutral ray of an invalid sample).  c_i is not carried through the scratch: with
// `light` the thread loads the pixel's three plane words again and repeats steps 3 and 4, operation for operation (shadow_facing, dot3), so
// the bits are k_shadow_rays's.  A pixel of step 1 or 2 has its outputs already.  The batch's traversal is over, so thread 0 clears the count
// word and the traversal's chunk counter for the next batch's k_shadow_rays (the call's memset cleared them for the first).
template <bool VIEWS>
__global__ void __launch_bounds__(256) k_shadow_reduce(ShadowArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0u) {
        *a.s.count = 0u;
        *a.s.work = 0u;
    }
    uint32_t nocc = 0u;
    if (i < a.n) {
        const uint2* pix = a.s.pix + (size_t)i * SH_LIGHTS;
        const uint2 p0 = pix[0];
        if (!(p0.x == SH_NO_RAYS && p0.y == SH_CONSTANT)) {
            const PassPixel px = pass_pixel<VIEWS>(vp, a.pixels[i], a.width, a.height);
            const size_t p = (size_t)px.Y * (size_t)a.width + px.X;
            v3 n = mk3(0.0f);
            if (a.light) {
                const float4 hb = tp_load4(a.hit + 8 * p + 4), P4 = tp_load4(a.position + 4 * p);
                const float4 E4 = a.view_ray ? tp_load4(a.view_ray + 8 * p) : make_float4(0.f, 0.f, 0.f, 0.f);
                n = shadow_facing(hb, P4, shadow_eye<VIEWS>(a, vp, px, E4));
            }
            float v[SH_LIGHTS] = {1.0f, 1.0f, 1.0f, 1.0f};
            v3 S = mk3(0.0f);
#pragma unroll
            for (uint32_t li = 0; li < SH_LIGHTS; ++li) {
                if (li >= a.num_lights) break;
                const uint2 pm = li ? pix[li] : p0;
                if (pm.x == SH_NO_RAYS) {
                    v[li] = 0.0f;
                    continue;
                }
                const uint32_t rays = a.lights[li].rays;
                uint32_t open = 0u;
                for (uint32_t k = 0; k < rays; ++k) {
                    const size_t slot = (size_t)pm.x + (size_t)k * pm.y;
                    if (__float_as_int(a.s.hit[slot].y) != 0) ++nocc;
                    else ++open;
                }
                v[li] = (float)open / (float)rays;
                if (a.light) {
                    const float c = dot3(n, a.lights[li].L);
                    const float cv = (c > 1.0f ? 1.0f : c) * v[li];
                    S = add3(S, scl3(a.radiance[li], cv));
                }
            }
            shadow_write(a, p, make_float4(v[0], v[1], v[2], v[3]), S);
        }
    }
    const uint32_t sums[1] = {nocc};
    pass_tally_sums(a.counts, 5u, sums);
#endif
}
