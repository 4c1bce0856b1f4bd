// pt_ao_layout and pt_ao_planes (include/pt_amd.h): ambient occlusion from the G-buffer, the one pass of the chain that asks the
// acceleration structure a question.  Two kernels around the existing any-hit traversal, per batch of the call's pixel list:
// k_ao_rays<VIEWS> builds a pixel's rays from hit and position in registers and writes them where k_trace8<TR_ANY_QUERY> reads its rays
// (PathState::rayO / rayD, the identity queue's count word); k_ao_reduce turns the traversal's records into ao, out and bent.  The rays,
// the records and two words per batch pixel live in the caller's scratch (AoScratch below); nothing is frame-sized.
//
// Layout of a batch: SAMPLE-MAJOR INSIDE A WORKGROUP.  A workgroup of k_ao_rays owns AO_GROUP consecutive entries of the pixel list, of
// which `total` shoot; one atomic on the count word gives it total * rays consecutive slots from `base`, and sample k of the pixel of
// rank r (its place among the group's shooting pixels, in list order) sits at base + k * total + r.  So the store of sample k is one
// coalesced run of 16-byte slots across the lanes, and so is the reduction's load of its record; the 64 rays a traversal wave loads are
// the same sample of 64 neighbouring pixels.  The reduction finds a pixel's records through two words: first = base + r, stride = total.
// The first version was pixel-major (sample k at first + k, one atomic per 256 pixels): its stores lay 16 * rays bytes apart across the
// lanes and its 8100 atomics a 1080p batch on one address (about 10 ns each, pt_pass_dev.h) cost more than the rays' arithmetic; figures
// in profiles/ao.md.
// A pixel of step 1 or 2 takes no slot (first = AO_NO_RAYS) and gets its constant outputs from k_ao_rays.  An invalid ray (step 7) keeps
// its slot and is staged as pt_trace_device stages one: as the neutral ray (tmin 1 > tmax -1), which no triangle can hit (the traversal
// asks t > tmin && t < tmax), so its record is 0, unoccluded, as the rule wants it; the reduction knows it by its tmax where bent needs to.
#pragma once
#include "pt_pass_dev.h"

// The host's table of a call: the spiral's directions (pass_spiral, pt_pass.h: depth of field's recurrence) and rho[k] = sqrtf((k + 0.5f) / rays)
struct AoTaps {
    float2 D[128];
    float rho[PT_AO_MAX_RAYS];
};

#define AO_NO_RAYS 0xffffffffu
#define AO_HEAD_BYTES 256u // count at byte 0, the traversal's chunk counter at 64, the fault word at 128
#define AO_PER_THREAD 4u
#define AO_GROUP (256u * AO_PER_THREAD) // entries of the pixel list a workgroup of k_ao_rays owns
// The scratch of a call, for batches of at most `pixels` pixels: the head, then rayO, rayD (16 bytes a slot), hit (8), pix (8 a pixel)
struct AoScratch {
    uint32_t *count, *work, *fault;
    float4 *rayO, *rayD;
    float2* hit;
    uint2* pix; // per batch pixel: first slot | stride between its samples
};
static inline size_t ao_scratch_bytes(uint64_t pixels, uint32_t rays) {
    const uint64_t slots = pixels * rays;
    return (size_t)((AO_HEAD_BYTES + slots * 40u + pixels * 8u + 15u) & ~(uint64_t)15u);
}
static inline AoScratch ao_scratch(void* p, uint64_t pixels, uint32_t rays) {
    uint8_t* b = reinterpret_cast<uint8_t*>(p);
    const uint64_t slots = pixels * rays;
    AoScratch s;
    s.count = reinterpret_cast<uint32_t*>(b);
    s.work = reinterpret_cast<uint32_t*>(b + 64);
    s.fault = reinterpret_cast<uint32_t*>(b + 128);
    s.rayO = reinterpret_cast<float4*>(b + AO_HEAD_BYTES);
    s.rayD = s.rayO + slots;
    s.hit = reinterpret_cast<float2*>(s.rayD + slots);
    s.pix = reinterpret_cast<uint2*>(s.hit + slots);
    return s;
}

struct AoArgs {
    const uint32_t* pixels; // the batch's part of the call's list
    uint32_t n;
    int width, height;
    const float *hit, *position;
    float *ao, *out, *bent;
    AoScratch s;
    const AoTaps* tt;
    v3 eye; // the frame's camera (unused with views)
    uint32_t rays;
    float radius, bias;
    uint32_t seed, jitter;
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] skipped, [1] nonfinite, [2] invalid (k_ao_rays), [3] occluded (k_ao_reduce)
};

PT_DEV void ao_write(const AoArgs& a, size_t p, float ao, v3 bent) {
    if (a.ao) a.ao[p] = ao;
    if (a.out) gb_store4(a.out + 4 * p, make_float4(ao, ao, ao, 1.0f));
    if (a.bent) gb_store4(a.bent + 4 * p, make_float4(bent.x, bent.y, bent.z, ao));
}

// ------------------------------------------------------------------ k_ao_rays: steps 1 to 7
// 256 threads, AO_PER_THREAD pixels a thread: entry blockIdx.x * AO_GROUP + j * 256 + threadIdx.x for j = 0 .. 3, so every load of a plane
// runs over consecutive entries across the lanes and all twelve 16-byte loads of a thread are in flight before the first is used.
template <bool VIEWS>
__global__ void __launch_bounds__(256) k_ao_rays(AoArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    __shared__ uint32_t s_cnt[AO_PER_THREAD * 4u]; // shooting pixels of (j, wave), in list order
    __shared__ uint32_t s_base, s_total;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t nskipped = 0u, nnonfinite = 0u, ninvalid = 0u;
    PassPixel px[AO_PER_THREAD];
    float4 ha[AO_PER_THREAD], hb[AO_PER_THREAD], P4[AO_PER_THREAD];
    unsigned long long m[AO_PER_THREAD];
    bool shoots[AO_PER_THREAD];
#pragma unroll
    for (uint32_t j = 0; j < AO_PER_THREAD; ++j) {
        const uint32_t i = blockIdx.x * AO_GROUP + j * 256u + threadIdx.x;
        px[j] = PassPixel{};
        ha[j] = hb[j] = P4[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < a.n) {
            px[j] = pass_pixel<VIEWS>(vp, a.pixels[i], a.width, a.height);
            const size_t p = (size_t)px[j].Y * (size_t)a.width + px[j].X;
            ha[j] = tp_load4(a.hit + 8 * p);
            hb[j] = tp_load4(a.hit + 8 * p + 4);
            P4[j] = tp_load4(a.position + 4 * p);
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < AO_PER_THREAD; ++j) {
        const uint32_t i = blockIdx.x * AO_GROUP + j * 256u + threadIdx.x;
        shoots[j] = false;
        if (i < a.n) {
            if (hit_is_miss(ha[j].w)) ++nskipped; // step 1
            else {
                const bool fin = tp_finite(P4[j].x) && tp_finite(P4[j].y) && tp_finite(P4[j].z) && tp_finite(hb[j].y) && tp_finite(hb[j].z) && tp_finite(hb[j].w) &&
                                 tp_finite(ha[j].x);
                shoots[j] = fin && ha[j].x > 0.0f; // step 2
                if (!shoots[j]) ++nnonfinite;
            }
        }
        m[j] = __ballot(shoots[j]);
        if (lane == 0u) s_cnt[j * 4u + wave] = (uint32_t)__popcll(m[j]);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u;
        for (uint32_t e = 0; e < AO_PER_THREAD * 4u; ++e) total += s_cnt[e];
        s_total = total;
        s_base = total ? atomicAdd(a.s.count, total * a.rays) : 0u; // the group's slots: [base, base + total * rays)
    }
    __syncthreads();
    const uint32_t total = s_total;
#pragma unroll
    for (uint32_t j = 0; j < AO_PER_THREAD; ++j) {
        const uint32_t i = blockIdx.x * AO_GROUP + j * 256u + threadIdx.x;
        if (i >= a.n) continue;
        const size_t p = (size_t)px[j].Y * (size_t)a.width + px[j].X;
        if (!shoots[j]) {
            a.s.pix[i] = make_uint2(AO_NO_RAYS, 0u);
            ao_write(a, p, 1.0f, mk3(0.0f));
            continue;
        }
        uint32_t rank = (uint32_t)__popcll(m[j] & ((1ull << lane) - 1ull));
        for (uint32_t e = 0; e < j * 4u + wave; ++e) rank += s_cnt[e];
        const uint32_t first = s_base + rank;
        const v3 P = mk3(P4[j].x, P4[j].y, P4[j].z), n0 = mk3(hb[j].y, hb[j].z, hb[j].w);
        v3 E = a.eye;
        if (VIEWS) {
            const pt_view& vw = vp.views[px[j].view];
            E = mk3(vw.eye[0], vw.eye[1], vw.eye[2]);
        }
        // ---------------- 3. face the viewer
        const float s = dot3(n0, sub3(E, P));
        const v3 n = s < 0.0f ? neg3(n0) : n0;
        // ---------------- 4. the frame
        const float sg = n.z >= 0.0f ? 1.0f : -1.0f;
        const float fa = -1.0f / (sg + n.z);
        const float fb = (n.x * n.y) * fa;
        const v3 T = mk3(1.0f + (sg * (n.x * n.x)) * fa, sg * fb, (-sg) * n.x);
        const v3 B = mk3(fb, sg + (n.y * n.y) * fa, -n.y);
        // ---------------- 5. the origin
        const float lift = a.bias * ha[j].x;
        const v3 O = add3(P, scl3(n, lift));
        const bool o_ok = tp_finite(O.x) && tp_finite(O.y) && tp_finite(O.z);
        const int x = (int)px[j].X - px[j].x0, y = (int)px[j].Y - px[j].y0;
        const uint32_t k0 = a.jitter ? pass_hash((uint32_t)x, (uint32_t)y, a.seed) & 63u : 0u;
        // ---------------- 6, 7. the rays
        for (uint32_t k = 0; k < a.rays; ++k) {
            const float rho = a.tt->rho[k];
            const float2 D = a.tt->D[(k + k0) & 127u];
            const float ak = rho * D.x, bk = rho * D.y;
            const float ck = sqrtf(fl_max0(1.0f - (ak * ak + bk * bk)));
            const v3 w = add3(add3(scl3(T, ak), scl3(B, bk)), scl3(n, ck));
            const v3 d = normalize3(w);
            // pt_trace_device's rule (k_stage_rays): eight finite words, dot3(d, d) and its reciprocal finite and not zero
            const float dd = dot3(d, d);
            const float inv = 1.0f / dd;
            const bool ok = o_ok && tp_finite(d.x) && tp_finite(d.y) && tp_finite(d.z) && tp_finite(dd) && query_nonzero(dd) && tp_finite(inv) && query_nonzero(inv);
            float4 o4 = make_float4(O.x, O.y, O.z, 0.0f), d4 = make_float4(d.x, d.y, d.z, a.radius);
            if (!ok) { // the neutral ray, as k_stage_rays leaves an invalid one: never traversed
                o4 = make_float4(0.f, 0.f, 0.f, 1.f);
                d4 = make_float4(0.f, 0.f, 1.f, -1.f);
                ++ninvalid;
            }
            const size_t slot = (size_t)first + (size_t)k * total;
            a.s.rayO[slot] = o4;
            a.s.rayD[slot] = d4;
        }
        a.s.pix[i] = make_uint2(first, total);
    }
    const uint32_t sums[3] = {nskipped, nnonfinite, ninvalid};
    pass_tally_sums(a.counts, 0u, sums);
#endif
}

// ------------------------------------------------------------------ k_ao_reduce: step 9, one thread per pixel of the batch
// occ_k is the traversal's record (1 occluded / 0; 0 for the neutral ray of an invalid sample); d_k is read back from the batch's
// direction array, which holds the bits k_ao_rays normalised, and only when bent is wanted (tmax < 0 marks the neutral ray).  A pixel
// without rays has its outputs already.  The batch's traversal is over, so thread 0 clears the count word and the traversal's chunk
// counter for the next batch's k_ao_rays (the call's memset cleared them for the first).
__global__ void __launch_bounds__(256) k_ao_reduce(AoArgs a) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0u) {
        *a.s.count = 0u;
        *a.s.work = 0u;
    }
    uint32_t nocc = 0u;
    if (i < a.n) {
        const uint2 pm = a.s.pix[i];
        if (pm.x != AO_NO_RAYS) {
            const uint32_t xy = a.pixels[i];
            const size_t p = (size_t)pass_y(xy) * (size_t)a.width + pass_x(xy);
            uint32_t open = 0u;
            v3 S = mk3(0.0f);
            for (uint32_t k = 0; k < a.rays; ++k) {
                const size_t slot = (size_t)pm.x + (size_t)k * pm.y;
                if (__float_as_int(a.s.hit[slot].y) != 0) ++nocc;
                else {
                    ++open;
                    if (a.bent) {
                        const float4 d = a.s.rayD[slot];
                        if (d.w > 0.0f) S = add3(S, mk3(d.x, d.y, d.z));
                    }
                }
            }
            const float fr = (float)a.rays;
            ao_write(a, p, (float)open / fr, mk3(S.x / fr, S.y / fr, S.z / fr));
        }
    }
    const uint32_t sums[1] = {nocc};
    pass_tally_sums(a.counts, 3u, sums);
#endif
}
