// pt_reflect_layout and pt_reflect_planes (include/pt_amd.h): mirror reflections from the G-buffer, a second G-buffer seen along each
// pixel's mirror ray.  Two kernels around the existing closest-hit traversal, per batch of the call's pixel list: k_reflect_rays<VIEWS>
// builds a pixel's one ray from hit, position and the eye in registers and writes it where k_trace8<TR_CLOSEST> reads its rays
// (PathState::rayO / rayD, the identity queue's count word); k_reflect_resolve turns the traversal's (t, leaf) record into hit2, position2
// and sky.  The rays, the records and one word per batch pixel live in the caller's scratch (ReflectScratch below); nothing is frame-sized.
//
// Layout of a batch, as pt_ao.h's with one ray a pixel: a workgroup of k_reflect_rays owns REFLECT_GROUP consecutive entries of the pixel
// list, of which `total` shoot; one atomic on the count word gives it `total` consecutive slots from `base`, and the pixel of rank r (its
// place among the group's shooting pixels, in list order) sits at base + r.  A pixel of step 1 or 2 takes no slot (REFLECT_NO_RAY) and
// gets its constant outputs from k_reflect_rays.  An invalid ray (step 6) keeps its slot and is staged as pt_trace_device stages one: as
// the neutral ray (tmin 1 > tmax -1), which no triangle can hit; the resolve knows it by its negative staged tmax (max_distance > 0, so
// no valid ray of the pass has one).
// The hit attributes restate k_hit_attributes's expressions (pt_kernels.h) rather than share them, as pt_gbuffer.h does and for the same
// reason: a common helper would change the code the query path is compiled from.
#pragma once
#include "pt_pass_dev.h"

#define REFLECT_NO_RAY 0xffffffffu
#define REFLECT_HEAD_BYTES 256u // count at byte 0, the traversal's chunk counter at 64, the fault word at 128
#define REFLECT_PER_THREAD 4u
#define REFLECT_GROUP (256u * REFLECT_PER_THREAD) // entries of the pixel list a workgroup of k_reflect_rays owns
// The scratch of a call, for batches of at most `pixels` pixels: the head, then rayO, rayD (16 bytes a slot), hit (8), pix (4 a pixel)
struct ReflectScratch {
    uint32_t *count, *work, *fault;
    float4 *rayO, *rayD;
    float2* hit;
    uint32_t* pix; // per batch pixel: its slot, or REFLECT_NO_RAY
};
static inline size_t reflect_scratch_bytes(uint64_t pixels) { return (size_t)((REFLECT_HEAD_BYTES + pixels * 40u + pixels * 4u + 15u) & ~(uint64_t)15u); }
static inline ReflectScratch reflect_scratch(void* p, uint64_t pixels) {
    uint8_t* b = reinterpret_cast<uint8_t*>(p);
    ReflectScratch s;
    s.count = reinterpret_cast<uint32_t*>(b);
    s.work = reinterpret_cast<uint32_t*>(b + 64);
    s.fault = reinterpret_cast<uint32_t*>(b + 128);
    s.rayO = reinterpret_cast<float4*>(b + REFLECT_HEAD_BYTES);
    s.rayD = s.rayO + pixels;
    s.hit = reinterpret_cast<float2*>(s.rayD + pixels);
    s.pix = reinterpret_cast<uint32_t*>(s.hit + pixels);
    return s;
}

struct ReflectArgs {
    const uint32_t* pixels; // the batch's part of the call's list
    uint32_t n;
    int width, height;
    const float *hit, *position;
    float *hit2, *position2, *ray, *sky;
    ReflectScratch s;
    v3 eye; // the frame's camera (unused with views)
    float bias, max_distance;
    const LeafTri* tris;
    const float4* tri_nrm;
    DevProbe probe; // read only when sky is wanted
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] skipped, [1] nonfinite, [2] invalid (k_reflect_rays), [3] hits, [4] escaped (k_reflect_resolve)
};

// what a pixel without a traced ray gets in hit2, position2 and sky: prim -1 for the empty record, -2 for an invalid ray
PT_DEV void reflect_write_none(const ReflectArgs& a, size_t p, int prim) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.hit2) {
        gb_store4(a.hit2 + 8 * p, make_float4(0.f, 0.f, 0.f, __int_as_float(prim)));
        gb_store4(a.hit2 + 8 * p + 4, make_float4(__int_as_float(-1), 0.f, 0.f, 0.f));
    }
    if (a.position2) gb_store4(a.position2 + 4 * p, zero);
    if (a.sky) gb_store4(a.sky + 4 * p, zero);
}

// ------------------------------------------------------------------ k_reflect_rays: steps 1 to 6
// 256 threads, REFLECT_PER_THREAD pixels a thread: entry blockIdx.x * REFLECT_GROUP + j * 256 + threadIdx.x for j = 0 .. 3, so every load of
// a plane runs over consecutive entries across the lanes and all twelve 16-byte loads of a thread are in flight before the first is used.
template <bool VIEWS>
__global__ void __launch_bounds__(256) k_reflect_rays(ReflectArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    __shared__ uint32_t s_cnt[REFLECT_PER_THREAD * 4u]; // shooting pixels of (j, wave), in list order
    __shared__ uint32_t s_base;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t nskipped = 0u, nnonfinite = 0u, ninvalid = 0u;
    PassPixel px[REFLECT_PER_THREAD];
    float4 ha[REFLECT_PER_THREAD], hb[REFLECT_PER_THREAD], P4[REFLECT_PER_THREAD];
    unsigned long long m[REFLECT_PER_THREAD];
    bool shoots[REFLECT_PER_THREAD];
#pragma unroll
    for (uint32_t j = 0; j < REFLECT_PER_THREAD; ++j) {
        const uint32_t i = blockIdx.x * REFLECT_GROUP + j * 256u + threadIdx.x;
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
    for (uint32_t j = 0; j < REFLECT_PER_THREAD; ++j) {
        const uint32_t i = blockIdx.x * REFLECT_GROUP + j * 256u + threadIdx.x;
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
        for (uint32_t e = 0; e < REFLECT_PER_THREAD * 4u; ++e) total += s_cnt[e];
        s_base = total ? atomicAdd(a.s.count, total) : 0u; // the group's slots: [base, base + total)
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < REFLECT_PER_THREAD; ++j) {
        const uint32_t i = blockIdx.x * REFLECT_GROUP + j * 256u + threadIdx.x;
        if (i >= a.n) continue;
        const size_t p = (size_t)px[j].Y * (size_t)a.width + px[j].X;
        if (!shoots[j]) { // the empty record
            a.s.pix[i] = REFLECT_NO_RAY;
            reflect_write_none(a, p, -1);
            if (a.ray) {
                gb_store4(a.ray + 8 * p, make_float4(0.f, 0.f, 0.f, 1.f));
                gb_store4(a.ray + 8 * p + 4, make_float4(0.f, 0.f, 1.f, -1.f));
            }
            continue;
        }
        uint32_t rank = (uint32_t)__popcll(m[j] & ((1ull << lane) - 1ull));
        for (uint32_t e = 0; e < j * 4u + wave; ++e) rank += s_cnt[e];
        const uint32_t slot = s_base + rank;
        const v3 P = mk3(P4[j].x, P4[j].y, P4[j].z), n0 = mk3(hb[j].y, hb[j].z, hb[j].w);
        v3 E = a.eye;
        if (VIEWS) {
            const pt_view& vw = vp.views[px[j].view];
            E = mk3(vw.eye[0], vw.eye[1], vw.eye[2]);
        }
        // ---------------- 3. face the viewer
        const float s = dot3(n0, sub3(E, P));
        const v3 n = s < 0.0f ? neg3(n0) : n0;
        // ---------------- 4. the mirror direction
        const v3 d = normalize3(sub3(P, E));
        const float c = dot3(d, n);
        const float k = 2.0f * c;
        const v3 r = normalize3(mk3(d.x - n.x * k, d.y - n.y * k, d.z - n.z * k));
        // ---------------- 5. the origin
        const float lift = a.bias * ha[j].x;
        const v3 O = add3(P, scl3(n, lift));
        // ---------------- 6. pt_trace_device's rule (k_stage_rays): eight finite words, dot3(r, r) and its reciprocal finite and not zero
        const float dd = dot3(r, r);
        const float inv = 1.0f / dd;
        const bool ok = tp_finite(O.x) && tp_finite(O.y) && tp_finite(O.z) && tp_finite(r.x) && tp_finite(r.y) && tp_finite(r.z) && tp_finite(dd) && query_nonzero(dd) &&
                        tp_finite(inv) && query_nonzero(inv);
        const float4 o4 = make_float4(O.x, O.y, O.z, 0.0f), d4 = make_float4(r.x, r.y, r.z, a.max_distance);
        if (a.ray) { // its own eight words, valid or not
            gb_store4(a.ray + 8 * p, o4);
            gb_store4(a.ray + 8 * p + 4, d4);
        }
        if (ok) {
            a.s.rayO[slot] = o4;
            a.s.rayD[slot] = d4;
        } else { // the neutral ray, as k_stage_rays leaves an invalid one: never traversed
            a.s.rayO[slot] = make_float4(0.f, 0.f, 0.f, 1.f);
            a.s.rayD[slot] = make_float4(0.f, 0.f, 1.f, -1.f);
            ++ninvalid;
        }
        a.s.pix[i] = slot;
    }
    const uint32_t sums[3] = {nskipped, nnonfinite, ninvalid};
    pass_tally_sums(a.counts, 0u, sums);
#endif
}

// ------------------------------------------------------------------ k_reflect_resolve: steps 7 to 9, one thread per pixel of the batch
// The record is the traversal's (t, leaf triangle or -1); the ray is read back as staged, so u and v come from the bits the traversal saw.
// A pixel without a ray has its outputs already.  The batch's traversal is over, so thread 0 clears the count word and the traversal's
// chunk counter for the next batch's k_reflect_rays (the call's memset cleared them for the first).
__global__ void __launch_bounds__(256) k_reflect_resolve(ReflectArgs a) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0u) {
        *a.s.count = 0u;
        *a.s.work = 0u;
    }
    uint32_t nhits = 0u, nescaped = 0u;
    if (i < a.n) {
        const uint32_t slot = a.s.pix[i];
        if (slot != REFLECT_NO_RAY) {
            const uint32_t xy = a.pixels[i];
            const size_t p = (size_t)pass_y(xy) * (size_t)a.width + pass_x(xy);
            const float4 d4 = a.s.rayD[slot];
            if (d4.w < 0.0f) reflect_write_none(a, p, -2); // step 6's invalid ray
            else {
                const float2 h = a.s.hit[slot];
                const int32_t rec = __float_as_int(h.y);
                const v3 ray_dir = mk3(d4.x, d4.y, d4.z);
                if (rec >= 0) {
                    ++nhits;
                    const float4 o4 = a.s.rayO[slot];
                    const v3 ray_o = mk3(o4.x, o4.y, o4.z);
                    if (a.hit2) { // pt_hit by the expressions of k_hit_attributes
                        const LeafTri tri = a.tris[rec];
                        const float4 tn = a.tri_nrm[rec];
                        const v3 v0 = mk3(tri.t0.x, tri.t0.y, tri.t0.z), v1 = mk3(tri.t0.w, tri.t1.x, tri.t1.y), v2 = mk3(tri.t1.z, tri.t1.w, tri.t2.x);
                        const v3 A = sub3(v0, ray_o), B = sub3(v1, ray_o), C = sub3(v2, ray_o);
                        const v3 CxB = cross3(C, B), AxC = cross3(A, C), BxA = cross3(B, A);
                        const float Uw = dot3(ray_dir, CxB), Vw = dot3(ray_dir, AxC), Ww = dot3(ray_dir, BxA);
                        const float det = Uw + Vw + Ww;
                        gb_store4(a.hit2 + 8 * p, make_float4(h.x, Vw / det, Ww / det, tri.t2.y /* the primitive's bits */));
                        gb_store4(a.hit2 + 8 * p + 4, make_float4(tri.t2.z /* the mesh's bits */, tn.x, tn.y, tn.z));
                    }
                    if (a.position2) gb_store4(a.position2 + 4 * p, make_float4(ray_o.x + h.x * ray_dir.x, ray_o.y + h.x * ray_dir.y, ray_o.z + h.x * ray_dir.z, 1.0f));
                    if (a.sky) gb_store4(a.sky + 4 * p, make_float4(0.f, 0.f, 0.f, 0.f));
                } else {
                    ++nescaped;
                    if (a.hit2) {
                        gb_store4(a.hit2 + 8 * p, make_float4(h.x, 0.f, 0.f, __int_as_float(-1)));
                        gb_store4(a.hit2 + 8 * p + 4, make_float4(__int_as_float(-1), 0.f, 0.f, 0.f));
                    }
                    if (a.position2) gb_store4(a.position2 + 4 * p, make_float4(0.f, 0.f, 0.f, 0.f));
                    if (a.sky) { // the frame's miss program: the probe's texel along the ray
                        float pu, pv;
                        probe_dir_to_uv(ray_dir, pu, pv);
                        const float4 texel = probe_eval(a.probe, pu, pv);
                        gb_store4(a.sky + 4 * p, make_float4(texel.x, texel.y, texel.z, 1.0f));
                    }
                }
            }
        }
    }
    const uint32_t sums[2] = {nhits, nescaped};
    pass_tally_sums(a.counts, 3u, sums);
#endif
}
