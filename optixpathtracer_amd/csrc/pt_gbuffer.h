// pt_render_gbuffer (include/pt_amd.h): the first hit under every pixel's centre — ids, depth, position, motion vectors — in ONE kernel.
#pragma once
#include "pt_bvh8.h"
#include "pt_kernels.h"
#include "pt_pass_dev.h"

// One wave per 64 consecutive entries of the frame's pixel list (8x8-block order: a full packet is one block's frustum).  Each lane builds
// its ray in registers from the pixel word and the camera (generate_path's expression with both jitter values 0.5f), the wave traverses
// the tree once for its 64 rays, and each lane turns its (best, bleaf) into the planes the caller asked for: 4 bytes read per pixel, the
// planes written, no ray or hit records in between.
//
// The traversal loop is k_trace8_cam's (pt_bvh8.h), RESTATED rather than shared with it: a common PT_DEV function would have changed the
// frame path's kernel, whose code this feature leaves as it is (k_hit_attributes restates the barycentrics for the same reason).  Node and
// leaf records through the constant address space, one group stack per wave in LDS, wave-uniform control flow, the same box and triangle
// arithmetic, the same acceptance rule (tt > tmin, lowest primitive on ties, hit_in_box), the same neutral ray for lanes past the end — so
// the answer is k_trace8<TR_CLOSEST>'s, bit for bit, by the argument written above k_trace8_cam.  Whoever changes one loop changes both;
// tests/test_gpu_gbuffer.py compares the hit plane with pt_trace_device and the CPU checker.
struct GBufferArgs {
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    Bvh8Dev bvh;
    const float4* tri_nrm;   // per leaf triangle: geometric normal (pt_hit.ng)
    uint32_t* work;          // the packet counter, zero at launch
    QueryCounters* counters; // hits, one atomic per wave into slots 64 bytes apart; the traversal's stack-overflow bit
    int width, height;       // the frame: the planes are indexed Y * width + X
    v3 eye, U, V, W;         // the frame's camera (unused with views)
    const float* prev;       // [max(1, views)][12] eye, U, V, W of the previous frame; null when no motion plane is asked for
    float *hit, *depth, *position, *motion, *ray; // the planes, null = not asked for
};

// the camera of frame pixel (X, Y), its coordinates in that camera's image and the index of its previous camera (pixel_camera, pt_kernels.h)
struct GBufferCamera {
    uint32_t x, y, index;
    int width, height;
    v3 eye, U, V, W;
};
template <bool VIEWS>
PT_DEV GBufferCamera gbuffer_camera(const GBufferArgs& a, const ViewParams& vp, uint32_t X, uint32_t Y) {
    if (VIEWS) {
        const uint32_t vi = vp.vblock[(Y >> 3) * vp.nbx + (X >> 3)]; // the list holds view pixels only: never 0xffff
        const pt_view v = vp.views[vi];
        return GBufferCamera{X - (uint32_t)v.x, Y - (uint32_t)v.y, vi, v.width, v.height, mk3(v.eye[0], v.eye[1], v.eye[2]), mk3(v.U[0], v.U[1], v.U[2]),
                             mk3(v.V[0], v.V[1], v.V[2]), mk3(v.W[0], v.W[1], v.W[2])};
    }
    return GBufferCamera{X, Y, 0u, a.width, a.height, a.eye, a.U, a.V, a.W};
}

template <bool VIEWS>
__global__ void __launch_bounds__(64) k_gbuffer(GBufferArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    __shared__ uint2 s_grp[PT8_CAM_STACK];
    const uint32_t lane = threadIdx.x;
    const uint32_t n = a.n;
    const uint32_t npk = (n + 63u) >> 6;
    // work distribution as in k_trace8_cam: a static first grab, then `per` packets at a time from one counter, in image order
    uint32_t per = npk / (gridDim.x * 4u);
    per = per < 4u ? 4u : (per > 16u ? 16u : per);
    uint32_t pk = blockIdx.x * per, pk_end = pk + per;
    const ConstNode8 nodes = (ConstNode8)(uintptr_t)a.bvh.nodes;
    const ConstLeafTri tris = (ConstLeafTri)(uintptr_t)a.bvh.tris;
    uint32_t nhit = 0; // lane 0: hits of this wave's packets
    for (;;) {
        if (pk == pk_end) {
            uint32_t c = 0;
            if (lane == 0) c = atomicAdd(a.work, 1u);
            c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c) + gridDim.x;
            pk = c * per;
            pk_end = pk + per;
        }
        if (pk >= npk) break;
        const uint32_t pos = (pk << 6) + lane;
        ++pk;
        const bool valid = pos < n;
        // ---------------- the ray of the pixel's centre, in registers
        uint32_t xy = 0u;
        float4 o4 = make_float4(0.f, 0.f, 0.f, 1.f), d4 = make_float4(0.f, 0.f, 1.f, -1.f); // the neutral ray of a lane past the end
        if (valid) {
            xy = a.pixels[pos];
            const GBufferCamera cam = gbuffer_camera<VIEWS>(a, vp, pass_x(xy), pass_y(xy));
            const float dx = 2.0f * (((float)cam.x + 0.5f) / (float)cam.width) - 1.0f;
            const float dy = 2.0f * (((float)cam.y + 0.5f) / (float)cam.height) - 1.0f;
            const v3 dir = normalize3(add3(add3(scl3(cam.U, dx), scl3(cam.V, dy)), cam.W));
            o4 = make_float4(cam.eye.x, cam.eye.y, cam.eye.z, 0.001f);
            d4 = make_float4(dir.x, dir.y, dir.z, 1e16f);
        }
        // ---------------- the traversal of k_trace8_cam
        RaySetup r;
        r.o = mk3(o4.x, o4.y, o4.z);
        r.d = mk3(d4.x, d4.y, d4.z);
        r.idir = mk3(__builtin_amdgcn_rcpf(d4.x), __builtin_amdgcn_rcpf(d4.y), __builtin_amdgcn_rcpf(d4.z));
        r.dn = scl3(r.d, 1.0f / dot3(r.d, r.d));
        if (!(fabsf(d4.x) > 1e-30f)) r.idir.x = copysignf(1e30f, d4.x);
        if (!(fabsf(d4.y) > 1e-30f)) r.idir.y = copysignf(1e30f, d4.y);
        if (!(fabsf(d4.z) > 1e-30f)) r.idir.z = copysignf(1e30f, d4.z);
        const float tmin = o4.w;
        float best = d4.w; // tmax; a lane past the end holds -1: every box test fails
        int32_t bprim = -1, bleaf = -1;
        const uint32_t pm_lane = ((__float_as_uint(d4.z) >> 31) ? 0xF0u : 0x0Fu) | (((__float_as_uint(d4.y) >> 31) ? 0xCCu : 0x33u) << 8) |
                                 (((__float_as_uint(d4.x) >> 31) ? 0xAAu : 0x55u) << 16);
        const uint32_t pm = (uint32_t)__builtin_amdgcn_readfirstlane((int)pm_lane);
        const bool nx = r.idir.x < 0.0f, ny = r.idir.y < 0.0f, nz = r.idir.z < 0.0f;
        uint32_t g_base = 0u, g_imask = 1u, g_hits = 1u; // the root is slot 0 of a virtual parent
        int sp = 0;
        for (;;) {
            if (g_hits == 0u) {
                if (sp == 0) break;
                --sp;
                const uint2 e = s_grp[sp];
                g_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.x);
                const uint32_t e1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.y);
                g_imask = e1 & 0xffu;
                g_hits = e1 >> 8;
            }
            uint32_t h = g_hits, t = h & pm;
            h = t ? t : h;
            t = h & (pm >> 8);
            h = t ? t : h;
            t = h & (pm >> 16);
            h = t ? t : h; // a single bit
            g_hits ^= h;
            const uint32_t idx = g_base + (uint32_t)__popc(g_imask & (h - 1u));
            if (g_hits != 0u) {
                if (sp < PT8_CAM_STACK) s_grp[sp] = make_uint2(g_base, g_imask | (g_hits << 8)); // every lane writes the same value
                else atomicOr(&a.counters->fault, 1u);
                sp = sp < PT8_CAM_STACK ? sp + 1 : sp;
            }
            const float4 n0 = nodes[idx].n0, n1 = nodes[idx].n1, n2 = nodes[idx].n2, n3 = nodes[idx].n3, n4 = nodes[idx].n4;
            const NodeHdr nh = node_hdr(n0, n1);
            const uint32_t imask = nh.imask;
            const float ax = nh.sx * r.idir.x, ay = nh.sy * r.idir.y, az = nh.sz * r.idir.z;
            const float bx = (nh.ox - r.o.x) * r.idir.x, by = (nh.oy - r.o.y) * r.idir.y, bz = (nh.oz - r.o.z) * r.idir.z;
            const uint32_t lox0 = __float_as_uint(n2.x), lox1 = __float_as_uint(n2.y), loy0 = __float_as_uint(n2.z), loy1 = __float_as_uint(n2.w);
            const uint32_t loz0 = __float_as_uint(n3.x), loz1 = __float_as_uint(n3.y), hix0 = __float_as_uint(n3.z), hix1 = __float_as_uint(n3.w);
            const uint32_t hiy0 = __float_as_uint(n4.x), hiy1 = __float_as_uint(n4.y), hiz0 = __float_as_uint(n4.z), hiz1 = __float_as_uint(n4.w);
            const uint32_t nearx[2] = {nx ? hix0 : lox0, nx ? hix1 : lox1}, farx[2] = {nx ? lox0 : hix0, nx ? lox1 : hix1};
            const uint32_t neary[2] = {ny ? hiy0 : loy0, ny ? hiy1 : loy1}, fary[2] = {ny ? loy0 : hiy0, ny ? loy1 : hiy1};
            const uint32_t nearz[2] = {nz ? hiz0 : loz0, nz ? hiz1 : loz1}, farz[2] = {nz ? loz0 : hiz0, nz ? loz1 : hiz1};
            uint32_t miss = 0u;
#pragma unroll
            for (int s = 7; s >= 0; --s) {
                const int w = s >> 2, k = s & 3;
                const float tnx = __builtin_fmaf(u8f(nearx[w], k), ax, bx), tfx = __builtin_fmaf(u8f(farx[w], k), ax, bx);
                const float tny = __builtin_fmaf(u8f(neary[w], k), ay, by), tfy = __builtin_fmaf(u8f(fary[w], k), ay, by);
                const float tnz = __builtin_fmaf(u8f(nearz[w], k), az, bz), tfz = __builtin_fmaf(u8f(farz[w], k), az, bz);
                const float tn = fmaxf(fmaxf(tnx, tny), fmaxf(tnz, tmin));
                const float tf = fminf(fminf(tfx, tfy), fminf(tfz, best));
                miss = __builtin_amdgcn_alignbit(miss, __float_as_uint(tf - tn), 31u);
            }
            const uint32_t hm = miss ^ 0xffu; // this lane's hit mask in slot positions
            uint32_t whm = 0u;                // slots hit by any lane of the packet
#pragma unroll
            for (int s = 0; s < 8; ++s) whm |= __ballot((hm >> s) & 1u) != 0ull ? (1u << s) : 0u;
            // the node's leaf triangles first ...
            uint32_t lm = whm & ~imask;
            while (lm != 0u) {
                const uint32_t s = (uint32_t)__ffs((int)lm) - 1u;
                lm &= lm - 1u;
                const bool mine = (hm >> s) & 1u;
                const uint32_t cnt = leaf_count(nh.lbits, s), first_leaf = leaf_first(nh.tri_base, nh.lbits, s);
                for (uint32_t k = 0; k < cnt; ++k) {
                    const uint32_t leaf = first_leaf + k;
                    const float4 ta = tris[leaf].t0, tb = tris[leaf].t1, tc = tris[leaf].t2;
                    if (mine) {
                        float tt, det;
                        const v3 v0 = mk3(ta.x, ta.y, ta.z), v1 = mk3(ta.w, tb.x, tb.y), v2 = mk3(tb.z, tb.w, tc.x);
                        if (tri_test_det(r, v0, v1, v2, tt, det)) {
                            const int32_t prim = __float_as_int(tc.y);
                            if (tt > tmin && (tt < best || (tt == best && bprim >= 0 && prim < bprim)) && hit_in_box(r, v0, v1, v2, a.bvh.hit_pad, tt)) {
                                best = tt;
                                bprim = prim;
                                bleaf = (int32_t)leaf;
                            }
                        }
                    }
                }
            }
            // ... then its internal children
            g_base = nh.child_base;
            g_imask = imask;
            g_hits = whm & imask;
        }
        // ---------------- (best, bleaf) -> the planes; which planes are wanted is uniform for the launch
        const bool is_hit = valid && bleaf >= 0;
        if (valid) {
            const uint32_t X = pass_x(xy), Y = pass_y(xy);
            const size_t pi = (size_t)Y * (size_t)a.width + X;
            const v3 ray_o = r.o, ray_dir = r.d;
            if (a.ray) {
                float* w = a.ray + 8 * pi;
                gb_store4(w, o4);
                gb_store4(w + 4, d4);
            }
            if (a.hit) { // pt_hit by the expressions of k_hit_attributes (the only plane that fetches the triangle again)
                float4 ha = make_float4(best, 0.f, 0.f, __int_as_float(-1)); // t, u, v, prim
                float4 hb = make_float4(__int_as_float(-1), 0.f, 0.f, 0.f); // mesh, ng.xyz
                if (is_hit) {
                    const LeafTri tri = a.bvh.tris[bleaf];
                    const float4 tn = a.tri_nrm[bleaf];
                    const v3 v0 = mk3(tri.t0.x, tri.t0.y, tri.t0.z), v1 = mk3(tri.t0.w, tri.t1.x, tri.t1.y), v2 = mk3(tri.t1.z, tri.t1.w, tri.t2.x);
                    const v3 A = sub3(v0, ray_o), B = sub3(v1, ray_o), C = sub3(v2, ray_o);
                    const v3 CxB = cross3(C, B), AxC = cross3(A, C), BxA = cross3(B, A);
                    const float Uw = dot3(ray_dir, CxB), Vw = dot3(ray_dir, AxC), Ww = dot3(ray_dir, BxA);
                    const float det = Uw + Vw + Ww;
                    ha.y = Vw / det;
                    ha.z = Ww / det;
                    ha.w = tri.t2.y; // the primitive's bits
                    hb = make_float4(tri.t2.z /* the mesh's bits */, tn.x, tn.y, tn.z);
                }
                float* w = a.hit + 8 * pi;
                gb_store4(w, ha);
                gb_store4(w + 4, hb);
            }
            if (a.depth || a.position || a.motion) {
                // fetched again rather than kept in registers through the traversal
                const GBufferCamera cam = gbuffer_camera<VIEWS>(a, vp, X, Y);
                const v3 P = mk3(ray_o.x + best * ray_dir.x, ray_o.y + best * ray_dir.y, ray_o.z + best * ray_dir.z);
                if (a.depth) a.depth[pi] = is_hit ? best * dot3(ray_dir, normalize3(cam.W)) : __uint_as_float(0x7f800000u);
                if (a.position) gb_store4(a.position + 4 * pi, is_hit ? make_float4(P.x, P.y, P.z, 1.0f) : make_float4(0.f, 0.f, 0.f, 0.f));
                if (a.motion) {
                    // where this surface point was in the previous image, minus where it is now; a miss is a point at infinity
                    const float* pc = a.prev + 12u * cam.index;
                    const v3 pe = mk3(pc[0], pc[1], pc[2]), pU = mk3(pc[3], pc[4], pc[5]), pV = mk3(pc[6], pc[7], pc[8]), pW = mk3(pc[9], pc[10], pc[11]);
                    const v3 q = is_hit ? sub3(P, pe) : ray_dir;
                    const v3 VxW = cross3(pV, pW);
                    const float ma = dot3(q, VxW), mb = dot3(q, cross3(pW, pU)), mc = dot3(q, cross3(pU, pV)), mdet = dot3(pU, VxW);
                    float mx = (((ma / mc) + 1.0f) * 0.5f) * (float)cam.width - 0.5f;
                    float my = (((mb / mc) + 1.0f) * 0.5f) * (float)cam.height - 0.5f;
                    mx = mx - (float)cam.x;
                    my = my - (float)cam.y;
                    if (!(mc * mdet > 0.0f)) mx = my = __uint_as_float(0x7fc00000u); // behind the previous camera, on its plane, or not a number
                    gb_store2(a.motion + 2 * pi, make_float2(mx, my));
                }
            }
        }
        const unsigned long long hm64 = __ballot(is_hit);
        if (lane == 0) nhit += (uint32_t)__popcll(hm64);
    }
    if (lane == 0 && nhit) atomicAdd(&a.counters->slot[blockIdx.x & (PT_QUERY_SLOTS - 1u)].hits, (unsigned long long)nhit);
#endif
}
