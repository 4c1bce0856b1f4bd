// pt_motion_planes (include/pt_amd.h): where each pixel's surface point was before the geometry moved — the motion plane, the previous
// point and the previous normal that let pt_temporal_accumulate follow a moving mesh — in ONE kernel, stateless, every plane the caller's.
#pragma once
#include "pt_pass_dev.h"

// One thread per entry of the frame's pixel list, 256 threads per block, no LDS, no scratch: the shape of k_temporal.  A pixel reads its
// hit record (two 16-byte loads), three indices of the context's index array and nine floats of the caller's previous vertices; in
// 8x8-block order the lanes of a wave lie on few triangles, so the gathered vertices share cache lines.  It writes up to 56 bytes.
//
// The arithmetic is the header's, in the header's order, one float32 rounding per operation (-ffp-contract=off is part of the library's
// flags): float32 NumPy evaluating it reproduces every output bit (tests/motion_ref.py).  The camera lookup and the ray expression of a
// miss are k_gbuffer's, RESTATED rather than shared with it or with the frame path, for the reason written above k_gbuffer.  The primitive
// word of the hit plane is caller memory: it is compared with the triangle count before any address is formed from it.
struct MotionArgs {
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    int width, height;         // the frame: the planes are indexed Y * width + X
    const float* hit;          // this frame's hit plane
    const float* prev_vertices; // [vertices][3], the layout of pt_copy_vertices_device
    const uint32_t* idx;       // [triangles][3] global vertex indices (the context's)
    uint32_t ntri;
    v3 eye, U, V, W;           // the frame's camera (unused with views)
    const float* prev;         // [max(1, views)][12] eye, U, V, W of the previous frame; null when no motion plane is asked for
    float *motion, *prev_point, *prev_surface; // the planes, null = not asked for
    unsigned long long* counts; // [0] hits, [1] stale; zero at launch; one atomic per wave each
};

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_motion(MotionArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool is_hit = false, is_stale = false;
    if (i < a.n) {
        const uint32_t xy = a.pixels[i];
        const size_t p = (size_t)pass_y(xy) * (size_t)a.width + pass_x(xy);
        const float4 ha = tp_load4(a.hit + 8 * p), hb = tp_load4(a.hit + 8 * p + 4); // t, u, v, prim | mesh, ng.xyz
        const int32_t prim = __float_as_int(ha.w);
        const bool miss = hit_is_miss(ha.w);
        is_hit = !miss && (uint32_t)prim < a.ntri;
        is_stale = !miss && !is_hit;
        v3 Q = mk3(0.0f);
        float4 sb = hb; // the second half of prev_surface: mesh, previous normal
        if (is_hit) {
            const uint32_t i0 = a.idx[3u * (size_t)prim], i1 = a.idx[3u * (size_t)prim + 1], i2 = a.idx[3u * (size_t)prim + 2];
            const float *f0 = a.prev_vertices + 3 * (size_t)i0, *f1 = a.prev_vertices + 3 * (size_t)i1, *f2 = a.prev_vertices + 3 * (size_t)i2;
            const v3 p0 = mk3(f0[0], f0[1], f0[2]), p1 = mk3(f1[0], f1[1], f1[2]), p2 = mk3(f2[0], f2[1], f2[2]);
            const float u = ha.y, v = ha.z;
            const float w0 = (1.0f - u) - v;
            Q = mk3((p0.x * w0 + p1.x * u) + p2.x * v, (p0.y * w0 + p1.y * u) + p2.y * v, (p0.z * w0 + p1.z * u) + p2.z * v);
            const v3 ngp = normalize3(cross3(sub3(p1, p0), sub3(p2, p0)));
            sb = make_float4(hb.x, ngp.x, ngp.y, ngp.z);
        }
        if (a.prev_point) gb_store4(a.prev_point + 4 * p, is_hit ? make_float4(Q.x, Q.y, Q.z, 1.0f) : make_float4(0.f, 0.f, 0.f, 0.f));
        if (a.prev_surface) {
            float* w = a.prev_surface + 8 * p;
            gb_store4(w, is_stale ? make_float4(ha.x, 0.f, 0.f, __int_as_float(-1)) : ha);
            gb_store4(w + 4, is_stale ? make_float4(__int_as_float(-1), 0.f, 0.f, 0.f) : sb);
        }
        if (a.motion) {
            float mx = __uint_as_float(0x7fc00000u), my = mx;
            if (!is_stale) {
                // the pixel's camera: its view's or the frame's
                const PassPixel px = pass_pixel<VIEWS>(vp, xy, a.width, a.height);
                const uint32_t x = px.X - (uint32_t)px.x0, y = px.Y - (uint32_t)px.y0, ci = px.view;
                const int wr = px.wr, hr = px.hr;
                v3 eU = a.U, eV = a.V, eW = a.W;
                if (VIEWS) {
                    const pt_view& vw = vp.views[ci];
                    eU = mk3(vw.U[0], vw.U[1], vw.U[2]);
                    eV = mk3(vw.V[0], vw.V[1], vw.V[2]);
                    eW = mk3(vw.W[0], vw.W[1], vw.W[2]);
                }
                const float* pc = a.prev + 12u * ci;
                const v3 pe = mk3(pc[0], pc[1], pc[2]), pU = mk3(pc[3], pc[4], pc[5]), pV = mk3(pc[6], pc[7], pc[8]), pW = mk3(pc[9], pc[10], pc[11]);
                v3 q;
                if (is_hit) {
                    q = sub3(Q, pe);
                } else { // a miss is a point at infinity along the pixel's ray: the G-buffer's expression
                    const float dx = 2.0f * (((float)x + 0.5f) / (float)wr) - 1.0f;
                    const float dy = 2.0f * (((float)y + 0.5f) / (float)hr) - 1.0f;
                    q = normalize3(add3(add3(scl3(eU, dx), scl3(eV, dy)), eW));
                }
                const v3 VxW = cross3(pV, pW);
                const float ma = dot3(q, VxW), mb = dot3(q, cross3(pW, pU)), mc = dot3(q, cross3(pU, pV)), mdet = dot3(pU, VxW);
                mx = (((ma / mc) + 1.0f) * 0.5f) * (float)wr - 0.5f;
                my = (((mb / mc) + 1.0f) * 0.5f) * (float)hr - 0.5f;
                mx = mx - (float)x;
                my = my - (float)y;
                if (!(mc * mdet > 0.0f)) mx = my = __uint_as_float(0x7fc00000u); // behind the previous camera, on its plane, or not a number
            }
            gb_store2(a.motion + 2 * p, make_float2(mx, my));
        }
    }
    pass_tally(a.counts, {is_hit, is_stale});
#endif
}
