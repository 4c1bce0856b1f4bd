// pt_edge_aa_planes (include/pt_amd.h): geometric edge antialiasing from the hit plane — ONE kernel, stateless, every plane the caller's.
// Where a pixel and one of its four neighbours show different surfaces, the nearer surface's triangle is intersected with the centre ray of
// the pixel on the other side: the barycentric that changes sign between the two centres says where the triangle's edge crosses the line
// between them, and a pixel whose own half of that line is crossed takes a share of the neighbour's colour.
#pragma once
#include "pt_pass_dev.h"

// One thread per entry of the frame's pixel list, 256 per block, no scratch, no LDS: the shape of k_upsample.  The list is in 8x8-block
// order, so a wave is one block and its 5-point stencil is the block and four copies of it displaced by one pixel: 56 of the 64 neighbour
// words of a direction are some other lane's own record, and the eight beyond the block's border lie in lines a neighbouring wave reads.
// The reuse is left to L1/L2 (profiles/edge_aa.md has what they leave of it).
//
// Loads go cheapest first.  Every pixel: its 16 bytes of colour, the first 16 bytes of its hit record, and the primitive word (4 bytes) of
// each reachable neighbour.  A pixel whose four neighbours show its own primitive (or that is a miss among misses) stops there — no
// position, no normal, no vertex, no camera — and stores its colour.  Only the others load the second half of their record, their position
// and their view's camera, and then per direction, each only while the direction is still alive: the neighbour's colour (16 bytes), the
// second half of its record, its position, the first half of its record (t, u, v) when both are hits, and at last the owner's three
// indices and nine floats of the context's CURRENT vertices.
//
// The arithmetic is the header's, in the header's order, one float32 rounding per operation (-ffp-contract=off is part of the library's
// flags); the camera lookup is k_motion's, RESTATED.  The primitive words of the hit plane are caller memory: the owner's is compared with
// the triangle count before any address is formed from it.  A neighbour's address is formed only after pass_reachable has placed it inside
// the pixel's rectangle, which lies inside the frame.
struct EdgeAaArgs {
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    int width, height;      // the frame: the planes are indexed Y * width + X
    const float *color, *hit, *position;
    const uint32_t* idx;    // [triangles][3] global vertex indices
    const float* verts;     // [vertices][3] the context's current vertices
    uint32_t ntri;
    v3 eye, U, V, W;        // the frame's camera (unused with views)
    float* out;
    float* edge;            // or null
    uint32_t* frame;        // or null
    const uint8_t* inset;   // [nbx * nby] 1 = the block belongs to the call's set (owned by the rank, named by the mask)
    uint32_t nbx;
    float normal_cos, plane_eps;
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] hits, [1] stale, [2] boundary, [3] blended of a slot (pass_slot); zero at launch
};

// Step 3 of the header for one direction: dist, the place of the owner's edge on the line from p's centre (0) to q's centre (1), or a NaN
// where the direction is dropped.  o_is_p: p owns the edge; oa: the first half of the owner's record (t, u, v, prim); (xr, yr): the local
// coordinates of r, the pixel of the pair that is not the owner.
PT_DEV float ea_dist(const EdgeAaArgs& a, bool o_is_p, float4 oa, int xr, int yr, float fw, float fh, v3 eye, v3 eU, v3 eV, v3 eW) {
    const float nan = __uint_as_float(0x7fc00000u);
    const uint32_t prim = __float_as_uint(oa.w);
    if (!(prim < a.ntri)) return nan; // a stale owner (a miss never owns)
    const uint32_t i0 = a.idx[3u * (size_t)prim], i1 = a.idx[3u * (size_t)prim + 1], i2 = a.idx[3u * (size_t)prim + 2];
    const float *f0 = a.verts + 3 * (size_t)i0, *f1 = a.verts + 3 * (size_t)i1, *f2 = a.verts + 3 * (size_t)i2;
    const v3 p0 = mk3(f0[0], f0[1], f0[2]), p1 = mk3(f1[0], f1[1], f1[2]), p2 = mk3(f2[0], f2[1], f2[2]);
    const v3 e1 = sub3(p1, p0), e2 = sub3(p2, p0), nrm = cross3(e1, e2);
    const float nn = dot3(nrm, nrm), hgt = dot3(nrm, sub3(p0, eye));
    const v3 dr = lod_ray(eU, eV, eW, (float)xr + 0.5f, (float)yr + 0.5f, fw, fh);
    const float t_r = hgt / dot3(nrm, dr);
    if (!(t_r > 0.0f)) return nan; // parallel, behind the eye, a zero-area primitive (0 / 0)
    const v3 g = sub3(add3(scl3(dr, t_r), eye), p0);
    const float u_r = dot3(cross3(g, e2), nrm) / nn, v_r = dot3(cross3(e1, g), nrm) / nn;
    const float br[3] = {(1.0f - u_r) - v_r, u_r, v_r};
    const float bo[3] = {fl_max0((1.0f - oa.y) - oa.z), fl_max0(oa.y), fl_max0(oa.z)};
    float s = nan;
    bool any = false;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (br[i] < 0.0f) { // a NaN fails
            const float si = bo[i] / (bo[i] - br[i]);
            if (!any || si < s) s = si; // a NaN never replaces, and a first NaN is never replaced
            any = true;
        }
    return o_is_p ? s : 1.0f - s; // no crossing: NaN
}

template <bool VIEWS>
__global__ void __launch_bounds__(256) k_edge_aa(EdgeAaArgs a, ViewParams vp) {
#if __HIP_DEVICE_COMPILE__
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool is_hit = false, is_stale = false, is_boundary = false, is_blended = false;
    if (i < a.n) {
        const PassPixel px = pass_pixel<VIEWS>(vp, a.pixels[i], a.width, a.height);
        const int X = (int)px.X, Y = (int)px.Y;
        const size_t pi = (size_t)Y * (size_t)a.width + (size_t)X;
        const float4 c = tp_load4(a.color + 4 * pi);
        const float4 ha = tp_load4(a.hit + 8 * pi); // t, u, v, prim
        const int32_t prim = __float_as_int(ha.w);
        const bool miss = hit_is_miss(ha.w);
        is_hit = !miss && (uint32_t)prim < a.ntri;
        is_stale = !miss && !is_hit;
        float4 o = make_float4(c.x, c.y, c.z, 1.0f);
        float2 e = make_float2(0.0f, 0.0f);
        if (tp_finite(c.x) && tp_finite(c.y) && tp_finite(c.z)) {
            // ---------------- 2a. the four primitive words: which directions can still be candidates
            uint32_t alive = 0u, qmisses = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int qx = X + (k == 0 ? -1 : k == 1 ? 1 : 0), qy = Y + (k == 2 ? -1 : k == 3 ? 1 : 0);
                if (pass_reachable(px, a.inset, a.nbx, qx, qy)) {
                    const int32_t qprim = __float_as_int(a.hit[8 * ((size_t)qy * (size_t)a.width + (size_t)qx) + 3]);
                    const bool qmiss = qprim < 0;
                    if (qmiss) qmisses |= 1u << k;
                    if (!(miss && qmiss) && !(!miss && !qmiss && qprim == prim)) alive |= 1u << k;
                }
            }
            if (alive) {
                // ---------------- the pixel's side of the surface test, and its camera
                SurfaceKey key = surface_key(miss, ha.x, make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f), a.plane_eps);
                if (!miss) key = surface_key(false, ha.x, tp_load4(a.hit + 8 * pi + 4), tp_load4(a.position + 4 * pi), a.plane_eps);
                v3 eye = a.eye, eU = a.U, eV = a.V, eW = a.W;
                if (VIEWS) {
                    const pt_view& vw = vp.views[px.view];
                    eye = mk3(vw.eye[0], vw.eye[1], vw.eye[2]);
                    eU = mk3(vw.U[0], vw.U[1], vw.U[2]);
                    eV = mk3(vw.V[0], vw.V[1], vw.V[2]);
                    eW = mk3(vw.W[0], vw.W[1], vw.W[2]);
                }
                const float fw = (float)px.wr, fh = (float)px.hr;
                const int x = X - px.x0, y = Y - px.y0;
                float wbest = 0.0f;
                int kbest = -1;
                v3 cbest = mk3(0.0f);
#pragma unroll 1
                for (int k = 0; k < 4; ++k) {
                    if (!((alive >> k) & 1u)) continue;
                    const int dx = k == 0 ? -1 : k == 1 ? 1 : 0, dy = k == 2 ? -1 : k == 3 ? 1 : 0;
                    const size_t q = (size_t)(Y + dy) * (size_t)a.width + (size_t)(X + dx);
                    // ---------------- 2b. the rest of the candidate test
                    const float4 cq = tp_load4(a.color + 4 * q);
                    if (!(tp_finite(cq.x) && tp_finite(cq.y) && tp_finite(cq.z))) continue;
                    const bool qmiss = (qmisses >> k) & 1u;
                    if (!miss && !qmiss && same_facet(key, a.hit, q, a.normal_cos) && same_plane(key, a.position, q)) continue;
                    is_boundary = true;
                    // ---------------- 3. the owner and the crossing
                    bool o_is_p = qmiss;
                    float4 oa = ha;
                    if (!miss) {
                        if (!qmiss) {
                            const float4 qa = tp_load4(a.hit + 8 * q);
                            o_is_p = ha.x <= qa.x; // a NaN gives q
                            if (!o_is_p) oa = qa;
                        }
                    } else {
                        oa = tp_load4(a.hit + 8 * q);
                    }
                    const float dist = ea_dist(a, o_is_p, oa, o_is_p ? x + dx : x, o_is_p ? y + dy : y, fw, fh, eye, eU, eV, eW);
                    if (dist < 0.5f) { // a NaN fails
                        const float w = 0.5f - dist;
                        if (w > wbest) { // ---------------- 4. the strongest direction, the first of equals
                            wbest = w;
                            kbest = k;
                            cbest = mk3(cq.x, cq.y, cq.z);
                        }
                    }
                }
                if (kbest >= 0) {
                    is_blended = true;
                    o = make_float4(c.x + (cbest.x - c.x) * wbest, c.y + (cbest.y - c.y) * wbest, c.z + (cbest.z - c.z) * wbest, 1.0f);
                    e = make_float2(wbest, (float)(kbest + 1));
                }
            }
        }
        gb_store4(a.out + 4 * pi, o);
        if (a.edge) gb_store2(a.edge + 2 * pi, e);
        if (a.frame) a.frame[pi] = make_color(mk3(o.x, o.y, o.z));
    }
    pass_tally(pass_slot(a.counts), {is_hit, is_stale, is_boundary, is_blended});
#endif
}
