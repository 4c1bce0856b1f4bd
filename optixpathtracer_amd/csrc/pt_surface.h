// pt_surface_planes (include/pt_amd.h): the albedo and the texcoord under the centre of every pixel, from the hit plane alone — what the
// shade kernel's first hit would write to PT_BUF_ALBEDO for that barycentric point, for every pixel of the call and under this frame's
// camera, whether the render visited the pixel or not.  ONE kernel, stateless, every plane the caller's.
#pragma once
#include "pt_pass_dev.h"

// One thread per entry of the frame's pixel list, 256 threads per block, no scratch: the shape of k_motion.  Loads go cheapest first and
// each one decides whether the next is needed: the first 16 bytes of the hit record (t, u, v, prim; the second half — mesh, ng — is
// never read), on a hit in range the primitive's mesh (4 bytes of the context's own table) and the three colour words of its material
// (not the 104-byte record), and only on a textured mesh the primitive's 24 bytes of texcoords and the four texels (one 128-byte tile 7/8 * 3/4
// of the time, DevTex).  A miss stops after 16 bytes.  In 8x8-block order the lanes of a wave lie on few primitives and on neighbouring
// texels, so the gathers share cache lines.  It writes 16 + 8 bytes.
//
// TEX: the scene has a textured mesh.  The 256 values (float)b / 255.0f live in LDS (1 KiB), built once per workgroup as k_shade builds
// them; the untextured instantiation has no LDS, no barrier and no texcoord load.
//
// The arithmetic is the header's, in the header's order, one float32 rounding per operation (-ffp-contract=off is part of the library's
// flags); it is shade_path's texcoord expression with the hit record's own u, v, RESTATED here rather than shared with the frame path.
// The primitive word of the hit plane is caller memory: it is compared with the triangle count before any address is formed from it, and
// the mesh comes from the context's table, never from the record.
struct SurfaceArgs {
    const uint32_t* pixels; // x | y << 16 in frame coordinates, block order
    uint32_t n;
    int width;                  // the planes are indexed Y * width + X
    const float* hit;           // this frame's hit plane
    const uint32_t* tri_mesh;   // [triangles] the context's mesh of every primitive
    uint32_t ntri;
    const pt_material* mats;    // [meshes]
    const int32_t* mesh_tex;    // [meshes] texture id or -1 (TEX only)
    const float* prim_uv;       // [triangles][6], the caller's table (TEX only)
    const DevTex* textures;     // (TEX only)
    float *albedo, *texcoord;   // the planes, null = not asked for
    unsigned long long* counts; // [PASS_SLOTS][8]: [0] hits, [1] stale, [2] textured of a slot (pass_slot); zero at launch
};

template <bool TEX>
__global__ void __launch_bounds__(256) k_surface(SurfaceArgs a) {
#if __HIP_DEVICE_COMPILE__
    __shared__ float s_u8[TEX ? 256 : 1];
    if (TEX) {
        s_u8[threadIdx.x] = (float)threadIdx.x / 255.0f;
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool is_hit = false, is_stale = false, is_tex = false;
    if (i < a.n) {
        const uint32_t xy = a.pixels[i];
        const size_t p = (size_t)pass_y(xy) * (size_t)a.width + pass_x(xy);
        const float4 ha = tp_load4(a.hit + 8 * p); // t, u, v, prim
        const int32_t prim = __float_as_int(ha.w);
        const bool miss = hit_is_miss(ha.w);
        is_hit = !miss && (uint32_t)prim < a.ntri;
        is_stale = !miss && !is_hit;
        float4 alb = make_float4(0.f, 0.f, 0.f, 1.0f);
        float2 tc = make_float2(0.f, 0.f);
        if (is_hit) {
            const uint32_t mesh = a.tri_mesh[prim];
            const float* col = a.mats[mesh].color;
            int tid = -1;
            if (TEX) tid = a.mesh_tex[mesh];
            if (TEX && tid >= 0) {
                is_tex = true;
                float c[6]; // uv0.xy, uv1.xy, uv2.xy
                __builtin_memcpy(c, a.prim_uv + 6 * (size_t)prim, 24);
                const float u = ha.y, v = ha.z;
                const float w0 = (1.0f - u) - v;
                const float s = ((w0 * c[0]) + (u * c[2])) + (v * c[4]);
                const float t = ((w0 * c[1]) + (u * c[3])) + (v * c[5]);
                const float4 tx = tex2d_wrap_linear(a.textures[tid], s, t, s_u8);
                alb = make_float4(tx.x, tx.y, tx.z, 1.0f);
                tc = make_float2(s, t);
            } else {
                alb = make_float4(col[0], col[1], col[2], 1.0f);
            }
        }
        if (a.albedo) gb_store4(a.albedo + 4 * p, alb);
        if (a.texcoord) gb_store2(a.texcoord + 2 * p, tc);
    }
    pass_tally(pass_slot(a.counts), {is_hit, is_stale, is_tex}); // is_tex: never without TEX
#endif
}
