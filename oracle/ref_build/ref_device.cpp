// ref_device.cpp — runs the REFERENCE's own device programs on the host: __raygen__renderFrame, __closesthit__radiance,
// __miss__radiance, the occlusion programs, SampleLights and SampleShadow of <variant>/deviceProgram.cu, included below from
// where it lies in the reference tree (never copied).  Test infrastructure: `make -C oracle ref` builds one library per
// variant directory and math flavour, oracle/_ref/libptref_device_<variant>{,_det}.so (glibc transcendentals / with
// -DREF_DETMATH those of include/pt_detmath.h, as ref_disney.cpp); tests/golden/make_ref_frames.py records their frames in
// tests/golden/ref_frames.npz.
//
// Which behaviour comes from where:
//   hit, t, (u, v)   OURS.  A ray's closest / any hit is the checker's own search, called through the function pointers given
//                    to ref_set_search (orc_trace_closest, orc_trace_any, orc_trace_any_cull, orc_hit_barycentrics):
//                    DESIGN.md §2 (tri_test_det + hit_in_box, lowest primitive on ties), tested there against brute force and
//                    double precision.  Nothing here pins OptiX's intersector.
//   texture filter   OURS, unpinned as before: tex2D<float4> forwards to orc_tex2d.
//   dispatch         the reference's host code, SimplePathtracer.cpp: ray type 0 binds __closesthit__radiance / __anyhit__radiance,
//                    ray type 1 __closesthit__occlusion / __anyhit__occlusion (:320-331), the miss programs are __miss__radiance
//                    and __miss__occlusion in that order (:287, :296), every triangle input has flags 0 so any-hit programs run
//                    (:510), one SBT record per mesh with the mesh's material, buffers and texture (:429-449), launch
//                    params filled as at :57 and :168-179.  The two payload words, the launch index, the ray, t, the
//                    primitive index, the SBT pointer and the barycentrics travel through ref_build/stub/optix_device.h.
//                    The SBT records point into the flattened vertex / index / texcoord arrays of the whole model and the
//                    primitive index is the model-wide one, so sbtData.index[prim] and sbtData.vertex[i] read the mesh's own data.
//   everything else  the REFERENCE's: sample loop, jitter, RNG stream order, the RadiancePRD state machine, MIS weight,
//                    composition, clamp, lerp, AOVs, the foveated variants' remap / annulus / splat / tone map.
//
// Build with clang++ (oracle/Makefile).  `make_float2(rnd(seed), rnd(seed))` (deviceProgram.cu:388 and the same line of
// every variant) depends on the evaluation order of function arguments, which C++ leaves unspecified: clang evaluates left to
// right (x jitter first: what the kernels and the checker assume of nvcc), g++ right to left.
// ref_device_compiler() lets the tests refuse a library built otherwise.
#include <cfloat>
#include <cmath>
#include <algorithm>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <vector>
#include <cuda_runtime.h>
using std::max; using std::min; using std::abs; using std::isfinite;
// as in ref_disney.cpp: the float overloads nvcc would bind the reference's unqualified calls to
using std::sqrt; using std::tan; using std::acos; using std::atan2; using std::exp; using std::log; using std::fabs;
#ifdef REF_DETMATH
#include "../../include/pt_detmath.h"
#define sinf pt_sinf
#define cosf pt_cosf
#define logf pt_logf
#define expf pt_expf
#define powf pt_powf
#define acosf pt_acosf
#define atan2f pt_atan2f
#define sin(x) pt_sinf(x)
#define cos(x) pt_cosf(x)
#define pow(x, y) pt_powf(x, y)
#else
using std::cos; using std::sin; using std::pow;
#endif
#include <optix_device.h>  // ref_build/stub/optix_device.h
thread_local RefTraceRecord ref_rec;

#include "deviceProgram.cu"  // <variant>/deviceProgram.cu: the only -I of the reference's program directories is the variant's own

// ---- the checker's search and texture filter (addresses of its C functions; no Python runs per ray)
typedef void (*closest_fn)(const void* scene, const float* rays, int n, float* t, int32_t* prim);
typedef void (*any_fn)(const void* scene, const float* rays, int n, uint8_t* occ);
typedef void (*bary_fn)(const void* scene, const float* ray, uint32_t prim, float uv[2]);
typedef void (*tex2d_fn)(const uint32_t* pix, int w, int h, float s, float t, float out[4]);
static closest_fn g_closest;
static any_fn g_any, g_any_cull;
static bary_fn g_bary;
static tex2d_fn g_tex2d;

struct RefTexture { const uint32_t* pixel; int w, h; };
struct RefScene {
    const void* orc_scene;
    const uint32_t* tri_mesh;
    std::vector<TriangleMeshSBTData> sbt;  // one record per mesh (SimplePathtracer.cpp:429-449)
    std::vector<RefTexture> tex;
};

template <> float4 tex2D<float4>(cudaTextureObject_t tex, float s, float t) {
    const RefTexture* x = (const RefTexture*)tex;
    float out[4];
    g_tex2d(x->pixel, x->w, x->h, s, t, out);
    return make_float4(out[0], out[1], out[2], out[3]);
}

// ---- branch counters: what the reference's programs did, observed from outside through the payload's RadiancePRD
enum {
    C_PRIMARY_MISS, C_SECONDARY_MISS, C_SHADOW_OCCLUDED, C_SHADOW_UNOCCLUDED, C_CATCHER_PASS_THROUGH, C_BSDF_PDF_LE_0, C_TRANSMISSION,
    C_DEPTH_CUTOFF, C_EMISSION_PRIMARY, C_TEXTURED_HIT, C_CLAMP_ACTIVE, C_COUNT
};
static thread_local uint64_t g_count[C_COUNT];
static thread_local bool g_counting;
static thread_local bool g_path_open;  // the last radiance ray of the current path came back without RAY_STATE_FLAGS_DONE
static inline void count(int which) { if (g_counting) ++g_count[which]; }
// a path that ends (the next camera ray, or the end of the thread) while it is open was stopped by the depth cutoff: the
// raygen loop has no other exit (deviceProgram.cu:429)
static inline void close_path() { if (g_path_open) count(C_DEPTH_CUTOFF); g_path_open = false; }

void ref_trace(OptixTraversableHandle handle, float3 o, float3 d, float tmin, float tmax, unsigned int flags, unsigned int sbt_offset,
               unsigned int miss_index, unsigned int* p0, unsigned int* p1) {
    const RefScene* sc = (const RefScene*)handle;
    const RefTraceRecord saved = ref_rec;  // closest-hit calls traceOcclusion: the record nests
    ref_rec.origin = o;
    ref_rec.direction = d;
    ref_rec.payload[0] = *p0;
    ref_rec.payload[1] = *p1;
    const float ray[8] = {o.x, o.y, o.z, tmin, d.x, d.y, d.z, tmax};
    if (sbt_offset == RAY_TYPE_RADIANCE) {
        RadiancePRD* prd = (RadiancePRD*)unpackPointer(*p0, *p1);
        const bool secondary = (prd->stateFlags & RAY_STATE_FLAGS_SECONDARY_RAY) != 0;
        if (!secondary) close_path();
        float t;
        int32_t prim;
        g_closest(sc->orc_scene, ray, 1, &t, &prim);
        if (prim >= 0) {
            const TriangleMeshSBTData& rec = sc->sbt[sc->tri_mesh[prim]];
            ref_rec.t = t;
            ref_rec.primitive = (unsigned int)prim;
            ref_rec.sbt_data = &rec;
            float uv[2];
            g_bary(sc->orc_scene, ray, (uint32_t)prim, uv);
            ref_rec.barycentrics = make_float2(uv[0], uv[1]);
            const bool catcher = (rec.material.flags & MATERIAL_FLAG_SHADOW_CATCHER) != 0;
            __anyhit__radiance();
            __closesthit__radiance();
            if (catcher && secondary) {
                count(C_CATCHER_PASS_THROUGH);
            } else {
                if (rec.hasTexture && rec.texcoord) count(C_TEXTURED_HIT);
                if (!secondary && (rec.material.emission.x != 0.0f || rec.material.emission.y != 0.0f || rec.material.emission.z != 0.0f))
                    count(C_EMISSION_PRIMARY);
                if (prd->stateFlags & RAY_STATE_FLAGS_DONE) {
                    if (prd->bsdfPdf <= 0.0f) count(C_BSDF_PDF_LE_0);
                } else if (dot(prd->direction, prd->normal) <= 0.0f) {
                    count(C_TRANSMISSION);
                }
            }
        } else {
            ref_rec.t = tmax;
            if (miss_index == RAY_TYPE_RADIANCE) __miss__radiance(); else __miss__occlusion();
            count(secondary ? C_SECONDARY_MISS : C_PRIMARY_MISS);
        }
        g_path_open = (prd->stateFlags & RAY_STATE_FLAGS_DONE) == 0;
    } else {
        // Any-hit programs are enabled (geometry flags 0).  __anyhit__occlusion neither ignores nor terminates, so it runs for
        // at least one hit inside (tmin, tmax) whenever there is one, then __closesthit__occlusion for the hit traversal ends
        // with; with OPTIX_RAY_FLAG_TERMINATE_ON_FIRST_HIT that is the first one accepted.  Otherwise the miss program runs.
        uint8_t occ;
        ((flags & OPTIX_RAY_FLAG_CULL_BACK_FACING_TRIANGLES) ? g_any_cull : g_any)(sc->orc_scene, ray, 1, &occ);
        if (occ) {
            __anyhit__occlusion();
            __closesthit__occlusion();
            count(C_SHADOW_OCCLUDED);
        } else {
            if (miss_index == RAY_TYPE_OCCLUSION) __miss__occlusion(); else __miss__radiance();
            count(C_SHADOW_UNOCCLUDED);
        }
    }
    *p0 = ref_rec.payload[0];
    *p1 = ref_rec.payload[1];
    ref_rec = saved;
}

// ---- C interface
struct RefFrame {
    int32_t width, height;
    uint32_t subframe_index, samples_per_launch;
    float eye[3], U[3], V[3], W[3];
    uint32_t launch_w, launch_h;  // optixLaunch dimensions (the original launches width x height)
    // the foveated variants' frame fields (LaunchParams.h of sv, sv2, sv3, sv4_vmv23); ignored by the original
    uint32_t factor_x, factor_y;
    int32_t fill_size;
    uint32_t cx, cy;
    float r_inner, r_outer;
    uint32_t offset_x, offset_y, redraw;
};
struct RefProbe {
    int32_t width, height;
    const float *data, *pdfX, *cdfX, *pdfY, *cdfY;
};
static float3 f3(const float* p) { return make_float3(p[0], p[1], p[2]); }

static void launch(uint32_t lw, uint32_t lh) {
    for (uint32_t y = 0; y < lh; ++y)
        for (uint32_t x = 0; x < lw; ++x) {
            ref_rec = RefTraceRecord();
            ref_rec.launch_index = make_uint3(x, y, 0);
            g_path_open = false;
            __raygen__renderFrame();
            close_path();
        }
}

extern "C" {
const char* ref_device_compiler() {
#if defined(__clang__)
    return "clang " __clang_version__;
#elif defined(__GNUC__)
    return "gcc " __VERSION__;
#else
    return "unknown";
#endif
}
const char* ref_device_variant() { return REF_VARIANT_NAME; }
int ref_device_detmath() {
#ifdef REF_DETMATH
    return 1;
#else
    return 0;
#endif
}
int ref_device_foveated() {
#ifdef REF_FOVEATED
    return 1;
#else
    return 0;
#endif
}
int ref_device_num_counters() { return C_COUNT; }

void ref_set_search(void* closest, void* any, void* any_cull, void* bary, void* tex2d) {
    g_closest = (closest_fn)closest; g_any = (any_fn)any; g_any_cull = (any_fn)any_cull; g_bary = (bary_fn)bary; g_tex2d = (tex2d_fn)tex2d;
}

// verts / idx / texcoord: the flattened arrays of the whole model (texcoord may be null); tri_mesh[ntri]: mesh of a triangle;
// mats: nmesh Materials of 104 bytes; mesh_tex[nmesh]: texture id or -1; mesh_has_uv[nmesh].  All arrays are borrowed.
void* ref_scene_create(const void* orc_scene, const float* verts, const uint32_t* idx, const uint32_t* tri_mesh, const void* mats, uint32_t nmesh,
                       const float* texcoord, const int32_t* mesh_tex, const uint8_t* mesh_has_uv, uint32_t ntex, const uint32_t* const* pixels,
                       const int32_t* widths, const int32_t* heights) {
    static_assert(sizeof(Material) == 104, "Material layout (Material.h)");
    RefScene* sc = new RefScene;
    sc->orc_scene = orc_scene;
    sc->tri_mesh = tri_mesh;
    sc->tex.resize(ntex);
    for (uint32_t k = 0; k < ntex; ++k) sc->tex[k] = RefTexture{pixels[k], widths[k], heights[k]};
    sc->sbt.resize(nmesh);
    for (uint32_t m = 0; m < nmesh; ++m) {
        TriangleMeshSBTData& r = sc->sbt[m];
        memcpy(&r.material, (const char*)mats + 104 * (size_t)m, 104);
        r.vertex = (float3*)verts;
        r.normal = nullptr;  // never read by the device programs
        r.index = (uint3*)idx;
        r.texcoord = (texcoord && mesh_has_uv && mesh_has_uv[m]) ? (float2*)texcoord : nullptr;  // an empty CUDABuffer's d_pointer() is null (:447, :488)
        const int tid = mesh_tex ? mesh_tex[m] : -1;
        r.hasTexture = tid >= 0;  // :436-443
        r.texture = tid >= 0 ? (cudaTextureObject_t)&sc->tex[tid] : 0;
    }
    return sc;
}
void ref_scene_destroy(void* sc) { delete (RefScene*)sc; }

// One optixLaunch(launch_w, launch_h, 1), launch indices in row order on one thread.  accum is read and written, the other
// buffers written; counters[ref_device_num_counters()] are added to.
void ref_render(void* scene, const RefProbe* probe, const RefFrame* f, float* accum, uint32_t* frame, float* normal, float* color, float* albedo,
                uint64_t* counters) {
    LaunchParams& p = params;
    p = LaunchParams();
    p.frame.accum_buffer = (float4*)accum;
    p.frame.frame_buffer = (uchar4*)frame;
    p.frame.color_buffer = (float4*)color;
    p.frame.normal_buffer = (float4*)normal;
    p.frame.albedo_buffer = (float4*)albedo;
    p.frame.size = make_int2(f->width, f->height);
    p.frame.subframe_index = f->subframe_index;
#ifdef REF_FOVEATED
    p.frame.factor = make_uint3(f->factor_x, f->factor_y, 1);
    p.frame.fillSize = f->fill_size;
    p.frame.c = make_uint2(f->cx, f->cy);
    p.frame.r_inner = f->r_inner;
    p.frame.r_outer = f->r_outer;
    p.frame.offset = make_uint2(f->offset_x, f->offset_y);
    p.frame.redraw = f->redraw;
    const bool blends = f->subframe_index > 0 && !f->redraw;
#else
    const bool blends = f->subframe_index > 0;
#endif
    p.camera.eye = f3(f->eye);
    p.camera.U = f3(f->U);
    p.camera.V = f3(f->V);
    p.camera.W = f3(f->W);
    p.samples_per_launch = f->samples_per_launch;
    p.traversable = (OptixTraversableHandle)scene;
    p.probe.width = probe->width;
    p.probe.height = probe->height;
    p.probe.data = (Color*)probe->data;
    p.probe.offset = make_float3(0.0f);
    p.probe.pdfValuesX = (float*)probe->pdfX;
    p.probe.cdfValuesX = (float*)probe->cdfX;
    p.probe.pdfValuesY = (float*)probe->pdfY;
    p.probe.cdfValuesY = (float*)probe->cdfY;

    memset(g_count, 0, sizeof(g_count));
    g_counting = true;
    launch(f->launch_w, f->launch_h);
    g_counting = false;
    if (blends) {
        // "clamp active": the unclamped colour is a local of the raygen program.  A second launch into scratch buffers whose
        // previous accumulation is zero leaves lerp(0, clamped, a) = a * clamped, which is a * 10 exactly where the clamp bit.
        const size_t n = (size_t)f->width * f->height;
        std::vector<float> s_accum(4 * n, 0.0f), s_normal(4 * n), s_color(4 * n), s_albedo(4 * n);
        std::vector<uint32_t> s_frame(n);
        p.frame.accum_buffer = (float4*)s_accum.data();
        p.frame.frame_buffer = (uchar4*)s_frame.data();
        p.frame.color_buffer = (float4*)s_color.data();
        p.frame.normal_buffer = (float4*)s_normal.data();
        p.frame.albedo_buffer = (float4*)s_albedo.data();
        launch(f->launch_w, f->launch_h);
        const float a = 1.0f / static_cast<float>(f->subframe_index + 1);
        const float top = 0.0f + a * (10.0f - 0.0f);
        for (size_t i = 0; i < n; ++i)
            if (s_accum[4 * i] == top || s_accum[4 * i + 1] == top || s_accum[4 * i + 2] == top) ++g_count[C_CLAMP_ACTIVE];
    }
    for (int k = 0; k < C_COUNT; ++k) counters[k] += g_count[k];
}
}
