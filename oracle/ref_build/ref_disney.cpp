// ref_disney.cpp — thin extern "C" shims over the REFERENCE's Disney BSDF (Disney.cuh:151-426) and
// ProbeData::BuildCDF (Probe.h:29-77), compiled from where they lie under /root/reference (never copied).
// Test infrastructure: builds oracle/_ref/libptref_disney.so (glibc transcendentals) and, with
// -DREF_DETMATH, oracle/_ref/libptref_disney_det.so (include/pt_detmath.h transcendentals, the ones the
// HIP kernels use).  tests/golden/make_disney_golden.py records their outputs in tests/golden/ref_disney.npz.
//
// Disney.cuh and Probe.h include <optix.h> (through LaunchParams.h and CUDABuffer.h), which the image lacks.
// ref_build/stub/ holds stand-ins of our own: a type declaration (OptixTraversableHandle), three no-op
// CUDA/OptiX check macros, an empty optix_stubs.h and the Windows case-insensitive lookup of "Maths.h".
// None of the functions pinned here reaches them.  deviceProgram.cu is built by a TU of its own, ref_device.cpp,
// over a dispatch-only stand-in for <optix_device.h> and the checker's ray search.
//
// Kept apart from ref_driver.cpp so that that TU's include resolution (and tests/golden/ref_tables.npz) is unchanged.
#include <cfloat>
#include <cmath>
#include <algorithm>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <cuda_runtime.h>
using std::max; using std::min; using std::abs; using std::isfinite;
// As in ref_driver.cpp: under nvcc the reference's unqualified calls on float arguments bind to CUDA's float
// overloads; make the same overloads visible so that g++ does not bind them to the double versions.
using std::sqrt; using std::tan; using std::acos; using std::atan2; using std::exp; using std::log; using std::fabs;
#ifdef REF_DETMATH
// The det flavour: every transcendental the pinned headers call goes to include/pt_detmath.h, as in the HIP
// kernels and the checker's liborc_det.so.  System headers are all in before these macros.
#include "../../include/pt_detmath.h"
#define sinf pt_sinf
#define cosf pt_cosf
#define logf pt_logf
#define expf pt_expf
#define powf pt_powf
#define acosf pt_acosf
#define atan2f pt_atan2f
// unqualified sin(x) / cos(x) on floats (maths.h:259): a using-declaration would be ambiguous with the global
// float overloads CUDA's host headers declare, so these are function-like macros
#define sin(x) pt_sinf(x)
#define cos(x) pt_cosf(x)
namespace ref_det {
static inline float pow(float x, float y) { return pt_powf(x, y); }
}
using ref_det::pow;
#else
using std::cos; using std::sin; using std::pow;
#endif
#include "Disney.cuh"     // HelloPathtracing_original/Disney.cuh (-> maths.h, sample.h, LaunchParams.h, Material.h)
#include "Probe.h"        // HelloPathtracing_original/Probe.h (-> CUDABuffer.h)

static float3 f3(const float* p) { return make_float3(p[0], p[1], p[2]); }
static Material mat_of(const void* m) {
    static_assert(sizeof(Material) == 104, "Material layout (Material.h:11-69)");
    Material r;
    memcpy(&r, m, sizeof(Material));
    return r;
}

extern "C" {
// Disney.cuh:151-192
float ref_bsdf_pdf(const void* mat, float etaI, float etaO, const float N[3], const float V[3], const float L[3]) {
    const Material m = mat_of(mat);
    return BSDFPdf(m, etaI, etaO, make_float3(0.0f), f3(N), f3(V), f3(L));
}
// Disney.cuh:317-426; albedo is a parameter of its own there (deviceProgram.cu passes the texture-modulated colour)
void ref_bsdf_eval(const void* mat, const float albedo[3], float etaI, float etaO, const float N[3], const float V[3], const float L[3], float out[3]) {
    const Material m = mat_of(mat);
    const float3 r = BSDFEval(m, f3(albedo), etaI, etaO, make_float3(0.0f), f3(N), f3(V), f3(L));
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}
// BasisFromVector(N) (maths.h:94-108), Random(seed) (maths.h:174-178), BSDFSample (Disney.cuh:196-314).  L starts at
// zero and is left so when the refraction branch finds total internal reflection (pdf 0).
void ref_bsdf_sample(const void* mat, float etaI, float etaO, const float N[3], const float V[3], uint32_t seed, float L[3], float* pdf, uint32_t st[2]) {
    const Material m = mat_of(mat);
    const float3 n = f3(N);
    float3 u, v, light = make_float3(0.0f);
    BasisFromVector(n, &u, &v);
    Random r(seed);
    BSDFType type;
    BSDFSample(m, etaI, etaO, make_float3(0.0f), u, v, n, f3(V), light, *pdf, type, r);
    L[0] = light.x; L[1] = light.y; L[2] = light.z;
    st[0] = r.seed1; st[1] = r.seed2;
}
// Probe.h:29-77 on a (h, w, 4) float image
void ref_build_cdf(const float* data, int width, int height, float* pdfX, float* cdfX, float* pdfY, float* cdfY) {
    ProbeData p;
    p.width = width; p.height = height;
    p.data = (Color*)data;
    p.BuildCDF();
    const size_t n = (size_t)width * height;
    memcpy(pdfX, p.pdfValuesX, sizeof(float) * n);
    memcpy(cdfX, p.cdfValuesX, sizeof(float) * n);
    memcpy(pdfY, p.pdfValuesY, sizeof(float) * height);
    memcpy(cdfY, p.cdfValuesY, sizeof(float) * height);
    delete[] p.pdfValuesX; delete[] p.cdfValuesX; delete[] p.pdfValuesY; delete[] p.cdfValuesY;
}
}
