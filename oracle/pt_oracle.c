/* pt_oracle.c — CPU restatement of the reference's optixLaunch hot path.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, the smoke check in
 * __graft_entry__.py and bench.py's cpu_baseline leg may load it; the product
 * (optixpathtracer_amd/, libptamd.so) never does.
 *
 * What it restates (reference = bipul-mohanto/OptixPathTracer, paths relative to
 * /root/reference; canonical variant HelloPathtracing_original/):
 *   cuda/random.h:34-99           tea<4>, lcg, rnd
 *   maths.h:94-108,144-275        BasisFromVector, SafeNormalize, Luminance, Random, samplers
 *   sample.h:252-258              Sample2D (USE_RANDOM=1)
 *   Probe.cuh:38-67,119-169       ProbeDirToUV, ProbeUVToDir, ProbeEval, LowerBound, ProbeSample
 *   Probe.h:29-77                 ProbeData::BuildCDF
 *   Disney.cuh:35-97,125-147,151-426  Refract, Fresnel, GTR1/2, SmithGGX, BSDFPdf/Sample/Eval (+Lambert)
 *   Material.h:11-69              Material layout, GetIndexOfRefraction
 *   deviceProgram.cu:209-594      miss, SampleLights, SampleShadow, raygen loop, closest-hit
 *   cuda/helpers.h:34-61          toSRGB, quantizeUnsigned8Bits, make_color
 *   toneMap.cu:41-58              computeFinalPixelColorsKernel
 *   sutil/Camera.cpp:34-45        Camera::UVWFrame
 *   sutil/vec_math.h:96-122,483-570  lerp, clamp, dot, cross, normalize, faceforward, float3/float
 * The ray-triangle search itself (optixTrace, closed-source OptiX 7.5 driver code,
 * call sites deviceProgram.cu:165,190) is restated as a brute-force loop / a
 * median-split BVH over a sign-consistent (watertight across shared edges) triangle test;
 * closest hit of a ray against a triangle soup is uniquely defined up to ties,
 * which are broken by lowest primitive index.
 *
 * PINNING STATUS.  RNG, samplers, probe lookup/sampling, make_color, Material
 * defaults/IOR and UVWFrame are pinned against the reference's own headers
 * compiled from where they lie (oracle/ref_build -> oracle/_ref, tests/golden).
 * So are the Disney BSDF (BSDFPdf/Sample/Eval) and BuildCDF: Disney.cuh and
 * Probe.h need optix.h, and oracle/ref_build/stub/ supplies stand-ins that only
 * declare OptixTraversableHandle, no-op the CUDA/OptiX check macros and redirect
 * "Maths.h" as Windows' case-insensitive lookup does; no pinned function reaches
 * them (ref_build/ref_disney.cpp, tests/golden/ref_disney.npz).  deviceProgram.cu
 * needs optixTrace and the payload calls, which a stand-in would define rather
 * than pin: for the raygen/closest-hit orchestration PARITY IS UNPINNED — it is
 * restated from reading the source, line by line.
 *
 * Math modes: built twice.  Default uses glibc sinf/cosf/acosf/atan2f/logf/powf
 * (independent of the product).  With -DORC_DETMATH it uses include/pt_detmath.h
 * so that its bits equal the HIP kernels' bits (see that header).
 * Compile with -ffp-contract=off.
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifdef ORC_DETMATH
#include "../include/pt_detmath.h"
#define M_SIN pt_sinf
#define M_COS pt_cosf
#define M_ACOS pt_acosf
#define M_ATAN2 pt_atan2f
#define M_LOG pt_logf
#define M_POW pt_powf
#define M_EXP pt_expf
#else
#define M_SIN sinf
#define M_COS cosf
#define M_ACOS acosf
#define M_ATAN2 atan2f
#define M_LOG logf
#define M_POW powf
#define M_EXP expf
#endif

/* ---------------------------------------------------------------- vec helpers
 * sutil/vec_math.h semantics; evaluation order kept left-to-right. */
typedef struct { float x, y, z; } f3;
static inline f3 mk3(float x, float y, float z) { f3 r = {x, y, z}; return r; }
static inline f3 mk3s(float s) { return mk3(s, s, s); }
static inline f3 add3(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline f3 sub3(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline f3 mul3(f3 a, f3 b) { return mk3(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline f3 scl3(f3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }
static inline f3 neg3(f3 a) { return mk3(-a.x, -a.y, -a.z); }
/* vec_math.h:483-487 float3/float = a * (1/s) */
static inline f3 div3s(f3 a, float s) { float inv = 1.0f / s; return scl3(a, inv); }
/* vec_math.h:535-538 */
static inline float dot3(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
/* vec_math.h:541-544 */
static inline f3 cross3(f3 a, f3 b) { return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
/* vec_math.h:553-557 */
static inline f3 normalize3(f3 v) { float invLen = 1.0f / sqrtf(dot3(v, v)); return scl3(v, invLen); }
/* vec_math.h:96-99, 500-503: a + t*(b-a) */
static inline float lerpf(float a, float b, float t) { return a + t * (b - a); }
static inline f3 lerp3(f3 a, f3 b, float t) { return add3(a, scl3(sub3(b, a), t)); }
/* vec_math.h:119-122 */
static inline float clampf(float f, float a, float b) { return fmaxf(a, fminf(f, b)); }
/* vec_math.h:567-570 */
static inline f3 faceforward3(f3 n, f3 i, f3 nref) { return scl3(n, copysignf(1.0f, dot3(i, nref))); }

#define kPi (3.141592653589793f)
#define k2Pi (3.141592653589793f * 2.0f)
#define kInvPi (1.0f / kPi)
#define kInv2Pi (1.0f / k2Pi)

/* ---------------------------------------------------------------- RNG */
/* cuda/random.h:34-49 */
uint32_t orc_tea4(uint32_t val0, uint32_t val1) {
    uint32_t v0 = val0, v1 = val1, s0 = 0;
    for (int n = 0; n < 4; n++) {
        s0 += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    return v0;
}
/* cuda/random.h:53-59 */
uint32_t orc_lcg(uint32_t* prev) {
    *prev = 1664525u * (*prev) + 1013904223u;
    return *prev & 0x00FFFFFFu;
}
/* cuda/random.h:96-99 */
float orc_rnd(uint32_t* prev) { return (float)orc_lcg(prev) / (float)0x01000000; }

/* maths.h:170-225 */
typedef struct { uint32_t seed1, seed2; } orc_random;
void orc_random_init(orc_random* r, uint32_t seed) {
    r->seed1 = 315645664u + seed;
    r->seed2 = r->seed1 ^ 0x13ab45feu;
}
uint32_t orc_rand(orc_random* r) {
    r->seed1 = (r->seed2 ^ ((r->seed1 << 5) | (r->seed1 >> 27))) ^ (r->seed1 * r->seed2);
    r->seed2 = r->seed1 ^ ((r->seed2 << 12) | (r->seed2 >> 20));
    return r->seed1;
}
float orc_randf(orc_random* r) {
    uint32_t value = orc_rand(r);
    uint32_t limit = 0xffffffffu;
    return clampf((float)value * (1.0f / (float)limit), 0.f, 0.999999f);
}
/* maths.h:211-215 Randf(min,max) */
static inline float randf_mm(orc_random* r, float mn, float mx) {
    float t = orc_randf(r);
    return (1.0f - t) * mn + t * mx;
}
/* sample.h:252-258 */
static inline void sample2d(orc_random* r, float* u1, float* u2) {
    *u1 = randf_mm(r, 0.0f, 1.0f);
    *u2 = randf_mm(r, 0.0f, 1.0f);
}

/* maths.h:94-108.  `1.0 / sqrt(float)` is a double division of a float-valued
 * sqrtf; rounding it to float equals 1.0f/sqrtf() (double rounding is innocuous
 * for p=53 >= 2*24+2), so it is written in float. */
static inline void basis_from_vector(f3 w, f3* u, f3* v) {
    if (fabsf(w.x) > fabsf(w.y)) {
        float invLen = 1.0f / sqrtf(w.x * w.x + w.z * w.z);
        *u = mk3(-w.z * invLen, 0.0f, w.x * invLen);
    } else {
        float invLen = 1.0f / sqrtf(w.y * w.y + w.z * w.z);
        *u = mk3(0.0f, w.z * invLen, -w.y * invLen);
    }
    *v = cross3(w, *u);
}
/* maths.h:144-156 */
static inline f3 safe_normalize(f3 a) {
    float m = dot3(a, a);
    if (m > 0.0f) return scl3(a, 1.0f / sqrtf(m));
    return mk3s(0.0f);
}
/* maths.h:241-252 */
static inline f3 uniform_sample_hemisphere(orc_random* r) {
    float z = randf_mm(r, 0.0f, 1.0f);
    float w = sqrtf(1.0f - z * z);
    float phi = k2Pi * randf_mm(r, 0.0f, 1.0f);
    float x = M_COS(phi) * w;
    float y = M_SIN(phi) * w;
    return mk3(x, y, z);
}
/* maths.h:254-275 */
static inline f3 cosine_sample_hemisphere(float u1, float u2) {
    float r = sqrtf(u1);
    float theta = k2Pi * u2;
    float sx = r * M_COS(theta), sy = r * M_SIN(theta);
    float z = sqrtf(fmaxf(0.0f, 1.0f - sx * sx - sy * sy));
    return mk3(sx, sy, z);
}

/* ---------------------------------------------------------------- material */
/* Material.h:11-69 — same field order, 104 bytes */
typedef struct {
    float emission[3], color[3], absorption[3];
    float eta, metallic, subsurface, specular, roughness, specularTint, anisotropic, sheen, sheenTint, clearcoat,
        clearcoatGloss, transmission;
    float bump, bumpTile[3];
    int flags;
} orc_material;
#define MATERIAL_FLAG_SHADOW_CATCHER 1

/* Material.h:13-37 defaults */
void orc_material_default(orc_material* m) {
    memset(m, 0, sizeof(*m));
    m->color[0] = m->color[1] = m->color[2] = 0.6f;
    m->specular = 0.5f;
    m->roughness = 1.0f;
    m->clearcoatGloss = 1.0f;
    m->bumpTile[0] = m->bumpTile[1] = m->bumpTile[2] = 10.0f;
}
/* Material.h:39-45 */
float orc_material_ior(const orc_material* m) {
    if (m->eta == 0.0f) return 2.0f / (1.0f - sqrtf(0.08f * m->specular)) - 1.0f;
    return m->eta;
}

/* ---------------------------------------------------------------- Disney BSDF */
static inline float sqrf(float a) { return a * a; }
/* Disney.cuh:35-48 */
static inline int refract(f3 wi, f3 n, float eta, f3* wt) {
    float cosThetaI = dot3(n, wi);
    float sin2ThetaI = fmaxf(0.0f, 1.0f - cosThetaI * cosThetaI);
    float sin2ThetaT = eta * eta * sin2ThetaI;
    if (sin2ThetaT >= 1) return 0;
    float cosThetaT = sqrtf(1.0f - sin2ThetaT);
    *wt = add3(scl3(neg3(wi), eta), scl3(n, eta * cosThetaI - cosThetaT));
    return 1;
}
/* Disney.cuh:50-55 */
static inline float schlick_fresnel(float u) {
    float m = clampf(1 - u, 0.0f, 1.0f);
    float m2 = m * m;
    return m2 * m2 * m;
}
/* Disney.cuh:57-63 */
static inline float gtr1(float NDotH, float a) {
    if (a >= 1) return kInvPi;
    float a2 = a * a;
    float t = 1 + (a2 - 1) * NDotH * NDotH;
    return (a2 - 1) / (kPi * M_LOG(a2) * t);
}
/* Disney.cuh:65-70 */
static inline float gtr2(float NDotH, float a) {
    float a2 = a * a;
    float t = 1.0f + (a2 - 1.0f) * NDotH * NDotH;
    return a2 / (kPi * t * t);
}
/* Disney.cuh:72-77 */
static inline float smith_ggx(float NDotv, float alphaG) {
    float a = alphaG * alphaG;
    float b = NDotv * NDotv;
    return 1 / (NDotv + sqrtf(a + b - a * b));
}
/* Disney.cuh:80-97 */
static inline float fresnel_dielectric(float VDotN, float etaI, float etaT) {
    float SinThetaT2 = sqrf(etaI / etaT) * (1.0f - VDotN * VDotN);
    if (SinThetaT2 > 1.0f) return 1.0f;
    float LDotN = sqrtf(1.0f - SinThetaT2);
    float eta = etaT / etaI;
    float r1 = (VDotN - eta * LDotN) / (VDotN + eta * LDotN);
    float r2 = (LDotN - eta * VDotN) / (LDotN + eta * VDotN);
    return 0.5f * (sqrf(r1) + sqrf(r2));
}

enum { BSDF_DISNEY = 0, BSDF_LAMBERT = 1 };

/* Disney.cuh:151-192 (Lambert: :127-133) */
static float bsdf_pdf(int mode, const orc_material* mat, float etaI, float etaO, f3 n, f3 V, f3 L) {
    if (mode == BSDF_LAMBERT) return (dot3(L, n) <= 0.0f) ? 0.0f : kInv2Pi;
    if (dot3(L, n) <= 0.0f) {
        float bsdfPdf = 0.0f;
        float brdfPdf = kInv2Pi * mat->subsurface * 0.5f;
        return lerpf(brdfPdf, bsdfPdf, mat->transmission);
    } else {
        float F = fresnel_dielectric(dot3(n, V), etaI, etaO);
        const float a = fmaxf(0.001f, mat->roughness);
        const f3 half = safe_normalize(add3(L, V));
        const float cosThetaHalf = fabsf(dot3(half, n));
        const float pdfHalf = gtr2(cosThetaHalf, a) * cosThetaHalf;
        float pdfSpec = 0.25f * pdfHalf / fmaxf(1.e-6f, dot3(L, half));
        float pdfDiff = fabsf(dot3(L, n)) * kInvPi * (1.0f - mat->subsurface);
        float bsdfPdf = pdfSpec * F;
        float brdfPdf = lerpf(pdfDiff, pdfSpec, 0.5f);
        return lerpf(brdfPdf, bsdfPdf, mat->transmission);
    }
}

/* GGX half-vector sample shared by Disney.cuh:207-225 and :286-307 */
static inline f3 sample_ggx_reflect(const orc_material* mat, f3 U, f3 V, f3 N, f3 view, float r1, float r2) {
    const float a = fmaxf(0.001f, mat->roughness);
    const float phiHalf = r1 * k2Pi;
    const float cosThetaHalf = sqrtf((1.0f - r2) / (1.0f + (sqrf(a) - 1.0f) * r2));
    const float sinThetaHalf = sqrtf(fmaxf(0.0f, 1.0f - sqrf(cosThetaHalf)));
    const float sinPhiHalf = M_SIN(phiHalf);
    const float cosPhiHalf = M_COS(phiHalf);
    f3 half = add3(add3(scl3(U, sinThetaHalf * cosPhiHalf), scl3(V, sinThetaHalf * sinPhiHalf)), scl3(N, cosThetaHalf));
    if (dot3(half, view) <= 0.0f) half = scl3(half, -1.0f);
    /* 2.0f * dot(view, half) * half - view */
    return sub3(scl3(half, 2.0f * dot3(view, half)), view);
}

/* Disney.cuh:196-314 (Lambert: :135-142) */
static void bsdf_sample(int mode, const orc_material* mat, float etaI, float etaO, f3 U, f3 V, f3 N, f3 view, f3* light,
                        float* pdf, orc_random* rand) {
    if (mode == BSDF_LAMBERT) {
        f3 d = uniform_sample_hemisphere(rand);
        *light = add3(add3(scl3(U, d.x), scl3(V, d.y)), scl3(N, d.z));
        *pdf = kInv2Pi;
        return;
    }
    if (orc_randf(rand) < mat->transmission) {
        float F = fresnel_dielectric(dot3(N, view), etaI, etaO);
        if (orc_randf(rand) < F) {
            float r1, r2;
            sample2d(rand, &r1, &r2);
            *light = sample_ggx_reflect(mat, U, V, N, view, r1, r2);
        } else {
            float eta = etaI / etaO;
            if (refract(view, N, eta, light)) {
                *pdf = (1.0f - F) * mat->transmission;
                return;
            } else {
                *pdf = 0.0f;
                return;
            }
        }
    } else {
        float r1, r2;
        sample2d(rand, &r1, &r2);
        if (orc_randf(rand) < 0.5f) {
            if (orc_randf(rand) < mat->subsurface) {
                const f3 d = uniform_sample_hemisphere(rand);
                *light = sub3(add3(scl3(U, d.x), scl3(V, d.y)), scl3(N, d.z));
            } else {
                const f3 d = cosine_sample_hemisphere(r1, r2);
                *light = add3(add3(scl3(U, d.x), scl3(V, d.y)), scl3(N, d.z));
            }
        } else {
            *light = sample_ggx_reflect(mat, U, V, N, view, r1, r2);
        }
    }
    *pdf = bsdf_pdf(mode, mat, etaI, etaO, N, view, *light);
}

/* Disney.cuh:317-426 (Lambert: :144-147).  The reference's bare double literals
 * (.3 .6 .1 at :328, .08 at :331, 0.5 at :397) promote those sub-expressions to
 * FP64; kept where it can change the float result (products with non-float
 * constants), dropped where double rounding is provably innocuous (:397). */
static f3 bsdf_eval(int mode, const orc_material* mat, f3 albedo, float etaI, float etaO, f3 N, f3 V, f3 L) {
    if (mode == BSDF_LAMBERT) return scl3(albedo, kInvPi);
    float NDotL = dot3(N, L);
    float NDotV = dot3(N, V);
    f3 H = normalize3(add3(L, V));
    float NDotH = dot3(N, H);
    float LDotH = dot3(L, H);
    f3 Cdlin = albedo;
    float Cdlum = (float)(.3 * (double)Cdlin.x + .6 * (double)Cdlin.y + .1 * (double)Cdlin.z);
    f3 Ctint = Cdlum > 0.0f ? div3s(Cdlin, Cdlum) : mk3s(1.0f);
    float spec08 = (float)((double)mat->specular * .08);
    f3 Cspec0 = lerp3(scl3(lerp3(mk3s(1.0f), Ctint, mat->specularTint), spec08), Cdlin, mat->metallic);
    f3 bsdf = mk3s(0.0f);
    f3 brdf = mk3s(0.0f);
    if (mat->transmission > 0.0f) {
        if (NDotL <= 0) {
            float F = fresnel_dielectric(NDotV, etaI, etaO);
            bsdf = mk3s(mat->transmission * (1.0f - F) / fabsf(NDotL) * (1.0f - mat->metallic));
        } else {
            float a = fmaxf(0.001f, mat->roughness);
            float Ds = gtr2(NDotH, a);
            float FH = fresnel_dielectric(LDotH, etaI, etaO);
            f3 Fs = lerp3(Cspec0, mk3s(1.0f), FH);
            float Gs = smith_ggx(NDotV, a) * smith_ggx(NDotL, a);
            bsdf = scl3(scl3(Fs, Gs), Ds); /* Gs * Fs * Ds */
        }
    }
    if (mat->transmission < 1.0f) {
        if (NDotL <= 0) {
            if (mat->subsurface > 0.0f) {
                f3 s = mk3(sqrtf(mat->color[0]), sqrtf(mat->color[1]), sqrtf(mat->color[2]));
                float FL = schlick_fresnel(fabsf(NDotL)), FV = schlick_fresnel(NDotV);
                float Fd = (1.0f - 0.5f * FL) * (1.0f - 0.5f * FV);
                /* kInvPi * s * subsurface * Fd * (1-metallic) */
                brdf = scl3(scl3(scl3(scl3(s, kInvPi), mat->subsurface), Fd), 1.0f - mat->metallic);
            }
        } else {
            float a = fmaxf(0.001f, mat->roughness);
            float Ds = gtr2(NDotH, a);
            float FH = schlick_fresnel(LDotH);
            f3 Fs = lerp3(Cspec0, mk3s(1.f), FH);
            float Gs = smith_ggx(NDotV, a) * smith_ggx(NDotL, a);
            float FL = schlick_fresnel(NDotL), FV = schlick_fresnel(NDotV);
            float Fd90 = 0.5f + 2.0f * LDotH * LDotH * mat->roughness;
            float Fd = lerpf(1.0f, Fd90, FL) * lerpf(1.0f, Fd90, FV);
            float Dr = gtr1(NDotH, lerpf(.1f, .001f, mat->clearcoatGloss));
            float Fc = lerpf(.04f, 1.0f, FH);
            float Gr = smith_ggx(NDotL, .25f) * smith_ggx(NDotV, .25f);
            /* kInvPi*Fd*Cdlin*(1-metallic)*(1-subsurface) + Gs*Fs*Ds + clearcoat*Gr*Fc*Dr */
            f3 diff = scl3(scl3(scl3(Cdlin, kInvPi * Fd), 1.0f - mat->metallic), 1.0f - mat->subsurface);
            f3 spec = scl3(scl3(Fs, Gs), Ds);
            float cc = mat->clearcoat * Gr * Fc * Dr;
            brdf = add3(add3(diff, spec), mk3s(cc));
        }
    }
    return lerp3(brdf, bsdf, mat->transmission);
}

/* ---------------------------------------------------------------- probe */
typedef struct {
    int width, height;
    const float* data; /* RGBA float4, row-major */
    const float *pdfX, *cdfX, *pdfY, *cdfY;
} orc_probe;

/* maths.h:165-168 */
static inline float luminance(const float* c) { return c[0] * 0.3f + c[1] * 0.6f + c[2] * 0.1f; }

/* Probe.h:29-77 — sequential float running sums, exactly as written */
void orc_build_cdf(const float* data, int width, int height, float* pdfX, float* cdfX, float* pdfY, float* cdfY) {
    float totalWeightY = 0.0f;
    for (int j = 0; j < height; ++j) {
        float totalWeightX = 0.0f;
        for (int i = 0; i < width; ++i) {
            float weight = luminance(&data[4 * ((size_t)j * width + i)]);
            totalWeightX += weight;
            pdfX[(size_t)j * width + i] = weight;
            cdfX[(size_t)j * width + i] = totalWeightX;
        }
        float invTotalWeightX = 1.0f / totalWeightX;
        for (int i = 0; i < width; ++i) {
            pdfX[(size_t)j * width + i] *= invTotalWeightX;
            cdfX[(size_t)j * width + i] *= invTotalWeightX;
        }
        totalWeightY += totalWeightX;
        pdfY[j] = totalWeightX;
        cdfY[j] = totalWeightY;
    }
    for (int j = 0; j < height; ++j) {
        cdfY[j] /= totalWeightY;
        pdfY[j] /= totalWeightY;
    }
}

/* Probe.cuh:38-46 */
void orc_probe_dir_to_uv(const float dir[3], float uv[2]) {
    float theta = M_ACOS(clampf(dir[1], -1.0f, 1.0f));
    float phi = (dir[0] == 0.0f && dir[2] == 0.0f) ? 0.0f : M_ATAN2(dir[2], dir[0]);
    uv[0] = (kPi + phi) * kInvPi * 0.5f;
    uv[1] = theta * kInvPi;
}
/* Probe.cuh:48-58 */
void orc_probe_uv_to_dir(const float uv[2], float dir[3]) {
    float theta = uv[1] * kPi;
    float phi = uv[0] * 2.0f * kPi;
    dir[0] = -M_SIN(theta) * M_COS(phi);
    dir[1] = M_COS(theta);
    dir[2] = -M_SIN(theta) * M_SIN(phi);
}
static inline int clampi(int v, int a, int b) { return v < a ? a : (v > b ? b : v); }
/* Probe.cuh:61-67 */
void orc_probe_eval(const orc_probe* p, const float uv[2], float rgba[4]) {
    int px = clampi((int)(uv[0] * p->width), 0, p->width - 1);
    int py = clampi((int)(uv[1] * p->height), 0, p->height - 1);
    memcpy(rgba, &p->data[4 * ((size_t)py * p->width + px)], 16);
}
/* Probe.cuh:69-93: pdf (solid angle) with which ProbeSample draws direction d.  Unused by the reference's device code (the MIS term of
 * __miss__radiance that called it is commented out, deviceProgram.cu:214-224); restated and pinned for completeness. */
float orc_probe_pdf(const orc_probe* p, const float d[3]) {
    float uv[2];
    orc_probe_dir_to_uv(d, uv);
    int col = clampi((int)(uv[0] * p->width), 0, p->width - 1);
    int row = clampi((int)(uv[1] * p->height), 0, p->height - 1);
    float pdf = p->pdfX[(size_t)row * p->width + col] * p->pdfY[row];
    float sinTheta = M_SIN(uv[1] * kPi);
    if (fabsf(sinTheta) < 0.0001f)
        pdf = 0.0f;
    else
        pdf *= (float)p->width * (float)p->height / (2.0f * kPi * kPi * sinTheta);
    return pdf;
}
/* Probe.cuh:119-136 */
static inline int lower_bound(const float* array, int lower, int upper, float value) {
    while (lower < upper) {
        int mid = lower + (upper - lower) / 2;
        if (array[mid] < value)
            lower = mid + 1;
        else
            upper = mid;
    }
    return lower;
}
/* Probe.cuh:138-169.  row==height / col==width are unreachable for a valid CDF
 * (Randf <= .999999 < last CDF entry) but clamped so a degenerate probe cannot
 * read out of bounds. */
static void probe_sample(const orc_probe* p, f3* dir, f3* color, float* pdf, orc_random* rand) {
    float r1, r2;
    sample2d(rand, &r1, &r2);
    int row = lower_bound(p->cdfY, 0, p->height, r1);
    if (row > p->height - 1) row = p->height - 1;
    int col = lower_bound(p->cdfX, row * p->width, (row + 1) * p->width, r2) - row * p->width;
    if (col > p->width - 1) col = p->width - 1;
    const float* px = &p->data[4 * ((size_t)row * p->width + col)];
    *color = mk3(px[0], px[1], px[2]);
    *pdf = p->pdfX[(size_t)row * p->width + col] * p->pdfY[row];
    float u = col / (float)p->width;
    float v = row / (float)p->height;
    float sinTheta = M_SIN(v * kPi);
    if (sinTheta == 0.0f)
        *pdf = 0.0f;
    else
        *pdf *= p->width * p->height / (2.0f * kPi * kPi * sinTheta);
    float uv[2] = {u, v}, d[3];
    orc_probe_uv_to_dir(uv, d);
    *dir = mk3(d[0], d[1], d[2]);
}
void orc_probe_sample(const orc_probe* p, uint32_t seed, float dir[3], float color[3], float* pdf, uint32_t state_out[2]) {
    orc_random r;
    orc_random_init(&r, seed);
    f3 d, c;
    probe_sample(p, &d, &c, pdf, &r);
    dir[0] = d.x; dir[1] = d.y; dir[2] = d.z;
    color[0] = c.x; color[1] = c.y; color[2] = c.z;
    state_out[0] = r.seed1; state_out[1] = r.seed2;
}

/* ---------------------------------------------------------------- output transforms */
/* cuda/helpers.h:34-61 */
static inline uint8_t quantize8(float x) {
    x = clampf(x, 0.0f, 1.0f);
    uint32_t q = (uint32_t)(x * 256.0f);
    return (uint8_t)(q < 255u ? q : 255u);
}
static inline float to_srgb1(float c) {
    float invGamma = 1.0f / 2.4f;
    float powed = M_POW(c, invGamma);
    return c < 0.0031308f ? 12.92f * c : 1.055f * powed - 0.055f;
}
uint32_t orc_make_color(const float c[3]) {
    uint8_t r = quantize8(to_srgb1(clampf(c[0], 0.0f, 1.0f)));
    uint8_t g = quantize8(to_srgb1(clampf(c[1], 0.0f, 1.0f)));
    uint8_t b = quantize8(to_srgb1(clampf(c[2], 0.0f, 1.0f)));
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | (255u << 24);
}
/* toneMap.cu:41-58: clamp(sqrt(f4)) * 255.9 packed r | g<<8 | b<<16 | a<<24 */
void orc_tonemap_sqrt(const float* rgba, uint32_t* out, int n) {
    for (int i = 0; i < n; ++i) {
        uint32_t ch[4];
        for (int k = 0; k < 4; ++k) {
            float f = sqrtf(rgba[4 * i + k]);
            f = fminf(1.0f, fmaxf(0.0f, f));
            ch[k] = (uint32_t)(255.9f * f);
        }
        out[i] = ch[0] | (ch[1] << 8) | (ch[2] << 16) | (ch[3] << 24);
    }
}

/* sutil/Camera.cpp:34-45 (tanf: host libm in both math modes — the product's
 * host facade calls the same libm, and U,V,W are inputs to the device path) */
void orc_uvw_frame(const float eye[3], const float lookat[3], const float up[3], float fovY, float aspect, float U[3],
                   float V[3], float W[3]) {
    f3 w = sub3(mk3(lookat[0], lookat[1], lookat[2]), mk3(eye[0], eye[1], eye[2]));
    float wlen = sqrtf(dot3(w, w));
    f3 u = normalize3(cross3(w, mk3(up[0], up[1], up[2])));
    f3 v = normalize3(cross3(u, w));
    float vlen = wlen * tanf(0.5f * fovY * 3.14159265358979323846f / 180.0f);
    v = scl3(v, vlen);
    float ulen = vlen * aspect;
    u = scl3(u, ulen);
    U[0] = u.x; U[1] = u.y; U[2] = u.z;
    V[0] = v.x; V[1] = v.y; V[2] = v.z;
    W[0] = w.x; W[1] = w.y; W[2] = w.z;
}

/* ---------------------------------------------------------------- scene + ray search */
typedef struct {
    float lo[3], hi[3];
    uint32_t left, right; /* internal: child node ids; leaf: right==0xffffffff, left=first, count in `count` */
    uint32_t count;
} onode;

typedef struct {
    uint32_t nv, ntri, nmesh;
    float* verts;       /* nv*3 */
    uint32_t* idx;      /* ntri*3 */
    uint32_t* tri_mesh; /* ntri */
    orc_material* mats; /* nmesh */
    int has_catcher;
    /* textures: per-vertex texcoords (or NULL), per-mesh texture id (-1 none) and uv flag */
    float* texcoord;    /* nv*2 or NULL */
    int32_t* mesh_tex;  /* nmesh */
    uint8_t* mesh_has_uv;
    struct { uint32_t* pixel; int w, h; }* tex;
    uint32_t ntex;
    /* optional BVH */
    int use_bvh;
    onode* nodes;
    uint32_t nnodes;
    uint32_t* order; /* leaf-order primitive ids */
    float pad;
    /* optional: the PRODUCT's 8-wide compressed tree, exported through pt_export_bvh (include/pt_amd.h documents the 80-byte
     * node and the 48-byte leaf triangle).  When set, closest_hit / any_hit_c traverse it with a scalar stack traversal: the
     * "scalar C++ CPU traversal of the same BVH" north_star asks for beside the GPU number, and an independent check that the
     * tree the GPU kernels walk holds every triangle. */
    const uint32_t* n8;    /* nnodes8 * 20 words */
    const float* t8;       /* ntris8 * 12 floats: v0.xyz v1.xyz v2.xyz, prim bits, mesh bits, 1 unused */
    uint32_t nnodes8, ntris8;
} orc_scene;

typedef struct {
    f3 o, d, dn;
    float hp; /* half the scene's box padding: see wtri2 */
} wray;

/* per-ray constants of the triangle test: dn = d / dot(d,d) so that t is in units of d */
static inline void wray_init(wray* r, f3 o, f3 d) {
    r->o = o;
    r->d = d;
    float inv_dd = 1.0f / dot3(d, d);
    r->dn = scl3(d, inv_dd);
    r->hp = 0.0f;
}

/* Sign-consistent scalar-triple-product ray/triangle test.  With A,B,C the vertices relative to the
 * ray origin, U = d.(CxB), V = d.(AxC), W = d.(BxA) are the (unnormalised) barycentric weights; the
 * edge function of a shared edge is the exact negation in the neighbouring triangle (products
 * commute, differences negate exactly), so no ray slips between two triangles that share an edge —
 * the property the RT-core test behind optixTrace has.  No backface culling (OPTIX_RAY_FLAG_NONE).
 * Returns 1 and *t_out if the supporting ray hits at some t > 0 (caller applies (tmin,tmax)).
 * Every operation is a single rounded IEEE op; the HIP kernel (pt_bvh.h tri_test) performs the
 * same ones in the same order, so t is bit-identical on both sides.
 * Last criterion (hit_in_box below, applied by the callers to candidates that passed the sign test and the t interval): the hit point o + t d must lie inside the triangle's bounding box widened by hp = half the padding every
 * acceleration structure gives its boxes (2^-17 of the largest |coordinate| of the scene).  In float arithmetic a needle triangle seen
 * along its axis yields three edge functions that are rounding noise, and the sign test then accepts rays that pass the triangle at
 * many times its width (measured on the stadium scene: 5 of 3 M camera rays) — hits OUTSIDE the triangle's box, which a hierarchy
 * finds or misses depending on which other boxes it happens to enter.  With the criterion every accepted hit lies inside every
 * structure's (more widely padded) box for that triangle, so brute force and all trees return the same answer again. */
static inline int wtri2(const wray* r, const float* p0, const float* p1, const float* p2, float* t_out, float* det_out) {
    const f3 A = sub3(mk3(p0[0], p0[1], p0[2]), r->o);
    const f3 B = sub3(mk3(p1[0], p1[1], p1[2]), r->o);
    const f3 C = sub3(mk3(p2[0], p2[1], p2[2]), r->o);
    const f3 CxB = cross3(C, B), AxC = cross3(A, C), BxA = cross3(B, A);
    const float U = dot3(r->d, CxB), V = dot3(r->d, AxC), W = dot3(r->d, BxA);
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return 0;
    const float det = U + V + W;
    if (det == 0.0f) return 0;
    const float Ad = dot3(r->dn, A), Bd = dot3(r->dn, B), Cd = dot3(r->dn, C);
    const float T = U * Ad + V * Bd + W * Cd;
    if (T == 0.0f || ((T < 0.0f) != (det < 0.0f))) return 0;
    *t_out = T / det;
    *det_out = det;
    return 1;
}
/* the hit point o + t d (one fused multiply-add per axis, like the kernel) inside the triangle's box widened by r->hp */
/* the tolerance grows with the distance travelled (the computed hit point is off by ~2^-22 of |t d|): hp + 2^-21 t (|dx| + |dy| + |dz|),
 * the same three rounded operations as pt_bvh.h */
static inline int hit_in_box(const wray* r, const float* p0, const float* p1, const float* p2, float t) {
    const float o[3] = {r->o.x, r->o.y, r->o.z}, d[3] = {r->d.x, r->d.y, r->d.z};
    const float l1 = (fabsf(d[0]) + fabsf(d[1])) + fabsf(d[2]);
    const float hpe = r->hp + (t * l1) * 4.76837158203125e-07f;
    for (int a = 0; a < 3; ++a) {
        const float pa = fmaf(d[a], t, o[a]);
        const float lo = fminf(fminf(p0[a], p1[a]), p2[a]) - hpe, hi = fmaxf(fmaxf(p0[a], p1[a]), p2[a]) + hpe;
        if (pa < lo || pa > hi) return 0;
    }
    return 1;
}
static inline int wtri(const wray* r, const float* p0, const float* p1, const float* p2, float* t_out) {
    float det;
    return wtri2(r, p0, p1, p2, t_out, &det);
}

static inline void tri_verts(const orc_scene* s, uint32_t prim, const float** v0, const float** v1, const float** v2) {
    const uint32_t* ix = &s->idx[3 * (size_t)prim];
    *v0 = &s->verts[3 * (size_t)ix[0]];
    *v1 = &s->verts[3 * (size_t)ix[1]];
    *v2 = &s->verts[3 * (size_t)ix[2]];
}

/* conservative slab test: (b-o)*inv form, far side widened (Ize 2013) */
static inline int slab(const onode* n, const float o[3], const float inv[3], float tmin, float tmax, float pad) {
    float t0 = tmin, t1 = tmax;
    for (int a = 0; a < 3; ++a) {
        float ta = ((n->lo[a] - pad) - o[a]) * inv[a];
        float tb = ((n->hi[a] + pad) - o[a]) * inv[a];
        float tn = fminf(ta, tb), tf = fmaxf(ta, tb);
        tf *= 1.0000004f;
        t0 = fmaxf(t0, tn); /* fmaxf/fminf drop NaN (0*inf) operands */
        t1 = fminf(t1, tf);
    }
    return t0 <= t1;
}

/* closest hit: smallest t in (tmin,tmax); ties -> lowest prim id. returns prim or -1 */
/* ---- scalar traversal of the product's 8-wide tree (layout: optixpathtracer_amd/csrc/pt_bvh8.h, include/pt_amd.h pt_export_bvh)
 * node words: [0..2] origin.xyz (f32) | [3] hi16(sx) | hi16(sy) << 16 | [4] child_base | [5] tri_base | [6] leafbits | [7] hi16(sz) | imask << 16
 *             [8,9] qlo.x[8] | [10,11] qlo.y[8] | [12,13] qlo.z[8] | [14,15] qhi.x[8] | [16,17] qhi.y[8] | [18,19] qhi.z[8]
 * child box s = origin + q * step per axis; internal child s = node child_base + popcount(imask & ((1 << s) - 1));
 * leafbits bit 3s+k: slot s holds more than k triangles; triangle (s,k) = tri_base + popcount(leafbits & ((1 << (3s+k)) - 1)).
 * The box test is done in double on the dequantised box (conservative: the GPU's float test may only ever admit more). */
static inline float n8_f(uint32_t bits) { float f; memcpy(&f, &bits, 4); return f; }
static inline uint32_t n8_q(const uint32_t* w, int first, int s) { return (w[first + (s >> 2)] >> (8 * (s & 3))) & 0xffu; }
/* any == 0: closest hit (returns prim or -1, *t_hit); any == 1: returns 1 at the first accepted hit */
static int64_t bvh8_traverse(const orc_scene* s, const wray* r, f3 o, f3 d, float tmin, float tmax, int any, int cull_back, float* t_hit) {
    float best = tmax;
    int64_t bp = -1;
    uint32_t stack[256];
    int sp = 0;
    stack[sp++] = 0;
    const double od[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    while (sp) {
        const uint32_t* w = &s->n8[(size_t)stack[--sp] * 20];
        const double org[3] = {n8_f(w[0]), n8_f(w[1]), n8_f(w[2])};
        const double stp[3] = {n8_f(w[3] << 16), n8_f(w[3] & 0xffff0000u), n8_f(w[7] << 16)};
        const uint32_t imask = w[7] >> 16, leafbits = w[6];
        for (int c = 0; c < 8; ++c) {
            double t0 = tmin, t1 = best;
            int empty = 0;
            for (int a = 0; a < 3 && !empty; ++a) {
                const uint32_t qlo = n8_q(w, 8 + 2 * a, c), qhi = n8_q(w, 14 + 2 * a, c);
                if (qlo > qhi) { empty = 1; break; } /* inverted = unused slot */
                const double lo = org[a] + qlo * stp[a], hi = org[a] + qhi * stp[a];
                if (dd[a] == 0.0) {
                    if (od[a] < lo - 1e-9 * (1.0 + fabs(lo)) || od[a] > hi + 1e-9 * (1.0 + fabs(hi))) empty = 1;
                    continue;
                }
                double ta = (lo - od[a]) / dd[a], tb = (hi - od[a]) / dd[a];
                if (ta > tb) { const double x = ta; ta = tb; tb = x; }
                ta -= 1e-9 * (1.0 + fabs(ta));
                tb += 1e-9 * (1.0 + fabs(tb));
                if (ta > t0) t0 = ta;
                if (tb < t1) t1 = tb;
            }
            if (empty || t0 > t1) continue;
            if (imask & (1u << c)) {
                if (sp < 255) stack[sp++] = w[4] + (uint32_t)__builtin_popcount(imask & ((1u << c) - 1u));
                continue;
            }
            for (int k = 0; k < 3; ++k) {
                const int bit = 3 * c + k;
                if (!(leafbits & (1u << bit))) break;
                const float* tv = &s->t8[(size_t)(w[5] + (uint32_t)__builtin_popcount(leafbits & ((1u << bit) - 1u))) * 12];
                uint32_t pbits;
                memcpy(&pbits, &tv[9], 4);
                const int64_t p = (int64_t)(int32_t)pbits;
                float t, det;
                if (!wtri2(r, &tv[0], &tv[3], &tv[6], &t, &det)) continue;
                if (any) {
                    if (t > tmin && t < tmax && (!cull_back || det > 0.0f) && hit_in_box(r, &tv[0], &tv[3], &tv[6], t)) return 1;
                } else if (t > tmin && (t < best || (t == best && bp >= 0 && p < bp)) && hit_in_box(r, &tv[0], &tv[3], &tv[6], t)) {
                    best = t;
                    bp = p;
                }
            }
        }
    }
    if (any) return 0;
    *t_hit = best;
    return bp;
}

static int64_t closest_hit(const orc_scene* s, f3 o, f3 d, float tmin, float tmax, float* t_hit) {
    wray r;
    wray_init(&r, o, d);
    r.hp = 0.5f * s->pad;
    if (s->n8) return bvh8_traverse(s, &r, o, d, tmin, tmax, 0, 0, t_hit);
    float best = tmax;
    int64_t bp = -1;
    if (!s->use_bvh) {
        for (uint32_t p = 0; p < s->ntri; ++p) {
            const float *v0, *v1, *v2;
            float t;
            tri_verts(s, p, &v0, &v1, &v2);
            if (wtri(&r, v0, v1, v2, &t) && t > tmin && (t < best || (t == best && bp >= 0 && (int64_t)p < bp)) && hit_in_box(&r, v0, v1, v2, t)) {
                best = t;
                bp = p;
            }
        }
    } else {
        float inv[3] = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z}, ro[3] = {o.x, o.y, o.z};
        uint32_t stack[128];
        int sp = 0;
        stack[sp++] = 0;
        while (sp) {
            const onode* n = &s->nodes[stack[--sp]];
            if (!slab(n, ro, inv, tmin, best, s->pad)) continue;
            if (n->right == 0xffffffffu) {
                for (uint32_t k = 0; k < n->count; ++k) {
                    uint32_t p = s->order[n->left + k];
                    const float *v0, *v1, *v2;
                    float t;
                    tri_verts(s, p, &v0, &v1, &v2);
                    if (wtri(&r, v0, v1, v2, &t) && t > tmin &&
                        (t < best || (t == best && bp >= 0 && (int64_t)p < bp)) && hit_in_box(&r, v0, v1, v2, t)) {
                        best = t;
                        bp = p;
                    }
                }
            } else {
                stack[sp++] = n->left;
                stack[sp++] = n->right;
            }
        }
    }
    *t_hit = best;
    return bp;
}

/* cull_back: OPTIX_RAY_FLAG_CULL_BACK_FACING_TRIANGLES (the sv3/sv4 occlusion ray, HelloPathtracing_sv4_vmv23/
 * deviceProgram.cu:240): only triangles whose front (counter-clockwise) side faces the ray origin count, i.e.
 * dot(d, (v1-v0)x(v2-v0)) < 0, which is det > 0 in wtri's convention (det = -d.n). */
static int any_hit_c(const orc_scene* s, f3 o, f3 d, float tmin, float tmax, int cull_back) {
    wray r;
    wray_init(&r, o, d);
    r.hp = 0.5f * s->pad;
    if (s->n8) return (int)bvh8_traverse(s, &r, o, d, tmin, tmax, 1, cull_back, NULL);
    if (!s->use_bvh) {
        for (uint32_t p = 0; p < s->ntri; ++p) {
            const float *v0, *v1, *v2;
            float t, det;
            tri_verts(s, p, &v0, &v1, &v2);
            if (wtri2(&r, v0, v1, v2, &t, &det) && t > tmin && t < tmax && (!cull_back || det > 0.0f) && hit_in_box(&r, v0, v1, v2, t)) return 1;
        }
        return 0;
    }
    float inv[3] = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z}, ro[3] = {o.x, o.y, o.z};
    uint32_t stack[128];
    int sp = 0;
    stack[sp++] = 0;
    while (sp) {
        const onode* n = &s->nodes[stack[--sp]];
        if (!slab(n, ro, inv, tmin, tmax, s->pad)) continue;
        if (n->right == 0xffffffffu) {
            for (uint32_t k = 0; k < n->count; ++k) {
                uint32_t p = s->order[n->left + k];
                const float *v0, *v1, *v2;
                float t, det;
                tri_verts(s, p, &v0, &v1, &v2);
                if (wtri2(&r, v0, v1, v2, &t, &det) && t > tmin && t < tmax && (!cull_back || det > 0.0f) && hit_in_box(&r, v0, v1, v2, t)) return 1;
            }
        } else {
            stack[sp++] = n->left;
            stack[sp++] = n->right;
        }
    }
    return 0;
}

static int any_hit(const orc_scene* s, f3 o, f3 d, float tmin, float tmax) { return any_hit_c(s, o, d, tmin, tmax, 0); }

/* --- median-split BVH2 (the oracle's own; unrelated to the product's LBVH) */
typedef struct { float c[3]; uint32_t prim; } cent;
static int g_axis;
static int cent_cmp(const void* a, const void* b) {
    float x = ((const cent*)a)->c[g_axis], y = ((const cent*)b)->c[g_axis];
    if (x < y) return -1;
    if (x > y) return 1;
    uint32_t p = ((const cent*)a)->prim, q = ((const cent*)b)->prim;
    return p < q ? -1 : (p > q);
}
static void prim_bounds(const orc_scene* s, uint32_t p, float lo[3], float hi[3]) {
    const float *v0, *v1, *v2;
    tri_verts(s, p, &v0, &v1, &v2);
    for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(v0[a], fminf(v1[a], v2[a]));
        hi[a] = fmaxf(v0[a], fmaxf(v1[a], v2[a]));
    }
}
static uint32_t build_rec(orc_scene* s, cent* cs, uint32_t first, uint32_t count) {
    uint32_t id = s->nnodes++;
    onode* n = &s->nodes[id];
    float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int a = 0; a < 3; ++a) { n->lo[a] = INFINITY; n->hi[a] = -INFINITY; }
    for (uint32_t k = 0; k < count; ++k) {
        float lo[3], hi[3];
        prim_bounds(s, cs[first + k].prim, lo, hi);
        for (int a = 0; a < 3; ++a) {
            n->lo[a] = fminf(n->lo[a], lo[a]);
            n->hi[a] = fmaxf(n->hi[a], hi[a]);
            clo[a] = fminf(clo[a], cs[first + k].c[a]);
            chi[a] = fmaxf(chi[a], cs[first + k].c[a]);
        }
    }
    if (count <= 4) {
        n->left = first; n->right = 0xffffffffu; n->count = count;
        return id;
    }
    int axis = 0;
    if (chi[1] - clo[1] > chi[axis] - clo[axis]) axis = 1;
    if (chi[2] - clo[2] > chi[axis] - clo[axis]) axis = 2;
    g_axis = axis;
    qsort(cs + first, count, sizeof(cent), cent_cmp);
    uint32_t half = count / 2;
    uint32_t l = build_rec(s, cs, first, half);
    uint32_t r = build_rec(s, cs, first + half, count - half);
    n = &s->nodes[id];
    n->left = l; n->right = r; n->count = 0;
    return id;
}

orc_scene* orc_scene_create(const float* verts, uint32_t nv, const uint32_t* idx, uint32_t ntri, const uint32_t* tri_mesh,
                            const orc_material* mats, uint32_t nmesh, int use_bvh) {
    orc_scene* s = (orc_scene*)calloc(1, sizeof(orc_scene));
    s->nv = nv; s->ntri = ntri; s->nmesh = nmesh;
    s->verts = (float*)malloc(sizeof(float) * 3 * (size_t)nv);
    memcpy(s->verts, verts, sizeof(float) * 3 * (size_t)nv);
    s->idx = (uint32_t*)malloc(sizeof(uint32_t) * 3 * (size_t)ntri);
    memcpy(s->idx, idx, sizeof(uint32_t) * 3 * (size_t)ntri);
    s->tri_mesh = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)ntri);
    memcpy(s->tri_mesh, tri_mesh, sizeof(uint32_t) * (size_t)ntri);
    s->mats = (orc_material*)malloc(sizeof(orc_material) * nmesh);
    memcpy(s->mats, mats, sizeof(orc_material) * nmesh);
    for (uint32_t m = 0; m < nmesh; ++m)
        if (mats[m].flags & MATERIAL_FLAG_SHADOW_CATCHER) s->has_catcher = 1;
    s->use_bvh = use_bvh && ntri > 0;
    {   /* box padding of every structure over this scene (pt_bvh_build.hip computes the same): 2^-16 of the largest |coordinate| */
        float mx = 0.0f;
        for (uint32_t p = 0; p < ntri; ++p) {
            float lo[3], hi[3];
            prim_bounds(s, p, lo, hi);
            for (int a = 0; a < 3; ++a) mx = fmaxf(mx, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
        }
        s->pad = mx * (1.0f / 65536.0f);
    }
    if (s->use_bvh) {
        cent* cs = (cent*)malloc(sizeof(cent) * (size_t)ntri);
        float mx = 0.0f;
        for (uint32_t p = 0; p < ntri; ++p) {
            float lo[3], hi[3];
            prim_bounds(s, p, lo, hi);
            for (int a = 0; a < 3; ++a) {
                cs[p].c[a] = 0.5f * (lo[a] + hi[a]);
                mx = fmaxf(mx, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
            }
            cs[p].prim = p;
        }
        s->pad = mx * (1.0f / 65536.0f);
        s->nodes = (onode*)malloc(sizeof(onode) * (2 * (size_t)ntri + 1));
        s->nnodes = 0;
        build_rec(s, cs, 0, ntri);
        s->order = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)ntri);
        for (uint32_t p = 0; p < ntri; ++p) s->order[p] = cs[p].prim;
        free(cs);
    }
    return s;
}
/* borrow the product's tree (arrays stay owned by the caller and must outlive the scene); NULL nodes = back to the checker's own search */
void orc_scene_set_bvh8(orc_scene* s, const uint32_t* nodes, uint32_t nnodes, const float* tris, uint32_t ntris) {
    s->n8 = nodes;
    s->nnodes8 = nnodes;
    s->t8 = tris;
    s->ntris8 = ntris;
}

void orc_scene_destroy(orc_scene* s) {
    if (!s) return;
    free(s->verts); free(s->idx); free(s->tri_mesh); free(s->mats); free(s->nodes); free(s->order);
    free(s->texcoord); free(s->mesh_tex); free(s->mesh_has_uv);
    for (uint32_t k = 0; k < s->ntex; ++k) free(s->tex[k].pixel);
    free(s->tex);
    free(s);
}

/* tex2D<float4> of a uchar4 CUDA array with addressMode Wrap, filterMode Linear, readMode NormalizedFloat,
 * normalizedCoords, no sRGB (SimplePathtracer.cpp:603-654), restated from the CUDA C Programming Guide appendix
 * "Texture Fetching" (linear filtering: xB = x - 0.5, i = floor(xB), alpha = frac(xB) kept in 9-bit fixed point with 8
 * fractional bits; wrap: x = frac(s) * N).  The hardware's exact rounding of alpha is not documented: round to nearest
 * is used.  PARITY UNPINNED (no CUDA hardware, no fixture in the reference). */
static inline float texel_ch(uint32_t p, int k) { return (float)((p >> (8 * k)) & 0xffu) / 255.0f; }
static void tex2d_wrap_linear(const uint32_t* pix, int W, int H, float s, float t, float out[4]) {
    const float x = (s - floorf(s)) * (float)W, y = (t - floorf(t)) * (float)H;
    const float xB = x - 0.5f, yB = y - 0.5f;
    const float fi = floorf(xB), fj = floorf(yB);
    const float alpha = floorf((xB - fi) * 256.0f + 0.5f) * (1.0f / 256.0f);
    const float beta = floorf((yB - fj) * 256.0f + 0.5f) * (1.0f / 256.0f);
    int i0 = (int)fi, j0 = (int)fj;
    int i1 = i0 + 1, j1 = j0 + 1;
    i0 = ((i0 % W) + W) % W; i1 = ((i1 % W) + W) % W;
    j0 = ((j0 % H) + H) % H; j1 = ((j1 % H) + H) % H;
    const uint32_t t00 = pix[(size_t)j0 * W + i0], t10 = pix[(size_t)j0 * W + i1], t01 = pix[(size_t)j1 * W + i0], t11 = pix[(size_t)j1 * W + i1];
    for (int k = 0; k < 4; ++k)
        out[k] = (1.0f - alpha) * (1.0f - beta) * texel_ch(t00, k) + alpha * (1.0f - beta) * texel_ch(t10, k) +
                 (1.0f - alpha) * beta * texel_ch(t01, k) + alpha * beta * texel_ch(t11, k);
}
void orc_tex2d(const uint32_t* pix, int W, int H, float s, float t, float out[4]) { tex2d_wrap_linear(pix, W, H, s, t, out); }

void orc_scene_set_textures(orc_scene* s, const float* texcoord, const int32_t* mesh_tex, const uint8_t* mesh_has_uv, uint32_t ntex,
                            const uint32_t* const* pixels, const int32_t* widths, const int32_t* heights) {
    if (texcoord) {
        s->texcoord = (float*)malloc(sizeof(float) * 2 * (size_t)s->nv);
        memcpy(s->texcoord, texcoord, sizeof(float) * 2 * (size_t)s->nv);
    }
    s->mesh_tex = (int32_t*)malloc(sizeof(int32_t) * s->nmesh);
    memcpy(s->mesh_tex, mesh_tex, sizeof(int32_t) * s->nmesh);
    s->mesh_has_uv = (uint8_t*)malloc(s->nmesh);
    memcpy(s->mesh_has_uv, mesh_has_uv, s->nmesh);
    s->ntex = ntex;
    s->tex = calloc(ntex ? ntex : 1, sizeof(*s->tex));
    for (uint32_t k = 0; k < ntex; ++k) {
        s->tex[k].w = widths[k]; s->tex[k].h = heights[k];
        s->tex[k].pixel = (uint32_t*)malloc(4 * (size_t)widths[k] * heights[k]);
        memcpy(s->tex[k].pixel, pixels[k], 4 * (size_t)widths[k] * heights[k]);
    }
}

/* batch ray queries for kernel-level tests: rays = n*8 floats (o.xyz,tmin,d.xyz,tmax) */
void orc_trace_closest(const orc_scene* s, const float* rays, int n, float* t_out, int32_t* prim_out) {
    for (int i = 0; i < n; ++i) {
        const float* r = &rays[8 * (size_t)i];
        float t;
        int64_t p = closest_hit(s, mk3(r[0], r[1], r[2]), mk3(r[4], r[5], r[6]), r[3], r[7], &t);
        t_out[i] = p >= 0 ? t : r[7];
        prim_out[i] = (int32_t)p;
    }
}
/* Census of the float acceptance rule (wtri2 + hit_in_box: this repository's definition of what optixTrace returns) against exact
 * geometry ("What's weak" 10).  For every ray all triangles whose (padded) boxes the ray enters are tested twice: with the
 * float rule and with Moller-Trumbore in double precision on the same float vertices (u, v >= 0, u + v <= 1, t in (tmin, tmax): exact up
 * to ~1e-15, i.e. the mathematical triangle).  Per ray the closest hit of either rule is compared.  out[0] rays, [1] rays whose two
 * closest hits are the same primitive (or both miss), [2] float rule's closest hit is a triangle the exact test REJECTS ("accepted but
 * inexact"), [3] the exact closest hit is a triangle the float rule rejected ("rejected but exact"), [4] both accept both triangles but
 * order them differently (|t| ties within rounding: coplanar / shared-edge neighbours), [5] candidate triangles tested, [6] candidates
 * the two rules classify differently, [7] rays with any such candidate.  Needs the scene's own BVH (use_bvh). */
static int mt_double(const double o[3], const double d[3], const float* p0, const float* p1, const float* p2, double tmin, double tmax, double* t_out) {
    const double e1[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
    const double e2[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
    const double pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
    const double det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
    if (det == 0.0) return 0;
    const double inv = 1.0 / det;
    const double tv[3] = {o[0] - p0[0], o[1] - p0[1], o[2] - p0[2]};
    const double u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * inv;
    if (u < 0.0 || u > 1.0) return 0;
    const double qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
    const double v = (d[0] * qv[0] + d[1] * qv[1] + d[2] * qv[2]) * inv;
    if (v < 0.0 || u + v > 1.0) return 0;
    const double t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv;
    if (!(t > tmin && t < tmax)) return 0;
    *t_out = t;
    return 1;
}
void orc_hit_census(const orc_scene* s, const float* rays, int n, unsigned long long out[8]) {
    for (int k = 0; k < 8; ++k) out[k] = 0;
    if (!s->use_bvh) return;
    for (int i = 0; i < n; ++i) {
        const float* q = rays + 8 * (size_t)i;
        const f3 o = mk3(q[0], q[1], q[2]), d = mk3(q[4], q[5], q[6]);
        const float tmin = q[3], tmax = q[7];
        wray r;
        wray_init(&r, o, d);
        r.hp = 0.5f * s->pad;
        const double od[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
        float inv[3] = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z}, ro[3] = {o.x, o.y, o.z};
        float fbest = tmax;
        int64_t fp = -1;
        double ebest = (double)tmax;
        int64_t ep = -1;
        int f_of_exact_best = 0; /* filled below: does the float rule accept the exact rule's closest triangle? */
        unsigned long long ndiff = 0;
        uint32_t stack[128];
        int sp = 0;
        stack[sp++] = 0;
        /* first pass: both closest hits, every box the ray enters (no culling by the best hit: the two rules would cull differently) */
        while (sp) {
            const onode* nd = &s->nodes[stack[--sp]];
            if (!slab(nd, ro, inv, tmin, tmax, 4.0f * s->pad)) continue;
            if (nd->right == 0xffffffffu) {
                for (uint32_t k = 0; k < nd->count; ++k) {
                    const uint32_t p = s->order[nd->left + k];
                    const float *v0, *v1, *v2;
                    tri_verts(s, p, &v0, &v1, &v2);
                    float t;
                    const int fa = wtri(&r, v0, v1, v2, &t) && t > tmin && t < tmax && hit_in_box(&r, v0, v1, v2, t);
                    double te;
                    const int ea = mt_double(od, dd, v0, v1, v2, (double)tmin, (double)tmax, &te);
                    ++out[5];
                    if (fa != ea) ++ndiff;
                    if (fa && (t < fbest || (t == fbest && fp >= 0 && (int64_t)p < fp))) { fbest = t; fp = p; }
                    if (ea && (te < ebest || (te == ebest && ep >= 0 && (int64_t)p < ep))) { ebest = te; ep = p; }
                }
            } else {
                stack[sp++] = nd->left;
                stack[sp++] = nd->right;
            }
        }
        ++out[0];
        out[6] += ndiff;
        if (ndiff) ++out[7];
        if (fp == ep) { ++out[1]; continue; }
        /* the closest hits differ: which rule disagrees about which triangle? */
        int e_of_float_best = 0;
        if (fp >= 0) {
            const float *v0, *v1, *v2;
            double te;
            tri_verts(s, (uint32_t)fp, &v0, &v1, &v2);
            e_of_float_best = mt_double(od, dd, v0, v1, v2, (double)tmin, (double)tmax, &te);
        }
        if (ep >= 0) {
            const float *v0, *v1, *v2;
            float t;
            tri_verts(s, (uint32_t)ep, &v0, &v1, &v2);
            f_of_exact_best = wtri(&r, v0, v1, v2, &t) && t > tmin && t < tmax && hit_in_box(&r, v0, v1, v2, t);
        }
        if (fp >= 0 && !e_of_float_best) ++out[2];
        else if (ep >= 0 && !f_of_exact_best) ++out[3];
        else ++out[4];
    }
}

void orc_trace_any(const orc_scene* s, const float* rays, int n, uint8_t* occ_out) {
    for (int i = 0; i < n; ++i) {
        const float* r = &rays[8 * (size_t)i];
        occ_out[i] = (uint8_t)any_hit(s, mk3(r[0], r[1], r[2]), mk3(r[4], r[5], r[6]), r[3], r[7]);
    }
}

/* optixGetTriangleBarycentrics: (weight of vertex 1, weight of vertex 2) — from the hit test's own weights (wtri2's U, V, W) */
static inline void hit_barycentrics(f3 ray_o, f3 ray_dir, f3 v0, f3 v1, f3 v2, float* bu, float* bv) {
    wray r;
    wray_init(&r, ray_o, ray_dir);
    const f3 A = sub3(v0, r.o), B = sub3(v1, r.o), C = sub3(v2, r.o);
    const f3 CxB = cross3(C, B), AxC = cross3(A, C), BxA = cross3(B, A);
    const float Uw = dot3(r.d, CxB), Vw = dot3(r.d, AxC), Ww = dot3(r.d, BxA);
    const float det = Uw + Vw + Ww;
    *bu = Vw / det;
    *bv = Ww / det;
}
/* the same for a (ray, primitive) pair of a batch query: ray = (o.xyz, tmin, d.xyz, tmax) as in orc_trace_closest */
void orc_hit_barycentrics(const orc_scene* s, const float* ray, uint32_t prim, float uv[2]) {
    const float *p0, *p1, *p2;
    tri_verts(s, prim, &p0, &p1, &p2);
    hit_barycentrics(mk3(ray[0], ray[1], ray[2]), mk3(ray[4], ray[5], ray[6]), mk3(p0[0], p0[1], p0[2]), mk3(p1[0], p1[1], p1[2]), mk3(p2[0], p2[1], p2[2]), &uv[0], &uv[1]);
}
/* orc_trace_any with OPTIX_RAY_FLAG_CULL_BACK_FACING_TRIANGLES (any_hit_c's cull_back: the sv3/sv4 occlusion ray) */
void orc_trace_any_cull(const orc_scene* s, const float* rays, int n, uint8_t* occ_out) {
    for (int i = 0; i < n; ++i) {
        const float* r = &rays[8 * (size_t)i];
        occ_out[i] = (uint8_t)any_hit_c(s, mk3(r[0], r[1], r[2]), mk3(r[4], r[5], r[6]), r[3], r[7], 1);
    }
}

/* ---------------------------------------------------------------- table entry points (function-level tests) */
void orc_bsdf_eval(int mode, const orc_material* mat, const float albedo[3], float etaI, float etaO, const float N[3],
                   const float V[3], const float L[3], float out[3]) {
    f3 r = bsdf_eval(mode, mat, mk3(albedo[0], albedo[1], albedo[2]), etaI, etaO, mk3(N[0], N[1], N[2]),
                     mk3(V[0], V[1], V[2]), mk3(L[0], L[1], L[2]));
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}
float orc_bsdf_pdf(int mode, const orc_material* mat, float etaI, float etaO, const float N[3], const float V[3],
                   const float L[3]) {
    return bsdf_pdf(mode, mat, etaI, etaO, mk3(N[0], N[1], N[2]), mk3(V[0], V[1], V[2]), mk3(L[0], L[1], L[2]));
}
/* BasisFromVector(N) + BSDFSample with Random(seed) */
void orc_bsdf_sample(int mode, const orc_material* mat, float etaI, float etaO, const float N[3], const float V[3],
                     uint32_t seed, float L[3], float* pdf, uint32_t state_out[2]) {
    orc_random r;
    orc_random_init(&r, seed);
    f3 n = mk3(N[0], N[1], N[2]), u, v, l = mk3s(0.0f);
    basis_from_vector(n, &u, &v);
    bsdf_sample(mode, mat, etaI, etaO, u, v, n, mk3(V[0], V[1], V[2]), &l, pdf, &r);
    L[0] = l.x; L[1] = l.y; L[2] = l.z;
    state_out[0] = r.seed1; state_out[1] = r.seed2;
}
/* the small vector helpers by themselves, for the golden fixture (tests/golden/ref_tables.npz): normalize / faceforward
 * (sutil/vec_math.h:553-570), SafeNormalize (maths.h:144-156), lerp / clamp (sutil/vec_math.h:500-516), toSRGB (cuda/helpers.h:34-42) */
void orc_normalize(const float a[3], float out[3]) { f3 r = normalize3(mk3(a[0], a[1], a[2])); out[0] = r.x; out[1] = r.y; out[2] = r.z; }
void orc_faceforward(const float n[3], const float i[3], float out[3]) { f3 N = mk3(n[0], n[1], n[2]); f3 r = faceforward3(N, mk3(i[0], i[1], i[2]), N); out[0] = r.x; out[1] = r.y; out[2] = r.z; }
void orc_safe_normalize(const float a[3], float out[3]) { f3 r = safe_normalize(mk3(a[0], a[1], a[2])); out[0] = r.x; out[1] = r.y; out[2] = r.z; }
void orc_lerp3(const float a[3], const float b[3], float t, float out[3]) { f3 r = lerp3(mk3(a[0], a[1], a[2]), mk3(b[0], b[1], b[2]), t); out[0] = r.x; out[1] = r.y; out[2] = r.z; }
void orc_clamp3(const float v[3], float lo, float hi, float out[3]) { out[0] = clampf(v[0], lo, hi); out[1] = clampf(v[1], lo, hi); out[2] = clampf(v[2], lo, hi); }
void orc_to_srgb(const float c[3], float out[3]) { out[0] = to_srgb1(c[0]); out[1] = to_srgb1(c[1]); out[2] = to_srgb1(c[2]); }
void orc_basis_from_vector(const float w[3], float u[3], float v[3]) {
    f3 uu, vv;
    basis_from_vector(mk3(w[0], w[1], w[2]), &uu, &vv);
    u[0] = uu.x; u[1] = uu.y; u[2] = uu.z;
    v[0] = vv.x; v[1] = vv.y; v[2] = vv.z;
}
void orc_uniform_sample_hemisphere(uint32_t seed, float d[3]) {
    orc_random r;
    orc_random_init(&r, seed);
    f3 v = uniform_sample_hemisphere(&r);
    d[0] = v.x; d[1] = v.y; d[2] = v.z;
}
void orc_cosine_sample_hemisphere(float u1, float u2, float d[3]) {
    f3 v = cosine_sample_hemisphere(u1, u2);
    d[0] = v.x; d[1] = v.y; d[2] = v.z;
}
/* detmath/libm function table: which: 0 sin 1 cos 2 acos 3 atan2(x,y2) 4 log 5 pow(x,y2) */
void orc_math_table(int which, const float* x, const float* y2, int n, float* out) {
    for (int i = 0; i < n; ++i) {
        switch (which) {
            case 0: out[i] = M_SIN(x[i]); break;
            case 1: out[i] = M_COS(x[i]); break;
            case 2: out[i] = M_ACOS(x[i]); break;
            case 3: out[i] = M_ATAN2(x[i], y2[i]); break;
            case 4: out[i] = M_LOG(x[i]); break;
            default: out[i] = M_POW(x[i], y2[i]); break;
        }
    }
}

/* ---------------------------------------------------------------- the render (raygen + closest-hit + miss) */
typedef struct {
    int width, height;
    uint32_t subframe_index;
    uint32_t samples_per_launch;
    int max_depth; /* the reference's literal 8 (deviceProgram.cu:429) */
    int bsdf_mode;
    float eye[3], U[3], V[3], W[3];
    /* pixel subset: render only rows y with (y % row_mod) == row_rem (threading) */
} orc_params;

enum { FLAG_DONE = 1, FLAG_SECONDARY = 2 };

typedef struct {
    f3 radiance, alpha, origin, direction, normal, albedo, throughput;
    float bsdfPdf, rayEta;
    int depth, flags;
    orc_random rand;
} prd_t;

typedef struct { uint64_t radiance_rays, shadow_rays; } orc_stats;

/* Knobs that differ between the canonical variant and the foveated sv3/sv4 variants */
typedef struct {
    float radiance_tmin;      /* 0.001 original (deviceProgram.cu:420); 0.01 in sv4 (global tmin, sv4 deviceProgram.cu:41,485) */
    int cull_back_occlusion;  /* 0 original (TERMINATE_ON_FIRST_HIT); 1 sv3/sv4 (CULL_BACK_FACING_TRIANGLES, :240) */
    int tonemap;              /* 0 = make_color(accum) ; 1 = make_color(reinhard(accum * exposure, white)) (sv4 :555-569); 2 = make_color(accum * exposure) (sv3) */
    float exposure, white;
    int initial_depth;        /* prd.depth at the camera ray: 1 in HelloPathtracing_sv / _sv2 (deviceProgram.cu:428), else 0 */
    int write_aov;            /* sv / sv2 also write normal/color/albedo buffers (sv deviceProgram.cu:553-555) */
} orc_variant;
static __thread orc_variant g_var = {0.001f, 0, 0, 1.0f, 1.0f, 0, 0};

/* deviceProgram.cu:252-334 SampleLights / SampleShadow (want_occluded selects) */
static f3 sample_lights(const orc_scene* s, const orc_probe* probe, int mode, const orc_material* mat, f3 albedo, float etaI,
                        float etaO, f3 P, f3 N, f3 wo, orc_random* rand, int want_occluded, orc_stats* st) {
    f3 sum = mk3s(0.0f);
    f3 skyColor, wi;
    float skyPdf;
    probe_sample(probe, &wi, &skyColor, &skyPdf, rand);
    st->shadow_rays++;
    const int occluded = any_hit_c(s, P, wi, 0.01f, 1e16f, g_var.cull_back_occlusion);
    if (occluded == want_occluded) {
        float bsdfPdf = bsdf_pdf(mode, mat, etaI, etaO, N, wo, wi);
        f3 f = bsdf_eval(mode, mat, albedo, etaI, etaO, N, wo, wi);
        if (bsdfPdf > 0.0f) {
            float cbsdf = 0.5f, csky = 0.5f; /* kBsdfSamples/N, kProbeSamples/N with N=2 */
            float weight = csky * skyPdf / (cbsdf * bsdfPdf + csky * skyPdf);
            if (weight > 0.0f) {
                /* weight * skyColor * f * abs(dot(wi,N)) / skyPdf * (1/kProbeSamples) */
                f3 val = scl3(div3s(scl3(mul3(scl3(skyColor, weight), f), fabsf(dot3(wi, N))), skyPdf), 1.0f);
                sum = add3(sum, val);
            }
        }
    }
    return sum;
}

/* deviceProgram.cu:477-594 */
static void closest_hit_program(const orc_scene* s, const orc_probe* probe, int mode, uint32_t prim, f3 ray_o, f3 ray_dir,
                                float t, prd_t* prd, orc_stats* st) {
    const orc_material* mat = &s->mats[s->tri_mesh[prim]];
    const float *p0, *p1, *p2;
    tri_verts(s, prim, &p0, &p1, &p2);
    f3 v0 = mk3(p0[0], p0[1], p0[2]), v1 = mk3(p1[0], p1[1], p1[2]), v2 = mk3(p2[0], p2[1], p2[2]);
    f3 N_0 = normalize3(cross3(sub3(v1, v0), sub3(v2, v0)));
    f3 N = faceforward3(N_0, neg3(ray_dir), N_0);
    f3 P = add3(ray_o, scl3(ray_dir, t));
    float outEta;
    if ((mat->flags & MATERIAL_FLAG_SHADOW_CATCHER) != 0 && (prd->flags & FLAG_SECONDARY) != 0) {
        prd->origin = P;
        prd->direction = ray_dir;
        --prd->depth;
        return;
    }
    prd->normal = N;
    prd->albedo = mk3(mat->color[0], mat->color[1], mat->color[2]);
    {   /* deviceProgram.cu:512-523: hasTexture && texcoord → albedo REPLACED by tex2D at the interpolated texcoord */
        const uint32_t mesh = s->tri_mesh[prim];
        if (s->mesh_tex && s->mesh_tex[mesh] >= 0 && s->mesh_has_uv[mesh] && s->texcoord) {
            float bu, bv;
            hit_barycentrics(ray_o, ray_dir, v0, v1, v2, &bu, &bv);
            const uint32_t* ix = &s->idx[3 * (size_t)prim];
            const float *c0 = &s->texcoord[2 * (size_t)ix[0]], *c1 = &s->texcoord[2 * (size_t)ix[1]], *c2 = &s->texcoord[2 * (size_t)ix[2]];
            const float w0 = 1.f - bu - bv;
            const float tcx = w0 * c0[0] + bu * c1[0] + bv * c2[0];
            const float tcy = w0 * c0[1] + bu * c1[1] + bv * c2[1];
            float tx[4];
            const int tid = s->mesh_tex[mesh];
            tex2d_wrap_linear(s->tex[tid].pixel, s->tex[tid].w, s->tex[tid].h, tcx, tcy, tx);
            prd->albedo = mk3(tx[0], tx[1], tx[2]);
        }
    }
    if (prd->rayEta == 1.0f)
        outEta = orc_material_ior(mat);
    else
        outEta = 1.0f;
    f3 wo = neg3(ray_dir);
    if ((mat->flags & MATERIAL_FLAG_SHADOW_CATCHER) == 0) {
        f3 ls = sample_lights(s, probe, mode, mat, prd->albedo, prd->rayEta, outEta, P, N, wo, &prd->rand, 0, st);
        prd->radiance = add3(prd->radiance, mul3(prd->throughput, ls));
        prd->alpha = mk3s(1.0f);
    } else {
        f3 ss = sample_lights(s, probe, mode, mat, prd->albedo, prd->rayEta, outEta, P, N, wo, &prd->rand, 1, st);
        prd->alpha = add3(prd->alpha, mul3(prd->throughput, ss));
    }
    if ((prd->flags & FLAG_SECONDARY) == 0)
        prd->radiance = add3(prd->radiance, mk3(mat->emission[0], mat->emission[1], mat->emission[2]));
    f3 u, v, bsdfDir = mk3s(0.0f);
    basis_from_vector(N, &u, &v);
    bsdf_sample(mode, mat, prd->rayEta, outEta, u, v, N, wo, &bsdfDir, &prd->bsdfPdf, &prd->rand);
    if (prd->bsdfPdf <= 0.0f) {
        prd->flags |= FLAG_DONE;
        return;
    }
    f3 f = bsdf_eval(mode, mat, prd->albedo, prd->rayEta, outEta, N, wo, bsdfDir);
    if (dot3(bsdfDir, N) <= 0.0f) prd->rayEta = outEta;
    /* pathThroughput *= f * abs(dot(N,bsdfDir)) / bsdfPdf */
    prd->throughput = mul3(prd->throughput, div3s(scl3(f, fabsf(dot3(N, bsdfDir))), prd->bsdfPdf));
    prd->direction = bsdfDir;
    prd->origin = P;
    prd->flags |= FLAG_SECONDARY;
}

/* deviceProgram.cu:340-475 for one pixel */
static void raygen_pixel(const orc_scene* s, const orc_probe* probe, const orc_params* prm, int ix, int iy, float* accum,
                         uint32_t* frame, float* normal_buf, float* color_buf, float* albedo_buf, orc_stats* st) {
    const int w = prm->width, h = prm->height;
    const f3 eye = mk3(prm->eye[0], prm->eye[1], prm->eye[2]);
    const f3 U = mk3(prm->U[0], prm->U[1], prm->U[2]), V = mk3(prm->V[0], prm->V[1], prm->V[2]),
             W = mk3(prm->W[0], prm->W[1], prm->W[2]);
    f3 result = mk3s(0.0f);
    const int spp = (int)prm->samples_per_launch;
    int i = spp;
    uint32_t seed = orc_tea4((uint32_t)(iy * w + ix), prm->subframe_index);
    f3 normal = mk3s(0.f), albedo = mk3s(0.f), alpha = mk3s(0.f), backplate = mk3s(0.f);
    do {
        f3 directLight = mk3s(0.0f), indirectLight = mk3s(0.0f);
        prd_t prd;
        prd.radiance = mk3s(0.f);
        prd.alpha = mk3s(0.f);
        orc_random_init(&prd.rand, seed);
        prd.rayEta = 1.0f;
        prd.throughput = mk3s(1.f);
        prd.bsdfPdf = 1.0f;
        prd.normal = mk3s(0.0f);
        prd.albedo = mk3s(0.0f);
        prd.flags = 0;
        prd.depth = 0;
        prd.origin = eye;
        prd.direction = mk3s(0.f);
        float jx = orc_rnd(&seed), jy = orc_rnd(&seed);
        float dx = 2.0f * (((float)ix + jx) / (float)w) - 1.0f;
        float dy = 2.0f * (((float)iy + jy) / (float)h) - 1.0f;
        f3 ray_direction = normalize3(add3(add3(scl3(U, dx), scl3(V, dy)), W));
        f3 ray_origin = eye;
        {
            float dir[3] = {ray_direction.x, ray_direction.y, ray_direction.z}, uv[2], px[4];
            orc_probe_dir_to_uv(dir, uv);
            orc_probe_eval(probe, uv, px);
            backplate = mk3(px[0], px[1], px[2]);
        }
        for (;;) {
            prd.radiance = mk3s(0.f);
            float t;
            st->radiance_rays++;
            int64_t prim = closest_hit(s, ray_origin, ray_direction, 0.001f, 1e16f, &t);
            if (prim >= 0) {
                closest_hit_program(s, probe, prm->bsdf_mode, (uint32_t)prim, ray_origin, ray_direction, t, &prd, st);
            } else { /* deviceProgram.cu:209-235 */
                prd.albedo = mk3s(0.f);
                prd.normal = mk3s(0.f);
                prd.flags |= FLAG_DONE;
            }
            if (prd.depth == 0) {
                normal = add3(normal, prd.normal);
                albedo = add3(albedo, prd.albedo);
            }
            if ((prd.flags & FLAG_DONE) || prd.depth >= prm->max_depth) break;
            if (prd.depth == 0)
                directLight = add3(directLight, prd.radiance);
            else
                indirectLight = add3(indirectLight, prd.radiance);
            ++prd.depth;
            ray_origin = prd.origin;
            ray_direction = prd.direction;
        }
        result = add3(result, add3(directLight, indirectLight));
        alpha = add3(alpha, prd.alpha);
    } while (--i);
    normal = div3s(normal, (float)spp);
    albedo = div3s(albedo, (float)spp);
    alpha = div3s(alpha, (float)spp);
    f3 color = add3(mul3(scl3(backplate, (float)spp), sub3(mk3s(1.0f), alpha)), result);
    const size_t image_index = (size_t)iy * w + ix;
    f3 accum_color = div3s(color, (float)spp);
    if (prm->subframe_index > 0) {
        accum_color = mk3(clampf(accum_color.x, 0.0f, 10.0f), clampf(accum_color.y, 0.0f, 10.0f),
                          clampf(accum_color.z, 0.0f, 10.0f));
        const float a = 1.0f / (float)(prm->subframe_index + 1);
        const f3 prev = mk3(accum[4 * image_index], accum[4 * image_index + 1], accum[4 * image_index + 2]);
        accum_color = lerp3(prev, accum_color, a);
    }
    float* o;
    o = &accum[4 * image_index]; o[0] = accum_color.x; o[1] = accum_color.y; o[2] = accum_color.z; o[3] = 1.0f;
    if (frame) {
        float c[3] = {accum_color.x, accum_color.y, accum_color.z};
        frame[image_index] = orc_make_color(c);
    }
    if (normal_buf) { o = &normal_buf[4 * image_index]; o[0] = normal.x; o[1] = normal.y; o[2] = normal.z; o[3] = 1.0f; }
    if (color_buf) { o = &color_buf[4 * image_index]; o[0] = accum_color.x; o[1] = accum_color.y; o[2] = accum_color.z; o[3] = 1.0f; }
    if (albedo_buf) { o = &albedo_buf[4 * image_index]; o[0] = albedo.x; o[1] = albedo.y; o[2] = albedo.z; o[3] = 1.0f; }
}

typedef struct {
    const orc_scene* s;
    const orc_probe* probe;
    const orc_params* prm;
    float* accum; uint32_t* frame; float *normal_buf, *color_buf, *albedo_buf;
    int tid, nthreads;
    orc_stats st;
} job_t;

static void* job_main(void* arg) {
    job_t* j = (job_t*)arg;
    for (int y = j->tid; y < j->prm->height; y += j->nthreads)
        for (int x = 0; x < j->prm->width; ++x)
            raygen_pixel(j->s, j->probe, j->prm, x, y, j->accum, j->frame, j->normal_buf, j->color_buf, j->albedo_buf,
                         &j->st);
    return NULL;
}

/* One optixLaunch(w,h,1) equivalent.  accum is read (subframe>0) and written.
 * nthreads rows are interleaved across threads; results do not depend on it. */
void orc_render(const orc_scene* s, const orc_probe* probe, const orc_params* prm, float* accum, uint32_t* frame,
                float* normal_buf, float* color_buf, float* albedo_buf, int nthreads, orc_stats* stats) {
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 256) nthreads = 256;
    job_t jobs[256];
    pthread_t th[256];
    for (int t = 0; t < nthreads; ++t) {
        job_t j = {s, probe, prm, accum, frame, normal_buf, color_buf, albedo_buf, t, nthreads, {0, 0}};
        jobs[t] = j;
        if (nthreads > 1) pthread_create(&th[t], NULL, job_main, &jobs[t]);
    }
    if (nthreads == 1) job_main(&jobs[0]);
    stats->radiance_rays = stats->shadow_rays = 0;
    for (int t = 0; t < nthreads; ++t) {
        if (nthreads > 1) pthread_join(th[t], NULL);
        stats->radiance_rays += jobs[t].st.radiance_rays;
        stats->shadow_rays += jobs[t].st.shadow_rays;
    }
}

/* Render only the listed rows of a full-size launch (same seeds as the full frame): lets a test check
 * windows of a 1920x1080 frame without rendering all of it on the CPU.  Only accum is written. */
typedef struct {
    const orc_scene* s; const orc_probe* probe; const orc_params* prm; float* accum; const int32_t* rows; int nrows;
    int tid, nthreads;
} rowjob_t;
static void* rowjob_main(void* arg) {
    rowjob_t* j = (rowjob_t*)arg;
    orc_stats st = {0, 0};
    for (int k = j->tid; k < j->nrows; k += j->nthreads)
        for (int x = 0; x < j->prm->width; ++x)
            raygen_pixel(j->s, j->probe, j->prm, x, j->rows[k], j->accum, NULL, NULL, NULL, NULL, &st);
    return NULL;
}
void orc_render_rows(const orc_scene* s, const orc_probe* probe, const orc_params* prm, float* accum, const int32_t* rows,
                     int nrows, int nthreads) {
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    rowjob_t jobs[64];
    pthread_t th[64];
    for (int t = 0; t < nthreads; ++t) {
        rowjob_t j = {s, probe, prm, accum, rows, nrows, t, nthreads};
        jobs[t] = j;
        pthread_create(&th[t], NULL, rowjob_main, &jobs[t]);
    }
    for (int t = 0; t < nthreads; ++t) pthread_join(th[t], NULL);
}

/* ---------------------------------------------------------------- foveated variant (HelloPathtracing_sv4_vmv23/)
 * One optixLaunch of the sv4 raygen (deviceProgram.cu:388-590): the launch index is remapped by
 * factor/offset, pixels outside the annulus [r_inner, r_outer] around c return early, the result is
 * splatted over fillSize^2 pixels, blended only when (subframe_index > 0 && !redraw), and only accum_buffer and
 * frame_buffer are written, the latter through exposure + Reinhard + make_color. */
typedef struct {
    uint32_t launch_w, launch_h;
    uint32_t factor_x, factor_y;
    int32_t fill_size;
    uint32_t cx, cy;
    float r_inner, r_outer;
    uint32_t offset_x, offset_y;
    uint32_t redraw;
    uint32_t spp;
    uint32_t subframe_index;
} orc_region;

static inline f3 reinhard(f3 color, float white) { /* sv4 deviceProgram.cu:124-128 */
    const float luminance = 0.2126f * color.x + 0.7152f * color.y + 0.0722f * color.z;
    return div3s(scl3(color, 1.0f), 1.0f + luminance / white);
}

static void raygen_region_thread(const orc_scene* s, const orc_probe* probe, const orc_params* prm, const orc_region* rg, uint32_t lx,
                                 uint32_t ly, float* accum, uint32_t* frame, float* normal_buf, float* color_buf, float* albedo_buf, orc_stats* st) {
    const int w = prm->width, h = prm->height;
    const f3 eye = mk3(prm->eye[0], prm->eye[1], prm->eye[2]);
    const f3 U = mk3(prm->U[0], prm->U[1], prm->U[2]), V = mk3(prm->V[0], prm->V[1], prm->V[2]), W = mk3(prm->W[0], prm->W[1], prm->W[2]);
    const int spp = (int)rg->spp;
    int i = spp;
    uint32_t seed = orc_tea4(ly * (uint32_t)w + lx, rg->subframe_index); /* seeded with the LAUNCH index (:406) */
    f3 result = mk3s(0.0f);
    const uint32_t ix = lx * rg->factor_x + rg->offset_x, iy = ly * rg->factor_y + rg->offset_y; /* :419, u32 wrap */
    {
        const f3 dv = sub3(mk3((float)ix, (float)iy, 0.0f), mk3((float)rg->cx, (float)rg->cy, 0.0f));
        const float range = sqrtf(dot3(dv, dv));
        if (range < rg->r_inner || range > rg->r_outer) return; /* :421-426 */
    }
    f3 alpha = mk3s(0.f), backplate = mk3s(0.f), normal = mk3s(0.f), albedo = mk3s(0.f);
    do {
        f3 directLight = mk3s(0.0f), indirectLight = mk3s(0.0f);
        prd_t prd;
        prd.radiance = mk3s(0.f);
        prd.alpha = mk3s(0.f);
        orc_random_init(&prd.rand, seed);
        prd.rayEta = 1.0f;
        prd.throughput = mk3s(1.f);
        prd.bsdfPdf = 1.0f;
        prd.normal = mk3s(0.0f);
        prd.albedo = mk3s(0.0f);
        prd.flags = 0;
        prd.depth = g_var.initial_depth; /* 0; sv / sv2: 1 (HelloPathtracing_sv/deviceProgram.cu:428) */
        prd.origin = eye;
        prd.direction = mk3s(0.f);
        float jx = orc_rnd(&seed), jy = orc_rnd(&seed);
        float dx = 2.0f * (((float)ix + jx) / (float)w) - 1.0f;
        float dy = 2.0f * (((float)iy + jy) / (float)h) - 1.0f;
        f3 ray_direction = normalize3(add3(add3(scl3(U, dx), scl3(V, dy)), W));
        f3 ray_origin = eye;
        {
            float dir[3] = {ray_direction.x, ray_direction.y, ray_direction.z}, uv[2], px[4];
            orc_probe_dir_to_uv(dir, uv);
            orc_probe_eval(probe, uv, px);
            backplate = mk3(px[0], px[1], px[2]);
        }
        for (;;) {
            prd.radiance = mk3s(0.f);
            float t;
            st->radiance_rays++;
            int64_t prim = closest_hit(s, ray_origin, ray_direction, g_var.radiance_tmin, 1e16f, &t);
            if (prim >= 0) {
                closest_hit_program(s, probe, prm->bsdf_mode, (uint32_t)prim, ray_origin, ray_direction, t, &prd, st);
            } else {
                prd.albedo = mk3s(0.f);
                prd.normal = mk3s(0.f);
                prd.flags |= FLAG_DONE;
            }
            if (prd.depth == 0) { /* sv :474-477 (never true when prd.depth starts at 1) */
                normal = add3(normal, prd.normal);
                albedo = add3(albedo, prd.albedo);
            }
            if ((prd.flags & FLAG_DONE) || prd.depth >= prm->max_depth) break;
            if (prd.depth == 0)
                directLight = add3(directLight, prd.radiance);
            else
                indirectLight = add3(indirectLight, prd.radiance);
            ++prd.depth;
            ray_origin = prd.origin;
            ray_direction = prd.direction;
        }
        result = add3(result, add3(directLight, indirectLight));
        alpha = add3(alpha, prd.alpha);
    } while (--i);
    alpha = div3s(alpha, (float)spp);
    normal = div3s(normal, (float)spp);
    albedo = div3s(albedo, (float)spp);
    for (int fi = 0; fi < rg->fill_size; ++fi) {
        for (int fj = 0; fj < rg->fill_size; ++fj) {
            uint32_t px = lx * rg->factor_x + (uint32_t)fi + rg->offset_x, py = ly * rg->factor_y + (uint32_t)fj + rg->offset_y;
            if (px > (uint32_t)(w - 1)) px = (uint32_t)(w - 1); /* clamp(index, 0, (w-1,h-1)) on unsigned */
            if (py > (uint32_t)(h - 1)) py = (uint32_t)(h - 1);
            const size_t image_index = (size_t)py * w + px;
            f3 color = add3(mul3(scl3(backplate, (float)spp), sub3(mk3s(1.0f), alpha)), result);
            f3 accum_color = div3s(color, (float)spp);
            if (rg->subframe_index > 0 && !rg->redraw) {
                accum_color = mk3(clampf(accum_color.x, 0.0f, 10.0f), clampf(accum_color.y, 0.0f, 10.0f), clampf(accum_color.z, 0.0f, 10.0f));
                const float a = 1.0f / (float)(rg->subframe_index + 1);
                const f3 prev = mk3(accum[4 * image_index], accum[4 * image_index + 1], accum[4 * image_index + 2]);
                accum_color = lerp3(prev, accum_color, a);
            }
            float* o = &accum[4 * image_index];
            o[0] = accum_color.x; o[1] = accum_color.y; o[2] = accum_color.z; o[3] = 1.0f;
            f3 shown = accum_color;
            if (g_var.tonemap == 1) shown = reinhard(scl3(accum_color, g_var.exposure), g_var.white);
            else if (g_var.tonemap == 2) shown = scl3(accum_color, g_var.exposure); /* sv3 :580-604: the Reinhard write is overwritten by make_color(exposure-corrected) */
            float c[3] = {shown.x, shown.y, shown.z};
            frame[image_index] = orc_make_color(c);
            if (g_var.write_aov && normal_buf && color_buf && albedo_buf) { /* sv :553-555 */
                float* nb = &normal_buf[4 * image_index];
                float* cb = &color_buf[4 * image_index];
                float* ab = &albedo_buf[4 * image_index];
                nb[0] = normal.x; nb[1] = normal.y; nb[2] = normal.z; nb[3] = 1.0f;
                cb[0] = accum_color.x; cb[1] = accum_color.y; cb[2] = accum_color.z; cb[3] = 1.0f;
                ab[0] = albedo.x; ab[1] = albedo.y; ab[2] = albedo.z; ab[3] = 1.0f;
            }
        }
    }
}

/* sequential over the launch grid (launches with overlapping splats are order-dependent in the reference too);
 * normal/color/albedo may be NULL (only written with var->write_aov) */
void orc_render_region_aov(const orc_scene* s, const orc_probe* probe, const orc_params* prm, const orc_region* rg, const orc_variant* var,
                           float* accum, uint32_t* frame, float* normal, float* color, float* albedo, orc_stats* stats) {
    g_var = *var;
    orc_stats st = {0, 0};
    for (uint32_t ly = 0; ly < rg->launch_h; ++ly)
        for (uint32_t lx = 0; lx < rg->launch_w; ++lx) raygen_region_thread(s, probe, prm, rg, lx, ly, accum, frame, normal, color, albedo, &st);
    if (stats) *stats = st;
    orc_variant def = {0.001f, 0, 0, 1.0f, 1.0f, 0, 0};
    g_var = def;
}
void orc_render_region(const orc_scene* s, const orc_probe* probe, const orc_params* prm, const orc_region* rg, const orc_variant* var,
                       float* accum, uint32_t* frame, orc_stats* stats) {
    orc_render_region_aov(s, probe, prm, rg, var, accum, frame, NULL, NULL, NULL, stats);
}

/* ---------------------------------------------------------------- AOV-guided a-trous filter (include/pt_amd.h pt_denoise)
 * The reference wires a denoiser pass (OptiXDenoiser::exec between render() and computeFinalPixelColors,
 * SimplePathtracer.cpp:104-105,138-146) whose implementation is empty (OptixDenoiser.cpp:15-18): there is no reference
 * behaviour to follow, so this restatement DEFINES the semantics ("parity unpinned").  One pass per iteration i with tap
 * spacing 2^i over a 5x5 B3-spline kernel, taps outside the image skipped, row-major summation, alpha carried through. */
static void atrous_pass(int w, int h, int step, float inv_color, float inv_normal, float inv_albedo, const float* src, const float* nrm,
                        const float* alb, float* dst) {
    static const float kern[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t ip = 4 * ((size_t)y * w + x);
            float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
            for (int dy = -2; dy <= 2; ++dy) {
                const int qy = y + dy * step;
                if (qy < 0 || qy >= h) continue;
                for (int dx = -2; dx <= 2; ++dx) {
                    const int qx = x + dx * step;
                    if (qx < 0 || qx >= w) continue;
                    const size_t iq = 4 * ((size_t)qy * w + qx);
                    const float dcx = src[ip] - src[iq], dcy = src[ip + 1] - src[iq + 1], dcz = src[ip + 2] - src[iq + 2];
                    const float dnx = nrm[ip] - nrm[iq], dny = nrm[ip + 1] - nrm[iq + 1], dnz = nrm[ip + 2] - nrm[iq + 2];
                    const float dax = alb[ip] - alb[iq], day = alb[ip + 1] - alb[iq + 1], daz = alb[ip + 2] - alb[iq + 2];
                    const float ec = (dcx * dcx + dcy * dcy + dcz * dcz) * inv_color;
                    const float en = (dnx * dnx + dny * dny + dnz * dnz) * inv_normal;
                    const float ea = (dax * dax + day * day + daz * daz) * inv_albedo;
                    const float wt = M_EXP(-fminf(ec + en + ea, 80.0f)) * (kern[dy + 2] * kern[dx + 2]);
                    sx += src[iq] * wt;
                    sy += src[iq + 1] * wt;
                    sz += src[iq + 2] * wt;
                    sw += wt;
                }
            }
            dst[ip] = sx / sw;
            dst[ip + 1] = sy / sw;
            dst[ip + 2] = sz / sw;
            dst[ip + 3] = src[ip + 3];
        }
}
void orc_denoise(int w, int h, int iterations, float sigma_color, float sigma_normal, float sigma_albedo, const float* color, const float* normal,
                 const float* albedo, float* out) {
    const size_t n = 4 * (size_t)w * h;
    if (iterations <= 0) {
        memcpy(out, color, sizeof(float) * n);
        return;
    }
    float* tmp = (float*)malloc(sizeof(float) * n);
    float* bufs[2] = {out, tmp};
    int cur = (iterations & 1) ? 0 : 1;
    const float* src = color;
    for (int i = 0; i < iterations; ++i) {
        const float sc = sigma_color / (float)(1 << i), sn = sigma_normal * (float)(1 << i);
        atrous_pass(w, h, 1 << i, 1.0f / (sc * sc), 1.0f / (sn * sn), 1.0f / (sigma_albedo * sigma_albedo), src, normal, albedo, bufs[cur]);
        src = bufs[cur];
        cur ^= 1;
    }
    free(tmp);
}

size_t orc_sizeof_material(void) { return sizeof(orc_material); }
int orc_detmath(void) {
#ifdef ORC_DETMATH
    return 1;
#else
    return 0;
#endif
}
