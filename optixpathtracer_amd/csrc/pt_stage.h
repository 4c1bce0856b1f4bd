// Staging of a vertex update on the GPU (pt_update_meshes_device, pt_transform_meshes; include/pt_amd.h): one launch writes the named
// meshes of a call into the scratch vertex array, from device arrays (a flat copy) or from the context's own positions through a 3x4
// matrix, and checks every coordinate it writes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One named mesh of the call.  A wave takes PT_STAGE_CHUNK elements of one segment — floats on the copy path, vertices on the transform
// path — so a segment of `count` elements owns the waves [first_wave, first_wave + ceil(count / PT_STAGE_CHUNK)).
struct StageSeg {
    const float* src;    // copy: the caller's 3 * nv floats (4-byte aligned, no more); transform: the mesh's source positions
    float* dst;          // the mesh's first float in the scratch vertex array
    uint64_t count;      // copy: 3 * nv; transform: nv
    uint32_t first_wave; // sum of the waves of the segments before this one
    uint32_t order;      // position of the mesh in the call: what the non-finite report holds
    uint32_t xform;      // 0: copy, 1: transform
    uint32_t pad_;
    float m[12];         // row-major 3x4
};
static_assert(sizeof(StageSeg) == 88, "StageSeg is uploaded as bytes");

constexpr uint32_t PT_STAGE_CHUNK = 512;        // elements per wave: 8 per lane
constexpr uint32_t PT_STAGE_NONE = 0xffffffffu; // *bad when every coordinate written was finite

// inf and NaN have all exponent bits set: a test on the bits, so no fast-math mode can fold it away
__device__ __forceinline__ bool stage_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ((a x + b y) + c z) + d, every operation rounded once: the documented order, which float32 NumPy reproduces bit for bit
__device__ __forceinline__ float stage_row(const float* __restrict__ m, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z)), m[3]);
}

// 256 threads = 4 waves; wave w of the grid serves the segment with first_wave <= w < next first_wave.  *bad receives the lowest `order`
// of a segment that wrote a non-finite coordinate: one atomicMin per wave, after the ballot over its lanes.
__global__ __launch_bounds__(256) void k_stage_vertices(const StageSeg* __restrict__ segs, uint32_t nseg, uint32_t nwaves, uint32_t* __restrict__ bad) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= nwaves) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t lo = 0, hi = nseg; // the last segment with first_wave <= wave (a segment without vertices owns no wave and is passed over)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (segs[mid].first_wave <= wave) lo = mid; else hi = mid;
    }
    const StageSeg& s = segs[lo];
    const uint64_t begin = (uint64_t)(wave - s.first_wave) * PT_STAGE_CHUNK;
    const uint64_t count = s.count;
    const uint64_t end = begin + PT_STAGE_CHUNK < count ? begin + PT_STAGE_CHUNK : count;
    typedef __attribute__((address_space(1))) float GlobalF; // pointers read from the table are generic to the compiler: say they are global
    const GlobalF* __restrict__ src = (const GlobalF*)s.src;
    GlobalF* __restrict__ dst = (GlobalF*)s.dst;
    bool ok = true;
    if (!s.xform) { // a flat run of floats: lane i reads float begin + i, 256 contiguous bytes per wave instruction
        for (uint64_t i = begin + lane; i < end; i += 64) {
            const float v = src[i];
            ok = ok && stage_finite(v);
            dst[i] = v;
        }
    } else {
        for (uint64_t i = begin + lane; i < end; i += 64) {
            const float x = src[3 * i + 0], y = src[3 * i + 1], z = src[3 * i + 2];
            const float ox = stage_row(s.m + 0, x, y, z), oy = stage_row(s.m + 4, x, y, z), oz = stage_row(s.m + 8, x, y, z);
            ok = ok && stage_finite(ox) && stage_finite(oy) && stage_finite(oz);
            dst[3 * i + 0] = ox;
            dst[3 * i + 1] = oy;
            dst[3 * i + 2] = oz;
        }
    }
    if (__ballot(!ok) != 0ull && lane == 0) atomicMin(bad, s.order);
}
