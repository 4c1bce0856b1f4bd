// Stand-in for <optix_device.h>, used only by oracle/ref_build/ref_device.cpp (test infrastructure).
// It is DISPATCH PLUMBING and nothing else: one thread-local record of the current launch index, ray, hit
// and payload words, the accessors deviceProgram.cu reads it through, and two optixTrace overloads that
// forward to ref_trace() in ref_device.cpp.  Which triangle a ray hits, at which t and with which
// barycentrics, is not decided here (ref_device.cpp takes it from the checker's own search).
#pragma once
#include <optix.h>  // ref_build/stub/optix.h: OptixTraversableHandle
typedef unsigned int OptixVisibilityMask;
enum { OPTIX_RAY_FLAG_NONE = 0, OPTIX_RAY_FLAG_TERMINATE_ON_FIRST_HIT = 1u << 2, OPTIX_RAY_FLAG_CULL_BACK_FACING_TRIANGLES = 1u << 4 };

struct RefTraceRecord {
    uint3 launch_index;
    float3 origin, direction;
    float t;
    unsigned int primitive;
    const void* sbt_data;
    float2 barycentrics;
    unsigned int payload[2];
};
extern thread_local RefTraceRecord ref_rec;
void ref_trace(OptixTraversableHandle handle, float3 o, float3 d, float tmin, float tmax, unsigned int flags, unsigned int sbt_offset,
               unsigned int miss_index, unsigned int* p0, unsigned int* p1);

static inline uint3 optixGetLaunchIndex() { return ref_rec.launch_index; }
static inline unsigned int optixGetPayload_0() { return ref_rec.payload[0]; }
static inline unsigned int optixGetPayload_1() { return ref_rec.payload[1]; }
static inline void optixSetPayload_0(unsigned int v) { ref_rec.payload[0] = v; }
static inline float3 optixGetWorldRayOrigin() { return ref_rec.origin; }
static inline float3 optixGetWorldRayDirection() { return ref_rec.direction; }
static inline float optixGetRayTmax() { return ref_rec.t; }
static inline unsigned int optixGetPrimitiveIndex() { return ref_rec.primitive; }
static inline unsigned long long optixGetSbtDataPointer() { return (unsigned long long)ref_rec.sbt_data; }
static inline float2 optixGetTriangleBarycentrics() { return ref_rec.barycentrics; }

static inline void optixTrace(OptixTraversableHandle h, float3 o, float3 d, float tmin, float tmax, float, OptixVisibilityMask, unsigned int flags,
                              unsigned int sbt_offset, unsigned int, unsigned int miss_index, unsigned int& p0) {
    unsigned int p1 = 0;
    ref_trace(h, o, d, tmin, tmax, flags, sbt_offset, miss_index, &p0, &p1);
}
static inline void optixTrace(OptixTraversableHandle h, float3 o, float3 d, float tmin, float tmax, float, OptixVisibilityMask, unsigned int flags,
                              unsigned int sbt_offset, unsigned int, unsigned int miss_index, unsigned int& p0, unsigned int& p1) {
    ref_trace(h, o, d, tmin, tmax, flags, sbt_offset, miss_index, &p0, &p1);
}

// texture fetch: forwarded to the checker's orc_tex2d by ref_device.cpp (the filter is ours, unpinned as before)
template <typename T> T tex2D(cudaTextureObject_t tex, float s, float t);
template <> float4 tex2D<float4>(cudaTextureObject_t tex, float s, float t);
