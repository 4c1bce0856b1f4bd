/* pt_amd.h — C ABI of libptamd.so, the MI355X-native replacement for the reference's
 * optixLaunch hot path (bipul-mohanto/OptixPathTracer, HelloPathtracing_original/).
 *
 * The reference has no FFI: its boundary is the C++ class SampleRenderer
 * (SimplePathtracer.h:38-176) plus the POD headers LaunchParams.h / Material.h /
 * Model.h / Probe.h.  A maintainer keeps that class (see INTEGRATION.md and
 * optixpathtracer_amd/csrc/SampleRenderer.h, a header-only facade with the same
 * public methods) and forwards each method to one entry point below.  Every entry
 * point cites the reference interface it replaces.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success
 * or a negative pt_status; no exception crosses the boundary; pt_last_error() gives
 * the message for the calling context (the reference throws sutil::Exception from
 * CUDA_CHECK/OPTIX_CHECK, sutil/Exception.h:93-195).  A context is single-threaded,
 * like the reference's renderer (one stream, device-synchronised render()).
 *
 * STREAM CONTRACT.  Every kernel and copy of a context runs on streams the context created with
 * hipStreamNonBlocking: they do NOT synchronise with the null stream or with any stream of the
 * caller (the current stream of a tensor framework included).  Entry points that take HOST pointers are complete when
 * they return.  Entry points that take or return DEVICE pointers — pt_pack, pt_unpack, pt_pack_async,
 * pt_unpack_display, pt_render_device, pt_device_buffer, pt_display_buffer, pt_update_meshes_device, pt_trace_device, pt_render_gbuffer, pt_temporal_accumulate, pt_filter_planes,
 * pt_copy_vertices_device, pt_motion_planes, pt_temporal_moments, pt_modulate_planes, pt_sample_plan, pt_temporal_carry, pt_copy_texcoords_device, pt_surface_planes,
 * pt_copy_texture_mips_device, pt_surface_lod_planes, pt_surface_aniso_planes, pt_upsample_planes — read and write them on
 * pt_stream(ctx), so:
 *   - a buffer the caller PRODUCED on another stream (the receive buffer of an all-gather, a buffer a
 *     memset just cleared) must be complete before the call: synchronise that stream on the host, or
 *     record an event on it and hand it to pt_wait_event(ctx, event) first (device-side ordering);
 *   - a buffer the library produced is complete when the call returned, for the synchronous entry
 *     points (pt_pack, pt_unpack, pt_render_device), and after pt_pack_wait / pt_display_sync for the
 *     asynchronous ones; to consume it on another stream without a host wait, enqueue the consumer
 *     on pt_stream(ctx) or make that stream wait for an event recorded on pt_stream(ctx).
 * pt_edge_aa_planes takes DEVICE pointers under the same contract: it is one more entry point of the list above (its ordering case
 * stands with its other GPU tests, in tests/test_gpu_edge_aa.py).  So do pt_exposure_planes and pt_tonemap_planes (their ordering
 * cases: tests/test_gpu_exposure.py).  pt_bloom_planes takes DEVICE pointers under the same contract, too (its ordering cases:
 * tests/test_gpu_bloom.py); pt_bloom_layout touches no device memory.  pt_motion_blur_planes takes DEVICE pointers under the same contract
 * (its ordering cases: tests/test_gpu_motion_blur.py); pt_motion_blur_layout touches no device memory.  pt_dof_planes takes DEVICE pointers
 * under the same contract (its ordering cases: tests/test_gpu_dof.py); pt_dof_layout touches no device memory.  pt_lens_warp_planes takes
 * DEVICE pointers under the same contract (its ordering cases: tests/test_gpu_lens_warp.py); pt_warp_matrix is host arithmetic and touches
 * no device at all.  pt_ao_planes takes DEVICE pointers under the same contract (its ordering case: tests/test_gpu_ao.py); pt_ao_layout
 * touches no device memory.  pt_reflect_planes takes DEVICE pointers under the same contract (its ordering case:
 * tests/test_gpu_reflect.py); pt_reflect_layout touches no device memory.  pt_shadow_planes takes DEVICE pointers under the same contract
 * (its ordering case: tests/test_gpu_shadow.py); pt_shadow_layout touches no device memory.
 *
 * VERSIONING.  pt_version() = "ptamd <major>.<minor> ...".  Structs only ever grow at the end; a caller
 * that may meet a newer or older library uses pt_get_stats_n(ctx, &s, sizeof s) (copies the common
 * prefix) instead of pt_get_stats, which writes sizeof(pt_stats) of the LIBRARY's header
 * (pt_stats_size()).  0.2 -> 0.4: pt_stats grew by bvh_builder + reserved_ (8 bytes), pt_multi_stats by
 * enqueue_ms, threads, frames_handed_over.  Entry points added since keep "0.4" (the string names the struct layouts, which they did not
 * change): pt_render_mask / pt_*adaptive*, pt_update_meshes_device / pt_transform_meshes, pt_trace_device / pt_query_wait, pt_set_views and
 * its camera setters, pt_render_gbuffer, pt_temporal_accumulate, pt_filter_planes, pt_vertex_count, pt_copy_vertices_device, pt_motion_planes,
 * pt_temporal_moments, pt_modulate_planes, pt_sample_plan, pt_temporal_carry, pt_copy_texcoords_device, pt_surface_planes,
 * pt_texture_mips_layout, pt_copy_texture_mips_device, pt_surface_lod_planes, pt_surface_aniso_planes, pt_upsample_planes, pt_edge_aa_planes,
 * pt_exposure_planes, pt_tonemap_planes.  A
 * caller that may meet an older library looks the symbol up (dlsym) before it relies on one.  pt_bloom_layout and pt_bloom_planes were added
 * in the same way and keep "0.4" as well; so were pt_motion_blur_layout and pt_motion_blur_planes, and pt_dof_layout and pt_dof_planes,
 * and pt_lens_warp_planes and pt_warp_matrix, and pt_ao_layout and pt_ao_planes, and
 * pt_reflect_layout and pt_reflect_planes, and pt_shadow_layout and pt_shadow_planes.
 */
#ifndef PT_AMD_H
#define PT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_ctx pt_ctx;

enum pt_status {
    PT_OK = 0,
    PT_ERR_INVALID = -1, /* bad argument / call order */
    PT_ERR_HIP = -2,     /* a HIP runtime call failed */
    PT_ERR_NO_DEVICE = -3,
    PT_ERR_UNSUPPORTED = -4
};

/* Material.h:47-68 — identical field order and size (104 bytes) */
typedef struct pt_material {
    float emission[3];
    float color[3];
    float absorption[3];
    float eta, metallic, subsurface, specular, roughness, specularTint, anisotropic, sheen, sheenTint, clearcoat,
        clearcoatGloss, transmission;
    float bump;
    float bumpTile[3];
    int32_t flags; /* bit0 = MATERIAL_FLAG_SHADOW_CATCHER (Material.h:9) */
} pt_material;

/* one TriangleMesh (Model.h:10-19): float3 vertices, uint3 indices, one material */
typedef struct pt_mesh_desc {
    const float* vertex; /* num_vertices * 3 */
    uint32_t num_vertices;
    const uint32_t* index; /* num_triangles * 3, local to this mesh */
    uint32_t num_triangles;
    pt_material material;
    int32_t diffuse_texture_id; /* index into pt_scene_desc.textures or -1 (TriangleMesh::diffuseTextureID) */
    const float* texcoord;      /* num_vertices * 2 (TriangleMesh::texcoord) or NULL */
} pt_mesh_desc;

/* Texture (Model.h:21-29): RGBA8 pixels, row 0 first (loadTexture already mirrored them in y, Model.cpp:112-121) */
typedef struct pt_texture_desc {
    const uint32_t* pixel;
    int32_t width, height;
} pt_texture_desc;

/* Model (Model.h:31-42) */
typedef struct pt_scene_desc {
    const pt_mesh_desc* meshes;
    uint32_t num_meshes;
    const pt_texture_desc* textures; /* may be NULL when num_textures == 0 */
    uint32_t num_textures;
} pt_scene_desc;

enum pt_bsdf_mode { PT_BSDF_DISNEY = 0, PT_BSDF_LAMBERT = 1 /* Disney.cuh:125-147 */ };

/* Everything the reference fixes at compile time (SURVEY.md §5 "config / flags") */
typedef struct pt_options {
    int32_t max_depth;      /* the literal 8 in deviceProgram.cu:429 */
    int32_t bsdf_mode;      /* pt_bsdf_mode */
    uint32_t max_paths;     /* paths in flight per wavefront batch (0 = default 8Mi; ≈280 bytes of path state and queues per path: 2.3 GB,
                             * three times that with frames_in_flight = 3, whose three batch sets each hold a whole frame) */
    int32_t kernel_timing;  /* 1: pt_stats.{trace,shadow,shade,other}_ms are measured with a pair of HIP events around every launch
                             *    (costs ≈0.3 ms of a 2 ms frame at a 1/8 share); 0 (default): only render_ms is measured */
    int32_t bvh_kind;       /* reserved, must be 0 (rounds 1-2: 1 = a binary BVH as an A/B path; removed — the 8-wide compressed tree is the structure) */
    int32_t trace_kernel;   /* reserved, must be 0 (rounds 1-2: 1 = the first grid-stride traversal kernel; removed) */
    int32_t streams;        /* pixel chunks of a frame run concurrently on this many stream pairs (0 = default 3, the measured optimum: tails of one chunk overlap the bulk of the others) */
    int32_t split_shadow;   /* 0 = default: shadow rays of bounce b share a launch with the closest-hit rays of b+1; 1 = separate kernels;
                             * 2 = asynchronous: per-bounce shadow records traced on side streams, nothing waits for them before the
                             *     resolve, which sums the visible contributions in bounce order (not with shadow-catcher materials) */
    int32_t frames_in_flight; /* 0 / 1 = default: pt_render returns when its frame is complete, like SampleRenderer::render()
                             * (SimplePathtracer.cpp:96 CUDA_SYNC_CHECK).  2 or 3: pt_render(k) enqueues frame k and returns once at most
                             * frames_in_flight - 1 frames are still running, so the kernel tails of a frame overlap the next frames (same
                             * images, bit for bit).  2: the frame is still cut into one pixel chunk per stream; every chunk stream orders
                             * its own frames and nothing else holds frame k+1 back.  3 (what bench.py times): frame k runs WHOLE on
                             * stream k mod `streams`, three frames overlap and every launch carries three times the rays; only the
                             * resolves, which blend into accum_buffer, are chained from frame to frame.  A single frame followed by a
                             * wait is slower in that mode than the default (one stream, no overlap inside the frame): it is for loops.
                             * Frame k completes — and its errors are reported — at a later pt_render, at pt_sync, or at any call that
                             * reads or changes device state (pt_download, pt_get_stats, pt_device_buffer, pt_resize, ...).
                             * pt_render_regions with 2 or 3: the frame's launches keep their schedule (passes dealt to the streams in turn) but
                             * no longer start together, and the first resolve of a frame waits for the end of the previous frame.  Ignored
                             * (synchronous) with kernel_timing and for a pt_multi_render that hands the frame over (gather_mask != 0 or
                             * host_rgba8); a pt_multi_render with neither keeps the frames in flight on every device. */
} pt_options;

enum pt_buffer {          /* LaunchParams.frame.* (LaunchParams.h:53-63) */
    PT_BUF_ACCUM = 0,     /* float4 accum_buffer */
    PT_BUF_FRAME = 1,     /* uchar4 frame_buffer (make_color) */
    PT_BUF_COLOR = 2,     /* float4 color_buffer */
    PT_BUF_NORMAL = 3,    /* float4 normal_buffer */
    PT_BUF_ALBEDO = 4,    /* float4 albedo_buffer */
    PT_BUF_DENOISED = 5   /* float4 denoisedBuffer (SimplePathtracer.h:149-150); allocated by the first pt_denoise */
};

typedef struct pt_stats {
    uint64_t radiance_rays; /* closest-hit rays traced by the last pt_render */
    uint64_t shadow_rays;   /* any-hit rays traced by the last pt_render */
    uint64_t paths;         /* camera paths started (pt_render_regions: launch indices x samples, before annulus / partition culling) */
    double render_ms;       /* device time of the last pt_render (hipEvent, stream-local) */
    double trace_ms;        /* with pt_options.kernel_timing (else 0) — of which: closest-hit traversal kernels */
    double shadow_ms;       /*           any-hit traversal kernels */
    double shade_ms;        /*           shade kernels */
    double other_ms;        /*           generate / resolve */
    uint32_t trace_launches, shadow_launches, shade_launches;
    uint32_t bvh_nodes;     /* internal nodes of the traversal structure */
    uint64_t bvh_bytes;     /* nodes + leaf triangles resident in HBM */
    double bvh_build_ms;    /* one-time on-GPU build (excluded from render_ms) */
    uint32_t bvh_levels;    /* levels of the traversal structure (must not exceed the traversal stack: pt_create checks) */
    uint64_t shaded_hits;   /* closest hits shaded by the last render whose BSDF sample was accepted (every one cost a BSDFSample, two
                             * BSDFEval and two BSDFPdf: the unit of the shade kernel's FLOP roofline) */
    uint64_t frames;        /* frames completed since pt_create, and the rays they traced: take differences around a */
    uint64_t total_radiance_rays; /* sequence of pt_render calls (pt_get_stats itself waits for the frames in flight) */
    uint64_t total_shadow_rays;
    uint32_t bvh_builder;   /* hierarchy under the wide tree: 0 = LBVH (Morton order), 1 = PLOC, 2 = imported (PT_BVH_IMPORT), 3 = binned SAH (round 5).
                             * pt_create builds the three and keeps the one through which a fixed batch of calibration rays takes fewest traversal
                             * steps; PT_BVH_BUILDER=lbvh|ploc|sah forces one, PT_BVH_SAH=0 leaves the SAH candidate out.  Images do not
                             * depend on the choice (closest hit, lowest primitive on ties, hits confined to the triangle's padded box). */
    uint32_t fused_passes;  /* passes of the last render that ran as ONE persistent kernel (generate -> trace -> shade rounds per wave, no launch
                             * chain: small synchronous frames, PT_FUSED; csrc/pt_fused.h); trace_launches counts each of them once.
                             * WHICH frames: a synchronous pt_render / pt_render_batch of a scene without shadow-catcher materials, default
                             * pt_options.streams and split_shadow, of at most PT_SCHED_MAX_PATHS (4.5 M) paths is rendered alternately as a
                             * launch chain and as one fused pass over its first 2 x (1 + PT_SCHED_TRIALS) frames (both leave the same bits)
                             * and then by whichever measured faster; `schedule`, `sched_chain_ms`, `sched_fused_ms` below report it.  The
                             * first trial frame — and every frame when PT_SCHED_TRIALS=0 — follows the rule of round 5: fused when the frame
                             * has at most PT_FUSED_MAX_PATHS (2.5 M) paths and the tree's calibration rays cost at most PT_FUSED_MAX_COST
                             * (22) traversal steps; a tree that was never calibrated (PT_BVH_BUILDER forced, PT_BVH_IMPORT, a challenger that
                             * could not be built) counts as expensive unless the scene has fewer than 4096 triangles. */
    uint32_t path_state_allocs; /* (re-)allocations of the per-path device state since pt_create.  The state only grows (sets, paths per set,
                             * pixels per set, each kept at the largest value any frame asked for), so alternating schedules — a fused-size
                             * synchronous frame, a foveated frame, frames in flight — re-allocates at most once per dimension. */
    uint32_t bvh_challengers_skipped; /* candidate hierarchies pt_create could not build (out of device memory, a failed bounds check): the standing
                             * tree then stayed without a comparison — also reported on stderr; 0 in every healthy build */
    uint32_t schedule;      /* how the last synchronous pt_render ran: 0 launch chain, 1 fused bounce loop (k_path_loop); bit 8 set while the context
                             * is still timing the two against each other for this frame configuration (sched_chain_ms / sched_fused_ms below; `fused_passes` above says which frames take part);
                             * bit 9 set when launch chains of the last render carried the paths' sums with their queue entries (PT_CARRY_SUMS);
                             * bit 10 set when its paths kept the first-hit normal and albedo as one word (PT_LEAN_FIRST) */
    double sched_chain_ms;  /* best device time of the configuration's trial frames as a launch chain / as one fused pass (0: not measured: */
    double sched_fused_ms;  /* the configuration is not eligible for both, or PT_SCHED_TRIALS=0) */
    double create_ms;       /* host time of pt_create from the flattened scene to the finished context: uploads, the acceleration structure
                             * (bvh_build_ms is the part between its first and last kernel), the probes that pick the streams — and, in the first
                             * pt_create of a process, what loading the library's code objects costs beyond the time the scene upload hides */
    uint32_t marg_lds_words_full; /* 4-byte words of the probe's marginal (row) arrays a shade workgroup copies to LDS, in the full layout and in */
    uint32_t marg_lds_words_lean; /* the lean one (PT_SHADE_LDS); 0: no probe set, or its row search reads global memory (more than 2048 rows, or a
                             * row count that is no multiple of 64) */
} pt_stats;

/* SampleRenderer::SampleRenderer(const Model*) (SimplePathtracer.cpp:39-71): uploads the meshes
 * (buildAccel :481-489) and textures (createTextures :603-654; sampled in software: wrap, bilinear, normalised
 * float, no sRGB), builds the acceleration structure ON THE GPU (replaces optixAccelBuild +
 * optixAccelCompact :561-591) and the per-mesh material table (replaces buildSBT :390-455).
 * `device` is the HIP device ordinal.  The scene is deep-copied; the caller keeps its arrays. */
int pt_create(const pt_scene_desc* scene, int device, pt_ctx** out_ctx);

/* no reference counterpart (the reference leaks everything at exit, CUDABuffer.h:32-88) */
int pt_destroy(pt_ctx* ctx);

const char* pt_last_error(const pt_ctx* ctx); /* ctx may be NULL: last error of a failed pt_create */

int pt_set_options(pt_ctx* ctx, const pt_options* opt);
int pt_get_options(const pt_ctx* ctx, pt_options* opt);

/* SampleRenderer::setProbe(const ProbeData&) (SimplePathtracer.cpp:164-180) + CUDAProbeData::createBuffer
 * (Probe.h:102-124): copies the five host arrays to the device. data = w*h float4; pdfX,cdfX = w*h; pdfY,cdfY = h */
int pt_set_probe(pt_ctx* ctx, const float* data_rgba, const float* pdfX, const float* cdfX, const float* pdfY,
                 const float* cdfY, int width, int height);

/* main.cpp:146-156 loadProbe + ProbeData::BuildCDF (Probe.h:29-77) + setProbe in one call, with the CDF built ON THE
 * GPU: one wave per row loads 64 texels at a time and every lane runs the reference's sequential
 * left-to-right float running sum over them (so the arrays are bit-identical to the host BuildCDF; a parallel scan would
 * reassociate the sums); one wave does the same over the row totals.  data = w*h float4. */
int pt_set_probe_image(pt_ctx* ctx, const float* data_rgba, int width, int height);
/* read back the device CDF arrays (pdfX,cdfX: w*h floats; pdfY,cdfY: h floats); any pointer may be NULL */
int pt_get_probe_cdf(pt_ctx* ctx, float* pdfX, float* cdfX, float* pdfY, float* cdfY);

/* ProbeData::BuildCDF (Probe.h:29-77), host side like the reference. Pure function, no context. */
int pt_build_cdf(const float* data_rgba, int width, int height, float* pdfX, float* cdfX, float* pdfY, float* cdfY);

/* SampleRenderer::resize(const int2&) (SimplePathtracer.cpp:109-147): (re)allocates the five frame
 * buffers; a 0-sized request is ignored like the reference (:112). */
int pt_resize(pt_ctx* ctx, int width, int height);

/* SampleRenderer::setCamera (SimplePathtracer.cpp:155-162): eye + the UVW frame of sutil::Camera::UVWFrame */
int pt_set_camera(pt_ctx* ctx, const float eye[3], const float U[3], const float V[3], const float W[3]);

/* sutil::Camera::UVWFrame (sutil/Camera.cpp:34-45), host side. Pure function. */
int pt_uvw_frame(const float eye[3], const float lookat[3], const float up[3], float fovY_deg, float aspect,
                 float U[3], float V[3], float W[3]);

/* Multi-GPU image partition (no reference counterpart; pattern of sutil/WorkDistribution.h:34-91):
 * the image is cut into tile_w x tile_h tiles and this context renders only tiles with
 * (tile_x + tile_y) % world == rank.  Default is rank 0 of 1.  Must be called before pt_resize
 * or is applied at the next pt_resize. */
int pt_set_partition(pt_ctx* ctx, int rank, int world, int tile_w, int tile_h);

/* SampleRenderer::render() (SimplePathtracer.cpp:73-97): one optixLaunch(w,h,1) equivalent with
 * launchParams.samples_per_launch = spp and launchParams.frame.subframe_index = subframe_index;
 * returns after the device finished (the reference ends render() in cudaDeviceSynchronize, :96).
 * Silently does nothing before the first pt_resize (:77). If host_rgba8 is non-NULL the frame
 * buffer is copied into it (render(CUDAOutputBuffer&) + downloadPixels, :99-107,149-153). */
int pt_render(pt_ctx* ctx, uint32_t spp, uint32_t subframe_index, uint32_t* host_rgba8);
/* `count` consecutive launches of the reference's progressive loop — render() with subframe_index = first_subframe, first_subframe + 1, ...
 * (main.cpp:273-278 renders, displays and increments every frame) — as ONE wavefront batch: the generate / traversal / shade launches carry
 * the rays of all `count` subframes (seeds are tea<4>(pixel, subframe_index), deviceProgram.cu:357: subframes are independent until they
 * blend) and the resolve blends them into accum_buffer in subframe order (:460-466).  All five buffers end up bit-identical to `count`
 * calls of pt_render; what changes is the number of rays per launch, which is what a small share of a tile-partitioned frame lacks
 * (a 1/8 share of 1080p x 4 spp is 1 M paths; a persistent traversal wave wants several chunks of work).  The intermediate frames are
 * not displayed: a display loop that shows every frame keeps calling pt_render.  count in [1,4096]; pt_render == count 1.
 * pt_stats.frames advances by count. */
int pt_render_batch(pt_ctx* ctx, uint32_t spp, uint32_t first_subframe, uint32_t count, uint32_t* host_rgba8);
/* SampleRenderer::render(sutil::CUDAOutputBuffer<uint32_t>&) (SimplePathtracer.cpp:99-107): the rgba8 frame lands in a caller-owned
 * DEVICE buffer (width*height*4 bytes on the context's device; the reference aliases the caller's mapped buffer as frame_buffer for
 * the launch).  Synchronous like render(): the buffer is complete when the call returns (also with frames in flight).
 * A pointer HIP does not know (plain malloc'ed host memory) is refused with PT_ERR_INVALID before anything is rendered. */
int pt_render_device(pt_ctx* ctx, uint32_t spp, uint32_t subframe_index, void* dev_rgba8);
/* SampleRenderer::stream (SimplePathtracer.h:107, handed to the display path at main.cpp:245): the hipStream_t (as void*) on which the
 * context's packs, unpacks, epilogues and device copies run — see STREAM CONTRACT at the top. */
void* pt_stream(pt_ctx* ctx);
/* Device-side ordering instead of a host wait: everything the context enqueues on pt_stream(ctx) from now on waits for `hip_event`
 * (a hipEvent_t the caller recorded on its own stream after producing a buffer it is about to hand in).  No reference counterpart. */
int pt_wait_event(pt_ctx* ctx, void* hip_event);
/* Waits for the frames in flight (pt_options.frames_in_flight = 2 or 3) and reports their errors; a no-op otherwise.  No reference
 * counterpart: the reference's render() is synchronous. */
int pt_sync(pt_ctx* ctx);

/* Foveated variants (the HelloPathtracing_sv, _sv2, _sv3, _sv4_vmv23 directories; sv and sv2 share one device
 * program and differ from sv3/sv4 by pt_variant.initial_depth / write_aov and their host schedules).  One pt_region = one optixLaunch of the sv4 raygen
 * (HelloPathtracing_sv4_vmv23/deviceProgram.cu:388-590): LaunchParams.frame.{factor,fillSize,c,r_inner,r_outer,offset,
 * redraw} (sv4 LaunchParams.h:62-70) + the launch dimensions, samples_per_launch and subframe_index of that launch. */
typedef struct pt_region {
    uint32_t launch_w, launch_h;  /* optixLaunch width/height */
    uint32_t factor_x, factor_y;  /* frame.factor */
    int32_t fill_size;            /* frame.fillSize: the result is splatted over fill_size^2 pixels */
    uint32_t cx, cy;              /* frame.c: gaze point in pixels */
    float r_inner, r_outer;       /* pixels whose distance to c is outside [r_inner, r_outer] are skipped */
    uint32_t offset_x, offset_y;  /* frame.offset */
    uint32_t redraw;              /* 1: never blend with accum_buffer */
    uint32_t spp;                 /* samples_per_launch */
    uint32_t subframe_index;
} pt_region;

/* what the sv3/sv4 device code changed relative to the canonical variant */
typedef struct pt_variant {
    float radiance_tmin;          /* 0.001 canonical (deviceProgram.cu:420); 0.01 sv4 (global tmin, sv4 :41,485) */
    int32_t cull_back_occlusion;  /* 0 canonical (TERMINATE_ON_FIRST_HIT); 1 sv3/sv4 (CULL_BACK_FACING_TRIANGLES, sv4 :240) */
    int32_t tonemap;              /* 0: make_color(accum); 1: make_color(reinhard(accum * exposure, white)) (sv4 :555-569);
                                   * 2: make_color(accum * exposure) (sv3 :580-604, where the later plain write wins) */
    float exposure;               /* sv4: pow(2,2) = 4; sv3: pow(2,3) = 8 */
    float white;                  /* sv4: 1 */
    int32_t initial_depth;        /* prd.depth at the camera ray: 0 canonical/sv3/sv4; 1 in sv and sv2 (HelloPathtracing_sv/deviceProgram.cu:428,
                                   * with the cutoff `prd.depth >= 3` at :483 = pt_options.max_depth 3): every contribution then goes to
                                   * indirectLight and no first-hit normal/albedo is ever accumulated */
    int32_t write_aov;            /* 1: the launch also writes normal_buffer, color_buffer and albedo_buffer like sv/sv2 (:553-555); 0: accum/frame only (sv3/sv4) */
} pt_variant;

/* SampleRenderer::render() of the foveated variants (HelloPathtracing_sv4_vmv23/SimplePathtracer.cpp:77-216): the
 * given launches in order (later ones overwrite earlier pixels).  Depth cutoff = pt_options.max_depth (sv4: 4).
 * Writes accum_buffer and frame_buffer (plus the three AOV buffers with pt_variant.write_aov).  variant may be NULL (canonical settings). */
int pt_render_regions(pt_ctx* ctx, const pt_region* regions, uint32_t n, const pt_variant* variant, uint32_t* host_rgba8);

/* BLOCK MASKS AND ADAPTIVE STOPPING (no reference counterpart): render only chosen 8x8 blocks of the image.
 * A block is one 8x8 tile of the image grid: bx = x / 8, by = y / 8, nbx = (width + 7) / 8, nby = (height + 7) / 8, block id by * nbx + bx
 * (edge blocks hold fewer than 64 pixels).  On a partitioned context (pt_set_partition) only the blocks the rank owns count; tile sizes are
 * multiples of 8, so a block never straddles ranks.  A pixel's result depends on nothing but (x, y, subframe_index, spp) and its own previous
 * accum value, so the pixels of a rendered block get the bits a full frame gives them.
 *
 * pt_render_mask: one byte per block (nbx * nby, host memory), non-zero = render this block.  Pixels of rendered blocks end up exactly as
 * pt_render(spp, subframe_index) leaves them, in all five buffers; pixels of other blocks are not touched in any buffer.  A compaction kernel
 * builds the list of active pixels on the device in the order of the rank's own list (whole blocks, block order kept); its count comes back
 * with one 4-byte copy and the frame then runs through the code of pt_render.  Synchronous whatever pt_options.frames_in_flight says: frames
 * in flight are waited for first and the call is complete when it returns.  The on-line schedule trial (pt_stats.schedule) neither sees nor
 * is reset by a masked frame: it takes the launch chain or the fused pass by the static rule on its own path count (both leave the same
 * bits; PT_FUSED=0/1 still forces it), and it never asks for more path state than the rank's full frame of the same samples does: after a full
 * frame it allocates nothing (pt_stats.path_state_allocs), before one it may grow the state up to that shape.  pt_stats of the call describe the active pixels only.  Zero active
 * pixels: no kernel launch, PT_OK.  Refused with PT_ERR_INVALID (text in pt_last_error): null context or mask, no pt_resize yet, spp
 * outside [1,4096]. */
int pt_render_mask(pt_ctx* ctx, uint32_t spp, uint32_t subframe_index, const uint8_t* block_mask,
                   uint32_t* host_rgba8 /* may be NULL; else the whole frame buffer */, uint32_t* active_pixels /* may be NULL */);

/* The policy on top of it: a progressive loop in which every block stops being rendered once its pixels have converged.
 *
 * Moments.  For every pixel a pt_render_adaptive call renders, the resolve records the value c that enters the blend (the subframe's own
 * colour, clamped to [0,10] when subframe_index > 0, unclamped at subframe 0): x = 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z evaluated
 * left to right, then n += 1, s1 += x, s2 += x * x.  pt_render and pt_render_mask never touch this state.
 *
 * Stopping rule, evaluated on the device after the resolve for the blocks the call rendered; float32 throughout, one rounding per
 * operation (no fused multiply-add), in exactly this order.  n = the block's subframe count, N = its pixel count as a float:
 *   per pixel p:  m_p = s1_p / n;   v_p = max(0, s2_p / n - m_p * m_p)
 *   V = sum v_p, M = sum m_p: each a butterfly over 64 slots, slot l = the pixel (8 bx + (l & 7), 8 by + (l >> 3)), slots outside the image
 *       hold 0; for off = 32, 16, 8, 4, 2, 1: every slot l becomes slot[l] + slot[l ^ off] (all slots end up equal)
 *   B = M + dark_floor * N;   lhs = V * N;   rhs = (((threshold * threshold) * (n - 1)) * B) * B
 *   the block stops when (n >= min_subframes and lhs <= rhs) or (max_subframes > 0 and n >= max_subframes)
 * i.e. the RMS standard error of a pixel's mean, relative to the block's mean luminance (plus dark_floor), is at most `threshold`.  A
 * stopped block stays stopped until the next pt_adaptive_begin.  Non-finite moments: the colour of subframe 0 enters unclamped, so an inf or
 * NaN sample there makes s1 or s2 of its pixel non-finite for good; lhs <= rhs is then false (a comparison with NaN, or inf <= inf * 0 -> NaN)
 * and the block is never stopped by the rule, only by max_subframes.  A loop that waits for active_blocks == 0 should therefore set
 * max_subframes (or bound its own iteration count). */
typedef struct pt_adaptive_params {
    float    threshold;     /* >= 0; see the rule above */
    float    dark_floor;    /* >= 0, added to the block's mean luminance (so that near-black blocks can stop) */
    uint32_t min_subframes; /* >= 2: a block is never stopped by the rule with fewer subframes behind it */
    uint32_t max_subframes; /* 0 = no limit; a block stops once it has this many */
} pt_adaptive_params;
typedef struct pt_adaptive_stats {
    uint32_t blocks, active_blocks;     /* owned blocks; still active after the last call */
    uint64_t active_pixels;             /* rendered by the last call */
    uint64_t pixel_subframes;           /* sum over owned pixels of subframes rendered since pt_adaptive_begin */
    double   decide_ms;                 /* device time of the compaction + decision kernels of the last call (events) */
} pt_adaptive_stats;
/* (re)allocates and clears the state, all owned blocks active; call it after a camera move, where one restarts at subframe 0.
 * Refused: null context or params, no pt_resize yet, min_subframes < 2, negative or non-finite threshold / dark_floor. */
int pt_adaptive_begin(pt_ctx* ctx, const pt_adaptive_params* params);
/* pt_render_mask with the blocks that are still active, recording the moments; then the decision for those blocks and the compaction for
 * the next call, both behind the frame on the device (their count returns with the frame's own final synchronisation: no host round trip
 * in front of a frame).  Synchronous.  With no block left it launches nothing.  Refused without pt_adaptive_begin. */
int pt_render_adaptive(pt_ctx* ctx, uint32_t spp, uint32_t subframe_index, uint32_t* host_rgba8 /* may be NULL */, pt_adaptive_stats* out /* may be NULL */);
/* frees the state; pt_resize, pt_set_partition and pt_destroy imply it */
int pt_adaptive_end(pt_ctx* ctx);
enum pt_adaptive_array { PT_ADAPT_MOMENTS = 0 /* width*height x {n, s1, s2, 0} f32 */, PT_ADAPT_ACTIVE = 1 /* nbx*nby u8 (0 for blocks of other ranks) */ };
int pt_download_adaptive(pt_ctx* ctx, int which /* pt_adaptive_array */, void* host, size_t bytes);

/* VIEWPORTS (no reference counterpart): several cameras rendered into rectangles of ONE frame, in one wavefront batch, over one copy of the
 * scene and its acceleration structure — a stereo pair for a head-mounted display, a camera array for synthetic data.
 *
 * What a view pixel holds.  Frame pixel (X, Y) inside view v has local coordinates x = X - v.x, y = Y - v.y and is rendered exactly as
 * pixel (x, y) of a v.width x v.height frame with camera v: seed tea4(y * v.width + x, subframe), jitter 2 * ((x + jx) / v.width) - 1 (and
 * likewise with y, jy, v.height), direction normalize(dx*U + dy*V + W) with v's vectors, origin v.eye; the backplate in the resolve comes from
 * the same ray.  Its five buffers at (X, Y) get the bits pt_render(spp, subframe_index) would leave at (x, y) of such a context, given the
 * same previous accum value.  A pixel in no view is not touched in any buffer by any render call.  pt_set_camera is remembered but unused
 * while views are set; it is in force again after pt_set_views(n = 0).
 *
 * pt_set_views is refused with PT_ERR_INVALID (text in pt_last_error, nothing changed) for: a null context; null `views` with n > 0; no
 * pt_resize yet; n > PT_MAX_VIEWS; x or y negative or not a multiple of 8; width or height < 1; a rectangle leaving the frame; two
 * rectangles sharing a pixel.  With origins on the 8x8 block grid and no shared pixels a block touches at most one view; the device code
 * looks the view up by block.
 *
 * Ordering.  pt_set_views and both camera setters wait for the frames in flight first (pt_options.frames_in_flight), as pt_resize does, and
 * are complete when they return.  A loop that moves its cameras every frame therefore runs one frame at a time; camera updates that do not
 * wait for the frames in flight are not part of this interface.
 *
 * pt_set_view_cameras / pt_set_view_cameras_device: n x 12 floats (eye, U, V, W per view, in the order of pt_set_views); n must equal the
 * current view count, else PT_ERR_INVALID.  They change cameras only — the rectangles and the pixel list stay as they are — so this is the
 * per-frame call.  Values are taken as given, as pt_set_camera takes them.  The device variant checks its pointer as pt_trace_device checks
 * its arrays (known to HIP, device memory of the context's device, 4-byte aligned, fitting its allocation; otherwise PT_ERR_INVALID), reads
 * the values on pt_stream(ctx) under the STREAM CONTRACT and returns when the copy is complete.
 *
 * State changes.  pt_resize and pt_set_partition drop the views: the order of calls is partition, resize, views.  pt_set_views implies
 * pt_adaptive_end.
 *
 * Honoured by pt_render, pt_render_batch and pt_render_device (launch chain and fused pass, frames_in_flight 0-3), by pt_render_mask (it
 * renders the view pixels of the blocks the mask names, and active_pixels counts those), on a partitioned context (the view pixels of the
 * blocks the rank owns; ownership stays a function of frame coordinates) and by pt_multi_render / pt_multi_render_batch.  Refused with
 * PT_ERR_UNSUPPORTED while views are set, state unchanged: pt_render_regions and pt_multi_render_regions (the foveated launches have their
 * own index mapping) and pt_adaptive_begin.  pt_denoise, pack / unpack and the downloads work on the whole buffers as before; the a-trous
 * filter does not know about view borders (its taps cross them).
 *
 * pt_stats.paths and the ray counts describe the pixels rendered.  The on-line chain/fused trial (pt_stats.schedule) treats a change of
 * the views' pixel count as any other change of the frame's path count, and a frame with views never asks for more path state than the
 * rank's full frame at the same samples. */
#define PT_MAX_VIEWS 4096
typedef struct pt_view {            /* 64 bytes */
    int32_t x, y;                   /* top-left pixel of the rectangle in the frame; multiples of 8 */
    int32_t width, height;          /* >= 1; the rectangle lies inside the frame */
    float eye[3], U[3], V[3], W[3]; /* what pt_set_camera takes */
} pt_view;
int pt_set_views(pt_ctx* ctx, const pt_view* views, uint32_t n); /* n == 0 (views may be NULL): back to the single camera */
int pt_get_views(const pt_ctx* ctx, pt_view* out /* may be NULL */, uint32_t cap, uint32_t* n /* may be NULL: the view count */); /* copies min(cap, count) views */
int pt_set_view_cameras(pt_ctx* ctx, const float* cams /* n x 12: eye,U,V,W */, uint32_t n);            /* host memory */
int pt_set_view_cameras_device(pt_ctx* ctx, const float* dev_cams /* n x 12 */, uint32_t n);            /* device memory */

/* SampleRenderer::downloadPixels (SimplePathtracer.cpp:149-153), generalised to all five buffers.
 * bytes must equal width*height*(16 or 4). */
int pt_download(pt_ctx* ctx, int which /* pt_buffer */, void* host, size_t bytes);

/* progressive state: overwrite accum_buffer (checkpoint/resume of an accumulation) */
int pt_upload_accum(pt_ctx* ctx, const float* host_rgba, size_t bytes);

/* device pointer of a frame buffer, for zero-copy consumers (display interop in the reference:
 * render(CUDAOutputBuffer&) maps the caller's buffer, SimplePathtracer.cpp:99-107) */
void* pt_device_buffer(pt_ctx* ctx, int which);

/* toneMap.cu:41-70 computeFinalPixelColors: rgba8 = clamp(sqrt(accum))*255.9 into the frame buffer
 * (the reference's disabled alternative epilogue, SimplePathtracer.cpp:105). */
int pt_tonemap_sqrt(pt_ctx* ctx, uint32_t* host_rgba8 /* may be NULL */);

/* The denoiser pass the reference wires up but leaves empty: OptiXDenoiser::{init,exec,finish} (OptixDenoiser.h:12-31,
 * OptixDenoiser.cpp:15-42 — init() has no body) with DenoiseData{width,height,color,albedo,normal,output} set in
 * resize() (SimplePathtracer.cpp:138-146) and the disabled calls "denoiser.exec(); computeFinalPixelColors(size,
 * denoisedBuffer, result)" in render(target) (SimplePathtracer.cpp:104-105).  Here exec() is an edge-avoiding
 * a-trous wavelet filter (Dammertz et al. 2010) guided by the first-hit normal and albedo AOVs the hot path already
 * writes: `iterations` passes of a 5x5 B3-spline kernel with tap spacing 2^i; tap weight =
 * k[dx]*k[dy] * exp(-|c_p-c_q|^2 / (sigma_color*2^-i)^2) * exp(-|n_p-n_q|^2 / (4^i * sigma_normal^2)) *
 * exp(-|a_p-a_q|^2 / sigma_albedo^2); taps outside the image are skipped; alpha is carried through.
 * input: PT_BUF_COLOR (this frame's radiance, what DenoiseData.color points at) or PT_BUF_ACCUM (the progressive
 * average).  epilogue: 0 none, 1 computeFinalPixelColors (toneMap.cu:41-58, as in the disabled call), 2 make_color;
 * 1 and 2 write the rgba8 frame buffer.  Works on the full-size buffers of this context (multi-GPU: after pt_unpack
 * of the three inputs).  The reference has no behaviour to match here: the CPU checker defines the semantics. */
typedef struct pt_denoise_params {
    int32_t iterations;   /* 0..8; 0 copies the input */
    float sigma_color;    /* > 0 */
    float sigma_normal;   /* > 0 */
    float sigma_albedo;   /* > 0 */
    int32_t input;        /* PT_BUF_COLOR or PT_BUF_ACCUM */
    int32_t epilogue;     /* 0, 1, 2 */
} pt_denoise_params;
int pt_denoise(pt_ctx* ctx, const pt_denoise_params* params, uint32_t* host_rgba8 /* may be NULL */, double* kernel_ms /* may be NULL */);

/* Multi-GPU exchange helpers. pt_owned_pixels = number of pixels this rank renders (padded count is
 * the same on every rank: pt_owned_pixels_padded). pt_pack packs this rank's pixels of buffer `which`
 * into dev_dst (padded count * elem bytes); pt_unpack scatters the concatenation of all ranks' packs
 * (world * padded * elem bytes, rank-major — exactly what an RCCL all-gather produces) into the
 * full-size local buffer `which`. */
int pt_owned_pixels(const pt_ctx* ctx, uint32_t* owned, uint32_t* padded);
int pt_pack(pt_ctx* ctx, int which, void* dev_dst);
int pt_unpack(pt_ctx* ctx, int which, const void* dev_src_all);

/* Display hand-off that overlaps the next frame (the reference's loop renders, then displays, every frame: main.cpp:273-278; on several
 * GPUs "display" is preceded by the exchange of the ranks' strips).  With pt_options.frames_in_flight = 2 or 3 the loop is
 *     pt_render(k);  pt_pack_async(FRAME, send[k & 1], k & 1);
 *     if (k > 0) { pt_pack_wait((k - 1) & 1);  all-gather(recv, send[(k - 1) & 1]);  pt_unpack_display(FRAME, recv);  show pt_display_buffer(FRAME); }
 * pt_pack_async enqueues the pack of buffer `which` behind the newest frame in flight WITHOUT waiting for it (pt_pack waits) and makes
 * the resolves of later frames wait for it, so the strip is frame k's whatever is enqueued next; pt_pack_wait blocks the host until that
 * strip is complete (frames enqueued after it keep running); pt_unpack_display scatters the all-gathered strips into the DISPLAY copy
 * of the buffer — a second, full-size buffer no render writes (allocated on first use) — so the exchange and display of frame k-1
 * overlap the rendering of frame k and never show pixels of two frames.  pt_display_sync waits for the newest pt_unpack_display,
 * pt_download_display copies a display buffer to the host.  Same bits as pt_pack / pt_unpack. */
int pt_pack_async(pt_ctx* ctx, int which, void* dev_dst, int slot /* 0 or 1: which of the caller's two send buffers */);
int pt_pack_wait(pt_ctx* ctx, int slot);
int pt_unpack_display(pt_ctx* ctx, int which, const void* dev_src_all);
int pt_display_sync(pt_ctx* ctx);
void* pt_display_buffer(pt_ctx* ctx, int which); /* NULL until the first pt_unpack_display of that buffer */
int pt_download_display(pt_ctx* ctx, int which, void* host, size_t bytes);

int pt_get_stats(const pt_ctx* ctx, pt_stats* out);
/* size-checked variant (see VERSIONING): copies min(out_bytes, pt_stats_size()) bytes, zero-fills the rest */
int pt_get_stats_n(const pt_ctx* ctx, void* out, size_t out_bytes);
size_t pt_stats_size(void);

/* ---------------------------------------------------------------------------------------------------------------------
 * Several GPUs from ONE process (SURVEY.md 8b "pt_create_multi"; the reference renders on whatever single device is
 * current, SimplePathtracer.cpp:203-212).  A pt_multi is ndev contexts — rank r on HIP device devices[r] — that share
 * one flattened scene (uploaded to every device, acceleration structure built on each), the same probe / camera /
 * options, and one frame cut into interleaved tile_w x tile_h tiles (pt_set_partition with world = ndev, the pattern of
 * sutil/WorkDistribution.h:34-91).  pt_multi_render enqueues the frame on every device before it waits for any, so
 * the devices work concurrently from one host thread; no collective is on the data path.  The display hand-off,
 * pt_multi_gather, makes a buffer complete on EVERY rank: pack of the owned pixels -> one all-gather of the packed
 * strips -> unpack.  The all-gather is RCCL's ncclAllGather, one communicator per rank inside one ncclGroup
 * (librccl is opened on first use); when two ranks share a device (rehearsal on a one-GPU box: RCCL refuses duplicate
 * devices) or librccl is absent, the strips travel as direct device-to-device copies (hipMemcpyPeerAsync over xGMI).
 * devices may repeat.  Every call returns a pt_status; pt_multi_last_error gives the message. */
typedef struct pt_multi pt_multi;
enum pt_exchange { PT_EXCHANGE_NONE = 0, PT_EXCHANGE_RCCL = 1, PT_EXCHANGE_PEER_COPY = 2 };
typedef struct pt_multi_stats {
    pt_stats sum;            /* rays / paths / frames summed over the ranks (frames = frames x ranks); the *_ms fields are the MAXIMUM over the ranks */
    double gather_ms;        /* wall time of the last pt_multi_gather (pack + exchange + unpack, all ranks); overlapped hand-off: host time of the exchange of the previous frame */
    int32_t exchange;        /* pt_exchange used by the last gather */
    int32_t ndev;
    double enqueue_ms;       /* host time of the enqueue phase of the last render (all launches of the frame on every device): the slowest
                              * rank's when the ranks have their own threads, the sum over the ranks otherwise */
    int32_t threads;         /* host threads that enqueue the ranks (0: the calling thread does it for all — one rank, or PT_MULTI_THREADS=0) */
    uint64_t frames_handed_over; /* frames that went through the overlapped hand-off (frames in flight + gather_mask) */
} pt_multi_stats;
int pt_create_multi(const pt_scene_desc* scene, const int* devices, int ndev, pt_multi** out);
int pt_multi_destroy(pt_multi* m);
const char* pt_multi_last_error(const pt_multi* m); /* m may be NULL: last error of a failed pt_create_multi */
int pt_multi_size(const pt_multi* m);
pt_ctx* pt_multi_ctx(pt_multi* m, int rank); /* the rank's context, for per-rank calls (pt_download, pt_get_stats, pt_device_buffer) */
int pt_multi_set_options(pt_multi* m, const pt_options* opt);
int pt_multi_set_probe(pt_multi* m, const float* data_rgba, const float* pdfX, const float* cdfX, const float* pdfY, const float* cdfY, int width, int height);
int pt_multi_set_probe_image(pt_multi* m, const float* data_rgba, int width, int height);
int pt_multi_resize(pt_multi* m, int width, int height, int tile_w, int tile_h); /* tile sizes: multiples of 8; 0 = 64 x 16 */
int pt_multi_set_camera(pt_multi* m, const float eye[3], const float U[3], const float V[3], const float W[3]);
/* VIEWPORTS on every rank (after pt_multi_resize): each rank renders the view pixels of the blocks it owns; the gathers are unchanged */
int pt_multi_set_views(pt_multi* m, const pt_view* views, uint32_t n);
int pt_multi_set_view_cameras(pt_multi* m, const float* cams /* n x 12, host memory */, uint32_t n);
/* gather_mask: bit (1 << pt_buffer) for every buffer to assemble on all ranks after the frame (0 = none: pure throughput);
 * host_rgba8 (may be NULL) receives rank 0's frame buffer and implies gathering PT_BUF_FRAME.
 * Every rank's launches are enqueued by a host thread of its own (pt_multi_stats.enqueue_ms, .threads), so the host time of a frame does
 * not grow with the number of devices.
 * With pt_options.frames_in_flight = 2 or 3 AND something to hand over, the hand-over overlaps the next frame: the call enqueues frame k,
 * then exchanges the strips frame k-1 packed behind its last kernel and scatters them into the ranks' DISPLAY buffers (pt_display_buffer /
 * pt_download_display of pt_multi_ctx(m, r); the ordinary buffers keep only the rank's own pixels) while frame k renders, and returns
 * when frame k-1 is on display: host_rgba8 receives frame k-1 (nothing on the first call), pt_multi_flush hands over the last frame.
 * Same bits as the synchronous hand-over. */
int pt_multi_render(pt_multi* m, uint32_t spp, uint32_t subframe_index, uint32_t gather_mask, uint32_t* host_rgba8);
/* pt_render_batch on every rank: `count` subframes in one wavefront batch per device, then the hand-over of the last one */
int pt_multi_render_batch(pt_multi* m, uint32_t spp, uint32_t first_subframe, uint32_t count, uint32_t gather_mask, uint32_t* host_rgba8);
int pt_multi_render_regions(pt_multi* m, const pt_region* regions, uint32_t n, const pt_variant* variant, uint32_t gather_mask, uint32_t* host_rgba8);
int pt_multi_gather(pt_multi* m, int which /* pt_buffer */);
int pt_multi_flush(pt_multi* m, uint32_t* host_rgba8 /* may be NULL */); /* overlapped hand-off: the newest frame goes on display now */
int pt_multi_get_stats(const pt_multi* m, pt_multi_stats* out);

/* Ray-search entry (what optixTrace did: deviceProgram.cu:165,190).  rays = n * 8 floats
 * (o.xyz, tmin, d.xyz, tmax) in HOST memory.  any_hit=0: t_out[n], prim_out[n] (global triangle
 * index in mesh order, -1 = miss; t_out = tmax on miss).  any_hit=1: prim_out[n] = 1 occluded / 0.
 * iters>1 repeats the kernel for timing; kernel_ms (may be NULL) receives the mean kernel time. */
int pt_trace(pt_ctx* ctx, const float* rays, uint32_t n, int any_hit, float* t_out, int32_t* prim_out, int iters,
             double* kernel_ms);

/* Ray queries from and to GPU memory (what optixTrace is to an application's own buffers): pt_trace with the rays and the results in DEVICE
 * memory, hit attributes, no per-call allocation and, with PT_QUERY_ASYNC, no host wait.  A simulation, picking, lidar, baking or collision
 * step that keeps its rays in a tensor asks its question without a host copy; together with pt_update_meshes_device / pt_transform_meshes a
 * whole interactive loop stays on the GPU.
 * Pointers and streams:
 *   - dev_rays (n x 8 floats: o.xyz, tmin, d.xyz, tmax) and dev_out (PT_QUERY_CLOSEST: n x pt_hit; PT_QUERY_ANY: n x int32) live on the
 *     context's device and are read and written on pt_stream(ctx), under the STREAM CONTRACT: rays produced on another stream must be
 *     complete, or ordered with pt_wait_event, before the call;
 *   - before any device work each pointer is checked with hipPointerGetAttributes, exactly as pt_update_meshes_device checks its arrays: a
 *     null pointer, a pointer HIP does not know, host memory (pinned or managed included), memory of another device, a pointer that is not
 *     4-byte aligned, an array that does not fit into what is left of its allocation, input and output ranges that overlap, unknown flag
 *     bits or more than 2^31 rays return PT_ERR_INVALID, and nothing is enqueued.  No wider alignment than 4 bytes is assumed (a tensor
 *     slice is routinely offset by one float); arrays that happen to be 16-byte aligned are moved with 16-byte loads and stores;
 *   - n == 0 returns PT_OK and launches nothing.
 * Validity of a ray, decided on the device by the staging kernel with tests on the exponent bits:
 *   - a ray is valid when its eight words are finite and s = (dx*dx + dy*dy) + dz*dz and 1.0f / s are both finite and non-zero (float32, one
 *     rounding per operation: what the traversal divides by);
 *   - an invalid ray never enters the traversal with its own values: it is staged as the neutral ray o = (0,0,0), tmin = 1, d = (0,0,1),
 *     tmax = -1 and remembered in a bit mask of its own (one bit per ray), so a caller's own ray (0,0,0,1, 0,0,1,-1) is still an ordinary miss;
 *   - it is reported as prim = -2 (closest hit) or -2 (any hit) and counted in invalid_rays; the call still returns PT_OK;
 *   - a valid ray with tmax <= tmin is an ordinary miss.
 * Results:
 *   - t and prim are pt_trace's, bit for bit (and so the CPU checker's); mesh is the leaf triangle's mesh word; ng is the geometric normal
 *     k_shade uses, normalize(cross(v1 - v0, v2 - v0)), not flipped towards the ray;
 *   - u, v are optixGetTriangleBarycentrics — the weights of vertex 1 and vertex 2 — from the triangle's vertices and the ray as given, by the
 *     expression the shade kernel uses for textured hits; float32, one rounding per operation, no fused multiply-add, dot = (x + y) + z:
 *       A = v0 - o, B = v1 - o, C = v2 - o;  Uw = dot(d, cross(C, B)), Vw = dot(d, cross(A, C)), Ww = dot(d, cross(B, A));
 *       det = (Uw + Vw) + Ww;  u = Vw / det;  v = Ww / det
 *     (float32 NumPy evaluating this reproduces them bit for bit);
 *   - any-hit output: 1 occluded, 0 not occluded, -2 invalid.
 * Ordering and completion:
 *   - the call first waits for the frames in flight, like pt_trace (queries already queued keep running);
 *   - without PT_QUERY_ASYNC it is complete when it returns and *stats describes what pt_query_wait would: the queries since the last wait
 *     (this one alone unless asynchronous ones were pending);
 *   - with PT_QUERY_ASYNC it returns after enqueueing on pt_stream(ctx) — no allocation after the first query of that size, no host copy, no
 *     synchronisation — and does not touch stats.  Results are complete after pt_query_wait or pt_sync; a consumer on another stream may
 *     instead wait for an event recorded on pt_stream(ctx).  Several asynchronous queries may be queued: they run in stream order;
 *   - pt_query_wait waits for the queued queries and reports the sums over the queries since the last pt_query_wait (or synchronous query).
 *     The traversal's stack-overflow bit is read there and gives PT_ERR_UNSUPPORTED, as in pt_trace;
 *   - every entry point that waits for the frames in flight (pt_update_meshes*, pt_resize, pt_get_stats, pt_destroy, ...) completes the queued
 *     queries first; what they counted stays for the next pt_query_wait.  A query enqueued after a mesh update sees the new geometry.
 * State: the staged rays, the hit records, the marks and a small counter block live in the context, are allocated by the first query, grow
 * when a query has more rays than any before it (never shrink) and are freed by pt_destroy; state_bytes reports their size.  If growing
 * fails the call returns PT_ERR_HIP and the context is unchanged. */
enum pt_query_flags { PT_QUERY_CLOSEST = 0, PT_QUERY_ANY = 1, PT_QUERY_ASYNC = 2 /* or-able with either */ };
typedef struct pt_hit {       /* 32 bytes, one per ray, closest-hit queries */
    float   t;                /* hit distance; the ray's own tmax on a miss; 0 for an invalid ray */
    float   u, v;             /* barycentric weights of vertex 1 and vertex 2; 0 when there is no hit */
    int32_t prim;             /* global triangle index in mesh order (pt_trace's); -1 miss; -2 invalid ray */
    int32_t mesh;             /* index into pt_scene_desc.meshes (= material record); -1 when there is no hit */
    float   ng[3];            /* geometric normal, not flipped towards the ray; 0 when there is no hit */
} pt_hit;
typedef struct pt_query_stats {
    uint64_t rays, hits, invalid_rays;      /* hits: closest hits found / rays found occluded */
    double stage_ms, trace_ms, attrib_ms;   /* device time of the three kernels (hipEvents) */
    uint64_t state_bytes;                   /* device memory the query state currently holds */
} pt_query_stats;
int pt_trace_device(pt_ctx* ctx, const float* dev_rays, uint32_t n, uint32_t flags /* pt_query_flags */, void* dev_out, pt_query_stats* stats /* may be NULL */);
int pt_query_wait(pt_ctx* ctx, pt_query_stats* stats /* may be NULL */);

/* FIRST-HIT G-BUFFER (no reference counterpart): what lies under the centre of every pixel of the frame, under the frame's camera or under
 * each view's (pt_set_views) — ids, barycentrics and normal, depth, position, screen-space motion against the previous frame's cameras —
 * written by one kernel into the caller's DEVICE planes.  What a synthetic-data pipeline stores beside the colour image, and what a
 * head-mounted display loop or a temporal filter reprojects with.
 * The ray of a pixel.  Frame pixel (X, Y) has local coordinates (x, y) in its camera: the frame's, or with views the camera of the pixel's
 * view (x = X - v.x, y = Y - v.y, width and height the view's).  The ray is the raygen prologue's with both jitter values replaced by 0.5f:
 *     dx = 2 * ((x + 0.5f) / width) - 1;  dy = 2 * ((y + 0.5f) / height) - 1;  dir = normalize3((U * dx + V * dy) + W)
 *     origin eye, tmin 0.001f, tmax 1e16f
 * float32, one rounding per operation, no fused multiply-add, dot = (x*x + y*y) + z*z, normalize3(v) = v * (1 / sqrt(dot(v, v))): float32
 * NumPy evaluating this reproduces the `ray` plane bit for bit.
 * Planes (caller-owned device memory of the context's device, frame-sized, indexed Y * width + X in frame coordinates; any subset, NULL =
 * not wanted).  With (t, leaf) the closest hit of that ray as pt_trace defines it:
 *   - ray:      the eight words o.xyz, tmin, d.xyz, tmax — pt_trace_device's ray layout;
 *   - hit:      the pt_hit that pt_trace_device(PT_QUERY_CLOSEST) returns for that ray, all eight words (a miss: t = 1e16f, prim = mesh = -1,
 *               the rest 0);
 *   - depth:    t * dot3(dir, normalize3(W)), the distance along the viewing axis; a miss holds +inf (0x7f800000);
 *   - position: (o.x + t*dir.x, o.y + t*dir.y, o.z + t*dir.z, 1.0f); a miss holds four zeros;
 *   - motion:   where this surface point was in the previous image minus where it is now, in pixels of the pixel's own camera rectangle.
 *               With the previous camera (e', U', V', W') of the pixel's view (of the frame without views), q = position - e' for a hit and
 *               q = dir for a miss (the environment is a point at infinity):
 *                   a = dot3(q, cross3(V', W'));  b = dot3(q, cross3(W', U'));  c = dot3(q, cross3(U', V'));  det = dot3(U', cross3(V', W'))
 *                   px = (((a / c) + 1) * 0.5f) * width - 0.5f;  py = (((b / c) + 1) * 0.5f) * height - 0.5f
 *                   motion = (px - (float)x, py - (float)y)
 *               When c * det > 0 is false (behind the previous camera, c == 0, a NaN) both words are 0x7fc00000.  Motion is camera motion
 *               over the CURRENT geometry; it knows nothing of geometry that moved (pt_motion_planes below gives the planes for that).
 * Which pixels: those a pt_render_mask with the same mask would render — the rank's owned pixels (pt_set_partition), view pixels only while
 * views are set, whole blocks of block_mask (NULL: every block).  A pixel outside that set is not written in any plane.  Zero active
 * pixels launch nothing and return PT_OK.
 * Pointers and streams: each plane is checked as pt_trace_device checks its arrays (known to HIP, device memory of the context's device,
 * 4-byte aligned, fitting what is left of its allocation) and the planes may not overlap one another; they are written on pt_stream(ctx)
 * under the STREAM CONTRACT.  No wider alignment than 4 bytes is assumed (records are written with 16-byte stores at whatever address they have).
 * prev_cameras and block_mask are HOST memory.
 * Ordering and state: the call first waits for the frames in flight and completes queued queries, and is complete when it returns.  It sees
 * the current geometry (after any pt_update_meshes*).  It neither reads nor writes the five frame buffers, the accumulation, the adaptive
 * state, the schedule trial or the path state; pt_stats is as it was.  The traversal's stack-overflow bit gives PT_ERR_UNSUPPORTED, as in
 * pt_trace.
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet; all five
 * planes NULL; a plane that fails the pointer checks or overlaps another plane; motion without prev_cameras; num_prev_cameras different
 * from max(1, view count) when prev_cameras is given; a non-finite previous camera value.
 * stats: pixels written; hits among them; device time of the pass (hipEvents; the mask compaction included when there is a mask).
 * Not part of this interface: an asynchronous variant, a pt_multi_* wrapper (per-rank calls through pt_multi_ctx work), G-buffers of the
 * foveated launches, object-space motion (a pass of its own: pt_motion_planes). */
typedef struct pt_gbuffer_desc {
    void*  hit;       /* width*height x pt_hit (32 B)            or NULL */
    float* depth;     /* width*height x f32                      or NULL */
    float* position;  /* width*height x 4 f32                    or NULL */
    float* motion;    /* width*height x 2 f32                    or NULL */
    float* ray;       /* width*height x 8 f32 (pt_trace_device's ray layout) or NULL */
    const float*   prev_cameras;     /* HOST, n x 12 (eye,U,V,W); required iff motion != NULL */
    uint32_t       num_prev_cameras; /* 1 without views, else the view count */
    const uint8_t* block_mask;       /* HOST, nbx*nby bytes as pt_render_mask, or NULL = every block */
} pt_gbuffer_desc;
typedef struct pt_gbuffer_stats { uint64_t pixels, hits; double kernel_ms; } pt_gbuffer_stats;
int pt_render_gbuffer(pt_ctx* ctx, const pt_gbuffer_desc* desc, pt_gbuffer_stats* stats /* may be NULL */);

/* TEMPORAL ACCUMULATION (no reference counterpart): reproject last frame's accumulated colour to where each surface point was, check that it
 * is the same surface, blend with a per-pixel history length, restart only the pixels that were disoccluded.  With pt_render_gbuffer in front
 * (hit, position, motion) and pt_denoise behind, a complete reproject / accumulate / filter chain for cameras that move every frame; it works
 * per view.  The call is stateless: every plane is caller-owned DEVICE memory of the context's device, frame-sized, indexed Y * width + X, and
 * checked exactly as pt_render_gbuffer checks its planes (known to HIP, device memory of the context's device, 4-byte aligned — no wider
 * alignment is assumed — fitting what is left of its allocation).  A pointer obtained from pt_device_buffer is accepted like any other.
 * Which pixels: exactly those pt_render_gbuffer would write with the same mask — the rank's owned pixels, view pixels only while views are
 * set, whole blocks of block_mask (HOST memory, NULL: every block).  No other pixel is written in any output.  Zero pixels launch nothing
 * and return PT_OK.
 * Each pixel works inside its own rectangle (x0, y0, wr, hr): its view (found by the pixel's 8x8 block), or the whole frame without views;
 * (x, y) are its local coordinates there.  Arithmetic per pixel p — float32 throughout, one rounding per operation, no fused multiply-add,
 * in exactly this order, dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; float32 NumPy evaluating this reproduces every output bit for bit:
 *   1. c = color[p].xyz * color_scale.  With PT_TEMPORAL_CLEAR_COLOR the four words of color[p] become 0 after the read.
 *   2. px = (float)x + motion[p].x;  py = (float)y + motion[p].y.  The lookup fails when (px >= -1 && px <= wr && py >= -1 && py <= hr) is
 *      false (a NaN motion word fails this way).  Otherwise flx = floorf(px), ix = (int)flx, fx = px - flx, likewise fly, iy, fy;
 *      wx0 = 1 - fx, wx1 = fx, wy0 = 1 - fy, wy1 = fy; tap weights w_ij = wx_i * wy_j.
 *   3. Tap (i, j) is frame pixel q = (x0 + ix + i, y0 + iy + j).  It counts when it lies inside the rectangle, w_ij > 0, length_in[q] >= 1,
 *      the three colour words of history_in[q] are finite (exponent-bit test) and the geometry agrees: with hit[p].prim < 0 (a miss) it
 *      needs prev_hit[q].prim < 0; otherwise prev_hit[q].mesh == hit[p].mesh, dot3(ng_p, ng_q) >= normal_cos and
 *      fabsf(dot3(ng_p, prev_position[q].xyz - position[p].xyz)) <= plane_eps * hit[p].t.
 *   4. Tap order (0,0), (1,0), (0,1), (1,1); a tap that does not count contributes +0.0f.  Wsum = ((w00 + w10) + w01) + w11; Hsum the same
 *      sum of w_ij * history_in[q] per component; nprev the minimum of length_in[q] over the counting taps;
 *      valid = (at least one tap counts) && Wsum >= min_weight.
 *   5. Valid: H = Hsum / Wsum; n = fminf(nprev, (float)(max_history - 1)); a = 1.0f / (n + 1.0f); out = H + (c - H) * a; len = n + 1.
 *      Otherwise out = c, len = 1.
 *   6. history_out[p] = (out, 1.0f); length_out[p] = len; frame_rgba8[p] = make_color(out); copy_out[p] = (out, 1.0f);
 *      stats->reprojected counts the valid pixels.
 * Overlap: each of the four outputs may overlap no other plane (the kernel gathers neighbours, so the caller ping-pongs history and
 * length); color may overlap no other plane; the read-only planes may alias one another (prev_hit == hit, say).
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet; a required
 * plane NULL (all but frame_rgba8, copy_out and block_mask); a plane that fails the pointer checks; a forbidden overlap; unknown flag bits; a
 * parameter out of its range or not finite.
 * Ordering and state, as pt_render_gbuffer: the call first waits for the frames in flight and completes queued queries, runs on
 * pt_stream(ctx) under the STREAM CONTRACT and is complete when it returns; the previous planes must be complete before the call.  It reads
 * and writes no context state except through the pointers the caller passed: the frame buffers, the accumulation, the adaptive state, the
 * schedule trial and pt_stats are as they were.  A partitioned context needs no special case: pixels the rank never wrote keep
 * length_in == 0, so those taps do not count, and a caller that all-gathers history and length gets a seamless image.
 * Per-frame colour recipe.  The resolve of subframe k > 0 leaves prev + (clamp(c) - prev) / (k + 1) in the accumulation buffer.  To hand this
 * pass one frame's colour: color = pt_device_buffer(PT_BUF_ACCUM), color_scale = (float)(k + 1) (1 for the frame rendered at subframe 0), and
 * PT_TEMPORAL_CLEAR_COLOR so that the next frame's blend starts from zero.  Seeds then differ from frame to frame, and the recipe works with
 * views, masks and partitions; the recovered colour differs from the frame's own by two roundings.  Without views, a full-frame
 * pt_render_regions launch with redraw = 1 is the exact alternative.
 * stats: pixels processed; valid pixels among them; device time of the pass (hipEvents; the mask compaction included when there is a mask).
 * Not part of this interface: an asynchronous variant, a pt_multi_* wrapper, variance estimates, motion of moving geometry inside this call (the motion
 * plane is camera motion only), any change to pt_denoise. */
enum pt_temporal_flags { PT_TEMPORAL_CLEAR_COLOR = 1 };
typedef struct pt_temporal_desc {
    float* color;              /* w*h x 4  this frame's colour; read, and zeroed afterwards with PT_TEMPORAL_CLEAR_COLOR */
    const float* motion;       /* w*h x 2  pt_render_gbuffer's motion plane of this frame */
    const void*  hit;          /* w*h x pt_hit, this frame */
    const float* position;     /* w*h x 4, this frame */
    const void*  prev_hit;     /* previous frame's hit plane */
    const float* prev_position;
    const float* history_in;   /* w*h x 4  accumulated colour after the previous frame */
    const float* length_in;    /* w*h f32  per-pixel history length (whole numbers; 0 = no history) */
    float* history_out;        /* w*h x 4 */
    float* length_out;         /* w*h */
    uint32_t* frame_rgba8;     /* w*h or NULL: make_color(out) */
    float* copy_out;           /* w*h x 4 or NULL: a second copy of (out,1), e.g. pt_device_buffer(PT_BUF_COLOR) for pt_denoise */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    float color_scale;         /* finite, > 0 */
    float normal_cos;          /* [-1,1] */
    float plane_eps;           /* finite, >= 0 */
    float min_weight;          /* [0,1] */
    uint32_t max_history;      /* 1..65535 */
    uint32_t flags;            /* PT_TEMPORAL_CLEAR_COLOR = 1 */
} pt_temporal_desc;
typedef struct pt_temporal_stats { uint64_t pixels, reprojected; double kernel_ms; } pt_temporal_stats;
int pt_temporal_accumulate(pt_ctx* ctx, const pt_temporal_desc* desc, pt_temporal_stats* stats /* may be NULL */);

/* VARIANCE-GUIDED A-TROUS FILTER OVER THE G-BUFFER'S PLANES (no reference counterpart): the last stage of the reproject / accumulate / filter
 * chain, for what pt_temporal_accumulate leaves.  Unlike pt_denoise it is guided by the exact first-hit planes of pt_render_gbuffer (hit,
 * position) with the geometry tests of pt_temporal_accumulate — one notion of "same surface" for the whole chain —, its colour weight follows
 * a per-pixel variance, no tap crosses a view border, and it works on exactly the pixel set pt_render_mask would render.  The call is
 * stateless: every plane is caller-owned DEVICE memory of the context's device, frame-sized, indexed Y * width + X, and checked exactly as
 * pt_render_gbuffer checks its planes (known to HIP, device memory of the context's device, 4-byte aligned — no wider alignment is assumed —
 * fitting what is left of its allocation).  A pointer obtained from pt_device_buffer is accepted like any other.
 * Which pixels: exactly those pt_render_gbuffer would write with the same mask — the rank's owned pixels, view pixels only while views are
 * set, whole blocks of block_mask (HOST memory, NULL: every block).  No other pixel is written in out, scratch or frame_rgba8; inside the
 * set the contents scratch is left with are unspecified.  Zero pixels launch nothing and return PT_OK.
 * Each pixel works inside its own rectangle: its view (found by the pixel's 8x8 block), or the whole frame without views.
 * Arithmetic per pixel p — float32 throughout, one rounding per operation, no fused multiply-add, in exactly this order; float32 NumPy
 * evaluating this reproduces every output bit for bit (a NaN is a NaN: its sign and payload are not specified), with
 *     dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z;      lum(c) = (0.2126f*c.x + 0.7152f*c.y) + 0.0722f*c.z;
 *     sel_max0(v) = v > 0 ? v : 0;   sel_min80(v) = v < 80 ? v : 80   (a NaN gives 0 and 80: these are not fmaxf / fminf);
 *     pt_expf: the one of pt_detmath.h.
 *   Inert pixels.  p is inert when hit[p].prim < 0 or one of the three colour words of color[p] is not finite (exponent-bit test).  An inert
 *     pixel's record is (color[p].xyz, 0) after every stage, it is written to out (and make_color'd) as it is, and it never counts as a tap.
 *     stats->filtered counts the non-inert pixels of the set.
 *   A tap q counts for p when q lies inside p's rectangle; q's 8x8 block belongs to the call's block set (owned by the rank, and named by
 *     the mask if there is one); q is not inert; hit[q].mesh == hit[p].mesh; dot3(ng_p, ng_q) >= normal_cos; and
 *     fabsf(dot3(ng_p, position[q].xyz - position[p].xyz)) <= plane_eps * hit[p].t.  p itself always counts.
 *   Stage 0, prepare.  v_in = sel_max0(variance[p]).  When variance == NULL, or length != NULL && length[p] < (float)min_length, the
 *     variance is estimated spatially instead and a non-inert p is counted in stats->spatial: over the 7x7 window at spacing 1, row-major (dy
 *     outer, dx inner), over the taps that count, n += 1, s1 += lum(c_q), s2 += lum(c_q) * lum(c_q); then m = s1 / n and
 *     v_in = sel_max0(s2 / n - m * m).  The record is (c_p.xyz, v_in).
 *   Stage i = 0 .. iterations-1, one a-trous pass, step = 2^i, reading the previous stage's records (r, v):
 *     1. g = G / K: G the sum of (k3[j] * k3[i]) * v_q over the 3x3 window at spacing 1, k3 = {0.25f, 0.5f, 0.25f}, row-major, over the taps
 *        that count; K the same sum of k3[j] * k3[i]; each product k3[j] * k3[i] is formed first.
 *     2. den = sigma_lum * sqrtf(g) + 1e-6f;  l_p = lum(r_p).
 *     3. For the 25 taps q = p + step * (dx, dy), dy = -2..2 outer, dx = -2..2 inner, kern = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f}: a
 *        tap that does not count contributes nothing; otherwise e = sel_min80(fabsf(l_p - lum(r_q)) / den);
 *        w = pt_expf(-e) * (kern[dy+2] * kern[dx+2]);  S += r_q * w per component;  V += (w * w) * v_q;  W += w.
 *     4. The new record is (S / W, V / (W * W)).
 *   Output.  out[p] = the last stage's record (filtered rgb, filtered variance); frame_rgba8[p] = make_color(out[p].xyz).  Which of out /
 *     scratch holds which intermediate stage is the implementation's business.
 * variance is the caller's estimate of the variance of lum(color[p]).  The recipe of examples/svgf_loop.py: a second pt_temporal_accumulate
 * over a moments plane (lum, lum * lum, 0, 1) with the same motion, hit and position planes gives reprojected moments (m1, m2), and
 * variance = max(0, m2 - m1 * m1); length is that call's length_out, so that pixels disoccluded fewer than min_length frames ago, whose
 * moments say nothing yet, take the spatial estimate.
 * Overlap: out, scratch and frame_rgba8 may overlap no other plane; the read-only planes may alias one another.
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet; a required
 * plane NULL (color, hit, position, out; scratch when iterations >= 1); a plane that fails the pointer checks; a forbidden overlap;
 * flags != 0; a parameter out of its range or not finite.
 * Ordering and state, as pt_temporal_accumulate: the call first waits for the frames in flight and completes queued queries, runs on
 * pt_stream(ctx) under the STREAM CONTRACT and is complete when it returns.  It reads and writes no context state except through the
 * pointers the caller passed: the frame buffers, the accumulation, the adaptive state, the schedule trial and pt_stats are as they were.
 * stats: pixels processed; non-inert pixels among them; those that took the spatial estimate; device time of all stages (hipEvents; the
 * mask compaction included when there is a mask).
 * Not part of this interface: an asynchronous variant, a pt_multi_* wrapper, albedo demodulation, neighbourhood clamping of the history,
 * motion of moving geometry, any change to pt_denoise. */
enum pt_filter_flags { PT_FILTER_RESERVED = 0 };   /* no flag defined yet: flags must be 0 */
typedef struct pt_filter_desc {
    const float* color;      /* w*h x 4  colour to filter (temporal's history_out / copy_out); .w is ignored */
    const void*  hit;        /* w*h x pt_hit, this frame (pt_render_gbuffer) */
    const float* position;   /* w*h x 4, this frame */
    const float* variance;   /* w*h f32 or NULL: the caller's estimate of the variance of the luminance of color[p] */
    const float* length;     /* w*h f32 or NULL: temporal's length_out */
    float* out;              /* w*h x 4: (filtered rgb, filtered variance) */
    float* scratch;          /* w*h x 4, required when iterations >= 1 (ping-pong), else may be NULL */
    uint32_t* frame_rgba8;   /* w*h or NULL: make_color(out.rgb) */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    int32_t  iterations;     /* 0..6; pass i uses tap spacing 2^i; 0 = the prepared record only */
    float    sigma_lum;      /* finite, > 0 */
    float    normal_cos;     /* [-1,1] */
    float    plane_eps;      /* finite, >= 0 */
    uint32_t min_length;     /* 0..65535: where length[p] < min_length the variance is estimated spatially */
    uint32_t flags;          /* 0 */
} pt_filter_desc;
typedef struct pt_filter_stats { uint64_t pixels, filtered, spatial; double kernel_ms; } pt_filter_stats;
int pt_filter_planes(pt_ctx* ctx, const pt_filter_desc* desc, pt_filter_stats* stats /* may be NULL */);

/* OBJECT MOTION FOR THE REPROJECTION CHAIN (no reference counterpart): the planes that let pt_temporal_accumulate follow geometry that moved
 * between two frames (pt_update_meshes*, pt_transform_meshes).  pt_render_gbuffer's motion plane is camera motion over the current geometry:
 * on a mesh that moved along its normal the temporal pass throws the history away (the plane test fails), on a mesh sliding in its own plane
 * it keeps the history of another surface point.  pt_motion_planes takes this frame's hit plane and the PREVIOUS frame's vertices and says,
 * per pixel, where the surface point under it was: in the previous image (motion), in space (prev_point) and with which normal
 * (prev_surface).  The library keeps no previous-vertex state: the caller snapshots the vertices with pt_copy_vertices_device before the
 * frame's pt_update_meshes* / pt_transform_meshes and ping-pongs the snapshot like prev_hit and prev_position.
 *
 * pt_vertex_count: the context's vertex and triangle totals over all meshes (either pointer may be NULL).  PT_ERR_INVALID for a null ctx.
 * pt_copy_vertices_device: writes the context's current world-space vertices into caller-owned DEVICE memory: all meshes in mesh order,
 * mesh m starting at the sum of num_vertices of the meshes before it, 3 floats per vertex.  bytes must equal vertices * 12.  dev_dst is
 * checked exactly as pt_render_gbuffer checks a plane.  The call first waits for the frames in flight and completes queued queries, copies
 * on pt_stream(ctx) under the STREAM CONTRACT and is complete when it returns.  PT_ERR_INVALID (nothing copied) for a null ctx, wrong
 * bytes, a pointer that fails the checks.
 *
 * pt_motion_planes.  Every plane is caller-owned DEVICE memory of the context's device, frame-sized, indexed Y * width + X, and checked exactly
 * as pt_render_gbuffer checks its planes (known to HIP, device memory of the context's device, 4-byte aligned — no wider alignment is
 * assumed — fitting what is left of its allocation); prev_vertices is checked against vertices * 12 bytes.  prev_cameras and block_mask are
 * HOST memory.
 * Which pixels: exactly those pt_temporal_accumulate would process with the same mask — the rank's owned pixels, view pixels only while views
 * are set, whole blocks of block_mask (NULL: every block).  No other pixel is written in any output.  Zero pixels launch nothing and return
 * PT_OK.  Each pixel works in its own rectangle: its view's (found by the pixel's 8x8 block), or the whole frame without views; (x, y) are
 * its local coordinates there and width, height the rectangle's.
 * Arithmetic per pixel p — float32 throughout, one rounding per operation, no fused multiply-add, in exactly this order, dot3, cross3 and
 * normalize3 as in pt_render_gbuffer's text (cross3(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)); float32 NumPy
 * evaluating this reproduces every output bit for bit.  `triangles` is pt_vertex_count's:
 *   - 0 <= hit[p].prim < triangles.  i_k = idx[3*prim + k], the triangle's global vertex indices (the mesh's own index + the mesh's first
 *     vertex); p_k = prev_vertices[3*i_k ..];  u = hit[p].u, v = hit[p].v (the weights of vertex 1 and vertex 2);
 *         w0 = (1.0f - u) - v;   Q = (p0*w0 + p1*u) + p2*v  per component;   ngp = normalize3(cross3(p1 - p0, p2 - p0))
 *     (a degenerate previous triangle gives NaN words, as computed: the temporal pass's normal test then rejects the tap).
 *     prev_point[p] = (Q, 1.0f);  prev_surface[p] = the eight words of hit[p] with words 5..7 (ng) replaced by ngp;
 *     motion[p] = pt_render_gbuffer's projection block with q = Q - e', the previous camera (e', U', V', W') of the pixel's view, the
 *     pixel's local (x, y) and the rectangle's width, height; when c * det > 0 is false both words are 0x7fc00000.
 *     stats->hits counts these pixels.
 *   - hit[p].prim < 0 (a miss).  prev_point[p] = four zeros;  prev_surface[p] = hit[p];  motion[p] = pt_render_gbuffer's for a miss: q = dir,
 *     with dir rebuilt from the pixel's CURRENT camera by the G-buffer's ray expression — equal to pt_render_gbuffer's motion plane bit for
 *     bit at every miss.
 *   - hit[p].prim >= triangles.  The plane is caller memory and is not trusted: no address is formed from it.  Both motion words are
 *     0x7fc00000, prev_point[p] is four zeros, prev_surface[p] = (hit[p].t, 0, 0, -1, -1, 0, 0, 0), and stats->stale counts the pixel.
 * Feeding the chain.  pt_temporal_accumulate gets hit = prev_surface, position = prev_point, motion = motion; prev_hit and prev_position
 * stay the previous frame's G-buffer planes.  Both sides of every surface test are then in the previous frame's space, and
 * pt_temporal_accumulate itself is unchanged (its plane_eps * hit.t uses this frame's t, which prev_surface keeps).  pt_filter_planes keeps
 * the CURRENT hit and position.  Loop order (examples/moving_geometry_loop.py): snapshot (pt_copy_vertices_device), move the geometry,
 * render, pt_render_gbuffer, pt_motion_planes, pt_temporal_accumulate, pt_filter_planes.  With prev_vertices equal to the current vertices the
 * planes are pt_render_gbuffer's up to the rounding of Q against o + t*dir.
 * Overlap: motion, prev_point and prev_surface may overlap no other plane nor prev_vertices; hit and prev_vertices are only read.
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet; hit or
 * prev_vertices NULL; all three outputs NULL; a plane that fails the pointer checks; a forbidden overlap; motion without prev_cameras;
 * num_prev_cameras different from max(1, view count) when prev_cameras is given; a non-finite previous camera value; flags != 0.
 * Ordering and state, as pt_temporal_accumulate: the call first waits for the frames in flight and completes queued queries, runs on
 * pt_stream(ctx) under the STREAM CONTRACT and is complete when it returns.  It sees the context's current index arrays (topology never
 * changes) and reads no vertex of the context, only prev_vertices.  It reads and writes no context state except through the pointers the
 * caller passed: the frame buffers, the accumulation, the adaptive state, the schedule trial and pt_stats are as they were.
 * stats: pixels processed; hits and stale among them; device time of the pass (hipEvents; the mask compaction included when there is a mask).
 * Not part of this interface: a pt_multi_* wrapper (per-rank calls through pt_multi_ctx work), an asynchronous variant, topology changes
 * (the triangle under a prim index must be the same triangle in both frames), any change to pt_render_gbuffer, pt_temporal_accumulate,
 * pt_filter_planes or pt_denoise. */
int pt_vertex_count(const pt_ctx* ctx, uint32_t* vertices /* may be NULL */, uint32_t* triangles /* may be NULL */);
int pt_copy_vertices_device(pt_ctx* ctx, float* dev_dst, size_t bytes);
enum pt_motion_flags { PT_MOTION_RESERVED = 0 };   /* no flag defined yet: flags must be 0 */
typedef struct pt_motion_desc {
    const void*  hit;            /* w*h x pt_hit, this frame (pt_render_gbuffer); required */
    const float* prev_vertices;  /* vertices x 3 f32, pt_copy_vertices_device's layout, of the previous frame; required */
    float* motion;               /* w*h x 2  or NULL */
    float* prev_point;           /* w*h x 4  or NULL: where the pixel's surface point was, (x, y, z, 1) */
    void*  prev_surface;         /* w*h x pt_hit or NULL: hit[p] with ng replaced by the previous normal */
    const float*   prev_cameras; /* HOST, n x 12 (eye,U,V,W); required iff motion != NULL */
    uint32_t       num_prev_cameras; /* 1 without views, else the view count */
    const uint8_t* block_mask;   /* HOST, as pt_render_gbuffer, or NULL */
    uint32_t flags;              /* 0 */
} pt_motion_desc;
typedef struct pt_motion_stats { uint64_t pixels, hits, stale; double kernel_ms; } pt_motion_stats;
int pt_motion_planes(pt_ctx* ctx, const pt_motion_desc* desc, pt_motion_stats* stats /* may be NULL */);

/* THE SVGF TEMPORAL STAGE IN ONE PASS (no reference counterpart): what examples/svgf_loop.py assembles from three pt_temporal_accumulate
 * calls and element-wise kernels — this frame's colour, the colour history, the luminance moments, the variance — as one kernel with one
 * gather of the taps, plus the two things pt_temporal_accumulate and pt_filter_planes leave out: the colour is DEMODULATED by the first-hit
 * albedo before it is accumulated (so pt_filter_planes works on irradiance-like values and keeps texture detail; pt_modulate_planes
 * multiplies the albedo back in behind the filter), and the reprojected history can be CLAMPED to the neighbourhood of this frame's colour
 * (so a history that passes the geometry tests but is stale — a moved shadow, a changed probe — does not ghost for max_history frames).
 *
 * pt_temporal_moments.  The call is stateless: every plane is caller-owned DEVICE memory of the context's device, frame-sized, indexed
 * Y * width + X, and checked exactly as pt_render_gbuffer checks its planes (known to HIP, device memory of the context's device, 4-byte
 * aligned — no wider alignment is assumed — fitting what is left of its allocation).  A pointer obtained from pt_device_buffer is accepted
 * like any other (PT_BUF_ACCUM as color, PT_BUF_ALBEDO as albedo).
 * Which pixels: exactly those pt_render_gbuffer would write with the same mask — the rank's owned pixels, view pixels only while views are
 * set, whole blocks of block_mask (HOST memory, NULL: every block).  No other pixel is written in any output.  Zero pixels launch nothing
 * and return PT_OK.
 * Each pixel works inside its own rectangle (x0, y0, wr, hr): its view (found by the pixel's 8x8 block), or the whole frame without views;
 * (x, y) are its local coordinates there.  Arithmetic per pixel p — float32 throughout, one rounding per operation, no fused multiply-add,
 * in exactly this order; float32 NumPy evaluating this reproduces every output bit for bit (a NaN is a NaN: its sign and payload are not
 * specified), with dot3, lum and sel_max0 as pt_temporal_accumulate and pt_filter_planes define them:
 *   0. The demodulated colour d(q) of a frame pixel q, per component k of x, y, z: den(q).k = 1.0f when albedo == NULL; otherwise, with
 *      a = albedo[q].k, den(q).k = a > albedo_min ? a : 1.0f (a NaN gives 1, a miss's zero gives 1);
 *      d(q).k = (color[q].k * color_scale) / den(q).k — the multiplication first, then the division.
 *   1. d_p = d(p); l = lum(d_p); m = (l, l * l).
 *   2-4. pt_temporal_accumulate's steps 2, 3 and 4 verbatim (tap order (0,0), (1,0), (0,1), (1,1), sums of the shape ((. + .) + .) + .),
 *      with two additions: a tap also needs both words of moments_in[q] finite (exponent-bit test), and Msum is formed like Hsum from
 *      w_ij * moments_in[q] per component.  valid is defined as there.
 *   5. Valid: H = Hsum / Wsum; M = Msum / Wsum; n = fminf(nprev, (float)(max_history - 1)); a = 1.0f / (n + 1.0f).
 *   5b. Only with PT_TMOM_CLAMP and only for a valid pixel.  Over the 3x3 window at spacing 1 around p, row-major (dy outer, dx inner), a
 *      window pixel q counts when q lies inside p's rectangle, q's 8x8 block belongs to the call's block set (pt_filter_planes's rule: owned
 *      by the rank, and named by the mask if there is one) and the three words of d(q) are finite (exponent-bit test; p itself is a window
 *      pixel like the others).  Per counting q: cnt += 1; s1.k += d(q).k; s2.k += d(q).k * d(q).k.  With cnt >= 1:
 *      mu = s1 / cnt; sd = sqrtf(sel_max0(s2 / cnt - mu * mu)); lo = mu - clamp_k * sd; hi = mu + clamp_k * sd (the product first); per
 *      channel H.k = H.k < lo.k ? lo.k : (H.k > hi.k ? hi.k : H.k).  stats->clamped counts the valid pixels for which one of the six
 *      comparisons H.k < lo.k, H.k > hi.k was true.  The moments are not clamped.
 *   5c. Valid: out = H + (d_p - H) * a; mo = M + (m - M) * a; len = n + 1.  Otherwise out = d_p; mo = m; len = 1.
 *   6. history_out[p] = (out, 1.0f); moments_out[p] = mo; length_out[p] = len; variance_out[p] = sel_max0(mo.y - mo.x * mo.x);
 *      stats->reprojected counts the valid pixels.
 * Clear.  With PT_TMOM_CLEAR_COLOR the four words of color[p] are 0 on return for every pixel of the set.  No read of the call observes the
 * clear (the window reads neighbours' colours: the clear is a second launch behind the kernel on the same stream).
 * Overlap: the four outputs and color may overlap no other plane; the read-only planes may alias one another (prev_hit == hit, say).
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet; a required
 * plane NULL (all but albedo, variance_out and block_mask); a plane that fails the pointer checks; a forbidden overlap; unknown flag bits;
 * a parameter out of its range or not finite — albedo_min negative or not finite; clamp_k negative or not finite when PT_TMOM_CLAMP is set
 * (without the flag clamp_k is not read).
 * Ordering and state, as pt_temporal_accumulate: the call first waits for the frames in flight and completes queued queries, runs on
 * pt_stream(ctx) under the STREAM CONTRACT and is complete when it returns; the previous planes must be complete before the call.  It reads
 * and writes no context state except through the pointers the caller passed: the frame buffers, the accumulation, the adaptive state, the
 * schedule trial and pt_stats are as they were.  The per-frame colour recipe of pt_temporal_accumulate (PT_BUF_ACCUM, color_scale = k + 1,
 * the clear flag) holds word for word.  The chain (examples/svgf_albedo_loop.py): pt_render_gbuffer, render, pt_temporal_moments,
 * pt_filter_planes on history_out with variance_out and length_out, pt_modulate_planes.
 * stats: pixels processed; valid pixels among them; clamped pixels among those; device time of the pass and of the clear (hipEvents; the
 * mask compaction included when there is a mask).
 * Not part of this interface: an asynchronous variant, a pt_multi_* wrapper, clamping of the moments.
 *
 * pt_modulate_planes, the end of the chain: r.k = color[p].k * den(p).k with den exactly as step 0 above; out[p] = (r, color[p].w);
 * frame_rgba8[p] = make_color(r).  At least one of out and frame_rgba8 is required.  The pass is pixel-local, so out may be exactly the
 * address of color (in place); every other overlap of an output with a plane is refused.  Planes, pointer checks, pixel set, ordering and
 * state are pt_temporal_moments's.  Refused with PT_ERR_INVALID (nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet;
 * color NULL; both outputs NULL; a plane that fails the pointer checks; a forbidden overlap; flags != 0; albedo_min negative or not finite.
 * stats: pixels processed; device time of the pass (the mask compaction included when there is a mask). */
enum pt_tmom_flags { PT_TMOM_CLEAR_COLOR = 1, PT_TMOM_CLAMP = 2 };
typedef struct pt_tmom_desc {
    float* color;               /* w*h x 4  this frame's colour; zeroed afterwards with PT_TMOM_CLEAR_COLOR */
    const float* albedo;        /* w*h x 4 or NULL (e.g. pt_device_buffer(PT_BUF_ALBEDO)) */
    const float* motion;        /* w*h x 2  pt_render_gbuffer's (or pt_motion_planes's) motion plane of this frame */
    const void*  hit;           /* w*h x pt_hit, this frame */
    const float* position;      /* w*h x 4, this frame */
    const void*  prev_hit;      /* previous frame's hit plane */
    const float* prev_position;
    const float* history_in;    /* w*h x 4  accumulated demodulated colour after the previous frame */
    const float* moments_in;    /* w*h x 2  accumulated (lum, lum * lum) after the previous frame */
    const float* length_in;     /* w*h      per-pixel history length (whole numbers; 0 = no history) */
    float* history_out;         /* w*h x 4 */
    float* moments_out;         /* w*h x 2 */
    float* length_out;          /* w*h */
    float* variance_out;        /* w*h or NULL */
    const uint8_t* block_mask;  /* HOST, as pt_render_gbuffer, or NULL */
    float color_scale;          /* finite, > 0 */
    float albedo_min;           /* finite, >= 0 */
    float normal_cos;           /* [-1,1] */
    float plane_eps;            /* finite, >= 0 */
    float min_weight;           /* [0,1] */
    float clamp_k;              /* finite, >= 0; read only with PT_TMOM_CLAMP */
    uint32_t max_history;       /* 1..65535 */
    uint32_t flags;             /* pt_tmom_flags */
} pt_tmom_desc;
typedef struct pt_tmom_stats { uint64_t pixels, reprojected, clamped; double kernel_ms; } pt_tmom_stats;
int pt_temporal_moments(pt_ctx* ctx, const pt_tmom_desc* desc, pt_tmom_stats* stats /* may be NULL */);
typedef struct pt_modulate_desc {
    const float* color;         /* w*h x 4  demodulated colour (pt_filter_planes's out); required */
    const float* albedo;        /* w*h x 4 or NULL */
    float* out;                 /* w*h x 4 or NULL; may be exactly color */
    uint32_t* frame_rgba8;      /* w*h or NULL: make_color(r) */
    const uint8_t* block_mask;  /* HOST, as pt_render_gbuffer, or NULL */
    float albedo_min;           /* finite, >= 0 */
    uint32_t flags;             /* 0 */
} pt_modulate_desc;
typedef struct pt_modulate_stats { uint64_t pixels; double kernel_ms; } pt_modulate_stats;
int pt_modulate_planes(pt_ctx* ctx, const pt_modulate_desc* desc, pt_modulate_stats* stats /* may be NULL */);

/* ADAPTIVE SAMPLING INSIDE THE REPROJECTION CHAIN (no reference counterpart): pt_sample_plan decides, BEFORE a frame is rendered, which 8x8
 * blocks need new samples — where the history was lost, where it is short, where the accumulated estimate is still noisy —, and
 * pt_temporal_carry is the temporal stage of the blocks that were not rendered: it carries their history, moments and length along the
 * motion plane unchanged, so that the ping-pong of history_out / moments_out / length_out stays whole.  The rule is pt_render_adaptive's
 * stopping rule per pixel, driven by the reprojected luminance moments of pt_temporal_moments and the history length in place of a per-context
 * moments buffer and the subframe count; it works for a camera and for geometry that move every frame.  Neither call reads a colour plane.
 *
 * Both calls are stateless: every plane is caller-owned DEVICE memory of the context's device, frame-sized, indexed Y * width + X, and
 * checked exactly as pt_render_gbuffer checks its planes (known to HIP, device memory of the context's device, 4-byte aligned — no wider
 * alignment is assumed — fitting what is left of its allocation).  The eight read-only planes are pt_temporal_moments's: motion, hit,
 * position (this frame's, pt_render_gbuffer / pt_motion_planes), prev_hit, prev_position (the previous frame's), history_in, moments_in,
 * length_in (what the previous frame's pt_temporal_moments and pt_temporal_carry left).  All eight are required.
 * Which pixels ("the set"): exactly those pt_render_gbuffer would write with the same mask — the rank's owned pixels, view pixels only while
 * views are set, whole blocks of block_mask (HOST memory, nbx * nby bytes with nbx = (width + 7) / 8, nby = (height + 7) / 8, block (bx, by)
 * at by * nbx + bx, non-zero = named; NULL: every block).  The call's block set: the blocks that hold at least one pixel of the set.
 * Each pixel works inside its own rectangle (x0, y0, wr, hr): its view (found by the pixel's 8x8 block), or the whole frame without views;
 * (x, y) are its local coordinates there.  Arithmetic — float32 throughout, one rounding per operation, no fused multiply-add, in exactly
 * the order stated; float32 NumPy evaluating this reproduces every output bit for bit (a NaN is a NaN: its sign and payload are not
 * specified), with dot3 and sel_max0 (sel_max0(v) = v > 0 ? v : 0, so a NaN gives 0) as pt_temporal_accumulate and pt_filter_planes define them.
 *
 * Step G, the gather, for a pixel p of the set — pt_temporal_moments's steps 2, 3 and 4, restated in full:
 *   G1. px = (float)x + motion[p].x;  py = (float)y + motion[p].y.  The lookup fails (no tap counts) when
 *       (px >= -1 && px <= wr && py >= -1 && py <= hr) is false (a NaN motion word fails this way).  Otherwise flx = floorf(px),
 *       ix = (int)flx, fx = px - flx, likewise fly, iy, fy; wx0 = 1 - fx, wx1 = fx, wy0 = 1 - fy, wy1 = fy; tap weights w_ij = wx_i * wy_j.
 *   G2. Tap (i, j) is frame pixel q = (x0 + ix + i, y0 + iy + j).  It counts when it lies inside the rectangle, w_ij > 0,
 *       length_in[q] >= 1, the three colour words of history_in[q] and both words of moments_in[q] are finite (exponent-bit test) and the
 *       geometry agrees: with hit[p].prim < 0 (a miss) it needs prev_hit[q].prim < 0; otherwise prev_hit[q].mesh == hit[p].mesh,
 *       dot3(ng_p, ng_q) >= normal_cos and fabsf(dot3(ng_p, prev_position[q].xyz - position[p].xyz)) <= plane_eps * hit[p].t.
 *   G3. Tap order (0,0), (1,0), (0,1), (1,1); a tap that does not count contributes +0.0f.  Wsum = ((w00 + w10) + w01) + w11; Hsum the same
 *       sum of w_ij * history_in[q].xyz per component; Msum the same sum of w_ij * moments_in[q] per component; nprev the minimum of
 *       length_in[q] over the counting taps;  valid = (at least one tap counts) && Wsum >= min_weight.
 *   For a valid pixel H = Hsum / Wsum and M = Msum / Wsum, per component.
 *
 * pt_sample_plan: which blocks to render this frame.  Per pixel p of the set, after step G:
 *   lost(p)  = !valid.
 *   short(p) = valid && nprev < (float)min_length.
 *   noisy(p), for a valid pixel that is not short: var = sel_max0(M.y - M.x * M.x); B = M.x + dark_floor;
 *            rhs = (((threshold * threshold) * nprev) * B) * B; noisy = !(var <= rhs) — a NaN makes it noisy.  (pt_render_adaptive's rule
 *            with the reprojected moments and the history length.)  Otherwise noisy(p) is false.
 * Per block b = (bx, by) of the call's block set: L = the number of its lost pixels, S = the number of its short or noisy pixels (integer
 * counts over the block's pixels of the set);
 *   refresh = refresh_period > 0 && ((uint64)bx + 3 * (uint64)by + frame_index) % refresh_period == 0;
 *   sampled = L >= 1 || S >= min_pixels || refresh;   block_mask_out[by * nbx + bx] = sampled ? 1 : 0.
 * Every other block of the frame gets 0; block_mask_out (HOST memory, nbx * nby bytes, required) is written whole, once, when the call
 * succeeds; it may be the array block_mask points to.  The refresh walks every block through a forced sample once per refresh_period
 * frames when frame_index counts frames (0: never), whatever its statistics say.  A block with a lost pixel is always sampled: that is what
 * lets pt_temporal_carry below never meet a pixel it cannot carry.
 * stats: blocks — blocks of the call's block set; sampled — those with sampled; by_lost — L >= 1; by_need — not by_lost, S >= min_pixels;
 * by_refresh — sampled by the refresh only (sampled = by_lost + by_need + by_refresh); pixels, lost, needy — the set's pixels, the lost
 * ones, the short or noisy ones; kernel_ms — device time of the pass (hipEvents; the upload of the block set and the copy of the answer
 * are outside it).
 * Nothing on the device is written except temporaries of the call, so there are no overlap rules: the planes may alias one another.
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written, block_mask_out untouched): a null ctx, desc or
 * block_mask_out; no pt_resize yet; a plane NULL; a plane that fails the pointer checks; flags != 0; a parameter out of its range or not
 * finite (the ranges stand beside the fields).
 *
 * pt_temporal_carry: the temporal stage for pixels that got no new sample.  Per pixel p of the set, after step G,
 *   valid:      history_out[p] = (H, 1.0f); moments_out[p] = M; length_out[p] = nprev (the length is carried: not incremented, not capped);
 *               variance_out[p] = sel_max0(M.y - M.x * M.x).
 *   not valid:  history_out[p] = three NaN words and 1.0f (pt_filter_planes treats such a pixel as inert and as no tap for its neighbours;
 *               the next frame's gather rejects it); moments_out[p] = (0, 0); length_out[p] = 0; variance_out[p] = 0; stats->lost counts it.
 * No other pixel is written in any output; zero pixels launch nothing and return PT_OK.  GUARANTEE: called with the complement of a plan's
 * block_mask_out (restricted by the plan's block_mask, if it had one), and the same planes and normal_cos / plane_eps / min_weight as that
 * plan, lost is 0 — both calls evaluate the same step G on the same words, and the plan samples every block that holds a lost pixel.
 * Overlap: the four outputs may overlap no other plane; the read-only planes may alias one another (prev_hit == hit, say).
 * stats: pixels processed; carried — the valid ones; lost = pixels - carried; kernel_ms — device time of the pass (hipEvents; the mask
 * compaction included when there is a mask).
 * Refused with PT_ERR_INVALID (nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet; a required plane NULL (all but
 * variance_out and block_mask); a plane that fails the pointer checks; a forbidden overlap; flags != 0; a parameter out of its range.
 *
 * Ordering and state, both calls, as pt_temporal_moments: the call first waits for the frames in flight and completes queued queries, runs
 * on pt_stream(ctx) under the STREAM CONTRACT and is complete when it returns; the planes must be complete before the call.  It reads and
 * writes no context state except through the pointers the caller passed.
 * The loop (examples/adaptive_svgf_loop.py), per frame: pt_render_gbuffer; pt_sample_plan -> mask; pt_render_mask(mask);
 * pt_temporal_moments(mask, color = PT_BUF_ACCUM, color_scale = k + 1, PT_TMOM_CLEAR_COLOR); pt_temporal_carry(the complement of mask);
 * pt_filter_planes on all pixels.  With min_length = 65535 and min_pixels = 1 every block is sampled (a history is shorter than 65535 whenever
 * max_history is) and the loop is the unmasked one, bit for bit.
 * ALBEDO: run this loop with albedo = NULL in pt_temporal_moments and without pt_modulate_planes.  PT_BUF_ALBEDO is written by the render, so
 * in a block that was not rendered it is stale: it holds the first-hit albedo of an older camera, and demodulating or remodulating with it
 * would be wrong.  (pt_surface_planes below derives a pixel-centre albedo plane from the hit plane; with it the loop demodulates:
 * examples/adaptive_svgf_albedo_loop.py.)
 * Not part of this interface: asynchronous variants, pt_multi_* wrappers, masks in device memory, per-block sample counts. */
typedef struct pt_plan_desc {
    const float* motion;        /* w*h x 2  this frame's motion plane */
    const void*  hit;           /* w*h x pt_hit, this frame */
    const float* position;      /* w*h x 4, this frame */
    const void*  prev_hit;      /* previous frame's hit plane */
    const float* prev_position;
    const float* history_in;    /* w*h x 4  accumulated colour after the previous frame */
    const float* moments_in;    /* w*h x 2  accumulated (lum, lum * lum) after the previous frame */
    const float* length_in;     /* w*h      per-pixel history length (whole numbers; 0 = no history) */
    const uint8_t* block_mask;  /* HOST, as pt_render_gbuffer, or NULL */
    uint8_t* block_mask_out;    /* HOST, nbx*nby bytes: 1 = sample the block; required */
    float normal_cos;           /* [-1,1] */
    float plane_eps;            /* finite, >= 0 */
    float min_weight;           /* [0,1] */
    float threshold;            /* finite, >= 0: the relative standard error a pixel is allowed (pt_adaptive_params.threshold) */
    float dark_floor;           /* finite, >= 0 */
    uint32_t min_length;        /* 0..65535: a history shorter than this always asks for samples */
    uint32_t min_pixels;        /* 1..64: short or noisy pixels that make a block sampled */
    uint32_t refresh_period;    /* 0..65535; 0 = no refresh */
    uint32_t frame_index;       /* any value; only the refresh reads it */
    uint32_t flags;             /* 0 */
} pt_plan_desc;
typedef struct pt_plan_stats { uint64_t blocks, sampled, by_lost, by_need, by_refresh, pixels, lost, needy; double kernel_ms; } pt_plan_stats;
int pt_sample_plan(pt_ctx* ctx, const pt_plan_desc* desc, pt_plan_stats* stats /* may be NULL */);
typedef struct pt_carry_desc {
    const float* motion;        /* the eight read-only planes of pt_plan_desc */
    const void*  hit;
    const float* position;
    const void*  prev_hit;
    const float* prev_position;
    const float* history_in;
    const float* moments_in;
    const float* length_in;
    float* history_out;         /* w*h x 4 */
    float* moments_out;         /* w*h x 2 */
    float* length_out;          /* w*h */
    float* variance_out;        /* w*h or NULL */
    const uint8_t* block_mask;  /* HOST, as pt_render_gbuffer, or NULL */
    float normal_cos;           /* [-1,1] */
    float plane_eps;            /* finite, >= 0 */
    float min_weight;           /* [0,1] */
    uint32_t flags;             /* 0 */
} pt_carry_desc;
typedef struct pt_carry_stats { uint64_t pixels, carried, lost; double kernel_ms; } pt_carry_stats;
int pt_temporal_carry(pt_ctx* ctx, const pt_carry_desc* desc, pt_carry_stats* stats /* may be NULL */);

/* PIXEL-CENTRE ALBEDO FROM THE HIT PLANE (no reference counterpart): the albedo and the texcoord of the surface point under the centre of
 * every pixel, computed from pt_render_gbuffer's hit plane alone.  PT_BUF_ALBEDO is written by the render — at a jittered sample, and only
 * where the render went — so in a block that pt_sample_plan left out it holds the first-hit albedo of an older camera.  pt_surface_planes
 * gives the plane that pt_temporal_moments and pt_modulate_planes need in such a loop: every pixel of the call, this frame's camera, no
 * rays, no state.
 *
 * pt_copy_texcoords_device: writes the scene's texcoords per primitive into caller-owned DEVICE memory: triangles x 6 f32 in global
 * primitive order (pt_hit.prim's), uv0.x, uv0.y, uv1.x, uv1.y, uv2.x, uv2.y — the texcoords of the primitive's three vertices as pt_create
 * received them (mesh_desc.texcoord[index[3*prim + k]]; zeros for the vertices of a mesh without texcoords).  bytes must equal
 * triangles * 24 (pt_vertex_count).  In a scene without a textured mesh (no mesh has both a texture id >= 0 and texcoords) the table is
 * zero-filled.  dev_dst is checked exactly as pt_copy_vertices_device checks its destination (4-byte aligned is enough).  The call first
 * waits for the frames in flight and completes queued queries, runs on pt_stream(ctx) under the STREAM CONTRACT and is complete when it
 * returns.  The table depends on the scene only: pt_update_meshes* (refit or rebuild) and pt_transform_meshes leave it valid, so a loop
 * takes it once.  PT_ERR_INVALID (nothing written) for a null ctx, wrong bytes, a pointer that fails the checks.
 *
 * pt_surface_planes.  Every plane is caller-owned DEVICE memory of the context's device, frame-sized, indexed Y * width + X, and checked
 * exactly as pt_render_gbuffer checks its planes (4-byte aligned — no wider alignment is assumed); prim_texcoords is checked against
 * triangles * 24 bytes.  block_mask is HOST memory.
 * Which pixels: exactly those pt_motion_planes would process with the same mask — the rank's owned pixels, view pixels only while views are
 * set, whole blocks of block_mask (NULL: every block).  No other pixel is written in either output.  Zero pixels launch nothing and return
 * PT_OK.  The pass is pixel-local and reads no camera.
 * Arithmetic per pixel p — float32 throughout, one rounding per operation, no fused multiply-add, in exactly this order; float32 NumPy
 * evaluating this reproduces every output bit for bit.  `triangles` is pt_vertex_count's; only the first four words of hit[p] are read:
 *   - hit[p].prim < 0 (a miss).  albedo[p] = (0, 0, 0, 1) — what the frame's resolve leaves in PT_BUF_ALBEDO for a primary miss, and what
 *     pt_temporal_moments' denominator turns into 1;  texcoord[p] = (0, 0).
 *   - hit[p].prim >= triangles.  The plane is caller memory and is not trusted: no address is formed from it.  The outputs are those of a
 *     miss, and stats->stale counts the pixel.
 *   - 0 <= hit[p].prim < triangles (stats->hits counts these).  mesh = the context's own mesh of primitive prim (hit[p].mesh is not read).
 *       albedo[p] = (material[mesh].color, 1.0f);  texcoord[p] = (0, 0)
 *     unless the mesh is textured (diffuse_texture_id = tid >= 0 AND texcoords, as the shade kernel decides it).  Then, with
 *     u = hit[p].u, v = hit[p].v (the weights of vertex 1 and vertex 2) and c = prim_texcoords[6*prim ..]:
 *         w0 = (1.0f - u) - v
 *         s  = ((w0 * c[0]) + (u * c[2])) + (v * c[4])
 *         t  = ((w0 * c[1]) + (u * c[3])) + (v * c[5])
 *         albedo[p] = (tex2D(texture[tid], s, t).xyz, 1.0f);  texcoord[p] = (s, t)
 *     and stats->textured counts the pixel.  This is the shade kernel's expression with the hit record's own barycentrics.
 *   - tex2D(texture of W x H RGBA8 texels, s, t): wrap addressing, bilinear, 8 fractional bits, normalised bytes:
 *         x  = (s - floorf(s)) * (float)W;             y  = (t - floorf(t)) * (float)H
 *         xB = x - 0.5f;                               yB = y - 0.5f
 *         fi = floorf(xB);                             fj = floorf(yB)
 *         alpha = floorf(((xB - fi) * 256.0f) + 0.5f) * (1.0f / 256.0f)
 *         beta  = floorf(((yB - fj) * 256.0f) + 0.5f) * (1.0f / 256.0f)
 *         i0 = (int)fi mod W;  i1 = ((int)fi + 1) mod W;  j0 = (int)fj mod H;  j1 = ((int)fj + 1) mod H     (mod: the result in [0, W) / [0, H))
 *         T(i, j)[k] = (float)(byte k of texel (i, j)) / 255.0f          (byte 0 = red = the lowest byte of the 32-bit texel; row 0 first)
 *         out[k] = (((((1.0f - alpha) * (1.0f - beta)) * T(i0, j0)[k]) + ((alpha * (1.0f - beta)) * T(i1, j0)[k]))
 *                   + (((1.0f - alpha) * beta) * T(i0, j1)[k])) + ((alpha * beta) * T(i1, j1)[k])
 *     — pt_eval_table(which = 7) evaluates the same function for texture 0.
 *   - Non-finite u or v in a caller's record (or texcoords that make s or t non-finite) fault nothing: the texel indices are clamped into
 *     the image before any texel is read.  On a textured mesh texcoord[p] then holds s and t as computed (NaN or infinite) and
 *     albedo[p].xyz are NaN (payload unspecified), albedo[p].w is 1.0f; on an untextured mesh u and v are not read at all.
 * Overlap: albedo and texcoord may overlap no other plane nor prim_texcoords; hit and prim_texcoords are only read.
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet;
 * flags != 0; both outputs NULL; a plane that fails the pointer checks; a forbidden overlap; prim_texcoords NULL when the scene has a
 * textured mesh.  On a scene without one prim_texcoords is ignored (NULL or not).
 * Ordering and state, as pt_motion_planes: the call first waits for the frames in flight and completes queued queries, runs on
 * pt_stream(ctx) under the STREAM CONTRACT and is complete when it returns.  It reads the context's materials, textures and
 * primitive-to-mesh table (none of which pt_update_meshes* changes) and writes no context state: the frame buffers, the accumulation, the
 * adaptive state, the schedule trial and pt_stats are as they were.
 * The loop (examples/adaptive_svgf_albedo_loop.py), per frame: pt_render_gbuffer; pt_surface_planes on all pixels; pt_sample_plan -> mask;
 * pt_render_mask(mask); pt_temporal_moments(mask, albedo = the surface albedo); pt_temporal_carry(the complement of mask) — the history is
 * demodulated already and is carried unchanged; pt_filter_planes; pt_modulate_planes(albedo = the surface albedo).
 * Against PT_BUF_ALBEDO: that buffer averages the albedo at the JITTERED first hits of the frame's samples, this plane is the albedo at
 * the pixel's centre; they agree bit for bit wherever every sample of the pixel meets one untextured mesh.
 * stats: pixels processed; hits, stale and textured among them; device time of the pass (hipEvents; the mask compaction included when
 * there is a mask).
 * Not part of this interface: emission, roughness or normal planes, an asynchronous variant, a pt_multi_* wrapper (per-rank calls through
 * pt_multi_ctx work), any change to pt_render_gbuffer or pt_temporal_moments.  texture LOD (mip-mapping) is a pass of its own:
 * pt_surface_lod_planes below; this one stays the point lookup at full resolution. */
int pt_copy_texcoords_device(pt_ctx* ctx, float* dev_dst, size_t bytes);
enum pt_surface_flags { PT_SURFACE_RESERVED = 0 };  /* no flag defined yet: flags must be 0 */
typedef struct pt_surface_desc {
    const void*  hit;             /* w*h x pt_hit, this frame (pt_render_gbuffer); required */
    const float* prim_texcoords;  /* triangles x 6 f32 (pt_copy_texcoords_device); required iff the scene has a textured mesh */
    float* albedo;                /* w*h x 4  or NULL */
    float* texcoord;              /* w*h x 2  or NULL */
    const uint8_t* block_mask;    /* HOST, as pt_render_gbuffer, or NULL */
    uint32_t flags;               /* 0 */
} pt_surface_desc;
typedef struct pt_surface_stats { uint64_t pixels, hits, stale, textured; double kernel_ms; } pt_surface_stats;
int pt_surface_planes(pt_ctx* ctx, const pt_surface_desc* desc, pt_surface_stats* stats /* may be NULL */);

/* FOOTPRINT-FILTERED ALBEDO (no reference counterpart): pt_surface_planes with a level of detail.  Where a texture is minified — a pixel
 * covers many texels — the point lookup of pt_surface_planes shows one of them, and the plane aliases under every camera move.
 * pt_surface_lod_planes derives the pixel's footprint in texture space from the hit plane, the context's CURRENT vertices and the pixel's
 * camera, and looks the albedo up trilinearly in a box-filtered mip pyramid that the caller keeps.
 *
 * pt_texture_mips_layout: the pyramid's shape.  *textures = the number of textures of the scene; dims (HOST, textures x 4 uint32, may be
 * NULL) receives per texture w, h, levels and the index of the first 16-byte texel of its level 1 in the pyramid;
 * levels = 1 + floor(log2(max(w, h))); level k has w_k = max(1, w >> k) by h_k = max(1, h >> k) texels.  The pyramid holds, for textures
 * in order, levels 1 .. levels-1, each row-major (row 0 first), 4 f32 per texel, contiguous; level 0 stays the context's RGBA8 texels.
 * *bytes = 16 * the texels of all those levels: 0 for a scene without textures or with only 1 x 1 textures.  Any of the three outputs may
 * be NULL.  The context keeps its textures' sizes in DEVICE memory only, so every call selects the context's device and reads those few
 * bytes back with one blocking copy (tens of microseconds; the const in the signature says that no state of the renderer changes, not
 * that the call is free).  The copy uses no stream of the context and waits for none: the sizes never change after pt_create, so the
 * call may be made while frames are in flight and orders nothing.  A caller takes the layout once per scene.  PT_ERR_INVALID for a null ctx.
 *
 * pt_copy_texture_mips_device: builds the pyramid on the GPU into caller-owned DEVICE memory, one kernel launch per level on pt_stream(ctx).
 * Texel (i, j) of level k+1, per channel, float32, one rounding per operation:
 *         ((S(2i, 2j) + S(i1, 2j)) + (S(2i, j1) + S(i1, j1))) * 0.25f        i1 = min(2i + 1, w_k - 1);  j1 = min(2j + 1, h_k - 1)
 * where S is level k, and at level 0 S = (float)byte / 255.0f.  An odd dimension drops its last row or column: w_k = 5 gives w_k+1 = 2 and
 * column 4 of level k is in no texel of level k+1 (a 1-wide or 1-high level repeats its only column or row instead).  bytes must equal the
 * layout's; dev_dst is checked exactly as pt_copy_texcoords_device checks its destination and must in addition be 16-byte aligned.
 * bytes == 0 is a no-op that returns PT_OK (dev_dst is not looked at).  The call first waits for the frames in flight and completes queued
 * queries, and is complete when it returns.  The pyramid depends on the scene only (no update of the geometry touches a texture), so a
 * loop takes it once.  PT_ERR_INVALID (nothing written) for a null ctx, wrong bytes, a pointer that fails the checks.
 *
 * pt_surface_lod_planes.  Pixel set, rectangles, views, partitions and pointer checks are exactly pt_motion_planes's; every plane is
 * caller-owned DEVICE memory of the context's device (4-byte aligned, frame-sized, indexed Y * width + X), prim_texcoords is checked
 * against triangles * 24 bytes, mips against mips_bytes, which must equal the layout's, and mips must be 16-byte aligned; block_mask is
 * HOST memory.  No other pixel is written in any output.  Zero pixels launch nothing and return PT_OK.
 * The pass reads from the context its current vertices and indices (so it follows pt_update_meshes* and pt_transform_meshes), the
 * materials, the primitive-to-mesh table, the textures, and the cameras: the frame's, or with views the camera and rectangle of the
 * pixel's view (x, y below are then relative to the view's rectangle and wr, hr are its width and height; otherwise the frame's).  Every
 * level address comes from the context's own texture sizes, never from caller memory, and hit[p].prim is compared with the triangle count
 * before any address is formed from it.
 * Arithmetic per pixel p — float32 throughout, one rounding per operation, no fused multiply-add, in exactly this order; float32 NumPy
 * evaluating this reproduces every output bit for bit (tests/surface_lod_ref.py).  dot3(a, b) = ((a.x * b.x) + (a.y * b.y)) + (a.z * b.z);
 * cross3(a, b) = ((a.y * b.z) - (a.z * b.y), (a.z * b.x) - (a.x * b.z), (a.x * b.y) - (a.y * b.x)); w0, s, t and tex2D as for pt_surface_planes.
 *   - A miss, a stale record (prim >= triangles; stats->stale) and a hit on an untextured mesh: albedo[p] and texcoord[p] are
 *     pt_surface_planes's, footprint[p] = (0, 0, 0, 0), lod[p] = 0.
 *   - A hit on a textured mesh (stats->textured), with c = prim_texcoords[6*prim ..], p0, p1, p2 the primitive's current vertices, eye, U,
 *     V, W the pixel's camera, W_t x H_t the texture's size and `levels` its level count:
 *         texcoord[p] = (s, t)
 *         d(a, b) = ((U * ((2.0f * (a / (float)wr)) - 1.0f)) + (V * ((2.0f * (b / (float)hr)) - 1.0f))) + W           (per component)
 *         d_c = d((float)x + 0.5f, (float)y + 0.5f);  d_x = d((float)x + 1.5f, (float)y + 0.5f);  d_y = d((float)x + 0.5f, (float)y + 1.5f)
 *         e1 = p1 - p0;  e2 = p2 - p0;  n = cross3(e1, e2);  nn = dot3(n, n);  hgt = dot3(n, p0 - eye)
 *         t_r = hgt / dot3(n, d_r);  P_r = (d_r * t_r) + eye                                                           (r = c, x, y)
 *         ok = t_c > 0 && t_x > 0 && t_y > 0
 *         g = P_r - P_c;  du = dot3(cross3(g, e2), n) / nn;  dv = dot3(cross3(e1, g), n) / nn                          (r = x, y)
 *         ds_r = (du * (c[2] - c[0])) + (dv * (c[4] - c[0]));  dt_r = (du * (c[3] - c[1])) + (dv * (c[5] - c[1]))
 *         footprint[p] = (ds_x, dt_x, ds_y, dt_y)                  (as computed, whatever ok is: the texcoord step per pixel step in x and y)
 *         rx = ((ds_x * (float)W_t) * (ds_x * (float)W_t)) + ((dt_x * (float)H_t) * (dt_x * (float)H_t));  ry likewise from ds_y, dt_y
 *         rho2 = ok ? (rx > ry ? rx : ry) : +infinity
 *         rho = sqrtf(rho2) * footprint_scale                      (sqrtf correctly rounded; +infinity * 0 is NaN)
 *       Level 0:   if !(rho > 1.0f): albedo[p] = (tex2D(texture[tid], s, t).xyz, 1.0f), lod[p] = 0 — pt_surface_planes's value; a NaN
 *                  lands here, and so does every pixel at footprint_scale = 0.
 *       Coarsest:  else (stats->minified counts the pixel), with Lm = levels - 1, if !(rho < (float)(1 << Lm)): the coarsest level alone,
 *                  albedo[p] = (tex2D_Lm(s, t).xyz, 1.0f), lod[p] = (float)Lm.
 *       Trilinear: otherwise k = the unbiased exponent field of rho (bits 23..30 minus 127, so 2^k <= rho < 2^(k+1) and 0 <= k < Lm),
 *                  m = rho with its exponent field set to 127 (in [1, 2)), frac = m - 1.0f,
 *                  out = c_k + ((c_k+1 - c_k) * frac) per channel with c_j = tex2D_j(s, t), albedo[p] = (out.xyz, 1.0f),
 *                  lod[p] = (float)k + frac.
 *       tex2D_0 is tex2D of the RGBA8 texels.  tex2D_j for j >= 1 is the tex2D text with W, H replaced by w_j, h_j and T(i, j)[k] the
 *       pyramid's float k of texel (i, j) of level j.
 *     A zero-area primitive has n = 0, so t_r is NaN, ok is false and the coarsest level is taken (level 0 at footprint_scale = 0); the
 *     footprint is NaN.  A ray parallel to the primitive's plane or meeting it behind the eye (a horizon pixel) makes ok false likewise.
 *     Non-finite u or v fault nothing, as in pt_surface_planes.
 * Overlap: the four outputs may overlap nothing; hit, prim_texcoords and mips are only read.
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet;
 * flags != 0; all four outputs NULL; footprint_scale negative or not finite; mips_bytes different from the layout's; a plane that fails
 * the pointer checks; a forbidden overlap; prim_texcoords NULL when the scene has a textured mesh; mips NULL or not 16-byte aligned when
 * the scene has a textured mesh and the layout's bytes are > 0.  On a scene without a textured mesh prim_texcoords, mips and mips_bytes
 * are ignored.
 * Ordering and state, as pt_surface_planes: waits for the frames in flight, runs on pt_stream(ctx) under the STREAM CONTRACT, is
 * complete when it returns, and writes no context state.  Host work per call on a textured scene, in front of the timed span (so
 * kernel_ms does not show it): the same readback of the texture sizes as pt_texture_mips_layout, and the upload of 128 bytes per texture
 * (the first texel of every level) into the call's one temporary allocation, next to the counters.
 * footprint_scale: 1 = the pixel's own footprint; 0 = pt_surface_planes's albedo and texcoord bit for bit.
 * stats: pixels processed; hits, stale, textured and minified (rho > 1) among them; device time of the pass.
 * Not part of this interface: anisotropic footprints (the larger axis picks the level; pt_surface_aniso_planes below takes several taps
 * along it), LOD in the frame path (PT_BUF_ALBEDO and the
 * shading stay point lookups), emission, roughness or normal planes, a pt_multi_* wrapper. */
int pt_texture_mips_layout(const pt_ctx* ctx, uint32_t* textures, uint32_t* dims /* HOST, textures x 4, may be NULL */, size_t* bytes);
int pt_copy_texture_mips_device(pt_ctx* ctx, void* dev_dst, size_t bytes);
enum pt_surface_lod_flags { PT_SURFACE_LOD_RESERVED = 0 };  /* no flag defined yet: flags must be 0 */
typedef struct pt_surface_lod_desc {
    const void*  hit;             /* w*h x pt_hit, this frame (pt_render_gbuffer); required */
    const float* prim_texcoords;  /* triangles x 6 f32 (pt_copy_texcoords_device); required iff the scene has a textured mesh */
    const void*  mips;            /* the pyramid (pt_copy_texture_mips_device); required iff textured and the layout's bytes > 0 */
    size_t mips_bytes;            /* pt_texture_mips_layout's bytes */
    float* albedo;                /* w*h x 4  or NULL */
    float* texcoord;              /* w*h x 2  or NULL */
    float* footprint;             /* w*h x 4  or NULL: ds/dx, dt/dx, ds/dy, dt/dy per pixel step */
    float* lod;                   /* w*h x 1  or NULL */
    const uint8_t* block_mask;    /* HOST, as pt_render_gbuffer, or NULL */
    float footprint_scale;        /* finite, >= 0; 1 = the pixel's own footprint */
    uint32_t flags;               /* 0 */
} pt_surface_lod_desc;
typedef struct pt_surface_lod_stats { uint64_t pixels, hits, stale, textured, minified; double kernel_ms; } pt_surface_lod_stats;
int pt_surface_lod_planes(pt_ctx* ctx, const pt_surface_lod_desc* desc, pt_surface_lod_stats* stats /* may be NULL */);

/* ANISOTROPIC FOOTPRINT-FILTERED ALBEDO (no reference counterpart): pt_surface_lod_planes with several taps along the footprint's longer
 * axis.  pt_surface_lod_planes lets the longer of the pixel's two footprint axes pick the level, so a ground seen at a grazing angle is
 * blurred along the shorter axis as well.  pt_surface_aniso_planes takes N <= max_aniso lookups spread along the longer axis, each at the
 * level that a footprint N times shorter picks, and averages them: the filter's extent along the longer axis stays the pixel's, across
 * it the filter narrows by up to max_aniso.
 * It uses the pyramid of pt_texture_mips_layout / pt_copy_texture_mips_device unchanged.  The pixel set, rectangles, views, partitions,
 * pointer checks, what is read from the context, ordering and state are exactly pt_surface_lod_planes's, and so are albedo, texcoord,
 * footprint, lod, block_mask, footprint_scale, mips and mips_bytes; taps is one more frame-sized output of 1 f32 per pixel.  Every tap
 * address comes from the context's own texture sizes, never from caller memory: hit[p].prim is compared with the triangle count before any
 * address is formed from it, and the texel indices are clamped into their level before a texel is read — the tap texcoords are
 * caller-influenced floats and may be anything.
 * Arithmetic per pixel p — float32 throughout, one rounding per operation, no fused multiply-add, in exactly this order; float32 NumPy
 * evaluating this reproduces every output bit for bit (tests/surface_aniso_ref.py):
 *   - A miss, a stale record and a hit on an untextured mesh: albedo, texcoord, footprint and lod hold pt_surface_lod_planes's values and
 *     taps[p] = 0.
 *   - A hit on a textured mesh, with s, t, ds_x, dt_x, ds_y, dt_y, rx, ry, ok, W_t, H_t and Lm = levels - 1 of pt_surface_lod_planes's text:
 *         texcoord[p] = (s, t);  footprint[p] = (ds_x, dt_x, ds_y, dt_y)
 *         xm = rx > ry                                    (pt_surface_lod_planes's own comparison: a tie takes y)
 *         r_maj2 = xm ? rx : ry;  r_min2 = xm ? ry : rx;  (a_s, a_t) = xm ? (ds_x, dt_x) : (ds_y, dt_y)
 *         rho_maj = (ok ? sqrtf(r_maj2) : +infinity) * footprint_scale;  rho_min = sqrtf(r_min2) * footprint_scale
 *         if !(rho_maj > 1.0f) or !ok: N = 1              (level 0 or the coarsest level, exactly as pt_surface_lod_planes)
 *         else q = rho_maj / rho_min;  N = (q <= (float)max_aniso) ? (uint)ceilf(q) : max_aniso        (+infinity and NaN take max_aniso)
 *         rho = rho_maj / (float)N                        (N = 1: rho_maj itself, no division)
 *       The level choice is pt_surface_lod_planes's, taken from this rho: level 0 if !(rho > 1.0f), with lod[p] = 0; else the coarsest
 *       level alone if !(rho < (float)(1 << Lm)), with lod[p] = (float)Lm; otherwise trilinear with k and frac from rho's bits,
 *       c = c_k + ((c_k+1 - c_k) * frac) per channel and lod[p] = (float)k + frac.
 *         tap i = 0 .. N-1:  o_i = (float)(2i + 1 - N) / (float)(2N)         (the numerator a signed integer: one rounding, the division's)
 *                            (s_i, t_i) = (s + ((o_i * footprint_scale) * a_s), t + ((o_i * footprint_scale) * a_t))
 *                            N = 1: the tap is (s, t) itself, with no arithmetic (a non-finite axis does not reach it)
 *         c_i = that level choice evaluated at (s_i, t_i);  acc = c_0;  acc = acc + c_i for i = 1 .. N-1 in order;  out = acc / (float)N
 *                            (N = 1: out = c_0, no division)
 *         albedo[p] = (out.xyz, 1.0f);  taps[p] = (float)N
 *     stats->minified counts rho_maj > 1.0f — the pixels pt_surface_lod_planes counts, whatever max_aniso is; stats->anisotropic counts
 *     N > 1; stats->taps is the sum of N over the textured pixels.
 *     The offsets o_i are symmetric about 0 bit for bit (o_i = -o_(N-1-i); the middle tap of an odd N is 0) and lie inside (-0.5, 0.5):
 *     the taps are the centres of N equal pieces of the longer axis through the pixel's centre.  A primitive whose texcoords are collinear can have rho_min = 0: q is +infinity and N = max_aniso.  ok
 *     false (a horizon pixel, a zero-area primitive) takes the coarsest level with one tap, as pt_surface_lod_planes does.  Non-finite
 *     tap texcoords fault nothing: albedo[p].xyz are then NaN.
 * max_aniso = 1 gives pt_surface_lod_planes's four planes bit for bit; footprint_scale = 0 gives pt_surface_planes's albedo and texcoord
 * bit for bit (rho_maj is 0 or NaN, so N = 1 and level 0).
 * Overlap: the five outputs may overlap nothing; hit, prim_texcoords and mips are only read.
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): everything pt_surface_lod_planes refuses, with
 * this function's name in the text (all FIVE outputs NULL for "no plane asked for"); max_aniso 0 or above 16; a taps plane that fails the
 * pointer checks or overlaps another plane.
 * stats: pixels processed; hits, stale, textured, minified, anisotropic among them; taps as above; device time of the pass.
 * Not part of this interface: an elliptical (EWA) weighting of the taps, anisotropy in the frame path's own lookup, a pt_multi_* wrapper,
 * an asynchronous variant. */
enum pt_surface_aniso_flags { PT_SURFACE_ANISO_RESERVED = 0 };  /* no flag defined yet: flags must be 0 */
typedef struct pt_surface_aniso_desc {   /* pt_surface_lod_desc's fields in its order, then taps, max_aniso, flags */
    const void*  hit;             /* w*h x pt_hit, this frame (pt_render_gbuffer); required */
    const float* prim_texcoords;  /* triangles x 6 f32 (pt_copy_texcoords_device); required iff the scene has a textured mesh */
    const void*  mips;            /* the pyramid (pt_copy_texture_mips_device); required iff textured and the layout's bytes > 0 */
    size_t mips_bytes;            /* pt_texture_mips_layout's bytes */
    float* albedo;                /* w*h x 4  or NULL */
    float* texcoord;              /* w*h x 2  or NULL */
    float* footprint;             /* w*h x 4  or NULL: ds/dx, dt/dx, ds/dy, dt/dy per pixel step */
    float* lod;                   /* w*h x 1  or NULL */
    const uint8_t* block_mask;    /* HOST, as pt_render_gbuffer, or NULL */
    float footprint_scale;        /* finite, >= 0; 1 = the pixel's own footprint */
    float* taps;                  /* w*h x 1  or NULL: the number of taps N taken, as a float; 0 where no texture was read */
    uint32_t max_aniso;           /* 1..16 */
    uint32_t flags;               /* 0 */
} pt_surface_aniso_desc;
typedef struct pt_surface_aniso_stats { uint64_t pixels, hits, stale, textured, minified, anisotropic, taps; double kernel_ms; } pt_surface_aniso_stats;
int pt_surface_aniso_planes(pt_ctx* ctx, const pt_surface_aniso_desc* desc, pt_surface_aniso_stats* stats /* may be NULL */);

/* GUIDED UPSAMPLING (no reference counterpart): a low-resolution colour plane brought to the context's resolution under the guidance of
 * both G-buffers — a joint-bilateral upsample.  The noisy, low-frequency part of the image (the demodulated irradiance) is traced and
 * filtered by a second context of width/scale x height/scale over the same scene; the full-size context only makes a G-buffer and an
 * albedo (pt_render_gbuffer, pt_surface[_lod]_planes), calls this pass, and multiplies the albedo back (pt_modulate_planes).  "Same
 * surface" is the chain's single notion of it: mesh, normal and plane distance, exactly the tests of pt_temporal_accumulate and
 * pt_filter_planes.  The call is made on the FULL-size context and is stateless: every plane is caller-owned DEVICE memory of the
 * context's device, checked exactly as pt_render_gbuffer checks its planes (4-byte aligned, no wider alignment assumed); hit, position,
 * out and weight_out are frame-sized and indexed Y * width + X, the three low-resolution planes hold lo_width * lo_height pixels and are
 * indexed y * lo_width + x.  block_mask is HOST memory.
 * Which pixels: exactly those pt_render_gbuffer would write with the same mask — the rank's owned pixels, view pixels only while views are
 * set, whole blocks of block_mask (NULL: every block).  No other pixel of out or weight_out is written.  Zero pixels launch nothing and
 * return PT_OK.
 * Rectangles.  A pixel p = (X, Y) works inside its rectangle [x0,x1) x [y0,y1): its view (found by the pixel's 8x8 block), or the whole
 * frame without views.  While views are set, every view's x, y, width and height must be multiples of scale.  The low-resolution
 * rectangle is that rectangle divided by scale, [x0/s, x1/s) x [y0/s, y1/s) in a plane lo_width wide — what a low-resolution context holds
 * whose views are the full-size ones divided by scale.  No tap leaves it.
 * Arithmetic per pixel p, with s = scale — integers and float32, one rounding per operation, no fused multiply-add, in exactly this order,
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z as pt_temporal_accumulate and pt_filter_planes define it; float32 NumPy evaluating this
 * reproduces every output bit for bit (tests/upsample_ref.py):
 *   1. Per axis, in integers and one float32 division.  For x: a = X - x0; r = a % s; cx = x0/s + a/s (the low-res pixel that contains p);
 *      t = (float)(2*r + 1 - s) / (float)(2*s).  If t < 0: i = cx - 1, fx = t + 1.0f.  Else i = cx, fx = t.  Likewise for y: cy, j, fy.
 *      (The centre of p lies at (a + 0.5)/s - 0.5 in low-res pixel units; i is its floor, fx its fraction.)
 *   2. A low-res pixel q counts for p when q lies inside the low-resolution rectangle; the three colour words of lo_color[q] are finite
 *      (exponent-bit test); and either both are misses (hit[p].prim < 0 and lo_hit[q].prim < 0) or both are hits (hit[p].prim >= 0 and
 *      lo_hit[q].prim >= 0) with lo_hit[q].mesh == hit[p].mesh, dot3(ng_p, ng_q) >= normal_cos and
 *      fabsf(dot3(ng_p, lo_position[q].xyz - position[p].xyz)) <= plane_eps * hit[p].t — the distance is the full-res pixel's, as in the
 *      filter.  There is no block test on q: the low-res plane is the caller's and is complete, or inert where it is not.
 *   3. Bilinear stage.  The taps are q = (i + dx, j + dy) in the order (0,0), (1,0), (0,1), (1,1); wx = dx ? fx : 1.0f - fx;
 *      wy = dy ? fy : 1.0f - fy; w = wx * wy.  A tap with w == 0 does not count (scale 3, the centre residue).  For a tap that counts,
 *      S += lo_color[q] * w per component (all four words) and W += w; a tap that does not count contributes nothing.
 *      If W > 0: out[p] = S / W per component, weight_out[p] = W.  stats->full counts the pixels whose four taps all counted.
 *   4. Rescue, when W == 0.  The 16 low-res pixels q = (i + dx, j + dy), dy = -1..2 outer, dx = -1..2 inner, go through the test of 2
 *      unweighted: for one that counts S += lo_color[q] per component and N += 1.0f.  If N > 0: out[p] = S / N, weight_out[p] = 0.0f and
 *      the pixel is counted in stats->rescued.
 *   5. Orphan, when the rescue finds none either.  out[p] = lo_color[(cx, cy)], the four words as they are (the low-res pixel that
 *      contains p); weight_out[p] = -1.0f; the pixel is counted in stats->orphans.  A caller can turn weight_out < 0 into a block mask and
 *      path-trace those blocks on the full-size context.
 * What the output means: where weight_out > 0 the pixel holds an interpolation of the low-res pixels of its own surface around it, where
 * it is 0 an average of such pixels from one ring further out, where it is -1 a value of another surface.  A miss is interpolated from
 * misses: the environment is not evaluated per pixel.
 * Overlap: out and weight_out may overlap no other plane; the read-only planes may alias one another.
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet; a required
 * plane NULL (all but weight_out and block_mask); a plane that fails the pointer checks (the low-res planes against lo_width * lo_height
 * pixels); a forbidden overlap; scale outside 2..4; lo_width * scale != width or lo_height * scale != height (the message holds both
 * sizes); a view rectangle that is not a multiple of scale (the message names the view); flags != 0; a parameter out of its range or not
 * finite.
 * Ordering and state, as pt_filter_planes: the call first waits for the frames in flight and completes queued queries, runs on
 * pt_stream(ctx) under the STREAM CONTRACT and is complete when it returns; the low-res planes, made on another context's stream, must be
 * complete before the call.  It reads and writes no context state except through the pointers the caller passed: the frame buffers, the
 * accumulation, the adaptive state, the schedule trial and pt_stats are as they were.
 * stats: pixels processed; hits (hit[p].prim >= 0) among them; full, rescued and orphans as above (pixels - full - rescued - orphans took
 * the bilinear stage with fewer than four taps); device time of the pass (hipEvents; the mask compaction included when there is a mask).
 * Not part of this interface: an asynchronous variant; a pt_multi_* wrapper (per-rank calls work when the rank holds the whole low-res
 * image); per-pixel evaluation of the probe on misses; non-integer scales; a low-res block set; the refill of the orphans. */
enum pt_upsample_flags { PT_UPSAMPLE_RESERVED = 0 };  /* no flag defined yet: flags must be 0 */
typedef struct pt_upsample_desc {
    const float* lo_color;     /* lw*lh x 4: what is upsampled (the low-res chain's pt_filter_planes out); required */
    const void*  lo_hit;       /* lw*lh x pt_hit: the low-res frame's G-buffer; required */
    const float* lo_position;  /* lw*lh x 4; required */
    const void*  hit;          /* w*h x pt_hit: this context's G-buffer of the same frame; required */
    const float* position;     /* w*h x 4; required */
    float*    out;             /* w*h x 4; required, exclusive */
    float*    weight_out;      /* w*h f32 or NULL, exclusive: W of the bilinear stage; 0.0f rescued; -1.0f orphan */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    uint32_t  lo_width, lo_height, scale;   /* scale 2..4; lo_width*scale == width, lo_height*scale == height */
    float     normal_cos;      /* [-1,1] */
    float     plane_eps;       /* finite, >= 0 */
    uint32_t  flags;           /* 0 */
} pt_upsample_desc;
typedef struct pt_upsample_stats { uint64_t pixels, hits, full, rescued, orphans; double kernel_ms; } pt_upsample_stats;
int pt_upsample_planes(pt_ctx* ctx, const pt_upsample_desc* desc, pt_upsample_stats* stats /* may be NULL */);

/* GEOMETRIC EDGE ANTIALIASING (no reference counterpart): the chain's final image with its silhouettes, creases and depth steps smoothed
 * from the hit plane alone.  Every plane of the chain describes the surface under the CENTRE of a pixel, so the final image has one-sample
 * staircases along every edge of the geometry.  Where a pixel and one of its four neighbours show different surfaces, pt_edge_aa_planes
 * intersects the centre ray of the pixel on the far side with the plane of the NEARER surface's triangle: the barycentric that changes
 * sign between the two centres gives the place where the triangle's edge crosses the line between them, and a pixel whose own half of that
 * line is crossed takes the matching share of the neighbour's colour.  No jitter, no history, no second frame: the pass is stateless.
 * The pixel set, rectangles, views, partitions and pointer checks are exactly pt_motion_planes's; every plane is caller-owned DEVICE memory
 * of the context's device (4-byte aligned, frame-sized, indexed Y * width + X); block_mask is HOST memory.  No pixel outside the set is
 * written in any output.  Zero pixels launch nothing and return PT_OK.
 * The pass reads from the context its CURRENT vertices and indices (so it follows pt_update_meshes* and pt_transform_meshes) and the
 * cameras: the frame's, or with views the camera and rectangle of the pixel's view (x, y below are then relative to the view's rectangle
 * and wr, hr are its width and height; otherwise the frame's).  hit[..].prim is compared with the triangle count before any address is
 * formed from it, for the pixel's record and for a neighbour's alike.
 * Arithmetic per pixel p of the set — float32 throughout, one rounding per operation, no fused multiply-add, in exactly this order;
 * float32 NumPy evaluating this reproduces every output bit for bit (tests/edge_aa_ref.py).  dot3, cross3, d(a, b) and, of a primitive
 * with current vertices p0, p1, p2, e1, e2, n, nn, hgt are as in pt_surface_lod_planes's text; sel_max0 is as in pt_filter_planes.  A
 * record is a miss when its prim is negative and a hit otherwise (a stale record, prim >= triangles, is a hit here).
 *   1. c_p = color[p].xyz.  If one of its three words is not finite (exponent-bit test): out[p] = (c_p, 1.0f), edge[p] = (0, 0), done.
 *   2. Directions k = 0..3 with (dx, dy) = (-1, 0), (+1, 0), (0, -1), (0, +1) and q = p + (dx, dy).  Direction k is a candidate when q lies
 *      inside p's rectangle; q's 8x8 block is in the call's block set (the rank's blocks that block_mask names); color[q].xyz is finite;
 *      p and q are not both misses; and p and q are not the same surface.  Same surface: both are hits and either
 *      hit[q].prim == hit[p].prim, or the chain's test holds from p's side: hit[q].mesh == hit[p].mesh and
 *      dot3(ng_p, ng_q) >= normal_cos and fabsf(dot3(ng_p, position[q].xyz - position[p].xyz)) <= plane_eps * hit[p].t.  A NaN in either
 *      comparison makes it false: the surfaces differ and the direction stays a candidate.  stats->boundary counts the pixels with at
 *      least one candidate.
 *   3. For a candidate, the owner o of the edge is the nearer surface: q if p is a miss; p if q is a miss; otherwise p when
 *      hit[p].t <= hit[q].t, else q (a NaN on either side makes the comparison false: q owns).  r is the other pixel of the pair.  A stale
 *      owner record (prim >= triangles) drops the direction.  With the owner's primitive and (x_r, y_r) the local coordinates of r:
 *         d_r = d((float)x_r + 0.5f, (float)y_r + 0.5f)
 *         t_r = hgt / dot3(n, d_r);  the direction is dropped unless t_r > 0                                    (a NaN drops it)
 *         P_r = (d_r * t_r) + eye;  g = P_r - p0
 *         u_r = dot3(cross3(g, e2), n) / nn;  v_r = dot3(cross3(e1, g), n) / nn
 *         b_r = ((1.0f - u_r) - v_r, u_r, v_r)
 *         b_o = (sel_max0((1.0f - u_o) - v_o), sel_max0(u_o), sel_max0(v_o))                                   (u_o, v_o from hit[o])
 *      For i = 0, 1, 2 in order with b_r[i] < 0 (a NaN fails: that i is skipped): s_i = b_o[i] / (b_o[i] - b_r[i]).  s is the first such
 *      s_i, replaced by a later one when s_i < s: the smallest, a strict < keeps the first, a NaN s_i never replaces and a first NaN s_i
 *      is never replaced.  If there is no such i, the direction is dropped.
 *         dist = (o is p) ? s : 1.0f - s
 *      The direction has weight w_k = 0.5f - dist when dist < 0.5f; otherwise it is dropped (a NaN fails the comparison and drops it).
 *      b_o[i] >= 0 > b_r[i], so 0 <= s <= 1 and 0 < w_k <= 0.5.
 *   4. The direction with the largest w_k wins; a strict > keeps the first.  No direction: out[p] = (c_p, 1.0f), edge[p] = (0, 0).
 *      Otherwise, with q the winner's neighbour and w its weight: out[p].xyz = c_p + ((c_q - c_p) * w) per component, out[p].w = 1.0f,
 *      edge[p] = (w, (float)(k + 1)); stats->blended counts these.  In every case, step 1's included, frame_rgba8[p] = make_color(out[p].xyz),
 *      the frame path's own transform (sRGB, 8 bits, alpha 255).
 *   5. stats->hits and stats->stale count p's own record, as the surface passes do (prim in range; prim >= triangles).  A zero-area
 *      owner primitive (nn == 0: t_r is 0 / 0), a ray parallel to the owner's plane or meeting it behind the eye, and non-finite u, v of
 *      either record all end in a dropped direction through the comparisons above, which a NaN fails.  None of them faults.
 * What the output means: dist is the place of the owner's edge on the line from p's centre (0) to q's centre (1).  The edge at dist < 0.5
 * lies in p's own half, and the far side of it, 0.5 - dist of the pixel's width along that line, shows q's surface.  Only the strongest of
 * the four directions is used: summing several overcorrects at corners.
 * Overlap: out, edge and frame_rgba8 may overlap nothing (the kernel gathers neighbours of color, so there is no in-place form); the
 * read-only planes may alias one another.
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet; color,
 * hit, position or out NULL; a plane that fails the pointer checks; a forbidden overlap; flags != 0; normal_cos outside [-1, 1] or NaN;
 * plane_eps negative or not finite.
 * Ordering and state, as pt_motion_planes and pt_surface_lod_planes: waits for the frames in flight, runs on pt_stream(ctx) under the
 * STREAM CONTRACT, is complete when it returns, and writes no context state.
 * stats: pixels processed; hits and stale among them; boundary and blended as above; device time of the pass.
 * Not part of this interface: jittered or temporal antialiasing; edges that are no triangle edge (interpenetrating surfaces, shadow and
 * texture edges); sub-pixel triangles; blending with more than one neighbour; an asynchronous variant; a pt_multi_* wrapper (per-rank calls
 * work, and a neighbour in another rank's block does not count). */
enum pt_edge_aa_flags { PT_EDGE_AA_RESERVED = 0 };  /* no flag defined yet: flags must be 0 */
typedef struct pt_edge_aa_desc {
    const float* color;        /* w*h x 4: the image to antialias (pt_modulate_planes's out); .w is ignored; required */
    const void*  hit;          /* w*h x pt_hit, this frame (pt_render_gbuffer); required */
    const float* position;     /* w*h x 4, this frame; required */
    float*    out;             /* w*h x 4; required, exclusive */
    float*    edge;            /* w*h x 2 or NULL, exclusive: the weight w and the direction code k + 1 (0, 0 where nothing was blended) */
    uint32_t* frame_rgba8;     /* w*h or NULL, exclusive */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    float     normal_cos;      /* [-1,1] */
    float     plane_eps;       /* finite, >= 0 */
    uint32_t  flags;           /* 0 */
} pt_edge_aa_desc;
typedef struct pt_edge_aa_stats { uint64_t pixels, hits, stale, boundary, blended; double kernel_ms; } pt_edge_aa_stats;
int pt_edge_aa_planes(pt_ctx* ctx, const pt_edge_aa_desc* desc, pt_edge_aa_stats* stats /* may be NULL */);

/* AUTO EXPOSURE AND DISPLAY TONE MAPPING (no reference counterpart: the reference's sv4 Reinhard write takes an exposure the caller already
 * knows).  The chain's colour planes are linear radiance under an HDR probe, without an upper bound; pt_modulate_planes and
 * pt_edge_aa_planes end in make_color, which shows the part of that range inside [0, 1] at exposure 1.  pt_exposure_planes METERS a colour
 * plane — a histogram of log2 luminance per view — and ADAPTS an exposure per view from it; pt_tonemap_planes APPLIES that exposure and a
 * display operator.  Both are stateless: the planes, the histogram and the exposure state are caller-owned DEVICE memory of the context's
 * device (4-byte aligned; the planes frame-sized, indexed Y * width + X); block_mask is HOST memory.  The exposure travels from the meter to
 * the tone mapper through `state` in device memory: no host round trip.  The pixel set, views, partitions and pointer checks are exactly
 * pt_modulate_planes's; nv = max(1, the view count), and a pixel's view is 0 without views.  No pixel outside the set is written.
 *
 * pt_exposure_planes.  hist: nv x PT_EXPOSURE_BINS uint32; state_in (or NULL) and state_out: nv x 4 float (ev, E, m, n).
 * Flags: PT_EXPOSURE_ACCUMULATE — hist is not zeroed first (several planes or several calls into one histogram);
 * PT_EXPOSURE_FROM_HISTOGRAM — no metering, hist is read as given (color, hit and block_mask must then be NULL; ACCUMULATE has no effect):
 * each rank of a partitioned frame meters its own pixels, the caller all-reduces the integer histograms, and every rank derives the same
 * exposure.  Otherwise hist is zeroed, also when the set is empty (zero pixels launch no metering kernel; the adaptation still runs).
 * Metering, per pixel p of the set, into its view's histogram, in this order:
 *   1. If hit is given and hit[p].prim is negative (a miss), the pixel is not counted: stats->skipped.  prim is compared for its sign only;
 *      no address is formed from it.
 *   2. c = color[p].xyz.  If one of its three words is not finite (exponent-bit test), the pixel is not counted: stats->nonfinite.
 *   3. Y = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z, float32, one rounding per operation, no fused multiply-add.
 *      If !(Y > 0): bin 0.  If Y is not finite (the sum overflowed): bin 255.  Otherwise k = (int)(bits(Y) >> 20) - 887 and the bin is
 *      0 for k < 1, 255 for k > 254, else k: the exponent and the top three mantissa bits, eight bins per stop.  Bin 1 starts at 2^-16,
 *      bin 254 ends below 2^15.75 on the piecewise-linear log2 of step 4 below (at 1.75 * 2^15); denormals land in bin 0.  Every bin is an integer function of the bit pattern: no transcendental.
 *   4. hist[view][bin] += 1 (integer adds: the order does not matter, which is what makes the histogram bit-reproducible; no float is
 *      accumulated anywhere).  stats->under counts bin 0, stats->over bin 255; stats->pixels is the size of the set.
 * Adaptation, per view v, on the histogram words c[0..255] as uint64, integer arithmetic until the last step:
 *   1. N = sum c[i].
 *   2. lo = N * low_permille / 1000 and hi = N * high_permille / 1000 (integer division).
 *   3. Walking up from bin 0, take = min(c[i], lo) is removed from c[i] and from lo; then walking down from bin 255 likewise with hi.
 *   4. n = sum over 1..254 of c[i]; S = sum over 1..254 of c[i] * (2i - 1).  Bin i stands for log2 luminance -16 + (2i - 1) / 16, its
 *      middle on the piecewise-linear log2 (exponent plus mantissa fraction), which is off from the true log2 by at most 0.09 stops.
 *   5. ev_prev = state_in[4v].  If n == 0: m = state_in[4v + 2], or a NaN (0x7fc00000) when state_in is NULL; ev = ev_prev when state_in is
 *      given and ev_prev is finite, else 0.0f.
 *   6. Otherwise q = (S << 12) / n in uint64 (q < 2^21); m = (float)q * (1.0f / 65536.0f) - 16.0f; t = key_log2 - m;
 *      t = t < ev_min ? ev_min : t; t = t > ev_max ? ev_max : t.  If state_in is NULL or ev_prev is not finite: ev = t.  Else
 *      r = (t > ev_prev) ? rate_up : rate_down and ev = ev_prev + ((t - ev_prev) * r).
 *   7. E = pt_expf(ev * 0.69314718f), include/pt_detmath.h's function (the same header compiled for the host gives the same bits).
 *   8. state_out[4v .. 4v + 3] = (ev, E, m, (float)n).  state_out may be exactly state_in.
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet; hist or
 * state_out NULL; color NULL without FROM_HISTOGRAM; color, hit or block_mask given with it; a plane that fails the pointer checks; a
 * forbidden overlap (hist and state_out overlap nothing, except state_out exactly state_in); an unknown flag bit;
 * low_permille + high_permille > 999; key_log2 not finite; ev_min or ev_max outside [-24, 24] or NaN, or ev_min > ev_max; a rate outside
 * [0, 1] or NaN.
 *
 * pt_tonemap_planes.  state: pt_exposure_planes's state_out, or NULL.  out may be exactly color (the pass is pixel-local); at least one
 * of out and frame_rgba8 is given.  Per pixel p of the set, float32, one rounding per operation:
 *   1. E_v = state ? state[4 * view + 1] : 1.0f; an E_v that is not finite or not > 0 counts as 1.0f.   2. s = E_v * exposure.
 *   3. Per component: x = c * s; x = x > 0 ? x : 0 (a NaN becomes 0); x = x < 65504.0f ? x : 65504.0f (an inf becomes 65504).
 *   4. PT_TONEMAP_LINEAR: y = x.  PT_TONEMAP_REINHARD: the frame path's own operator on the whole colour,
 *      L = (0.2126f * x.r + 0.7152f * x.g) + 0.0722f * x.b; i = 1.0f / (1.0f + L / white); y = (x * 1.0f) * i per component (so that
 *      pt_render_regions with tonemap = 1 and this pass leave the same bytes).  PT_TONEMAP_ACES (Narkowicz's fit), per component:
 *      a = x * (2.51f * x + 0.03f); b = x * (2.43f * x + 0.59f) + 0.14f; y = a / b.
 *   5. out[p] = (y, 1.0f); frame_rgba8[p] = make_color(y), the frame path's transform (clamp, sRGB, 8 bits, alpha 255).
 *      stats->clipped counts the pixels with a component of y above 1.
 * Refused with PT_ERR_INVALID likewise: a null ctx or desc; no pt_resize yet; color NULL; out and frame_rgba8 both NULL; a plane that
 * fails the pointer checks; a forbidden overlap (out and frame_rgba8 overlap nothing, except out exactly color); flags != 0; an unknown
 * op; exposure or white not finite or not > 0.
 * Ordering and state, both entry points, as pt_modulate_planes: they wait for the frames in flight, run on pt_stream(ctx) under the STREAM
 * CONTRACT, are complete when they return, and write no context state.
 * Not part of this interface: spatially varying or centre-weighted metering; local tone mapping; bloom (pt_bloom_planes below, in front of
 * the tone mapper); a colour-managed output other than sRGB; an asynchronous variant; a pt_multi_* wrapper (per-rank calls and FROM_HISTOGRAM serve a partitioned frame). */
#define PT_EXPOSURE_BINS 256
enum pt_exposure_flags { PT_EXPOSURE_ACCUMULATE = 1, PT_EXPOSURE_FROM_HISTOGRAM = 2 };
typedef struct pt_exposure_desc {
    const float* color;        /* w*h x 4: linear radiance (.w ignored); required unless FROM_HISTOGRAM */
    const void*  hit;          /* w*h x pt_hit or NULL: misses are not metered */
    uint32_t*    hist;         /* nv x PT_EXPOSURE_BINS; required, exclusive */
    const float* state_in;     /* nv x 4 or NULL: the previous frame's state_out */
    float*       state_out;    /* nv x 4: ev, E = 2^ev, m (mean log2 luminance), n (pixels metered after trimming); required */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    uint32_t  low_permille, high_permille; /* shares of the histogram trimmed at its dark and bright ends; sum <= 999 */
    float     key_log2;        /* log2 of the luminance the mean is mapped to (log2(0.18) = -2.47); finite */
    float     ev_min, ev_max;  /* [-24, 24], ev_min <= ev_max */
    float     rate_up, rate_down; /* [0, 1]: the share of the step taken per call towards a larger / smaller ev */
    uint32_t  flags;           /* pt_exposure_flags */
} pt_exposure_desc;
typedef struct pt_exposure_stats { uint64_t pixels, skipped, nonfinite, under, over; double kernel_ms; } pt_exposure_stats;
int pt_exposure_planes(pt_ctx* ctx, const pt_exposure_desc* desc, pt_exposure_stats* stats /* may be NULL */);

enum pt_tonemap_op { PT_TONEMAP_LINEAR = 0, PT_TONEMAP_REINHARD = 1, PT_TONEMAP_ACES = 2 };
typedef struct pt_tonemap_desc {
    const float* color;        /* w*h x 4: linear radiance (.w ignored); required */
    const float* state;        /* nv x 4 (pt_exposure_planes's state_out) or NULL */
    float*    out;             /* w*h x 4 or NULL, exclusive except that it may be exactly color */
    uint32_t* frame_rgba8;     /* w*h or NULL, exclusive */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    float     exposure;        /* finite, > 0: multiplies the metered exposure */
    float     white;           /* finite, > 0: PT_TONEMAP_REINHARD's white point */
    uint32_t  op;              /* pt_tonemap_op */
    uint32_t  flags;           /* 0 */
} pt_tonemap_desc;
typedef struct pt_tonemap_stats { uint64_t pixels, clipped; double kernel_ms; } pt_tonemap_stats;
int pt_tonemap_planes(pt_ctx* ctx, const pt_tonemap_desc* desc, pt_tonemap_stats* stats /* may be NULL */);

/* BLOOM (no reference counterpart).  Under an HDR probe a sun disc, a window or an emitter lies stops above the key; pt_tonemap_planes
 * compresses it to a hard-edged white shape and nothing of its energy reaches the pixels around it.  pt_bloom_planes spreads the part of
 * the colour plane above a threshold over a pyramid of levels and adds it back: out = color + a * (the filtered bright part).  It is
 * stateless like every pass here: the planes, the state and the scratch pyramid are caller-owned DEVICE memory of the context's device
 * (4-byte aligned, the scratch 16-byte aligned; the planes frame-sized, indexed Y * width + X); block_mask is HOST memory.  It runs behind
 * pt_modulate_planes / pt_edge_aa_planes and in front of pt_tonemap_planes: the bloom stays in scene-linear units, so `out` goes through
 * pt_tonemap_planes with the same state.  Float32 throughout, one rounding per operation, no fused multiply-add, in the stated order.
 *
 * Rectangles.  Each view's rectangle (x0, y0, w_0, h_0) has a pyramid of its own; without views there is one rectangle, the whole frame;
 * nv = max(1, the view count).  Level k = 1 .. levels has w_k = (w_{k-1} + 1) / 2 and h_k = (h_{k-1} + 1) / 2 (integer division): sizes
 * bottom out at 1 and the level count is not reduced.  No tap ever leaves its rectangle: indices clamp to it, so a bright pixel in one eye
 * of a stereo pair puts nothing into the other.
 * pt_bloom_layout gives the scratch: *bytes for `levels` levels of every view, view after view, level 1 first, each level w_k * h_k texels
 * of 16 bytes (x, y, z, 0) in row order; dims (HOST, nv x PT_BLOOM_MAX_LEVELS x 4, may be NULL) receives w_k, h_k, the index of the
 * level's first 16-byte texel and 0 for k = 1 .. levels, and zeros for the levels above.  It refuses (PT_ERR_INVALID) a null ctx or
 * bytes, a context without pt_resize, and levels outside 1 .. PT_BLOOM_MAX_LEVELS.
 *
 * What is read, what is written.  The pyramid reads EVERY pixel of every rectangle from color, whether or not the rank owns it or the mask
 * names it; the set decides only which pixels of out are written.  The set is exactly pt_modulate_planes's: owned pixels, view pixels
 * while views are set, whole blocks of the mask.  Bloom is not local: the ranks of a partitioned frame all-gather their colour first and
 * then each composites its own pixels, and a masked call still sees the light of the blocks it does not write.  stats->sources is the
 * number of rectangle pixels read, stats->pixels the size of the set.  The whole scratch is written by every call, also with an empty set.
 *
 * Source.  For each rectangle pixel q, B(q):
 *   1. c = color[q].xyz.  If one of its three words is not finite (exponent-bit test): B = 0 and stats->nonfinite counts it — one NaN must
 *      not spread through the pyramid.
 *   2. Per component: x = c > 0 ? c : 0; x = x < clamp ? x : clamp (one firefly must not own the frame).
 *   3. s = E_v * exposure, E_v read exactly as pt_tonemap_planes step 1 reads it (state ? state[4 * view + 1] : 1.0f; not finite or not > 0
 *      counts as 1.0f).
 *   4. Y = ((0.2126f * x.r + 0.7152f * x.g) + 0.0722f * x.b) * s; d = Y - threshold.
 *   5. t = d + knee; t = t > 0 ? t : 0; t = t < 2.0f * knee ? t : 2.0f * knee.
 *   6. t = (t * t) / (4.0f * knee + 1e-4f).
 *   7. m = t > d ? t : d; m = m > 0 ? m : 0.
 *   8. g = m / (Y > 1e-4f ? Y : 1e-4f); B = x * g per component.
 *   9. stats->bright counts g > 0.
 * g is 0 at and below threshold - knee, and Y * g rises with Y.  For knee <= threshold g stays within [0, 1]; a knee larger than the
 * threshold reaches below Y = 0, where g = m / Y exceeds 1 for dim pixels while their contribution m stays below knee / 4.
 * Down.  D_0 = B.  Texel (i, j) of D_k from D_{k-1}: columns 2i - 1, 2i, 2i + 1, 2i + 2, each clamped to [0, w_{k-1} - 1], rows likewise
 * from j; with S0 .. S3 the four columns of a row, r = ((S0 + 3.0f * S1) + 3.0f * S2) + S3; with r0 .. r3 the four rows,
 * v = ((r0 + 3.0f * r1) + 3.0f * r2) + r3; D_k = v * (1.0f / 64.0f).
 * Up, in place in the scratch.  U_levels = D_levels; for k = levels - 1 down to 1: U_k = D_k + spread * up_k(U_{k+1}).  up_k at texel
 * (x, y) of level k: i = x >> 1; i2 = (x & 1) ? min(i + 1, w_{k+1} - 1) : max(i - 1, 0); j and j2 likewise from y and h_{k+1};
 * up = 0.75f * (0.75f * U(i, j) + 0.25f * U(i2, j)) + 0.25f * (0.75f * U(i, j2) + 0.25f * U(i2, j2)).  After the call level k of the
 * scratch holds U_k.
 * Composite.  For a pixel p of the set, with (x, y) its coordinates in its rectangle: out[p].xyz = color[p].xyz + a * up_0(U_1) and
 * out[p].w = 1.0f, where a = intensity * (1.0f / n) with n = 1; repeat levels - 1 times: n = n * spread + 1 (float32, on the host): a
 * constant source of value B comes back as intensity * B.  color[p] enters raw: a NaN pixel stays NaN, and the tone mapper turns it into 0.
 * out may be exactly color: the pyramid is complete before the first pixel is written.
 *
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx, desc, color, out or scratch; no
 * pt_resize yet; a plane that fails the pointer checks; scratch not 16-byte aligned; a forbidden overlap (out and scratch overlap nothing,
 * except out exactly color); flags != 0; levels outside 1 .. PT_BLOOM_MAX_LEVELS; exposure or clamp not finite or not > 0; threshold, knee
 * or intensity not finite or < 0; spread outside [0, 1] or NaN.
 * Ordering and state, as pt_tonemap_planes: the call waits for the frames in flight, runs on pt_stream(ctx) under the STREAM CONTRACT, is
 * complete when it returns, and writes no context state.
 * Not part of this interface: lens-flare or anamorphic shapes and a dirt mask; sources restricted by the hit plane (sky only, emitters
 * only); temporal smoothing of the pyramid; a pyramid kept across calls; an asynchronous variant; a pt_multi_* wrapper (per-rank calls work
 * once the colour is gathered); the composite fused into pt_tonemap_planes. */
#define PT_BLOOM_MAX_LEVELS 8
/* scratch pyramid in caller memory: bytes for `levels` levels of every view (or of the frame without views);
 * dims (HOST, nv x PT_BLOOM_MAX_LEVELS x 4: w_k, h_k, first float4 of the level, 0; may be NULL) */
int pt_bloom_layout(const pt_ctx* ctx, uint32_t levels, uint32_t* dims, size_t* bytes);

typedef struct pt_bloom_desc {
    const float* color;      /* w*h x 4 linear radiance (.w ignored); required */
    const float* state;      /* nv x 4 (pt_exposure_planes's state_out) or NULL */
    float*       out;        /* w*h x 4; required; exclusive except that it may be exactly color */
    void*        scratch;    /* pt_bloom_layout's bytes, 16-byte aligned; required, exclusive */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    float exposure;          /* finite, > 0: multiplies the metered exposure, as in pt_tonemap_desc */
    float threshold;         /* finite, >= 0, on exposed luminance */
    float knee;              /* finite, >= 0 */
    float clamp;             /* finite, > 0: source radiance is clamped to it (one firefly must not own the frame) */
    float spread;            /* [0, 1]: weight of each coarser level relative to the next finer one */
    float intensity;         /* finite, >= 0 */
    uint32_t levels;         /* 1..PT_BLOOM_MAX_LEVELS */
    uint32_t flags;          /* 0 */
} pt_bloom_desc;
typedef struct pt_bloom_stats { uint64_t pixels, sources, bright, nonfinite; double kernel_ms; } pt_bloom_stats;
int pt_bloom_planes(pt_ctx* ctx, const pt_bloom_desc* desc, pt_bloom_stats* stats /* may be NULL */);

/* MOTION BLUR (no reference counterpart).  The motion plane of pt_render_gbuffer / pt_motion_planes is used by the reprojection passes to
 * REMOVE the effect of motion; every frame of the chain has a shutter time of zero, and a loop whose camera or meshes move looks like a
 * stop-motion sequence.  pt_motion_blur_planes blurs each pixel of a linear colour plane along the dominant motion around it, after McGuire
 * et al., "A Reconstruction Filter for Plausible Motion Blur" (2012): tile maximum, neighbourhood maximum, then a depth-aware gather.  It
 * runs behind pt_edge_aa_planes / pt_bloom_planes and in front of pt_tonemap_planes.  Stateless like every pass here: the planes and the
 * scratch are caller-owned DEVICE memory of the context's device (4-byte aligned, the scratch 8-byte aligned; the planes frame-sized,
 * indexed Y * width + X); block_mask is HOST memory.  Float32 throughout, one rounding per operation, no fused multiply-add, sqrtf and /
 * correctly rounded (pt_detmath.h's contract), in the stated order; max(a, b) is a > b ? a : b, min(a, b) is a < b ? a : b, and
 * clamp01(x) is x = x > 0 ? x : 0; x = x < 1 ? x : 1 (a NaN becomes 0).
 *
 * Rectangles and tiles.  Each view's rectangle (x0, y0, wr, hr) has a tile grid of its own, anchored at the rectangle's origin; without
 * views there is one rectangle, the whole frame; nv = max(1, the view count).  The grid is tw = (wr + 15) / 16 by th = (hr + 15) / 16
 * tiles of PT_MOTION_BLUR_TILE = 16 pixels a side, partial at the right and at the bottom.  No tap and no tile neighbour ever leaves its
 * rectangle: a fast object in one eye of a stereo pair puts nothing into the other, and a view holds the bits a context of its own size
 * would hold.
 * pt_motion_blur_layout gives the scratch: view after view, a plane T of tw * th texels of 8 bytes (V.x, V.y) in row order, then a plane
 * N of the same size; *bytes is their sum.  dims (HOST, nv x 4, may be NULL) receives tw, th, the index of T's first 8-byte texel and the
 * index of N's.  It refuses (PT_ERR_INVALID) a null ctx or bytes and a context without pt_resize.
 *
 * What is read, what is written.  The tile pass reads EVERY pixel of every rectangle from motion, whether or not the rank owns it or the
 * mask names it, and a tap of the gather reads color, motion and depth wherever in the rectangle it lands; the set decides only which pixels
 * of out are written.  The set is exactly pt_modulate_planes's: owned pixels, view pixels while views are set, whole blocks of the mask.
 * The ranks of a partitioned frame all-gather colour, motion and depth first.  stats->sources is the number of rectangle pixels read by
 * the tile pass, stats->pixels the size of the set.  The whole scratch is written by every call, also with an empty set.
 *
 * The host computes hs = 0.5f * shutter, R = max_blur and R2 = R * R.
 *   1. Velocity V(q), l2(q) of a rectangle pixel q, from m = motion[q] (previous minus current position, in pixels).  If one of the two
 *      words of m is not finite (exponent-bit test): V = (0, 0), l2 = 0, and stats->unknown counts it (in the tile pass: once per rectangle
 *      pixel).  Otherwise V = m * hs per component — the half-spread: the blur is centred on the current position — then per component
 *      v = v < -4096.0f ? -4096.0f : v; v = v > 4096.0f ? 4096.0f : v (l2 cannot overflow); l2 = V.x * V.x + V.y * V.y.  If l2 > R2:
 *      s = R / sqrtf(l2); V = V * s per component; l2 = V.x * V.x + V.y * V.y again, from the scaled V.
 *   2. Tile maximum.  T(i, j) is the V of greatest l2 among the pixels of tile (i, j) that lie inside the rectangle; ties go to the first
 *      pixel in row order.
 *   3. Neighbourhood maximum.  N(i, j) is the T of greatest l2 = T.x * T.x + T.y * T.y over the 3 x 3 tiles around (i, j) that exist in
 *      the rectangle's grid, visited in row order with a strict >: the first maximum wins.  Because R <= PT_MOTION_BLUR_TILE nothing
 *      farther away can reach the tile.
 *   4. Gather, for a pixel p of the set with (x, y) its coordinates in its rectangle: c = color[p].xyz; vN = N(x / 16, y / 16);
 *      n2 = vN.x * vN.x + vN.y * vN.y.  If n2 > 0.25f is false, or a word of c is not finite: out[p] = (c, 1.0f), raw, and that is all.
 *      Otherwise stats->moving counts p, and
 *        lN = sqrtf(n2); lp = max(sqrtf(l2(p)), 0.5f); wp = 1.0f / lp; zp = Z(depth[p]);
 *        Z(d) = (d > 1e-6f && d <= FLT_MAX) ? d : FLT_MAX — a NaN, an inf, 0 and negatives all become FLT_MAX (a miss holds +inf);
 *        sum = (0, 0, 0); Wt = 0; then for tap i = 0 .. taps - 1, in this order:
 *          a = ((float)i + 0.5f) + j;  t = (2.0f * a) / (float)taps - 1.0f;
 *          qx = (int)floorf(((float)x + vN.x * t) + 0.5f), clamped to [0, wr - 1]; qy = (int)floorf(((float)y + vN.y * t) + 0.5f), clamped
 *          to [0, hr - 1]; q is that pixel of the rectangle.
 *          If a word of color[q].xyz is not finite the tap is skipped and stats->nonfinite counts it.  Otherwise
 *          d = fabsf(t) * lN; lq = max(sqrtf(l2(q)), 0.5f), with V(q) recomputed by step 1; zq = Z(depth[q]);
 *          e = depth_soft * min(zp, zq);
 *          fg = clamp01(1.0f - (zq - zp) / e); bg = clamp01(1.0f - (zp - zq) / e);
 *          cone(l) = clamp01(1.0f - d / l);
 *          cyl(l) = 1.0f - (u * u) * (3.0f - 2.0f * u), with u = clamp01((d - 0.95f * l) / (1.05f * l - 0.95f * l));
 *          w = (fg * cone(lq) + bg * cone(lp)) + (cyl(lq) * cyl(lp)) * 2.0f;
 *          sum = sum + color[q].xyz * w per component; Wt = Wt + w; stats->taps counts w > 0.
 *      The jitter j is 0.0f without PT_MOTION_BLUR_JITTER.  With it, j = (float)(h >> 8) * 5.9604644775390625e-8f - 0.5f (2^-24: j lies in
 *      [-0.5, 0.5)), where h is this hash of the LOCAL coordinates and the seed, exact in uint32 arithmetic:
 *          h = ((uint32_t)x * 0x9E3779B1u) ^ ((uint32_t)y * 0x85EBCA77u) ^ (seed * 0xC2B2AE3Du);
 *          h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16.
 *      If Wt == 0: out[p].xyz = c exactly.  Else out[p].xyz = (c * wp + sum) / (wp + Wt) per component.  out[p].w = 1.0f.
 * Zero motion, an all-unknown motion plane and shutter = 0 give out = (color.xyz, 1) bit for bit, with T and N all zero.  A pixel that
 * stands still (lp = 0.5) in front of a moving background takes nothing from it once a tap is 0.525 pixels away: with an even tap count and
 * lN / taps >= 0.525 it keeps its bits (Wt == 0).  Every weight is >= 0, so a finite out[p] lies within the range of the finite colours
 * up to the roundings of its sums; a non-finite motion, depth or colour word reaches no pixel but the one that holds the bad colour.
 *
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx, desc, color, motion, depth, out or
 * scratch; no pt_resize yet; a plane that fails the pointer checks; scratch not 8-byte aligned; any overlap that involves out or scratch
 * (out may NOT be color: the gather reads neighbours); flag bits other than PT_MOTION_BLUR_JITTER; shutter not finite or outside [0, 4];
 * max_blur not finite or outside [1, PT_MOTION_BLUR_TILE]; depth_soft not finite or outside (0, 1]; taps outside 1 .. 64.
 * Ordering and state, as pt_bloom_planes: the call waits for the frames in flight, runs on pt_stream(ctx) under the STREAM CONTRACT, is
 * complete when it returns, and writes no context state.
 * Not part of this interface: the paper's refinement of the neighbour maximum (off-diagonal tiles only when they point at the centre);
 * more than one dominant direction per tile; sub-pixel (bilinear) taps; blur of the bloom pyramid; an asynchronous variant; a pt_multi_*
 * wrapper (per-rank calls work once colour, motion and depth are gathered); camera-shutter curves. */
#define PT_MOTION_BLUR_TILE 16
typedef enum pt_motion_blur_flags { PT_MOTION_BLUR_JITTER = 1 } pt_motion_blur_flags;
/* scratch in caller memory: bytes for T and N of every view (or of the frame without views);
 * dims (HOST, nv x 4: tw, th, first 8-byte texel of T, first 8-byte texel of N; may be NULL) */
int pt_motion_blur_layout(const pt_ctx* ctx, uint32_t* dims, size_t* bytes);

typedef struct pt_motion_blur_desc {
    const float* color;      /* w*h x 4 linear radiance (.w ignored); required */
    const float* motion;     /* w*h x 2, pt_render_gbuffer's / pt_motion_planes's format (a NaN pair: unknown); required */
    const float* depth;      /* w*h, the G-buffer's depth (a miss holds +inf); required */
    float*       out;        /* w*h x 4; required; exclusive (it may NOT be color) */
    void*        scratch;    /* pt_motion_blur_layout's bytes, 8-byte aligned; required, exclusive */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    float shutter;           /* finite, in [0, 4]: the open fraction of the frame interval */
    float max_blur;          /* finite, in [1, PT_MOTION_BLUR_TILE]: R, in pixels */
    float depth_soft;        /* finite, in (0, 1]: the relative depth extent over which foreground turns into background */
    uint32_t taps;           /* 1..64 */
    uint32_t seed;           /* of the jitter's hash */
    uint32_t flags;          /* pt_motion_blur_flags */
} pt_motion_blur_desc;
typedef struct pt_motion_blur_stats { uint64_t pixels, sources, unknown, moving, taps, nonfinite; double kernel_ms; } pt_motion_blur_stats;
int pt_motion_blur_planes(pt_ctx* ctx, const pt_motion_blur_desc* desc, pt_motion_blur_stats* stats /* may be NULL */);

/* DEPTH OF FIELD (no reference counterpart).  The frame path's camera is a pinhole (it is pinned to the reference's device programs), so
 * every frame of the chain is sharp from the near plane to the sky.  pt_dof_planes gives the chain a thin lens as a post pass: each pixel of
 * a linear colour plane gathers a disc of up to 64 taps whose radius is the largest blur circle around it, with a foreground/background rule
 * that decides who may bleed over whom.  It is motion blur's family — tile maximum, neighbourhood maximum, then a variable gather — with a
 * 2-D disc for the line.  It runs behind pt_edge_aa_planes and in front of pt_bloom_planes, pt_motion_blur_planes and pt_tonemap_planes, so
 * that bright out-of-focus points bloom as discs.  Stateless like every pass here: the planes and the scratch are caller-owned DEVICE memory
 * of the context's device (4-byte aligned; the planes frame-sized, indexed Y * width + X); block_mask and view_focus are HOST memory.
 * Float32 throughout, one rounding per operation, no fused multiply-add, sqrtf and / correctly rounded (pt_detmath.h's contract), in the
 * stated order; max(a, b) is a > b ? a : b, min(a, b) is a < b ? a : b, and clamp01(x) is x = x > 0 ? x : 0; x = x < 1 ? x : 1 (a NaN
 * becomes 0).
 *
 * The lens.  depth is pt_render_gbuffer's: distance along the viewing axis, which is the thin lens's z.  A point at depth z seen through a
 * lens of aperture diameter A and focal length f focused at distance s has a blur circle of diameter A * f / (s - f) * |1 - s / z| on the
 * sensor.  `aperture` folds the lens into one number, the blur-circle RADIUS in pixels of a point at infinity:
 *     K = 0.5 * A * f / (s - f) * px_per_unit        (px_per_unit: pixels per unit of length on the sensor, frame height / sensor height)
 * and `focus` is s in depth units.  Autofocus is the caller's: read depth under a view's centre and smooth it over frames.
 *
 * Rectangles and tiles are exactly motion blur's.  Each view's rectangle (x0, y0, wr, hr) has a tile grid of its own, anchored at the
 * rectangle's origin; without views there is one rectangle, the whole frame; nv = max(1, the view count).  The grid is tw = (wr + 15) / 16
 * by th = (hr + 15) / 16 tiles of PT_DOF_TILE = 16 pixels a side, partial at the right and at the bottom.  No tap and no tile neighbour ever
 * leaves its rectangle, and a view holds the bits a context of its own size would hold.
 * pt_dof_layout gives the scratch: view after view, a plane T of tw * th floats of 4 bytes in row order, then a plane N of the same size;
 * *bytes is their sum.  dims (HOST, nv x 4, may be NULL) receives tw, th, the index of T's first 4-byte texel and the index of N's.  It
 * refuses (PT_ERR_INVALID) a null ctx or bytes and a context without pt_resize.
 *
 * What is read, what is written.  The tile pass reads EVERY pixel of every rectangle from depth, whether or not the rank owns it or the mask
 * names it, and a tap of the gather reads depth and color wherever in the rectangle it lands; the set decides only which pixels of out are
 * written.  The set is exactly pt_modulate_planes's: owned pixels, view pixels while views are set, whole blocks of the mask.  The ranks of
 * a partitioned frame all-gather colour and depth first.  stats->sources is the number of rectangle pixels read by the tile pass,
 * stats->pixels the size of the set.  The whole scratch is written by every call, also with an empty set.
 *
 * The host computes K = aperture + 0.0f (a -0 becomes +0), R = max_radius, PI = 3.14159274f, and per view Fv = view_focus ? view_focus[v]
 * : focus.
 *   1. Blur radius r(q) of a rectangle pixel q: z = Z(depth[q]) with motion blur's Z(d) = (d > 1e-6f && d <= FLT_MAX) ? d : FLT_MAX — a NaN,
 *      an inf, 0 and negatives all become FLT_MAX: a miss (+inf) is far; r = K * fabsf(1.0f - Fv / z); r = r < R ? r : R.  Fv <= 1e30 and
 *      z > 1e-6, so Fv / z cannot overflow: r is never NaN and r >= 0 (K times a finite number, possibly +inf, then the minimum).
 *   2. Tile maximum.  T(i, j) = max r over the pixels of tile (i, j) that lie inside the rectangle: a maximum of non-negative, non-NaN
 *      floats, so it is independent of the order of the reduction.
 *   3. Neighbourhood maximum.  N(i, j) = max T over the 3 x 3 tiles around (i, j) that exist in the rectangle's grid.  Because
 *      R <= PT_DOF_TILE nothing farther away can reach the tile.
 *   4. Gather, for a pixel p of the set with (x, y) its coordinates in its rectangle: c = color[p].xyz; rN = N(x / 16, y / 16).
 *      If rN > 0.5f is false, or a word of c is not finite (exponent-bit test): out[p] = (c, 1.0f), raw, and that is all.
 *      Otherwise stats->gathered counts p, and
 *        rp = r(p); zp = Z(depth[p]); area(r) = max((r * r) * PI, 1.0f); wp = 1.0f / area(rp);
 *        At = ((rN * rN) * PI) / (float)taps — the disc area one tap stands for;
 *        sum = (0, 0, 0); Wt = 0; then for tap i = 0 .. taps - 1, in this order:
 *          rho = sqrtf(((float)i + 0.5f) / (float)taps); d = rN * rho;
 *          qx = (int)floorf(((float)x + d * D[i + k0].x) + 0.5f), clamped to [0, wr - 1]; qy = (int)floorf(((float)y + d * D[i + k0].y) +
 *          0.5f), clamped to [0, hr - 1]; q is that pixel of the rectangle.
 *          rq = r(q); zq = Z(depth[q]);
 *          re = zq > zp ? rp : rq — a tap behind p is seen through p's own blur, a tap in front of p spreads by its own;
 *          cov = clamp01((re - d) + 0.5f); w = (cov * At) / area(re).
 *          If w > 0 is false the tap is done: its colour is never looked at.
 *          Otherwise, if a word of color[q].xyz is not finite the tap is skipped and stats->nonfinite counts it.
 *          Otherwise sum = sum + color[q].xyz * w per component; Wt = Wt + w; stats->taps counts it.
 *      If Wt == 0: out[p].xyz = c exactly.  Else out[p].xyz = (c * wp + sum) / (wp + Wt) per component.  out[p].w = 1.0f.
 *      The directions D[0 .. 127] are a Vogel spiral by recurrence, so that nobody's cosf enters the bits: D[0] = (1, 0) and
 *          D[n + 1] = (D[n].x * C - D[n].y * S, D[n].x * S + D[n].y * C),
 *      each component two products and one sum (a difference for x), rounded separately, in this order, with C = -0x1.79886ap-1f (bits
 *      0xBF3CC435, -0.73736888) and S = 0x1.59d9dep-1f (bits 0x3F2CECEF, 0.67549032) the floats nearest to the cosine and the sine of the
 *      golden angle pi (3 - sqrt 5).  Over 128 steps the norm drifts by less than 3e-6.
 *      The jitter k0 is 0 without PT_DOF_JITTER.  With it, k0 = h & 63 — the whole pattern turned by k0 golden angles — where h is motion
 *      blur's hash of the LOCAL coordinates and the seed, exact in uint32 arithmetic:
 *          h = ((uint32_t)x * 0x9E3779B1u) ^ ((uint32_t)y * 0x85EBCA77u) ^ (seed * 0xC2B2AE3Du);
 *          h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16.
 * aperture = 0, and a depth plane equal to the focus everywhere, give out = (color.xyz, 1) bit for bit, with T and N all +0.  Every r, T
 * and N lies in [0, R], and N >= T for the tile itself.  Every weight is >= 0, so a finite out[p] lies within the range of the finite
 * colours up to the roundings of its sums.  A pixel in focus (rp = 0) in front of a blurred background keeps its bits once the first tap is
 * half a pixel away, rN * sqrtf(0.5f / taps) >= 0.5: every tap then has cov = 0 or lands on a pixel with r = 0 at d >= 0.5.  A blurred
 * foreground reaches at most ceil(rq + 0.5) pixels outside its edge.  A hostile word in depth, or a non-finite colour, reaches no pixel but
 * the one that holds the bad colour.
 *
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx, desc, color, depth, out or scratch;
 * no pt_resize yet; a plane that fails the pointer checks; any overlap that involves out or scratch (out may NOT be color: the gather reads
 * neighbours); flag bits other than PT_DOF_JITTER; focus, or any view_focus[v], not finite or outside (0, 1e30]; aperture not finite or
 * outside [0, 4096]; max_radius not finite or outside [1, PT_DOF_TILE]; taps outside 1 .. 64.
 * Ordering and state, as pt_motion_blur_planes: the call waits for the frames in flight, runs on pt_stream(ctx) under the STREAM CONTRACT,
 * is complete when it returns, and writes no context state.
 * Not part of this interface: hexagonal or cat-eye bokeh; a separate near-field layer and background reconstruction behind blurred
 * foregrounds; sub-pixel (bilinear) taps; a half-resolution pre-filter; per-view apertures; motion blur that knows the blur circle; an
 * asynchronous variant; a pt_multi_* wrapper (per-rank calls work once colour and depth are gathered). */
#define PT_DOF_TILE 16
typedef enum pt_dof_flags { PT_DOF_JITTER = 1 } pt_dof_flags;
/* scratch in caller memory: bytes for T and N of every view (or of the frame without views);
 * dims (HOST, nv x 4: tw, th, first 4-byte texel of T, first 4-byte texel of N; may be NULL) */
int pt_dof_layout(const pt_ctx* ctx, uint32_t* dims, size_t* bytes);

typedef struct pt_dof_desc {
    const float* color;        /* w*h x 4 linear radiance (.w ignored); required */
    const float* depth;        /* w*h, the G-buffer's depth (a miss holds +inf); required */
    float*       out;          /* w*h x 4; required; exclusive (it may NOT be color) */
    void*        scratch;      /* pt_dof_layout's bytes, 4-byte aligned; required, exclusive */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    const float* view_focus;   /* HOST, nv floats: a focus distance per view; NULL: `focus` for all */
    float focus;               /* finite, in (0, 1e30]: the distance (depth units) that is sharp */
    float aperture;            /* finite, in [0, 4096]: K, the blur-circle RADIUS in pixels of a point at infinity */
    float max_radius;          /* finite, in [1, PT_DOF_TILE]: R, in pixels */
    uint32_t taps;             /* 1..64 */
    uint32_t seed;             /* of the jitter's hash */
    uint32_t flags;            /* pt_dof_flags */
} pt_dof_desc;
typedef struct pt_dof_stats { uint64_t pixels, sources, gathered, taps, nonfinite; double kernel_ms; } pt_dof_stats;
int pt_dof_planes(pt_ctx* ctx, const pt_dof_desc* desc, pt_dof_stats* stats /* may be NULL */);

/* LENS WARP AND LATE REPROJECTION (no reference counterpart).  The chain ends in a tone-mapped PINHOLE image per view, which no head-mounted
 * display can show: its lenses bend the image, each colour a little differently, and by scan-out the head has turned.  pt_lens_warp_planes
 * is the last pass, behind pt_tonemap_planes: per view it resamples the display colour through (a) a radial polynomial around the lens
 * centre, with its own coefficients for red, green and blue (lens pre-distortion and chromatic-aberration correction), and (b) a 3x3
 * matrix in the view's pixel coordinates (rotational late reprojection, "timewarp": pt_warp_matrix below builds it from two cameras).  The
 * same pass gives a synthetic-data user a camera with radial distortion.  Both map an OUTPUT pixel to the SOURCE point its colour comes
 * from, so the pass is a gather: three data-dependent sub-pixel positions per pixel, bilinear or Catmull-Rom.  The frame path's camera
 * stays the reference's pinhole, as for depth of field.  Stateless like every pass here: the planes are caller-owned DEVICE memory of the
 * context's device (4-byte aligned, frame-sized, indexed Y * width + X); block_mask and lenses are HOST memory.
 *
 * Rule, per pixel.  The pixel set, the views, the partitions, the pointer checks and nv = max(1, the view count) are exactly
 * pt_modulate_planes's.  A pixel p of the set lies in rectangle (x0, y0, wr, hr) of view v at local (x, y); without views the rectangle is
 * the frame.  Arithmetic is float32, one rounding per operation, no fused multiply-add, / correctly rounded (pt_detmath.h's contract), in
 * this order.  For channel ch = 0, 1, 2 with (k1, k2, k3) = lenses[v].k[ch], (cx, cy) = center, (irx, iry) = inv_radius and H = warp:
 *   1. px = (float)x + 0.5f; py = (float)y + 0.5f; qx = px - cx; qy = py - cy.
 *   2. ax = qx * irx; ay = qy * iry; r2 = ax * ax + ay * ay; g = r2 * (k1 + r2 * (k2 + r2 * k3)).
 *   3. ux = px + qx * g; uy = py + qy * g.  Written like this, k = 0 gives ux = px bit for bit.
 *   4. a = (H[0]*ux + H[1]*uy) + H[2]; b = (H[3]*ux + H[4]*uy) + H[5]; c = (H[6]*ux + H[7]*uy) + H[8].
 *   5. The channel is OUTSIDE unless c > 0.  Then sx = a / c; sy = b / c, and the channel is outside unless
 *      sx >= 0 && sx <= (float)wr && sy >= 0 && sy <= (float)hr.  Every comparison is written so that a NaN is outside.  No float is
 *      converted to int and no address is formed before this test has passed.
 *   6. fx = sx - 0.5f; fy = sy - 0.5f; flx = floorf(fx); fly = floorf(fy); ix = (int)flx; iy = (int)fly; tx = fx - flx; ty = fy - fly.
 *   7. Bilinear (no flag).  Taps are (ix + i, iy + j) for i, j in {0, 1}, each coordinate clamped to the rectangle ([0, wr - 1], [0, hr - 1]).
 *      Weights are wx = {1.0f - tx, tx}, wy likewise, and w_ij = wx[i] * wy[j].  Channel word c_ij of color at the tap is read as 0.0f
 *      if it is not finite (exponent-bit test); stats->nonfinite counts such words, once per channel and tap that read them.
 *      val = ((c00*w00 + c10*w10) + c01*w01) + c11*w11.  All four taps are always read.
 *   8. Bicubic (PT_LENS_WARP_BICUBIC, Catmull-Rom, separable).  Taps are ix - 1 .. ix + 2 by iy - 1 .. iy + 2, clamped to the rectangle.
 *      w0 = ((-0.5f*t + 1.0f)*t - 0.5f)*t; w1 = ((1.5f*t - 2.5f)*t)*t + 1.0f; w2 = ((-1.5f*t + 2.0f)*t + 0.5f)*t; w3 = ((0.5f*t - 0.5f)*t)*t,
 *      in x from tx (wx0 .. wx3) and in y from ty (wy0 .. wy3).  Row j: row_j = ((c0j*wx0 + c1j*wx1) + c2j*wx2) + c3j*wx3.
 *      val = ((row0*wy0 + row1*wy1) + row2*wy2) + row3*wy3.  Non-finite words are handled as in step 7.
 *   9. The channel's value is val, or border[ch] when outside.  out[p] = (r, g, b, all three inside ? 1.0f : 0.0f);
 *      frame_rgba8[p] = make_color(r, g, b).  stats->outside counts pixels with .w == 0; stats->pixels is the size of the set.
 * No tap leaves its view's rectangle.  A tap reads color wherever in the rectangle it lands, whether or not the rank owns that pixel or the
 * mask names it: the set decides only what is written (the rule depth of field and motion blur state; the ranks of a partitioned frame
 * all-gather the colour first).  lenses == NULL stands for k = 0 and warp = identity for every view; that, or explicit lenses with k = 0
 * and the identity matrix, gives out.xyz equal to color.xyz (finite words) with .w = 1: steps 1 to 6 return fx == x and fy == y exactly,
 * so tx = ty = 0 and the one tap of weight 1 is the pixel itself; the only bit that may differ is a -0 that becomes +0.  Coefficients as
 * large as 1e6 make r2 and g overflow: the pixel comes out outside, nothing faults.  A matrix that turns the camera by more than 90
 * degrees has c <= 0 over part of the frame: that part is border colour.  inv_radius = 0 switches the polynomial off (r2 = 0).
 * When the three k rows of every view are equal word for word, the three channels share one source point and the library computes it once;
 * the bits are the same.
 *
 * Refused with PT_ERR_INVALID (nothing enqueued, nothing written, message prefixed "pt_lens_warp_planes: "): a null ctx, desc or color, or
 * both outputs null; no pt_resize yet; a plane that fails the pointer checks; any overlap that involves out or frame_rgba8 (out may NOT be
 * color: the gather reads neighbours); an unknown flag bit; a non-finite border; per view: any non-finite field, inv_radius < 0, |center|
 * or |k| above 1e6, or reserved != 0.
 * Ordering and state, as pt_dof_planes: the call waits for the frames in flight, runs on pt_stream(ctx) under the STREAM CONTRACT, is
 * complete when it returns, and writes no context state.
 *
 * pt_warp_matrix is a host function: no context, no GPU.  Cameras are eye, U, V, W as pt_set_camera takes them; the eyes are ignored, so
 * the reprojection is rotational.  src_cam is the camera the frame was rendered with, dst_cam the camera at scan-out.  In float64, with P
 * the matrix that maps (nx, ny) in [-1, 1]^2 to pixels (px = (nx + 1) * width / 2, likewise y):
 *     H = P * [U V W]_src^-1 * [U' V' W']_dst * P^-1,
 * each entry rounded to float32 once.  No rescaling and no sign change, because step 5 tests c > 0.  If the words of U, V, W of the two
 * cameras are equal word for word the result is the identity exactly (checked first).  PT_ERR_INVALID (text in pt_last_error(NULL)) for
 * null pointers, zero sizes, non-finite input, a source matrix whose |det| is below 1e-12 times the product of its column norms, or an
 * entry that does not fit float32.
 * Not part of this interface: positional reprojection with the depth plane; tangential (decentring) terms and mesh-based warps; the exact
 * inverse of a camera-calibration model (a dataset user fits output -> source coefficients); vignette compensation; a fusion into
 * pt_tonemap_planes's kernel; an asynchronous variant; a pt_multi_* wrapper (per-rank calls work once the colour is gathered). */
typedef enum pt_lens_warp_flags { PT_LENS_WARP_BICUBIC = 1 } pt_lens_warp_flags;
typedef struct pt_lens_view {       /* 96 bytes, HOST */
    float center[2];     /* lens centre in the view's own pixel coordinates (pixel centres at +0.5) */
    float inv_radius[2]; /* 1 / (the pixel distance at which r = 1), per axis; >= 0 */
    float k[3][3];       /* k[channel][0..2] = k1, k2, k3 for r, g, b */
    float warp[9];       /* row-major 3x3 in the view's pixel coordinates: output pixel -> source pixel */
    float reserved[2];   /* 0 */
} pt_lens_view;
typedef struct pt_lens_warp_desc {
    const float* color;        /* w*h x 4 (.w ignored); required */
    float*       out;          /* w*h x 4 or NULL; exclusive (it may NOT be color: the gather reads neighbours) */
    uint32_t*    frame_rgba8;  /* w*h or NULL; exclusive; at least one of out, frame_rgba8 */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    const pt_lens_view* lenses;/* HOST, nv entries, or NULL: k = 0 and warp = identity for every view */
    float    border[3];        /* finite: the colour of a channel whose source point is outside */
    uint32_t flags;            /* pt_lens_warp_flags */
} pt_lens_warp_desc;
typedef struct pt_lens_warp_stats { uint64_t pixels, outside, nonfinite; double kernel_ms; } pt_lens_warp_stats;
int pt_lens_warp_planes(pt_ctx* ctx, const pt_lens_warp_desc* desc, pt_lens_warp_stats* stats /* may be NULL */);
/* host only: out = the warp of a frame rendered under src_cam and shown under dst_cam (12 floats each: eye, U, V, W) */
int pt_warp_matrix(const float src_cam[12], const float dst_cam[12], uint32_t width, uint32_t height, float out[9]);

/* AMBIENT OCCLUSION FROM THE G-BUFFER (no reference counterpart).  Every other pass of the chain is an image filter; this one asks the
 * acceleration structure a new question.  Per pixel of a hit it shoots `rays` short any-hit rays over the cosine-weighted hemisphere around
 * the geometric normal, through the context's CURRENT tree (it follows pt_update_meshes* and pt_transform_meshes), and writes the open
 * fraction.  It is what a caller could build from pt_trace_device(PT_QUERY_ANY) — occ_k below is by definition that call's answer — without
 * 32 bytes a ray in and 4 out through the caller's memory, a second staging, a validation kernel over rays the library built itself, an
 * attribute kernel, and an unbounded ray buffer: the rays are built in registers from the hit plane, traced in bounded batches and reduced
 * per pixel.  In the upsampled loop (examples/upsampled_svgf_loop.py --ao) the full-size context computes it, so contact shadows smaller than
 * a low-resolution pixel reach the display; a dataset user gets an occlusion AOV.  Stateless like every pass here: the planes and the scratch
 * are caller-owned DEVICE memory of the context's device (the planes 4-byte aligned, frame-sized, indexed Y * width + X; the scratch 16-byte
 * aligned); block_mask is HOST memory.
 *
 * The pixel set is pt_edge_aa_planes's: the pixels a pt_render_mask with the same mask would render — the rank's owned pixels, view pixels
 * only while views are set, whole blocks of block_mask.  The pass reads hit and position of this frame's pt_render_gbuffer, the cameras of the
 * context (for the eye of the pixel's view) and the current tree.  It reads no vertices: the normal is pt_hit.ng, and no address is formed
 * from prim, which is looked at for its sign only (a stale prim >= the triangle count is processed like any other hit).
 *
 * Rule.  Float32 throughout, one rounding per operation, no fused multiply-add, sqrtf and / correctly rounded (pt_detmath.h's contract), with
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, normalize3(v) = v * (1 / sqrt(dot3(v, v))) as in pt_render_gbuffer's text, sel_max0(v) = v > 0
 * ? v : 0 as in pt_filter_planes's, and "finite" the exponent-bit test (exponent bits not all ones).  Per pixel p of the set, with LOCAL
 * coordinates (x, y) in its rectangle and E the eye of p's camera (the frame's, or with views the one of p's view):
 *   1. h = hit[p].  If h.prim < 0 (a miss): ao = 1.0f, out = (1, 1, 1, 1), bent = (0, 0, 0, 1); stats->skipped counts it; it shoots no ray.
 *   2. P = position[p].xyz, n0 = h.ng, t = h.t.  If one of those seven words is not finite, or t > 0 is false: the same outputs as a miss;
 *      stats->nonfinite counts it; it shoots no ray.
 *   3. Face the viewer: s = dot3(n0, E - P); n = (s < 0) ? -n0 : n0.
 *   4. The frame, branch-free but for the sign, no transcendental:
 *        sg = (n.z >= 0) ? 1.0f : -1.0f;  a = -1.0f / (sg + n.z);  b = (n.x * n.y) * a;
 *        T = (1.0f + (sg * (n.x * n.x)) * a,  sg * b,  (-sg) * n.x);   B = (b,  sg + (n.y * n.y) * a,  -n.y).
 *   5. The origin: O = P + n * (bias * t) per component, the product first and then the sum.
 *   6. For sample k = 0 .. rays - 1, a cosine-weighted direction from depth of field's spiral (no table and no constant of its own):
 *        rho_k = sqrtf(((float)k + 0.5f) / (float)rays);  Dk = D[(k + k0) & 127], D being pt_dof_planes's recurrence; k0 = 0 without
 *        PT_AO_JITTER, with it k0 = h & 63 where h is pt_dof_planes's hash of the LOCAL coordinates (x, y) and seed;
 *        a_k = rho_k * Dk.x;  b_k = rho_k * Dk.y;  c_k = sqrtf(sel_max0(1.0f - (a_k*a_k + b_k*b_k)));
 *        w = ((T * a_k) + (B * b_k)) + (n * c_k) per component;  d_k = normalize3(w).
 *      The ray is (O, tmin = 0.0f, d_k, tmax = radius), in pt_trace_device's eight words.
 *   7. The ray is tested with pt_trace_device's validity rule: the eight words finite, dot3(d_k, d_k) and 1.0f / dot3(d_k, d_k) finite and not
 *      zero.  An invalid ray is not traced; it counts as unoccluded, and stats->invalid counts it.
 *   8. occ_k is exactly what pt_trace_device(PT_QUERY_ANY) returns for that ray over the current geometry (1 occluded, 0 not).  Back faces
 *      count.
 *   9. open = the number of rays with occ_k == 0 (the invalid ones included);  ao = (float)open / (float)rays;
 *      bent.xyz = S / (float)rays per component, where S starts at +0 and adds d_k per component, for k ascending, over the unoccluded VALID
 *      rays only (the mean unoccluded direction, not normalised);  bent.w = ao;  out = (ao, ao, ao, 1.0f).
 * stats->pixels is the size of the set; traced the pixels that passed steps 1 and 2 (pixels = skipped + nonfinite + traced); rays the rays
 * traced (traced * rays - invalid); occluded those with occ_k == 1.
 *
 * Batches and scratch.  The pixel list is cut into batches of floor(M / rays) pixels, M = max_rays_in_flight or, when that is 0,
 * PT_AO_DEFAULT_RAYS_IN_FLIGHT.  For each batch, in stream order, the pass generates the rays, traces them (the traversal kernel and grid
 * of pt_trace_device) and reduces them; stats->batches says how many ran.  The scratch holds ONE batch — a 256-byte head (the traversal's
 * count word, its work counter, the fault word, zeroed by the call), then per ray slot an origin and a direction of 16 bytes and a record of
 * 8, then 8 bytes per batch pixel — and nothing per frame pixel.  pt_ao_layout returns its size for min(floor(M / rays), frame pixels) pixels
 * a batch: 256 + pixels * (40 * rays + 8), rounded up to 16.  The result does not depend on M, bit for bit.
 *
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet; hit, position
 * or scratch NULL; ao, out and bent all NULL; a plane that fails the pointer checks; a written plane or the scratch overlapping anything;
 * a scratch that is not 16-byte aligned or smaller than the layout; rays outside 1 .. PT_AO_MAX_RAYS; max_rays_in_flight non-zero and below
 * rays; radius not finite or not > 0; bias negative or not finite; an unknown flag bit.  The traversal's stack-overflow bit gives
 * PT_ERR_UNSUPPORTED, as in pt_trace.
 * Ordering and state, as pt_render_gbuffer: the call waits for the frames in flight and completes queued queries (their counts stay for
 * pt_query_wait), runs on pt_stream(ctx) under the STREAM CONTRACT, is complete when it returns, and touches neither the context's query
 * state, nor the frame buffers, nor pt_stats.  For zero pixels it launches nothing and returns PT_OK.
 * Not part of this interface: distance-weighted occlusion; a shading normal; reflections or shadows towards the probe; an asynchronous
 * variant; a pt_multi_* wrapper (per-rank calls work: each rank traces the whole tree for its own pixels). */
#define PT_AO_MAX_RAYS 32
#define PT_AO_DEFAULT_RAYS_IN_FLIGHT 8388608u /* 2^23 rays: 336 MB of ray slots and 8 bytes a batch pixel, or the frame's if that is less */
typedef enum pt_ao_flags { PT_AO_JITTER = 1 } pt_ao_flags;
typedef struct pt_ao_desc {
    const void*  hit;          /* w*h x pt_hit, required */
    const float* position;     /* w*h x 4, required */
    float* ao;                 /* w*h      or NULL, exclusive */
    float* out;                /* w*h x 4  or NULL, exclusive: (ao, ao, ao, 1.0f) — what pt_modulate_planes / the filters take as a colour */
    float* bent;               /* w*h x 4  or NULL, exclusive: mean unoccluded direction (not normalised), .w = ao */
    void*  scratch;            /* pt_ao_layout's bytes, 16-byte aligned, required, exclusive */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    uint32_t rays;             /* 1 .. PT_AO_MAX_RAYS per pixel */
    uint32_t max_rays_in_flight; /* 0 = PT_AO_DEFAULT_RAYS_IN_FLIGHT; else >= rays: bounds the scratch */
    float radius;              /* finite, > 0: the rays' tmax, world units */
    float bias;                /* finite, >= 0: the origin is lifted by bias * hit.t along the normal */
    uint32_t seed;             /* PT_AO_JITTER: e.g. the frame index */
    uint32_t flags;            /* pt_ao_flags */
} pt_ao_desc;
typedef struct pt_ao_stats { uint64_t pixels, traced, skipped, nonfinite, rays, occluded, invalid, batches; double kernel_ms, trace_ms; } pt_ao_stats;
int pt_ao_layout(const pt_ctx* ctx, uint32_t rays, uint32_t max_rays_in_flight, size_t* bytes);
int pt_ao_planes(pt_ctx* ctx, const pt_ao_desc* desc, pt_ao_stats* stats /* may be NULL */);

/* MIRROR REFLECTIONS FROM THE G-BUFFER (no reference counterpart).  The second pass of the chain that asks the acceleration structure: per
 * pixel of a hit it shoots ONE ray, the mirror image of the eye ray about the geometric normal, through the context's CURRENT tree (it
 * follows pt_update_meshes* and pt_transform_meshes), and writes what that ray sees as a SECOND G-BUFFER: a pt_hit plane, a position plane,
 * the ray itself, and the probe's radiance where the ray escapes.  It is what a caller could build from pt_trace_device(PT_QUERY_CLOSEST) —
 * hit2 below is by definition that call's answer — without 32 bytes a ray through the caller's memory, a second staging, a validation kernel
 * over rays the library built itself, a scatter of linear records back to the frame, and an unbounded ray buffer.  Every pass that reads a
 * hit plane (pt_surface_planes for the reflected surface's albedo, pt_ao_planes, ...) works on hit2 / position2 unchanged
 * (examples/upsampled_svgf_loop.py --reflect).  Stateless like every pass here: the planes and the scratch are caller-owned DEVICE memory of
 * the context's device (the planes 4-byte aligned, frame-sized, indexed Y * width + X; the scratch 16-byte aligned); block_mask is HOST memory.
 *
 * The pixel set is pt_ao_planes's and pt_edge_aa_planes's: the pixels a pt_render_mask with the same mask would render — the rank's owned
 * pixels, view pixels only while views are set, whole blocks of block_mask.  A pixel outside the set is not written in any plane.  The pass
 * reads hit and position of this frame's pt_render_gbuffer, the cameras of the context (for the eye of the pixel's view), the current tree
 * and, for sky, the probe.  No address is formed from hit's prim, which is looked at for its sign only (a stale prim >= the triangle count
 * is processed like any other hit).
 *
 * Rule.  Float32 throughout, one rounding per operation, no fused multiply-add, sqrtf and / correctly rounded (pt_detmath.h's contract), with
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, normalize3(v) = v * (1 / sqrt(dot3(v, v))) as in pt_render_gbuffer's text, and "finite" the
 * exponent-bit test (exponent bits not all ones).  The EMPTY RECORD is hit2 = {t 0, u 0, v 0, prim -1, mesh -1, ng 0}, position2 = (0, 0, 0, 0),
 * sky = (0, 0, 0, 0), ray = the neutral ray (0, 0, 0, 1, 0, 0, 1, -1).  Per pixel p of the set, with E the eye of p's camera (the frame's,
 * or with views the one of p's view):
 *   1. h = hit[p].  If h.prim < 0 (a miss): the empty record; stats->skipped counts it; it shoots no ray.
 *   2. P = position[p].xyz, n0 = h.ng, t = h.t.  If one of those seven words is not finite, or t > 0 is false: the empty record;
 *      stats->nonfinite counts it; it shoots no ray.
 *   3. Face the viewer: s = dot3(n0, E - P); n = (s < 0) ? -n0 : n0.  (pt_ao_planes's step 3.)
 *   4. The mirror direction: d = normalize3(P - E); c = dot3(d, n); k = 2.0f * c;
 *      r = normalize3((d.x - n.x*k, d.y - n.y*k, d.z - n.z*k)).
 *   5. The origin: O = P + n * (bias * t) per component, the product first and then the sum.  The ray is (O, tmin = 0.0f, r, tmax =
 *      max_distance), in pt_trace_device's eight words.
 *   6. The ray is tested with pt_trace_device's validity rule: the eight words finite, dot3(r, r) and 1.0f / dot3(r, r) finite and not zero.
 *      An invalid ray is not traced: hit2 = {t 0, u 0, v 0, prim -2, mesh -1, ng 0}, position2 = 0, sky = 0, ray = its own eight words as
 *      computed; stats->invalid counts it.
 *   7. hit2 is exactly the pt_hit that pt_trace_device(PT_QUERY_CLOSEST) returns for that ray over the current geometry, all eight words:
 *      for a hit t2, the barycentrics u, v, prim, mesh and the geometric normal of the triangle; for an escaped ray t = max_distance,
 *      prim = mesh = -1 and 0 in the rest.  Back faces count.
 *   8. position2 = (O.x + t2*r.x, O.y + t2*r.y, O.z + t2*r.z, 1.0f) for a hit, the product first and then the sum; (0, 0, 0, 0) otherwise.
 *   9. sky: for an escaped valid ray the probe's texel along r, by the frame's miss program (what pt_eval_table 3 returns for r, columns
 *      2..4): (texel.x, texel.y, texel.z, 1.0f); for a hit (0, 0, 0, 0).  sky.w therefore says where the ray escaped.
 * stats->pixels is the size of the set; traced the pixels that passed steps 1 and 2 (pixels = skipped + nonfinite + traced, and traced =
 * invalid + hits + escaped); hits the rays that hit, escaped the valid rays that did not.
 *
 * Batches and scratch.  The pixel list is cut into batches of M pixels, M = max_rays_in_flight or, when that is 0,
 * PT_REFLECT_DEFAULT_RAYS_IN_FLIGHT.  For each batch, in stream order, the pass generates the rays, traces them (the traversal kernel and
 * grid of pt_trace_device) and resolves them; stats->batches says how many ran.  The scratch holds ONE batch — a 256-byte head (the
 * traversal's count word, its work counter, the fault word, zeroed by the call), then per ray slot an origin and a direction of 16 bytes and
 * a record of 8, then 4 bytes per batch pixel — and nothing per frame pixel.  pt_reflect_layout returns its size for min(M, frame pixels)
 * pixels a batch: 256 + pixels * 44, rounded up to 16.  The result does not depend on M, bit for bit.
 *
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): a null ctx or desc; no pt_resize yet; hit, position
 * or scratch NULL; hit2, position2, ray and sky all NULL; a plane that fails the pointer checks; a written plane or the scratch overlapping
 * anything; a scratch that is not 16-byte aligned or smaller than the layout; bias negative or not finite; max_distance not finite or not
 * > 0; an unknown flag bit; sky asked for while the context has no probe ("no probe set (setProbe)": without sky a context without a probe
 * works).  The traversal's stack-overflow bit gives PT_ERR_UNSUPPORTED, as in pt_trace.
 * Ordering and state, as pt_ao_planes: the call waits for the frames in flight and completes queued queries (their counts stay for
 * pt_query_wait), runs on pt_stream(ctx) under the STREAM CONTRACT, is complete when it returns, and touches neither the context's query
 * state, nor the frame buffers, nor pt_stats.  For zero pixels it launches nothing and returns PT_OK.
 * Not part of this interface: a shading or bent normal as input; glossy lobes (several rays a pixel); refraction; lighting of the reflected
 * surface; an asynchronous variant; a pt_multi_* wrapper (per-rank calls work: each rank traces the whole tree for its own pixels). */
#define PT_REFLECT_DEFAULT_RAYS_IN_FLIGHT 8388608u /* 2^23 rays: 352 MB of ray slots and pixel words, or the frame's if that is less */
typedef struct pt_reflect_desc {
    const void*  hit;          /* w*h x pt_hit, required */
    const float* position;     /* w*h x 4, required */
    void*  hit2;               /* w*h x pt_hit or NULL, exclusive: what the mirror ray hits */
    float* position2;          /* w*h x 4  or NULL, exclusive: where it hits, .w = 1; zeros where it does not */
    float* ray;                /* w*h x 8  or NULL, exclusive: the mirror ray in pt_trace_device's layout */
    float* sky;                /* w*h x 4  or NULL, exclusive: the probe's radiance where the ray escapes, .w = 1; zeros elsewhere.  Needs a probe */
    void*  scratch;            /* pt_reflect_layout's bytes, 16-byte aligned, required, exclusive */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    float bias;                /* finite, >= 0: the origin is lifted by bias * hit.t along the normal */
    float max_distance;        /* finite, > 0: the ray's tmax, world units (1e16f is the G-buffer's) */
    uint32_t max_rays_in_flight; /* 0 = PT_REFLECT_DEFAULT_RAYS_IN_FLIGHT: bounds the scratch */
    uint32_t flags;            /* must be 0 */
} pt_reflect_desc;
typedef struct pt_reflect_stats { uint64_t pixels, traced, skipped, nonfinite, invalid, hits, escaped, batches; double kernel_ms, trace_ms; } pt_reflect_stats;
int pt_reflect_layout(const pt_ctx* ctx, uint32_t max_rays_in_flight, size_t* bytes);
int pt_reflect_planes(pt_ctx* ctx, const pt_reflect_desc* desc, pt_reflect_stats* stats /* may be NULL */);

/* SUN SHADOWS AND DIRECT LIGHT FROM THE G-BUFFER (no reference counterpart).  The third pass of the chain that asks the acceleration
 * structure, and the most common question: does this surface point see the light?  The caller names up to PT_SHADOW_MAX_LIGHTS distant
 * disc lights — a direction, an angular size, a radiance: a sun, a moon, a key light — and per pixel of a hit the pass shoots rays_i any-hit
 * rays towards each light that stands above the pixel's horizon, through the context's CURRENT tree (it follows pt_update_meshes* and
 * pt_transform_meshes), and writes the open fraction per light (visibility) and the lights' sum (light), which pt_modulate_planes multiplies
 * by an albedo.  It works on any hit plane: renderGBuffer's, or pt_reflect_planes's hit2 / position2 with view_ray = its ray plane, which
 * lights the mirrored surface (examples/upsampled_svgf_loop.py --sun, --sun --reflect).  The rule holds no random numbers, no CDF search
 * and no transcendental: it is built from dot3, normalize3, pt_ao_planes's frame, pt_dof_planes's spiral and hash, and the any-hit query.
 * Stateless like every pass here: the planes and the scratch are caller-owned DEVICE memory of the context's device (the planes 4-byte
 * aligned, frame-sized, indexed Y * width + X; the scratch 16-byte aligned); block_mask and lights are HOST memory.
 *
 * The pixel set is pt_ao_planes's: the rank's owned pixels, view pixels only while views are set, whole blocks of block_mask.  A pixel
 * outside the set is not written.  No address is formed from hit's prim, which is looked at for its sign only.
 *
 * Rule.  Float32 throughout, one rounding per operation, no fused multiply-add, sqrtf and / correctly rounded (pt_detmath.h's contract);
 * dot3, normalize3, sel_max0 and "finite" are pt_ao_planes's.  R is the sum of the lights' rays.  (x, y) are the LOCAL coordinates of the
 * pixel in its rectangle.
 * Per light i, the same for every pixel: L_i = normalize3(dir_i); T_i, B_i = the frame of pt_ao_planes's step 4 with L_i in place of n:
 *        sg = (L.z >= 0) ? 1.0f : -1.0f;  a = -1.0f / (sg + L.z);  b = (L.x * L.y) * a;
 *        T = (1.0f + (sg * (L.x * L.x)) * a,  sg * b,  (-sg) * L.x);   B = (b,  sg + (L.y * L.y) * a,  -L.y).
 * Per pixel p of the set:
 *   1. h = hit[p].  If h.prim < 0 (the sign only; a miss): visibility = (1, 1, 1, 1), light = (0, 0, 0, 1); stats->skipped counts it; it
 *      shoots no ray.
 *   2. P = position[p].xyz, ng = h.ng, t = h.t.  If one of those seven words is not finite, or t > 0 is false, or, with view_ray, one of
 *      view_ray[p]'s first three words is not finite: the same outputs as a miss; stats->nonfinite counts it; it shoots no ray.
 *   3. Facing: E = view_ray[p].xyz when view_ray is given, else the eye of p's camera (the frame's, or with views the one of p's view).
 *      n = dot3(ng, E - P) < 0 ? -ng : ng.  The origin: O = P + n * (bias * t) per component, the product first and then the sum.
 *   4. Per light i, ascending: c = dot3(n, L_i).  If c > 0.0f is false the light is under the pixel's horizon: v_i = 0.0f, no ray is shot,
 *      and stats->backfacing counts the pair.  Otherwise c_i = c > 1.0f ? 1.0f : c, and the rays of step 5 are shot.
 *   5. The rays of light i, for k = 0 .. rays_i - 1:
 *        rho = sqrtf(((float)k + 0.5f) / (float)rays_i);  Dk = D[(k + k0) & 127], D being pt_dof_planes's spiral; k0 = 0 without
 *        PT_SHADOW_JITTER, with it k0 = pass_hash(x, y, seed + i) & 63, pt_dof_planes's hash, the addition in uint32_t (it wraps);
 *        a = (rho * Dk.x) * spread_i;  b = (rho * Dk.y) * spread_i;
 *        w = (L_i + T_i * a) + B_i * b per component;  d = normalize3(w).
 *      The ray is (O, tmin = 0.0f, d, tmax = max_distance), in pt_trace_device's eight words, and is tested with pt_trace_device's validity
 *      rule as in pt_ao_planes: an invalid ray is not traced, counts as unoccluded, and stats->invalid counts it.  occ is exactly what
 *      pt_trace_device(PT_QUERY_ANY) returns for that ray over the current geometry.  A sample under the surface's horizon is not
 *      special-cased: the tree decides.
 *   6. v_i = (float)open_i / (float)rays_i, open_i the rays of light i with occ == 0 (the invalid ones included).  Absent lights
 *      (i >= num_lights) have v_i = 1.0f.  visibility = (v_0, v_1, v_2, v_3).
 *   7. light.xyz starts at +0 and adds radiance_i * (c_i * v_i) per component, over i ascending, over the lights of step 5 only;
 *      light.w = 1.0f.  The clamp of step 4 and the finite, non-negative radiances keep light free of NaN for any finite input.
 * stats->pixels is the size of the set; traced the pixels that passed steps 1 and 2 (pixels = skipped + nonfinite + traced); backfacing the
 * (pixel, light) pairs under the horizon; rays the rays traced (the slots of step 5 minus invalid); occluded those with occ == 1.
 *
 * Batches and scratch.  The pixel list is cut into batches of floor(M / R) pixels, M = max_rays_in_flight or, when that is 0,
 * PT_SHADOW_DEFAULT_RAYS_IN_FLIGHT.  For each batch, in stream order, the pass generates the rays, traces them (the traversal kernel and
 * grid of pt_trace_device) and reduces them; stats->batches says how many ran.  The scratch holds ONE batch — a 256-byte head, as in
 * pt_ao_planes, then 40 bytes a ray slot, then 32 bytes a batch pixel (a first slot and a stride per light) — and nothing per frame
 * pixel.  pt_shadow_layout returns its size for min(floor(M / R), width * height) pixels a batch: 256 + pixels * (40 * R + 32), rounded up
 * to 16.  It looks at the lights' rays only.  The result does not depend on M, bit for bit.
 *
 * Refused with PT_ERR_INVALID (text in pt_last_error, nothing enqueued, nothing written): pt_ao_planes's list (a null ctx or desc; no
 * pt_resize yet; hit, position or scratch NULL; a plane that fails the pointer checks; a written plane or the scratch overlapping anything;
 * a scratch that is not 16-byte aligned or smaller than the layout; bias negative or not finite), and: num_lights outside
 * 1 .. PT_SHADOW_MAX_LIGHTS; lights NULL; a light with rays == 0, or R > PT_SHADOW_MAX_RAYS; a non-finite dir, or a dir for which normalize3
 * does not give finite components with dot3(L, L) > 0.5f; spread not finite or outside [0, 1]; a radiance that is not finite or negative;
 * max_distance not finite or not > 0; max_rays_in_flight non-zero and below R; visibility and light both NULL; an unknown flag bit.  The
 * traversal's stack-overflow bit gives PT_ERR_UNSUPPORTED, as in pt_trace.
 * Ordering and state, as pt_ao_planes: the call waits for the frames in flight and completes queued queries (their counts stay for
 * pt_query_wait), runs on pt_stream(ctx) under the STREAM CONTRACT, is complete when it returns, and touches neither the context's query
 * state, nor the frame buffers, nor pt_stats.  For zero pixels it launches nothing and returns PT_OK.
 * Not part of this interface: lights sampled from the probe; point or area lights at a finite distance; a shading normal; coloured or
 * partial occluders; an asynchronous variant; a pt_multi_* wrapper (per-rank calls work). */
#define PT_SHADOW_MAX_LIGHTS 4
#define PT_SHADOW_MAX_RAYS 32                 /* the SUM of the lights' rays */
#define PT_SHADOW_DEFAULT_RAYS_IN_FLIGHT 8388608u
typedef struct pt_shadow_light {              /* 32 bytes */
    float dir[3];       /* towards the light, any length the checks above accept */
    float spread;       /* tan of the disc's angular radius, 0 .. 1; 0 = a point at infinity */
    float radiance[3];  /* finite, >= 0 */
    uint32_t rays;      /* >= 1 */
} pt_shadow_light;
typedef enum pt_shadow_flags { PT_SHADOW_JITTER = 1 } pt_shadow_flags;
typedef struct pt_shadow_desc {
    const void*  hit;          /* w*h x pt_hit, required */
    const float* position;     /* w*h x 4, required */
    const float* view_ray;     /* w*h x 8 or NULL: pt_reflect_planes's `ray` plane; its origin replaces the eye in step 3 */
    float* visibility;         /* w*h x 4 or NULL, exclusive: v_0 .. v_3 */
    float* light;              /* w*h x 4 or NULL, exclusive: (sum_i radiance_i * (c_i * v_i), 1) */
    void*  scratch;            /* pt_shadow_layout's bytes, 16-byte aligned, required, exclusive */
    const uint8_t* block_mask; /* HOST, as pt_render_gbuffer, or NULL */
    const pt_shadow_light* lights; /* HOST, num_lights entries */
    uint32_t num_lights;       /* 1 .. PT_SHADOW_MAX_LIGHTS */
    uint32_t max_rays_in_flight; /* 0 = PT_SHADOW_DEFAULT_RAYS_IN_FLIGHT; else >= R: bounds the scratch */
    float max_distance;        /* finite, > 0: the rays' tmax, world units */
    float bias;                /* finite, >= 0: the origin is lifted by bias * hit.t along the normal */
    uint32_t seed;             /* PT_SHADOW_JITTER: e.g. the frame index */
    uint32_t flags;            /* pt_shadow_flags */
} pt_shadow_desc;
typedef struct pt_shadow_stats { uint64_t pixels, traced, skipped, nonfinite, backfacing, rays, occluded, invalid, batches;
                                 double kernel_ms, trace_ms; } pt_shadow_stats;
int pt_shadow_layout(const pt_ctx* ctx, const pt_shadow_light* lights, uint32_t num_lights, uint32_t max_rays_in_flight, size_t* bytes);
int pt_shadow_planes(pt_ctx* ctx, const pt_shadow_desc* desc, pt_shadow_stats* stats /* may be NULL */);

/* The acceleration structure as the traversal kernels see it, copied to host memory — for inspection, for a host-side
 * traversal of the SAME tree (bench.py's CPU baseline, tests) or for serialisation.  Call with nodes == tris == NULL to get the
 * counts.  nodes: num_nodes x 80 bytes, node 0 = root, breadth-first by level (20 little-endian 32-bit words each):
 *   [0..2] origin.xyz (f32) | [3] upper 16 bits of the f32 grid steps sx (low half) and sy (high half) | [4] child_base |
 *   [5] tri_base | [6] leafbits | [7] upper 16 bits of sz (low half), imask (high half) |
 *   [8,9] qlo.x[8] | [10,11] qlo.y[8] | [12,13] qlo.z[8] | [14,15] qhi.x[8] | [16,17] qhi.y[8] | [18,19] qhi.z[8]  (one byte per child slot)
 * child box s = origin + q * step per axis (rounded outward at build; an unused slot has qlo 255 > qhi 0);
 * internal child s = node child_base + popcount(imask & ((1 << s) - 1)); leafbits bit 3s+k: slot s holds more than k
 * triangles, triangle (s,k) = tris[tri_base + popcount(leafbits & ((1 << (3s+k)) - 1))].
 * tris: num_tris x 48 bytes = 12 f32: v0.xyz, v1.xyz, v2.xyz, the global primitive index (i32 bits), the mesh index (i32 bits; = the material
 * record: k_shade reads these very triangles through the leaf index a closest-hit record holds), 1 unused. */
int pt_export_bvh(pt_ctx* ctx, void* nodes, size_t nodes_bytes, void* tris, size_t tris_bytes, uint32_t* num_nodes, uint32_t* num_tris);

/* In-place vertex updates (no reference counterpart: the reference builds its GAS once with OPTIX_BUILD_OPERATION_BUILD,
 * SimplePathtracer.cpp:529; the OptiX analogue is OPTIX_BUILD_FLAG_ALLOW_UPDATE + OPTIX_BUILD_OPERATION_UPDATE).
 * Contract:
 *   - only vertex positions change: index buffers, texcoords, materials and the mesh count stay as created;
 *   - one call updates `n` >= 1 meshes with ONE refit or ONE rebuild and is atomic: on any error (mesh index out of range, a mesh named
 *     twice, num_vertices different from the mesh's, a non-finite coordinate, out of memory, a rebuilt tree deeper than the traversal
 *     stack) the context is exactly as before — vertices, tree and side arrays — and PT_ERR_INVALID / PT_ERR_HIP / PT_ERR_UNSUPPORTED
 *     is returned.  The vertices are validated on the host and staged in a scratch buffer first;
 *   - it waits for the frames in flight (pt_sync) and is complete when it returns (STREAM CONTRACT): frames enqueued before the call see
 *     the old geometry, frames after it the new.  accum_buffer is left alone: restart the accumulation at subframe 0, as after a camera move;
 *   - PT_UPDATE_REFIT keeps the tree's topology and recomputes its boxes on the GPU (leaf triangles, then one launch per level, deepest
 *     first).  Images are those of a fresh pt_create over the new vertices, bit for bit (a hit does not depend on the tree); the traversal
 *     cost grows as the vertices drift from where the tree was built — rebuild when frames get slower.  The calibration cost is kept,
 *     the on-line chain/fused schedule trial starts over;
 *   - PT_UPDATE_REBUILD runs the whole build of pt_create over the new vertices (calibration, stack-depth check, pt_stats.bvh_build_ms)
 *     into a new tree, then swaps it in;
 *   - kernel_ms (may be NULL): device time of the update (hipEvents around its kernels; the host-to-device copy is not included). */
typedef struct pt_mesh_update {
    uint32_t mesh;          /* index into the pt_scene_desc.meshes the context was created from */
    const float* vertex;    /* num_vertices * 3, host memory */
    uint32_t num_vertices;  /* must equal that mesh's num_vertices */
} pt_mesh_update;

enum pt_update_mode { PT_UPDATE_REFIT = 0, PT_UPDATE_REBUILD = 1 };

int pt_update_meshes(pt_ctx* ctx, const pt_mesh_update* updates, uint32_t n, int mode, double* kernel_ms /* may be NULL */);
/* every rank of a pt_multi (all ranks drained first, like pt_multi_resize); validation and staging happen on every rank before any rank
 * changes, so a failure leaves all ranks as they were.  kernel_ms: the slowest rank's */
int pt_multi_update_meshes(pt_multi* m, const pt_mesh_update* updates, uint32_t n, int mode, double* kernel_ms /* may be NULL: the slowest rank */);

/* Updates fed from GPU memory: the same update, with the staging and the validation on the device.
 * pt_update_meshes_device is pt_update_meshes with pt_mesh_update.vertex a DEVICE pointer on the context's device (a simulation or
 * skinning step that leaves its vertices in GPU memory); pt_transform_meshes gives a 3x4 matrix per mesh instead of vertices (the OptiX
 * analogue is an instance transform).  One kernel stages all named meshes of a call into the scratch vertex array; everything behind that
 * array — refit, rebuild, commit — is pt_update_meshes' code.
 * Same contract as pt_update_meshes, item by item:
 *   - only vertex positions change;
 *   - one call does ONE refit or ONE rebuild and is atomic: on any error the context is exactly as before;
 *   - it waits for the frames in flight and is complete when it returns; accum_buffer is left alone;
 *   - the on-line chain/fused schedule trial starts over;
 *   - kernel_ms (may be NULL) covers the staging kernel as well as the refit or the build.
 * Device pointers:
 *   - the library reads them on pt_stream(ctx), under the STREAM CONTRACT: an array produced on another stream must be complete, or ordered
 *     with pt_wait_event, before the call;
 *   - before any device work each pointer is checked with hipPointerGetAttributes (as pt_render_device checks its buffer): a null pointer, a
 *     pointer HIP does not know, host memory (pinned or managed included), memory of another device, a pointer that is not 4-byte aligned, or
 *     an array that does not fit into what is left of its allocation returns PT_ERR_INVALID.  No wider alignment than 4 bytes is assumed.
 * Validation on the device:
 *   - the staging kernel tests the exponent bits of every coordinate it writes (no compiler mode can remove the test) and records the lowest
 *     position in the call of a mesh with a non-finite coordinate; the host reads that word at the synchronisation the staging makes anyway
 *     (PT_UPDATE_REBUILD waits once more, before the build: the builder never sees a non-finite vertex);
 *   - on a bad mesh the call returns PT_ERR_INVALID, pt_last_error names the mesh index, and nothing of the context has changed.
 * Transform arithmetic:
 *   - float32, one rounding per operation, no fused multiply-add, in exactly this order:
 *       x' = ((m[0]*x + m[1]*y) + m[2]*z) + m[3],  y' likewise with m[4..7],  z' with m[8..11];
 *     float32 NumPy evaluating that expression reproduces the vertices bit for bit.  The identity matrix therefore maps -0.0f to +0.0f;
 *   - a matrix entry that is not finite is refused on the host, a result that is not finite (an overflow) by the device check.
 * Rest positions:
 *   - a mesh's rest positions are the ones last given explicitly: by pt_create, pt_update_meshes or pt_update_meshes_device;
 *   - the first pt_transform_meshes of a context (either source) allocates the rest array as a copy of the current vertices: 12 bytes per
 *     vertex, only for contexts that use transforms; if that allocation fails the call returns PT_ERR_HIP and nothing has changed.  From then
 *     on explicit updates write both arrays at commit;
 *   - PT_FROM_REST transforms the rest positions (repeated calls do not drift), PT_FROM_CURRENT what is there now; meshes not named in a
 *     call keep their current positions;
 *   - pt_download_vertices(rest = 1) before any transform returns the current positions.
 * PT_ERR_INVALID also for: null arguments, n == 0, a mesh out of range, a mesh named twice, a wrong num_vertices, an unknown source or mode. */
int pt_update_meshes_device(pt_ctx* ctx, const pt_mesh_update* updates /* .vertex: device memory */, uint32_t n, int mode, double* kernel_ms /* may be NULL */);

typedef struct pt_mesh_transform {
    uint32_t mesh; /* index into the pt_scene_desc.meshes the context was created from */
    float m[12];   /* row-major 3x4; p' = M[:, :3] p + M[:, 3] */
} pt_mesh_transform;

enum pt_transform_source { PT_FROM_REST = 0, PT_FROM_CURRENT = 1 };

int pt_transform_meshes(pt_ctx* ctx, const pt_mesh_transform* t, uint32_t n, int source, int mode, double* kernel_ms /* may be NULL */);
/* the transforms are host data and go to every rank; every rank stages before any rank commits, like pt_multi_update_meshes.  (There is no
 * multi-rank variant of the device-pointer call: the pointer lives on one device; with one process per GPU call the rank's own context.) */
int pt_multi_transform_meshes(pt_multi* m, const pt_mesh_transform* t, uint32_t n, int source, int mode, double* kernel_ms /* may be NULL: the slowest rank */);

/* current (rest = 0) or rest (rest = 1) positions of one mesh, to host memory.  bytes must equal num_vertices * 12. */
int pt_download_vertices(pt_ctx* ctx, uint32_t mesh, int rest, float* host, size_t bytes);

/* Scene ingestion, host only (no GPU needed): loadOBJ (HelloPathtracing_original/Model.cpp:137-212 — tinyobjloader 2.0.0's LoadObj with
 * triangulation, then one TriangleMesh per (shape, material id)) as native code.  The arrays are the reference's bit for bit
 * (tests/test_objloader.py: the reference's own Model.cpp, compiled from where it lies, on committed fixtures and random files):
 * vertices, normals (null when the mesh has none), texcoords (null when none), indices, the Material bytes (Kd -> color, Ke ->
 * emission, defaults otherwise), mesh order.
 * per_mesh_vertex_map = 0 reproduces the reference's ONE knownVertices map per shape shared by its materials (Model.cpp:176): a
 * second material's mesh then indexes vertices it does not own — out of bounds for the renderer (pt_create refuses such a mesh);
 * per_mesh_vertex_map = 1 gives every mesh its own map: what a renderer needs, and the default of the Python facade's
 * load_obj.  Images are not decoded here (the reference uses stb_image): texture_ref numbers a mesh's texture REFERENCE
 * — (shape, file name) pairs in loadTexture's order of first use (Model.cpp:88-135, :177), path = model directory + "/" + name with
 * '\\' -> '/' — or is -1; the caller decodes pt_obj_texture_path(i) (RGBA8, rows mirrored in y), gives unreadable files the id -1
 * and numbers the others in order, as loadTexture does.  Errors: PT_ERR_INVALID, text in pt_obj_last_error() (thread-local). */
typedef struct pt_obj pt_obj;
typedef struct pt_obj_mesh {
    const float* vertex;   /* num_vertices * 3 */
    const float* normal;   /* num_vertices * 3 or NULL */
    const float* texcoord; /* num_vertices * 2 or NULL */
    const uint32_t* index; /* num_triangles * 3 */
    uint32_t num_vertices, num_triangles;
    pt_material material;
    int32_t texture_ref; /* index for pt_obj_texture_path, or -1 */
} pt_obj_mesh;
int pt_load_obj(const char* obj_path, int per_mesh_vertex_map, pt_obj** out);
void pt_obj_free(pt_obj* obj);
uint32_t pt_obj_num_meshes(const pt_obj* obj);
int pt_obj_get_mesh(const pt_obj* obj, uint32_t i, pt_obj_mesh* out); /* the pointers live until pt_obj_free */
uint32_t pt_obj_num_textures(const pt_obj* obj);
const char* pt_obj_texture_path(const pt_obj* obj, uint32_t i);
const char* pt_obj_last_error(void);

/* Device-function tables for function-level parity tests (the reference's commented-out BSDFTest /
 * ProbeCreateTest, Disney.cuh:430-503, Probe.cuh:207-269, turned into entry points).
 *  which = 0: BSDFEval+BSDFPdf  in: n x {N[3],V[3],L[3],etaI,etaO} (11 floats)  out: n x {f[3],pdf}
 *  which = 1: BasisFromVector+BSDFSample  in: n x {N[3],V[3],etaI,etaO,seed(as u32 bits)} (9)  out: n x {L[3],pdf,seed1,seed2 (bits)}
 *  which = 2: ProbeSample  in: n x {seed bits} (1)  out: n x {dir[3],color[3],pdf,seed1,seed2} (9)
 *  which = 3: ProbeEval(ProbeDirToUV(dir)) in: n x dir[3] out: n x {u,v,r,g,b,a} (6)
 *  which = 4: make_color in: n x rgb[3] out: n x {packed bits} (1)
 *  which = 5: detmath in: n x {fn, x, y} (3) out: n x 1   fn: 0 sin 1 cos 2 acos 3 atan2(x,y) 4 log 5 pow(x,y) 6 x/y 7 sqrt(x)
 *  which = 6: tea4/lcg/Random in: n x {a bits, b bits} out: n x {tea4(a,b), lcg state, rnd, Randf bits...} (8)
 *  which = 7: tex2D of scene texture 0 in: n x {s,t} (2) out: n x rgba (4)
 *  which = 8: ProbePdf (Probe.cuh:69-93; unused by the reference's device code) in: n x dir[3] out: n x pdf (1)
 *  which = 9, 10, 11: ProbeSample's row and column search at chosen random numbers  in: n x {r1,r2} (2), each in [0,1)
 *      out: n x {row, lo, hi, column (int32 bits), r, g, b, pdfX of texel (row, column), pdfY[row]} (9); lo, hi = the guide's line counts for
 *      r2's cell, before the clamp to the row's last line.  9 searches the marginal arrays in global memory; 10 and 11 search the copy a
 *      shade workgroup holds in LDS (PT_SHADE_WG threads; 10 the full layout, 11 the lean one, whatever PT_SHADE_LDS says), or the global
 *      arrays where pt_stats.marg_lds_words_full / _lean is 0
 * material applies to which 0,1; the context's probe to 2,3,8-11. All arrays are host memory. */
int pt_eval_table(pt_ctx* ctx, int which, const pt_material* material, int bsdf_mode, const float* in, uint32_t n,
                  float* out);

const char* pt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PT_AMD_H */
