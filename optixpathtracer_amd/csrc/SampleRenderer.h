// SampleRenderer.h — header-only C++ facade with the reference's public surface
// (HelloPathtracing_original/SimplePathtracer.h:38-176, Model.h:10-42, Material.h:11-69, Probe.h:8-88,
// LaunchParams.h:32-38,51-79) over the C ABI of libptamd.so (include/pt_amd.h).  A maintainer of the reference swaps
// SimplePathtracer.{h,cpp} + deviceProgram.cu for this header and links -lptamd; what main.cpp does with the
// renderer (main.cpp:131-144 initLaunchParams, :211-218, :245 output_buffer.setStream(sample.stream), :259, :273
// sample.render(output_buffer), :286) compiles against it as written — tests/test_cabi.py compiles those statements.
// Errors surface as std::runtime_error, like sutil::Exception did.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pt_amd.h"

namespace ptamd {

struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct uint3 { uint32_t x, y, z; };
typedef float4 Color;
// the few sutil/vec_math.h helpers main.cpp's renderer set-up uses (main.cpp:138-143,215)
inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
inline int2 make_int2(int x, int y) { return int2{x, y}; }
inline float3 cross(const float3& a, const float3& b) { return float3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline float3 normalize(const float3& v) { const float inv = 1.0f / std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z); return float3{v.x * inv, v.y * inv, v.z * inv}; }

static const int MATERIAL_FLAG_NONE = 0;
static const int MATERIAL_FLAG_SHADOW_CATCHER = 1 << 0; // Material.h:9

// Material.h:11-69 — same fields, same defaults, layout-compatible with pt_material
struct Material {
    Material() {
        color = {0.6f, 0.6f, 0.6f};
        emission = {0.f, 0.f, 0.f};
        absorption = {0.f, 0.f, 0.f};
        eta = 0.0f; metallic = 0.0f; subsurface = 0.0f; specular = 0.5f; roughness = 1.0f; specularTint = 0.0f;
        anisotropic = 0.0f; sheen = 0.0f; sheenTint = 0.0f; clearcoat = 0.0f; clearcoatGloss = 1.0f; transmission = 0.0f;
        bump = 0.0f; bumpTile = {10.0f, 10.0f, 10.0f};
        flags = 0;
    }
    float GetIndexOfRefraction() const { return eta == 0.0f ? 2.0f / (1.0f - std::sqrt(0.08f * specular)) - 1.0f : eta; }
    float3 emission, color, absorption;
    float eta, metallic, subsurface, specular, roughness, specularTint, anisotropic, sheen, sheenTint, clearcoat, clearcoatGloss, transmission;
    float bump;
    float3 bumpTile;
    int flags;
};
static_assert(sizeof(Material) == sizeof(pt_material), "Material must stay layout-compatible with pt_material");

// Model.h:10-42
struct TriangleMesh {
    std::vector<float3> vertex;
    std::vector<float3> normal;   // carried like the reference; the hot path shades with geometric normals (deviceProgram.cu:490)
    std::vector<float2> texcoord; // uploaded when the mesh has a diffuse texture
    std::vector<uint3> index;
    Material material;
    int diffuseTextureID{-1};
};
struct Texture { // Model.h:21-29
    ~Texture() { delete[] pixel; }
    uint32_t* pixel{nullptr};
    int2 resolution{-1, -1};
};
struct Model {
    ~Model() { for (auto m : meshes) delete m; for (auto t : textures) delete t; }
    std::vector<TriangleMesh*> meshes;
    std::vector<Texture*> textures;
};

// Probe.h:8-88
struct ProbeData {
    int width = 0, height = 0;
    Color* data = nullptr;
    float3 offset{0, 0, 0};
    bool valid = false;
    std::vector<float> pdfValuesX, cdfValuesX, pdfValuesY, cdfValuesY;
    void BuildCDF() { // Probe.h:29-77, native host implementation in libptamd
        pdfValuesX.resize((size_t)width * height); cdfValuesX.resize((size_t)width * height);
        pdfValuesY.resize(height); cdfValuesY.resize(height);
        if (pt_build_cdf(&data[0].x, width, height, pdfValuesX.data(), cdfValuesX.data(), pdfValuesY.data(), cdfValuesY.data()) != PT_OK)
            throw std::runtime_error("BuildCDF failed");
        valid = true;
    }
};

// sutil::Camera subset the renderer reads (sutil/Camera.h)
struct Camera {
    float3 eye{0, 0, 0}, lookat{0, 0, 1}, up{0, 1, 0};
    float fovY = 35.f, aspectRatio = 1.f;
    void UVWFrame(float3& U, float3& V, float3& W) const { pt_uvw_frame(&eye.x, &lookat.x, &up.x, fovY, aspectRatio, &U.x, &V.x, &W.x); }
};

// Beyond the reference: one rectangle of the frame with a camera of its own (pt_view, include/pt_amd.h "VIEWPORTS"); x and y are
// multiples of 8, and the camera's aspectRatio is the view's own width / height
struct View {
    int x = 0, y = 0, width = 0, height = 0;
    Camera camera;
};
inline std::vector<pt_view> toViews(const std::vector<View>& views) {
    std::vector<pt_view> out(views.size());
    for (size_t i = 0; i < views.size(); ++i) {
        const View& v = views[i];
        float3 U, V, W;
        v.camera.UVWFrame(U, V, W);
        out[i] = pt_view{v.x, v.y, v.width, v.height, {v.camera.eye.x, v.camera.eye.y, v.camera.eye.z}, {U.x, U.y, U.z}, {V.x, V.y, V.z}, {W.x, W.y, W.z}};
    }
    return out;
}

// LaunchParams.h:32-38 — set by initLaunchParams (main.cpp:138-143), never read by the device code
struct ParallelogramLight {
    float3 corner{0, 0, 0};
    float3 v1{0, 0, 0}, v2{0, 0, 0};
    float3 normal{0, 0, 0};
    float3 emission{0, 0, 0};
};

// the host-visible part of LaunchParams (LaunchParams.h:51-79; main.cpp:131-144,259,286): the device pointers, the traversable and the
// probe of the reference's struct live inside the context
struct LaunchParams {
    struct { int2 size{0, 0}; unsigned int subframe_index = 0; } frame;
    struct { float3 eye{0, 0, 0}, U{0, 0, 0}, V{0, 0, 0}, W{0, 0, 0}; } camera; // written by setCamera (SimplePathtracer.cpp:155-162)
    unsigned int samples_per_launch = 1;
    ParallelogramLight light; // dead in the reference too
};

typedef void* stream_t; // hipStream_t, kept opaque so that the application side needs no HIP header

class SampleRenderer {
  public:
    explicit SampleRenderer(const Model* model, int device = 0) {
        std::vector<pt_mesh_desc> md(model->meshes.size());
        for (size_t i = 0; i < md.size(); ++i) {
            const TriangleMesh* m = model->meshes[i];
            md[i].vertex = &m->vertex[0].x; md[i].num_vertices = (uint32_t)m->vertex.size();
            md[i].index = &m->index[0].x; md[i].num_triangles = (uint32_t)m->index.size();
            static_assert(sizeof(pt_material) == 104, "");
            md[i].material = *reinterpret_cast<const pt_material*>(&m->material);
            md[i].diffuse_texture_id = m->diffuseTextureID;
            md[i].texcoord = m->texcoord.size() == m->vertex.size() && !m->texcoord.empty() ? &m->texcoord[0].x : nullptr;
        }
        std::vector<pt_texture_desc> td(model->textures.size());
        for (size_t i = 0; i < td.size(); ++i) td[i] = pt_texture_desc{model->textures[i]->pixel, model->textures[i]->resolution.x, model->textures[i]->resolution.y};
        pt_scene_desc sd{md.data(), (uint32_t)md.size(), td.data(), (uint32_t)td.size()};
        if (pt_create(&sd, device, &ctx) != PT_OK) throw std::runtime_error(std::string("SampleRenderer: ") + pt_last_error(nullptr));
        stream = pt_stream(ctx);
    }
    ~SampleRenderer() { pt_destroy(ctx); }
    SampleRenderer(const SampleRenderer&) = delete;
    SampleRenderer& operator=(const SampleRenderer&) = delete;

    void render() { ck(pt_render(ctx, launchParams.samples_per_launch, launchParams.frame.subframe_index, nullptr)); }
    // render(sutil::CUDAOutputBuffer<uint32_t>&) (SimplePathtracer.cpp:99-107): `renderTarget.map()` yields the caller's DEVICE buffer, the
    // rgba8 frame is written there, `unmap()`.  Any type with map() -> uint32_t* (device) and unmap() fits, sutil's buffer included.
    template <class OutputBuffer> void render(OutputBuffer& renderTarget) {
        uint32_t* d_pixels = renderTarget.map();
        const int rc = pt_render_device(ctx, launchParams.samples_per_launch, launchParams.frame.subframe_index, d_pixels);
        renderTarget.unmap();
        ck(rc);
    }
    // the same with the mapped DEVICE pointer itself (pt_render_device refuses plain host memory with PT_ERR_INVALID)
    void renderToDevice(uint32_t* d_pixels) { ck(pt_render_device(ctx, launchParams.samples_per_launch, launchParams.frame.subframe_index, d_pixels)); }
    // No render(uint32_t*): rounds 1-3 had one that took HOST memory, round 4 one that took DEVICE memory under the same signature; a caller
    // written against either must not compile silently against the other — say renderToDevice(d_pixels) or renderToHost(h_pixels).
    void render(uint32_t*) = delete;
    // render() + downloadPixels() in one call: the frame in HOST memory
    void renderToHost(uint32_t* h_pixels) { ck(pt_render(ctx, launchParams.samples_per_launch, launchParams.frame.subframe_index, h_pixels)); }
    // `count` iterations of the application's progressive loop (render(); launchParams.frame.subframe_index++ — main.cpp:273-278) as one
    // wavefront batch: the same buffers bit for bit, count times the rays per launch (pt_render_batch).  Advances subframe_index by count.
    void renderBatch(uint32_t count, uint32_t* h_pixels = nullptr) {
        ck(pt_render_batch(ctx, launchParams.samples_per_launch, launchParams.frame.subframe_index, count, h_pixels));
        launchParams.frame.subframe_index += count;
    }
    void resize(const int2& newSize) {
        ck(pt_resize(ctx, newSize.x, newSize.y));
        if (newSize.x && newSize.y) launchParams.frame.size = newSize;
    }
    void downloadPixels(uint32_t h_pixels[]) {
        ck(pt_download(ctx, PT_BUF_FRAME, h_pixels, sizeof(uint32_t) * (size_t)launchParams.frame.size.x * launchParams.frame.size.y));
    }
    void setCamera(const Camera& camera) {
        float3 U, V, W;
        camera.UVWFrame(U, V, W);
        launchParams.camera.eye = camera.eye; launchParams.camera.U = U; launchParams.camera.V = V; launchParams.camera.W = W;
        ck(pt_set_camera(ctx, &camera.eye.x, &U.x, &V.x, &W.x));
    }
    // Beyond the reference: several cameras in rectangles of this one frame (pt_set_views): a stereo pair, a camera array.  Every render call
    // then fills each rectangle as a frame of its size with its camera would be filled; pixels in no view are left alone; an empty vector
    // returns to setCamera's camera.  setViewCameras moves the cameras of the current views (the per-frame call).
    void setViews(const std::vector<View>& views) {
        const std::vector<pt_view> v = toViews(views);
        ck(pt_set_views(ctx, v.data(), (uint32_t)v.size()));
    }
    void setViewCameras(const std::vector<Camera>& cameras) {
        std::vector<float> rows;
        for (const Camera& c : cameras) {
            float3 U, V, W;
            c.UVWFrame(U, V, W);
            for (const float3& f : {c.eye, U, V, W}) rows.insert(rows.end(), {f.x, f.y, f.z});
        }
        ck(pt_set_view_cameras(ctx, rows.data(), (uint32_t)cameras.size()));
    }
    void setProbe(const ProbeData& probe) {
        if (!probe.valid) throw std::runtime_error("Probe Data is not valid"); // Probe.h:104-105
        ck(pt_set_probe(ctx, &probe.data[0].x, probe.pdfValuesX.data(), probe.cdfValuesX.data(), probe.pdfValuesY.data(), probe.cdfValuesY.data(), probe.width, probe.height));
    }
    // The pass the reference leaves disabled in render(target): "denoiser.exec(); computeFinalPixelColors(size, denoisedBuffer, result)"
    // (SimplePathtracer.cpp:104-105).  Call after render(); h_pixels may be null.
    void denoiseAndTonemap(uint32_t h_pixels[], int iterations = 5, float sigma_color = 1.0f, float sigma_normal = 0.25f, float sigma_albedo = 0.1f) {
        pt_denoise_params p{iterations, sigma_color, sigma_normal, sigma_albedo, PT_BUF_COLOR, 1};
        ck(pt_denoise(ctx, &p, h_pixels, nullptr));
    }
    // Beyond the reference: render() normally returns when its frame is complete (SimplePathtracer.cpp:96); with 2 or 3 frames in flight
    // (pt_options.frames_in_flight) it returns while its own frame is still running, so a progressive loop overlaps consecutive frames.
    // downloadPixels / renderToHost(h_pixels) / renderToDevice(d_pixels) / resize / sync() wait for the frames in flight; the images are the same bit for bit.
    void setFramesInFlight(int n) {
        pt_options o;
        ck(pt_get_options(ctx, &o));
        o.frames_in_flight = n;
        ck(pt_set_options(ctx, &o));
    }
    void sync() { ck(pt_sync(ctx)); }
    // Beyond the reference: render() for chosen 8x8 blocks only (pt_render_mask; one byte per block, (size.x + 7) / 8 per row, non-zero =
    // render).  Those pixels end up as render() leaves them, the others are untouched.  Returns the number of pixels rendered.
    uint32_t renderMask(const std::vector<uint8_t>& block_mask, uint32_t* h_pixels = nullptr) {
        const size_t need = (size_t)((launchParams.frame.size.x + 7) / 8) * (size_t)((launchParams.frame.size.y + 7) / 8);
        if (block_mask.size() != need) throw std::runtime_error("renderMask: the mask needs one byte per 8x8 block");
        uint32_t active = 0;
        ck(pt_render_mask(ctx, launchParams.samples_per_launch, launchParams.frame.subframe_index, block_mask.data(), h_pixels, &active));
        return active;
    }
    // ... and the progressive loop that stops rendering a block once it has converged (pt_adaptive_begin / pt_render_adaptive): call
    // adaptiveBegin after a camera move, where the accumulation restarts at subframe 0, then renderAdaptive() + subframe_index++ until
    // active_blocks is 0.
    void adaptiveBegin(const pt_adaptive_params& params) { ck(pt_adaptive_begin(ctx, &params)); }
    pt_adaptive_stats renderAdaptive(uint32_t* h_pixels = nullptr) {
        pt_adaptive_stats st{};
        ck(pt_render_adaptive(ctx, launchParams.samples_per_launch, launchParams.frame.subframe_index, h_pixels, &st));
        return st;
    }
    void adaptiveEnd() { ck(pt_adaptive_end(ctx)); }
    // Moved vertices (no reference counterpart; OptiX: OPTIX_BUILD_OPERATION_UPDATE): after changing model->meshes[m]->vertex in place for
    // every m in `meshes` (same vertex count, same indices), the context takes the new positions — the tree refitted on the GPU, or rebuilt
    // with rebuild = true (pt_update_meshes).  Restart the accumulation at subframe 0 afterwards.  Returns the device time in ms.
    double updateMeshes(const Model* model, const std::vector<uint32_t>& meshes, bool rebuild = false) {
        double ms = 0;
        const std::vector<pt_mesh_update> u = mesh_updates(model, meshes);
        ck(pt_update_meshes(ctx, u.data(), (uint32_t)u.size(), rebuild ? PT_UPDATE_REBUILD : PT_UPDATE_REFIT, &ms));
        return ms;
    }
    // ... with the new positions in DEVICE memory (pt_update_meshes_device): `updates` name a mesh, a device pointer on the context's device to
    // num_vertices * 3 floats (4-byte aligned) and that count; the arrays must be complete, or ordered with pt_wait_event.  The vertices are
    // validated on the GPU; Model is not touched.
    double updateMeshesDevice(const std::vector<pt_mesh_update>& updates, bool rebuild = false) {
        double ms = 0;
        ck(pt_update_meshes_device(ctx, updates.data(), (uint32_t)updates.size(), rebuild ? PT_UPDATE_REBUILD : PT_UPDATE_REFIT, &ms));
        return ms;
    }
    // ... or a 3x4 matrix per mesh (pt_transform_meshes; the OptiX analogue is an instance transform): applied on the GPU to the mesh's rest
    // positions — the ones last given explicitly — or with from_current = true to what is there now.
    double transformMeshes(const std::vector<pt_mesh_transform>& transforms, bool from_current = false, bool rebuild = false) {
        double ms = 0;
        ck(pt_transform_meshes(ctx, transforms.data(), (uint32_t)transforms.size(), from_current ? PT_FROM_CURRENT : PT_FROM_REST,
                               rebuild ? PT_UPDATE_REBUILD : PT_UPDATE_REFIT, &ms));
        return ms;
    }
    // optixTrace from the application's own DEVICE buffers (pt_trace_device): d_rays = n x 8 floats (o.xyz, tmin, d.xyz, tmax), d_out = n x
    // pt_hit (closest hit) or n x int32 (any_hit), both on this context's device, read and written on stream().  wait = false enqueues and
    // returns: the results are complete after queryWait(), or for a consumer that waits on an event recorded on stream().
    pt_query_stats traceDevice(const float* d_rays, uint32_t n, void* d_out, bool any_hit = false, bool wait = true) {
        pt_query_stats s{};
        ck(pt_trace_device(ctx, d_rays, n, (any_hit ? PT_QUERY_ANY : PT_QUERY_CLOSEST) | (wait ? 0u : (uint32_t)PT_QUERY_ASYNC), d_out, wait ? &s : nullptr));
        return s;
    }
    pt_query_stats queryWait() { // waits for the queued queries; the sums over the queries since the last wait
        pt_query_stats s{};
        ck(pt_query_wait(ctx, &s));
        return s;
    }
    // The first hit under every pixel's centre, under the frame's camera or each view's (pt_render_gbuffer): the planes of `d` are DEVICE
    // memory of this context's device, frame-sized, any subset; prev_cameras and block_mask are host memory.  Synchronous; the frame buffers
    // and the accumulation are left alone.  Returns the pixels written, the hits among them and the device time of the pass.
    pt_gbuffer_stats renderGBuffer(const pt_gbuffer_desc& d, pt_gbuffer_stats* stats = nullptr) {
        pt_gbuffer_stats s{};
        ck(pt_render_gbuffer(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // Reproject / accumulate over a moving camera (pt_temporal_accumulate): every plane of `d` is DEVICE memory of this context's device,
    // frame-sized; block_mask is host memory.  Stateless and synchronous; the caller ping-pongs history and length.  Returns the pixels
    // processed, those that kept their history and the device time of the pass.
    pt_temporal_stats temporalAccumulate(const pt_temporal_desc& d, pt_temporal_stats* stats = nullptr) {
        pt_temporal_stats s{};
        ck(pt_temporal_accumulate(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // The chain's filter (pt_filter_planes): a variance-guided a-trous filter over the G-buffer's exact planes, per view and on the pixel set
    // of the mask.  Every plane of `d` is DEVICE memory of this context's device, frame-sized; block_mask is host memory.  Stateless and
    // synchronous.  Returns the pixels processed, the non-inert ones, those whose variance was estimated spatially and the device time.
    pt_filter_stats filterPlanes(const pt_filter_desc& d, pt_filter_stats* stats = nullptr) {
        pt_filter_stats s{};
        ck(pt_filter_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // The context's current world-space vertices, all meshes in mesh order, into DEVICE memory of `bytes` = vertices * 12 bytes
    // (pt_copy_vertices_device): the snapshot motionPlanes needs, taken before the frame's updateMeshes / transformMeshes.  With dev_dst ==
    // nullptr only the count is returned.  Returns the number of vertices.
    uint32_t copyVerticesDevice(float* dev_dst, size_t bytes) {
        uint32_t nv = 0;
        ck(pt_vertex_count(ctx, &nv, nullptr));
        if (dev_dst) ck(pt_copy_vertices_device(ctx, dev_dst, bytes));
        return nv;
    }
    // Object motion for the chain (pt_motion_planes): from this frame's hit plane and the previous frame's vertices, where each pixel's
    // surface point was — motion, prev_point, prev_surface — for temporalAccumulate(hit = prev_surface, position = prev_point).  Stateless
    // and synchronous.  Returns the pixels processed, the hits and the stale primitive indices among them and the device time.
    pt_motion_stats motionPlanes(const pt_motion_desc& d, pt_motion_stats* stats = nullptr) {
        pt_motion_stats s{};
        ck(pt_motion_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // The scene's texcoords per primitive, uv0.xy uv1.xy uv2.xy in global primitive order, into DEVICE memory of `bytes` = triangles * 24
    // bytes (pt_copy_texcoords_device): the prim_texcoords of surfacePlanes; zeros for a scene without a textured mesh.  It depends on the
    // scene only, so a loop takes it once.  With dev_dst == nullptr only the count is returned.  Returns the number of triangles.
    uint32_t copyTexcoordsDevice(float* dev_dst, size_t bytes) {
        uint32_t nt = 0;
        ck(pt_vertex_count(ctx, nullptr, &nt));
        if (dev_dst) ck(pt_copy_texcoords_device(ctx, dev_dst, bytes));
        return nt;
    }
    // The albedo and the texcoord under every pixel's centre, from this frame's hit plane (pt_surface_planes): the material's colour, or the
    // texture lookup at the barycentric texcoord on a textured mesh; valid in every pixel of the call, rendered or not.  Stateless and
    // synchronous.  Returns the pixels processed, the hits, the stale primitive indices and the texture lookups among them and the device time.
    pt_surface_stats surfacePlanes(const pt_surface_desc& d, pt_surface_stats* stats = nullptr) {
        pt_surface_stats s{};
        ck(pt_surface_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // The shape of the texture mip pyramid (pt_texture_mips_layout): the bytes of the whole pyramid (0: no level above 0) and, when `dims`
    // is given, per texture w, h, levels and the index of the first 16-byte texel of its level 1.  It depends on the scene only.
    size_t textureMipsLayout(std::vector<uint32_t>* dims = nullptr) {
        uint32_t n = 0;
        size_t bytes = 0;
        ck(pt_texture_mips_layout(ctx, &n, nullptr, &bytes));
        if (dims) {
            dims->assign((size_t)4 * n, 0u);
            if (n) ck(pt_texture_mips_layout(ctx, nullptr, dims->data(), nullptr));
        }
        return bytes;
    }
    // The mip pyramid of the scene's textures, levels 1 and up, built on the GPU into DEVICE memory of `bytes` = textureMipsLayout()
    // bytes, 16-byte aligned (pt_copy_texture_mips_device): the mips of surfaceLodPlanes.  A loop takes it once.
    void copyTextureMipsDevice(void* dev_dst, size_t bytes) { ck(pt_copy_texture_mips_device(ctx, dev_dst, bytes)); }
    // surfacePlanes with a level of detail (pt_surface_lod_planes): on a textured mesh the albedo is a trilinear lookup in the mip pyramid
    // over the pixel's footprint in texture space; the footprint and the level can be had as planes.  Stateless and synchronous.  Returns
    // the pixels processed, the hits, the stale records, the texture lookups and the minified ones among them and the device time.
    pt_surface_lod_stats surfaceLodPlanes(const pt_surface_lod_desc& d, pt_surface_lod_stats* stats = nullptr) {
        pt_surface_lod_stats s{};
        ck(pt_surface_lod_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // surfaceLodPlanes with up to d.max_aniso lookups along the longer axis of the pixel's footprint (pt_surface_aniso_planes): a texture
    // seen at a grazing angle is no longer blurred across that axis.  Stateless and synchronous.  Returns surfaceLodPlanes's counters, the
    // pixels that took more than one lookup, the sum of the lookups and the device time.
    pt_surface_aniso_stats surfaceAnisoPlanes(const pt_surface_aniso_desc& d, pt_surface_aniso_stats* stats = nullptr) {
        pt_surface_aniso_stats s{};
        ck(pt_surface_aniso_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // Guided upsampling (pt_upsample_planes), on the FULL-size renderer: a low-resolution colour plane (a second renderer's filterPlanes
    // out) brought to this resolution under both G-buffers with the chain's mesh / normal / plane tests.  Stateless and synchronous.
    // Returns the pixels processed, the hits, and how many took four taps, the rescue and the orphan branch, and the device time.
    pt_upsample_stats upsamplePlanes(const pt_upsample_desc& d, pt_upsample_stats* stats = nullptr) {
        pt_upsample_stats s{};
        ck(pt_upsample_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // The SVGF temporal stage in one pass (pt_temporal_moments): demodulated colour, colour history, luminance moments and variance through
    // one gather, with an optional clamp of the history to this frame's 3x3 neighbourhood.  Every plane of `d` is DEVICE memory of this
    // context's device, frame-sized; block_mask is host memory.  Stateless and synchronous; the caller ping-pongs history, moments and
    // length.  Returns the pixels processed, those that kept their history, the clamped ones among them and the device time.
    pt_tmom_stats temporalMoments(const pt_tmom_desc& d, pt_tmom_stats* stats = nullptr) {
        pt_tmom_stats s{};
        ck(pt_temporal_moments(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // The end of the chain (pt_modulate_planes): multiplies the albedo back into the filtered, demodulated colour; out may be color itself.
    pt_modulate_stats modulatePlanes(const pt_modulate_desc& d, pt_modulate_stats* stats = nullptr) {
        pt_modulate_stats s{};
        ck(pt_modulate_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // Geometric edge antialiasing, the last pass before display (pt_edge_aa_planes): where a pixel and a neighbour show different surfaces,
    // the nearer triangle's edge is located between the two pixel centres and the pixel takes the matching share of the neighbour's colour.
    // d.out may not be d.color.  Returns the pixel, boundary and blended counts and the device time.
    pt_edge_aa_stats edgeAaPlanes(const pt_edge_aa_desc& d, pt_edge_aa_stats* stats = nullptr) {
        pt_edge_aa_stats s{};
        ck(pt_edge_aa_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // Auto exposure (pt_exposure_planes): meters d.color into d.hist, a histogram of log2 luminance per view, and adapts an exposure per
    // view from its trimmed mean into d.state_out (ev, E, mean log2 luminance, pixels metered), all DEVICE memory of the caller's.
    pt_exposure_stats exposurePlanes(const pt_exposure_desc& d, pt_exposure_stats* stats = nullptr) {
        pt_exposure_stats s{};
        ck(pt_exposure_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // The display operator under the metered exposure (pt_tonemap_planes): d.state is exposurePlanes's state_out, read on the device;
    // d.out may be d.color.  Returns the pixel and clipped counts and the device time.
    pt_tonemap_stats tonemapPlanes(const pt_tonemap_desc& d, pt_tonemap_stats* stats = nullptr) {
        pt_tonemap_stats s{};
        ck(pt_tonemap_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // The size in bytes of bloomPlanes's scratch pyramid for `levels` levels of every view (pt_bloom_layout); dims (host memory,
    // views x PT_BLOOM_MAX_LEVELS x 4: w, h, first 16-byte texel, 0) may be null.
    size_t bloomLayout(uint32_t levels, uint32_t* dims = nullptr) {
        size_t bytes = 0;
        ck(pt_bloom_layout(ctx, levels, dims, &bytes));
        return bytes;
    }
    // Bloom in front of the tone mapper (pt_bloom_planes): the part of d.color above d.threshold, spread over a pyramid per view in
    // d.scratch (bloomLayout's bytes, 16-byte aligned) and added back into d.out, which may be d.color.  Returns the pixels written, the
    // source pixels read, the bright and the non-finite ones among them and the device time.
    pt_bloom_stats bloomPlanes(const pt_bloom_desc& d, pt_bloom_stats* stats = nullptr) {
        pt_bloom_stats s{};
        ck(pt_bloom_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // The size in bytes of motionBlurPlanes's scratch, T and N of every view (pt_motion_blur_layout); dims (host memory, views x 4: tw, th,
    // the first 8-byte texel of T, the first of N) may be null.
    size_t motionBlurLayout(uint32_t* dims = nullptr) {
        size_t bytes = 0;
        ck(pt_motion_blur_layout(ctx, dims, &bytes));
        return bytes;
    }
    // Motion blur in front of the tone mapper (pt_motion_blur_planes): d.color blurred along the fastest motion (d.motion) of the tiles
    // around each pixel, depth-aware (d.depth), into d.out, which may not be d.color; d.scratch is motionBlurLayout's bytes, 8-byte
    // aligned.  Returns the pixels written, the rectangle pixels read, the unknown-motion ones among them, the pixels that gathered, the
    // taps that counted and the non-finite ones skipped, and the device time.
    pt_motion_blur_stats motionBlurPlanes(const pt_motion_blur_desc& d, pt_motion_blur_stats* stats = nullptr) {
        pt_motion_blur_stats s{};
        ck(pt_motion_blur_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // dofPlanes's `aperture` of a thin lens: K = 0.5 * A * f / (s - f) * px_per_unit, the blur-circle radius in pixels of a point at
    // infinity, with A = focal_length / f_number, s = focus (> focal_length, the same units) and px_per_unit = frame_height / sensor_height.
    static float dofAperture(float focal_length, float f_number, float focus, float sensor_height, float frame_height) {
        return 0.5f * (focal_length / f_number) * focal_length / (focus - focal_length) * (frame_height / sensor_height);
    }
    // The size in bytes of dofPlanes's scratch, T and N of every view (pt_dof_layout); dims (host memory, views x 4: tw, th, the first
    // 4-byte texel of T, the first of N) may be null.
    size_t dofLayout(uint32_t* dims = nullptr) {
        size_t bytes = 0;
        ck(pt_dof_layout(ctx, dims, &bytes));
        return bytes;
    }
    // Depth of field behind edge antialiasing and in front of bloom, motion blur and the tone mapper (pt_dof_planes): d.color gathered over
    // a disc of the largest blur circle (from d.depth, d.focus and d.aperture) of the tiles around each pixel, into d.out, which may not be
    // d.color; d.scratch is dofLayout's bytes.  Returns the pixels written, the rectangle pixels read, the pixels that gathered, the taps
    // that counted and the non-finite ones skipped, and the device time.
    pt_dof_stats dofPlanes(const pt_dof_desc& d, pt_dof_stats* stats = nullptr) {
        pt_dof_stats s{};
        ck(pt_dof_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // Lens pre-distortion, chromatic-aberration correction and rotational late reprojection, the last pass of the chain, behind the tone
    // mapper (pt_lens_warp_planes): per view and colour channel a radial polynomial around the lens centre, then a 3x3 matrix in pixel
    // coordinates (warpMatrix), name the source point that d.color is resampled at, into d.out and / or d.frame_rgba8, neither of which
    // may be d.color.  d.lenses is HOST memory, one pt_lens_view per view, or null.  Returns the pixels written, those with a channel
    // outside its rectangle, the non-finite words read as 0, and the device time.
    pt_lens_warp_stats lensWarpPlanes(const pt_lens_warp_desc& d, pt_lens_warp_stats* stats = nullptr) {
        pt_lens_warp_stats s{};
        ck(pt_lens_warp_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // lensWarpPlanes's matrix of a camera turn (pt_warp_matrix, host only): out maps a pixel under dst_cam to the pixel of the frame
    // rendered under src_cam (12 floats each: eye, U, V, W); the eyes are ignored.
    static void warpMatrix(const float src_cam[12], const float dst_cam[12], uint32_t width, uint32_t height, float out[9]) {
        if (pt_warp_matrix(src_cam, dst_cam, width, height, out) != PT_OK) throw std::runtime_error(pt_last_error(nullptr));
    }
    // The size in bytes of aoPlanes's scratch: one batch of rays (pt_ao_layout); max_rays_in_flight 0 is the library's default.
    size_t aoLayout(uint32_t rays, uint32_t max_rays_in_flight = 0) {
        size_t bytes = 0;
        ck(pt_ao_layout(ctx, rays, max_rays_in_flight, &bytes));
        return bytes;
    }
    // Ray-traced ambient occlusion from the G-buffer (pt_ao_planes): every pixel of a hit in d.hit shoots d.rays any-hit rays of length
    // d.radius over the cosine-weighted hemisphere around its geometric normal, through the current tree, into d.ao, d.out (ao as a colour)
    // and / or d.bent; d.scratch is aoLayout's bytes, 16-byte aligned.  Returns the pixels, those traced, skipped (misses) and non-finite,
    // the rays traced, occluded and invalid, the batches, and the device times of the pass and of its traversal launches.
    pt_ao_stats aoPlanes(const pt_ao_desc& d, pt_ao_stats* stats = nullptr) {
        pt_ao_stats s{};
        ck(pt_ao_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // The size in bytes of reflectPlanes's scratch: one batch of rays (pt_reflect_layout); max_rays_in_flight 0 is the library's default.
    size_t reflectLayout(uint32_t max_rays_in_flight = 0) {
        size_t bytes = 0;
        ck(pt_reflect_layout(ctx, max_rays_in_flight, &bytes));
        return bytes;
    }
    // Mirror reflections from the G-buffer (pt_reflect_planes): every pixel of a hit in d.hit shoots its mirror ray through the current tree;
    // what it sees is a second G-buffer — d.hit2 (pt_trace_device's pt_hit for that ray), d.position2, d.ray — and d.sky, the probe's radiance
    // where the ray escapes.  d.scratch is reflectLayout's bytes, 16-byte aligned.  Returns the pixels, those traced, skipped (misses),
    // non-finite and invalid, the rays that hit and escaped, the batches, and the device times of the pass and of its traversal launches.
    pt_reflect_stats reflectPlanes(const pt_reflect_desc& d, pt_reflect_stats* stats = nullptr) {
        pt_reflect_stats s{};
        ck(pt_reflect_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // The size in bytes of shadowPlanes's scratch: one batch of rays (pt_shadow_layout) for these lights' ray counts; max_rays_in_flight 0
    // is the library's default.
    size_t shadowLayout(const pt_shadow_light* lights, uint32_t num_lights, uint32_t max_rays_in_flight = 0) {
        size_t bytes = 0;
        ck(pt_shadow_layout(ctx, lights, num_lights, max_rays_in_flight, &bytes));
        return bytes;
    }
    // Shadows and direct light of d.num_lights distant disc lights from the G-buffer (pt_shadow_planes): every pixel of a hit in d.hit
    // shoots each light's rays, for the lights above its horizon, through the current tree, into d.visibility (the open fraction per light)
    // and / or d.light (the sum of radiance * cosine * visibility, 1 in .w); d.view_ray, pt_reflect_planes's ray plane, lights a reflected
    // surface.  d.scratch is shadowLayout's bytes, 16-byte aligned.  Returns the pixels, those traced, skipped (misses) and non-finite, the
    // (pixel, light) pairs under the horizon, the rays traced, occluded and invalid, the batches, and the device times.
    pt_shadow_stats shadowPlanes(const pt_shadow_desc& d, pt_shadow_stats* stats = nullptr) {
        pt_shadow_stats s{};
        ck(pt_shadow_planes(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // Which 8x8 blocks of the coming frame need new samples (pt_sample_plan): those where the reprojection loses a pixel, where enough
    // pixels have a short history or moments that are still noisy, and those the refresh names.  d.block_mask_out is HOST memory, one
    // byte per block: what renderMask and the passes take as their mask.  Returns the block and pixel counts and the device time.
    pt_plan_stats samplePlan(const pt_plan_desc& d, pt_plan_stats* stats = nullptr) {
        pt_plan_stats s{};
        ck(pt_sample_plan(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    // The temporal stage of the blocks that were not rendered (pt_temporal_carry): history, moments and length reprojected and written
    // unchanged.  With the complement of a plan's mask and the plan's planes and parameters, `lost` is 0.
    pt_carry_stats temporalCarry(const pt_carry_desc& d, pt_carry_stats* stats = nullptr) {
        pt_carry_stats s{};
        ck(pt_temporal_carry(ctx, &d, &s));
        if (stats) *stats = s;
        return s;
    }
    static std::vector<pt_mesh_update> mesh_updates(const Model* model, const std::vector<uint32_t>& meshes) {
        static_assert(sizeof(float3) == 3 * sizeof(float), "TriangleMesh::vertex must stay float3-packed");
        std::vector<pt_mesh_update> u;
        for (uint32_t m : meshes) {
            if (m >= model->meshes.size()) throw std::runtime_error("updateMeshes: mesh index out of range");
            const TriangleMesh* tm = model->meshes[m];
            u.push_back(pt_mesh_update{m, tm->vertex.empty() ? nullptr : &tm->vertex[0].x, (uint32_t)tm->vertex.size()});
        }
        return u;
    }
    bool denoiserOn = true;  // SimplePathtracer.h:63 (default true there too); nothing reads it in the reference (OptixDenoiser.cpp:15-42 is empty)
    LaunchParams launchParams;   // SimplePathtracer.h:137
    stream_t stream = nullptr;   // SimplePathtracer.h:107: the context's stream (pt_stream), e.g. for output_buffer.setStream(sample.stream), main.cpp:245
    pt_ctx* ctx = nullptr;

  private:
    void ck(int rc) { if (rc != PT_OK) throw std::runtime_error(pt_last_error(ctx)); }
};

// The same surface over several GPUs of one process (pt_create_multi, include/pt_amd.h): the frame is tile-partitioned over
// `devices`, rendered concurrently, and the rgba8 frame is assembled on every rank by one RCCL all-gather per displayed frame.
class MultiSampleRenderer {
  public:
    MultiSampleRenderer(const Model* model, const std::vector<int>& devices) {
        std::vector<pt_mesh_desc> md(model->meshes.size());
        for (size_t i = 0; i < md.size(); ++i) {
            const TriangleMesh* m = model->meshes[i];
            md[i].vertex = &m->vertex[0].x; md[i].num_vertices = (uint32_t)m->vertex.size();
            md[i].index = &m->index[0].x; md[i].num_triangles = (uint32_t)m->index.size();
            md[i].material = *reinterpret_cast<const pt_material*>(&m->material);
            md[i].diffuse_texture_id = m->diffuseTextureID;
            md[i].texcoord = m->texcoord.size() == m->vertex.size() && !m->texcoord.empty() ? &m->texcoord[0].x : nullptr;
        }
        std::vector<pt_texture_desc> td(model->textures.size());
        for (size_t i = 0; i < td.size(); ++i) td[i] = pt_texture_desc{model->textures[i]->pixel, model->textures[i]->resolution.x, model->textures[i]->resolution.y};
        pt_scene_desc sd{md.data(), (uint32_t)md.size(), td.data(), (uint32_t)td.size()};
        if (pt_create_multi(&sd, devices.data(), (int)devices.size(), &multi) != PT_OK) throw std::runtime_error(std::string("MultiSampleRenderer: ") + pt_multi_last_error(nullptr));
    }
    ~MultiSampleRenderer() { pt_multi_destroy(multi); }
    MultiSampleRenderer(const MultiSampleRenderer&) = delete;
    MultiSampleRenderer& operator=(const MultiSampleRenderer&) = delete;

    void render() { ck(pt_multi_render(multi, launchParams.samples_per_launch, launchParams.frame.subframe_index, 1u << PT_BUF_FRAME, nullptr)); }
    // render() + the assembled frame in HOST memory (same name and meaning as SampleRenderer::renderToHost)
    void renderToHost(uint32_t* h_pixels) { ck(pt_multi_render(multi, launchParams.samples_per_launch, launchParams.frame.subframe_index, 1u << PT_BUF_FRAME, h_pixels)); }
    void render(uint32_t*) = delete; // see SampleRenderer: the memory kind is part of the name
    void renderBatch(uint32_t count, uint32_t* h_pixels = nullptr) {
        ck(pt_multi_render_batch(multi, launchParams.samples_per_launch, launchParams.frame.subframe_index, count, 1u << PT_BUF_FRAME, h_pixels));
        launchParams.frame.subframe_index += count;
    }
    void resize(const int2& newSize) {
        ck(pt_multi_resize(multi, newSize.x, newSize.y, 0, 0));
        if (newSize.x && newSize.y) launchParams.frame.size = newSize;
    }
    void downloadPixels(uint32_t h_pixels[]) { // rank 0 holds the assembled frame after render()
        if (pt_download(pt_multi_ctx(multi, 0), PT_BUF_FRAME, h_pixels, sizeof(uint32_t) * (size_t)launchParams.frame.size.x * launchParams.frame.size.y) != PT_OK)
            throw std::runtime_error(pt_last_error(pt_multi_ctx(multi, 0)));
    }
    void setCamera(const Camera& camera) {
        float3 U, V, W;
        camera.UVWFrame(U, V, W);
        ck(pt_multi_set_camera(multi, &camera.eye.x, &U.x, &V.x, &W.x));
    }
    void setViews(const std::vector<View>& views) { // SampleRenderer::setViews on every rank, after resize()
        const std::vector<pt_view> v = toViews(views);
        ck(pt_multi_set_views(multi, v.data(), (uint32_t)v.size()));
    }
    void setProbe(const ProbeData& probe) {
        if (!probe.valid) throw std::runtime_error("Probe Data is not valid");
        ck(pt_multi_set_probe(multi, &probe.data[0].x, probe.pdfValuesX.data(), probe.cdfValuesX.data(), probe.pdfValuesY.data(), probe.cdfValuesY.data(), probe.width, probe.height));
    }
    void gather(int which) { ck(pt_multi_gather(multi, which)); } // assemble another buffer (e.g. PT_BUF_ACCUM) on every rank
    // Frames in flight (2 or 3): renderToHost(h_pixels) then shows frame k-1 while frame k renders — the exchange of the strips overlaps the
    // rendering and lands in the ranks' display buffers — and flush(h_pixels) hands over the last frame.
    void setFramesInFlight(int n) {
        pt_options o;
        if (pt_get_options(pt_multi_ctx(multi, 0), &o) != PT_OK) throw std::runtime_error("MultiSampleRenderer: pt_get_options failed");
        o.frames_in_flight = n;
        ck(pt_multi_set_options(multi, &o));
    }
    void flush(uint32_t* h_pixels = nullptr) { ck(pt_multi_flush(multi, h_pixels)); }
    double updateMeshes(const Model* model, const std::vector<uint32_t>& meshes, bool rebuild = false) { // SampleRenderer::updateMeshes on every rank
        double ms = 0;
        const std::vector<pt_mesh_update> u = SampleRenderer::mesh_updates(model, meshes);
        ck(pt_multi_update_meshes(multi, u.data(), (uint32_t)u.size(), rebuild ? PT_UPDATE_REBUILD : PT_UPDATE_REFIT, &ms));
        return ms;
    }
    double transformMeshes(const std::vector<pt_mesh_transform>& transforms, bool from_current = false, bool rebuild = false) { // on every rank
        double ms = 0;
        ck(pt_multi_transform_meshes(multi, transforms.data(), (uint32_t)transforms.size(), from_current ? PT_FROM_CURRENT : PT_FROM_REST,
                                     rebuild ? PT_UPDATE_REBUILD : PT_UPDATE_REFIT, &ms));
        return ms;
    }
    void downloadDisplayedPixels(uint32_t h_pixels[]) { // the frame on display (rank 0's display buffer) in the frames-in-flight mode
        if (pt_download_display(pt_multi_ctx(multi, 0), PT_BUF_FRAME, h_pixels, sizeof(uint32_t) * (size_t)launchParams.frame.size.x * launchParams.frame.size.y) != PT_OK)
            throw std::runtime_error(pt_last_error(pt_multi_ctx(multi, 0)));
    }
    LaunchParams launchParams;
    pt_multi* multi = nullptr;

  private:
    void ck(int rc) { if (rc != PT_OK) throw std::runtime_error(pt_multi_last_error(multi)); }
};

} // namespace ptamd
