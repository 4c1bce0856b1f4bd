"""Host-side mirror of the reference's SampleRenderer (SimplePathtracer.h:38-176) over the C ABI.

Same public surface — SampleRenderer(model), render(), resize(size), downloadPixels(), setCamera(camera),
setProbe(probe), the public `launchParams` the app pokes directly (samples_per_launch, frame.subframe_index,
frame.size) — and the same error behaviour: failures raise RuntimeError (the reference throws
sutil::Exception : std::runtime_error), render() before resize() silently does nothing, resize to 0 is ignored.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import Material as CMaterial
from ._lib import MeshDesc, Options, Region, SceneDesc, Stats, TextureDesc, Variant
from .scenes import Model, ProbeData, uvw_frame

PT_BUF_ACCUM, PT_BUF_FRAME, PT_BUF_COLOR, PT_BUF_NORMAL, PT_BUF_ALBEDO, PT_BUF_DENOISED = range(6)
PT_BSDF_DISNEY, PT_BSDF_LAMBERT = 0, 1


@dataclass
class Camera:
    """sutil::Camera (eye, lookat, up, fovY in degrees, aspectRatio)."""

    eye: tuple
    lookat: tuple
    up: tuple = (0.0, 1.0, 0.0)
    fovY: float = 35.0
    aspectRatio: float = 1.0

    def UVWFrame(self):
        L = _lib.load_library()
        f3 = C.c_float * 3
        U, V, W = f3(), f3(), f3()
        rc = L.pt_uvw_frame(C.byref(f3(*self.eye)), C.byref(f3(*self.lookat)), C.byref(f3(*self.up)), self.fovY, self.aspectRatio, C.byref(U), C.byref(V), C.byref(W))
        if rc:
            raise RuntimeError("pt_uvw_frame failed")
        return np.array(U, np.float32), np.array(V, np.float32), np.array(W, np.float32)


@dataclass
class _Frame:
    size: tuple = (0, 0)
    subframe_index: int = 0


@dataclass
class LaunchParams:
    """The fields of LaunchParams (LaunchParams.h:51-79) the application sets directly."""

    frame: _Frame = field(default_factory=_Frame)
    samples_per_launch: int = 1


def _scene_desc(model: Model):
    """pt_scene_desc for a Model plus the arrays it points into (keep them alive until pt_create returns)."""
    meshes = (MeshDesc * len(model.meshes))()
    keep = []
    for k, m in enumerate(model.meshes):
        v = np.ascontiguousarray(m.vertex, np.float32)
        ix = np.ascontiguousarray(m.index, np.uint32)
        keep += [v, ix]
        meshes[k].vertex = v.ctypes.data
        meshes[k].num_vertices = len(v)
        meshes[k].index = ix.ctypes.data
        meshes[k].num_triangles = len(ix)
        C.memmove(C.byref(meshes[k].material), np.asarray(m.material).tobytes(), 104)
        meshes[k].diffuse_texture_id = m.diffuseTextureID
        if m.texcoord is not None and len(m.texcoord):
            tc = np.ascontiguousarray(m.texcoord, np.float32)
            assert tc.shape == (len(v), 2)
            keep.append(tc)
            meshes[k].texcoord = tc.ctypes.data
    textures = getattr(model, "textures", []) or []
    tdesc = (TextureDesc * max(1, len(textures)))()
    for k, t in enumerate(textures):
        px = np.ascontiguousarray(t.pixel, np.uint32)
        keep.append(px)
        tdesc[k].pixel = px.ctypes.data
        tdesc[k].height, tdesc[k].width = px.shape
    keep += [meshes, tdesc]
    return SceneDesc(meshes, len(model.meshes), tdesc, len(textures)), keep


def _mesh_updates(vertices: dict):
    """pt_mesh_update[] for {mesh_index: (num_vertices, 3) float32 array} plus the arrays it points into (keep them alive for the call)."""
    ups = (_lib.MeshUpdate * max(1, len(vertices)))()
    keep = []
    for k, (mesh, v) in enumerate(vertices.items()):
        v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
        keep.append(v)
        ups[k].mesh = int(mesh)
        ups[k].vertex = v.ctypes.data_as(C.POINTER(C.c_float))
        ups[k].num_vertices = len(v)
    return ups, len(vertices), keep


def _pairs(d):
    """{mesh: value} or [(mesh, value), ...] (the list form can name a mesh twice: the library refuses that)."""
    return list(d.items()) if hasattr(d, "items") else list(d)


def _device_updates(vertices, device: int):
    """pt_mesh_update[] over DEVICE memory: a value is a CUDA float32 contiguous (nv, 3) torch tensor on `device`, or (pointer, nv)."""
    pairs = _pairs(vertices)
    ups = (_lib.MeshUpdate * max(1, len(pairs)))()
    keep = []
    for k, (mesh, v) in enumerate(pairs):
        if isinstance(v, tuple):
            ptr, nv = int(v[0]), int(v[1])
        else:
            import torch

            if not isinstance(v, torch.Tensor):
                raise TypeError(f"updateMeshesDevice: mesh {mesh}: a torch tensor or (device pointer, num_vertices) is expected (host arrays: updateMeshes)")
            if not v.is_cuda or (v.device.index or 0) != device:
                raise ValueError(f"updateMeshesDevice: mesh {mesh}: the tensor is on {v.device}, the context on GPU {device}")
            if v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3 or not v.is_contiguous():
                raise ValueError(f"updateMeshesDevice: mesh {mesh}: a contiguous float32 (num_vertices, 3) tensor is expected")
            torch.cuda.current_stream(v.device).synchronize()  # the library reads on its own stream: what torch enqueued must be complete
            keep.append(v)
            ptr, nv = v.data_ptr(), v.shape[0]
        ups[k].mesh = int(mesh)
        ups[k].vertex = C.cast(C.c_void_p(ptr), C.POINTER(C.c_float))
        ups[k].num_vertices = nv
    return ups, len(pairs), keep


def _check_query_tensor(name, t, device: int, dtype, tail: tuple):
    """traceDevice: a CUDA tensor of `dtype` on GPU `device`, shape (n,) + tail, rows dense (any storage offset) — checked before the library is called."""
    import torch

    if not isinstance(t, torch.Tensor):
        raise TypeError(f"traceDevice: {name}: a torch tensor or a device pointer is expected (host arrays: trace)")
    if not t.is_cuda or (t.device.index or 0) != device:
        raise ValueError(f"traceDevice: {name}: the tensor is on {t.device}, the context on GPU {device}")
    if t.dtype != dtype or t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tuple(tail) or not t.is_contiguous():
        raise ValueError(f"traceDevice: {name}: a contiguous {dtype} tensor of shape (n{''.join(f', {k}' for k in tail)}) is expected, got {t.dtype} {tuple(t.shape)}")


def _check_temporal_tensor(name, t, device: int, shapes: dict, fn="temporalAccumulate"):
    """The plane check of every method that takes GPU planes: a CUDA tensor on GPU `device` whose (dtype, shape) is one of `shapes`, dense
    (any storage offset) — checked before the library is called."""
    import torch

    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{fn}: {name}: a torch tensor or a device pointer is expected")
    if not t.is_cuda or (t.device.index or 0) != device:
        raise ValueError(f"{fn}: {name}: the tensor is on {t.device}, the context on GPU {device}")
    if shapes.get(t.dtype) != tuple(t.shape) or not t.is_contiguous():
        want = " or ".join(f"{d} tensor of shape {sh}" for d, sh in shapes.items())
        raise ValueError(f"{fn}: {name}: a contiguous {want} is expected, got {t.dtype} {tuple(t.shape)}")


def _mesh_transforms(transforms):
    """pt_mesh_transform[] for {mesh_index: 3x4 or 4x4 array} (the last row of a 4x4 is dropped)."""
    pairs = _pairs(transforms)
    arr = (_lib.MeshTransform * max(1, len(pairs)))()
    for k, (mesh, m) in enumerate(pairs):
        m = np.asarray(m, np.float32)
        if m.shape not in ((3, 4), (4, 4)):
            raise ValueError(f"transformMeshes: mesh {mesh}: a 3x4 or 4x4 matrix is expected, got {m.shape}")
        arr[k].mesh = int(mesh)
        arr[k].m[:] = [float(x) for x in m[:3].reshape(-1)]
    return arr, len(pairs)


def _view_array(views):
    """pt_view[] for [(x, y, width, height, Camera), ...]: the camera's U, V, W are those setCamera would give it (take the view's own aspect)."""
    arr = (_lib.View * max(1, len(views)))()
    for k, (x, y, w, h, cam) in enumerate(views):
        U, V, W = cam.UVWFrame()
        arr[k].x, arr[k].y, arr[k].width, arr[k].height = int(x), int(y), int(w), int(h)
        for name, val in (("eye", cam.eye), ("U", U), ("V", V), ("W", W)):
            getattr(arr[k], name)[:] = [float(c) for c in val]
    return arr


def _camera_rows(cameras) -> np.ndarray:
    """(n, 12) float32 rows eye, U, V, W for a list of Cameras or an array-like of that shape."""
    if len(cameras) and isinstance(cameras[0], Camera):
        cameras = [np.concatenate([np.asarray(c.eye, np.float32), *c.UVWFrame()]) for c in cameras]
    rows = np.ascontiguousarray(cameras, np.float32)
    if rows.ndim != 2 or rows.shape[1] != 12:
        raise ValueError(f"setViewCameras: n cameras or an (n, 12) array (eye, U, V, W) is expected, got shape {rows.shape}")
    return rows


def _is_torch_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def _views_list(L, ctx):
    n = C.c_uint32()
    L.pt_get_views(ctx, None, 0, C.byref(n))
    arr = (_lib.View * max(1, n.value))()
    L.pt_get_views(ctx, arr, n.value, None)
    return [dict(x=v.x, y=v.y, width=v.width, height=v.height, eye=np.array(v.eye, np.float32), U=np.array(v.U, np.float32),
                 V=np.array(v.V, np.float32), W=np.array(v.W, np.float32)) for v in arr[:n.value]]


class SampleRenderer:
    def __init__(self, model: Model, device: int = 0):
        self._device = int(device)
        self._nv = [len(m.vertex) for m in model.meshes]
        self._L = L = _lib.load_library()
        self._ctx = C.c_void_p()
        self.launchParams = LaunchParams()
        sd, self._keep = _scene_desc(model)
        rc = L.pt_create(C.byref(sd), device, C.byref(self._ctx))
        if rc:
            self._ctx = C.c_void_p()
            raise RuntimeError(f"pt_create failed ({rc}): {L.pt_last_error(None).decode()}")
        self._keep = []  # the scene was deep-copied

    # -- internals
    def _ck(self, rc, what):
        if rc:
            raise RuntimeError(f"{what} failed ({rc}): {self._L.pt_last_error(self._ctx).decode()}")

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.pt_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- reference API
    def render(self, out: np.ndarray | None = None):
        """render() / render(CUDAOutputBuffer&): one launch with the current launchParams."""
        ptr = None
        if out is not None:
            assert out.dtype == np.uint32 and out.flags["C_CONTIGUOUS"]
            ptr = out.ctypes.data
        self._ck(self._L.pt_render(self._ctx, int(self.launchParams.samples_per_launch), int(self.launchParams.frame.subframe_index), ptr), "pt_render")

    def renderDevice(self, dev_ptr: int):
        """render(sutil::CUDAOutputBuffer<uint32_t>&) (SimplePathtracer.cpp:99-107): the rgba8 frame lands in the caller's DEVICE buffer
        (width*height*4 bytes, e.g. tensor.data_ptr()); complete when the call returns (pt_render_device)."""
        self._ck(self._L.pt_render_device(self._ctx, int(self.launchParams.samples_per_launch), int(self.launchParams.frame.subframe_index), dev_ptr), "pt_render_device")

    @property
    def stream(self) -> int:
        """SampleRenderer::stream (SimplePathtracer.h:107): the context's hipStream_t as an integer (pt_stream); non-blocking."""
        return self._L.pt_stream(self._ctx)

    def waitEvent(self, hip_event: int):
        """Everything enqueued on the context's stream from now on waits for the caller's event (pt_wait_event; torch: event.cuda_event)."""
        self._ck(self._L.pt_wait_event(self._ctx, hip_event), "pt_wait_event")

    def renderBatch(self, count: int, out: np.ndarray | None = None):
        """`count` iterations of the reference's progressive loop (render(); subframe_index++, main.cpp:273-278) as ONE wavefront
        batch (pt_render_batch): same buffers bit for bit, count times the rays per launch.  Like render(), it leaves
        launchParams.frame.subframe_index to the application (advance it by `count`)."""
        ptr = None
        if out is not None:
            assert out.dtype == np.uint32 and out.flags["C_CONTIGUOUS"]
            ptr = out.ctypes.data
        self._ck(self._L.pt_render_batch(self._ctx, int(self.launchParams.samples_per_launch), int(self.launchParams.frame.subframe_index), int(count), ptr), "pt_render_batch")

    def resize(self, newSize):
        w, h = int(newSize[0]), int(newSize[1])
        self._ck(self._L.pt_resize(self._ctx, w, h), "pt_resize")
        if w and h:
            self.launchParams.frame.size = (w, h)

    def downloadPixels(self) -> np.ndarray:
        return self.download(PT_BUF_FRAME)

    def setCamera(self, camera: Camera):
        U, V, W = camera.UVWFrame()
        self.setCameraUVW(camera.eye, U, V, W)

    def setCameraUVW(self, eye, U, V, W):
        f3 = C.c_float * 3
        self._ck(self._L.pt_set_camera(self._ctx, C.byref(f3(*[float(x) for x in eye])), C.byref(f3(*[float(x) for x in U])), C.byref(f3(*[float(x) for x in V])), C.byref(f3(*[float(x) for x in W]))), "pt_set_camera")

    # -- viewports (pt_set_views, include/pt_amd.h): several cameras in rectangles of one frame
    def setViews(self, views):
        """[(x, y, width, height, Camera), ...] after resize(): every render call then fills each rectangle as a frame of its own size with
        its own camera would be filled, in one batch; pixels in no view are left alone.  [] returns to the single camera of setCamera."""
        views = list(views)
        self._ck(self._L.pt_set_views(self._ctx, _view_array(views) if views else None, len(views)), "pt_set_views")

    def views(self):
        """The current views as dicts x, y, width, height, eye, U, V, W (pt_get_views)."""
        return _views_list(self._L, self._ctx)

    def setViewCameras(self, cameras):
        """New cameras for the current views, rectangles unchanged (the per-frame call): a list of Cameras, an (n, 12) array of eye, U, V, W
        rows, or a CUDA float32 torch tensor of that shape on the context's GPU, which is read on the device (pt_set_view_cameras_device)
        after torch's current stream has been synchronised on the host."""
        if _is_torch_tensor(cameras):
            import torch

            t = cameras
            if not t.is_cuda or (t.device.index or 0) != self._device:
                raise ValueError(f"setViewCameras: the tensor is on {t.device}, the context on GPU {self._device}")
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 12 or not t.is_contiguous():
                raise ValueError(f"setViewCameras: a contiguous float32 (n, 12) tensor is expected, got {t.dtype} {tuple(t.shape)}")
            torch.cuda.current_stream(t.device).synchronize()  # the library reads on its own stream: what torch enqueued must be complete
            self._ck(self._L.pt_set_view_cameras_device(self._ctx, t.data_ptr(), t.shape[0]), "pt_set_view_cameras_device")
            return
        rows = _camera_rows(cameras)
        self._ck(self._L.pt_set_view_cameras(self._ctx, rows.ctypes.data, rows.shape[0]), "pt_set_view_cameras")

    def setProbe(self, probe: ProbeData):
        if not probe.valid:
            raise RuntimeError("Probe Data is not valid")  # Probe.h:104-105
        arrs = [np.ascontiguousarray(a, np.float32) for a in (probe.data, probe.pdfValuesX, probe.cdfValuesX, probe.pdfValuesY, probe.cdfValuesY)]
        self._ck(self._L.pt_set_probe(self._ctx, *[a.ctypes.data for a in arrs], probe.width, probe.height), "pt_set_probe")
        self._probe_wh = (probe.width, probe.height)

    def setProbeImage(self, data: np.ndarray):
        """loadProbe + BuildCDF + setProbe with the CDF built on the GPU (bit-identical to the host BuildCDF)."""
        d = np.ascontiguousarray(data, np.float32)
        h, w = d.shape[0], d.shape[1]
        self._ck(self._L.pt_set_probe_image(self._ctx, d.ctypes.data, w, h), "pt_set_probe_image")
        self._probe_wh = (w, h)

    def probeCDF(self):
        w, h = self._probe_wh
        pdfX = np.empty((h, w), np.float32); cdfX = np.empty((h, w), np.float32)
        pdfY = np.empty(h, np.float32); cdfY = np.empty(h, np.float32)
        self._ck(self._L.pt_get_probe_cdf(self._ctx, pdfX.ctypes.data, cdfX.ctypes.data, pdfY.ctypes.data, cdfY.ctypes.data), "pt_get_probe_cdf")
        return pdfX, cdfX, pdfY, cdfY

    # -- the foveated variants' render() (HelloPathtracing_sv4_vmv23/SimplePathtracer.cpp:77-216)
    SV4_VARIANT = dict(radiance_tmin=0.01, cull_back_occlusion=1, tonemap=1, exposure=4.0, white=1.0)
    # HelloPathtracing_sv3: same device code except exposure 2^3 and no Reinhard in the final write; host radii 100/200, spp 2/8/64
    SV3_VARIANT = dict(radiance_tmin=0.01, cull_back_occlusion=1, tonemap=2, exposure=8.0, white=1.0)
    SV3_SCHEDULE = dict(inner_radius=100, outer_radius=200, spp=(2, 8, 64))
    # HelloPathtracing_sv and _sv2 (one device program): canonical tmin / occlusion flags / make_color, but prd.depth starts at 1 with
    # the cutoff `depth >= 3` (deviceProgram.cu:428,483 -> setOptions(max_depth=3)) and the launch also writes the AOV buffers (:553-555);
    # host schedule = sv3's radii and sample counts (HelloPathtracing_sv/SimplePathtracer.cpp:131-198)
    SV_VARIANT = dict(radiance_tmin=0.001, cull_back_occlusion=0, tonemap=0, exposure=1.0, white=1.0, initial_depth=1, write_aov=1)
    SV_MAX_DEPTH = 3

    def renderRegions(self, regions, variant=None, out: np.ndarray | None = None):
        """regions: list of dicts with pt_region's fields; variant: dict with pt_variant's fields (None = canonical)."""
        arr = (Region * len(regions))()
        for k, g in enumerate(regions):
            for name, _ in Region._fields_:
                setattr(arr[k], name, g[name])
        vp = None
        if variant is not None:
            v = Variant(**variant)
            vp = C.byref(v)
        ptr = out.ctypes.data if out is not None else None
        self._ck(self._L.pt_render_regions(self._ctx, arr, len(regions), vp, ptr), "pt_render_regions")

    @staticmethod
    def foveatedRegions(size, c, subframe_index, inner_radius=157, outer_radius=515, spp=(1, 2, 8)):
        """The three launches of sv4's FOV_ON render(): periphery at 1/4 resolution (accumulating), an annulus at 1/2
        resolution and the fovea at full resolution (both redrawn every frame with subframe_index 0)."""
        w, h = size
        cx, cy = c
        u32 = lambda v: int(v) & 0xFFFFFFFF  # uint2 arithmetic wraps like the reference's
        return [
            dict(launch_w=w // 4, launch_h=h // 4, factor_x=4, factor_y=4, fill_size=4, cx=cx, cy=cy, r_inner=float(outer_radius), r_outer=1000000000.0,
                 offset_x=0, offset_y=0, redraw=0, spp=spp[0], subframe_index=subframe_index),
            dict(launch_w=outer_radius + 2, launch_h=outer_radius + 2, factor_x=2, factor_y=2, fill_size=2, cx=cx, cy=cy, r_inner=float(inner_radius),
                 r_outer=float(outer_radius + 2), offset_x=u32(cx - (outer_radius + 2)), offset_y=u32(cy - (outer_radius + 2)), redraw=1, spp=spp[1], subframe_index=0),
            dict(launch_w=(inner_radius + 1) * 2, launch_h=(inner_radius + 1) * 2, factor_x=1, factor_y=1, fill_size=1, cx=cx, cy=cy, r_inner=0.0,
                 r_outer=float(inner_radius + 1), offset_x=u32(cx - (inner_radius + 1)), offset_y=u32(cy - (inner_radius + 1)), redraw=1, spp=spp[2], subframe_index=0),
        ]

    def renderFoveated(self, c, inner_radius=157, outer_radius=515, spp=(1, 2, 8), out=None, variant=None):
        """sv4 SampleRenderer::render() with FOV_ON: three launches around the gaze point c (launchParams.frame.c),
        then launchParams.frame.subframe_index++ (SimplePathtracer.cpp:132-216)."""
        regs = self.foveatedRegions(self.launchParams.frame.size, c, int(self.launchParams.frame.subframe_index), inner_radius, outer_radius, spp)
        self.renderRegions(regs, variant or self.SV4_VARIANT, out)
        self.launchParams.frame.subframe_index += 1

    # -- block masks and adaptive stopping (pt_render_mask, pt_render_adaptive; include/pt_amd.h)
    def blockGrid(self):
        """(nby, nbx): the 8x8 blocks of the current frame size."""
        w, h = self.launchParams.frame.size
        return (h + 7) // 8, (w + 7) // 8

    def renderMask(self, mask: np.ndarray, out: np.ndarray | None = None) -> int:
        """render() for the 8x8 blocks whose byte in `mask` (nby x nbx, or flat) is non-zero: those pixels end up as render() leaves them,
        all others are untouched.  Synchronous.  Like render(), it leaves launchParams.frame.subframe_index to the application.
        Returns the number of pixels rendered."""
        nby, nbx = self.blockGrid()
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        if m.size != nby * nbx:
            raise ValueError(f"renderMask: the mask needs {nby} x {nbx} entries, got {m.size}")
        ptr = None
        if out is not None:
            assert out.dtype == np.uint32 and out.flags["C_CONTIGUOUS"]
            ptr = out.ctypes.data
        n = C.c_uint32()
        self._ck(self._L.pt_render_mask(self._ctx, int(self.launchParams.samples_per_launch), int(self.launchParams.frame.subframe_index), m.ctypes.data, ptr, C.byref(n)), "pt_render_mask")
        return n.value

    def adaptiveBegin(self, threshold=0.02, dark_floor=0.01, min_subframes=8, max_subframes=0):
        """Starts (or restarts, after a camera move) an adaptive accumulation: all blocks active, moments cleared."""
        prm = _lib.AdaptiveParams(float(threshold), float(dark_floor), int(min_subframes), int(max_subframes))
        self._ck(self._L.pt_adaptive_begin(self._ctx, C.byref(prm)), "pt_adaptive_begin")

    def renderAdaptive(self, out: np.ndarray | None = None) -> dict:
        """render() for the blocks that have not converged yet, then the stopping rule for them on the GPU.  Returns pt_adaptive_stats as a
        dict; a progressive loop ends when its active_blocks is 0.  Advancing subframe_index stays the caller's job."""
        ptr = None
        if out is not None:
            assert out.dtype == np.uint32 and out.flags["C_CONTIGUOUS"]
            ptr = out.ctypes.data
        st = _lib.AdaptiveStats()
        self._ck(self._L.pt_render_adaptive(self._ctx, int(self.launchParams.samples_per_launch), int(self.launchParams.frame.subframe_index), ptr, C.byref(st)), "pt_render_adaptive")
        return st.as_dict()

    def adaptiveArrays(self):
        """(moments float32[h, w, 4] = {n, s1, s2, 0} per pixel, active uint8[nby, nbx])"""
        w, h = self.launchParams.frame.size
        nby, nbx = self.blockGrid()
        moments = np.empty((h, w, 4), np.float32)
        active = np.empty((nby, nbx), np.uint8)
        self._ck(self._L.pt_download_adaptive(self._ctx, _lib.PT_ADAPT_MOMENTS, moments.ctypes.data, moments.nbytes), "pt_download_adaptive")
        self._ck(self._L.pt_download_adaptive(self._ctx, _lib.PT_ADAPT_ACTIVE, active.ctypes.data, active.nbytes), "pt_download_adaptive")
        return moments, active

    def adaptiveEnd(self):
        self._ck(self._L.pt_adaptive_end(self._ctx), "pt_adaptive_end")

    # -- beyond the reference (runtime versions of its compile-time constants, multi-GPU, stats)
    def setOptions(self, max_depth=8, bsdf_mode=PT_BSDF_DISNEY, max_paths=0, bvh_kind=0, trace_kernel=0, streams=0, split_shadow=0, kernel_timing=0, frames_in_flight=0):
        o = Options(max_depth, bsdf_mode, max_paths, kernel_timing, bvh_kind, trace_kernel, streams, split_shadow, frames_in_flight)
        self._ck(self._L.pt_set_options(self._ctx, C.byref(o)), "pt_set_options")

    def setPartition(self, rank, world, tile_w=64, tile_h=16):
        self._ck(self._L.pt_set_partition(self._ctx, rank, world, tile_w, tile_h), "pt_set_partition")

    def sync(self):
        """Waits for the frames in flight (setOptions(frames_in_flight=2 or 3)); their errors surface here."""
        self._ck(self._L.pt_sync(self._ctx), "pt_sync")

    def download(self, which) -> np.ndarray:
        w, h = self.launchParams.frame.size
        if which == PT_BUF_FRAME:
            out = np.empty((h, w), np.uint32)
        else:
            out = np.empty((h, w, 4), np.float32)
        self._ck(self._L.pt_download(self._ctx, which, out.ctypes.data, out.nbytes), "pt_download")
        return out

    def uploadAccum(self, accum: np.ndarray):
        a = np.ascontiguousarray(accum, np.float32)
        self._ck(self._L.pt_upload_accum(self._ctx, a.ctypes.data, a.nbytes), "pt_upload_accum")

    def tonemapSqrt(self) -> np.ndarray:
        w, h = self.launchParams.frame.size
        out = np.empty((h, w), np.uint32)
        self._ck(self._L.pt_tonemap_sqrt(self._ctx, out.ctypes.data), "pt_tonemap_sqrt")
        return out

    def denoise(self, iterations=5, sigma_color=1.0, sigma_normal=0.25, sigma_albedo=0.1, input=PT_BUF_COLOR, epilogue=0):
        """OptiXDenoiser::exec() as the reference wires it (SimplePathtracer.cpp:104-105,138-146; its own body is empty): an
        a-trous filter of `input` guided by normal_buffer and albedo_buffer → PT_BUF_DENOISED; epilogue 1 = computeFinalPixelColors,
        2 = make_color into frame_buffer.  Returns (denoised float4 image, kernel ms)."""
        from ._lib import DenoiseParams

        prm = DenoiseParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_albedo), int(input), int(epilogue))
        ms = C.c_double()
        self._ck(self._L.pt_denoise(self._ctx, C.byref(prm), None, C.byref(ms)), "pt_denoise")
        return self.download(PT_BUF_DENOISED), ms.value

    def stats(self) -> dict:
        s = Stats()
        self._ck(self._L.pt_get_stats(self._ctx, C.byref(s)), "pt_get_stats")
        return s.as_dict()

    def ownedPixels(self):
        a, b = C.c_uint32(), C.c_uint32()
        self._ck(self._L.pt_owned_pixels(self._ctx, C.byref(a), C.byref(b)), "pt_owned_pixels")
        return a.value, b.value

    def deviceBuffer(self, which) -> int:
        return self._L.pt_device_buffer(self._ctx, which)

    def pack(self, which, dev_ptr: int):
        self._ck(self._L.pt_pack(self._ctx, which, dev_ptr), "pt_pack")

    def unpack(self, which, dev_ptr: int):
        self._ck(self._L.pt_unpack(self._ctx, which, dev_ptr), "pt_unpack")

    # -- display hand-off that overlaps the next frame (pt_pack_async ... pt_download_display, include/pt_amd.h)
    def packAsync(self, which, dev_ptr: int, slot: int):
        self._ck(self._L.pt_pack_async(self._ctx, which, dev_ptr, int(slot)), "pt_pack_async")

    def packWait(self, slot: int):
        self._ck(self._L.pt_pack_wait(self._ctx, int(slot)), "pt_pack_wait")

    def unpackDisplay(self, which, dev_ptr: int):
        self._ck(self._L.pt_unpack_display(self._ctx, which, dev_ptr), "pt_unpack_display")

    def displaySync(self):
        self._ck(self._L.pt_display_sync(self._ctx), "pt_display_sync")

    def downloadDisplay(self, which) -> np.ndarray:
        w, h = self.launchParams.frame.size
        out = np.empty((h, w), np.uint32) if which == PT_BUF_FRAME else np.empty((h, w, 4), np.float32)
        self._ck(self._L.pt_download_display(self._ctx, which, out.ctypes.data, out.nbytes), "pt_download_display")
        return out

    def exportBVH(self):
        """The traversal structure as the kernels see it (pt_export_bvh): (nodes uint32[num_nodes, 20], tris float32[num_tris, 12])."""
        nn, nt = C.c_uint32(), C.c_uint32()
        self._ck(self._L.pt_export_bvh(self._ctx, None, 0, None, 0, C.byref(nn), C.byref(nt)), "pt_export_bvh")
        nodes = np.empty((nn.value, 20), np.uint32)
        tris = np.empty((nt.value, 12), np.float32)
        self._ck(self._L.pt_export_bvh(self._ctx, nodes.ctypes.data, nodes.nbytes, tris.ctypes.data, tris.nbytes, None, None), "pt_export_bvh")
        return nodes, tris

    def updateMeshes(self, vertices: dict, rebuild: bool = False) -> float:
        """New vertex positions for some meshes ({mesh_index: (num_vertices, 3) array}, pt_update_meshes): the tree is refitted on the GPU,
        or rebuilt with rebuild=True.  Waits for frames in flight; restart the accumulation at subframe 0 afterwards.  Returns kernel ms."""
        ups, n, keep = _mesh_updates(vertices)
        ms = C.c_double()
        self._ck(self._L.pt_update_meshes(self._ctx, ups if n else None, n, _lib.PT_UPDATE_REBUILD if rebuild else _lib.PT_UPDATE_REFIT, C.byref(ms)), "pt_update_meshes")
        del keep
        return ms.value

    def updateMeshesDevice(self, vertices, rebuild: bool = False) -> float:
        """updateMeshes with the vertices in GPU memory (pt_update_meshes_device): {mesh_index: tensor} with CUDA float32 contiguous
        (num_vertices, 3) torch tensors on the context's device, or {mesh_index: (device pointer, num_vertices)}.  A tensor's current
        torch stream is synchronised on the host first; a raw pointer gets no synchronise: its producer must be complete, or ordered with
        waitEvent(event recorded behind it) before the call.  Non-finite coordinates are found on the GPU."""
        ups, n, keep = _device_updates(vertices, getattr(self, "_device", 0))
        ms = C.c_double()
        self._ck(self._L.pt_update_meshes_device(self._ctx, ups if n else None, n, _lib.PT_UPDATE_REBUILD if rebuild else _lib.PT_UPDATE_REFIT, C.byref(ms)),
                 "pt_update_meshes_device")
        del keep
        return ms.value

    def transformMeshes(self, transforms, from_current: bool = False, rebuild: bool = False) -> float:
        """A 3x4 (or 4x4) matrix per mesh ({mesh_index: array}, pt_transform_meshes): p' = M[:, :3] p + M[:, 3] in float32, applied to the
        mesh's rest positions — the ones last given explicitly — or with from_current=True to what is there now.  Returns kernel ms."""
        arr, n = _mesh_transforms(transforms)
        ms = C.c_double()
        self._ck(self._L.pt_transform_meshes(self._ctx, arr if n else None, n, _lib.PT_FROM_CURRENT if from_current else _lib.PT_FROM_REST,
                                             _lib.PT_UPDATE_REBUILD if rebuild else _lib.PT_UPDATE_REFIT, C.byref(ms)), "pt_transform_meshes")
        return ms.value

    def downloadVertices(self, mesh: int, rest: bool = False) -> np.ndarray:
        """The current (or rest) positions of one mesh as the context holds them: float32 (num_vertices, 3) (pt_download_vertices)."""
        if not 0 <= int(mesh) < len(self._nv):
            raise IndexError(f"downloadVertices: mesh {mesh} out of range")
        nv = self._nv[int(mesh)]
        out = np.empty((nv, 3), np.float32)
        self._ck(self._L.pt_download_vertices(self._ctx, int(mesh), int(bool(rest)), out.ctypes.data, out.nbytes), "pt_download_vertices")
        return out

    def trace(self, rays: np.ndarray, any_hit=False, iters=1):
        """optixTrace as a batch query: rays (n,8) = o.xyz,tmin,d.xyz,tmax → (t, prim) or occluded flags; + kernel ms."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = len(rays)
        t = np.empty(n, np.float32)
        prim = np.empty(n, np.int32)
        ms = C.c_double()
        self._ck(self._L.pt_trace(self._ctx, rays.ctypes.data, n, int(any_hit), t.ctypes.data, prim.ctypes.data, iters, C.byref(ms)), "pt_trace")
        return (prim.astype(np.uint8) if any_hit else (t, prim)), ms.value

    def traceDevice(self, rays, any_hit=False, out=None, wait=True):
        """optixTrace from the application's own GPU buffers (pt_trace_device): nothing touches the host.

        rays: a CUDA float32 (n, 8) torch tensor on the context's device — o.xyz, tmin, d.xyz, tmax per row, rows 32 bytes apart, any
        4-byte-aligned storage offset — or a (device pointer, n) tuple.  out: where the results go — a float32 (n, 8) tensor (closest hit:
        one 32-byte pt_hit per ray) or an int32 (n,) tensor (any_hit: 1 occluded, 0 not, -2 invalid ray), or a raw device pointer; allocated
        with torch when None.
        Returns, for a closest-hit query, a dict of typed views of `out`, no copies: t, u, v (float32 (n,)), prim, mesh (int32 (n,)), ng
        (float32 (n, 3)) and "record", the (n, 8) tensor itself; prim is -1 for a miss (t = the ray's tmax) and -2 for an invalid ray (a
        non-finite word, a direction of length zero).  For an any-hit query the int32 tensor.  None when `out` was a raw pointer.
        Ordering is on the device: for a tensor, the library's stream waits for an event recorded on torch's current stream (no host
        synchronise); with raw pointers for both rays and out nothing is waited for: their producers must be complete, or ordered with
        waitEvent(event recorded behind them) before the call.  wait=True returns when the results are complete, wait=False after
        enqueueing (several queries may be queued): torch's current stream is then made to wait for the query, so torch work enqueued
        afterwards on that stream sees the results; queryWait() waits on the host and returns the statistics (after a wait=True call
        they are in self.queryStats)."""
        torch, dev = None, getattr(self, "_device", 0)
        if isinstance(rays, tuple):
            ptr, n = int(rays[0]), int(rays[1])
        else:
            import torch

            _check_query_tensor("rays", rays, dev, torch.float32, (8,))
            ptr, n = rays.data_ptr(), rays.shape[0]
        if out is None:
            import torch

            out = torch.empty((n,) if any_hit else (n, 8), dtype=torch.int32 if any_hit else torch.float32, device=f"cuda:{dev}")
        if isinstance(out, int):
            optr = out
        else:
            import torch

            _check_query_tensor("out", out, dev, torch.int32 if any_hit else torch.float32, () if any_hit else (8,))
            if out.shape[0] != n:
                raise ValueError(f"traceDevice: out has {out.shape[0]} rows for {n} rays")
            optr = out.data_ptr()
        if torch is not None:  # the rays' producer, earlier users of `out`
            self._after_torch()
        flags = (_lib.PT_QUERY_ANY if any_hit else _lib.PT_QUERY_CLOSEST) | (0 if wait else _lib.PT_QUERY_ASYNC)
        stats = _lib.QueryStats()
        self._ck(self._L.pt_trace_device(self._ctx, ptr, n, flags, optr, C.byref(stats) if wait else None), "pt_trace_device")
        if wait:
            self.queryStats = stats.as_dict()  # of the query just completed (and of asynchronous ones that were still queued)
        if torch is not None and not wait:
            done = torch.cuda.Event()
            done.record(torch.cuda.ExternalStream(self.stream, device=dev))
            torch.cuda.current_stream(dev).wait_event(done)
        if isinstance(out, int):
            return None
        if any_hit:
            return out
        words = out.view(torch.int32)
        return dict(t=out[:, 0], u=out[:, 1], v=out[:, 2], prim=words[:, 3], mesh=words[:, 4], ng=out[:, 5:8], record=out)

    def queryWait(self) -> dict:
        """Waits for the queued traceDevice(wait=False) queries (pt_query_wait).  Returns pt_query_stats summed over the queries since the
        last wait: rays, hits, invalid_rays, stage_ms / trace_ms / attrib_ms (device time of the three kernels), state_bytes."""
        s = _lib.QueryStats()
        self._ck(self._L.pt_query_wait(self._ctx, C.byref(s)), "pt_query_wait")
        return s.as_dict()

    # ---- what the image-space passes share (renderGBuffer .. motionPlanes)
    def _bind_planes(self, fn, desc, given, widths, required=(), outputs=(), alloc=()):
        """Sets desc.<name> for every plane of `given` ({name: None, a raw device pointer or a tensor}, in the order they are checked in).
        widths: floats per pixel ((h, w) for 1, else (h, w, k)) or a whole shape; frame_rgba8 is int32 (h, w) or uint8 (h, w, 4).
        A plane of `alloc` that is None is allocated with torch, zero-filled.
        Returns {name: the tensor, None for a raw pointer or an absent plane} for the planes of `outputs`."""
        import torch

        dev = getattr(self, "_device", 0)
        w, h = self.launchParams.frame.size
        result = {}
        for name, t in given.items():
            k = widths[name]
            shape = k if isinstance(k, tuple) else (h, w) if k == 1 else (h, w, k)
            if t is None and name in alloc:
                t = torch.zeros(shape, dtype=torch.float32, device=f"cuda:{dev}")
            if t is None:
                if name in required:
                    raise ValueError(f"{fn}: {name} is required")
                ptr = None
            elif isinstance(t, int):
                ptr = t
            else:
                shapes = {torch.int32: (h, w), torch.uint8: (h, w, 4)} if name == "frame_rgba8" else {torch.float32: shape}
                _check_temporal_tensor(name, t, dev, shapes, fn)
                ptr = t.data_ptr()
            setattr(desc, name, ptr)
            if name in outputs:
                result[name] = None if t is None or isinstance(t, int) else t
        return result

    def _bind_mask(self, fn, desc, mask):
        """desc.block_mask for 8x8 blocks as renderMask takes them; returns the array, which the caller keeps until the library has returned."""
        if mask is None:
            return None
        nby, nbx = self.blockGrid()
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        if m.size != nby * nbx:
            raise ValueError(f"{fn}: the mask needs {nby} x {nbx} entries, got {m.size}")
        desc.block_mask = m.ctypes.data
        return m

    @staticmethod
    def _bind_prev_cameras(desc, prev_cameras):
        """desc.prev_cameras for one Camera, one (12,) row or one per view; returns the rows, which the caller keeps as it keeps a mask."""
        if prev_cameras is None:
            return None
        if isinstance(prev_cameras, Camera) or (len(prev_cameras) == 12 and not isinstance(prev_cameras[0], Camera) and np.ndim(prev_cameras) == 1):
            prev_cameras = [prev_cameras]  # one camera, or one (12,) row
        rows = _camera_rows(prev_cameras)
        desc.prev_cameras = rows.ctypes.data
        desc.num_prev_cameras = rows.shape[0]
        return rows

    def _after_torch(self):
        """What torch enqueued so far on its current stream (the producers of the planes, a fill of the outputs) comes first, on the device."""
        import torch

        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(getattr(self, "_device", 0)))
        self.waitEvent(ev.cuda_event)

    def _run_pass(self, cname, desc, stats, result):
        self._after_torch()
        self._ck(getattr(self._L, cname)(self._ctx, C.byref(desc), C.byref(stats)), cname)
        result["stats"] = stats.as_dict()
        return result

    def renderGBuffer(self, planes=("hit",), prev_cameras=None, mask=None, out=None) -> dict:
        """The first hit under the centre of every pixel, written by one kernel into GPU tensors (pt_render_gbuffer, include/pt_amd.h).

        planes: any of "hit" (h, w, 8: one 32-byte pt_hit per pixel), "depth" (h, w), "position" (h, w, 4), "motion" (h, w, 2) and "ray"
        (h, w, 8), float32.  out: {plane: tensor} for planes the caller owns — CUDA float32 tensors of those shapes on the context's device,
        dense, any 4-byte-aligned storage offset — or raw device pointers; the others are allocated with torch, zero-filled (pixels outside
        the views, the mask or the rank's partition are not written).  prev_cameras, needed by "motion": the previous frame's camera — one
        Camera or (12,) row eye, U, V, W without views, else one per view as setViewCameras takes them.  mask: 8x8 blocks as renderMask
        takes them, None = every block.
        Ordering is on the device: the library's stream waits for what torch has enqueued on its current stream; the call returns when
        the planes are complete.  The frame buffers, the accumulation and the path state are left alone.
        Returns {plane: tensor (None for a raw pointer), ..., "stats": {pixels, hits, kernel_ms}}."""
        planes = tuple(planes)
        out = dict(out or {})
        for name in list(planes) + list(out):
            if name not in _lib.GBUFFER_PLANES:
                raise ValueError(f"renderGBuffer: unknown plane {name!r} (one of {', '.join(_lib.GBUFFER_PLANES)})")
        if any(name not in planes for name in out):
            raise ValueError("renderGBuffer: `out` names a plane that `planes` does not")
        desc = _lib.GBufferDesc()
        result = self._bind_planes("renderGBuffer", desc, {name: out.get(name) for name in planes}, _lib.GBUFFER_PLANES, outputs=planes, alloc=planes)
        rows = self._bind_prev_cameras(desc, prev_cameras)  # noqa: F841 (kept until the call has returned, as m is)
        m = self._bind_mask("renderGBuffer", desc, mask)  # noqa: F841
        return self._run_pass("pt_render_gbuffer", desc, _lib.GBufferStats(), result)

    def temporalAccumulate(self, color, motion, hit, position, prev_hit, prev_position, history_in, length_in, history_out=None, length_out=None,
                           frame_rgba8=None, copy_out=None, mask=None, color_scale=1.0, normal_cos=0.9, plane_eps=0.01, min_weight=0.25,
                           max_history=32, clear_color=False) -> dict:
        """Reprojects last frame's accumulated colour along the motion plane, keeps it where it is the same surface and blends this frame's
        colour in with a per-pixel history length (pt_temporal_accumulate, include/pt_amd.h: the arithmetic, in full).

        Every plane is a CUDA tensor on the context's device — float32 (h, w, k), dense, any 4-byte-aligned storage offset — or a raw
        device pointer (deviceBuffer(PT_BUF_ACCUM) as `color`, deviceBuffer(PT_BUF_COLOR) as `copy_out`): color (k = 4; read, and zeroed
        afterwards with clear_color), motion (2), hit and position (8, 4: renderGBuffer's planes of this frame), prev_hit and prev_position
        (last frame's), history_in (4) and length_in ((h, w)): what the previous call returned.  history_out and length_out are allocated
        with torch, zero-filled, when None (pixels outside the views, the mask or the rank's partition are not written); they may overlap
        no other plane, so a loop ping-pongs two pairs.  frame_rgba8 (int32 (h, w) or uint8 (h, w, 4)) and copy_out (4) are optional.
        mask: 8x8 blocks as renderMask takes them, None = every block.
        Ordering is on the device: the library's stream waits for what torch has enqueued on its current stream; the call returns when
        the outputs are complete.  The frame buffers, the accumulation and the path state are left alone (unless passed in as planes).
        Returns {"history_out", "length_out", "frame_rgba8", "copy_out": the tensor (None for a raw pointer or an absent plane),
        "stats": {pixels, reprojected, kernel_ms}}."""
        given = dict(color=color, motion=motion, hit=hit, position=position, prev_hit=prev_hit, prev_position=prev_position, history_in=history_in,
                     length_in=length_in, history_out=history_out, length_out=length_out, frame_rgba8=frame_rgba8, copy_out=copy_out)
        desc = _lib.TemporalDesc()
        result = self._bind_planes("temporalAccumulate", desc, given, _lib.TEMPORAL_PLANES, set(given) - {"frame_rgba8", "copy_out"}, _lib.TEMPORAL_OUTPUTS,
                                   alloc=("history_out", "length_out"))
        m = self._bind_mask("temporalAccumulate", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.color_scale, desc.normal_cos, desc.plane_eps, desc.min_weight = float(color_scale), float(normal_cos), float(plane_eps), float(min_weight)
        if not 0 <= int(max_history) < 2**32:
            raise ValueError("temporalAccumulate: max_history must be in [1,65535]")
        desc.max_history = int(max_history)
        desc.flags = _lib.PT_TEMPORAL_CLEAR_COLOR if clear_color else 0
        return self._run_pass("pt_temporal_accumulate", desc, _lib.TemporalStats(), result)

    def filterPlanes(self, color, hit, position, variance=None, length=None, out=None, scratch=None, frame=None, mask=None, iterations=5,
                     sigma_lum=4.0, normal_cos=0.9, plane_eps=0.01, min_length=4) -> dict:
        """The chain's filter: a variance-guided a-trous filter over the G-buffer's exact planes, per view and on the pixel set of the mask
        (pt_filter_planes, include/pt_amd.h: the arithmetic, in full).

        Every plane is a CUDA tensor on the context's device — float32, dense, any 4-byte-aligned storage offset — or a raw device
        pointer (deviceBuffer(PT_BUF_COLOR) as `color`, deviceBuffer(PT_BUF_DENOISED) as `out`): color (h, w, 4), hit (h, w, 8) and
        position (h, w, 4) (renderGBuffer's planes of this frame), variance and length ((h, w), optional: without a variance, and where
        length < min_length, the variance is estimated over a 7x7 window).  out and scratch (h, w, 4) are allocated with torch,
        zero-filled, when None (scratch only when iterations >= 1); pixels outside the views, the mask or the rank's partition are not
        written.  frame (int32 (h, w) or uint8 (h, w, 4)) is optional.  mask: 8x8 blocks as renderMask takes them, None = every block.
        Ordering is on the device: the library's stream waits for what torch has enqueued on its current stream; the call returns when
        the outputs are complete.  The frame buffers, the accumulation and the path state are left alone (unless passed in as planes).
        Returns {"out", "scratch", "frame_rgba8": the tensor (None for a raw pointer or an absent plane), "stats": {pixels, filtered,
        spatial, kernel_ms}}."""
        if not 0 <= int(iterations) <= 6:
            raise ValueError("filterPlanes: iterations must be in [0,6]")
        given = dict(color=color, hit=hit, position=position, variance=variance, length=length, out=out, scratch=scratch, frame_rgba8=frame)
        desc = _lib.FilterDesc()
        result = self._bind_planes("filterPlanes", desc, given, _lib.FILTER_PLANES, ("color", "hit", "position"), _lib.FILTER_OUTPUTS,
                                   alloc=("out", "scratch") if int(iterations) >= 1 else ("out",))
        m = self._bind_mask("filterPlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.iterations = int(iterations)
        desc.sigma_lum, desc.normal_cos, desc.plane_eps = float(sigma_lum), float(normal_cos), float(plane_eps)
        if not 0 <= int(min_length) < 2**32:
            raise ValueError("filterPlanes: min_length must be in [0,65535]")
        desc.min_length = int(min_length)
        desc.flags = 0
        return self._run_pass("pt_filter_planes", desc, _lib.FilterStats(), result)

    def upsamplePlanes(self, lo_color, lo_hit, lo_position, hit, position, scale, out=None, weight_out=None, mask=None, normal_cos=0.9,
                       plane_eps=0.01) -> dict:
        """Guided upsampling: brings a low-resolution colour plane to this renderer's resolution with a joint-bilateral rule over both
        G-buffers — mesh, normal and plane distance, the tests of temporalAccumulate and filterPlanes — per view and on the pixel set of the
        mask (pt_upsample_planes, include/pt_amd.h: the arithmetic, in full).  Called on the FULL-size renderer.

        Every plane is a CUDA tensor on the context's device — float32, dense, any 4-byte-aligned storage offset — or a raw device
        pointer.  lo_color (h/scale, w/scale, 4), lo_hit (.., 8) and lo_position (.., 4) come from a second renderer of that size over
        the same model (its filterPlanes out, its renderGBuffer planes of the same frame; with views, its views are this renderer's divided
        by scale); hit (h, w, 8) and position (h, w, 4) are this renderer's renderGBuffer planes.  scale is 2, 3 or 4 and divides the
        frame's size (and every view's rectangle).  out (h, w, 4) is allocated with torch, zero-filled, when None; weight_out ((h, w),
        optional) receives the bilinear stage's weight sum, 0 for a rescued pixel and -1 for an orphan; pixels outside the views, the mask
        or the rank's partition are not written.  mask: 8x8 blocks as renderMask takes them, None = every block.
        Ordering is on the device: the library's stream waits for what torch has enqueued on its current stream; the low-res renderer's
        calls are complete when they return; the call returns when the outputs are complete.  The frame buffers, the accumulation and the
        path state are left alone (unless passed in as planes).
        Returns {"out", "weight_out": the tensor (None for a raw pointer or an absent plane), "stats": {pixels, hits, full, rescued,
        orphans, kernel_ms}}."""
        s = int(scale)
        if not 2 <= s <= 4:
            raise ValueError("upsamplePlanes: scale must be in [2,4]")
        w, h = self.launchParams.frame.size
        if w % s or h % s:
            raise ValueError(f"upsamplePlanes: scale {s} does not divide the frame's {w} x {h}")
        lw, lh = w // s, h // s
        widths = dict(_lib.UPSAMPLE_PLANES, lo_color=(lh, lw, 4), lo_hit=(lh, lw, 8), lo_position=(lh, lw, 4))
        given = dict(lo_color=lo_color, lo_hit=lo_hit, lo_position=lo_position, hit=hit, position=position, out=out, weight_out=weight_out)
        desc = _lib.UpsampleDesc()
        result = self._bind_planes("upsamplePlanes", desc, given, widths, ("lo_color", "lo_hit", "lo_position", "hit", "position"), _lib.UPSAMPLE_OUTPUTS,
                                   alloc=("out",))
        m = self._bind_mask("upsamplePlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.lo_width, desc.lo_height, desc.scale = lw, lh, s
        desc.normal_cos, desc.plane_eps = float(normal_cos), float(plane_eps)
        desc.flags = 0
        return self._run_pass("pt_upsample_planes", desc, _lib.UpsampleStats(), result)

    def temporalMoments(self, color, motion, hit, position, prev_hit, prev_position, history_in, moments_in, length_in, albedo=None,
                        history_out=None, moments_out=None, length_out=None, variance_out=None, variance=True, mask=None, color_scale=1.0,
                        albedo_min=0.0, normal_cos=0.9, plane_eps=0.01, min_weight=0.25, clamp_k=None, max_history=32, clear_color=False) -> dict:
        """The SVGF temporal stage in one pass: demodulates this frame's colour by the albedo, reprojects the colour history and the
        luminance moments through one gather, optionally clamps the history to the 3x3 neighbourhood of this frame's colour, blends and
        writes the variance (pt_temporal_moments, include/pt_amd.h: the arithmetic, in full).

        Every plane is a CUDA tensor on the context's device — float32 (h, w, k), dense, any 4-byte-aligned storage offset — or a raw
        device pointer (deviceBuffer(PT_BUF_ACCUM) as `color`, deviceBuffer(PT_BUF_ALBEDO) as `albedo`): color (k = 4; zeroed afterwards
        with clear_color), albedo (4, optional), motion (2), hit and position (8, 4), prev_hit and prev_position (last frame's),
        history_in (4), moments_in (2) and length_in ((h, w)): what the previous call returned.  history_out, moments_out, length_out
        and (unless variance=False) variance_out are allocated with torch, zero-filled, when None (pixels outside the views, the mask or
        the rank's partition are not written); they may overlap no other plane, so a loop ping-pongs two sets.  clamp_k: None = no clamp,
        else the half-width of the clamp window in standard deviations.  mask: 8x8 blocks as renderMask takes them, None = every block.
        Ordering is on the device: the library's stream waits for what torch has enqueued on its current stream; the call returns when
        the outputs are complete.  The frame buffers, the accumulation and the path state are left alone (unless passed in as planes).
        Returns {"history_out", "moments_out", "length_out", "variance_out": the tensor (None for a raw pointer or an absent plane),
        "stats": {pixels, reprojected, clamped, kernel_ms}}."""
        given = dict(color=color, albedo=albedo, motion=motion, hit=hit, position=position, prev_hit=prev_hit, prev_position=prev_position,
                     history_in=history_in, moments_in=moments_in, length_in=length_in, history_out=history_out, moments_out=moments_out,
                     length_out=length_out, variance_out=variance_out)
        desc = _lib.TMomDesc()
        result = self._bind_planes("temporalMoments", desc, given, _lib.TMOM_PLANES, set(given) - {"albedo", "variance_out"}, _lib.TMOM_OUTPUTS,
                                   alloc=_lib.TMOM_OUTPUTS if variance else _lib.TMOM_OUTPUTS[:3])
        m = self._bind_mask("temporalMoments", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.color_scale, desc.albedo_min = float(color_scale), float(albedo_min)
        desc.normal_cos, desc.plane_eps, desc.min_weight = float(normal_cos), float(plane_eps), float(min_weight)
        desc.clamp_k = 0.0 if clamp_k is None else float(clamp_k)
        if not 0 <= int(max_history) < 2**32:
            raise ValueError("temporalMoments: max_history must be in [1,65535]")
        desc.max_history = int(max_history)
        desc.flags = (_lib.PT_TMOM_CLEAR_COLOR if clear_color else 0) | (_lib.PT_TMOM_CLAMP if clamp_k is not None else 0)
        return self._run_pass("pt_temporal_moments", desc, _lib.TMomStats(), result)

    def modulatePlanes(self, color, albedo=None, out=None, frame=None, mask=None, albedo_min=0.0, write_out=True) -> dict:
        """The end of the chain: multiplies the albedo back into a demodulated colour plane (pt_modulate_planes, include/pt_amd.h), with the
        denominator rule of temporalMoments, and writes float colour and / or packed RGBA8.

        color (h, w, 4) and albedo (h, w, 4, optional) are CUDA float32 tensors on the context's device — dense, any 4-byte-aligned storage
        offset — or raw device pointers.  out (h, w, 4) is allocated with torch, zero-filled, when None and write_out is true; it may be
        `color` itself (in place: the pass is pixel-local) and may overlap no plane otherwise.  frame (int32 (h, w) or uint8 (h, w, 4)) is
        optional; with write_out=False it is the only output.  mask: 8x8 blocks as renderMask takes them, None = every block.
        Ordering is on the device, as temporalMoments.  Returns {"out", "frame_rgba8": the tensor (None for a raw pointer or an absent
        plane), "stats": {pixels, kernel_ms}}."""
        if out is None and not write_out and frame is None:
            raise ValueError("modulatePlanes: no output asked for (out and frame are both None)")
        given = dict(color=color, albedo=albedo, out=out, frame_rgba8=frame)
        desc = _lib.ModulateDesc()
        result = self._bind_planes("modulatePlanes", desc, given, _lib.MODULATE_PLANES, ("color",), _lib.MODULATE_OUTPUTS, alloc=("out",) if write_out else ())
        m = self._bind_mask("modulatePlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.albedo_min = float(albedo_min)
        desc.flags = 0
        return self._run_pass("pt_modulate_planes", desc, _lib.ModulateStats(), result)

    def edgeAaPlanes(self, color, hit, position, out=None, edge=None, frame=None, mask=None, normal_cos=0.9, plane_eps=0.01) -> dict:
        """Geometric edge antialiasing, the last pass before display: where a pixel and one of its four neighbours show different surfaces,
        the nearer surface's triangle edge is located between the two pixel centres from the hit plane, the current vertices and the
        pixel's camera, and the pixel takes the matching share of that neighbour's colour (pt_edge_aa_planes, include/pt_amd.h: the rule,
        in full).  Stateless: no jitter, no history.

        color (h, w, 4: modulatePlanes's out), hit (h, w, 8) and position (h, w, 4) (renderGBuffer's planes of this frame) are CUDA float32
        tensors on the context's device — dense, any 4-byte-aligned storage offset — or raw device pointers.  out (h, w, 4) is allocated
        with torch, zero-filled, when None; it may NOT be `color` (the pass reads neighbours).  edge ((h, w, 2), optional) receives the
        blend weight and the direction code 1..4 (0, 0 where nothing was blended); frame (int32 (h, w) or uint8 (h, w, 4)) is optional.
        Pixels outside the views, the mask or the rank's partition are not written, and a neighbour there never counts.  mask: 8x8 blocks
        as renderMask takes them, None = every block.  normal_cos, plane_eps: the chain's "same surface" test, as filterPlanes.
        Ordering is on the device, as temporalMoments.  Returns {"out", "edge", "frame_rgba8": the tensor (None for a raw pointer or an
        absent plane), "stats": {pixels, hits, stale, boundary, blended, kernel_ms}}."""
        given = dict(color=color, hit=hit, position=position, out=out, edge=edge, frame_rgba8=frame)
        desc = _lib.EdgeAaDesc()
        result = self._bind_planes("edgeAaPlanes", desc, given, _lib.EDGE_AA_PLANES, ("color", "hit", "position"), _lib.EDGE_AA_OUTPUTS, alloc=("out",))
        m = self._bind_mask("edgeAaPlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.normal_cos, desc.plane_eps = float(normal_cos), float(plane_eps)
        desc.flags = 0
        return self._run_pass("pt_edge_aa_planes", desc, _lib.EdgeAaStats(), result)

    def _view_count(self):
        """max(1, the view count): how many rectangles, cameras and per-view words a pass works with"""
        count = C.c_uint32(0)
        if getattr(self, "_ctx", None):
            self._L.pt_get_views(self._ctx, None, 0, C.byref(count))
        return max(1, count.value)

    def _view_words(self, fn, name, t, dtype, width, alloc=False):
        """A per-view array of pt_exposure_planes / pt_tonemap_planes: (max(1, views), width) of dtype, a tensor, a raw pointer or None."""
        import torch

        dev = getattr(self, "_device", 0)
        nv = self._view_count()
        if t is None and alloc:
            t = torch.zeros((nv, width), dtype=dtype, device=f"cuda:{dev}")
        if t is None or isinstance(t, int):
            return t, None
        _check_temporal_tensor(name, t, dev, {dtype: (nv, width)}, fn)
        return t.data_ptr(), t

    def exposurePlanes(self, color=None, hit=None, hist=None, state_in=None, state_out=None, mask=None, low_permille=50, high_permille=20,
                       key_log2=-2.4739312, ev_min=-16.0, ev_max=16.0, rate_up=1.0, rate_down=1.0, accumulate=False, from_histogram=False) -> dict:
        """Auto exposure: meters `color` into a histogram of log2 luminance per view (eight bins a stop, integer counts) and adapts an
        exposure per view from its trimmed mean (pt_exposure_planes, include/pt_amd.h: the rule, in full).  Stateless: the caller keeps
        hist and the state.

        color (h, w, 4) and hit ((h, w, 8), optional: misses are not metered) are CUDA float32 tensors or raw device pointers.  hist is an
        int32 (views, 256) tensor and state_in / state_out float32 (views, 4) tensors (ev, E = 2^ev, mean log2 luminance, pixels metered)
        with views = max(1, the view count), or raw pointers; hist and state_out are allocated when None; state_out may be state_in.
        accumulate: hist is not zeroed first.  from_histogram: no metering, hist is read as given (the all-reduced histogram of a
        partitioned frame); color, hit and mask must then be None.  tonemapPlanes reads state_out on the device.
        Returns {"hist", "state_out": the tensor (None for a raw pointer), "stats": {pixels, skipped, nonfinite, under, over, kernel_ms}}."""
        import torch

        desc = _lib.ExposureDesc()
        self._bind_planes("exposurePlanes", desc, dict(color=color, hit=hit), _lib.EXPOSURE_PLANES, () if from_histogram else ("color",))
        desc.hist, th = self._view_words("exposurePlanes", "hist", hist, torch.int32, _lib.PT_EXPOSURE_BINS, alloc=True)
        desc.state_in, _ = self._view_words("exposurePlanes", "state_in", state_in, torch.float32, 4)
        desc.state_out, ts = self._view_words("exposurePlanes", "state_out", state_out, torch.float32, 4, alloc=True)
        m = self._bind_mask("exposurePlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.low_permille, desc.high_permille = int(low_permille), int(high_permille)
        desc.key_log2, desc.ev_min, desc.ev_max = float(key_log2), float(ev_min), float(ev_max)
        desc.rate_up, desc.rate_down = float(rate_up), float(rate_down)
        desc.flags = (_lib.PT_EXPOSURE_ACCUMULATE if accumulate else 0) | (_lib.PT_EXPOSURE_FROM_HISTOGRAM if from_histogram else 0)
        return self._run_pass("pt_exposure_planes", desc, _lib.ExposureStats(), dict(hist=th, state_out=ts))

    def tonemapPlanes(self, color, state=None, out=None, frame=None, mask=None, op="aces", exposure=1.0, white=1.0, write_out=True) -> dict:
        """The display operator under the metered exposure (pt_tonemap_planes, include/pt_amd.h): per pixel the colour times its view's
        E (state[view][1], read on the device; 1 when state is None) times `exposure`, clamped to [0, 65504], through op — "linear",
        "reinhard" (the frame path's operator, with `white`) or "aces" (Narkowicz's fit) — into out (h, w, 4; may be `color` itself;
        allocated when None and write_out) and / or frame (int32 (h, w) or uint8 (h, w, 4): sRGB, 8 bits).
        Returns {"out", "frame_rgba8": the tensor (None for a raw pointer or an absent plane), "stats": {pixels, clipped, kernel_ms}}."""
        import torch

        if op not in _lib.TONEMAP_OPS:
            raise ValueError(f"tonemapPlanes: unknown operator {op!r} (one of {', '.join(_lib.TONEMAP_OPS)})")
        if out is None and frame is None and not write_out:
            raise ValueError("tonemapPlanes: no output asked for (out and frame are both None)")
        given = dict(color=color, out=out, frame_rgba8=frame)
        desc = _lib.TonemapDesc()
        result = self._bind_planes("tonemapPlanes", desc, given, _lib.TONEMAP_PLANES, ("color",), _lib.TONEMAP_OUTPUTS, alloc=("out",) if write_out else ())
        desc.state, _ = self._view_words("tonemapPlanes", "state", state, torch.float32, 4)
        m = self._bind_mask("tonemapPlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.exposure, desc.white, desc.op, desc.flags = float(exposure), float(white), _lib.TONEMAP_OPS[op], 0
        return self._run_pass("pt_tonemap_planes", desc, _lib.TonemapStats(), result)

    def _bind_scratch(self, fn, desc, result, scratch, shape):
        """desc.scratch and result["scratch"] of a pass with a scratch plane: a raw pointer as it is, or a float32 tensor of shape() — the
        pass's layout, asked for only then — allocated when None."""
        import torch

        if isinstance(scratch, int):
            desc.scratch, result["scratch"] = scratch, None
            return
        dev = getattr(self, "_device", 0)
        shape = shape()
        if scratch is None:
            scratch = torch.empty(shape, dtype=torch.float32, device=f"cuda:{dev}")
        _check_temporal_tensor("scratch", scratch, dev, {torch.float32: shape}, fn)
        desc.scratch, result["scratch"] = scratch.data_ptr(), scratch

    def _tile_layout(self, cname):
        """(dims, bytes) of a tiled pass's scratch: motionBlurLayout and dofLayout"""
        nbytes = C.c_size_t()
        dims = np.zeros((self._view_count(), 4), np.uint32)
        self._ck(getattr(self._L, cname)(self._ctx, dims.ctypes.data, C.byref(nbytes)), cname)
        return dims, nbytes.value

    def bloomLayout(self, levels=6):
        """The shape of bloomPlanes's scratch pyramid (pt_bloom_layout): (dims, bytes) with dims a uint32 (views, 8, 4) array of w, h, the
        index of the level's first 16-byte texel and 0 per level (zeros above `levels`), views = max(1, the view count), and bytes the
        size of the scratch for `levels` levels of every view."""
        levels = int(levels)
        if not 1 <= levels <= _lib.PT_BLOOM_MAX_LEVELS:
            raise ValueError(f"bloomLayout: levels must be 1..{_lib.PT_BLOOM_MAX_LEVELS}, not {levels}")
        nbytes = C.c_size_t()
        dims = np.zeros((self._view_count(), _lib.PT_BLOOM_MAX_LEVELS, 4), np.uint32)
        self._ck(self._L.pt_bloom_layout(self._ctx, levels, dims.ctypes.data, C.byref(nbytes)), "pt_bloom_layout")
        return dims, nbytes.value

    def bloomPlanes(self, color, state=None, out=None, scratch=None, mask=None, exposure=1.0, threshold=1.0, knee=0.5, clamp=65504.0,
                    spread=0.7, intensity=0.25, levels=6) -> dict:
        """Bloom in front of the tone mapper (pt_bloom_planes, include/pt_amd.h: the rule, in full): the part of `color` whose exposed
        luminance lies above `threshold` (soft over `knee`, the source clamped to `clamp`) is filtered down a pyramid of `levels` levels
        per view and back up, each coarser level weighing `spread` of the next finer one, and added to the colour: out = color +
        intensity * bloom, scene-linear, for tonemapPlanes with the same state.

        color (h, w, 4) is a CUDA float32 tensor or a raw device pointer; state as tonemapPlanes takes it (the exposure is read on the
        device; 1 when None).  out (h, w, 4) may be `color` itself; allocated when None.  scratch: a float32 (texels, 4) tensor with
        16 * texels = bloomLayout(levels)'s bytes, 16-byte aligned, or a raw pointer; allocated when None.  After the call it holds the
        pyramid U_1 .. U_levels of every view.  The pyramid reads every pixel of every view whatever the mask and the rank's partition:
        they decide only which pixels of out are written (a partitioned frame gathers its colour first).
        Returns {"out", "scratch": the tensor (None for a raw pointer), "stats": {pixels, sources, bright, nonfinite, kernel_ms}}."""
        import torch

        levels = int(levels)
        if not 1 <= levels <= _lib.PT_BLOOM_MAX_LEVELS:
            raise ValueError(f"bloomPlanes: levels must be 1..{_lib.PT_BLOOM_MAX_LEVELS}, not {levels}")
        desc = _lib.BloomDesc()
        result = self._bind_planes("bloomPlanes", desc, dict(color=color, out=out), _lib.BLOOM_PLANES, ("color",), _lib.BLOOM_OUTPUTS, alloc=("out",))
        desc.state, _ = self._view_words("bloomPlanes", "state", state, torch.float32, 4)
        self._bind_scratch("bloomPlanes", desc, result, scratch, lambda: (self.bloomLayout(levels)[1] // 16, 4))
        m = self._bind_mask("bloomPlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.exposure, desc.threshold, desc.knee, desc.clamp = float(exposure), float(threshold), float(knee), float(clamp)
        desc.spread, desc.intensity, desc.levels, desc.flags = float(spread), float(intensity), levels, 0
        return self._run_pass("pt_bloom_planes", desc, _lib.BloomStats(), result)

    def motionBlurLayout(self):
        """The shape of motionBlurPlanes's scratch (pt_motion_blur_layout): (dims, bytes) with dims a uint32 (views, 4) array of tw, th, the
        index of T's first 8-byte texel and the index of N's, views = max(1, the view count), and bytes the size of the scratch."""
        return self._tile_layout("pt_motion_blur_layout")

    def motionBlurPlanes(self, color, motion, depth, out=None, scratch=None, mask=None, shutter=0.5, max_blur=16.0, depth_soft=0.05, taps=12,
                         seed=0, jitter=False) -> dict:
        """Motion blur behind edgeAaPlanes / bloomPlanes and in front of tonemapPlanes (pt_motion_blur_planes, include/pt_amd.h: the rule,
        in full): each pixel of `color` is blurred along the fastest motion of the 16 x 16 tiles around it — `shutter` of the frame
        interval, centred on the current position, at most `max_blur` pixels to either side — by a depth-aware gather of `taps` pixels.

        color (h, w, 4), motion ((h, w, 2): renderGBuffer's or motionPlanes's) and depth ((h, w): renderGBuffer's) are CUDA float32 tensors
        on the context's device — dense, any 4-byte-aligned storage offset — or raw device pointers.  out (h, w, 4) is allocated with
        torch, zero-filled, when None; it may NOT be `color` (the pass reads neighbours).  scratch: a float32 (texels, 2) tensor with
        8 * texels = motionBlurLayout()'s bytes, 8-byte aligned, or a raw pointer; allocated when None.  After the call it holds the tile
        maxima T and the neighbourhood maxima N of every view.  The tile pass reads every pixel of every view whatever the mask and the
        rank's partition: they decide only which pixels of out are written (a partitioned frame gathers its three planes first).
        jitter: each pixel's taps are shifted by a hash of its coordinates and `seed`.
        Returns {"out", "scratch": the tensor (None for a raw pointer), "stats": {pixels, sources, unknown, moving, taps, nonfinite,
        kernel_ms}}."""
        taps, seed = int(taps), int(seed)
        if not 1 <= taps <= 64:
            raise ValueError(f"motionBlurPlanes: taps must be 1..64, not {taps}")
        if not 0 <= seed < 2**32:
            raise ValueError("motionBlurPlanes: seed must be in [0,4294967295]")
        if not 0.0 <= float(shutter) <= 4.0:
            raise ValueError("motionBlurPlanes: shutter must be in [0,4]")
        if not 1.0 <= float(max_blur) <= _lib.PT_MOTION_BLUR_TILE:
            raise ValueError(f"motionBlurPlanes: max_blur must be in [1,{_lib.PT_MOTION_BLUR_TILE}]")
        if not 0.0 < float(depth_soft) <= 1.0:
            raise ValueError("motionBlurPlanes: depth_soft must be in (0,1]")
        desc = _lib.MotionBlurDesc()
        result = self._bind_planes("motionBlurPlanes", desc, dict(color=color, motion=motion, depth=depth, out=out), _lib.MOTION_BLUR_PLANES,
                                   ("color", "motion", "depth"), _lib.MOTION_BLUR_OUTPUTS, alloc=("out",))
        self._bind_scratch("motionBlurPlanes", desc, result, scratch, lambda: (self.motionBlurLayout()[1] // 8, 2))
        m = self._bind_mask("motionBlurPlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.shutter, desc.max_blur, desc.depth_soft = float(shutter), float(max_blur), float(depth_soft)
        desc.taps, desc.seed, desc.flags = taps, seed, _lib.PT_MOTION_BLUR_JITTER if jitter else 0
        return self._run_pass("pt_motion_blur_planes", desc, _lib.MotionBlurStats(), result)

    @staticmethod
    def dofAperture(focal_length, f_number, focus, sensor_height, frame_height):
        """dofPlanes's `aperture` of a thin lens: K = 0.5 * A * f / (s - f) * px_per_unit, the blur-circle radius in pixels of a point at
        infinity, with A = focal_length / f_number the aperture's diameter, f = focal_length, s = focus (all three in the depth plane's
        units, s > f) and px_per_unit = frame_height / sensor_height (sensor_height in the same units)."""
        f, n, s, sensor, h = float(focal_length), float(f_number), float(focus), float(sensor_height), float(frame_height)
        if not (f > 0.0 and n > 0.0 and sensor > 0.0 and h > 0.0 and s > f):
            raise ValueError("dofAperture: focal_length, f_number, sensor_height and frame_height must be > 0 and focus > focal_length")
        return 0.5 * (f / n) * f / (s - f) * (h / sensor)

    def dofLayout(self):
        """The shape of dofPlanes's scratch (pt_dof_layout): (dims, bytes) with dims a uint32 (views, 4) array of tw, th, the index of T's
        first 4-byte texel and the index of N's, views = max(1, the view count), and bytes the size of the scratch."""
        return self._tile_layout("pt_dof_layout")

    def dofPlanes(self, color, depth, out=None, scratch=None, mask=None, focus=None, aperture=None, max_radius=16.0, taps=32, seed=0,
                  jitter=False, view_focus=None) -> dict:
        """Depth of field behind edgeAaPlanes and in front of bloomPlanes, motionBlurPlanes and tonemapPlanes (pt_dof_planes,
        include/pt_amd.h: the rule, in full): each pixel of `color` gathers `taps` pixels of a disc whose radius is the largest blur
        circle of the 16 x 16 tiles around it, at most `max_radius` pixels.  A pixel at depth z has the blur radius
        aperture * |1 - focus / z|: `focus` is the depth that is sharp, `aperture` the radius in pixels of a point at infinity
        (dofAperture computes it from a lens).  A tap behind the pixel is seen through the pixel's own blur, a tap in front spreads by
        its own.

        color (h, w, 4) and depth ((h, w): renderGBuffer's) are CUDA float32 tensors on the context's device — dense, any
        4-byte-aligned storage offset — or raw device pointers.  out (h, w, 4) is allocated with torch, zero-filled, when None; it may
        NOT be `color` (the pass reads neighbours).  scratch: a float32 (texels,) tensor with 4 * texels = dofLayout()'s bytes, or a raw
        pointer; allocated when None.  After the call it holds the tile maxima T and the neighbourhood maxima N of every view.  The tile
        pass reads every pixel of every view whatever the mask and the rank's partition: they decide only which pixels of out are
        written (a partitioned frame gathers its two planes first).  view_focus: a focus distance per view (max(1, the view count)
        floats), None: `focus` for all.  jitter: each pixel's pattern is turned by a hash of its coordinates and `seed`.
        Returns {"out", "scratch": the tensor (None for a raw pointer), "stats": {pixels, sources, gathered, taps, nonfinite,
        kernel_ms}}."""
        if focus is None or aperture is None:
            raise ValueError("dofPlanes: focus and aperture are required")
        taps, seed = int(taps), int(seed)
        if not 1 <= taps <= 64:
            raise ValueError(f"dofPlanes: taps must be 1..64, not {taps}")
        if not 0 <= seed < 2**32:
            raise ValueError("dofPlanes: seed must be in [0,4294967295]")
        if not 0.0 < float(focus) <= 1e30:
            raise ValueError("dofPlanes: focus must be in (0,1e30]")
        if not 0.0 <= float(aperture) <= 4096.0:
            raise ValueError("dofPlanes: aperture must be in [0,4096]")
        if not 1.0 <= float(max_radius) <= _lib.PT_DOF_TILE:
            raise ValueError(f"dofPlanes: max_radius must be in [1,{_lib.PT_DOF_TILE}]")
        desc = _lib.DofDesc()
        result = self._bind_planes("dofPlanes", desc, dict(color=color, depth=depth, out=out), _lib.DOF_PLANES, ("color", "depth"),
                                   _lib.DOF_OUTPUTS, alloc=("out",))
        self._bind_scratch("dofPlanes", desc, result, scratch, lambda: (self.dofLayout()[1] // 4,))
        vf = None
        if view_focus is not None:
            vf = np.ascontiguousarray(view_focus, np.float32).reshape(-1)
            if vf.size != self._view_count():
                raise ValueError(f"dofPlanes: view_focus has {vf.size} values, expected {self._view_count()}")
            if not ((vf > 0) & (vf <= np.float32(1e30))).all():
                raise ValueError("dofPlanes: view_focus must be in (0,1e30]")
            desc.view_focus = vf.ctypes.data  # (vf is kept until the call has returned)
        m = self._bind_mask("dofPlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.focus, desc.aperture, desc.max_radius = float(focus), float(aperture), float(max_radius)
        desc.taps, desc.seed, desc.flags = taps, seed, _lib.PT_DOF_JITTER if jitter else 0
        return self._run_pass("pt_dof_planes", desc, _lib.DofStats(), result)

    def lensWarpPlanes(self, color, out=None, frame=None, mask=None, lenses=None, border=(0.0, 0.0, 0.0), bicubic=False) -> dict:
        """The last pass of the chain, behind tonemapPlanes: lens pre-distortion with per-channel coefficients (chromatic-aberration
        correction) and rotational late reprojection for a head-mounted display, or radial distortion for a synthetic camera
        (pt_lens_warp_planes, include/pt_amd.h: the rule, in full).  Each output pixel finds, per colour channel, the source point of its
        view's lens (make_lens: a radial polynomial around the lens centre, then a 3x3 matrix in pixel coordinates, e.g. warpMatrix's) and
        resamples `color` there, bilinear or (bicubic=True) Catmull-Rom; a channel whose source point lies outside the view's rectangle
        takes `border`.

        color (h, w, 4) is a CUDA float32 tensor on the context's device — dense, any 4-byte-aligned storage offset — or a raw device
        pointer.  out (h, w, 4; .w is 1 where all three channels were inside, else 0) and frame (int32 (h, w) or uint8 (h, w, 4)) are
        optional; out is allocated with torch, zero-filled, when neither is given; neither may be `color` (the pass reads neighbours).
        lenses: one pt_lens_view per view (max(1, the view count) of them: make_lens's, or anything np.asarray turns into (views, 24)
        float32), None: no distortion and the identity matrix.  A tap reads `color` wherever in its view's rectangle it lands; the mask
        and the rank's partition decide only which pixels are written.  mask: 8x8 blocks as renderMask takes them, None = every block.
        Ordering is on the device, as temporalMoments.  Returns {"out", "frame_rgba8": the tensor (None for a raw pointer or an absent
        plane), "stats": {pixels, outside, nonfinite, kernel_ms}}."""
        given = dict(color=color, out=out, frame_rgba8=frame)
        desc = _lib.LensWarpDesc()
        result = self._bind_planes("lensWarpPlanes", desc, given, _lib.LENS_WARP_PLANES, ("color",), _lib.LENS_WARP_OUTPUTS,
                                   alloc=("out",) if frame is None else ())
        table = None
        if lenses is not None:
            if isinstance(lenses, _lib.LensView):
                lenses = [lenses]
            rows = [np.frombuffer(bytes(v), np.float32) if isinstance(v, _lib.LensView) else np.asarray(v, np.float32).reshape(-1) for v in lenses]
            if len(rows) != self._view_count() or any(r.size != 24 for r in rows):
                raise ValueError(f"lensWarpPlanes: lenses must be {self._view_count()} records of 24 floats (one pt_lens_view per view)")
            table = np.ascontiguousarray(np.stack(rows), np.float32)
            desc.lenses = table.ctypes.data  # (table is kept until the call has returned)
        border = tuple(float(b) for b in border)
        if len(border) != 3:
            raise ValueError("lensWarpPlanes: border must be three floats")
        desc.border[0], desc.border[1], desc.border[2] = border
        m = self._bind_mask("lensWarpPlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.flags = _lib.PT_LENS_WARP_BICUBIC if bicubic else 0
        return self._run_pass("pt_lens_warp_planes", desc, _lib.LensWarpStats(), result)

    def aoLayout(self, rays, max_rays_in_flight=0):
        """The size in bytes of aoPlanes's scratch (pt_ao_layout): one batch of min(floor(M / rays), frame pixels) pixels, M =
        max_rays_in_flight or the library's default (_lib.PT_AO_DEFAULT_RAYS_IN_FLIGHT) when 0."""
        nbytes = C.c_size_t()
        self._ck(self._L.pt_ao_layout(self._ctx, int(rays), int(max_rays_in_flight), C.byref(nbytes)), "pt_ao_layout")
        return nbytes.value

    def aoPlanes(self, hit, position, ao=None, out=None, bent=None, scratch=None, mask=None, rays=4, radius=None, bias=1e-3, seed=0,
                 jitter=False, max_rays_in_flight=0) -> dict:
        """Ray-traced ambient occlusion from the G-buffer (pt_ao_planes, include/pt_amd.h: the rule, in full): every pixel of a hit shoots
        `rays` any-hit rays of length `radius` (world units) over the cosine-weighted hemisphere around its geometric normal, through
        the context's current tree, from the hit position lifted by bias * hit.t along the normal.  ao is the fraction that got away
        (1 for a miss), out the same as a colour (ao, ao, ao, 1) for temporalAccumulate / filterPlanes / modulatePlanes, bent the mean
        unoccluded direction (not normalised) with ao in .w.

        hit (h, w, 8) and position (h, w, 4) are renderGBuffer's planes of this frame: CUDA float32 tensors on the context's device —
        dense, any 4-byte-aligned storage offset — or raw device pointers.  ao (h, w), out and bent (h, w, 4) are optional; out is
        allocated with torch, zero-filled, when none of the three is given.  scratch: a float32 (bytes / 4,) tensor of
        aoLayout(rays, max_rays_in_flight) bytes, 16-byte aligned, or a raw pointer; allocated when None.  The rays are traced in batches
        of at most max_rays_in_flight (0: the library's default); the result does not depend on it.  jitter: each pixel's pattern is
        turned by a hash of its coordinates and `seed` (e.g. the frame index).  mask: 8x8 blocks as renderMask takes them, None = every
        block.  Ordering is on the device, as temporalMoments.
        Returns {"ao", "out", "bent": the tensors (None for a raw pointer or an absent plane), "scratch", "stats": {pixels, traced,
        skipped, nonfinite, rays, occluded, invalid, batches, kernel_ms, trace_ms}}."""
        if radius is None:
            raise ValueError("aoPlanes: radius is required")
        rays, seed, max_rays_in_flight = int(rays), int(seed), int(max_rays_in_flight)
        if not 1 <= rays <= _lib.PT_AO_MAX_RAYS:
            raise ValueError(f"aoPlanes: rays must be 1..{_lib.PT_AO_MAX_RAYS}, not {rays}")
        if not 0 <= seed < 2**32:
            raise ValueError("aoPlanes: seed must be in [0,4294967295]")
        if not 0 <= max_rays_in_flight < 2**32 or 0 < max_rays_in_flight < rays:
            raise ValueError("aoPlanes: max_rays_in_flight must be 0 or in [rays,4294967295]")
        given = dict(hit=hit, position=position, ao=ao, out=out, bent=bent)
        desc = _lib.AoDesc()
        result = self._bind_planes("aoPlanes", desc, given, _lib.AO_PLANES, ("hit", "position"), _lib.AO_OUTPUTS,
                                   alloc=("out",) if ao is None and bent is None else ())
        self._bind_scratch("aoPlanes", desc, result, scratch, lambda: (self.aoLayout(rays, max_rays_in_flight) // 4,))
        m = self._bind_mask("aoPlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.rays, desc.max_rays_in_flight, desc.radius, desc.bias = rays, max_rays_in_flight, float(radius), float(bias)
        desc.seed, desc.flags = seed, _lib.PT_AO_JITTER if jitter else 0
        return self._run_pass("pt_ao_planes", desc, _lib.AoStats(), result)

    def reflectLayout(self, max_rays_in_flight=0):
        """The size in bytes of reflectPlanes's scratch (pt_reflect_layout): one batch of min(M, frame pixels) pixels, M = max_rays_in_flight
        or the library's default (_lib.PT_REFLECT_DEFAULT_RAYS_IN_FLIGHT) when 0."""
        nbytes = C.c_size_t()
        self._ck(self._L.pt_reflect_layout(self._ctx, int(max_rays_in_flight), C.byref(nbytes)), "pt_reflect_layout")
        return nbytes.value

    def reflectPlanes(self, hit, position, hit2=None, position2=None, ray=None, sky=None, scratch=None, mask=None, bias=1e-3,
                      max_distance=1e16, max_rays_in_flight=0) -> dict:
        """Mirror reflections from the G-buffer (pt_reflect_planes, include/pt_amd.h: the rule, in full): every pixel of a hit shoots the
        mirror image of its eye ray about the geometric normal through the context's current tree, from the hit position lifted by
        bias * hit.t along the normal, and what the ray sees is written as a second G-buffer: hit2 (h, w, 8), the pt_hit that
        traceDevice returns for that ray; position2 (h, w, 4), where it hits (.w 1; zeros where it does not); ray (h, w, 8), the ray in
        traceDevice's layout; sky (h, w, 4), the probe's radiance where the ray escapes (.w 1; zeros elsewhere; needs setProbe).
        surfacePlanes(hit=hit2), aoPlanes(hit2, position2) and every other pass that reads a hit plane work on the reflected surface.

        hit (h, w, 8) and position (h, w, 4) are renderGBuffer's planes of this frame: CUDA float32 tensors on the context's device —
        dense, any 4-byte-aligned storage offset — or raw device pointers.  The four outputs are optional; hit2 is allocated with torch,
        zero-filled, when none is given.  scratch: a float32 (bytes / 4,) tensor of reflectLayout(max_rays_in_flight) bytes, 16-byte
        aligned, or a raw pointer; allocated when None.  The rays are traced in batches of at most max_rays_in_flight (0: the library's
        default); the result does not depend on it.  max_distance is the rays' tmax (the G-buffer's 1e16 by default).  mask: 8x8 blocks
        as renderMask takes them, None = every block.  Ordering is on the device, as temporalMoments.
        Returns {"hit2", "position2", "ray", "sky": the tensors (None for a raw pointer or an absent plane), "scratch", "stats": {pixels,
        traced, skipped, nonfinite, invalid, hits, escaped, batches, kernel_ms, trace_ms}}."""
        max_rays_in_flight = int(max_rays_in_flight)
        if not 0 <= max_rays_in_flight < 2**32:
            raise ValueError("reflectPlanes: max_rays_in_flight must be in [0,4294967295]")
        given = dict(hit=hit, position=position, hit2=hit2, position2=position2, ray=ray, sky=sky)
        desc = _lib.ReflectDesc()
        result = self._bind_planes("reflectPlanes", desc, given, _lib.REFLECT_PLANES, ("hit", "position"), _lib.REFLECT_OUTPUTS,
                                   alloc=("hit2",) if position2 is None and ray is None and sky is None else ())
        self._bind_scratch("reflectPlanes", desc, result, scratch, lambda: (self.reflectLayout(max_rays_in_flight) // 4,))
        m = self._bind_mask("reflectPlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.bias, desc.max_distance, desc.max_rays_in_flight, desc.flags = float(bias), float(max_distance), max_rays_in_flight, 0
        return self._run_pass("pt_reflect_planes", desc, _lib.ReflectStats(), result)

    @staticmethod
    def _shadow_lights(fn, lights, max_rays_in_flight=0):
        """The ctypes array of `lights`: _lib.ShadowLight records or dicts / sequences of (dir, spread, radiance, rays), or one of them
        alone; checks the counts"""
        # one (dir, spread, radiance, rays) tuple, not four lights: its second item is a number
        lone_tuple = isinstance(lights, (tuple, list)) and len(lights) == 4 and isinstance(lights[1], (int, float, np.floating, np.integer))
        if isinstance(lights, (_lib.ShadowLight, dict)) or lone_tuple:
            lights = [lights]
        lights = list(lights) if lights is not None else []
        if not 1 <= len(lights) <= _lib.PT_SHADOW_MAX_LIGHTS:
            raise ValueError(f"{fn}: 1..{_lib.PT_SHADOW_MAX_LIGHTS} lights are expected, not {len(lights)}")
        arr = (_lib.ShadowLight * len(lights))()
        for i, l in enumerate(lights):
            if isinstance(l, _lib.ShadowLight):
                d, spread, rad, rays = tuple(l.dir), l.spread, tuple(l.radiance), l.rays
            elif isinstance(l, dict):
                d, spread, rad, rays = l["dir"], l.get("spread", 0.0), l.get("radiance", (1.0, 1.0, 1.0)), l.get("rays", 1)
            else:
                d, spread, rad, rays = l
            d, rad, rays = tuple(float(v) for v in d), tuple(float(v) for v in rad), int(rays)
            if len(d) != 3 or len(rad) != 3:
                raise ValueError(f"{fn}: light {i}: dir and radiance must be three floats")
            if not 1 <= rays < 2**32:
                raise ValueError(f"{fn}: light {i}: rays must be >= 1, not {rays}")
            arr[i].dir[:], arr[i].spread, arr[i].radiance[:], arr[i].rays = d, float(spread), rad, rays
        total = sum(l.rays for l in arr)
        if total > _lib.PT_SHADOW_MAX_RAYS:
            raise ValueError(f"{fn}: the lights' rays add up to {total}, above {_lib.PT_SHADOW_MAX_RAYS}")
        max_rays_in_flight = int(max_rays_in_flight)
        if not 0 <= max_rays_in_flight < 2**32 or 0 < max_rays_in_flight < total:
            raise ValueError(f"{fn}: max_rays_in_flight must be 0 or in [the lights' rays,4294967295]")
        return arr

    def shadowLayout(self, lights, max_rays_in_flight=0):
        """The size in bytes of shadowPlanes's scratch (pt_shadow_layout): one batch of min(floor(M / R), frame pixels) pixels, R the sum of
        the lights' rays, M = max_rays_in_flight or the library's default (_lib.PT_SHADOW_DEFAULT_RAYS_IN_FLIGHT) when 0."""
        arr = self._shadow_lights("shadowLayout", lights, max_rays_in_flight)
        nbytes = C.c_size_t()
        self._ck(self._L.pt_shadow_layout(self._ctx, arr, len(arr), int(max_rays_in_flight), C.byref(nbytes)), "pt_shadow_layout")
        return nbytes.value

    def shadowPlanes(self, hit, position, lights=None, view_ray=None, visibility=None, light=None, scratch=None, mask=None,
                     max_distance=1e16, bias=1e-3, seed=0, jitter=False, max_rays_in_flight=0) -> dict:
        """Shadows and direct light of up to four distant disc lights from the G-buffer (pt_shadow_planes, include/pt_amd.h: the rule, in
        full).  lights: 1..4 of _lib.ShadowLight, dict(dir=, spread=, radiance=, rays=) or (dir, spread, radiance, rays): `dir` points
        towards the light, `spread` is the tangent of the disc's angular radius (0: a point at infinity), `rays` the any-hit rays a pixel
        shoots at it; the rays of all lights add up to at most 32.  Every pixel of a hit shoots them, for each light above its horizon,
        through the context's current tree, from the hit position lifted by bias * hit.t along the normal.  visibility (h, w, 4) holds the
        open fraction per light (1 for an absent light and for a miss), light (h, w, 4) the sum of radiance * cosine * visibility with 1
        in .w: what modulatePlanes multiplies by an albedo.

        hit (h, w, 8) and position (h, w, 4) are renderGBuffer's planes of this frame, or reflectPlanes's hit2 and position2 with
        view_ray = its `ray` plane (h, w, 8), whose origin then stands in for the eye: CUDA float32 tensors on the context's device —
        dense, any 4-byte-aligned storage offset — or raw device pointers.  light is allocated with torch, zero-filled, when neither
        output is given.  scratch: a float32 (bytes / 4,) tensor of shadowLayout(lights, max_rays_in_flight) bytes, 16-byte aligned, or a
        raw pointer; allocated when None.  The rays are traced in batches of at most max_rays_in_flight (0: the library's default); the
        result does not depend on it.  jitter: each pixel's pattern is turned by a hash of its coordinates, `seed` and the light's index.
        mask: 8x8 blocks as renderMask takes them, None = every block.  Ordering is on the device, as temporalMoments.
        Returns {"visibility", "light": the tensors (None for a raw pointer or an absent plane), "scratch", "stats": {pixels, traced,
        skipped, nonfinite, backfacing, rays, occluded, invalid, batches, kernel_ms, trace_ms}}."""
        if lights is None:
            raise ValueError("shadowPlanes: lights is required")
        seed = int(seed)
        if not 0 <= seed < 2**32:
            raise ValueError("shadowPlanes: seed must be in [0,4294967295]")
        arr = self._shadow_lights("shadowPlanes", lights, max_rays_in_flight)
        given = dict(hit=hit, position=position, view_ray=view_ray, visibility=visibility, light=light)
        desc = _lib.ShadowDesc()
        result = self._bind_planes("shadowPlanes", desc, given, _lib.SHADOW_PLANES, ("hit", "position"), _lib.SHADOW_OUTPUTS,
                                   alloc=("light",) if visibility is None else ())
        self._bind_scratch("shadowPlanes", desc, result, scratch, lambda: (self.shadowLayout(arr, max_rays_in_flight) // 4,))
        m = self._bind_mask("shadowPlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.lights, desc.num_lights = C.addressof(arr), len(arr)  # (arr is kept until the call has returned)
        desc.max_rays_in_flight, desc.max_distance, desc.bias = int(max_rays_in_flight), float(max_distance), float(bias)
        desc.seed, desc.flags = seed, _lib.PT_SHADOW_JITTER if jitter else 0
        return self._run_pass("pt_shadow_planes", desc, _lib.ShadowStats(), result)

    def samplePlan(self, motion, hit, position, prev_hit, prev_position, history_in, moments_in, length_in, mask=None, normal_cos=0.9,
                   plane_eps=0.01, min_weight=0.25, threshold=0.05, dark_floor=0.01, min_length=4, min_pixels=4, refresh_period=0,
                   frame_index=0) -> dict:
        """Which 8x8 blocks of the coming frame need new samples (pt_sample_plan, include/pt_amd.h: the rule, in full): a block is sampled
        when the reprojection of the history loses one of its pixels, when at least min_pixels of them have a history shorter than
        min_length or reprojected luminance moments that still miss `threshold` (renderAdaptive's rule per pixel, with the history length
        in place of the subframe count), or when the refresh (every refresh_period frames, by frame_index) names it.

        The eight planes are temporalMoments's — motion, hit, position (renderGBuffer's of this frame), prev_hit, prev_position (last
        frame's), history_in, moments_in, length_in (what last frame's temporalMoments and temporalCarry left) — as CUDA float32 tensors
        on the context's device (dense, any 4-byte-aligned storage offset) or raw device pointers; none is written.  mask: 8x8 blocks as
        renderMask takes them, None = every block; a block outside it is never sampled.
        Ordering is on the device: the library's stream waits for what torch has enqueued on its current stream; the call returns when
        the plan is complete.  Returns {"mask": uint8 (nby, nbx), what renderMask and the passes' `mask` take (its complement, within the
        input mask, is temporalCarry's), "stats": {blocks, sampled, by_lost, by_need, by_refresh, pixels, lost, needy, kernel_ms}}."""
        given = dict(motion=motion, hit=hit, position=position, prev_hit=prev_hit, prev_position=prev_position, history_in=history_in,
                     moments_in=moments_in, length_in=length_in)
        desc = _lib.PlanDesc()
        self._bind_planes("samplePlan", desc, given, _lib.PLAN_PLANES, set(given))
        m = self._bind_mask("samplePlan", desc, mask)  # noqa: F841 (kept until the call has returned)
        for name, value, top in (("min_length", min_length, 65535), ("min_pixels", min_pixels, 64), ("refresh_period", refresh_period, 65535),
                                 ("frame_index", frame_index, 2**32 - 1)):
            if not 0 <= int(value) < 2**32:
                raise ValueError(f"samplePlan: {name} must be in [{1 if name == 'min_pixels' else 0},{top}]")
            setattr(desc, name, int(value))
        desc.normal_cos, desc.plane_eps, desc.min_weight = float(normal_cos), float(plane_eps), float(min_weight)
        desc.threshold, desc.dark_floor = float(threshold), float(dark_floor)
        desc.flags = 0
        nby, nbx = self.blockGrid()
        out = np.zeros((nby, nbx), np.uint8)
        desc.block_mask_out = out.ctypes.data
        return self._run_pass("pt_sample_plan", desc, _lib.PlanStats(), dict(mask=out))

    def temporalCarry(self, motion, hit, position, prev_hit, prev_position, history_in, moments_in, length_in, history_out=None, moments_out=None,
                      length_out=None, variance_out=None, variance=True, mask=None, normal_cos=0.9, plane_eps=0.01, min_weight=0.25) -> dict:
        """The temporal stage of the pixels that got no new sample (pt_temporal_carry, include/pt_amd.h): reprojects history, moments and
        length along the motion plane exactly as temporalMoments does and writes them unchanged — the length is carried, not incremented;
        a pixel whose history cannot be reprojected gets NaN colour words and length 0 and is counted in stats["lost"].  Called with the
        complement of samplePlan's mask and samplePlan's planes and normal_cos / plane_eps / min_weight, lost is 0.

        The planes are temporalMoments's without color and albedo, the outputs likewise: allocated with torch, zero-filled, when None
        (variance_out unless variance=False); pixels outside the views, the mask or the rank's partition are not written, so the outputs
        of a temporalMoments call on the plan's mask are completed in place by passing them here.  They may overlap no other plane.
        Ordering is on the device, as temporalMoments.  Returns {"history_out", "moments_out", "length_out", "variance_out": the tensor
        (None for a raw pointer or an absent plane), "stats": {pixels, carried, lost, kernel_ms}}."""
        given = dict(motion=motion, hit=hit, position=position, prev_hit=prev_hit, prev_position=prev_position, history_in=history_in,
                     moments_in=moments_in, length_in=length_in, history_out=history_out, moments_out=moments_out, length_out=length_out,
                     variance_out=variance_out)
        desc = _lib.CarryDesc()
        result = self._bind_planes("temporalCarry", desc, given, _lib.CARRY_PLANES, set(given) - {"variance_out"}, _lib.CARRY_OUTPUTS,
                                   alloc=_lib.CARRY_OUTPUTS if variance else _lib.CARRY_OUTPUTS[:3])
        m = self._bind_mask("temporalCarry", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.normal_cos, desc.plane_eps, desc.min_weight = float(normal_cos), float(plane_eps), float(min_weight)
        desc.flags = 0
        return self._run_pass("pt_temporal_carry", desc, _lib.CarryStats(), result)

    def vertexCount(self):
        """(vertices, triangles) of the context, summed over its meshes (pt_vertex_count)."""
        nv, nt = C.c_uint32(), C.c_uint32()
        self._ck(self._L.pt_vertex_count(self._ctx, C.byref(nv), C.byref(nt)), "pt_vertex_count")
        return nv.value, nt.value

    def copyVerticesDevice(self, out=None):
        """The context's current world-space vertices, all meshes in mesh order, copied on the GPU into a float32 (vertices, 3) CUDA tensor
        (pt_copy_vertices_device): the "previous vertices" of motionPlanes when taken before the frame's updateMeshes* / transformMeshes.
        out: a tensor of that shape on the context's device (dense, any 4-byte-aligned storage offset) or a raw device pointer; allocated
        with torch when None.  Waits for frames in flight; complete on return.  Returns the tensor (None for a raw pointer)."""
        import torch

        dev = getattr(self, "_device", 0)
        nv = sum(self._nv)
        if out is None:
            out = torch.empty((nv, 3), dtype=torch.float32, device=f"cuda:{dev}")
        if isinstance(out, int):
            ptr, result = out, None
        else:
            _check_temporal_tensor("out", out, dev, {torch.float32: (nv, 3)}, "copyVerticesDevice")
            ptr, result = out.data_ptr(), out
        self._after_torch()  # earlier users of `out`
        self._ck(self._L.pt_copy_vertices_device(self._ctx, ptr, nv * 12), "pt_copy_vertices_device")
        return result

    def motionPlanes(self, hit, prev_vertices, prev_cameras=None, planes=("motion", "prev_point", "prev_surface"), mask=None, out=None) -> dict:
        """Where each pixel's surface point was before the geometry moved (pt_motion_planes, include/pt_amd.h: the arithmetic, in full).

        hit: this frame's renderGBuffer hit plane, float32 (h, w, 8); prev_vertices: the previous frame's vertices, float32 (vertices, 3)
        (copyVerticesDevice before the geometry moved) — CUDA tensors on the context's device, dense, any 4-byte-aligned storage offset,
        or raw device pointers.  planes: any of "motion" (h, w, 2), "prev_point" (h, w, 4), "prev_surface" (h, w, 8).  out: {plane: tensor
        or raw pointer} for planes the caller owns; the others are allocated with torch, zero-filled (pixels outside the views, the mask
        or the rank's partition are not written).  prev_cameras, needed by "motion": as renderGBuffer takes them.  mask: 8x8 blocks as
        renderMask takes them, None = every block.
        Feeding the chain: temporalAccumulate(hit=prev_surface, position=prev_point, motion=motion) with prev_hit and prev_position the
        previous frame's G-buffer planes; filterPlanes keeps the current hit and position.
        Ordering is on the device: the library's stream waits for what torch has enqueued on its current stream; the call returns when
        the planes are complete.  The frame buffers, the accumulation and the path state are left alone.
        Returns {plane: tensor (None for a raw pointer), ..., "stats": {pixels, hits, stale, kernel_ms}}."""
        planes = tuple(planes)
        out = dict(out or {})
        for name in list(planes) + list(out):
            if name not in _lib.MOTION_PLANES:
                raise ValueError(f"motionPlanes: unknown plane {name!r} (one of {', '.join(_lib.MOTION_PLANES)})")
        if any(name not in planes for name in out):
            raise ValueError("motionPlanes: `out` names a plane that `planes` does not")
        if not planes:
            raise ValueError("motionPlanes: no plane asked for")
        if "motion" in planes and prev_cameras is None:
            raise ValueError("motionPlanes: motion needs prev_cameras")
        desc = _lib.MotionDesc()
        widths = dict(_lib.MOTION_PLANES, hit=8, prev_vertices=(sum(self._nv), 3))
        self._bind_planes("motionPlanes", desc, dict(hit=hit, prev_vertices=prev_vertices), widths, ("hit", "prev_vertices"))
        result = self._bind_planes("motionPlanes", desc, {name: out.get(name) for name in planes}, widths, outputs=planes, alloc=planes)
        rows = self._bind_prev_cameras(desc, prev_cameras)  # noqa: F841 (kept until the call has returned, as m is)
        m = self._bind_mask("motionPlanes", desc, mask)  # noqa: F841
        desc.flags = 0
        return self._run_pass("pt_motion_planes", desc, _lib.MotionStats(), result)

    def copyTexcoordsDevice(self, out=None):
        """The scene's texcoords per primitive, written on the GPU into a float32 (triangles, 6) CUDA tensor — uv0.xy, uv1.xy, uv2.xy in
        global primitive order (pt_copy_texcoords_device): the `prim_texcoords` of surfacePlanes.  All zeros for a scene without a
        textured mesh.  It depends on the scene only (updateMeshes*, transformMeshes, a rebuild leave it valid): take it once.
        out: a tensor of that shape on the context's device (dense, any 4-byte-aligned storage offset) or a raw device pointer; allocated
        with torch when None.  Waits for frames in flight; complete on return.  Returns the tensor (None for a raw pointer)."""
        import torch

        dev = getattr(self, "_device", 0)
        nt = self.vertexCount()[1]
        if out is None:
            out = torch.empty((nt, 6), dtype=torch.float32, device=f"cuda:{dev}")
        if isinstance(out, int):
            ptr, result = out, None
        else:
            _check_temporal_tensor("out", out, dev, {torch.float32: (nt, 6)}, "copyTexcoordsDevice")
            ptr, result = out.data_ptr(), out
        self._after_torch()  # earlier users of `out`
        self._ck(self._L.pt_copy_texcoords_device(self._ctx, ptr, nt * 24), "pt_copy_texcoords_device")
        return result

    def surfacePlanes(self, hit, prim_texcoords=None, planes=("albedo",), mask=None, out=None) -> dict:
        """The albedo and the texcoord under the centre of every pixel, from the hit plane (pt_surface_planes, include/pt_amd.h: the
        arithmetic, in full): the material's colour, replaced by the texture lookup at the barycentric texcoord on a textured mesh;
        (0, 0, 0, 1) at a miss.  Unlike deviceBuffer(PT_BUF_ALBEDO) it covers every pixel of the call under this frame's camera, whether
        the render visited the pixel or not: the albedo of temporalMoments / modulatePlanes in a loop that renders only some blocks.

        hit: this frame's renderGBuffer hit plane, float32 (h, w, 8); prim_texcoords: copyTexcoordsDevice's table, float32 (triangles, 6),
        needed when the scene has a textured mesh — CUDA tensors on the context's device, dense, any 4-byte-aligned storage offset, or
        raw device pointers.  planes: any of "albedo" (h, w, 4), "texcoord" (h, w, 2).  out: {plane: tensor or raw pointer} for planes
        the caller owns; the others are allocated with torch, zero-filled (pixels outside the views, the mask or the rank's partition
        are not written).  mask: 8x8 blocks as renderMask takes them, None = every block.
        Ordering is on the device: the library's stream waits for what torch has enqueued on its current stream; the call returns when
        the planes are complete.  The frame buffers, the accumulation and the path state are left alone.
        Returns {plane: tensor (None for a raw pointer), ..., "stats": {pixels, hits, stale, textured, kernel_ms}}."""
        planes = tuple(planes)
        out = dict(out or {})
        for name in list(planes) + list(out):
            if name not in _lib.SURFACE_PLANES:
                raise ValueError(f"surfacePlanes: unknown plane {name!r} (one of {', '.join(_lib.SURFACE_PLANES)})")
        if any(name not in planes for name in out):
            raise ValueError("surfacePlanes: `out` names a plane that `planes` does not")
        if not planes:
            raise ValueError("surfacePlanes: no plane asked for")
        desc = _lib.SurfaceDesc()
        is_tensor = prim_texcoords is not None and not isinstance(prim_texcoords, int)  # (a raw pointer or None: no shape to check)
        widths = dict(_lib.SURFACE_PLANES, hit=8, prim_texcoords=(self.vertexCount()[1] if is_tensor else 0, 6))
        self._bind_planes("surfacePlanes", desc, dict(hit=hit, prim_texcoords=prim_texcoords), widths, ("hit",))
        result = self._bind_planes("surfacePlanes", desc, {name: out.get(name) for name in planes}, widths, outputs=planes, alloc=planes)
        m = self._bind_mask("surfacePlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.flags = 0
        return self._run_pass("pt_surface_planes", desc, _lib.SurfaceStats(), result)

    def textureMipsLayout(self):
        """The shape of the texture mip pyramid (pt_texture_mips_layout): (dims, bytes) with dims a uint32 (textures, 4) array of w, h,
        levels and the index of the first 16-byte texel of level 1, and bytes the size of the whole pyramid (0: no level above 0)."""
        key = getattr(self._ctx, "value", self._ctx)
        cached = getattr(self, "_mips_layout", None)  # a context's textures never change
        if cached is None or cached[0] != key:
            nt, nbytes = C.c_uint32(), C.c_size_t()
            self._ck(self._L.pt_texture_mips_layout(self._ctx, C.byref(nt), None, C.byref(nbytes)), "pt_texture_mips_layout")
            dims = np.zeros((nt.value, 4), np.uint32)
            self._ck(self._L.pt_texture_mips_layout(self._ctx, None, dims.ctypes.data if nt.value else None, None), "pt_texture_mips_layout")
            cached = self._mips_layout = (key, dims, nbytes.value)
        return cached[1].copy(), cached[2]

    def copyTextureMipsDevice(self, out=None):
        """The box-filtered mip pyramid of the scene's textures, levels 1 and up, built on the GPU into a float32 (texels, 4) CUDA tensor
        (pt_copy_texture_mips_device; the layout is textureMipsLayout's): the `mips` of surfaceLodPlanes.  It depends on the scene only:
        take it once.  out: a tensor of that shape on the context's device (dense, 16-byte aligned) or a raw device pointer; allocated
        with torch when None.  Waits for frames in flight; complete on return.  Returns the tensor (None for a raw pointer)."""
        import torch

        dev = getattr(self, "_device", 0)
        nbytes = self.textureMipsLayout()[1]
        if out is None:
            out = torch.empty((nbytes // 16, 4), dtype=torch.float32, device=f"cuda:{dev}")
        if isinstance(out, int):
            ptr, result = out, None
        else:
            _check_temporal_tensor("out", out, dev, {torch.float32: (nbytes // 16, 4)}, "copyTextureMipsDevice")
            ptr, result = out.data_ptr(), out
        self._after_torch()  # earlier users of `out`
        self._ck(self._L.pt_copy_texture_mips_device(self._ctx, ptr, nbytes), "pt_copy_texture_mips_device")
        return result

    def surfaceLodPlanes(self, hit, prim_texcoords=None, mips=None, planes=("albedo",), footprint_scale=1.0, mask=None, out=None) -> dict:
        """surfacePlanes with a level of detail (pt_surface_lod_planes, include/pt_amd.h: the arithmetic, in full): on a textured mesh the
        pixel's footprint in texture space is derived from the hit plane, the current vertices and the pixel's camera, and the albedo is
        a trilinear lookup in the mip pyramid, so a minified texture no longer aliases.  Everything else is surfacePlanes's.

        hit, prim_texcoords, mask, out: as surfacePlanes takes them.  mips: copyTextureMipsDevice's pyramid, float32 (texels, 4), needed
        when the scene has a textured mesh and a texture larger than 1 x 1; a raw pointer stands for textureMipsLayout's bytes.
        planes: any of "albedo" (h, w, 4), "texcoord" (h, w, 2), "footprint" (h, w, 4: ds/dx, dt/dx, ds/dy, dt/dy per pixel step),
        "lod" (h, w).  footprint_scale: 1 = the pixel's own footprint, 0 = surfacePlanes's albedo bit for bit.
        Returns {plane: tensor (None for a raw pointer), ..., "stats": {pixels, hits, stale, textured, minified, kernel_ms}}."""
        planes = tuple(planes)
        out = dict(out or {})
        for name in list(planes) + list(out):
            if name not in _lib.SURFACE_LOD_PLANES:
                raise ValueError(f"surfaceLodPlanes: unknown plane {name!r} (one of {', '.join(_lib.SURFACE_LOD_PLANES)})")
        if any(name not in planes for name in out):
            raise ValueError("surfaceLodPlanes: `out` names a plane that `planes` does not")
        if not planes:
            raise ValueError("surfaceLodPlanes: no plane asked for")
        desc = _lib.SurfaceLodDesc()
        is_tensor = lambda t: t is not None and not isinstance(t, int)  # noqa: E731 (a raw pointer or None: no shape to check)
        nbytes = self.textureMipsLayout()[1] if mips is not None else 0
        widths = dict(_lib.SURFACE_LOD_PLANES, hit=8, prim_texcoords=(self.vertexCount()[1] if is_tensor(prim_texcoords) else 0, 6), mips=(nbytes // 16, 4))
        self._bind_planes("surfaceLodPlanes", desc, dict(hit=hit, prim_texcoords=prim_texcoords, mips=mips), widths, ("hit",))
        desc.mips_bytes = nbytes
        result = self._bind_planes("surfaceLodPlanes", desc, {name: out.get(name) for name in planes}, widths, outputs=planes, alloc=planes)
        m = self._bind_mask("surfaceLodPlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.footprint_scale = float(footprint_scale)
        desc.flags = 0
        return self._run_pass("pt_surface_lod_planes", desc, _lib.SurfaceLodStats(), result)

    def surfaceAnisoPlanes(self, hit, prim_texcoords=None, mips=None, max_aniso=8, planes=("albedo",), footprint_scale=1.0, mask=None, out=None) -> dict:
        """surfaceLodPlanes with up to max_aniso (1..16) lookups along the longer axis of the pixel's footprint (pt_surface_aniso_planes,
        include/pt_amd.h: the arithmetic, in full): each lookup takes the level of a footprint N times shorter, so a texture seen at a
        grazing angle is no longer blurred across the longer axis.  max_aniso = 1 is surfaceLodPlanes bit for bit.

        hit, prim_texcoords, mips, mask, out, footprint_scale: as surfaceLodPlanes takes them.  planes: any of surfaceLodPlanes's and
        "taps" (h, w): the number of lookups taken, 0 where no texture was read.
        Returns {plane: tensor (None for a raw pointer), ..., "stats": {pixels, hits, stale, textured, minified, anisotropic, taps,
        kernel_ms}}."""
        planes = tuple(planes)
        out = dict(out or {})
        for name in list(planes) + list(out):
            if name not in _lib.SURFACE_ANISO_PLANES:
                raise ValueError(f"surfaceAnisoPlanes: unknown plane {name!r} (one of {', '.join(_lib.SURFACE_ANISO_PLANES)})")
        if any(name not in planes for name in out):
            raise ValueError("surfaceAnisoPlanes: `out` names a plane that `planes` does not")
        if not planes:
            raise ValueError("surfaceAnisoPlanes: no plane asked for")
        if int(max_aniso) != max_aniso or not 1 <= int(max_aniso) <= 16:
            raise ValueError(f"surfaceAnisoPlanes: max_aniso must be an integer in 1..16, not {max_aniso!r}")
        desc = _lib.SurfaceAnisoDesc()
        is_tensor = lambda t: t is not None and not isinstance(t, int)  # noqa: E731 (a raw pointer or None: no shape to check)
        nbytes = self.textureMipsLayout()[1] if mips is not None else 0
        widths = dict(_lib.SURFACE_ANISO_PLANES, hit=8, prim_texcoords=(self.vertexCount()[1] if is_tensor(prim_texcoords) else 0, 6), mips=(nbytes // 16, 4))
        self._bind_planes("surfaceAnisoPlanes", desc, dict(hit=hit, prim_texcoords=prim_texcoords, mips=mips), widths, ("hit",))
        desc.mips_bytes = nbytes
        result = self._bind_planes("surfaceAnisoPlanes", desc, {name: out.get(name) for name in planes}, widths, outputs=planes, alloc=planes)
        m = self._bind_mask("surfaceAnisoPlanes", desc, mask)  # noqa: F841 (kept until the call has returned)
        desc.footprint_scale = float(footprint_scale)
        desc.max_aniso = int(max_aniso)
        desc.flags = 0
        return self._run_pass("pt_surface_aniso_planes", desc, _lib.SurfaceAnisoStats(), result)

    def evalTable(self, which, inp: np.ndarray, out_width: int, material=None, bsdf_mode=PT_BSDF_DISNEY) -> np.ndarray:
        inp = np.ascontiguousarray(inp, np.float32)
        n = inp.shape[0]
        out = np.empty((n, out_width), np.float32)
        mp = None
        if material is not None:
            mbuf = CMaterial()
            C.memmove(C.byref(mbuf), np.asarray(material).tobytes(), 104)
            mp = C.cast(C.byref(mbuf), C.c_void_p)
        self._ck(self._L.pt_eval_table(self._ctx, which, mp, bsdf_mode, inp.ctypes.data, n, out.ctypes.data), "pt_eval_table")
        return out


class _RankView(SampleRenderer):
    """A rank's context of a MultiRenderer seen through the single-context facade (download, stats, deviceBuffer ...).
    It does not own the context."""

    def __init__(self, L, ctx, launchParams, nv=(), device=0):
        self._L, self._ctx, self.launchParams, self._nv, self._device = L, ctx, launchParams, list(nv), device

    def close(self):
        self._ctx = C.c_void_p()


class MultiRenderer:
    """SampleRenderer over several GPUs of ONE process (pt_create_multi, include/pt_amd.h): the same call sequence as
    the reference's renderer; the frame is tile-partitioned over `devices`, rendered concurrently, and gathered on every
    rank by one RCCL all-gather (direct device-to-device copies when ranks share a device)."""

    EXCHANGE = {0: "none", 1: "rccl", 2: "peer_copy"}

    def __init__(self, model: Model, devices=(0,)):
        from ._lib import MultiStats  # noqa: F401

        self._L = L = _lib.load_library()
        self._m = C.c_void_p()
        self.launchParams = LaunchParams()
        self.devices = [int(d) for d in devices]
        self._nv = [len(m.vertex) for m in model.meshes]
        sd, keep = _scene_desc(model)
        dv = (C.c_int * len(self.devices))(*self.devices)
        rc = L.pt_create_multi(C.byref(sd), dv, len(self.devices), C.byref(self._m))
        del keep
        if rc:
            self._m = C.c_void_p()
            raise RuntimeError(f"pt_create_multi failed ({rc}): {L.pt_multi_last_error(None).decode()}")
        self.gather_mask = 1 << PT_BUF_FRAME  # what render() assembles on every rank (the reference displays frame_buffer)

    def _ck(self, rc, what):
        if rc:
            raise RuntimeError(f"{what} failed ({rc}): {self._L.pt_multi_last_error(self._m).decode()}")

    def close(self):
        if getattr(self, "_m", None):
            self._L.pt_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def world(self):
        return self._L.pt_multi_size(self._m)

    def rank(self, r) -> SampleRenderer:
        ctx = self._L.pt_multi_ctx(self._m, int(r))
        if not ctx:
            raise IndexError(r)
        return _RankView(self._L, C.c_void_p(ctx), self.launchParams, self._nv, self.devices[int(r)])

    def setOptions(self, max_depth=8, bsdf_mode=PT_BSDF_DISNEY, max_paths=0, bvh_kind=0, trace_kernel=0, streams=0, split_shadow=0, kernel_timing=0, frames_in_flight=0):
        o = Options(max_depth, bsdf_mode, max_paths, kernel_timing, bvh_kind, trace_kernel, streams, split_shadow, frames_in_flight)
        self._ck(self._L.pt_multi_set_options(self._m, C.byref(o)), "pt_multi_set_options")

    def setProbe(self, probe):
        if not getattr(probe, "valid", False):
            raise RuntimeError("Probe Data is not valid")  # Probe.h:104-105
        d = np.ascontiguousarray(probe.data, np.float32)
        a = [np.ascontiguousarray(x, np.float32) for x in (probe.pdfValuesX, probe.cdfValuesX, probe.pdfValuesY, probe.cdfValuesY)]
        self._ck(self._L.pt_multi_set_probe(self._m, d.ctypes.data, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, probe.width, probe.height), "pt_multi_set_probe")

    def resize(self, newSize, tile=(64, 16)):
        w, h = int(newSize[0]), int(newSize[1])
        self._ck(self._L.pt_multi_resize(self._m, w, h, int(tile[0]), int(tile[1])), "pt_multi_resize")
        if w and h:
            self.launchParams.frame.size = (w, h)

    def setCamera(self, camera: Camera):
        U, V, W = camera.UVWFrame()
        f3 = C.c_float * 3
        self._ck(self._L.pt_multi_set_camera(self._m, C.byref(f3(*[float(x) for x in camera.eye])), C.byref(f3(*[float(x) for x in U])), C.byref(f3(*[float(x) for x in V])), C.byref(f3(*[float(x) for x in W]))), "pt_multi_set_camera")

    def setViews(self, views):
        """SampleRenderer.setViews on every rank (pt_multi_set_views), after resize(): each rank renders the view pixels of its own blocks."""
        views = list(views)
        self._ck(self._L.pt_multi_set_views(self._m, _view_array(views) if views else None, len(views)), "pt_multi_set_views")

    def views(self):
        return _views_list(self._L, C.c_void_p(self._L.pt_multi_ctx(self._m, 0)))

    def setViewCameras(self, cameras):
        """SampleRenderer.setViewCameras on every rank (pt_multi_set_view_cameras).  The ranks may sit on different GPUs, so a torch tensor
        is copied to the host once and handed to every rank from there."""
        if _is_torch_tensor(cameras):
            cameras = cameras.detach().cpu().numpy()
        rows = _camera_rows(cameras)
        self._ck(self._L.pt_multi_set_view_cameras(self._m, rows.ctypes.data, rows.shape[0]), "pt_multi_set_view_cameras")

    def updateMeshes(self, vertices: dict, rebuild: bool = False) -> float:
        """SampleRenderer.updateMeshes on every rank (pt_multi_update_meshes); returns the slowest rank's kernel ms."""
        ups, n, keep = _mesh_updates(vertices)
        ms = C.c_double()
        self._ck(self._L.pt_multi_update_meshes(self._m, ups if n else None, n, _lib.PT_UPDATE_REBUILD if rebuild else _lib.PT_UPDATE_REFIT, C.byref(ms)), "pt_multi_update_meshes")
        del keep
        return ms.value

    def transformMeshes(self, transforms, from_current: bool = False, rebuild: bool = False) -> float:
        """SampleRenderer.transformMeshes on every rank (pt_multi_transform_meshes); returns the slowest rank's kernel ms."""
        arr, n = _mesh_transforms(transforms)
        ms = C.c_double()
        self._ck(self._L.pt_multi_transform_meshes(self._m, arr if n else None, n, _lib.PT_FROM_CURRENT if from_current else _lib.PT_FROM_REST,
                                                   _lib.PT_UPDATE_REBUILD if rebuild else _lib.PT_UPDATE_REFIT, C.byref(ms)), "pt_multi_transform_meshes")
        return ms.value

    def render(self, out: np.ndarray | None = None):
        ptr = out.ctypes.data if out is not None else None
        self._ck(self._L.pt_multi_render(self._m, int(self.launchParams.samples_per_launch), int(self.launchParams.frame.subframe_index), int(self.gather_mask), ptr), "pt_multi_render")

    def renderBatch(self, count: int, out: np.ndarray | None = None):
        ptr = out.ctypes.data if out is not None else None
        self._ck(self._L.pt_multi_render_batch(self._m, int(self.launchParams.samples_per_launch), int(self.launchParams.frame.subframe_index), int(count), int(self.gather_mask), ptr), "pt_multi_render_batch")

    def renderRegions(self, regions, variant=None, out: np.ndarray | None = None):
        arr = (Region * len(regions))()
        for k, g in enumerate(regions):
            for name, _ in Region._fields_:
                setattr(arr[k], name, g[name])
        vp = None
        if variant is not None:
            v = Variant(**variant)
            vp = C.byref(v)
        ptr = out.ctypes.data if out is not None else None
        self._ck(self._L.pt_multi_render_regions(self._m, arr, len(regions), vp, int(self.gather_mask), ptr), "pt_multi_render_regions")

    def renderFoveated(self, c, inner_radius=157, outer_radius=515, spp=(1, 2, 8), out=None, variant=None):
        regs = SampleRenderer.foveatedRegions(self.launchParams.frame.size, c, int(self.launchParams.frame.subframe_index), inner_radius, outer_radius, spp)
        self.renderRegions(regs, variant or SampleRenderer.SV4_VARIANT, out)
        self.launchParams.frame.subframe_index += 1

    def gather(self, which):
        self._ck(self._L.pt_multi_gather(self._m, int(which)), "pt_multi_gather")

    def flush(self, out: np.ndarray | None = None):
        """Overlapped hand-off (frames in flight + gather_mask): the newest frame goes on display now (pt_multi_flush)."""
        ptr = out.ctypes.data if out is not None else None
        self._ck(self._L.pt_multi_flush(self._m, ptr), "pt_multi_flush")

    def downloadDisplay(self, which, rank=0) -> np.ndarray:
        return self.rank(rank).downloadDisplay(which)

    def download(self, which, rank=0) -> np.ndarray:
        return self.rank(rank).download(which)

    def downloadPixels(self) -> np.ndarray:
        return self.download(PT_BUF_FRAME)

    def stats(self) -> dict:
        from ._lib import MultiStats

        s = MultiStats()
        self._ck(self._L.pt_multi_get_stats(self._m, C.byref(s)), "pt_multi_get_stats")
        d = s.sum.as_dict()
        d.update(gather_ms=s.gather_ms, exchange=self.EXCHANGE.get(s.exchange, "?"), ndev=s.ndev, enqueue_ms=s.enqueue_ms, threads=s.threads,
                 frames_handed_over=s.frames_handed_over)
        return d


def make_camera(cam: dict, aspect: float) -> Camera:
    return Camera(cam["eye"], cam["lookat"], cam["up"], cam["fovY"], aspect)


def warpMatrix(src_cam, dst_cam, size) -> np.ndarray:
    """The 3x3 matrix (row-major (9,) float32, output pixel -> source pixel of a size = (width, height) rectangle) that shows a frame
    rendered under src_cam as dst_cam sees it, for a pt_lens_view's `warp` (pt_warp_matrix, include/pt_amd.h).  Each camera is a Camera
    or a (12,) row eye, U, V, W; the eyes are ignored: the reprojection is rotational.  Host arithmetic, no GPU."""
    rows = [_camera_rows([c])[0] if isinstance(c, Camera) else np.ascontiguousarray(c, np.float32).reshape(-1) for c in (src_cam, dst_cam)]
    if any(r.size != 12 for r in rows):
        raise ValueError("warpMatrix: a Camera or 12 floats (eye, U, V, W) is expected per camera")
    out = np.zeros(9, np.float32)
    L = _lib.load_library()
    if L.pt_warp_matrix(rows[0].ctypes.data, rows[1].ctypes.data, int(size[0]), int(size[1]), out.ctypes.data):
        raise RuntimeError(L.pt_last_error(None).decode())
    return out


def make_lens(size, k=(0.0, 0.0, 0.0), center=None, radius=None, warp=None) -> "_lib.LensView":
    """A pt_lens_view for a view's rectangle of size = (width, height).  k: (k1, k2, k3) for all three channels, or three such rows for
    red, green and blue.  center: the lens centre in the rectangle's pixel coordinates (default: its middle).  radius: the pixel distance at
    which r = 1, one number or one per axis (default: half the width, on both axes); 0 or inf switches the polynomial off.  warp: a 3x3
    matrix in pixel coordinates, output pixel -> source pixel (warpMatrix's; default: the identity)."""
    w, h = float(size[0]), float(size[1])
    kk = np.asarray(k, np.float32)
    if kk.shape == (3,):
        kk = np.stack([kk] * 3)
    if kk.shape != (3, 3):
        raise ValueError("make_lens: k is (k1, k2, k3) or three such rows (red, green, blue)")
    cx, cy = (0.5 * w, 0.5 * h) if center is None else (float(center[0]), float(center[1]))
    rad = (0.5 * w, 0.5 * w) if radius is None else (float(radius), float(radius)) if np.ndim(radius) == 0 else (float(radius[0]), float(radius[1]))
    H = np.eye(3, dtype=np.float32).reshape(-1) if warp is None else np.asarray(warp, np.float32).reshape(-1)
    if H.size != 9:
        raise ValueError("make_lens: warp is a 3x3 matrix")
    v = _lib.LensView()
    v.center[0], v.center[1] = cx, cy
    for a in (0, 1):
        v.inv_radius[a] = 0.0 if rad[a] == 0.0 else float(np.float32(1.0) / np.float32(rad[a]))
    for ch in range(3):
        for j in range(3):
            v.k[ch][j] = float(kk[ch, j])
    for j in range(9):
        v.warp[j] = float(H[j])
    return v
