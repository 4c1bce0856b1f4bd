"""The seam between torch's streams and the library's: every device-pointer entry point of include/pt_amd.h's STREAM CONTRACT that the
facade wraps, called while work is still PENDING on torch's current stream — the producer of its inputs and a sentinel fill of its outputs —
with no host wait between the two.  GPU against GPU: each call is pinned to its NumPy or C reference elsewhere; here the outputs must equal,
bit for bit over the whole planes (NaN words as NaN), those of the same call made after a host synchronise.

One case (_pin), eight steps: (1) reference R from inputs B, synchronously, its host wall time taken; (2) the same call on stale inputs A
gives S, which must differ from R; (3) inputs hold A, outputs hold S, everything complete; (4) on torch's current stream a filler
(tests/busy_stream.py) of max(10 ms, 50 x that wall time), behind it device-to-device copies of B into the inputs, behind them a 0xA5 fill
of every output, behind that event E; (5) E is still pending; (6) the call, no host wait of any kind; (7) E is complete as soon as a
synchronous entry point has returned; (8) outputs and counters equal R's.  A lost input ordering shows as S, a lost output ordering as
sentinel words.  Every case runs on torch's default stream and under a fresh side stream.

The pin is timing based, and it can only see a lost ordering when the library's stream and torch's run side by side: HIP deals streams onto
a few hardware queues, and two streams on one queue serialise whatever the program says (Streams).  So every case asks first
(busy_stream.concurrent) and prints the answer; the side-stream run takes, of up to three fresh streams, the first that runs beside the
library's.  test_the_pin_has_teeth removes the ordering on purpose and must see S: it fails if no stream runs beside the library's.
What the cases can see: a case that hands tensors over fails without SampleRenderer._after_torch, a raw-pointer case without
pt_wait_event, a host-synchronising case without the facade's Stream.synchronize — on every stream that runs beside the library's.  A run
printed as BEHIND cannot see any of it, so the side-stream run of a case fails if neither of its two runs was beside the library's stream.
setViewCameras on the default stream is ordered by its own blocking copy on the null stream as well, and the loop has no long producer: it
checks that a side stream changes nothing, not that an ordering is there.
The pin found no call that was ordered wrongly.  It found two waits that hid a lost ordering, and both are gone from the library: a pass
allocated and freed its counter words per call, and hipFree waits for the whole device, the caller's streams included, so the call of
test_the_pin_has_teeth could not return before E (the blocks are recycled now: pass_counter_pool, pt_pass.h); surfaceLodPlanes, surfaceAnisoPlanes
and copyTextureMipsDevice began with a blocking device-to-host copy of the texture records, which ordered them behind torch's work by
accident (the copy goes through the context's stream now).

Filler numbers seen on an MI355X: 0.0729 ms per repeat of big.add_(1.0); host wall time of the reference call between 0.014 ms (pack,
unpackDisplay) and 0.179 ms (filterPlanes, two iterations; renderDevice 0.174, updateMeshesDevice 0.11 - 0.13, the other passes 0.04 -
0.12, traceDevice 0.06 - 0.10, the device copies 0.03 - 0.07), so 50 x the wall time stayed under 10 ms and every filler was the minimum:
10.0 ms = 139 repeats."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from gbuffer_ref import PLANES, _moved
from gpu_kit import filled, hip_runtime, plane_renderer, plane_shape, to_numpy
from gpu_kit import differ as _differ
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from pass_cases import FILTER_INPUTS, MOMENTS_INPUTS, filter_case, moments_case, moments_kwargs, motion_case, plan_case, surface_aniso_case, upsample_case
from scene_kit import VIEW_H, VIEW_W, _aimed_rays, _cam_dicts, _rows, _views, _wave
from stream_kit import _dev, _pin, _raw, _res, _same, _snapshot

gpu = pytest.mark.gpu
f32 = np.float32
SENTINEL = 0xA5A5A5A5
RAYS = 4097
MODES = ["default", "side"]
COVERS = {}  # test name -> the entry points of the contract it orders


def covers(*names):
    def mark(fn):
        COVERS[fn.__name__] = names
        return fn
    return mark


# ------------------------------------------------------------------ the protocol
# ------------------------------------------------------------------ inputs: the existing small cases, built once
def _filled(words, name, h, w):
    """a sentinel-filled output plane of a pass, from the pass's table of words per pixel"""
    return filled(plane_shape(h, w, words[name]), dtype=torch.int32 if name == "frame_rgba8" else torch.float32)


def _size(r):
    w, h = r.launchParams.frame.size
    return h, w


# ------------------------------------------------------------------ passes with tensor inputs and outputs
@gpu
@covers("pt_temporal_accumulate", "pt_device_buffer")
@pytest.mark.parametrize("mode", MODES)
def test_temporal_accumulate(ptlib, mode):
    """`color` is the context's own accumulation buffer (pt_device_buffer), a raw pointer; the seven other inputs are pending tensors"""
    r, planes, _ = moments_case("two_box")
    h, w = _size(r)
    r.uploadAccum(planes["color"])
    color = r.deviceBuffer(R.PT_BUF_ACCUM)
    assert color
    B = {k: planes[k] for k in ("motion", "hit", "position", "prev_hit", "prev_position", "history_in", "length_in")}
    outs = {k: _filled(_lib.TEMPORAL_PLANES, k, h, w) for k in _lib.TEMPORAL_OUTPUTS}

    def call(dev, outs, returned):
        res = r.temporalAccumulate(color, **dev, **outs)
        returned()
        return _res(res, outs)

    _pin("temporalAccumulate", mode, r, B, outs, call)


@gpu
@covers("pt_temporal_moments")
@pytest.mark.parametrize("mode", MODES)
def test_temporal_moments(ptlib, mode):
    r, planes, prm = moments_case("two_box")
    h, w = _size(r)
    outs = {k: _filled(_lib.TMOM_PLANES, k, h, w) for k in _lib.TMOM_OUTPUTS}

    def call(dev, outs, returned):
        res = r.temporalMoments(**dev, **outs, **moments_kwargs(dict(prm, clamp=True)))
        returned()
        return _res(res, outs)

    _pin("temporalMoments", mode, r, {k: planes[k] for k in MOMENTS_INPUTS}, outs, call)


@gpu
@covers("pt_temporal_carry")
@pytest.mark.parametrize("mode", MODES)
def test_temporal_carry(ptlib, mode):
    import plan_ref as PR
    r, planes, prm = plan_case("two_box")
    h, w = _size(r)
    outs = {k: _filled(_lib.CARRY_PLANES, k, h, w) for k in _lib.CARRY_OUTPUTS}

    def call(dev, outs, returned):
        res = r.temporalCarry(**dev, **outs, **prm)
        returned()
        return _res(res, outs)

    _pin("temporalCarry", mode, r, {k: planes[k] for k in PR.INPUTS}, outs, call)


@gpu
@covers("pt_sample_plan")
@pytest.mark.parametrize("mode", MODES)
def test_sample_plan(ptlib, mode):
    """no device output: the plan's mask comes back on the host, so only the inputs' producer is pending"""
    import plan_ref as PR

    r, planes, prm = plan_case("two_box")

    def call(dev, outs, returned):
        res = r.samplePlan(**dev, **dict(PR.REAL_PLAN, **prm))
        returned()
        return res

    ref, _ = _pin("samplePlan", mode, r, {k: planes[k] for k in PR.INPUTS}, {}, call)
    assert 0 < ref["stats"]["sampled"] < ref["stats"]["blocks"]


@gpu
@covers("pt_filter_planes")
@pytest.mark.parametrize("mode", MODES)
def test_filter_planes(ptlib, mode):
    r, planes, prm = filter_case("two_box")
    h, w = _size(r)
    outs = {k: _filled(_lib.FILTER_PLANES, k, h, w) for k in ("out", "scratch", "frame_rgba8")}

    def call(dev, outs, returned):
        res = r.filterPlanes(**dev, out=outs["out"], scratch=outs["scratch"], frame=outs["frame_rgba8"], iterations=2, **prm)
        returned()
        return _res(res, outs)

    _pin("filterPlanes", mode, r, {k: planes[k] for k in FILTER_INPUTS}, outs, call)


@gpu
@covers("pt_modulate_planes")
@pytest.mark.parametrize("mode", MODES)
def test_modulate_planes(ptlib, mode):
    r, planes, _ = moments_case("two_box")
    h, w = _size(r)
    outs = {k: _filled(dict(out=4, frame_rgba8=1), k, h, w) for k in ("out", "frame_rgba8")}

    def call(dev, outs, returned):
        res = r.modulatePlanes(dev["color"], albedo=dev["albedo"], out=outs["out"], frame=outs["frame_rgba8"])
        returned()
        return _res(res, outs)

    _pin("modulatePlanes", mode, r, dict(color=planes["color"], albedo=planes["albedo"]), outs, call)


@gpu
@covers("pt_motion_planes")
@pytest.mark.parametrize("mode", MODES)
def test_motion_planes(ptlib, mode):
    import motion_ref as M
    c = motion_case("two_box")
    h, w = _size(c.r)
    outs = {k: _filled(M.WORDS, k, h, w) for k in M.PLANES}

    def call(dev, outs, returned):
        res = c.r.motionPlanes(dev["hit"], dev["prev_vertices"], prev_cameras=c.prev_row, planes=M.PLANES, out=outs)
        returned()
        return _res(res, outs)

    _pin("motionPlanes", mode, c.r, dict(hit=c.cur["hit"], prev_vertices=c.after_create), outs, call)


def _surface(fn, planes, mode, broken=False, **kw):
    c = surface_aniso_case("textured")
    h, w = _size(c.r)
    outs = {k: _filled(planes, k, h, w) for k in planes}

    def call(dev, outs, returned):
        res = getattr(c.r, fn)(dev["hit"], dev["prim_texcoords"], *([dev["mips"]] if "mips" in dev else []), planes=tuple(planes), out=outs, **kw)
        returned()
        return _res(res, outs)

    B = dict(hit=c.hit, prim_texcoords=to_numpy(c.table))
    if fn != "surfacePlanes":
        B["mips"] = to_numpy(c.mips)
    return _pin(fn, mode, c.r, B, outs, call, broken=broken)


@gpu
@covers("pt_surface_planes")
@pytest.mark.parametrize("mode", MODES)
def test_surface_planes(ptlib, mode):
    ref, _ = _surface("surfacePlanes", _lib.SURFACE_PLANES, mode)
    assert ref["stats"]["textured"] > 0


@gpu
@covers("pt_surface_lod_planes")
@pytest.mark.parametrize("mode", MODES)
def test_surface_lod_planes(ptlib, mode):
    ref, _ = _surface("surfaceLodPlanes", _lib.SURFACE_LOD_PLANES, mode)
    assert ref["stats"]["textured"] > 0


@gpu
@covers("pt_surface_aniso_planes")
@pytest.mark.parametrize("mode", MODES)
def test_surface_aniso_planes(ptlib, mode):
    ref, _ = _surface("surfaceAnisoPlanes", _lib.SURFACE_ANISO_PLANES, mode, max_aniso=8)
    assert ref["stats"]["textured"] > 0


@gpu
@covers("pt_upsample_planes")
@pytest.mark.parametrize("mode", MODES)
def test_upsample_planes_into_planes_the_facade_allocates(ptlib, mode):
    """out=None: the facade's torch.zeros lands behind the filler as well, and the pass behind it"""
    r, lo, hi = upsample_case("two_box", 2)
    h, w = _size(r)
    outs = dict(weight_out=_filled(_lib.UPSAMPLE_PLANES, "weight_out", h, w))

    def call(dev, outs, returned):
        res = r.upsamplePlanes(**dev, scale=2, out=None, weight_out=outs["weight_out"])
        returned()
        assert res["out"] is not None and res["weight_out"] is outs["weight_out"]
        return dict(out=res["out"], weight_out=outs["weight_out"], stats=res["stats"])

    B = dict(lo_color=lo["color"], lo_hit=lo["hit"], lo_position=lo["position"], hit=hi["hit"], position=hi["position"])
    _pin("upsamplePlanes", mode, r, B, outs, call)


# ------------------------------------------------------------------ output-only calls: the pending work is the sentinel fill of `out`
def _no_sentinel_where_the_reference_wrote(ref, got):
    for k, a in got.items():
        if k != "stats" and a.dtype.itemsize == 4:
            assert not ((a.view(np.uint32) == SENTINEL) & (ref[k].view(np.uint32) != SENTINEL)).any(), k


@gpu
@covers("pt_render_gbuffer")
@pytest.mark.parametrize("mode", MODES)
def test_render_gbuffer(ptlib, mode):
    c = surface_aniso_case("textured")
    h, w = _size(c.r)
    outs = {k: _filled(_lib.GBUFFER_PLANES, k, h, w) for k in PLANES}

    def call(dev, outs, returned):
        res = c.r.renderGBuffer(PLANES, prev_cameras=c.row, out=outs)
        returned()
        return _res(res, outs)

    ref, got = _pin("renderGBuffer", mode, c.r, {}, outs, call)
    assert ref["stats"]["hits"] > 0
    _no_sentinel_where_the_reference_wrote(ref, got)


@gpu
@covers("pt_copy_vertices_device", "pt_copy_texcoords_device", "pt_copy_texture_mips_device")
@pytest.mark.parametrize("fn", ["copyVerticesDevice", "copyTexcoordsDevice", "copyTextureMipsDevice"])
@pytest.mark.parametrize("mode", MODES)
def test_device_copies(ptlib, mode, fn):
    c = surface_aniso_case("textured")
    nv, nt = c.r.vertexCount()
    shape = dict(copyVerticesDevice=(nv, 3), copyTexcoordsDevice=(nt, 6), copyTextureMipsDevice=(c.r.textureMipsLayout()[1] // 16, 4))[fn]
    assert shape[0] > 0
    outs = dict(out=_raw(shape))

    def call(dev, outs, returned):
        assert getattr(c.r, fn)(outs["out"]) is outs["out"]
        returned()
        return dict(outs)

    ref, got = _pin(fn, mode, c.r, {}, outs, call)
    assert not (ref["out"].view(np.uint32) == SENTINEL).any()
    _no_sentinel_where_the_reference_wrote(ref, got)


# ------------------------------------------------------------------ ray queries
def _rays(model):
    return _aimed_rays(model, RAYS, 5)


@gpu
@covers("pt_trace_device")
@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("mode", MODES)
def test_trace_device(ptlib, mode, any_hit):
    c = motion_case("two_box")
    outs = dict(out=_raw((RAYS,), torch.int32) if any_hit else _raw((RAYS, 8)))

    def call(dev, outs, returned):
        c.r.traceDevice(dev["rays"], any_hit=any_hit, out=outs["out"])
        returned()
        return dict(out=outs["out"], stats=c.r.queryStats)

    ref, _ = _pin(f"traceDevice, {'any' if any_hit else 'closest'} hit", mode, c.r, dict(rays=_rays(c.model)), outs, call)
    assert ref["stats"]["rays"] == RAYS and ref["stats"]["hits"] > 0


@gpu
@covers("pt_trace_device")
@pytest.mark.parametrize("mode", MODES)
def test_trace_device_without_wait_then_a_clone_on_the_same_stream(ptlib, mode):
    """wait=False: the query is only enqueued; torch's current stream is made to wait for it, so a clone enqueued directly behind the call,
    with no host wait, holds the reference's records"""
    c = motion_case("two_box")
    outs = dict(out=_raw((RAYS, 8)))

    def call(dev, outs, returned):
        c.r.traceDevice(dev["rays"], out=outs["out"], wait=False)
        clone = outs["out"].clone()
        stats = c.r.queryWait()
        returned()
        return dict(out=outs["out"], clone=clone, stats=stats)

    ref, got = _pin("traceDevice(wait=False) + clone", mode, c.r, dict(rays=_rays(c.model)), outs, call)
    assert not _differ(got["clone"], ref["out"]).any()


@gpu
@covers("pt_trace_device")
@pytest.mark.parametrize("mode", MODES)
def test_trace_device_raw_pointers_behind_wait_event(ptlib, mode):
    c = motion_case("two_box")
    outs = dict(out=_raw((RAYS, 8)))

    def call(dev, outs, returned):
        assert c.r.traceDevice((dev["rays"].data_ptr(), RAYS), out=outs["out"].data_ptr()) is None
        returned()
        return dict(out=outs["out"], stats=c.r.queryStats)

    _pin("traceDevice, raw pointers", mode, c.r, dict(rays=_rays(c.model)), outs, call, raw=True)


# ------------------------------------------------------------------ geometry and cameras from device memory
def _update_case(mode, raw):
    model = scenes.two_box_scene(shadow_catcher=False)
    r = plane_renderer(model, (131, 61), scenes.TWO_BOX_CAMERA)
    mesh = 0
    rest = np.ascontiguousarray(model.meshes[mesh].vertex, f32)
    moved = _wave(model, 0.05)[mesh]
    nv = len(rest)
    first = sum(len(m.vertex) for m in model.meshes[:mesh])
    rays = _dev(_rays(model))

    def call(dev, outs, returned):
        r.updateMeshesDevice({mesh: (dev["vertices"].data_ptr(), nv) if raw else dev["vertices"]})
        returned()
        return dict(vertices=r.copyVerticesDevice(), record=r.traceDevice(rays)["record"], stats=r.queryStats)

    ref, got = _pin(f"updateMeshesDevice, {'a raw pointer' if raw else 'a tensor'}", mode, r, dict(vertices=moved), {}, call, A=dict(vertices=rest), raw=raw)
    assert np.array_equal(got["vertices"][first:first + nv].view(np.uint32), moved.view(np.uint32))
    # R came from this context, refitted to the rest vertices and back in between: equal only if a refit depends on nothing but the current
    # vertices (tests/test_gpu_refit.py pins that).  So also: a second context, updated once, after a host synchronise.
    other = plane_renderer(model, (131, 61), scenes.TWO_BOX_CAMERA)
    t = _dev(moved)
    torch.cuda.synchronize()
    other.updateMeshesDevice({mesh: t})
    want = _snapshot(dict(vertices=other.copyVerticesDevice(), record=other.traceDevice(rays)["record"], stats=other.queryStats))
    _same(got, want, "updateMeshesDevice against a context updated after a host synchronise")
    other.close()
    r.close()


@gpu
@covers("pt_update_meshes_device")
@pytest.mark.parametrize("mode", MODES)
def test_update_meshes_device_synchronises_a_tensors_stream(ptlib, mode):
    """the facade synchronises torch's current stream on the host for a tensor; afterwards the context holds B and the tree is B's"""
    _update_case(mode, raw=False)


@gpu
@covers("pt_update_meshes_device")
@pytest.mark.parametrize("mode", MODES)
def test_update_meshes_device_raw_pointer_behind_wait_event(ptlib, mode):
    """a raw pointer gets no synchronise from the facade: pt_wait_event(E) is the ordering"""
    _update_case(mode, raw=True)


@gpu
@covers("pt_set_view_cameras_device")
@pytest.mark.parametrize("mode", MODES)
def test_set_view_cameras_from_a_tensor(ptlib, mode):
    r = plane_renderer(scenes.two_box_scene(shadow_catcher=False), (VIEW_W, VIEW_H), scenes.TWO_BOX_CAMERA)
    r.setViews(_views())
    rows = _rows(_views([_moved(c) for c in _cam_dicts()]))

    def call(dev, outs, returned):
        r.setViewCameras(dev["rows"])
        returned()
        return dict(rows=np.stack([np.concatenate([v["eye"], v["U"], v["V"], v["W"]]) for v in r.views()]))

    _, got = _pin("setViewCameras", mode, r, dict(rows=rows), {}, call, A=dict(rows=_rows(_views())))
    assert np.array_equal(got["rows"].view(np.uint32), rows.view(np.uint32))
    r.close()


# ------------------------------------------------------------------ raw pointers of the display hand-off, ordered by pt_wait_event
_RENDERED = {}


def _rendered():
    """a context that has rendered one frame (67 x 45, the smallest G-buffer case's size)"""
    if not _RENDERED:
        w, h = 67, 45
        r = R.SampleRenderer(scenes.cornell_box())
        r.setProbe(scenes.sky_probe(64, 32).BuildCDF())
        r.setOptions(max_depth=3)
        r.resize((w, h))
        r.setCamera(R.make_camera(scenes.CORNELL_CAMERA, w / h))
        r.render()
        owned, padded = r.ownedPixels()
        assert owned == w * h
        _RENDERED.update(r=r, padded=padded, size=(h, w))
    return _RENDERED["r"], _RENDERED["padded"], _RENDERED["size"]


@gpu
@covers("pt_pack", "pt_pack_async", "pt_render_device")
@pytest.mark.parametrize("fn", ["pack", "packAsync", "renderDevice"])
@pytest.mark.parametrize("mode", MODES)
def test_pack_and_render_into_a_buffer_whose_fill_is_pending(ptlib, mode, fn):
    r, padded, size = _rendered()
    outs = dict(dst=_raw(size if fn == "renderDevice" else (padded,), torch.int32))

    def call(dev, outs, returned):
        ptr = outs["dst"].data_ptr()
        if fn == "pack":
            r.pack(R.PT_BUF_FRAME, ptr)
        elif fn == "packAsync":
            r.packAsync(R.PT_BUF_FRAME, ptr, 0)
            r.packWait(0)
        else:
            r.launchParams.frame.subframe_index = 0
            r.renderDevice(ptr)
        returned()
        return dict(outs)

    ref, got = _pin(fn, mode, r, {}, outs, call, raw=True)
    assert (ref["dst"] != 0).any() and not (ref["dst"].view(np.uint32)[:size[0] * size[1]] == SENTINEL).any()  # (the frame is there)
    _no_sentinel_where_the_reference_wrote(ref, got)


@gpu
@covers("pt_unpack_display", "pt_display_buffer")
@pytest.mark.parametrize("mode", MODES)
def test_unpack_display_from_a_buffer_whose_producer_is_pending(ptlib, mode):
    """pt_unpack_display + pt_display_sync + pt_download_display; what pt_display_buffer points to is the same image once the sync is back"""
    r, padded, (h, w) = _rendered()
    hip = hip_runtime()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    src = np.random.default_rng(17).integers(1, 0x7F000000, padded).astype(np.int32)

    def call(dev, outs, returned):
        r.unpackDisplay(R.PT_BUF_FRAME, dev["src"].data_ptr())
        r.displaySync()
        returned()
        ptr = r._L.pt_display_buffer(r._ctx, R.PT_BUF_FRAME)
        seen = np.empty((h, w), np.uint32)
        assert ptr and hip.hipMemcpy(seen.ctypes.data, ptr, seen.nbytes, 2) == 0  # (device to host)
        return dict(display=r.downloadDisplay(R.PT_BUF_FRAME), buffer=seen)

    ref, got = _pin("unpackDisplay", mode, r, dict(src=src), {}, call, raw=True)
    assert np.array_equal(got["display"], got["buffer"]) and np.isin(got["display"], src.view(np.uint32)).all()


# ------------------------------------------------------------------ the pin has teeth
@gpu
def test_the_pin_has_teeth(ptlib, monkeypatch):
    """surfacePlanes with SampleRenderer._after_torch doing nothing: the pass reads the stale planes while their producer is pending, the
    call returns before E, the outputs are S.  With the ordering in place, on the same kind of stream, they are R (test_surface_planes)."""
    monkeypatch.setattr(R.SampleRenderer, "_after_torch", lambda self: None)
    _surface("surfacePlanes", _lib.SURFACE_PLANES, "teeth", broken=True)
    monkeypatch.undo()
    _surface("surfacePlanes", _lib.SURFACE_PLANES, "teeth")


# ------------------------------------------------------------------ a real loop on either stream
@gpu
def test_upsampled_loop_is_the_same_on_a_side_stream(ptlib):
    """examples/upsampled_svgf_loop.py's UpsampledLoop, two frames at 128 x 56, scale 2, from fresh contexts with the same cameras: once on
    torch's default stream, once entirely under a side stream (the planes' zero fills of its constructor and whatever torch does between
    the passes are the pending work).  `final` is the same bit for bit."""
    import surface_ref as S

    spec = importlib.util.spec_from_file_location("upsampled_svgf_loop", os.path.join(ROOT, "examples", "upsampled_svgf_loop.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    w, h = 128, 56
    probe = scenes.sky_probe(256, 128).BuildCDF()
    cam0 = ex.SCENES["textured"][1]

    def run():
        up = ex.UpsampledLoop(S.textured_scene(), (w, h), 2, probe=probe)
        cam = R.make_camera(cam0, w / h)
        for k in range(2):
            prev, cam = cam, R.make_camera(ex.orbit(cam0, 0.01 * k), w / h)
            x = up.frame(k, prev, cam)
            assert x["pixels"] == w * h
        final = up.final.cpu().numpy().view(np.uint32).copy()
        rgba = up.frame_rgba8.cpu().numpy().view(np.uint32).copy()
        up.close()
        return final, rgba

    torch.cuda.synchronize()
    on_default = run()
    with torch.cuda.stream(torch.cuda.Stream()):
        on_side = run()
    torch.cuda.synchronize()
    assert (on_default[0].view(f32)[..., :3] > 0).any()
    for a, b, name in zip(on_default, on_side, ("final", "frame_rgba8")):
        assert not _differ(a, b).any(), f"{name} differs in {int(_differ(a, b).sum())} words between the default and the side stream"


# ------------------------------------------------------------------ completeness (no GPU)
def contract_entry_points():
    """the names in the list of the STREAM CONTRACT paragraph of include/pt_amd.h: 'Entry points that take or return DEVICE pointers — ... —'"""
    text = open(os.path.join(ROOT, "include", "pt_amd.h"), encoding="utf-8").read()
    para = text.split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    listed = para.split("DEVICE pointers")[1].split("read and write them")[0]
    return re.findall(r"\bpt_\w+", listed)


def test_every_entry_point_of_the_contract_has_an_ordering_case():
    names = contract_entry_points()
    assert len(names) >= 24 and len(set(names)) == len(names) and "pt_pack" in names and "pt_upsample_planes" in names
    here = open(__file__, encoding="utf-8").read()
    for test, eps in COVERS.items():  # what this file says it covers is there, marked gpu, and names the entry point's facade method
        assert callable(globals().get(test)) and f"def {test}(" in here, test
        assert any(m.name == "gpu" for m in getattr(globals()[test], "pytestmark", [])), test
    covered = {n for eps in COVERS.values() for n in eps}
    schedule = open(os.path.join(ROOT, "tests", "test_gpu_schedule.py"), encoding="utf-8").read()
    body = schedule.split("def test_wait_event_orders_the_context_behind_the_callers_stream(")[1].split("\ndef ")[0]
    if "r.waitEvent(" in body and "r.unpack(" in body:
        covered.add("pt_unpack")
    missing = [n for n in names if n not in covered]
    assert not missing, f"entry points of the STREAM CONTRACT without an ordering case in tests/test_gpu_stream_contract.py: {missing}"
    # the facade reaches each of them (pt_display_buffer has no method of its own: the case calls it through the library handle)
    facade = open(os.path.join(ROOT, "optixpathtracer_amd", "renderer.py"), encoding="utf-8").read()
    assert [n for n in names if n not in facade] == ["pt_display_buffer"]
