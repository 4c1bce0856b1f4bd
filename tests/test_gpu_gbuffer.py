"""The first-hit G-buffer (pt_render_gbuffer) on the GPU.  No tolerance anywhere except the one sanity bound that says so.

Yardsticks, all independent of the kernel under test: the `ray` plane is float32 NumPy's evaluation of the header's expression; the `hit` plane
is pt_trace_device's answer for those rays (itself pinned to the CPU checker) and (t, prim) are the CPU checker's; depth, position and motion
are float32 NumPy's evaluation of the header's formulas from the NumPy rays and the checker's t.  References are computed once per input and
never modified.

Inputs (first hits of the pixel-centre rays counted with the checker; every one has hits and misses):
  two_box_scene(shadow_catcher=False)    131 x 61  TWO_BOX_CAMERA   4862 hits 3129 misses   (17 x 8 blocks, last column 3 wide, last row 5 high)
  cornell_box()                           67 x 45  CORNELL_CAMERA   1899 hits 1116 misses
  voxel_terrain(n=64, target_tris=20000) 131 x 61  TERRAIN_CAMERA   5287 hits 2704 misses   (deep tree, leaves with several triangles)
  two-box under the four views of tests/test_gpu_views.py: 1429/828, 1172/771, 301/203, 25/10"""
import ctypes as C

import numpy as np
import pytest
import torch

from gbuffer_ref import PLANES, QNAN, _behind, _moved, _np_planes, _np_rays, _row
from gpu_kit import filled, pixel_mask, plane_shape
from gpu_kit import bits as _bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from scene_kit import M1, RECTS, _cam_dicts, _np_transform, _views_and_prev, _with_vertices

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 131, 61
WORDS = _lib.GBUFFER_PLANES
SENTINEL = 0xA5A5A5A5
INPUTS = {
    "two_box": (lambda: scenes.two_box_scene(shadow_catcher=False), (W, H), scenes.TWO_BOX_CAMERA, (4862, 3129)),
    "cornell": (scenes.cornell_box, (67, 45), scenes.CORNELL_CAMERA, (1899, 1116)),
    "terrain": (lambda: scenes.voxel_terrain(n=64, target_tris=20000), (W, H), scenes.TERRAIN_CAMERA, (5287, 2704)),
}
VIEW_COUNTS = [(1429, 828), (1172, 771), (301, 203), (25, 10)]


# ------------------------------------------------------------------ GPU helpers
def _filled(name, h, w, offset=False):
    """a sentinel-filled plane of the pass; offset: one float into its allocation (4-byte aligned only)"""
    return filled(plane_shape(h, w, WORDS[name]), offset)


def _gbuffer(r, planes=PLANES, prev=None, mask=None, offset=False):
    """renderGBuffer into sentinel-filled planes -> ({plane: uint32 bits}, stats)"""
    w, h = r.launchParams.frame.size
    out = {p: _filled(p, h, w, offset) for p in planes}
    res = r.renderGBuffer(planes, prev_cameras=prev, mask=mask, out=out)
    assert all(res[p] is out[p] for p in planes)
    return {p: _bits(out[p]) for p in planes}, res["stats"]


def _same(got, want, what, where=None):
    for p in want:
        if p not in got:
            continue
        a, b = got[p], want[p]
        if where is not None:
            a, b = a[where], b[where]
        assert np.array_equal(a, b), f"{what}: plane {p} differs in {int((a != b).sum())} words"


def _untouched(got, where, what):
    for p, a in got.items():
        assert (a[where] == SENTINEL).all(), f"{what}: plane {p} was written outside the active pixels"


class _Case:
    pass


_CASES = {}


def _case(name, orc_det):
    """The input's model, renderer, NumPy rays, checker answer, and the full five-plane pass with the camera moved by 0.25 in x as the previous
    one.  Built once; the arrays are read-only."""
    if name not in _CASES:
        make, size, cam, counts = INPUTS[name]
        c = _Case()
        c.model, c.size, c.cam, c.counts = make(), size, cam, counts
        w, h = size
        c.row = _row(cam, w / h)
        c.prev = _row(_moved(cam), w / h)
        c.rays = _np_rays(c.row, w, h)
        c.sc = orc_det.make_scene(c.model, use_bvh=True)
        t, prim = orc_det.trace_closest(c.sc, c.rays.reshape(-1, 8))
        c.t, c.prim = np.asarray(t, f32).reshape(h, w), np.asarray(prim, np.int32).reshape(h, w)
        c.hit = c.prim >= 0
        c.r = _renderer(c.model, size, cam)
        c.full, c.stats = _gbuffer(c.r, prev=c.prev)
        for a in [c.rays, c.t, c.prim, c.hit] + list(c.full.values()):
            a.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


def _check_ray_and_hit(r, got, stats, rays, t, prim, what):
    """item 1 of the contract: ray == NumPy, hit == pt_trace_device of that ray plane, (t, prim) == the checker, stats.hits == hit records"""
    h, w = prim.shape
    assert np.array_equal(got["ray"], rays.view(np.uint32)), f"{what}: the ray plane differs from float32 NumPy"
    dev_rays = torch.from_numpy(got["ray"].view(f32).reshape(-1, 8).copy()).to("cuda:0")
    want = _bits(r.traceDevice(dev_rays)["record"]).reshape(h, w, 8)
    assert np.array_equal(got["hit"], want), f"{what}: the hit plane differs from pt_trace_device in {int((got['hit'] != want).any(-1).sum())} records"
    rec = got["hit"].view(_lib.HIT_DTYPE).reshape(h, w)
    assert np.array_equal(rec["prim"], prim) and np.array_equal(rec["t"].view(np.uint32), t.view(np.uint32)), f"{what}: (t, prim) against the checker"
    nhit = int((rec["prim"] >= 0).sum())
    assert stats["hits"] == nhit and stats["pixels"] == w * h and stats["kernel_ms"] > 0
    return nhit


# ------------------------------------------------------------------ 1. ray and hit
@pytest.mark.parametrize("name", list(INPUTS))
def test_ray_and_hit(ptlib, orc_det, name):
    c = _case(name, orc_det)
    nhit = _check_ray_and_hit(c.r, c.full, c.stats, c.rays, c.t, c.prim, name)
    assert (nhit, c.prim.size - nhit) == c.counts and nhit > 0 and nhit < c.prim.size  # hits and misses are both present
    miss = c.full["hit"][~c.hit]
    assert (miss[:, 0] == f32(1e16).view(np.uint32)).all() and (miss[:, 3].view(np.int32) == -1).all() and (miss[:, 4].view(np.int32) == -1).all()
    assert not miss[:, [1, 2, 5, 6, 7]].any()
    if name == "terrain":
        assert len(np.unique(c.prim[c.hit])) == 2477


def test_ray_and_hit_one_pixel(ptlib, orc_det):
    model = scenes.two_box_scene(shadow_catcher=False)
    r = _renderer(model, (1, 1), scenes.TWO_BOX_CAMERA)
    rays = _np_rays(_row(scenes.TWO_BOX_CAMERA, 1.0), 1, 1)
    t, prim = orc_det.trace_closest(orc_det.make_scene(model, use_bvh=True), rays.reshape(-1, 8))
    got, stats = _gbuffer(r, ("hit", "ray"))
    assert _check_ray_and_hit(r, got, stats, rays, np.asarray(t, f32).reshape(1, 1), np.asarray(prim, np.int32).reshape(1, 1), "1 x 1") == 1
    r.close()


# ------------------------------------------------------------------ 2. derived planes
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_derived_planes_equal_numpy(ptlib, orc_det, name):
    c = _case(name, orc_det)
    depth, position, motion, ok = _np_planes(c.rays, c.t, c.hit, c.row, c.prev)
    assert ok[c.hit].all()  # a camera moved by 0.25 still sees every hit point in front of it
    _same(c.full, dict(depth=depth, position=position, motion=motion), f"{name}, previous camera moved by 0.25 in x")
    assert (depth[~c.hit] == 0x7F800000).all() and not position[~c.hit].any()
    # a previous camera behind the scene, looking away: every hit pixel takes the NaN pattern, exactly where NumPy's c * det > 0 is false
    w, h = c.size
    behind = _row(_behind(c.cam), w / h)
    _, _, motion_b, ok_b = _np_planes(c.rays, c.t, c.hit, c.row, behind)
    assert not ok_b[c.hit].any()
    got, _ = _gbuffer(c.r, ("motion",), prev=behind)
    assert np.array_equal(got["motion"], motion_b)
    assert np.array_equal((got["motion"] == QNAN).all(-1), ~ok_b)
    # sanity (the one bound of this file): previous camera == current camera -> no motion.  float32 NumPy gives at most 3.1e-5 pixel on these
    # inputs; 1e-3 is about 30 times that and catches a wrong sign or cross product, not rounding
    got, _ = _gbuffer(c.r, ("motion",), prev=c.row)
    still = got["motion"].view(f32)[c.hit]
    assert np.isfinite(still).all() and np.abs(still).max() < 1e-3, float(np.abs(still).max())


# ------------------------------------------------------------------ 3. plane subsets
@pytest.mark.parametrize("plane", PLANES)
def test_each_plane_alone(ptlib, orc_det, plane):
    c = _case("two_box", orc_det)
    got, stats = _gbuffer(c.r, (plane,), prev=c.prev if plane == "motion" else None)
    _same(got, c.full, f"{plane} alone")
    assert stats["hits"] == c.counts[0] and stats["pixels"] == W * H


_VIEW_WANT = {}


def _view_want():
    """each view's planes from a context of the view's own size with the view's camera (and its own previous camera)"""
    if not _VIEW_WANT:
        model = scenes.two_box_scene(shadow_catcher=False)
        _, prev = _views_and_prev()
        for k, ((x, y, w, h), cd) in enumerate(zip(RECTS, _cam_dicts())):
            r = _renderer(model, (w, h), cd)
            got, stats = _gbuffer(r, prev=prev[k])
            assert (stats["hits"], w * h - stats["hits"]) == VIEW_COUNTS[k]
            _VIEW_WANT[k] = got
            r.close()
    return _VIEW_WANT


@pytest.mark.parametrize("packets", ["1", "0"])
def test_views(ptlib, monkeypatch, packets):
    want = _view_want()
    monkeypatch.setenv("PT_CAM_PACKETS", packets)  # the G-buffer kernel does not read the switch; run both for symmetry with the views tests
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), (W, H), scenes.TWO_BOX_CAMERA)
    monkeypatch.delenv("PT_CAM_PACKETS")
    views, prev = _views_and_prev()
    r.setViews(views)
    got, stats = _gbuffer(r, prev=prev)
    inside = np.zeros((H, W), bool)
    for k, (x, y, w, h) in enumerate(RECTS):
        inside[y:y + h, x:x + w] = True
        for p in PLANES:
            assert np.array_equal(got[p][y:y + h, x:x + w], want[k][p]), f"view {k}, plane {p}"
    _untouched(got, ~inside, "views")
    assert stats["pixels"] == int(inside.sum()) and stats["hits"] == sum(a for a, _ in VIEW_COUNTS)
    # back to the single camera: the whole frame again
    r.setViews([])
    got, stats = _gbuffer(r, ("depth",))
    assert stats["pixels"] == W * H and not (got["depth"] == SENTINEL).any()
    r.close()


# ------------------------------------------------------------------ 5. mask
def test_mask(ptlib, orc_det):
    c = _case("two_box", orc_det)
    nby, nbx = c.r.blockGrid()
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.4
    mask[0, 0] = mask[nby - 1, nbx - 1] = mask[0, nbx - 1] = mask[nby - 1, 3] = True  # corner and edge blocks, the 3-wide column and the 5-high row
    mask[1, 1] = False
    got, stats = _gbuffer(c.r, prev=c.prev, mask=mask)
    px = pixel_mask(mask, h=H, w=W)
    _same(got, c.full, "masked-in pixels", px)
    _untouched(got, ~px, "mask")
    c.r.setProbe(scenes.sky_probe(64, 32).BuildCDF())  # (renderMask renders; the G-buffer pass needs no probe)
    c.r.launchParams.samples_per_launch = 1
    assert stats["pixels"] == c.r.renderMask(mask) == int(px.sum())
    assert stats["hits"] == int((c.hit & px).sum())
    got, stats = _gbuffer(c.r, prev=c.prev, mask=np.zeros((nby, nbx), bool))
    assert stats["pixels"] == 0 and stats["hits"] == 0
    _untouched(got, np.ones((H, W), bool), "the empty mask")


# ------------------------------------------------------------------ 6. partition
def test_partition(ptlib, orc_det):
    c = _case("two_box", orc_det)
    written = np.zeros((H, W), int)
    for rank in range(3):
        r = _renderer(c.model, c.size, c.cam, partition=(rank, 3, 8, 8))
        got, stats = _gbuffer(r, prev=c.prev)
        own = got["depth"] != SENTINEL  # (no depth has the sentinel's bits: a negative number)
        by, bx = np.mgrid[0:H, 0:W] // 8
        assert np.array_equal(own, (bx + by) % 3 == rank)
        assert stats["pixels"] == int(own.sum()) and stats["hits"] == int((c.hit & own).sum())
        _same(got, c.full, f"rank {rank}", own)
        _untouched(got, ~own, f"rank {rank}")
        written += own
        r.close()
    assert (written == 1).all()  # the union is the frame, overlaps are empty


# ------------------------------------------------------------------ 7. alignment and small frames
def test_planes_four_byte_aligned_only(ptlib, orc_det):
    c = _case("two_box", orc_det)
    got, stats = _gbuffer(c.r, prev=c.prev, offset=True)
    _same(got, c.full, "planes one float into their allocations")
    assert stats["hits"] == c.counts[0]


@pytest.mark.parametrize("size", [(1, 1), (8, 8), (9, 8), (63, 1), (65, 3)])
def test_small_frames(ptlib, orc_det, size):
    w, h = size
    model = scenes.two_box_scene(shadow_catcher=False)
    r = _renderer(model, size, scenes.TWO_BOX_CAMERA)
    rays = _np_rays(_row(scenes.TWO_BOX_CAMERA, w / h), w, h)
    t, prim = orc_det.trace_closest(orc_det.make_scene(model, use_bvh=True), rays.reshape(-1, 8))
    got, stats = _gbuffer(r, ("hit", "ray"))
    _check_ray_and_hit(r, got, stats, rays, np.asarray(t, f32).reshape(h, w), np.asarray(prim, np.int32).reshape(h, w), f"{w} x {h}")
    r.close()


# ------------------------------------------------------------------ 8. the rendering state is left alone
@pytest.mark.parametrize("frames_in_flight", [0, 3])
def test_rendering_state_is_left_alone(ptlib, frames_in_flight):
    probe = scenes.sky_probe(256, 128).BuildCDF()

    def run(with_call):
        r = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
        r.setProbe(probe)
        r.setOptions(frames_in_flight=frames_in_flight)
        r.resize((W, H))
        r.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, W / H))
        r.launchParams.samples_per_launch = 2
        for k in (0, 1):
            r.launchParams.frame.subframe_index = k
            r.render()
        if with_call:
            if frames_in_flight == 0:
                before = r.stats()
            got, stats = _gbuffer(r, prev=_row(_moved(scenes.TWO_BOX_CAMERA), W / H))
            assert stats["pixels"] == W * H and not (got["depth"] == SENTINEL).any()
            if frames_in_flight == 0:  # (with frames in flight the call completes them, and stats() would have, too)
                assert r.stats() == before
        allocs = r.stats()["path_state_allocs"]
        r.launchParams.frame.subframe_index = 2
        r.render()
        r.sync()
        bufs = [r.download(k) for k in range(5)]
        assert r.stats()["path_state_allocs"] == allocs
        r.close()
        return bufs, allocs

    (a, allocs_a), (b, allocs_b) = run(True), run(False)
    assert allocs_a == allocs_b
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), f"buffer {k} differs after a renderGBuffer between the frames"


# ------------------------------------------------------------------ 9. after a geometry update
@pytest.mark.parametrize("rebuild", [False, True], ids=["refit", "rebuild"])
def test_after_a_geometry_update(ptlib, orc_det, rebuild):
    c = _case("two_box", orc_det)
    moved = _with_vertices(c.model, {1: _np_transform(M1, c.model.meshes[1].vertex)})
    fresh = _renderer(moved, c.size, c.cam)
    want, wstats = _gbuffer(fresh, prev=c.prev)
    fresh.close()
    r = _renderer(c.model, c.size, c.cam)
    r.transformMeshes({1: M1}, rebuild=rebuild)
    got, stats = _gbuffer(r, prev=c.prev)
    r.close()
    _same(got, want, "after transformMeshes")
    assert stats["hits"] == wstats["hits"] and not np.array_equal(want["hit"], c.full["hit"])  # the update moved something under the camera


def test_refusals(ptlib, orc_det):
    c = _case("two_box", orc_det)
    L = _lib.load_library()
    r = R.SampleRenderer(c.model)
    planes = {p: _filled(p, H, W) for p in PLANES}
    prev = np.ascontiguousarray(c.prev, f32)

    def refused(what, pattern, **fields):
        d = _lib.GBufferDesc()
        for k, v in fields.items():
            setattr(d, k, v)
        torch.cuda.synchronize()
        s = _lib.GBufferStats(7, 7, 7.0)
        rc = L.pt_render_gbuffer(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_render_gbuffer") and pattern in msg, f"{what}: {msg!r}"
        assert (s.pixels, s.hits, s.kernel_ms) == (7, 7, 7.0)
        for p, t in planes.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: plane {p} was written"

    ptr = {p: t.data_ptr() for p, t in planes.items()}
    refused("no resize yet", "pt_resize", depth=ptr["depth"])
    r.resize((W, H))
    r.setCamera(R.make_camera(c.cam, W / H))
    assert L.pt_render_gbuffer(r._ctx, None, None) == -1 and "null description" in L.pt_last_error(r._ctx).decode()
    refused("no plane at all", "no plane")
    host = np.zeros((H, W), f32)
    refused("a host pointer", "depth is not device memory", depth=host.ctypes.data, hit=ptr["hit"])
    refused("a pointer offset by 2 bytes", "position is not 4-byte aligned", position=ptr["position"] + 2)
    # one element too small for what is left of its allocation (an allocation of the runtime's own: torch's allocator hands out parts of larger ones)
    hip = _hip_runtime()
    raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(raw), C.c_size_t(H * W * 8)) == 0
    try:
        assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= H * W * 8
        refused("a plane one element too small", f"motion has fewer than {H * W * 8} bytes left", motion=raw.value + size.value - (H * W * 8 - 4),
                prev_cameras=prev.ctypes.data, num_prev_cameras=1, ray=ptr["ray"])
    finally:
        assert hip.hipFree(raw) == 0
    both = torch.zeros(2 * H * W * 8, dtype=torch.float32, device="cuda:0")  # room for either plane at either address
    refused("two planes sharing memory", "hit and ray overlap", hit=both.data_ptr(), ray=both.data_ptr() + 16)
    assert not _bits(both).any()
    refused("depth inside position", "depth and position overlap", depth=ptr["position"] + 4 * (H * W * 3), position=ptr["position"])
    refused("motion without previous cameras", "motion needs prev_cameras", motion=ptr["motion"])
    refused("two previous cameras without views", "num_prev_cameras is 2, expected 1", motion=ptr["motion"], prev_cameras=np.tile(prev, 2).ctypes.data, num_prev_cameras=2)
    refused("no previous camera count", "num_prev_cameras is 0, expected 1", motion=ptr["motion"], prev_cameras=prev.ctypes.data)
    bad = prev.copy()
    bad[7] = np.inf
    refused("an infinite previous camera value", "prev_cameras: value 7 is not finite", motion=ptr["motion"], prev_cameras=bad.ctypes.data, num_prev_cameras=1)
    bad[7] = np.nan
    refused("a NaN previous camera value", "prev_cameras: value 7 is not finite", depth=ptr["depth"], prev_cameras=bad.ctypes.data, num_prev_cameras=1)
    views = [(x, y, w, h, R.make_camera(cd, w / h)) for (x, y, w, h), cd in zip(RECTS, _cam_dicts())]
    r.setViews(views)
    refused("one previous camera for four views", "num_prev_cameras is 1, expected 4", motion=ptr["motion"], prev_cameras=prev.ctypes.data, num_prev_cameras=1)
    r.setViews([])
    # the Python facade checks dtype, shape and device before the library is called
    with pytest.raises(ValueError, match="depth.*shape"):
        r.renderGBuffer(("depth",), out=dict(depth=planes["position"]))
    with pytest.raises(ValueError, match="hit.*float32"):
        r.renderGBuffer(("hit",), out=dict(hit=torch.zeros((H, W, 8), dtype=torch.int32, device="cuda:0")))
    with pytest.raises(ValueError, match="the tensor is on cpu"):
        r.renderGBuffer(("depth",), out=dict(depth=torch.zeros((H, W))))
    with pytest.raises(ValueError, match="unknown plane"):
        r.renderGBuffer(("normal",))
    with pytest.raises(RuntimeError, match="motion needs prev_cameras"):
        r.renderGBuffer(("motion",))
    # a valid call afterwards still works, into the same planes
    res = r.renderGBuffer(PLANES, prev_cameras=c.prev, out=planes)
    _same({p: _bits(planes[p]) for p in PLANES}, c.full, "a valid call after the refusals")
    assert res["stats"]["hits"] == c.counts[0]
    # ... and so does one that lets the facade allocate
    res = r.renderGBuffer(("hit", "depth"))
    _same({p: _bits(res[p]) for p in ("hit", "depth")}, c.full, "allocated planes")
    r.close()
