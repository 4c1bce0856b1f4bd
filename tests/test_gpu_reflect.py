"""Mirror reflections from the G-buffer (pt_reflect_layout, pt_reflect_planes) on the GPU.  hit2, position2, ray and sky are compared word
for word over WHOLE sentinel-filled planes, and every counter exactly, with an expectation the code under test never produces:
tests/reflect_ref.py builds the rays in float32 NumPy from the same hit and position planes, the EXISTING traceDevice(any_hit=False)
returns their pt_hit records, NumPy scatters them and computes position2, and the EXISTING evalTable(3) gives the probe's texel along every
ray.  The scratch is exactly pt_reflect_layout's bytes between guard words (its content is not specified: slots are handed out by
atomics).  Frames are 64 x 40 and smaller, but for the four views of scene_kit.RECTS (131 x 61)."""
import ctypes as C

import numpy as np
import pytest
import torch

import reflect_ref as F
from gpu_kit import bits3 as _bits
from gpu_kit import filled, pixel_mask
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from gpu_kit import words_differ as _differ
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from scene_kit import RECTS, VIEW_H, VIEW_W

pytestmark = pytest.mark.gpu

f32 = np.float32
u32 = np.uint32
i32 = np.int32
W, H = 64, 40
GUARD = 4  # sentinel words on either side of the scratch (16 bytes: the scratch stays 16-byte aligned)
SENTINEL = F.SENTINEL
CAM = scenes.TWO_BOX_CAMERA
BEHIND = dict(CAM, eye=(3.0, 2.5, 5.0))
PLANES = F.PLANES
NO_SKY = ("hit2", "position2", "ray")
WALL = [(-3.0, 0.0, 0.6), (3.0, 0.0, 0.6), (3.0, 3.0, 0.6), (-3.0, 3.0, 0.6)]


def _scene():
    """pt_ao_planes's scene: the unit box on its ground slab, and one free-standing quad 0.1 behind the box, seen from both sides"""
    m = scenes.two_box_scene(False)
    m.meshes.append(scenes._quads_to_mesh([WALL], scenes.Material(color=(0.7, 0.7, 0.7))))
    return m


def _probe():
    return scenes.sky_probe(256, 128).BuildCDF()


def _all(h=H, w=W):
    return np.ones((h, w), bool)


def _scratch(nbytes):
    n = nbytes // 4
    buf = torch.full((4 * (n + 2 * GUARD),), 0xA5, dtype=torch.uint8, device="cuda:0").view(torch.int32)
    t = buf[GUARD:GUARD + n].view(torch.float32)
    assert t.is_contiguous() and t.data_ptr() % 16 == 0
    return buf, t


def _gbuffer(r, mask=None):
    g = r.renderGBuffer(planes=("hit", "position"), mask=mask)
    return _np(g["hit"]), _np(g["position"])


def _cams(r, views=None):
    """the (nv, 12) rows of the context's cameras: the views' own, or the one of setCamera"""
    if views:
        return R._camera_rows([v[4] for v in views])
    return R._camera_rows([r._test_camera])


def _expect(r, hit, pos, pixels, rects=None, cams=None, sky=True, max_rays_in_flight=0, **prm):
    """the reference: reflect_ref's rays through the existing closest-hit query of the same context, scattered in NumPy; the probe's texels
    from the existing function table"""
    Rr = F.rays_of(hit, pos, cams if cams is not None else _cams(r), rects, pixels, prm.get("bias", 1e-3), prm.get("max_distance", F.DEFAULT_MAX_DISTANCE))
    n = len(Rr["rays"])
    rec, rgb = np.zeros((n, 8), u32), None
    if n:
        rec = _np(r.traceDevice(torch.from_numpy(Rr["rays"]).to("cuda:0"), any_hit=False)["record"]).view(u32)
        assert np.array_equal(rec[:, 3].view(i32) == -2, ~Rr["valid"]), "the reference's validity rule is not pt_trace_device's"
    if sky:
        dirs = np.where(Rr["valid"][:, None], Rr["rays"][:, 4:7], np.array([0, 1, 0], f32)).astype(f32)  # (an invalid ray's texel is never used)
        rgb = r.evalTable(3, dirs, 6)[:, 2:5] if n else np.zeros((0, 3), f32)
    return F.scatter(rec, Rr, pixels, rgb, max_rays_in_flight), Rr


def _reflect(r, hit, pos, pixels, what, rects=None, cams=None, mask=None, offset=False, planes=PLANES, ref=None, **prm):
    """reflectPlanes into sentinel-filled planes and a guarded scratch of exactly pt_reflect_layout's bytes, against the reference: the
    layout, every plane over the whole frame, the eight counters; hit and position are unchanged afterwards.  Returns the reference."""
    h, w = pixels.shape
    M = prm.get("max_rays_in_flight", 0)
    nbytes = r.reflectLayout(M)
    assert nbytes == F.layout(h, w, M), f"{what}: the layout is {nbytes} bytes, the reference {F.layout(h, w, M)}"
    if ref is None:
        ref, _ = _expect(r, hit, pos, pixels, rects, cams, sky="sky" in planes, **prm)
    hdev, pdev = _upload(hit, offset), _upload(pos, offset)
    outs = {n: filled((h, w, F.WORDS[n]), offset) for n in planes}
    sbuf, scratch = _scratch(nbytes)
    res = r.reflectPlanes(hdev, pdev, scratch=scratch, mask=mask, **outs, **prm)
    st = res["stats"]
    print(f"{what}: {({k: st[k] for k in F.COUNTERS})}, {st['kernel_ms']:.4f} ms, trace {st['trace_ms']:.4f} ms")
    for n in PLANES:
        if n not in planes:
            assert res[n] is None
            continue
        assert res[n] is outs[n]
        got = _bits(outs[n])
        neq = _differ(got, ref[n])
        assert not neq.any(), f"{what}: {n} differs in {int(neq.sum())} words, first at {np.argwhere(neq)[:3].tolist()}"
    words = _np(sbuf).view(u32)
    assert (words[:GUARD] == SENTINEL).all() and (words[-GUARD:] == SENTINEL).all(), f"{what}: a word outside the scratch was written"
    assert {k: st[k] for k in F.COUNTERS} == {k: ref[k] for k in F.COUNTERS}, (what, st, {k: ref[k] for k in F.COUNTERS})
    assert st["pixels"] == st["traced"] + st["skipped"] + st["nonfinite"] and st["traced"] == st["invalid"] + st["hits"] + st["escaped"]
    assert st["trace_ms"] <= st["kernel_ms"]
    assert np.array_equal(_np(hdev).view(u32), np.ascontiguousarray(hit, f32).view(u32)), f"{what}: hit was written"
    assert np.array_equal(_np(pdev).view(u32), np.ascontiguousarray(pos, f32).view(u32)), f"{what}: position was written"
    return ref


def _make(size, cam=CAM, partition=None, model=None, probe=True):
    r = _renderer(model or _scene(), size, cam, partition=partition)
    r._test_camera = R.make_camera(cam, size[0] / size[1])
    if probe:
        r.setProbe(_probe())
    return r


_CASES = {}


def _frame():
    """a W x H renderer on the scene, with a probe, and its G-buffer's two planes, shared by the tests that only read them"""
    if "frame" not in _CASES:
        r = _make((W, H))
        hit, pos = _gbuffer(r)
        for a in (hit, pos):
            a.setflags(write=False)
        _CASES["frame"] = (r, hit, pos)
    return _CASES["frame"]


def _default():
    """the reference of the shared frame with every output: computed once"""
    if "default" not in _CASES:
        r, hit, pos = _frame()
        _CASES["default"] = _expect(r, hit, pos, _all())[0]
    return _CASES["default"]


# ------------------------------------------------------------------ 1. outputs
def test_all_outputs(ptlib):
    r, hit, pos = _frame()
    ref = _reflect(r, hit, pos, _all(), "all outputs", ref=_default())
    assert ref["hits"] > 0 and ref["escaped"] > 0 and ref["skipped"] > 0 and ref["invalid"] == 0 and ref["batches"] == 1
    hit2, sky = ref["hit2"], ref["sky"].view(f32)
    traced = np.zeros(H * W, bool)
    traced[_expect(r, hit, pos, _all(), sky=False)[1]["pixel"]] = True
    traced = traced.reshape(H, W)
    escaped = traced & (hit2[..., 3].view(i32) == -1)
    assert (sky[escaped][:, 3] == 1).all() and (sky[escaped][:, 0:3] > 0).any() and (sky[~escaped] == 0).all()
    assert (hit2[escaped][:, 0].view(f32) == f32(1e16)).all()
    # the reflections see more than one mesh: the slab mirrors the box and the wall, the box and the wall mirror the slab
    assert len(np.unique(hit2[traced & ~escaped][:, 4])) >= 2


@pytest.mark.parametrize("planes", [("hit2",), ("position2",), ("ray",), ("sky",), ("hit2", "sky")], ids="+".join)
def test_each_output_alone(ptlib, planes):
    r, hit, pos = _frame()
    _reflect(r, hit, pos, _all(), f"only {planes}", planes=planes, ref=_default())


def test_the_facade_allocates_hit2_and_scratch(ptlib):
    r, hit, pos = _frame()
    res = r.reflectPlanes(_upload(hit), _upload(pos))
    assert res["position2"] is None and res["ray"] is None and res["sky"] is None and not _differ(_bits(res["hit2"]), _default()["hit2"]).any()
    assert res["scratch"].numel() * 4 == F.layout(H, W)


# ------------------------------------------------------------------ 2. batches
def test_one_pixel_per_batch(ptlib):
    w, h = 16, 8
    r = _make((w, h))
    hit, pos = _gbuffer(r)
    ref = _reflect(r, hit, pos, _all(h, w), "16 x 8, max_rays_in_flight = 1", max_rays_in_flight=1)
    assert ref["batches"] == w * h
    whole = _reflect(r, hit, pos, _all(h, w), "16 x 8, the default")
    assert whole["batches"] == 1 and all(np.array_equal(whole[n], ref[n]) for n in PLANES)
    r.close()


@pytest.mark.parametrize("M", [63, 64, 65, 1023, 1024, 1025, W * H - 1, W * H, 1 << 30, 0])
def test_the_result_does_not_depend_on_the_batch(ptlib, M):
    """a boundary inside a wave, on one and one pixel behind it; inside a workgroup of k_reflect_rays (1024 pixels), on one and behind it;
    one pixel short of the frame, the frame, more than it, the default"""
    r, hit, pos = _frame()
    ref = dict(_default(), batches=F.batches_of(W * H, H, W, M))
    _reflect(r, hit, pos, _all(), f"max_rays_in_flight {M}", ref=ref, max_rays_in_flight=M)
    assert ref["batches"] == -(-W * H // min(M or 1 << 23, W * H))


def test_the_layout_grows_with_the_batch_and_stops_at_the_frame(ptlib):
    r, _, _ = _frame()
    sizes = [r.reflectLayout(M) for M in (1, 2, 100, W * H - 1, W * H, W * H + 1, (1 << 32) - 1, 0)]
    assert sizes[:5] == sorted(set(sizes[:5])) and sizes[4] == sizes[5] == sizes[6] == sizes[7] == 256 + W * H * 44
    assert sizes[0] == 304 and sizes[1] == (256 + 88 + 15) // 16 * 16 == 352 and sizes[2] == 256 + 4400


# ------------------------------------------------------------------ 3. sizes, alignment, masks
@pytest.mark.parametrize("size", [(1, 1), (63, 5)])
def test_sizes(ptlib, size):
    w, h = size
    r = _make(size)
    hit, pos = _gbuffer(r)
    _reflect(r, hit, pos, _all(h, w), f"{w} x {h}")
    _reflect(r, hit, pos, _all(h, w), f"{w} x {h}, 7 rays in flight", max_rays_in_flight=7)
    r.close()


def test_every_plane_one_float_into_its_allocation(ptlib):
    r, hit, pos = _frame()
    _reflect(r, hit, pos, _all(), "every plane 4 bytes off a 16-byte boundary", offset=True, ref=_default())


def test_block_masks(ptlib):
    r, hit, pos = _frame()
    nby, nbx = r.blockGrid()
    rng = np.random.default_rng(4)
    for name, m in (("random", rng.random((nby, nbx)) < 0.4), ("one block", np.arange(nby * nbx).reshape(nby, nbx) == 17), ("empty", np.zeros((nby, nbx), bool))):
        ref = _reflect(r, hit, pos, pixel_mask(m, h=H, w=W), f"mask: {name}", mask=m, max_rays_in_flight=100)
        assert ref["pixels"] == int(m.sum()) * 64
        if name == "empty":
            assert ref["batches"] == 0 and all((ref[n] == SENTINEL).all() for n in PLANES)


# ------------------------------------------------------------------ 4. views and partitions
def test_two_sides_of_a_wall_in_four_views(ptlib):
    """RECTS with two cameras in front of the free-standing quad and two behind it: pixels in no view are untouched, and the ray is mirrored
    about the normal turned to each view's own eye — with the cameras of the other side the reference gives other planes"""
    w, h = VIEW_W, VIEW_H
    r = _make((w, h))
    dicts = [CAM, BEHIND, dict(CAM, eye=(2.5, 2.0, -4.5)), dict(BEHIND, fovY=55.0)]
    views = [(x, y, ww, hh, R.make_camera(c, ww / hh)) for (x, y, ww, hh), c in zip(RECTS, dicts)]
    r.setViews(views)
    inside = np.zeros((h, w), bool)
    for x, y, ww, hh in RECTS:
        inside[y:y + hh, x:x + ww] = True
    hit, pos = _gbuffer(r)
    cams = _cams(r, views)
    ref = _reflect(r, hit, pos, inside, "four views", rects=RECTS, cams=cams)
    assert ref["pixels"] == int(inside.sum()) and all((ref[n][~inside] == SENTINEL).all() for n in PLANES) and ref["hits"] > 0 and ref["escaped"] > 0
    wrong, _ = _expect(r, hit, pos, inside, rects=RECTS, cams=cams[[1, 0, 3, 2]])
    assert _differ(wrong["ray"], ref["ray"]).any() and _differ(wrong["hit2"], ref["hit2"]).any(), "the scene cannot tell one view's eye from another's"
    m = np.random.default_rng(8).random(r.blockGrid()) < 0.5
    _reflect(r, hit, pos, inside & pixel_mask(m, h=h, w=w), "four views under a mask", rects=RECTS, cams=cams, mask=m, max_rays_in_flight=333)
    r.close()


def test_partitions_add_up(ptlib):
    _, hit, pos = _frame()
    whole = _default()
    by, bx = np.mgrid[0:H, 0:W] // 8
    union = {n: np.full(whole[n].shape, SENTINEL, u32) for n in PLANES}
    model = _scene()
    for rank in range(2):
        rr = _make((W, H), partition=(rank, 2, 8, 8), model=model)
        own = (bx + by) % 2 == rank
        part = _reflect(rr, hit, pos, own, f"rank {rank} of 2")
        assert part["pixels"] == int(own.sum())
        for n in PLANES:
            assert (union[n][own] == SENTINEL).all()
            union[n][own] = part[n][own]
        rr.close()
    for n in PLANES:
        assert not _differ(union[n], whole[n]).any(), n


# ------------------------------------------------------------------ 5. misses, hostile records, parameters
def test_misses_and_hostile_records(ptlib):
    r, hit, pos = _frame()
    clean = _default()
    hit, pos = hit.copy(), pos.copy()
    hits = np.argwhere(hit[..., 3].view(i32) >= 0)
    assert len(hits) > 64 and (hit[..., 3].view(i32) < 0).any()
    pick = hits[np.random.default_rng(6).permutation(len(hits))[:15]]
    nan, inf = f32(np.nan), f32(np.inf)
    edits = [("hit", 5, nan), ("hit", 6, inf), ("hit", 7, -inf), ("hit", 0, nan), ("hit", 0, inf), ("hit", 0, f32(0.0)), ("hit", 0, f32(-0.0)), ("hit", 0, f32(-2.0)),
             ("pos", 0, nan), ("pos", 1, -inf), ("pos", 2, inf)]
    for (y, x), (plane, word, value) in zip(pick, edits):
        (hit if plane == "hit" else pos)[y, x, word] = value
    for (y, x), prim in zip(pick[11:14], (0x7FFFFFFF, 12345678, 36)):  # stale primitives: no address is formed from them
        hit[y, x, 3] = np.array([prim], i32).view(f32)[0]
    y, x = pick[14]
    pos[y, x, 0:3] = R._camera_rows([r._test_camera])[0, 0:3]  # the eye itself: d = 0 * inf, an invalid ray
    ref = _reflect(r, hit, pos, _all(), "hostile records")
    assert ref["nonfinite"] == 11 and ref["skipped"] == clean["skipped"] > 0 and ref["traced"] == clean["traced"] - 11 and ref["invalid"] == 1
    for y, x in pick[:11]:
        assert np.array_equal(ref["hit2"][y, x], F.EMPTY_HIT) and not ref["sky"][y, x].any() and np.array_equal(ref["ray"][y, x].view(f32), F.NEUTRAL_RAY)
    for y, x in pick[11:14]:
        assert all(np.array_equal(ref[n][y, x], clean[n][y, x]) for n in PLANES)
    y, x = pick[14]
    assert np.array_equal(ref["hit2"][y, x], F.INVALID_HIT) and not ref["position2"][y, x].any() and np.isnan(ref["ray"][y, x].view(f32)[4:7]).all()
    miss = hit[..., 3].view(i32) < 0
    assert (ref["hit2"][miss] == F.EMPTY_HIT).all() and (ref["ray"][miss].view(f32) == F.NEUTRAL_RAY).all() and not ref["position2"][miss].any()


@pytest.mark.parametrize("prm", [dict(bias=0.0), dict(bias=0.05), dict(max_distance=1e-6), dict(max_distance=1e30), dict(max_distance=2.0)],
                         ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()))
def test_bias_and_max_distance(ptlib, prm):
    r, hit, pos = _frame()
    ref = _reflect(r, hit, pos, _all(), f"{prm}", **prm)
    if prm.get("max_distance") == 1e-6:
        assert ref["hits"] == 0 and ref["escaped"] == ref["traced"] > 0
    if prm.get("max_distance") == 1e30:
        assert ref["hits"] == _default()["hits"] and _differ(ref["hit2"], _default()["hit2"]).any()  # (the escaped rays' t)
    if prm.get("max_distance") == 2.0:
        assert 0 < ref["hits"] <= _default()["hits"] and ref["escaped"] >= _default()["escaped"]


def test_the_pass_follows_the_current_tree(ptlib):
    """the same G-buffer before and after transformMeshes has moved the box away: both match the query over the geometry of the moment"""
    r = _make((W, H))
    hit, pos = _gbuffer(r)
    before = _reflect(r, hit, pos, _all(), "the box in place")
    r.transformMeshes({0: np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -10.0]], f32)})
    after = _reflect(r, hit, pos, _all(), "the box moved away")
    assert _differ(after["hit2"], before["hit2"]).any() and not _differ(after["ray"], before["ray"]).any()
    r.close()


@pytest.mark.parametrize("ceiling", [True, False], ids=["lid", "open"])
def test_two_analytic_scenes(ptlib, ceiling):
    """tests/test_reflect_cabi.py's two scenes on the GPU's tree, without a probe: under the lid every ray hits the lid's mesh, position2 on
    it; without it every ray escapes"""
    hit, pos, cam = F.analytic_planes()
    h, w = hit.shape[:2]
    model = scenes.Model([scenes._quads_to_mesh([q], scenes.Material()) for q in F.analytic_quads(ceiling)])
    r = R.SampleRenderer(model)
    r.resize((w, h))
    r.setCamera(R.Camera(F.ANALYTIC_EYE, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 35.0, w / h))
    assert np.array_equal(R._camera_rows([R.Camera(F.ANALYTIC_EYE, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 35.0, w / h)])[0, 0:3], cam[0, 0:3])
    ref = _reflect(r, hit, pos, _all(h, w), f"analytic, lid {ceiling}", cams=cam, planes=NO_SKY, max_distance=100.0)
    if ceiling:
        assert ref["hits"] == h * w and (ref["hit2"][..., 4].view(i32) == 1).all()
        assert np.abs(ref["position2"].view(f32)[..., 1] - F.LID).max() <= 1e-5
        t, _, _ = F.closest_hit_quads(ref["ray"].view(f32).reshape(-1, 8), F.analytic_quads(True))
        assert np.abs(ref["hit2"][..., 0].view(f32).reshape(-1) - t).max() <= 1e-5
    else:
        assert ref["escaped"] == h * w and (ref["hit2"][..., 3].view(i32) == -1).all() and (ref["hit2"][..., 0].view(f32) == f32(100.0)).all()
    r.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals(ptlib):
    L = _lib.load_library()
    r = R.SampleRenderer(_scene())
    _, hit, pos = _frame()
    hdev, pdev = _upload(hit), _upload(pos)
    outs = {n: filled((H, W, F.WORDS[n])) for n in PLANES}
    nbytes = F.layout(H, W)
    sbuf, scratch = _scratch(nbytes)
    good = dict(hit=hdev.data_ptr(), position=pdev.data_ptr(), hit2=outs["hit2"].data_ptr(), position2=outs["position2"].data_ptr(), ray=outs["ray"].data_ptr(),
                sky=None, scratch=scratch.data_ptr(), bias=1e-3, max_distance=1e16, max_rays_in_flight=0, flags=0)

    def untouched(what):
        assert (_np(sbuf).view(u32) == SENTINEL).all(), f"{what}: the scratch was written"
        for n in PLANES:
            assert (_bits(outs[n]) == SENTINEL).all(), f"{what}: {n} was written"

    def refused(what, pattern, **fields):
        d = _lib.ReflectDesc()
        for n, v in dict(good, **fields).items():
            setattr(d, n, v)
        torch.cuda.synchronize()
        s = _lib.ReflectStats(7, 7, 7, 7, 7, 7, 7, 7, 7.0, 7.0)
        rc = L.pt_reflect_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_reflect_planes") and pattern in msg, f"{what}: {msg!r}"
        assert tuple(getattr(s, n) for n, _ in s._fields_) == (7, 7, 7, 7, 7, 7, 7, 7, 7.0, 7.0)
        untouched(what)

    def layout_refused(what, pattern, M=0, with_bytes=True):
        nb = C.c_size_t(77)
        rc = L.pt_reflect_layout(r._ctx, M, C.byref(nb) if with_bytes else None)
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1 and msg.startswith("pt_reflect_layout") and pattern in msg, f"{what}: {rc}, {msg!r}"
        assert nb.value == 77, f"{what}: bytes was written"

    refused("no resize yet", "pt_resize")
    layout_refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(CAM, W / H))
    layout_refused("bytes null", "bytes is null", with_bytes=False)
    assert L.pt_reflect_planes(r._ctx, None, None) == -1 and "pt_reflect_planes: null description" in L.pt_last_error(r._ctx).decode()
    refused("an unknown flag", "unknown flag bits 1", flags=1)
    refused("an unknown flag", "unknown flag bits 2147483648", flags=0x80000000)
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf")):
        refused(f"bias {bad}", "bias must be finite and >= 0", bias=bad)
    for bad in (0.0, -0.0, -1.0, float("nan"), float("inf")):
        refused(f"max_distance {bad}", "max_distance must be finite and > 0", max_distance=bad)
    for name in ("hit", "position", "scratch"):
        refused(f"{name} null", f"{name} is null", **{name: None})
    refused("no output", "no output asked for", hit2=None, position2=None, ray=None, sky=None)
    refused("sky without a probe", "no probe set (setProbe)", sky=outs["sky"].data_ptr())
    refused("only sky without a probe", "no probe set (setProbe)", hit2=None, position2=None, ray=None, sky=outs["sky"].data_ptr())
    host = np.zeros((H, W, 8), f32)
    refused("a host pointer", "hit is not device memory", hit=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "ray is not 4-byte aligned", ray=good["ray"] + 2)
    for off in (4, 8, 2):
        refused(f"the scratch {off} bytes off", "scratch is not 16-byte aligned", scratch=good["scratch"] + off)
    big = torch.zeros(2 * H * W * 8 + 8, dtype=torch.float32, device="cuda:0")
    refused("hit2 inside hit", "hit and hit2 overlap", hit=big.data_ptr(), hit2=big.data_ptr() + 16)
    refused("position2 inside position", "position and position2 overlap", position=big.data_ptr() + 64, position2=big.data_ptr())
    refused("hit2 exactly ray", "hit2 and ray overlap", hit2=good["ray"])
    refused("position2 inside hit2", "hit2 and position2 overlap", position2=good["hit2"] + 32)
    refused("the scratch inside hit", "hit and scratch overlap", scratch=good["hit"] + 16)
    refused("the scratch inside ray", "ray and scratch overlap", scratch=good["ray"] + 32)
    hip = _hip_runtime()
    for name, nb in (("scratch", nbytes), ("ray", H * W * 32)):
        raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert hip.hipMalloc(C.byref(raw), C.c_size_t(nb)) == 0
        try:
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= nb
            refused(f"{name} one element too small", f"{name} has fewer than {nb} bytes left", **{name: raw.value + size.value - (nb - 16)})
        finally:
            assert hip.hipFree(raw) == 0
    # the Python facade passes the library's refusals on; a valid call afterwards works, into the same arrays, without a probe and without sky
    with pytest.raises(RuntimeError, match="hit2 and ray overlap"):
        r.reflectPlanes(hdev, pdev, hit2=outs["hit2"], ray=outs["hit2"])
    with pytest.raises(RuntimeError, match=r"no probe set \(setProbe\)"):
        r.reflectPlanes(hdev, pdev, sky=outs["sky"])
    with pytest.raises(ValueError, match=r"scratch: a contiguous torch.float32 tensor of shape \(%d,\) is expected" % (nbytes // 4)):
        r.reflectPlanes(hdev, pdev, scratch=torch.zeros((nbytes // 4 + 4,), device="cuda:0"))
    untouched("the facade's refusals")
    r._test_camera = R.make_camera(CAM, W / H)
    ref, _ = _expect(r, hit, pos, _all(), sky=False)
    res = r.reflectPlanes(hdev, pdev, scratch=scratch, **{n: outs[n] for n in NO_SKY})
    for n in NO_SKY:
        assert not _differ(_bits(outs[n]), ref[n]).any(), n
        assert not _differ(ref[n], _default()[n]).any(), n  # (the probe plays no part in them)
    assert (_bits(outs["sky"]) == SENTINEL).all()
    assert {k: res["stats"][k] for k in F.COUNTERS} == {k: ref[k] for k in F.COUNTERS}
    r.close()


# ------------------------------------------------------------------ 7. state and ordering
def test_queued_queries_and_rendering_state(ptlib):
    """asynchronous queries queued in front of the call are completed by it, and queryWait still delivers their counts; stats() and the
    frame buffers are what they were"""
    r = _make((W, H))
    r.launchParams.samples_per_launch = 1
    r.render()
    hit, pos = _gbuffer(r)
    ref, Rr = _expect(r, hit, pos, _all())
    r.queryWait()
    rays = torch.from_numpy(Rr["rays"]).to("cuda:0")
    queued = [r.traceDevice(rays, any_hit=False, wait=False) for _ in range(2)]
    before, frame = r.stats(), r.download(R.PT_BUF_ACCUM)
    res = r.reflectPlanes(_upload(hit), _upload(pos), hit2=filled((H, W, 8)), sky=filled((H, W, 4)))
    assert r.stats() == before and r.download(R.PT_BUF_ACCUM).tobytes() == frame.tobytes()
    assert not _differ(_bits(res["hit2"]), ref["hit2"]).any() and not _differ(_bits(res["sky"]), ref["sky"]).any()
    q = r.queryWait()
    assert q["rays"] == 2 * len(Rr["rays"]) and q["hits"] == 2 * ref["hits"] and q["invalid_rays"] == 0
    for t in queued:
        assert np.array_equal(_np(t["record"]).view(u32), ref["hit2"].reshape(-1, 8)[Rr["pixel"]])
    assert r.queryWait()["rays"] == 0
    r.close()


@pytest.mark.parametrize("mode", ["default", "side"])
def test_under_a_busy_torch_stream(ptlib, mode):
    """tests/test_gpu_stream_contract.py's protocol: the planes are produced, and the outputs sentinel-filled, by work still pending on
    torch's current stream when the call is made; the result equals the synchronous call's, and that equals the reference"""
    from stream_kit import _pin, _res

    r, hit, pos = _frame()
    outs = {n: filled((H, W, F.WORDS[n])) for n in PLANES}
    scratch = torch.zeros((r.reflectLayout() // 4,), dtype=torch.float32, device="cuda:0")  # (not an output of the case: its slots are handed out by atomics)

    def reflection(dev, outs, returned):
        res = r.reflectPlanes(dev["hit"], dev["position"], scratch=scratch, **outs)
        returned()
        return _res(res, outs)

    sync, got = _pin("reflectPlanes", mode, r, dict(hit=hit, position=pos), outs, reflection)
    ref = _default()
    for n in PLANES:
        assert not _differ(got[n].view(u32).reshape(ref[n].shape), ref[n]).any(), f"{n} under a busy stream [{mode}]"
    assert got["stats"] == {k: ref[k] for k in F.COUNTERS}


# ------------------------------------------------------------------ 8. the chain on the second G-buffer
def test_surface_planes_on_the_reflected_hits(ptlib):
    """surfacePlanes(hit=hit2) is the reflected surface's albedo: surface_ref on the expected hit2"""
    import surface_ref as S

    r, hit, pos = _frame()
    ref = _default()
    res = r.reflectPlanes(_upload(hit), _upload(pos))
    assert not _differ(_bits(res["hit2"]), ref["hit2"]).any()
    alb = r.surfacePlanes(res["hit2"])
    want = S.surface_ref(ref["hit2"], S.scene_arrays(_scene()), _all(), planes=("albedo",))
    assert not _differ(_bits(alb["albedo"]), want["albedo"]).any()
    assert alb["stats"]["hits"] == want["hits"] == ref["hits"] and alb["stats"]["stale"] == 0


# ------------------------------------------------------------------ 9. the upsampled loop with --reflect
def _example(name):
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def test_upsampled_loop_with_reflect_mirrors_the_floor(ptlib):
    """examples/upsampled_svgf_loop.py's UpsampledLoop with reflect at 128 x 56, scale 2: hit2 and sky are reflectPlanes of the full-size
    G-buffer, the reflected albedo is surfacePlanes of hit2, and the floor's pixels (mesh 0) are the only ones the reflection changes"""
    import surface_ref as S

    ex = _example("upsampled_svgf_loop")
    w, h = 128, 56
    cam0 = dict(eye=(2.0, 0.35, -3.0), lookat=(0.0, 0.2, 0.5), up=(0.0, 1.0, 0.0), fovY=35.0)
    model = S.textured_scene()
    up = ex.UpsampledLoop(model, (w, h), 2, probe=_probe(), reflect=True, reflect_mesh=0, reflectivity=0.25)
    plain = ex.UpsampledLoop(model, (w, h), 2, probe=_probe())
    cam = R.make_camera(cam0, w / h)
    for k in range(2):
        prev, cam = cam, R.make_camera(ex.orbit(cam0, 0.02 * k), w / h)
        x = up.frame(k, prev, cam)
        plain.frame(k, prev, cam)
        assert x["pixels"] == w * h and x["reflect_ms"] > 0 and x["reflect_trace_ms"] > 0 and x["reflect_batches"] == 1
        assert x["reflect_hits"] > 0 and x["reflect_escaped"] > 0 and 0 < x["mirrored"] < w * h
    ref, _ = _expect(up.hi, _np(up.hi_gbuf["hit"]), _np(up.hi_gbuf["position"]), _all(h, w), cams=R._camera_rows([cam]))
    assert not _differ(_bits(up.hit2), ref["hit2"]).any() and not _differ(_bits(up.sky), ref["sky"]).any()
    assert (x["reflect_hits"], x["reflect_escaped"]) == (ref["hits"], ref["escaped"])
    want = S.surface_ref(ref["hit2"], S.scene_arrays(model), _all(h, w), planes=("albedo",))
    assert not _differ(_bits(up.albedo2), want["albedo"]).any()
    words = _np(up.hi_gbuf["hit"]).view(i32)
    floor = (words[..., 3] >= 0) & (words[..., 4] == 0)
    assert x["mirrored"] == int(floor.sum())  # (every floor pixel's ray is valid here)
    sky, refl, alb2 = _np(up.sky), _np(up.reflection), _np(up.albedo2)
    esc = sky[..., 3] == 1
    assert np.array_equal(refl[esc][:, 0:3], sky[esc][:, 0:3]) and (refl[..., 3] == (esc | (ref["hit2"][..., 3].view(i32) >= 0))).all()
    mean = _np(up.upsampled)[..., 0:3].astype(np.float64).mean((0, 1))
    assert np.allclose(refl[~esc][:, 0:3], alb2[~esc][:, 0:3] * mean, rtol=1e-4, atol=1e-7)  # (torch's float32 mean against a float64 one)
    a, b = _np(up.final), _np(plain.final)
    assert np.array_equal(a[~floor], b[~floor]) and not np.array_equal(a[floor], b[floor])
    assert np.allclose(a[floor][:, 0:3], 0.75 * b[floor][:, 0:3] + 0.25 * refl[floor][:, 0:3], rtol=1e-5, atol=1e-7)
    up.close()
    plain.close()


def test_upsampled_loop_runs_with_reflect(ptlib, tmp_path, capsys):
    ex = _example("upsampled_svgf_loop")
    ex.main(["--size", "128", "56", "--frames", "2", "--reflect", "--reflect-mesh", "0", "--reflectivity", "0.3", "--out-dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert out.count("reflection ") == 2 and "rays hit" in out and "pixels mirror" in out
    refl = np.load(tmp_path / "upsampled_svgf_reflection.npy")
    assert refl.shape == (56, 128, 4) and np.isfinite(refl).all() and refl[..., 3].max() == 1 and (refl[..., 0:3] >= 0).all()
    frame = np.load(tmp_path / "upsampled_svgf_frame.npy")
    assert frame.shape == (56, 128) and frame.any()
