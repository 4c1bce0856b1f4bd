"""Ambient occlusion from the G-buffer (pt_ao_layout, pt_ao_planes) on the GPU.  ao, out and bent are compared bit for bit over WHOLE
sentinel-filled planes, and every counter exactly, with an expectation the code under test never produces: tests/ao_ref.py builds the rays
in float32 NumPy from the same hit and position planes, the EXISTING traceDevice(any_hit=True) says which of them are occluded, and NumPy
reduces them.  The scratch is exactly pt_ao_layout's bytes between guard words (its content is not specified: slots are handed out by
atomics).  Frames are 64 x 40 and smaller, but for the four views of scene_kit.RECTS (131 x 61)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ao_ref as A
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
W, H = 64, 40
GUARD = 4  # sentinel words on either side of the scratch (16 bytes: the scratch stays 16-byte aligned)
SENTINEL = A.SENTINEL
CAM = scenes.TWO_BOX_CAMERA
BEHIND = dict(CAM, eye=(3.0, 2.5, 5.0))
PRM = dict(rays=4, radius=0.6, bias=1e-3)
PLANES = ("ao", "out", "bent")
WALL = [(-3.0, 0.0, 0.6), (3.0, 0.0, 0.6), (3.0, 3.0, 0.6), (-3.0, 3.0, 0.6)]


def _scene():
    """the unit box on its ground slab, and one free-standing quad 0.1 behind the box: a surface seen from both sides, with the box on one"""
    m = scenes.two_box_scene(False)
    m.meshes.append(scenes._quads_to_mesh([WALL], scenes.Material(color=(0.7, 0.7, 0.7))))
    return m


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


def _expect(r, hit, pos, pixels, rects=None, cams=None, max_rays_in_flight=0, **prm):
    """the reference: ao_ref's rays through the existing any-hit query of the same context, reduced in NumPy"""
    prm = dict(PRM, **prm)
    rays = prm["rays"]
    Rr = A.rays_of(hit, pos, cams if cams is not None else _cams(r), rects, pixels, rays, prm["radius"], prm["bias"], prm.get("seed", 0), prm.get("jitter", False))
    if len(Rr["rays"]):
        occ = _np(r.traceDevice(torch.from_numpy(Rr["rays"]).to("cuda:0"), any_hit=True))
        assert np.array_equal(occ == -2, ~Rr["valid"]), "the reference's validity rule is not pt_trace_device's"
    else:
        occ = np.zeros(0, np.int32)
    return A.reduce(occ == 1, Rr, rays, pixels, max_rays_in_flight), Rr


def _ao(r, hit, pos, pixels, what, rects=None, cams=None, mask=None, offset=False, planes=PLANES, ref=None, **prm):
    """aoPlanes into sentinel-filled planes and a guarded scratch of exactly pt_ao_layout's bytes, against the reference: the layout, every
    plane over the whole frame, the eight counters; hit and position are unchanged afterwards.  Returns the reference."""
    prm = dict(PRM, **prm)
    h, w = pixels.shape
    M = prm.get("max_rays_in_flight", 0)
    nbytes = r.aoLayout(prm["rays"], M)
    assert nbytes == A.layout(h, w, prm["rays"], M), f"{what}: the layout is {nbytes} bytes, the reference {A.layout(h, w, prm['rays'], M)}"
    if ref is None:
        ref, _ = _expect(r, hit, pos, pixels, rects, cams, **prm)
    hdev, pdev = _upload(hit, offset), _upload(pos, offset)
    outs = {n: filled((h, w) if n == "ao" else (h, w, 4), offset) for n in planes}
    sbuf, scratch = _scratch(nbytes)
    res = r.aoPlanes(hdev, pdev, scratch=scratch, mask=mask, **outs, **prm)
    st = res["stats"]
    print(f"{what}: {({k: st[k] for k in A.COUNTERS})}, {st['kernel_ms']:.4f} ms, trace {st['trace_ms']:.4f} ms")
    for n in PLANES:
        if n not in planes:
            assert res[n] is None
            continue
        assert res[n] is outs[n]
        got = _bits(outs[n])
        want = ref[n].reshape(got.shape)
        neq = _differ(got, want)
        assert not neq.any(), f"{what}: {n} differs in {int(neq.sum())} words, first at {np.argwhere(neq)[:3].tolist()}"
    words = _np(sbuf).view(u32)
    assert (words[:GUARD] == SENTINEL).all() and (words[-GUARD:] == SENTINEL).all(), f"{what}: a word outside the scratch was written"
    assert {k: st[k] for k in A.COUNTERS} == {k: ref[k] for k in A.COUNTERS}, (what, st, {k: ref[k] for k in A.COUNTERS})
    assert st["pixels"] == st["traced"] + st["skipped"] + st["nonfinite"] and st["trace_ms"] <= st["kernel_ms"]
    assert np.array_equal(_np(hdev).view(u32), np.ascontiguousarray(hit, f32).view(u32)), f"{what}: hit was written"
    assert np.array_equal(_np(pdev).view(u32), np.ascontiguousarray(pos, f32).view(u32)), f"{what}: position was written"
    return ref


def _make(size, cam=CAM, partition=None, model=None):
    r = _renderer(model or _scene(), size, cam, partition=partition)
    r._test_camera = R.make_camera(cam, size[0] / size[1])
    return r


_CASES = {}


def _frame():
    """a W x H renderer on the scene and its G-buffer's two planes, shared by the tests that only read them"""
    if "frame" not in _CASES:
        r = _make((W, H))
        hit, pos = _gbuffer(r)
        for a in (hit, pos):
            a.setflags(write=False)
        _CASES["frame"] = (r, hit, pos)
    return _CASES["frame"]


def _as(ref, name):
    return ref[name].view(f32)


# ------------------------------------------------------------------ 1. rays, jitter, outputs
@pytest.mark.parametrize("jitter", [dict(), dict(jitter=True, seed=1), dict(jitter=True, seed=0xFFFFFFFF)], ids=["fixed", "seed1", "seedmax"])
@pytest.mark.parametrize("rays", [1, 4, 5, 32])
def test_rays_and_jitter(ptlib, rays, jitter):
    r, hit, pos = _frame()
    ref = _ao(r, hit, pos, _all(), f"{rays} rays, {jitter}", rays=rays, **jitter)
    assert ref["traced"] > 0 and ref["skipped"] > 0 and 0 < ref["occluded"] < ref["rays"] and ref["invalid"] == 0
    ao = _as(ref, "ao")
    assert ao.min() < 1 and ((ao * f32(rays)) == np.round(ao * f32(rays))).all()
    if jitter and rays > 1:
        other, _ = _expect(r, hit, pos, _all(), rays=rays, **dict(jitter, seed=2))
        assert _differ(other["bent"], ref["bent"]).any()


@pytest.mark.parametrize("planes", [("ao",), ("out",), ("bent",), ("ao", "bent")], ids="+".join)
def test_each_output_alone(ptlib, planes):
    r, hit, pos = _frame()
    _ao(r, hit, pos, _all(), f"only {planes}", planes=planes, rays=5, jitter=True, seed=7)


def test_the_facade_allocates_out_and_scratch(ptlib):
    r, hit, pos = _frame()
    ref, _ = _expect(r, hit, pos, _all())
    res = r.aoPlanes(_upload(hit), _upload(pos), **PRM)
    assert res["ao"] is None and res["bent"] is None and not _differ(_bits(res["out"]), ref["out"]).any()
    assert res["scratch"].numel() * 4 == A.layout(H, W, 4)


# ------------------------------------------------------------------ 2. batches
def test_one_pixel_per_batch(ptlib):
    w, h = 16, 8
    r = _make((w, h))
    hit, pos = _gbuffer(r)
    ref = _ao(r, hit, pos, _all(h, w), "16 x 8, max_rays_in_flight = rays", rays=5, max_rays_in_flight=5, jitter=True, seed=3)
    assert ref["batches"] == w * h
    whole = _ao(r, hit, pos, _all(h, w), "16 x 8, the default", rays=5, jitter=True, seed=3)
    assert whole["batches"] == 1 and all(np.array_equal(whole[n], ref[n]) for n in PLANES)
    r.close()


@pytest.mark.parametrize("M", [100, 4 * 64 * 3 + 4, 4 * 256, 4 * 257, 4 * 1024, 4 * 1025, 4 * 2559, 4 * 2560, 1 << 30])
def test_the_result_does_not_depend_on_the_batch(ptlib, M):
    """a boundary inside a wave (100 rays: 25 pixels), inside a workgroup of k_ao_rays (1024 pixels), on one and one pixel behind it, one
    pixel short of the frame, the frame, more than it; every batch is smaller than the traversal grid: the wide start"""
    r, hit, pos = _frame()
    if "default" not in _CASES:
        _CASES["default"] = _expect(r, hit, pos, _all(), jitter=True, seed=5)[0]
    base = _CASES["default"]
    ref = dict(base, batches=A.batches_of(W * H, H, W, 4, M))
    _ao(r, hit, pos, _all(), f"max_rays_in_flight {M}", ref=ref, jitter=True, seed=5, max_rays_in_flight=M)
    assert ref["batches"] == -(-W * H // min(M // 4, W * H))


def test_the_layout_grows_with_the_batch_and_stops_at_the_frame(ptlib):
    r, _, _ = _frame()
    sizes = [r.aoLayout(4, M) for M in (4, 8, 400, 4 * W * H - 4, 4 * W * H, 4 * W * H + 4, 1 << 31, 0)]
    assert sizes[:5] == sorted(set(sizes[:5])) and sizes[4] == sizes[5] == sizes[6] == sizes[7] == 256 + W * H * 168
    assert sizes[0] == 256 + 168 + 8 and r.aoLayout(32, 32) == (256 + 40 * 32 + 8 + 15) // 16 * 16 == A.layout(H, W, 32, 32) and r.aoLayout(5, 7) == (256 + 208 + 15) // 16 * 16


# ------------------------------------------------------------------ 3. sizes, alignment, masks
@pytest.mark.parametrize("size", [(1, 1), (13, 7), (33, 9), (63, 5)])
def test_sizes(ptlib, size):
    w, h = size
    r = _make(size)
    hit, pos = _gbuffer(r)
    _ao(r, hit, pos, _all(h, w), f"{w} x {h}", jitter=True, seed=w)
    _ao(r, hit, pos, _all(h, w), f"{w} x {h}, 7 rays in flight", rays=3, max_rays_in_flight=7)
    r.close()


def test_every_plane_one_float_into_its_allocation(ptlib):
    r, hit, pos = _frame()
    _ao(r, hit, pos, _all(), "every plane 4 bytes off a 16-byte boundary", offset=True, rays=5)


def test_block_masks(ptlib):
    r, hit, pos = _frame()
    nby, nbx = r.blockGrid()
    rng = np.random.default_rng(4)
    for name, m in (("random", rng.random((nby, nbx)) < 0.4), ("one block", np.arange(nby * nbx).reshape(nby, nbx) == 17), ("empty", np.zeros((nby, nbx), bool))):
        ref = _ao(r, hit, pos, pixel_mask(m, h=H, w=W), f"mask: {name}", mask=m, max_rays_in_flight=4 * 100)
        assert ref["pixels"] == int(m.sum()) * 64
        if name == "empty":
            assert ref["batches"] == 0 and (ref["out"] == SENTINEL).all()


# ------------------------------------------------------------------ 4. views and partitions
def test_two_sides_of_a_wall_in_four_views(ptlib):
    """RECTS with two cameras in front of the free-standing quad and two behind it: pixels in no view are untouched, and the normal is
    turned to each view's own eye — with the cameras of the other side the reference gives another plane"""
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
    ref = _ao(r, hit, pos, inside, "four views", rects=RECTS, cams=cams, rays=5, jitter=True, seed=2)
    assert ref["pixels"] == int(inside.sum()) and (ref["ao"][~inside] == SENTINEL).all() and ref["occluded"] > 0
    wrong, _ = _expect(r, hit, pos, inside, rects=RECTS, cams=cams[[1, 0, 3, 2]], rays=5, jitter=True, seed=2)
    assert _differ(wrong["ao"], ref["ao"]).any(), "the scene cannot tell one view's eye from another's"
    m = np.random.default_rng(8).random(r.blockGrid()) < 0.5
    _ao(r, hit, pos, inside & pixel_mask(m, h=h, w=w), "four views under a mask", rects=RECTS, cams=cams, mask=m, max_rays_in_flight=4 * 333)
    r.close()


def test_partitions_add_up(ptlib):
    r, hit, pos = _frame()
    whole, _ = _expect(r, hit, pos, _all(), rays=5)
    by, bx = np.mgrid[0:H, 0:W] // 8
    union = {n: np.full(whole[n].shape, SENTINEL, u32) for n in PLANES}
    model = _scene()
    for rank in range(2):
        rr = _make((W, H), partition=(rank, 2, 8, 8), model=model)
        own = (bx + by) % 2 == rank
        part = _ao(rr, hit, pos, own, f"rank {rank} of 2", rays=5)
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
    hit, pos = hit.copy(), pos.copy()
    hits = np.argwhere(hit[..., 3].view(np.int32) >= 0)
    assert len(hits) > 64 and (hit[..., 3].view(np.int32) < 0).any()
    pick = hits[np.random.default_rng(6).permutation(len(hits))[:14]]
    nan, inf = f32(np.nan), f32(np.inf)
    edits = [("hit", 5, nan), ("hit", 6, inf), ("hit", 7, -inf), ("hit", 0, nan), ("hit", 0, inf), ("hit", 0, f32(0.0)), ("hit", 0, f32(-0.0)), ("hit", 0, f32(-2.0)),
             ("pos", 0, nan), ("pos", 1, -inf), ("pos", 2, inf)]
    for (y, x), (plane, word, value) in zip(pick, edits):
        (hit if plane == "hit" else pos)[y, x, word] = value
    for (y, x), prim in zip(pick[11:], (0x7FFFFFFF, 12345678, 36)):  # stale primitives: no address is formed from them
        hit[y, x, 3] = np.array([prim], np.int32).view(f32)[0]
    clean, _ = _expect(r, _frame()[1], _frame()[2], _all())
    ref = _ao(r, hit, pos, _all(), "hostile records")
    assert ref["nonfinite"] == 11 and ref["skipped"] == clean["skipped"] > 0 and ref["traced"] == clean["traced"] - 11
    one = f32(1).view(u32)
    for y, x in pick[:11]:
        assert ref["ao"][y, x] == one and tuple(ref["bent"][y, x]) == (0, 0, 0, one)
    for y, x in pick[11:]:
        assert np.array_equal(ref["bent"][y, x], clean["bent"][y, x])
    miss = hit[..., 3].view(np.int32) < 0
    assert (ref["ao"][miss] == one).all() and (ref["out"][miss] == one).all()


@pytest.mark.parametrize("prm", [dict(bias=0.0), dict(bias=0.05), dict(radius=1e-6), dict(radius=1e30), dict(radius=3.0, rays=8)],
                         ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()))
def test_bias_and_radius(ptlib, prm):
    r, hit, pos = _frame()
    ref = _ao(r, hit, pos, _all(), f"{prm}", **prm)
    if prm.get("radius") == 1e-6:
        assert ref["occluded"] == 0 and (_as(ref, "ao")[ref["ao"] != SENTINEL] == 1).all()
    if prm.get("radius") == 1e30:
        assert ref["occluded"] > _expect(r, hit, pos, _all())[0]["occluded"]


def test_the_pass_follows_the_current_tree(ptlib):
    """the same G-buffer before and after transformMeshes has moved the box away: both match the query over the geometry of the moment"""
    r = _make((W, H))
    hit, pos = _gbuffer(r)
    before = _ao(r, hit, pos, _all(), "the box in place")
    r.transformMeshes({0: np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -10.0]], f32)})
    after = _ao(r, hit, pos, _all(), "the box moved away")
    assert after["occluded"] < before["occluded"] and _differ(after["ao"], before["ao"]).any()
    r.close()


@pytest.mark.parametrize("rays", [1, 8, 32])
def test_two_analytic_scenes_are_exact(ptlib, rays):
    """tests/test_ao_cabi.py's two scenes on the GPU's tree: the open floor gives ao == 1.0, the lid ao == 0.0, exactly"""
    hit, pos, cam = A.analytic_planes()
    h, w = hit.shape[:2]
    for ceiling, want in ((False, 1.0), (True, 0.0)):
        quads = A.analytic_quads(ceiling)
        model = scenes.Model([scenes._quads_to_mesh([q], scenes.Material()) for q in quads])
        r = R.SampleRenderer(model)
        r.resize((w, h))
        r.setCamera(R.Camera(A.ANALYTIC_EYE, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 35.0, w / h))
        assert np.array_equal(R._camera_rows([R.Camera(A.ANALYTIC_EYE, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 35.0, w / h)])[0, 0:3], cam[0, 0:3])
        ref = _ao(r, hit, pos, _all(h, w), f"analytic, lid {ceiling}, {rays} rays", cams=cam, rays=rays, radius=A.RADIUS, jitter=True, seed=3)
        assert (_as(ref, "ao") == f32(want)).all() and ref["occluded"] == (h * w * rays if ceiling else 0)
        r.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals(ptlib):
    L = _lib.load_library()
    r = R.SampleRenderer(_scene())
    _, hit, pos = _frame()
    hdev, pdev = _upload(hit), _upload(pos)
    outs = {n: filled((H, W) if n == "ao" else (H, W, 4)) for n in PLANES}
    nbytes = A.layout(H, W, 4)
    sbuf, scratch = _scratch(nbytes)
    good = dict(hit=hdev.data_ptr(), position=pdev.data_ptr(), ao=outs["ao"].data_ptr(), out=outs["out"].data_ptr(), bent=outs["bent"].data_ptr(),
                scratch=scratch.data_ptr(), rays=4, max_rays_in_flight=0, radius=0.6, bias=1e-3, seed=0, flags=0)

    def untouched(what):
        assert (_np(sbuf).view(u32) == SENTINEL).all(), f"{what}: the scratch was written"
        for n in PLANES:
            assert (_bits(outs[n]) == SENTINEL).all(), f"{what}: {n} was written"

    def refused(what, pattern, **fields):
        d = _lib.AoDesc()
        for n, v in dict(good, **fields).items():
            setattr(d, n, v)
        torch.cuda.synchronize()
        s = _lib.AoStats(7, 7, 7, 7, 7, 7, 7, 7, 7.0, 7.0)
        rc = L.pt_ao_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_ao_planes") and pattern in msg, f"{what}: {msg!r}"
        assert tuple(getattr(s, n) for n, _ in s._fields_) == (7, 7, 7, 7, 7, 7, 7, 7, 7.0, 7.0)
        untouched(what)

    def layout_refused(what, pattern, rays=4, M=0, with_bytes=True):
        nb = C.c_size_t(77)
        rc = L.pt_ao_layout(r._ctx, rays, M, C.byref(nb) if with_bytes else None)
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1 and msg.startswith("pt_ao_layout") and pattern in msg, f"{what}: {rc}, {msg!r}"
        assert nb.value == 77, f"{what}: bytes was written"

    refused("no resize yet", "pt_resize")
    layout_refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(CAM, W / H))
    layout_refused("bytes null", "bytes is null", with_bytes=False)
    assert L.pt_ao_planes(r._ctx, None, None) == -1 and "pt_ao_planes: null description" in L.pt_last_error(r._ctx).decode()
    refused("an unknown flag", "unknown flag bits 2", flags=3)
    refused("an unknown flag", "unknown flag bits 2147483648", flags=0x80000000)
    for bad in (0, 33, 0xFFFFFFFF):
        refused(f"rays {bad}", f"rays must be 1..32, not {bad}", rays=bad)
        layout_refused(f"rays {bad}", f"rays must be 1..32, not {bad}", rays=bad)
    refused("fewer rays in flight than rays", "max_rays_in_flight is 3, below rays (4)", max_rays_in_flight=3)
    layout_refused("fewer rays in flight than rays", "max_rays_in_flight is 3, below rays (4)", M=3)
    for bad in (0.0, -0.0, -1.0, float("nan"), float("inf")):
        refused(f"radius {bad}", "radius must be finite and > 0", radius=bad)
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf")):
        refused(f"bias {bad}", "bias must be finite and >= 0", bias=bad)
    for name in ("hit", "position", "scratch"):
        refused(f"{name} null", f"{name} is null", **{name: None})
    refused("no output", "no output asked for", ao=None, out=None, bent=None)
    host = np.zeros((H, W, 8), f32)
    refused("a host pointer", "hit is not device memory", hit=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "bent is not 4-byte aligned", bent=good["bent"] + 2)
    for off in (4, 8, 2):
        refused(f"the scratch {off} bytes off", "scratch is not 16-byte aligned", scratch=good["scratch"] + off)
    big = torch.zeros(2 * H * W * 8 + 8, dtype=torch.float32, device="cuda:0")
    refused("out inside hit", "hit and out overlap", hit=big.data_ptr(), out=big.data_ptr() + 16)
    refused("ao inside position", "position and ao overlap", position=big.data_ptr() + 64, ao=big.data_ptr())
    refused("out exactly bent", "out and bent overlap", out=good["bent"])
    refused("ao inside out", "ao and out overlap", ao=good["out"] + 32)
    refused("the scratch inside hit", "hit and scratch overlap", scratch=good["hit"] + 16)
    refused("the scratch inside bent", "bent and scratch overlap", scratch=good["bent"] + 32)
    hip = _hip_runtime()
    for name, nb in (("scratch", nbytes), ("bent", H * W * 16)):
        raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert hip.hipMalloc(C.byref(raw), C.c_size_t(nb)) == 0
        try:
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= nb
            refused(f"{name} one element too small", f"{name} has fewer than {nb} bytes left", **{name: raw.value + size.value - (nb - 16)})
        finally:
            assert hip.hipFree(raw) == 0
    # the Python facade passes the library's refusals on; a valid call afterwards works, into the same arrays
    with pytest.raises(RuntimeError, match="out and bent overlap"):
        r.aoPlanes(hdev, pdev, out=outs["out"], bent=outs["out"], **PRM)
    with pytest.raises(ValueError, match=r"scratch: a contiguous torch.float32 tensor of shape \(%d,\) is expected" % (nbytes // 4)):
        r.aoPlanes(hdev, pdev, scratch=torch.zeros((nbytes // 4 + 4,), device="cuda:0"), **PRM)
    untouched("the facade's refusals")
    r._test_camera = R.make_camera(CAM, W / H)
    ref, _ = _expect(r, hit, pos, _all())
    res = r.aoPlanes(hdev, pdev, scratch=scratch, **outs, **PRM)
    for n in PLANES:
        assert not _differ(_bits(outs[n]), ref[n].reshape(_bits(outs[n]).shape)).any(), n
    assert {k: res["stats"][k] for k in A.COUNTERS} == {k: ref[k] for k in A.COUNTERS}
    r.close()


# ------------------------------------------------------------------ 7. state and ordering
def test_queued_queries_and_rendering_state(ptlib):
    """asynchronous queries queued in front of the call are completed by it, and queryWait still delivers their counts; stats() and the
    frame buffers are what they were"""
    r = _make((W, H))
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.launchParams.samples_per_launch = 1
    r.render()
    hit, pos = _gbuffer(r)
    ref, Rr = _expect(r, hit, pos, _all())
    r.queryWait()
    rays = torch.from_numpy(Rr["rays"]).to("cuda:0")
    queued = [r.traceDevice(rays, any_hit=True, wait=False) for _ in range(2)]
    before, frame = r.stats(), r.download(R.PT_BUF_ACCUM)
    res = r.aoPlanes(_upload(hit), _upload(pos), ao=filled((H, W)), **PRM)
    assert r.stats() == before and r.download(R.PT_BUF_ACCUM).tobytes() == frame.tobytes()
    assert not _differ(_bits(res["ao"])[..., 0], ref["ao"]).any()
    q = r.queryWait()
    assert q["rays"] == 2 * len(Rr["rays"]) and q["hits"] == 2 * ref["occluded"] and q["invalid_rays"] == 0
    for t in queued:
        assert np.array_equal(_np(t) == 1, _np(queued[0]) == 1) and int((_np(t) == 1).sum()) == ref["occluded"]
    assert r.queryWait()["rays"] == 0
    r.close()


@pytest.mark.parametrize("mode", ["default", "side"])
def test_under_a_busy_torch_stream(ptlib, mode):
    """tests/test_gpu_stream_contract.py's protocol: the planes are produced, and the outputs sentinel-filled, by work still pending on
    torch's current stream when the call is made; the result equals the synchronous call's, and that equals the reference"""
    from stream_kit import _pin, _res

    r, hit, pos = _frame()
    outs = {n: filled((H, W) if n == "ao" else (H, W, 4)) for n in PLANES}
    scratch = torch.zeros((r.aoLayout(4) // 4,), dtype=torch.float32, device="cuda:0")  # (not an output of the case: its slots are handed out by atomics)

    def occlusion(dev, outs, returned):
        res = r.aoPlanes(dev["hit"], dev["position"], scratch=scratch, **outs, **PRM)
        returned()
        return _res(res, outs)

    sync, got = _pin("aoPlanes", mode, r, dict(hit=hit, position=pos), outs, occlusion)
    ref, _ = _expect(r, hit, pos, _all())
    for n in PLANES:
        assert not _differ(got[n].view(u32).reshape(ref[n].shape), ref[n]).any(), f"{n} under a busy stream [{mode}]"
    assert got["stats"] == {k: ref[k] for k in A.COUNTERS}


# ------------------------------------------------------------------ 8. the upsampled loop with --ao
def _example(name):
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def test_upsampled_loop_with_ao_shades_the_irradiance(ptlib):
    """examples/upsampled_svgf_loop.py's UpsampledLoop with ao at 128 x 56, scale 2: the raw occlusion is aoPlanes of the full-size
    G-buffer, jittered by the frame index; what reaches the albedo's product is the upsampled irradiance times the filtered occlusion"""
    import surface_ref as S

    ex = _example("upsampled_svgf_loop")
    w, h = 128, 56
    probe = scenes.sky_probe(256, 128).BuildCDF()
    cam0 = dict(eye=(2.0, 0.35, -3.0), lookat=(0.0, 0.2, 0.5), up=(0.0, 1.0, 0.0), fovY=35.0)
    up = ex.UpsampledLoop(S.textured_scene(), (w, h), 2, probe=probe, ao=True, ao_rays=5, ao_radius=0.4)
    cam = R.make_camera(cam0, w / h)
    for k in range(3):
        prev, cam = cam, R.make_camera(ex.orbit(cam0, 0.02 * k), w / h)
        x = up.frame(k, prev, cam)
        assert x["pixels"] == w * h and x["ao_ms"] > 0 and x["ao_trace_ms"] > 0 and x["ao_batches"] == 1 and 0 < x["ao_occluded"] < x["ao_rays"]
    ref, _ = _expect(up.hi, _np(up.hi_gbuf["hit"]), _np(up.hi_gbuf["position"]), _all(h, w), cams=R._camera_rows([cam]), rays=5, radius=0.4, jitter=True, seed=2)
    assert not _differ(_bits(up.ao_raw), ref["out"]).any() and x["ao_occluded"] == ref["occluded"]
    f = _np(up.ao_filtered)
    assert (f[..., 0:3] >= f32(2.0 ** -10)).all() and (f[..., 0:3] <= 1 + 1e-5).all() and f[..., 0].min() < 1
    want = _np(up.upsampled)[..., 0:3] * f[..., 0:3]
    assert np.array_equal(_np(up.shaded)[..., 0:3].view(u32), want.view(u32))
    up.close()


def test_upsampled_loop_runs_with_ao(ptlib, tmp_path, capsys):
    ex = _example("upsampled_svgf_loop")
    ex.main(["--size", "128", "56", "--frames", "2", "--ao", "--ao-rays", "2", "--ao-radius", "0.3", "--out-dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert out.count("occlusion ") == 2 and "rays occluded" in out
    ao = np.load(tmp_path / "upsampled_svgf_ao.npy")
    assert ao.shape == (56, 128, 4) and np.isfinite(ao).all() and ao[..., 0:3].max() <= 1 + 1e-5 and ao[..., 0:3].min() > 0
