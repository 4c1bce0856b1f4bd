"""Temporal accumulation (pt_temporal_accumulate) on the GPU.  Every output plane is compared bit for bit, over the WHOLE plane (so a pixel
written outside the chosen set shows as a lost sentinel), with tests/temporal_ref.py: float32 NumPy evaluating the header's arithmetic, with
the CPU checker's make_color.  The one tolerance of this file is the sanity bound of the recipe test, which says where it comes from.

Real-plane inputs (planes from renderGBuffer, pinned by tests/test_gpu_gbuffer.py; previous camera: temporal_ref.forward; history: random
lengths 0..9 with zeros, a few NaN and inf words).  Valid / invalid pixels and, among the invalid, the pixels showing each rejection reason,
as tests/test_temporal_cabi.py counts them on CPU-built planes (the test asserts the same coverage on the GPU's planes and prints its counts):
  two_box 131 x 61, dolly 0.65, plane_eps 0:  1240 / 6751  rect 3895 nolookup 102 length 1478 history 160 miss 1835 mesh 213 normal 11 plane 722 min_weight 264
  terrain 131 x 61, dolly 0.5:                2113 / 5878  rect 3385 nolookup 717 length 1031 history 152 miss 1458 mesh 122 normal 186 plane 39 min_weight 299
  two_box, previous camera behind the scene (gbuffer_ref._behind): every hit pixel's motion is NaN, 0 valid"""
import ctypes as C

import numpy as np
import pytest
import torch

import temporal_ref as T
from gbuffer_ref import _behind, _row
from gpu_kit import filled, pixel_mask, plane_shape, whole_frame
from gpu_kit import bits as _bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from scene_kit import RECTS, _views_and_prev

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 131, 61
SENTINEL = T.SENTINEL
INPUTS = ("color", "motion", "hit", "position", "prev_hit", "prev_position", "history_in", "length_in")
WORDS = _lib.TEMPORAL_PLANES


# ------------------------------------------------------------------ GPU helpers
def _filled(name, h, w, offset=False):
    """a sentinel-filled plane of the pass; offset: one float into its allocation (4-byte aligned only)"""
    return filled(plane_shape(h, w, WORDS[name]), offset, torch.int32 if name == "frame_rgba8" else torch.float32)


def _same(got, ref, what):
    for name, a in got.items():
        b = ref[name]
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {name} differs from float32 NumPy in {int((a != b).sum())} words"


def _run(r, orc, planes, rects, pixels, what, mask=None, offset=False, outputs=T.OUTPUTS, **prm):
    """uploads the planes, calls temporalAccumulate into sentinel-filled outputs, compares every output and the colour plane with the NumPy
    reference over the whole frame; returns (reference, stats)"""
    h, w = planes["length_in"].shape
    dev = {k: _upload(planes[k], offset) for k in INPUTS}
    for k in ("prev_hit", "prev_position"):  # read-only planes may alias one another
        if planes[k] is planes[k[5:]]:
            dev[k] = dev[k[5:]]
    out = {k: _filled(k, h, w, offset) for k in outputs}
    kw = {k: v for k, v in prm.items() if k != "clear"}
    res = r.temporalAccumulate(**dev, **out, mask=mask, clear_color=bool(prm.get("clear")), **kw)
    assert all(res[k] is out[k] for k in outputs)
    ref = T.temporal_ref(orc, planes, rects, pixels, **prm)
    got = {k: _bits(out[k]) for k in outputs}
    got["color"] = _bits(dev["color"])
    _same(got, ref, what)
    st = res["stats"]
    assert st["pixels"] == int(np.asarray(pixels).sum()) and st["reprojected"] == ref["reprojected"], (what, st, ref["reprojected"])
    assert st["kernel_ms"] > 0 if st["pixels"] else st["kernel_ms"] >= 0
    return ref, st


_CASES = {}


def _case(name):
    """The input's renderer and its G-buffer planes of the current and of the previous camera, with a random history.  Built once; the
    arrays are read-only."""
    if name not in _CASES:
        make, size, cam, prev, prm, seed = T.real_inputs()[name]
        w, h = size
        r = _renderer(make(), size, cam)
        cur = r.renderGBuffer(("hit", "position", "motion"), prev_cameras=_row(prev, w / h))
        behind = r.renderGBuffer(("motion",), prev_cameras=_row(_behind(cam), w / h))
        r.setCamera(R.make_camera(prev, w / h))
        old = r.renderGBuffer(("hit", "position"))
        r.setCamera(R.make_camera(cam, w / h))
        planes = T.with_random_history(dict(motion=_np(cur["motion"]), hit=_np(cur["hit"]), position=_np(cur["position"]), prev_hit=_np(old["hit"]),
                                            prev_position=_np(old["position"])), seed)
        planes["motion_behind"] = _np(behind["motion"])
        for a in planes.values():
            a.setflags(write=False)
        _CASES[name] = (r, planes, prm)
    return _CASES[name]


def _frame(w=W, h=H):
    return whole_frame(w, h)


# ------------------------------------------------------------------ 1. real planes
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_real_planes(ptlib, orc_det, name):
    r, planes, prm = _case(name)
    rects, px = _frame()
    ref, st = _run(r, orc_det, planes, rects, px, name, **prm)
    valid, invalid, counts = T.check_coverage(ref, px, name)
    print(f"{name}: valid {valid} invalid {invalid} {counts} kernel_ms {st['kernel_ms']:.4f}")
    # the other parameters' paths: the clear flag, a colour scale, a short history cap, no optional output
    _run(r, orc_det, planes, rects, px, f"{name}, clear + scale + cap", clear=True, color_scale=3.0, max_history=4, min_weight=0.0, **prm)
    _run(r, orc_det, planes, rects, px, f"{name}, required outputs only", outputs=("history_out", "length_out"), min_weight=1.0, normal_cos=-1.0, **prm)


def test_previous_camera_behind_the_scene(ptlib, orc_det):
    r, planes, prm = _case("two_box")
    rects, px = _frame()
    p = dict(planes, motion=planes["motion_behind"])
    hit = planes["hit"].view(np.int32)[..., 3] >= 0
    assert np.isnan(p["motion"][hit]).all()
    ref, _ = _run(r, orc_det, p, rects, px, "behind", **prm)
    assert not ref["valid"][hit].any() and (ref["reason"][hit] == T.BIT["nolookup"]).all()
    assert (ref["length_out"].view(f32)[hit] == 1).all()


# ------------------------------------------------------------------ 2. synthetic planes on small frames
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (9, 8), (63, 1), (65, 3)])
def test_synthetic_planes_on_small_frames(ptlib, orc_det, size):
    w, h = size
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), size, scenes.TWO_BOX_CAMERA)
    planes = T.synthetic_planes(w, h, 7 + w)
    rects, px = _frame(w, h)
    xs = np.arange(w, dtype=f32)[None, :] + planes["motion"][..., 0]
    ysv = np.arange(h, dtype=f32)[:, None] + planes["motion"][..., 1]
    if w * h >= 12:  # the crafted values are there: both ends of the range, an exact integer, the first value past either end
        assert (xs == -1).any() and (xs == w).any() and (xs == np.floor(xs)).any() and (xs < -1).any() and (xs > w).any()
        assert (ysv == -1).any() and (ysv == h).any() and (ysv < -1).any() and (ysv > h).any()
    ref, _ = _run(r, orc_det, planes, rects, px, f"{w} x {h}", min_weight=0.6)
    if w * h >= 64:
        counts = T.reason_counts(ref, px)
        assert counts["rect"] and counts["nolookup"] and counts["min_weight"] and ref["reprojected"] > 0, counts
    _run(r, orc_det, planes, rects, px, f"{w} x {h}, any weight", min_weight=0.0, clear=True)
    r.close()


# ------------------------------------------------------------------ 3. views
def test_views(ptlib, orc_det):
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), (W, H), scenes.TWO_BOX_CAMERA)
    views, prev = _views_and_prev()
    r.setViews(views)
    cur = r.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev)
    r.setViewCameras(prev)
    old = r.renderGBuffer(("hit", "position"))
    r.setViewCameras([v[4] for v in views])
    rng = np.random.default_rng(21)
    motion = _np(cur["motion"]).copy()
    inside = np.zeros((H, W), bool)
    for x, y, w, h in RECTS:
        inside[y:y + h, x:x + w] = True
        # across the view's right and lower border: half a pixel (one tap column / row outside the view, inside the frame) and three pixels
        motion[y:y + h, x + w - 1, 0] = 0.5
        motion[y + h - 1, x:x + w, 1] = 0.5
        motion[y, x + w - 1] = (3.0, 0.0)
        motion[y, x] = (-0.5, -0.5)  # across the left and upper border (views 1 and 3 have frame pixels there)
    # history everywhere, also between the views: a tap taken across a border would change the answer
    hist = rng.random((H, W, 4), dtype=f32)
    ln = rng.integers(1, 9, (H, W)).astype(f32)
    planes = dict(color=rng.random((H, W, 4), dtype=f32), motion=motion, hit=_np(cur["hit"]), position=_np(cur["position"]), prev_hit=_np(old["hit"]),
                  prev_position=_np(old["position"]), history_in=hist, length_in=ln)
    ref, st = _run(r, orc_det, planes, RECTS, inside, "four views", clear=True)
    assert st["pixels"] == sum(w * h for _, _, w, h in RECTS) and 0 < ref["reprojected"] < st["pixels"]
    for x, y, w, h in RECTS:
        assert ref["reason"][y + 1, x + w - 1] & T.BIT["rect"] or ref["valid"][y + 1, x + w - 1]
        assert not ref["valid"][y, x + w - 1]  # three pixels past the border: no lookup
    for name in T.OUTPUTS:  # (the whole-plane comparison already said so)
        assert (ref[name][~inside] == SENTINEL).all()
    # back to the single camera: the whole frame, one rectangle
    r.setViews([])
    rects, px = _frame()
    _run(r, orc_det, planes, rects, px, "views dropped")
    r.close()


# ------------------------------------------------------------------ 4. masks and partition
def test_masks(ptlib, orc_det):
    r, planes, prm = _case("two_box")
    nby, nbx = r.blockGrid()
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.4
    mask[0, 0] = mask[nby - 1, nbx - 1] = mask[0, nbx - 1] = mask[nby - 1, 3] = True  # corner and edge blocks, the 3-wide column and the 5-high row
    mask[1, 1] = False
    px = pixel_mask(mask, h=H, w=W)
    ref, st = _run(r, orc_det, planes, [(0, 0, W, H)], px, "a random block mask", mask=mask, clear=True, **prm)
    assert 0 < st["pixels"] < W * H and (ref["history_out"][~px] == SENTINEL).all() and not (ref["length_out"][px] == SENTINEL).any()
    _, st = _run(r, orc_det, planes, [(0, 0, W, H)], np.zeros((H, W), bool), "the empty mask", mask=np.zeros((nby, nbx), bool), clear=True, **prm)
    assert st == dict(pixels=0, reprojected=0, kernel_ms=st["kernel_ms"])


def test_partition(ptlib, orc_det):
    _, planes, prm = _case("two_box")
    make, size, cam, _, _, _ = T.real_inputs()["two_box"]
    by, bx = np.mgrid[0:H, 0:W] // 8
    written = np.zeros((H, W), int)
    for rank in range(3):
        r = _renderer(make(), size, cam, partition=(rank, 3, 8, 8))
        own = (bx + by) % 3 == rank
        p = dict(planes, length_in=np.where(own, planes["length_in"], f32(0)))  # the rank never wrote the others' pixels
        ref, st = _run(r, orc_det, p, [(0, 0, W, H)], own, f"rank {rank}", **prm)
        assert st["pixels"] == int(own.sum()) and ref["reprojected"] > 0
        written += ref["length_out"] != SENTINEL
        r.close()
    assert (written == 1).all()  # the union is the frame, overlaps are empty


# ------------------------------------------------------------------ 5. alignment and the context's own buffers
def test_planes_four_byte_aligned_only(ptlib, orc_det):
    r, planes, prm = _case("terrain")
    rects, px = _frame()
    _run(r, orc_det, planes, rects, px, "planes one float into their allocations", offset=True, clear=True, **prm)


def test_context_buffers_as_planes(ptlib, orc_det):
    _, planes, prm = _case("two_box")
    make, size, cam, _, _, _ = T.real_inputs()["two_box"]
    r = _renderer(make(), size, cam)
    nby, nbx = r.blockGrid()
    mask = np.random.default_rng(9).random((nby, nbx)) < 0.5
    px = pixel_mask(mask, h=H, w=W)
    r.uploadAccum(planes["color"])
    before = {k: r.download(k).view(np.uint32) for k in (R.PT_BUF_ACCUM, R.PT_BUF_FRAME, R.PT_BUF_COLOR, R.PT_BUF_NORMAL, R.PT_BUF_ALBEDO)}
    assert np.array_equal(before[R.PT_BUF_ACCUM], planes["color"].view(np.uint32))
    dev = {k: _upload(planes[k]) for k in INPUTS if k != "color"}
    out = {k: _filled(k, H, W) for k in ("history_out", "length_out")}
    res = r.temporalAccumulate(color=r.deviceBuffer(R.PT_BUF_ACCUM), **dev, **out, frame_rgba8=r.deviceBuffer(R.PT_BUF_FRAME),
                               copy_out=r.deviceBuffer(R.PT_BUF_COLOR), mask=mask, clear_color=True, **prm)
    ref = T.temporal_ref(orc_det, planes, [(0, 0, W, H)], px, clear=True, **prm)
    assert res["frame_rgba8"] is None and res["copy_out"] is None and res["stats"]["reprojected"] == ref["reprojected"]
    _same({k: _bits(out[k]) for k in out}, ref, "context buffers")
    after = {k: r.download(k).view(np.uint32) for k in before}
    accum = after[R.PT_BUF_ACCUM]
    assert not accum[px].any() and np.array_equal(accum[~px], before[R.PT_BUF_ACCUM][~px])  # zero exactly at the processed pixels
    assert np.array_equal(after[R.PT_BUF_COLOR][px], ref["copy_out"][px]) and np.array_equal(after[R.PT_BUF_COLOR][~px], before[R.PT_BUF_COLOR][~px])
    assert np.array_equal(after[R.PT_BUF_FRAME][px], ref["frame_rgba8"][px]) and np.array_equal(after[R.PT_BUF_FRAME][~px], before[R.PT_BUF_FRAME][~px])
    for k in (R.PT_BUF_NORMAL, R.PT_BUF_ALBEDO):
        assert np.array_equal(after[k], before[k])
    r.close()


# ------------------------------------------------------------------ 6. the per-frame colour recipe, end to end
def test_recipe_end_to_end(ptlib, orc_det):
    """Cornell 67 x 45, static camera, frames k = 0..3 rendered at subframe k.  The sanity bound against the plain progressive average: each
    frame the recipe's colour differs from the resolve's by two roundings ((c / (k+1)) * (k+1)) and the blend multiplies by a rounded
    reciprocal where the resolve divides: about four roundings of relative size 2^-24 per frame on values no larger than the frame's colour,
    sixteen over the four frames, about 1e-6 of the largest colour blended.  Colours are not negative, so the mean of four is at least a
    quarter of the largest: 4e-6 of the result, under 1e-5 relative; the 1e-6 absolute covers results near zero.  Derived, not measured."""
    w, h, spp = 67, 45, 2
    probe = scenes.sky_probe(256, 128).BuildCDF()

    def ctx():
        r = R.SampleRenderer(scenes.cornell_box())
        r.setProbe(probe)
        r.resize((w, h))
        r.setCamera(R.make_camera(scenes.CORNELL_CAMERA, w / h))
        r.launchParams.samples_per_launch = spp
        return r

    a, b, c = ctx(), ctx(), ctx()
    g = a.renderGBuffer(("hit", "position"))
    hit, pos = g["hit"], g["position"]
    motion = torch.zeros((h, w, 2), device="cuda:0")
    hist = [torch.zeros((h, w, 4), device="cuda:0") for _ in range(2)]
    ln = [torch.zeros((h, w), device="cuda:0") for _ in range(2)]
    planes = dict(motion=np.zeros((h, w, 2), f32), hit=_np(hit), position=_np(pos))
    planes.update(prev_hit=planes["hit"], prev_position=planes["position"])
    chain_h, chain_l = np.zeros((h, w, 4), f32), np.zeros((h, w), f32)
    rects, px = _frame(w, h)
    a.uploadAccum(np.zeros((h, w, 4), f32))
    for k in range(4):
        # this frame's colour, from a second context: subframe k over a zeroed accumulation
        b.uploadAccum(np.zeros((h, w, 4), f32))
        b.launchParams.frame.subframe_index = k
        b.render()
        colour = b.download(R.PT_BUF_ACCUM)
        ref = T.temporal_ref(orc_det, dict(planes, color=colour, history_in=chain_h, length_in=chain_l), rects, px, color_scale=float(k + 1), clear=True)
        chain_h, chain_l = ref["history_out"].view(f32), ref["length_out"].view(f32)
        # the loop under test: render, then the pass with the recipe
        a.launchParams.frame.subframe_index = k
        a.render()
        res = a.temporalAccumulate(a.deviceBuffer(R.PT_BUF_ACCUM), motion, hit, pos, hit, pos, hist[k & 1], ln[k & 1], history_out=hist[~k & 1],
                                   length_out=ln[~k & 1], color_scale=float(k + 1), clear_color=True)
        assert res["stats"]["reprojected"] == (w * h if k else 0)
        assert not a.download(R.PT_BUF_ACCUM).any()
        # the plain progressive average
        c.launchParams.frame.subframe_index = k
        c.render()
    got_h, got_l = _np(hist[0]), _np(ln[0])
    assert np.array_equal(got_h.view(np.uint32), chain_h.view(np.uint32)) and np.array_equal(got_l, chain_l) and (got_l == 4).all()
    plain = c.download(R.PT_BUF_ACCUM)[..., :3]
    err = np.abs(got_h[..., :3].astype(np.float64) - plain)
    bound = 1e-5 * np.abs(plain) + 1e-6
    print("recipe: largest error / bound", float((err / bound).max()))
    assert (err <= bound).all(), float((err / bound).max())
    for r in (a, b, c):
        r.close()


# ------------------------------------------------------------------ 7. the rendering state is left alone
@pytest.mark.parametrize("frames_in_flight", [0, 3])
def test_rendering_state_is_left_alone(ptlib, orc_det, frames_in_flight):
    _, planes, prm = _case("two_box")
    probe = scenes.sky_probe(256, 128).BuildCDF()
    rects, px = _frame()

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
            _run(r, orc_det, planes, rects, px, "between the frames", clear=True, **prm)
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
        assert x.tobytes() == y.tobytes(), f"buffer {k} differs after a temporalAccumulate between the frames"


# ------------------------------------------------------------------ 8. refusals
def test_refusals(ptlib, orc_det):
    _, planes, prm = _case("two_box")
    L = _lib.load_library()
    r = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    dev = {k: _upload(planes[k]) for k in INPUTS}
    out = {k: _filled(k, H, W) for k in T.OUTPUTS}
    colour = planes["color"].view(np.uint32)
    ptr = {k: t.data_ptr() for k, t in list(dev.items()) + list(out.items())}
    good = dict(ptr, color_scale=1.0, normal_cos=0.9, plane_eps=0.01, min_weight=0.25, max_history=32, flags=0)

    def refused(what, pattern, **fields):
        d = _lib.TemporalDesc()
        for k, v in dict(good, **fields).items():
            setattr(d, k, v)
        torch.cuda.synchronize()
        s = _lib.TemporalStats(7, 7, 7.0)
        rc = L.pt_temporal_accumulate(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_temporal_accumulate") and pattern in msg, f"{what}: {msg!r}"
        assert (s.pixels, s.reprojected, s.kernel_ms) == (7, 7, 7.0)
        for k, t in out.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {k} was written"
        assert np.array_equal(_bits(dev["color"]), colour), f"{what}: color was written"

    refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, W / H))
    assert L.pt_temporal_accumulate(r._ctx, None, None) == -1 and "null description" in L.pt_last_error(r._ctx).decode()
    for name in INPUTS + ("history_out", "length_out"):
        refused(f"{name} null", f"{name} is null", **{name: None})
    host = np.zeros((H, W, 4), f32)
    refused("a host pointer", "history_in is not device memory", history_in=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "position is not 4-byte aligned", position=ptr["position"] + 2)
    refused("an optional plane offset by 1 byte", "copy_out is not 4-byte aligned", copy_out=ptr["copy_out"] + 1)
    # one element too small for what is left of its allocation (an allocation of the runtime's own: torch's allocator hands out parts of larger ones)
    hip = _hip_runtime()
    raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(raw), C.c_size_t(H * W * 8)) == 0
    try:
        assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= H * W * 8
        refused("a plane one element too small", f"motion has fewer than {H * W * 8} bytes left", motion=raw.value + size.value - (H * W * 8 - 4))
    finally:
        assert hip.hipFree(raw) == 0
    # forbidden overlaps: an output or the colour plane against anything; the read-only planes may alias (the recipe test passes prev_hit == hit)
    refused("history in place", "history_in and history_out overlap", history_out=ptr["history_in"])
    refused("length in place", "length_in and length_out overlap", length_out=ptr["length_in"])
    refused("the copy on the history", "history_out and copy_out overlap", copy_out=ptr["history_out"])
    refused("the frame on the lengths", "length_out and frame_rgba8 overlap", frame_rgba8=ptr["length_out"])
    refused("the lengths inside the colour plane", "color and length_out overlap", length_out=ptr["color"] + 4 * (H * W * 3))
    refused("colour as history", "color and history_in overlap", color=ptr["history_in"])
    refused("colour as output", "color and history_out overlap", history_out=ptr["color"])
    refused("an unknown flag", "unknown flag bits 2", flags=3)
    for name, bad, pattern in (("color_scale", (0.0, -1.0, np.inf, np.nan), "color_scale must be finite and > 0"),
                               ("normal_cos", (1.5, -1.5, np.nan), "normal_cos must be in [-1,1]"),
                               ("plane_eps", (-1.0, np.inf, np.nan), "plane_eps must be finite and >= 0"),
                               ("min_weight", (-0.1, 1.5, np.nan), "min_weight must be in [0,1]"),
                               ("max_history", (0, 65536), "max_history must be in [1,65535]")):
        for v in bad:
            refused(f"{name} = {v}", pattern, **{name: v})
    # the Python facade checks dtype, shape and device before the library is called
    args = dict(dev, **out)
    with pytest.raises(ValueError, match="length_in.*shape"):
        r.temporalAccumulate(**dict(args, length_in=dev["motion"]))
    with pytest.raises(ValueError, match="the tensor is on cpu"):
        r.temporalAccumulate(**dict(args, hit=torch.zeros((H, W, 8))))
    with pytest.raises(RuntimeError, match="history_in and history_out overlap"):
        r.temporalAccumulate(**dict(args, history_out=dev["history_in"]))
    # a valid call afterwards still works, into the same planes; the limits of the ranges are accepted
    rects, px = _frame()
    res = r.temporalAccumulate(**args, color_scale=1.0, normal_cos=-1.0, plane_eps=0.0, min_weight=1.0, max_history=65535)
    ref = T.temporal_ref(orc_det, planes, rects, px, normal_cos=-1.0, plane_eps=0.0, min_weight=1.0, max_history=65535)
    _same({k: _bits(out[k]) for k in out}, ref, "a valid call after the refusals")
    assert res["stats"]["reprojected"] == ref["reprojected"]
    # ... and so does one that lets the facade allocate its outputs (zero-filled)
    res = r.temporalAccumulate(**dev, max_history=1)
    ref = T.temporal_ref(orc_det, planes, rects, px, max_history=1, fill=0)
    _same({k: _bits(res[k]) for k in ("history_out", "length_out")}, ref, "allocated outputs")
    assert (_np(res["length_out"]) == 1).all()
    r.close()
