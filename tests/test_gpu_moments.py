"""The fused SVGF temporal stage (pt_temporal_moments) and the remodulation pass (pt_modulate_planes) on the GPU.  Every output plane is
compared bit for bit, over the WHOLE plane (so a pixel written outside the chosen set shows as a lost sentinel), with tests/moments_ref.py:
float32 NumPy evaluating the header's arithmetic; the colour plane (the clear) and the counters likewise.  One thing is not compared: which
NaN a NaN is (moments_ref.canon; the header leaves sign and payload open).  No tolerance anywhere.

Real-plane inputs: hit, position and motion from renderGBuffer (pinned by tests/test_gpu_gbuffer.py), tests/test_gpu_temporal.py's models,
cameras and seeds; colour, history, moments and albedo random, with NaN and inf colour and history words, length holes and one albedo word
in eight below albedo_min = 0.1.  tests/test_moments_cabi.py asserts on CPU-built planes, and this file on the GPU's, that at least 10 % of
the pixels are valid and 10 % are not, that at least 10 % of the valid pixels are clamped and 10 % are not, and that both denominator
branches are taken by at least 5 % of the albedo words (CPU-built planes: two_box 1240 valid of 7991, 556 clamped; terrain 2113, 978)."""
import ctypes as C

import numpy as np
import pytest
import torch

import moments_ref as MR
import temporal_ref as T
from gbuffer_ref import _row
from gpu_kit import filled, pixel_mask, plane_shape, whole_frame
from gpu_kit import bits as _bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from pass_cases import MOMENTS_INPUTS, moments_kwargs
from pass_cases import moments_case as _case

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 131, 61
SENTINEL = MR.SENTINEL
WORDS = dict(_lib.TMOM_PLANES, out=4, frame_rgba8=1)
FLAGS = [dict(), dict(clear=True), dict(clamp=True), dict(clamp=True, clear=True)]
FLAG_IDS = ["plain", "clear", "clamp", "clamp-clear"]


# ------------------------------------------------------------------ GPU helpers
def _filled(name, h, w, offset=False):
    """a sentinel-filled plane of the pass; offset: one float into its allocation (4-byte aligned only)"""
    return filled(plane_shape(h, w, WORDS[name]), offset, torch.int32 if name == "frame_rgba8" else torch.float32)


def _same(got, ref, what):
    for name, a in got.items():
        b = ref[name]
        if name not in ("frame_rgba8", "color"):  # (packed bytes and copied words are compared as they are)
            a, b = MR.canon(a), MR.canon(b)
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {name} differs from float32 NumPy in {int((a != b).sum())} words"


def _run(r, planes, rects, pixels, what, mask=None, blocks=None, offset=False, outputs=MR.OUTPUTS, **prm):
    """uploads the planes, calls temporalMoments into sentinel-filled outputs, compares every output, the colour plane and the counters
    with the NumPy reference over the whole frame; returns (reference, stats, the outputs' bits)"""
    h, w = planes["length_in"].shape
    dev = {k: _upload(planes[k], offset) for k in MOMENTS_INPUTS if planes.get(k) is not None}
    for k in ("prev_hit", "prev_position"):  # read-only planes may alias one another
        if planes[k] is planes[k[5:]]:
            dev[k] = dev[k[5:]]
    out = {k: _filled(k, h, w, offset) for k in outputs}
    res = r.temporalMoments(**dev, **out, variance="variance_out" in outputs, mask=mask, **moments_kwargs(prm))
    assert all(res[k] is out[k] for k in outputs)
    ref = MR.moments_ref(planes, rects, pixels, blocks=blocks, **prm)
    got = {k: _bits(out[k]) for k in outputs}
    _same(dict(got, color=_bits(dev["color"])), ref, what)
    st = res["stats"]
    want = (int(np.asarray(pixels).sum()), ref["reprojected"], ref["clamped"])
    assert (st["pixels"], st["reprojected"], st["clamped"]) == want, (what, st, want)
    assert st["kernel_ms"] > 0 if st["pixels"] else st["kernel_ms"] >= 0
    return ref, st, got


def _flat(w, h, seed):
    """one surface, no motion, one frame of history everywhere (every pixel valid), a random albedo"""
    rng = np.random.default_rng(seed)
    hit = np.zeros((h, w, 8), f32)
    hit[..., 0], hit[..., 7] = 4, 1
    pos = np.zeros((h, w, 4), f32)
    pos[..., 3] = 1
    return dict(color=rng.random((h, w, 4), dtype=f32), albedo=MR.random_albedo(rng, h, w), motion=np.zeros((h, w, 2), f32), hit=hit, position=pos,
                prev_hit=hit, prev_position=pos, history_in=rng.random((h, w, 4), dtype=f32), moments_in=MR.random_moments(rng, h, w),
                length_in=np.ones((h, w), f32))


def _synthetic(w, h):
    planes = T.synthetic_planes(w, h, 7 + w)
    rng = np.random.default_rng(70 + w)
    return dict(planes, moments_in=MR.random_moments(rng, h, w), albedo=MR.random_albedo(rng, h, w))


def _frame(w=W, h=H):
    return whole_frame(w, h)


# ------------------------------------------------------------------ 1. real planes, the four flag combinations
@pytest.mark.parametrize("prm", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_real_planes(ptlib, name, prm):
    r, planes, base = _case(name)
    rects, px = _frame()
    ref, st, _ = _run(r, planes, rects, px, f"{name} {prm}", **dict(base, **prm))
    print(f"{name} {prm}: reprojected {st['reprojected']} clamped {st['clamped']} window rejects {ref['window_rejects']} kernel_ms {st['kernel_ms']:.4f}")
    if prm.get("clamp"):
        MR.check_coverage(planes, ref, px, name)
        assert ref["window_rejects"]["rect"] > 0 and ref["window_rejects"]["finite"] > 0
    else:
        assert st["clamped"] == 0


def test_optional_planes_and_the_ends_of_the_ranges(ptlib):
    r, planes, base = _case("terrain")
    rects, px = _frame()
    _run(r, dict(planes, albedo=None), rects, px, "no albedo, clamp", clamp=True, color_scale=3.0, max_history=4, **dict(base, clamp_k=0.5))
    _run(r, planes, rects, px, "no variance_out", outputs=MR.OUTPUTS[:3], clamp=True, **base)
    _run(r, planes, rects, px, "clamp_k 0", clamp=True, **dict(base, clamp_k=0.0, albedo_min=0.0, min_weight=0.0))
    _run(r, planes, rects, px, "the other ends", clamp=True, **dict(base, clamp_k=1e6, albedo_min=2.0, min_weight=1.0, normal_cos=-1.0, max_history=1))
    # without the flag clamp_k is not read: a NaN there is not refused
    dev = {k: _upload(planes[k]) for k in MOMENTS_INPUTS}
    res = r.temporalMoments(**dev, **dict(moments_kwargs(base), clamp_k=None))
    d = _lib.TMomDesc()
    for k, t in list(dev.items()) + [(k, res[k]) for k in MR.OUTPUTS]:
        setattr(d, k, t.data_ptr())
    for k, v in dict(color_scale=1.0, albedo_min=base["albedo_min"], normal_cos=0.9, plane_eps=base.get("plane_eps", 0.01), min_weight=0.25, clamp_k=np.nan,
                     max_history=32, flags=0).items():
        setattr(d, k, v)
    want = {k: _bits(res[k]) for k in MR.OUTPUTS}
    torch.cuda.synchronize()
    assert _lib.load_library().pt_temporal_moments(r._ctx, C.byref(d), None) == 0
    _same({k: _bits(res[k]) for k in MR.OUTPUTS}, want, "clamp_k NaN without the flag")


# ------------------------------------------------------------------ 2. against the existing pass, on the GPU
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_reduces_to_two_temporal_accumulate_calls(ptlib, name):
    """albedo=None, flags 0, finite moments: history_out, length_out and moments_out equal two temporalAccumulate calls — one on the colour,
    one on the plane (l, l*l, 0, 1) against the history (moments_in, z, 1), z as tests/test_moments_cabi.py's reduction states it (0 where
    the colour history is finite, the offending word elsewhere: the fused pass has ONE tap set)."""
    r, planes, base = _case(name)
    h, w = planes["length_in"].shape
    prm = dict(plane_eps=base.get("plane_eps", 0.01), color_scale=2.0, max_history=8)
    dev = {k: _upload(planes[k]) for k in MOMENTS_INPUTS if k != "albedo"}
    fused = r.temporalMoments(**dev, **prm)
    geo = [dev[k] for k in ("motion", "hit", "position", "prev_hit", "prev_position")]
    col = r.temporalAccumulate(dev["color"], *geo, dev["history_in"], dev["length_in"], **prm)
    with np.errstate(all="ignore"):
        l = MR.lum(planes["color"][..., :3] * f32(2.0))
        mplane = np.stack([l, l * l, np.zeros_like(l), np.ones_like(l)], -1)
    hist = planes["history_in"][..., :3]
    bad = ~MR._finite(hist)
    z = np.where(bad.any(-1), np.take_along_axis(hist, bad.argmax(-1)[..., None], -1)[..., 0], f32(0)).astype(f32)
    mhist = np.concatenate([planes["moments_in"], z[..., None], np.ones((h, w, 1), f32)], -1)
    mom = r.temporalAccumulate(_upload(mplane), *geo, _upload(mhist), dev["length_in"], **dict(prm, color_scale=1.0))
    _same(dict(history_out=_bits(fused["history_out"]), length_out=_bits(fused["length_out"])),
          dict(history_out=_bits(col["history_out"]), length_out=_bits(col["length_out"])), name)
    _same(dict(moments_out=_bits(fused["moments_out"])), dict(moments_out=_bits(mom["history_out"])[..., :2]), name)
    assert np.array_equal(_bits(mom["length_out"]), _bits(col["length_out"]))
    assert fused["stats"]["reprojected"] == col["stats"]["reprojected"] == mom["stats"]["reprojected"] > 0 and fused["stats"]["clamped"] == 0


# ------------------------------------------------------------------ 3. hand-made planes on small frames
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (9, 8), (63, 1), (65, 3)])
def test_synthetic_planes_on_small_frames(ptlib, size):
    w, h = size
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), size, scenes.TWO_BOX_CAMERA)
    planes = _synthetic(w, h)
    rects, px = _frame(w, h)
    ref, _, _ = _run(r, planes, rects, px, f"{w} x {h}", clamp=True, clear=True, min_weight=0.6, albedo_min=MR.ALBEDO_MIN)
    if w * h >= 64:
        assert 0 < ref["reprojected"] < w * h and ref["window_rejects"]["rect"] > 0
    _run(r, planes, rects, px, f"{w} x {h}, any weight, no clamp", min_weight=0.0, albedo_min=MR.ALBEDO_MIN)
    # every pixel valid: the window meets every edge of the rectangle and the partial last block
    flat = _flat(w, h, 3 + w)
    ref, _, _ = _run(r, flat, rects, px, f"{w} x {h}, flat", clamp=True, albedo_min=MR.ALBEDO_MIN)
    assert ref["reprojected"] == w * h and ref["window"].max() == min(w, 3) * min(h, 3) and ref["window"].min() == min(w, 2) * min(h, 2)
    r.close()


# ------------------------------------------------------------------ 4. views
def test_two_views_side_by_side(ptlib):
    w, h, ew = 64, 16, 32
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), (w, h), scenes.TWO_BOX_CAMERA)
    cam = R.make_camera(scenes.TWO_BOX_CAMERA, ew / h)
    r.setViews([(0, 0, ew, h, cam), (ew, 0, ew, h, cam)])
    rects = [(0, 0, ew, h), (ew, 0, ew, h)]
    px = np.ones((h, w), bool)
    base = _flat(w, h, 17)
    spiked = dict(base, color=base["color"].copy())
    spiked["color"][:, ew, :3] = 1e6  # the first column of the right view
    prm = dict(clamp=True, albedo_min=MR.ALBEDO_MIN)
    ra, _, a = _run(r, base, rects, px, "two views", **prm)
    rb, _, b = _run(r, spiked, rects, px, "two views, a bright column across the border", **prm)
    assert ra["window"][h // 2, ew - 1] == 6 and ra["window_rejects"]["rect"] == 2 * 3 * 2 * (ew + h) - 8
    for name in MR.OUTPUTS:  # no output bit of the left view changes; the right view's does
        assert np.array_equal(a[name][:, :ew], b[name][:, :ew]), name
    assert not np.array_equal(a["history_out"][:, ew:], b["history_out"][:, ew:])
    # views dropped: one rectangle, and now the window does cross
    r.setViews([])
    _, _, c = _run(r, spiked, [(0, 0, w, h)], px, "views dropped", **prm)
    assert not np.array_equal(c["history_out"][:, ew - 1], b["history_out"][:, ew - 1])
    r.close()


# ------------------------------------------------------------------ 5. masks and partition
def test_masks(ptlib):
    r, planes, base = _case("two_box")
    nby, nbx = r.blockGrid()
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.4
    mask[0, 0] = mask[nby - 1, nbx - 1] = mask[0, nbx - 1] = mask[nby - 1, 3] = True  # corner and edge blocks, the 3-wide column and the 5-high row
    mask[1, 1] = False
    px = pixel_mask(mask, h=H, w=W)
    color = planes["color"].copy()
    color[~px, :3] = 1e6  # the excluded blocks: the window does not count them
    p = dict(planes, color=color)
    ref, st, got = _run(r, p, [(0, 0, W, H)], px, "a random block mask", mask=mask, blocks=mask, clamp=True, clear=True, **base)
    assert 0 < st["pixels"] < W * H and ref["window_rejects"]["block"] > 0 and (got["history_out"][~px] == SENTINEL).all()
    v = got["history_out"].view(f32)[px][:, :3]
    assert not (np.isfinite(v) & (v >= 1e5)).any()
    _run(r, p, [(0, 0, W, H)], px, "the mask, no clamp", mask=mask, blocks=mask, **base)
    none = np.zeros((nby, nbx), bool)
    _, st, _ = _run(r, p, [(0, 0, W, H)], np.zeros((H, W), bool), "the empty mask", mask=none, blocks=none, clamp=True, clear=True, **base)
    assert st == dict(pixels=0, reprojected=0, clamped=0, kernel_ms=st["kernel_ms"])


def test_partition(ptlib):
    _, planes, base = _case("two_box")
    make, size, cam, _, _, _ = T.real_inputs()["two_box"]
    by, bx = np.mgrid[0:H, 0:W] // 8
    written = np.zeros((H, W), int)
    for rank in range(2):
        r = _renderer(make(), size, cam, partition=(rank, 2, 8, 8))
        own = (bx + by) % 2 == rank
        color = planes["color"].copy()
        color[~own, :3] = 1e6  # the other rank's blocks: a neighbour there does not count
        p = dict(planes, color=color, length_in=np.where(own, planes["length_in"], f32(0)))  # the rank never wrote the others' pixels
        blocks = _block_set(own)
        ref, st, got = _run(r, p, [(0, 0, W, H)], own, f"rank {rank}", blocks=blocks, clamp=True, **base)
        assert st["pixels"] == int(own.sum()) and ref["reprojected"] > 0 and ref["window_rejects"]["block"] > 0
        v = got["history_out"].view(f32)[own][:, :3]
        assert not (np.isfinite(v) & (v >= 1e5)).any()
        written += got["length_out"] != SENTINEL
        r.close()
    assert (written == 1).all()  # the union is the frame, overlaps are empty


def _block_set(pixels):
    h, w = pixels.shape
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    pad = np.zeros((nby * 8, nbx * 8), bool)
    pad[:h, :w] = pixels
    return pad.reshape(nby, 8, nbx, 8).any((1, 3))


# ------------------------------------------------------------------ 6. the clear
@pytest.mark.parametrize("size", [(65, 3), (131, 61)])
def test_clear_is_behind_every_read(ptlib, size):
    """more than one block (65 x 3) and more than one workgroup (131 x 61): the outputs equal the run without the flag — no window read saw
    a zeroed neighbour — and color is 0 inside the set and untouched outside"""
    w, h = size
    if size == (W, H):
        r, planes, base = _case("terrain")
    else:
        r, planes, base = _renderer(scenes.two_box_scene(shadow_catcher=False), size, scenes.TWO_BOX_CAMERA), _flat(w, h, 9), dict(albedo_min=MR.ALBEDO_MIN)
    nby, nbx = r.blockGrid()
    mask = np.ones((nby, nbx), bool)
    mask[nby - 1, 1] = mask[0, nbx - 2] = False
    px = pixel_mask(mask, h=h, w=w)
    rects = [(0, 0, w, h)]
    _, _, plain = _run(r, planes, rects, px, "without the clear", mask=mask, blocks=mask, clamp=True, **base)
    ref, _, cleared = _run(r, planes, rects, px, "with the clear", mask=mask, blocks=mask, clamp=True, clear=True, **base)
    for name in MR.OUTPUTS:
        assert np.array_equal(plain[name], cleared[name]), name
    assert not ref["color"][px].any() and np.array_equal(ref["color"][~px], np.ascontiguousarray(planes["color"]).view(np.uint32)[~px]) and (~px).any()
    if size != (W, H):
        r.close()


# ------------------------------------------------------------------ 7. alignment and the context's own buffers
def test_planes_four_byte_aligned_only(ptlib):
    r, planes, base = _case("terrain")
    rects, px = _frame()
    _run(r, planes, rects, px, "planes one float into their allocations", offset=True, clamp=True, clear=True, **base)


def test_context_buffers_as_planes(ptlib, orc_det):
    """PT_BUF_ACCUM (with the clear) and PT_BUF_ALBEDO as planes after a real render of the textured scene, then the chain's end:
    modulatePlanes with PT_BUF_ALBEDO into PT_BUF_COLOR and PT_BUF_FRAME"""
    w, h = 96, 64
    r = _renderer(scenes.textured_scene(), (w, h), scenes.TWO_BOX_CAMERA)  # (the scene spans +-4 about the origin, like the two-box scene)
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.launchParams.samples_per_launch = 2
    r.uploadAccum(np.zeros((h, w, 4), f32))
    r.launchParams.frame.subframe_index = 2
    r.render()
    g = r.renderGBuffer(("hit", "position", "motion"), prev_cameras=_row(scenes.TWO_BOX_CAMERA, w / h))
    kinds = (R.PT_BUF_ACCUM, R.PT_BUF_FRAME, R.PT_BUF_COLOR, R.PT_BUF_NORMAL, R.PT_BUF_ALBEDO)
    before = {k: r.download(k) for k in kinds}
    albedo = before[R.PT_BUF_ALBEDO]
    print(f"context buffers: {float((albedo[..., :3] > 0.05).mean()):.3f} of the albedo words above albedo_min")
    assert (albedo[..., :3] > 0.05).any()  # the render wrote a first-hit albedo: the demodulation divides by it
    rng = np.random.default_rng(41)
    planes = dict(color=before[R.PT_BUF_ACCUM], albedo=albedo, motion=_np(g["motion"]), hit=_np(g["hit"]), position=_np(g["position"]),
                  history_in=rng.random((h, w, 4), dtype=f32), moments_in=MR.random_moments(rng, h, w), length_in=rng.integers(0, 6, (h, w)).astype(f32))
    planes["prev_hit"], planes["prev_position"] = planes["hit"], planes["position"]
    nby, nbx = r.blockGrid()
    mask = np.random.default_rng(9).random((nby, nbx)) < 0.6
    px = pixel_mask(mask, h=h, w=w)
    prm = dict(color_scale=3.0, albedo_min=0.05, clamp=True, clamp_k=1.5, clear=True)
    dev = {k: _upload(planes[k]) for k in MOMENTS_INPUTS if k not in ("color", "albedo", "prev_hit", "prev_position")}
    out = {k: _filled(k, h, w) for k in MR.OUTPUTS}
    res = r.temporalMoments(color=r.deviceBuffer(R.PT_BUF_ACCUM), albedo=r.deviceBuffer(R.PT_BUF_ALBEDO), prev_hit=dev["hit"], prev_position=dev["position"],
                            **dev, **out, mask=mask, **moments_kwargs(prm))
    ref = MR.moments_ref(planes, [(0, 0, w, h)], px, blocks=mask, **prm)
    _same({k: _bits(out[k]) for k in MR.OUTPUTS}, ref, "context buffers")
    st = res["stats"]
    assert (st["pixels"], st["reprojected"], st["clamped"]) == (int(px.sum()), ref["reprojected"], ref["clamped"]) and ref["reprojected"] > 0
    after = {k: r.download(k) for k in kinds}
    accum = after[R.PT_BUF_ACCUM].view(np.uint32)
    assert not accum[px].any() and np.array_equal(accum[~px], before[R.PT_BUF_ACCUM].view(np.uint32)[~px])  # zero exactly at the processed pixels
    for k in kinds[1:]:
        assert after[k].tobytes() == before[k].tobytes()
    # the end of the chain into the context's own buffers
    m = r.modulatePlanes(out["history_out"], albedo=r.deviceBuffer(R.PT_BUF_ALBEDO), out=r.deviceBuffer(R.PT_BUF_COLOR), frame=r.deviceBuffer(R.PT_BUF_FRAME),
                         mask=mask, albedo_min=0.05)
    want = MR.modulate_ref(orc_det, _np(out["history_out"]), albedo, px, albedo_min=0.05)
    assert m["out"] is None and m["frame_rgba8"] is None and m["stats"]["pixels"] == int(px.sum())
    col, fr = r.download(R.PT_BUF_COLOR).view(np.uint32), r.download(R.PT_BUF_FRAME).view(np.uint32)
    assert np.array_equal(MR.canon(col[px]), MR.canon(want["out"][px])) and np.array_equal(col[~px], before[R.PT_BUF_COLOR].view(np.uint32)[~px])
    assert np.array_equal(fr[px], want["frame_rgba8"][px]) and np.array_equal(fr[~px], before[R.PT_BUF_FRAME].view(np.uint32)[~px])
    r.close()


# ------------------------------------------------------------------ 8. the rendering state is left alone
@pytest.mark.parametrize("frames_in_flight", [0, 3])
def test_rendering_state_is_left_alone(ptlib, orc_det, frames_in_flight):
    _, planes, base = _case("two_box")
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
            _, _, got = _run(r, planes, rects, px, "between the frames", clamp=True, **base)
            _modulate(r, orc_det, got["history_out"], planes["albedo"], px, "between the frames")
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
        assert x.tobytes() == y.tobytes(), f"buffer {k} differs after a temporalMoments and a modulatePlanes between the frames"


# ------------------------------------------------------------------ 9. refusals
def test_refusals(ptlib):
    _, planes, base = _case("two_box")
    L = _lib.load_library()
    r = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    dev = {k: _upload(planes[k]) for k in MOMENTS_INPUTS}
    out = {k: _filled(k, H, W) for k in MR.OUTPUTS}
    color_before = _bits(dev["color"])
    ptr = {k: t.data_ptr() for k, t in list(dev.items()) + list(out.items())}
    good = dict(ptr, color_scale=1.0, albedo_min=0.1, normal_cos=0.9, plane_eps=0.01, min_weight=0.25, clamp_k=1.0, max_history=32, flags=3)

    def refused(what, pattern, **fields):
        d = _lib.TMomDesc()
        for k, v in dict(good, **fields).items():
            setattr(d, k, v)
        torch.cuda.synchronize()
        s = _lib.TMomStats(7, 7, 7, 7.0)
        rc = L.pt_temporal_moments(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_temporal_moments") and pattern in msg, f"{what}: {msg!r}"
        assert (s.pixels, s.reprojected, s.clamped, s.kernel_ms) == (7, 7, 7, 7.0)
        for k, t in out.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {k} was written"
        assert np.array_equal(_bits(dev["color"]), color_before), f"{what}: color was cleared"

    refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, W / H))
    assert L.pt_temporal_moments(r._ctx, None, None) == -1 and "null description" in L.pt_last_error(r._ctx).decode()
    for name in MOMENTS_INPUTS + MR.OUTPUTS:
        if name not in ("albedo", "variance_out"):
            refused(f"{name} null", f"{name} is null", **{name: None})
    host = np.zeros((H, W, 4), f32)
    refused("a host pointer", "albedo is not device memory", albedo=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "moments_in is not 4-byte aligned", moments_in=ptr["moments_in"] + 2)
    refused("an optional output offset by 1 byte", "variance_out is not 4-byte aligned", variance_out=ptr["variance_out"] + 1)
    # one element too small for what is left of its allocation (an allocation of the runtime's own: torch's allocator hands out parts of larger ones)
    hip = _hip_runtime()
    raw, base_, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(raw), C.c_size_t(H * W * 8)) == 0
    try:
        assert hip.hipMemGetAddressRange(C.byref(base_), C.byref(size), raw) == 0 and base_.value == raw.value and size.value >= H * W * 8
        refused("a plane one element too small", f"moments_out has fewer than {H * W * 8} bytes left", moments_out=raw.value + size.value - (H * W * 8 - 4))
    finally:
        assert hip.hipFree(raw) == 0
    # forbidden overlaps: color and the four outputs against anything; the read-only planes may alias
    refused("history in place", "history_in and history_out overlap", history_out=ptr["history_in"])
    refused("moments in place", "moments_in and moments_out overlap", moments_out=ptr["moments_in"])
    refused("the variance inside the history", "history_out and variance_out overlap", variance_out=ptr["history_out"] + 16)
    refused("color on the albedo", "color and albedo overlap", albedo=ptr["color"])
    refused("color as the history", "color and history_in overlap", history_in=ptr["color"])
    refused("the moments on the output", "history_out and moments_out overlap", moments_out=ptr["history_out"] + 8)
    refused("a flag", "unknown flag bits 4", flags=7)
    for name, bad, pattern in (("color_scale", (0.0, -1.0, np.inf, np.nan), "color_scale must be finite and > 0"),
                               ("albedo_min", (-0.5, np.inf, np.nan), "albedo_min must be finite and >= 0"),
                               ("normal_cos", (1.5, -1.5, np.nan), "normal_cos must be in [-1,1]"),
                               ("plane_eps", (-1.0, np.inf, np.nan), "plane_eps must be finite and >= 0"),
                               ("min_weight", (-0.1, 1.5, np.nan), "min_weight must be in [0,1]"),
                               ("clamp_k", (-1.0, np.inf, np.nan), "clamp_k must be finite and >= 0"),
                               ("max_history", (0, 65536), "max_history must be in [1,65535]")):
        for v in bad:
            refused(f"{name} = {v}", pattern, **{name: v})
    # the Python facade checks dtype, shape and device before the library is called; the library's refusal is an exception
    with pytest.raises(ValueError, match="moments_in.*shape"):
        r.temporalMoments(**dict(dev, moments_in=dev["position"]), **out)
    with pytest.raises(ValueError, match="the tensor is on cpu"):
        r.temporalMoments(**dict(dev, hit=torch.zeros((H, W, 8))), **out)
    with pytest.raises(RuntimeError, match="history_in and history_out overlap"):
        r.temporalMoments(**dev, **dict(out, history_out=dev["history_in"]))
    # a valid call afterwards still works, into the same planes; read-only planes may alias (prev_hit == hit)
    rects, px = _frame()
    p = dict(planes, prev_hit=planes["hit"], prev_position=planes["position"])
    res = r.temporalMoments(**dict(dev, prev_hit=dev["hit"], prev_position=dev["position"]), **out, **moments_kwargs(dict(base, clamp=True)))
    ref = MR.moments_ref(p, rects, px, clamp=True, **base)
    _same({k: _bits(out[k]) for k in MR.OUTPUTS}, ref, "a valid call after the refusals")
    assert res["stats"]["reprojected"] == ref["reprojected"] and res["stats"]["clamped"] == ref["clamped"]
    # ... and so does one that lets the facade allocate its outputs (zero-filled)
    res = r.temporalMoments(**dev, **moments_kwargs(base))
    _same({k: _bits(res[k]) for k in MR.OUTPUTS}, MR.moments_ref(planes, rects, px, fill=0, **base), "allocated outputs")
    r.close()


# ------------------------------------------------------------------ 10. modulatePlanes
def _modulate(r, orc, color, albedo, pixels, what, mask=None, albedo_min=MR.ALBEDO_MIN, offset=False):
    """out of place into sentinel-filled planes (float and RGBA8), RGBA8 alone, and in place; each against modulate_ref over the whole frame"""
    color = np.ascontiguousarray(color).view(f32)
    h, w = color.shape[:2]
    ref = MR.modulate_ref(orc, color, albedo, pixels, albedo_min=albedo_min)
    n = int(np.asarray(pixels).sum())
    c, a = _upload(color, offset), (None if albedo is None else _upload(albedo, offset))
    out, fr = _filled("out", h, w, offset), _filled("frame_rgba8", h, w, offset)
    res = r.modulatePlanes(c, albedo=a, out=out, frame=fr, mask=mask, albedo_min=albedo_min)
    assert res["out"] is out and res["frame_rgba8"] is fr and res["stats"]["pixels"] == n
    _same(dict(out=_bits(out), frame_rgba8=_bits(fr)), ref, f"{what}: out of place")
    assert np.array_equal(_bits(c), color.view(np.uint32))
    fr8 = _filled("frame_rgba8", h, w, offset).view(torch.uint8).view(h, w, 4)
    res = r.modulatePlanes(c, albedo=a, frame=fr8, mask=mask, albedo_min=albedo_min, write_out=False)
    assert res["out"] is None and np.array_equal(_bits(fr8.view(torch.int32).view(h, w)), ref["frame_rgba8"]), f"{what}: RGBA8 only"
    res = r.modulatePlanes(c, albedo=a, out=c, mask=mask, albedo_min=albedo_min)
    inplace = dict(out=np.where(np.asarray(pixels, bool)[..., None], ref["out"], color.view(np.uint32)))
    _same(dict(out=_bits(c)), inplace, f"{what}: in place")
    return ref


def test_modulate_planes(ptlib, orc_det):
    r, planes, _ = _case("terrain")
    rects, px = _frame()
    rng = np.random.default_rng(3)
    color = planes["color"].copy()
    color[..., 3] = rng.random((H, W), dtype=f32)  # the fourth word is carried over
    ref = _modulate(r, orc_det, color, planes["albedo"], px, "whole frame")
    assert not (ref["out"] == SENTINEL).any()
    _modulate(r, orc_det, color, None, px, "no albedo")
    _modulate(r, orc_det, color, planes["albedo"], px, "one float into the allocations", offset=True)
    nby, nbx = r.blockGrid()
    mask = rng.random((nby, nbx)) < 0.4
    mask[nby - 1, nbx - 1] = True
    _modulate(r, orc_det, color, planes["albedo"], pixel_mask(mask, h=H, w=W), "a block mask", mask=mask)
    none = np.zeros((nby, nbx), bool)
    _modulate(r, orc_det, color, planes["albedo"], np.zeros((H, W), bool), "the empty mask", mask=none)
    # the stated branches of the denominator
    amin = f32(0.1)
    alb = np.ones((H, W, 4), f32)
    alb[0, :7, 1] = [0.0, np.nan, amin, np.nextafter(amin, f32(1)), -1.0, np.inf, 0.75]
    _modulate(r, orc_det, color, alb, px, "branch words", albedo_min=float(amin))


def test_modulate_planes_with_views(ptlib, orc_det):
    from scene_kit import RECTS, _views_and_prev

    r = _renderer(scenes.two_box_scene(shadow_catcher=False), (W, H), scenes.TWO_BOX_CAMERA)
    views, _ = _views_and_prev()
    r.setViews(views)
    inside = np.zeros((H, W), bool)
    for x, y, w, h in RECTS:
        inside[y:y + h, x:x + w] = True
    rng = np.random.default_rng(8)
    _modulate(r, orc_det, rng.random((H, W, 4), dtype=f32), MR.random_albedo(rng, H, W), inside, "four views")
    r.close()


def test_modulate_refusals(ptlib):
    _, planes, _ = _case("two_box")
    L = _lib.load_library()
    r = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    dev = dict(color=_upload(planes["color"]), albedo=_upload(planes["albedo"]))
    out = dict(out=_filled("out", H, W), frame_rgba8=_filled("frame_rgba8", H, W))
    ptr = {k: t.data_ptr() for k, t in list(dev.items()) + list(out.items())}
    good = dict(ptr, albedo_min=0.1, flags=0)
    color_before = _bits(dev["color"])

    def refused(what, pattern, **fields):
        d = _lib.ModulateDesc()
        for k, v in dict(good, **fields).items():
            setattr(d, k, v)
        torch.cuda.synchronize()
        s = _lib.ModulateStats(7, 7.0)
        rc = L.pt_modulate_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_modulate_planes") and pattern in msg, f"{what}: {msg!r}"
        assert (s.pixels, s.kernel_ms) == (7, 7.0)
        for k, t in out.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {k} was written"
        assert np.array_equal(_bits(dev["color"]), color_before), f"{what}: color was written"

    refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, W / H))
    assert L.pt_modulate_planes(r._ctx, None, None) == -1 and "null description" in L.pt_last_error(r._ctx).decode()
    refused("color null", "color is null", color=None)
    refused("no output", "no output asked for", out=None, frame_rgba8=None)
    refused("a host pointer", "albedo is not device memory", albedo=np.zeros((H, W, 4), f32).ctypes.data)
    refused("a pointer offset by 2 bytes", "out is not 4-byte aligned", out=ptr["out"] + 2)
    refused("the output one word into the colour", "color and out overlap", out=ptr["color"] + 4)  # (the allocation has one spare word)
    refused("the output on the albedo", "albedo and out overlap", out=ptr["albedo"])
    refused("the frame on the colour", "color and frame_rgba8 overlap", frame_rgba8=ptr["color"])
    refused("the frame inside the output", "out and frame_rgba8 overlap", frame_rgba8=ptr["out"] + 4 * (H * W * 3))
    refused("in place with the frame on it", "frame_rgba8 overlap", out=ptr["color"], frame_rgba8=ptr["color"] + 16)
    refused("a flag", "unknown flag bits 1", flags=1)
    for v in (-0.5, np.inf, np.nan):
        refused(f"albedo_min = {v}", "albedo_min must be finite and >= 0", albedo_min=v)
    with pytest.raises(RuntimeError, match="albedo and out overlap"):
        r.modulatePlanes(dev["color"], albedo=dev["albedo"], out=dev["albedo"])
    r.close()
