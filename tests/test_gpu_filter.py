"""The chain's filter (pt_filter_planes) on the GPU.  `out` and `frame_rgba8` are compared bit for bit, over the WHOLE plane (so a pixel
written outside the chosen set shows as a lost sentinel), with tests/filter_ref.py: float32 NumPy evaluating the header's arithmetic, with
the CPU checker's make_color; `scratch` must keep its sentinel outside the set.  One thing is not compared: which NaN a NaN variance word
is (filter_ref.canon says why).  No tolerance anywhere; the one inequality of this file is the chain test's, which says where it comes from.

Real-plane inputs (hit and position from renderGBuffer, pinned by tests/test_gpu_gbuffer.py; colour, variance and length: random, with NaN,
inf, negative and zero words).  Rejected candidate taps per reason / counting taps / pixels taking the spatial estimate / non-inert pixels,
as tests/test_filter_cabi.py counts them on CPU-built planes with five passes (the test asserts the same coverage on the GPU's planes and
prints its counts):
  two_box 131 x 61, plane_eps 0:  rect 93251 inert 68922 mesh 34588 normal 9455 plane 406468 / 241092 / 1897 / 4767
  terrain 131 x 61:               rect 100640 inert 69237 mesh 255486 normal 223179 plane 69223 / 212779 / 2113 / 5182"""
import ctypes as C

import numpy as np
import pytest
import torch

import filter_ref as F
from gpu_kit import filled, pixel_mask, plane_shape, whole_frame
from gpu_kit import bits as _bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from pass_cases import FILTER_INPUTS
from pass_cases import filter_case as _case
from scene_kit import RECTS, _views_and_prev

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 131, 61
SENTINEL = F.SENTINEL
WORDS = _lib.FILTER_PLANES


# ------------------------------------------------------------------ GPU helpers
def _filled(name, h, w, offset=False):
    """a sentinel-filled plane of the pass; offset: one float into its allocation (4-byte aligned only)"""
    return filled(plane_shape(h, w, WORDS[name]), offset, torch.int32 if name == "frame_rgba8" else torch.float32)


def _same(out, frame, scratch, ref, pixels, what):
    a, b = F.canon(out), F.canon(ref["out"])
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: out differs from float32 NumPy in {int((a != b).sum())} words"
    if frame is not None:
        assert np.array_equal(frame, ref["frame_rgba8"]), f"{what}: frame_rgba8 differs in {int((frame != ref['frame_rgba8']).sum())} pixels"
    if scratch is not None:
        assert (scratch[~np.asarray(pixels, bool)] == SENTINEL).all(), f"{what}: scratch was written outside the set"


def _run(r, orc, planes, rects, pixels, what, mask=None, blocks=None, offset=False, frame=True, **prm):
    """uploads the planes, calls filterPlanes into sentinel-filled outputs, compares out and frame_rgba8 with the NumPy reference over the
    whole frame and scratch outside the set with its sentinel; returns (reference, stats)"""
    h, w = planes["hit"].shape[:2]
    dev = {k: _upload(planes[k], offset) for k in FILTER_INPUTS if planes.get(k) is not None}
    its = prm.get("iterations", F.DEFAULTS["iterations"])
    out = _filled("out", h, w, offset)
    scratch = _filled("scratch", h, w, offset) if its >= 1 else None
    fr = _filled("frame_rgba8", h, w, offset) if frame else None
    res = r.filterPlanes(**dev, out=out, scratch=scratch, frame=fr, mask=mask, **prm)
    assert res["out"] is out and res["scratch"] is scratch and res["frame_rgba8"] is fr
    ref = F.filter_ref(orc, planes, rects, pixels, blocks=blocks, **prm)
    _same(_bits(out), _bits(fr) if frame else None, _bits(scratch) if scratch is not None else None, ref, pixels, what)
    st = res["stats"]
    assert (st["pixels"], st["filtered"], st["spatial"]) == (int(np.asarray(pixels).sum()), ref["filtered"], ref["spatial"]), (what, st, ref["filtered"], ref["spatial"])
    assert st["kernel_ms"] > 0 if st["pixels"] else st["kernel_ms"] >= 0
    return ref, st


def _frame(w=W, h=H):
    return whole_frame(w, h)


# ------------------------------------------------------------------ 1. real planes
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_real_planes(ptlib, orc_det, name):
    r, planes, prm = _case(name)
    rects, px = _frame()
    ref, st = _run(r, orc_det, planes, rects, px, name, iterations=5, **prm)
    rej, cnt, sp, fl = F.check_coverage(ref, name)
    print(f"{name}: rejected {rej} counting {cnt} spatial {sp} filtered {fl} kernel_ms {st['kernel_ms']:.4f}")
    assert all(rej[k] > 0 for k in ("rect", "inert", "mesh", "normal", "plane"))
    # step 16 exceeds a quarter of the height: in the middle row both outer tap rows of the fifth pass leave the rectangle
    assert ref["taps"]["rect"][H // 2][~ref["inert"][H // 2]].min() >= 10
    # the prepared record alone, and one pass (scratch holds the prepared record then)
    _run(r, orc_det, planes, rects, px, f"{name}, no pass", iterations=0, **prm)
    _run(r, orc_det, planes, rects, px, f"{name}, one pass", iterations=1, **prm)


def test_optional_planes_and_the_ends_of_the_ranges(ptlib, orc_det):
    r, planes, prm = _case("terrain")
    rects, px = _frame()
    ref, _ = _run(r, orc_det, dict(planes, variance=None), rects, px, "no variance", iterations=2)
    assert ref["spatial"] == ref["filtered"]
    ref, _ = _run(r, orc_det, dict(planes, length=None), rects, px, "no length", iterations=2, frame=False)
    assert ref["spatial"] == 0
    ref, _ = _run(r, orc_det, planes, rects, px, "min_length 0", iterations=2, min_length=0)
    assert ref["spatial"] == 0
    ref, _ = _run(r, orc_det, dict(planes, variance=None, length=None), rects, px, "neither", iterations=1, normal_cos=-1.0, plane_eps=0.0, sigma_lum=0.5)
    assert ref["spatial"] == ref["filtered"]
    _run(r, orc_det, planes, rects, px, "the other ends", iterations=3, normal_cos=1.0, plane_eps=10.0, sigma_lum=100.0, min_length=65535)


# ------------------------------------------------------------------ 2. hand-made planes on small frames
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (9, 8), (63, 1), (65, 3)])
def test_synthetic_planes_on_small_frames(ptlib, orc_det, size):
    w, h = size
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), size, scenes.TWO_BOX_CAMERA)
    planes = F.synthetic_planes(w, h, 7 + w)
    rects, px = _frame(w, h)
    ref, _ = _run(r, orc_det, planes, rects, px, f"{w} x {h}", **F.SYNTHETIC_PARAMS)
    rej, cnt = F.tap_counts(ref)
    if w * h == 1:
        assert cnt == 0 and rej["rect"] == ref["filtered"] * 6 * (8 + 24) + ref["spatial"] * 48
    if w * h >= 64:
        assert all(rej[k] > 0 for k in ("rect", "inert", "mesh", "normal", "plane")) and cnt > 0, rej
    _run(r, orc_det, dict(planes, variance=None), rects, px, f"{w} x {h}, spatial everywhere", **F.SYNTHETIC_PARAMS)
    r.close()


# ------------------------------------------------------------------ 3. views
def test_views(ptlib, orc_det):
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), (W, H), scenes.TWO_BOX_CAMERA)
    views, _ = _views_and_prev()
    r.setViews(views)
    g = r.renderGBuffer(("hit", "position"))
    rng = np.random.default_rng(23)
    inside = np.zeros((H, W), bool)
    # colour, variance and length everywhere, also between the views, and a different colour range per view: a tap taken across a border
    # would change the answer
    color, var, length = F.random_planes(rng, H, W)
    for k, (x, y, w, h) in enumerate(RECTS):
        inside[y:y + h, x:x + w] = True
        color[y:y + h, x:x + w, :3] += f32(2.0 * k)
    color[~inside, :3] += f32(50.0)
    hit, pos = _np(g["hit"]).copy(), _np(g["position"]).copy()
    # the G-buffer leaves the pixels between the views alone: make them one surface with its neighbours in every view, so that only the
    # rectangle keeps their taps out
    hit[~inside] = hit[inside][np.argmax(hit.view(np.int32)[inside][:, 3] >= 0)]
    planes = dict(color=color, hit=hit, position=pos, variance=var, length=length)
    ref, st = _run(r, orc_det, planes, RECTS, inside, "four views", iterations=5, normal_cos=-1.0, plane_eps=1e3)
    assert st["pixels"] == sum(w * h for _, _, w, h in RECTS) and ref["taps"]["rect"].sum() > 0
    out = ref["out"].view(f32)
    for k, (x, y, w, h) in enumerate(RECTS):  # no bleed: every filtered colour stays in its own view's range
        v = out[y:y + h, x:x + w, :3][~ref["inert"][y:y + h, x:x + w]]
        assert len(v) and (v >= 2.0 * k - 1e-5).all() and (v < 2.0 * k + 1 + 1e-5).all()
        own = {n: np.ascontiguousarray(a[y:y + h, x:x + w]) for n, a in planes.items()}
        alone = F.filter_ref(orc_det, own, *_frame(w, h), iterations=5, normal_cos=-1.0, plane_eps=1e3)
        assert np.array_equal(F.canon(ref["out"][y:y + h, x:x + w]), F.canon(alone["out"]))
    # back to the single camera: the whole frame, one rectangle, and now the taps do cross
    r.setViews([])
    rects, px = _frame()
    whole, _ = _run(r, orc_det, planes, rects, px, "views dropped", iterations=5, normal_cos=-1.0, plane_eps=1e3)
    assert not np.array_equal(whole["out"][inside], ref["out"][inside])
    r.close()


# ------------------------------------------------------------------ 4. masks and partition
def test_masks(ptlib, orc_det):
    r, planes, prm = _case("two_box")
    nby, nbx = r.blockGrid()
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.4
    mask[0, 0] = mask[nby - 1, nbx - 1] = mask[0, nbx - 1] = mask[nby - 1, 3] = True  # corner and edge blocks, the 3-wide column and the 5-high row
    mask[1, 1] = False
    px = pixel_mask(mask, h=H, w=W)
    ref, st = _run(r, orc_det, planes, [(0, 0, W, H)], px, "a random block mask", mask=mask, blocks=mask, **prm)
    assert 0 < st["pixels"] < W * H and ref["taps"]["block"].sum() > 0 and (ref["out"][~px] == SENTINEL).all()
    _run(r, orc_det, planes, [(0, 0, W, H)], px, "the mask, two passes", mask=mask, blocks=mask, iterations=2, **prm)
    none = np.zeros((nby, nbx), bool)
    _, st = _run(r, orc_det, planes, [(0, 0, W, H)], np.zeros((H, W), bool), "the empty mask", mask=none, blocks=none, **prm)
    assert st == dict(pixels=0, filtered=0, spatial=0, kernel_ms=st["kernel_ms"])


def test_partition(ptlib, orc_det):
    _, planes, prm = _case("two_box")
    make, size, cam, _, _ = F.real_inputs()["two_box"]
    by, bx = np.mgrid[0:H, 0:W] // 8
    written = np.zeros((H, W), int)
    for rank in range(3):
        r = _renderer(make(), size, cam, partition=(rank, 3, 8, 8))
        own = (bx + by) % 3 == rank
        ref, st = _run(r, orc_det, planes, [(0, 0, W, H)], own, f"rank {rank}", blocks=F.block_set_of(own), **prm)
        assert st["pixels"] == int(own.sum()) and ref["taps"]["block"].sum() > 0
        written += ref["frame_rgba8"] != SENTINEL
        r.close()
    assert (written == 1).all()  # the union is the frame, overlaps are empty


# ------------------------------------------------------------------ 5. alignment and the context's own buffers
def test_planes_four_byte_aligned_only(ptlib, orc_det):
    r, planes, prm = _case("terrain")
    rects, px = _frame()
    _run(r, orc_det, planes, rects, px, "planes one float into their allocations", offset=True, iterations=3, **prm)


def test_context_buffers_as_planes(ptlib, orc_det):
    _, planes, prm = _case("two_box")
    make, size, cam, _, _ = F.real_inputs()["two_box"]
    r = _renderer(make(), size, cam)
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.launchParams.samples_per_launch = 1
    r.render()
    r.denoise(iterations=1)  # allocates PT_BUF_DENOISED
    nby, nbx = r.blockGrid()
    mask = np.random.default_rng(9).random((nby, nbx)) < 0.5
    px = pixel_mask(mask, h=H, w=W)
    kinds = (R.PT_BUF_ACCUM, R.PT_BUF_FRAME, R.PT_BUF_COLOR, R.PT_BUF_NORMAL, R.PT_BUF_ALBEDO, R.PT_BUF_DENOISED)
    before = {k: r.download(k).view(np.uint32) for k in kinds}
    dev = {k: _upload(planes[k]) for k in ("hit", "position", "variance", "length")}
    scratch = _filled("scratch", H, W)
    res = r.filterPlanes(color=r.deviceBuffer(R.PT_BUF_COLOR), **dev, out=r.deviceBuffer(R.PT_BUF_DENOISED), scratch=scratch,
                         frame=r.deviceBuffer(R.PT_BUF_FRAME), mask=mask, iterations=4, **prm)
    ref = F.filter_ref(orc_det, dict(planes, color=before[R.PT_BUF_COLOR]), [(0, 0, W, H)], px, blocks=mask, iterations=4, **prm)
    assert res["out"] is None and res["frame_rgba8"] is None and res["scratch"] is scratch
    assert (res["stats"]["filtered"], res["stats"]["spatial"]) == (ref["filtered"], ref["spatial"]) and ref["filtered"] > 0
    after = {k: r.download(k).view(np.uint32) for k in kinds}
    den, fr = after[R.PT_BUF_DENOISED], after[R.PT_BUF_FRAME]
    assert np.array_equal(F.canon(den[px]), F.canon(ref["out"][px])) and np.array_equal(den[~px], before[R.PT_BUF_DENOISED][~px])
    assert np.array_equal(fr[px], ref["frame_rgba8"][px]) and np.array_equal(fr[~px], before[R.PT_BUF_FRAME][~px])
    assert (_bits(scratch)[~px] == SENTINEL).all()
    for k in (R.PT_BUF_ACCUM, R.PT_BUF_COLOR, R.PT_BUF_NORMAL, R.PT_BUF_ALBEDO):
        assert np.array_equal(after[k], before[k])
    r.close()


# ------------------------------------------------------------------ 6. the chain end to end
def test_chain_end_to_end(ptlib, orc_det):
    """Two-box, 64 x 48, static camera, 8 frames of 1 spp: G-buffer -> temporal -> moments -> temporal -> filter on the GPU against the same
    chain in NumPy (temporal_ref, filter_ref) fed with the GPU's per-frame colours, bit for bit.  Then the point of the whole chain: the
    filtered image is nearer to a 256-spp render of the same frame than history_out is (RMS over the three colour words).  With the CPU
    checker's frames and the NumPy chain alone tests/test_filter_cabi.py finds 0.0727 (history_out) against 0.0193 (filtered), default
    parameters; no ratio is asserted, only the inequality."""
    w, h = F.CHAIN["size"]
    frames = F.CHAIN["frames"]
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), (w, h), scenes.TWO_BOX_CAMERA)
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    g = r.renderGBuffer(("hit", "position"))
    hit, pos = g["hit"], g["position"]
    dev = "cuda:0"
    motion = torch.zeros((h, w, 2), device=dev)
    hist = [torch.zeros((h, w, 4), device=dev) for _ in range(2)]
    mom = [torch.zeros((h, w, 4), device=dev) for _ in range(2)]
    ln = [torch.zeros((h, w), device=dev) for _ in range(2)]
    ln_m = torch.zeros((h, w), device=dev)
    zeros = np.zeros((h, w, 4), f32)
    colours = []
    r.launchParams.samples_per_launch = F.CHAIN["spp"]
    for k in range(frames):
        # this frame's colour: subframe k over a zeroed accumulation (the header's recipe: color_scale = k + 1)
        r.uploadAccum(zeros)
        r.launchParams.frame.subframe_index = k
        r.render()
        colours.append(r.download(R.PT_BUF_ACCUM))
        c = torch.from_numpy(colours[-1]).to(dev)
        i, o = k & 1, ~k & 1
        r.temporalAccumulate(c, motion, hit, pos, hit, pos, hist[i], ln[i], history_out=hist[o], length_out=ln[o], color_scale=float(k + 1))
        # the moments plane (lum, lum^2, 0, 1) of the same colour, one torch operation per rounding
        s = c[..., :3] * float(k + 1)
        lum = (0.2126 * s[..., 0] + 0.7152 * s[..., 1]) + 0.0722 * s[..., 2]
        m = torch.stack([lum, lum * lum, torch.zeros_like(lum), torch.ones_like(lum)], -1).contiguous()
        assert np.array_equal(_bits(m), F.moments_plane(colours[-1], k + 1).view(np.uint32))
        r.temporalAccumulate(m, motion, hit, pos, hit, pos, mom[i], ln[i], history_out=mom[o], length_out=ln_m)
    last = frames & 1
    m1, m2 = mom[last][..., 0], mom[last][..., 1]
    var = torch.clamp_min(m2 - m1 * m1, 0.0).contiguous()
    res = r.filterPlanes(hist[last], hit, pos, variance=var, length=ln[last])
    want_hist, ref, want_var, want_ln = F.chain_ref(orc_det, colours, _np(hit), _np(pos))
    assert np.array_equal(_bits(hist[last]), want_hist.view(np.uint32)) and np.array_equal(_np(ln[last]), want_ln) and np.array_equal(_np(ln_m), want_ln)
    assert np.array_equal(_bits(var), want_var.view(np.uint32))
    _same(_bits(res["out"]), None, None, ref, np.ones((h, w), bool), "the chain")
    assert (res["stats"]["filtered"], res["stats"]["spatial"]) == (ref["filtered"], ref["spatial"])
    # the 256-spp frame
    r.uploadAccum(zeros)
    r.launchParams.samples_per_launch = F.CHAIN["reference_spp"]
    r.launchParams.frame.subframe_index = 0
    r.render()
    reference = r.download(R.PT_BUF_ACCUM)
    plain, filtered = F.rms(_np(hist[last]), reference), F.rms(_np(res["out"]), reference)
    print(f"chain: rms of history_out {plain:.5f}, filtered {filtered:.5f}")
    assert filtered < plain
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
            _run(r, orc_det, planes, rects, px, "between the frames", iterations=2, **prm)
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
        assert x.tobytes() == y.tobytes(), f"buffer {k} differs after a filterPlanes between the frames"


# ------------------------------------------------------------------ 8. refusals
def test_refusals(ptlib, orc_det):
    _, planes, prm = _case("two_box")
    L = _lib.load_library()
    r = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    dev = {k: _upload(planes[k]) for k in FILTER_INPUTS}
    out = {k: _filled(k, H, W) for k in _lib.FILTER_OUTPUTS}
    ptr = {k: t.data_ptr() for k, t in list(dev.items()) + list(out.items())}
    good = dict(ptr, iterations=5, sigma_lum=4.0, normal_cos=0.9, plane_eps=0.01, min_length=4, flags=0)

    def refused(what, pattern, **fields):
        d = _lib.FilterDesc()
        for k, v in dict(good, **fields).items():
            setattr(d, k, v)
        torch.cuda.synchronize()
        s = _lib.FilterStats(7, 7, 7, 7.0)
        rc = L.pt_filter_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_filter_planes") and pattern in msg, f"{what}: {msg!r}"
        assert (s.pixels, s.filtered, s.spatial, s.kernel_ms) == (7, 7, 7, 7.0)
        for k, t in out.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {k} was written"

    refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, W / H))
    assert L.pt_filter_planes(r._ctx, None, None) == -1 and "null description" in L.pt_last_error(r._ctx).decode()
    for name in ("color", "hit", "position", "out", "scratch"):
        refused(f"{name} null", f"{name} is null", **{name: None})
    refused("scratch null with one pass", "scratch is null", scratch=None, iterations=1)
    host = np.zeros((H, W, 4), f32)
    refused("a host pointer", "color is not device memory", color=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "position is not 4-byte aligned", position=ptr["position"] + 2)
    refused("an optional plane offset by 1 byte", "variance is not 4-byte aligned", variance=ptr["variance"] + 1)
    refused("an optional output offset by 1 byte", "frame_rgba8 is not 4-byte aligned", frame_rgba8=ptr["frame_rgba8"] + 1)
    # one element too small for what is left of its allocation (an allocation of the runtime's own: torch's allocator hands out parts of larger ones)
    hip = _hip_runtime()
    raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(raw), C.c_size_t(H * W * 4)) == 0
    try:
        assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= H * W * 4
        refused("a plane one element too small", f"length has fewer than {H * W * 4} bytes left", length=raw.value + size.value - (H * W * 4 - 4))
    finally:
        assert hip.hipFree(raw) == 0
    # forbidden overlaps: a written plane against anything; the read-only planes may alias
    refused("in place", "color and out overlap", out=ptr["color"])
    refused("scratch on the output", "out and scratch overlap", scratch=ptr["out"])
    refused("scratch on a guide", "position and scratch overlap", scratch=ptr["position"])
    refused("the frame inside the output", "out and frame_rgba8 overlap", frame_rgba8=ptr["out"] + 4 * (H * W * 3))
    refused("the frame on the variance", "variance and frame_rgba8 overlap", frame_rgba8=ptr["variance"])
    refused("the output on the lengths", "length and out overlap", length=ptr["out"])
    refused("a flag", "unknown flag bits 1", flags=1)
    for name, bad, pattern in (("iterations", (-1, 7), "iterations must be in [0,6]"),
                               ("sigma_lum", (0.0, -1.0, np.inf, np.nan), "sigma_lum must be finite and > 0"),
                               ("normal_cos", (1.5, -1.5, np.nan), "normal_cos must be in [-1,1]"),
                               ("plane_eps", (-1.0, np.inf, np.nan), "plane_eps must be finite and >= 0"),
                               ("min_length", (65536,), "min_length must be in [0,65535]")):
        for v in bad:
            refused(f"{name} = {v}", pattern, **{name: v})
    # the Python facade checks dtype, shape and device before the library is called
    args = dict(dev, out=out["out"], scratch=out["scratch"], frame=out["frame_rgba8"])
    with pytest.raises(ValueError, match="variance.*shape"):
        r.filterPlanes(**dict(args, variance=dev["position"]))
    with pytest.raises(ValueError, match="the tensor is on cpu"):
        r.filterPlanes(**dict(args, hit=torch.zeros((H, W, 8))))
    with pytest.raises(RuntimeError, match="out and scratch overlap"):
        r.filterPlanes(**dict(args, scratch=out["out"]))
    # a valid call afterwards still works, into the same planes; read-only planes may alias (variance == length); without a pass scratch may be null
    rects, px = _frame()
    res = r.filterPlanes(**dict(args, variance=dev["length"]), iterations=6, **prm)
    ref = F.filter_ref(orc_det, dict(planes, variance=planes["length"]), rects, px, iterations=6, **prm)
    _same(_bits(out["out"]), _bits(out["frame_rgba8"]), _bits(out["scratch"]), ref, px, "a valid call after the refusals")
    assert res["stats"]["filtered"] == ref["filtered"]
    # ... and so does one that lets the facade allocate its outputs (zero-filled), without a pass and without scratch
    res = r.filterPlanes(dev["color"], dev["hit"], dev["position"], dev["variance"], dev["length"], iterations=0, **prm)
    ref = F.filter_ref(orc_det, planes, rects, px, iterations=0, fill=0, **prm)
    assert res["scratch"] is None
    _same(_bits(res["out"]), None, None, ref, px, "allocated outputs")
    r.close()
