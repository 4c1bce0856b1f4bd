"""Guided upsampling (pt_upsample_planes) on the GPU.  `out` and `weight_out` are compared bit for bit, over the WHOLE plane against the
sentinel fill (so a pixel written outside the chosen set shows as a lost sentinel), and all five counters exactly, with
tests/upsample_ref.py: float32 NumPy evaluating the header's arithmetic.  No tolerance anywhere.

Real-plane inputs: the low-resolution and the full-resolution hit and position planes come from renderGBuffer of two contexts over one model
(pinned by tests/test_gpu_gbuffer.py); the colour is tests/filter_ref.random_planes, with its NaN and inf words.

The views of this file are (0, 0, 60, 36) and (96, 0, 36, 48) in the 132 x 60 frame, not the (72, 12, 60, 48) one could wish for: pt_set_views
takes x and y in multiples of 8 only, and the low-resolution context, which carries the views divided by the scale, needs x / s and y / s in
multiples of 8 as well, so x and y are multiples of 96 for s = 2, 3, 4.  Widths and heights are multiples of 12 and off the 8-grid."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import filter_ref as F
import upsample_ref as U
from conftest import ROOT
from gpu_kit import filled, pixel_mask, plane_shape, whole_frame
from gpu_kit import bits as _bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import upload as _upload
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from pass_cases import _UPSAMPLE as _CASES
from pass_cases import _hit_and_position as _gbuffer
from pass_cases import _upsample_model as _model
from pass_cases import upsample_case as _case

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 132, 60
SCALES = (2, 3, 4)
SENTINEL = U.SENTINEL
WORDS = _lib.UPSAMPLE_PLANES
VIEWS = ((0, 0, 60, 36), (96, 0, 36, 48))


# ------------------------------------------------------------------ GPU helpers
def _filled(name, h, w, offset=False):
    """a sentinel-filled plane of the pass; offset: one float into its allocation (4-byte aligned only)"""
    return filled(plane_shape(h, w, WORDS[name]), offset)


def _run(r, lo, hi, s, rects, pixels, what, mask=None, offset=False, weight=True, **prm):
    """uploads the planes, calls upsamplePlanes into sentinel-filled outputs and compares both outputs over the whole frame and the five
    counters with the NumPy reference; returns (reference, stats)"""
    h, w = hi["hit"].shape[:2]
    dev = dict(lo_color=_upload(lo["color"], offset), lo_hit=_upload(lo["hit"], offset), lo_position=_upload(lo["position"], offset),
               hit=_upload(hi["hit"], offset), position=_upload(hi["position"], offset))
    out = _filled("out", h, w, offset)
    wgt = _filled("weight_out", h, w, offset) if weight else None
    res = r.upsamplePlanes(**dev, scale=s, out=out, weight_out=wgt, mask=mask, **prm)
    assert res["out"] is out and res["weight_out"] is wgt
    ref = U.upsample_ref(lo, hi, s, rects, pixels, **prm)
    got = _bits(out)
    assert got.shape == ref["out"].shape and np.array_equal(got, ref["out"]), f"{what}: out differs from float32 NumPy in {int((got != ref['out']).sum())} words"
    if weight:
        got = _bits(wgt)
        assert np.array_equal(got, ref["weight_out"]), f"{what}: weight_out differs in {int((got != ref['weight_out']).sum())} pixels"
    st = res["stats"]
    assert tuple(st[k] for k in ("pixels", "hits", "full", "rescued", "orphans")) == U.counters(ref), (what, st, U.counters(ref))
    assert st["kernel_ms"] > 0 if st["pixels"] else st["kernel_ms"] >= 0
    return ref, st


def _frame(w=W, h=H):
    return whole_frame(w, h)


# ------------------------------------------------------------------ 1. real planes
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_real_planes(ptlib, name, s):
    r, lo, hi = _case(name, s)
    ref, st = _run(r, lo, hi, s, *_frame(), f"{name} at scale {s}")
    rej = {k: int(v.sum()) for k, v in ref["taps"].items()}
    print(f"{name} scale {s}: full {st['full']} rescued {st['rescued']} orphans {st['orphans']} of {st['pixels']}, rejected {rej}, kernel_ms {st['kernel_ms']:.4f}")
    assert np.isnan(lo["color"]).any() and np.isinf(lo["color"]).any() and rej["colour"] > 0 and rej["rect"] > 0 and rej["kind"] > 0 and rej["mesh"] > 0
    assert 0 < st["hits"] < st["pixels"] and st["full"] > 0
    if name == "terrain":  # the facets are smaller than a low-res pixel: the rescue and the orphan branch on real planes
        assert rej["normal"] > 0 and rej["plane"] > 0 and st["rescued"] > 0 and st["orphans"] > 0


def test_the_ends_of_the_ranges_and_no_weight_plane(ptlib):
    r, lo, hi = _case("terrain", 2)
    rects, px = _frame()
    _run(r, lo, hi, 2, rects, px, "weight_out = NULL", weight=False)
    ref, _ = _run(r, lo, hi, 2, rects, px, "the loose ends", normal_cos=-1.0, plane_eps=1e3)
    assert ref["taps"]["normal"].sum() == 0 and ref["taps"]["plane"].sum() == 0
    ref, _ = _run(r, lo, hi, 2, rects, px, "the tight ends", normal_cos=1.0, plane_eps=0.0)
    assert ref["orphans"] > 0
    _run(r, lo, hi, 2, rects, px, "planes one float into their allocations", offset=True)


# ------------------------------------------------------------------ 2. views
@pytest.mark.parametrize("s", SCALES)
def test_views(ptlib, s):
    """two views with different cameras; the low-resolution context carries the views divided by the scale"""
    model = scenes.two_box_scene(shadow_catcher=False)
    cams = (scenes.TWO_BOX_CAMERA, dict(scenes.TWO_BOX_CAMERA, eye=(-2.5, 2.0, -4.5)))
    hi_r, lo_r = _renderer(model, (W, H), cams[0]), _renderer(model, (W // s, H // s), cams[0])
    hi_r.setViews([(x, y, w, h, R.make_camera(cd, w / h)) for (x, y, w, h), cd in zip(VIEWS, cams)])
    lo_r.setViews([(x // s, y // s, w // s, h // s, R.make_camera(cd, w / h)) for (x, y, w, h), cd in zip(VIEWS, cams)])
    hi, lo = _gbuffer(hi_r), _gbuffer(lo_r)
    lo_r.close()
    inside, lo_inside = np.zeros((H, W), bool), np.zeros((H // s, W // s), bool)
    color = F.random_planes(np.random.default_rng(60 + s), H // s, W // s)[0]
    for k, (x, y, w, h) in enumerate(VIEWS):  # a different colour range per view, and a third between them: a tap taken across a border would show
        inside[y:y + h, x:x + w] = True
        lo_inside[y // s:(y + h) // s, x // s:(x + w) // s] = True
        color[y // s:(y + h) // s, x // s:(x + w) // s, :3] += f32(2.0 * k)
    color[~lo_inside, :3] += f32(50.0)
    # the G-buffers leave the pixels between the views alone: make them one surface with a hit pixel of the first view
    for planes, where in ((hi, inside), (lo, lo_inside)):
        ys, xs = np.nonzero(where & (planes["hit"].view(np.int32)[..., 3] >= 0))
        planes["hit"][~where], planes["position"][~where] = planes["hit"][ys[0], xs[0]], planes["position"][ys[0], xs[0]]
    lo["color"] = color
    ref, st = _run(hi_r, lo, hi, s, VIEWS, inside, f"two views at scale {s}", normal_cos=-1.0, plane_eps=1e3)
    assert st["pixels"] == sum(w * h for _, _, w, h in VIEWS) and ref["taps"]["rect"].sum() > 0 and (ref["out"][~inside] == SENTINEL).all()
    out = ref["out"].view(f32)
    for k, (x, y, w, h) in enumerate(VIEWS):  # no bleed: every finite colour stays in its own view's range
        v = out[y:y + h, x:x + w, :3]
        v = v[np.isfinite(v)]
        assert len(v) and (v >= 2.0 * k - 1e-5).all() and (v < 2.0 * k + 1 + 1e-5).all()
    # a view that is not a multiple of the scale is refused, and names the view
    bad = [(0, 0, 60, 36), (96, 0, 36 - 1, 48)] if s != 3 else [(0, 0, 60, 36), (8, 40, 36, 12)]
    hi_r.setViews([(x, y, w, h, R.make_camera(cams[0], w / h)) for x, y, w, h in bad])
    dev = dict(lo_color=_upload(lo["color"]), lo_hit=_upload(lo["hit"]), lo_position=_upload(lo["position"]), hit=_upload(hi["hit"]), position=_upload(hi["position"]))
    out_t = _filled("out", H, W)
    with pytest.raises(RuntimeError, match=rf"pt_upsample_planes: view 1 \(x {bad[1][0]}, y {bad[1][1]}, {bad[1][2]} x {bad[1][3]}\) is not a multiple of scale {s}"):
        hi_r.upsamplePlanes(**dev, scale=s, out=out_t)
    assert (_bits(out_t) == SENTINEL).all()
    hi_r.close()


# ------------------------------------------------------------------ 3. masks and partition
def test_block_mask(ptlib):
    r, lo, hi = _case("two_box", 3)
    nby, nbx = r.blockGrid()
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.4
    mask[0, 0] = mask[nby - 1, nbx - 1] = mask[0, nbx - 1] = mask[nby - 1, 3] = True  # corner and edge blocks, the 4-wide column and the 4-high row
    mask[1, 1] = False
    px = pixel_mask(mask, h=H, w=W)
    ref, st = _run(r, lo, hi, 3, [(0, 0, W, H)], px, "a random block mask", mask=mask)
    assert 0 < st["pixels"] < W * H and (ref["out"][~px] == SENTINEL).all()
    # the low-res plane has no block set: a masked pixel gets what it gets in the whole frame
    whole = U.upsample_ref(lo, hi, 3, *_frame())
    assert np.array_equal(ref["out"][px], whole["out"][px])
    none = np.zeros((nby, nbx), bool)
    _, st = _run(r, lo, hi, 3, [(0, 0, W, H)], np.zeros((H, W), bool), "the empty mask", mask=none)
    assert st == dict(pixels=0, hits=0, full=0, rescued=0, orphans=0, kernel_ms=st["kernel_ms"])


def test_rank_one_of_three(ptlib):
    _, lo, hi = _case("terrain", 4)
    make, cam = _model("terrain")
    by, bx = np.mgrid[0:H, 0:W] // 8
    own = (bx + by) % 3 == 1
    r = _renderer(_CASES["terrain"][0], (W, H), cam, partition=(1, 3, 8, 8))
    ref, st = _run(r, lo, hi, 4, [(0, 0, W, H)], own, "rank 1 of 3")
    assert st["pixels"] == int(own.sum()) and (ref["weight_out"][~own] == SENTINEL).all()
    r.close()


# ------------------------------------------------------------------ 4. small frames and the hand-made planes
@pytest.mark.parametrize("size,s", [((8, 8), 2), ((8, 8), 4), ((12, 18), 3), ((2, 2), 2), ((3, 3), 3), ((4, 4), 4)])
def test_small_frames(ptlib, size, s):
    """one block, a frame off the 8-grid, and s x s over a single low-res pixel (every tap but one leaves the rectangle)"""
    w, h = size
    model = scenes.two_box_scene(shadow_catcher=False)
    hi_r, lo_r = _renderer(model, size, scenes.TWO_BOX_CAMERA), _renderer(model, (w // s, h // s), scenes.TWO_BOX_CAMERA)
    hi, lo = _gbuffer(hi_r), _gbuffer(lo_r)
    lo_r.close()
    lo["color"] = np.random.default_rng(70 + w).random((h // s, w // s, 4), dtype=f32)
    ref, st = _run(hi_r, lo, hi, s, *_frame(w, h), f"{w} x {h} at scale {s}", normal_cos=-1.0, plane_eps=1e3)
    assert st["pixels"] == w * h and ref["taps"]["rect"].sum() > 0
    if w == s:
        assert ref["full"] == 0 and int(ref["counted"].max()) <= 1
    hi_r.close()


@pytest.mark.parametrize("s", SCALES)
def test_synthetic_planes(ptlib, s):
    d = U.synthetic_planes(s)
    w, h = d["size"]
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), (w, h), scenes.TWO_BOX_CAMERA)
    r.setViews([(x, y, rw, rh, R.make_camera(scenes.TWO_BOX_CAMERA, rw / rh)) for x, y, rw, rh in d["rects"]])
    ref, st = _run(r, d["lo"], d["hi"], s, d["rects"], np.ones((h, w), bool), f"hand-made planes at scale {s}", **d["params"])
    for name, (X, Y, branch, _) in d["known"].items():
        assert ref["branch"][Y, X] == branch, name
    assert st["rescued"] >= 1 and st["orphans"] == 2
    r.close()


# ------------------------------------------------------------------ 5. refusals
def test_refusals(ptlib):
    _, lo, hi = _case("two_box", 2)
    L = _lib.load_library()
    r = R.SampleRenderer(_CASES["two_box"][0])
    lw, lh = W // 2, H // 2
    dev = dict(lo_color=_upload(lo["color"]), lo_hit=_upload(lo["hit"]), lo_position=_upload(lo["position"]), hit=_upload(hi["hit"]), position=_upload(hi["position"]))
    out = {k: _filled(k, H, W) for k in _lib.UPSAMPLE_OUTPUTS}
    ptr = {k: t.data_ptr() for k, t in list(dev.items()) + list(out.items())}
    good = dict(ptr, lo_width=lw, lo_height=lh, scale=2, normal_cos=0.9, plane_eps=0.01, flags=0)

    def refused(what, pattern, **fields):
        d = _lib.UpsampleDesc()
        for k, v in dict(good, **fields).items():
            setattr(d, k, v)
        torch.cuda.synchronize()
        s = _lib.UpsampleStats(7, 7, 7, 7, 7, 7.0)
        rc = L.pt_upsample_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_upsample_planes") and pattern in msg, f"{what}: {msg!r}"
        assert (s.pixels, s.hits, s.full, s.rescued, s.orphans, s.kernel_ms) == (7, 7, 7, 7, 7, 7.0)
        for k, t in out.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {k} was written"

    refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, W / H))
    assert L.pt_upsample_planes(r._ctx, None, None) == -1 and "null description" in L.pt_last_error(r._ctx).decode()
    for name in ("lo_color", "lo_hit", "lo_position", "hit", "position", "out"):
        refused(f"{name} null", f"{name} is null", **{name: None})
    host = np.zeros((H, W, 4), f32)
    refused("a host pointer", "position is not device memory", position=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "lo_position is not 4-byte aligned", lo_position=ptr["lo_position"] + 2)
    refused("an optional output offset by 1 byte", "weight_out is not 4-byte aligned", weight_out=ptr["weight_out"] + 1)
    # one element too small for what is left of its allocation (an allocation of the runtime's own), at the LOW resolution's size
    hip = _hip_runtime()
    raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(raw), C.c_size_t(lh * lw * 16)) == 0
    try:
        assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= lh * lw * 16
        refused("a low-res plane one element too small", f"lo_color has fewer than {lh * lw * 16} bytes left", lo_color=raw.value + size.value - (lh * lw * 16 - 4))
    finally:
        assert hip.hipFree(raw) == 0
    # forbidden overlaps: a written plane against anything; the read-only planes may alias
    both = torch.full((H * W * 4 + lh * lw * 4,), 0.5, dtype=torch.float32, device="cuda:0")  # the low-res colour with the output starting inside it
    refused("the output inside the low-res colour", "lo_color and out overlap", lo_color=both.data_ptr() + 4 * (lh * lw * 2), out=both.data_ptr() + 4 * (lh * lw * 4))
    assert (both == 0.5).all()
    refused("out inside the guide", "hit and out overlap", out=ptr["hit"])
    refused("the weights inside the output", "out and weight_out overlap", weight_out=ptr["out"] + 4 * (H * W * 3))
    refused("the weights on the low-res guide", "lo_hit and weight_out overlap", weight_out=ptr["lo_hit"])
    refused("a flag", "unknown flag bits 1", flags=1)
    for v in (0, 1, 5, 2**31):
        refused(f"scale = {v}", "scale must be in [2,4]", scale=v)
    refused("a low-res size that does not match", f"the low-resolution size {lw - 1} x {lh} times scale 2 is not the frame's {W} x {H}", lo_width=lw - 1)
    refused("a low-res height that does not match", f"the low-resolution size {lw} x {lh + 1} times scale 2 is not the frame's {W} x {H}", lo_height=lh + 1)
    refused("the other scale's size", f"the low-resolution size {lw} x {lh} times scale 3 is not the frame's {W} x {H}", scale=3)
    for name, bad, pattern in (("normal_cos", (1.5, -1.5, np.nan), "normal_cos must be in [-1,1]"),
                               ("plane_eps", (-1.0, np.inf, np.nan), "plane_eps must be finite and >= 0")):
        for v in bad:
            refused(f"{name} = {v}", pattern, **{name: v})
    # the Python facade checks dtype, shape and device before the library is called
    args = dict(dev, scale=2, out=out["out"], weight_out=out["weight_out"])
    with pytest.raises(ValueError, match="lo_hit.*shape"):
        r.upsamplePlanes(**dict(args, lo_hit=dev["hit"]))
    with pytest.raises(ValueError, match="the tensor is on cpu"):
        r.upsamplePlanes(**dict(args, hit=torch.zeros((H, W, 8))))
    with pytest.raises(RuntimeError, match="out and weight_out overlap"):
        r.upsamplePlanes(**dict(args, weight_out=out["out"].view(-1)[: H * W].view(H, W)))
    # a valid call afterwards still works, into the same planes; read-only planes may alias (lo_position == lo_color); out is allocated when None
    rects, px = _frame()
    res = r.upsamplePlanes(**dict(args, lo_position=dev["lo_color"]))
    ref = U.upsample_ref(dict(lo, position=lo["color"]), hi, 2, rects, px)
    assert np.array_equal(_bits(out["out"]), ref["out"]) and np.array_equal(_bits(out["weight_out"]), ref["weight_out"]) and res["stats"]["orphans"] == ref["orphans"]
    res = r.upsamplePlanes(dev["lo_color"], dev["lo_hit"], dev["lo_position"], dev["hit"], dev["position"], 2)
    ref = U.upsample_ref(lo, hi, 2, rects, px)
    assert res["weight_out"] is None and np.array_equal(_bits(res["out"]), ref["out"])
    r.close()


# ------------------------------------------------------------------ 6. the rendering state is left alone
def test_rendering_state_is_left_alone(ptlib):
    _, lo, hi = _case("two_box", 2)
    probe = scenes.sky_probe(256, 128).BuildCDF()
    rects, px = _frame()

    def run(with_call):
        r = R.SampleRenderer(_CASES["two_box"][0])
        r.setProbe(probe)
        r.resize((W, H))
        r.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, W / H))
        r.launchParams.samples_per_launch = 2
        for k in (0, 1):
            r.launchParams.frame.subframe_index = k
            r.render()
        if with_call:
            before = r.stats()
            _run(r, lo, hi, 2, rects, px, "between the frames")
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
        assert x.tobytes() == y.tobytes(), f"buffer {k} differs after an upsamplePlanes between the frames"


# ------------------------------------------------------------------ 7. the loop
def test_example_loop_runs_to_its_end(ptlib, tmp_path, capsys):
    """examples/upsampled_svgf_loop.py --scale 2, three frames at 128 x 64, in this process: every frame reports its orphans, the counters
    add up, and the final frame is written and finite"""
    spec = importlib.util.spec_from_file_location("upsampled_svgf_loop", os.path.join(ROOT, "examples", "upsampled_svgf_loop.py"))
    loop = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(loop)
    assert loop.main(["--scale", "2", "--size", "128", "64", "--frames", "3", "--lod", "--out-dir", str(tmp_path)]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("frame ")]
    assert len(lines) == 3 and all(" orphans " in l and f"of {128 * 64} pixels full " in l for l in lines)
    final = np.load(tmp_path / "upsampled_svgf_final.npy")
    assert final.shape == (64, 128, 4) and np.isfinite(final[..., :3]).all() and final[..., :3].max() > 0
