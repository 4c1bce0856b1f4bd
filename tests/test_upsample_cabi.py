"""Guided upsampling (pt_upsample_planes) without a GPU: the entry point is declared and exported, the ctypes mirrors of pt_upsample_desc and
pt_upsample_stats match the compiler's layout, the header compiles as C99 and as C++17, a null context and a null description are refused
before any device work, both facades have the method and the Python one checks its arguments before the library is called; the header's
per-axis index and weight table is the pixel-centre mapping (a + 0.5) / s - 0.5; the hand-made planes of tests/upsample_ref.py put every
branch and every rejection reason on its known pixel; and on CPU-built G-buffer planes the rule does what it is for: an analytic irradiance,
sampled on the low-resolution planes and upsampled, is much nearer to the same function on the full-resolution planes than plain bilinear
interpolation is."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import temporal_ref as T
import upsample_ref as U
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_text
from conftest import ROOT
from optixpathtracer_amd import _lib

f32 = np.float32
DESC_FIELDS = ("lo_color", "lo_hit", "lo_position", "hit", "position", "out", "weight_out", "block_mask", "lo_width", "lo_height", "scale",
               "normal_cos", "plane_eps", "flags")
STATS_FIELDS = ("pixels", "hits", "full", "rescued", "orphans", "kernel_ms")
SCALES = (2, 3, 4)


def test_library_exports_the_entry_point():
    L = _lib.load_library()
    assert "pt_upsample_planes" in _lib.EXPORTS and hasattr(L, "pt_upsample_planes")
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int\s+pt_upsample_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_upsample_desc\s*\*\s*\w+\s*,\s*pt_upsample_stats\s*\*", src)
    assert re.search(r"PT_UPSAMPLE_RESERVED\s*=\s*0\b", src)
    assert L.pt_version().startswith(b"ptamd 0.4")
    assert "pt_upsample_planes" in header().split("VERSIONING.")[1].split("*/")[0]  # the note names it among the entry points added at 0.4
    assert "pt_upsample_planes" in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    lib = open(os.path.join(ROOT, "optixpathtracer_amd", "csrc", "pt_lib.hip")).read()
    assert '#include "pt_upsample.hip"' in lib


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.UpsampleDesc, "pt_upsample_desc", DESC_FIELDS), (_lib.UpsampleStats, "pt_upsample_stats", STATS_FIELDS)],
                 [88] + [8 * k for k in range(8)] + [64, 68, 72, 76, 80, 84] + [48, 0, 8, 16, 24, 32, 40])
    assert set(_lib.UPSAMPLE_PLANES) == set(DESC_FIELDS[:7]) and _lib.UPSAMPLE_OUTPUTS == ("out", "weight_out")


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const float* lo, const void* hit, float* out) {\n"
            "    pt_upsample_desc d = {0, 0, 0, 0, 0, 0, 0, 0, 960u, 540u, 2u, 0.9f, 0.01f, 0u};\n"
            "    pt_upsample_stats s;\n"
            "    d.lo_color = lo; d.hit = hit; d.out = out; d.flags = PT_UPSAMPLE_RESERVED;\n"
            "    return pt_upsample_planes(c, &d, &s);\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_context_and_null_description_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.UpsampleDesc(), _lib.UpsampleStats(7, 7, 7, 7, 7, 7.0)
    assert L.pt_upsample_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_upsample_planes: null context" in L.pt_last_error(None)
    assert L.pt_upsample_planes(None, None, None) == -1
    assert (s.pixels, s.hits, s.full, s.rescued, s.orphans, s.kernel_ms) == (7, 7, 7, 7, 7, 7.0)
    # a null description and every range are refused before anything is enqueued (the text of pt_upsample.hip; a live context needs a GPU)
    body = open(os.path.join(ROOT, "optixpathtracer_amd", "csrc", "pt_upsample.hip")).read().split('extern "C" int pt_upsample_planes(')[1]
    assert body.index("null description") < body.index("ctx->width")
    for text in ("unknown flag bits", "scale must be in [2,4]", "is not the frame's", "normal_cos must be in [-1,1]", "plane_eps must be finite and >= 0",
                 "is not a multiple of scale", "pass_planes_check"):
        assert body.index(text) < body.index("run.open"), text


def test_python_facade_checks_its_arguments():
    import torch

    from optixpathtracer_amd import renderer as R

    assert callable(getattr(R.SampleRenderer, "upsamplePlanes", None))
    r = bare_renderer(size=(12, 8))
    ok = dict(lo_color=fake_cuda((4, 6, 4)), lo_hit=fake_cuda((4, 6, 8)), lo_position=fake_cuda((4, 6, 4)), hit=fake_cuda((8, 12, 8)),
              position=fake_cuda((8, 12, 4)), scale=2, out=1)
    for bad in (1, 5, 0):
        with pytest.raises(ValueError, match=r"upsamplePlanes: scale must be in \[2,4\]"):
            r.upsamplePlanes(**dict(ok, scale=bad))
    with pytest.raises(ValueError, match="upsamplePlanes: scale 3 does not divide the frame's 12 x 8"):
        r.upsamplePlanes(**dict(ok, scale=3))
    with pytest.raises(ValueError, match="upsamplePlanes: lo_hit is required"):
        r.upsamplePlanes(**dict(ok, lo_hit=None))
    with pytest.raises(TypeError, match="upsamplePlanes: lo_color: a torch tensor or a device pointer"):
        r.upsamplePlanes(**dict(ok, lo_color=np.zeros((4, 6, 4), f32)))
    with pytest.raises(ValueError, match="upsamplePlanes: position: the tensor is on cpu"):
        r.upsamplePlanes(**dict(ok, position=torch.zeros((8, 12, 4))))
    # the low-res planes are checked against the low-res shape, the others against the frame's
    with pytest.raises(ValueError, match=r"upsamplePlanes: lo_color: a contiguous torch.float32 tensor of shape \(4, 6, 4\) is expected"):
        r.upsamplePlanes(**dict(ok, lo_color=fake_cuda((8, 12, 4))))
    with pytest.raises(ValueError, match=r"upsamplePlanes: lo_color: a contiguous torch.float32 tensor of shape \(2, 3, 4\) is expected"):
        r.upsamplePlanes(**dict(ok, scale=4))
    with pytest.raises(ValueError, match=r"upsamplePlanes: hit: a contiguous torch.float32 tensor of shape \(8, 12, 8\) is expected"):
        r.upsamplePlanes(**dict(ok, hit=fake_cuda((4, 6, 8))))
    with pytest.raises(ValueError, match=r"upsamplePlanes: weight_out: a contiguous torch.float32 tensor of shape \(8, 12\) is expected"):
        r.upsamplePlanes(**ok, weight_out=fake_cuda((8, 12, 1)))
    with pytest.raises(ValueError, match="the mask needs"):
        r.blockGrid = lambda: (1, 2)
        r.upsamplePlanes(**ok, mask=np.ones((2, 2)))


def test_cxx_facade_compiles(tmp_path):
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t upsample(SampleRenderer& sample, pt_upsample_desc d) {\n"
        "    d.scale = 2;\n"
        "    pt_upsample_stats s{};\n"
        "    sample.upsamplePlanes(d, &s);\n"
        "    return sample.upsamplePlanes(d).orphans + s.rescued;\n"
        "}\n"
    )


def test_header_states_the_contract():
    text = header_text()
    for item in ("a = X - x0; r = a % s; cx = x0/s + a/s", "t = (float)(2*r + 1 - s) / (float)(2*s)", "If t < 0: i = cx - 1, fx = t + 1.0f. Else i = cx, fx = t",
                 "fabsf(dot3(ng_p, lo_position[q].xyz - position[p].xyz)) <= plane_eps * hit[p].t", "lo_hit[q].mesh == hit[p].mesh",
                 "hit[p].prim < 0 and lo_hit[q].prim < 0", "There is no block test on q", "in the order (0,0), (1,0), (0,1), (1,1)",
                 "wx = dx ? fx : 1.0f - fx", "A tap with w == 0 does not count", "out[p] = S / W per component, weight_out[p] = W",
                 "dy = -1..2 outer, dx = -1..2 inner", "out[p] = S / N, weight_out[p] = 0.0f", "out[p] = lo_color[(cx, cy)], the four words as they are",
                 "weight_out[p] = -1.0f", "must be multiples of scale", "No other pixel of out or weight_out is written",
                 "Zero pixels launch nothing and return PT_OK", "scale outside 2..4", "flags != 0"):
        assert item in text, item


# ------------------------------------------------------------------ the per-axis table
@pytest.mark.parametrize("s", SCALES)
def test_axis_table_is_the_pixel_centre_mapping(s):
    """The centre of full-res pixel a lies at (a + 0.5) / s - 0.5 in low-res pixel units: i is its floor, f its fraction.  The float64
    restatement uses no expression of the header.  With s = 2 and 4 every weight is a dyadic fraction and exact; with s = 3 the header's one
    float32 division and one addition stay within one float32 ulp of the float64 value."""
    for x0 in (0, 12, 24 * s):
        X = x0 + np.arange(0, 40 * s)
        c, i, f = U.axis(X, x0, s)
        at = ((X - x0).astype(np.float64) + 0.5) / s - 0.5
        fl = np.floor(at)
        assert f.dtype == f32 and np.array_equal(i, x0 // s + fl.astype(np.int64)) and np.array_equal(c, X // s)
        frac = at - fl
        if s == 3:
            assert (np.abs(f.astype(np.float64) - frac) <= np.spacing(frac.astype(f32)).astype(np.float64)).all()
            assert (f[(X - x0) % 3 == 1] == 0).all()  # the centre residue: the second tap's weight is exactly zero
        else:
            assert np.array_equal(f.astype(np.float64), frac)
        assert ((f >= 0) & (f < 1)).all() and ((i == c) | (i == c - 1)).all()
    # the table itself
    _, i, f = U.axis(np.arange(s), 0, s)
    want = {2: ([-1, 0], [0.75, 0.25]), 3: ([-1, 0, 0], [f32(-2.0) / f32(6.0) + f32(1.0), 0.0, f32(2.0) / f32(6.0)]),
            4: ([-1, -1, 0, 0], [0.625, 0.875, 0.125, 0.375])}[s]
    assert i.tolist() == want[0] and np.array_equal(f, np.array(want[1], f32))


# ------------------------------------------------------------------ the hand-made planes
@pytest.mark.parametrize("s", SCALES)
def test_synthetic_planes_put_every_branch_on_its_known_pixel(s):
    d = U.synthetic_planes(s)
    w, h = d["size"]
    px = np.ones((h, w), bool)
    ref = U.upsample_ref(d["lo"], d["hi"], s, d["rects"], px, **d["params"])
    for name, (X, Y, branch, why) in d["known"].items():
        got = {r: int(ref["taps"][r][Y, X]) for r in U.REASONS if ref["taps"][r][Y, X]}
        assert (int(ref["branch"][Y, X]), got) == (branch, why), (name, X, Y, int(ref["branch"][Y, X]), got)
    assert ("weight_zero_taps" in d["known"]) == (s == 3)
    assert set(np.unique(ref["branch"])) == {U.FULL, U.PARTIAL, U.RESCUE, U.ORPHAN}
    assert U.counters(ref)[0] == w * h and ref["rescued"] >= 1 and ref["orphans"] == 2 and 0 < ref["hits"] < w * h
    out, wgt, lo_bits = ref["out"].view(f32), ref["weight_out"].view(f32), d["lo"]["color"].view(np.uint32)
    # the rescued pixel: the one match of the ring, unweighted; the orphans: the low-res pixel that contains them, NaN word and all
    X, Y = d["known"]["rescue"][:2]
    assert wgt[Y, X] == 0 and np.array_equal(ref["out"][Y, X], lo_bits[10, 10])
    for name in ("orphan", "orphan_over_nan"):
        X, Y = d["known"][name][:2]
        assert wgt[Y, X] == -1 and np.array_equal(ref["out"][Y, X], lo_bits[Y // s, X // s])
    assert np.isnan(out[d["known"]["orphan_over_nan"][1], d["known"]["orphan_over_nan"][0], 1])
    # a plane distance exactly on plane_eps * t counts, one ulp beyond does not; a hair less plane_eps loses the first, too
    less = U.upsample_ref(d["lo"], d["hi"], s, d["rects"], px, normal_cos=0.9, plane_eps=float(np.nextafter(f32(0.125), f32(0))))
    X, Y = d["known"]["plane_exactly_on"][:2]
    assert ref["taps"]["plane"][Y, X] == 0 and less["taps"]["plane"][Y, X] == 3
    # a miss is interpolated from misses, with all four weights: exactly the bilinear formula
    X, Y = d["known"]["miss_miss"][:2]
    assert d["hi"]["hit"].view(np.int32)[Y, X, 3] < 0 and wgt[Y, X] == pytest.approx(1.0, abs=2e-7)
    if s == 3:
        X, Y = d["known"]["weight_zero_taps"][:2]
        assert wgt[Y, X] == 1 and np.array_equal(ref["out"][Y, X], lo_bits[Y // 3, X // 3])
    # no tap crosses the view border: B's colours are 2 higher than A's, and both views are the same surface there
    V = U.SYNTHETIC_VIEW
    fin = np.isfinite(out[..., :3]).all(-1)
    assert (out[:, :V, :3][fin[:, :V]] < 1.0 + 1e-6).all() and (out[:, V:, :3][fin[:, V:]] >= 2.0 - 1e-6).all()
    # ... and each view is upsampled as a frame of its own
    for k, (x, y, rw, rh) in enumerate(d["rects"]):
        lo = {n: np.ascontiguousarray(a[y // s:(y + rh) // s, x // s:(x + rw) // s]) for n, a in d["lo"].items()}
        hi = {n: np.ascontiguousarray(a[y:y + rh, x:x + rw]) for n, a in d["hi"].items()}
        alone = U.upsample_ref(lo, hi, s, [(0, 0, rw, rh)], np.ones((rh, rw), bool), **d["params"])
        assert np.array_equal(alone["out"], ref["out"][y:y + rh, x:x + rw]) and np.array_equal(alone["weight_out"], ref["weight_out"][y:y + rh, x:x + rw])
    # pixels outside the set keep the sentinel
    part = px.copy()
    part[:, 40:56] = False
    some = U.upsample_ref(d["lo"], d["hi"], s, d["rects"], part, **d["params"])
    assert (some["out"][~part] == U.SENTINEL).all() and (some["weight_out"][~part] == U.SENTINEL).all() and (some["branch"][~part] == U.OUTSIDE).all()
    assert np.array_equal(some["out"][part], ref["out"][part])


# ------------------------------------------------------------------ what the plane means
# rms(guided) / rms(plain bilinear) of the NumPy reference on the CPU-built planes below, as this test measures it (it prints its figures):
# the bound of the assertion is halfway between this ratio and 1.
RATIOS = {("two_box", 2): 0.1444, ("two_box", 3): 0.2262, ("two_box", 4): 0.2851,
          ("terrain", 2): 0.8114, ("terrain", 3): 0.8724, ("terrain", 4): 0.9150}
# rms against the analytic function on the full-resolution planes, measured with them: guided / plain bilinear / normal and plane tests off / fx
# and fy swapped / both, and the pixels of 7920 that took the rescue / the orphan branch:
#   two_box 2: 0.00524 / 0.03630 / 0.01478 / 0.01469 / 0.02770, 4 / 0       terrain 2: 0.15567 / 0.19186 / 0.18830 / 0.16017 / 0.20796, 208 / 399
#   two_box 3: 0.00963 / 0.04256 / 0.02395 / 0.02343 / 0.03543, 12 / 0      terrain 3: 0.18597 / 0.21317 / 0.21497 / 0.18645 / 0.22478, 524 / 778
#   two_box 4: 0.01338 / 0.04693 / 0.02559 / 0.03128 / 0.04584, 8 / 0       terrain 4: 0.21380 / 0.23366 / 0.23984 / 0.21503 / 0.24883, 501 / 1297
_MEANING = {}


def _scene(name):
    from optixpathtracer_amd import scenes

    return {"two_box": (lambda: scenes.two_box_scene(shadow_catcher=False), scenes.TWO_BOX_CAMERA),
            "terrain": (lambda: scenes.voxel_terrain(n=64, target_tris=20000), scenes.TERRAIN_CAMERA)}[name]


def _meaning(orc, name, s):
    """The CPU-built planes of `name` at 132 x 60 and at 132/s x 60/s under the library's own camera, the analytic irradiance on both, and
    the rms error of the rule and of its variants against the full-resolution one.  Built once per (scene, scale)."""
    if (name, s) not in _MEANING:
        make, cam = _scene(name)
        w, h = U.MEANING_SIZE
        if name not in _MEANING:
            _MEANING[name] = (make(), None)
            _MEANING[name] = (_MEANING[name][0], T.cpu_planes(orc, _MEANING[name][0], (w, h), cam, cam))
        model, hi = _MEANING[name]
        low = T.cpu_planes(orc, model, (w // s, h // s), cam, cam)
        colour = np.concatenate([U.irradiance(low), np.ones((h // s, w // s, 1))], -1).astype(f32)
        lo = dict(color=colour, hit=low["hit"], position=low["position"])
        truth = U.irradiance(hi)
        refs = {k: U.upsample_ref(lo, hi, s, [(0, 0, w, h)], np.ones((h, w), bool), **kw)
                for k, kw in dict(guided={}, plain=dict(guided=False), no_geometry=dict(geometry=False), swapped=dict(swap=True),
                                   weakened=dict(geometry=False, swap=True)).items()}
        err = {k: U.rms(r["out"].view(f32), truth) for k, r in refs.items()}
        print(f"{name} scale {s}: rms " + " ".join(f"{k} {v:.5f}" for k, v in err.items()) + f"; ratio {err['guided'] / err['plain']:.4f}; "
              f"full {refs['guided']['full']} rescued {refs['guided']['rescued']} orphans {refs['guided']['orphans']} of {w * h}")
        _MEANING[(name, s)] = (err, refs["guided"])
    return _MEANING[(name, s)]


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_the_guided_plane_is_nearer_to_the_full_resolution_function(orc_det, name, s):
    err, ref = _meaning(orc_det, name, s)
    ratio = err["guided"] / err["plain"]
    assert abs(ratio - RATIOS[(name, s)]) <= 5e-4 * max(1.0, RATIOS[(name, s)] / 0.1), f"the recorded ratio {RATIOS[(name, s)]} is stale: {ratio:.4f}"
    assert err["guided"] <= 0.5 * (RATIOS[(name, s)] + 1.0) * err["plain"]
    w, h = U.MEANING_SIZE
    assert U.counters(ref)[0] == w * h and not np.isnan(ref["out"].view(f32)).any()
    # conditions, not measurements
    if name == "two_box":
        assert ref["orphans"] == 0 and ref["rescued"] * 100 <= w * h
    else:  # the facets are smaller than a low-res pixel: the input that exercises the rescue and the orphan branch on real planes
        assert ref["rescued"] * 50 >= w * h and ref["orphans"] * 50 >= w * h


@pytest.mark.parametrize("s", SCALES)
def test_the_weakened_rule_misses_the_bound_on_two_box(orc_det, s):
    """The teeth: the same rule with the normal and plane tests switched off and with fx and fy swapped — one rule, both changes — must MISS
    the bound of test_the_guided_plane_is_nearer_to_the_full_resolution_function on two_box.  As a share of plain bilinear's rms at
    scales 2 / 3 / 4 it reaches 0.763 / 0.832 / 0.977 against bounds of 0.572 / 0.613 / 0.643.
    Either change alone is not enough to miss that bound at every scale (normal and plane tests off: 0.407 / 0.563 / 0.545; fx and fy
    swapped: 0.405 / 0.550 / 0.666): the mesh test and the miss / hit test stay on and keep most of the gain over plain bilinear, so each
    change alone is held to the nearer comparison of test_each_weakened_rule_is_worse_than_the_rule.  upsample_ref.irradiance is chosen
    so that both guides have something to do, and says how; a first function with less contrast across creases and a weaker
    oscillation left the doubly weakened rule at 0.491 / 0.491 / 0.535 of plain bilinear against bounds of 0.520 / 0.534 / 0.543, just
    inside them: an input on which this bound could see neither guide."""
    err, _ = _meaning(orc_det, "two_box", s)
    assert err["weakened"] > 0.5 * (RATIOS[("two_box", s)] + 1.0) * err["plain"], (s, err["weakened"] / err["plain"])


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("variant", ["no_geometry", "swapped", "weakened"])
def test_each_weakened_rule_is_worse_than_the_rule(orc_det, variant, s):
    """Dropping the normal and the plane test, exchanging fx and fy, or both, cannot help: on two_box every variant is strictly further
    from the full-resolution function than the rule is (they measure 1.9 to 5.3 times the rule's error; no factor is asserted)."""
    err, _ = _meaning(orc_det, "two_box", s)
    assert err[variant] > err["guided"], (variant, s, err[variant] / err["guided"])
