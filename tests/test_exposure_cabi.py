"""Auto exposure and display tone mapping (pt_exposure_planes, pt_tonemap_planes) without a GPU: the entry points are declared and exported,
the ctypes mirrors match the compiler's layout, the header compiles as C99 and C++17 and states the rules, null arguments are refused before
any device work, both facades have the methods; and properties of the NumPy reference (tests/exposure_ref.py) that pin what the rules
mean.  No bound here comes from a kernel's output: (f)'s are derived from the operators' formulas in the test's own docstring."""
import ctypes as C
import re

import numpy as np
import pytest

import exposure_ref as X
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_section
from optixpathtracer_amd import _lib

f32 = np.float32
u32 = np.uint32
NAMES = ("pt_exposure_planes", "pt_tonemap_planes")
E_DESC = ("color", "hit", "hist", "state_in", "state_out", "block_mask", "low_permille", "high_permille", "key_log2", "ev_min", "ev_max", "rate_up",
          "rate_down", "flags")
E_STATS = ("pixels", "skipped", "nonfinite", "under", "over", "kernel_ms")
T_DESC = ("color", "state", "out", "frame_rgba8", "block_mask", "exposure", "white", "op", "flags")
T_STATS = ("pixels", "clipped", "kernel_ms")


def test_library_exports_the_entry_points():
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name, stem in zip(NAMES, ("exposure", "tonemap")):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert name in header().split("VERSIONING.")[1].split("*/")[0]
        assert name in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
        assert re.search(rf"int\s+{name}\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_{stem}_desc\s*\*\s*\w+\s*,\s*pt_{stem}_stats\s*\*", src)
    assert b"0.4" in L.pt_version()
    assert (_lib.PT_EXPOSURE_BINS, _lib.PT_EXPOSURE_ACCUMULATE, _lib.PT_EXPOSURE_FROM_HISTOGRAM) == (256, 1, 2) == (X.BINS, 1, 2)
    assert _lib.TONEMAP_OPS == {"linear": 0, "reinhard": 1, "aces": 2} and tuple(_lib.TONEMAP_OPS) == X.OPS
    assert re.search(r"#define\s+PT_EXPOSURE_BINS\s+256\b", src) and re.search(r"PT_EXPOSURE_ACCUMULATE\s*=\s*1\s*,\s*PT_EXPOSURE_FROM_HISTOGRAM\s*=\s*2", src)
    assert re.search(r"PT_TONEMAP_LINEAR\s*=\s*0\s*,\s*PT_TONEMAP_REINHARD\s*=\s*1\s*,\s*PT_TONEMAP_ACES\s*=\s*2", src)


def test_struct_layouts_match_the_compiler(tmp_path):
    structs = [(_lib.ExposureDesc, "pt_exposure_desc", E_DESC), (_lib.ExposureStats, "pt_exposure_stats", E_STATS),
               (_lib.TonemapDesc, "pt_tonemap_desc", T_DESC), (_lib.TonemapStats, "pt_tonemap_stats", T_STATS)]
    check_layout(tmp_path, structs, [80, 0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 68, 72, 76] + [48, 0, 8, 16, 24, 32, 40] + [56, 0, 8, 16, 24, 32, 40, 44, 48, 52] + [24, 0, 8, 16])
    assert _lib.EXPOSURE_PLANES == {"color": 4, "hit": 8} and _lib.TONEMAP_PLANES == {"color": 4, "out": 4, "frame_rgba8": 1}
    assert _lib.TONEMAP_OUTPUTS == ("out", "frame_rgba8")


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const float* color, const void* hit, uint32_t* hist, float* state, float* out, uint32_t* frame) {\n"
            "    pt_exposure_desc d = {0, 0, 0, 0, 0, 0, 50u, 20u, -2.47f, -16.0f, 16.0f, 1.0f, 0.25f, 0u};\n"
            "    pt_tonemap_desc t = {0, 0, 0, 0, 0, 1.0f, 1.0f, 0u, 0u};\n"
            "    pt_exposure_stats s;\n"
            "    pt_tonemap_stats ts;\n"
            "    uint32_t bins[PT_EXPOSURE_BINS];\n"
            "    d.color = color; d.hit = hit; d.hist = hist; d.state_in = state; d.state_out = state;\n"
            "    d.flags = PT_EXPOSURE_ACCUMULATE | PT_EXPOSURE_FROM_HISTOGRAM;\n"
            "    t.color = color; t.state = state; t.out = out; t.frame_rgba8 = frame; t.op = PT_TONEMAP_ACES;\n"
            "    bins[0] = PT_TONEMAP_LINEAR + PT_TONEMAP_REINHARD;\n"
            "    return pt_exposure_planes(c, &d, &s) || pt_tonemap_planes(c, &t, &ts) || s.under + s.over + s.skipped + s.nonfinite > s.pixels\n"
            "           || ts.clipped > ts.pixels || bins[0] != 1u;\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.ExposureDesc(), _lib.ExposureStats(7, 7, 7, 7, 7, 7.0)
    assert L.pt_exposure_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_exposure_planes: null context" in L.pt_last_error(None)
    assert L.pt_exposure_planes(None, None, None) == -1
    assert tuple(getattr(s, n) for n in E_STATS) == (7, 7, 7, 7, 7, 7.0)
    t, ts = _lib.TonemapDesc(), _lib.TonemapStats(7, 7, 7.0)
    assert L.pt_tonemap_planes(None, C.byref(t), C.byref(ts)) == -1
    assert b"pt_tonemap_planes: null context" in L.pt_last_error(None)
    assert L.pt_tonemap_planes(None, None, None) == -1
    assert tuple(getattr(ts, n) for n in T_STATS) == (7, 7, 7.0)


def test_facades_have_the_methods(tmp_path):
    import torch  # noqa: F401

    from optixpathtracer_amd import renderer as R

    for name in ("exposurePlanes", "tonemapPlanes"):
        assert callable(getattr(R.SampleRenderer, name, None)) and callable(getattr(R._RankView, name, None))
    r = bare_renderer()
    color = fake_cuda((4, 4, 4))
    with pytest.raises(ValueError, match="color is required"):
        r.exposurePlanes(None)
    with pytest.raises(ValueError, match=r"hit: a contiguous torch.float32 tensor of shape \(4, 4, 8\) is expected"):
        r.exposurePlanes(color, hit=fake_cuda((4, 4, 4)))
    with pytest.raises(ValueError, match="color is required"):
        r.tonemapPlanes(None)
    with pytest.raises(ValueError, match="unknown operator 'filmic'"):
        r.tonemapPlanes(color, op="filmic")
    with pytest.raises(ValueError, match="no output asked for"):
        r.tonemapPlanes(color, write_out=False)
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t expose(SampleRenderer& sample, pt_exposure_desc d, pt_tonemap_desc t) {\n"
        "    d.key_log2 = -2.47f;\n"
        "    pt_exposure_stats s{};\n"
        "    pt_tonemap_stats ts{};\n"
        "    sample.exposurePlanes(d, &s);\n"
        "    t.state = d.state_out;\n"
        "    t.op = PT_TONEMAP_ACES;\n"
        "    sample.tonemapPlanes(t, &ts);\n"
        "    return sample.exposurePlanes(d).under + s.over + sample.tonemapPlanes(t).clipped + ts.pixels;\n"
        "}\n"
    )


def test_header_states_the_rules():
    text = header_section("AUTO EXPOSURE AND DISPLAY TONE MAPPING", "The acceleration structure as the traversal kernels see it")
    for item in ("nv = max(1, the view count)", "hist: nv x PT_EXPOSURE_BINS uint32", "PT_EXPOSURE_ACCUMULATE — hist is not zeroed first",
                 "PT_EXPOSURE_FROM_HISTOGRAM — no metering, hist is read as given", "all-reduces the integer histograms",
                 "hit[p].prim is negative (a miss), the pixel is not counted: stats->skipped", "no address is formed from it", "exponent-bit test",
                 "stats->nonfinite", "Y = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z", "If !(Y > 0): bin 0", "(the sum overflowed): bin 255",
                 "k = (int)(bits(Y) >> 20) - 887", "0 for k < 1, 255 for k > 254, else k", "eight bins per stop", "Bin 1 starts at 2^-16",
                 "bin 254 ends below 2^15.75", "denormals land in bin 0", "no transcendental", "hist[view][bin] += 1", "no float is accumulated anywhere",
                 "stats->under counts bin 0, stats->over bin 255", "N = sum c[i]", "lo = N * low_permille / 1000 and hi = N * high_permille / 1000",
                 "take = min(c[i], lo)", "walking down from bin 255", "S = sum over 1..254 of c[i] * (2i - 1)", "-16 + (2i - 1) / 16",
                 "at most 0.09 stops", "a NaN (0x7fc00000) when state_in is NULL", "else 0.0f", "q = (S << 12) / n in uint64 (q < 2^21)",
                 "m = (float)q * (1.0f / 65536.0f) - 16.0f", "t = key_log2 - m", "t = t < ev_min ? ev_min : t; t = t > ev_max ? ev_max : t",
                 "r = (t > ev_prev) ? rate_up : rate_down and ev = ev_prev + ((t - ev_prev) * r)", "E = pt_expf(ev * 0.69314718f)",
                 "state_out[4v .. 4v + 3] = (ev, E, m, (float)n)", "state_out may be exactly state_in", "low_permille + high_permille > 999",
                 "key_log2 not finite", "outside [-24, 24]", "ev_min > ev_max", "a rate outside [0, 1] or NaN",
                 "E_v = state ? state[4 * view + 1] : 1.0f", "not finite or not > 0 counts as 1.0f", "s = E_v * exposure", "x = x > 0 ? x : 0 (a NaN becomes 0)",
                 "x = x < 65504.0f ? x : 65504.0f (an inf becomes 65504)", "i = 1.0f / (1.0f + L / white); y = (x * 1.0f) * i",
                 "a = x * (2.51f * x + 0.03f); b = x * (2.43f * x + 0.59f) + 0.14f; y = a / b", "out[p] = (y, 1.0f); frame_rgba8[p] = make_color(y)",
                 "stats->clipped counts the pixels with a component of y above 1", "out exactly color", "flags != 0", "an unknown op",
                 "exposure or white not finite or not > 0", "write no context state", "centre-weighted metering", "local tone mapping", "bloom",
                 "a colour-managed output other than sRGB", "a pt_multi_* wrapper"):
        assert item in text, item


# ------------------------------------------------------------------ properties of the reference
def _image(seed=3, h=37, w=53, lo=-10.0, hi=6.0):
    """colours whose luminance spreads over [2^lo, 2^hi]"""
    rng = np.random.default_rng(seed)
    e = rng.uniform(lo, hi, (h, w, 1))
    c = (np.exp2(e) * rng.uniform(0.5, 1.0, (h, w, 3))).astype(f32)
    return np.concatenate([c, np.ones((h, w, 1), f32)], -1)


def _all(c):
    return np.ones(c.shape[:2], bool)


def test_a_scaling_by_a_power_of_two_shifts_the_histogram_and_the_mean_exactly():
    """(a): scaling by 2^k is exact in float32 and moves only the exponent field, so every bin moves by 8k and m by exactly k"""
    c = _image()
    h0, s0, _ = X.exposure_ref(c, _all(c), low_permille=30, high_permille=30)
    assert h0[0, 0] == h0[0, 255] == 0 and h0.sum() == c.shape[0] * c.shape[1]
    for k in (-5, -1, 1, 3, 8):
        ck = c.copy()
        ck[..., 0:3] *= f32(2.0 ** k)
        hk, sk, _ = X.exposure_ref(ck, _all(c), low_permille=30, high_permille=30)
        assert hk[0, 0] == hk[0, 255] == 0, "a pixel left bins 1..254: the case is wrong"
        assert np.array_equal(np.roll(h0[0], 8 * k), hk[0])
        assert float(sk[0, 2]) - float(s0[0, 2]) == k and sk[0, 3] == s0[0, 3]
        assert float(s0[0, 0]) - float(sk[0, 0]) == k  # ev = key - m, inside [ev_min, ev_max]


def test_bin_edges():
    """(b): 2^e * (1 + j / 8) opens a bin and the float below it closes the one before; the ends of the scale and the words outside it"""
    for e in (-16, -9, -1, 0, 1, 7, 15):
        for j in range(8):
            v = f32(2.0 ** e * (1 + j / 8))
            k = 8 * (e + 16) + j + 1
            if 1 <= k <= 254:
                assert X.bin_of(v) == k and X.bin_of(np.nextafter(v, f32(0))) == k - 1, (e, j)
    assert X.bin_of(f32(2.0 ** -16)) == 1 and X.bin_of(np.nextafter(f32(2.0 ** -16), f32(0))) == 0
    top = f32(2.0 ** 15 * 1.625)  # bin 254 is [2^15 * 1.625, 2^15 * 1.75): 15.75 on the piecewise-linear log2
    assert X.bin_of(top) == 254 and X.bin_of(np.nextafter(f32(2.0 ** 15 * 1.75), f32(0))) == 254 and X.bin_of(f32(2.0 ** 15 * 1.75)) == 255
    words = np.array([0x00000000, 0x80000000, 0xBF800000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000], u32).view(f32)
    #                 +0          -0          -1          denormals               FLT_MIN     FLT_MAX     +inf        -inf        NaN
    assert X.bin_of(words).tolist() == [0, 0, 0, 0, 0, 0, 255, 255, 0, 0]
    # an overflowing luminance lands in bin 255 (bin_of(+inf) above).  The three weights sum to 1 within rounding, so the largest finite
    # colour's luminance is FLT_MAX itself: with finite components the overflow rule is a guard, and the pixel lands in 255 either way
    big = np.array([[[np.finfo(f32).max] * 3 + [1.0]]], f32)
    assert X.finite(big[..., 0:3]).all() and X.bin_of(X.luminance(big)) == 255
    h, cnt = X.meter_ref(big, np.ones((1, 1), bool))
    assert h[0, 255] == 1 and h.sum() == 1 and cnt["over"] == 1
    # a pixel with a non-finite component is not counted at all, a miss is skipped before its colour is looked at
    bad = np.array([[[np.nan, 1, 1, 1], [np.inf, 1, 1, 1], [1, 1, 1, 1]]], f32)
    hit = np.zeros((1, 3, 8), f32)
    hit.view(np.int32)[0, 0, 3] = -1
    h, cnt = X.meter_ref(bad, np.ones((1, 3), bool), hit)
    assert h.sum() == 1 and cnt == dict(pixels=3, skipped=1, nonfinite=1, under=0, over=0)


def test_trimming_removes_the_bright_tail():
    """(c): 5 % of the pixels at 2^12: high_permille = 50 removes their whole effect, high_permille = 0 does not"""
    base = np.full((20, 50, 4), 0.25, f32)
    img = base.copy()
    img.reshape(-1, 4)[:50, 0:3] = f32(4096.0)
    _, plain, _ = X.exposure_ref(base, _all(base), low_permille=0, high_permille=0)
    _, trimmed, _ = X.exposure_ref(img, _all(img), low_permille=0, high_permille=50)
    _, untrimmed, _ = X.exposure_ref(img, _all(img), low_permille=0, high_permille=0)
    assert trimmed[0, 2] == plain[0, 2] and trimmed[0, 0] == plain[0, 0] and trimmed[0, 3] == 950
    assert untrimmed[0, 2] > plain[0, 2] + 0.5 and untrimmed[0, 3] == 1000
    # the value of m: 0.25's luminance lies in the bin of [2^-2, 2^-2 * 1.125) or the one below it (the weights sum to 1 within rounding)
    assert abs(float(plain[0, 2]) + 2.0) <= 0.125


def test_partitions_histograms_add_up():
    """(d): the histograms of three partitions' pixel sets sum to the whole frame's"""
    c = _image(seed=5)
    h, w = c.shape[:2]
    by, bx = np.mgrid[0:h, 0:w] // 8
    whole, state, _ = X.exposure_ref(c, _all(c))
    parts = [X.meter_ref(c, (bx + by) % 3 == k)[0] for k in range(3)]
    total = sum(p.astype(np.int64) for p in parts)
    assert np.array_equal(total, whole) and all(p.sum() > 0 for p in parts)
    assert np.array_equal(X.adapt_ref(total).view(u32), state.view(u32))
    # ACCUMULATE: metering into a given histogram
    acc, _ = X.meter_ref(c, (bx + by) % 3 == 1, hist=parts[0])
    assert np.array_equal(acc, parts[0] + parts[1])


def test_adaptation_rates():
    """(e): rate 1 reaches t in one step, rate 0 never moves, and the sign of the step picks the rate"""
    c = _image(seed=7)
    hist, free, _ = X.exposure_ref(c, _all(c))
    t = free[0, 0]
    assert free[0, 1] == X.expf(t * f32(0.69314718)) and abs(float(free[0, 1]) / 2.0 ** float(t) - 1) < 1e-6
    for prev in (t - f32(3), t + f32(3)):
        state = np.array([[prev, 1.0, 0.0, 0.0]], f32)
        assert X.adapt_ref(hist, state, rate_up=1.0, rate_down=1.0)[0, 0] == t
        assert X.adapt_ref(hist, state, rate_up=0.0, rate_down=0.0)[0, 0] == prev
        up = X.adapt_ref(hist, state, rate_up=0.5, rate_down=0.25)[0, 0]
        assert up == prev + (t - prev) * f32(0.5 if t > prev else 0.25)
        assert X.adapt_ref(hist, state, rate_up=0.5, rate_down=0.0)[0, 0] == (up if t > prev else prev)
    # no previous exposure, or one that is not finite: the target itself; an empty histogram keeps what there was
    assert X.adapt_ref(hist, np.array([[np.nan, 1, 0, 0]], f32), rate_up=0.0, rate_down=0.0)[0, 0] == t
    empty = np.zeros((1, 256), u32)
    out = X.adapt_ref(empty)
    assert out[0, 0] == 0 and out[0, 1] == 1 and out.view(u32)[0, 2] == X.NAN_BITS and out[0, 3] == 0
    out = X.adapt_ref(empty, np.array([[1.5, 9.0, -3.25, 77.0]], f32))
    assert out[0].tolist() == [1.5, float(X.expf(f32(1.5) * f32(0.69314718))), -3.25, 0.0]
    assert X.adapt_ref(empty, np.array([[np.inf, 1, -3.25, 0]], f32))[0, 0] == 0
    # bins 0 and 255 alone leave n == 0; the clamp holds
    ends = empty.copy()
    ends[0, 0], ends[0, 255] = 10, 10
    assert X.adapt_ref(ends, low_permille=0, high_permille=0)[0, 3] == 0
    assert X.adapt_ref(hist, ev_min=-1.0, ev_max=-0.5)[0, 0] == f32(-0.5 if t > -0.5 else -1.0 if t < -1 else t)


def test_operators_are_monotone_and_bounded():
    """(f), from the formulas.  ACES: a / b with a = 2.51 x^2 + 0.03 x, b = 2.43 x^2 + 0.59 x + 0.14.  (a / b)' has the sign of
    a'b - ab' = (2.51 * 0.59 - 2.43 * 0.03) x^2 + 2 * 2.51 * 0.14 x + 0.03 * 0.14 > 0 for x >= 0: increasing, from 0 towards its limit
    2.51 / 2.43 = 1.0329 < 1.04.  Reinhard on a grey colour v: y = v / (1 + L / white) with L = v within rounding: increasing, below
    white by white^2 / (white + v) — relative white / (white + 65504) >= 7.6e-6 for white >= 0.5.
    In float32 each operator is at most ten operations, each rounding once (relative 2^-24), all on non-negative terms, so the computed
    value is within 10 * 2^-24 relative of the true one: the bounds above hold with that room to spare, and two computed values can
    stand in the wrong order by at most 2 * 10 * 2^-24 relative — where the true function rises by more than that between two samples
    the computed one rises too.  Both are asserted."""
    x = np.unique(np.concatenate([np.zeros(1, f32), np.geomspace(1e-8, 65504.0, 200001).astype(f32), np.linspace(0, 65504.0, 100001).astype(f32),
                                  np.array([65504.0], f32)]))
    assert x[0] == 0 and x[-1] == f32(65504.0) and (np.diff(x) > 0).all()
    room = 20 * 2.0 ** -24
    y = X.aces(x)
    assert y[0] == 0 and y.min() >= 0 and y.max() <= 1.04 and y.max() > 1.03
    assert (np.diff(y.astype(np.float64)) >= -room * y[1:]).all()
    true = lambda v: (2.51 * v * v + 0.03 * v) / (2.43 * v * v + 0.59 * v + 0.14)  # noqa: E731
    t64 = true(x.astype(np.float64))
    rises = np.diff(t64) > room * t64[1:]
    assert rises.sum() > 100000 and (np.diff(y)[rises] > 0).all()
    for white in (0.5, 1.0, 4.0):
        g = X.reinhard(np.stack([x, x, x], -1), white)
        assert (g[:, 0] == g[:, 1]).all() and (g[:, 1] == g[:, 2]).all()
        y = g[:, 0]
        assert y[0] == 0 and y.min() >= 0 and y.max() <= white and y.max() > white * (1 - 2 * white / 65504.0)
        assert (np.diff(y.astype(np.float64)) >= -room * y[1:]).all()
        t64 = x.astype(np.float64) / (1 + x.astype(np.float64) / white)
        rises = np.diff(t64) > room * t64[1:]
        assert rises.sum() > 100000 and (np.diff(y)[rises] > 0).all()
    # the clamp in front of the operators
    w = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-45, 65504.0, 65505.0, 3e38, np.inf], f32)
    assert X._clamp(w).tolist() == [0, 0, 0, 0, 0, float(f32(1e-45)), 65504.0, 65504.0, 65504.0, 65504.0]


def test_the_tone_mapped_reference_on_a_small_frame(orc_det):
    """tonemap_ref end to end: the exposure word of each view, the invalid words that count as 1, the counters, the sentinel outside the set"""
    c = _image(seed=9, h=16, w=24, lo=-4, hi=4)
    rects = [(0, 0, 8, 16), (8, 0, 16, 8)]
    pixels = X.view_index(rects, 16, 24) >= 0
    state = np.array([[1.0, 2.0, 0, 0], [0.0, np.nan, 0, 0]], f32)
    r = X.tonemap_ref(c, pixels, state, rects, op="linear", exposure=0.5, orc=orc_det)
    out = r["out"].view(f32)
    assert np.array_equal(out[:, 0:8, 0:3], c[:, 0:8, 0:3]) and np.array_equal(out[0:8, 8:24, 0:3], c[0:8, 8:24, 0:3] * f32(0.5))
    assert (r["out"][~pixels] == X.SENTINEL).all() and (r["frame_rgba8"][~pixels] == X.SENTINEL).all() and (out[..., 3][pixels] == 1).all()
    assert r["pixels"] == int(pixels.sum()) and 0 < r["clipped"] < r["pixels"]
    assert (r["frame_rgba8"][pixels] >> 24 == 255).all()
    # a grey image: Reinhard with white 1 clips nothing, the linear operator clips what lies above 1
    grey = np.repeat(c[..., 0:1], 4, -1)
    assert X.tonemap_ref(grey, pixels, None, rects, op="reinhard", planes=())["clipped"] == 0
    assert X.tonemap_ref(grey, pixels, None, rects, op="linear", planes=())["clipped"] == int((grey[..., 0][pixels] > 1).sum()) > 0
