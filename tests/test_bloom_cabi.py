"""Bloom (pt_bloom_layout, pt_bloom_planes) without a GPU: the entry points are declared and exported, the ctypes mirrors match the compiler's
layout, the header compiles as C99 and C++17 and states the rule, null arguments are refused before any device work, both facades check
their arguments; and properties of the NumPy reference (tests/bloom_ref.py) that pin what the rule means.  No bound here comes from a
kernel's output: each is exact, or derived in the test's own docstring."""
import ctypes as C
import re

import numpy as np
import pytest

import bloom_ref as B
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_section
from optixpathtracer_amd import _lib

f32 = np.float32
u32 = np.uint32
NAMES = ("pt_bloom_layout", "pt_bloom_planes")
DESC = ("color", "state", "out", "scratch", "block_mask", "exposure", "threshold", "knee", "clamp", "spread", "intensity", "levels", "flags")
STATS = ("pixels", "sources", "bright", "nonfinite", "kernel_ms")
SIZES = [(1, 1), (2, 2), (5, 3), (9, 17), (131, 59)]  # (w, h)


def test_library_exports_the_entry_points():
    assert all(name in _lib.EXPORTS for name in NAMES)
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NAMES:
        assert hasattr(L, name)
        assert name in header().split("VERSIONING.")[1].split("*/")[0]
        assert name in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_bloom_layout\s*\(\s*const\s+pt_ctx\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*size_t\s*\*\s*\w+\s*\)", src)
    assert re.search(r"int\s+pt_bloom_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_bloom_desc\s*\*\s*\w+\s*,\s*pt_bloom_stats\s*\*", src)
    assert b"0.4" in L.pt_version()
    assert _lib.PT_BLOOM_MAX_LEVELS == 8 == B.MAX_LEVELS and re.search(r"#define\s+PT_BLOOM_MAX_LEVELS\s+8\b", src)


def test_struct_layouts_match_the_compiler(tmp_path):
    structs = [(_lib.BloomDesc, "pt_bloom_desc", DESC), (_lib.BloomStats, "pt_bloom_stats", STATS)]
    check_layout(tmp_path, structs, [72, 0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60, 64, 68] + [40, 0, 8, 16, 24, 32])
    assert _lib.BLOOM_PLANES == {"color": 4, "out": 4} and _lib.BLOOM_OUTPUTS == ("out",)


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const float* color, const float* state, float* out, void* scratch) {\n"
            "    pt_bloom_desc d = {0, 0, 0, 0, 0, 1.0f, 1.0f, 0.5f, 65504.0f, 0.7f, 0.25f, 6u, 0u};\n"
            "    pt_bloom_stats s;\n"
            "    uint32_t dims[PT_BLOOM_MAX_LEVELS * 4];\n"
            "    size_t bytes = 0;\n"
            "    d.color = color; d.state = state; d.out = out; d.scratch = scratch;\n"
            "    return pt_bloom_layout(c, d.levels, dims, &bytes) || pt_bloom_planes(c, &d, &s) || s.bright + s.nonfinite > s.sources\n"
            "           || s.pixels > s.sources || dims[0] == 0u || bytes == 0;\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.BloomDesc(), _lib.BloomStats(7, 7, 7, 7, 7.0)
    assert L.pt_bloom_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_bloom_planes: null context" in L.pt_last_error(None)
    assert L.pt_bloom_planes(None, None, None) == -1
    assert tuple(getattr(s, n) for n in STATS) == (7, 7, 7, 7, 7.0)
    nbytes = C.c_size_t(77)
    dims = np.full(32, 9, u32)
    assert L.pt_bloom_layout(None, 6, dims.ctypes.data, C.byref(nbytes)) == -1
    assert b"pt_bloom_layout: null context" in L.pt_last_error(None)
    assert L.pt_bloom_layout(None, 6, None, None) == -1
    assert nbytes.value == 77 and (dims == 9).all()


def test_facades_check_their_arguments(tmp_path):
    import torch  # noqa: F401

    from optixpathtracer_amd import renderer as R

    for name in ("bloomLayout", "bloomPlanes"):
        assert callable(getattr(R.SampleRenderer, name, None)) and callable(getattr(R._RankView, name, None))
    r = bare_renderer()
    color = fake_cuda((4, 4, 4))
    with pytest.raises(ValueError, match="color is required"):
        r.bloomPlanes(None)
    with pytest.raises(ValueError, match=r"out: a contiguous torch.float32 tensor of shape \(4, 4, 4\) is expected"):
        r.bloomPlanes(color, out=fake_cuda((4, 4, 3)))
    with pytest.raises(ValueError, match=r"state: a contiguous torch.float32 tensor of shape \(1, 4\) is expected"):
        r.bloomPlanes(color, state=fake_cuda((2, 4)), out=fake_cuda((4, 4, 4)))
    for bad in (0, 9):
        with pytest.raises(ValueError, match=f"bloomPlanes: levels must be 1..8, not {bad}"):
            r.bloomPlanes(color, levels=bad)
        with pytest.raises(ValueError, match=f"bloomLayout: levels must be 1..8, not {bad}"):
            r.bloomLayout(bad)
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t bloom(SampleRenderer& sample, pt_bloom_desc d) {\n"
        "    uint32_t dims[PT_BLOOM_MAX_LEVELS * 4];\n"
        "    const size_t bytes = sample.bloomLayout(d.levels, dims) + sample.bloomLayout(6);\n"
        "    pt_bloom_stats s{};\n"
        "    sample.bloomPlanes(d, &s);\n"
        "    return sample.bloomPlanes(d).bright + s.sources + bytes + dims[2];\n"
        "}\n"
    )


def test_header_states_the_rule():
    text = header_section("BLOOM (no reference counterpart)", "The acceleration structure as the traversal kernels see it")
    for item in ("nv = max(1, the view count)", "w_k = (w_{k-1} + 1) / 2 and h_k = (h_{k-1} + 1) / 2", "the level count is not reduced",
                 "No tap ever leaves its rectangle", "puts nothing into the other", "view after view, level 1 first", "(x, y, z, 0)",
                 "zeros for the levels above", "The pyramid reads EVERY pixel of every rectangle", "the set decides only which pixels of out are written",
                 "exactly pt_modulate_planes's", "all-gather their colour first", "still sees the light of the blocks it does not write",
                 "stats->sources is the number of rectangle pixels read", "stats->pixels the size of the set", "exponent-bit test",
                 "B = 0 and stats->nonfinite counts it", "x = c > 0 ? c : 0; x = x < clamp ? x : clamp", "s = E_v * exposure",
                 "state ? state[4 * view + 1] : 1.0f", "Y = ((0.2126f * x.r + 0.7152f * x.g) + 0.0722f * x.b) * s; d = Y - threshold",
                 "t = d + knee; t = t > 0 ? t : 0; t = t < 2.0f * knee ? t : 2.0f * knee", "t = (t * t) / (4.0f * knee + 1e-4f)",
                 "m = t > d ? t : d; m = m > 0 ? m : 0", "g = m / (Y > 1e-4f ? Y : 1e-4f); B = x * g", "stats->bright counts g > 0",
                 "For knee <= threshold g stays within [0, 1]",
                 "columns 2i - 1, 2i, 2i + 1, 2i + 2, each clamped to [0, w_{k-1} - 1]", "r = ((S0 + 3.0f * S1) + 3.0f * S2) + S3",
                 "v = ((r0 + 3.0f * r1) + 3.0f * r2) + r3; D_k = v * (1.0f / 64.0f)", "U_levels = D_levels", "U_k = D_k + spread * up_k(U_{k+1})",
                 "i = x >> 1; i2 = (x & 1) ? min(i + 1, w_{k+1} - 1) : max(i - 1, 0)",
                 "up = 0.75f * (0.75f * U(i, j) + 0.25f * U(i2, j)) + 0.25f * (0.75f * U(i, j2) + 0.25f * U(i2, j2))", "level k of the scratch holds U_k",
                 "out[p].xyz = color[p].xyz + a * up_0(U_1)", "out[p].w = 1.0f", "a = intensity * (1.0f / n)", "n = n * spread + 1",
                 "a NaN pixel stays NaN", "out may be exactly color", "scratch not 16-byte aligned", "flags != 0", "levels outside 1 .. PT_BLOOM_MAX_LEVELS",
                 "spread outside [0, 1] or NaN", "no fused multiply-add", "writes no context state", "a dirt mask", "temporal smoothing of the pyramid",
                 "an asynchronous variant", "a pt_multi_* wrapper"):
        assert item in text, item


# ------------------------------------------------------------------ properties of the reference
def _all(c):
    return np.ones(c.shape[:2], bool)


def _image(seed, h, w, lo=-6.0, hi=6.0):
    rng = np.random.default_rng(seed)
    c = (np.exp2(rng.uniform(lo, hi, (h, w, 1))) * rng.uniform(0.4, 1.0, (h, w, 3))).astype(f32)
    return np.concatenate([c, np.ones((h, w, 1), f32)], -1)


def test_layout_sizes():
    """odd sizes round up; sizes bottom out at 1 and the level count is not reduced (3 x 5 with 8 levels: 2x3, 1x2, then 1x1 six times)"""
    dims, nbytes = B.layout(None, 5, 3, 8)
    assert dims[0, :, 0:2].tolist() == [[2, 3], [1, 2]] + [[1, 1]] * 6
    assert dims[0, :, 2].tolist() == [0, 6, 8, 9, 10, 11, 12, 13] and nbytes == 16 * 14 and (dims[..., 3] == 0).all()
    dims, nbytes = B.layout(None, 59, 131, 3)
    assert dims[0, :, 0:2].tolist() == [[66, 30], [33, 15], [17, 8]] + [[0, 0]] * 5 and nbytes == 16 * (66 * 30 + 33 * 15 + 17 * 8)
    # views: view after view, each with all its levels
    dims, nbytes = B.layout([(0, 0, 9, 17), (16, 0, 7, 5)], 24, 32, 2)
    assert dims[0, 0:2].tolist() == [[5, 9, 0, 0], [3, 5, 45, 0]] and dims[1, 0:2].tolist() == [[4, 3, 60, 0], [2, 2, 72, 0]] and nbytes == 16 * 76


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("levels", [1, 2, 6, 8])
def test_a_constant_plane_comes_through_every_level_exactly(size, levels):
    """1.5 * 2^-3 has two mantissa bits.  Threshold 0 and knee 0 give g = Y / Y = 1 exactly, so B = x.  A down step of a constant v is
    ((v + 3v) + 3v) + v = 8v per row, 64v over the rows, times 1/64: every step exact, so D_k = B.  With spread 0.5 the up step of a
    constant u is 0.75 (0.75u + 0.25u) + 0.25 (0.75u + 0.25u) = u, exact for few bits, and U_k = B + 0.5 U_{k+1} = B * n_k with
    n_k = 1 + n_{k+1} / 2 < 2, a multiple of 2^-7: exact.  So U_1 = B * n, and out = color + intensity * (1 / n) * (B * n)."""
    w, h = size
    v = f32(1.5 * 2.0 ** -3)
    c = np.full((h, w, 4), v, f32)
    r = B.bloom_ref(c, _all(c), threshold=0.0, knee=0.0, spread=0.5, intensity=1.0, levels=levels)
    a, n = B.gain(1.0, 0.5, levels)
    assert float(n) == 2.0 - 0.5 ** (levels - 1)
    assert (r["B"][0] == v).all() and r["bright"] == w * h and r["sources"] == w * h and r["nonfinite"] == 0
    for k in range(levels):
        assert (r["D"][0][k] == v).all(), f"D_{k + 1}"
    assert (r["U"][0][0] == v * n).all() and (r["U"][0][levels - 1] == v).all()
    out = r["out"].view(f32)
    assert (out[..., 3] == 1).all() and (out[..., 0:3] == v + a * (v * n)).all()
    assert abs(float(out[0, 0, 0]) / float(v) - 2.0) <= 2.0 ** -22


def test_an_impulse_keeps_its_energy():
    """One texel of value 1 in the interior of 64 x 64, spread 1, 4 levels.  Per axis a down step gives source column c the weights
    3 + 1 of 8 from the two outputs that read it (2i: S1 of i and S3 of i - 1; 2i + 1: S2 of i and S0 of i + 1), and at the borders of a
    level of EVEN width the clamped tap supplies the missing one (column 0: S1 and the clamped S0 of output 0), so a down step keeps a
    quarter of the sum wherever the energy lies; an up step gives source texel i the weights 0.75 + 0.75 + 0.25 + 0.25 = 2 per axis,
    borders included (x = 0: i2 = i).  64, 32, 16, 8 are even.  So D_k sums to 4^-k, up_k(U_{k+1}) to 4 * sum U_{k+1}, U_k to
    4^-k * (levels - k + 1), and the full-resolution up_0(U_1) to 4 * sum U_1 = 4 for 4 levels: one unit per level.
    Rounding: at most 40 operations lie between the impulse and a composite pixel, each within 2^-24 relative on non-negative terms, and
    the float64 sum adds nothing: 40 * 2^-24 relative on a sum of 4."""
    c = np.zeros((64, 64, 4), f32)
    c[29, 34, 0:3] = (1.0, 2.0, 0.5)
    r = B.bloom_ref(c, _all(c), threshold=0.0, knee=0.0, spread=1.0, intensity=4.0, levels=4)
    a, n = B.gain(4.0, 1.0, 4)
    assert n == 4 and a == 1
    got = r["out"].view(f32)[..., 0:3].astype(np.float64) - c[..., 0:3]
    for ch, val in enumerate((1.0, 2.0, 0.5)):
        assert abs(got[..., ch].sum() / (4.0 * val) - 1.0) <= 40 * 2.0 ** -24, ch
    for k in range(4):
        assert abs(r["D"][0][k][..., 0].astype(np.float64).sum() * 4.0 ** (k + 1) - 1.0) <= 40 * 2.0 ** -24
    assert r["bright"] == 1 and (got >= 0).all()


def test_the_source_weight():
    """m = Y * g is max(d, t, 0) with d = Y - threshold and t = clamp(d + knee, 0, 2 knee)^2 / (4 knee + 1e-4).
    Zero: at and below threshold - knee both d and d + knee are <= 0, so m = 0 and g = 0 exactly.
    Monotone: d rises with Y, t is a clamped rising value squared, and so does their maximum.
    Bounded: write u = Y - (threshold - knee) = d + knee.  On the knee (0 <= u <= 2 knee) t <= u^2 / (4 knee) <= u / 2, and u <= Y where
    knee <= threshold, so t <= Y / 2; beyond it (d > knee) t is below (2 knee)^2 / (4 knee) = knee < d; and d < Y throughout.  So m <= Y
    and g <= 1 for knee <= threshold.  (With knee > threshold the knee reaches below Y = 0: m stays below knee / 4 there, but g = m / Y
    does not stay below 1; such a pair is accepted, and what holds is the bound on m.)
    In float32 m <= Y survives (every step rounds monotonically), a correctly rounded quotient of m <= Y is <= 1, and Y * g may fall
    short of m by the quotient's rounding and the product's: two computed values can stand in the wrong order by 2^-22 relative."""
    Y = np.unique(np.concatenate([np.zeros(1, f32), np.geomspace(1e-7, 6e4, 200001).astype(f32), np.linspace(0, 8, 100001).astype(f32)]))
    for threshold, knee in ((1.0, 0.5), (1.0, 0.0), (0.0, 0.0), (2.0, 2.0), (0.75, 0.25), (0.25, 1.0)):
        g = B.weight(Y, threshold, knee)
        assert g.dtype == f32 and np.isfinite(g).all() and g.min() >= 0
        below = Y <= f32(threshold) - f32(knee)
        assert (g[below] == 0).all() and (below.sum() > 1000 or threshold <= knee)
        m = Y.astype(np.float64) * g
        assert (np.diff(m) >= -(2.0 ** -22) * m[1:]).all()
        assert (g[Y > f32(threshold) + f32(knee)] > 0).all() and g[-1] > 0.99
        if knee <= threshold:
            assert g.max() <= 1
        else:
            assert m[Y <= f32(1e-4)].max() <= knee / 4 and g.max() > 1
    # the edge of the zero region itself
    assert (B.weight(np.array([0.0, 0.25, 0.5], f32), 1.0, 0.5) == 0).all() and B.weight(np.array([0.5001], f32), 1.0, 0.5)[0] > 0


def test_nonfinite_and_negative_pixels_do_not_spread():
    """one NaN, one +inf and one negative pixel: every other pixel's bloom is finite and equals the bloom of the plane with the three at 0"""
    c = _image(3, 59, 131)
    bad = c.copy()
    spots = [(7, 11), (30, 64), (58, 130)]
    bad[spots[0]][0] = np.nan
    bad[spots[1]][1] = np.inf
    bad[spots[2]][0:3] = -5.0
    zero = c.copy()
    for s in spots:
        zero[s][0:3] = 0
    prm = dict(threshold=0.5, knee=0.25, spread=0.8, intensity=0.5, levels=6)
    rb, rz = B.bloom_ref(bad, _all(c), **prm), B.bloom_ref(zero, _all(c), **prm)
    assert rb["nonfinite"] == 2 and rz["nonfinite"] == 0 and rb["bright"] == rz["bright"]
    assert np.array_equal(rb["scratch"], rz["scratch"]) and np.isfinite(rb["scratch"].view(f32)).all()
    keep = np.ones((59, 131), bool)
    for s in spots:
        keep[s] = False
    assert np.array_equal(rb["out"][keep], rz["out"][keep]) and np.isfinite(rb["out"].view(f32)[keep]).all()
    out = rb["out"].view(f32)
    assert np.isnan(out[spots[0]][0]) and np.isinf(out[spots[1]][1]) and out[spots[2]][0] < 0  # color enters the composite raw


def test_a_view_puts_nothing_into_its_neighbour():
    """two views side by side, the left one black but for a pixel at `clamp` beside the seam: the right view's pyramid is all zeros"""
    h, w = 24, 48
    rects = [(0, 0, 24, 24), (24, 0, 24, 24)]
    c = np.zeros((h, w, 4), f32)
    c[12, 23, 0:3] = 1e6
    r = B.bloom_ref(c, _all(c), rects=rects, threshold=1.0, knee=0.5, clamp=64.0, spread=1.0, intensity=1.0, levels=5)
    assert r["bright"] == 1 and float(r["B"][0][12, 23, 0]) <= 64.0
    assert all((u == 0).all() for u in r["U"][1]) and all((u > 0).any() for u in r["U"][0])
    out = r["out"].view(f32)
    assert (out[:, 24:, 0:3] == 0).all() and (out[:, 20:24, 0:3] > 0).all()
    dims, _ = B.layout(rects, h, w, 5)
    first = int(dims[1, 0, 2])
    assert (r["scratch"][4 * first:] == 0).all() and (r["scratch"][:4 * first] != 0).any()
    # without views the same plane bleeds across
    r = B.bloom_ref(c, _all(c), threshold=1.0, knee=0.5, clamp=64.0, spread=1.0, intensity=1.0, levels=5)
    assert (r["out"].view(f32)[:, 24:28, 0:3] > 0).all()
