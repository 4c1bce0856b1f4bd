"""Motion blur (pt_motion_blur_layout, pt_motion_blur_planes) without a GPU: the entry points are declared and exported, the ctypes mirrors
match the compiler's layout, the header compiles as C99 and C++17 and states the rule, null arguments are refused before any device work,
both facades check their arguments; and properties of the NumPy reference (tests/motion_blur_ref.py) that pin what the rule means.  No bound
here comes from a kernel's output: each is exact, or derived in the test's own docstring.  u = 2^-24 is float32's unit roundoff."""
import ctypes as C
import re

import numpy as np
import pytest

import motion_blur_ref as M
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_section
from optixpathtracer_amd import _lib

f32 = np.float32
u32 = np.uint32
U = 2.0 ** -24
NAMES = ("pt_motion_blur_layout", "pt_motion_blur_planes")
DESC = ("color", "motion", "depth", "out", "scratch", "block_mask", "shutter", "max_blur", "depth_soft", "taps", "seed", "flags")
STATS = ("pixels", "sources", "unknown", "moving", "taps", "nonfinite", "kernel_ms")


def test_library_exports_the_entry_points():
    assert all(name in _lib.EXPORTS for name in NAMES)
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NAMES:
        assert hasattr(L, name)
        assert name in header().split("VERSIONING.")[1].split("*/")[0]
        assert name in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_motion_blur_layout\s*\(\s*const\s+pt_ctx\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*size_t\s*\*\s*\w+\s*\)", src)
    assert re.search(r"int\s+pt_motion_blur_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_motion_blur_desc\s*\*\s*\w+\s*,\s*pt_motion_blur_stats\s*\*", src)
    assert b"0.4" in L.pt_version()
    assert _lib.PT_MOTION_BLUR_TILE == 16 == M.TILE and re.search(r"#define\s+PT_MOTION_BLUR_TILE\s+16\b", src)
    assert _lib.PT_MOTION_BLUR_JITTER == 1 == M.JITTER and re.search(r"PT_MOTION_BLUR_JITTER\s*=\s*1\b", src)


def test_struct_layouts_match_the_compiler(tmp_path):
    structs = [(_lib.MotionBlurDesc, "pt_motion_blur_desc", DESC), (_lib.MotionBlurStats, "pt_motion_blur_stats", STATS)]
    check_layout(tmp_path, structs, [72, 0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 68] + [56, 0, 8, 16, 24, 32, 40, 48])
    assert _lib.MOTION_BLUR_PLANES == {"color": 4, "motion": 2, "depth": 1, "out": 4} and _lib.MOTION_BLUR_OUTPUTS == ("out",)


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const float* color, const float* motion, const float* depth, float* out, void* scratch) {\n"
            "    pt_motion_blur_desc d = {0, 0, 0, 0, 0, 0, 0.5f, 16.0f, 0.05f, 12u, 0u, PT_MOTION_BLUR_JITTER};\n"
            "    pt_motion_blur_stats s;\n"
            "    uint32_t dims[4];\n"
            "    size_t bytes = 0;\n"
            "    d.color = color; d.motion = motion; d.depth = depth; d.out = out; d.scratch = scratch;\n"
            "    return pt_motion_blur_layout(c, dims, &bytes) || pt_motion_blur_planes(c, &d, &s) || s.unknown > s.sources\n"
            "           || s.moving > s.pixels || s.taps + s.nonfinite > s.moving * d.taps || dims[0] * PT_MOTION_BLUR_TILE == 0u || bytes == 0;\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.MotionBlurDesc(), _lib.MotionBlurStats(7, 7, 7, 7, 7, 7, 7.0)
    assert L.pt_motion_blur_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_motion_blur_planes: null context" in L.pt_last_error(None)
    assert L.pt_motion_blur_planes(None, None, None) == -1
    assert tuple(getattr(s, n) for n in STATS) == (7, 7, 7, 7, 7, 7, 7.0)
    nbytes = C.c_size_t(77)
    dims = np.full(4, 9, u32)
    assert L.pt_motion_blur_layout(None, dims.ctypes.data, C.byref(nbytes)) == -1
    assert b"pt_motion_blur_layout: null context" in L.pt_last_error(None)
    assert L.pt_motion_blur_layout(None, None, None) == -1
    assert nbytes.value == 77 and (dims == 9).all()


def test_facades_check_their_arguments(tmp_path):
    import torch  # noqa: F401

    from optixpathtracer_amd import renderer as R

    for name in ("motionBlurLayout", "motionBlurPlanes"):
        assert callable(getattr(R.SampleRenderer, name, None)) and callable(getattr(R._RankView, name, None))
    r = bare_renderer()
    color, motion, depth = fake_cuda((4, 4, 4)), fake_cuda((4, 4, 2)), fake_cuda((4, 4))
    with pytest.raises(ValueError, match="color is required"):
        r.motionBlurPlanes(None, motion, depth)
    with pytest.raises(ValueError, match="motion is required"):
        r.motionBlurPlanes(color, None, depth)
    with pytest.raises(ValueError, match="depth is required"):
        r.motionBlurPlanes(color, motion, None)
    with pytest.raises(ValueError, match=r"motion: a contiguous torch.float32 tensor of shape \(4, 4, 2\) is expected"):
        r.motionBlurPlanes(color, fake_cuda((4, 4, 4)), depth)
    with pytest.raises(ValueError, match=r"depth: a contiguous torch.float32 tensor of shape \(4, 4\) is expected"):
        r.motionBlurPlanes(color, motion, fake_cuda((4, 4, 1)))
    with pytest.raises(ValueError, match=r"out: a contiguous torch.float32 tensor of shape \(4, 4, 4\) is expected"):
        r.motionBlurPlanes(color, motion, depth, out=fake_cuda((4, 4, 3)))
    for bad in (0, 65):
        with pytest.raises(ValueError, match=f"motionBlurPlanes: taps must be 1..64, not {bad}"):
            r.motionBlurPlanes(color, motion, depth, taps=bad)
    for name, bad, text in (("shutter", -0.1, r"shutter must be in \[0,4\]"), ("shutter", 4.5, r"shutter must be in \[0,4\]"),
                            ("shutter", float("nan"), r"shutter must be in \[0,4\]"), ("max_blur", 0.5, r"max_blur must be in \[1,16\]"),
                            ("max_blur", 16.5, r"max_blur must be in \[1,16\]"), ("depth_soft", 0.0, r"depth_soft must be in \(0,1\]"),
                            ("depth_soft", 1.5, r"depth_soft must be in \(0,1\]"), ("seed", -1, r"seed must be in \[0,4294967295\]"),
                            ("seed", 2 ** 32, r"seed must be in \[0,4294967295\]")):
        with pytest.raises(ValueError, match="motionBlurPlanes: " + text):
            r.motionBlurPlanes(color, motion, depth, **{name: bad})
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t blur(SampleRenderer& sample, pt_motion_blur_desc d) {\n"
        "    uint32_t dims[4];\n"
        "    const size_t bytes = sample.motionBlurLayout(dims) + sample.motionBlurLayout();\n"
        "    pt_motion_blur_stats s{};\n"
        "    sample.motionBlurPlanes(d, &s);\n"
        "    return sample.motionBlurPlanes(d).moving + s.sources + bytes + dims[3];\n"
        "}\n"
    )


def test_header_states_the_rule():
    text = header_section("MOTION BLUR (no reference counterpart)", "The acceleration structure as the traversal kernels see it")
    for item in ("McGuire et al.", "tile maximum, neighbourhood maximum, then a depth-aware gather", "nv = max(1, the view count)",
                 "tw = (wr + 15) / 16 by th = (hr + 15) / 16", "anchored at the rectangle's origin", "No tap and no tile neighbour ever leaves its rectangle",
                 "a view holds the bits a context of its own size would hold", "a plane T of tw * th texels of 8 bytes", "then a plane N of the same size",
                 "tw, th, the index of T's first 8-byte texel and the index of N's", "The tile pass reads EVERY pixel of every rectangle",
                 "the set decides only which pixels of out are written", "exactly pt_modulate_planes's", "all-gather colour, motion and depth first",
                 "The whole scratch is written by every call, also with an empty set", "hs = 0.5f * shutter, R = max_blur and R2 = R * R",
                 "exponent-bit test", "V = (0, 0), l2 = 0, and stats->unknown counts it", "V = m * hs per component",
                 "v = v < -4096.0f ? -4096.0f : v; v = v > 4096.0f ? 4096.0f : v", "l2 = V.x * V.x + V.y * V.y", "If l2 > R2",
                 "s = R / sqrtf(l2); V = V * s per component", "ties go to the first pixel in row order", "visited in row order with a strict >: the first maximum wins",
                 "Because R <= PT_MOTION_BLUR_TILE nothing farther away can reach the tile", "vN = N(x / 16, y / 16)", "n2 = vN.x * vN.x + vN.y * vN.y",
                 "If n2 > 0.25f is false, or a word of c is not finite: out[p] = (c, 1.0f), raw", "stats->moving counts p",
                 "lN = sqrtf(n2); lp = max(sqrtf(l2(p)), 0.5f); wp = 1.0f / lp", "Z(d) = (d > 1e-6f && d <= FLT_MAX) ? d : FLT_MAX",
                 "a = ((float)i + 0.5f) + j", "t = (2.0f * a) / (float)taps - 1.0f", "qx = (int)floorf(((float)x + vN.x * t) + 0.5f), clamped to [0, wr - 1]",
                 "the tap is skipped and stats->nonfinite counts it", "d = fabsf(t) * lN", "with V(q) recomputed by step 1", "e = depth_soft * min(zp, zq)",
                 "fg = clamp01(1.0f - (zq - zp) / e); bg = clamp01(1.0f - (zp - zq) / e)", "cone(l) = clamp01(1.0f - d / l)",
                 "cyl(l) = 1.0f - (u * u) * (3.0f - 2.0f * u), with u = clamp01((d - 0.95f * l) / (1.05f * l - 0.95f * l))",
                 "w = (fg * cone(lq) + bg * cone(lp)) + (cyl(lq) * cyl(lp)) * 2.0f", "sum = sum + color[q].xyz * w per component; Wt = Wt + w; stats->taps counts w > 0",
                 "j = (float)(h >> 8) * 5.9604644775390625e-8f - 0.5f", "h = ((uint32_t)x * 0x9E3779B1u) ^ ((uint32_t)y * 0x85EBCA77u) ^ (seed * 0xC2B2AE3Du)",
                 "h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16", "If Wt == 0: out[p].xyz = c exactly",
                 "out[p].xyz = (c * wp + sum) / (wp + Wt) per component", "out[p].w = 1.0f", "x = x > 0 ? x : 0; x = x < 1 ? x : 1", "no fused multiply-add",
                 "scratch not 8-byte aligned", "out may NOT be color", "flag bits other than PT_MOTION_BLUR_JITTER", "shutter not finite or outside [0, 4]",
                 "max_blur not finite or outside [1, PT_MOTION_BLUR_TILE]", "depth_soft not finite or outside (0, 1]", "taps outside 1 .. 64",
                 "writes no context state", "off-diagonal tiles only when they point at the centre", "more than one dominant direction per tile",
                 "sub-pixel (bilinear) taps", "blur of the bloom pyramid", "an asynchronous variant", "a pt_multi_* wrapper", "camera-shutter curves"):
        assert item in text, item


# ------------------------------------------------------------------ the layout
@pytest.mark.parametrize("size, grid", [((1, 1), (1, 1)), ((16, 16), (1, 1)), ((17, 16), (2, 1)), ((33, 49), (3, 4))])
def test_layout_sizes(size, grid):
    w, h = size
    dims, nbytes = M.layout(None, h, w)
    n = grid[0] * grid[1]
    assert dims.tolist() == [[grid[0], grid[1], 0, n]] and nbytes == 16 * n


def test_layout_under_two_views_of_odd_sizes():
    """view after view, T then N: 17 x 33 has 2 x 3 tiles, 31 x 5 has 2 x 1"""
    dims, nbytes = M.layout([(0, 0, 17, 33), (24, 8, 31, 5)], 48, 64)
    assert dims.tolist() == [[2, 3, 0, 6], [2, 1, 12, 14]] and nbytes == 8 * 16


# ------------------------------------------------------------------ properties of the reference
W, H = 67, 41


def _all(h=H, w=W):
    return np.ones((h, w), bool)


def _image(seed, h=H, w=W):
    rng = np.random.default_rng(seed)
    c = (np.exp2(rng.uniform(-6, 4, (h, w, 1))) * rng.uniform(0.4, 1.0, (h, w, 3))).astype(f32)
    return np.concatenate([c, np.ones((h, w, 1), f32)], -1)


def _depth(seed, h=H, w=W):
    return np.random.default_rng(seed).uniform(1.0, 9.0, (h, w)).astype(f32)


def _is_color(r, c):
    out = r["out"]
    return np.array_equal(out[..., 0:3], np.ascontiguousarray(c[..., 0:3]).view(u32)) and (out.view(f32)[..., 3] == 1).all()


@pytest.mark.parametrize("case", ["zero", "unknown", "shutter 0"])
def test_no_motion_gives_the_colour_back(case):
    c, z = _image(1), _depth(2)
    m = np.zeros((H, W, 2), f32)
    shutter = 0.5
    if case == "unknown":
        m[:] = np.nan
    if case == "shutter 0":
        m = np.random.default_rng(3).uniform(-40, 40, (H, W, 2)).astype(f32)
        shutter = 0.0
    r = M.motion_blur_ref(c, m, z, _all(), shutter=shutter)
    assert _is_color(r, c) and (r["scratch"].view(f32) == 0).all()
    if case != "shutter 0":  # (a negative motion word times hs = 0 is -0: zero, with the sign bit)
        assert (r["scratch"] == 0).all()
    assert r["moving"] == 0 and r["taps"] == 0 and r["unknown"] == (W * H if case == "unknown" else 0) and r["sources"] == W * H == r["pixels"]


def test_tile_maxima_stay_within_max_blur():
    """A scaled V: l2 = fl(x^2 + y^2) <= |V|^2 (1 + 2u) (each square one rounding, the sum one more); sqrtf halves that and rounds:
    (1 + 2u); s = R / that: (1 + 3u); V * s: each component within (1 + 4u) of the vector of length exactly R; the new l2
    <= R^2 (1 + 4u)^2 (1 + 2u) <= R^2 (1 + 11u), and R2 = fl(R * R) >= R^2 (1 - u): l2 <= R2 (1 + 13u)."""
    rng = np.random.default_rng(4)
    m = (rng.uniform(-1, 1, (H, W, 2)) * np.exp2(rng.uniform(-4, 12, (H, W, 1)))).astype(f32)
    for R in (1.0, 7.3, 16.0):
        for shutter in (0.5, 4.0):
            r = M.motion_blur_ref(_image(1), m, _depth(2), _all(), max_blur=R, shutter=shutter, taps=2)
            R2 = float(f32(R) * f32(R))
            for plane in (r["T"][0], r["N"][0]):
                l2 = plane[..., 0].astype(np.float64) ** 2 + plane[..., 1].astype(np.float64) ** 2
                assert (l2 <= R2 * (1 + 13 * U)).all() and l2.max() >= R2 * (1 - 13 * U)


def _sum_bound(taps):
    """out = (c wp + sum) / (wp + Wt) for a constant colour c.  sum: the first term is 0 + c w, exact but for the product; every term then
    passes through at most taps - 1 further additions: <= taps roundings a term, and one more for the addition of c wp (itself one
    product and that addition: 2).  The numerator is c (wp + sum of w) within (taps + 1) u; the denominator wp + Wt is (wp + sum of w)
    within taps u by the same count without the products; the quotient rounds once.  All terms are >= 0, so the relative errors add:
    (taps + 1) + taps + 1 = 2 taps + 2 roundings, and one more for the second-order terms."""
    return (2 * taps + 3) * U


@pytest.mark.parametrize("taps", [1, 8, 12, 64])
def test_a_constant_colour_under_uniform_motion_comes_back(taps):
    c = np.empty((H, W, 4), f32)
    c[:] = (0.7310, 1.9125, 0.0421, 1.0)
    m = np.empty((H, W, 2), f32)
    m[:] = (13.7, -6.1)
    for jitter in (False, True):
        r = M.motion_blur_ref(c, m, _depth(2), _all(), taps=taps, jitter=jitter, seed=5)
        out = r["out"].view(f32)[..., 0:3].astype(np.float64)
        ref = c[..., 0:3].astype(np.float64)
        assert r["moving"] == W * H and r["taps"] > 0
        assert (np.abs(out - ref) <= _sum_bound(taps) * ref).all(), float((np.abs(out - ref) / ref).max() / U)


def test_out_lies_within_the_range_of_the_colours():
    """every weight is >= 0, so out is a weighted mean of colours: within [min, max] per channel up to the bound above on the largest"""
    rng = np.random.default_rng(6)
    c, z = _image(7), _depth(8)
    m = (rng.uniform(-1, 1, (H, W, 2)) * np.exp2(rng.uniform(-2, 7, (H, W, 1)))).astype(f32)
    for taps in (2, 12, 33):
        r = M.motion_blur_ref(c, m, z, _all(), taps=taps, shutter=1.0)
        out = r["out"].view(f32)[..., 0:3].astype(np.float64)
        assert r["moving"] > W * H // 2 and np.isfinite(out).all()
        for ch in range(3):
            lo, hi = float(c[..., ch].min()), float(c[..., ch].max())
            assert out[..., ch].min() >= lo - _sum_bound(taps) * hi and out[..., ch].max() <= hi * (1 + _sum_bound(taps)), (taps, ch)


def _near_rect_scene(moving_near):
    """a near rectangle (depth 2) over a far background (depth 50); one of the two moves by 24 pixels a frame in x"""
    c = np.zeros((H, W, 4), f32)
    c[..., 0:3] = (0.0, 0.25, 0.5)
    c[..., 3] = 1
    z = np.full((H, W), 50.0, f32)
    near = np.zeros((H, W), bool)
    near[12:30, 20:45] = True
    c[near, 0:3] = (1.0, 0.5, 0.125)
    z[near] = 2.0
    m = np.zeros((H, W, 2), f32)
    m[near if moving_near else ~near] = (24.0, 0.0)
    return c, m, z, near


def test_a_static_near_rectangle_keeps_its_bits():
    """shutter 1: |V| = 12 on the background, 0 on the rectangle (lp = 0.5).  With 12 taps the nearest tap is at d = 12 / 12 = 1 >= 0.525:
    cone(lp) = cyl(lp) = 0, and fg = 0 because (zq - zp) / e = 48 / (0.05 * 2) > 1: every weight of a near pixel is 0 or falls on near
    pixels at d >= 1, where both cones and cyl(lp) are 0 as well: Wt == 0 and out = c exactly."""
    c, m, z, near = _near_rect_scene(False)
    r = M.motion_blur_ref(c, m, z, _all(), shutter=1.0, taps=12)
    out = r["out"]
    assert r["moving"] == W * H
    assert np.array_equal(out[near][:, 0:3], c[near][:, 0:3].view(u32))
    assert (out.view(f32)[..., 0] == 0).sum() > 0  # and the background stays free of the rectangle's red except where it gathers it


def test_a_moving_near_rectangle_spreads_within_max_blur_only():
    """shutter 1, max_blur 8: |V| = 8 (12 scaled down).  A static background pixel gathers red (which the background lacks) from a tap on
    the rectangle: fg = 1, cone(lq) = 1 - d / 8 > 0 for d < 8.  Taps reach at most R (1 + 5u) pixels along x and 0 along y, rounded to
    the nearest pixel: no red beyond 8 pixels left or right of the rectangle, none above or below it."""
    c, m, z, near = _near_rect_scene(True)
    r = M.motion_blur_ref(c, m, z, _all(), shutter=1.0, max_blur=8.0, taps=16)
    red = r["out"].view(f32)[..., 0]
    reach = np.zeros((H, W), bool)
    reach[12:30, 20 - 8:45 + 8] = True
    assert (red[~reach] == 0).all()
    assert (red[12:30, 14:20] > 0).all() and (red[12:30, 45:51] > 0).all()
    assert np.array_equal(r["out"][~reach][:, 0:3], c[~reach][:, 0:3].view(u32))


HOSTILE = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF], u32).view(f32)


def test_hostile_words_stay_where_they_are():
    """NaN, +-inf and denormals in each plane, and 3e38 motion of opposite signs: every pixel but those with a bad COLOUR is finite"""
    rng = np.random.default_rng(9)
    c, z = _image(10), _depth(11)
    m = (rng.uniform(-1, 1, (H, W, 2)) * 20).astype(f32)
    pos = rng.permutation(H * W)[:64]
    bad_color = np.zeros(H * W, bool)
    for k, word in enumerate(HOSTILE):
        c.reshape(-1, 4)[pos[k], k % 3] = word
        bad_color[pos[k]] = not np.isfinite(word)
        m.reshape(-1, 2)[pos[8 + k], k % 2] = word
        z.reshape(-1)[pos[16 + k]] = word
    z.reshape(-1)[pos[24:27]] = (0.0, -3.0, 1e-7)
    m.reshape(-1, 2)[pos[27]] = (3e38, -3e38)
    m.reshape(-1, 2)[pos[28]] = (-3e38, 3e38)
    for prm in (dict(), dict(shutter=4.0, taps=5), dict(jitter=True, seed=3, max_blur=3.0)):
        r = M.motion_blur_ref(c, m, z, _all(), **prm)
        out = r["out"].view(f32)[..., 0:3].reshape(-1, 3)
        assert np.isfinite(out[~bad_color]).all() and not np.isfinite(out[bad_color]).all(-1).any()
        assert np.isfinite(r["scratch"].view(f32)).all() and r["unknown"] == 4 and r["nonfinite"] > 0
        assert np.array_equal(r["out"].reshape(-1, 4)[bad_color][:, 0:3], c.reshape(-1, 4)[bad_color][:, 0:3].view(u32))


def test_a_view_puts_nothing_into_its_neighbour():
    """two views side by side; a fast bright region against the seam in the left one: the right view's out is its colour, its T and N zero"""
    h, w = 32, 64
    rects = [(0, 0, 32, 32), (32, 0, 32, 32)]
    c, z = _image(12, h, w), _depth(13, h, w)
    c[8:24, 24:32, 0:3] = 500.0
    m = np.zeros((h, w, 2), f32)
    m[8:24, 24:32] = (-30.0, 4.0)
    r = M.motion_blur_ref(c, m, z, _all(h, w), rects=rects)
    dims, _ = M.layout(rects, h, w)
    first = int(dims[1, 2])
    assert (r["scratch"][2 * first:] == 0).all() and (r["scratch"][:2 * first] != 0).any()
    assert (r["T"][1] == 0).all() and (r["N"][1] == 0).all()
    assert np.array_equal(r["out"][:, 32:, 0:3], c[:, 32:, 0:3].view(u32)) and not np.array_equal(r["out"][:, :32, 0:3], c[:, :32, 0:3].view(u32))
    # without views the same planes bleed across
    r = M.motion_blur_ref(c, m, z, _all(h, w))
    assert not np.array_equal(r["out"][:, 32:, 0:3], c[:, 32:, 0:3].view(u32))
    # and each view holds the bits a frame of its own size holds
    r = M.motion_blur_ref(c, m, z, _all(h, w), rects=rects, jitter=True, seed=2)
    for x0, y0, wr, hr in rects:
        box = (slice(y0, y0 + hr), slice(x0, x0 + wr))
        alone = M.motion_blur_ref(c[box], m[box], z[box], _all(hr, wr), jitter=True, seed=2)
        assert np.array_equal(r["out"][box], alone["out"])


def test_the_jitter():
    y, x = np.mgrid[0:64, 0:64]
    j0, j1 = M.jitter_of(x, y, 0), M.jitter_of(x, y, 1)
    assert j0.dtype == f32 and j0.min() >= -0.5 and j0.max() < 0.5 and (j0 != j1).mean() > 0.99
    assert len(np.unique(j0)) > 4000 and abs(float(j0.mean())) < 0.02
    # the extremes of the mapping: h >> 8 = 0 and 2^24 - 1
    ends = (np.array([0, 0xFFFFFF], u32).astype(f32) * f32(2.0 ** -24) - f32(0.5))
    assert ends[0] == -0.5 and ends[1] == f32(0.5) - f32(2.0 ** -24) and ends[1] < 0.5
    # a function of LOCAL coordinates: a view at (32, 8) jitters its pixel (3, 5) as a frame jitters its own (3, 5)
    assert M.hash32(3, 5, 7) == M.hash32(np.array([3]), np.array([5]), 7)[0]
    assert int(M.hash32(0, 0, 0)) == 0 and int(M.hash32(1, 0, 0)) != int(M.hash32(0, 1, 0))
