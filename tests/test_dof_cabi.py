"""Depth of field (pt_dof_layout, pt_dof_planes) without a GPU: the entry points are declared and exported, the ctypes mirrors match the
compiler's layout, the header compiles as C99 and C++17 and states the rule, null arguments are refused before any device work, both
facades check their arguments; and properties of the NumPy reference (tests/dof_ref.py) that pin what the rule means.  No bound here comes
from a kernel's output: each is exact, or derived in the test's own docstring.  u = 2^-24 is float32's unit roundoff."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import dof_ref as M
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_section
from optixpathtracer_amd import _lib

f32 = np.float32
u32 = np.uint32
U = 2.0 ** -24
NAMES = ("pt_dof_layout", "pt_dof_planes")
DESC = ("color", "depth", "out", "scratch", "block_mask", "view_focus", "focus", "aperture", "max_radius", "taps", "seed", "flags")
STATS = ("pixels", "sources", "gathered", "taps", "nonfinite", "kernel_ms")


def test_library_exports_the_entry_points():
    assert all(name in _lib.EXPORTS for name in NAMES)
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NAMES:
        assert hasattr(L, name)
        assert name in header().split("VERSIONING.")[1].split("*/")[0]
        assert name in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_dof_layout\s*\(\s*const\s+pt_ctx\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*size_t\s*\*\s*\w+\s*\)", src)
    assert re.search(r"int\s+pt_dof_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_dof_desc\s*\*\s*\w+\s*,\s*pt_dof_stats\s*\*", src)
    assert b"0.4" in L.pt_version()
    assert _lib.PT_DOF_TILE == 16 == M.TILE and re.search(r"#define\s+PT_DOF_TILE\s+16\b", src)
    assert _lib.PT_DOF_JITTER == 1 == M.JITTER and re.search(r"PT_DOF_JITTER\s*=\s*1\b", src)


def test_struct_layouts_match_the_compiler(tmp_path):
    structs = [(_lib.DofDesc, "pt_dof_desc", DESC), (_lib.DofStats, "pt_dof_stats", STATS)]
    check_layout(tmp_path, structs, [72, 0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 68] + [48, 0, 8, 16, 24, 32, 40])
    assert _lib.DOF_PLANES == {"color": 4, "depth": 1, "out": 4} and _lib.DOF_OUTPUTS == ("out",)


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const float* color, const float* depth, float* out, void* scratch, const float* view_focus) {\n"
            "    pt_dof_desc d = {0, 0, 0, 0, 0, 0, 2.5f, 8.0f, 16.0f, 32u, 0u, PT_DOF_JITTER};\n"
            "    pt_dof_stats s;\n"
            "    uint32_t dims[4];\n"
            "    size_t bytes = 0;\n"
            "    d.color = color; d.depth = depth; d.out = out; d.scratch = scratch; d.view_focus = view_focus;\n"
            "    return pt_dof_layout(c, dims, &bytes) || pt_dof_planes(c, &d, &s) || s.gathered > s.pixels\n"
            "           || s.taps + s.nonfinite > s.gathered * d.taps || s.pixels > s.sources || dims[0] * PT_DOF_TILE == 0u || bytes == 0;\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.DofDesc(), _lib.DofStats(7, 7, 7, 7, 7, 7.0)
    assert L.pt_dof_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_dof_planes: null context" in L.pt_last_error(None)
    assert L.pt_dof_planes(None, None, None) == -1
    assert tuple(getattr(s, n) for n in STATS) == (7, 7, 7, 7, 7, 7.0)
    nbytes = C.c_size_t(77)
    dims = np.full(4, 9, u32)
    assert L.pt_dof_layout(None, dims.ctypes.data, C.byref(nbytes)) == -1
    assert b"pt_dof_layout: null context" in L.pt_last_error(None)
    assert L.pt_dof_layout(None, None, None) == -1
    assert nbytes.value == 77 and (dims == 9).all()


def test_facades_check_their_arguments(tmp_path):
    import torch  # noqa: F401

    from optixpathtracer_amd import renderer as R

    for name in ("dofLayout", "dofPlanes", "dofAperture"):
        assert callable(getattr(R.SampleRenderer, name, None)) and callable(getattr(R._RankView, name, None))
    r = bare_renderer()
    color, depth = fake_cuda((4, 4, 4)), fake_cuda((4, 4))
    good = dict(focus=2.0, aperture=4.0)
    with pytest.raises(ValueError, match="color is required"):
        r.dofPlanes(None, depth, **good)
    with pytest.raises(ValueError, match="depth is required"):
        r.dofPlanes(color, None, **good)
    with pytest.raises(ValueError, match="focus and aperture are required"):
        r.dofPlanes(color, depth, focus=2.0)
    with pytest.raises(ValueError, match="focus and aperture are required"):
        r.dofPlanes(color, depth, aperture=2.0)
    with pytest.raises(ValueError, match=r"color: a contiguous torch.float32 tensor of shape \(4, 4, 4\) is expected"):
        r.dofPlanes(fake_cuda((4, 4, 3)), depth, **good)
    with pytest.raises(ValueError, match=r"depth: a contiguous torch.float32 tensor of shape \(4, 4\) is expected"):
        r.dofPlanes(color, fake_cuda((4, 4, 1)), **good)
    with pytest.raises(ValueError, match=r"out: a contiguous torch.float32 tensor of shape \(4, 4, 4\) is expected"):
        r.dofPlanes(color, depth, out=fake_cuda((4, 4, 3)), **good)
    for bad in (0, 65):
        with pytest.raises(ValueError, match=f"dofPlanes: taps must be 1..64, not {bad}"):
            r.dofPlanes(color, depth, taps=bad, **good)
    for name, bad, text in (("focus", 0.0, r"focus must be in \(0,1e30\]"), ("focus", -1.0, r"focus must be in \(0,1e30\]"),
                            ("focus", 2e30, r"focus must be in \(0,1e30\]"), ("focus", float("nan"), r"focus must be in \(0,1e30\]"),
                            ("aperture", -0.1, r"aperture must be in \[0,4096\]"), ("aperture", 4097.0, r"aperture must be in \[0,4096\]"),
                            ("aperture", float("nan"), r"aperture must be in \[0,4096\]"), ("max_radius", 0.5, r"max_radius must be in \[1,16\]"),
                            ("max_radius", 16.5, r"max_radius must be in \[1,16\]"), ("seed", -1, r"seed must be in \[0,4294967295\]"),
                            ("seed", 2 ** 32, r"seed must be in \[0,4294967295\]")):
        with pytest.raises(ValueError, match="dofPlanes: " + text):
            r.dofPlanes(color, depth, **dict(good, **{name: bad}))
    # the lens: a 50 mm lens at f/2 focused at 2 m on a 24 mm sensor, 1080 rows: A = 25 mm, K = 0.5 * 25 * 50 / 1950 * 45 pixels
    K = R.SampleRenderer.dofAperture(0.050, 2.0, 2.0, 0.024, 1080)
    assert abs(K - 0.5 * 0.025 * 0.050 / 1.950 * 45000.0) < 1e-9 and abs(K - 14.4231) < 1e-3
    with pytest.raises(ValueError, match="focus > focal_length"):
        R.SampleRenderer.dofAperture(0.050, 2.0, 0.050, 0.024, 1080)
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t lens(SampleRenderer& sample, pt_dof_desc d) {\n"
        "    uint32_t dims[4];\n"
        "    const size_t bytes = sample.dofLayout(dims) + sample.dofLayout();\n"
        "    d.aperture = SampleRenderer::dofAperture(0.05f, 2.0f, d.focus, 0.024f, 1080.0f);\n"
        "    pt_dof_stats s{};\n"
        "    sample.dofPlanes(d, &s);\n"
        "    return sample.dofPlanes(d).gathered + s.sources + bytes + dims[3];\n"
        "}\n"
    )


def test_header_states_the_rule():
    text = header_section("DEPTH OF FIELD (no reference counterpart)", "The acceleration structure as the traversal kernels see it")
    for item in ("tile maximum, neighbourhood maximum, then a variable gather", "K = 0.5 * A * f / (s - f) * px_per_unit",
                 "the blur-circle RADIUS in pixels of a point at infinity", "Autofocus is the caller's", "nv = max(1, the view count)",
                 "tw = (wr + 15) / 16 by th = (hr + 15) / 16", "anchored at the rectangle's origin", "No tap and no tile neighbour ever leaves its rectangle",
                 "a view holds the bits a context of its own size would hold", "a plane T of tw * th floats of 4 bytes", "then a plane N of the same size",
                 "tw, th, the index of T's first 4-byte texel and the index of N's", "The tile pass reads EVERY pixel of every rectangle from depth",
                 "the set decides only which pixels of out are written", "exactly pt_modulate_planes's", "all-gather colour and depth first",
                 "The whole scratch is written by every call, also with an empty set", "K = aperture + 0.0f", "R = max_radius", "PI = 3.14159274f",
                 "Fv = view_focus ? view_focus[v] : focus", "Z(d) = (d > 1e-6f && d <= FLT_MAX) ? d : FLT_MAX", "r = K * fabsf(1.0f - Fv / z); r = r < R ? r : R",
                 "Fv / z cannot overflow", "T(i, j) = max r over the pixels of tile (i, j) that lie inside the rectangle",
                 "independent of the order of the reduction", "N(i, j) = max T over the 3 x 3 tiles around (i, j) that exist",
                 "Because R <= PT_DOF_TILE nothing farther away can reach the tile", "rN = N(x / 16, y / 16)",
                 "If rN > 0.5f is false, or a word of c is not finite (exponent-bit test): out[p] = (c, 1.0f), raw", "stats->gathered counts p",
                 "rp = r(p); zp = Z(depth[p]); area(r) = max((r * r) * PI, 1.0f); wp = 1.0f / area(rp)", "At = ((rN * rN) * PI) / (float)taps",
                 "rho = sqrtf(((float)i + 0.5f) / (float)taps); d = rN * rho", "qx = (int)floorf(((float)x + d * D[i + k0].x) + 0.5f), clamped to [0, wr - 1]",
                 "clamped to [0, hr - 1]", "rq = r(q); zq = Z(depth[q])", "re = zq > zp ? rp : rq", "cov = clamp01((re - d) + 0.5f); w = (cov * At) / area(re)",
                 "If w > 0 is false the tap is done: its colour is never looked at", "the tap is skipped and stats->nonfinite counts it",
                 "sum = sum + color[q].xyz * w per component; Wt = Wt + w; stats->taps counts it", "If Wt == 0: out[p].xyz = c exactly",
                 "out[p].xyz = (c * wp + sum) / (wp + Wt) per component", "out[p].w = 1.0f", "D[0] = (1, 0)",
                 "D[n + 1] = (D[n].x * C - D[n].y * S, D[n].x * S + D[n].y * C)", "C = -0x1.79886ap-1f", "0xBF3CC435", "S = 0x1.59d9dep-1f", "0x3F2CECEF",
                 "the golden angle pi (3 - sqrt 5)", "the norm drifts by less than 3e-6", "k0 = h & 63", "the LOCAL coordinates",
                 "h = ((uint32_t)x * 0x9E3779B1u) ^ ((uint32_t)y * 0x85EBCA77u) ^ (seed * 0xC2B2AE3Du)",
                 "h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16", "x = x > 0 ? x : 0; x = x < 1 ? x : 1", "no fused multiply-add",
                 "with T and N all +0", "rN * sqrtf(0.5f / taps) >= 0.5", "at most ceil(rq + 0.5) pixels outside its edge", "out may NOT be color",
                 "flag bits other than PT_DOF_JITTER", "focus, or any view_focus[v], not finite or outside (0, 1e30]", "aperture not finite or outside [0, 4096]",
                 "max_radius not finite or outside [1, PT_DOF_TILE]", "taps outside 1 .. 64", "writes no context state", "hexagonal or cat-eye bokeh",
                 "a separate near-field layer", "sub-pixel (bilinear) taps", "a half-resolution pre-filter", "per-view apertures", "an asynchronous variant",
                 "a pt_multi_* wrapper"):
        assert item in text, item


# ------------------------------------------------------------------ the layout
@pytest.mark.parametrize("size, grid", [((1, 1), (1, 1)), ((16, 16), (1, 1)), ((17, 16), (2, 1)), ((33, 49), (3, 4))])
def test_layout_sizes(size, grid):
    w, h = size
    dims, nbytes = M.layout(None, h, w)
    n = grid[0] * grid[1]
    assert dims.tolist() == [[grid[0], grid[1], 0, n]] and nbytes == 8 * n


def test_layout_under_two_views_of_odd_sizes():
    """view after view, T then N: 17 x 33 has 2 x 3 tiles, 31 x 5 has 2 x 1"""
    dims, nbytes = M.layout([(0, 0, 17, 33), (24, 8, 31, 5)], 48, 64)
    assert dims.tolist() == [[2, 3, 0, 6], [2, 1, 12, 14]] and nbytes == 4 * 16


# ------------------------------------------------------------------ the directions
def test_the_direction_table():
    """D[1] = (C, S) exactly (1 * C - 0 * S and 1 * S + 0 * C are exact); D[2] from four float32 products and two sums; D[127] by the same
    recurrence written with scalars.  The norm stays within 3e-6 of 1 and D[n] within 1e-4 of the exact direction n golden angles on."""
    D = M.directions()
    Cf, Sf = np.array([0xBF3CC435, 0x3F2CECEF], u32).view(f32)
    ga = math.pi * (3.0 - math.sqrt(5.0))
    assert f32(math.cos(ga)).view(u32) == 0xBF3CC435 and f32(math.sin(ga)).view(u32) == 0x3F2CECEF
    assert float(Cf).hex() == "-0x1.79886a0000000p-1" and float(Sf).hex() == "0x1.59d9de0000000p-1"
    assert D.dtype == f32 and D.shape == (128, 2) and D[0].tolist() == [1.0, 0.0]
    assert D[1].view(u32).tolist() == [0xBF3CC435, 0x3F2CECEF]
    d2 = np.array([f32(Cf * Cf) - f32(Sf * Sf), f32(Cf * Sf) + f32(Sf * Cf)], f32)
    assert D[2].view(u32).tolist() == d2.view(u32).tolist()
    x, y = f32(1.0), f32(0.0)
    for _ in range(127):
        x, y = f32(f32(x * Cf) - f32(y * Sf)), f32(f32(x * Sf) + f32(y * Cf))
    assert D[127].view(u32).tolist() == [int(x.view(u32)), int(y.view(u32))]
    norm = np.hypot(D[:, 0].astype(np.float64), D[:, 1].astype(np.float64))
    assert np.abs(norm - 1).max() < 3e-6
    n = np.arange(128)
    assert np.abs(D[:, 0] - np.cos(n * ga)).max() < 1e-4 and np.abs(D[:, 1] - np.sin(n * ga)).max() < 1e-4


def test_the_jitter():
    y, x = np.mgrid[0:64, 0:64]
    k0, k1 = M.jitter_of(x, y, 0), M.jitter_of(x, y, 1)
    assert k0.min() == 0 and k0.max() == 63 and len(np.unique(k0)) == 64 and (k0 != k1).mean() > 0.95
    # a function of LOCAL coordinates and the seed
    assert M.hash32(3, 5, 7) == M.hash32(np.array([3]), np.array([5]), 7)[0] and int(M.hash32(0, 0, 0)) == 0
    # and a rotation of the pattern: D[i + k] is D[i] turned by k golden angles, up to the recurrence's drift
    D = M.directions().astype(np.float64)
    ga = math.pi * (3.0 - math.sqrt(5.0))
    for k in (1, 17, 63):
        c, s = math.cos(k * ga), math.sin(k * ga)
        turned = np.stack([D[:64, 0] * c - D[:64, 1] * s, D[:64, 0] * s + D[:64, 1] * c], -1)
        assert np.abs(D[k:k + 64] - turned).max() < 1e-4
    # it changes which pixels a pixel gathers, and nothing else
    c, z = _image(1), _depth(2)
    a = M.dof_ref(c, z, _all(), focus=3.0, aperture=6.0, taps=8, jitter=True, seed=4)
    b = M.dof_ref(c, z, _all(), focus=3.0, aperture=6.0, taps=8)
    assert np.array_equal(a["scratch"], b["scratch"]) and a["gathered"] == b["gathered"] and not np.array_equal(a["out"], b["out"])


# ------------------------------------------------------------------ properties of the reference
W, H = 67, 41


def _all(h=H, w=W):
    return np.ones((h, w), bool)


def _image(seed, h=H, w=W):
    rng = np.random.default_rng(seed)
    c = (np.exp2(rng.uniform(-6, 4, (h, w, 1))) * rng.uniform(0.4, 1.0, (h, w, 3))).astype(f32)
    return np.concatenate([c, np.ones((h, w, 1), f32)], -1)


def _depth(seed, h=H, w=W, lo=0.1, hi=100.0, focus=3.0):
    """depths spread from lo to hi times the focus, log-uniform"""
    return (focus * np.exp(np.random.default_rng(seed).uniform(np.log(lo), np.log(hi), (h, w)))).astype(f32)


def _is_color(r, c):
    out = r["out"]
    return np.array_equal(out[..., 0:3], np.ascontiguousarray(c[..., 0:3]).view(u32)) and (out.view(f32)[..., 3] == 1).all()


@pytest.mark.parametrize("case", ["aperture 0", "aperture -0", "depth equals focus"])
def test_a_closed_lens_and_a_flat_scene_give_the_colour_back(case):
    c, z = _image(1), _depth(2)
    aperture = 8.0
    if case == "aperture 0":
        aperture = 0.0
    if case == "aperture -0":
        aperture = -0.0
    if case == "depth equals focus":
        z = np.full((H, W), 3.0, f32)
    r = M.dof_ref(c, z, _all(), focus=3.0, aperture=aperture)
    assert _is_color(r, c) and (r["scratch"] == 0).all()  # +0: not a sign bit among them
    assert r["gathered"] == 0 and r["taps"] == 0 and r["nonfinite"] == 0 and r["sources"] == W * H == r["pixels"]


def test_radii_stay_within_max_radius():
    """r = min(K |1 - F / z|, R) with K >= 0: in [0, R] by construction, and R itself is reached where the lens allows it.  N is a maximum
    over a set that holds the tile's own T."""
    z = _depth(4)
    z.reshape(-1)[::97] = np.inf
    for R in (1.0, 7.3, 16.0):
        for K in (0.3, 3.0, 4096.0):
            r = M.dof_ref(_image(1), z, _all(), focus=3.0, aperture=K, max_radius=R, taps=2)
            for plane in (r["r"][0], r["T"][0], r["N"][0]):
                assert (plane >= 0).all() and (plane <= f32(R)).all() and not np.signbit(plane).any()
            assert (r["N"][0] >= r["T"][0]).all()
            if K >= 3.0:
                assert r["T"][0].max() == f32(R)
            if K == 0.3:  # the far limit is K itself: nothing above 0.5 but what is nearer than F / (1 + 0.5 / K)
                assert (r["r"][0][z > 3.0] <= f32(0.3)).all()


def _sum_bound(taps):
    """out = (c wp + sum) / (wp + Wt) for a constant colour c.  sum: the first term is 0 + c w, exact but for the product; every term then
    passes through at most taps - 1 further additions: <= taps roundings a term, and one more for the addition of c wp (itself one
    product and that addition: 2).  The numerator is c (wp + sum of w) within (taps + 1) u; the denominator wp + Wt is (wp + sum of w)
    within taps u by the same count without the products; the quotient rounds once.  All terms are >= 0, so the relative errors add:
    (taps + 1) + taps + 1 = 2 taps + 2 roundings, and one more for the second-order terms."""
    return (2 * taps + 3) * U


@pytest.mark.parametrize("taps", [1, 8, 48, 64])
def test_a_constant_colour_comes_back(taps):
    c = np.empty((H, W, 4), f32)
    c[:] = (0.7310, 1.9125, 0.0421, 1.0)
    for jitter in (False, True):
        r = M.dof_ref(c, _depth(2), _all(), focus=3.0, aperture=9.0, taps=taps, jitter=jitter, seed=5)
        out = r["out"].view(f32)[..., 0:3].astype(np.float64)
        ref = c[..., 0:3].astype(np.float64)
        assert r["gathered"] == W * H and r["taps"] > 0
        assert (np.abs(out - ref) <= _sum_bound(taps) * ref).all(), float((np.abs(out - ref) / ref).max() / U)


def test_out_lies_within_the_range_of_the_colours():
    """every weight is >= 0, so out is a weighted mean of colours: within [min, max] per channel up to the bound above on the largest"""
    c, z = _image(7), _depth(8)
    for taps in (2, 16, 33):
        r = M.dof_ref(c, z, _all(), focus=3.0, aperture=12.0, taps=taps)
        out = r["out"].view(f32)[..., 0:3].astype(np.float64)
        assert r["gathered"] == W * H and np.isfinite(out).all() and r["taps"] > W * H
        for ch in range(3):
            lo, hi = float(c[..., ch].min()), float(c[..., ch].max())
            assert out[..., ch].min() >= lo - _sum_bound(taps) * hi and out[..., ch].max() <= hi * (1 + _sum_bound(taps)), (taps, ch)


def _rect_scene(z_rect, z_back):
    """a rectangle at depth z_rect over a background at z_back; the rectangle is orange, the background has no red at all"""
    c = np.zeros((H, W, 4), f32)
    c[..., 0:3] = (0.0, 0.25, 0.5)
    c[..., 3] = 1
    z = np.full((H, W), z_back, f32)
    rect = np.zeros((H, W), bool)
    rect[12:30, 20:45] = True
    c[rect, 0:3] = (1.0, 0.5, 0.0)
    z[rect] = z_rect
    return c, z, rect


@pytest.mark.parametrize("taps", [8, 16, 48, 64])
def test_a_sharp_foreground_keeps_its_bits(taps):
    """the rectangle at the focus distance (rp = 0) in front of a background of radius 11.25 * (1 - 2 / 50) = 10.8.  A tap of a rectangle
    pixel that lands on the background is behind it: re = rp = 0; one that lands on the rectangle has zq == zp: re = rq = 0.  Either way
    cov = clamp01(0.5 - d) = 0 once d >= 0.5, and the nearest tap is at d = rN sqrtf(0.5 / taps) = 0.95 at 64 taps: Wt == 0, out = c."""
    c, z, rect = _rect_scene(2.0, 50.0)
    r = M.dof_ref(c, z, _all(), focus=2.0, aperture=11.25, taps=taps)
    rN = float(r["N"][0].max())
    assert abs(rN - 10.8) < 1e-4 and (r["N"][0] == r["N"][0].max()).all() and rN * math.sqrt(0.5 / taps) >= 0.5
    assert r["gathered"] == W * H and (r["r"][0][rect] == 0).all()
    assert np.array_equal(r["out"][rect][:, 0:3], c[rect][:, 0:3].view(u32))
    # the background around it is blurred, but takes none of the rectangle's red: those taps are in front of it and have r = 0
    assert (r["out"].view(f32)[..., 0][~rect] == 0).all() and r["taps"] > 0


def test_a_blurred_foreground_spreads_by_its_own_radius_only():
    """the background at the focus distance (r = 0), the rectangle in front with rq = 0.7 * |1 - 10 / 1| = 6.3.  A background pixel takes
    red from a tap on the rectangle only where cov > 0: d < rq + 0.5.  The tap lies within d of the pixel (the directions' norm is 1 within
    3e-6) and is rounded to the nearest pixel, so per axis the integer offset is < rq + 1 + 1e-4: at most ceil(rq + 0.5) = 7 pixels outside
    the rectangle's edge.  Farther out a background pixel's taps all have re = 0 and d >= rN sqrtf(0.5 / 16) = 1.1: it keeps its bits.
    Inside the edge a rectangle pixel sees the background through its own blur (re = rp): its red falls below 1."""
    c, z, rect = _rect_scene(1.0, 10.0)
    r = M.dof_ref(c, z, _all(), focus=10.0, aperture=0.7, taps=16)
    rq = float(r["r"][0][rect].max())
    assert abs(rq - 6.3) < 1e-5 and (r["r"][0][~rect] == 0).all()
    reach = math.ceil(rq + 0.5)
    assert reach == 7
    red = r["out"].view(f32)[..., 0]
    near = np.zeros((H, W), bool)
    near[12 - reach:30 + reach, 20 - reach:45 + reach] = True
    assert (red[~near] == 0).all() and np.array_equal(r["out"][~near][:, 0:3], c[~near][:, 0:3].view(u32))
    assert (red[12:30, 19] > 0).all() and (red[12:30, 45] > 0).all() and (red[11, 20:45] > 0).all()
    assert (red[rect] <= 1).all() and (red[12:30, 20] < 1).all() and (red[12:30, 44] < 1).all() and red[21, 32] > 0.99


HOSTILE = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0x80000000], u32).view(f32)


def test_hostile_words_stay_where_they_are():
    """NaN, +-inf, denormals, FLT_MAX and -0 in each plane, and 0, negative and tiny depths: every pixel but those with a bad COLOUR is
    finite, a bad colour comes back raw, and T and N are finite"""
    rng = np.random.default_rng(9)
    c, z = _image(10), _depth(11)
    pos = rng.permutation(H * W)[:64]
    bad_color = np.zeros(H * W, bool)
    for k, word in enumerate(HOSTILE):
        if k != 6:  # (FLT_MAX is a finite colour, but FLT_MAX * w summed with others need not stay finite: depth only)
            c.reshape(-1, 4)[pos[k], k % 3] = word
            bad_color[pos[k]] = not np.isfinite(word)
        z.reshape(-1)[pos[16 + k]] = word
    z.reshape(-1)[pos[24:27]] = (0.0, -3.0, 1e-7)
    for prm in (dict(aperture=12.0), dict(aperture=4096.0, taps=5), dict(aperture=3.0, jitter=True, seed=3, max_radius=3.0)):
        r = M.dof_ref(c, z, _all(), focus=3.0, **prm)
        out = r["out"].view(f32)[..., 0:3].reshape(-1, 3)
        assert np.isfinite(out[~bad_color]).all() and not np.isfinite(out[bad_color]).all(-1).any()
        assert np.isfinite(r["scratch"].view(f32)).all() and r["nonfinite"] > 0
        assert np.array_equal(r["out"].reshape(-1, 4)[bad_color][:, 0:3], c.reshape(-1, 4)[bad_color][:, 0:3].view(u32))


def test_views_stand_alone_and_focus_on_their_own():
    """two views side by side; a strongly blurred bright region against the seam in the left one: the right view, all in focus, keeps its
    colour and its T and N are zero; each view holds the bits a frame of its own size holds; with view_focus each uses its own distance"""
    h, w = 32, 64
    rects = [(0, 0, 32, 32), (32, 0, 32, 32)]
    c = _image(12, h, w)
    z = np.full((h, w), 4.0, f32)
    c[8:24, 24:32, 0:3] = 500.0
    z[8:24, 24:32] = 0.5
    r = M.dof_ref(c, z, _all(h, w), rects=rects, focus=4.0, aperture=3.0)
    dims, _ = M.layout(rects, h, w)
    first = int(dims[1, 2])
    assert (r["scratch"][first:] == 0).all() and (r["scratch"][:first] != 0).any()
    assert np.array_equal(r["out"][:, 32:, 0:3], c[:, 32:, 0:3].view(u32)) and not np.array_equal(r["out"][:, :32, 0:3], c[:, :32, 0:3].view(u32))
    # without views the same planes bleed across
    r = M.dof_ref(c, z, _all(h, w), focus=4.0, aperture=3.0)
    assert not np.array_equal(r["out"][:, 32:, 0:3], c[:, 32:, 0:3].view(u32))
    z = _depth(13, h, w)
    focus = [0.7, 40.0]
    r = M.dof_ref(c, z, _all(h, w), rects=rects, aperture=5.0, jitter=True, seed=2, taps=9, view_focus=focus)
    for (x0, y0, wr, hr), F in zip(rects, focus):
        box = (slice(y0, y0 + hr), slice(x0, x0 + wr))
        alone = M.dof_ref(c[box], z[box], _all(hr, wr), aperture=5.0, jitter=True, seed=2, taps=9, focus=F)
        assert np.array_equal(r["out"][box], alone["out"])
    same = M.dof_ref(c, z, _all(h, w), rects=rects, aperture=5.0, jitter=True, seed=2, taps=9, focus=0.7)
    assert np.array_equal(same["out"][:, :32], r["out"][:, :32]) and not np.array_equal(same["out"][:, 32:], r["out"][:, 32:])
