"""Lens warp and late reprojection (pt_lens_warp_planes, pt_warp_matrix) without a GPU: the entry points are declared and exported, the
ctypes mirrors match the compiler's layout, the header compiles as C99 and C++17 and states the rule, null arguments are refused before any
device work, both facades have the methods; pt_warp_matrix (host arithmetic) is held against a float64 restatement and against the
cameras' own ray directions; and the float32 NumPy reference (tests/lens_warp_ref.py) is held against float64 on an affine ramp.

This file pins one figure (kept in tests/lens_warp_ref.py) for tests/test_gpu_lens_warp.py, from the references alone — no bound comes from
a kernel's output; profiles/lens_warp.md holds the same figure:

  R_WARP: rms(warp(A) - B) / rms(A - B) over the pixels with .w == 1, bilinear, at 131 x 59 on CPU-built planes of the textured scene.  A is
  the pixel-centre albedo (surface_ref.surface_ref) under the scene's camera, B the same under that camera turned 3 degrees in yaw about its
  own eye (the same rays exist), and warp is the rule with pt_warp_matrix(A's camera, B's camera).  The GPU test asserts
  rms(warp(A) - B) <= ((1 + R_WARP) / 2) * rms(A - B) on the GPU's own planes.  The transposed matrix and the matrix of the opposite yaw
  both miss that bound (shown below)."""
import ctypes as C
import re

import numpy as np
import pytest

import lens_warp_ref as LW
import motion_ref as M
import surface_ref as S
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_section
from lens_warp_ref import INPUTS, R_WARP, YAW, H, W
from optixpathtracer_amd import _lib
from optixpathtracer_amd import renderer as R

f32 = np.float32
VIEW_FIELDS = ("center", "inv_radius", "k", "warp", "reserved")
DESC_FIELDS = ("color", "out", "frame_rgba8", "block_mask", "lenses", "border", "flags")
STATS_FIELDS = ("pixels", "outside", "nonfinite", "kernel_ms")
NAMES = ("pt_lens_warp_planes", "pt_warp_matrix")


def test_library_exports_the_entry_points():
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert name in header().split("VERSIONING.")[1].split("*/")[0]
        assert name in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_lens_warp_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_lens_warp_desc\s*\*\s*\w+\s*,\s*pt_lens_warp_stats\s*\*", src)
    assert re.search(r"int\s+pt_warp_matrix\s*\(\s*const\s+float\s+\w+\[12\]\s*,\s*const\s+float\s+\w+\[12\]\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*float\s+\w+\[9\]\s*\)", src)
    assert b"0.4" in L.pt_version()


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.LensView, "pt_lens_view", VIEW_FIELDS), (_lib.LensWarpDesc, "pt_lens_warp_desc", DESC_FIELDS),
                            (_lib.LensWarpStats, "pt_lens_warp_stats", STATS_FIELDS)],
                 [96, 0, 8, 16, 52, 88] + [56, 0, 8, 16, 24, 32, 40, 52] + [32, 0, 8, 16, 24])
    assert {k: _lib.LENS_WARP_PLANES[k] for k in LW.PLANES} == LW.WORDS and _lib.LENS_WARP_OUTPUTS == LW.PLANES
    assert _lib.PT_LENS_WARP_BICUBIC == 1 and LW.LENS_WORDS * 4 == C.sizeof(_lib.LensView)


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const float* color, float* out, uint32_t* frame, const float* cam0, const float* cam1) {\n"
            "    pt_lens_view v = {{65.5f, 29.5f}, {0.015f, 0.015f}, {{0.1f, 0.05f, 0.0f}, {0.1f, 0.05f, 0.0f}, {0.1f, 0.05f, 0.0f}}, {1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0}};\n"
            "    pt_lens_warp_desc d = {0, 0, 0, 0, 0, {0.0f, 0.0f, 0.0f}, 0u};\n"
            "    pt_lens_warp_stats s;\n"
            "    if (pt_warp_matrix(cam0, cam1, 131u, 59u, v.warp)) return 1;\n"
            "    d.color = color; d.out = out; d.frame_rgba8 = frame; d.lenses = &v;\n"
            "    d.flags = PT_LENS_WARP_BICUBIC;\n"
            "    return pt_lens_warp_planes(c, &d, &s) || s.outside > s.pixels || s.nonfinite > 48 * s.pixels;\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.LensWarpDesc(), _lib.LensWarpStats(7, 7, 7, 7.0)
    assert L.pt_lens_warp_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_lens_warp_planes: null context" in L.pt_last_error(None)
    assert L.pt_lens_warp_planes(None, None, None) == -1
    assert tuple(getattr(s, n) for n in STATS_FIELDS) == (7, 7, 7, 7.0)


def test_facades_have_the_methods(tmp_path):
    import torch  # noqa: F401

    assert callable(getattr(R.SampleRenderer, "lensWarpPlanes", None)) and callable(getattr(R._RankView, "lensWarpPlanes", None))
    assert callable(R.warpMatrix) and callable(R.make_lens)
    r = bare_renderer()
    color = fake_cuda((4, 4, 4))
    with pytest.raises(ValueError, match="color is required"):
        r.lensWarpPlanes(None)
    with pytest.raises(ValueError, match=r"out: a contiguous torch.float32 tensor of shape \(4, 4, 4\) is expected"):
        r.lensWarpPlanes(color, out=fake_cuda((4, 4)))
    with pytest.raises(ValueError, match="lenses must be 1 records of 24 floats"):
        r.lensWarpPlanes(color, out=fake_cuda((4, 4, 4)), lenses=[R.make_lens((4, 4)), R.make_lens((4, 4))])
    with pytest.raises(ValueError, match="border must be three floats"):
        r.lensWarpPlanes(color, out=fake_cuda((4, 4, 4)), border=(0.0, 0.0))
    with pytest.raises(ValueError, match="k is"):
        R.make_lens((4, 4), k=(1.0, 2.0))
    with pytest.raises(ValueError, match="12 floats"):
        R.warpMatrix(np.zeros(11, f32), np.zeros(12, f32), (4, 4))
    # make_lens fills the record the reference's own writer fills
    for kw in (dict(), dict(k=(0.1, 0.05, 0.0)), dict(k=((0.1, 0, 0), (0.2, 0, 0), (0.3, 0.01, -0.02)), center=(3.0, 1.5), radius=(7.0, 5.0), warp=np.arange(9.0)),
               dict(radius=0.0)):
        assert np.array_equal(np.frombuffer(bytes(R.make_lens((131, 59), **kw)), f32).view(np.uint32), LW.lens_row((131, 59), **kw).view(np.uint32)), kw
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t warp(SampleRenderer& sample, pt_lens_warp_desc d, pt_lens_view v, const float* cam0, const float* cam1) {\n"
        "    SampleRenderer::warpMatrix(cam0, cam1, 131u, 59u, v.warp);\n"
        "    d.lenses = &v;\n"
        "    pt_lens_warp_stats s{};\n"
        "    sample.lensWarpPlanes(d, &s);\n"
        "    return sample.lensWarpPlanes(d).outside + s.nonfinite;\n"
        "}\n"
    )


def test_header_states_the_rule():
    text = header_section("LENS WARP AND LATE REPROJECTION", "The acceleration structure as the traversal kernels see it")
    for item in ("exactly pt_modulate_planes's", "nv = max(1, the view count)", "no fused multiply-add", "/ correctly rounded",
                 "px = (float)x + 0.5f; py = (float)y + 0.5f; qx = px - cx; qy = py - cy",
                 "ax = qx * irx; ay = qy * iry; r2 = ax * ax + ay * ay; g = r2 * (k1 + r2 * (k2 + r2 * k3))",
                 "ux = px + qx * g; uy = py + qy * g", "k = 0 gives ux = px bit for bit",
                 "a = (H[0]*ux + H[1]*uy) + H[2]; b = (H[3]*ux + H[4]*uy) + H[5]; c = (H[6]*ux + H[7]*uy) + H[8]",
                 "OUTSIDE unless c > 0", "sx = a / c; sy = b / c", "sx >= 0 && sx <= (float)wr && sy >= 0 && sy <= (float)hr", "a NaN is outside",
                 "No float is converted to int and no address is formed before this test has passed",
                 "fx = sx - 0.5f; fy = sy - 0.5f; flx = floorf(fx); fly = floorf(fy); ix = (int)flx; iy = (int)fly; tx = fx - flx; ty = fy - fly",
                 "each coordinate clamped to the rectangle", "wx = {1.0f - tx, tx}", "w_ij = wx[i] * wy[j]", "exponent-bit test",
                 "stats->nonfinite counts such words", "val = ((c00*w00 + c10*w10) + c01*w01) + c11*w11", "All four taps are always read",
                 "PT_LENS_WARP_BICUBIC, Catmull-Rom, separable", "ix - 1 .. ix + 2 by iy - 1 .. iy + 2",
                 "w0 = ((-0.5f*t + 1.0f)*t - 0.5f)*t; w1 = ((1.5f*t - 2.5f)*t)*t + 1.0f; w2 = ((-1.5f*t + 2.0f)*t + 0.5f)*t; w3 = ((0.5f*t - 0.5f)*t)*t",
                 "row_j = ((c0j*wx0 + c1j*wx1) + c2j*wx2) + c3j*wx3", "val = ((row0*wy0 + row1*wy1) + row2*wy2) + row3*wy3",
                 "border[ch] when outside", "all three inside ? 1.0f : 0.0f", "frame_rgba8[p] = make_color(r, g, b)",
                 "stats->outside counts pixels with .w == 0", "No tap leaves its view's rectangle", "the set decides only what is written",
                 "a -0 that becomes +0", "both outputs null", "any overlap that involves out or frame_rgba8", "an unknown flag bit", "a non-finite border",
                 "inv_radius < 0", "above 1e6", "reserved != 0", "writes no context state",
                 "H = P * [U V W]_src^-1 * [U' V' W']_dst * P^-1", "the eyes are ignored", "the identity exactly", "1e-12 times the product of its column norms",
                 "positional reprojection with the depth plane", "tangential (decentring) terms and mesh-based warps", "vignette compensation",
                 "an asynchronous variant", "a pt_multi_* wrapper"):
        assert item in text, item


# ------------------------------------------------------------------ pt_warp_matrix
def _row(cam, w=W, h=H):
    return R._camera_rows([R.make_camera(cam, w / h)])[0]


TURNS = [(3.0, 0.0, 0.0), (-2.0, 1.5, 0.0), (0.0, -3.0, 0.0), (0.0, 0.0, 4.0), (1.0, -2.0, 3.0), (5.0, 2.0, -1.0)]


def test_warp_matrix_of_equal_cameras_is_the_identity_exactly():
    eye = np.eye(3, dtype=f32).reshape(-1)
    for name in ("cornell", "textured"):
        row = _row(INPUTS[name][1])
        assert np.array_equal(R.warpMatrix(row, row, (W, H)).view(np.uint32), eye.view(np.uint32))
        moved = row.copy()
        moved[0:3] += 5.0  # another eye: ignored
        assert np.array_equal(R.warpMatrix(row, moved, (W, H)).view(np.uint32), eye.view(np.uint32))
    cam = R.make_camera(INPUTS["cornell"][1], W / H)
    assert np.array_equal(R.warpMatrix(cam, cam, (W, H)), eye)  # Cameras are taken as well


@pytest.mark.parametrize("name", ["cornell", "textured"])
def test_warp_matrix_against_float64_and_the_cameras_own_rays(name):
    """Every entry against warp_matrix64 (a linear solve in NumPy; the library inverts by the adjugate): both are float64, so they differ by
    a few 2^-53 of the row's size and their float32 roundings by at most one unit in the last place of the entry, which is at most
    2 x 2^-24 of the row's largest magnitude; 4 x 2^-24 is asserted.  Then the matrix's meaning, in float64: the direction through an
    output pixel under the new camera, expressed in the old camera's U, V, W, lands on the source pixel the float32 matrix names; the
    entries' roundings (2^-24 relative, coordinates below 256) stay below 1e-4 px."""
    cam = INPUTS[name][1]
    src = _row(cam)
    worst_e = worst_px = 0.0
    for yaw, pitch, roll in TURNS:
        dst = _row(LW.turned(cam, yaw, pitch, roll))
        got = R.warpMatrix(src, dst, (W, H)).astype(np.float64).reshape(3, 3)
        want = LW.warp_matrix64(src, dst, W, H)
        err = np.abs(got - want) / np.abs(want).max(1, keepdims=True)
        worst_e = max(worst_e, float(err.max()))
        assert not np.array_equal(got, np.eye(3))
        # a row of pixels and a column of pixels, centres and corners
        px = np.concatenate([np.linspace(0.0, W, 23), np.full(11, 0.37 * W)])
        py = np.concatenate([np.full(23, 0.61 * H), np.linspace(0.0, H, 11)])
        s, d = src.astype(np.float64), dst.astype(np.float64)
        dirs = np.multiply.outer(2 * px / W - 1, d[3:6]) + np.multiply.outer(2 * py / H - 1, d[6:9]) + d[9:12]  # the new camera's rays
        abc = np.linalg.lstsq(np.stack([s[3:6], s[6:9], s[9:12]], 1), dirs.T, rcond=None)[0]  # dirs = a U + b V + c W of the old camera
        assert (abc[2] > 0).all()
        sx, sy = (abc[0] / abc[2] + 1) * W / 2, (abc[1] / abc[2] + 1) * H / 2
        hom = got @ np.stack([px, py, np.ones_like(px)])
        worst_px = max(worst_px, float(np.abs(hom[0] / hom[2] - sx).max()), float(np.abs(hom[1] / hom[2] - sy).max()))
    print(f"{name}: worst entry error {worst_e / 2.0**-24:.3f} x 2^-24 of its row's largest, worst source pixel error {worst_px:.3g} px")
    assert worst_e <= 4 * 2.0**-24 and worst_px <= 1e-4


def test_warp_matrix_refusals():
    L = _lib.load_library()
    row = _row(INPUTS["cornell"][1])
    other = _row(LW.turned(INPUTS["cornell"][1], 3.0))
    out = np.full(9, 7.0, f32)

    def refused(what, src, dst, w, h, o=out):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        assert L.pt_warp_matrix(p(src), p(dst), w, h, p(o)) == -1, what
        assert L.pt_last_error(None).decode().startswith("pt_warp_matrix: "), what
        assert (out == 7.0).all(), what

    refused("null source", None, other, W, H)
    refused("null destination", row, None, W, H)
    refused("null out", row, other, W, H, None)
    refused("zero width", row, other, 0, H)
    refused("zero height", row, other, W, 0)
    for k in (0, 4, 11):
        for bad in (np.nan, np.inf):
            b = row.copy()
            b[k] = bad
            refused(f"source word {k} {bad}", b, other, W, H)
            refused(f"destination word {k} {bad}", row, b, W, H)
    flat = row.copy()
    flat[9:12] = flat[3:6] * f32(2.0) + flat[6:9]  # W in the plane of U and V
    refused("a singular source", flat, other, W, H)
    assert L.pt_warp_matrix(row.ctypes.data, other.ctypes.data, W, H, out.ctypes.data) == 0 and not (out == 7.0).any()


# ------------------------------------------------------------------ the reference against float64 on an affine ramp
RAMP = ((0.004, 0.002, 0.1), (-0.003, 0.005, 0.6), (0.002, -0.004, 0.5))  # (a, b, d) per channel: values in (0, 1.1)
CHROMA_K = ((0.09, 0.05, 0.0), (0.1, 0.05, 0.0), (0.11, 0.05, 0.0))
LENSES = {"barrel": dict(k=(0.1, 0.05, 0.0)), "pincushion": dict(k=(-0.15, 0.02, 0.0)), "per-channel": dict(k=CHROMA_K)}
E_POS = 2e-4  # px, derived in test_reference_against_float64_on_an_affine_ramp's docstring


def _yaw_matrix(name="textured", yaw=YAW):
    cam = INPUTS[name][1]
    return R.warpMatrix(_row(cam), _row(LW.turned(cam, yaw)), (W, H))


@pytest.mark.parametrize("bicubic", [False, True], ids=["bilinear", "bicubic"])
@pytest.mark.parametrize("with_yaw", [False, True], ids=["lens", "lens+yaw"])
@pytest.mark.parametrize("lens", sorted(LENSES))
def test_reference_against_float64_on_an_affine_ramp(lens, with_yaw, bicubic):
    """The colour is c = a (i + 0.5) + b (j + 0.5) + d per channel.  Bilinear interpolation reproduces an affine image, and where the
    clamp folds a tap onto the rectangle's first or last row or column it reproduces the image at the clamped point, so at EVERY inside
    pixel the reference's value must equal the ramp at the source point computed in float64 from the same parameters, that point clamped
    to [0.5, wr - 0.5] x [0.5, hr - 0.5].  Catmull-Rom reproduces affine data too, but not under the clamp: bicubic is checked where the
    source point lies at least 2 px inside.

    The bound, from float32 alone.  Every coordinate is below 256, so a rounding of one costs at most 2^-25 * 256 = 2^-17 = 7.7e-6 px.
    u = p + q * g: g carries six roundings (relative 6 * 2^-24) on |q * g| < 32, 1.2e-5, the product and the sum one rounding each:
    2.2e-5.  a = (H0 u + H1 v) + H2 with |H0| about 1 passes that on and adds four roundings: 5.3e-5.  c is about 1 with four roundings of
    values below 1.3, 3e-7 relative, which a / c turns into 256 * 3e-7 = 8e-5; the division rounds once more: 1.4e-4.  f = s - 0.5 and
    t = f - floor(f) add two roundings: 1.6e-4 < E_POS = 2e-4 px per axis.  The value: the position error times the gradient, (|a| + |b|) *
    E_POS, plus the weights' products and the sum's roundings, eight (bicubic: 32) of relative 2^-24 on values below V = 1.2."""
    row = LW.lens_row((W, H), warp=_yaw_matrix() if with_yaw else None, **LENSES[lens])
    color = LW.affine_ramp(W, H, RAMP)
    assert np.abs(color[..., 0:3]).max() < 1.2
    r = LW.lens_warp_ref(color, [(0, 0, W, H)], [row], np.ones((H, W), bool), bicubic=bicubic)
    x, y = r["X"], r["Y"]
    assert r["pixels"] == W * H and r["nonfinite"] == 0 and r["outside"] <= W * H // 4, r["outside"]
    worst = worst_pos = 0.0
    checked = 0
    for ch, (a, b, d) in enumerate(RAMP):
        sx, sy, c = LW.source_point64(row, W, H, x, y, ch)
        ins = r["inside"][:, ch]
        worst_pos = max(worst_pos, float(np.abs(r["sx"][ins, ch] - sx[ins]).max()), float(np.abs(r["sy"][ins, ch] - sy[ins]).max()))
        # float32 and float64 agree on inside / outside except within E_POS of the rectangle's edge
        clear = (np.minimum(np.minimum(sx, W - sx), np.minimum(sy, H - sy)) > E_POS) & (c > 0)
        assert ins[clear].all() and not ins[(sx < -E_POS) | (sx > W + E_POS) | (sy < -E_POS) | (sy > H + E_POS) | ~(c > 0)].any()
        use = ins & ((np.minimum(np.minimum(sx, W - sx), np.minimum(sy, H - sy)) >= 2.0) if bicubic else True)
        want = a * np.clip(sx, 0.5, W - 0.5) + b * np.clip(sy, 0.5, H - 0.5) + d
        bound = (abs(a) + abs(b)) * E_POS + (32 if bicubic else 8) * 2.0**-24 * 1.2
        err = np.abs(r["rgb"][use, ch].astype(np.float64) - want[use])
        worst = max(worst, float((err / bound).max()))
        checked += int(use.sum())
    print(f"{lens}{' + yaw' if with_yaw else ''}, {'bicubic' if bicubic else 'bilinear'}: outside {r['outside']} of {W * H} ({100 * r['outside'] / (W * H):.1f} %), "
          f"{checked} channel values checked, worst |s - float64| {worst_pos:.3g} px, worst value error {worst:.3f} of its bound")
    assert checked > W * H and worst_pos <= E_POS and worst <= 1.0
    if lens == "per-channel":
        assert (r["sx"][:, 0] != r["sx"][:, 2]).any()
    # .w is 1 exactly where all three channels were inside
    assert np.array_equal(r["out"].view(f32)[..., 3].reshape(-1) == 1, r["inside"].all(1))


def test_identity_returns_the_pixel_itself():
    """steps 1 to 6 at 131 x 59 with k = 0 and the identity: fx == x and fy == y exactly, so out is the colour, a -0 turned into +0"""
    rng = np.random.default_rng(11)
    color = rng.standard_normal((H, W, 4)).astype(f32)
    color[3, 5, 1] = f32(-0.0)
    for lenses in (None, [LW.lens_row((W, H))], [LW.lens_row((W, H), center=(3.0, 50.0), radius=0.0)]):
        r = LW.lens_warp_ref(color, [(0, 0, W, H)], lenses, np.ones((H, W), bool))
        assert np.array_equal(r["sx"][:, 0], r["X"] + f32(0.5)) and np.array_equal(r["sy"][:, 2], r["Y"] + f32(0.5)) and r["outside"] == 0
        out = r["out"].view(f32)
        assert np.array_equal(out[..., 0:3], color[..., 0:3]) and (out[..., 3] == 1).all()
        differ = out[..., 0:3].view(np.uint32) != color[..., 0:3].view(np.uint32)
        assert differ.sum() == 1 and differ[3, 5, 1] and out.view(np.uint32)[3, 5, 1] == 0


# ------------------------------------------------------------------ the meaning: a warped frame is closer to the turned camera's
_CACHE = {}


def albedo_pair(orc, name="textured"):
    """the scene's pixel-centre albedo on CPU-built planes under its camera (A) and under the camera turned YAW degrees (B), and the rows"""
    if name not in _CACHE:
        make, cam = INPUTS[name]
        model = make()
        sc = S.scene_arrays(model)
        res = {}
        for key, c in (("A", cam), ("B", LW.turned(cam, YAW))):
            hit = M.cpu_planes(orc, model, (W, H), c, c)["hit"]
            res[key] = S.surface_ref(hit, sc, np.ones((H, W), bool), planes=("albedo",))["albedo"].view(f32)
            res[key].setflags(write=False)
            res["row" + key] = _row(c)
        _CACHE[name] = res
    return _CACHE[name]


def warp_ratio(A, B, matrix, ok=None):
    """(rms(warp(A) - B) / rms(A - B) over the pixels `ok` — None: those the warp gives .w == 1 —, ok, the count of pixels with .w == 0).
    The two controls are measured over the right rule's pixels: where they are outside they hold the border colour, 0."""
    r = LW.lens_warp_ref(A, [(0, 0, W, H)], [LW.lens_row((W, H), warp=matrix)], np.ones((H, W), bool))
    out = r["out"].view(f32)
    ok = out[..., 3] == 1 if ok is None else ok
    return LW.rms(out[..., 0:3][ok], B[..., 0:3][ok]) / LW.rms(A[..., 0:3][ok], B[..., 0:3][ok]), ok, r["outside"]


def test_warped_albedo_is_closer_to_the_turned_camera(orc_det):
    p = albedo_pair(orc_det)
    A, B = p["A"], p["B"]
    Hm = R.warpMatrix(p["rowA"], p["rowB"], (W, H))
    ratio, ok, outside = warp_ratio(A, B, Hm)
    transposed, _, _ = warp_ratio(A, B, Hm.reshape(3, 3).T.reshape(-1), ok)
    opposite, _, _ = warp_ratio(A, B, R.warpMatrix(p["rowA"], _row(LW.turned(INPUTS["textured"][1], -YAW)), (W, H)), ok)
    bound = (1 + R_WARP) / 2
    print(f"lens warp, {W} x {H}, yaw {YAW}: rms(A - B) {LW.rms(A[..., 0:3], B[..., 0:3]):.6f}, ratio {ratio:.5f}; transposed matrix {transposed:.5f}, "
          f"opposite yaw {opposite:.5f}; bound {bound:.4f}; outside {outside} of {W * H} ({100 * outside / (W * H):.1f} %)")
    assert outside <= W * H // 8
    assert abs(ratio - R_WARP) < 5e-4
    assert ratio <= bound and transposed > bound and opposite > bound
