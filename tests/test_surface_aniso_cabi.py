"""Anisotropic footprint-filtered albedo (pt_surface_aniso_planes) without a GPU: the entry point is declared and exported, the ctypes mirrors
match the compiler's layout, the header compiles as C99 and C++17 and states the rule, null arguments are refused before any device work,
both facades have the method; and the float32 NumPy reference (tests/surface_aniso_ref.py) is held against the two passes it must fall back
to, against a float64 restatement of its tap offsets, and against a float64 supersample of the pixel.

This file pins one figure (kept in tests/surface_aniso_ref.py) for tests/test_gpu_surface_aniso.py, from the references alone, on CPU-built planes of the textured scene's
ground under GRAZING_CAMERA (temporal_ref.cpu_planes through motion_ref.cpu_planes, under the library's own camera) — no bound comes from a kernel's output;
profiles/surface_aniso.md holds the same figure:

  R_ANISO: rms(anisotropic albedo, max_aniso 8 - truth) / rms(isotropic albedo - truth) on ground pixels whose 3 x 3 hit neighbourhood
  lies on the ground mesh, the truth being a 16 x 16 supersample of the pixel in float64 and the isotropic side tests/surface_lod_ref.py.
  The GPU test asserts rms(aniso) <= ((1 + R_ANISO) / 2) * rms(lod) on the GPU's own planes.  The same taps laid along the minor axis and
  the rule with N forced to 1 both miss that bound (shown below)."""
import ctypes as C
import re

import numpy as np
import pytest

import motion_ref as M
import surface_aniso_ref as SA
import surface_lod_ref as SL
import surface_ref as S
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_section
from gbuffer_ref import _row
from optixpathtracer_amd import _lib
from surface_aniso_ref import GRAZING_CAMERA, R_ANISO, H, W, check_hand_made, ground_truth
from surface_lod_ref import ground_pixels, rms_against

f32 = np.float32
DESC_FIELDS = ("hit", "prim_texcoords", "mips", "mips_bytes", "albedo", "texcoord", "footprint", "lod", "block_mask", "footprint_scale", "taps", "max_aniso",
               "flags")
STATS_FIELDS = ("pixels", "hits", "stale", "textured", "minified", "anisotropic", "taps", "kernel_ms")
NAME = "pt_surface_aniso_planes"


def test_library_exports_the_entry_point():
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert NAME in _lib.EXPORTS and hasattr(L, NAME)
    assert NAME in header().split("VERSIONING.")[1].split("*/")[0]
    assert NAME in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_surface_aniso_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_surface_aniso_desc\s*\*\s*\w+\s*,\s*pt_surface_aniso_stats\s*\*", src)


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.SurfaceAnisoDesc, "pt_surface_aniso_desc", DESC_FIELDS), (_lib.SurfaceAnisoStats, "pt_surface_aniso_stats", STATS_FIELDS)],
                 [96, 0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 92] + [64, 0, 8, 16, 24, 32, 40, 48, 56])
    assert _lib.SURFACE_ANISO_PLANES == SA.WORDS and tuple(_lib.SURFACE_ANISO_PLANES) == SA.PLANES
    # the first ten fields are pt_surface_lod_desc's, at its offsets; that struct and its stats keep their layout
    D, Dl = _lib.SurfaceAnisoDesc, _lib.SurfaceLodDesc
    assert [(n, getattr(D, n).offset) for n in DESC_FIELDS[:10]] == [(n, getattr(Dl, n).offset) for n, _ in Dl._fields_[:10]]
    assert C.sizeof(Dl) == 80 and C.sizeof(_lib.SurfaceLodStats) == 48 and _lib.SURFACE_LOD_PLANES == SL.WORDS


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const void* hit, const float* table, void* mips, size_t bytes, float* albedo, float* taps) {\n"
            "    pt_surface_aniso_desc d = {0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0f, 0, 8u, 0u};\n"
            "    pt_surface_aniso_stats s;\n"
            "    d.hit = hit; d.prim_texcoords = table; d.mips = mips; d.mips_bytes = bytes; d.albedo = albedo; d.taps = taps;\n"
            "    d.flags = PT_SURFACE_ANISO_RESERVED;\n"
            "    return pt_surface_aniso_planes(c, &d, &s) || s.anisotropic > s.minified || s.taps < s.textured;\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.SurfaceAnisoDesc(), _lib.SurfaceAnisoStats(7, 7, 7, 7, 7, 7, 7, 7.0)
    assert L.pt_surface_aniso_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_surface_aniso_planes: null context" in L.pt_last_error(None)
    assert L.pt_surface_aniso_planes(None, None, None) == -1
    assert tuple(getattr(s, n) for n in STATS_FIELDS) == (7, 7, 7, 7, 7, 7, 7, 7.0)


def test_facades_have_the_method(tmp_path):
    import torch  # noqa: F401

    from optixpathtracer_amd import renderer as R

    assert callable(getattr(R.SampleRenderer, "surfaceAnisoPlanes", None))
    r = bare_renderer()
    hit = fake_cuda((4, 4, 8))
    with pytest.raises(ValueError, match="unknown plane 'depth'"):
        r.surfaceAnisoPlanes(hit, planes=("depth",))
    with pytest.raises(ValueError, match="`out` names a plane that `planes` does not"):
        r.surfaceAnisoPlanes(hit, planes=("albedo",), out=dict(taps=1))
    with pytest.raises(ValueError, match="no plane asked for"):
        r.surfaceAnisoPlanes(hit, planes=())
    for bad in (0, 17, 2.5, -1):
        with pytest.raises(ValueError, match="max_aniso must be an integer in 1..16"):
            r.surfaceAnisoPlanes(hit, max_aniso=bad)
    with pytest.raises(ValueError, match="hit is required"):
        r.surfaceAnisoPlanes(None)
    with pytest.raises(ValueError, match=r"taps: a contiguous torch.float32 tensor of shape \(4, 4\) is expected"):
        r.surfaceAnisoPlanes(hit, planes=("taps",), out=dict(taps=fake_cuda((4, 4, 2))))
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t aniso(SampleRenderer& sample, pt_surface_aniso_desc d) {\n"
        "    d.max_aniso = 8;\n"
        "    pt_surface_aniso_stats s{};\n"
        "    sample.surfaceAnisoPlanes(d, &s);\n"
        "    return sample.surfaceAnisoPlanes(d).anisotropic + s.taps;\n"
        "}\n"
    )


def test_header_states_the_rule():
    text = header_section("ANISOTROPIC FOOTPRINT-FILTERED ALBEDO", "GUIDED UPSAMPLING")
    for item in ("xm = rx > ry", "a tie takes y", "r_maj2 = xm ? rx : ry; r_min2 = xm ? ry : rx; (a_s, a_t) = xm ? (ds_x, dt_x) : (ds_y, dt_y)",
                 "rho_maj = (ok ? sqrtf(r_maj2) : +infinity) * footprint_scale; rho_min = sqrtf(r_min2) * footprint_scale",
                 "if !(rho_maj > 1.0f) or !ok: N = 1", "q = rho_maj / rho_min; N = (q <= (float)max_aniso) ? (uint)ceilf(q) : max_aniso",
                 "+infinity and NaN take max_aniso", "rho = rho_maj / (float)N", "N = 1: rho_maj itself, no division",
                 "level 0 if !(rho > 1.0f)", "if !(rho < (float)(1 << Lm))", "c = c_k + ((c_k+1 - c_k) * frac)", "lod[p] = (float)k + frac",
                 "o_i = (float)(2i + 1 - N) / (float)(2N)", "(s_i, t_i) = (s + ((o_i * footprint_scale) * a_s), t + ((o_i * footprint_scale) * a_t))",
                 "N = 1: the tap is (s, t) itself, with no arithmetic", "acc = c_0; acc = acc + c_i for i = 1 .. N-1 in order; out = acc / (float)N",
                 "albedo[p] = (out.xyz, 1.0f); taps[p] = (float)N", "taps[p] = 0", "stats->minified counts rho_maj > 1.0f", "stats->anisotropic counts N > 1",
                 "stats->taps is the sum of N over the textured pixels", "symmetric about 0 bit for bit", "lie inside (-0.5, 0.5)",
                 "max_aniso = 1 gives pt_surface_lod_planes's four planes bit for bit",
                 "footprint_scale = 0 gives pt_surface_planes's albedo and texcoord bit for bit", "never from caller memory",
                 "before any address is formed from it", "clamped into their level before a texel is read", "max_aniso 0 or above 16",
                 "the five outputs may overlap nothing", "an elliptical (EWA) weighting of the taps", "anisotropy in the frame path's own lookup",
                 "a pt_multi_* wrapper", "an asynchronous variant"):
        assert item in text, item


# ------------------------------------------------------------------ the tap offsets
def test_tap_offsets_are_symmetric_and_inside_the_footprint():
    for n in range(1, 17):
        o = SA.tap_offsets(n)
        want = (2.0 * np.arange(n) + 1.0) / (2.0 * n) - 0.5  # float64: the centres of n equal pieces of (-0.5, 0.5)
        assert o.dtype == f32 and o.shape == (n,)
        assert np.abs(o.astype(np.float64) - want).max() <= 2.0 ** -26, n  # one rounding, of a quotient inside (-0.5, 0.5): half an ulp there
        assert np.array_equal(o, -o[::-1]), n  # symmetric about 0, bit for bit
        assert (o > f32(-0.5)).all() and (o < f32(0.5)).all() and (np.diff(o) > 0).all(), n
        if n % 2:
            assert o[n // 2] == 0
    assert SA.tap_offsets(1)[0] == 0 and np.array_equal(SA.tap_offsets(2), np.array([-0.25, 0.25], f32))


# ------------------------------------------------------------------ the reference on CPU-built planes
_CACHE = {}


def _args(c, w, h):
    return (c["hit"], c["sc"], c["verts"], c["idx"], [(0, 0, w, h)], [c["row"]], np.ones((h, w), bool))


def grazing_case(orc):
    """the textured scene's CPU-built planes under GRAZING_CAMERA at W x H, with the isotropic reference and the anisotropic one at 8"""
    if "g" not in _CACHE:
        model = S.textured_scene()
        c = dict(model=model, sc=S.scene_arrays(model), cam=GRAZING_CAMERA)
        c["hit"] = M.cpu_planes(orc, model, (W, H), GRAZING_CAMERA, GRAZING_CAMERA)["hit"]
        c["verts"], c["idx"] = M.model_arrays(model)
        c["row"] = _row(GRAZING_CAMERA, W / H)
        c["lod"] = SL.surface_lod_ref(*_args(c, W, H))
        c["aniso"] = SA.surface_aniso_ref(*_args(c, W, H), max_aniso=8)
        _CACHE["g"] = c
    return _CACHE["g"]


def test_reference_at_max_aniso_1_is_the_isotropic_reference(orc_det):
    for c, w, h in ((grazing_case(orc_det), W, H), (SL.cpu_case(orc_det), SL.W, SL.H)):
        one = SA.surface_aniso_ref(*_args(c, w, h), max_aniso=1)
        for name in SL.PLANES:
            assert np.array_equal(one[name], c["lod"][name]), name
        tex = c["lod"]["kind"] == 4
        assert np.array_equal(one["taps"].view(f32)[..., 0], tex.astype(f32))  # one tap on every textured pixel, none elsewhere
        assert (one["hits"], one["stale"], one["textured"], one["minified"]) == tuple(c["lod"][k] for k in ("hits", "stale", "textured", "minified"))
        assert one["anisotropic"] == 0 and one["taps_sum"] == one["textured"] > 1000
        # and the scale multiplies both axes: the pass at another scale and max_aniso 1 is the isotropic pass at that scale
        a, b = SA.surface_aniso_ref(*_args(c, w, h), max_aniso=1, scale=3.7), SL.surface_lod_ref(*_args(c, w, h), scale=3.7)
        assert all(np.array_equal(a[name], b[name]) for name in SL.PLANES)


def test_reference_at_scale_0_is_the_point_lookup(orc_det):
    c = grazing_case(orc_det)
    surface = S.surface_ref(c["hit"], c["sc"], np.ones((H, W), bool))
    for amax in (1, 8, 16):
        point = SA.surface_aniso_ref(*_args(c, W, H), max_aniso=amax, scale=0.0)
        for name in ("albedo", "texcoord"):
            assert np.array_equal(point[name], surface[name]), (amax, name)
        assert not point["lod"].any() and point["minified"] == 0 and point["anisotropic"] == 0 and point["taps_sum"] == point["textured"]
        assert np.array_equal(point["footprint"], c["lod"]["footprint"])


def test_counters_and_planes_of_the_reference(orc_det):
    c = grazing_case(orc_det)
    a = c["aniso"]
    n = a["n"]
    tex = a["kind"] == 4
    assert (n[~tex] == 0).all() and (n[tex] >= 1).all() and n.max() == 8
    assert a["anisotropic"] == int((n > 1).sum()) and a["taps_sum"] == int(n.sum()) and a["minified"] == c["lod"]["minified"]
    assert np.array_equal(a["texcoord"], c["lod"]["texcoord"]) and np.array_equal(a["footprint"], c["lod"]["footprint"])
    lod_a, lod_i = a["lod"].view(f32)[..., 0], c["lod"]["lod"].view(f32)[..., 0]
    assert (lod_a <= lod_i).all() and (lod_a[n > 1] < lod_i[n > 1]).all()  # a footprint N times shorter picks a finer level
    sixteen = SA.surface_aniso_ref(*_args(c, W, H), max_aniso=16)
    assert 8 < sixteen["n"].max() <= 16 and (sixteen["n"] >= n).all()


def _quality(c, w, h, what):
    q = ground_pixels(c["lod"]["mesh"])
    truth = ground_truth(c, w, h, q)
    n = c["aniso"]["n"][q]
    e_iso, e_aniso = rms_against(c["lod"]["albedo"], truth, q), rms_against(c["aniso"]["albedo"], truth, q)
    print(f"quality, {what}: {int(q.sum())} ground pixels, N >= 3 on {float((n >= 3).mean()):.3f} of them (median {int(np.median(n))}), "
          f"rms isotropic {e_iso:.4f}, rms anisotropic {e_aniso:.4f}, ratio {e_aniso / e_iso:.5f}")
    return q, truth, n, e_iso, e_aniso


def test_anisotropic_albedo_of_the_reference_is_closer_to_the_pixel_average(orc_det):
    c = grazing_case(orc_det)
    q, truth, n, e_iso, e_aniso = _quality(c, W, H, "the grazing camera")
    assert q.sum() > 2000 and (n >= 3).mean() >= 0.5  # the input condition: at least half of the interior ground pixels take N >= 3
    r = e_aniso / e_iso
    assert abs(r - R_ANISO) < 5e-4 and R_ANISO <= 0.8
    # teeth: the same taps laid along the minor axis, and the rule with N forced to 1, both miss the GPU test's bound
    bound = ((1 + R_ANISO) / 2) * e_iso
    minor = rms_against(SA.surface_aniso_ref(*_args(c, W, H), max_aniso=8, axis="minor")["albedo"], truth, q)
    forced = rms_against(SA.surface_aniso_ref(*_args(c, W, H), max_aniso=8, force_n=1)["albedo"], truth, q)
    print(f"  along the minor axis {minor:.4f} ({minor / e_iso:.3f} x isotropic), N forced to 1 {forced:.4f} ({forced / e_iso:.3f} x), bound {bound:.4f}")
    assert minor > bound and forced > bound and e_aniso <= bound


def test_anisotropic_albedo_under_the_non_grazing_camera_is_no_worse(orc_det):
    c = dict(SL.cpu_case(orc_det))
    c["aniso"] = SA.surface_aniso_ref(*_args(c, SL.W, SL.H), max_aniso=8)
    q, _, _, e_iso, e_aniso = _quality(c, SL.W, SL.H, "the non-grazing camera")  # measured: see R_ANISO's comment
    assert q.sum() > 2000 and e_aniso <= e_iso


# ------------------------------------------------------------------ the hand-made inputs of the GPU test
def test_hand_made_inputs_place_every_case_of_the_rule():
    model = SA.hand_made_model()
    sc = S.scene_arrays(model)
    verts, idx = SA.hand_made_verts(model)
    hit, where = SA.hand_made_hit()
    assert [t.shape for t in sc["textures"]] == [(8, 16), (3, 5), (1, 1)] and len(idx) == len(SA.HAND_PRIMS)
    frame = np.ones((SA.HAND_H, SA.HAND_W), bool)
    args = (hit, sc, verts, idx, [(0, 0, SA.HAND_W, SA.HAND_H)], [SA.HAND_ROW], frame)
    for amax in (8, 16):
        r = SA.surface_aniso_ref(*args, max_aniso=amax)
        check_hand_made(r["n"], r["lod"].view(f32)[..., 0], where, amax)
        assert r["stale"] == 2 and r["hits"] == 252 and r["taps_sum"] == int(r["n"].sum())
    fp = r["footprint"].view(f32)
    # the fronto-parallel footprints are exact: texcoord differences over 16
    assert (fp[where["q_is_3"]] == np.array([6 / 16, 0, 0, 4 / 16], f32)).all() and (fp[where["q_above_8"]][:, 0] == f32(SA.ABOVE_8) / f32(16)).all()
    assert np.isnan(fp[where["zero_area"]]).all() and np.isfinite(fp[7]).all()
    # the taps of "y_major" span 0.75 of t and those of the records at s = t = 0 reach left of 0: both wrap
    s_t = r["texcoord"].view(f32)
    assert (s_t[0, :len(SA.HAND_PRIMS)] == 0).all()
    one, iso = SA.surface_aniso_ref(*args, max_aniso=1), SL.surface_lod_ref(*args)
    for name in SL.PLANES:
        a, b = one[name], iso[name]
        with np.errstate(all="ignore"):
            assert not ((a != b) & ~(np.isnan(a.view(f32)) & np.isnan(b.view(f32)))).any(), name
