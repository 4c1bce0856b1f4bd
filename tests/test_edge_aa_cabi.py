"""Geometric edge antialiasing (pt_edge_aa_planes) without a GPU: the entry point is declared and exported, the ctypes mirrors match the
compiler's layout, the header compiles as C99 and C++17 and states the rule, null arguments are refused before any device work, both facades
have the method; and the float32 NumPy reference (tests/edge_aa_ref.py) is held against a float64 restatement of the crossing (s and b_r)
on CPU-built planes (motion_ref.cpu_planes) of the Cornell box and of the textured scene.

This file pins one figure (kept in tests/edge_aa_ref.py) for tests/test_gpu_edge_aa.py, from the references alone — no bound comes from a kernel's output;
profiles/edge_aa.md holds the same figure:

  R_EDGE: rms(reference output - truth) / rms(colour - truth) over the whole 131 x 59 frame of the Cornell box, on CPU-built planes.  The
  colour is the pixel-centre albedo (surface_ref.surface_ref); the truth is the same albedo on a CPU hit plane of 8 * 131 x 8 * 59 pixels
  under the same camera, box-averaged 8 x 8 (the ray formula makes such a block tile its pixel exactly).  The GPU test asserts
  rms(out - truth) <= ((1 + R_EDGE) / 2) * rms(colour - truth) on the GPU's own planes.  The rule with the owner inverted and the rule with
  every weight forced to 0 both miss that bound (shown below)."""
import ctypes as C
import re

import numpy as np
import pytest

import edge_aa_ref as E
import motion_ref as M
import surface_ref as S
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_section
from edge_aa_ref import INPUTS, R_EDGE, SUPER, H, W, supersampled_truth
from gbuffer_ref import _row
from optixpathtracer_amd import _lib

f32 = np.float32
DESC_FIELDS = ("color", "hit", "position", "out", "edge", "frame_rgba8", "block_mask", "normal_cos", "plane_eps", "flags")
STATS_FIELDS = ("pixels", "hits", "stale", "boundary", "blended", "kernel_ms")
NAME = "pt_edge_aa_planes"


def test_library_exports_the_entry_point():
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert NAME in _lib.EXPORTS and hasattr(L, NAME)
    assert NAME in header().split("VERSIONING.")[1].split("*/")[0]
    assert NAME in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_edge_aa_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_edge_aa_desc\s*\*\s*\w+\s*,\s*pt_edge_aa_stats\s*\*", src)
    assert b"0.4" in L.pt_version()


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.EdgeAaDesc, "pt_edge_aa_desc", DESC_FIELDS), (_lib.EdgeAaStats, "pt_edge_aa_stats", STATS_FIELDS)],
                 [72, 0, 8, 16, 24, 32, 40, 48, 56, 60, 64] + [48, 0, 8, 16, 24, 32, 40])
    assert {k: _lib.EDGE_AA_PLANES[k] for k in E.PLANES} == E.WORDS and _lib.EDGE_AA_OUTPUTS == E.PLANES


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const float* color, const void* hit, const float* position, float* out, float* edge, uint32_t* frame) {\n"
            "    pt_edge_aa_desc d = {0, 0, 0, 0, 0, 0, 0, 0.9f, 0.01f, 0u};\n"
            "    pt_edge_aa_stats s;\n"
            "    d.color = color; d.hit = hit; d.position = position; d.out = out; d.edge = edge; d.frame_rgba8 = frame;\n"
            "    d.flags = PT_EDGE_AA_RESERVED;\n"
            "    return pt_edge_aa_planes(c, &d, &s) || s.blended > s.boundary || s.hits + s.stale > s.pixels;\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.EdgeAaDesc(), _lib.EdgeAaStats(7, 7, 7, 7, 7, 7.0)
    assert L.pt_edge_aa_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_edge_aa_planes: null context" in L.pt_last_error(None)
    assert L.pt_edge_aa_planes(None, None, None) == -1
    assert tuple(getattr(s, n) for n in STATS_FIELDS) == (7, 7, 7, 7, 7, 7.0)


def test_facades_have_the_method(tmp_path):
    import torch  # noqa: F401

    from optixpathtracer_amd import renderer as R

    assert callable(getattr(R.SampleRenderer, "edgeAaPlanes", None)) and callable(getattr(R._RankView, "edgeAaPlanes", None))
    r = bare_renderer()
    color, hit, position = fake_cuda((4, 4, 4)), fake_cuda((4, 4, 8)), fake_cuda((4, 4, 4))
    with pytest.raises(ValueError, match="hit is required"):
        r.edgeAaPlanes(color, None, position)
    with pytest.raises(ValueError, match="color is required"):
        r.edgeAaPlanes(None, hit, position)
    with pytest.raises(ValueError, match=r"edge: a contiguous torch.float32 tensor of shape \(4, 4, 2\) is expected"):
        r.edgeAaPlanes(color, hit, position, out=fake_cuda((4, 4, 4)), edge=fake_cuda((4, 4)))
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t aa(SampleRenderer& sample, pt_edge_aa_desc d) {\n"
        "    d.normal_cos = 0.9f;\n"
        "    pt_edge_aa_stats s{};\n"
        "    sample.edgeAaPlanes(d, &s);\n"
        "    return sample.edgeAaPlanes(d).blended + s.boundary;\n"
        "}\n"
    )


def test_header_states_the_rule():
    text = header_section("GEOMETRIC EDGE ANTIALIASING", "The acceleration structure as the traversal kernels see it")
    for item in ("(dx, dy) = (-1, 0), (+1, 0), (0, -1), (0, +1)", "exponent-bit test", "p and q are not both misses", "hit[q].prim == hit[p].prim",
                 "dot3(ng_p, ng_q) >= normal_cos", "fabsf(dot3(ng_p, position[q].xyz - position[p].xyz)) <= plane_eps * hit[p].t",
                 "stats->boundary counts the pixels with at least one candidate", "hit[p].t <= hit[q].t, else q", "q owns",
                 "A stale owner record (prim >= triangles) drops the direction", "d_r = d((float)x_r + 0.5f, (float)y_r + 0.5f)",
                 "t_r = hgt / dot3(n, d_r)", "dropped unless t_r > 0", "P_r = (d_r * t_r) + eye; g = P_r - p0",
                 "u_r = dot3(cross3(g, e2), n) / nn; v_r = dot3(cross3(e1, g), n) / nn", "b_r = ((1.0f - u_r) - v_r, u_r, v_r)",
                 "b_o = (sel_max0((1.0f - u_o) - v_o), sel_max0(u_o), sel_max0(v_o))", "s_i = b_o[i] / (b_o[i] - b_r[i])", "a strict < keeps the first",
                 "a NaN s_i never replaces", "dist = (o is p) ? s : 1.0f - s", "w_k = 0.5f - dist when dist < 0.5f", "a strict > keeps the first",
                 "out[p].xyz = c_p + ((c_q - c_p) * w)", "edge[p] = (w, (float)(k + 1))", "stats->blended counts these",
                 "frame_rgba8[p] = make_color(out[p].xyz)", "before any address is formed from it", "None of them faults",
                 "out, edge and frame_rgba8 may overlap nothing", "flags != 0", "writes no context state", "a pt_multi_* wrapper", "an asynchronous variant",
                 "sub-pixel triangles", "blending with more than one neighbour"):
        assert item in text, item


# ------------------------------------------------------------------ the reference on CPU-built planes
_CACHE = {}


def cpu_case(orc, name):
    """the scene's CPU-built planes at W x H under its camera, the pixel-centre albedo as the colour, and the reference's result"""
    if name not in _CACHE:
        make, cam = INPUTS[name]
        model = make()
        c = dict(model=model, sc=S.scene_arrays(model), cam=cam, row=_row(cam, W / H))
        P = M.cpu_planes(orc, model, (W, H), cam, cam)
        c["hit"], c["position"] = P["hit"], P["position"]
        c["verts"], c["idx"] = M.model_arrays(model)
        c["color"] = S.surface_ref(c["hit"], c["sc"], np.ones((H, W), bool), planes=("albedo",))["albedo"].view(f32)
        c["ref"] = E.edge_aa_ref(*ref_args(c))
        for k in ("hit", "position", "color"):
            c[k].setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


def ref_args(c, w=W, h=H):
    return (c["hit"], c["position"], c["color"], c["verts"], c["idx"], [(0, 0, w, h)], [c["row"]], np.ones((h, w), bool))


@pytest.mark.parametrize("name", ["cornell", "textured"])
def test_reference_against_a_float64_restatement_of_the_crossing(orc_det, name):
    """Every candidate direction whose owner has a primitive: b_r and s of the reference against float64 geometry that shares no expression
    with the header (least-squares barycentrics of both centre rays' plane points).  The float32 chain t_r -> P_r -> g -> cross -> dot -> / nn
    carries a few roundings of quantities of the scene's size (coordinates up to 8 here, so 2^-21 absolute in g) against edges no shorter
    than 0.3: the barycentrics agree to 2^-21 / 0.3 times a small factor for the chain's length, bounded here by 1e-4 absolute, scaled
    by the barycentric's size where it exceeds 1.  s = b_o / (b_o - b_r) divides by the same denominator in both, so the difference times
    that denominator is bounded likewise — with the reference's own b_o, u and v of the CPU hit plane, in place of float64's."""
    c = cpu_case(orc_det, name)
    r = c["ref"]
    assert r["boundary"] > 300 and 0 < r["blended"] <= r["boundary"] and r["pixels"] == W * H and r["stale"] == 0
    ntri = len(c["idx"])
    checked = crossed = 0
    worst_b = worst_s = 0.0
    for j, k in zip(*np.nonzero(r["cand"])):
        prim = r["oprim"][j, k]
        if not 0 <= prim < ntri:
            continue
        own_p = r["own_p"][j, k]
        x, y = int(r["X"][j]), int(r["Y"][j])
        xr, yr = int(r["xr"][j, k]), int(r["yr"][j, k])
        dx, dy = E.DIRS[k]
        xo, yo = (x, y) if own_p else (x + dx, y + dy)
        assert (xr, yr) == ((x + dx, y + dy) if own_p else (x, y))
        s64, br64 = E.crossing64(c["row"], W, H, c["verts"][c["idx"][prim]], xo, yo, xr, yr)
        br32 = r["b_r"][j, k].astype(np.float64)
        scale = np.maximum(1.0, np.abs(br64))
        worst_b = max(worst_b, float(np.max(np.abs(br32 - br64) / scale)))
        checked += 1
        if np.isfinite(s64) and np.isfinite(r["s"][j, k]) and br64.min() < -1e-3:
            rec = c["hit"][yo, xo]
            bo = np.maximum(np.array([1.0 - float(rec[1]) - float(rec[2]), float(rec[1]), float(rec[2])]), 0.0)
            neg = br64 < 0
            s_own = float(np.min(bo[neg] / (bo[neg] - br64[neg])))  # float64 on the record's own u, v
            den = float(np.min((bo - br64)[neg]))
            worst_s = max(worst_s, abs(float(r["s"][j, k]) - s_own) * den)
            assert abs(s_own - s64) <= 1e-3 / den, (j, k, s_own, s64)  # the record's u, v against the centre ray's: the CPU plane's own error
            crossed += 1
    print(f"{name}: {checked} directions, {crossed} crossings, worst |b_r - float64| {worst_b:.3g}, worst |s - float64| * (b_o - b_r) {worst_s:.3g}")
    assert checked > 300 and crossed > 200 and worst_b <= 1e-4 and worst_s <= 1e-4
    # the weights are in (0, 0.5], the codes 0..4, and 0 exactly where the weight is 0
    e = r["edge"].view(f32)
    assert ((e[..., 0] == 0) == (e[..., 1] == 0)).all() and set(np.unique(e[..., 1]).tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0}
    assert (e[..., 0][e[..., 1] > 0] > 0).all() and (e[..., 0] <= 0.5).all()


def test_reference_output_is_closer_to_the_supersampled_truth(orc_det):
    c = cpu_case(orc_det, "cornell")
    big = M.cpu_planes(orc_det, c["model"], (SUPER * W, SUPER * H), c["cam"], c["cam"])["hit"]
    albedo_big = S.surface_ref(big, c["sc"], np.ones((SUPER * H, SUPER * W), bool), planes=("albedo",))["albedo"].view(f32)
    truth = supersampled_truth(albedo_big)
    col = c["color"][..., 0:3]
    e0 = E.rms(col, truth)
    e1 = E.rms(c["ref"]["out"].view(f32)[..., 0:3], truth)
    far = E.rms(E.edge_aa_ref(*ref_args(c), owner="far")["out"].view(f32)[..., 0:3], truth)
    zero = E.rms(E.edge_aa_ref(*ref_args(c), zero_weight=True)["out"].view(f32)[..., 0:3], truth)
    bound = (1 + R_EDGE) / 2
    print(f"edge aa, {W} x {H}, {SUPER} x {SUPER} truth: rms colour {e0:.6f}, rms output {e1:.6f}, ratio {e1 / e0:.5f}; owner inverted {far / e0:.5f}, "
          f"weights 0 {zero / e0:.5f}; bound {bound:.4f}; boundary {c['ref']['boundary']}, blended {c['ref']['blended']} of {W * H}")
    assert abs(e1 / e0 - R_EDGE) < 5e-4 and R_EDGE <= 0.8
    assert e1 <= bound * e0 and far > bound * e0 and zero > bound * e0
