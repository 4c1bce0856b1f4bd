"""Footprint-filtered albedo (pt_texture_mips_layout, pt_copy_texture_mips_device, pt_surface_lod_planes) without a GPU: the entry points are
declared and exported, the ctypes mirrors match the compiler's layout, the header compiles as C99 and C++17 and states the arithmetic, null
arguments are refused before any device work, the layout is the hand-computed one, both facades have the methods; and the float32 NumPy
reference (tests/surface_lod_ref.py) is held against float64 geometry that shares no expression with it.

This file pins two figures (kept in tests/surface_lod_ref.py) for tests/test_gpu_surface_lod.py, both from the reference alone, on CPU-built planes of the textured scene
(test_geometry_cabi.textured_case) — no bound comes from a kernel's output; profiles/surface_lod.md holds the same figures:

  FOOT_MEASURED: the largest |footprint - (texcoord[neighbour] - texcoord[p])| per component, over the pixels whose right (lower)
  neighbour is a textured hit on the same primitive.  FOOT_BOUND is four times that.  The check fails on x/y-swapped and on halved
  footprints (shown below).

  R_REF: rms(filtered albedo - truth) / rms(point albedo - truth) on ground pixels whose 3 x 3 hit neighbourhood lies on the ground mesh,
  the truth being a 16 x 16 supersample of the pixel in float64.  The GPU test asserts rms(lod) <= ((1 + R_REF) / 2) * rms(point) against
  a 256-spp PT_BUF_ALBEDO."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import surface_lod_ref as SL
import surface_ref as S
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_text
from conftest import ROOT
from optixpathtracer_amd import _lib
from surface_lod_ref import FOOT_BOUND, FOOT_MEASURED, R_REF, H, W, check_footprints, cpu_case, ground_pixels, rms_against

f32 = np.float32
DESC_FIELDS = ("hit", "prim_texcoords", "mips", "mips_bytes", "albedo", "texcoord", "footprint", "lod", "block_mask", "footprint_scale", "flags")
STATS_FIELDS = ("pixels", "hits", "stale", "textured", "minified", "kernel_ms")
NEW = ("pt_texture_mips_layout", "pt_copy_texture_mips_device", "pt_surface_lod_planes")


def test_library_exports_the_entry_points():
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert name in header().split("VERSIONING.")[1].split("*/")[0]
    for name in NEW[1:]:
        assert name in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_texture_mips_layout\s*\(\s*const\s+pt_ctx\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*size_t\s*\*\s*\w+\s*\)", src)
    assert re.search(r"int\s+pt_copy_texture_mips_device\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)", src)
    assert re.search(r"int\s+pt_surface_lod_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_surface_lod_desc\s*\*\s*\w+\s*,\s*pt_surface_lod_stats\s*\*", src)


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.SurfaceLodDesc, "pt_surface_lod_desc", DESC_FIELDS), (_lib.SurfaceLodStats, "pt_surface_lod_stats", STATS_FIELDS)],
                 [80, 0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76] + [48, 0, 8, 16, 24, 32, 40])
    assert _lib.SURFACE_LOD_PLANES == SL.WORDS and tuple(_lib.SURFACE_LOD_PLANES) == SL.PLANES
    # pt_surface_planes keeps its layout
    assert _lib.SURFACE_PLANES == S.WORDS and C.sizeof(_lib.SurfaceDesc) == 48 and C.sizeof(_lib.SurfaceStats) == 40


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const void* hit, const float* table, void* mips, float* albedo, float* lod) {\n"
            "    pt_surface_lod_desc d = {0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0f, 0u};\n"
            "    pt_surface_lod_stats s;\n"
            "    uint32_t nt = 0, dims[4];\n"
            "    size_t bytes = 0;\n"
            "    if (pt_texture_mips_layout(c, &nt, nt == 1 ? dims : 0, &bytes) || pt_copy_texture_mips_device(c, mips, bytes)) return -1;\n"
            "    d.hit = hit; d.prim_texcoords = table; d.mips = mips; d.mips_bytes = bytes; d.albedo = albedo; d.lod = lod;\n"
            "    d.flags = PT_SURFACE_LOD_RESERVED;\n"
            "    return pt_surface_lod_planes(c, &d, &s) || s.minified > s.textured;\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.SurfaceLodDesc(), _lib.SurfaceLodStats(7, 7, 7, 7, 7, 7.0)
    assert L.pt_surface_lod_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_surface_lod_planes: null context" in L.pt_last_error(None)
    assert L.pt_surface_lod_planes(None, None, None) == -1
    assert (s.pixels, s.hits, s.stale, s.textured, s.minified, s.kernel_ms) == (7, 7, 7, 7, 7, 7.0)
    nt, nb = C.c_uint32(7), C.c_size_t(7)
    assert L.pt_texture_mips_layout(None, C.byref(nt), None, C.byref(nb)) == -1 and (nt.value, nb.value) == (7, 7)
    assert b"pt_texture_mips_layout: null context" in L.pt_last_error(None)
    assert L.pt_copy_texture_mips_device(None, None, 0) == -1
    assert b"pt_copy_texture_mips_device: null context" in L.pt_last_error(None)


# ------------------------------------------------------------------ the layout
HAND_SIZES = [(64, 32), (48, 40), (1, 1), (1, 7)]
# 64 x 32: 32x16 + 16x8 + 8x4 + 4x2 + 2x1 + 1x1 = 683;  48 x 40: 24x20 + 12x10 + 6x5 + 3x2 + 1x1 = 637 (6 x 5 and 3 x 2: an odd side drops
# its last row / column);  1 x 1: nothing;  1 x 7: 1x3 + 1x1 = 4
HAND_DIMS = [[64, 32, 7, 0], [48, 40, 6, 683], [1, 1, 1, 1320], [1, 7, 3, 1320]]
HAND_BYTES = 16 * 1324


def test_layout_of_hand_computed_sizes(tmp_path):
    dims, nbytes = SL.layout(HAND_SIZES)
    assert dims.tolist() == HAND_DIMS and nbytes == HAND_BYTES
    assert SL.layout([])[1] == 0 and SL.layout([(1, 1), (1, 1)])[1] == 0
    # the library's own layout function (the host part of pt_surface_lod.h, which needs no HIP header)
    src = tmp_path / "layout.cpp"
    flat = ", ".join(str(v) for wh in HAND_SIZES for v in wh)
    src.write_text('#include <cstdio>\n#include "pt_surface_lod.h"\n'
                   f"int main() {{ const int wh[] = {{{flat}}}; uint32_t d[16];\n"
                   '    const uint64_t n = lod_layout(wh, 4, d); for (int k = 0; k < 16; ++k) printf("%u ", d[k]);\n'
                   '    printf("%llu %llu %llu\\n", (unsigned long long)n, (unsigned long long)lod_layout(wh, 0, nullptr), (unsigned long long)lod_layout(wh + 4, 1, nullptr));\n'
                   "    return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "optixpathtracer_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [v for row in HAND_DIMS for v in row] + [1324, 0, 0]


def test_reference_pyramid_on_small_textures():
    # 3 x 2 texels, one channel each for clarity: level 1 is 1 x 1 = ((S00 + S10) + (S01 + S11)) * 0.25, column 2 dropped
    px = np.array([[10, 20, 250], [30, 40, 250]], np.uint32)
    lv = SL.mip_levels(px)
    assert len(lv) == 1 and lv[0].shape == (1, 1, 4)
    S_ = px.astype(f32) / f32(255)
    assert lv[0][0, 0, 0] == ((S_[0, 0] + S_[0, 1]) + (S_[1, 0] + S_[1, 1])) * f32(0.25) and lv[0][0, 0, 1] == 0
    # 1 x 7: level 1 is 1 x 3 with the only column taken twice, row 6 dropped; level 2 is 1 x 1 from rows 0, 1 of level 1
    px = (np.arange(7, dtype=np.uint32) * 30).reshape(7, 1)
    lv = SL.mip_levels(px)
    assert [x.shape for x in lv] == [(3, 1, 4), (1, 1, 4)]
    S_ = px[:, 0].astype(f32) / f32(255)
    assert lv[0][1, 0, 0] == ((S_[2] + S_[2]) + (S_[3] + S_[3])) * f32(0.25)
    assert lv[1][0, 0, 0] == ((lv[0][0, 0, 0] + lv[0][0, 0, 0]) + (lv[0][1, 0, 0] + lv[0][1, 0, 0])) * f32(0.25)
    sc = S.scene_arrays(S.textured_scene())
    assert SL.pyramid(sc["textures"]).shape == (683 + 637, 4)
    assert SL.layout([(t.shape[1], t.shape[0]) for t in sc["textures"]])[0].tolist() == HAND_DIMS[:2]
    # a constant texture stays constant on every level (the sums of four equal values and the quarter are exact)
    const = np.full((40, 48), 0x80402010, np.uint32)
    for x in SL.mip_levels(const):
        assert (x == x[0, 0]).all() and x[0, 0, 0] == f32(0x10) / f32(255)


def test_facades_have_the_methods(tmp_path):
    import torch  # noqa: F401

    from optixpathtracer_amd import renderer as R

    for name in ("textureMipsLayout", "copyTextureMipsDevice", "surfaceLodPlanes"):
        assert callable(getattr(R.SampleRenderer, name, None))
    r = bare_renderer()
    hit = fake_cuda((4, 4, 8))
    with pytest.raises(ValueError, match="unknown plane 'depth'"):
        r.surfaceLodPlanes(hit, planes=("depth",))
    with pytest.raises(ValueError, match="`out` names a plane that `planes` does not"):
        r.surfaceLodPlanes(hit, planes=("albedo",), out=dict(lod=1))
    with pytest.raises(ValueError, match="no plane asked for"):
        r.surfaceLodPlanes(hit, planes=())
    with pytest.raises(ValueError, match="hit is required"):
        r.surfaceLodPlanes(None)
    with pytest.raises(ValueError, match=r"lod: a contiguous torch.float32 tensor of shape \(4, 4\) is expected"):
        r.surfaceLodPlanes(hit, planes=("lod",), out=dict(lod=fake_cuda((4, 4, 2))))
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t lod(SampleRenderer& sample, pt_surface_lod_desc d, void* mips) {\n"
        "    std::vector<uint32_t> dims;\n"
        "    const size_t bytes = sample.textureMipsLayout(&dims);\n"
        "    if (sample.textureMipsLayout() != bytes || dims.size() % 4) return 0;\n"
        "    sample.copyTextureMipsDevice(mips, bytes);\n"
        "    d.mips = mips; d.mips_bytes = bytes;\n"
        "    pt_surface_lod_stats s{};\n"
        "    sample.surfaceLodPlanes(d, &s);\n"
        "    return sample.surfaceLodPlanes(d).minified + s.stale;\n"
        "}\n"
    )


def test_header_states_the_arithmetic():
    text = header_text()
    for item in ("levels = 1 + floor(log2(max(w, h)))", "w_k = max(1, w >> k)", "((S(2i, 2j) + S(i1, 2j)) + (S(2i, j1) + S(i1, j1))) * 0.25f",
                 "i1 = min(2i + 1, w_k - 1); j1 = min(2j + 1, h_k - 1)", "S = (float)byte / 255.0f", "An odd dimension drops its last row or column",
                 "must in addition be 16-byte aligned", "bytes == 0 is a no-op that returns PT_OK", "one blocking copy", "may be made while frames are in flight",
                 "Host work per call on a textured scene",
                 "d(a, b) = ((U * ((2.0f * (a / (float)wr)) - 1.0f)) + (V * ((2.0f * (b / (float)hr)) - 1.0f))) + W",
                 "d_c = d((float)x + 0.5f, (float)y + 0.5f); d_x = d((float)x + 1.5f, (float)y + 0.5f); d_y = d((float)x + 0.5f, (float)y + 1.5f)",
                 "e1 = p1 - p0; e2 = p2 - p0; n = cross3(e1, e2); nn = dot3(n, n); hgt = dot3(n, p0 - eye)",
                 "t_r = hgt / dot3(n, d_r); P_r = (d_r * t_r) + eye", "ok = t_c > 0 && t_x > 0 && t_y > 0",
                 "g = P_r - P_c; du = dot3(cross3(g, e2), n) / nn; dv = dot3(cross3(e1, g), n) / nn",
                 "ds_r = (du * (c[2] - c[0])) + (dv * (c[4] - c[0])); dt_r = (du * (c[3] - c[1])) + (dv * (c[5] - c[1]))",
                 "footprint[p] = (ds_x, dt_x, ds_y, dt_y)", "rho2 = ok ? (rx > ry ? rx : ry) : +infinity", "rho = sqrtf(rho2) * footprint_scale",
                 "if !(rho > 1.0f)", "if !(rho < (float)(1 << Lm))", "frac = m - 1.0f", "out = c_k + ((c_k+1 - c_k) * frac)", "lod[p] = (float)k + frac",
                 "footprint[p] = (0, 0, 0, 0), lod[p] = 0", "never from caller memory", "before any address is formed from it",
                 "anisotropic footprints", "LOD in the frame path", "texture LOD"):
        assert item in text, item


# ------------------------------------------------------------------ the reference on CPU-built planes
def test_reference_at_scale_0_and_at_a_large_scale(orc_det):
    c = cpu_case(orc_det)
    for name in ("albedo", "texcoord"):  # footprint_scale = 0: pt_surface_planes's planes bit for bit
        assert np.array_equal(c["point"][name], c["surface"][name])
    assert not c["point"]["lod"].any() and c["point"]["minified"] == 0 and np.array_equal(c["point"]["footprint"], c["lod"]["footprint"])
    tex = c["lod"]["kind"] == 4
    assert c["lod"]["textured"] == int(tex.sum()) > 1000 and 0 < c["lod"]["minified"] < c["lod"]["textured"]
    assert not c["lod"]["footprint"][~tex].any() and not c["lod"]["lod"][~tex].any()
    lod = c["lod"]["lod"].view(f32)[..., 0]
    assert lod.min() == 0 and 1 < lod.max() < 6 and (lod[c["lod"]["level"] >= 0] >= c["lod"]["level"][c["lod"]["level"] >= 0]).all()
    big = SL.surface_lod_ref(c["hit"], c["sc"], c["verts"], c["idx"], [(0, 0, W, H)], [c["row"]], np.ones((H, W), bool), scale=1e9)
    lb = big["lod"].view(f32)[..., 0]
    for mesh, Lm in ((0, 6), (1, 5)):  # the coarsest level everywhere textured: one texel, so one colour per texture, up to the weights' rounding
        on = c["lod"]["mesh"] == mesh
        assert (lb[on] == Lm).all() and np.ptp(big["albedo"][on].astype(np.int64), axis=0).max() <= 4
    assert big["minified"] == big["textured"]


def test_footprints_of_the_reference_are_the_neighbour_differences(orc_det):
    c = cpu_case(orc_det)
    prim = np.ascontiguousarray(c["hit"], f32).view(np.int32)[..., 3]
    kind = c["lod"]["kind"]
    fp, tc = c["lod"]["footprint"].view(f32), c["lod"]["texcoord"].view(f32)
    res = check_footprints(fp, tc, prim, kind)
    print(f"footprints: largest error {res['err']:.3e} over {res['nx']} + {res['ny']} pixels, largest footprint {res['size']:.3e}")
    assert res["nx"] > 4000 and res["ny"] > 4000
    assert res["err"] <= FOOT_MEASURED, res
    # teeth: x and y swapped, and halved
    swapped = check_footprints(fp[..., [2, 3, 0, 1]], tc, prim, kind)
    halved = check_footprints(fp * f32(0.5), tc, prim, kind)
    print(f"  swapped {swapped['err']:.3e}, halved {halved['err']:.3e}, bound {FOOT_BOUND:.3e}")
    assert swapped["err"] > 100 * FOOT_BOUND and halved["err"] > 100 * FOOT_BOUND


def test_filtered_albedo_of_the_reference_is_closer_to_the_pixel_average(orc_det):
    c = cpu_case(orc_det)
    q = ground_pixels(c["lod"]["mesh"])
    Y, X = np.nonzero(q)
    tri = c["verts"][c["idx"][0]]
    uv = c["sc"]["uv"][0].reshape(3, 2)
    # both ground triangles carry one affine texcoord map
    probe = SL.plane_uv64(c["row"], W, H, X[:50] + 0.5, Y[:50] + 0.5, c["verts"][c["idx"][1]], c["sc"]["uv"][1].reshape(3, 2))
    assert np.abs(probe - SL.plane_uv64(c["row"], W, H, X[:50] + 0.5, Y[:50] + 0.5, tri, uv)).max() < 1e-9
    truth = SL.supersample64(c["sc"]["textures"][0], c["row"], W, H, X.astype(np.float64), Y.astype(np.float64), tri, uv, 16)
    e_point, e_lod = rms_against(c["point"]["albedo"], truth, q), rms_against(c["lod"]["albedo"], truth, q)
    r = e_lod / e_point
    print(f"quality: {int(q.sum())} ground pixels, rms point {e_point:.4f}, rms filtered {e_lod:.4f}, ratio {r:.5f}")
    assert q.sum() > 2000 and abs(r - R_REF) < 5e-4 and R_REF < 0.8
