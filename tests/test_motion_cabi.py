"""Object motion for the reprojection chain (pt_vertex_count, pt_copy_vertices_device, pt_motion_planes) without a GPU: the entry points are
declared and exported, the ctypes mirrors match the compiler's layout, the header still compiles as C99 and as C++17, a null context and a
null description are refused before any device work, both facades have the methods and the Python one checks its arguments before the
library is called; and the float32 NumPy reference (tests/motion_ref.py), on planes built with the CPU checker, has the properties the
feature exists for: a mesh moved along its normal keeps its history, static geometry gives the G-buffer's motion, stale primitive indices
give the stated words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import motion_ref as M
import temporal_ref as T
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_text
from conftest import ROOT
from optixpathtracer_amd import _lib

f32 = np.float32
DESC_FIELDS = ("hit", "prev_vertices", "motion", "prev_point", "prev_surface", "prev_cameras", "num_prev_cameras", "block_mask", "flags")
STATS_FIELDS = ("pixels", "hits", "stale", "kernel_ms")
NEW = ("pt_vertex_count", "pt_copy_vertices_device", "pt_motion_planes")


def test_library_exports_the_entry_points():
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert name in header().split("VERSIONING.")[1].split("*/")[0]  # the note names it among the entry points added at 0.4
    for name in NEW[1:]:  # the two that take device pointers
        assert name in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_vertex_count\s*\(\s*const\s+pt_ctx\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)", src)
    assert re.search(r"int\s+pt_copy_vertices_device\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)", src)
    assert re.search(r"int\s+pt_motion_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_motion_desc\s*\*\s*\w+\s*,\s*pt_motion_stats\s*\*", src)
    assert L.pt_version().startswith(b"ptamd 0.4")


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.MotionDesc, "pt_motion_desc", DESC_FIELDS), (_lib.MotionStats, "pt_motion_stats", STATS_FIELDS)],
                 [72, 0, 8, 16, 24, 32, 40, 48, 56, 64] + [32, 0, 8, 16, 24])
    assert _lib.MOTION_PLANES == M.WORDS and tuple(_lib.MOTION_PLANES) == M.PLANES == DESC_FIELDS[2:5]


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const void* hit, float* snapshot, float* motion, const float* cams) {\n"
            "    pt_motion_desc d = {0, 0, 0, 0, 0, 0, 1u, 0, 0u};\n"
            "    pt_motion_stats s;\n"
            "    uint32_t nv = 0, nt = 0;\n"
            "    if (pt_vertex_count(c, &nv, &nt) || pt_copy_vertices_device(c, snapshot, (size_t)nv * 12)) return -1;\n"
            "    d.hit = hit; d.prev_vertices = snapshot; d.motion = motion; d.prev_cameras = cams; d.flags = PT_MOTION_RESERVED;\n"
            "    return pt_motion_planes(c, &d, &s);\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_context_and_null_description_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.MotionDesc(), _lib.MotionStats(7, 7, 7, 7.0)
    assert L.pt_motion_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_motion_planes: null context" in L.pt_last_error(None)
    assert L.pt_motion_planes(None, None, None) == -1
    assert (s.pixels, s.hits, s.stale, s.kernel_ms) == (7, 7, 7, 7.0)
    nv, nt = C.c_uint32(7), C.c_uint32(7)
    assert L.pt_vertex_count(None, C.byref(nv), C.byref(nt)) == -1 and (nv.value, nt.value) == (7, 7)
    assert b"pt_vertex_count: null context" in L.pt_last_error(None)
    assert L.pt_copy_vertices_device(None, None, 0) == -1
    assert b"pt_copy_vertices_device: null context" in L.pt_last_error(None)
    # a null description is refused before the context is looked at (the text of pt_motion.hip; a live context needs a GPU)
    api = open(os.path.join(ROOT, "optixpathtracer_amd", "csrc", "pt_motion.hip")).read()
    body = api.split('extern "C" int pt_motion_planes(')[1]
    assert body.index("null description") < body.index("ctx->width")


def test_python_facade_checks_its_arguments():
    import torch

    from optixpathtracer_amd import renderer as R

    for name in ("copyVerticesDevice", "motionPlanes", "vertexCount"):
        assert callable(getattr(R.SampleRenderer, name, None))
    # on an object without a context: what the methods refuse, they refuse before the library is called
    r = bare_renderer()
    hit, pv = fake_cuda((4, 4, 8)), fake_cuda((8, 3))
    with pytest.raises(ValueError, match="unknown plane 'depth'"):
        r.motionPlanes(hit, pv, planes=("depth",))
    with pytest.raises(ValueError, match="`out` names a plane that `planes` does not"):
        r.motionPlanes(hit, pv, planes=("prev_point",), out=dict(prev_surface=1))
    with pytest.raises(ValueError, match="no plane asked for"):
        r.motionPlanes(hit, pv, planes=())
    with pytest.raises(ValueError, match="motion needs prev_cameras"):
        r.motionPlanes(hit, pv)
    with pytest.raises(ValueError, match="hit is required"):
        r.motionPlanes(None, pv, planes=("prev_point",))
    with pytest.raises(TypeError, match="motionPlanes: hit: a torch tensor or a device pointer"):
        r.motionPlanes(np.zeros((4, 4, 8), f32), pv, planes=("prev_point",))
    with pytest.raises(ValueError, match="motionPlanes: hit: the tensor is on cpu"):
        r.motionPlanes(torch.zeros((4, 4, 8)), pv, planes=("prev_point",))
    with pytest.raises(ValueError, match=r"prev_vertices: a contiguous torch.float32 tensor of shape \(8, 3\) is expected"):
        r.motionPlanes(hit, fake_cuda((7, 3)), planes=("prev_point",))
    with pytest.raises(ValueError, match=r"prev_surface: a contiguous torch.float32 tensor of shape \(4, 4, 8\) is expected"):
        r.motionPlanes(hit, pv, planes=("prev_surface",), out=dict(prev_surface=fake_cuda((4, 4, 4))))
    with pytest.raises(ValueError, match="the mask needs"):
        r.blockGrid = lambda: (1, 1)
        r.motionPlanes(hit, pv, planes=("prev_point",), out=dict(prev_point=fake_cuda((4, 4, 4))), mask=np.ones((2, 2)))
    with pytest.raises(ValueError, match=r"copyVerticesDevice: out: a contiguous torch.float32 tensor of shape \(8, 3\) is expected"):
        r.copyVerticesDevice(out=fake_cuda((8, 4)))
    with pytest.raises(ValueError, match="the context on GPU 1"):
        r._device = 1
        r.copyVerticesDevice(out=fake_cuda((8, 3)))


def test_cxx_facade_compiles(tmp_path):
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t motion(SampleRenderer& sample, pt_motion_desc d, float* snapshot) {\n"
        "    const uint32_t nv = sample.copyVerticesDevice(nullptr, 0);\n"
        "    sample.copyVerticesDevice(snapshot, (size_t)nv * 12);\n"
        "    d.prev_vertices = snapshot;\n"
        "    pt_motion_stats s{};\n"
        "    sample.motionPlanes(d, &s);\n"
        "    return sample.motionPlanes(d).hits + s.stale;\n"
        "}\n"
    )


def test_header_states_the_contract():
    text = header_text()
    for item in ("w0 = (1.0f - u) - v; Q = (p0*w0 + p1*u) + p2*v per component; ngp = normalize3(cross3(p1 - p0, p2 - p0))",
                 "i_k = idx[3*prim + k]", "prev_point[p] = (Q, 1.0f)", "with words 5..7 (ng) replaced by ngp", "q = Q - e'",
                 "equal to pt_render_gbuffer's motion plane bit for bit at every miss", "no address is formed from it",
                 "prev_surface[p] = (hit[p].t, 0, 0, -1, -1, 0, 0, 0)", "stats->stale counts the pixel",
                 "pt_temporal_accumulate gets hit = prev_surface, position = prev_point, motion = motion",
                 "pt_filter_planes keeps the CURRENT hit and position", "bytes must equal vertices * 12",
                 "float32 NumPy evaluating this reproduces every output bit for bit", "No other pixel is written in any output",
                 "Zero pixels launch nothing and return PT_OK", "flags != 0", "a pt_multi_* wrapper", "topology changes",
                 "pt_motion_planes below gives the planes for that"):
        assert item in text, item


# ------------------------------------------------------------------ 1. a mesh moved along its normal keeps its history
# (pixels of the current frame on mesh 1; of those, the ones whose four taps lie on mesh 1 in the previous frame under the camera-only
#  motion / under the new motion; valid pixels among the latter two sets by route)
NORMAL_MOVE_COUNTS = (504, 423, 468, 0, 504)


def _four_taps_on_mesh(motion, prev_mesh, mesh):
    h, w = prev_mesh.shape
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        px, py = xs.astype(f32) + motion[..., 0], ys.astype(f32) + motion[..., 1]
        ok = np.isfinite(px) & np.isfinite(py)
        ix, iy = np.floor(np.where(ok, px, 0)).astype(int), np.floor(np.where(ok, py, 0)).astype(int)
    ok &= (ix >= 0) & (ix + 1 < w) & (iy >= 0) & (iy + 1 < h)
    ixc, iyc = np.clip(ix, 0, w - 2), np.clip(iy, 0, h - 2)
    for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
        ok &= prev_mesh[iyc + j, ixc + i] == mesh
    return ok


def test_normal_wise_move_keeps_the_history(orc_det):
    import gbuffer_ref as G

    w, h = M.QUAD_SIZE
    cam = M.QUAD_CAMERA
    before, after = M.quad_scene(0.0), M.quad_scene(M.QUAD_DELTA)
    cur = M.cpu_planes(orc_det, after, (w, h), cam, cam)
    old = M.cpu_planes(orc_det, before, (w, h), cam, cam)
    px = np.ones((h, w), bool)
    rects = [(0, 0, w, h)]
    row = G._row(cam, w / h)
    prev_vertices, idx = M.model_arrays(before)
    rng = np.random.default_rng(31)
    base = dict(prev_hit=old["hit"], prev_position=old["position"], color=rng.random((h, w, 4), dtype=f32),
                history_in=rng.random((h, w, 4), dtype=f32), length_in=np.ones((h, w), f32))
    prm = dict(plane_eps=0.01)
    mesh_cur, mesh_old = cur["hit"].view(np.int32)[..., 4], old["hit"].view(np.int32)[..., 4]
    on1 = mesh_cur == 1
    assert M.QUAD_DELTA > prm["plane_eps"] * float(cur["hit"][..., 0][on1].max())  # the move is larger than the plane test allows
    # camera-only planes: every mesh-1 pixel whose taps land on mesh 1 is rejected, by the plane test
    camera_only = T.temporal_ref(orc_det, dict(base, motion=cur["motion"], hit=cur["hit"], position=cur["position"]), rects, px, **prm)
    s_cam = on1 & _four_taps_on_mesh(cur["motion"], mesh_old, 1)
    assert not camera_only["valid"][s_cam].any() and ((camera_only["reason"][s_cam] & T.BIT["plane"]) != 0).all()
    assert not camera_only["valid"][on1 & (mesh_old == 1)].any()
    # the new planes: every such pixel is valid
    ref = M.motion_ref(cur["hit"], prev_vertices, idx, rects, px, cams=[row], prev_cams=[row])
    planes = dict(base, motion=ref["motion"].view(f32), hit=ref["prev_surface"].view(f32), position=ref["prev_point"].view(f32))
    with_motion = T.temporal_ref(orc_det, planes, rects, px, **prm)
    s_new = on1 & _four_taps_on_mesh(planes["motion"], mesh_old, 1)
    assert with_motion["valid"][s_new].all()
    assert int(s_new.sum()) * 10 >= w * h, int(s_new.sum())
    # the surface point moved towards the camera: it was nearer the image centre before
    far = on1 & (np.abs(np.arange(w) - (w - 1) / 2)[None, :] > 4)
    assert (np.sign(planes["motion"][far][:, 0]) == -np.sign(np.arange(w) - (w - 1) / 2)[None, :].repeat(h, 0)[far]).all()
    got = (int(on1.sum()), int(s_cam.sum()), int(s_new.sum()), int(camera_only["valid"][on1].sum()), int(with_motion["valid"][on1].sum()))
    print("normal-wise move:", got)
    assert got == NORMAL_MOVE_COUNTS, got


# ------------------------------------------------------------------ 2. static geometry: the G-buffer's motion
# Q = (p0*w0 + p1*u) + p2*v against o + t*dir: the two expressions share no intermediate, so the bound is empirical: the largest difference
# measured with the reference on these two inputs (profiles/motion.md), times four.
STATIC_MEASURED_PX = 1.1e4  # terrain 1.097e+04 (a surface point almost on the previous camera's plane: c near 0), two_box 3.211e+01
STATIC_BOUND_PX = 4 * STATIC_MEASURED_PX


def test_static_geometry_gives_the_gbuffer_motion(orc_det):
    import gbuffer_ref as G

    worst = 0.0
    for name, (make, size, cam, prev, _, _) in T.real_inputs().items():
        w, h = size
        model = make()
        P = M.cpu_planes(orc_det, model, size, cam, prev)
        verts, idx = M.model_arrays(model)
        ref = M.motion_ref(P["hit"], verts, idx, [(0, 0, w, h)], np.ones((h, w), bool), cams=[G._row(cam, w / h)], prev_cams=[G._row(prev, w / h)])
        assert ref["stale"] == 0
        miss = ref["kind"] == 2
        gb = np.ascontiguousarray(P["motion"]).view(np.uint32)
        assert miss.any() and np.array_equal(ref["motion"][miss], gb[miss]), f"{name}: motion at misses differs from the G-buffer formula"
        # prev_surface is the hit record itself up to the normal's rounding; prev_point the position's
        assert np.array_equal(ref["prev_surface"][..., 0:5], np.ascontiguousarray(P["hit"]).view(np.uint32)[..., 0:5])
        hit = ref["kind"] == 1
        a, b = ref["motion"].view(f32)[hit], gb.view(f32)[hit]
        both = np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
        one = np.isfinite(a).all(-1) ^ np.isfinite(b).all(-1)
        d = float(np.abs(a[both].astype(np.float64) - b[both]).max())
        dd = np.abs(a[both].astype(np.float64) - b[both]).max(-1)
        near = np.abs(b[both]).max(-1) <= 64  # lookups that stay within 64 pixels: the ones a temporal pass can use
        print(f"{name}: largest motion difference at hits {d:.3e} px over {int(both.sum())} pixels (median {np.median(dd):.3e}, largest where "
              f"|motion| <= 64 px {dd[near].max():.3e} over {int(near.sum())}); finite in one route only: {int(one.sum())}")
        worst = max(worst, d)
        assert d <= STATIC_BOUND_PX, (name, d)
        dp = np.abs(ref["prev_point"].view(f32)[hit][:, :3].astype(np.float64) - P["position"][hit][:, :3])
        assert (dp <= 1e-5 * np.abs(P["position"][hit][:, :3]).max()).all()
    print(f"static geometry: largest difference {worst:.3e} px (recorded {STATIC_MEASURED_PX})")


# ------------------------------------------------------------------ 3. stale and negative primitive indices
def test_stale_and_negative_prims_give_the_stated_words():
    model = M.quad_scene()
    verts, idx = M.model_arrays(model)
    ntri = len(idx)
    h, w = 2, 5
    hit = np.zeros((h, w, 8), f32)
    words = hit.view(np.int32)
    hit[..., 0] = np.arange(10, dtype=f32).reshape(h, w) + 1
    hit[..., 1], hit[..., 2] = 0.25, 0.5
    words[..., 4] = 1
    hit[..., 5:8] = (0.0, 0.0, -1.0)
    prims = np.array([[0, ntri - 1, ntri, ntri + 1, 2**31 - 1], [-1, -2, -(2**31), 1, 2]], np.int32)
    words[..., 3] = prims
    row = np.array([0, 1, -5, 1, 0, 0, 0, 1, 0, 0, 0, 1], f32)
    ref = M.motion_ref(hit, verts, idx, [(0, 0, w, h)], np.ones((h, w), bool), cams=[row], prev_cams=[row])
    stale, miss = prims >= ntri, prims < 0
    assert ref["stale"] == int(stale.sum()) == 3 and ref["hits"] == 4
    assert (ref["motion"][stale] == M.QNAN).all() and not ref["prev_point"][stale].any()
    want = np.zeros((3, 8), np.uint32)
    want[:, 0] = hit[..., 0][stale].view(np.uint32)
    want[:, 3] = want[:, 4] = 0xFFFFFFFF
    assert np.array_equal(ref["prev_surface"][stale], want)
    assert not ref["prev_point"][miss].any() and np.array_equal(ref["prev_surface"][miss], hit.view(np.uint32)[miss])
    assert not (ref["motion"][miss] == M.QNAN).any()  # the miss direction of the pixel's ray, in front of the same camera
    inr = ~stale & ~miss
    assert (ref["prev_point"][inr][:, 3] == f32(1).view(np.uint32)).all()
    tri = verts[idx[prims[inr]]]
    q = (tri[:, 0] * f32(0.25) + tri[:, 1] * f32(0.25)) + tri[:, 2] * f32(0.5)
    assert np.array_equal(ref["prev_point"][inr][:, :3], q.view(np.uint32))
    # a pixel outside the set keeps the fill in every plane
    px = np.ones((h, w), bool)
    px[0, 2] = False
    ref = M.motion_ref(hit, verts, idx, [(0, 0, w, h)], px, cams=[row], prev_cams=[row])
    for name in M.PLANES:
        assert (ref[name][0, 2] == M.SENTINEL).all() and not (ref[name][px] == M.SENTINEL).any()
    assert ref["stale"] == 2
