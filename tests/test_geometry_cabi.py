"""The reprojection chain against float64 geometry (tests/geometry_ref.py), without a GPU.

The float32 references of the chain (temporal_ref, motion_ref, surface_ref, plan_ref and the G-buffer formulas of gbuffer_ref) pin the
kernels' bits; here they are themselves held against a truth that shares no expression with them, on CPU-built planes of two different
real frames: a camera that moved, turned and zoomed, a mesh that moved rigidly, two views with different previous cameras, textured hits.
This file does two things for tests/test_gpu_geometry.py, which applies the same checks (the check_* functions below) to the GPU's planes:

  it records the bounds.  Every *_BOUND constant is four times the *_MEASURED constant next to it, and that is the largest error the
  float32 reference alone shows on that input, measured here; the tests assert the reference still shows no more.  The GPU planes equal these
  references bit for bit where the inputs are the same (the existing tests), so the factor of four only has to cover inputs that differ in
  the last bit.  profiles/geometry.md holds the same table.  No bound comes from a kernel's output.

  it proves the checks have teeth.  Each check is applied once more to reference data made wrong on purpose — motion negated, motion
  shifted by half a pixel, u and v swapped in the hit plane, the two views' previous cameras swapped — and must then exceed its bound by a
  factor of 100 at least (the carry check: fail its conditions)."""
import numpy as np
import pytest

import geometry_ref as G64
import plan_ref as PL
import surface_ref as S
import temporal_ref as T
from geometry_cases import (
    MOVES, ORBIT, T1_BOUND_PX, T1_COVERAGE, T1_MEASURED_PX, T2_BOUND, T2_COVERAGE, T2_MEASURED, T3_BOUND, T3_MEASURED, TEXTURED_MESHES, VIEW_RECTS, H, W,
    _carry, _motion_planes, _swap_uv, _t1_figures, camera_case, carry_inputs, carry_passes, check_barycentrics, check_camera_motion, check_carry,
    check_object_motion, check_texcoords_tell_v1_from_v2, f32, lookups, object_case, orbit_cameras, t2_figures, textured_case, view_case)


@pytest.mark.parametrize("move", MOVES)
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_camera_motion_of_the_reference(orc_det, name, move):
    c = camera_case(orc_det, name, move)
    res = check_camera_motion(c["motion"], c["hit"], c["position"], c["rays"], c["prev_rays"], (0, 0, W, H), c["size"])
    worst = _t1_figures(res, f"{name} ({move})")
    assert len(res["hit_err"]) >= T1_COVERAGE * res["hits"] and len(res["miss_err"]) > 0
    assert worst <= T1_MEASURED_PX[name, move], (worst, T1_MEASURED_PX[name, move])


def test_camera_motion_of_the_reference_in_two_views(orc_det):
    c = view_case(orc_det)
    worst = 0.0
    for k, rect in enumerate(VIEW_RECTS):
        res = check_camera_motion(c["motion"], c["hit"], c["position"], c["rays"], c["prev_rays"], rect, c["size"])
        worst = max(worst, _t1_figures(res, f"view {k}"))
        assert len(res["hit_err"]) >= T1_COVERAGE * res["hits"] and len(res["miss_err"]) > 0
    assert worst <= T1_MEASURED_PX["views"], worst


@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_camera_motion_check_has_teeth(orc_det, name):
    c = camera_case(orc_det, name, "a")
    bound = T1_BOUND_PX[name, "a"]
    for what, wrong in (("negated", -c["motion"]), ("shifted by half a pixel", c["motion"] + f32(0.5))):
        _, inside = lookups(c["motion"], (0, 0, W, H))
        wrong = np.where(inside[..., None], wrong, f32(np.nan))  # the pixels the right plane's check covers
        res = check_camera_motion(wrong, c["hit"], c["position"], c["rays"], c["prev_rays"], (0, 0, W, H), c["size"])
        e = res["hit_err"]
        print(f"T1 {name}, motion {what}: largest {e.max():.3e} px, median {np.median(e):.3e} (bound {bound:.1e})")
        assert np.median(e) >= 100 * bound and np.median(res["miss_err"]) >= 100 * bound


def test_view_check_has_teeth(orc_det):
    right, wrong = view_case(orc_det), view_case(orc_det, swapped=True)
    for k, rect in enumerate(VIEW_RECTS):
        res = check_camera_motion(wrong["motion"], right["hit"], right["position"], right["rays"], right["prev_rays"], rect, right["size"])
        e = res["hit_err"]
        print(f"T1 view {k}, previous cameras swapped: {len(e)} checked, largest {e.max():.3e} px, median {np.median(e):.3e}")
        assert len(e) > 0 and np.median(e) >= 100 * T1_BOUND_PX["views"]


@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_object_motion_of_the_reference(orc_det, name):
    c = object_case(orc_det, name)
    cur = c["cur"]
    res = check_object_motion(_motion_planes(c, cur["hit"]), cur["hit"], cur["position"], c["prev_rays"], c["mesh"], c["R"], c["c"], c["t"], c["size"])
    got = t2_figures(res, f"{name}, mesh {c['mesh']}")
    assert res["on"] >= T2_COVERAGE * res["hits"] and res["checked"] >= 0.5 * res["hits"]
    for k, v in got.items():
        assert v <= T2_MEASURED[name][k], (k, v)
    # the move is a real one: the moved mesh's points were somewhere else by more than a hundred times the bound
    words = np.ascontiguousarray(cur["hit"]).view(np.int32)
    on = (words[..., 3] >= 0) & (words[..., 4] == c["mesh"])
    pos = np.asarray(cur["position"], np.float64)[on][:, :3]
    assert (np.linalg.norm(G64.inverse_rigid(pos, c["R"], c["c"], c["t"]) - pos, axis=1) / c["size"]).min() >= 100 * T2_BOUND[name]["point_on"]


@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_object_motion_check_has_teeth(orc_det, name):
    c = object_case(orc_det, name)
    cur = c["cur"]
    right = _motion_planes(c, cur["hit"])
    args = (cur["hit"], cur["position"], c["prev_rays"], c["mesh"], c["R"], c["c"], c["t"], c["size"])
    # u and v swapped in the hit plane the pass reads: the previous point lands elsewhere in its triangle
    wrong = _motion_planes(c, _swap_uv(cur["hit"]))
    res = check_object_motion(wrong, *args)
    print(f"T2 {name}, u and v swapped: point_on {res['point_on']:.3e}, point_off {res['point_off']:.3e}, lookup {res['lookup_err'].max():.3e} px")
    assert res["point_on"] >= 100 * T2_BOUND[name]["point_on"] and res["point_off"] >= 100 * T2_BOUND[name]["point_off"]
    assert res["lookup_err"].max() >= 100 * T2_BOUND[name]["lookup_px"]
    for what, motion in (("negated", -right["motion"]), ("shifted by half a pixel", right["motion"] + f32(0.5))):
        _, inside = lookups(right["motion"], (0, 0, W, H))
        res = check_object_motion(dict(right, motion=np.where(inside[..., None], motion, f32(np.nan))), *args)
        print(f"T2 {name}, motion {what}: lookup median {np.median(res['lookup_err']):.3e} px")
        assert np.median(res["lookup_err"]) >= 100 * T2_BOUND[name]["lookup_px"]


def test_barycentrics_and_texcoords_of_the_reference(orc_det):
    c = textured_case(orc_det)
    check_texcoords_tell_v1_from_v2(c["model"])
    ref = S.surface_ref(c["hit"], c["sc"], np.ones((H, W), bool))
    res = check_barycentrics(c["hit"], c["position"], ref["texcoord"].view(f32), c["model"], TEXTURED_MESHES)
    print(f"T3: uv {res['uv_err']:.3e}, texcoord {res['st_err']:.3e} over {res['hits']} hits, {res['textured']} textured")
    assert res["textured"] == ref["textured"] and res["textured"] * 10 >= W * H
    assert res["uv_err"] <= T3_MEASURED["uv"] and res["st_err"] <= T3_MEASURED["st"]


def test_barycentric_check_has_teeth(orc_det):
    c = textured_case(orc_det)
    wrong = _swap_uv(c["hit"])
    ref = S.surface_ref(wrong, c["sc"], np.ones((H, W), bool))
    # the swapped plane against the truth; and the texcoords the reference makes of it against the truth's
    res = check_barycentrics(wrong, c["position"], ref["texcoord"].view(f32), c["model"], TEXTURED_MESHES)
    print(f"T3, u and v swapped: uv {res['uv_err']:.3e}, texcoord {res['st_err']:.3e}")
    assert res["uv_err"] >= 100 * T3_BOUND["uv"] and res["st_err"] >= 100 * T3_BOUND["st"]


@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_carry_of_the_reference_lands_on_the_surface_point(orc_det, name):
    c = camera_case(orc_det, name, "a")
    truth = np.asarray(c["position"], np.float64)[..., :3]
    res = _carry(c, truth, name)
    print(f"T4 {name}: median error/d {res[0]:.4f}, share <= 1 {res[1]:.4f}, share of hit pixels checked {res[2]:.3f}")
    assert all(carry_passes(res)), res
    # the blend of temporal_ref with color = the current position plane stays within the same bound
    planes = dict(carry_inputs(c), color=np.array(c["position"], f32))
    del planes["moments_in"]
    out = T.temporal_ref(orc_det, planes, [(0, 0, W, H)], np.ones((H, W), bool), **PL.REAL_GATHER[name])
    is_hit = np.ascontiguousarray(c["hit"]).view(np.int32)[..., 3] >= 0
    res = check_carry(out["history_out"].view(f32), out["valid"], truth, c["motion"], c["prev_position"], c["prev_hit"], is_hit)
    print(f"T4 {name}, blended: median {res[0]:.4f}, share <= 1 {res[1]:.4f}, checked {res[2]:.3f}")
    assert all(carry_passes(res)), res
    # wrong on purpose.  Negated motion fails both conditions (median 2.8 / 4.6, share 0.11 / 0.11).  The half-pixel slip fails the median
    # (0.48 / 0.44 against 0.1); its error of 0.7 px stays below the taps' diameter of 1.4 px and more, so the share condition cannot see it
    # on the two-box scene (1.0000; terrain 0.9845 fails) and is not asserted for it
    for what, motion in (("negated", -c["motion"]), ("shifted by half a pixel", c["motion"] + f32(0.5))):
        res = _carry(c, truth, name, motion)
        ok = carry_passes(res)
        print(f"T4 {name}, motion {what}: median {res[0]:.4f}, share <= 1 {res[1]:.4f}, checked {res[2]:.3f} -> passes {ok}")
        assert not ok[0], (what, res)
        if what == "negated":
            assert not ok[1], (what, res)


@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_carry_of_the_reference_follows_a_moved_mesh(orc_det, name):
    c = object_case(orc_det, name)
    cur, old = c["cur"], c["old"]
    mp = _motion_planes(c, cur["hit"])
    words = np.ascontiguousarray(cur["hit"]).view(np.int32)
    on = (words[..., 3] >= 0) & (words[..., 4] == c["mesh"])
    pos = np.asarray(cur["position"], np.float64)[..., :3]
    truth = np.where(on[..., None], G64.inverse_rigid(pos, c["R"], c["c"], c["t"]), pos)
    P = dict(motion=mp["motion"], hit=mp["prev_surface"], position=mp["prev_point"], prev_hit=old["hit"], prev_position=old["position"])
    res = _carry(P, truth, name)
    print(f"T4 {name}, moved mesh: median error/d {res[0]:.4f}, share <= 1 {res[1]:.4f}, share of hit pixels checked {res[2]:.3f}")
    assert all(carry_passes(res)), res
    res = _carry(P, truth, name, -mp["motion"])
    print(f"T4 {name}, moved mesh, motion negated: median {res[0]:.4f}, share <= 1 {res[1]:.4f}")
    assert not carry_passes(res)[0] and not carry_passes(res)[1]


def test_real_motion_beats_no_motion_in_the_reference_chain(orc_det):
    """Two-box, 64 x 48, 8 frames of 1 spp, the camera orbiting by 0.03 rad per frame (the first choice of step and frame count; neither
    had to be raised): the checker's frames through the NumPy temporal stage, once with the CPU-built motion plane and once with an
    all-zero one, against the checker's 256-spp frame at the last camera.  RMS of history_out: 0.0491 with the real motion, 0.0752 with
    none — ahead by a third, more than the fifth asked of the reference chain before the GPU test may assert the inequality."""
    from optixpathtracer_amd import scenes

    w, h = ORBIT["size"]
    model = scenes.two_box_scene(shadow_catcher=False)
    sc, pr = orc_det.make_scene(model), orc_det.make_probe(scenes.sky_probe(256, 128).BuildCDF())
    cams = orbit_cameras()
    rects, px = [(0, 0, w, h)], np.ones((h, w), bool)
    hist = {True: np.zeros((h, w, 4), f32), False: np.zeros((h, w, 4), f32)}
    ln = {True: np.zeros((h, w), f32), False: np.zeros((h, w), f32)}
    for k, cam in enumerate(cams):
        uvw = scenes.uvw_frame(**cam, aspect=w / h)
        colour = orc_det.render(sc, pr, uvw, cam["eye"], w, h, ORBIT["spp"], subframe=k)["accum"]
        P = T.cpu_planes(orc_det, model, (w, h), cam, cams[max(k - 1, 0)])
        for real in (True, False):
            planes = dict(P, motion=P["motion"] if real else np.zeros((h, w, 2), f32), color=colour, history_in=hist[real], length_in=ln[real])
            out = T.temporal_ref(orc_det, planes, rects, px, color_scale=float(k + 1))
            hist[real], ln[real] = out["history_out"].view(f32), out["length_out"].view(f32)
    cam = cams[-1]
    reference = orc_det.render(sc, pr, scenes.uvw_frame(**cam, aspect=w / h), cam["eye"], w, h, ORBIT["reference_spp"])["accum"]
    import filter_ref as F

    real, zero = F.rms(hist[True], reference), F.rms(hist[False], reference)
    print(f"T5: rms of history_out with the real motion {real:.5f}, with zero motion {zero:.5f}; mean length {ln[True].mean():.2f} / {ln[False].mean():.2f}")
    assert real <= 0.8 * zero, (real, zero)
