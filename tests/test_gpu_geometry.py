"""The reprojection chain on the GPU against float64 geometry (tests/geometry_ref.py): two different real frames against each other.

The other GPU tests of the chain compare every plane bit for bit with a float32 transcription of the header, which shares the header's
conventions.  Here the planes of renderGBuffer, motionPlanes and surfacePlanes, and what temporalCarry, temporalAccumulate and
temporalMoments make of them, are held against a truth that shares no expression with the kernels: the previous frame's own ray plane,
the inverse of the rigid move, least-squares barycentrics.  The checks and every bound are those of tests/test_geometry_cabi.py, where each
bound was measured on the float32 references alone (four times the largest error they show; profiles/geometry.md) and where each check is
shown to fail by a factor of 100 on data made wrong on purpose.  Nothing here derives a bound from a kernel's output.

Inputs: the suite's small frame, 131 x 61 (17 x 8 blocks, the last column 3 wide, the last row 5 high), on the two scenes of
temporal_ref.real_inputs(); T3 on surface_ref.textured_scene(); T5 the two-box scene at 64 x 48."""
import numpy as np
import pytest
import torch

import filter_ref as F
import geometry_cases as GC
import geometry_ref as G64
import plan_ref as PL
import surface_ref as S
import temporal_ref as T
from gbuffer_ref import _row
from gpu_kit import plane_renderer as _renderer
from gpu_kit import to_numpy as _np
from optixpathtracer_amd import scenes
from optixpathtracer_amd import renderer as R
from scene_kit import _np_transform

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = GC.W, GC.H
FRAME = (0, 0, W, H)
DEV = "cuda:0"


def _is_hit(hit):
    return np.ascontiguousarray(hit).view(np.int32)[..., 3] >= 0


_MODELS = {}


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = GC.scenes_and_cameras()[name][0]()
    return _MODELS[name]


def _two_frames(r, cam_rows_prev, set_prev, set_cur, planes=("hit", "position", "motion", "ray")):
    """the previous frame's hit, position and ray planes, then this frame's planes with the motion against the previous cameras"""
    set_prev()
    old = r.renderGBuffer(("hit", "position", "ray"))
    set_cur()
    cur = r.renderGBuffer(planes, prev_cameras=cam_rows_prev)
    return {k: _np(old[k]) for k in ("hit", "position", "ray")}, {k: _np(cur[k]) for k in planes}


# ------------------------------------------------------------------ T1: camera motion
@pytest.mark.parametrize("move", GC.MOVES)
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_camera_motion(ptlib, name, move):
    cam = GC.scenes_and_cameras()[name][1]
    prev = GC.previous_camera(name, move)
    model = _model(name)
    r = _renderer(model, (W, H), prev)
    old, cur = _two_frames(r, _row(prev, W / H), lambda: None, lambda: r.setCamera(R.make_camera(cam, W / H)))
    r.close()
    res = GC.check_camera_motion(cur["motion"], cur["hit"], cur["position"], cur["ray"], old["ray"], FRAME, GC.scene_size(model))
    worst = GC._t1_figures(res, f"{name} ({move}), GPU")
    assert len(res["hit_err"]) >= GC.T1_COVERAGE * res["hits"] and len(res["miss_err"]) > 0
    assert worst <= GC.T1_BOUND_PX[name, move], (worst, GC.T1_BOUND_PX[name, move])


def test_camera_motion_in_two_views(ptlib):
    model = _model("two_box")
    cur_cams, prev_cams = GC.view_cameras()
    views = [(x, y, w, h, R.make_camera(cd, w / h)) for (x, y, w, h), cd in zip(GC.VIEW_RECTS, cur_cams)]
    prev = [R.make_camera(cd, w / h) for (x, y, w, h), cd in zip(GC.VIEW_RECTS, prev_cams)]
    prev_rows = np.stack([_row(cd, w / h) for (x, y, w, h), cd in zip(GC.VIEW_RECTS, prev_cams)])
    assert not np.array_equal(prev_rows[0], prev_rows[1])
    r = _renderer(model, (W, H), scenes.TWO_BOX_CAMERA)
    r.setViews(views)
    old, cur = _two_frames(r, prev_rows, lambda: r.setViewCameras(prev), lambda: r.setViewCameras([v[4] for v in views]))
    r.close()
    for k, rect in enumerate(GC.VIEW_RECTS):
        res = GC.check_camera_motion(cur["motion"], cur["hit"], cur["position"], cur["ray"], old["ray"], rect, GC.scene_size(model))
        worst = GC._t1_figures(res, f"view {k}, GPU")
        assert len(res["hit_err"]) >= GC.T1_COVERAGE * res["hits"] and len(res["miss_err"]) > 0
        assert worst <= GC.T1_BOUND_PX["views"], (k, worst)


# ------------------------------------------------------------------ T2: object motion
_OBJECT = {}


def _object_case(name, route):
    """One step of a loop with a moving mesh: the previous frame's planes, the snapshot of its vertices, the mesh moved through `route`,
    this frame's planes and motionPlanes' three.  Built once per (name, route); arrays only, the context is closed."""
    if (name, route) not in _OBJECT:
        model = _model(name)
        cam = GC.scenes_and_cameras()[name][1]
        prev = T.forward(cam, GC.OBJECT_CAMERA_MOVE["f"], dx=GC.OBJECT_CAMERA_MOVE["dx"])
        r = _renderer(model, (W, H), cam)
        mesh = GC.OBJECT_MESH.get(name)
        if mesh is None:
            mesh = GC.most_visible_mesh(_np(r.renderGBuffer(("hit",))["hit"]))
        Rm, c, t, A = GC.object_move(model, mesh)
        r.setCamera(R.make_camera(prev, W / H))
        old = r.renderGBuffer(("hit", "position", "ray"))
        snapshot = r.copyVerticesDevice()
        if route == "transform":
            r.transformMeshes({mesh: A})
        else:
            r.updateMeshesDevice({mesh: torch.from_numpy(_np_transform(A, model.meshes[mesh].vertex)).to(DEV)})
        r.setCamera(R.make_camera(cam, W / H))
        cur = r.renderGBuffer(("hit", "position"))
        mp = r.motionPlanes(cur["hit"], snapshot, prev_cameras=_row(prev, W / H))
        assert mp["stats"]["stale"] == 0
        case = dict(mesh=mesh, R=Rm, c=c, t=t, size=GC.scene_size(model), old={k: _np(old[k]) for k in ("hit", "position", "ray")},
                    cur={k: _np(cur[k]) for k in ("hit", "position")}, mp={k: _np(mp[k]) for k in ("motion", "prev_point", "prev_surface")})
        r.close()
        _OBJECT[name, route] = case
    return _OBJECT[name, route]


@pytest.mark.parametrize("route", ["transform", "update_device"])
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_object_motion(ptlib, name, route):
    c = _object_case(name, route)
    res = GC.check_object_motion(c["mp"], c["cur"]["hit"], c["cur"]["position"], c["old"]["ray"], c["mesh"], c["R"], c["c"], c["t"], c["size"])
    got = GC.t2_figures(res, f"{name}, mesh {c['mesh']}, {route}, GPU")
    assert res["on"] >= GC.T2_COVERAGE * res["hits"] and res["checked"] >= 0.5 * res["hits"]
    for k, v in got.items():
        assert v <= GC.T2_BOUND[name][k], (k, v, GC.T2_BOUND[name][k])


# ------------------------------------------------------------------ T3: barycentrics and texcoords
def test_barycentrics_and_texcoords(ptlib):
    model = S.textured_scene()
    GC.check_texcoords_tell_v1_from_v2(model)
    r = _renderer(model, (W, H), S.TEX_CAMERA)
    g = r.renderGBuffer(("hit", "position"))
    sp = r.surfacePlanes(g["hit"], r.copyTexcoordsDevice(), planes=("texcoord",))
    res = GC.check_barycentrics(_np(g["hit"]), _np(g["position"]), _np(sp["texcoord"]), model, GC.TEXTURED_MESHES)
    r.close()
    print(f"T3, GPU: uv {res['uv_err']:.3e}, texcoord {res['st_err']:.3e} over {res['hits']} hits, {res['textured']} textured")
    assert res["textured"] == sp["stats"]["textured"] and res["textured"] * 10 >= W * H
    assert res["uv_err"] <= GC.T3_BOUND["uv"] and res["st_err"] <= GC.T3_BOUND["st"], res


# ------------------------------------------------------------------ T4: the consumers read the motion the way the producers write it
def _consumers(r, name, P, truth, what):
    """P: motion, hit, position, prev_hit, prev_position as arrays.  temporalCarry with history_in = the previous frame's position plane,
    then temporalAccumulate and temporalMoments with color = this frame's position plane: each must land on `truth`."""
    up = {k: torch.from_numpy(np.array(v, f32)).to(DEV) for k, v in GC.carry_inputs(P).items()}
    geo = [up[k] for k in ("motion", "hit", "position", "prev_hit", "prev_position")]
    prm = PL.REAL_GATHER[name]
    is_hit = _is_hit(P["hit"])
    colour = torch.from_numpy(np.array(P["position"], f32)).to(DEV)

    def check(out, valid, which):
        res = GC.check_carry(_np(out["history_out"]), valid, truth, P["motion"], P["prev_position"], P["prev_hit"], is_hit)
        print(f"T4 {what}, {which}, GPU: median error/d {res[0]:.4f}, share <= 1 {res[1]:.4f}, share of hit pixels checked {res[2]:.3f}")
        assert all(GC.carry_passes(res)), (which, res)

    out = r.temporalCarry(*geo, up["history_in"], up["moments_in"], up["length_in"], **prm)
    check(out, _np(out["length_out"]) == GC.CARRY_LENGTH, "temporalCarry")
    assert out["stats"]["carried"] == int((_np(out["length_out"]) == GC.CARRY_LENGTH).sum())
    out = r.temporalAccumulate(colour, *geo, up["history_in"], up["length_in"], color_scale=1.0, **prm)
    check(out, _np(out["length_out"]) == GC.CARRY_LENGTH + 1, "temporalAccumulate")
    out = r.temporalMoments(colour, *geo, up["history_in"], up["moments_in"], up["length_in"], color_scale=1.0, **prm)
    check(out, _np(out["length_out"]) == GC.CARRY_LENGTH + 1, "temporalMoments")


@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_consumers_land_on_the_surface_point(ptlib, name):
    cam = GC.scenes_and_cameras()[name][1]
    prev = GC.previous_camera(name, "a")
    r = _renderer(_model(name), (W, H), prev)
    old, cur = _two_frames(r, _row(prev, W / H), lambda: None, lambda: r.setCamera(R.make_camera(cam, W / H)), planes=("hit", "position", "motion"))
    P = dict(cur, prev_hit=old["hit"], prev_position=old["position"])
    _consumers(r, name, P, np.asarray(cur["position"], np.float64)[..., :3], name)
    r.close()


@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_consumers_follow_a_moved_mesh(ptlib, name):
    c = _object_case(name, "transform")
    hit = np.ascontiguousarray(c["cur"]["hit"])
    on = _is_hit(hit) & (hit.view(np.int32)[..., 4] == c["mesh"])
    pos = np.asarray(c["cur"]["position"], np.float64)[..., :3]
    truth = np.where(on[..., None], G64.inverse_rigid(pos, c["R"], c["c"], c["t"]), pos)
    P = dict(motion=c["mp"]["motion"], hit=c["mp"]["prev_surface"], position=c["mp"]["prev_point"], prev_hit=c["old"]["hit"],
             prev_position=c["old"]["position"])
    r = _renderer(_model(name), (W, H), GC.scenes_and_cameras()[name][1])  # (the passes read their planes, not the scene)
    _consumers(r, name, P, truth, f"{name}, moved mesh")
    r.close()


# ------------------------------------------------------------------ T5: the point of the chain, under motion
def test_real_motion_beats_no_motion(ptlib):
    """The temporal stage of examples/svgf_loop.py — G-buffer with motion against last frame's camera, one sample per pixel, the colour
    blended into the reprojected history — on the two-box scene at 64 x 48 for 8 frames, the camera orbiting by 0.03 rad per frame; once
    with the real motion plane and once with an all-zero one.  history_out of the last frame against a 256-spp render at the last camera:
    the real motion is nearer.  With the CPU checker's frames and the NumPy chain, tests/test_geometry_cabi.py finds 0.0491 against
    0.0752; no ratio is asserted here, only the inequality."""
    w, h = GC.ORBIT["size"]
    cams = GC.orbit_cameras()
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), (w, h), cams[0])
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.launchParams.samples_per_launch = GC.ORBIT["spp"]
    zeros = np.zeros((h, w, 4), f32)
    still = torch.zeros((h, w, 2), device=DEV)
    hist = {m: [torch.zeros((h, w, 4), device=DEV) for _ in range(2)] for m in ("real", "zero")}
    ln = {m: [torch.zeros((h, w), device=DEV) for _ in range(2)] for m in ("real", "zero")}
    old = None
    for k, cam in enumerate(cams):
        r.setCamera(R.make_camera(cam, w / h))
        cur = r.renderGBuffer(("hit", "position", "motion"), prev_cameras=_row(cams[max(k - 1, 0)], w / h))
        old = old or cur
        r.uploadAccum(zeros)
        r.launchParams.frame.subframe_index = k
        r.render()
        colour = torch.from_numpy(r.download(R.PT_BUF_ACCUM)).to(DEV)
        i, o = k & 1, ~k & 1
        for m, motion in (("real", cur["motion"]), ("zero", still)):
            r.temporalAccumulate(colour, motion, cur["hit"], cur["position"], old["hit"], old["position"], hist[m][i], ln[m][i],
                                 history_out=hist[m][o], length_out=ln[m][o], color_scale=float(k + 1))
        old = cur
    last = len(cams) & 1
    r.uploadAccum(zeros)
    r.launchParams.samples_per_launch = GC.ORBIT["reference_spp"]
    r.launchParams.frame.subframe_index = 0
    r.render()
    reference = r.download(R.PT_BUF_ACCUM)
    real, zero = F.rms(_np(hist["real"][last]), reference), F.rms(_np(hist["zero"][last]), reference)
    print(f"T5, GPU: rms of history_out with the real motion {real:.5f}, with zero motion {zero:.5f}; mean length "
          f"{float(ln['real'][last].mean()):.2f} / {float(ln['zero'][last].mean()):.2f}")
    r.close()
    assert real < zero, (real, zero)
