"""The image-space passes' inputs on real planes, for the tests that share them: each pass's own GPU test and the stream contract, which
pins every pass on the case its test already built.  A case is a context with the G-buffer planes it rendered (and what the pass needs
besides); it is built once per process and its arrays are read-only."""
import numpy as np

import conftest  # noqa: F401  (puts the repository's root on sys.path)
import filter_ref as F
import moments_ref as MR
import motion_ref as M
import plan_ref as PR
import surface_aniso_ref as SA
import surface_ref as S
import temporal_ref as T
from gbuffer_ref import _moved, _row
from gpu_kit import plane_renderer
from gpu_kit import to_numpy as _np
from optixpathtracer_amd import scenes
from optixpathtracer_amd import renderer as R
from scene_kit import _affine

W, H = 131, 61  # every case but the two below
ANISO_W, ANISO_H = SA.W, SA.H
UPSAMPLE_W, UPSAMPLE_H = 132, 60


f32 = np.float32


class _Case:
    pass


_MOMENTS = {}


def moments_case(name):
    """The input's renderer and its G-buffer planes of the current and of the previous camera, with random colour, history, moments and
    albedo.  Built once; the arrays are read-only."""
    if name not in _MOMENTS:
        make, size, cam, prev, _, seed = T.real_inputs()[name]
        w, h = size
        r = plane_renderer(make(), size, cam)
        cur = r.renderGBuffer(("hit", "position", "motion"), prev_cameras=_row(prev, w / h))
        r.setCamera(R.make_camera(prev, w / h))
        old = r.renderGBuffer(("hit", "position"))
        r.setCamera(R.make_camera(cam, w / h))
        planes = MR.with_random_inputs(dict(motion=_np(cur["motion"]), hit=_np(cur["hit"]), position=_np(cur["position"]), prev_hit=_np(old["hit"]),
                                            prev_position=_np(old["position"])), seed)
        for a in planes.values():
            a.setflags(write=False)
        _MOMENTS[name] = (r, planes, MR.real_params(name))
    return _MOMENTS[name]


_PLAN = {}


def plan_case(name):
    """The input's renderer, its G-buffer planes of the current and of the previous camera (the mild move) with a block history, and the
    gather parameters.  Built once; the arrays are read-only."""
    if name not in _PLAN:
        make, size, cam, prev, prm, seed = PR.real_case(name)
        w, h = size
        r = plane_renderer(make(), size, cam)
        cur = r.renderGBuffer(("hit", "position", "motion"), prev_cameras=_row(prev, w / h))
        r.setCamera(R.make_camera(prev, w / h))
        old = r.renderGBuffer(("hit", "position"))
        r.setCamera(R.make_camera(cam, w / h))
        planes = PR.with_block_history(dict(motion=_np(cur["motion"]), hit=_np(cur["hit"]), position=_np(cur["position"]), prev_hit=_np(old["hit"]),
                                            prev_position=_np(old["position"])), seed)
        for a in planes.values():
            a.setflags(write=False)
        _PLAN[name] = (r, planes, prm)
    return _PLAN[name]


_FILTER = {}


def filter_case(name):
    """The input's renderer and its G-buffer planes with random colour, variance and length planes.  Built once; the arrays are read-only."""
    if name not in _FILTER:
        make, size, cam, prm, seed = F.real_inputs()[name]
        r = plane_renderer(make(), size, cam)
        g = r.renderGBuffer(("hit", "position"))
        planes = F.with_random_planes(dict(hit=_np(g["hit"]), position=_np(g["position"])), seed)
        for a in planes.values():
            a.setflags(write=False)
        _FILTER[name] = (r, planes, prm)
    return _FILTER[name]


MOTION_INPUTS = {
    "two_box": (lambda: scenes.two_box_scene(shadow_catcher=False), scenes.TWO_BOX_CAMERA, 0, _affine((0.0, 1.0, 0.0), 0.2, (1.0, 1.0, 1.0), (0.1, 0.15, -0.05))),
    "terrain": (lambda: scenes.voxel_terrain(n=64, target_tris=20000), scenes.TERRAIN_CAMERA, 3, _affine((0.0, 1.0, 0.0), 0.03, (1.0, 1.0, 1.0), (1.5, 0.8, -1.0))),
}


def _vertices(r, model):
    return M.stack_vertices([r.downloadVertices(k) for k in range(len(model.meshes))])


_MOTION = {}


def motion_case(name):
    """The input after one step of the loop: the previous frame's G-buffer planes, the snapshot of its vertices, the mesh moved with a refit,
    this frame's G-buffer planes under the current camera.  Built once; the arrays are read-only."""
    if name not in _MOTION:
        make, cam, mesh, A = MOTION_INPUTS[name]
        c = _Case()
        c.model, c.cam, c.prev, c.mesh, c.A = make(), cam, _moved(cam), mesh, A
        c.row, c.prev_row = _row(c.cam, W / H), _row(c.prev, W / H)
        c.verts0, c.idx = M.model_arrays(c.model)
        c.r = r = plane_renderer(c.model, (W, H), c.prev)
        old = r.renderGBuffer(("hit", "position"))
        c.snapshot = r.copyVerticesDevice()
        c.after_create = _np(c.snapshot)
        r.transformMeshes({mesh: A})
        c.verts1 = _vertices(r, c.model)
        c.after_refit = _np(r.copyVerticesDevice())
        r.setCamera(R.make_camera(cam, W / H))
        cur = r.renderGBuffer(("hit", "position", "motion"), prev_cameras=c.prev_row)
        c.gstats = cur["stats"]
        c.old = {k: _np(old[k]) for k in ("hit", "position")}
        c.cur = {k: _np(cur[k]) for k in ("hit", "position", "motion")}
        for a in [c.verts0, c.verts1, c.idx, c.after_create, c.after_refit] + list(c.old.values()) + list(c.cur.values()):
            a.setflags(write=False)
        _MOTION[name] = c
    return _MOTION[name]


SURFACE_INPUTS = {"textured": (S.textured_scene, S.TEX_CAMERA), "cornell": (scenes.cornell_box, scenes.CORNELL_CAMERA)}
_SURFACE = {}


def surface_case(name):
    """The model, its reference arrays, a renderer under the input's camera, its hit plane and its texcoord table.  Built once; the arrays
    are read-only."""
    if name not in _SURFACE:
        make, cam = SURFACE_INPUTS[name]
        c = _Case()
        c.model, c.cam = make(), cam
        c.sc = S.scene_arrays(c.model)
        c.r = plane_renderer(c.model, (W, H), cam)
        g = c.r.renderGBuffer(("hit",))
        c.gstats = g["stats"]
        c.hit = _np(g["hit"])
        c.table = _np(c.r.copyTexcoordsDevice())
        for a in [c.hit, c.table] + [v for v in c.sc.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _SURFACE[name] = c
    return _SURFACE[name]


_ANISO = {}
ANISO_INPUTS = {"textured": (S.textured_scene, SA.GRAZING_CAMERA), "cornell": (scenes.cornell_box, scenes.CORNELL_CAMERA)}


def surface_aniso_case(name):
    """the model, its reference arrays, a renderer under the input's camera at W x H, its hit plane, its texcoord table and its pyramid.
    Built once; the arrays are read-only."""
    if name not in _ANISO:
        make, cam = ANISO_INPUTS[name]
        c = _Case()
        c.model, c.cam = make(), cam
        c.sc = S.scene_arrays(c.model)
        c.verts, c.idx = M.model_arrays(c.model)
        c.r = plane_renderer(c.model, (ANISO_W, ANISO_H), cam)
        c.row = R._camera_rows([R.make_camera(cam, ANISO_W / ANISO_H)])[0]
        g = c.r.renderGBuffer(("hit",))
        c.gstats, c.hit = g["stats"], _np(g["hit"])
        c.table = c.r.copyTexcoordsDevice()
        c.bytes = c.r.textureMipsLayout()[1]
        c.mips = c.r.copyTextureMipsDevice()
        c.hit.setflags(write=False)
        _ANISO[name] = c
    return _ANISO[name]


def _upsample_model(name):
    return {"two_box": (lambda: scenes.two_box_scene(shadow_catcher=False), scenes.TWO_BOX_CAMERA),
            "terrain": (lambda: scenes.voxel_terrain(n=64, target_tris=20000), scenes.TERRAIN_CAMERA)}[name]


_UPSAMPLE = {}


def _hit_and_position(r):
    g = r.renderGBuffer(("hit", "position"))
    return dict(hit=_np(g["hit"]), position=_np(g["position"]))


def upsample_case(name, s):
    """(the full-size renderer, lo planes with a random colour, hi planes) of `name` at 132 x 60 over 132/s x 60/s: two contexts over one
    model.  Built once; the arrays are read-only."""
    if (name, s) not in _UPSAMPLE:
        make, cam = _upsample_model(name)
        if name not in _UPSAMPLE:
            model = make()
            r = plane_renderer(model, (UPSAMPLE_W, UPSAMPLE_H), cam)
            _UPSAMPLE[name] = (model, r, _hit_and_position(r))
        model, r, hi = _UPSAMPLE[name]
        low = plane_renderer(model, (UPSAMPLE_W // s, UPSAMPLE_H // s), cam)
        lo = _hit_and_position(low)
        low.close()
        lo["color"] = F.random_planes(np.random.default_rng(50 + s), UPSAMPLE_H // s, UPSAMPLE_W // s)[0]
        for a in list(lo.values()) + list(hi.values()):
            a.setflags(write=False)
        _UPSAMPLE[(name, s)] = (r, lo, hi)
    return _UPSAMPLE[(name, s)]


MOMENTS_INPUTS = ("color", "albedo", "motion", "hit", "position", "prev_hit", "prev_position", "history_in", "moments_in", "length_in")


def moments_kwargs(prm):
    """moments_ref's parameters as temporalMoments takes them: the two flags are clear_color and a clamp_k that is not None"""
    kw = {k: v for k, v in prm.items() if k not in ("clear", "clamp", "clamp_k")}
    kw["clear_color"] = bool(prm.get("clear"))
    kw["clamp_k"] = prm.get("clamp_k", MR.DEFAULTS["clamp_k"]) if prm.get("clamp") else None
    return kw


FILTER_INPUTS = ("color", "hit", "position", "variance", "length")


# ------------------------------------------------------------------ 4. hand-made hit planes
def _hand_made(sc, h=H, w=W, seed=29):
    """(hit plane, category (h, w)): sixteen categories, one pixel in sixteen each, interleaved so that every wave holds all of them"""
    rng = np.random.default_rng(seed)
    ntri = len(sc["tri_mesh"])
    ys, xs = np.mgrid[0:h, 0:w]
    cat = (xs + 3 * ys) % 16
    hit = np.zeros((h, w, 8), f32)
    words = hit.view(np.int32)
    hit[..., 0] = rng.random((h, w), dtype=f32) * 5 + 1
    words[..., 4] = rng.integers(-3, 9, (h, w))  # the record's mesh word is never used
    hit[..., 5:8] = rng.random((h, w, 3), dtype=f32)
    by_mesh = [np.nonzero(sc["tri_mesh"] == m)[0] for m in range(3)]
    textured = np.concatenate([by_mesh[0], by_mesh[1]])
    prim = rng.choice(textured, (h, w)).astype(np.int64)
    u, v = rng.random((h, w), dtype=f32) * f32(0.5), rng.random((h, w), dtype=f32) * f32(0.5)
    corners = {0: (0, 0), 1: (1, 0), 2: (0, 1)}
    for k, (cu, cv) in corners.items():
        u[cat == k], v[cat == k] = cu, cv
    e = rng.integers(0, 3, (h, w))
    s = rng.random((h, w), dtype=f32)
    u[cat == 3] = np.where(e == 0, s, np.where(e == 1, f32(0), s))[cat == 3]  # the three edges: v = 0, u = 0, u + v = 1
    v[cat == 3] = np.where(e == 0, f32(0), np.where(e == 1, s, f32(1) - s))[cat == 3]
    # primitive 0 (the ground, texture 0, 64 x 32): s = 4 (u + v) - 1.5, t = 4 v - 1.5, exact for multiples of 1/256
    prim[(cat == 4) | (cat == 5)] = 0
    u[cat == 4], v[cat == 4] = 0.25, 0.375  # (s, t) = (1, 0): exact integers
    a, b = rng.integers(0, 129, (h, w)), rng.integers(0, 129, (h, w))
    u[cat == 5], v[cat == 5] = (a / 256).astype(f32)[cat == 5], (b / 256).astype(f32)[cat == 5]  # texel borders and centres
    for k, m in ((6, 0), (7, 1), (8, 2)):
        prim[cat == k] = rng.choice(by_mesh[m], (h, w))[cat == k]
    prim[cat == 9], prim[cat == 10], prim[cat == 11], prim[cat == 12] = -1, ntri, 0x7FFFFFFF, -2
    u[cat == 13] = np.nan
    v[cat == 14] = np.where(rng.random((h, w)) < 0.5, f32(np.inf), f32(-np.inf))[cat == 14]
    prim[cat == 15] = rng.integers(0, ntri, (h, w))[cat == 15]
    nan_box = (cat == 15) & (sc["tri_mesh"][np.clip(prim, 0, ntri - 1)] == 2) & (xs % 2 == 0)
    u[nan_box] = np.nan  # non-finite barycentrics on the colour path: not read
    hit[..., 1], hit[..., 2] = u, v
    words[..., 3] = prim.astype(np.int32)
    return hit, cat, nan_box
