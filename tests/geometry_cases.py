"""The inputs, checks and recorded bounds of the reprojection chain against float64 geometry (tests/geometry_ref.py):
tests/test_geometry_cabi.py measures and pins every figure on CPU-built planes (its docstring states the rule for the bounds),
tests/test_gpu_geometry.py applies the same check_* functions to the GPU's planes.  NumPy only."""
import numpy as np

import geometry_ref as G64
import motion_ref as M
import plan_ref as PL
import surface_ref as S
import temporal_ref as T


f32 = np.float32
W, H = 131, 61
MOVES = ("a", "b", "c")
VIEW_RECTS = [(0, 0, 61, 37), (64, 0, 67, 29)]  # scene_kit.RECTS[:2]: off the 8x8 block grid


# ------------------------------------------------------------------ inputs
def turned(cam_dict):
    """a previous camera that is also turned (the look-at point shifted sideways and up by a tenth of the eye distance) and zoomed (fovY x 1.1)"""
    e, l = np.asarray(cam_dict["eye"], np.float64), np.asarray(cam_dict["lookat"], np.float64)
    s = 0.1 * float(np.linalg.norm(l - e))
    return dict(cam_dict, lookat=(float(l[0] + s * 0.8), float(l[1] + s * 0.6), float(l[2])), fovY=cam_dict["fovY"] * 1.1)


def scenes_and_cameras():
    """name -> (model factory, current camera): the inputs of temporal_ref.real_inputs()"""
    return {name: (make, cam) for name, (make, _, cam, _, _, _) in T.real_inputs().items()}


def previous_camera(name, move):
    """(a) a small dolly and side step, (b) the large move of temporal_ref.real_inputs(), (c) turned and zoomed"""
    _, _, cam, large, _, _ = T.real_inputs()[name]
    return {"a": T.forward(cam, 0.1, dx=0.25), "b": large, "c": turned(cam)}[move]


def view_cameras():
    """(current camera dicts, previous camera dicts) of the two views: view 0 moves as (a), view 1 as (c)"""
    from scene_kit import _cam_dicts

    cur = _cam_dicts()[:2]
    return cur, [T.forward(cur[0], 0.1, dx=0.25), turned(cur[1])]


def scene_size(model):
    """the scene's largest |coordinate|"""
    return float(max(np.abs(np.asarray(m.vertex, np.float64)).max() for m in model.meshes))


OBJECT_CAMERA_MOVE = dict(f=0.05, dx=0.1)


def object_move(model, mesh):
    """(R, c, t, A): mesh `mesh` turned by 0.05 rad about (0.2, 1, 0.1) through its centroid and shifted by 3 % of the scene size along
    (1, 0.5, -0.7); A: the float32 3x4 matrix transformMeshes takes"""
    v = np.asarray(model.meshes[mesh].vertex, np.float64).reshape(-1, 3)
    R = G64.rotation((0.2, 1.0, 0.1), 0.05)
    c = v.mean(0)
    t = 0.03 * scene_size(model) * np.array([1.0, 0.5, -0.7]) / np.linalg.norm([1.0, 0.5, -0.7])
    return R, c, t, G64.rigid_matrix(R, c, t).astype(f32)


def most_visible_mesh(hit):
    mesh = np.ascontiguousarray(hit).view(np.int32)[..., 4]
    ids, counts = np.unique(mesh[mesh >= 0], return_counts=True)
    return int(ids[np.argmax(counts)])


OBJECT_MESH = {"two_box": 0}  # the terrain: the mesh most pixels show (most_visible_mesh of the unmoved scene's hit plane)


# ------------------------------------------------------------------ the checks (shared with tests/test_gpu_geometry.py)
def _local_xy(rect, shape):
    h, w = shape
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs - rect[0], ys - rect[1]], -1).astype(np.float64)


def _in_rect(rect, shape):
    x0, y0, wr, hr = rect
    m = np.zeros(shape, bool)
    m[y0:y0 + hr, x0:x0 + wr] = True
    return m


def lookups(motion, rect):
    """(lookup (h, w, 2): a pixel's own coordinates in its rectangle plus its motion vector — the way every consumer of the chain reads the
    plane; inside (h, w): finite and within the rectangle's pixel centres)"""
    motion = np.asarray(motion, np.float64)
    xy = _local_xy(rect, motion.shape[:2]) + motion
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(xy).all(-1) & (xy[..., 0] >= 0) & (xy[..., 0] <= rect[2] - 1) & (xy[..., 1] >= 0) & (xy[..., 1] <= rect[3] - 1)
    return xy, inside & _in_rect(rect, motion.shape[:2])


def check_camera_motion(motion, hit, position, rays, prev_rays, rect, size):
    """T1 in one rectangle.  hit pixels: the position plane's point must have been seen at the pixel's lookup by the previous frame's rays.
    miss pixels: a point at infinity — the point one scene size along the pixel's ray, seen from the current eye with the previous frame's
    ray directions.  Returns dict(hit_err: px per checked hit pixel, hits, miss_err, misses: the pixels of the rectangle of either kind)."""
    shape = np.asarray(motion).shape[:2]
    xy, inside = lookups(motion, rect)
    is_hit = np.ascontiguousarray(hit).view(np.int32)[..., 3] >= 0
    inr = _in_rect(rect, shape)
    sel = inside & is_hit
    hit_err = G64.lookup_error_px(np.asarray(position, np.float64)[sel][:, :3], prev_rays, xy[sel], rect)
    sel_m = inside & ~is_hit
    cur = np.asarray(rays, np.float64)
    far = cur[sel_m][:, 0:3] + size * cur[sel_m][:, 4:7]
    from_here = np.array(prev_rays, np.float64)
    from_here[..., 0:3] = cur[..., 0:3]
    miss_err = G64.lookup_error_px(far, from_here, xy[sel_m], rect)
    return dict(hit_err=hit_err, hits=int((is_hit & inr).sum()), miss_err=miss_err, misses=int((~is_hit & inr).sum()))


def check_object_motion(planes, hit, position, prev_rays, mesh, R, c, t, size):
    """T2 on the whole frame.  planes: motion, prev_point, prev_surface of motionPlanes; hit, position: this frame's G-buffer planes.
    Returns dict(point_err: the largest |prev_point - truth| over the scene size, on and off the moved mesh; lookup_err: px per checked
    pixel; normal_err: the largest |prev_surface normal - R^T ng| on the moved mesh; on, hits: pixels of the moved mesh, hit pixels)."""
    hit = np.ascontiguousarray(hit, f32)
    words = hit.view(np.int32)
    is_hit, on = words[..., 3] >= 0, (words[..., 3] >= 0) & (words[..., 4] == mesh)
    pos = np.asarray(position, np.float64)[..., :3]
    truth = np.where(on[..., None], G64.inverse_rigid(pos, R, c, t), pos)
    pp = np.asarray(planes["prev_point"], np.float64)
    assert (pp[..., 3][is_hit] == 1).all(), "prev_point.w is not 1 on every hit"
    d = np.linalg.norm(pp[..., :3] - truth, axis=-1) / size
    rect = (0, 0, hit.shape[1], hit.shape[0])
    xy, inside = lookups(planes["motion"], rect)
    sel = inside & is_hit
    lookup_err = G64.lookup_error_px(truth[sel], prev_rays, xy[sel], rect)
    ng = np.asarray(hit[..., 5:8], np.float64)
    was = ng @ np.asarray(R, np.float64)  # R^T applied to each normal
    ps = np.asarray(planes["prev_surface"], np.float64)[..., 5:8]
    normal_err = np.linalg.norm(ps - was, axis=-1)[on].max()
    normal_off = np.linalg.norm(ps - ng, axis=-1)[is_hit & ~on].max()
    return dict(point_on=float(d[on].max()), point_off=float(d[is_hit & ~on].max()), lookup_err=lookup_err, checked=int(sel.sum()),
                normal_err=float(max(normal_err, normal_off)), on=int(on.sum()), hits=int(is_hit.sum()))


def model_texcoords(model):
    """(V, 2) float64 in the global vertex order of motion_ref.model_arrays: a mesh's own texcoords, zeros where it has none"""
    out = []
    for m in model.meshes:
        has = m.texcoord is not None and len(m.texcoord) > 0
        out.append(np.asarray(m.texcoord, np.float64).reshape(-1, 2) if has else np.zeros((len(m.vertex), 2)))
    return np.concatenate(out)


def check_barycentrics(hit, position, texcoord, model, textured_meshes):
    """T3.  hit.u, hit.v against the least-squares coordinates of the position plane's point in the model's own triangle; the texcoord plane
    against the model's texcoords at those coordinates, on the meshes that take the texture path.  Returns dict(uv_err, st_err: the largest
    absolute differences; hits, textured: pixels)."""
    verts, idx = M.model_arrays(model)
    hit = np.ascontiguousarray(hit, f32)
    words = hit.view(np.int32)
    is_hit = words[..., 3] >= 0
    tri = idx[words[..., 3][is_hit]]
    u, v = G64.barycentric(np.asarray(position, np.float64)[is_hit][:, :3], verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]])
    uv_err = max(np.abs(hit[..., 1][is_hit] - u).max(), np.abs(hit[..., 2][is_hit] - v).max())
    tc = model_texcoords(model)
    st = G64.interpolate(u, v, tc[tri[:, 0]], tc[tri[:, 1]], tc[tri[:, 2]])
    tex = np.isin(words[..., 4][is_hit], textured_meshes)
    st_err = np.abs(np.asarray(texcoord, np.float64)[is_hit][tex] - st[tex]).max()
    return dict(uv_err=float(uv_err), st_err=float(st_err), hits=int(is_hit.sum()), textured=int(tex.sum()))


CARRY_MEDIAN, CARRY_SHARE, CARRY_COVERAGE = 0.1, 0.99, 0.5  # T4's conditions, fixed before anything was measured (profiles/geometry.md: right and wrong lie a factor of four apart at least)


def check_carry(history_out, valid, truth, motion, prev_position, prev_hit, is_hit, rect=None):
    """T4.  history_out: what a consumer made of history_in = the previous frame's position plane; valid: the pixels where it reprojected;
    truth (h, w, 3): where each pixel's surface point was in the previous frame.  At the valid hit pixels whose four taps are hits of the
    previous frame, |history_out - truth| is compared with the taps' diameter d.  Returns (median of error / d, share with error <= d,
    share of the hit pixels checked)."""
    shape = np.asarray(motion).shape[:2]
    rect = rect or (0, 0, shape[1], shape[0])
    xy, _ = lookups(motion, rect)
    prev_is_hit = np.ascontiguousarray(prev_hit).view(np.int32)[..., 3] >= 0
    sel = np.asarray(valid, bool) & np.asarray(is_hit, bool) & _in_rect(rect, shape)
    d, ok = G64.tap_diameter(prev_position, prev_is_hit, xy[sel], rect)
    err = np.linalg.norm(np.asarray(history_out, np.float64)[sel][:, :3] - np.asarray(truth, np.float64)[sel], axis=1)[ok]
    ratio = err / d[ok]
    return float(np.median(ratio)), float((ratio <= 1).mean()), float(ok.sum() / max(1, int((np.asarray(is_hit, bool) & _in_rect(rect, shape)).sum())))


def carry_passes(result):
    med, share, cover = result
    return med <= CARRY_MEDIAN, share >= CARRY_SHARE, cover >= CARRY_COVERAGE


def position_history(prev_position):
    """the previous frame's position plane as a colour history: w = 1 everywhere"""
    h = np.array(prev_position, f32)
    h[..., 3] = 1
    return h


# ------------------------------------------------------------------ CPU-built planes, once per input
_CACHE = {}


def _cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def _rays(cam_dict, w, h):
    import gbuffer_ref as G

    return G._np_rays(G._row(cam_dict, w / h), w, h)


def camera_case(orc, name, move):
    def build():
        make, cam = scenes_and_cameras()[name]
        model = _cached(("model", name), make)
        prev = previous_camera(name, move)
        P = T.cpu_planes(orc, model, (W, H), cam, prev)
        return dict(P, rays=_rays(cam, W, H), prev_rays=_rays(prev, W, H), size=scene_size(model), cam=cam, prev=prev, model=model)

    return _cached(("camera", name, move), build)


def view_case(orc, swapped=False):
    """the two views' planes side by side in one 131 x 61 frame, as renderGBuffer lays them out; swapped: each view's motion computed
    against the OTHER view's previous camera"""
    def build():
        make, _ = scenes_and_cameras()["two_box"]
        model = _cached(("model", "two_box"), make)
        cur, prev = view_cameras()
        out = dict(motion=np.full((H, W, 2), np.nan, f32), hit=np.zeros((H, W, 8), f32), position=np.zeros((H, W, 4), f32),
                   rays=np.zeros((H, W, 8), f32), prev_rays=np.zeros((H, W, 8), f32), size=scene_size(model))
        for k, (x, y, w, h) in enumerate(VIEW_RECTS):
            P = T.cpu_planes(orc, model, (w, h), cur[k], prev[1 - k] if swapped else prev[k])
            for plane in ("motion", "hit", "position"):
                out[plane][y:y + h, x:x + w] = P[plane]
            out["rays"][y:y + h, x:x + w] = _rays(cur[k], w, h)
            out["prev_rays"][y:y + h, x:x + w] = _rays(prev[k], w, h)
        return out

    return _cached(("views", swapped), build)


def object_case(orc, name):
    def build():
        import gbuffer_ref as G
        from scene_kit import _np_transform, _with_vertices

        make, cam = scenes_and_cameras()[name]
        model = _cached(("model", name), make)
        prev = T.forward(cam, OBJECT_CAMERA_MOVE["f"], dx=OBJECT_CAMERA_MOVE["dx"])
        old = M.cpu_planes(orc, model, (W, H), prev, prev)
        mesh = OBJECT_MESH.get(name)
        if mesh is None:
            mesh = most_visible_mesh(T.cpu_planes(orc, model, (W, H), cam, cam)["hit"])
        R, c, t, A = object_move(model, mesh)
        moved = _with_vertices(model, {mesh: _np_transform(A, model.meshes[mesh].vertex)})
        cur = M.cpu_planes(orc, moved, (W, H), cam, prev)
        verts, idx = M.model_arrays(model)
        rows = dict(cams=[G._row(cam, W / H)], prev_cams=[G._row(prev, W / H)])
        return dict(cur=cur, old=old, mesh=mesh, R=R, c=c, t=t, A=A, verts=verts, idx=idx, rows=rows, prev_rays=_rays(prev, W, H),
                    size=scene_size(model), model=model, moved=moved)

    return _cached(("object", name), build)


def _motion_planes(c, hit):
    ref = M.motion_ref(hit, c["verts"], c["idx"], [(0, 0, W, H)], np.ones((H, W), bool), **c["rows"])
    assert ref["stale"] == 0, f"the reference counts {ref['stale']} stale records on planes that have none"
    return {k: ref[k].view(f32) for k in M.PLANES}


def _swap_uv(hit):
    out = np.array(hit, f32)
    out[..., 1], out[..., 2] = np.array(hit, f32)[..., 2], np.array(hit, f32)[..., 1]
    return out


# ------------------------------------------------------------------ T1: camera motion
# the largest lookup error of the float32 G-buffer formulas against the previous frame's own rays, in pixels, at hits and at misses
T1_MEASURED_PX = {
    ("two_box", "a"): 2.44e-5, ("two_box", "b"): 1.78e-5, ("two_box", "c"): 2.43e-5,
    ("terrain", "a"): 2.14e-5, ("terrain", "b"): 2.01e-5, ("terrain", "c"): 1.56e-5,
    "views": 1.18e-5,
}
T1_BOUND_PX = {k: 4 * v for k, v in T1_MEASURED_PX.items()}
T1_COVERAGE = 0.2  # of the hit pixels, in every case


def _t1_figures(res, what):
    e, m = res["hit_err"], res["miss_err"]
    worst = float(max(e.max(), m.max() if len(m) else 0.0))
    print(f"T1 {what}: hits checked {len(e)} of {res['hits']}, largest {e.max():.3e} px, median {np.median(e):.3e}; misses checked {len(m)} of "
          f"{res['misses']}, largest {m.max() if len(m) else 0.0:.3e}")
    return worst


# ------------------------------------------------------------------ T2: object motion
# per input: |prev_point - truth| / scene size on the moved mesh, off it; lookup error in px; |normal - R^T ng|
T2_MEASURED = {
    "two_box": dict(point_on=3.36e-7, point_off=5.97e-7, lookup_px=2.91e-5, normal=9.38e-8),  # mesh 0 (the unit box): 421 of 4862 hit pixels
    "terrain": dict(point_on=1.19e-5, point_off=5.83e-7, lookup_px=4.99e-4, normal=2.27e-6),  # mesh 4: 1742 of 5142 hit pixels
}
T2_BOUND = {name: {k: 4 * v for k, v in m.items()} for name, m in T2_MEASURED.items()}
T2_COVERAGE = 0.05  # of the hit pixels show the moved mesh


def t2_figures(res, what):
    got = dict(point_on=res["point_on"], point_off=res["point_off"], lookup_px=float(res["lookup_err"].max()), normal=res["normal_err"])
    print(f"T2 {what}: moved mesh on {res['on']} of {res['hits']} hit pixels; " + ", ".join(f"{k} {v:.3e}" for k, v in got.items()) +
          f"; lookups checked {res['checked']}, median {np.median(res['lookup_err']):.3e} px")
    return got


# ------------------------------------------------------------------ T3: barycentrics and texcoords
T3_MEASURED = dict(uv=7.23e-7, st=7.16e-7)  # the largest |u - u64|, |v - v64|; the largest |texcoord - truth| per component
T3_BOUND = {k: 4 * v for k, v in T3_MEASURED.items()}
TEXTURED_MESHES = (0, 1)


def textured_case(orc):
    def build():
        model = S.textured_scene()
        P = M.cpu_planes(orc, model, (W, H), S.TEX_CAMERA, S.TEX_CAMERA)
        return dict(model=model, hit=P["hit"], position=P["position"], sc=S.scene_arrays(model), cam=S.TEX_CAMERA)

    return _cached("textured", build)


def check_texcoords_tell_v1_from_v2(model):
    """every textured triangle's texcoords change when v1 and v2 change places, and so does the map as a whole: no symmetry hides a swap"""
    sc = S.scene_arrays(model)
    tex = sc["mesh_tex"][sc["tri_mesh"]] >= 0
    uv = sc["uv"][tex]
    assert tex.sum() >= 4 and (np.abs(uv[:, 2:4] - uv[:, 4:6]).max(1) >= 1.0).all(), "the textured triangles' texcoords at v1 and v2 are less than 1 apart: swapped u, v would not show"


# ------------------------------------------------------------------ T4: the consumers read the motion the way the producers write it
CARRY_LENGTH = 5.0


def carry_inputs(P):
    """plan_ref's eight inputs: history_in = the previous frame's position plane, length 5 everywhere, zero moments"""
    h, w = P["motion"].shape[:2]
    return dict(motion=P["motion"], hit=P["hit"], position=P["position"], prev_hit=P["prev_hit"], prev_position=P["prev_position"],
                history_in=position_history(P["prev_position"]), moments_in=np.zeros((h, w, 2), f32), length_in=np.full((h, w), CARRY_LENGTH, f32))


def _carry(P, truth, name, motion=None):
    planes = carry_inputs(P if motion is None else dict(P, motion=motion))
    ref = PL.carry_ref(planes, [(0, 0, W, H)], np.ones((H, W), bool), **PL.REAL_GATHER[name])
    is_hit = np.ascontiguousarray(P["hit"]).view(np.int32)[..., 3] >= 0
    return check_carry(ref["history_out"].view(f32), ref["valid"], truth, planes["motion"], P["prev_position"], P["prev_hit"], is_hit)


# ------------------------------------------------------------------ T5: the point of the chain, under motion
ORBIT = dict(size=(64, 48), frames=8, spp=1, reference_spp=256, step=0.03)  # the issue's first choice; see the test's docstring


def orbit(cam_dict, angle):
    """the camera turned by `angle` radians about the vertical axis through its look-at point, as the examples' orbit() turns it"""
    e, l = np.asarray(cam_dict["eye"], np.float64), np.asarray(cam_dict["lookat"], np.float64)
    d = e - l
    c, s = np.cos(angle), np.sin(angle)
    return dict(cam_dict, eye=(float(l[0] + c * d[0] + s * d[2]), float(e[1]), float(l[2] - s * d[0] + c * d[2])))


def orbit_cameras():
    from optixpathtracer_amd import scenes

    return [orbit(scenes.TWO_BOX_CAMERA, ORBIT["step"] * k) for k in range(ORBIT["frames"])]
