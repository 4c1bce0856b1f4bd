"""float32 NumPy evaluation of pt_motion_planes' arithmetic (include/pt_amd.h), shared by tests/test_motion_cabi.py and
tests/test_gpu_motion.py.  A helper, not a test.  One rounding per operation, in the header's order; it never calls the kernel under test.
The index array is built from the model's host arrays: global index = the mesh's own index + the mesh's first vertex."""
import numpy as np

import temporal_ref as T

f32 = np.float32
SENTINEL = T.SENTINEL
QNAN = 0x7FC00000
PLANES = ("motion", "prev_point", "prev_surface")
WORDS = {"motion": 2, "prev_point": 4, "prev_surface": 8}


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _normalize(v):
    return v * (f32(1.0) / np.sqrt(_dot(v, v)))[..., None]


def model_arrays(model):
    """(vertices (V, 3) float32 in pt_copy_vertices_device's layout, idx (T, 3) int64 global vertex indices) from the model's host arrays"""
    verts, idx, base = [], [], 0
    for m in model.meshes:
        verts.append(np.ascontiguousarray(m.vertex, f32).reshape(-1, 3))
        idx.append(np.asarray(m.index, np.int64).reshape(-1, 3) + base)
        base += len(verts[-1])
    return np.concatenate(verts), np.concatenate(idx)


def stack_vertices(per_mesh):
    return np.ascontiguousarray(np.concatenate([np.asarray(v, f32).reshape(-1, 3) for v in per_mesh]))


def _project(q, prev, x, y, wr, hr):
    """pt_render_gbuffer's projection block: (n, 2) uint32 bits"""
    pe, pU, pV, pW = prev[:, 0:3], prev[:, 3:6], prev[:, 6:9], prev[:, 9:12]
    VxW = _cross(pV, pW)
    a, b, c, det = _dot(q, VxW), _dot(q, _cross(pW, pU)), _dot(q, _cross(pU, pV)), _dot(pU, VxW)
    px = (((a / c) + f32(1.0)) * f32(0.5)) * wr.astype(f32) - f32(0.5)
    py = (((b / c) + f32(1.0)) * f32(0.5)) * hr.astype(f32) - f32(0.5)
    mx, my = px - x.astype(f32), py - y.astype(f32)
    ok = c * det > 0
    for arr in (a, c, det, px, mx, my):
        assert arr.dtype == f32
    m = np.stack([mx, my], -1).view(np.uint32).copy()
    m[~ok] = QNAN
    return m


def motion_ref(hit, prev_vertices, idx, rects, pixels, cams=None, prev_cams=None, planes=PLANES, fill=SENTINEL):
    """hit: (h, w, 8) float32 or its uint32 bits; prev_vertices (V, 3); idx (T, 3) global; rects: [(x0, y0, wr, hr)], the views, or
    [(0, 0, w, h)]; pixels: bool (h, w), the set the call processes; cams / prev_cams: (len(rects), 12) rows eye, U, V, W of the current and
    the previous frame (needed by "motion").  Returns {plane: uint32 bits of the whole plane, `fill` outside the set; hits, stale: int;
    kind: int8 (h, w): 0 outside the set, 1 hit, 2 miss, 3 stale}."""
    hit = np.ascontiguousarray(hit)
    hit = hit.view(f32) if hit.dtype == np.uint32 else np.ascontiguousarray(hit, f32)
    h, w = hit.shape[:2]
    pv = np.ascontiguousarray(prev_vertices, f32).reshape(-1, 3)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    ntri = len(idx)
    pixels = np.asarray(pixels, bool)
    Y, X = np.nonzero(pixels)
    n = len(Y)
    rid = np.full(n, -1)
    for k, (x0, y0, wr, hr) in enumerate(rects):
        inside = (X >= x0) & (X < x0 + wr) & (Y >= y0) & (Y < y0 + hr)
        assert (rid[inside] == -1).all()
        rid[inside] = k
    assert (rid >= 0).all(), "a pixel of the set lies in no rectangle"
    R = np.asarray(rects, np.int64).reshape(-1, 4)[rid]
    x, y, wr, hr = X - R[:, 0], Y - R[:, 1], R[:, 2], R[:, 3]
    rec = hit[Y, X]
    words = rec.view(np.int32)
    prim = words[:, 3]
    miss = prim < 0
    is_hit = ~miss & (prim < ntri)
    stale = ~miss & ~is_hit
    with np.errstate(all="ignore"):
        tri = idx[np.where(is_hit, prim, 0)]
        p0, p1, p2 = pv[tri[:, 0]], pv[tri[:, 1]], pv[tri[:, 2]]
        u, v = rec[:, 1], rec[:, 2]
        w0 = (f32(1.0) - u) - v
        Q = (p0 * w0[:, None] + p1 * u[:, None]) + p2 * v[:, None]
        ngp = _normalize(_cross(p1 - p0, p2 - p0))
        assert Q.dtype == f32 and ngp.dtype == f32 and w0.dtype == f32
        res = {}
        if "prev_point" in planes:
            pt = np.zeros((n, 4), f32)
            pt[is_hit, 0:3] = Q[is_hit]
            pt[is_hit, 3] = 1
            res["prev_point"] = np.full((h, w, 4), fill, np.uint32)
            res["prev_point"][Y, X] = pt.view(np.uint32)
        if "prev_surface" in planes:
            ps = rec.copy()
            ps[is_hit, 5:8] = ngp[is_hit]
            ps[stale, 1:3] = 0
            ps[stale, 5:8] = 0
            ps.view(np.int32)[stale, 3:5] = -1
            res["prev_surface"] = np.full((h, w, 8), fill, np.uint32)
            res["prev_surface"][Y, X] = ps.view(np.uint32)
        if "motion" in planes:
            cams, prev_cams = np.asarray(cams, f32).reshape(-1, 12)[rid], np.asarray(prev_cams, f32).reshape(-1, 12)[rid]
            dx = f32(2.0) * ((x.astype(f32) + f32(0.5)) / wr.astype(f32)) - f32(1.0)
            dy = f32(2.0) * ((y.astype(f32) + f32(0.5)) / hr.astype(f32)) - f32(1.0)
            d = _normalize((cams[:, 3:6] * dx[:, None] + cams[:, 6:9] * dy[:, None]) + cams[:, 9:12])
            q = np.where(is_hit[:, None], Q - prev_cams[:, 0:3], d).astype(f32)
            assert d.dtype == f32
            m = _project(q, prev_cams, x, y, wr, hr)
            m[stale] = QNAN
            res["motion"] = np.full((h, w, 2), fill, np.uint32)
            res["motion"][Y, X] = m
    res["hits"], res["stale"] = int(is_hit.sum()), int(stale.sum())
    res["kind"] = np.zeros((h, w), np.int8)
    res["kind"][Y, X] = np.where(is_hit, 1, np.where(miss, 2, 3))
    return res


# ------------------------------------------------------------------ CPU planes with barycentrics
def fill_uv(rec, model, row, w, h):
    """A copy of the hit plane `rec` (h, w, 8) with u, v filled by the header's expression for pt_hit, from the ray of each pixel's centre
    under the camera row: A = v0 - o, B = v1 - o, C = v2 - o; Uw = dot(d, cross(C, B)), Vw = dot(d, cross(A, C)), Ww = dot(d, cross(B, A));
    det = (Uw + Vw) + Ww; u = Vw / det; v = Ww / det"""
    import gbuffer_ref as G

    verts, idx = model_arrays(model)
    rays = G._np_rays(row, w, h)
    o, d = rays[..., 0:3], rays[..., 4:7]
    prim = rec.view(np.int32)[..., 3]
    hit = prim >= 0
    tri = idx[np.maximum(prim, 0)]
    A, B, Cc = verts[tri[..., 0]] - o, verts[tri[..., 1]] - o, verts[tri[..., 2]] - o
    with np.errstate(all="ignore"):
        Uw, Vw, Ww = _dot(d, _cross(Cc, B)), _dot(d, _cross(A, Cc)), _dot(d, _cross(B, A))
        det = (Uw + Vw) + Ww
        u, v = Vw / det, Ww / det
    assert u.dtype == f32
    out = np.array(rec, f32)
    out[..., 1] = np.where(hit, u, f32(0))
    out[..., 2] = np.where(hit, v, f32(0))
    return out


def cpu_planes(orc, model, size, cam_dict, prev_dict):
    """temporal_ref.cpu_planes with u, v of both hit planes filled in (that helper leaves them 0)"""
    import gbuffer_ref as G

    w, h = size
    P = T.cpu_planes(orc, model, size, cam_dict, prev_dict)
    P["hit"] = fill_uv(P["hit"], model, G._row(cam_dict, w / h), w, h)
    P["prev_hit"] = fill_uv(P["prev_hit"], model, G._row(prev_dict, w / h), w, h)
    return P


# ------------------------------------------------------------------ the hand-made scene of the normal-wise move
QUAD_CAMERA = dict(eye=(0.0, 1.0, -5.0), lookat=(0.0, 1.0, 0.0), up=(0.0, 1.0, 0.0), fovY=40.0)
QUAD_SIZE = (64, 40)
QUAD_DELTA = 0.25  # towards the camera; plane_eps * max t = 0.01 * 1e16 at a miss, but the plane test only runs at hits: t < 8 there


def quad_scene(dz=0.0):
    """mesh 0: a floor at y = 0; mesh 1: a 2.4 x 1.6 quad in the plane z = -dz facing the camera (normal -z), centred at (0, 1)"""
    from optixpathtracer_amd import scenes

    floor = scenes._quads_to_mesh([[(-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6)]], scenes.Material())
    z = -float(dz)
    quad = scenes._quads_to_mesh([[(-1.2, 0.2, z), (-1.2, 1.8, z), (1.2, 1.8, z), (1.2, 0.2, z)]], scenes.Material())
    return scenes.Model(meshes=[floor, quad])
