"""float32 NumPy evaluation of pt_edge_aa_planes' rule, written from the text of include/pt_amd.h alone; shared by tests/test_edge_aa_cabi.py
and tests/test_gpu_edge_aa.py.  A helper, not a test.  One rounding per operation, in the header's order, no fused multiply-add; it never
calls the kernel under test.  The float64 half at the end (the crossing of a triangle's edge restated, the supersampled truth) uses no
expression of the header."""
import numpy as np

import conftest  # noqa: F401  (puts the repository's root on sys.path)
import surface_ref as S
from motion_ref import _cross, _dot
from optixpathtracer_amd import scenes
from surface_lod_ref import _rays, camera_rays64

f32 = np.float32
SENTINEL = S.SENTINEL
PLANES = ("out", "edge", "frame_rgba8")
WORDS = {"out": 4, "edge": 2, "frame_rgba8": 1}
DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1))


def _finite3(c):
    return ((np.ascontiguousarray(c, f32).view(np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)).all(-1)


def _max0(v):
    return np.where(v > 0, v, f32(0)).astype(f32)  # a NaN gives 0


def edge_aa_ref(hit, position, color, verts, idx, rects, cams, pixels, normal_cos=0.9, plane_eps=0.01, planes=("out", "edge"), fill=SENTINEL, orc=None,
                owner="near", zero_weight=False):
    """hit: (h, w, 8) float32 or its bits; position, color: (h, w, 4); verts (V, 3) the CURRENT vertices, idx (T, 3) global
    (motion_ref.model_arrays); rects: [(x0, y0, wr, hr)], the views, or [(0, 0, w, h)]; cams: (len(rects), 12) rows eye, U, V, W; pixels:
    bool (h, w), the set the call processes (a neighbour inside the pixel's rectangle is in a block of the call's set exactly when it is
    in the pixel set).  orc: the CPU checker, needed by "frame_rgba8" alone (its make_color).
    owner="far" and zero_weight=True are the two controls of tests/test_edge_aa_cabi.py, not the header's rule.
    Returns {plane: uint32 bits of the whole plane, `fill` outside the set; pixels, hits, stale, boundary, blended: int; Y, X: the set's
    pixels in order; per direction (n, 4): cand, own_p, s, dist, w, oprim, xr, yr and b_r (n, 4, 3): the header's step 3 as evaluated}."""
    def as_f32(a):
        a = np.ascontiguousarray(a)
        return a.view(f32) if a.dtype == np.uint32 else np.ascontiguousarray(a, f32)

    hit, position, color = as_f32(hit), as_f32(position), as_f32(color)
    h, w = hit.shape[:2]
    verts = np.ascontiguousarray(verts, f32).reshape(-1, 3)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    ntri = len(idx)
    pixels = np.asarray(pixels, bool)
    Y, X = np.nonzero(pixels)
    n = len(Y)
    rid = np.full(n, -1)
    for k, (x0, y0, wr, hr) in enumerate(rects):
        rid[(X >= x0) & (X < x0 + wr) & (Y >= y0) & (Y < y0 + hr)] = k
    assert (rid >= 0).all(), "a pixel of the set lies in no rectangle"
    R = np.asarray(rects, np.int64).reshape(-1, 4)[rid] if n else np.zeros((0, 4), np.int64)
    x, y = X - R[:, 0], Y - R[:, 1]
    wr, hr = R[:, 2].astype(f32), R[:, 3].astype(f32)
    cam = np.asarray(cams, f32).reshape(-1, 12)[rid] if n else np.zeros((0, 12), f32)
    eye = cam[:, 0:3]
    ncos, eps = f32(normal_cos), f32(plane_eps)
    half, one = f32(0.5), f32(1.0)

    rec_p = hit[Y, X]
    prim_p = rec_p.view(np.int32)[:, 3].astype(np.int64)
    miss_p = prim_p < 0
    mesh_p = rec_p.view(np.int32)[:, 4]
    ng_p, pos_p, t_p = rec_p[:, 5:8], position[Y, X, 0:3], rec_p[:, 0]
    c_p = color[Y, X, 0:3]
    fin_p = _finite3(c_p)

    D = {k: np.zeros((n, 4), t) for k, t in (("cand", bool), ("own_p", bool), ("s", f32), ("dist", f32), ("w", f32), ("oprim", np.int64), ("xr", np.int64),
                                              ("yr", np.int64), ("good", bool))}
    D["b_r"] = np.zeros((n, 4, 3), f32)
    wbest, kbest, cbest = np.zeros(n, f32), np.full(n, -1), np.zeros((n, 3), f32)
    with np.errstate(all="ignore"):
        for k, (dx, dy) in enumerate(DIRS):
            qx, qy = X + dx, Y + dy
            inrect = (qx >= R[:, 0]) & (qx < R[:, 0] + R[:, 2]) & (qy >= R[:, 1]) & (qy < R[:, 1] + R[:, 3])
            qxc, qyc = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            reach = inrect & pixels[qyc, qxc]
            rec_q = hit[qyc, qxc]
            prim_q = rec_q.view(np.int32)[:, 3].astype(np.int64)
            miss_q = prim_q < 0
            c_q = color[qyc, qxc, 0:3]
            # ---- 2. the candidate test
            facet = (rec_q.view(np.int32)[:, 4] == mesh_p) & (_dot(ng_p, rec_q[:, 5:8]) >= ncos)
            plane = np.abs(_dot(ng_p, position[qyc, qxc, 0:3] - pos_p)) <= eps * t_p
            same = ~miss_p & ~miss_q & ((prim_q == prim_p) | (facet & plane))
            cand = fin_p & reach & _finite3(c_q) & ~(miss_p & miss_q) & ~same
            # ---- 3. the owner, the crossing
            own_p = np.where(miss_p, False, np.where(miss_q, True, t_p <= rec_q[:, 0]))  # a NaN gives q
            if owner == "far":  # the control: the other pixel of the pair owns the edge, a miss included (it has no primitive: dropped)
                own_p = ~own_p
            rec_o = np.where(own_p[:, None], rec_p, rec_q)
            oprim = np.where(own_p, prim_p, prim_q)
            in_range = (oprim >= 0) & (oprim < ntri)
            xr, yr = np.where(own_p, x + dx, x), np.where(own_p, y + dy, y)
            tri = idx[np.where(in_range, oprim, 0)] if ntri else np.zeros((n, 3), np.int64)
            p0, p1, p2 = verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]]
            e1, e2 = p1 - p0, p2 - p0
            nrm = _cross(e1, e2)
            nn, hgt = _dot(nrm, nrm), _dot(nrm, p0 - eye)
            d_r = _rays(cam, xr.astype(f32) + half, yr.astype(f32) + half, wr, hr)
            t_r = hgt / _dot(nrm, d_r)
            g = (d_r * t_r[:, None] + eye) - p0
            u_r, v_r = _dot(_cross(g, e2), nrm) / nn, _dot(_cross(e1, g), nrm) / nn
            b_r = np.stack([(one - u_r) - v_r, u_r, v_r], -1)
            u_o, v_o = rec_o[:, 1], rec_o[:, 2]
            b_o = np.stack([_max0((one - u_o) - v_o), _max0(u_o), _max0(v_o)], -1)
            assert b_r.dtype == f32 and b_o.dtype == f32 and t_r.dtype == f32 and d_r.dtype == f32
            s, found = np.full(n, np.nan, f32), np.zeros(n, bool)
            for i in range(3):
                neg = b_r[:, i] < 0
                s_i = b_o[:, i] / (b_o[:, i] - b_r[:, i])
                take = neg & (~found | (s_i < s))
                s = np.where(take, s_i, s).astype(f32)
                found |= neg
            dist = np.where(own_p, s, one - s).astype(f32)
            good = cand & in_range & (t_r > 0) & found & (dist < half)
            wk = np.where(good, half - dist, f32(0)).astype(f32)
            # ---- 4. the strongest direction, the first of equals
            take = good & (wk > wbest)
            wbest, kbest = np.where(take, wk, wbest).astype(f32), np.where(take, k, kbest)
            cbest = np.where(take[:, None], c_q, cbest).astype(f32)
            for name, v in (("cand", cand), ("own_p", own_p), ("s", s), ("dist", dist), ("w", wk), ("oprim", oprim), ("xr", xr), ("yr", yr), ("good", good)):
                D[name][:, k] = v
            D["b_r"][:, k] = b_r
        blended = kbest >= 0
        wuse = np.zeros(n, f32) if zero_weight else wbest
        rgb = np.where(blended[:, None], c_p + (cbest - c_p) * wuse[:, None], c_p).astype(f32)
    out = np.concatenate([rgb, np.ones((n, 1), f32)], -1)
    edge = np.stack([wbest, (kbest + 1).astype(f32)], -1).astype(f32)
    res = {}
    if "out" in planes:
        res["out"] = np.full((h, w, 4), fill, np.uint32)
        res["out"][Y, X] = out.view(np.uint32)
    if "edge" in planes:
        res["edge"] = np.full((h, w, 2), fill, np.uint32)
        res["edge"][Y, X] = edge.view(np.uint32)
    if "frame_rgba8" in planes:
        import temporal_ref as T

        res["frame_rgba8"] = np.full((h, w, 1), fill, np.uint32)
        if n:
            res["frame_rgba8"][Y, X, 0] = T.make_color_bits(orc, np.ascontiguousarray(rgb))
    res.update(pixels=n, hits=int((~miss_p & (prim_p < ntri)).sum()), stale=int((prim_p >= ntri).sum()), boundary=int(D["cand"].any(1).sum()),
               blended=int(blended.sum()), Y=Y, X=X, rgb=rgb, **D)
    return res


# ------------------------------------------------------------------ float64, no expression of the header
def crossing64(row, wr, hr, tri, xo, yo, xr, yr):
    """Where the line from the centre of pixel (xo, yo) to the centre of (xr, yr) (local coordinates of a wr x hr rectangle under the camera
    row) leaves the triangle tri (3, 3), as seen from the eye: both centre rays are intersected with the triangle's plane, the barycentrics
    (by least squares on the edge matrix) are linear along the segment between the two plane points, and the first of them to reach 0 names
    the place.  Returns (s in [0, 1] from o's centre, or NaN; the barycentrics of r's point (3,)) in float64."""
    row, tri = np.asarray(row, np.float64), np.asarray(tri, np.float64)
    o = row[0:3]
    nrm = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    E = np.stack([tri[1] - tri[0], tri[2] - tri[0]], -1)
    pinv = np.linalg.pinv(E)

    def bary(px, py):
        d = camera_rays64(row, wr, hr, np.array([px + 0.5]), np.array([py + 0.5]))[0]
        tt = np.dot(tri[0] - o, nrm) / np.dot(d, nrm)
        ab = pinv @ (o + d * tt - tri[0])
        return np.array([1.0 - ab[0] - ab[1], ab[0], ab[1]]), tt

    bo, _ = bary(xo, yo)
    br, tt = bary(xr, yr)
    bo = np.maximum(bo, 0.0)
    neg = br < 0
    if not (tt > 0) or not neg.any():
        return np.nan, br
    return float(np.min(bo[neg] / (bo[neg] - br[neg]))), br


def box_average(plane, S_):
    """(S*h, S*w, k) -> (h, w, k) float64: the mean over every S x S block"""
    hh, ww, k = plane.shape
    return np.asarray(plane, np.float64).reshape(hh // S_, S_, ww // S_, S_, k).mean((1, 3))


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


# ------------------------------------------------------------------ the inputs and the figure the tests share (tests/test_edge_aa_cabi.py measures and pins it)
W, H = 131, 59
SUPER = 8
# measured 0.30530 (rms 0.009637 after the rule, 0.031566 before it; 1140 boundary pixels, 556 blended, of 7729); the owner inverted gives
# 0.71213, every weight forced to 0 gives 1.00000, against the bound (1 + R_EDGE) / 2 = 0.6525: see
# test_reference_output_is_closer_to_the_supersampled_truth.  With a 4 x 4 supersample as the truth the same rule gives 0.43955 (recorded only).
R_EDGE = 0.305
INPUTS = {"cornell": (scenes.cornell_box, scenes.CORNELL_CAMERA), "textured": (S.textured_scene, dict(eye=(2.0, 0.35, -3.0), lookat=(0.0, 0.2, 0.5), up=(0.0, 1.0, 0.0), fovY=35.0))}


def supersampled_truth(albedo_big, s=SUPER):
    """(s*h, s*w, >=3) float32 pixel-centre albedo of the s times larger frame -> (h, w, 3) float64"""
    return box_average(np.asarray(albedo_big)[..., 0:3], s)
