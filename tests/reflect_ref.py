"""NumPy evaluation of pt_reflect_layout's and pt_reflect_planes's rules, written from the text of include/pt_amd.h alone; shared by
tests/test_reflect_cabi.py and tests/test_gpu_reflect.py.  A helper, not a test; it never calls the kernels under test.  Everything is
float32 arrays and float32 scalars, one rounding per operation, in the header's order (NumPy never contracts a product and a sum; its sqrt
and its division are correctly rounded).  The reference builds the rays (rays_of: steps 1 to 6) and scatters closest-hit records back to
the frame (scatter: steps 6 to 9); where the records come from is the caller's business: the GPU tests send the rays through the existing
traceDevice(any_hit=False) and take sky from the existing evalTable(3), the tests without a GPU use a float64 brute force over quads
(closest_hit_quads).  Vectorised over the pixels."""
import numpy as np

from tile_ref import SENTINEL, finite, rectangles

f32 = np.float32
u32 = np.uint32
i32 = np.int32
DEFAULT_RAYS_IN_FLIGHT = 1 << 23
DEFAULT_MAX_DISTANCE = 1e16
HEAD_BYTES = 256
PLANES = ("hit2", "position2", "ray", "sky")
WORDS = {"hit2": 8, "position2": 4, "ray": 8, "sky": 4}
COUNTERS = ("pixels", "traced", "skipped", "nonfinite", "invalid", "hits", "escaped", "batches")
NEUTRAL_RAY = np.array([0, 0, 0, 1, 0, 0, 1, -1], f32)


def _record(prim):
    r = np.zeros(8, u32)
    r[3] = r[4] = u32(0xFFFFFFFF)
    r[3] = np.array([prim], i32).view(u32)[0]
    return r


EMPTY_HIT = _record(-1)  # {t 0, u 0, v 0, prim -1, mesh -1, ng 0}
INVALID_HIT = _record(-2)


def batch_pixels(h, w, max_rays_in_flight=0):
    """pixels a batch: M, at most the frame's"""
    return min(max_rays_in_flight or DEFAULT_RAYS_IN_FLIGHT, h * w)


def layout(h, w, max_rays_in_flight=0):
    """pt_reflect_layout's bytes: the head, 40 bytes a ray slot and 4 a batch pixel, rounded up to 16"""
    return (HEAD_BYTES + batch_pixels(h, w, max_rays_in_flight) * 44 + 15) // 16 * 16


def batches_of(pixels, h, w, max_rays_in_flight=0):
    p = batch_pixels(h, w, max_rays_in_flight)
    return (int(pixels) + p - 1) // p


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize3(v):
    with np.errstate(all="ignore"):
        inv = f32(1.0) / np.sqrt(dot3(v, v))
        return (v * inv[..., None]).astype(f32)


def mirror(d, n):
    """step 4 from the unit eye ray d and the normal n ((m, 3) float32): c, k = 2c, r"""
    with np.errstate(all="ignore"):
        c = dot3(d, n)
        k = f32(2.0) * c
        r = normalize3(d - n * k[:, None])
    assert c.dtype == f32 and k.dtype == f32 and r.dtype == f32
    return r


def ray_valid(r):
    """pt_trace_device's rule for (m, 8) rays"""
    d = r[..., 4:7]
    with np.errstate(all="ignore"):
        s = dot3(d, d)
        inv = f32(1.0) / s
    return finite(r).all(-1) & finite(s) & (s != 0) & finite(inv) & (inv != 0)


def rays_of(hit, position, cams, rects, pixels, bias=1e-3, max_distance=DEFAULT_MAX_DISTANCE):
    """Steps 1 to 6 over the pixel set `pixels` ((h, w) bool), row by row.  hit (h, w, 8), position (h, w, 4); cams (nv, 12): eye, U, V, W
    per view (one row without views); rects: the views' (x0, y0, wr, hr), None without views.
    Returns {"rays": (n, 8), one per traced pixel in row order; "valid": (n,) bool; "pixel": (n,) the traced pixels' indices Y * w + X;
    "skipped", "nonfinite", "traced": (h, w) bool; "n", "d": (n, 3) the facing normal and the unit eye ray}"""
    hit, position = np.ascontiguousarray(hit, f32), np.ascontiguousarray(position, f32)
    h, w = pixels.shape
    cams = np.ascontiguousarray(cams, f32).reshape(-1, 12)
    rs = rectangles(rects, h, w)
    assert len(rs) == len(cams)
    view = np.full((h, w), -1, np.int64)
    for v, (x0, y0, wr, hr) in enumerate(rs):
        view[y0:y0 + hr, x0:x0 + wr] = v
    assert (view[pixels] >= 0).all(), "a pixel of the set lies in no view"
    miss = hit[..., 3].view(i32) < 0
    seven = np.concatenate([position[..., 0:3], hit[..., 5:8], hit[..., 0:1]], -1)
    with np.errstate(all="ignore"):
        bad = ~(finite(seven).all(-1) & (hit[..., 0] > f32(0)))
    skipped = pixels & miss
    nonfinite = pixels & ~miss & bad
    traced = pixels & ~miss & ~bad
    sel = np.flatnonzero(traced)
    P = position.reshape(-1, 4)[sel, 0:3]
    n0 = hit.reshape(-1, 8)[sel, 5:8]
    t = hit.reshape(-1, 8)[sel, 0]
    E = cams[view.reshape(-1)[sel], 0:3]
    with np.errstate(all="ignore"):
        s = dot3(n0, E - P)
        n = np.where((s < f32(0))[:, None], -n0, n0).astype(f32)
        d = normalize3(P - E)
        r = mirror(d, n)
        O = P + n * (f32(bias) * t)[:, None]
    assert O.dtype == f32
    rays = np.zeros((len(sel), 8), f32)
    rays[:, 0:3] = O
    rays[:, 3] = f32(0.0)
    rays[:, 4:7] = r
    rays[:, 7] = f32(max_distance)
    return dict(rays=rays, valid=ray_valid(rays), pixel=sel, skipped=skipped, nonfinite=nonfinite, traced=traced, n=n, d=d)


def position_of(rays, t2):
    """step 8: O + t2 * r per component, the product first"""
    with np.errstate(all="ignore"):
        p = rays[:, 0:3] + t2[:, None] * rays[:, 4:7]
    assert p.dtype == f32
    return np.concatenate([p, np.ones((len(p), 1), f32)], -1)


def scatter(records, R, pixels, sky_rgb=None, max_rays_in_flight=0):
    """Steps 6 to 9.  records: (n, 8) float32 or uint32 — the pt_hit of every ray of R["rays"] as a closest-hit query returns it (what it
    holds for an invalid ray is ignored).  sky_rgb: (n, 3) the probe's texel along every ray's direction, or None when sky is not asked for
    (rows of rays that hit or are invalid are ignored).  R: rays_of's result.
    Returns the four planes as uint32 words, SENTINEL outside the set, and the counters."""
    h, w = pixels.shape
    n = len(R["pixel"])
    rec = np.ascontiguousarray(records).view(u32).reshape(n, 8).copy()
    valid = R["valid"]
    rec[~valid] = INVALID_HIT
    prim = rec[:, 3].view(i32)
    is_hit = valid & (prim >= 0)
    escaped = valid & (prim < 0)
    pos = np.zeros((n, 4), f32)
    pos[is_hit] = position_of(R["rays"][is_hit], rec[is_hit, 0].view(f32))
    sky = np.zeros((n, 4), f32)
    if sky_rgb is not None:
        sky[escaped, 0:3] = np.ascontiguousarray(sky_rgb, f32)[escaped]
        sky[escaped, 3] = 1.0
    out = {name: np.full((h, w, WORDS[name]), SENTINEL, u32) for name in PLANES}
    const = R["skipped"] | R["nonfinite"]
    out["hit2"][const] = EMPTY_HIT
    out["position2"][const] = 0
    out["sky"][const] = 0
    out["ray"][const] = NEUTRAL_RAY.view(u32)
    px = R["pixel"]
    out["hit2"].reshape(-1, 8)[px] = rec
    out["position2"].reshape(-1, 4)[px] = pos.view(u32)
    out["sky"].reshape(-1, 4)[px] = sky.view(u32)
    out["ray"].reshape(-1, 8)[px] = R["rays"].view(u32)
    counters = dict(pixels=int(pixels.sum()), traced=n, skipped=int(R["skipped"].sum()), nonfinite=int(R["nonfinite"].sum()),
                    invalid=int((~valid).sum()), hits=int(is_hit.sum()), escaped=int(escaped.sum()),
                    batches=batches_of(pixels.sum(), h, w, max_rays_in_flight))
    return dict(out, **counters)


# ------------------------------------------------------------------ float64 brute force over quads (no GPU)
def quad_triangles(quads):
    """(2q, 3, 3) triangles and (2q,) the quad (the mesh, one quad a mesh) of each"""
    q = np.asarray(quads, np.float64).reshape(-1, 4, 3)
    return np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3, 3), np.repeat(np.arange(len(q)), 2)


def closest_hit_quads(rays, quads):
    """(t (n,) float64, prim (n,), mesh (n,)): the closest triangle of the quads a ray (o, tmin, d, tmax) meets at tmin < t < tmax, both
    faces; prim = mesh = -1 and t = tmax for none.  Primitives are numbered quad by quad, two each; Moeller-Trumbore in float64"""
    tri, quad = quad_triangles(quads)
    r = np.asarray(rays, np.float64)
    o, d, tmin, tmax = r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7]
    best, prim = tmax.copy(), np.full(len(r), -1, np.int64)
    for k, (v0, v1, v2) in enumerate(tri):
        e1, e2 = v1 - v0, v2 - v0
        pv = np.cross(d, e2)
        det = pv @ e1
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = o - v0
            u = (tv * pv).sum(1) * inv
            qv = np.cross(tv, e1)
            v = (d * qv).sum(1) * inv
            t = (qv @ e2) * inv
            hit = (np.abs(det) > 1e-300) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin) & (t < best)
        best = np.where(hit, t, best)
        prim = np.where(hit, k, prim)
    return best, prim, np.where(prim >= 0, quad[np.maximum(prim, 0)], -1)


def records_of(t, prim, mesh):
    """pt_hit records (n, 8) uint32 of a brute-force answer: t, prim and mesh; u, v and ng are left 0 (the analytic tests do not judge them)"""
    rec = np.zeros((len(t), 8), u32)
    rec[:, 0] = np.asarray(t, f32).view(u32)
    rec[:, 3] = np.asarray(prim, i32).view(u32)
    rec[:, 4] = np.asarray(mesh, i32).view(u32)
    return rec


# ------------------------------------------------------------------ the two analytic scenes
# A floor y = 0 over [-4, 4]^2 seen from ANALYTIC_EYE; with `ceiling`, a lid at y = LID over [-40, 40]^2.  The probed pixels lie within
# [-1, 1]^2.  The steepest mirror ray leaves the floor at (1, 0, 1) with the eye ray's slope mirrored: from the eye at height 6 and at most
# |(1, 1) - (0, -0.5)| = 1.81 away horizontally, it rises 6 per 1.81 — it reaches y = LID = 2 within 0.61 horizontally, far inside the lid.
LID = 2.0
FLOOR_QUAD = [(-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4)]  # wound so that the geometric normal is +y
LID_QUAD = [(-40, LID, -40), (-40, LID, 40), (40, LID, 40), (40, LID, -40)]
ANALYTIC_EYE = (0.0, 6.0, -0.5)


def analytic_quads(ceiling):
    return [FLOOR_QUAD] + ([LID_QUAD] if ceiling else [])


def analytic_planes(h=5, w=7):
    """hand-made hit and position planes of floor points in [-1, 1]^2 under ANALYTIC_EYE, and the one camera row"""
    ys, xs = np.mgrid[0:h, 0:w]
    P = np.zeros((h, w, 4), f32)
    P[..., 0] = (-1.0 + 2.0 * xs / (w - 1)).astype(f32)
    P[..., 2] = (-1.0 + 2.0 * ys / (h - 1)).astype(f32)
    P[..., 3] = 1.0
    hit = np.zeros((h, w, 8), f32)
    E = np.array(ANALYTIC_EYE, f32)
    hit[..., 0] = np.sqrt(((P[..., 0:3] - E) ** 2).sum(-1)).astype(f32)
    hit[..., 3] = np.zeros((h, w), i32).view(f32)
    hit[..., 4] = np.zeros((h, w), i32).view(f32)
    hit[..., 5:8] = (0.0, 1.0, 0.0)
    cam = np.zeros((1, 12), f32)
    cam[0, 0:3] = E
    return hit, P, cam
