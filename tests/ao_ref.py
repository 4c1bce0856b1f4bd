"""NumPy evaluation of pt_ao_layout's and pt_ao_planes's rules, written from the text of include/pt_amd.h alone; shared by
tests/test_ao_cabi.py and tests/test_gpu_ao.py.  A helper, not a test; it never calls the kernels under test.  Everything is float32
arrays and float32 scalars, one rounding per operation, in the header's order (NumPy never contracts a product and a sum; its sqrt and
its division are correctly rounded).  The reference builds the rays (rays_of) and reduces occlusion flags (reduce); where the flags come
from is the caller's business: the GPU tests send the rays through the existing traceDevice(any_hit=True), the tests without a GPU through
a float64 brute force over quads (any_hit_quads).  Vectorised over the pixels; the only loop is over the samples."""
import numpy as np

from dof_ref import directions, jitter_of
from tile_ref import SENTINEL, finite, rectangles

f32 = np.float32
u32 = np.uint32
MAX_RAYS = 32
DEFAULT_RAYS_IN_FLIGHT = 1 << 23
HEAD_BYTES = 256
COUNTERS = ("pixels", "traced", "skipped", "nonfinite", "rays", "occluded", "invalid", "batches")


def batch_pixels(h, w, rays, max_rays_in_flight=0):
    """pixels a batch: floor(M / rays), at most the frame's"""
    M = max_rays_in_flight or DEFAULT_RAYS_IN_FLIGHT
    return min(M // rays, h * w)


def layout(h, w, rays, max_rays_in_flight=0):
    """pt_ao_layout's bytes: the head, 40 bytes a ray slot, 8 a batch pixel, rounded up to 16"""
    p = batch_pixels(h, w, rays, max_rays_in_flight)
    return (HEAD_BYTES + p * (40 * rays + 8) + 15) // 16 * 16


def batches_of(pixels, h, w, rays, max_rays_in_flight=0):
    p = batch_pixels(h, w, rays, max_rays_in_flight)
    return (int(pixels) + p - 1) // p


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize3(v):
    with np.errstate(all="ignore"):
        inv = f32(1.0) / np.sqrt(dot3(v, v))
        return (v * inv[..., None]).astype(f32)


def sel_max0(v):
    with np.errstate(all="ignore"):
        return np.where(v > f32(0), v, f32(0)).astype(f32)  # a NaN gives 0


def frame_of(n):
    """step 4: T, B of unit normals n (m, 3)"""
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        sg = np.where(nz >= f32(0), f32(1.0), f32(-1.0)).astype(f32)
        a = f32(-1.0) / (sg + nz)
        b = (nx * ny) * a
        T = np.stack([f32(1.0) + (sg * (nx * nx)) * a, sg * b, (-sg) * nx], -1)
        B = np.stack([b, sg + (ny * ny) * a, -ny], -1)
    assert T.dtype == f32 and B.dtype == f32
    return T, B


def rho_of(rays):
    k = np.arange(rays).astype(f32)
    return np.sqrt((k + f32(0.5)) / f32(rays)).astype(f32)


def sample_dirs(n, T, B, k0, rays):
    """step 6: d (m, rays, 3) for normals n, frames T, B and jitters k0 (m,)"""
    D, rho = directions(), rho_of(rays)
    d = np.zeros((len(n), rays, 3), f32)
    for k in range(rays):
        idx = (k + k0) & 127
        assert (k + k0 <= 127).all()
        Dk = D[idx]
        with np.errstate(all="ignore"):
            ak, bk = rho[k] * Dk[:, 0], rho[k] * Dk[:, 1]
            ck = np.sqrt(sel_max0(f32(1.0) - (ak * ak + bk * bk)))
            w = ((T * ak[:, None]) + (B * bk[:, None])) + (n * ck[:, None])
        assert w.dtype == f32
        d[:, k] = normalize3(w)
    return d


def ray_valid(r):
    """pt_trace_device's rule for (m, 8) rays"""
    d = r[..., 4:7]
    with np.errstate(all="ignore"):
        s = dot3(d, d)
        inv = f32(1.0) / s
    return finite(r).all(-1) & finite(s) & (s != 0) & finite(inv) & (inv != 0)


def rays_of(hit, position, cams, rects, pixels, rays, radius, bias=1e-3, seed=0, jitter=False):
    """Steps 1 to 7 over the pixel set `pixels` ((h, w) bool), row by row.  hit (h, w, 8), position (h, w, 4); cams (nv, 12): eye, U, V, W
    per view (one row without views); rects: the views' (x0, y0, wr, hr), None without views.
    Returns {"rays": (n * rays, 8), pixel-major, sample k of traced pixel j at j * rays + k; "valid": (n * rays,) bool; "pixel": (n,) the
    traced pixels' indices Y * w + X; "skipped", "nonfinite", "traced": (h, w) bool}"""
    hit, position = np.ascontiguousarray(hit, f32), np.ascontiguousarray(position, f32)
    h, w = pixels.shape
    cams = np.ascontiguousarray(cams, f32).reshape(-1, 12)
    rs = rectangles(rects, h, w)
    assert len(rs) == len(cams)
    view = np.full((h, w), -1, np.int64)
    lx, ly = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    Y, X = np.mgrid[0:h, 0:w]
    for v, (x0, y0, wr, hr) in enumerate(rs):
        view[y0:y0 + hr, x0:x0 + wr] = v
        lx[y0:y0 + hr, x0:x0 + wr] = X[y0:y0 + hr, x0:x0 + wr] - x0
        ly[y0:y0 + hr, x0:x0 + wr] = Y[y0:y0 + hr, x0:x0 + wr] - y0
    assert (view[pixels] >= 0).all(), "a pixel of the set lies in no view"
    miss = hit[..., 3].view(np.int32) < 0
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
        T, B = frame_of(n)
        O = P + n * (f32(bias) * t)[:, None]
    assert O.dtype == f32
    k0 = jitter_of(lx.reshape(-1)[sel], ly.reshape(-1)[sel], seed) if jitter else np.zeros(len(sel), np.int64)
    d = sample_dirs(n, T, B, k0, rays)
    r = np.zeros((len(sel), rays, 8), f32)
    r[:, :, 0:3] = O[:, None, :]
    r[:, :, 3] = f32(0.0)
    r[:, :, 4:7] = d
    r[:, :, 7] = f32(radius)
    r = r.reshape(-1, 8)
    return dict(rays=r, valid=ray_valid(r), pixel=sel, skipped=skipped, nonfinite=nonfinite, traced=traced, n=n, T=T, B=B)


def reduce(occ, R, rays, pixels, max_rays_in_flight=0):
    """Step 9.  occ: (n * rays,) — non-zero where the ray is occluded; the flags of invalid rays are ignored.  R: rays_of's result.
    Returns the three planes as uint32 words ((h, w), (h, w, 4), (h, w, 4)), SENTINEL outside the set, and the counters."""
    h, w = pixels.shape
    n = len(R["pixel"])
    valid = R["valid"].reshape(n, rays)
    occ = (np.asarray(occ).reshape(n, rays) != 0) & valid
    d = R["rays"][:, 4:7].reshape(n, rays, 3)
    fr = f32(rays)
    opened = (~occ).sum(1)
    ao_t = opened.astype(f32) / fr
    S = np.zeros((n, 3), f32)
    for k in range(rays):
        add = (~occ[:, k]) & valid[:, k]
        with np.errstate(all="ignore"):
            S = np.where(add[:, None], S + d[:, k], S).astype(f32)
    bent_t = (S / fr).astype(f32)
    ao = np.full((h, w), SENTINEL, u32)
    out = np.full((h, w, 4), SENTINEL, u32)
    bent = np.full((h, w, 4), SENTINEL, u32)
    const = R["skipped"] | R["nonfinite"]
    one = f32(1.0).view(u32)
    ao[const] = one
    out[const] = one
    bent[const] = (0, 0, 0, one)
    a = ao_t.view(u32)
    ao.reshape(-1)[R["pixel"]] = a
    out.reshape(-1, 4)[R["pixel"]] = np.stack([a, a, a, np.full(n, one, u32)], -1)
    bent.reshape(-1, 4)[R["pixel"]] = np.concatenate([bent_t.view(u32), a[:, None]], -1)
    invalid = int((~valid).sum())
    counters = dict(pixels=int(pixels.sum()), traced=n, skipped=int(R["skipped"].sum()), nonfinite=int(R["nonfinite"].sum()),
                    rays=n * rays - invalid, occluded=int(occ.sum()), invalid=invalid,
                    batches=batches_of(pixels.sum(), h, w, rays, max_rays_in_flight))
    return dict(ao=ao, out=out, bent=bent, **counters)


# ------------------------------------------------------------------ float64 brute force over quads (no GPU)
def quad_triangles(quads):
    q = np.asarray(quads, np.float64).reshape(-1, 4, 3)
    return np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])


def any_hit_quads(rays, quads):
    """(n,) int: 1 where a ray (o, tmin, d, tmax) meets a triangle of the quads at tmin <= t <= tmax, both faces; Moeller-Trumbore in float64"""
    tri = quad_triangles(quads)
    r = np.asarray(rays, np.float64)
    o, d, tmin, tmax = r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7]
    occ = np.zeros(len(r), np.int32)
    for v0, v1, v2 in tri:
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
            hit = (np.abs(det) > 1e-300) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= tmin) & (t <= tmax)
        occ |= hit.astype(np.int32)
    return occ


# ------------------------------------------------------------------ the two analytic scenes
# A floor y = 0 over [-4, 4]^2 seen from above; with `ceiling`, a lid at y = LID over [-3, 3]^2.  The probed pixels lie within [-1, 1]^2:
# with RADIUS 1 no ray leaves the lid's extent, and the flattest ray of 32 (c = sqrt(0.5 / 32) = 0.125) reaches y = LID after 0.8 < RADIUS.
LID, RADIUS = 0.1, 1.0
FLOOR_QUAD = [(-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4)]  # wound so that the geometric normal is +y
LID_QUAD = [(-3, LID, -3), (-3, LID, 3), (3, LID, 3), (3, LID, -3)]
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
    hit[..., 3] = np.zeros((h, w), np.int32).view(f32)
    hit[..., 4] = np.zeros((h, w), np.int32).view(f32)
    hit[..., 5:8] = (0.0, 1.0, 0.0)
    cam = np.zeros((1, 12), f32)
    cam[0, 0:3] = E
    return hit, P, cam
