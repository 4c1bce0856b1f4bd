"""NumPy evaluation of pt_shadow_layout's and pt_shadow_planes's rules, written from the text of include/pt_amd.h alone; shared by
tests/test_shadow_cabi.py and tests/test_gpu_shadow.py.  A helper, not a test; it never calls the kernels under test.  Everything is
float32 arrays and float32 scalars, one rounding per operation, in the header's order.  The reference builds the rays (rays_of) and reduces
occlusion flags (reduce); where the flags come from is the caller's business: the GPU tests send the rays through the existing
traceDevice(any_hit=True), the tests without a GPU through ao_ref's float64 brute force over quads.  A light is (dir, spread, radiance,
rays).  Vectorised over the pixels; the loops are over the lights and the samples."""
import numpy as np

from ao_ref import FLOOR_QUAD, LID, LID_QUAD, analytic_quads, any_hit_quads, dot3, frame_of, normalize3, ray_valid, rho_of  # noqa: F401
from dof_ref import directions, jitter_of
from tile_ref import SENTINEL, finite, rectangles

f32 = np.float32
u32 = np.uint32
MAX_LIGHTS = 4
MAX_RAYS = 32
DEFAULT_RAYS_IN_FLIGHT = 1 << 23
HEAD_BYTES = 256
COUNTERS = ("pixels", "traced", "skipped", "nonfinite", "backfacing", "rays", "occluded", "invalid", "batches")
PLANES = ("visibility", "light")


def total_rays(lights):
    return sum(int(l[3]) for l in lights)


def batch_pixels(h, w, R, max_rays_in_flight=0):
    """pixels a batch: floor(M / R), at most the frame's"""
    M = max_rays_in_flight or DEFAULT_RAYS_IN_FLIGHT
    return min(M // R, h * w)


def layout(h, w, lights, max_rays_in_flight=0):
    """pt_shadow_layout's bytes: the head, 40 bytes a ray slot, 32 a batch pixel, rounded up to 16"""
    R = total_rays(lights)
    p = batch_pixels(h, w, R, max_rays_in_flight)
    return (HEAD_BYTES + p * (40 * R + 32) + 15) // 16 * 16


def batches_of(pixels, h, w, lights, max_rays_in_flight=0):
    p = batch_pixels(h, w, total_rays(lights), max_rays_in_flight)
    return (int(pixels) + p - 1) // p


def lights_of(lights):
    """per light, the same for all pixels: L = normalize3(dir), T and B (ao_ref.frame_of around L), spread, radiance, rays"""
    assert 1 <= len(lights) <= MAX_LIGHTS and total_rays(lights) <= MAX_RAYS and all(int(l[3]) >= 1 for l in lights)
    d = np.array([l[0] for l in lights], f32).reshape(-1, 3)
    L = normalize3(d)
    T, B = frame_of(L)
    return dict(L=L, T=T, B=B, spread=np.array([l[1] for l in lights], f32), radiance=np.array([l[2] for l in lights], f32).reshape(-1, 3),
                rays=np.array([int(l[3]) for l in lights], np.int64))


def sample_dirs(L, T, B, spread, rays, k0):
    """step 5: d (m, rays, 3) for the jitters k0 (m,) — of one light (L, T, B (3,)), or of a light per row (L, T, B (m, 3))"""
    D, rho = directions(), rho_of(rays)
    L, T, B = (np.atleast_2d(np.asarray(v, f32)) for v in (L, T, B))
    d = np.zeros((len(k0), rays, 3), f32)
    for k in range(rays):
        Dk = D[(k + k0) & 127]
        with np.errstate(all="ignore"):
            a = (rho[k] * Dk[:, 0]) * f32(spread)
            b = (rho[k] * Dk[:, 1]) * f32(spread)
            w = (L + T * a[:, None]) + B * b[:, None]
        assert w.dtype == f32
        d[:, k] = normalize3(w)
    return d


def rays_of(hit, position, cams, rects, pixels, lights, max_distance, bias=1e-3, seed=0, jitter=False, view_ray=None):
    """Steps 1 to 5 over the pixel set `pixels` ((h, w) bool), row by row.  hit (h, w, 8), position (h, w, 4), view_ray (h, w, 8) or None;
    cams (nv, 12): eye, U, V, W per view (one row without views); rects: the views' (x0, y0, wr, hr), None without views.
    Returns {"rays": (m, 8): light after light, per light its shooting pixels in row order, per pixel its samples; "valid": (m,) bool;
    "pixel": (n,) the traced pixels' indices Y * w + X; "first": (n, lights) where the rays of (pixel, light) start in "rays", -1 for a
    light under the horizon; "c": (n, lights) the clamped cosines; "skipped", "nonfinite", "traced": (h, w) bool}"""
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
    words = [position[..., 0:3], hit[..., 5:8], hit[..., 0:1]]
    if view_ray is not None:
        view_ray = np.ascontiguousarray(view_ray, f32)
        words.append(view_ray[..., 0:3])
    with np.errstate(all="ignore"):
        bad = ~(finite(np.concatenate(words, -1)).all(-1) & (hit[..., 0] > f32(0)))
    skipped = pixels & miss
    nonfinite = pixels & ~miss & bad
    traced = pixels & ~miss & ~bad
    sel = np.flatnonzero(traced)
    P = position.reshape(-1, 4)[sel, 0:3]
    ng = hit.reshape(-1, 8)[sel, 5:8]
    t = hit.reshape(-1, 8)[sel, 0]
    E = view_ray.reshape(-1, 8)[sel, 0:3] if view_ray is not None else cams[view.reshape(-1)[sel], 0:3]
    with np.errstate(all="ignore"):
        s = dot3(ng, E - P)
        n = np.where((s < f32(0))[:, None], -ng, ng).astype(f32)
        O = P + n * (f32(bias) * t)[:, None]
    assert O.dtype == f32
    Lt = lights_of(lights)
    nl = len(lights)
    first = np.full((len(sel), nl), -1, np.int64)
    c = np.zeros((len(sel), nl), f32)
    parts, at = [], 0
    for i in range(nl):
        with np.errstate(all="ignore"):
            ci = dot3(n, Lt["L"][i][None, :])
            shoots = ci > f32(0.0)
        c[:, i] = np.where(ci > f32(1.0), f32(1.0), ci)
        who = np.flatnonzero(shoots)
        rays = int(Lt["rays"][i])
        si = u32((int(seed) + i) & 0xFFFFFFFF)
        k0 = jitter_of(lx.reshape(-1)[sel[who]], ly.reshape(-1)[sel[who]], si) if jitter else np.zeros(len(who), np.int64)
        d = sample_dirs(Lt["L"][i], Lt["T"][i], Lt["B"][i], Lt["spread"][i], rays, k0)
        r = np.zeros((len(who), rays, 8), f32)
        r[:, :, 0:3] = O[who][:, None, :]
        r[:, :, 3] = f32(0.0)
        r[:, :, 4:7] = d
        r[:, :, 7] = f32(max_distance)
        first[who, i] = at + np.arange(len(who)) * rays
        at += len(who) * rays
        parts.append(r.reshape(-1, 8))
    r = np.concatenate(parts) if parts else np.zeros((0, 8), f32)
    return dict(rays=r, valid=ray_valid(r), pixel=sel, first=first, c=c, skipped=skipped, nonfinite=nonfinite, traced=traced, n=n, O=O, lights=Lt)


def reduce(occ, R, lights, pixels, max_rays_in_flight=0):
    """Steps 6 and 7.  occ: (m,) — non-zero where the ray is occluded; the flags of invalid rays are ignored.  R: rays_of's result.
    Returns the two planes as uint32 words (h, w, 4), SENTINEL outside the set, and the counters."""
    h, w = pixels.shape
    n, nl = len(R["pixel"]), len(lights)
    Lt = R["lights"]
    occ = (np.asarray(occ).reshape(-1) != 0) & R["valid"]
    v = np.ones((n, 4), f32)
    S = np.zeros((n, 3), f32)
    backfacing = 0
    for i in range(nl):
        rays = int(Lt["rays"][i])
        shoots = R["first"][:, i] >= 0
        backfacing += int((~shoots).sum())
        idx = R["first"][shoots, i][:, None] + np.arange(rays)[None, :]
        opened = (~occ[idx]).sum(1)
        vi = np.zeros(n, f32)
        vi[shoots] = opened.astype(f32) / f32(rays)
        v[:, i] = vi
        with np.errstate(all="ignore"):
            cv = R["c"][:, i] * vi
            add = Lt["radiance"][i][None, :] * cv[:, None]
            S = np.where(shoots[:, None], S + add, S).astype(f32)
    assert S.dtype == f32 and v.dtype == f32
    vis = np.full((h, w, 4), SENTINEL, u32)
    light = np.full((h, w, 4), SENTINEL, u32)
    const = R["skipped"] | R["nonfinite"]
    one = f32(1.0).view(u32)
    vis[const] = one
    light[const] = (0, 0, 0, one)
    vis.reshape(-1, 4)[R["pixel"]] = v.view(u32)
    light.reshape(-1, 4)[R["pixel"]] = np.concatenate([S.view(u32), np.full((n, 1), one, u32)], -1)
    invalid = int((~R["valid"]).sum())
    counters = dict(pixels=int(pixels.sum()), traced=n, skipped=int(R["skipped"].sum()), nonfinite=int(R["nonfinite"].sum()), backfacing=backfacing,
                    rays=len(R["rays"]) - invalid, occluded=int(occ.sum()), invalid=invalid,
                    batches=batches_of(pixels.sum(), h, w, lights, max_rays_in_flight))
    return dict(visibility=vis, light=light, **counters)


# ------------------------------------------------------------------ the analytic scene: ao_ref's floor and lid, seen beyond the lid's edge
# Floor points on a grid over [-EXTENT, EXTENT]^2 of the floor [-4, 4]^2; the lid covers [-3, 3]^2 at y = LID.  At 14 x 9 the columns are
# 0.6 apart from -3.9 and the rows 0.975: no point lies within 0.07 of the lid's projected edge or on the diagonal the lid's two triangles
# share, so a light straight up leaves no pixel undecided.
EXTENT = 3.9
ANALYTIC_SIZE = (14, 9)  # w, h
ANALYTIC_EYE = (0.0, 6.0, -0.5)
LID_HALF = 3.0


def analytic_planes(h=ANALYTIC_SIZE[1], w=ANALYTIC_SIZE[0], extent=EXTENT):
    """hand-made hit and position planes of floor points under ANALYTIC_EYE, and the one camera row"""
    ys, xs = np.mgrid[0:h, 0:w]
    P = np.zeros((h, w, 4), f32)
    P[..., 0] = (-extent + 2.0 * extent * xs / max(w - 1, 1)).astype(f32)
    P[..., 2] = (-extent + 2.0 * extent * ys / max(h - 1, 1)).astype(f32)
    P[..., 3] = 1.0
    hit = np.zeros((h, w, 8), f32)
    E = np.array(ANALYTIC_EYE, f32)
    hit[..., 0] = np.sqrt(((P[..., 0:3] - E) ** 2).sum(-1)).astype(f32)
    hit[..., 5:8] = (0.0, 1.0, 0.0)
    cam = np.zeros((1, 12), f32)
    cam[0, 0:3] = E
    return hit, P, cam


def under_the_lid(P, margin=1e-3):
    """(under, undecided): floor points whose vertical ray meets the lid, and those within `margin` of its projected edge"""
    ax, az = np.abs(P[..., 0].astype(np.float64)), np.abs(P[..., 2].astype(np.float64))
    undecided = (np.abs(ax - LID_HALF) <= margin) & (az <= LID_HALF + margin) | (np.abs(az - LID_HALF) <= margin) & (ax <= LID_HALF + margin)
    return (ax < LID_HALF) & (az < LID_HALF), undecided
