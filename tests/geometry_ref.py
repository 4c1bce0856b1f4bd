"""The float64 truth of the image-space chain, written from the geometry and not from the header.  A helper, not a test; shared by
tests/test_geometry_cabi.py and tests/test_gpu_geometry.py.

The other *_ref.py files transcribe the arithmetic blocks of include/pt_amd.h in float32 and pin the kernels' bits.  A transcription shares
every error of convention with what it transcribes: a motion vector of the wrong sign, a half-pixel slip, u and v on the wrong vertices, a
previous camera taken by the wrong index.  This file is there to disagree with them when they are wrong, so it imports none of them and
restates no formula of the header: it has no projection of a point through a camera (no Cramer's rule, no NDC-to-pixel expression), no
camera formula at all, and no barycentrics from a ray and a triangle's edges.  What it uses instead:

  lookup_error_px  the rays the generator really emits for the previous frame (the `ray` plane, pinned by test_ray_and_hit): a claimed
                   lookup is right when the previous frame's rays, interpolated at the claimed coordinates, pass through the point;
  inverse_rigid    the inverse of a rigid move, from its rotation matrix, centre and translation;
  barycentric      least-squares coordinates of a point in the basis of a triangle's two edges; interpolate() then weights an attribute by
                   (1 - u - v, u, v) on (v0, v1, v2), the order pt_hit documents — the one convention it takes from the header's text.

Everything is plain NumPy float64."""
import numpy as np

f64 = np.float64


def image_plane_normal(rays):
    """The viewing axis of the camera that emitted the ray plane (h, w, 8), up to scale, from five of its unit directions alone.

    Pixel centres are equally spaced on an image plane, so along a row the un-normalised directions are D_b = (1 - s) D_a + s D_c for the
    pixels a, b, c at 0, s and 1 of the row's length.  Writing the unit direction d_b = alpha d_a + gamma d_c (they are coplanar) gives the
    lengths of D_a and D_c in proportion alpha / (1 - s) : gamma / s, hence the row's direction D_c - D_a; a column gives the other one, and
    the axis is perpendicular to both."""
    d = np.asarray(rays, f64)[..., 4:7]
    h, w = d.shape[:2]

    def along(a, b, c, s):
        (alpha, gamma), *_ = np.linalg.lstsq(np.stack([a, c], 1), b, rcond=None)
        return c * (gamma / s) - a * (alpha / (1 - s))

    mx, my = (w - 1) // 2, (h - 1) // 2
    row = along(d[my, 0], d[my, mx], d[my, w - 1], mx / (w - 1))
    col = along(d[0, mx], d[my, mx], d[h - 1, mx], my / (h - 1))
    n = np.cross(row, col)
    return n * np.sign(n @ d[my, mx]) / np.linalg.norm(n)


def lookup_error_px(points, prev_rays, lookup_xy, rect=None, normal=None):
    """How far, in pixels of the previous image, the claim "world point points[k] was seen at fractional pixel lookup_xy[k]" is off.

    points (n, 3); prev_rays (h, w, 8): the previous frame's ray plane (origin, tmin, direction, tmax per pixel centre); lookup_xy (n, 2):
    x, y in pixels of the rectangle rect = (x0, y0, wr, hr) of that plane (None: the whole plane), a pixel's centre at its integer index;
    normal: the previous camera's viewing axis if known (None: image_plane_normal of the rectangle's rays).

    The rays of the four pixel centres around the claimed position are cut with the plane through the point perpendicular to the viewing
    axis.  Cutting with such a plane is affine in the pixel coordinates, so the bilinear interpolation of the four cuts at the claimed
    position is where the previous camera saw that position, exactly; its distance from the point, over the distance between two
    horizontally neighbouring cuts, is the error in pixels.  (The cell is clamped into the rectangle; an affine map extrapolates exactly.)"""
    X = np.asarray(points, f64).reshape(-1, 3)
    xy = np.asarray(lookup_xy, f64).reshape(-1, 2)
    rays = np.asarray(prev_rays, f64)
    x0, y0, wr, hr = rect if rect is not None else (0, 0, rays.shape[1], rays.shape[0])
    rays = rays[y0:y0 + hr, x0:x0 + wr]
    n = image_plane_normal(rays) if normal is None else np.asarray(normal, f64)
    ix = np.clip(np.floor(xy[:, 0]), 0, wr - 2).astype(int)
    iy = np.clip(np.floor(xy[:, 1]), 0, hr - 2).astype(int)
    fx, fy = xy[:, 0] - ix, xy[:, 1] - iy

    def cut(i, j):
        r = rays[iy + j, ix + i]
        o, d = r[:, 0:3], r[:, 4:7]
        s = ((X - o) @ n) / (d @ n)
        return o + s[:, None] * d

    c00, c10, c01, c11 = cut(0, 0), cut(1, 0), cut(0, 1), cut(1, 1)
    top = c00 + (c10 - c00) * fx[:, None]
    bottom = c01 + (c11 - c01) * fx[:, None]
    seen = top + (bottom - top) * fy[:, None]
    return np.linalg.norm(seen - X, axis=1) / np.linalg.norm(c10 - c00, axis=1)


def rotation(axis, angle):
    """the rotation matrix by `angle` radians about `axis`, as the matrix exponential of the axis' cross-product matrix (a power series)"""
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = angle * np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], f64)
    R, term = np.eye(3), np.eye(3)
    for k in range(1, 30):
        term = term @ K / k
        R = R + term
    return R


def rigid_matrix(R, c, t):
    """the 3x4 matrix of "rotate by R about c, then translate by t": p -> R (p - c) + c + t"""
    R, c, t = np.asarray(R, f64), np.asarray(c, f64), np.asarray(t, f64)
    return np.concatenate([R, (c + t - R @ c)[:, None]], 1)


def inverse_rigid(points, R, c, t):
    """where the points were before "rotate by R about c, then translate by t": R^T (p - c - t) + c"""
    R, c, t = np.asarray(R, f64), np.asarray(c, f64), np.asarray(t, f64)
    return (np.asarray(points, f64) - c - t) @ R + c


def barycentric(points, v0, v1, v2):
    """(u, v) of each point in its triangle's plane, by least squares: the coefficients of (v1 - v0, v2 - v0) nearest to p - v0.  pt_hit
    documents the weights (1 - u - v, u, v) on (v0, v1, v2); interpolate() applies them."""
    p, v0, v1, v2 = (np.asarray(a, f64).reshape(-1, 3) for a in (points, v0, v1, v2))
    out = np.empty((len(p), 2))
    for k in range(len(p)):
        out[k] = np.linalg.lstsq(np.stack([v1[k] - v0[k], v2[k] - v0[k]], 1), p[k] - v0[k], rcond=None)[0]
    return out[:, 0], out[:, 1]


def interpolate(u, v, a0, a1, a2):
    """the attribute of (v0, v1, v2) at weights (1 - u - v, u, v)"""
    u, v = np.asarray(u, f64)[:, None], np.asarray(v, f64)[:, None]
    return np.asarray(a0, f64) * (1 - u - v) + np.asarray(a1, f64) * u + np.asarray(a2, f64) * v


def tap_diameter(prev_position, prev_is_hit, lookup_xy, rect=None):
    """For the bilinear lookup at lookup_xy (n, 2) into the previous frame's position plane (h, w, 4): (d, ok) — the largest distance between
    two of its four taps, and whether all four lie in the rectangle and are hits."""
    P = np.asarray(prev_position, f64)[..., 0:3]
    x0, y0, wr, hr = rect if rect is not None else (0, 0, P.shape[1], P.shape[0])
    xy = np.asarray(lookup_xy, f64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(xy).all(1)
        ix, iy = np.floor(np.where(fin, xy[:, 0], -9)).astype(int), np.floor(np.where(fin, xy[:, 1], -9)).astype(int)
    ok = fin & (ix >= 0) & (ix + 1 < wr) & (iy >= 0) & (iy + 1 < hr)
    ix, iy = np.clip(ix, 0, wr - 2) + x0, np.clip(iy, 0, hr - 2) + y0
    taps = [P[iy + j, ix + i] for i, j in ((0, 0), (1, 0), (0, 1), (1, 1))]
    for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
        ok &= np.asarray(prev_is_hit, bool)[iy + j, ix + i]
    d = np.zeros(len(xy))
    for a in range(4):
        for b in range(a + 1, 4):
            d = np.maximum(d, np.linalg.norm(taps[a] - taps[b], axis=1))
    return d, ok
