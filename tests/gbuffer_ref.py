"""The first-hit G-buffer in float32 NumPy: the header's expressions for the camera rays and for the depth, position and motion planes, one
rounding per operation, and the camera moves its tests share.  NumPy only: the references of the later passes (temporal_ref, motion_ref)
and the tests without a GPU build their planes from this."""
import numpy as np

import conftest  # noqa: F401  (puts the repository's root on sys.path)
from optixpathtracer_amd import renderer as R

f32 = np.float32


QNAN = 0x7FC00000


# ------------------------------------------------------------------ float32 NumPy: the header's expressions, one rounding per operation
def _row(cam_dict, aspect):
    return R._camera_rows([R.make_camera(cam_dict, aspect)])[0]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _normalize(v):
    return v * (f32(1.0) / np.sqrt(_dot(v, v)))[..., None]


def _np_rays(row, w, h):
    """(h, w, 8): origin eye, tmin 0.001f, dir = normalize3((U*dx + V*dy) + W), tmax 1e16f"""
    row = np.asarray(row, f32)
    eye, U, V, Wv = row[0:3], row[3:6], row[6:9], row[9:12]
    dx = f32(2.0) * ((np.arange(w, dtype=f32) + f32(0.5)) / f32(w)) - f32(1.0)
    dy = f32(2.0) * ((np.arange(h, dtype=f32) + f32(0.5)) / f32(h)) - f32(1.0)
    d = (U[None, None, :] * dx[None, :, None] + V[None, None, :] * dy[:, None, None]) + Wv[None, None, :]
    d = _normalize(d)
    rays = np.empty((h, w, 8), f32)
    rays[..., 0:3] = eye
    rays[..., 3] = f32(0.001)
    rays[..., 4:7] = d
    rays[..., 7] = f32(1e16)
    assert d.dtype == f32
    return rays


def _np_planes(rays, t, hit, row, prev):
    """depth (h, w), position (h, w, 4), motion (h, w, 2) as uint32 bits, from the NumPy rays, the checker's t and hit mask, the camera row and
    the previous camera row"""
    h, w = hit.shape
    row, prev = np.asarray(row, f32), np.asarray(prev, f32)
    o, d = rays[..., 0:3], rays[..., 4:7]
    t = np.asarray(t, f32).reshape(h, w)
    depth = np.where(hit, t * _dot(d, _normalize(row[9:12])[None, None, :]), f32(np.inf)).astype(f32)
    P = o + t[..., None] * d
    position = np.zeros((h, w, 4), f32)
    position[..., 0:3] = np.where(hit[..., None], P, f32(0.0))
    position[..., 3] = np.where(hit, f32(1.0), f32(0.0))
    pe, pU, pV, pW = prev[0:3], prev[3:6], prev[6:9], prev[9:12]
    q = np.where(hit[..., None], P - pe, d).astype(f32)
    VxW = _cross(pV, pW)
    with np.errstate(all="ignore"):
        a, b, c, det = _dot(q, VxW), _dot(q, _cross(pW, pU)), _dot(q, _cross(pU, pV)), _dot(pU, VxW)
        px = (((a / c) + f32(1.0)) * f32(0.5)) * f32(w) - f32(0.5)
        py = (((b / c) + f32(1.0)) * f32(0.5)) * f32(h) - f32(0.5)
        mx = px - np.arange(w, dtype=f32)[None, :]
        my = py - np.arange(h, dtype=f32)[:, None]
        ok = c * det > 0
    for x in (depth, P, a, c, px, mx, my):
        assert x.dtype == f32
    motion = np.stack([mx, my], -1).view(np.uint32).copy()
    motion[~ok] = QNAN
    return depth.view(np.uint32), position.view(np.uint32), motion, ok


def _moved(cam_dict, dx=0.25):
    ex, ey, ez = cam_dict["eye"]
    return dict(cam_dict, eye=(ex + dx, ey, ez))


def _behind(cam_dict):
    """behind the scene, looking away from it: the eye mirrored through the look-at point, keeping the viewing direction"""
    e, l = np.asarray(cam_dict["eye"], np.float64), np.asarray(cam_dict["lookat"], np.float64)
    far = l + 4.0 * (l - e)
    return dict(cam_dict, eye=tuple(far), lookat=tuple(far + (l - e)))


PLANES = ("hit", "depth", "position", "motion", "ray")
