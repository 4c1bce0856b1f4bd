"""Scene, geometry and view helpers that more than one test file uses: moved and transformed vertices, ray sets aimed at a scene, the
exported tree without its node numbering, and the four views of the viewport tests.  NumPy only."""
import copy

import numpy as np

import conftest  # noqa: F401  (puts the repository's root on sys.path)
from gbuffer_ref import _moved, _row
from optixpathtracer_amd import renderer as R
from optixpathtracer_amd import scenes

VIEW_W, VIEW_H = 131, 61  # the frame the four views of RECTS lie in (tests/test_gpu_views.py)


def _np_transform(M, v):
    """The header's expression in float32, one rounding per operation: x' = ((m0 x + m1 y) + m2 z) + m3, ..."""
    M = np.asarray(M, np.float32)[:3]
    v = np.asarray(v, np.float32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    out = np.empty_like(v)
    for r in range(3):
        m = M[r]
        out[:, r] = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
    assert out.dtype == np.float32
    return out


def _affine(axis, angle, scale, translate):
    """translate . rotate(axis, angle) . scale as a float32 3x4, composed in float64."""
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    Rm = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    M = np.zeros((3, 4))
    M[:, :3] = Rm @ np.diag(scale)
    M[:, 3] = translate
    return M.astype(np.float32)


M1 = _affine((1.0, 2.0, -0.5), 0.7, (1.3, 0.8, 1.1), (0.4, 0.25, -0.3))


def _with_vertices(model, verts: dict):
    m = copy.deepcopy(model)
    for k, v in verts.items():
        m.meshes[k].vertex = np.ascontiguousarray(v, np.float32)
    return m


def _wave(model, amp, phase=0.0, seed=7):
    """Seeded smooth displacement of every vertex (a travelling wave across the scene)."""
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.03, 0.08, 3)
    out = {}
    for i, m in enumerate(model.meshes):
        v = np.asarray(m.vertex, np.float64)
        d = amp * np.stack([np.sin(k[0] * v[:, 2] + phase), np.sin(k[1] * v[:, 0] + 1.3 * phase), np.cos(k[2] * v[:, 0] + k[2] * v[:, 2] + phase)], 1)
        out[i] = (v + d).astype(np.float32)
    return out


def _moved_mesh(model, mesh, offset):
    return {mesh: (np.asarray(model.meshes[mesh].vertex, np.float32) + np.float32(offset)).astype(np.float32)}


def _aimed_rays(model, n, seed):
    rng = np.random.default_rng(seed)
    v = model.flatten()[0]
    lo, hi = v.min(0), v.max(0)
    o = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), (n, 3))
    t = v[rng.integers(0, len(v), n)]
    d = t - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-3, d, 1e30
    rays[n // 2:, 7] = rng.uniform(1, 200, n - n // 2)  # segments for the any-hit query
    return rays


def _canonical(nodes_bytes, tris_bytes):
    """The exported tree without its node numbering: k_collapse8 hands out child and triangle ranges with atomic counters, so the order
    of the nodes inside a level (and of the leaf-triangle groups) differs from build to build.  Walk from the root in slot order and
    emit every node's content (grid, masks, planes) and its leaf triangles: equal trees give equal bytes."""
    N = np.frombuffer(nodes_bytes, np.uint32).reshape(-1, 20)
    T = np.frombuffer(tris_bytes, np.uint32).reshape(-1, 12)
    out_nodes, out_tris = [], []
    stack = [0]
    while stack:
        i = stack.pop()
        nd = N[i]
        child_base, tri_base, leafbits, imask = int(nd[4]), int(nd[5]), int(nd[6]), int(nd[7]) >> 16
        out_nodes.append(np.concatenate([nd[:4], nd[6:]]))
        ntri = bin(leafbits).count("1")
        out_tris.append(T[tri_base:tri_base + ntri])
        kids = [child_base + k for k in range(bin(imask).count("1"))]
        stack.extend(reversed(kids))
    return np.concatenate(out_nodes).tobytes(), np.concatenate(out_tris).tobytes(), len(out_nodes)


RECTS = [(0, 0, 61, 37), (64, 0, 67, 29), (0, 40, 24, 21), (72, 32, 7, 5)]


def _cam_dicts():
    base = scenes.TWO_BOX_CAMERA
    ex, ey, ez = base["eye"]
    return [dict(base, eye=(ex + 0.1, ey, ez)), dict(base, eye=(ex - 0.1, ey, ez)), dict(base, fovY=55.0), dict(base, eye=(2.0, 3.0, -4.5))]


def _views(cams=None):
    from optixpathtracer_amd import renderer as R

    cams = cams or _cam_dicts()
    return [(x, y, w, h, R.make_camera(c, w / h)) for (x, y, w, h), c in zip(RECTS, cams)]


def _rows(views):
    """the (n, 12) eye, U, V, W rows of a list of views"""
    from optixpathtracer_amd import renderer as R

    return R._camera_rows([v[4] for v in views])


# ------------------------------------------------------------------ 4. views
def _views_and_prev():
    views = [(x, y, w, h, R.make_camera(cd, w / h)) for (x, y, w, h), cd in zip(RECTS, _cam_dicts())]
    prev = np.stack([_row(_moved(cd, 0.1 * (k + 1)), w / h) for k, ((x, y, w, h), cd) in enumerate(zip(RECTS, _cam_dicts()))])
    return views, prev
