"""Updates fed from GPU memory (pt_update_meshes_device, pt_transform_meshes): the staged vertices are those of the host path — or of
float32 NumPy evaluating the header's expression — bit for bit, so tree, vertices and images equal the host-fed context's, a fresh
pt_create's and the CPU checker's; a refused call leaves every bit of the context alone."""
import numpy as np
import pytest
import torch

from gpu_kit import _dev, _dev_all
from optixpathtracer_amd import scenes
from optixpathtracer_amd import renderer as R
from parity_kit import _compare, _gpu_render, _oracle_render, _renderer
from scene_kit import M1, _affine, _canonical, _moved_mesh, _np_transform, _wave, _with_vertices

pytestmark = pytest.mark.gpu

W, H = 96, 64


@pytest.fixture(scope="module")
def terrain():
    return scenes.voxel_terrain(n=96, target_tris=70000)


@pytest.fixture(scope="module")
def probe():
    return scenes.sky_probe(256, 128).BuildCDF()


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("PT_BVH_BUILDER", "PT_BVH_CLIMB", "PT_FUSED", "PT_BVH_IMPORT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PT_SCHED_TRIALS", "0")
    return monkeypatch


IDENTITY = np.eye(4, dtype=np.float32)[:3]
M2 = _affine((-0.3, 1.0, 0.9), -1.1, (0.9, 1.2, 0.7), (-0.2, 0.1, 0.5))


def _verts(r, model, rest=False):
    return [r.downloadVertices(i, rest=rest) for i in range(len(model.meshes))]


def _same_vertices(r, model, expect: dict, rest=False):
    """Bitwise (also the sign of a zero) against `expect`, meshes not listed against the model's own."""
    for i, m in enumerate(model.meshes):
        want = np.ascontiguousarray(expect.get(i, m.vertex), np.float32)
        assert r.downloadVertices(i, rest=rest).tobytes() == want.tobytes(), f"mesh {i}"


def _same_tree(a, b):
    """Two contexts' trees, byte for byte up to the numbering of the nodes: k_collapse8 hands out node and triangle ranges with atomic
    counters, so two builds of one scene number their nodes differently (scene_kit._canonical), and a refit keeps the numbering."""
    (n0, t0), (n1, t1) = a.exportBVH(), b.exportBVH()
    assert n0.shape == n1.shape and t0.shape == t1.shape
    assert _canonical(n0.tobytes(), t0.tobytes()) == _canonical(n1.tobytes(), t1.tobytes())


# ------------------------------------------------------------------ 1. device update equals host update
@pytest.mark.parametrize("rebuild", [False, True])
@pytest.mark.parametrize("scene", ["cornell", "two_box", "terrain"])
def test_device_update_equals_host_update(ptlib, clean_env, terrain, scene, rebuild):
    model = {"cornell": scenes.cornell_box, "two_box": scenes.two_box_scene}.get(scene, lambda: terrain)()
    amp = 20.0 if scene == "cornell" else (0.2 if scene == "two_box" else 2.0)
    new = _wave(model, amp, 0.6)  # every mesh, all in one call (Cornell: 52, 4, 4 and 4 vertices)
    d, h = R.SampleRenderer(model), R.SampleRenderer(model)
    assert _verts(d, model, rest=True)[0].tobytes() == np.ascontiguousarray(model.meshes[0].vertex, np.float32).tobytes()
    ms = d.updateMeshesDevice(_dev_all(new, offset_mesh=0), rebuild=rebuild)
    assert ms > 0
    h.updateMeshes(new, rebuild=rebuild)
    _same_vertices(d, model, new)
    _same_vertices(d, model, new, rest=True)  # no transform yet: rest positions are the current ones
    _same_tree(d, h)
    # a raw pointer with its vertex count, one mesh of several
    k = len(model.meshes) - 1
    one = _moved_mesh(model, k, (0.25, -0.5, 0.125))
    t = _dev(one[k])
    d.updateMeshesDevice({k: (t.data_ptr(), len(one[k]))}, rebuild=rebuild)
    h.updateMeshes(one, rebuild=rebuild)
    _same_vertices(d, model, {**new, **one})
    _same_tree(d, h)
    d.close()
    h.close()


# ------------------------------------------------------------------ 2. rendered bits
@pytest.mark.parametrize("sched", ["chain", "fused"])
def test_device_update_render_equals_fresh_build_and_checker(ptlib, orc_det, clean_env, terrain, probe, sched):
    clean_env.setenv("PT_FUSED", "0" if sched == "chain" else "1")
    clean_env.setenv("PT_FUSED_MAX_COST", "1e9")
    new = _wave(terrain, 2.0, 0.7)
    B = _with_vertices(terrain, new)
    r = _renderer(terrain, probe, scenes.TERRAIN_CAMERA, W, H)
    _gpu_render(r, 2)
    r.updateMeshesDevice(_dev_all(new))
    g = _gpu_render(r, 2, subframes=2)
    _compare(g, _gpu_render(_renderer(B, probe, scenes.TERRAIN_CAMERA, W, H), 2, subframes=2))
    _compare(g, _oracle_render(orc_det, B, probe, scenes.TERRAIN_CAMERA, W, H, 2, subframes=2))
    if sched == "fused":
        assert g["stats"]["fused_passes"] > 0


def test_device_update_shadow_catcher_scene(ptlib, orc_det, clean_env, probe):
    A = scenes.two_box_scene(shadow_catcher=True)
    up = _moved_mesh(A, len(A.meshes) - 1, (0.35, 0.1, -0.2))
    B = _with_vertices(A, up)
    cam = scenes.TWO_BOX_CAMERA
    r = _renderer(A, probe, cam, W, H)
    _gpu_render(r, 2)
    r.updateMeshesDevice(_dev_all(up))
    g = _gpu_render(r, 2, subframes=2)
    _compare(g, _gpu_render(_renderer(B, probe, cam, W, H), 2, subframes=2))
    _compare(g, _oracle_render(orc_det, B, probe, cam, W, H, 2, subframes=2))


def test_device_update_textured_scene(ptlib, orc_det, clean_env, probe):
    A = scenes.textured_scene()  # the texture records of k_refit_leaves
    new = _wave(A, 0.15, 0.3)
    B = _with_vertices(A, new)
    cam = dict(eye=(3.0, 2.5, -4.5), lookat=(0.0, 0.6, 0.5), up=(0.0, 1.0, 0.0), fovY=45.0)
    r = _renderer(A, probe, cam, W, H)
    _gpu_render(r, 2)
    r.updateMeshesDevice(_dev_all(new, offset_mesh=1))
    g = _gpu_render(r, 2, subframes=2)
    _compare(g, _gpu_render(_renderer(B, probe, cam, W, H), 2, subframes=2))
    _compare(g, _oracle_render(orc_det, B, probe, cam, W, H, 2, subframes=2))


# ------------------------------------------------------------------ 3. transform parity
@pytest.mark.parametrize("rebuild", [False, True])
def test_transform_parity_two_box(ptlib, orc_det, clean_env, probe, rebuild):
    A = scenes.two_box_scene()
    want = {0: _np_transform(M1, A.meshes[0].vertex)}  # rotation about a skew axis, non-uniform scale, translation
    B = _with_vertices(A, want)
    cam = scenes.TWO_BOX_CAMERA
    r = _renderer(A, probe, cam, W, H)
    _gpu_render(r, 2)
    assert r.transformMeshes({0: M1}, rebuild=rebuild) > 0
    _same_vertices(r, A, want)
    _same_vertices(r, A, {}, rest=True)  # a transform leaves the rest positions alone
    h = R.SampleRenderer(A)
    h.updateMeshes(want, rebuild=rebuild)
    _same_tree(r, h)
    g = _gpu_render(r, 2, subframes=2)
    _compare(g, _oracle_render(orc_det, B, probe, cam, W, H, 2, subframes=2))


def test_transform_parity_cornell_two_of_four(ptlib, orc_det, clean_env, probe):
    A = scenes.cornell_box()
    Ma = _affine((0.2, 1.0, 0.1), 0.2, (0.9, 0.95, 0.9), (20.0, 3.0, 15.0))  # the 52-vertex mesh: walls and blocks
    Mb = np.eye(4, dtype=np.float32)  # the light, as a 4x4: slides along the ceiling
    Mb[:3, 3] = (-60.0, -0.5, 40.0)
    want = {0: _np_transform(Ma, A.meshes[0].vertex), 3: _np_transform(Mb, A.meshes[3].vertex)}
    B = _with_vertices(A, want)
    cam = scenes.CORNELL_CAMERA
    r = _renderer(A, probe, cam, W, H)
    r.transformMeshes({0: Ma, 3: Mb})
    _same_vertices(r, A, want)
    h = R.SampleRenderer(A)
    h.updateMeshes(want)
    _same_tree(r, h)
    g = _gpu_render(r, 2, subframes=2)
    _compare(g, _oracle_render(orc_det, B, probe, cam, W, H, 2, subframes=2))


def test_transform_parity_terrain_many_waves(ptlib, clean_env, terrain):
    """Segments of thousands of vertices: several waves per mesh, the last one partly filled."""
    want = {i: _np_transform(M2 if i & 1 else M1, m.vertex) for i, m in enumerate(terrain.meshes)}
    r = R.SampleRenderer(terrain)
    r.transformMeshes({i: (M2 if i & 1 else M1) for i in want})
    _same_vertices(r, terrain, want)
    h = R.SampleRenderer(terrain)
    h.updateMeshes(want)
    _same_tree(r, h)


# ------------------------------------------------------------------ 4. rest against current
def test_rest_against_current(ptlib, clean_env):
    A = scenes.two_box_scene()
    v0, v1 = (np.asarray(m.vertex, np.float32) for m in A.meshes)
    r = R.SampleRenderer(A)
    r.transformMeshes({0: M1})
    r.transformMeshes({0: M2})  # from rest: M2 alone, no drift
    _same_vertices(r, A, {0: _np_transform(M2, v0)})
    r.transformMeshes({0: M1})
    r.transformMeshes({0: M2}, from_current=True)  # M1 then M2, in turn
    both = _np_transform(M2, _np_transform(M1, v0))
    _same_vertices(r, A, {0: both})
    _same_vertices(r, A, {}, rest=True)
    # an unnamed mesh keeps its transformed positions
    r.transformMeshes({1: M1})
    _same_vertices(r, A, {0: both, 1: _np_transform(M1, v1)})
    # an explicit update resets that mesh's rest positions (host and device path), the other mesh's stay
    e0 = _moved_mesh(A, 0, (0.5, 0.25, -0.75))[0]
    r.updateMeshes({0: e0})
    _same_vertices(r, A, {0: e0}, rest=True)
    _same_vertices(r, A, {0: e0, 1: _np_transform(M1, v1)})
    r.transformMeshes({0: M2})
    _same_vertices(r, A, {0: _np_transform(M2, e0), 1: _np_transform(M1, v1)})
    e1 = _moved_mesh(A, 1, (-0.125, 0.0, 0.375))[1]
    r.updateMeshesDevice({1: _dev(e1)})
    _same_vertices(r, A, {0: e0, 1: e1}, rest=True)
    r.transformMeshes({1: M2, 0: IDENTITY})
    _same_vertices(r, A, {0: _np_transform(IDENTITY, e0), 1: _np_transform(M2, e1)})
    r.close()


def test_identity_from_rest(ptlib, clean_env):
    """((1 x + 0 y) + 0 z) + 0 turns -0.0 into +0.0, so the vertices — and the tree — are NumPy's, not necessarily the original ones."""
    A = scenes.two_box_scene()
    v = np.asarray(A.meshes[0].vertex, np.float32).copy()
    v[0, 0], v[1, 2] = -0.0, -0.0
    A.meshes[0].vertex = v
    want = {0: _np_transform(IDENTITY, v)}
    assert want[0].tobytes() != v.tobytes() and np.array_equal(want[0], v)
    r = R.SampleRenderer(A)
    r.transformMeshes({0: IDENTITY})
    _same_vertices(r, A, want)
    h = R.SampleRenderer(A)
    h.updateMeshes(want)
    _same_tree(r, h)


# ------------------------------------------------------------------ 5. atomic refusal
class _Frozen:
    """A context whose every observable bit must survive refused calls."""

    def __init__(self, model, probe, cam):
        self.model = model
        self.r = _renderer(model, probe, cam, W, H)
        self.frame = _gpu_render(self.r, 1)
        self.tree = self.r.exportBVH()
        self.verts = _verts(self.r, model)

    def refused(self, what, call, match):
        with pytest.raises(RuntimeError, match=match):
            call()
        t = self.r.exportBVH()
        assert t[0].tobytes() == self.tree[0].tobytes() and t[1].tobytes() == self.tree[1].tobytes(), what
        for rest in (False, True):
            for a, b in zip(_verts(self.r, self.model, rest=rest), self.verts):
                assert a.tobytes() == b.tobytes(), what
        _compare(_gpu_render(self.r, 1), self.frame)


def test_refused_device_updates_leave_the_context_unchanged(ptlib, clean_env, terrain, probe):
    F = _Frozen(terrain, probe, scenes.TERRAIN_CAMERA)
    r = F.r
    v0, v1 = (np.asarray(terrain.meshes[i].vertex, np.float32) for i in (0, 1))
    nv = len(v0)
    assert nv > 128
    for k, (at, value) in enumerate(((0, np.nan), (63, np.inf), (64, -np.inf), (nv - 1, np.nan))):
        bad = v0.copy()
        bad[at, k % 3] = value
        for rebuild in (False, True):
            F.refused(f"{value} at vertex {at}", lambda: r.updateMeshesDevice({0: _dev(bad)}, rebuild=rebuild), r"\(-1\).*non-finite coordinate in mesh 0")
    bad = v1.copy()
    bad[len(bad) // 2, 1] = np.nan
    F.refused("the second of two meshes", lambda: r.updateMeshesDevice({0: _dev(v0), 1: _dev(bad)}), r"\(-1\).*non-finite coordinate in mesh 1")
    F.refused("the lowest position in the call is reported", lambda: r.updateMeshesDevice([(1, _dev(bad)), (0, _dev(v0))]), r"\(-1\).*mesh 1")
    host = v0.copy()
    F.refused("a host pointer", lambda: r.updateMeshesDevice({0: (host.ctypes.data, nv)}), r"\(-1\).*mesh 0 is not device memory")
    good = _dev(v0)
    F.refused("a null pointer", lambda: r.updateMeshesDevice({0: (0, nv)}), r"\(-1\).*null")
    F.refused("a pointer that is not 4-byte aligned", lambda: r.updateMeshesDevice({0: (good.data_ptr() + 2, nv)}), r"\(-1\).*not 4-byte aligned")
    F.refused("a mesh named twice", lambda: r.updateMeshesDevice([(0, good), (0, good)]), r"\(-1\).*named twice")
    F.refused("a wrong vertex count", lambda: r.updateMeshesDevice({0: _dev(v0[:-1])}), r"\(-1\).*vertices")
    F.refused("a mesh out of range", lambda: r.updateMeshesDevice({len(terrain.meshes): good}), r"\(-1\).*out of range")
    F.refused("no updates", lambda: r.updateMeshesDevice({}), r"\(-1\)")
    with pytest.raises(ValueError):
        r.updateMeshesDevice({0: good.double()})
    with pytest.raises(ValueError):
        r.updateMeshesDevice({0: good.t().contiguous().t()})
    with pytest.raises(ValueError):
        r.updateMeshesDevice({0: good.cpu()})
    # a valid update succeeds afterwards
    new = _wave(terrain, 1.0, 0.2)
    r.updateMeshesDevice(_dev_all(new))
    _same_vertices(r, terrain, new)
    h = R.SampleRenderer(terrain)
    h.updateMeshes(new)
    _same_tree(r, h)


def test_refused_transforms_leave_the_context_unchanged(ptlib, clean_env, probe):
    import ctypes as C

    from optixpathtracer_amd import _lib

    A = scenes.cornell_box()
    F = _Frozen(A, probe, scenes.CORNELL_CAMERA)
    r = F.r
    huge = np.diag([3e38, 3e38, 3e38, 1.0]).astype(np.float32)  # 556 * 3e38 overflows
    for rebuild in (False, True):
        F.refused("overflow", lambda: r.transformMeshes({0: huge}, rebuild=rebuild), r"\(-1\).*non-finite coordinate in mesh 0")
    F.refused("overflow in the second mesh", lambda: r.transformMeshes({3: IDENTITY, 2: huge}), r"\(-1\).*non-finite coordinate in mesh 2")
    nan = IDENTITY.copy()
    nan[1, 2] = np.nan
    F.refused("a NaN matrix entry", lambda: r.transformMeshes({1: nan}), r"\(-1\).*non-finite matrix entry for mesh 1")
    inf = IDENTITY.copy()
    inf[2, 3] = np.inf
    F.refused("an infinite matrix entry", lambda: r.transformMeshes({0: IDENTITY, 1: inf}, from_current=True), r"\(-1\).*mesh 1")
    F.refused("a mesh named twice", lambda: r.transformMeshes([(2, IDENTITY), (2, M1)]), r"\(-1\).*named twice")
    F.refused("a mesh out of range", lambda: r.transformMeshes({4: IDENTITY}), r"\(-1\).*out of range")
    F.refused("no transforms", lambda: r.transformMeshes({}), r"\(-1\)")
    xf = (_lib.MeshTransform * 1)()
    xf[0].m[:] = [float(x) for x in IDENTITY.reshape(-1)]
    ms = C.c_double(-1.0)
    assert r._L.pt_transform_meshes(r._ctx, xf, 1, 2, _lib.PT_UPDATE_REFIT, C.byref(ms)) == -1  # unknown source
    assert r._L.pt_transform_meshes(r._ctx, xf, 1, _lib.PT_FROM_REST, 2, C.byref(ms)) == -1  # unknown mode
    assert r._L.pt_transform_meshes(r._ctx, None, 1, _lib.PT_FROM_REST, _lib.PT_UPDATE_REFIT, C.byref(ms)) == -1
    buf = np.empty((4, 3), np.float32)
    assert r._L.pt_download_vertices(r._ctx, 1, 0, buf.ctypes.data, buf.nbytes - 4) == -1
    assert r._L.pt_download_vertices(r._ctx, 1, 2, buf.ctypes.data, buf.nbytes) == -1
    assert r._L.pt_download_vertices(r._ctx, 4, 0, buf.ctypes.data, buf.nbytes) == -1
    assert ms.value == -1.0
    F.refused("still as before", lambda: r.transformMeshes({0: nan}), r"\(-1\)")
    # a valid transform succeeds afterwards
    M = _affine((0.0, 1.0, 0.0), 0.1, (1.0, 1.0, 1.0), (5.0, 0.0, 0.0))
    r.transformMeshes({0: M})
    _same_vertices(r, A, {0: _np_transform(M, A.meshes[0].vertex)})


# ------------------------------------------------------------------ 6. frames in flight
def test_device_update_with_frames_in_flight(ptlib, clean_env, terrain, probe):
    from conftest import assert_bits_equal

    new = _wave(terrain, 2.0, 0.5)
    B = _with_vertices(terrain, new)
    ref_a = _gpu_render(_renderer(terrain, probe, scenes.TERRAIN_CAMERA, W, H), 2)
    ref_b = _gpu_render(_renderer(B, probe, scenes.TERRAIN_CAMERA, W, H), 2)
    r = _renderer(terrain, probe, scenes.TERRAIN_CAMERA, W, H, frames_in_flight=2)
    r.launchParams.samples_per_launch = 2
    r.launchParams.frame.subframe_index = 0
    r.render()  # enqueued, not waited for
    r.updateMeshesDevice(_dev_all(new))
    assert_bits_equal(r.download(R.PT_BUF_ACCUM), ref_a["accum"], "frame enqueued before the update")
    r.render()
    assert_bits_equal(r.download(R.PT_BUF_ACCUM), ref_b["accum"], "frame after the update")
    assert np.array_equal(r.download(R.PT_BUF_FRAME), ref_b["frame"])


# ------------------------------------------------------------------ 7. multi
@pytest.mark.parametrize("rebuild", [False, True])
def test_multi_transform_equals_single_context(ptlib, clean_env, terrain, rebuild):
    xf = {0: M1, 3: M2, len(terrain.meshes) - 1: M1}
    want = {i: _np_transform(M, terrain.meshes[i].vertex) for i, M in xf.items()}
    mr = R.MultiRenderer(terrain, devices=(0, 0))
    assert mr.transformMeshes(xf, rebuild=rebuild) > 0
    s = R.SampleRenderer(terrain)
    s.updateMeshes(want, rebuild=rebuild)
    for k in range(mr.world):
        rank = mr.rank(k)
        _same_tree(rank, s)
        _same_vertices(rank, terrain, want)
    with pytest.raises(RuntimeError, match=r"\(-1\).*named twice"):
        mr.transformMeshes([(0, M1), (0, M2)])
    mr.transformMeshes({0: M2}, from_current=True, rebuild=rebuild)
    s.updateMeshes({0: _np_transform(M2, want[0])}, rebuild=rebuild)
    for k in range(mr.world):
        _same_tree(mr.rank(k), s)
    mr.close()
