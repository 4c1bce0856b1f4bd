"""In-place vertex updates (pt_update_meshes): a refitted tree must render the same bits as a fresh pt_create over the moved vertices —
and as the CPU checker — because a hit does not depend on the tree (closest t, lowest primitive on ties, hits confined to the triangle's
padded box).  A refit over unchanged vertices gives the tree back byte for byte; a rebuild gives the fresh build's tree."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from optixpathtracer_amd import scenes
from optixpathtracer_amd import renderer as R
from parity_kit import _compare, _gpu_render, _oracle_render, _renderer
from scene_kit import _aimed_rays, _canonical, _moved_mesh, _wave, _with_vertices

pytestmark = pytest.mark.gpu

W, H = 96, 64


def _all(model):
    return {i: np.asarray(m.vertex, np.float32) for i, m in enumerate(model.meshes)}


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


@pytest.mark.parametrize("builder", [None, "lbvh", "ploc", "sah"])
def test_identity_refit_is_byte_identical(ptlib, clean_env, terrain, builder):
    if builder:
        clean_env.setenv("PT_BVH_BUILDER", builder)
    r = R.SampleRenderer(terrain)
    n0, t0 = r.exportBVH()
    ms = r.updateMeshes(_all(terrain))
    assert ms > 0
    n1, t1 = r.exportBVH()
    assert n1.tobytes() == n0.tobytes() and t1.tobytes() == t0.tobytes()
    for step in range(10):  # animate away, then back
        r.updateMeshes(_wave(terrain, 1.5, 0.4 * step))
    assert r.exportBVH()[0].tobytes() != n0.tobytes()
    r.updateMeshes(_all(terrain))
    n2, t2 = r.exportBVH()
    assert n2.tobytes() == n0.tobytes() and t2.tobytes() == t0.tobytes()
    r.close()


def test_identity_refit_small_scenes(ptlib, clean_env):
    for model in (scenes.cornell_box(), scenes.two_box_scene()):
        r = R.SampleRenderer(model)
        n0, t0 = r.exportBVH()
        r.updateMeshes(_moved_mesh(model, 0, (3.0, -1.0, 2.0)))
        r.updateMeshes(_all(model))
        n1, t1 = r.exportBVH()
        assert n1.tobytes() == n0.tobytes() and t1.tobytes() == t0.tobytes()
        r.close()


@pytest.mark.parametrize("sched", ["chain", "fused"])
@pytest.mark.parametrize("split_shadow", [0, 2])
def test_refit_render_equals_fresh_build_and_checker(ptlib, orc_det, clean_env, terrain, probe, sched, split_shadow):
    clean_env.setenv("PT_FUSED", "0" if sched == "chain" else "1")
    clean_env.setenv("PT_FUSED_MAX_COST", "1e9")
    B = _with_vertices(terrain, _wave(terrain, 2.0, 0.7))
    r = _renderer(terrain, probe, scenes.TERRAIN_CAMERA, W, H, split_shadow=split_shadow)
    _gpu_render(r, 2)
    r.updateMeshes(_all(B))
    g = _gpu_render(r, 2, subframes=2)
    f = _gpu_render(_renderer(B, probe, scenes.TERRAIN_CAMERA, W, H, split_shadow=split_shadow), 2, subframes=2)
    _compare(g, f)
    _compare(g, _oracle_render(orc_det, B, probe, scenes.TERRAIN_CAMERA, W, H, 2, subframes=2))
    if sched == "fused" and split_shadow == 0:
        assert g["stats"]["fused_passes"] > 0


def test_refit_shadow_catcher_scene(ptlib, orc_det, clean_env, probe):
    A = scenes.two_box_scene(shadow_catcher=True)
    up = _moved_mesh(A, len(A.meshes) - 1, (0.35, 0.1, -0.2))
    B = _with_vertices(A, up)
    cam = scenes.TWO_BOX_CAMERA
    r = _renderer(A, probe, cam, W, H)
    _gpu_render(r, 2)
    r.updateMeshes(up)
    g = _gpu_render(r, 2)
    _compare(g, _gpu_render(_renderer(B, probe, cam, W, H), 2))
    _compare(g, _oracle_render(orc_det, B, probe, cam, W, H, 2))


def test_refit_foveated_regions(ptlib, clean_env, terrain, probe):
    B = _with_vertices(terrain, _wave(terrain, 2.0, 1.1))
    r = _renderer(terrain, probe, scenes.TERRAIN_CAMERA, W, H)
    f = _renderer(B, probe, scenes.TERRAIN_CAMERA, W, H)
    r.updateMeshes(_all(B))
    regs = r.foveatedRegions((W, H), (48, 32), 0, inner_radius=10, outer_radius=30, spp=(1, 2, 4))
    a, b = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
    r.renderRegions(regs, out=a)
    f.renderRegions(regs, out=b)
    assert np.array_equal(a, b)
    assert_bits_equal(r.download(R.PT_BUF_ACCUM), f.download(R.PT_BUF_ACCUM), "foveated accum")


@pytest.mark.parametrize("rebuild", [False, True])
def test_textured_scene_update(ptlib, orc_det, clean_env, probe, rebuild):
    A = scenes.textured_terrain(n=96, target_tris=70000, tex_size=256)
    B = _with_vertices(A, _wave(A, 1.5, 0.3))
    r = _renderer(A, probe, scenes.TERRAIN_CAMERA, W, H)
    _gpu_render(r, 2)
    r.updateMeshes(_all(B), rebuild=rebuild)
    g = _gpu_render(r, 2)
    _compare(g, _gpu_render(_renderer(B, probe, scenes.TERRAIN_CAMERA, W, H), 2))
    _compare(g, _oracle_render(orc_det, B, probe, scenes.TERRAIN_CAMERA, W, H, 2))


def _check_enclosure(nodes, tris):
    """Every child box of the exported tree encloses the padded boxes of all triangles below it."""
    f = nodes.view(np.float32)
    nn = len(nodes)
    V = tris[:, :9].reshape(-1, 3, 3)
    pad = np.float32(np.abs(V).max()) * np.float32(1.0 / 65536.0)  # the builder's padding: 2^-16 of the largest |coordinate|
    tlo, thi = V.min(1), V.max(1)
    # the triangles under every node (leaf order is breadth-first-compatible: collect bottom-up)
    below_lo, below_hi = np.full((nn, 3), np.inf, np.float32), np.full((nn, 3), -np.inf, np.float32)
    for i in range(nn - 1, -1, -1):
        nd = nodes[i]
        origin = f[i, 0:3]
        st = np.array([(nd[3] & 0xFFFF) << 16, (nd[3] >> 16) << 16, (nd[7] & 0xFFFF) << 16], np.uint32).view(np.float32)
        cb, tb, lb, im = int(nd[4]), int(nd[5]), int(nd[6]), int(nd[7]) >> 16
        q = nd[8:20].view(np.uint8).reshape(6, 8)  # qlo.x qlo.y qlo.z qhi.x qhi.y qhi.z, one byte per slot
        irank, toff = 0, 0
        for s in range(8):
            if im >> s & 1:
                c = cb + irank
                irank += 1
                clo, chi = below_lo[c], below_hi[c]
            elif (lb >> 3 * s) & 7:
                k = bin((lb >> 3 * s) & 7).count("1")
                clo, chi = tlo[tb + toff:tb + toff + k].min(0), thi[tb + toff:tb + toff + k].max(0)
                toff += k
            else:
                continue
            blo = origin + q[0:3, s].astype(np.float32) * st
            bhi = origin + q[3:6, s].astype(np.float32) * st
            assert (blo <= clo - pad).all() and (bhi >= chi + pad).all(), f"node {i} slot {s}"
            below_lo[i] = np.minimum(below_lo[i], clo)
            below_hi[i] = np.maximum(below_hi[i], chi)


def test_queries_after_refit(ptlib, orc_det, clean_env, terrain):
    B = _with_vertices(terrain, _wave(terrain, 2.5, 0.9))
    r = R.SampleRenderer(terrain)
    r.updateMeshes(_all(B))
    rays = _aimed_rays(B, 20000, 3)
    sc = orc_det.make_scene(B)
    (t, prim), _ = r.trace(rays)
    ot, oprim = orc_det.trace_closest(sc, rays)
    assert np.array_equal(prim, oprim)
    assert_bits_equal(t, ot, "closest t")
    occ, _ = r.trace(rays, any_hit=True)
    oocc = orc_det.trace_any(sc, rays)
    assert np.array_equal(occ, oocc)
    nodes, tris = r.exportBVH()
    orc_det.set_bvh8(sc, nodes, tris)
    bt, bprim = orc_det.trace_closest(sc, rays)
    assert np.array_equal(bprim, oprim) and np.array_equal(orc_det.trace_any(sc, rays), oocc)
    assert_bits_equal(bt, ot, "closest t through the refitted tree")
    orc_det.set_bvh8(sc, None, None)
    _check_enclosure(nodes, tris)


def test_rebuild_equals_fresh_tree(ptlib, clean_env, terrain):
    B = _with_vertices(terrain, _wave(terrain, 3.0, 0.2))
    r = R.SampleRenderer(terrain)
    r.updateMeshes(_all(B), rebuild=True)
    f = R.SampleRenderer(B)
    a, b = r.exportBVH(), f.exportBVH()
    assert _canonical(a[0].tobytes(), a[1].tobytes()) == _canonical(b[0].tobytes(), b[1].tobytes())
    sa, sb = r.stats(), f.stats()
    assert sa["bvh_builder"] == sb["bvh_builder"] and sa["bvh_levels"] == sb["bvh_levels"]


@pytest.mark.parametrize("case", ["scale1000", "point", "far"])
def test_hostile_updates_render_exactly(ptlib, clean_env, probe, case):
    A = scenes.cornell_box()
    cam = dict(scenes.CORNELL_CAMERA)
    if case == "scale1000":
        up = {i: (np.asarray(m.vertex, np.float32) * np.float32(1000)).astype(np.float32) for i, m in enumerate(A.meshes)}
        cam = dict(eye=tuple(1000 * np.array(cam["eye"])), lookat=tuple(1000 * np.array(cam["lookat"])), up=cam["up"], fovY=cam["fovY"])
    elif case == "point":
        v = np.asarray(A.meshes[1].vertex, np.float32)
        up = {1: np.repeat(v[:1], len(v), 0)}
    else:
        up = _moved_mesh(A, 2, (1e4, 0.0, 0.0))
    B = _with_vertices(A, up)
    r = _renderer(A, probe, cam, W, H)
    _gpu_render(r, 2)
    r.updateMeshes(up)
    _compare(_gpu_render(r, 2), _gpu_render(_renderer(B, probe, cam, W, H), 2))


def test_frames_in_flight_see_the_geometry_of_their_call(ptlib, clean_env, terrain, probe):
    B = _with_vertices(terrain, _wave(terrain, 2.0, 0.5))
    ref_a = _gpu_render(_renderer(terrain, probe, scenes.TERRAIN_CAMERA, W, H), 2)
    ref_b = _gpu_render(_renderer(B, probe, scenes.TERRAIN_CAMERA, W, H), 2)
    r = _renderer(terrain, probe, scenes.TERRAIN_CAMERA, W, H, frames_in_flight=3)
    r.launchParams.samples_per_launch = 2
    r.launchParams.frame.subframe_index = 0
    r.render()  # enqueued, not waited for
    r.updateMeshes(_all(B))
    assert_bits_equal(r.download(R.PT_BUF_ACCUM), ref_a["accum"], "frame enqueued before the update")
    r.render()
    assert_bits_equal(r.download(R.PT_BUF_ACCUM), ref_b["accum"], "frame after the update")


def test_errors_leave_the_context_unchanged(ptlib, clean_env, terrain, probe):
    import ctypes as C

    from optixpathtracer_amd import _lib

    r = _renderer(terrain, probe, scenes.TERRAIN_CAMERA, W, H)
    before = _gpu_render(r, 2)
    tree = r.exportBVH()
    nv = len(terrain.meshes[0].vertex)
    bad_nan = np.asarray(terrain.meshes[0].vertex, np.float32).copy()
    bad_nan[nv // 2, 1] = np.nan
    for upd in ({0: np.zeros((nv - 1, 3), np.float32)}, {len(terrain.meshes): np.zeros((3, 3), np.float32)}, {0: bad_nan}):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            r.updateMeshes(upd)
    assert r._L.pt_update_meshes(r._ctx, None, 0, _lib.PT_UPDATE_REFIT, None) == -1
    assert r._L.pt_update_meshes(r._ctx, None, 0, _lib.PT_UPDATE_REBUILD, C.byref(C.c_double())) == -1
    after = _gpu_render(r, 2)
    _compare(after, before)
    t2 = r.exportBVH()
    assert t2[0].tobytes() == tree[0].tobytes() and t2[1].tobytes() == tree[1].tobytes()


@pytest.mark.parametrize("rebuild", [False, True])
def test_multi_update_equals_single_context(ptlib, clean_env, terrain, probe, rebuild):
    B = _with_vertices(terrain, _wave(terrain, 2.0, 1.7))
    mr = R.MultiRenderer(terrain, devices=(0,))
    mr.setProbe(probe)
    mr.resize((W, H))
    mr.setCamera(R.make_camera(scenes.TERRAIN_CAMERA, W / H))
    ms = mr.updateMeshes(_all(B), rebuild=rebuild)
    assert ms > 0
    mr.launchParams.samples_per_launch = 2
    mr.launchParams.frame.subframe_index = 0
    mr.render()
    s = _renderer(terrain, probe, scenes.TERRAIN_CAMERA, W, H)
    s.updateMeshes(_all(B), rebuild=rebuild)
    g = _gpu_render(s, 2)
    assert_bits_equal(mr.download(R.PT_BUF_ACCUM), g["accum"], "pt_multi_update_meshes")
    assert np.array_equal(mr.downloadPixels(), g["frame"])
    mr.close()


def test_stadium_refit_matches_fresh(ptlib, orc_det, clean_env, probe):
    A = scenes.stadium_scene(target_tris=200_000)
    B = _with_vertices(A, _wave(A, 0.4, 0.6, seed=11))
    r = _renderer(A, probe, scenes.STADIUM_CAMERA, W, H)
    n0, t0 = r.exportBVH()
    r.updateMeshes(_all(A))
    assert r.exportBVH()[0].tobytes() == n0.tobytes()
    r.updateMeshes(_all(B))
    g = _gpu_render(r, 2)
    _compare(g, _gpu_render(_renderer(B, probe, scenes.STADIUM_CAMERA, W, H), 2))
    _compare(g, _oracle_render(orc_det, B, probe, scenes.STADIUM_CAMERA, W, H, 2))
