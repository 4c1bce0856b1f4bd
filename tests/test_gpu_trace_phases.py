"""The hand-over between the two loops of trace8_wave (pt_bvh8.h): a wave traverses in the bulk loop while the queue has rays for it and
crosses, once, to the stealing loop when it has taken its last chunk.  The cases sit where that crossing changes shape.  With nw the
persistent grid (CUs x 4 x 5 waves) a launch of up to 64 nw rays gives every wave exactly one chunk of 64, so every wave crosses at its
first refill; from 64 nw + 1 rays on the first waves fetch a second chunk through the atomic counter and stay in the bulk loop while the
others cross at once; at 3 x 64 nw every wave refills several times in the bulk loop and crosses with finished lanes, whose results are not
written yet, among its 64.  Closest-hit and any-hit device queries against brute force over all triangles, bit for bit.

The ray sets are one set of 5000 brute-forced rays per scene, tiled in a seeded random order up to the count of the case (brute force over a
million distinct rays takes minutes on the terrain); the expected answers tile with the rays.  An any-hit launch that culls back faces is
a foveated frame of the sv4 variant (launch chain) against the checker's own render of the same regions."""
import numpy as np
import pytest
import torch

from conftest import assert_bits_equal
from optixpathtracer_amd import renderer as R
from optixpathtracer_amd import scenes
from parity_kit import _random_rays

pytestmark = pytest.mark.gpu

BASE_RAYS = 5000
WAVES_PER_SIMD = 5  # PT8_WAVES_PER_EU
LDS_LEVELS = 10  # PT8_LDS_DEPTH


def _grid():
    """waves of the persistent traversal grid"""
    return torch.cuda.get_device_properties(0).multi_processor_count * 4 * WAVES_PER_SIMD


def _counts():
    k = 64 * _grid()
    return {"one_chunk_less_a_ray": k - 1, "one_chunk_each": k, "one_ray_more": k + 1, "a_second_chunk_and_a_ray": k + 65, "three_chunks_each": 3 * k}


COUNT_NAMES = ("one_chunk_less_a_ray", "one_chunk_each", "one_ray_more", "a_second_chunk_and_a_ray", "three_chunks_each")


class _Case:
    pass


def _case(orc_det, model, rays, seed):
    c = _Case()
    c.model = model
    sc = orc_det.make_scene(model, use_bvh=False)  # brute force: independent of any tree
    t, prim = orc_det.trace_closest(sc, rays)
    occ = orc_det.trace_any(sc, rays).astype(np.int32)
    assert (prim >= 0).mean() >= 0.2 and (prim < 0).mean() >= 0.05, "the rays must exercise hits and misses"
    # one order for every count: a case of n rays is the first n of it
    c.order = np.random.default_rng(seed).integers(0, len(rays), 3 * 64 * _grid())
    c.rays, c.t, c.prim, c.occ = rays, np.asarray(t, np.float32), np.asarray(prim), occ
    for a in (c.order, c.rays, c.t, c.prim, c.occ):
        a.setflags(write=False)
    return c


@pytest.fixture(scope="module")
def cornell(ptlib, orc_det):
    return _case(orc_det, scenes.cornell_box(), _random_rays(np.random.default_rng(41), BASE_RAYS, -100, 700), 43)


@pytest.fixture(scope="module")
def terrain(ptlib, orc_det):
    rng = np.random.default_rng(42)
    rays = _random_rays(rng, BASE_RAYS, -110, 110)
    rays[:, 1] = rng.uniform(-30, 60, len(rays)).astype(np.float32)
    return _case(orc_det, scenes.voxel_terrain(n=96, target_tris=70000), rays, 44)


@pytest.fixture(scope="module")
def renderers(ptlib, cornell, terrain):
    """one default context per scene for all counts"""
    rs = {"cornell": R.SampleRenderer(cornell.model), "terrain": R.SampleRenderer(terrain.model)}
    yield rs
    for r in rs.values():
        r.close()


def _check(r, c, n, what):
    idx = c.order[:n]
    prim_ref, t_ref, occ_ref = c.prim[idx], c.t[idx], c.occ[idx]
    assert (prim_ref >= 0).mean() >= 0.2 and (prim_ref < 0).mean() >= 0.05, "the rays must exercise hits and misses"
    d = torch.from_numpy(c.rays[idx]).to("cuda:0")
    res = r.traceDevice(d)
    prim, t = res["prim"].cpu().numpy(), res["t"].cpu().numpy()
    bad = np.flatnonzero(prim != prim_ref)
    assert bad.size == 0, f"{what}: closest-hit primitive differs at {bad.size} of {n} rays, first at {bad[:4]}"
    assert_bits_equal(t, t_ref, f"{what}: closest-hit t")
    occ = r.traceDevice(d, any_hit=True).cpu().numpy()
    bad = np.flatnonzero(occ != occ_ref)
    assert bad.size == 0, f"{what}: any-hit differs at {bad.size} of {n} rays, first at {bad[:4]}"


@pytest.mark.parametrize("count", COUNT_NAMES)
@pytest.mark.parametrize("scene", ["cornell", "terrain"])
def test_queries_around_the_grid_equal_brute_force(renderers, cornell, terrain, scene, count):
    n = _counts()[count]
    print(f"{scene}: {n} rays on a grid of {_grid()} waves")
    _check(renderers[scene], cornell if scene == "cornell" else terrain, n, f"{scene}, {n} rays")


def test_spill_levels_in_both_loops(monkeypatch, terrain):
    """three stack levels in LDS, fewer than the terrain's tree has: the spill pop and push run in the bulk loop of the waves with a second
    chunk and in the stealing loop of all"""
    monkeypatch.setenv("PT_STACK_LDS_SKIP", "7")
    r = R.SampleRenderer(terrain.model)
    monkeypatch.delenv("PT_STACK_LDS_SKIP")
    assert r.stats()["bvh_levels"] > LDS_LEVELS - 7, "the terrain's tree must be deeper than the LDS levels the hook at 7 leaves"
    n = _counts()["a_second_chunk_and_a_ray"]
    _check(r, terrain, n, f"terrain, PT_STACK_LDS_SKIP=7, {n} rays")
    r.close()


def test_back_face_culling_shadow_rays_equal_the_checker(ptlib, orc_det):
    """sv4's occlusion rays ignore back faces (cull_back in the traversal's any-hit lanes): a foveated frame, three launches, against the
    checker's render of the same regions"""
    model = scenes.cornell_box()
    sky = scenes.sky_probe(256, 128).BuildCDF()
    w, h = 128, 96
    regs = R.SampleRenderer.foveatedRegions((w, h), (64, 48), 0, inner_radius=14, outer_radius=44, spp=(1, 2, 3))
    r = R.SampleRenderer(model)
    r.setProbe(sky)
    r.setOptions(max_depth=4)
    r.resize((w, h))
    r.setCamera(R.make_camera(scenes.CORNELL_CAMERA, w / h))
    r.renderRegions(regs, R.SampleRenderer.SV4_VARIANT)
    st = r.stats()
    got_accum, got_frame = r.download(R.PT_BUF_ACCUM).copy(), r.downloadPixels().copy()
    r.close()
    assert st["shadow_rays"] > 0 and st["trace_launches"] > 0, st  # a foveated frame goes through the launch chain: k_trace8 with cull_back set
    U, V, W = scenes.uvw_frame(**scenes.CORNELL_CAMERA, aspect=w / h)
    accum = np.zeros((h, w, 4), np.float32)
    frame = np.zeros((h, w), np.uint32)
    orc_det.render_regions(orc_det.make_scene(model, True), orc_det.make_probe(sky), (U, V, W), scenes.CORNELL_CAMERA["eye"], w, h, regs, R.SampleRenderer.SV4_VARIANT, 4,
                           accum, frame)
    assert_bits_equal(got_accum, accum, "foveated accum against the checker")
    assert np.array_equal(got_frame, frame), "foveated frame buffer"
