"""The per-ray traversal loop (trace8_wave, pt_bvh8.h) at its edges: launches of a lone lane, one full wave and a wave plus one lane, whose
rays all finish in the stealing phase (every wave takes its only chunk at once); the traversal stack with its LDS levels whole, cut to
three and cut to none (PT_STACK_LDS_SKIP: at the maximum every push and pop takes the spill path); closest-hit and any-hit queries
against brute force over all triangles, and small frames of one rank of a partition — launch chain and fused loop — against the default
context.  Every comparison is bit for bit.

What is NOT asserted: that the spill levels are written with the hook at 0.  The library exposes no stack-depth statistic in a release
build (the maximum depth is counted in PT_DEBUG_STATS builds only); pt_stats.bvh_levels bounds the depth from above, and the wide trees of
the suite's small scenes have fewer levels than the ten kept in LDS (the Cornell box 2, the 70 k-triangle terrain 8).  The hook at 7 leaves three LDS levels, fewer than the terrain's
tree has (asserted), so its deep rays spill; at the maximum every ray does."""
import numpy as np
import pytest
import torch

from conftest import assert_bits_equal
from optixpathtracer_amd import renderer as R
from optixpathtracer_amd import scenes
from parity_kit import _random_rays

pytestmark = pytest.mark.gpu

LDS_LEVELS = 10  # PT8_LDS_DEPTH
SKIPS = ("0", "7", "64")  # pt_create clamps the hook to the number of LDS levels: "64" is its maximum
COUNTS_OF_RAYS = (1, 63, 64, 65, 129, 5000)
TOTALS = ("radiance_rays", "shadow_rays", "shaded_hits")


class _Case:
    pass


def _case(orc_det, model, rays):
    c = _Case()
    c.model = model
    c.rays = rays
    c.rays.setflags(write=False)
    sc = orc_det.make_scene(model, use_bvh=False)  # brute force: independent of any tree
    c.t, c.prim = orc_det.trace_closest(sc, rays)
    c.t = np.asarray(c.t, np.float32)
    c.occ = orc_det.trace_any(sc, rays).astype(np.int32)
    assert (c.prim >= 0).mean() >= 0.2 and (c.prim < 0).mean() >= 0.05, "the rays must exercise hits and misses"
    return c


@pytest.fixture(scope="module")
def cornell_rays(ptlib, orc_det):
    return _case(orc_det, scenes.cornell_box(), _random_rays(np.random.default_rng(31), max(COUNTS_OF_RAYS), -100, 700))


@pytest.fixture(scope="module")
def terrain_model():
    return scenes.voxel_terrain(n=96, target_tris=70000)


@pytest.fixture(scope="module")
def terrain_rays(ptlib, orc_det, terrain_model):
    rng = np.random.default_rng(32)
    rays = _random_rays(rng, max(COUNTS_OF_RAYS), -110, 110)
    rays[:, 1] = rng.uniform(-30, 60, len(rays)).astype(np.float32)
    return _case(orc_det, terrain_model, rays)


@pytest.fixture(scope="module")
def sky():
    return scenes.sky_probe(256, 128).BuildCDF()


# ------------------------------------------------------------------ device ray queries
@pytest.mark.parametrize("skip", SKIPS)
@pytest.mark.parametrize("scene", ["cornell", "terrain"])
def test_device_queries_equal_brute_force(monkeypatch, cornell_rays, terrain_rays, scene, skip):
    c = cornell_rays if scene == "cornell" else terrain_rays
    monkeypatch.setenv("PT_STACK_LDS_SKIP", skip)
    r = R.SampleRenderer(c.model)
    monkeypatch.delenv("PT_STACK_LDS_SKIP")
    levels = r.stats()["bvh_levels"]
    print(f"{scene}: {levels} levels in the wide tree, {LDS_LEVELS - min(int(skip), LDS_LEVELS)} of the stack in LDS")
    if scene == "terrain":
        assert levels > LDS_LEVELS - 7, "the terrain's tree must be deeper than the LDS levels the hook at 7 leaves"
    for n in COUNTS_OF_RAYS:
        d = torch.from_numpy(np.array(c.rays[:n], copy=True)).to("cuda:0")
        res = r.traceDevice(d)
        t, prim = res["t"].cpu().numpy(), res["prim"].cpu().numpy()
        assert np.array_equal(prim, c.prim[:n]), f"closest-hit primitive, {n} rays"
        assert_bits_equal(t, c.t[:n], f"closest-hit t, {n} rays")
        occ = r.traceDevice(d, any_hit=True).cpu().numpy()
        assert np.array_equal(occ, c.occ[:n]), f"any-hit, {n} rays"
    r.close()


# ------------------------------------------------------------------ frames of one rank of a partition
def _frame(monkeypatch, env, model, probe, camera, size, spp, depth):
    """one context under `env` (read at pt_create), rank 1 of a 3-way partition: (buffers, totals, stats)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = R.SampleRenderer(model)
    for k in env:
        monkeypatch.delenv(k)
    r.setProbe(probe)
    r.setOptions(max_depth=depth)
    r.setPartition(1, 3, 64, 16)
    w, h = size
    r.resize((w, h))
    r.setCamera(R.make_camera(camera, w / h))
    r.launchParams.samples_per_launch = spp
    r.launchParams.frame.subframe_index = 0
    r.render()
    st = r.stats()
    out = {name: r.download(b).copy() for name, b in (("accum", R.PT_BUF_ACCUM), ("color", R.PT_BUF_COLOR), ("normal", R.PT_BUF_NORMAL), ("albedo", R.PT_BUF_ALBEDO))}
    out["frame"] = r.downloadPixels().copy()
    r.close()
    return out, {k: st[k] for k in TOTALS}, st


FRAMES = {"cornell": (scenes.CORNELL_CAMERA, (64, 64), 2, 4), "terrain": (scenes.TERRAIN_CAMERA, (320, 192), 2, 4)}


@pytest.fixture(scope="module")
def default_frames(ptlib, sky, terrain_model):
    """the default context's frame of either scene: rendered once, never changed"""
    mp = pytest.MonkeyPatch()
    out = {}
    for scene, (cam, size, spp, depth) in FRAMES.items():
        model = scenes.cornell_box() if scene == "cornell" else terrain_model
        out[scene] = (model, _frame(mp, {}, model, sky, cam, size, spp, depth))
        assert out[scene][1][1]["shadow_rays"] > 0
    mp.undo()
    return out


@pytest.mark.parametrize("fused", ["0", "2"])
@pytest.mark.parametrize("skip", ["0", "64"])
@pytest.mark.parametrize("scene", ["cornell", "terrain"])
def test_partition_frames_equal_the_default_context(monkeypatch, sky, default_frames, scene, skip, fused):
    cam, size, spp, depth = FRAMES[scene]
    model, (ref, ref_totals, _) = default_frames[scene]
    got, totals, st = _frame(monkeypatch, {"PT_STACK_LDS_SKIP": skip, "PT_FUSED": fused}, model, sky, cam, size, spp, depth)
    what = f"{scene}, PT_STACK_LDS_SKIP={skip}, PT_FUSED={fused}"
    print(what, "fused passes", st["fused_passes"], "trace launches", st["trace_launches"])
    assert (st["fused_passes"] > 0) == (fused == "2"), st["fused_passes"]
    if scene == "terrain" and fused == "0":
        assert st["trace_launches"] > 3  # three pixel chunks, each launch far below the grid size: the rays finish in the stealing phase
    assert totals == ref_totals, (what, totals, ref_totals)
    for k in ref:
        if k == "frame":
            assert np.array_equal(got[k], ref[k]), f"{what}: {k}"
        else:
            assert_bits_equal(got[k], ref[k], f"{what}: {k}")
