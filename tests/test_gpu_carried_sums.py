"""Carried sums (PT_CARRY_SUMS): in the launch chain of a scene without shadow catchers the unified traversal launch only
stores one visibility word per shadow ray, and k_shade keeps the path's direct / indirect sums with its queue entry, adding the previous
bounce's contribution where the ray was visible and writing the slot arrays once, when the path ends.  Per path the additions and their
order are those of the traversal kernel's write-back, so every case renders with PT_CARRY_SUMS=1 and =0 (PT_FUSED=0: the launch chain)
and compares all five buffers and the device-counted totals bit for bit — and the accumulation buffer with the CPU checker where the
case has a counterpart there.  pt_stats.schedule bit 9 says whether the last render's chains carried the sums."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from optixpathtracer_amd import scenes

pytestmark = pytest.mark.gpu

CARRIED = 0x200
COUNTS = ("radiance_rays", "shadow_rays", "shaded_hits")


def _buffers(r):
    from optixpathtracer_amd import renderer as R

    out = {name: r.download(b).copy() for name, b in (("accum", R.PT_BUF_ACCUM), ("color", R.PT_BUF_COLOR), ("normal", R.PT_BUF_NORMAL), ("albedo", R.PT_BUF_ALBEDO))}
    out["frame"] = r.downloadPixels().copy()
    return out


def _run(monkeypatch, env, model, probe, camera, size, draw, options=None, partition=None):
    """one context under `env` (the switches are read at pt_create): draw(r) renders; returns (buffers, counts, stats)"""
    from optixpathtracer_amd import renderer as R

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = R.SampleRenderer(model)
    r.setProbe(probe)
    if options:
        r.setOptions(**options)
    if partition:
        r.setPartition(*partition)
    w, h = size
    r.resize((w, h))
    r.setCamera(R.make_camera(camera, w / h))
    draw(r)
    st = r.stats()
    out = _buffers(r)
    r.close()
    for k in env:
        monkeypatch.delenv(k)
    return out, {k: st[k] for k in COUNTS}, st


def _same(a, b, what):
    (ba, ca, _), (bb, cb, _) = a, b
    assert ca == cb, (what, ca, cb)
    for k in ba:
        if k == "frame":
            assert np.array_equal(ba[k], bb[k]), f"{what}: {k}"
        else:
            assert_bits_equal(ba[k], bb[k], f"{what}: {k}")


def _both(monkeypatch, *args, extra_env=None, carried=True, **kw):
    """the same render with carried sums and with the traversal write-back; returns the carried run"""
    extra_env = extra_env or {}
    on = _run(monkeypatch, {"PT_FUSED": "0", "PT_CARRY_SUMS": "1", **extra_env}, *args, **kw)
    off = _run(monkeypatch, {"PT_FUSED": "0", "PT_CARRY_SUMS": "0", **extra_env}, *args, **kw)
    assert bool(on[2]["schedule"] & CARRIED) == carried and not off[2]["schedule"] & CARRIED, (on[2]["schedule"], off[2]["schedule"])
    assert on[2]["fused_passes"] == 0 and off[2]["fused_passes"] == 0
    _same(on, off, "PT_CARRY_SUMS=1 against =0")
    return on


def _frames(spp, n=1, batch=0):
    def draw(r):
        r.launchParams.samples_per_launch = spp
        if batch:
            r.launchParams.frame.subframe_index = 0
            r.renderBatch(batch)
            return
        for k in range(n):
            r.launchParams.frame.subframe_index = k
            r.render()

    return draw


@pytest.fixture(scope="module")
def sky():
    return scenes.sky_probe(256, 128).BuildCDF()


@pytest.fixture(scope="module")
def terrain():
    return scenes.voxel_terrain(n=96, target_tris=70000)


@pytest.mark.parametrize("max_depth", [1, 2, 3, 4])
def test_cornell_box_every_chain_length(ptlib, orc_det, monkeypatch, sky, max_depth):
    """max_depth 1: the first launch is also the last (sums written at once, the shadow rays go out with their pending contribution);
    2: exactly one unified launch; the emissive light adds its emission to a primary hit ahead of a visible first contribution."""
    model = scenes.cornell_box()
    w, h, spp = 64, 64, 2
    on = _both(monkeypatch, model, sky, scenes.CORNELL_CAMERA, (w, h), _frames(spp), options=dict(max_depth=max_depth))
    U, V, W = scenes.uvw_frame(**scenes.CORNELL_CAMERA, aspect=w / h)
    ref = orc_det.render(orc_det.make_scene(model), orc_det.make_probe(sky), (U, V, W), scenes.CORNELL_CAMERA["eye"], w, h, spp, max_depth=max_depth)
    assert_bits_equal(on[0]["accum"], ref["accum"], f"accum against the checker, max_depth={max_depth}")
    assert np.array_equal(on[0]["frame"], ref["frame"])


@pytest.mark.parametrize("lds_skip", [None, "7"])
def test_small_chunks_steal_and_paths_end_in_the_sky(ptlib, monkeypatch, sky, terrain, lds_skip):
    """Rank 1 of a 3-way partition of a small frame: three pixel chunks whose launches are far below the grid size, so shadow rays finish in
    the stealing phase (the last co-worker stores the visibility word); paths leave into the sky right after a visible shadow ray.  Two
    subframes; once more with the traversal stack's LDS levels cut down (global spill path)."""
    extra = {"PT_STACK_LDS_SKIP": lds_skip} if lds_skip else {}
    on = _both(monkeypatch, terrain, sky, scenes.TERRAIN_CAMERA, (320, 192), _frames(3, n=2), partition=(1, 3, 64, 16), extra_env=extra)
    assert on[2]["trace_launches"] > 3 and on[1]["shadow_rays"] > 0


def test_fused_bounce_loop_agrees_with_the_carried_chain(ptlib, monkeypatch, sky, terrain):
    """the fused loop keeps the traversal write-back; both schedules still leave the same bits"""
    args = (terrain, sky, scenes.TERRAIN_CAMERA, (320, 192), _frames(3, n=2))
    chain = _run(monkeypatch, {"PT_FUSED": "0", "PT_CARRY_SUMS": "1"}, *args, partition=(1, 3, 64, 16))
    fused = _run(monkeypatch, {"PT_FUSED": "2", "PT_CARRY_SUMS": "1"}, *args, partition=(1, 3, 64, 16))
    assert chain[2]["schedule"] & CARRIED and chain[2]["fused_passes"] == 0
    assert fused[2]["fused_passes"] == 3 and not fused[2]["schedule"] & CARRIED
    _same(chain, fused, "launch chain with carried sums against the fused loop")


def test_two_sample_passes_per_chunk_and_a_batch(ptlib, monkeypatch, sky, terrain):
    """max_paths so small that a chunk's six samples (two subframes of three, one batch) take two passes of three: the arrays are reused by
    the second pass without a clear"""
    depth = 4
    on = _both(monkeypatch, terrain, sky, scenes.TERRAIN_CAMERA, (320, 192), _frames(3, batch=2), options=dict(max_depth=depth, max_paths=82000), partition=(1, 3, 64, 16))
    assert on[2]["trace_launches"] == 3 * 2 * depth, on[2]["trace_launches"]  # chunks x passes x (camera launch + depth - 1 unified launches)


def test_foveated_launches_leave_culled_slots_zero(ptlib, orc_det, monkeypatch, sky):
    """pt_render_regions with an annulus: paths outside it are never queued, their slots keep the generate kernel's zeros (a carried sum that
    is all +0 is not stored either)"""
    from optixpathtracer_amd.renderer import SampleRenderer

    model = scenes.cornell_box()
    w, h = 128, 96
    regs = SampleRenderer.foveatedRegions((w, h), (64, 48), 0, inner_radius=14, outer_radius=44, spp=(1, 2, 3))

    def draw(r):
        r.renderRegions(regs, SampleRenderer.SV4_VARIANT)

    on = _both(monkeypatch, model, sky, scenes.CORNELL_CAMERA, (w, h), draw, options=dict(max_depth=4))
    U, V, W = scenes.uvw_frame(**scenes.CORNELL_CAMERA, aspect=w / h)
    accum = np.zeros((h, w, 4), np.float32)
    frame = np.zeros((h, w), np.uint32)
    orc_det.render_regions(orc_det.make_scene(model, True), orc_det.make_probe(sky), (U, V, W), scenes.CORNELL_CAMERA["eye"], w, h, regs, SampleRenderer.SV4_VARIANT, 4, accum, frame)
    assert_bits_equal(on[0]["accum"], accum, "foveated accum against the checker")
    assert np.array_equal(on[0]["frame"], frame)


def test_paths_without_a_shadow_ray_beside_paths_with_one(ptlib, orc_det, monkeypatch, sky):
    """two materials, one with subsurface > 0: continuing paths whose record holds no pending contribution (kind 0) share waves with
    paths that wait for a shadow ray"""
    model = scenes.Model()
    scenes.add_box(model, scenes.Material(color=(0.8, 0.4, 0.3), subsurface=0.6, roughness=0.7), (0.0, 0.5, 0.0), (0.5, 0.5, 0.5))
    scenes.add_box(model, scenes.Material(), (0.0, -0.1, 0.0), (4.0, 0.1, 4.0))
    w, h, spp = 96, 64, 3
    on = _both(monkeypatch, model, sky, scenes.TWO_BOX_CAMERA, (w, h), _frames(spp), options=dict(max_depth=4))
    print("shadow rays", on[1]["shadow_rays"], "shaded hits", on[1]["shaded_hits"])
    assert 0 < on[1]["shadow_rays"] < on[1]["shaded_hits"]  # some shaded hits queued no shadow ray
    U, V, W = scenes.uvw_frame(**scenes.TWO_BOX_CAMERA, aspect=w / h)
    ref = orc_det.render(orc_det.make_scene(model), orc_det.make_probe(sky), (U, V, W), scenes.TWO_BOX_CAMERA["eye"], w, h, spp, max_depth=4)
    assert_bits_equal(on[0]["accum"], ref["accum"], "accum against the checker")


def test_shadow_catcher_scene_keeps_the_write_back(ptlib, monkeypatch, sky):
    model = scenes.two_box_scene(shadow_catcher=True)
    _both(monkeypatch, model, sky, scenes.TWO_BOX_CAMERA, (96, 64), _frames(2), options=dict(max_depth=3), carried=False)


@pytest.mark.parametrize("split_shadow", [1, 2])
def test_split_and_asynchronous_shadow_placement_keep_the_write_back(ptlib, monkeypatch, sky, split_shadow):
    model = scenes.cornell_box()
    off = _both(monkeypatch, model, sky, scenes.CORNELL_CAMERA, (64, 64), _frames(2), options=dict(max_depth=3, split_shadow=split_shadow), carried=False)
    on = _run(monkeypatch, {"PT_FUSED": "0"}, model, sky, scenes.CORNELL_CAMERA, (64, 64), _frames(2), options=dict(max_depth=3))
    assert on[2]["schedule"] & CARRIED  # the default: carried where eligible
    _same(on, off, "unified placement with carried sums against the other placements")
