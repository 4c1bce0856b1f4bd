"""The depth limit over its whole range: pt_options.max_depth 0, 29 ... 32 (the asynchronous shadow records stop at 31), 64, 249, 250, and
changes of the limit on a live context.

The limit is the most special-cased index of the bounce code: enqueue_chunk's last_bounce and the first / second / last flags of k_shade,
the per-bounce counter slots and the (b & 1) side stream of the asynchronous shadow rays, ensure_path_state's nq, async_shadows() turning
itself off at 31, depth | flags << 8 in the path state, the fused loop's own cutoff.  Every comparison here is bit for bit — all five
buffers against the CPU checker (or, where the existing tests do the same, against a fresh context) — and the device-counted totals are
pinned to the checker's ray counts:

  the chain skips the provably dead trace at depth == max_depth and counts the paths that would continue, so for a scene without catchers
      radiance_rays_gpu(D) == radiance_rays_checker(D - 1)   (D >= 1;  D = 0: the one trace is live, == paths)
      shaded_hits_gpu(D)   == radiance_rays_checker(D) - paths
  and radiance_rays, shadow_rays, shaded_hits and paths are the same for every schedule and placement of a case.

The scene is tests/test_depth_limit_scene.py's skylight box, whose conditions (paths alive at depth 249, different frames at 0, 1, 2, 30,
31, 32) are checked there on the checker alone."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
from depth_limit_scene import CAMERA, DEEP_DEPTHS, LAMBERT, SPP_DEEP, SPP_EDGE, S_DEEP, S_EDGE, H, W, checker_frame, sky, skylight_box
from optixpathtracer_amd import scenes
from parity_kit import _check_sched, _compare, _gpu_render, _oracle_render, _renderer

pytestmark = pytest.mark.gpu

COUNTS = ("radiance_rays", "shadow_rays", "shaded_hits", "paths")
TEXTURED_CAMERA = dict(eye=(3.0, 2.5, -4.5), lookat=(0.0, 0.6, 0.5), up=(0.0, 1.0, 0.0), fovY=45.0)


@pytest.fixture(scope="module")
def probe():
    return sky()


def _pin(monkeypatch, sched, carry=None, cap=None, always_fused=False):
    """the switches a context reads at pt_create: which schedule a synchronous frame takes, carried sums, the fused loop's window"""
    monkeypatch.setenv("PT_FUSED", "0" if sched == "chain" else "2" if always_fused else "1")
    monkeypatch.setenv("PT_SCHED_TRIALS", "0")
    monkeypatch.setenv("PT_FUSED_MAX_COST", "1e9")
    if carry is not None:
        monkeypatch.setenv("PT_CARRY_SUMS", carry)
    else:
        monkeypatch.delenv("PT_CARRY_SUMS", raising=False)
    if cap is not None:
        monkeypatch.setenv("PT_FUSED_CAP", cap)
    else:
        monkeypatch.delenv("PT_FUSED_CAP", raising=False)


def _counts(st):
    return {k: int(st[k]) for k in COUNTS}


def _check_counts(counts, at_depth, below, npaths, depth):
    """the identities of the module docstring; at_depth / below: the checker's one-subframe frames at max_depth and max_depth - 1"""
    print(f"max_depth {depth}: gpu {counts}, checker radiance {at_depth['radiance_rays']} shadow {at_depth['shadow_rays']}")
    assert counts["paths"] == npaths
    assert counts["radiance_rays"] <= at_depth["radiance_rays"] and counts["shadow_rays"] <= at_depth["shadow_rays"], (counts, at_depth["radiance_rays"], at_depth["shadow_rays"])
    assert counts["radiance_rays"] == (npaths if depth == 0 else below["radiance_rays"]), (depth, counts)
    assert counts["shaded_hits"] == at_depth["radiance_rays"] - npaths, (depth, counts, at_depth["radiance_rays"])


_BOX_COUNTS = {}


def _box_case(orc_det, probe, s, spp, depth, sched=None, subframes=1, **opt):
    """One context on the skylight box: subframe 0 (the counts: against the checker's, and against every other run of the same case),
    then up to `subframes`: all five buffers against the checker's."""
    from optixpathtracer_amd import renderer as R

    r = _renderer(skylight_box(s), probe, CAMERA, W, H, max_depth=depth, bsdf_mode=LAMBERT, **opt)
    g = _gpu_render(r, spp)
    if sched:
        _check_sched(g, sched)
    _compare(g, checker_frame(orc_det, s, spp, depth))
    counts = _counts(g["stats"])
    _check_counts(counts, checker_frame(orc_det, s, spp, depth), checker_frame(orc_det, s, spp, max(depth - 1, 0)), W * H * spp, depth)
    assert _BOX_COUNTS.setdefault((s, spp, depth), counts) == counts, (depth, opt, counts, _BOX_COUNTS[(s, spp, depth)])
    for sf in range(1, subframes):
        r.launchParams.frame.subframe_index = sf
        r.render()
    if subframes > 1:
        g = dict(accum=r.download(R.PT_BUF_ACCUM), frame=r.download(R.PT_BUF_FRAME), normal=r.download(R.PT_BUF_NORMAL), color=r.download(R.PT_BUF_COLOR), albedo=r.download(R.PT_BUF_ALBEDO))
        _compare(g, checker_frame(orc_det, s, spp, depth, subframes=subframes))
    r.close()
    return g


# ---------------------------------------------------------------- the count identities where the suite already passes
def test_count_identities_hold_at_depth_8(ptlib, orc_det, monkeypatch, probe):
    """test_render_cornell_disney_4spp_depth8's setup (Cornell box, 240 x 136, 4 spp, Disney, depth 8), both schedules: the identities the
    cases below rely on, where the buffers are known to agree"""
    m = scenes.cornell_box()
    w, h, spp = 240, 136, 4
    o8 = _oracle_render(orc_det, m, probe, scenes.CORNELL_CAMERA, w, h, spp)
    o7 = _oracle_render(orc_det, m, probe, scenes.CORNELL_CAMERA, w, h, spp, max_depth=7)
    seen = []
    for sched in ("chain", "fused"):
        _pin(monkeypatch, sched)
        g = _gpu_render(_renderer(m, probe, scenes.CORNELL_CAMERA, w, h), spp)
        _check_sched(g, sched)
        _compare(g, o8)
        _check_counts(_counts(g["stats"]), o8, o7, w * h * spp, 8)
        seen.append(_counts(g["stats"]))
    assert seen[0] == seen[1]


# ---------------------------------------------------------------- 1. max_depth = 0
def _depth0_scene(name):
    if name == "cornell":
        return scenes.cornell_box(), scenes.CORNELL_CAMERA, False
    if name == "textured":
        return scenes.textured_scene(), TEXTURED_CAMERA, False
    if name == "skylight":
        return skylight_box(S_EDGE), CAMERA, False
    return scenes.two_box_scene(True), scenes.TWO_BOX_CAMERA, True


_DEPTH0 = {}


def _depth0_checker(O, name, probe, mode, subframes, spp):
    key = (name, mode, subframes, spp)
    if key not in _DEPTH0:
        m, cam, _ = _depth0_scene(name)
        _DEPTH0[key] = _oracle_render(O, m, probe, cam, W, H, spp, subframes=subframes, max_depth=0, bsdf_mode=mode, use_bvh=False)
        for v in _DEPTH0[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _DEPTH0[key]


@pytest.mark.parametrize("sched", ["chain", "fused"])
@pytest.mark.parametrize("name", ["cornell", "textured", "skylight", "two_box_catcher"])
def test_depth_0_is_the_first_hit_without_light(ptlib, orc_det, monkeypatch, probe, name, sched):
    """The reference at max_depth 0 (deviceProgram.cu:411-443): the camera ray is traced and its closest-hit program runs — first-hit normal
    and albedo are added (from a texture in the textured scene), alpha becomes 1 — and the loop breaks before any radiance is added: hit
    pixels are black with their AOVs written, miss pixels show the backplate.  Disney and Lambert, one and two subframes."""
    m, cam, catcher = _depth0_scene(name)
    spp = 2 if catcher else 4
    _pin(monkeypatch, sched)
    for mode in (0, 1):
        for subframes in (1, 2):
            g = _gpu_render(_renderer(m, probe, cam, W, H, max_depth=0, bsdf_mode=mode), spp, subframes=subframes)
            _check_sched(g, "chain" if catcher else sched)  # (a scene with shadow catchers always takes the chain)
            o = _depth0_checker(orc_det, name, probe, mode, subframes, spp)
            _compare(g, o)
            st = _counts(g["stats"])
            assert st["paths"] == W * H * spp and st["radiance_rays"] <= o["radiance_rays"] and st["shadow_rays"] <= o["shadow_rays"], (st, o["radiance_rays"], o["shadow_rays"])
            if not catcher:  # the one trace per path is live, nothing is shaded on, no light sample is used
                assert st == dict(radiance_rays=W * H * spp, shadow_rays=0, shaded_hits=0, paths=W * H * spp), st
                assert o["radiance_rays"] == W * H * spp and g["stats"]["shadow_launches"] == 0
    hit = (o["normal"][..., :3] != 0).any(axis=-1)
    assert hit.mean() > 0.2 and (name == "skylight" or hit.mean() < 1.0)  # hits and (outside the closed room) misses are both in the frame


@pytest.mark.parametrize("sched", ["chain", "fused"])
def test_depth_0_batch_views_and_mask(ptlib, orc_det, monkeypatch, probe, sched):
    from optixpathtracer_amd import renderer as R

    m, cam, spp = scenes.cornell_box(), scenes.CORNELL_CAMERA, 4
    _pin(monkeypatch, sched)
    # pt_render_batch: three subframes as one batch
    r = _renderer(m, probe, cam, W, H, max_depth=0)
    r.launchParams.samples_per_launch = spp
    r.launchParams.frame.subframe_index = 0
    r.renderBatch(3)
    g = dict(accum=r.download(R.PT_BUF_ACCUM), frame=r.download(R.PT_BUF_FRAME), normal=r.download(R.PT_BUF_NORMAL), color=r.download(R.PT_BUF_COLOR), albedo=r.download(R.PT_BUF_ALBEDO), stats=r.stats())
    _check_sched(g, sched)
    _compare(g, _depth0_checker(orc_det, "cornell", probe, 0, 3, spp))
    assert g["stats"]["paths"] == g["stats"]["radiance_rays"] == 3 * W * H * spp
    # a block mask: the chosen 8 x 8 blocks are the frame's, every other pixel stays what pt_resize left
    r = _renderer(m, probe, cam, W, H, max_depth=0)
    r.launchParams.samples_per_launch = spp
    nby, nbx = r.blockGrid()
    mask = (np.add.outer(np.arange(nby), np.arange(nbx)) % 3 != 1).astype(np.uint8)
    assert r.renderMask(mask) == int(mask.sum()) * 64
    px = np.kron(mask, np.ones((8, 8), np.uint8)).astype(bool)[:H, :W]
    o = _depth0_checker(orc_det, "cornell", probe, 0, 1, spp)
    for name, which in (("accum", R.PT_BUF_ACCUM), ("frame", R.PT_BUF_FRAME), ("normal", R.PT_BUF_NORMAL), ("color", R.PT_BUF_COLOR), ("albedo", R.PT_BUF_ALBEDO)):
        got = r.download(which)
        assert np.array_equal(got[px].view(np.uint32), np.asarray(o[name]).reshape(got.shape)[px].view(np.uint32)), f"masked frame: {name}"
        assert not got[~px].any(), f"masked frame: {name} outside the mask"
    # two views: each rectangle holds the checker's frame of the view's own size and camera
    r = _renderer(m, probe, cam, W, H, max_depth=0)
    rects = [(0, 0, 21, 32), (24, 8, 24, 13)]  # (views begin on 8 x 8 block boundaries and share no block)
    cams = [cam, dict(cam, eye=(100.0, 300.0, -700.0))]
    r.setViews([(x, y, w, h, R.make_camera(c, w / h)) for (x, y, w, h), c in zip(rects, cams)])
    g = _gpu_render(r, spp, subframes=2)
    _check_sched(g, sched)
    inside = np.zeros((H, W), bool)
    for (x, y, w, h), c in zip(rects, cams):
        o = _oracle_render(orc_det, m, probe, c, w, h, spp, subframes=2, max_depth=0, use_bvh=False)
        _compare({k: g[k][y:y + h, x:x + w] for k in ("accum", "color", "normal", "albedo", "frame")}, o)
        inside[y:y + h, x:x + w] = True
    assert all(not g[k][~inside].any() for k in ("accum", "color", "normal", "albedo", "frame"))


def test_depth_0_frames_in_flight_and_regions(ptlib, orc_det, monkeypatch, probe):
    from optixpathtracer_amd.renderer import SampleRenderer

    m, cam, spp = scenes.cornell_box(), scenes.CORNELL_CAMERA, 4
    _pin(monkeypatch, "chain")
    g = _gpu_render(_renderer(m, probe, cam, W, H, max_depth=0, frames_in_flight=3), spp, subframes=3)
    _compare(g, _depth0_checker(orc_det, "cornell", probe, 0, 3, spp))
    # pt_render_regions with initial_depth 0 goes through the same chain: the sv4 variant's three launches, two frames with a moving gaze
    r = _renderer(m, probe, cam, W, H, max_depth=0)
    accum, frame = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32)
    sc, pr = orc_det.make_scene(m, False), orc_det.make_probe(probe)
    U, V, Wv = scenes.uvw_frame(**cam, aspect=W / H)
    for k, gaze in enumerate(FOV_GAZES):
        regs = SampleRenderer.foveatedRegions((W, H), gaze, k, **FOV)
        r.renderRegions(regs, SampleRenderer.SV4_VARIANT)
        orc_det.render_regions(sc, pr, (U, V, Wv), cam["eye"], W, H, regs, SampleRenderer.SV4_VARIANT, 0, accum, frame)
        assert_bits_equal(r.download(0), accum, f"depth 0, foveated accum, frame {k}")
        assert np.array_equal(r.download(1), frame), f"depth 0, foveated frame buffer, frame {k}"
    assert r.stats()["shade_launches"] >= 1 and r.stats()["shadow_launches"] == 0


# ---------------------------------------------------------------- 2. the asynchronous-shadow boundary
@pytest.mark.parametrize("split_shadow", [0, 1, 2])
@pytest.mark.parametrize("depth", [29, 30, 31, 32])
def test_async_shadow_boundary(ptlib, orc_det, monkeypatch, probe, depth, split_shadow):
    """split_shadow = 2 keeps per-bounce shadow records (one visibility bit per bounce) below max_depth 31 and silently falls back to the
    split placement from 31 on; one and three chunk streams"""
    _pin(monkeypatch, "chain")
    for streams in (1, 3):
        _box_case(orc_det, probe, S_EDGE, SPP_EDGE, depth, "chain", split_shadow=split_shadow, streams=streams)


# ---------------------------------------------------------------- 3. deep
DEEP_CONFIGS = {
    "chain_carried": dict(sched="chain", carry="1"),
    "chain_write_back": dict(sched="chain", carry="0"),
    "fused": dict(sched="fused"),
    "fused_cap64": dict(sched="fused", cap="64"),
    "chain_sample_passes": dict(sched="chain", opt=dict(max_paths=3000)),
    "fused_sample_passes": dict(sched="fused", always_fused=True, opt=dict(max_paths=3000)),
}


@pytest.mark.parametrize("config", list(DEEP_CONFIGS))
@pytest.mark.parametrize("depth", DEEP_DEPTHS)
def test_deep_limits(ptlib, orc_det, monkeypatch, probe, depth, config):
    """max_depth 64, 249, 250 with thousands of paths alive at the limit: the image stops changing near depth 100, the ray counts do not.
    max_paths = 3000 cuts the frame's 12288 paths into several sample passes per chunk."""
    c = DEEP_CONFIGS[config]
    _pin(monkeypatch, c["sched"], carry=c.get("carry"), cap=c.get("cap"), always_fused=c.get("always_fused", False))
    _box_case(orc_det, probe, S_DEEP, SPP_DEEP, depth, c["sched"], subframes=2, **c.get("opt", {}))


def test_deep_limit_with_a_shadow_catcher(ptlib, orc_det, monkeypatch, probe):
    """the catcher variant at 250 on the chain: one sample per pass, max_depth + 1 launches and the pass-through iterations behind them"""
    _pin(monkeypatch, "chain")
    spp = 2
    r = _renderer(skylight_box(S_DEEP, catcher=True), probe, CAMERA, W, H, max_depth=250, bsdf_mode=LAMBERT)
    g = _gpu_render(r, spp, subframes=2)
    _check_sched(g, "chain")
    o = checker_frame(orc_det, S_DEEP, spp, 250, subframes=2, catcher=True)
    _compare(g, o)
    assert g["stats"]["radiance_rays"] <= o["radiance_rays"] and g["stats"]["shadow_rays"] <= o["shadow_rays"]
    assert g["stats"]["trace_launches"] >= spp * 251


# ---------------------------------------------------------------- 4. foveated launches
FOV = dict(inner_radius=3, outer_radius=6, spp=(1, 2, 2))  # the regions stay inside the 48 x 32 image for both gaze points
FOV_GAZES = [(24, 16), (20, 14)]


@pytest.mark.parametrize("variant_name,depth,split_shadow", [("SV_VARIANT", 2, 0), ("SV_VARIANT", 250, 0), ("SV4_VARIANT", 1, 0), ("SV4_VARIANT", 250, 0),
                                                             ("SV_VARIANT", 2, 2), ("SV_VARIANT", 30, 2), ("SV4_VARIANT", 30, 2)])
def test_foveated_launches_at_the_ends_of_the_range(ptlib, orc_det, monkeypatch, probe, variant_name, depth, split_shadow):
    """The sv / sv2 variants start their paths at depth 1 (max_depth 2 is the smallest the API allows: one live bounce), sv4 at 0.  With
    split_shadow = 2 the per-bounce shadow records are addressed by the path's depth, one ahead of the bounce for sv / sv2."""
    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd.renderer import SampleRenderer

    _pin(monkeypatch, "chain")
    variant = getattr(SampleRenderer, variant_name)
    m = skylight_box(S_DEEP)
    r = _renderer(m, probe, CAMERA, W, H, max_depth=depth, bsdf_mode=LAMBERT, split_shadow=split_shadow)
    sc, pr = orc_det.make_scene(m, False), orc_det.make_probe(probe)
    U, V, Wv = scenes.uvw_frame(**CAMERA, aspect=W / H)
    accum, frame = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32)
    aov = [np.zeros((H, W, 4), np.float32) for _ in range(3)] if variant.get("write_aov") else None
    for k, gaze in enumerate(FOV_GAZES):
        regs = SampleRenderer.foveatedRegions((W, H), gaze, k, **FOV)
        r.renderRegions(regs, variant)
        orc_det.render_regions(sc, pr, (U, V, Wv), CAMERA["eye"], W, H, regs, variant, depth, accum, frame, bsdf_mode=LAMBERT, aov=aov)
        assert_bits_equal(r.download(R.PT_BUF_ACCUM), accum, f"{variant_name} at {depth}: accum_buffer, frame {k}")
        assert np.array_equal(r.download(R.PT_BUF_FRAME), frame), f"{variant_name} at {depth}: frame_buffer, frame {k}"
        if aov:
            for which, a in zip((R.PT_BUF_NORMAL, R.PT_BUF_COLOR, R.PT_BUF_ALBEDO), aov):
                assert_bits_equal(r.download(which), a, f"{variant_name} at {depth}: buffer {which}, frame {k}")
    assert (accum[..., :3] != 0).any() and r.stats()["shade_launches"] >= depth - variant.get("initial_depth", 0)


def test_foveated_initial_depth_needs_a_live_bounce(ptlib, monkeypatch, probe):
    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd.renderer import SampleRenderer

    _pin(monkeypatch, "chain")
    r = _renderer(skylight_box(S_EDGE), probe, CAMERA, W, H, max_depth=1, bsdf_mode=LAMBERT)
    before = _gpu_render(r, 2)
    regs = SampleRenderer.foveatedRegions((W, H), FOV_GAZES[0], 0, **FOV)
    with pytest.raises(RuntimeError, match="initial_depth must be 0 or below max_depth"):
        r.renderRegions(regs, SampleRenderer.SV_VARIANT)
    for k, which in (("accum", R.PT_BUF_ACCUM), ("frame", R.PT_BUF_FRAME), ("normal", R.PT_BUF_NORMAL), ("color", R.PT_BUF_COLOR), ("albedo", R.PT_BUF_ALBEDO)):
        assert np.array_equal(r.download(which).view(np.uint32), before[k].view(np.uint32)), k


# ---------------------------------------------------------------- 5. the limit changes on a live context
LIVE_DEPTHS = (8, 1, 250, 31, 30, 0, 2)
_LIVE_FRESH = {}


def _live_frame(r, spp):
    g = _gpu_render(r, spp, subframes=2)
    r.sync()
    return g


@pytest.mark.parametrize("fif", [0, 2])
def test_the_limit_changes_on_a_live_context(ptlib, monkeypatch, probe, fif):
    """8 -> 1 -> 250 -> 31 -> 30 -> 0 -> 2 with split_shadow = 2: the counter slots only grow, the asynchronous records go at 250 and come
    back at 30.  Two progressive subframes at each step; buffers and counts must be a fresh context's at that depth, and the path state is
    re-allocated exactly where the asynchronous records flip (a smaller limit alone re-allocates nothing)."""
    _pin(monkeypatch, "chain")
    m = skylight_box(S_DEEP)
    r = _renderer(m, probe, CAMERA, W, H, max_depth=LIVE_DEPTHS[0], bsdf_mode=LAMBERT, split_shadow=2, frames_in_flight=fif)
    allocs = []
    for depth in LIVE_DEPTHS:
        r.setOptions(max_depth=depth, bsdf_mode=LAMBERT, split_shadow=2, frames_in_flight=fif)
        g = _live_frame(r, SPP_DEEP)
        allocs.append(g["stats"]["path_state_allocs"])
        if depth not in _LIVE_FRESH:  # (a synchronous fresh context: the yardstick of both runs)
            f = _renderer(m, probe, CAMERA, W, H, max_depth=depth, bsdf_mode=LAMBERT, split_shadow=2)
            _LIVE_FRESH[depth] = _live_frame(f, SPP_DEEP)
            f.close()
        fresh = _LIVE_FRESH[depth]
        _compare(g, fresh)
        assert _counts(g["stats"]) == _counts(fresh["stats"]), (depth, _counts(g["stats"]), _counts(fresh["stats"]))
    print("path_state_allocs after each step:", dict(zip(LIVE_DEPTHS, allocs)))
    steps = [b - a for a, b in zip([0] + allocs, allocs)]
    assert steps == [1, 0, 1, 0, 1, 0, 0], steps
    # the frames of different limits really differ (else the comparisons above could not tell a stale limit)
    c = {d: tuple(_counts(_LIVE_FRESH[d]["stats"]).values()) for d in LIVE_DEPTHS}  # (0 and 1 trace the same rays; 1 shades on)
    assert len(set(c.values())) == len(LIVE_DEPTHS), c


# ---------------------------------------------------------------- 6. refusals
def test_limits_out_of_range_are_refused(ptlib, monkeypatch, probe):
    from optixpathtracer_amd import _lib

    _pin(monkeypatch, "chain")
    m = skylight_box(S_EDGE)
    r = _renderer(m, probe, CAMERA, W, H, max_depth=30, bsdf_mode=LAMBERT, split_shadow=2)

    def options():
        o = _lib.Options()
        assert r._L.pt_get_options(r._ctx, C.byref(o)) == 0
        return bytes(o)

    _gpu_render(r, SPP_EDGE)
    before = options()
    for bad in (-1, 251):
        with pytest.raises(RuntimeError, match=r"out of range \[0,250\]"):
            r.setOptions(max_depth=bad, bsdf_mode=LAMBERT, split_shadow=2)
        assert options() == before
    g = _gpu_render(r, SPP_EDGE, subframes=2)
    f = _gpu_render(_renderer(m, probe, CAMERA, W, H, max_depth=30, bsdf_mode=LAMBERT, split_shadow=2), SPP_EDGE, subframes=2)
    _compare(g, f)
    assert _counts(g["stats"]) == _counts(f["stats"])
