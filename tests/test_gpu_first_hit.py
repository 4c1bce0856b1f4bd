"""The first-hit word (PT_LEAN_FIRST): in a scene without shadow catchers and without textures the first-hit normal and albedo
travel as ONE word per path — the hit's leaf triangle and the side it was seen from, in the place of the path's flag word — which the
resolve kernels turn back into 0 + (±N_0) and 0 + mat.color; nrm / alb are neither written nor read.  Every value is re-derived with the operations that produced it, so every case renders with PT_LEAN_FIRST=1 and =0 and
compares all five buffers and the three device-counted totals bit for bit (the sign of a zero included), and the accumulation buffer with
the CPU checker where the case has a counterpart there.  pt_stats.schedule bit 10 says whether the last render's paths kept the word."""
import numpy as np
import pytest

from conftest import assert_bits_equal, bits
from optixpathtracer_amd import scenes

pytestmark = pytest.mark.gpu

HITWORD = 0x400
COUNTS = ("radiance_rays", "shadow_rays", "shaded_hits")


def _buffers(r):
    from optixpathtracer_amd import renderer as R

    out = {name: r.download(b).copy() for name, b in (("accum", R.PT_BUF_ACCUM), ("color", R.PT_BUF_COLOR), ("normal", R.PT_BUF_NORMAL), ("albedo", R.PT_BUF_ALBEDO))}
    out["frame"] = r.downloadPixels().copy()
    return out


def _run(monkeypatch, env, model, probe, camera, size, draw, options=None, partition=None, views=None):
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
    if views:
        r.setViews([(x, y, vw, vh, R.make_camera(cam, vw / vh)) for x, y, vw, vh, cam in views])
    draw(r)
    st = r.stats()
    out = _buffers(r)
    r.close()
    for k in env:
        monkeypatch.delenv(k)
    return out, {k: st[k] for k in COUNTS}, st


def _same(a, b, what):
    """bit for bit: a -0 where the other run has +0 is a difference here"""
    (ba, ca, _), (bb, cb, _) = a, b
    assert ca == cb, (what, ca, cb)
    for k in ba:
        if k == "frame":
            assert np.array_equal(ba[k], bb[k]), f"{what}: {k}"
        else:
            assert_bits_equal(ba[k], bb[k], f"{what}: {k}")
            assert np.array_equal(bits(ba[k]), bits(bb[k])), f"{what}: {k} differs in the sign of a zero"


def _both(monkeypatch, *args, extra_env=None, word=True, **kw):
    """the same render with the first-hit word and with nrm / alb; `word`: whether the first run must report the word; returns the first run"""
    extra_env = extra_env or {}
    on = _run(monkeypatch, {"PT_LEAN_FIRST": "1", **extra_env}, *args, **kw)
    off = _run(monkeypatch, {"PT_LEAN_FIRST": "0", **extra_env}, *args, **kw)
    assert bool(on[2]["schedule"] & HITWORD) == word and not off[2]["schedule"] & HITWORD, (hex(on[2]["schedule"]), hex(off[2]["schedule"]))
    _same(on, off, "PT_LEAN_FIRST=1 against =0")
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


def _first_hit_sides(model, camera, w, h):
    """Pixel-centre camera rays against every triangle of the scene, on the CPU: per pixel the nearest triangle (-1: none) and, per
    triangle, the stored normal normalize(cross(v1 - v0, v2 - v0)) in float32 with the device's expressions.  Returns (flip bit of each
    pixel's first hit, -1 where it hit nothing; the normals of the triangles that are somebody's first hit)."""
    f = np.float32
    verts, idx, _, _ = model.flatten()
    v0, v1, v2 = (verts[idx[:, k]].astype(f) for k in range(3))
    a, b = v1 - v0, v2 - v0
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(f)
    n0 = (c * (f(1.0) / np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]).astype(f)))[:, None]).astype(f)
    U, V, W = (np.asarray(x, np.float64) for x in scenes.uvw_frame(**camera, aspect=w / h))
    ys, xs = np.mgrid[0:h, 0:w]
    dx, dy = 2.0 * (xs + 0.5) / w - 1.0, 2.0 * (ys + 0.5) / h - 1.0
    d = dx[..., None] * U + dy[..., None] * V + W
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 1, 3)
    o = np.asarray(camera["eye"], np.float64)
    e1, e2 = (v1 - v0).astype(np.float64)[None], (v2 - v0).astype(np.float64)[None]  # Moeller-Trumbore, rays x triangles
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        tv = o - v0.astype(np.float64)[None]
        u = (tv * p).sum(-1) / det
        q = np.cross(tv, e1)
        v = (d * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
    ok = (np.abs(det) > 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-3)
    t = np.where(ok, t, np.inf)
    tri = np.where(np.isfinite(t.min(1)), t.argmin(1), -1)
    hit = tri >= 0
    facing = (-(d[:, 0, :]) * n0[np.maximum(tri, 0)].astype(np.float64)).sum(-1)
    flip = np.where(hit, np.signbit(facing).astype(np.int64), -1)
    return flip, n0[np.unique(tri[hit])]


# The scene's own camera looks in through the open front and sees every face from the side its winding faces.  This one stands outside, to the
# left of and above the box: the green wall and the ceiling from behind (flip bit 1), the floor, the back and the blocks through the opening
# (flip bit 0), and sky around the box.
OUTSIDE_CAMERA = dict(eye=(-500.0, 800.0, -700.0), lookat=(278.0, 273.0, 280.0), up=(0.0, 1.0, 0.0), fovY=40.0)


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("max_depth", [0, 1, 8])
def test_cornell_box_both_sides_and_negative_zero_normals(ptlib, orc_det, monkeypatch, sky, spp, max_depth):
    """Axis-aligned walls store normals with -0 components (0 + -0 = +0 in the buffer), and the camera sees faces from both sides of their
    stored winding.  max_depth 0: the bounce-0 shade is the chain's first and last launch — it writes the word and ends every path; 1 and 8:
    the word is written by the first launch of a longer chain and survives the later ones."""
    model = scenes.cornell_box()
    w, h = 64, 64
    flip, normals = _first_hit_sides(model, OUTSIDE_CAMERA, w, h)
    print("pixels seen from the stored side / from behind / hitting nothing:", int((flip == 0).sum()), int((flip == 1).sum()), int((flip < 0).sum()))
    assert (flip == 0).sum() >= 256 and (flip == 1).sum() >= 256  # both values of the flip bit, far more than a handful of edge pixels
    assert (np.signbit(normals) & (normals == 0)).any()  # a first-hit normal with a -0 component
    on = _both(monkeypatch, model, sky, OUTSIDE_CAMERA, (w, h), _frames(spp), options=dict(max_depth=max_depth), extra_env={"PT_FUSED": "0"})
    U, V, W = scenes.uvw_frame(**OUTSIDE_CAMERA, aspect=w / h)
    ref = orc_det.render(orc_det.make_scene(model), orc_det.make_probe(sky), (U, V, W), OUTSIDE_CAMERA["eye"], w, h, spp, max_depth=max_depth)
    assert_bits_equal(on[0]["accum"], ref["accum"], f"accum against the checker, max_depth={max_depth}")
    assert np.array_equal(on[0]["frame"], ref["frame"])
    assert np.abs(on[0]["normal"][..., :3]).max() > 0.9 and on[0]["albedo"][..., :3].max() > 0.7  # the AOVs are there at all


def test_terrain_with_sky_paths_that_never_hit(ptlib, monkeypatch, sky, terrain):
    """sky pixels: their paths keep the word the generate kernel wrote and add +0"""
    w, h, spp = 96, 64, 4
    on = _both(monkeypatch, terrain, sky, scenes.TERRAIN_CAMERA, (w, h), _frames(spp), extra_env={"PT_FUSED": "0"})
    alpha_free = on[0]["albedo"][..., :3].sum(-1) == 0
    print("pixels without a first hit in any sample:", int(alpha_free.sum()))
    assert 0 < alpha_free.sum() < w * h


def test_two_sample_passes_per_chunk_and_a_batch(ptlib, monkeypatch, sky, terrain):
    """max_paths so small that the eight samples of a pixel (two subframes of four, one batch) take two passes: the first-hit words of the
    first pass are overwritten by the second pass's generate"""
    w, h = 96, 64
    on = _both(monkeypatch, terrain, sky, scenes.TERRAIN_CAMERA, (w, h), _frames(4, batch=2), options=dict(max_depth=4, max_paths=w * h * 4), extra_env={"PT_FUSED": "0"})
    assert on[2]["trace_launches"] >= 2 * 4, on[2]["trace_launches"]  # at least two passes of (camera launch + depth - 1 unified launches)


@pytest.mark.parametrize("env", [{"PT_CAM_MIN_PATHS": "1"}, {"PT_CAM_PACKETS": "0"}], ids=["packets", "per_ray"])
def test_packet_kernel_and_per_ray_camera_kernel(ptlib, monkeypatch, sky, terrain, env):
    """the word is the leaf index of either camera kernel's hit record (by default a frame this small takes the per-ray kernel)"""
    a = _both(monkeypatch, terrain, sky, scenes.TERRAIN_CAMERA, (96, 64), _frames(3), extra_env={"PT_FUSED": "0", **env})
    b = _run(monkeypatch, {"PT_FUSED": "0", "PT_LEAN_FIRST": "0"}, terrain, sky, scenes.TERRAIN_CAMERA, (96, 64), _frames(3))
    _same(a, b, "against the default camera kernel of the parent's layout")


def test_fused_loop_against_the_chain(ptlib, monkeypatch, sky, terrain):
    """the fused loop shares generate_path and shade_path, so its paths keep the word as well; both schedules leave the same bits"""
    args = (terrain, sky, scenes.TERRAIN_CAMERA, (320, 192), _frames(3, n=2))
    chain = _both(monkeypatch, *args, partition=(1, 3, 64, 16), extra_env={"PT_FUSED": "0"})
    fused = _both(monkeypatch, *args, partition=(1, 3, 64, 16), extra_env={"PT_FUSED": "2"})
    assert chain[2]["fused_passes"] == 0 and fused[2]["fused_passes"] == 3
    _same(chain, fused, "launch chain against the fused loop")


def test_textured_scene_keeps_the_arrays(ptlib, monkeypatch, sky):
    """a textured mesh's albedo is a texture lookup at the hit point: nrm / alb stay, both values of the switch give the same bits"""
    from surface_ref import TEX_CAMERA, textured_scene

    for fused in ("0", "2"):
        _both(monkeypatch, textured_scene(), sky, TEX_CAMERA, (96, 64), _frames(2), options=dict(max_depth=3), extra_env={"PT_FUSED": fused}, word=False)


def test_shadow_catcher_scene_keeps_the_arrays(ptlib, monkeypatch, sky):
    """pass-throughs re-add prd.normal: nrm / alb are running sums, alpha a float"""
    model = scenes.two_box_scene(shadow_catcher=True)
    _both(monkeypatch, model, sky, scenes.TWO_BOX_CAMERA, (96, 64), _frames(2), options=dict(max_depth=3), word=False)


def test_viewports_with_different_eyes(ptlib, monkeypatch, sky):
    """two views with different eyes: the *_views kernels generate and resolve; the side a face is seen from is the view's"""
    model = scenes.cornell_box()
    left = dict(scenes.CORNELL_CAMERA, eye=(200.0, 273.0, -900.0))
    right = dict(scenes.CORNELL_CAMERA, eye=(356.0, 300.0, -850.0))
    views = [(0, 0, 64, 64, left), (64, 0, 64, 64, right)]
    on = _both(monkeypatch, model, sky, scenes.CORNELL_CAMERA, (128, 64), _frames(2), options=dict(max_depth=3), views=views, extra_env={"PT_FUSED": "0"})
    assert not np.array_equal(on[0]["accum"][:, :64], on[0]["accum"][:, 64:])  # two different cameras


def test_foveated_launch_with_a_culled_annulus(ptlib, orc_det, monkeypatch, sky):
    """pt_render_regions: paths outside the annulus are never queued and contribute nothing; the launches keep pflags / nrm / alb, in a context
    whose plain frames use the word"""
    from optixpathtracer_amd.renderer import SampleRenderer

    model = scenes.cornell_box()
    w, h = 128, 96
    regs = SampleRenderer.foveatedRegions((w, h), (64, 48), 0, inner_radius=14, outer_radius=44, spp=(1, 2, 3))

    def draw(r):
        r.launchParams.samples_per_launch = 2
        r.launchParams.frame.subframe_index = 0
        r.render()  # a plain frame first: the sets' flag words hold first-hit words when the foveated frame arrives
        r.renderRegions(regs, SampleRenderer.SV4_VARIANT)

    on = _both(monkeypatch, model, sky, scenes.CORNELL_CAMERA, (w, h), draw, options=dict(max_depth=4), word=False)

    def only_regions(r):
        r.renderRegions(regs, SampleRenderer.SV4_VARIANT)

    alone = _both(monkeypatch, model, sky, scenes.CORNELL_CAMERA, (w, h), only_regions, options=dict(max_depth=4), word=False)
    U, V, W = scenes.uvw_frame(**scenes.CORNELL_CAMERA, aspect=w / h)
    accum = np.zeros((h, w, 4), np.float32)
    frame = np.zeros((h, w), np.uint32)
    orc_det.render_regions(orc_det.make_scene(model, True), orc_det.make_probe(sky), (U, V, W), scenes.CORNELL_CAMERA["eye"], w, h, regs, SampleRenderer.SV4_VARIANT, 4, accum, frame)
    assert_bits_equal(alone[0]["accum"], accum, "foveated accum against the checker")
    assert np.array_equal(alone[0]["frame"], frame)
    assert on[1] == alone[1]  # the totals are those of the last render


@pytest.mark.parametrize("split_shadow", [1, 2])
def test_split_and_asynchronous_shadow_placement(ptlib, monkeypatch, sky, split_shadow):
    """the other shadow placements keep k_shade (not k_shade_carry) and the traversal write-back: the word is written by that kernel too"""
    model = scenes.cornell_box()
    on = _both(monkeypatch, model, sky, scenes.CORNELL_CAMERA, (64, 64), _frames(2), options=dict(max_depth=3, split_shadow=split_shadow))
    unified = _run(monkeypatch, {"PT_FUSED": "0"}, model, sky, scenes.CORNELL_CAMERA, (64, 64), _frames(2), options=dict(max_depth=3))
    _same(on, unified, "against the unified placement")
