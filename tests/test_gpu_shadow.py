"""Sun shadows and direct light from the G-buffer (pt_shadow_layout, pt_shadow_planes) on the GPU.  visibility and light are compared bit
for bit over WHOLE sentinel-filled planes, and all nine counters exactly, with an expectation the code under test never produces:
tests/shadow_ref.py builds the rays in float32 NumPy from the same planes, the EXISTING traceDevice(any_hit=True) says which of them are
occluded, and NumPy reduces them.  The scratch is exactly pt_shadow_layout's bytes between guard words (its content is not specified: slots
are handed out by atomics).  Frames are 64 x 40 and smaller, but for the four views of scene_kit.RECTS (131 x 61)."""
import ctypes as C

import numpy as np
import pytest
import torch

import shadow_ref as S
from gpu_kit import bits3 as _bits
from gpu_kit import filled, pixel_mask
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from gpu_kit import words_differ as _differ
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from scene_kit import RECTS, VIEW_H, VIEW_W

pytestmark = pytest.mark.gpu

f32 = np.float32
u32 = np.uint32
W, H = 64, 40
GUARD = 4  # sentinel words on either side of the scratch (16 bytes: the scratch stays 16-byte aligned)
SENTINEL = S.SENTINEL
CAM = scenes.TWO_BOX_CAMERA
BEHIND = dict(CAM, eye=(3.0, 2.5, 5.0))
PLANES = S.PLANES
WALL = [(-3.0, 0.0, 0.6), (3.0, 0.0, 0.6), (3.0, 3.0, 0.6), (-3.0, 3.0, 0.6)]
# a light is (dir, spread, radiance, rays): a high sun, a low side light, one through the free-standing wall, one from below the ground
SUN = ((0.3, 1.0, 0.2), 0.05, (3.0, 2.5, 2.0))
SIDE = ((-1.0, 0.4, 0.1), 0.3, (0.2, 0.3, 0.5))
BACK = ((0.2, 0.5, 1.0), 0.01, (1.0, 0.0, 0.25))
BELOW = ((0.1, -1.0, 0.3), 1.0, (0.5, 0.5, 0.5))


def _lights(*rays):
    return [(d, s, c, n) for (d, s, c), n in zip((SUN, SIDE, BACK, BELOW), rays)]


PRM = dict(lights=_lights(2, 3), max_distance=1e16, bias=1e-3)


def _scene():
    """the unit box on its ground slab, and one free-standing quad 0.1 behind the box: a surface seen from both sides, with the box on one"""
    m = scenes.two_box_scene(False)
    m.meshes.append(scenes._quads_to_mesh([WALL], scenes.Material(color=(0.7, 0.7, 0.7))))
    return m


def _all(h=H, w=W):
    return np.ones((h, w), bool)


def _scratch(nbytes):
    n = nbytes // 4
    buf = torch.full((4 * (n + 2 * GUARD),), 0xA5, dtype=torch.uint8, device="cuda:0").view(torch.int32)
    t = buf[GUARD:GUARD + n].view(torch.float32)
    assert t.is_contiguous() and t.data_ptr() % 16 == 0
    return buf, t


def _gbuffer(r, mask=None):
    g = r.renderGBuffer(planes=("hit", "position"), mask=mask)
    return _np(g["hit"]), _np(g["position"])


def _cams(r, views=None):
    """the (nv, 12) rows of the context's cameras: the views' own, or the one of setCamera"""
    if views:
        return R._camera_rows([v[4] for v in views])
    return R._camera_rows([r._test_camera])


def _expect(r, hit, pos, pixels, rects=None, cams=None, max_rays_in_flight=0, view_ray=None, **prm):
    """the reference: shadow_ref's rays through the existing any-hit query of the same context, reduced in NumPy"""
    prm = dict(PRM, **prm)
    Rr = S.rays_of(hit, pos, cams if cams is not None else _cams(r), rects, pixels, prm["lights"], prm["max_distance"], prm["bias"], prm.get("seed", 0),
                   prm.get("jitter", False), view_ray=view_ray)
    if len(Rr["rays"]):
        occ = _np(r.traceDevice(torch.from_numpy(Rr["rays"]).to("cuda:0"), any_hit=True))
        assert np.array_equal(occ == -2, ~Rr["valid"]), "the reference's validity rule is not pt_trace_device's"
    else:
        occ = np.zeros(0, np.int32)
    return S.reduce(occ == 1, Rr, prm["lights"], pixels, max_rays_in_flight), Rr


def _shadow(r, hit, pos, pixels, what, rects=None, cams=None, mask=None, offset=False, planes=PLANES, ref=None, view_ray=None, **prm):
    """shadowPlanes into sentinel-filled planes and a guarded scratch of exactly pt_shadow_layout's bytes, against the reference: the layout,
    both planes over the whole frame, the nine counters; the inputs are unchanged afterwards.  Returns the reference."""
    prm = dict(PRM, **prm)
    h, w = pixels.shape
    M = prm.get("max_rays_in_flight", 0)
    nbytes = r.shadowLayout(prm["lights"], M)
    assert nbytes == S.layout(h, w, prm["lights"], M), f"{what}: the layout is {nbytes} bytes, the reference {S.layout(h, w, prm['lights'], M)}"
    if ref is None:
        ref, _ = _expect(r, hit, pos, pixels, rects, cams, view_ray=view_ray, **prm)
    hdev, pdev = _upload(hit, offset), _upload(pos, offset)
    vdev = _upload(view_ray, offset) if view_ray is not None else None
    outs = {n: filled((h, w, 4), offset) for n in planes}
    sbuf, scratch = _scratch(nbytes)
    res = r.shadowPlanes(hdev, pdev, view_ray=vdev, scratch=scratch, mask=mask, **outs, **prm)
    st = res["stats"]
    print(f"{what}: {({k: st[k] for k in S.COUNTERS})}, {st['kernel_ms']:.4f} ms, trace {st['trace_ms']:.4f} ms")
    for n in PLANES:
        if n not in planes:
            assert res[n] is None
            continue
        assert res[n] is outs[n]
        got = _bits(outs[n])
        neq = _differ(got, ref[n])
        assert not neq.any(), f"{what}: {n} differs in {int(neq.sum())} words, first at {np.argwhere(neq)[:3].tolist()}"
    words = _np(sbuf).view(u32)
    assert (words[:GUARD] == SENTINEL).all() and (words[-GUARD:] == SENTINEL).all(), f"{what}: a word outside the scratch was written"
    assert {k: st[k] for k in S.COUNTERS} == {k: ref[k] for k in S.COUNTERS}, (what, st, {k: ref[k] for k in S.COUNTERS})
    assert st["pixels"] == st["traced"] + st["skipped"] + st["nonfinite"] and st["trace_ms"] <= st["kernel_ms"]
    assert np.array_equal(_np(hdev).view(u32), np.ascontiguousarray(hit, f32).view(u32)), f"{what}: hit was written"
    assert np.array_equal(_np(pdev).view(u32), np.ascontiguousarray(pos, f32).view(u32)), f"{what}: position was written"
    if vdev is not None:
        assert np.array_equal(_np(vdev).view(u32), np.ascontiguousarray(view_ray, f32).view(u32)), f"{what}: view_ray was written"
    return ref


def _make(size, cam=CAM, partition=None, model=None):
    r = _renderer(model or _scene(), size, cam, partition=partition)
    r._test_camera = R.make_camera(cam, size[0] / size[1])
    return r


_CASES = {}


def _frame():
    """a W x H renderer on the scene and its G-buffer's two planes, shared by the tests that only read them"""
    if "frame" not in _CASES:
        r = _make((W, H))
        hit, pos = _gbuffer(r)
        for a in (hit, pos):
            a.setflags(write=False)
        _CASES["frame"] = (r, hit, pos)
    return _CASES["frame"]


def _as(ref, name):
    return ref[name].view(f32)


# ------------------------------------------------------------------ 1. light sets, jitter, outputs
@pytest.mark.parametrize("jitter", [dict(), dict(jitter=True, seed=1), dict(jitter=True, seed=0xFFFFFFFF)], ids=["fixed", "seed1", "seedmax"])
@pytest.mark.parametrize("rays", [(1,), (1, 3, 8, 16), (8, 8, 8, 8), (5,), (2, 30)], ids=lambda t: "+".join(map(str, t)))
def test_light_sets_and_jitter(ptlib, rays, jitter):
    r, hit, pos = _frame()
    lights = _lights(*rays)
    ref = _shadow(r, hit, pos, _all(), f"rays {rays}, {jitter}", lights=lights, **jitter)
    assert ref["traced"] > 0 and ref["skipped"] > 0 and 0 < ref["occluded"] < ref["rays"] and ref["invalid"] == 0
    v = _as(ref, "visibility")
    assert (v[..., len(rays):][ref["visibility"][..., len(rays):] != SENTINEL] == 1).all()
    for i, n in enumerate(rays):
        vi = v[..., i][ref["visibility"][..., i] != SENTINEL]
        assert ((vi * f32(n)) == np.round(vi * f32(n))).all() and vi.min() >= 0 and vi.max() <= 1
    if len(rays) > 1:
        assert 0 < ref["backfacing"] < ref["traced"] * len(rays)
    if jitter and len(rays) > 1:  # (the side light is wide and has three rays or more)
        other, _ = _expect(r, hit, pos, _all(), lights=lights, **dict(jitter, seed=2))
        assert _differ(other["visibility"], ref["visibility"]).any()


@pytest.mark.parametrize("planes", [("visibility",), ("light",)], ids="+".join)
def test_each_output_alone(ptlib, planes):
    r, hit, pos = _frame()
    _shadow(r, hit, pos, _all(), f"only {planes}", planes=planes, lights=_lights(5, 1, 2), jitter=True, seed=7)


def test_the_facade_allocates_light_and_scratch(ptlib):
    r, hit, pos = _frame()
    ref, _ = _expect(r, hit, pos, _all())
    res = r.shadowPlanes(_upload(hit), _upload(pos), **PRM)
    assert res["visibility"] is None and not _differ(_bits(res["light"]), ref["light"]).any()
    assert res["scratch"].numel() * 4 == S.layout(H, W, PRM["lights"])
    as_dicts = [dict(dir=d, spread=s, radiance=c, rays=n) for d, s, c, n in PRM["lights"]]
    again = r.shadowPlanes(_upload(hit), _upload(pos), lights=as_dicts, visibility=filled((H, W, 4)))
    assert again["light"] is None and not _differ(_bits(again["visibility"]), ref["visibility"]).any()


# ------------------------------------------------------------------ 2. the per-light compaction
def _walls(h=H, w=W):
    """hand-made planes over the scene's tree: points around the box whose normals alternate, pixel by pixel, between +x, +z and +y, seen
    from far along (1, 1, 1) (FAR) so that no normal is turned.  Returns hit and position."""
    ys, xs = np.mgrid[0:h, 0:w]
    P = np.zeros((h, w, 4), f32)
    P[..., 0] = (-2.0 + 4.0 * xs / max(w - 1, 1)).astype(f32)
    P[..., 1] = (0.05 + 1.0 * ys / max(h - 1, 1)).astype(f32)
    P[..., 2] = (-0.4 + 0.05 * ((xs * 7 + ys * 3) % 40)).astype(f32)  # (in front of the free-standing wall at z = 0.6 and behind it)
    P[..., 3] = 1.0
    eye = np.array([50.0, 50.0, 50.0], f32)
    hit = np.zeros((h, w, 8), f32)
    hit[..., 0] = np.sqrt(((P[..., 0:3] - eye) ** 2).sum(-1)).astype(f32)
    normals = np.array([(1, 0, 0), (0, 0, 1), (0, 1, 0)], f32)
    hit[..., 5:8] = normals[(xs + 2 * ys) % 3]
    return hit, P


FAR = dict(eye=(50.0, 50.0, 50.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovY=10.0)


def _far():
    """a W x H renderer on the scene whose eye is _walls's: facing is judged from the context's camera, not from the planes"""
    if "far" not in _CASES:
        _CASES["far"] = _make((W, H), cam=FAR)
        assert np.array_equal(_cams(_CASES["far"])[0, 0:3], np.array([50, 50, 50], f32))
    return _CASES["far"]


# +x lies exactly in the planes of the +z and +y walls (c == 0: no ray); the second faces +z and +y; the third all three; the last none
WALL_LIGHTS = [((1.0, 0.0, 0.0), 0.1, (1.0, 0.5, 0.25), 3), ((0.0, 0.6, 0.8), 0.2, (0.25, 1.0, 0.5), 2), ((1.0, 1.0, 1.0), 0.05, (0.5, 0.25, 1.0), 5),
               ((-1.0, -1.0, -1.0), 0.3, (9.0, 9.0, 9.0), 4)]


def test_neighbouring_pixels_face_different_lights(ptlib):
    r = _far()
    hit, pos = _walls()
    ref, Rr = _expect(r, hit, pos, _all(), lights=WALL_LIGHTS, max_distance=10.0)
    shoots = Rr["first"] >= 0
    assert np.array_equal(Rr["lights"]["L"][0], np.array([1, 0, 0], f32)), "the first light normalises to the axis exactly"
    kind = ((np.mgrid[0:H, 0:W][1] + 2 * np.mgrid[0:H, 0:W][0]) % 3).reshape(-1)
    assert (shoots[kind == 0] == [True, False, True, False]).all() and (shoots[kind == 1] == [False, True, True, False]).all()
    assert (shoots[kind == 2] == [False, True, True, False]).all() and (Rr["c"][kind != 0, 0] == 0).all(), "c == 0 shoots no ray"
    assert ref["backfacing"] == int((~shoots).sum()) and 0 < ref["occluded"] < ref["rays"] == int((shoots * Rr["lights"]["rays"]).sum())
    v = _as(ref, "visibility").reshape(-1, 4)
    for i in range(3):  # every light that shoots is seen from some pixels and hidden from others: a mixed-up slot would show
        assert (v[shoots[:, i], i] > 0).any() and (v[shoots[:, i], i] < 1).any(), i
        assert (v[~shoots[:, i], i] == 0).all()
    _shadow(r, hit, pos, _all(), "two walls and a floor under four lights", ref=ref, lights=WALL_LIGHTS, max_distance=10.0)
    for M in (14 * 100, 14 * 1025):  # a batch boundary inside a wave and one pixel behind a workgroup
        _shadow(r, hit, pos, _all(), f"the walls, {M} rays in flight", ref=dict(ref, batches=S.batches_of(W * H, H, W, WALL_LIGHTS, M)),
                lights=WALL_LIGHTS, max_distance=10.0, max_rays_in_flight=M)
    # jittered: each light hashes its own seed
    _shadow(r, hit, pos, _all(), "the walls, jittered", lights=WALL_LIGHTS, max_distance=10.0, jitter=True, seed=0xFFFFFFFE)


def test_a_light_under_every_horizon_and_a_lone_last_pixel(ptlib):
    r = _far()
    hit, pos = _walls()
    hit = hit.copy()
    hit[..., 5:8] = (0.0, 1.0, 0.0)
    down = [((0.0, -1.0, 0.0), 0.2, (1.0, 1.0, 1.0), 4), ((1.0, -1.0, 0.0), 0.0, (1.0, 2.0, 3.0), 3)]
    ref = _shadow(r, hit, pos, _all(), "every light under every horizon", lights=down, max_distance=10.0)
    assert ref["rays"] == 0 and ref["backfacing"] == 2 * W * H and (_as(ref, "light") == np.array([0, 0, 0, 1], f32)).all()
    assert (_as(ref, "visibility") == np.array([0, 0, 1, 1], f32)).all()
    hit[H - 1, W - 1, 5:8] = (1.0, 0.0, 0.0)  # the last pixel of the list alone faces the second light
    ref = _shadow(r, hit, pos, _all(), "only the last pixel shoots", lights=down, max_distance=10.0)
    assert ref["rays"] == 3 and ref["backfacing"] == 2 * W * H - 1
    ref = _shadow(r, hit, pos, _all(), "only the last pixel shoots, 7 rays in flight", lights=down, max_distance=10.0, max_rays_in_flight=7)
    assert ref["rays"] == 3 and ref["batches"] == W * H
    miss = hit.copy()
    miss[..., 3] = np.array([-1], np.int32).view(f32)[0]
    miss[H - 1, W - 1, 3] = 0.0
    ref = _shadow(r, miss, pos, _all(), "every pixel but the last is a miss", lights=down, max_distance=10.0)
    assert ref["skipped"] == W * H - 1 and ref["traced"] == 1 and ref["rays"] == 3 and ref["backfacing"] == 1


# ------------------------------------------------------------------ 3. batches
def test_one_pixel_per_batch(ptlib):
    w, h = 16, 8
    r = _make((w, h))
    hit, pos = _gbuffer(r)
    lights = _lights(1, 3, 1)
    ref = _shadow(r, hit, pos, _all(h, w), "16 x 8, max_rays_in_flight = R", lights=lights, max_rays_in_flight=5, jitter=True, seed=3)
    assert ref["batches"] == w * h
    whole = _shadow(r, hit, pos, _all(h, w), "16 x 8, the default", lights=lights, jitter=True, seed=3)
    assert whole["batches"] == 1 and all(np.array_equal(whole[n], ref[n]) for n in PLANES)
    r.close()


@pytest.mark.parametrize("M", [5 * 1023, 5 * 1024, 5 * 1025, 5 * 2559, 5 * 2560, 1 << 30])
def test_the_result_does_not_depend_on_the_batch(ptlib, M):
    """one pixel short of a workgroup of k_shadow_rays (1024 pixels), on it and one pixel behind it, one pixel short of the frame, the
    frame, more than it"""
    r, hit, pos = _frame()
    if "default" not in _CASES:
        _CASES["default"] = _expect(r, hit, pos, _all(), jitter=True, seed=5)[0]
    base = _CASES["default"]
    ref = dict(base, batches=S.batches_of(W * H, H, W, PRM["lights"], M))
    _shadow(r, hit, pos, _all(), f"max_rays_in_flight {M}", ref=ref, jitter=True, seed=5, max_rays_in_flight=M)
    assert ref["batches"] == -(-W * H // min(M // 5, W * H))


def test_the_layout_grows_with_the_batch_and_stops_at_the_frame(ptlib):
    r, _, _ = _frame()
    L5 = PRM["lights"]
    sizes = [r.shadowLayout(L5, M) for M in (5, 10, 500, 5 * W * H - 5, 5 * W * H, 5 * W * H + 5, 1 << 31, 0)]
    assert sizes[:5] == sorted(set(sizes[:5])) and sizes[4] == sizes[5] == sizes[6] == sizes[7] == 256 + W * H * 232
    assert sizes[0] == (256 + 232 + 15) // 16 * 16 and r.shadowLayout(_lights(8, 8, 8, 8), 32) == 256 + 40 * 32 + 32 == S.layout(H, W, _lights(8, 8, 8, 8), 32)
    assert r.shadowLayout(_lights(1), 1) == (256 + 72 + 15) // 16 * 16


# ------------------------------------------------------------------ 4. sizes, alignment, masks
@pytest.mark.parametrize("size", [(1, 1), (13, 7), (33, 9), (63, 5)])
def test_sizes(ptlib, size):
    w, h = size
    r = _make(size)
    hit, pos = _gbuffer(r)
    _shadow(r, hit, pos, _all(h, w), f"{w} x {h}", lights=_lights(2, 1, 3, 2), jitter=True, seed=w)
    _shadow(r, hit, pos, _all(h, w), f"{w} x {h}, 11 rays in flight", max_rays_in_flight=11)
    r.close()


def test_every_plane_one_float_into_its_allocation(ptlib):
    r, hit, pos = _frame()
    _shadow(r, hit, pos, _all(), "every plane 4 bytes off a 16-byte boundary", offset=True, lights=_lights(5, 2))


def test_block_masks(ptlib):
    r, hit, pos = _frame()
    nby, nbx = r.blockGrid()
    rng = np.random.default_rng(4)
    for name, m in (("random", rng.random((nby, nbx)) < 0.4), ("one block", np.arange(nby * nbx).reshape(nby, nbx) == 17), ("empty", np.zeros((nby, nbx), bool))):
        ref = _shadow(r, hit, pos, pixel_mask(m, h=H, w=W), f"mask: {name}", mask=m, max_rays_in_flight=5 * 100)
        assert ref["pixels"] == int(m.sum()) * 64
        if name == "empty":
            assert ref["batches"] == 0 and (ref["light"] == SENTINEL).all()


# ------------------------------------------------------------------ 5. views and partitions
def test_two_sides_of_a_wall_in_four_views(ptlib):
    """RECTS with two cameras in front of the free-standing quad and two behind it: pixels in no view are untouched, and the normal is
    turned to each view's own eye — with the cameras of the other side the reference gives another plane"""
    w, h = VIEW_W, VIEW_H
    r = _make((w, h))
    dicts = [CAM, BEHIND, dict(CAM, eye=(2.5, 2.0, -4.5)), dict(BEHIND, fovY=55.0)]
    views = [(x, y, ww, hh, R.make_camera(c, ww / hh)) for (x, y, ww, hh), c in zip(RECTS, dicts)]
    r.setViews(views)
    inside = np.zeros((h, w), bool)
    for x, y, ww, hh in RECTS:
        inside[y:y + hh, x:x + ww] = True
    hit, pos = _gbuffer(r)
    cams = _cams(r, views)
    lights = _lights(2, 1, 2)
    ref = _shadow(r, hit, pos, inside, "four views", rects=RECTS, cams=cams, lights=lights, jitter=True, seed=2)
    assert ref["pixels"] == int(inside.sum()) and (ref["light"][~inside] == SENTINEL).all() and ref["occluded"] > 0
    wrong, _ = _expect(r, hit, pos, inside, rects=RECTS, cams=cams[[1, 0, 3, 2]], lights=lights, jitter=True, seed=2)
    assert _differ(wrong["visibility"], ref["visibility"]).any(), "the scene cannot tell one view's eye from another's"
    m = np.random.default_rng(8).random(r.blockGrid()) < 0.5
    _shadow(r, hit, pos, inside & pixel_mask(m, h=h, w=w), "four views under a mask", rects=RECTS, cams=cams, mask=m, max_rays_in_flight=5 * 333)
    r.close()


def test_partitions_add_up(ptlib):
    r, hit, pos = _frame()
    whole, _ = _expect(r, hit, pos, _all())
    by, bx = np.mgrid[0:H, 0:W] // 8
    union = {n: np.full(whole[n].shape, SENTINEL, u32) for n in PLANES}
    model = _scene()
    for rank in range(2):
        rr = _make((W, H), partition=(rank, 2, 8, 8), model=model)
        own = (bx + by) % 2 == rank
        part = _shadow(rr, hit, pos, own, f"rank {rank} of 2")
        assert part["pixels"] == int(own.sum())
        for n in PLANES:
            assert (union[n][own] == SENTINEL).all()
            union[n][own] = part[n][own]
        rr.close()
    for n in PLANES:
        assert not _differ(union[n], whole[n]).any(), n


# ------------------------------------------------------------------ 6. misses, hostile records, parameters
def test_misses_hostile_records_and_an_invalid_ray(ptlib):
    r, hit, pos = _frame()
    hit, pos = hit.copy(), pos.copy()
    hits = np.argwhere(hit[..., 3].view(np.int32) >= 0)
    assert len(hits) > 64 and (hit[..., 3].view(np.int32) < 0).any()
    pick = hits[np.random.default_rng(6).permutation(len(hits))[:14]]
    taken = {(int(y), int(x)) for y, x in pick}
    faces_up = [(y, x) for y, x in np.argwhere((hit[..., 3].view(np.int32) >= 0) & (hit[..., 6] > 0.9)) if (int(y), int(x)) not in taken]
    pick = np.concatenate([pick, np.array(faces_up[len(faces_up) // 2:len(faces_up) // 2 + 1])])  # (the sun stands above this one's horizon)
    nan, inf = f32(np.nan), f32(np.inf)
    edits = [("hit", 5, nan), ("hit", 6, inf), ("hit", 7, -inf), ("hit", 0, nan), ("hit", 0, inf), ("hit", 0, f32(0.0)), ("hit", 0, f32(-0.0)), ("hit", 0, f32(-2.0)),
             ("pos", 0, nan), ("pos", 1, -inf), ("pos", 2, inf)]
    for (y, x), (plane, word, value) in zip(pick, edits):
        (hit if plane == "hit" else pos)[y, x, word] = value
    for (y, x), prim in zip(pick[11:14], (0x7FFFFFFF, 12345678, 36)):  # stale primitives: no address is formed from them
        hit[y, x, 3] = np.array([prim], np.int32).view(f32)[0]
    clean, _ = _expect(r, _frame()[1], _frame()[2], _all(), bias=4.0)
    y, x = pick[14]
    hit[y, x, 0] = f32(1e38)  # bias * t overflows: the origin is not finite, every ray of the pixel is invalid
    ref = _shadow(r, hit, pos, _all(), "hostile records", bias=4.0)
    assert ref["nonfinite"] == 11 and ref["skipped"] == clean["skipped"] > 0 and ref["traced"] == clean["traced"] - 11
    assert 0 < ref["invalid"] <= 5 and _as(ref, "visibility")[y, x].min() >= 0 and set(_as(ref, "visibility")[y, x].tolist()) <= {0.0, 1.0}
    one = f32(1).view(u32)
    for yy, xx in pick[:11]:
        assert (ref["visibility"][yy, xx] == one).all() and tuple(ref["light"][yy, xx]) == (0, 0, 0, one)
    for yy, xx in pick[11:14]:
        assert np.array_equal(ref["light"][yy, xx], clean["light"][yy, xx])
    miss = hit[..., 3].view(np.int32) < 0
    assert (ref["visibility"][miss] == one).all() and (ref["light"][miss] == (0, 0, 0, one)).all()


@pytest.mark.parametrize("prm", [dict(bias=0.0), dict(bias=0.05), dict(max_distance=1e-6), dict(max_distance=2.0), dict(max_distance=1e30)],
                         ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()))
def test_bias_and_max_distance(ptlib, prm):
    r, hit, pos = _frame()
    ref = _shadow(r, hit, pos, _all(), f"{prm}", **prm)
    default = _expect(r, hit, pos, _all())[0]
    if prm.get("max_distance") == 1e-6:
        assert ref["occluded"] == 0 and ref["rays"] == default["rays"]
    if prm.get("max_distance") == 2.0:
        assert 0 < ref["occluded"] <= default["occluded"]
    if prm.get("max_distance") == 1e30:
        assert ref["occluded"] == default["occluded"]


def test_the_pass_follows_the_current_tree(ptlib):
    """the same G-buffer before and after transformMeshes has moved the box away: both match the query over the geometry of the moment"""
    r = _make((W, H))
    hit, pos = _gbuffer(r)
    before = _shadow(r, hit, pos, _all(), "the box in place")
    r.transformMeshes({0: np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -10.0]], f32)})
    after = _shadow(r, hit, pos, _all(), "the box moved away")
    assert after["occluded"] < before["occluded"] and _differ(after["visibility"], before["visibility"]).any()
    r.close()


def _quad_renderer(quads, size, camera):
    model = scenes.Model([scenes._quads_to_mesh([q], scenes.Material()) for q in quads])
    r = R.SampleRenderer(model)
    r.resize(size)
    r.setCamera(camera)
    r._test_camera = camera
    return r


@pytest.mark.parametrize("light", ["up", "down"])
def test_the_analytic_scenes_on_the_gpus_tree(ptlib, light):
    """tests/test_shadow_cabi.py's floor and lid: under a light straight up the lid's shadow is exact, under one straight down no ray is built"""
    hit, pos, cam = S.analytic_planes()
    h, w = hit.shape[:2]
    camera = R.Camera(S.ANALYTIC_EYE, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 35.0, w / h)
    assert np.array_equal(R._camera_rows([camera])[0, 0:3], cam[0, 0:3])
    r = _quad_renderer(S.analytic_quads(True), (w, h), camera)
    under, undecided = S.under_the_lid(pos)
    assert undecided.sum() == 0
    if light == "up":
        up = [((0.0, 1.0, 0.0), 0.0, (2.0, 1.5, 1.0), 1)]
        ref = _shadow(r, hit, pos, _all(h, w), "analytic, the light straight up", cams=cam, lights=up, max_distance=10.0)
        v = _as(ref, "visibility")[..., 0]
        assert (v[under] == 0).all() and (v[~under] == 1).all() and ref["occluded"] == int(under.sum()) and ref["backfacing"] == 0
        assert (_as(ref, "light")[~under] == np.array([2.0, 1.5, 1.0, 1.0], f32)).all()
    else:
        down = [((0.0, -1.0, 0.0), 0.0, (2.0, 1.5, 1.0), 3)]
        ref = _shadow(r, hit, pos, _all(h, w), "analytic, the light straight down", lights=down, max_distance=10.0)
        assert ref["backfacing"] == h * w and ref["rays"] == 0 and (_as(ref, "light") == np.array([0, 0, 0, 1], f32)).all()
    r.close()


# ------------------------------------------------------------------ 7. view_ray: the reflected surface
def test_view_ray_turns_the_normal_to_the_mirror_rays_origin(ptlib):
    """a floor under a lid at y = 1, seen from above the lid's plane through the gap under its edge: the mirror rays of the floor hit the
    lid's underside.  Judged from the eye (above the lid) that surface faces up, judged from the mirror ray's origin it faces down; a light
    from below reaches it only then"""
    floor = [(-8, 0, -8), (-8, 0, 8), (8, 0, 8), (8, 0, -8)]
    lid = [(-3, 1, -3), (-3, 1, 3), (3, 1, 3), (3, 1, -3)]
    w, h = 48, 24
    cam = dict(eye=(0.0, 1.5, -7.0), lookat=(0.0, 0.0, -2.5), up=(0.0, 1.0, 0.0), fovY=30.0)
    camera = R.make_camera(cam, w / h)
    r = _quad_renderer([floor, lid], (w, h), camera)
    hit, pos = _gbuffer(r)
    g2 = r.reflectPlanes(_upload(hit), _upload(pos), hit2=filled((h, w, 8)), position2=filled((h, w, 4)), ray=filled((h, w, 8)))
    hit2, pos2, ray = _np(g2["hit2"]), _np(g2["position2"]), _np(g2["ray"])
    on_lid = (hit2[..., 3].view(np.int32) >= 0) & (hit2[..., 4].view(np.int32) == 1)
    assert on_lid.sum() > 50 and (ray[on_lid][:, 1] < 1).all(), "some mirror rays start under the lid and hit it"
    lights = [((0.2, -1.0, 0.1), 0.1, (1.0, 2.0, 3.0), 4), ((0.0, 1.0, 0.0), 0.0, (1.0, 1.0, 1.0), 1)]
    ref = _shadow(r, hit2, pos2, _all(h, w), "the second G-buffer under view_ray", view_ray=ray, lights=lights, max_distance=100.0, jitter=True, seed=9)
    from_eye, _ = _expect(r, hit2, pos2, _all(h, w), lights=lights, max_distance=100.0, jitter=True, seed=9)
    assert _differ(from_eye["visibility"], ref["visibility"]).any(), "the scene cannot tell the mirror ray's origin from the eye"
    v, ve = _as(ref, "visibility"), _as(from_eye, "visibility")
    assert (v[on_lid][:, 1] == 0).all(), "judged from the mirror ray's origin, the light straight up is behind the lid's underside"
    assert (ve[on_lid][:, 1] == 1).all() and (ve[on_lid][:, 0] == 0).all(), "judged from the eye the lid faces up: lit from above, not from below"
    assert (v[on_lid][:, 0] == 0).all() and ref["rays"] > 0 and ref["occluded"] >= 4 * int(on_lid.sum()), "the rays from below are shot, and meet the floor"


def test_a_view_ray_without_a_finite_origin_shoots_no_ray(ptlib):
    r, hit, pos = _frame()
    ray = np.zeros((H, W, 8), f32)
    ray[..., 0:3] = CAM["eye"]
    ray[..., 3:8] = np.nan  # only the origin is read
    hits = np.argwhere(hit[..., 3].view(np.int32) >= 0)
    for (y, x), (word, value) in zip(hits[::37][:3], ((0, np.nan), (1, np.inf), (2, -np.inf))):
        ray[y, x, word] = value
    ref = _shadow(r, hit, pos, _all(), "view_ray with three hostile origins", view_ray=ray)
    plain, _ = _expect(r, hit, pos, _all())
    assert ref["nonfinite"] == 3 and ref["traced"] == plain["traced"] - 3
    one = f32(1).view(u32)
    for y, x in hits[::37][:3]:
        assert (ref["visibility"][y, x] == one).all() and tuple(ref["light"][y, x]) == (0, 0, 0, one)


# ------------------------------------------------------------------ 8. refusals
def test_refusals(ptlib):
    L = _lib.load_library()
    r = R.SampleRenderer(_scene())
    _, hit, pos = _frame()
    hdev, pdev = _upload(hit), _upload(pos)
    outs = {n: filled((H, W, 4)) for n in PLANES}
    two = _lights(1, 1)  # (a small scratch: a pointer into another plane's allocation must still have its bytes behind it)
    prm = dict(PRM, lights=two)
    nbytes = S.layout(H, W, two)
    sbuf, scratch = _scratch(nbytes)
    good = dict(hit=hdev.data_ptr(), position=pdev.data_ptr(), view_ray=None, visibility=outs["visibility"].data_ptr(), light=outs["light"].data_ptr(),
                scratch=scratch.data_ptr(), num_lights=2, max_rays_in_flight=0, max_distance=1e16, bias=1e-3, seed=0, flags=0)
    sevens = (7, 7, 7, 7, 7, 7, 7, 7, 7, 7.0, 7.0)

    def raw(lights):
        """a ctypes array without the facade's checks"""
        arr = (_lib.ShadowLight * len(lights))()
        for a, (d, s, c, n) in zip(arr, lights):
            a.dir[:], a.spread, a.radiance[:], a.rays = d, s, c, n
        return arr

    def untouched(what):
        assert (_np(sbuf).view(u32) == SENTINEL).all(), f"{what}: the scratch was written"
        for n in PLANES:
            assert (_bits(outs[n]) == SENTINEL).all(), f"{what}: {n} was written"

    def refused(what, pattern, lights=two, **fields):
        d = _lib.ShadowDesc()
        arr = raw(lights) if lights is not None else None
        for n, v in dict(good, **fields).items():
            setattr(d, n, v)
        d.lights = C.addressof(arr) if arr is not None else None
        torch.cuda.synchronize()
        s = _lib.ShadowStats(*sevens)
        rc = L.pt_shadow_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_shadow_planes") and pattern in msg, f"{what}: {msg!r}"
        assert tuple(getattr(s, n) for n, _ in s._fields_) == sevens
        untouched(what)

    def layout_refused(what, pattern, lights=two, M=0, with_bytes=True, count=None):
        nb = C.c_size_t(77)
        arr = raw(lights) if lights is not None else None
        rc = L.pt_shadow_layout(r._ctx, arr, len(lights) if count is None else count, M, C.byref(nb) if with_bytes else None)
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1 and msg.startswith("pt_shadow_layout") and pattern in msg, f"{what}: {rc}, {msg!r}"
        assert nb.value == 77, f"{what}: bytes was written"

    def light(**edit):
        d = dict(dir=SUN[0], spread=SUN[1], radiance=SUN[2], rays=2)
        d.update(edit)
        return (d["dir"], d["spread"], d["radiance"], d["rays"])

    refused("no resize yet", "pt_resize")
    layout_refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(CAM, W / H))
    layout_refused("bytes null", "bytes is null", with_bytes=False)
    assert L.pt_shadow_planes(r._ctx, None, None) == -1 and "pt_shadow_planes: null description" in L.pt_last_error(r._ctx).decode()
    refused("an unknown flag", "unknown flag bits 2", flags=3)
    refused("an unknown flag", "unknown flag bits 2147483648", flags=0x80000000)
    for bad in (0, 5, 0xFFFFFFFF):
        refused(f"num_lights {bad}", f"num_lights must be 1..4, not {bad}", num_lights=bad)
        layout_refused(f"num_lights {bad}", f"num_lights must be 1..4, not {bad}", count=bad)
    refused("lights null", "lights is null", lights=None)
    layout_refused("lights null", "lights is null", lights=None, count=2)
    refused("a light without rays", "light 1: rays must be >= 1", lights=[light(), light(rays=0)])
    layout_refused("a light without rays", "light 1: rays must be >= 1", lights=[light(), light(rays=0)])
    refused("33 rays", "the lights' rays add up to 33, above 32", lights=[light(rays=30), light(rays=3)])
    layout_refused("33 rays", "the lights' rays add up to 33, above 32", lights=[light(rays=30), light(rays=3)])
    refused("rays that wrap in 32 bits", "above 32", lights=[light(rays=0xFFFFFFFF), light(rays=2)])
    refused("fewer rays in flight than rays", "max_rays_in_flight is 1, below the lights' rays (2)", max_rays_in_flight=1)
    layout_refused("fewer rays in flight than rays", "max_rays_in_flight is 1, below the lights' rays (2)", M=1)
    for bad in ((float("nan"), 1.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 1.0, -float("inf"))):
        refused(f"dir {bad}", "light 0: dir is not finite", lights=[light(dir=bad), light()])
    for bad in ((0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (1e-30, 0.0, 0.0), (3e38, 3e38, 0.0)):  # no length, one that underflows, one that overflows
        refused(f"dir {bad}", "light 1: dir cannot be normalised", lights=[light(), light(dir=bad)])
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf")):
        refused(f"spread {bad}", "light 0: spread must be finite and in [0, 1]", lights=[light(spread=bad), light()])
    for bad in ((-1e-9, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, float("inf"))):
        refused(f"radiance {bad}", "light 1: radiance must be finite and >= 0", lights=[light(), light(radiance=bad)])
    for bad in (0.0, -0.0, -1.0, float("nan"), float("inf")):
        refused(f"max_distance {bad}", "max_distance must be finite and > 0", max_distance=bad)
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf")):
        refused(f"bias {bad}", "bias must be finite and >= 0", bias=bad)
    for name in ("hit", "position", "scratch"):
        refused(f"{name} null", f"{name} is null", **{name: None})
    refused("no output", "no output asked for", visibility=None, light=None)
    host = np.zeros((H, W, 8), f32)
    refused("a host pointer", "hit is not device memory", hit=host.ctypes.data)
    refused("a host view_ray", "view_ray is not device memory", view_ray=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "light is not 4-byte aligned", light=good["light"] + 2)
    for off in (4, 8, 2):
        refused(f"the scratch {off} bytes off", "scratch is not 16-byte aligned", scratch=good["scratch"] + off)
    big = torch.zeros(2 * H * W * 8 + 8, dtype=torch.float32, device="cuda:0")
    refused("light inside hit", "hit and light overlap", hit=big.data_ptr(), light=big.data_ptr() + 16)
    refused("visibility inside position", "position and visibility overlap", position=big.data_ptr() + 64, visibility=big.data_ptr())
    refused("visibility inside view_ray", "view_ray and visibility overlap", view_ray=big.data_ptr(), visibility=big.data_ptr() + 32)
    refused("visibility exactly light", "visibility and light overlap", visibility=good["light"])
    refused("the scratch inside hit", "hit and scratch overlap", scratch=good["hit"] + 16)
    refused("the scratch inside light", "light and scratch overlap", scratch=good["light"] + 32)
    hip = _hip_runtime()
    for name, nb in (("scratch", nbytes), ("light", H * W * 16)):
        rawp, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert hip.hipMalloc(C.byref(rawp), C.c_size_t(nb)) == 0
        try:
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), rawp) == 0 and base.value == rawp.value and size.value >= nb
            refused(f"{name} one element too small", f"{name} has fewer than {nb} bytes left", **{name: rawp.value + size.value - (nb - 16)})
        finally:
            assert hip.hipFree(rawp) == 0
    # the Python facade passes the library's refusals on; a valid call afterwards works, into the same arrays
    with pytest.raises(RuntimeError, match="visibility and light overlap"):
        r.shadowPlanes(hdev, pdev, visibility=outs["light"], light=outs["light"], **prm)
    with pytest.raises(RuntimeError, match="light 0: dir cannot be normalised"):
        r.shadowPlanes(hdev, pdev, lights=[((0, 0, 0), 0.0, (1, 1, 1), 1)], light=outs["light"])
    with pytest.raises(ValueError, match=r"scratch: a contiguous torch.float32 tensor of shape \(%d,\) is expected" % (nbytes // 4)):
        r.shadowPlanes(hdev, pdev, scratch=torch.zeros((nbytes // 4 + 4,), device="cuda:0"), **prm)
    untouched("the facade's refusals")
    r._test_camera = R.make_camera(CAM, W / H)
    ref, _ = _expect(r, hit, pos, _all(), lights=two)
    res = r.shadowPlanes(hdev, pdev, scratch=scratch, **outs, **prm)
    for n in PLANES:
        assert not _differ(_bits(outs[n]), ref[n]).any(), n
    assert {k: res["stats"][k] for k in S.COUNTERS} == {k: ref[k] for k in S.COUNTERS}
    r.close()


# ------------------------------------------------------------------ 9. state and ordering
def test_queued_queries_and_rendering_state(ptlib):
    """asynchronous queries queued in front of the call are completed by it, and queryWait still delivers their counts; stats() and the
    frame buffers are what they were"""
    r = _make((W, H))
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.launchParams.samples_per_launch = 1
    r.render()
    hit, pos = _gbuffer(r)
    ref, Rr = _expect(r, hit, pos, _all())
    r.queryWait()
    rays = torch.from_numpy(Rr["rays"]).to("cuda:0")
    queued = [r.traceDevice(rays, any_hit=True, wait=False) for _ in range(2)]
    before, frame = r.stats(), r.download(R.PT_BUF_ACCUM)
    res = r.shadowPlanes(_upload(hit), _upload(pos), light=filled((H, W, 4)), **PRM)
    assert r.stats() == before and r.download(R.PT_BUF_ACCUM).tobytes() == frame.tobytes()
    assert not _differ(_bits(res["light"]), ref["light"]).any()
    q = r.queryWait()
    assert q["rays"] == 2 * len(Rr["rays"]) and q["hits"] == 2 * ref["occluded"] and q["invalid_rays"] == 0
    for t in queued:
        assert np.array_equal(_np(t) == 1, _np(queued[0]) == 1) and int((_np(t) == 1).sum()) == ref["occluded"]
    assert r.queryWait()["rays"] == 0
    r.close()


@pytest.mark.parametrize("mode", ["default", "side"])
def test_under_a_busy_torch_stream(ptlib, mode):
    """tests/test_gpu_stream_contract.py's protocol: the planes are produced, and the outputs sentinel-filled, by work still pending on
    torch's current stream when the call is made; the result equals the synchronous call's, and that equals the reference"""
    from stream_kit import _pin, _res

    r, hit, pos = _frame()
    outs = {n: filled((H, W, 4)) for n in PLANES}
    scratch = torch.zeros((r.shadowLayout(PRM["lights"]) // 4,), dtype=torch.float32, device="cuda:0")  # (not an output of the case: its slots are handed out by atomics)

    def shadows(dev, outs, returned):
        res = r.shadowPlanes(dev["hit"], dev["position"], scratch=scratch, **outs, **PRM)
        returned()
        return _res(res, outs)

    sync, got = _pin("shadowPlanes", mode, r, dict(hit=hit, position=pos), outs, shadows)
    ref, _ = _expect(r, hit, pos, _all())
    for n in PLANES:
        assert not _differ(got[n].view(u32).reshape(ref[n].shape), ref[n]).any(), f"{n} under a busy stream [{mode}]"
    assert got["stats"] == {k: ref[k] for k in S.COUNTERS}


# ------------------------------------------------------------------ 10. the light as a colour: modulatePlanes, the upsampled loop
def test_modulate_planes_multiplies_the_albedo_into_the_light(ptlib):
    import moments_ref as MR

    r, hit, pos = _frame()
    ref, _ = _expect(r, hit, pos, _all())
    light = _as(ref, "light")
    albedo = MR.random_albedo(np.random.default_rng(3), H, W)
    res = r.modulatePlanes(_upload(light), albedo=_upload(albedo), out=filled((H, W, 4)))
    with np.errstate(all="ignore"):
        want = np.concatenate([light[..., 0:3] * MR.den(albedo, 0.0, light[..., 0:3].shape), light[..., 3:4]], -1)
    assert want.dtype == f32 and not _differ(_bits(res["out"]), want.view(u32)).any()
    assert (want[..., 3] == 1).all() and want[..., 0:3].max() > 0


def _example(name):
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def test_upsampled_loop_with_sun_adds_the_direct_light(ptlib):
    """examples/upsampled_svgf_loop.py's UpsampledLoop with sun at 128 x 56, scale 2: the light is shadowPlanes of the full-size G-buffer,
    jittered by the frame index, and what is added to the frame is its product with the full-size albedo"""
    import surface_ref as SR

    ex = _example("upsampled_svgf_loop")
    w, h = 128, 56
    probe = scenes.sky_probe(256, 128).BuildCDF()
    cam0 = dict(eye=(2.0, 0.35, -3.0), lookat=(0.0, 0.2, 0.5), up=(0.0, 1.0, 0.0), fovY=35.0)
    up = ex.UpsampledLoop(SR.textured_scene(), (w, h), 2, probe=probe, sun=True, sun_rays=3, sun_spread=0.05)
    cam = R.make_camera(cam0, w / h)
    for k in range(3):
        prev, cam = cam, R.make_camera(ex.orbit(cam0, 0.02 * k), w / h)
        x = up.frame(k, prev, cam)
        assert x["pixels"] == w * h and x["sun_ms"] > 0 and x["sun_trace_ms"] > 0 and x["sun_batches"] == 1 and 0 < x["sun_occluded"] < x["sun_rays"]
    lights = [((0.4, 1.0, -0.3), 0.05, (3.0, 2.9, 2.7), 3)]
    ref, _ = _expect(up.hi, _np(up.hi_gbuf["hit"]), _np(up.hi_gbuf["position"]), _all(h, w), cams=R._camera_rows([cam]), lights=lights, jitter=True, seed=2)
    assert not _differ(_bits(up.sun_light), ref["light"]).any() and x["sun_occluded"] == ref["occluded"] and x["sun_backfacing"] == ref["backfacing"]
    lit = _np(up.sun_lit)
    assert np.isfinite(lit).all() and lit[..., 0:3].max() > 0 and (lit[..., 0:3] >= 0).all()
    assert (_np(up.final)[..., 0:3] >= lit[..., 0:3]).all(), "the product was added to a non-negative frame"
    up.close()


@pytest.mark.parametrize("flags", [["--sun"], ["--sun", "--reflect"]], ids=["sun", "sun+reflect"])
def test_upsampled_loop_runs_with_sun(ptlib, tmp_path, capsys, flags):
    ex = _example("upsampled_svgf_loop")
    ex.main(["--size", "128", "56", "--frames", "2", "--sun-rays", "2", "--sun-dir", "0.3", "1.0", "-0.2", "--sun-spread", "0.02", "--sun-radiance", "2", "2", "1.5",
             "--out-dir", str(tmp_path)] + flags)
    out = capsys.readouterr().out
    assert out.count("sun ") == 2 and "rays shadowed" in out and ("on the reflected surface" in out) == ("--reflect" in flags)
    sun = np.load(tmp_path / "upsampled_svgf_sun.npy")
    assert sun.shape == (56, 128, 4) and np.isfinite(sun).all() and (sun[..., 3] == 1).all() and sun[..., 0:3].max() > 0 and sun[..., 0:3].min() == 0
    if "--reflect" in flags:
        refl = np.load(tmp_path / "upsampled_svgf_reflection.npy")
        assert refl.shape == (56, 128, 4) and np.isfinite(refl).all() and (refl[..., 0:3] >= 0).all()
