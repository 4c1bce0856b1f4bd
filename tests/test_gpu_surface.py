"""Pixel-centre albedo from the hit plane (pt_copy_texcoords_device, pt_surface_planes) on the GPU.  Every plane is compared bit for bit, over
the WHOLE plane (a pixel written outside the chosen set shows as a lost sentinel), with tests/surface_ref.py: float32 NumPy evaluating the
header's arithmetic on the hit plane renderGBuffer gave (pinned by tests/test_gpu_gbuffer.py) and the model's own host arrays; its tex2D is
tied to the oracle's in tests/test_surface_cabi.py.  No tolerance anywhere; the hand-made plane with non-finite barycentrics compares NaN
words as NaN (payloads are not specified).

Inputs, 131 x 61 (17 x 8 blocks, last column 3 wide, last row 5 high):
  textured: surface_ref.textured_scene() — scenes.textured_scene() with the box's zero texcoords removed, so the box names a texture, has no
            texcoords and keeps its colour, as that scene's docstring says — under S.TEX_CAMERA: 7991 pixels, 1844 misses, 5055 on the texture
            path (ground 2916, wall 2139), 1092 on the colour path (the box), counted with the CPU checker before the first GPU run;
  cornell:  the untextured Cornell box under CORNELL_CAMERA: 3481 hit pixels, 2897 of them with a 3 x 3 neighbourhood on one mesh; at those
            PT_BUF_ALBEDO of a 1-spp frame equals the plane in every bit (0 mismatches; 34 of the other 584 hit pixels differ: the jittered
            sample met the neighbouring mesh), counted with the CPU checker's frame before the first GPU run."""
import ctypes as C

import numpy as np
import pytest
import torch

import surface_ref as S
import temporal_ref as T
from gpu_kit import filled, pixel_mask, plane_shape, whole_frame_mask
from gpu_kit import bits as _bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from pass_cases import _hand_made
from pass_cases import surface_case as _case
from scene_kit import RECTS, _affine, _cam_dicts

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 131, 61
SENTINEL = S.SENTINEL


# ------------------------------------------------------------------ GPU helpers
def _filled(name, h, w, offset=False):
    """a sentinel-filled plane of the pass; offset: one float into its allocation (4-byte aligned only)"""
    return filled(plane_shape(h, w, S.WORDS[name]), offset)


def _same(got, ref, what, nan_aware=False):
    for name, a in got.items():
        b = ref[name]
        neq = a != b
        if nan_aware:
            with np.errstate(all="ignore"):
                neq &= ~(np.isnan(a.view(f32)) & np.isnan(b.view(f32)))
        assert a.shape == b.shape and not neq.any(), f"{what}: {name} differs from float32 NumPy in {int(neq.sum())} words"


def _run(r, sc, hit, pixels, what, planes=S.PLANES, mask=None, offset=False, nan_aware=False, table=True):
    """uploads hit (a NumPy plane) and the reference's texcoord table, calls surfacePlanes into sentinel-filled outputs, compares every
    output with the NumPy reference over the whole frame and the counters with its counts; returns (reference, {plane: bits}, stats)"""
    h, w = hit.shape[:2]
    out = {k: _filled(k, h, w, offset) for k in planes}
    res = r.surfacePlanes(_upload(hit, offset), _upload(sc["uv"], offset) if table else None, planes=planes, mask=mask, out=out)
    assert all(res[k] is out[k] for k in planes)
    ref = S.surface_ref(hit, sc, pixels, planes=planes)
    got = {k: _bits(out[k]) for k in planes}
    _same(got, ref, what, nan_aware)
    st = res["stats"]
    assert (st["pixels"], st["hits"], st["stale"], st["textured"]) == (int(np.asarray(pixels).sum()), ref["hits"], ref["stale"], ref["textured"]), (what, st)
    assert st["kernel_ms"] > 0 if st["pixels"] else st["kernel_ms"] >= 0
    return ref, got, st


def _frame(w=W, h=H):
    return whole_frame_mask(h, w)


# ------------------------------------------------------------------ 1. the texcoord table
def test_texcoord_table(ptlib):
    c = _case("textured")
    nt = c.r.vertexCount()[1]
    want = c.sc["uv"]
    assert nt == 16 and c.table.shape == (nt, 6) and want.any()
    assert np.array_equal(c.table.view(np.uint32), want.view(np.uint32))
    # the table depends on the scene only: after a rebuild and after a refit it is what it was
    A = _affine((0.0, 1.0, 0.0), 0.2, (1.0, 1.0, 1.0), (0.1, 0.15, -0.05))
    r = _renderer(c.model, (W, H), c.cam)
    r.transformMeshes({2: A}, rebuild=True)
    assert np.array_equal(_np(r.copyTexcoordsDevice()).view(np.uint32), want.view(np.uint32)), "after PT_UPDATE_REBUILD"
    r.transformMeshes({1: A})
    assert np.array_equal(_np(r.copyTexcoordsDevice()).view(np.uint32), want.view(np.uint32)), "after a refit"
    # into the caller's tensor one float into its allocation; the float in front of it and the one behind stay
    buf = torch.full((6 * nt + 2,), float("nan"), device="cuda:0")
    out = buf[1:-1].view(nt, 6)
    assert r.copyTexcoordsDevice(out=out) is out and out.data_ptr() % 8 == 4
    assert np.array_equal(_np(out).view(np.uint32), want.view(np.uint32)) and np.isnan(_np(buf[:1])).all() and np.isnan(_np(buf[-1:])).all()
    r.close()
    # the scene as scenes.py builds it: the box has zero texcoords, so all three meshes are textured
    m = scenes.textured_scene()
    r = _renderer(m, (W, H), c.cam)
    sc = S.scene_arrays(m)
    assert np.array_equal(_np(r.copyTexcoordsDevice()).view(np.uint32), sc["uv"].view(np.uint32))
    ref, _, st = _run(r, sc, _np(r.renderGBuffer(("hit",))["hit"]), _frame(), "the box with zero texcoords")
    assert st["textured"] == st["hits"] == c.gstats["hits"]
    r.close()
    # no textured mesh: zeros, also over a destination that held something else
    k = _case("cornell")
    assert k.table.shape == (32, 6) and not k.table.view(np.uint32).any()
    buf = torch.full((6 * 32 + 1,), float("nan"), device="cuda:0")
    out = buf[1:].view(32, 6)
    assert k.r.copyTexcoordsDevice(out=out) is out and not _bits(out).any() and np.isnan(_np(buf[:1])).all()


# ------------------------------------------------------------------ 2. the planes of real hit planes
@pytest.mark.parametrize("name", ["textured", "cornell"])
def test_real_planes(ptlib, name):
    c = _case(name)
    n = W * H
    ref, got, st = _run(c.r, c.sc, c.hit, _frame(), name)
    print(f"{name}: pixels {st['pixels']} hits {st['hits']} textured {st['textured']} kernel_ms {st['kernel_ms']:.4f}")
    assert st["hits"] == c.gstats["hits"] and st["stale"] == 0 and 0 < st["hits"] < n
    if name == "textured":
        colour = st["hits"] - st["textured"]
        assert st["textured"] * 10 >= n and colour * 10 >= n, (st, n)
        box = ref["mesh"] == 2  # names texture 0, has no texcoords: visible, its material's colour, no texcoord
        assert int(box.sum()) == colour and (got["albedo"][box] == np.array([0.3, 0.4, 0.8, 1.0], f32).view(np.uint32)).all() and not got["texcoord"][box].any()
        for mesh in (0, 1):  # the texture shows: many distinct albedos on each textured mesh
            assert len(np.unique(got["albedo"][ref["mesh"] == mesh], axis=0)) > 50
    else:
        assert st["textured"] == 0 and not got["texcoord"].any()
        assert len(np.unique(got["albedo"][ref["kind"] == 1], axis=0)) == 3  # white, red, green
        _run(c.r, c.sc, c.hit, _frame(), "cornell without a table", table=False)
    for plane in S.PLANES:
        _run(c.r, c.sc, c.hit, _frame(), f"{name}: {plane} alone", planes=(plane,))
    miss = ref["kind"] == 2
    assert miss.any() and (got["albedo"][miss] == np.array([0, 0, 0, S.ONE], np.uint32)).all()


# ------------------------------------------------------------------ 3. a second route to the same texels
def test_texture_0_through_the_table_evaluator(ptlib):
    c = _case("textured")
    ref = S.surface_ref(c.hit, c.sc, _frame())
    res = c.r.surfacePlanes(_upload(c.hit), _upload(c.table), planes=S.PLANES)
    on0 = ref["mesh"] == 0
    assert on0.sum() > 1000
    st = np.ascontiguousarray(ref["st"][on0])
    assert np.array_equal(_bits(res["texcoord"])[on0], st.view(np.uint32))
    rgba = c.r.evalTable(7, st, 4)
    assert np.array_equal(_bits(res["albedo"])[on0][:, :3], rgba.view(np.uint32)[:, :3])


def test_hand_made_hit_planes(ptlib):
    c = _case("textured")
    hit, cat, nan_box = _hand_made(c.sc)
    n = W * H
    assert all(int((cat == k).sum()) * 20 >= n for k in range(16))  # every category in at least 5 % of the pixels
    ref, got, st = _run(c.r, c.sc, hit, _frame(), "hand-made", nan_aware=True)
    ntri = 16
    prim = hit.view(np.int32)[..., 3]
    assert st["stale"] == int(((cat == 10) | (cat == 11)).sum()) and st["hits"] == int(((prim >= 0) & (prim < ntri)).sum())
    assert (ref["kind"][(cat == 9) | (cat == 12)] == 2).all() and (ref["kind"][(cat == 10) | (cat == 11)] == 3).all()
    flat = np.array([0, 0, 0, S.ONE], np.uint32)
    for k in (9, 10, 11, 12):
        assert (got["albedo"][cat == k] == flat).all() and not got["texcoord"][cat == k].any()
    for m in range(3):
        assert int((ref["mesh"] == m).sum()) * 20 >= n
    tc = got["texcoord"].view(f32)
    assert (tc[cat == 4] == np.array([1, 0], f32)).all()
    on5 = tc[cat == 5]
    assert (on5[:, 0] * 64 == np.round(on5[:, 0] * 64)).all() and (on5[:, 1] * 64 == np.round(on5[:, 1] * 64)).all()
    assert ((on5[:, 1] * 32 == np.round(on5[:, 1] * 32)).mean() > 0.3) and ((on5[:, 1] * 32 != np.round(on5[:, 1] * 32)).mean() > 0.3)
    # non-finite barycentrics: NaN colour and w = 1 on the texture path, the plain colour on the colour path
    for k in (13, 14):
        assert np.isnan(got["albedo"].view(f32)[cat == k][:, :3]).all() and (got["albedo"][cat == k][:, 3] == S.ONE).all()
        assert not np.isfinite(tc[cat == k]).all(-1).any()
    assert nan_box.sum() > 10 and (got["albedo"][nan_box] == np.array([0.3, 0.4, 0.8, 1.0], f32).view(np.uint32)).all()
    # the same plane through a block mask: nothing outside the set is written
    nby, nbx = c.r.blockGrid()
    mask = np.random.default_rng(6).random((nby, nbx)) < 0.5
    mask[0, 0] = mask[nby - 1, nbx - 1] = True
    px = pixel_mask(mask, h=H, w=W)
    _, got, st = _run(c.r, c.sc, hit, px, "hand-made, masked", mask=mask, nan_aware=True)
    assert 0 < st["pixels"] < n and all((got[k][~px] == SENTINEL).all() for k in S.PLANES)


# ------------------------------------------------------------------ 5. the tie to the frame path
def test_albedo_buffer_of_a_frame_where_the_neighbourhood_is_one_mesh(ptlib):
    c = _case("cornell")
    r = R.SampleRenderer(c.model)
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.resize((W, H))
    r.setCamera(R.make_camera(c.cam, W / H))
    r.launchParams.samples_per_launch = 1
    r.launchParams.frame.subframe_index = 0
    r.render()
    buf = np.ascontiguousarray(r.download(R.PT_BUF_ALBEDO), f32).reshape(H, W, 4).view(np.uint32)
    res = r.surfacePlanes(r.renderGBuffer(("hit",))["hit"])
    alb = _bits(res["albedo"])
    ref = S.surface_ref(c.hit, c.sc, _frame())
    assert np.array_equal(alb, ref["albedo"])
    mesh = ref["mesh"]
    pad = np.pad(mesh, 1, mode="edge")
    one = np.ones((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            one &= pad[dy:dy + H, dx:dx + W] == mesh
    q = one & (mesh >= 0)
    hits, mismatches = int((mesh >= 0).sum()), int((buf[q] != alb[q]).any(-1).sum())
    print(f"cornell: {hits} hit pixels, {int(q.sum())} with a one-mesh 3 x 3 neighbourhood, {mismatches} mismatches against PT_BUF_ALBEDO")
    assert int(q.sum()) * 2 >= hits and mismatches == 0
    r.close()


# ------------------------------------------------------------------ 6. pixel sets
def test_block_mask(ptlib):
    c = _case("textured")
    nby, nbx = c.r.blockGrid()
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.4
    mask[0, 0] = mask[nby - 1, nbx - 1] = mask[0, nbx - 1] = mask[nby - 1, 3] = True  # corner and edge blocks, the 3-wide column and the 5-high row
    mask[1, 1] = False
    px = pixel_mask(mask, h=H, w=W)
    _, got, st = _run(c.r, c.sc, c.hit, px, "a random block mask", mask=mask)
    assert 0 < st["pixels"] < W * H
    for name in S.PLANES:
        assert (got[name][~px] == SENTINEL).all()
    assert not (got["albedo"][px][:, 3] == SENTINEL).any()
    _, _, st = _run(c.r, c.sc, c.hit, np.zeros((H, W), bool), "the empty mask", mask=np.zeros((nby, nbx), bool))
    assert st == dict(pixels=0, hits=0, stale=0, textured=0, kernel_ms=st["kernel_ms"])


def test_partition_rank_1_of_3(ptlib):
    c = _case("textured")
    by, bx = np.mgrid[0:H, 0:W] // 8
    r = _renderer(c.model, (W, H), c.cam, partition=(1, 3, 8, 8))
    own = (bx + by) % 3 == 1
    _, got, st = _run(r, c.sc, c.hit, own, "rank 1 of 3")
    assert st["pixels"] == int(own.sum()) and (got["albedo"][~own] == SENTINEL).all()
    r.close()


def test_two_views_off_the_block_grid(ptlib):
    c = _case("textured")
    r = _renderer(c.model, (W, H), c.cam)
    rects = RECTS[:2]
    assert any(v % 8 for rect in rects for v in rect)
    r.setViews([(x, y, w, h, R.make_camera(dict(cd, **{k: S.TEX_CAMERA[k] for k in ("eye", "lookat", "fovY")}), w / h)) for (x, y, w, h), cd in zip(rects, _cam_dicts())])
    inside = np.zeros((H, W), bool)
    for x, y, w, h in rects:
        inside[y:y + h, x:x + w] = True
    hit = _np(r.renderGBuffer(("hit",), out=dict(hit=_upload(np.zeros((H, W, 8), f32))))["hit"])
    _, got, st = _run(r, c.sc, hit, inside, "two views")
    assert st["pixels"] == sum(w * h for _, _, w, h in rects) and 0 < st["textured"] < st["pixels"]
    for name in S.PLANES:
        assert (got[name][~inside] == SENTINEL).all()
    r.setViews([])
    r.setCamera(R.make_camera(c.cam, W / H))
    _run(r, c.sc, c.hit, _frame(), "views dropped")
    r.close()


def test_planes_and_table_four_byte_aligned_only(ptlib):
    c = _case("textured")
    _run(c.r, c.sc, c.hit, _frame(), "everything one float into its allocation", offset=True)
    hit, _, _ = _hand_made(c.sc)
    _run(c.r, c.sc, hit, _frame(), "hand-made, one float into its allocation", offset=True, nan_aware=True)


@pytest.mark.parametrize("size", [(8, 8), (1, 1), (9, 17)])
def test_small_frames(ptlib, size):
    c = _case("textured")
    w, h = size
    cam = dict(c.cam, lookat=(0.0, 0.05, -0.8), fovY=12.0) if size == (1, 1) else c.cam  # the one pixel looks at the ground
    r = _renderer(c.model, size, cam)
    g = r.renderGBuffer(("hit",))
    _, _, st = _run(r, c.sc, _np(g["hit"]), _frame(w, h), f"{w} x {h}")
    assert st["pixels"] == w * h and st["hits"] == g["stats"]["hits"] > 0 and st["textured"] > 0
    r.close()


# ------------------------------------------------------------------ 7. the loop
def _loop(model, cam0, frames, adaptive, plan):
    """examples/adaptive_svgf_albedo_loop.py (adaptive) or the unmasked chain of examples/svgf_albedo_loop.py fed the same surface albedo;
    returns per frame the bits of every output, the hit mask and the plan's statistics"""
    r = R.SampleRenderer(model)
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.resize((W, H))
    r.launchParams.samples_per_launch = 1
    r.uploadAccum(np.zeros((H, W, 4), f32))
    z = lambda k: torch.zeros((H, W, k) if k > 1 else (H, W), device="cuda:0")  # noqa: E731
    gbuf = [dict(hit=z(8), position=z(4), motion=z(2)) for _ in range(2)]
    hist, mom, ln = [z(4), z(4)], [z(2), z(2)], [z(1), z(1)]
    var, filt, scratch, albedo = z(1), z(4), z(4), z(4)
    table = r.copyTexcoordsDevice()
    accum = r.deviceBuffer(R.PT_BUF_ACCUM)
    cam = R.make_camera(cam0, W / H)
    out = []
    for k in range(frames):
        prev, cam = cam, R.make_camera(T.forward(cam0, 0.01 * k, dx=0.02 * k), W / H)
        cur, old, i, o = gbuf[k & 1], gbuf[~k & 1], k & 1, ~k & 1
        r.setCamera(cam)
        r.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev, out=cur)
        s = r.surfacePlanes(cur["hit"], table, out=dict(albedo=albedo))
        r.launchParams.frame.subframe_index = k
        geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], hist[i], mom[i], ln[i])
        outs = dict(history_out=hist[o], moments_out=mom[o], length_out=ln[o], variance_out=var)
        stats = None
        if adaptive:
            p = r.samplePlan(*geo, frame_index=k, **plan)
            mask, stats = p["mask"], p["stats"]
            r.renderMask(mask)
            r.temporalMoments(accum, *geo, albedo=albedo, **outs, mask=mask, color_scale=float(k + 1), clear_color=True)
            r.temporalCarry(*geo, **outs, mask=mask == 0)
        else:
            r.render()
            r.temporalMoments(accum, *geo, albedo=albedo, **outs, color_scale=float(k + 1), clear_color=True)
        r.filterPlanes(hist[o], cur["hit"], cur["position"], variance=var, length=ln[o], out=filt, scratch=scratch)
        final = _filled("albedo", H, W)
        r.modulatePlanes(filt, albedo=albedo, out=final)
        bits = {n: _bits(t) for n, t in (("history", hist[o]), ("moments", mom[o]), ("length", ln[o]), ("variance", var), ("filtered", filt), ("final", final))}
        out.append(dict(bits=bits, hit=_np(cur["hit"]).view(np.int32)[..., 3] >= 0, plan=stats, surface=s["stats"]))
    r.close()
    return out


def test_loop_with_every_block_sampled_is_the_unmasked_chain(ptlib):
    a = _loop(S.textured_scene(), S.TEX_CAMERA, 3, True, dict(min_length=65535, min_pixels=1))
    b = _loop(S.textured_scene(), S.TEX_CAMERA, 3, False, None)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["plan"]["sampled"] == x["plan"]["blocks"]
        for n in x["bits"]:
            assert np.array_equal(x["bits"][n], y["bits"][n]), f"frame {k}: {n} differs in {int((x['bits'][n] != y['bits'][n]).sum())} words"
    assert (a[2]["bits"]["length"].view(f32) > 1).any() and a[2]["bits"]["history"].any() and a[2]["surface"]["textured"] > 0


def test_loop_under_a_real_plan_fills_every_hit_pixel(ptlib):
    frames = _loop(S.textured_scene(), S.TEX_CAMERA, 6, True, dict(threshold=1e3, dark_floor=1.0, min_length=2, min_pixels=8))
    skipped = [f["plan"]["blocks"] - f["plan"]["sampled"] for f in frames]
    print("blocks left unrendered per frame:", skipped)
    assert max(skipped[2:]) > 0
    for k, f in enumerate(frames):
        final = f["bits"]["final"][f["hit"]]
        assert not (final == SENTINEL).any() and np.isfinite(final.view(f32)).all(), f"frame {k}"


# ------------------------------------------------------------------ 8. the rendering state is left alone
@pytest.mark.parametrize("frames_in_flight", [1, 3])
def test_rendering_state_is_left_alone(ptlib, frames_in_flight):
    c = _case("textured")
    probe = scenes.sky_probe(256, 128).BuildCDF()

    def run(with_call):
        r = R.SampleRenderer(S.textured_scene())
        r.setProbe(probe)
        r.setOptions(frames_in_flight=frames_in_flight)
        r.resize((W, H))
        r.setCamera(R.make_camera(c.cam, W / H))
        r.launchParams.samples_per_launch = 2
        for k in (0, 1):
            r.launchParams.frame.subframe_index = k
            r.render()
        if with_call:
            r.sync()
            before = r.stats()
            assert np.array_equal(_np(r.copyTexcoordsDevice()), c.table)
            _run(r, c.sc, c.hit, _frame(), "between the frames")
            assert r.stats() == before
        allocs = r.stats()["path_state_allocs"]
        r.launchParams.frame.subframe_index = 2
        r.render()
        r.sync()
        bufs = [r.download(k) for k in range(5)]
        assert r.stats()["path_state_allocs"] == allocs
        r.close()
        return bufs, allocs

    (a, allocs_a), (b, allocs_b) = run(True), run(False)
    assert allocs_a == allocs_b
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), f"buffer {k} differs after copyTexcoordsDevice and surfacePlanes between the frames"


# ------------------------------------------------------------------ 9. refusals
def test_refusals(ptlib):
    c = _case("textured")
    L = _lib.load_library()
    r = R.SampleRenderer(c.model)
    nt = 16
    dev = dict(hit=_upload(c.hit), prim_texcoords=_upload(c.table))
    out = {k: _filled(k, H, W) for k in S.PLANES}
    good = {k: t.data_ptr() for k, t in list(dev.items()) + list(out.items())}
    good["flags"] = 0

    def refused(what, pattern, ctx=None, **fields):
        d = _lib.SurfaceDesc()
        for k, v in dict(good, **fields).items():
            setattr(d, k, v)
        torch.cuda.synchronize()
        s = _lib.SurfaceStats(7, 7, 7, 7, 7.0)
        ctx = ctx or r
        rc = L.pt_surface_planes(ctx._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(ctx._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_surface_planes") and pattern in msg, f"{what}: {msg!r}"
        assert (s.pixels, s.hits, s.stale, s.textured, s.kernel_ms) == (7, 7, 7, 7, 7.0)
        for k, t in out.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {k} was written"

    refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(c.cam, W / H))
    assert L.pt_surface_planes(r._ctx, None, None) == -1 and "null description" in L.pt_last_error(r._ctx).decode()
    refused("a flag", "unknown flag bits 1", flags=1)
    refused("a flag comes before the planes", "unknown flag bits 4", flags=4, hit=None)
    refused("no output", "no plane asked for", albedo=None, texcoord=None)
    refused("hit null", "hit is null", hit=None)
    host = np.zeros((H, W, 8), f32)
    refused("a host pointer", "hit is not device memory", hit=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "albedo is not 4-byte aligned", albedo=good["albedo"] + 2)
    refused("the table offset by 1 byte", "prim_texcoords is not 4-byte aligned", prim_texcoords=good["prim_texcoords"] + 1)
    # one element too small for what is left of its allocation (an allocation of the runtime's own: torch's allocator hands out parts of larger ones)
    hip = _hip_runtime()
    for name, nbytes in (("prim_texcoords", nt * 24), ("texcoord", H * W * 8)):
        raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert hip.hipMalloc(C.byref(raw), C.c_size_t(nbytes)) == 0
        try:
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= nbytes
            refused(f"{name} one element too small", f"{name} has fewer than {nbytes} bytes left", **{name: raw.value + size.value - (nbytes - 4)})
        finally:
            assert hip.hipFree(raw) == 0
    # an output may overlap no other plane, nor the table; hit and prim_texcoords are only read
    refused("the albedo on the hit plane", "hit and albedo overlap", albedo=good["hit"])
    refused("the texcoord inside the hit plane", "hit and texcoord overlap", texcoord=good["hit"] + 4 * (H * W * 6))
    refused("the table inside the albedo", "prim_texcoords and albedo overlap", prim_texcoords=good["albedo"] + 16)
    refused("two outputs", "albedo and texcoord overlap", texcoord=good["albedo"] + 4 * (H * W * 2))
    refused("no table on a textured scene", "prim_texcoords is required", prim_texcoords=None)
    # pt_copy_texcoords_device
    dst = torch.full((nt + 1, 6), float("nan"), device="cuda:0")

    def copy_refused(what, pattern, p, nbytes):
        torch.cuda.synchronize()
        rc = L.pt_copy_texcoords_device(r._ctx, p, nbytes)
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1 and msg.startswith("pt_copy_texcoords_device") and pattern in msg, f"{what}: {rc} {msg!r}"
        assert np.isnan(_np(dst)).all(), f"{what}: the destination was written"

    copy_refused("too few bytes", f"bytes must equal triangles * 24 = {nt * 24}", dst.data_ptr(), nt * 24 - 24)
    copy_refused("too many bytes", "bytes must equal triangles * 24", dst.data_ptr(), nt * 24 + 24)
    copy_refused("a null pointer", "dev_dst is null", None, nt * 24)
    copy_refused("a host pointer", "dev_dst is not device memory", host.ctypes.data, nt * 24)
    copy_refused("a pointer offset by 2 bytes", "dev_dst is not 4-byte aligned", dst.data_ptr() + 2, nt * 24)
    # an untextured scene takes no table, and ignores one that is given — even a pointer that would fail the checks
    k = _case("cornell")
    res = k.r.surfacePlanes(_upload(k.hit), 2, out=dict(albedo=out["albedo"]))
    assert np.array_equal(_bits(out["albedo"]), S.surface_ref(k.hit, k.sc, _frame())["albedo"]) and res["stats"]["textured"] == 0
    out["albedo"].view(torch.uint8).fill_(0xA5)
    # the Python facade checks dtype, shape and device before the library is called, and passes the library's refusals on
    with pytest.raises(ValueError, match="albedo.*shape"):
        r.surfacePlanes(dev["hit"], dev["prim_texcoords"], out=dict(albedo=out["texcoord"]))
    with pytest.raises(ValueError, match="the tensor is on cpu"):
        r.surfacePlanes(torch.zeros((H, W, 8)), dev["prim_texcoords"])
    with pytest.raises(ValueError, match=r"prim_texcoords: a contiguous torch.float32 tensor of shape \(16, 6\) is expected"):
        r.surfacePlanes(dev["hit"], torch.zeros((15, 6), device="cuda:0"))
    with pytest.raises(RuntimeError, match="prim_texcoords is required"):
        r.surfacePlanes(dev["hit"])
    assert np.array_equal(_bits(dev["hit"]), c.hit.view(np.uint32))
    # a valid call afterwards still works, into the same planes
    res = r.surfacePlanes(dev["hit"], dev["prim_texcoords"], planes=S.PLANES, out=out)
    ref = S.surface_ref(c.hit, c.sc, _frame())
    _same({k: _bits(out[k]) for k in S.PLANES}, ref, "a valid call after the refusals")
    assert res["stats"]["textured"] == ref["textured"]
    # ... and so does one that lets the facade allocate its output (zero-filled)
    res = r.surfacePlanes(dev["hit"], dev["prim_texcoords"])
    assert np.array_equal(_bits(res["albedo"]), ref["albedo"]) and set(res) == {"albedo", "stats"}
    r.close()
