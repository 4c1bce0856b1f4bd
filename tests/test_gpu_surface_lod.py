"""Footprint-filtered albedo (pt_texture_mips_layout, pt_copy_texture_mips_device, pt_surface_lod_planes) on the GPU.  Every plane is compared
bit for bit, over the WHOLE plane (a pixel written outside the chosen set shows as a lost sentinel), with tests/surface_lod_ref.py: float32
NumPy evaluating the header's arithmetic on the hit plane renderGBuffer gave, the model's host arrays, the current vertices and the cameras.
Counters are compared exactly.  NaN words compare as NaN (payloads are not specified).  The inputs are those of tests/test_gpu_surface.py
(131 x 61 and smaller), and its cached renderers are shared.

Two checks carry a meaning beyond the reference, with bounds recorded by tests/test_surface_lod_cabi.py from the reference alone: the
footprint plane against the differences of the texcoord plane between neighbouring pixels (FOOT_BOUND), and the filtered albedo against a
256-spp PT_BUF_ALBEDO, which is the pixel average (R_REF)."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_ref as M
import surface_lod_ref as SL
import surface_ref as S
import temporal_ref as T
from gpu_kit import filled, pixel_mask, plane_shape, whole_frame_mask
from gpu_kit import bits as _bits
from gpu_kit import bits3 as _plane_bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import same_words as _same
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from pass_cases import H, W, _hand_made
from pass_cases import surface_case as _case
from scene_kit import RECTS, _affine
from surface_lod_ref import FOOT_BOUND, R_REF, check_footprints, ground_pixels, rms_against

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = S.SENTINEL


def _filled(name, h, w):
    """a sentinel-filled plane of the pass"""
    return filled(plane_shape(h, w, SL.WORDS[name]))


class _Lod:
    pass


_LOD = {}


def _lod_case(name):
    """pass_cases.surface_case with what the LOD pass needs beside it: the model's vertices and indices, the camera row, the pyramid"""
    if name not in _LOD:
        c = _case(name)
        k = _Lod()
        k.c = c
        k.verts, k.idx = M.model_arrays(c.model)
        k.row = R._camera_rows([R.make_camera(c.cam, W / H)])[0]
        k.dims, k.bytes = c.r.textureMipsLayout()
        k.mips = c.r.copyTextureMipsDevice()
        _LOD[name] = k
    return _LOD[name]


def _run(r, k, hit, pixels, what, planes=SL.PLANES, mask=None, scale=1.0, verts=None, rects=None, cams=None):
    """uploads hit, calls surfaceLodPlanes into sentinel-filled outputs, compares every output with the NumPy reference over the whole frame
    and the counters with its counts; returns (reference, {plane: bits}, stats)"""
    h, w = hit.shape[:2]
    out = {n: _filled(n, h, w) for n in planes}
    res = r.surfaceLodPlanes(_upload(hit), _upload(k.c.sc["uv"]), k.mips, planes=planes, footprint_scale=scale, mask=mask, out=out)
    assert all(res[n] is out[n] for n in planes)
    ref = SL.surface_lod_ref(hit, k.c.sc, k.verts if verts is None else verts, k.idx, rects or [(0, 0, w, h)], [k.row] if cams is None else cams, pixels,
                             scale=scale, planes=planes)
    got = {n: _plane_bits(out[n]) for n in planes}
    _same(got, ref, what)
    st = res["stats"]
    want = (int(np.asarray(pixels).sum()), ref["hits"], ref["stale"], ref["textured"], ref["minified"])
    assert (st["pixels"], st["hits"], st["stale"], st["textured"], st["minified"]) == want, (what, st, want)
    return ref, got, st


def _frame(w=W, h=H):
    return whole_frame_mask(h, w)


# ------------------------------------------------------------------ 1. the pyramid
def test_pyramid(ptlib):
    k = _lod_case("textured")
    c = k.c
    want = SL.pyramid(c.sc["textures"])
    dims, nbytes = SL.layout([(t.shape[1], t.shape[0]) for t in c.sc["textures"]])
    assert np.array_equal(k.dims, dims) and k.bytes == nbytes == 16 * (683 + 637)
    assert k.mips.shape == want.shape and np.array_equal(_bits(k.mips), want.view(np.uint32))
    # the scene as scenes.py builds it holds the same textures
    r = _renderer(scenes.textured_scene(), (W, H), c.cam)
    assert np.array_equal(_bits(r.copyTextureMipsDevice()), want.view(np.uint32))
    # into the caller's tensor; the 16 bytes in front of it and the 16 behind stay
    buf = torch.full((want.shape[0] + 2, 4), float("nan"), device="cuda:0")
    out = buf[1:-1]
    assert r.copyTextureMipsDevice(out=out) is out and np.array_equal(_bits(out), want.view(np.uint32))
    assert np.isnan(_np(buf[:1])).all() and np.isnan(_np(buf[-1:])).all()
    # refusals: a misaligned destination, wrong bytes, null, host memory; nothing is written
    L = _lib.load_library()
    dst = torch.full((want.shape[0] + 1, 4), float("nan"), device="cuda:0")

    def refused(what, pattern, p, n):
        torch.cuda.synchronize()
        rc = L.pt_copy_texture_mips_device(r._ctx, p, n)
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1 and msg.startswith("pt_copy_texture_mips_device") and pattern in msg, f"{what}: {rc} {msg!r}"
        assert np.isnan(_np(dst)).all(), f"{what}: the destination was written"

    refused("4 bytes off", "dev_dst is not 16-byte aligned", dst.data_ptr() + 4, nbytes)
    refused("8 bytes off", "dev_dst is not 16-byte aligned", dst.data_ptr() + 8, nbytes)
    refused("2 bytes off", "dev_dst is not 4-byte aligned", dst.data_ptr() + 2, nbytes)
    refused("too few bytes", f"bytes must equal pt_texture_mips_layout's {nbytes}", dst.data_ptr(), nbytes - 16)
    refused("too many bytes", "bytes must equal", dst.data_ptr(), nbytes + 16)
    refused("zero bytes on a textured scene", "bytes must equal", dst.data_ptr(), 0)
    refused("null", "dev_dst is null", None, nbytes)
    refused("host memory", "dev_dst is not device memory", np.zeros(nbytes // 4, f32).ctypes.data, nbytes)
    r.close()
    # no texture: zero bytes, and the copy is a no-op whatever the pointer is
    q = _lod_case("cornell")
    assert q.dims.shape == (0, 4) and q.bytes == 0 and q.mips.shape == (0, 4)
    assert L.pt_copy_texture_mips_device(q.c.r._ctx, None, 0) == 0 and L.pt_copy_texture_mips_device(q.c.r._ctx, 3, 0) == 0
    assert L.pt_copy_texture_mips_device(q.c.r._ctx, dst.data_ptr(), 16) == -1 and np.isnan(_np(dst)).all()


# ------------------------------------------------------------------ 2. the pass against the reference
@pytest.mark.parametrize("name", ["textured", "cornell"])
def test_real_planes(ptlib, name):
    k = _lod_case(name)
    c = k.c
    ref, got, st = _run(c.r, k, c.hit, _frame(), name)
    print(f"{name}: pixels {st['pixels']} hits {st['hits']} textured {st['textured']} minified {st['minified']} kernel_ms {st['kernel_ms']:.4f}")
    assert st["hits"] == c.gstats["hits"] and st["stale"] == 0
    if name == "textured":
        lod = got["lod"].view(f32)[..., 0]
        tex = ref["kind"] == 4
        assert 0 < st["minified"] < st["textured"] and lod.max() > 1 and (lod[~tex] == 0).all() and not got["footprint"][~tex].any()
        assert len(np.unique(ref["level"][tex])) >= 2  # levels 0 | 1 and 1 | 2 at least
        box = ref["mesh"] == 2
        assert (got["albedo"][box] == np.array([0.3, 0.4, 0.8, 1.0], f32).view(np.uint32)).all()
    else:
        assert st["textured"] == st["minified"] == 0 and not got["texcoord"].any() and not got["footprint"].any() and not got["lod"].any()
        res = c.r.surfaceLodPlanes(_upload(c.hit), planes=SL.PLANES)  # no table, no pyramid
        assert np.array_equal(_plane_bits(res["albedo"]), ref["albedo"])
    for plane in SL.PLANES:
        _run(c.r, k, c.hit, _frame(), f"{name}: {plane} alone", planes=(plane,))


def test_two_views_off_the_block_grid_with_different_cameras(ptlib):
    k = _lod_case("textured")
    c = k.c
    r = _renderer(c.model, (W, H), c.cam)
    rects = RECTS[:2]
    cams = [R.make_camera(S.TEX_CAMERA, rects[0][2] / rects[0][3]), R.make_camera(dict(S.TEX_CAMERA, eye=(-1.5, 2.5, -3.5), fovY=50.0), rects[1][2] / rects[1][3])]
    r.setViews([(x, y, w, h, cam) for (x, y, w, h), cam in zip(rects, cams)])
    rows = R._camera_rows(cams)
    assert not np.array_equal(rows[0], rows[1])
    inside = np.zeros((H, W), bool)
    for x, y, w, h in rects:
        inside[y:y + h, x:x + w] = True
    hit = _np(r.renderGBuffer(("hit",), out=dict(hit=_upload(np.zeros((H, W, 8), f32))))["hit"])
    ref, got, st = _run(r, k, hit, inside, "two views", rects=rects, cams=rows)
    assert st["pixels"] == sum(w * h for _, _, w, h in rects) and st["minified"] > 0
    for x, y, w, h in rects:
        assert (ref["kind"][y:y + h, x:x + w] == 4).sum() > 100
    for name in SL.PLANES:
        assert (got[name][~inside] == SENTINEL).all()
    r.setViews([])
    r.setCamera(R.make_camera(c.cam, W / H))
    _run(r, k, c.hit, _frame(), "views dropped")
    r.close()


def test_block_mask_and_rank_1_of_3(ptlib):
    k = _lod_case("textured")
    c = k.c
    nby, nbx = c.r.blockGrid()
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.4
    mask[0, 0] = mask[nby - 1, nbx - 1] = mask[0, nbx - 1] = mask[nby - 1, 3] = True
    mask[1, 1] = False
    px = pixel_mask(mask, h=H, w=W)
    _, got, st = _run(c.r, k, c.hit, px, "a random block mask", mask=mask)
    assert 0 < st["pixels"] < W * H and all((got[n][~px] == SENTINEL).all() for n in SL.PLANES)
    _, _, st = _run(c.r, k, c.hit, np.zeros((H, W), bool), "the empty mask", mask=np.zeros((nby, nbx), bool))
    assert st == dict(pixels=0, hits=0, stale=0, textured=0, minified=0, kernel_ms=st["kernel_ms"])
    by, bx = np.mgrid[0:H, 0:W] // 8
    r = _renderer(c.model, (W, H), c.cam, partition=(1, 3, 8, 8))
    own = (bx + by) % 3 == 1
    _, got, st = _run(r, k, c.hit, own, "rank 1 of 3")
    assert st["pixels"] == int(own.sum()) and (got["albedo"][~own] == SENTINEL).all()
    r.close()


@pytest.mark.parametrize("size", [(8, 8), (1, 1), (9, 17)])
def test_small_frames(ptlib, size):
    k = _lod_case("textured")
    c = k.c
    w, h = size
    cam = dict(c.cam, lookat=(0.0, 0.05, -0.8), fovY=12.0) if size == (1, 1) else c.cam
    r = _renderer(c.model, size, cam)
    g = r.renderGBuffer(("hit",))
    row = R._camera_rows([R.make_camera(cam, w / h)])
    _, _, st = _run(r, k, _np(g["hit"]), _frame(w, h), f"{w} x {h}", cams=row)
    assert st["pixels"] == w * h and st["hits"] == g["stats"]["hits"] > 0 and st["minified"] > 0  # few pixels: each covers many texels
    r.close()


def _hand_made_checks(k, r, hit, cat, what, verts=None):
    ref, got, st = _run(r, k, hit, _frame(), what, verts=verts)
    flat = np.array([0, 0, 0, S.ONE], np.uint32)
    for n in (9, 10, 11, 12):  # misses, prim = ntri, 0x7fffffff, -2
        on = cat == n
        assert (got["albedo"][on] == flat).all() and not got["texcoord"][on].any() and not got["footprint"][on].any() and not got["lod"][on].any()
    assert st["stale"] == int(((cat == 10) | (cat == 11)).sum())
    for n in (13, 14):  # NaN and infinite barycentrics: NaN colour, w = 1; the footprint does not depend on them
        on = cat == n
        assert np.isnan(got["albedo"].view(f32)[on][:, :3]).all() and (got["albedo"][on][:, 3] == S.ONE).all()
    return ref, got, st


def test_hand_made_hit_planes(ptlib):
    k = _lod_case("textured")
    c = k.c
    hit, cat, _ = _hand_made(c.sc)
    ref, got, st = _hand_made_checks(k, c.r, hit, cat, "hand-made")
    # every record names a primitive chosen at random, so many pixels name a plane their rays do not meet in front of the eye — sky pixels
    # naming the ground, as at a horizon: ok is false there, the footprint is finite and the coarsest level is taken
    tex = ref["kind"] == 4
    lod, fp = got["lod"].view(f32)[..., 0], got["footprint"].view(f32)
    Lm = np.where(ref["mesh"] == 0, 6, 5)
    verts64, row = k.verts.astype(np.float64), k.row.astype(np.float64)
    prim = np.clip(hit.view(np.int32)[..., 3], 0, 15)
    tri = verts64[k.idx[prim]]
    nrm = np.cross(tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :])
    ys, xs = np.mgrid[0:H, 0:W]
    d = SL.camera_rays64(row, W, H, xs + 0.5, ys + 0.5)
    t_c = ((tri[..., 0, :] - row[0:3]) * nrm).sum(-1) / (d * nrm).sum(-1)
    behind = tex & (t_c < -1e-3)
    assert behind.sum() > 200 and (lod[behind] == Lm[behind]).all() and np.isfinite(fp[behind]).all()
    _, got, st = _run(c.r, k, hit, pixel_mask(np.ones(c.r.blockGrid(), bool), h=H, w=W), "hand-made, a full mask", mask=np.ones(c.r.blockGrid(), bool))


def test_horizon_pixels_whose_offset_ray_misses_the_plane(ptlib):
    """Hand-placed records at the ground's horizon: the centre ray meets the ground plane in front of the eye (t_c > 0) and the ray through
    the lower or right neighbour's centre does not (t <= 0), found in float64 without an expression of the header.  footprint_scale is
    1e-6, so every pixel whose three rays meet the plane stays at level 0 however long its footprint is, and only `ok == false` — an
    infinite rho2, which no scale brings down — reaches the coarsest level."""
    k = _lod_case("textured")
    c = k.c
    row = k.row.astype(np.float64)
    tri = k.verts[k.idx[0]].astype(np.float64)  # primitive 0: the ground
    nrm = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    ys, xs = np.mgrid[0:H, 0:W]

    def t_of(ax, ay):
        d = SL.camera_rays64(row, W, H, ax, ay)
        with np.errstate(all="ignore"):
            return ((tri[0] - row[0:3]) * nrm).sum() / (d * nrm).sum(-1)

    t_c, t_x, t_y = t_of(xs + 0.5, ys + 0.5), t_of(xs + 1.5, ys + 0.5), t_of(xs + 0.5, ys + 1.5)
    edge = (t_c > 0) & ((t_x <= 0) | (t_y <= 0))
    only_y = (t_c > 0) & (t_x > 0) & (t_y <= 0)
    inside = (t_c > 0) & (t_x > 0) & (t_y > 0) & (t_c < 50)
    assert edge.sum() >= W // 2 and only_y.sum() >= W // 2 and inside.sum() > 1000, (int(edge.sum()), int(only_y.sum()), int(inside.sum()))
    hit = np.zeros((H, W, 8), f32)
    words = hit.view(np.int32)
    words[..., 3] = -1
    put = edge | inside
    hit[put, 0], hit[put, 1], hit[put, 2] = 1.0, 0.25, 0.5
    words[put, 3] = 0
    ref, got, st = _run(c.r, k, hit, _frame(), "horizon pixels", scale=1e-6)
    lod = got["lod"].view(f32)[..., 0]
    assert (lod[edge] == 6).all() and (lod[inside] == 0).all() and st["minified"] == int(edge.sum()) and st["textured"] == int(put.sum())
    assert np.isfinite(got["footprint"].view(f32)[only_y]).all()
    ref, got, st = _run(c.r, k, hit, _frame(), "horizon pixels, scale 1")
    assert (got["lod"].view(f32)[..., 0][edge] == 6).all()


def test_after_transform_meshes_and_on_a_zero_area_triangle(ptlib):
    k = _lod_case("textured")
    c = k.c
    r = _renderer(c.model, (W, H), c.cam)
    r.transformMeshes({0: _affine((0.0, 1.0, 0.0), 0.3, (1.5, 1.0, 0.8), (0.1, -0.05, 0.2)), 1: _affine((1.0, 0.0, 0.0), 0.2, (1.0, 1.2, 1.0), (0.0, 0.1, 0.0))})
    verts = _np(r.copyVerticesDevice())
    assert not np.array_equal(verts, k.verts)
    hit = _np(r.renderGBuffer(("hit",))["hit"])
    ref, got, st = _run(r, k, hit, _frame(), "after transformMeshes", verts=verts)
    stale_geometry = SL.surface_lod_ref(hit, c.sc, k.verts, k.idx, [(0, 0, W, H)], [k.row], _frame())
    assert st["minified"] > 0 and not np.array_equal(stale_geometry["footprint"], got["footprint"])  # the rest vertices give other footprints
    # the wall collapsed onto a line: zero-area triangles.  n = 0, every t_r is NaN, ok is false: NaN footprints, the coarsest level
    r.transformMeshes({1: _affine((0.0, 1.0, 0.0), 0.0, (1.0, 0.0, 0.0), (0.0, 0.5, 0.0))})
    verts = _np(r.copyVerticesDevice())
    tri = verts[k.idx[2]].astype(np.float64)
    assert not np.cross(tri[1] - tri[0], tri[2] - tri[0]).any()
    hand, cat, _ = _hand_made(c.sc)
    ref, got, st = _hand_made_checks(k, r, hand, cat, "hand-made, the wall has zero area", verts=verts)
    wall = ref["mesh"] == 1
    assert wall.sum() > 500 and np.isnan(got["footprint"].view(f32)[wall]).all() and (got["lod"].view(f32)[..., 0][wall] == 5).all()
    r.close()


# ------------------------------------------------------------------ 3. footprint_scale
def test_footprint_scale_0_is_surface_planes_and_a_large_scale_is_the_coarsest_level(ptlib):
    k = _lod_case("textured")
    c = k.c
    hand, _, _ = _hand_made(c.sc)
    for what, hit in (("real", c.hit), ("hand-made", hand)):
        ref, got, st = _run(c.r, k, hit, _frame(), f"{what}, scale 0", scale=0.0)
        point = c.r.surfacePlanes(_upload(hit), _upload(c.sc["uv"]), planes=S.PLANES)
        for name in S.PLANES:
            a, b = got[name], _bits(point[name])
            with np.errstate(all="ignore"):
                neq = (a != b) & ~(np.isnan(a.view(f32)) & np.isnan(b.view(f32)))
            assert not neq.any(), f"{what}: {name} differs from pt_surface_planes's in {int(neq.sum())} words"
        assert st["minified"] == 0 and not got["lod"].any()
    ref, got, st = _run(c.r, k, c.hit, _frame(), "scale 1e9", scale=1e9)
    lod = got["lod"].view(f32)[..., 0]
    assert st["minified"] == st["textured"] and (lod[ref["mesh"] == 0] == 6).all() and (lod[ref["mesh"] == 1] == 5).all()
    _run(c.r, k, c.hit, _frame(), "scale 3.7", scale=3.7)


# ------------------------------------------------------------------ 4. what the planes mean
def test_footprints_are_the_neighbour_differences_of_the_texcoord_plane(ptlib):
    k = _lod_case("textured")
    c = k.c
    res = c.r.surfaceLodPlanes(_upload(c.hit), _upload(c.sc["uv"]), k.mips, planes=("footprint", "texcoord"))
    prim = c.hit.view(np.int32)[..., 3]
    kind = S.surface_ref(c.hit, c.sc, _frame())["kind"]
    fp, tc = _np(res["footprint"]), _np(res["texcoord"])
    out = check_footprints(fp, tc, prim, kind)
    print(f"footprints: largest error {out['err']:.3e} over {out['nx']} + {out['ny']} pixels (bound {FOOT_BOUND:.3e}), largest footprint {out['size']:.3e}")
    assert out["nx"] > 4000 and out["ny"] > 4000 and out["err"] <= FOOT_BOUND
    assert check_footprints(fp[..., [2, 3, 0, 1]], tc, prim, kind)["err"] > 100 * FOOT_BOUND
    assert check_footprints(fp * f32(0.5), tc, prim, kind)["err"] > 100 * FOOT_BOUND


def test_filtered_albedo_is_closer_to_the_pixel_average(ptlib):
    k = _lod_case("textured")
    c = k.c
    r = R.SampleRenderer(c.model)
    r.setProbe(scenes.sky_probe(64, 32).BuildCDF())
    r.resize((W, H))
    r.setCamera(R.make_camera(c.cam, W / H))
    r.launchParams.samples_per_launch = 256
    r.launchParams.frame.subframe_index = 0
    r.render()
    truth = np.ascontiguousarray(r.download(R.PT_BUF_ALBEDO), f32).reshape(H, W, 4)
    r.close()
    mesh = S.surface_ref(c.hit, c.sc, _frame())["mesh"]
    q = ground_pixels(mesh)
    out = {}
    for what, scale in (("point", 0.0), ("lod", 1.0)):
        res = c.r.surfaceLodPlanes(_upload(c.hit), _upload(c.sc["uv"]), k.mips, footprint_scale=scale)
        out[what] = rms_against(_bits(res["albedo"]), truth[..., :3][q].astype(np.float64), q)
    bound = (1 + R_REF) / 2
    print(f"quality: {int(q.sum())} ground pixels, rms point {out['point']:.4f}, rms filtered {out['lod']:.4f}, ratio {out['lod'] / out['point']:.4f} "
          f"(the reference: {R_REF}; asserted: <= {bound:.4f})")
    assert q.sum() > 2000 and out["lod"] <= bound * out["point"]


# ------------------------------------------------------------------ 5. refusals
def test_refusals(ptlib):
    k = _lod_case("textured")
    c = k.c
    L = _lib.load_library()
    r = R.SampleRenderer(c.model)
    nt = 16
    dev = dict(hit=_upload(c.hit), prim_texcoords=_upload(c.table), mips=k.mips)
    out = {n: _filled(n, H, W) for n in SL.PLANES}
    good = {n: t.data_ptr() for n, t in list(dev.items()) + list(out.items())}
    good.update(flags=0, mips_bytes=k.bytes, footprint_scale=1.0)

    def refused(what, pattern, **fields):
        d = _lib.SurfaceLodDesc()
        for n, v in dict(good, **fields).items():
            setattr(d, n, v)
        torch.cuda.synchronize()
        s = _lib.SurfaceLodStats(7, 7, 7, 7, 7, 7.0)
        rc = L.pt_surface_lod_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_surface_lod_planes") and pattern in msg, f"{what}: {msg!r}"
        assert (s.pixels, s.hits, s.stale, s.textured, s.minified, s.kernel_ms) == (7, 7, 7, 7, 7, 7.0)
        for n, t in out.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {n} was written"

    refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(c.cam, W / H))
    assert L.pt_surface_lod_planes(r._ctx, None, None) == -1 and "null description" in L.pt_last_error(r._ctx).decode()
    refused("a flag", "unknown flag bits 1", flags=1)
    refused("a flag comes before the planes", "unknown flag bits 4", flags=4, hit=None)
    refused("no output", "no plane asked for", albedo=None, texcoord=None, footprint=None, lod=None)
    for bad in (-1.0, float("nan"), float("inf"), -0.5):
        refused(f"footprint_scale {bad}", "footprint_scale must be finite and >= 0", footprint_scale=bad)
    refused("wrong mips_bytes", f"mips_bytes must equal pt_texture_mips_layout's {k.bytes}", mips_bytes=k.bytes - 16)
    refused("zero mips_bytes", "mips_bytes must equal", mips_bytes=0)
    refused("hit null", "hit is null", hit=None)
    host = np.zeros((H, W, 8), f32)
    refused("a host pointer", "hit is not device memory", hit=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "footprint is not 4-byte aligned", footprint=good["footprint"] + 2)
    refused("the pyramid offset by 1 byte", "mips is not 4-byte aligned", mips=good["mips"] + 1)
    hip = _hip_runtime()
    for name, nbytes in (("mips", k.bytes), ("lod", H * W * 4), ("footprint", H * W * 16)):
        raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert hip.hipMalloc(C.byref(raw), C.c_size_t(nbytes)) == 0
        try:
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= nbytes
            refused(f"{name} one element too small", f"{name} has fewer than {nbytes} bytes left", **{name: raw.value + size.value - (nbytes - 16)})
        finally:
            assert hip.hipFree(raw) == 0
    refused("the albedo on the hit plane", "hit and albedo overlap", albedo=good["hit"])
    refused("the lod inside the hit plane", "hit and lod overlap", lod=good["hit"] + 4 * (H * W * 6))
    refused("the table inside the footprint", "prim_texcoords and footprint overlap", prim_texcoords=good["footprint"] + 16)
    refused("the pyramid inside the albedo", "mips and albedo overlap", mips=good["albedo"] + 16)
    refused("two outputs", "albedo and texcoord overlap", texcoord=good["albedo"] + 4 * (H * W * 2))
    refused("two outputs", "footprint and lod overlap", lod=good["footprint"] + 4 * (H * W * 3))
    refused("no table on a textured scene", "prim_texcoords is required", prim_texcoords=None)
    refused("no pyramid on a textured scene", "mips is required", mips=None)
    big = torch.zeros((k.bytes // 16 + 1, 4), device="cuda:0")
    refused("the pyramid 4 bytes off", "mips is not 16-byte aligned", mips=big.data_ptr() + 4)
    # an untextured scene ignores the table and the pyramid — even pointers that would fail the checks
    q = _lod_case("cornell")
    res = q.c.r.surfaceLodPlanes(_upload(q.c.hit), 2, 6, out=dict(albedo=out["albedo"]))
    assert np.array_equal(_bits(out["albedo"]), S.surface_ref(q.c.hit, q.c.sc, _frame())["albedo"]) and res["stats"]["textured"] == 0
    out["albedo"].view(torch.uint8).fill_(0xA5)
    # the Python facade checks dtype, shape and device before the library is called, and passes the library's refusals on
    with pytest.raises(ValueError, match=r"mips: a contiguous torch.float32 tensor of shape \(1320, 4\) is expected"):
        r.surfaceLodPlanes(dev["hit"], dev["prim_texcoords"], torch.zeros((1319, 4), device="cuda:0"))
    with pytest.raises(RuntimeError, match="mips is required"):
        r.surfaceLodPlanes(dev["hit"], dev["prim_texcoords"])
    with pytest.raises(RuntimeError, match="footprint_scale must be finite"):
        r.surfaceLodPlanes(dev["hit"], dev["prim_texcoords"], dev["mips"], footprint_scale=-2.0)
    assert np.array_equal(_bits(dev["hit"]), c.hit.view(np.uint32)) and np.array_equal(_bits(k.mips), SL.pyramid(c.sc["textures"]).view(np.uint32))
    # a valid call afterwards still works, into the same planes; and one that lets the facade allocate its output
    res = r.surfaceLodPlanes(dev["hit"], dev["prim_texcoords"], dev["mips"], planes=SL.PLANES, out=out)
    ref = SL.surface_lod_ref(c.hit, c.sc, k.verts, k.idx, [(0, 0, W, H)], [k.row], _frame())
    _same({n: _plane_bits(out[n]) for n in SL.PLANES}, ref, "a valid call after the refusals")
    assert res["stats"]["minified"] == ref["minified"]
    res = r.surfaceLodPlanes(dev["hit"], dev["prim_texcoords"], dev["mips"])
    assert np.array_equal(_bits(res["albedo"]), ref["albedo"]) and set(res) == {"albedo", "stats"}
    r.close()


# ------------------------------------------------------------------ 6. the rendering state is left alone
def test_rendering_state_is_left_alone(ptlib):
    k = _lod_case("textured")
    c = k.c
    probe = scenes.sky_probe(256, 128).BuildCDF()

    def run(with_call):
        r = R.SampleRenderer(S.textured_scene())
        r.setProbe(probe)
        r.setOptions(frames_in_flight=3)
        r.resize((W, H))
        r.setCamera(R.make_camera(c.cam, W / H))
        r.launchParams.samples_per_launch = 2
        for n in (0, 1):
            r.launchParams.frame.subframe_index = n
            r.render()
        if with_call:
            mips = r.copyTextureMipsDevice()  # with frames in flight: it drains them first
            before = r.stats()
            assert np.array_equal(_bits(mips), _bits(k.mips)) and r.textureMipsLayout()[1] == k.bytes
            res = r.surfaceLodPlanes(_upload(c.hit), _upload(c.table), mips, planes=SL.PLANES)
            assert res["stats"]["minified"] > 0 and r.stats() == before
        allocs = r.stats()["path_state_allocs"]
        r.launchParams.frame.subframe_index = 2
        r.render()
        r.sync()
        bufs = [r.download(n) for n in range(5)]
        assert r.stats()["path_state_allocs"] == allocs
        r.close()
        return bufs

    for n, (x, y) in enumerate(zip(run(True), run(False))):
        assert x.tobytes() == y.tobytes(), f"buffer {n} differs after copyTextureMipsDevice and surfaceLodPlanes between the frames"


# ------------------------------------------------------------------ 7. the loop with --lod
def test_loop_with_lod_fills_every_hit_pixel(ptlib):
    """examples/adaptive_svgf_albedo_loop.py --lod, at 131 x 61: the chain of tests/test_gpu_surface.py's _loop with surfaceLodPlanes in
    the place of surfacePlanes"""
    r = R.SampleRenderer(S.textured_scene())
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.resize((W, H))
    r.launchParams.samples_per_launch = 1
    r.uploadAccum(np.zeros((H, W, 4), f32))
    z = lambda n: torch.zeros((H, W, n) if n > 1 else (H, W), device="cuda:0")  # noqa: E731
    gbuf = [dict(hit=z(8), position=z(4), motion=z(2)) for _ in range(2)]
    hist, mom, ln = [z(4), z(4)], [z(2), z(2)], [z(1), z(1)]
    var, filt, scratch, albedo = z(1), z(4), z(4), z(4)
    table, mips = r.copyTexcoordsDevice(), r.copyTextureMipsDevice()
    accum = r.deviceBuffer(R.PT_BUF_ACCUM)
    cam = R.make_camera(S.TEX_CAMERA, W / H)
    skipped = []
    for n in range(5):
        prev, cam = cam, R.make_camera(T.forward(S.TEX_CAMERA, 0.01 * n, dx=0.02 * n), W / H)
        cur, old, i, o = gbuf[n & 1], gbuf[~n & 1], n & 1, ~n & 1
        r.setCamera(cam)
        r.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev, out=cur)
        s = r.surfaceLodPlanes(cur["hit"], table, mips, out=dict(albedo=albedo))
        assert s["stats"]["minified"] > 0
        r.launchParams.frame.subframe_index = n
        geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], hist[i], mom[i], ln[i])
        outs = dict(history_out=hist[o], moments_out=mom[o], length_out=ln[o], variance_out=var)
        p = r.samplePlan(*geo, frame_index=n, threshold=1e3, dark_floor=1.0, min_length=2, min_pixels=8)
        mask = p["mask"]
        skipped.append(p["stats"]["blocks"] - p["stats"]["sampled"])
        r.renderMask(mask)
        r.temporalMoments(accum, *geo, albedo=albedo, **outs, mask=mask, color_scale=float(n + 1), clear_color=True)
        r.temporalCarry(*geo, **outs, mask=mask == 0)
        r.filterPlanes(hist[o], cur["hit"], cur["position"], variance=var, length=ln[o], out=filt, scratch=scratch)
        final = _filled("albedo", H, W)
        r.modulatePlanes(filt, albedo=albedo, out=final)
        is_hit = _np(cur["hit"]).view(np.int32)[..., 3] >= 0
        bits = _bits(final)[is_hit]
        assert not (bits == SENTINEL).any() and np.isfinite(bits.view(f32)).all(), f"frame {n}"
    assert max(skipped[2:]) > 0
    r.close()
