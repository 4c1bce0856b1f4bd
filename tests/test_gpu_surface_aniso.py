"""Anisotropic footprint-filtered albedo (pt_surface_aniso_planes) on the GPU.  Every plane is compared bit for bit, over the WHOLE plane (a pixel
written outside the chosen set shows as a lost sentinel), with tests/surface_aniso_ref.py: float32 NumPy evaluating the header's rule on the
hit plane renderGBuffer gave (or a hand-made one), the model's host arrays, the current vertices and the cameras.  All seven counters are
compared exactly.  NaN words compare as NaN (payloads are not specified).  Frames are 131 x 59 and smaller.

Two invariants are checked GPU against GPU — max_aniso = 1 is pt_surface_lod_planes, footprint_scale = 0 is pt_surface_planes — and one check
carries a meaning beyond the reference, with its bound recorded by tests/test_surface_aniso_cabi.py from the references alone: under the
grazing camera the anisotropic albedo is closer to the pixel's average than the isotropic one (R_ANISO)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import surface_aniso_ref as SA
import surface_lod_ref as SL
import surface_ref as S
from conftest import ROOT
from gpu_kit import filled, pixel_mask, plane_shape, whole_frame_mask
from gpu_kit import bits3 as _bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import same_words as _same
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from gpu_kit import words_differ as _differ
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from pass_cases import _Case
from pass_cases import surface_aniso_case as _case
from scene_kit import RECTS, _affine
from surface_aniso_ref import GRAZING_CAMERA, R_ANISO, H, W, check_hand_made, ground_truth
from surface_lod_ref import ground_pixels, rms_against

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = S.SENTINEL
COUNTERS = ("pixels", "hits", "stale", "textured", "minified", "anisotropic", "taps")


def _filled(name, h, w, offset=False):
    """a sentinel-filled plane of the pass; offset: one float into its allocation (4-byte aligned only)"""
    return filled(plane_shape(h, w, SA.WORDS[name]), offset)


def _run(r, c, hit, pixels, what, max_aniso=8, planes=SA.PLANES, mask=None, scale=1.0, verts=None, rects=None, cams=None, offset=False, sc=None, idx=None,
         table=None, mips=None):
    """uploads hit, calls surfaceAnisoPlanes into sentinel-filled outputs, compares every output with the NumPy reference over the whole frame
    and the seven counters with its counts; returns (reference, {plane: bits}, stats)"""
    h, w = hit.shape[:2]
    sc = c.sc if sc is None else sc
    out = {n: _filled(n, h, w, offset) for n in planes}
    res = r.surfaceAnisoPlanes(_upload(hit, offset), c.table if table is None else table, c.mips if mips is None else mips, max_aniso=max_aniso, planes=planes,
                               footprint_scale=scale, mask=mask, out=out)
    assert all(res[n] is out[n] for n in planes)
    ref = SA.surface_aniso_ref(hit, sc, c.verts if verts is None else verts, c.idx if idx is None else idx, rects or [(0, 0, w, h)],
                               [c.row] if cams is None else cams, pixels, max_aniso=max_aniso, scale=scale, planes=planes)
    got = {n: _bits(out[n]) for n in planes}
    _same(got, ref, what)
    st = res["stats"]
    want = (int(np.asarray(pixels).sum()), ref["hits"], ref["stale"], ref["textured"], ref["minified"], ref["anisotropic"], ref["taps_sum"])
    assert tuple(st[k] for k in COUNTERS) == want, (what, st, want)
    return ref, got, st


def _frame(w=W, h=H):
    return whole_frame_mask(h, w)


# ------------------------------------------------------------------ 1. the pass against the reference
@pytest.mark.parametrize("name", ["textured", "cornell"])
def test_real_planes(ptlib, name):
    c = _case(name)
    for amax in (2, 8, 16):
        ref, got, st = _run(c.r, c, c.hit, _frame(), f"{name}, max_aniso {amax}", max_aniso=amax)
        print(f"{name}, max_aniso {amax}: " + ", ".join(f"{k} {st[k]}" for k in COUNTERS) + f", kernel_ms {st['kernel_ms']:.4f}")
        assert st["hits"] == c.gstats["hits"] and st["stale"] == 0
        taps = got["taps"].view(f32)[..., 0]
        if name == "textured":
            tex = ref["kind"] == 4
            assert 0 < st["anisotropic"] <= st["minified"] < st["textured"] < st["taps"] and taps.max() == amax and (taps[~tex] == 0).all() and (taps[tex] >= 1).all()
            box = ref["mesh"] == 2
            assert (got["albedo"][box] == np.array([0.3, 0.4, 0.8, 1.0], f32).view(np.uint32)).all()
        else:
            assert st["textured"] == st["minified"] == st["anisotropic"] == st["taps"] == 0
            assert not got["texcoord"].any() and not got["footprint"].any() and not got["lod"].any() and not got["taps"].any()
    if name == "cornell":
        res = c.r.surfaceAnisoPlanes(_upload(c.hit), planes=SA.PLANES)  # no table, no pyramid
        assert np.array_equal(_bits(res["albedo"]), ref["albedo"])


def test_each_output_alone_and_without_the_taps_plane(ptlib):
    c = _case("textured")
    for plane in SA.PLANES:
        _run(c.r, c, c.hit, _frame(), f"{plane} alone", planes=(plane,))
    _, _, st = _run(c.r, c, c.hit, _frame(), "taps = NULL", planes=SL.PLANES)
    assert st["taps"] > st["textured"]  # the counter does not need the plane


def test_planes_one_float_into_their_allocations(ptlib):
    c = _case("textured")
    table = _upload(c.sc["uv"], True)
    _run(c.r, c, c.hit, _frame(), "every plane 4 bytes off a 16-byte boundary", offset=True, table=table)


def test_two_views_off_the_block_grid_with_different_cameras(ptlib):
    c = _case("textured")
    r = _renderer(c.model, (W, H), c.cam)
    rects = RECTS[:2]
    cams = [R.make_camera(GRAZING_CAMERA, rects[0][2] / rects[0][3]), R.make_camera(dict(GRAZING_CAMERA, eye=(-1.5, 2.5, -3.5), fovY=50.0), rects[1][2] / rects[1][3])]
    r.setViews([(x, y, w, h, cam) for (x, y, w, h), cam in zip(rects, cams)])
    rows = R._camera_rows(cams)
    inside = np.zeros((H, W), bool)
    for x, y, w, h in rects:
        inside[y:y + h, x:x + w] = True
    hit = _np(r.renderGBuffer(("hit",), out=dict(hit=_upload(np.zeros((H, W, 8), f32))))["hit"])
    ref, got, st = _run(r, c, hit, inside, "two views", rects=rects, cams=rows)
    assert st["pixels"] == sum(w * h for _, _, w, h in rects) and st["anisotropic"] > 0
    for x, y, w, h in rects:
        assert (ref["n"][y:y + h, x:x + w] > 1).sum() > 100
    for name in SA.PLANES:
        assert (got[name][~inside] == SENTINEL).all()
    r.setViews([])
    r.setCamera(R.make_camera(c.cam, W / H))
    _run(r, c, c.hit, _frame(), "views dropped")
    r.close()


def test_block_mask_and_rank_1_of_3(ptlib):
    c = _case("textured")
    nby, nbx = c.r.blockGrid()
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.4
    mask[0, 0] = mask[nby - 1, nbx - 1] = mask[0, nbx - 1] = mask[nby - 1, 3] = True
    mask[1, 1] = False
    px = pixel_mask(mask, h=H, w=W)
    _, got, st = _run(c.r, c, c.hit, px, "a random block mask", mask=mask)
    assert 0 < st["pixels"] < W * H and all((got[n][~px] == SENTINEL).all() for n in SA.PLANES)
    _, _, st = _run(c.r, c, c.hit, np.zeros((H, W), bool), "the empty mask", mask=np.zeros((nby, nbx), bool))
    assert st == dict({k: 0 for k in COUNTERS}, kernel_ms=st["kernel_ms"])
    by, bx = np.mgrid[0:H, 0:W] // 8
    r = _renderer(c.model, (W, H), c.cam, partition=(1, 3, 8, 8))
    own = (bx + by) % 3 == 1
    _, got, st = _run(r, c, c.hit, own, "rank 1 of 3")
    assert st["pixels"] == int(own.sum()) and (got["albedo"][~own] == SENTINEL).all() and (got["taps"][~own] == SENTINEL).all()
    r.close()


@pytest.mark.parametrize("size", [(8, 8), (1, 1), (9, 17)])
def test_small_frames(ptlib, size):
    c = _case("textured")
    w, h = size
    cam = dict(c.cam, lookat=(0.0, 0.0, -0.8), fovY=12.0) if size == (1, 1) else c.cam
    r = _renderer(c.model, size, cam)
    g = r.renderGBuffer(("hit",))
    row = R._camera_rows([R.make_camera(cam, w / h)])
    _, _, st = _run(r, c, _np(g["hit"]), _frame(w, h), f"{w} x {h}", cams=row)
    assert st["pixels"] == w * h and st["hits"] == g["stats"]["hits"] > 0 and st["minified"] > 0  # few pixels: each covers many texels
    r.close()


# ------------------------------------------------------------------ 2. hand-made hit planes over small textures
def test_hand_made_hit_planes_over_small_textures(ptlib):
    """tests/surface_aniso_ref.py's hand-made inputs: 16 x 16 pixels under an exact camera, textures of 16 x 8, 5 x 3 and 1 x 1, one primitive
    per case of the rule (HAND_PRIMS names them and the N each must take).  The camera is a view's, so this is the kernel's view path."""
    c = _Case()
    c.model = SA.hand_made_model()
    c.sc = S.scene_arrays(c.model)
    hit, where = SA.hand_made_hit()
    w, h = SA.HAND_W, SA.HAND_H
    r = _renderer(c.model, (w, h), dict(eye=(0.0, 0.0, 0.0), lookat=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fovY=90.0))
    r.setViews([(0, 0, w, h, R.make_camera(dict(eye=(0.0, 0.0, 0.0), lookat=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fovY=90.0), 1.0))])
    r.setViewCameras(SA.HAND_ROW[None, :])
    k = list(SA.HAND_PRIMS).index("zero_area")
    r.transformMeshes({k: _affine((0.0, 1.0, 0.0), 0.0, (1.0, 0.0, 0.0), (0.0, 0.0, 1.0))})  # onto the line y = 0, z = 1
    c.verts, c.idx = SA.hand_made_verts(c.model)
    assert np.array_equal(_np(r.copyVerticesDevice()).view(np.uint32), c.verts.view(np.uint32))
    c.row, c.table, c.mips = SA.HAND_ROW, r.copyTexcoordsDevice(), r.copyTextureMipsDevice()
    dims, nbytes = r.textureMipsLayout()
    assert dims[:, :3].tolist() == [[16, 8, 5], [5, 3, 3], [1, 1, 1]] and nbytes == 16 * ((8 * 4 + 4 * 2 + 2 * 1 + 1) + (2 * 1 + 1))
    rect = [(0, 0, w, h)]
    for amax in (8, 16):
        ref, got, st = _run(r, c, hit, _frame(w, h), f"hand-made, max_aniso {amax}", max_aniso=amax, rects=rect)
        check_hand_made(got["taps"].view(f32)[..., 0].astype(np.int64), got["lod"].view(f32)[..., 0], where, amax)
        assert st["stale"] == 2 and st["hits"] == 252
    taps, fp, alb = got["taps"].view(f32)[..., 0], got["footprint"].view(f32), got["albedo"].view(f32)
    assert (taps[where["rho_min_0"]] == 16).all() and np.isnan(fp[where["zero_area"]]).all() and np.isfinite(fp[7]).all()
    for name in ("nan_u", "inf_v"):  # non-finite barycentrics: NaN colour, w = 1; the footprint and N do not depend on them
        assert np.isnan(alb[where[name]][:, :3]).all() and (alb[where[name]][:, 3] == 1).all() and (taps[where[name]] >= 3).all()
    flat = np.array([0, 0, 0, S.ONE], np.uint32)
    for name in ("miss", "miss_2", "stale_ntri", "stale_max"):
        assert (got["albedo"][where[name]] == flat).all() and not got["texcoord"][where[name]].any() and not got["taps"][where[name]].any()
    # other caps: the same records take other N, and with them other levels
    for amax in (1, 2, 3):
        _run(r, c, hit, _frame(w, h), f"hand-made, max_aniso {amax}", max_aniso=amax, rects=rect)
    _run(r, c, hit, _frame(w, h), "hand-made, scale 0.37", scale=0.37, rects=rect)
    # both invariants on these records as well, GPU against GPU
    _invariants(r, c, hit, "hand-made")
    r.close()


# ------------------------------------------------------------------ 3. the invariants, GPU against GPU
def _invariants(r, c, hit, what):
    d_hit = _upload(hit)
    for scale in (1.0, 3.7):
        one = r.surfaceAnisoPlanes(d_hit, c.table, c.mips, max_aniso=1, planes=SA.PLANES, footprint_scale=scale)
        iso = r.surfaceLodPlanes(d_hit, c.table, c.mips, planes=SL.PLANES, footprint_scale=scale)
        for name in SL.PLANES:
            neq = _differ(_bits(one[name]), _bits(iso[name]))
            assert not neq.any(), f"{what}, scale {scale}: {name} at max_aniso 1 differs from pt_surface_lod_planes's in {int(neq.sum())} words"
        assert all(one["stats"][k] == iso["stats"][k] for k in ("pixels", "hits", "stale", "textured", "minified"))
        assert one["stats"]["anisotropic"] == 0 and one["stats"]["taps"] == one["stats"]["textured"]
    point = r.surfacePlanes(d_hit, c.table, planes=S.PLANES)
    for amax in (1, 8, 16):
        zero = r.surfaceAnisoPlanes(d_hit, c.table, c.mips, max_aniso=amax, planes=SA.PLANES, footprint_scale=0.0)
        for name in S.PLANES:
            neq = _differ(_bits(zero[name]), _bits(point[name]))
            assert not neq.any(), f"{what}, max_aniso {amax}: {name} at footprint_scale 0 differs from pt_surface_planes's in {int(neq.sum())} words"
        assert zero["stats"]["minified"] == zero["stats"]["anisotropic"] == 0 and zero["stats"]["taps"] == zero["stats"]["textured"] and not _bits(zero["lod"]).any()


def test_max_aniso_1_is_surface_lod_planes_and_scale_0_is_surface_planes(ptlib):
    c = _case("textured")
    _invariants(c.r, c, c.hit, "real")
    _run(c.r, c, c.hit, _frame(), "scale 0", scale=0.0)
    _run(c.r, c, c.hit, _frame(), "scale 3.7", scale=3.7)
    _, got, st = _run(c.r, c, c.hit, _frame(), "scale 1e9", scale=1e9)
    assert st["minified"] == st["textured"]


# ------------------------------------------------------------------ 4. state
def test_after_transform_meshes_the_planes_follow_the_moved_geometry(ptlib):
    c = _case("textured")
    r = _renderer(c.model, (W, H), c.cam)
    r.transformMeshes({0: _affine((0.0, 1.0, 0.0), 0.3, (1.5, 1.0, 0.8), (0.1, -0.05, 0.2)), 1: _affine((1.0, 0.0, 0.0), 0.2, (1.0, 1.2, 1.0), (0.0, 0.1, 0.0))})
    verts = _np(r.copyVerticesDevice())
    assert not np.array_equal(verts, c.verts)
    hit = _np(r.renderGBuffer(("hit",))["hit"])
    ref, got, st = _run(r, c, hit, _frame(), "after transformMeshes", verts=verts)
    stale_geometry = SA.surface_aniso_ref(hit, c.sc, c.verts, c.idx, [(0, 0, W, H)], [c.row], _frame())
    assert st["anisotropic"] > 0 and not np.array_equal(stale_geometry["footprint"], got["footprint"]) and not np.array_equal(stale_geometry["taps"], got["taps"])
    r.close()


def test_rendering_state_is_left_alone(ptlib):
    c = _case("textured")
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
            res = r.surfaceAnisoPlanes(_upload(c.hit), c.table, mips, planes=SA.PLANES)
            assert res["stats"]["anisotropic"] > 0 and r.stats() == before
        allocs = r.stats()["path_state_allocs"]
        r.launchParams.frame.subframe_index = 2
        r.render()
        r.sync()
        bufs = [r.download(n) for n in range(5)]
        assert r.stats()["path_state_allocs"] == allocs
        r.close()
        return bufs

    for n, (x, y) in enumerate(zip(run(True), run(False))):
        assert x.tobytes() == y.tobytes(), f"buffer {n} differs after surfaceAnisoPlanes between the frames"


# ------------------------------------------------------------------ 5. what the plane means
def test_anisotropic_albedo_is_closer_to_the_pixel_average(ptlib):
    c = _case("textured")
    d_hit = _upload(c.hit)
    mesh = S.surface_ref(c.hit, c.sc, _frame())["mesh"]
    q = ground_pixels(mesh)
    truth = ground_truth(dict(verts=c.verts, idx=c.idx, sc=c.sc, row=c.row), W, H, q)
    iso = c.r.surfaceLodPlanes(d_hit, c.table, c.mips)
    aniso = c.r.surfaceAnisoPlanes(d_hit, c.table, c.mips, max_aniso=8, planes=("albedo", "taps"))
    n = _np(aniso["taps"])[q]
    e_iso, e_aniso = rms_against(_bits(iso["albedo"]), truth, q), rms_against(_bits(aniso["albedo"]), truth, q)
    bound = (1 + R_ANISO) / 2
    print(f"quality: {int(q.sum())} ground pixels, N >= 3 on {float((n >= 3).mean()):.3f} of them, rms isotropic {e_iso:.4f}, rms anisotropic {e_aniso:.4f}, "
          f"ratio {e_aniso / e_iso:.4f} (the reference: {R_ANISO}; asserted: <= {bound:.4f})")
    assert q.sum() > 2000 and (n >= 3).mean() >= 0.5 and e_aniso <= bound * e_iso


# ------------------------------------------------------------------ 6. refusals
def test_refusals(ptlib):
    c = _case("textured")
    L = _lib.load_library()
    r = R.SampleRenderer(c.model)
    dev = dict(hit=_upload(c.hit), prim_texcoords=c.table, mips=c.mips)
    out = {n: _filled(n, H, W) for n in SA.PLANES}
    good = {n: t.data_ptr() for n, t in list(dev.items()) + list(out.items())}
    good.update(flags=0, mips_bytes=c.bytes, footprint_scale=1.0, max_aniso=8)

    def refused(what, pattern, **fields):
        d = _lib.SurfaceAnisoDesc()
        for n, v in dict(good, **fields).items():
            setattr(d, n, v)
        torch.cuda.synchronize()
        s = _lib.SurfaceAnisoStats(7, 7, 7, 7, 7, 7, 7, 7.0)
        rc = L.pt_surface_aniso_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_surface_aniso_planes") and pattern in msg, f"{what}: {msg!r}"
        assert tuple(getattr(s, n) for n, _ in s._fields_) == (7, 7, 7, 7, 7, 7, 7, 7.0)
        for n, t in out.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {n} was written"

    refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(c.cam, W / H))
    assert L.pt_surface_aniso_planes(r._ctx, None, None) == -1 and "pt_surface_aniso_planes: null description" in L.pt_last_error(r._ctx).decode()
    refused("a flag", "unknown flag bits 1", flags=1)
    refused("a flag comes before the planes", "unknown flag bits 4", flags=4, hit=None)
    refused("max_aniso 0", "max_aniso must be 1..16, not 0", max_aniso=0)
    refused("max_aniso 17", "max_aniso must be 1..16, not 17", max_aniso=17)
    refused("max_aniso 2^31", "max_aniso must be 1..16", max_aniso=1 << 31)
    refused("no output", "no plane asked for (albedo, texcoord, footprint, lod, taps are all null)", albedo=None, texcoord=None, footprint=None, lod=None, taps=None)
    for bad in (-1.0, float("nan"), float("inf"), -0.5):
        refused(f"footprint_scale {bad}", "footprint_scale must be finite and >= 0", footprint_scale=bad)
    refused("wrong mips_bytes", f"mips_bytes must equal pt_texture_mips_layout's {c.bytes}", mips_bytes=c.bytes - 16)
    refused("zero mips_bytes", "mips_bytes must equal", mips_bytes=0)
    refused("hit null", "hit is null", hit=None)
    host = np.zeros((H, W, 8), f32)
    refused("a host pointer", "hit is not device memory", hit=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "taps is not 4-byte aligned", taps=good["taps"] + 2)
    refused("the pyramid offset by 1 byte", "mips is not 4-byte aligned", mips=good["mips"] + 1)
    hip = _hip_runtime()
    for name, nbytes in (("taps", H * W * 4), ("footprint", H * W * 16)):
        raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert hip.hipMalloc(C.byref(raw), C.c_size_t(nbytes)) == 0
        try:
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= nbytes
            refused(f"{name} one element too small", f"{name} has fewer than {nbytes} bytes left", **{name: raw.value + size.value - (nbytes - 16)})
        finally:
            assert hip.hipFree(raw) == 0
    refused("the albedo on the hit plane", "hit and albedo overlap", albedo=good["hit"])
    refused("the taps inside the hit plane", "hit and taps overlap", taps=good["hit"] + 4 * (H * W * 6))
    refused("the table inside the taps", "prim_texcoords and taps overlap", prim_texcoords=good["taps"] + 16)
    refused("the pyramid inside the taps", "mips and taps overlap", mips=good["taps"] + 16)
    refused("two outputs", "albedo and taps overlap", taps=good["albedo"] + 4 * (H * W * 2))
    refused("two outputs", "lod and taps overlap", taps=good["lod"])
    refused("two outputs", "footprint and lod overlap", lod=good["footprint"] + 4 * (H * W * 3))
    refused("no table on a textured scene", "prim_texcoords is required", prim_texcoords=None)
    refused("no pyramid on a textured scene", "mips is required", mips=None)
    big = torch.zeros((c.bytes // 16 + 1, 4), device="cuda:0")
    refused("the pyramid 4 bytes off", "mips is not 16-byte aligned", mips=big.data_ptr() + 4)
    # the Python facade checks before the library is called, and passes the library's refusals on
    with pytest.raises(ValueError, match="max_aniso must be an integer in 1..16"):
        r.surfaceAnisoPlanes(dev["hit"], dev["prim_texcoords"], dev["mips"], max_aniso=17)
    with pytest.raises(RuntimeError, match="mips is required"):
        r.surfaceAnisoPlanes(dev["hit"], dev["prim_texcoords"])
    with pytest.raises(RuntimeError, match="footprint_scale must be finite"):
        r.surfaceAnisoPlanes(dev["hit"], dev["prim_texcoords"], dev["mips"], footprint_scale=-2.0)
    # a valid call afterwards still works, into the same planes; and one that lets the facade allocate its output
    res = r.surfaceAnisoPlanes(dev["hit"], dev["prim_texcoords"], dev["mips"], planes=SA.PLANES, out=out)
    ref = SA.surface_aniso_ref(c.hit, c.sc, c.verts, c.idx, [(0, 0, W, H)], [c.row], _frame())
    _same({n: _bits(out[n]) for n in SA.PLANES}, ref, "a valid call after the refusals")
    assert res["stats"]["taps"] == ref["taps_sum"]
    res = r.surfaceAnisoPlanes(dev["hit"], dev["prim_texcoords"], dev["mips"])
    assert np.array_equal(_bits(res["albedo"]), ref["albedo"]) and set(res) == {"albedo", "stats"}
    r.close()


# ------------------------------------------------------------------ 7. the loops with --aniso 8
def test_adaptive_loop_with_aniso_fills_every_hit_pixel(ptlib):
    """examples/adaptive_svgf_albedo_loop.py --aniso 8, at W x H: the chain of tests/test_gpu_surface_lod.py's loop with surfaceAnisoPlanes in
    the place of surfaceLodPlanes"""
    import temporal_ref as T

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
    cam = R.make_camera(GRAZING_CAMERA, W / H)
    for n in range(4):
        prev, cam = cam, R.make_camera(T.forward(GRAZING_CAMERA, 0.01 * n, dx=0.02 * n), W / H)
        cur, old, i, o = gbuf[n & 1], gbuf[~n & 1], n & 1, ~n & 1
        r.setCamera(cam)
        r.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev, out=cur)
        s = r.surfaceAnisoPlanes(cur["hit"], table, mips, max_aniso=8, out=dict(albedo=albedo))
        assert s["stats"]["anisotropic"] > 0
        r.launchParams.frame.subframe_index = n
        geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], hist[i], mom[i], ln[i])
        outs = dict(history_out=hist[o], moments_out=mom[o], length_out=ln[o], variance_out=var)
        mask = r.samplePlan(*geo, frame_index=n, threshold=1e3, dark_floor=1.0, min_length=2, min_pixels=8)["mask"]
        r.renderMask(mask)
        r.temporalMoments(accum, *geo, albedo=albedo, **outs, mask=mask, color_scale=float(n + 1), clear_color=True)
        r.temporalCarry(*geo, **outs, mask=mask == 0)
        r.filterPlanes(hist[o], cur["hit"], cur["position"], variance=var, length=ln[o], out=filt, scratch=scratch)
        final = _filled("albedo", H, W)
        r.modulatePlanes(filt, albedo=albedo, out=final)
        is_hit = _np(cur["hit"]).view(np.int32)[..., 3] >= 0
        bits = _bits(final)[is_hit]
        assert not (bits == SENTINEL).any() and np.isfinite(bits.view(f32)).all(), f"frame {n}"
    r.close()


def test_upsampled_loop_with_aniso_fills_every_hit_pixel(ptlib):
    """examples/upsampled_svgf_loop.py's UpsampledLoop with aniso=8 at 128 x 56, scale 2; without aniso the class is what it was"""
    spec = importlib.util.spec_from_file_location("upsampled_svgf_loop", os.path.join(ROOT, "examples", "upsampled_svgf_loop.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    w, h = 128, 56
    probe = scenes.sky_probe(256, 128).BuildCDF()
    up = ex.UpsampledLoop(S.textured_scene(), (w, h), 2, aniso=8, probe=probe)
    assert up.lod and up.aniso == 8 and up.mips[id(up.hi)] is not None
    cam = R.make_camera(GRAZING_CAMERA, w / h)
    for k in range(3):
        prev, cam = cam, R.make_camera(ex.orbit(GRAZING_CAMERA, 0.01 * k), w / h)
        up.final.view(torch.uint8).fill_(0xA5)
        x = up.frame(k, prev, cam)
        is_hit = _np(up.hi_gbuf["hit"]).view(np.int32)[..., 3] >= 0
        bits = _bits(up.final)[is_hit]
        assert x["pixels"] == w * h and not (bits == SENTINEL).any() and np.isfinite(bits.view(f32)).all(), f"frame {k}"
    # the display-resolution albedo is the anisotropic pass's
    want = up.hi.surfaceAnisoPlanes(up.hi_gbuf["hit"], up.table[id(up.hi)], up.mips[id(up.hi)], max_aniso=8)
    assert np.array_equal(_bits(up.albedo), _bits(want["albedo"])) and want["stats"]["anisotropic"] > 0
    up.close()
    plain = ex.UpsampledLoop(S.textured_scene(), (w, h), 2, probe=probe)
    assert not plain.lod and plain.aniso == 0 and plain.mips[id(plain.hi)] is None
    plain.close()
