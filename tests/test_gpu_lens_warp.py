"""Lens warp and late reprojection (pt_lens_warp_planes) on the GPU.  Every output is compared bit for bit, over the WHOLE plane (a pixel
written outside the chosen set shows as a lost sentinel), with tests/lens_warp_ref.py: float32 NumPy evaluating the header's rule on the
same colour plane, rectangles and lens records.  All three counters are compared exactly.  NaN words compare as NaN (payloads are not
specified).  Frames are 131 x 59 and smaller.

One check carries a meaning beyond the reference, with its bound (lens_warp_ref.R_WARP) measured by tests/test_lens_warp_cabi.py from the
references alone: a frame warped by pt_warp_matrix is closer than the unwarped one to the frame the turned camera renders."""
import ctypes as C

import numpy as np
import pytest
import torch

import lens_warp_ref as LW
import surface_ref as S
from gpu_kit import filled, pixel_mask, plane_shape, whole_frame_mask
from gpu_kit import bits3 as _bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import same_words as _same
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from lens_warp_ref import INPUTS, R_WARP, YAW, H, W
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from scene_kit import RECTS

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = LW.SENTINEL
COUNTERS = ("pixels", "outside", "nonfinite")
NAN, INF = f32(np.nan), f32(np.inf)
BORDER = (0.25, 0.5, 0.75)


def _filled(name, h, w, offset=False):
    """a sentinel-filled plane of the pass; offset: one float into its allocation (4-byte aligned only)"""
    return filled(plane_shape(h, w, LW.WORDS[name]), offset, torch.int32 if name == "frame_rgba8" else torch.float32)


class _Case:
    pass


_CASES = {}


def _case(name):
    """the model, a renderer under the input's camera at W x H and its pixel-centre albedo as the colour.  Built once; read-only."""
    if name not in _CASES:
        make, cam = INPUTS[name]
        c = _Case()
        c.model, c.cam = make(), cam
        c.r = _renderer(c.model, (W, H), cam)
        c.table = c.r.copyTexcoordsDevice()
        c.color = _albedo(c.r, c.table)
        c.color.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


def _albedo(r, table, out=None):
    g = r.renderGBuffer(("hit",), out=None if out is None else dict(hit=out[0]))
    return _np(r.surfacePlanes(g["hit"], table, planes=("albedo",), out=None if out is None else dict(albedo=out[1]))["albedo"])


def _row(cam, w=W, h=H):
    return R._camera_rows([R.make_camera(cam, w / h)])[0]


def _turn(name="textured", yaw=0.0, pitch=0.0, roll=0.0, size=(W, H)):
    cam = INPUTS[name][1]
    return R.warpMatrix(_row(cam, *size), _row(LW.turned(cam, yaw, pitch, roll), *size), size)


def _run(r, orc, color, pixels, what, lenses=None, rects=None, mask=None, offset=False, planes=LW.PLANES, border=(0.0, 0.0, 0.0), bicubic=False):
    """uploads the colour, calls lensWarpPlanes into sentinel-filled outputs, compares every output with the NumPy reference over the whole
    frame and the three counters with its counts; returns (reference, {plane: bits}, stats)"""
    h, w = color.shape[:2]
    out = {n: _filled(n, h, w, offset) for n in planes}
    res = r.lensWarpPlanes(_upload(color, offset), out=out.get("out"), frame=out.get("frame_rgba8"), mask=mask, lenses=lenses, border=border, bicubic=bicubic)
    assert all(res[n] is out[n] for n in planes)
    ref = LW.lens_warp_ref(color, rects or [(0, 0, w, h)], lenses, pixels, border=border, bicubic=bicubic, planes=planes, orc=orc)
    got = {n: _bits(out[n]) for n in planes}
    _same(got, ref, what)
    st = res["stats"]
    want = tuple(ref[k] for k in COUNTERS)
    assert tuple(st[k] for k in COUNTERS) == want and want[0] == int(np.asarray(pixels).sum()), (what, st, want)
    return ref, got, st


def _frame(w=W, h=H):
    return whole_frame_mask(h, w)


def _one_ulp(k):
    """three k rows, green's first coefficient one unit in the last place above the others'"""
    rows = np.stack([np.asarray(k, f32)] * 3)
    rows[1, 0] = np.nextafter(rows[1, 0], f32(np.inf))
    return rows


# name -> make_lens's keywords for a W x H rectangle
CHROMA_K = ((0.09, 0.05, 0.0), (0.1, 0.05, 0.0), (0.11, 0.05, 0.0))
LENSES = {
    "barrel": lambda: dict(k=(0.1, 0.05, 0.0)),
    "pincushion": lambda: dict(k=(-0.15, 0.02, 0.0)),
    "per-channel": lambda: dict(k=CHROMA_K),
    "rows equal": lambda: dict(k=np.stack([np.asarray((-0.15, 0.02, 0.01), f32)] * 3)),
    "rows one ulp apart": lambda: dict(k=_one_ulp((-0.15, 0.02, 0.01))),
    "off-centre": lambda: dict(k=(-0.2, 0.03, 0.0), center=(40.25, 11.0), radius=(50.0, 33.0)),
    "yaw pitch roll": lambda: dict(warp=_turn(yaw=2.0, pitch=-1.5, roll=4.0)),
    "lens and matrix": lambda: dict(k=CHROMA_K, warp=_turn(yaw=YAW, pitch=1.0)),
}


# ------------------------------------------------------------------ 1. the pass against the reference
@pytest.mark.parametrize("name", ["cornell", "textured"])
def test_identity_returns_the_colour(ptlib, orc_det, name):
    c = _case(name)
    for what, lenses in (("lenses=None", None), ("explicit identity", [R.make_lens((W, H))]), ("k = 0, radius 0", [R.make_lens((W, H), center=(1.0, 2.0), radius=0.0)])):
        for bicubic in (False, True):
            ref, got, st = _run(c.r, orc_det, c.color, _frame(), f"{name}, {what}", lenses=lenses, bicubic=bicubic)
            assert st["outside"] == 0 and st["nonfinite"] == 0
            assert np.array_equal(got["out"].view(f32)[..., 0:3], c.color[..., 0:3]) and (got["out"][..., 3] == S.ONE).all()
            words, mine = c.color.view(np.uint32)[..., 0:3], got["out"][..., 0:3]
            assert ((mine == words) | ((words == 0x80000000) & (mine == 0))).all()  # bit for bit, but for a -0 that became +0


@pytest.mark.parametrize("bicubic", [False, True], ids=["bilinear", "bicubic"])
@pytest.mark.parametrize("lens", sorted(LENSES))
def test_lens_and_matrix_cases(ptlib, orc_det, lens, bicubic):
    c = _case("textured")
    lenses = [R.make_lens((W, H), **LENSES[lens]())]
    ref, got, st = _run(c.r, orc_det, c.color, _frame(), lens, lenses=lenses, border=BORDER, bicubic=bicubic)
    print(f"{lens}, {'bicubic' if bicubic else 'bilinear'}: " + ", ".join(f"{k} {st[k]}" for k in COUNTERS) + f", kernel_ms {st['kernel_ms']:.4f}")
    assert st["outside"] <= W * H // 4 and st["nonfinite"] == 0
    moved = (ref["sx"][:, 1] != ref["X"] + f32(0.5)) | (ref["sy"][:, 1] != ref["Y"] + f32(0.5))
    assert moved.sum() > W * H // 2
    apart = (ref["sx"][:, 0] != ref["sx"][:, 2]).any()
    assert apart if lens in ("per-channel", "lens and matrix") else not apart or lens == "rows one ulp apart"


def test_each_optional_output_may_be_absent(ptlib, orc_det):
    c = _case("textured")
    lenses = [R.make_lens((W, H), **LENSES["lens and matrix"]())]
    for planes in (("out",), ("frame_rgba8",), ("out", "frame_rgba8")):
        _run(c.r, orc_det, c.color, _frame(), f"planes {planes}", lenses=lenses, planes=planes, border=BORDER)
    res = c.r.lensWarpPlanes(_upload(c.color), lenses=lenses, border=BORDER)  # the facade allocates out
    assert set(res) == {"out", "frame_rgba8", "stats"} and res["frame_rgba8"] is None
    assert np.array_equal(_bits(res["out"]), LW.lens_warp_ref(c.color, [(0, 0, W, H)], lenses, _frame(), border=BORDER)["out"])
    frame = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")  # with a frame alone, out is not allocated; uint8 (h, w, 4) is taken
    res = c.r.lensWarpPlanes(_upload(c.color), frame=frame, lenses=lenses, border=BORDER)
    assert res["out"] is None and res["frame_rgba8"] is frame
    want = LW.lens_warp_ref(c.color, [(0, 0, W, H)], lenses, _frame(), border=BORDER, planes=("frame_rgba8",), orc=orc_det)["frame_rgba8"]
    assert np.array_equal(_np(frame).view(np.uint32).reshape(H, W, 1), want)


@pytest.mark.parametrize("bicubic", [False, True], ids=["bilinear", "bicubic"])
def test_planes_one_float_into_their_allocations(ptlib, orc_det, bicubic):
    c = _case("textured")
    for lens in ("pincushion", "lens and matrix"):
        _run(c.r, orc_det, c.color, _frame(), f"{lens}, every plane 4 bytes off a 16-byte boundary", lenses=[R.make_lens((W, H), **LENSES[lens]())], offset=True,
             bicubic=bicubic)


@pytest.mark.parametrize("size", [(1, 1), (8, 8), (9, 17), (64, 3)])
def test_small_frames(ptlib, orc_det, size):
    """the clamp of the 2 x 2 and 4 x 4 windows in rectangles narrower than a window, partial blocks, a one-pixel rectangle"""
    c = _case("cornell")
    w, h = size
    r = _renderer(c.model, size, c.cam)
    color = np.random.default_rng(w * 100 + h).random((h, w, 4)).astype(f32)
    for what, kw in (("identity", dict()), ("pincushion", dict(k=(-0.3, 0.05, 0.0))), ("per-channel and a turn", dict(k=CHROMA_K, warp=_turn("cornell", yaw=1.0, roll=5.0, size=size)))):
        for bicubic in (False, True):
            _, _, st = _run(r, orc_det, color, _frame(w, h), f"{w} x {h}, {what}", lenses=[R.make_lens(size, **kw)], border=BORDER, bicubic=bicubic)
            assert st["pixels"] == w * h and (what != "identity" or st["outside"] == 0)
    r.close()


# ------------------------------------------------------------------ 2. hostile but legal inputs
@pytest.mark.parametrize("bicubic", [False, True], ids=["bilinear", "bicubic"])
def test_hostile_but_legal_inputs(ptlib, orc_det, bicubic):
    c = _case("textured")
    run = lambda what, **kw: _run(c.r, orc_det, kw.pop("color", c.color), _frame(), what, border=BORDER, bicubic=bicubic, **kw)  # noqa: E731
    # a turn of 60 degrees under a horizontal half-angle of 35: c <= 0 over part of the frame, the rest lands outside or near the border
    ref, got, st = run("a turn by 60 degrees", lenses=[R.make_lens((W, H), warp=_turn(yaw=60.0))])
    behind = np.isnan(ref["sx"][:, 0])
    assert 0 < behind.sum() < W * H and st["outside"] > behind.sum() and (got["out"][..., 3].reshape(-1)[behind] == 0).all()
    assert (got["out"].view(f32)[..., 0:3].reshape(-1, 3)[behind] == np.asarray(BORDER, f32)).all()
    ref, got, st = run("a turn by 170 degrees", lenses=[R.make_lens((W, H), warp=_turn(yaw=170.0))])
    assert st["outside"] == W * H and np.isnan(ref["sx"]).all()
    # k at its limit: r2 * k overflows towards the corners, NaN and inf source points are outside
    for k in ((1e6, 1e6, 1e6), (-1e6, 1e6, -1e6), ((1e6, 0, 0), (0, -1e6, 0), (0, 0, 1e6))):
        ref, got, st = run(f"k = {k}", lenses=[R.make_lens((W, H), k=k, radius=1e-12)])
        assert st["outside"] > W * H - 8
    ref, got, st = run("inv_radius = 0", lenses=[R.make_lens((W, H), k=(1e6, -1e6, 1e6), radius=0.0)])
    assert st["outside"] == 0 and np.array_equal(got["out"].view(f32)[..., 0:3], c.color[..., 0:3])
    ref, got, st = run("inv_radius = 0 on one axis", lenses=[R.make_lens((W, H), k=(-0.2, 0.0, 0.0), radius=(0.0, 30.0))])
    assert np.array_equal(ref["sx"][ref["Y"] == 29, 0], ref["X"][ref["Y"] == 29] + f32(0.5)) and st["outside"] < W * H // 4  # r2 = 0 on the centre row only
    # NaN, inf and 3e38 bands in the colour
    color = c.color.copy()
    color[:, 20:23, 0] = NAN
    color[:, 40:42, 1] = INF
    color[:, 60:63, 2] = -INF
    color[10:12, :, 1] = NAN
    color[:, 80:83, 0] = f32(3e38)
    color[:, 100:102, :] = f32(-3e38)
    for lens in ("pincushion", "lens and matrix"):
        ref, got, st = run(f"bands, {lens}", color=color, lenses=[R.make_lens((W, H), **LENSES[lens]())])
        assert st["nonfinite"] > 1000
        if not bicubic:  # (a Catmull-Rom sum of 3e38s may overflow: the reference's bits, whatever they are; bilinear weights sum to 1)
            assert np.isfinite(got["out"].view(f32)).all()


# ------------------------------------------------------------------ 3. views, masks, partitions
def test_two_views_off_the_block_grid_with_different_lenses(ptlib, orc_det):
    c = _case("cornell")
    r = _renderer(c.model, (W, H), c.cam)
    rects = RECTS[:2]
    cams = [R.make_camera(c.cam, rects[0][2] / rects[0][3]), R.make_camera(dict(c.cam, fovY=c.cam["fovY"] * 1.3), rects[1][2] / rects[1][3])]
    r.setViews([(x, y, w, h, cam) for (x, y, w, h), cam in zip(rects, cams)])
    inside = np.zeros((H, W), bool)
    for x, y, w, h in rects:
        inside[y:y + h, x:x + w] = True
    size = lambda k: (rects[k][2], rects[k][3])  # noqa: E731
    lenses = [R.make_lens(size(0), k=(-0.3, 0.05, 0.0), warp=R.warpMatrix(cams[0], LW_turned_camera(cams[0], 2.0), size(0))),
              R.make_lens(size(1), k=CHROMA_K, center=(20.0, 9.5), warp=R.warpMatrix(cams[1], LW_turned_camera(cams[1], -4.0), size(1)))]
    color = np.random.default_rng(3).random((H, W, 4)).astype(f32)
    for bicubic in (False, True):
        ref, got, st = _run(r, orc_det, color, inside, "two views", lenses=lenses, rects=rects, border=BORDER, bicubic=bicubic)
        assert st["pixels"] == sum(w * h for _, _, w, h in rects) and 0 < st["outside"] < st["pixels"]
        assert all((got[n][~inside] == SENTINEL).all() for n in LW.PLANES)  # pixels in no view keep the sentinel
        assert (ref["sx"][ref["rid"] == 1, 0] != ref["sx"][ref["rid"] == 1, 2]).any()
        # no tap crosses a view's border: each view a constant colour, the rest of the frame a third one
        paint = np.full((H, W, 4), 9.0, f32)
        consts = (1.0, 3.0)
        for (x, y, w, h), v in zip(rects, consts):
            paint[y:y + h, x:x + w] = v
        ref, got, st = _run(r, orc_det, paint, inside, "two painted views", lenses=lenses, rects=rects, border=(5.0, 5.0, 5.0), bicubic=bicubic)
        for (x, y, w, h), v in zip(rects, consts):
            vals = got["out"].view(f32)[y:y + h, x:x + w, 0:3]
            assert ((np.abs(vals - v) <= 4e-6 * v) | (vals == 5.0)).all() and (np.abs(vals - v) <= 4e-6 * v).sum() > w * h
    with pytest.raises(ValueError, match="lenses must be 2 records"):
        r.lensWarpPlanes(_upload(color), lenses=lenses[:1])
    r.setViews([])
    r.setCamera(R.make_camera(c.cam, W / H))
    _run(r, orc_det, color, _frame(), "views dropped", lenses=[R.make_lens((W, H), **LENSES["lens and matrix"]())])
    r.close()


def LW_turned_camera(cam, yaw):
    t = LW.turned(dict(eye=cam.eye, lookat=cam.lookat, up=cam.up), yaw)
    return R.Camera(cam.eye, t["lookat"], t["up"], cam.fovY, cam.aspectRatio)


@pytest.mark.parametrize("bicubic", [False, True], ids=["bilinear", "bicubic"])
def test_block_mask_and_rank_1_of_3(ptlib, orc_det, bicubic):
    c = _case("textured")
    lenses = [R.make_lens((W, H), **LENSES["lens and matrix"]())]
    whole = LW.lens_warp_ref(c.color, [(0, 0, W, H)], lenses, _frame(), border=BORDER, bicubic=bicubic, planes=LW.PLANES, orc=orc_det)
    nby, nbx = c.r.blockGrid()
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.5
    mask[0, 0] = mask[nby - 1, nbx - 1] = mask[0, nbx - 1] = mask[nby - 1, 3] = True
    mask[1, 1] = False
    px = pixel_mask(mask, h=H, w=W)
    _, got, st = _run(c.r, orc_det, c.color, px, "a random block mask", lenses=lenses, mask=mask, border=BORDER, bicubic=bicubic)
    assert 0 < st["pixels"] < W * H and all((got[n][~px] == SENTINEL).all() for n in LW.PLANES)
    assert all(np.array_equal(got[n][px], whole[n][px]) for n in LW.PLANES)  # taps read pixels outside the set
    _, _, st = _run(c.r, orc_det, c.color, np.zeros((H, W), bool), "the empty mask", lenses=lenses, mask=np.zeros((nby, nbx), bool), border=BORDER, bicubic=bicubic)
    assert st == dict({k: 0 for k in COUNTERS}, kernel_ms=st["kernel_ms"])
    by, bx = np.mgrid[0:H, 0:W] // 8
    r = _renderer(c.model, (W, H), c.cam, partition=(1, 3, 8, 8))
    own = (bx + by) % 3 == 1
    _, got, st = _run(r, orc_det, c.color, own, "rank 1 of 3", lenses=lenses, border=BORDER, bicubic=bicubic)
    assert st["pixels"] == int(own.sum()) and all((got[n][~own] == SENTINEL).all() for n in LW.PLANES)
    assert all(np.array_equal(got[n][own], whole[n][own]) for n in LW.PLANES)
    r.close()


# ------------------------------------------------------------------ 4. what the output means
def test_warped_frame_is_closer_to_the_turned_cameras(ptlib):
    c = _case("textured")
    turned = LW.turned(c.cam, YAW)
    rb = _renderer(c.model, (W, H), turned)
    B = _albedo(rb, c.table)
    rb.close()
    A = c.color
    res = c.r.lensWarpPlanes(_upload(A), lenses=[R.make_lens((W, H), warp=R.warpMatrix(_row(c.cam), _row(turned), (W, H)))])
    out = _np(res["out"])
    ok = out[..., 3] == 1
    e0, e1 = LW.rms(A[..., 0:3][ok], B[..., 0:3][ok]), LW.rms(out[..., 0:3][ok], B[..., 0:3][ok])
    bound = (1 + R_WARP) / 2
    print(f"lens warp: rms(A - B) {e0:.6f}, rms(warp(A) - B) {e1:.6f}, ratio {e1 / e0:.5f} (the reference: {R_WARP}; asserted: <= {bound:.4f}); "
          f"outside {res['stats']['outside']} of {W * H}")
    assert res["stats"]["outside"] == int((~ok).sum()) <= W * H // 8
    assert e0 > 0.01 and e1 <= bound * e0


# ------------------------------------------------------------------ 5. refusals
def test_refusals(ptlib, orc_det):
    c = _case("textured")
    L = _lib.load_library()
    r = R.SampleRenderer(c.model)
    dev = dict(color=_upload(c.color))
    out = {n: _filled(n, H, W) for n in LW.PLANES}
    good = {n: t.data_ptr() for n, t in list(dev.items()) + list(out.items())}
    lens = (_lib.LensView * 1)(R.make_lens((W, H), **LENSES["lens and matrix"]()))
    good.update(flags=0, lenses=C.addressof(lens), border=(0.0, 0.0, 0.0))

    def refused(what, pattern, lens_words=None, **fields):
        d = _lib.LensWarpDesc()
        bad = (_lib.LensView * 1)(lens[0])
        for k, v in (lens_words or {}).items():
            C.cast(bad, C.POINTER(C.c_float))[k] = v
        for n, v in dict(good, **fields).items():
            if n == "border":
                d.border[0], d.border[1], d.border[2] = v
            else:
                setattr(d, n, C.addressof(bad) if n == "lenses" and lens_words else v)
        torch.cuda.synchronize()
        s = _lib.LensWarpStats(7, 7, 7, 7.0)
        rc = L.pt_lens_warp_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_lens_warp_planes: ") and pattern in msg, f"{what}: {msg!r}"
        assert tuple(getattr(s, n) for n, _ in s._fields_) == (7, 7, 7, 7.0)
        for n, t in out.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {n} was written"

    refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(c.cam, W / H))
    assert L.pt_lens_warp_planes(r._ctx, None, None) == -1 and "pt_lens_warp_planes: null description" in L.pt_last_error(r._ctx).decode()
    refused("a flag", "unknown flag bits 2", flags=2)
    refused("a flag beside the known one", "unknown flag bits 4", flags=5)
    refused("a flag comes before the planes", "unknown flag bits 8", flags=8, color=None)
    for k in range(3):
        for v in (float("nan"), float("inf"), -float("inf")):
            b = [0.0, 0.0, 0.0]
            b[k] = v
            refused(f"border[{k}] {v}", "border must be finite", border=tuple(b))
    refused("both outputs null", "no output asked for", out=None, frame_rgba8=None)
    refused("color null", "color is null", color=None)
    host = np.zeros((H, W, 4), f32)
    refused("a host pointer", "color is not device memory", color=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "out is not 4-byte aligned", out=good["out"] + 2)
    refused("a pointer offset by 1 byte", "frame_rgba8 is not 4-byte aligned", frame_rgba8=good["frame_rgba8"] + 1)
    hip = _hip_runtime()
    for name, nbytes in (("frame_rgba8", H * W * 4), ("out", H * W * 16)):
        raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert hip.hipMalloc(C.byref(raw), C.c_size_t(nbytes)) == 0
        try:
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= nbytes
            refused(f"{name} one element too small", f"{name} has fewer than {nbytes} bytes left", **{name: raw.value + size.value - (nbytes - 16)})
        finally:
            assert hip.hipFree(raw) == 0
    refused("in place", "color and out overlap", out=good["color"])
    refused("the frame inside the colour", "color and frame_rgba8 overlap", frame_rgba8=good["color"] + 16)
    refused("two outputs", "out and frame_rgba8 overlap", frame_rgba8=good["out"])
    # per view: words 0, 1 center; 2, 3 inv_radius; 4 .. 12 k; 13 .. 21 warp; 22, 23 reserved
    for k in (0, 3, 4, 12, 13, 21, 22, 23):
        for v in (float("nan"), float("inf")):
            refused(f"lens word {k} {v}", f"lenses[0]: word {k} is not finite", lens_words={k: v})
    refused("inv_radius < 0", "lenses[0]: inv_radius must be >= 0", lens_words={2: -1e-30})
    refused("inv_radius < 0", "lenses[0]: inv_radius must be >= 0", lens_words={3: -1.0})
    refused("a far centre", "lenses[0]: |center| must be <= 1e6", lens_words={1: -1.1e6})
    refused("a large k", "lenses[0]: |k| must be <= 1e6", lens_words={4: 1.000001e6})
    refused("a large k", "lenses[0]: |k| must be <= 1e6", lens_words={12: -2e6})
    refused("reserved", "lenses[0]: reserved must be 0", lens_words={22: 1.0})
    refused("reserved", "lenses[0]: reserved must be 0", lens_words={23: -1e-30})
    # the Python facade passes the library's refusals on; a valid call afterwards still works, into the same planes
    with pytest.raises(RuntimeError, match="border must be finite"):
        r.lensWarpPlanes(dev["color"], border=(0.0, float("nan"), 0.0))
    with pytest.raises(RuntimeError, match="color and out overlap"):
        r.lensWarpPlanes(dev["color"], out=dev["color"])
    res = r.lensWarpPlanes(dev["color"], out=out["out"], frame=out["frame_rgba8"], lenses=[lens[0]], border=BORDER)
    ref = LW.lens_warp_ref(c.color, [(0, 0, W, H)], [lens[0]], _frame(), border=BORDER, planes=LW.PLANES, orc=orc_det)
    _same({n: _bits(out[n]) for n in LW.PLANES}, ref, "a valid call after the refusals")
    assert res["stats"]["outside"] == ref["outside"] > 0
    r.close()


# ------------------------------------------------------------------ 6. state and the stream contract
def test_rendering_state_is_left_alone(ptlib):
    c = _case("cornell")
    probe = scenes.sky_probe(256, 128).BuildCDF()

    def run(with_call):
        r = R.SampleRenderer(scenes.cornell_box())
        r.setProbe(probe)
        r.setOptions(frames_in_flight=3)
        r.resize((W, H))
        r.setCamera(R.make_camera(c.cam, W / H))
        r.launchParams.samples_per_launch = 2
        for n in (0, 1):
            r.launchParams.frame.subframe_index = n
            r.render()
        if with_call:
            r.sync()
            before = r.stats()
            res = r.lensWarpPlanes(_upload(c.color), frame=_filled("frame_rgba8", H, W), lenses=[R.make_lens((W, H), **LENSES["lens and matrix"]())], bicubic=True)
            assert res["stats"]["outside"] > 0 and r.stats() == before
        r.launchParams.frame.subframe_index = 2
        r.render()
        r.sync()
        bufs = [r.download(n) for n in range(5)]
        r.close()
        return bufs

    for n, (x, y) in enumerate(zip(run(True), run(False))):
        assert x.tobytes() == y.tobytes(), f"buffer {n} differs after lensWarpPlanes between the frames"


@pytest.mark.parametrize("mode", ["default", "side"])
def test_under_a_busy_torch_stream(ptlib, orc_det, mode):
    """tests/test_gpu_stream_contract.py's protocol for this entry point: the colour is produced, and the two outputs sentinel-filled, by
    work still pending on torch's current stream when the call is made; the result equals the synchronous call's, and that equals the
    reference"""
    from stream_kit import _pin, _res

    c = _case("textured")
    outs = {n: _filled(n, H, W) for n in LW.PLANES}
    lenses = [R.make_lens((W, H), **LENSES["lens and matrix"]())]

    def call(dev, outs, returned):
        res = c.r.lensWarpPlanes(dev["color"], out=outs["out"], frame=outs["frame_rgba8"], lenses=lenses, border=BORDER)
        returned()
        return _res(res, outs)

    sync, got = _pin("lensWarpPlanes", mode, c.r, dict(color=c.color), outs, call)
    ref = LW.lens_warp_ref(c.color, [(0, 0, W, H)], lenses, _frame(), border=BORDER, planes=LW.PLANES, orc=orc_det)
    _same({n: got[n].view(np.uint32).reshape(H, W, -1) for n in LW.PLANES}, ref, f"under a busy stream [{mode}]")
    assert got["stats"] == {k: ref[k] for k in COUNTERS}


# ------------------------------------------------------------------ 7. the stereo example with --lens-warp
def _example():
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location("stereo_views", os.path.join(ROOT, "examples", "stereo_views.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def test_stereo_example_displays_the_warped_tone_mapped_pair(ptlib, orc_det, tmp_path):
    """examples/stereo_views.py's warp path at 128 x 56: the displayed frame is lensWarpPlanes of the tone-mapped one, per eye around the
    centre of its own rectangle; without the flag the example writes what it wrote"""
    ex = _example()
    ew, eh = 64, 56
    sample = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    sample.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    sample.launchParams.samples_per_launch = 2
    views = ex.stereo_views(scenes.TWO_BOX_CAMERA, ew, eh, 0.065)
    sample.resize((2 * ew, eh))
    sample.setViews(views)
    sample.render()
    lenses = ex.stereo_lenses(views, 0.22, 0.24, 0.015, 1.5)
    rows = [np.frombuffer(bytes(v), f32) for v in lenses]
    assert [tuple(v[0:2]) for v in rows] == [(ew / 2, eh / 2)] * 2 and all(v[4] < v[7] < v[10] for v in rows) and all(v[15] != 0 for v in rows)
    shown = ex.warp_display(sample, lenses)
    tm = sample.tonemapPlanes(sample.deviceBuffer(R.PT_BUF_COLOR), op="reinhard")["out"]
    assert np.array_equal(_bits(tm), _bits(shown["tonemapped"])) and _np(tm)[..., 0:3].max() > 0.1
    rects = [(x, y, w, h) for x, y, w, h, _ in views]
    ref = LW.lens_warp_ref(_np(tm), rects, lenses, _frame(2 * ew, eh), planes=("frame_rgba8",), orc=orc_det)
    assert np.array_equal(_bits(shown["frame_rgba8"]), ref["frame_rgba8"]) and shown["stats"]["outside"] == ref["outside"]
    assert 0 < ref["outside"] < 2 * ew * eh and not np.array_equal(_bits(shown["frame_rgba8"])[..., 0], sample.downloadPixels())
    sample.close()
    common = ["--eye-size", str(ew), str(eh), "--tile", "8", "--spp", "1", "--subframes", "1", "--npy"]
    (tmp_path / "plain").mkdir()
    (tmp_path / "warp").mkdir()
    ex.main(common + ["--out-dir", str(tmp_path / "plain")])
    ex.main(common + ["--out-dir", str(tmp_path / "warp"), "--lens-warp"])
    for name in ("stereo_pair.npy", "camera_atlas.npy"):
        assert np.array_equal(np.load(tmp_path / "plain" / name), np.load(tmp_path / "warp" / name)), name
    assert not (tmp_path / "plain" / "stereo_pair_warped.npy").exists()
    warped = np.load(tmp_path / "warp" / "stereo_pair_warped.npy")
    assert warped.shape == (eh, 2 * ew) and not np.array_equal(warped, np.load(tmp_path / "warp" / "stereo_pair.npy"))
