"""Motion blur (pt_motion_blur_layout, pt_motion_blur_planes) on the GPU.  out, every word of the scratch (T and N of every view) and every
counter are compared word for word with tests/motion_blur_ref.py — NumPy evaluating the header's rule — over WHOLE sentinel-filled
allocations: out as a whole plane (a word written outside the pixel set shows as a lost sentinel), the scratch exactly
pt_motion_blur_layout's bytes between guard words.  NaN words compare as NaN (payloads are not specified).  Frames are 131 x 59 and smaller."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_blur_ref as M
from gbuffer_ref import _moved, _row
from gpu_kit import filled, pixel_mask
from gpu_kit import bits3 as _bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from gpu_kit import words_differ as _differ
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from pass_cases import MOTION_INPUTS
from scene_kit import RECTS

pytestmark = pytest.mark.gpu

f32 = np.float32
u32 = np.uint32
W, H = 131, 59
GUARD = 2  # sentinel words on either side of the scratch: 8 bytes, so T and N stay 8-byte aligned
SENTINEL = M.SENTINEL
CAM = scenes.CORNELL_CAMERA
HOSTILE = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x80000000], u32).view(f32)


def _all(h=H, w=W):
    return np.ones((h, w), bool)


def _scratch(nbytes):
    """(the whole allocation as int32, the (texels, 2) float32 tensor inside it): sentinel-filled, GUARD words on either side"""
    n = nbytes // 4
    buf = torch.full((4 * (n + 2 * GUARD),), 0xA5, dtype=torch.uint8, device="cuda:0").view(torch.int32)
    t = buf[GUARD:GUARD + n].view(torch.float32).view(n // 2, 2)
    assert t.is_contiguous() and t.data_ptr() % 8 == 0
    return buf, t


def _planes(seed, h=H, w=W, hostile=True, speed=256.0):
    """hand-made planes: colours over ten stops with a random fourth word, depths in [1, 9] with steps, motion whose magnitude spreads
    from 0 to `speed` pixels (4 R of velocity at shutter 0.5 and R = 16) in every direction; with `hostile`, NaN, +-inf, denormals,
    +-FLT_MAX and -0 in each plane, and 3e38 motion of opposite signs"""
    rng = np.random.default_rng(seed)
    c = (np.exp2(rng.uniform(-6, 4, (h, w, 1))) * rng.uniform(0.4, 1.0, (h, w, 3))).astype(f32)
    c = np.concatenate([c, rng.uniform(0, 1, (h, w, 1)).astype(f32)], -1)
    z = (rng.uniform(1.0, 1.2, (h, w)) * np.where(rng.random((h, w)) < 0.3, 1.0, 6.0)).astype(f32)
    a = rng.uniform(0, 2 * np.pi, (h, w))
    mag = rng.uniform(0, 1, (h, w)) ** 3 * speed
    m = np.stack([np.cos(a) * mag, np.sin(a) * mag], -1).astype(f32)
    m[rng.random((h, w)) < 0.2] = 0
    if hostile and h * w >= 64:
        pos = rng.permutation(h * w)
        k = len(HOSTILE)
        for n, word in enumerate(HOSTILE):
            c.reshape(-1, 4)[pos[n], n % 3] = word
            m.reshape(-1, 2)[pos[k + n], n % 2] = word
            z.reshape(-1)[pos[2 * k + n]] = word
        m.reshape(-1, 2)[pos[3 * k]] = (3e38, -3e38)
        m.reshape(-1, 2)[pos[3 * k + 1]] = (-3e38, 3e38)
        z.reshape(-1)[pos[3 * k + 2:3 * k + 5]] = (0.0, -2.0, 1e-7)
    return c, m, z


def _blur(r, color, motion, depth, pixels, what, rects=None, mask=None, offset=False, **prm):
    """motionBlurPlanes into a sentinel-filled out plane and a guarded scratch of exactly pt_motion_blur_layout's bytes, against the
    reference: the layout, out over the whole frame, every word of the scratch, the six counters; color is unchanged afterwards.
    Returns (the reference, the scratch's words)"""
    h, w = depth.shape
    dims, nbytes = r.motionBlurLayout()
    rdims, rbytes = M.layout(rects, h, w)
    assert nbytes == rbytes and np.array_equal(dims, rdims), f"{what}: the layout is {dims.tolist()}, {nbytes} bytes; the reference {rdims.tolist()}, {rbytes}"
    dev = _upload(color, offset)
    out = filled((h, w, 4), offset)
    sbuf, scratch = _scratch(nbytes)
    res = r.motionBlurPlanes(dev, _upload(motion, offset), _upload(depth, offset), out=out, scratch=scratch, mask=mask, **prm)
    assert res["out"] is out and res["scratch"] is scratch
    ref = M.motion_blur_ref(color, motion, depth, pixels, rects, **prm)
    st = res["stats"]
    print(f"{what}: {({k: st[k] for k in M.COUNTERS})}, {st['kernel_ms']:.4f} ms")
    got = _bits(out)
    neq = _differ(got, ref["out"])
    assert got.shape == ref["out"].shape and not neq.any(), f"{what}: out differs in {int(neq.sum())} words, first at {np.argwhere(neq)[:3].tolist()}"
    words = _np(sbuf).view(u32)
    assert (words[:GUARD] == SENTINEL).all() and (words[-GUARD:] == SENTINEL).all(), f"{what}: a word outside the scratch was written"
    tn = words[GUARD:-GUARD]
    neq = _differ(tn, ref["scratch"])
    assert not neq.any(), f"{what}: the scratch differs in {int(neq.sum())} words, first in texel {int(np.argwhere(neq)[0, 0]) // 2} (layout {dims.tolist()})"
    assert {k: st[k] for k in M.COUNTERS} == {k: ref[k] for k in M.COUNTERS}, (what, st, {k: ref[k] for k in M.COUNTERS})
    assert np.array_equal(_np(dev).view(u32), np.ascontiguousarray(color, f32).view(u32)), f"{what}: color was written"
    return ref, tn


def _plain(size):
    """a renderer of the given size on the Cornell box; no frame is rendered"""
    return _renderer(scenes.cornell_box(), size, CAM)


def _set_views(r, rects, w, h):
    r.setViews([(x, y, ww, hh, R.make_camera(CAM, ww / hh)) for x, y, ww, hh in rects])
    inside = np.zeros((h, w), bool)
    for x, y, ww, hh in rects:
        inside[y:y + hh, x:x + ww] = True
    return inside


_CASES = {}


def _frame():
    """a W x H renderer and one set of hand-made planes, shared by the tests that only read them"""
    if "frame" not in _CASES:
        r = _plain((W, H))
        planes = _planes(1)
        for a in planes:
            a.setflags(write=False)
        _CASES["frame"] = (r, planes)
    return _CASES["frame"]


# ------------------------------------------------------------------ 1. sizes and parameters
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (15, 17), (16, 16), (17, 16), (33, 49), (131, 59)])
def test_sizes(ptlib, size):
    w, h = size
    r = _plain(size)
    c, m, z = _planes(w * 100 + h, h, w)
    ref, _ = _blur(r, c, m, z, _all(h, w), f"{w} x {h}")
    assert ref["sources"] == w * h == ref["pixels"]
    if w * h > 64:
        assert 0 < ref["moving"] and 0 < ref["taps"] and ref["unknown"] == 4
    _blur(r, c, m, z, _all(h, w), f"{w} x {h}, jitter, 5 taps", taps=5, jitter=True, seed=9)
    r.close()


@pytest.mark.parametrize("prm", [dict(taps=1), dict(taps=2), dict(taps=64), dict(max_blur=1.0), dict(max_blur=7.3), dict(shutter=0.0), dict(shutter=4.0),
                                 dict(depth_soft=1.0), dict(depth_soft=1e-3), dict(jitter=True, seed=1), dict(jitter=True, seed=0xFFFFFFFF)],
                         ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()))
def test_the_parameters(ptlib, prm):
    r, (c, m, z) = _frame()
    ref, tn = _blur(r, c, m, z, _all(), f"{prm}", **prm)
    if prm.get("shutter") == 0.0:
        assert ref["moving"] == 0 and (tn.view(f32) == 0).all()
    if "seed" in prm:
        other, _ = _blur(r, c, m, z, _all(), f"{prm}, seed 2", **dict(prm, seed=2))
        assert _differ(other["out"], ref["out"]).any()


def test_every_plane_one_float_into_its_allocation(ptlib):
    r, (c, m, z) = _frame()
    _blur(r, c, m, z, _all(), "every plane 4 bytes off a 16-byte boundary", offset=True)


def test_ties_go_to_the_first(ptlib):
    """equal l2 at several pixels of a tile (the four axis directions and a diagonal of the same length are not available exactly, so the
    same vector with different signs), and equal maxima in several tiles of a neighbourhood: the first in row order wins both times"""
    w, h = 48, 48
    r = _plain((w, h))
    c, _, z = _planes(5, h, w, hostile=False)
    m = np.zeros((h, w, 2), f32)
    for k, (y, x, v) in enumerate([(3, 9, (24.0, 8.0)), (3, 10, (-24.0, 8.0)), (7, 2, (8.0, 24.0)), (15, 15, (-8.0, -24.0)),       # tile (0, 0)
                                   (20, 40, (8.0, -24.0)), (20, 41, (24.0, 8.0)),                                               # tile (2, 1)
                                   (40, 5, (-24.0, -8.0)), (33, 6, (8.0, 24.0)),                                                # tile (0, 2)
                                   (47, 47, (24.0, -8.0))]):                                                                    # tile (2, 2)
        m[y, x] = v
    ref, _ = _blur(r, c, m, z, _all(h, w), "ties")
    T, N = ref["T"][0], ref["N"][0]
    assert T[0, 0].tolist() == [6.0, 2.0] and T[1, 2].tolist() == [2.0, -6.0] and T[2, 0].tolist() == [2.0, 6.0] and T[2, 2].tolist() == [6.0, -2.0]
    assert N[1, 1].tolist() == [6.0, 2.0] and N[2, 1].tolist() == [2.0, -6.0] and N[0, 2].tolist() == [2.0, -6.0]
    _blur(r, c, m, z, _all(h, w), "ties, clamped to max_blur 4", max_blur=4.0)
    r.close()


def test_one_fast_pixel_in_the_corner_tile(ptlib):
    """the last pixel of a partial corner tile of 33 x 49 moves: its tile and the three around it gather, the rest keeps its colour"""
    w, h = 33, 49
    r = _plain((w, h))
    c, _, z = _planes(6, h, w, hostile=False)
    m = np.zeros((h, w, 2), f32)
    m[48, 32] = (-40.0, 55.0)
    ref, tn = _blur(r, c, m, z, _all(h, w), "one fast pixel")
    assert ref["moving"] == (33 - 16) * (49 - 32) and (ref["T"][0][:3, :2] == 0).all() and (ref["N"][0][:2] == 0).all()
    r.close()


def test_a_constant_colour_under_uniform_motion(ptlib):
    """tests/test_motion_blur_cabi.py's case on the GPU: the word-for-word comparison, and the bound of (2 taps + 3) roundings derived there"""
    r, (_, _, z) = _frame()
    c = np.empty((H, W, 4), f32)
    c[:] = (0.7310, 1.9125, 0.0421, 1.0)
    m = np.empty((H, W, 2), f32)
    m[:] = (13.7, -6.1)
    ref, _ = _blur(r, c, m, np.where(np.isfinite(z) & (z > 0), z, f32(3.0)).astype(f32), _all(), "constant colour", taps=8)
    out = ref["out"].view(f32)[..., 0:3].astype(np.float64)
    assert (np.abs(out - c[..., 0:3]) <= (2 * 8 + 3) * 2.0 ** -24 * c[..., 0:3]).all()


# ------------------------------------------------------------------ 2. a real frame
def _two_box():
    """the two-box scene of pass_cases.MOTION_INPUTS after a camera move and transformMeshes: the colour from the frame path, depth and the
    camera's motion from renderGBuffer, the moved mesh's motion from motionPlanes.  Built once; read-only."""
    if "two_box" not in _CASES:
        make, cam, mesh, A = MOTION_INPUTS["two_box"]
        prev = _moved(cam)
        r = R.SampleRenderer(make())
        r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
        r.resize((W, H))
        r.setCamera(R.make_camera(prev, W / H))
        snapshot = r.copyVerticesDevice()
        r.transformMeshes({mesh: A})
        r.setCamera(R.make_camera(cam, W / H))
        r.launchParams.samples_per_launch = 2
        r.launchParams.frame.subframe_index = 0
        r.render()
        r.sync()
        color = r.download(R.PT_BUF_ACCUM).astype(f32).reshape(H, W, 4)
        row = _row(prev, W / H)
        g = r.renderGBuffer(("hit", "depth", "motion"), prev_cameras=row)
        mp = r.motionPlanes(g["hit"], snapshot, prev_cameras=row, planes=("motion",))
        planes = dict(color=color, depth=_np(g["depth"]), camera_motion=_np(g["motion"]), motion=_np(mp["motion"]))
        for a in planes.values():
            a.setflags(write=False)
        _CASES["two_box"] = (r, planes)
    return _CASES["two_box"]


def test_two_box_frame_from_the_real_chain(ptlib):
    r, p = _two_box()
    assert np.isfinite(p["color"]).all() and not np.array_equal(p["motion"], p["camera_motion"])
    for name in ("motion", "camera_motion"):
        for prm in (dict(shutter=0.5), dict(shutter=4.0, taps=24), dict(shutter=1.0, jitter=True, seed=4)):
            ref, _ = _blur(r, p["color"], p[name], p["depth"], _all(), f"two-box, {name}, {prm}", **prm)
            assert ref["sources"] == W * H
            if prm["shutter"] == 4.0:
                assert 0 < ref["moving"] and 0 < ref["taps"]


# ------------------------------------------------------------------ 3. views, masks, partitions
def test_two_views_of_odd_sizes_hold_a_standalone_frames_bits(ptlib):
    r = _plain((W, H))
    rects = RECTS[:2]
    inside = _set_views(r, rects, W, H)
    c, m, z = _planes(11)
    prm = dict(jitter=True, seed=3, taps=9)
    ref, _ = _blur(r, c, m, z, inside, "two views", rects=rects, **prm)
    assert ref["sources"] == sum(w * h for _, _, w, h in rects) == ref["pixels"]
    for x0, y0, wr, hr in rects:
        box = (slice(y0, y0 + hr), slice(x0, x0 + wr))
        alone = _plain((wr, hr))
        one, _ = _blur(alone, c[box], m[box], z[box], _all(hr, wr), f"a frame of {wr} x {hr}", **prm)
        assert not _differ(ref["out"][box], one["out"]).any()
        alone.close()
    r.setViews([])
    r.setCamera(R.make_camera(CAM, W / H))
    _blur(r, c, m, z, _all(), "views dropped")
    r.close()


def test_sixteen_views(ptlib):
    """16 views of 8 x 8 in a 32 x 32 frame: one launch, blockIdx.y the view, one partial tile each"""
    r = _plain((32, 32))
    rects = [(8 * i, 8 * j, 8, 8) for j in range(4) for i in range(4)]
    inside = _set_views(r, rects, 32, 32)
    c, m, z = _planes(13, 32, 32)
    ref, _ = _blur(r, c, m, z, inside, "16 views", rects=rects, taps=6)
    assert ref["sources"] == 1024
    r.close()


def test_a_view_puts_nothing_into_its_neighbour(ptlib):
    """tests/test_motion_blur_cabi.py's seam case: the right view's T and N are zero, its pixels come back as they were"""
    h, w = 32, 64
    rects = [(0, 0, 32, 32), (32, 0, 32, 32)]
    r = _plain((w, h))
    inside = _set_views(r, rects, w, h)
    c, _, z = _planes(12, h, w, hostile=False)
    c[8:24, 24:32, 0:3] = 500.0
    m = np.zeros((h, w, 2), f32)
    m[8:24, 24:32] = (-30.0, 4.0)
    ref, tn = _blur(r, c, m, z, inside, "the seam", rects=rects)
    first = int(r.motionBlurLayout()[0][1, 2])
    assert (tn[2 * first:] == 0).all() and (tn[:2 * first] != 0).any()
    assert np.array_equal(ref["out"][:, 32:, 0:3], c[:, 32:, 0:3].view(u32)) and ref["moving"] > 0
    r.close()


def test_masks_write_their_blocks_and_read_every_pixel(ptlib):
    r, (c, m, z) = _frame()
    nby, nbx = r.blockGrid()
    _, whole = _blur(r, c, m, z, _all(), "no mask")
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.5
    mask[0, 0] = mask[nby - 1, nbx - 1] = True
    mask[1, 1] = False
    ref, tn = _blur(r, c, m, z, pixel_mask(mask, h=H, w=W), "a random block mask", mask=mask)
    assert 0 < ref["pixels"] < W * H and ref["sources"] == W * H and np.array_equal(tn, whole)
    ref, tn = _blur(r, c, m, z, np.zeros((H, W), bool), "the empty mask", mask=np.zeros((nby, nbx), bool))
    assert ref["pixels"] == 0 and ref["sources"] == W * H and ref["moving"] == 0 and np.array_equal(tn, whole)


def test_partitions_gather_their_own_pixels(ptlib):
    r, (c, m, z) = _frame()
    ref, whole = _blur(r, c, m, z, _all(), "unpartitioned")
    by, bx = np.mgrid[0:H, 0:W] // 8
    union = np.full((H, W, 4), SENTINEL, u32)
    model = scenes.cornell_box()
    for rank in range(3):
        rr = _renderer(model, (W, H), CAM, partition=(rank, 3, 8, 8))
        own = (bx + by) % 3 == rank
        part, tn = _blur(rr, c, m, z, own, f"rank {rank} of 3")
        assert part["pixels"] == int(own.sum()) and part["sources"] == W * H and np.array_equal(tn, whole)
        assert (union[own] == SENTINEL).all()
        union[own] = part["out"][own]
        rr.close()
    assert not _differ(union, ref["out"]).any()


# ------------------------------------------------------------------ 4. refusals
def test_refusals(ptlib):
    L = _lib.load_library()
    r = R.SampleRenderer(scenes.cornell_box())
    c, m, z = _planes(1)
    color, motion, depth = _upload(c), _upload(m), _upload(z)
    out = filled((H, W, 4))
    nbytes = M.layout(None, H, W)[1]
    sbuf, scratch = _scratch(nbytes)
    good = dict(color=color.data_ptr(), motion=motion.data_ptr(), depth=depth.data_ptr(), out=out.data_ptr(), scratch=scratch.data_ptr(), shutter=0.5,
                max_blur=16.0, depth_soft=0.05, taps=12, seed=0, flags=0)

    def untouched(what):
        assert (_np(sbuf).view(u32) == SENTINEL).all(), f"{what}: the scratch was written"
        assert (_bits(out) == SENTINEL).all(), f"{what}: out was written"

    def refused(what, pattern, **fields):
        d = _lib.MotionBlurDesc()
        for n, v in dict(good, **fields).items():
            setattr(d, n, v)
        torch.cuda.synchronize()
        s = _lib.MotionBlurStats(7, 7, 7, 7, 7, 7, 7.0)
        rc = L.pt_motion_blur_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_motion_blur_planes") and pattern in msg, f"{what}: {msg!r}"
        assert tuple(getattr(s, n) for n, _ in s._fields_) == (7, 7, 7, 7, 7, 7, 7.0)
        untouched(what)

    def layout_refused(what, pattern, with_bytes=True):
        nb = C.c_size_t(77)
        dims = np.full(4, 9, u32)
        rc = L.pt_motion_blur_layout(r._ctx, dims.ctypes.data, C.byref(nb) if with_bytes else None)
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1 and msg.startswith("pt_motion_blur_layout") and pattern in msg, f"{what}: {rc}, {msg!r}"
        assert nb.value == 77 and (dims == 9).all(), f"{what}: an output was written"

    refused("no resize yet", "pt_resize")
    layout_refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(CAM, W / H))
    layout_refused("bytes null", "bytes is null", with_bytes=False)
    nb = C.c_size_t(0)
    assert L.pt_motion_blur_layout(r._ctx, None, C.byref(nb)) == 0 and nb.value == nbytes  # dims may be NULL
    assert L.pt_motion_blur_planes(r._ctx, None, None) == -1 and "pt_motion_blur_planes: null description" in L.pt_last_error(r._ctx).decode()
    refused("an unknown flag", "unknown flag bits 2", flags=3)
    refused("an unknown flag", "unknown flag bits 2147483648", flags=0x80000000)
    for bad in (0, 65, 0xFFFFFFFF):
        refused(f"taps {bad}", f"taps must be 1..64, not {bad}", taps=bad)
    for bad in (-0.5, 4.5, float("nan"), float("inf")):
        refused(f"shutter {bad}", "shutter must be finite and in [0,4]", shutter=bad)
    for bad in (0.5, 16.5, float("nan"), float("inf")):
        refused(f"max_blur {bad}", "max_blur must be finite and in [1,16]", max_blur=bad)
    for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        refused(f"depth_soft {bad}", "depth_soft must be finite and in (0,1]", depth_soft=bad)
    for name in ("color", "motion", "depth", "out", "scratch"):
        refused(f"{name} null", f"{name} is null", **{name: None})
    host = np.zeros((H, W, 4), f32)
    refused("a host pointer", "color is not device memory", color=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "out is not 4-byte aligned", out=good["out"] + 2)
    refused("the scratch 4 bytes off", "scratch is not 8-byte aligned", scratch=good["scratch"] - 4)
    refused("out exactly color", "color and out overlap", out=good["color"])
    big = torch.zeros(2 * H * W * 4 + 8, dtype=torch.float32, device="cuda:0")
    refused("out offset against the colour", "color and out overlap", color=big.data_ptr(), out=big.data_ptr() + 16)
    refused("out is the motion plane", "motion and out overlap", motion=big.data_ptr(), out=big.data_ptr())
    refused("out inside the depth plane", "depth and out overlap", depth=big.data_ptr() + 64, out=big.data_ptr())
    refused("the scratch inside the colour", "color and scratch overlap", scratch=good["color"] + 16)
    refused("the scratch inside the motion", "motion and scratch overlap", scratch=good["motion"] + 16)
    refused("the scratch inside the depth", "depth and scratch overlap", scratch=good["depth"] + 16)
    refused("the scratch inside out", "out and scratch overlap", scratch=good["out"] + 32)
    hip = _hip_runtime()
    for name, nb in (("scratch", nbytes), ("out", H * W * 16)):
        raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert hip.hipMalloc(C.byref(raw), C.c_size_t(nb)) == 0
        try:
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= nb
            refused(f"{name} one element too small", f"{name} has fewer than {nb} bytes left", **{name: raw.value + size.value - (nb - 16)})
        finally:
            assert hip.hipFree(raw) == 0
    # the Python facade passes the library's refusals on; a valid call afterwards works, into the same arrays
    with pytest.raises(RuntimeError, match="color and out overlap"):
        r.motionBlurPlanes(color, motion, depth, out=color)
    with pytest.raises(ValueError, match=r"scratch: a contiguous torch.float32 tensor of shape \(%d, 2\) is expected" % (nbytes // 8)):
        r.motionBlurPlanes(color, motion, depth, scratch=torch.zeros((nbytes // 8 + 1, 2), device="cuda:0"))
    res = r.motionBlurPlanes(color, motion, depth, out=out, scratch=scratch)
    ref = M.motion_blur_ref(c, m, z, _all())
    assert not _differ(_bits(out), ref["out"]).any() and not _differ(_np(sbuf).view(u32)[GUARD:-GUARD], ref["scratch"]).any()
    assert {k: res["stats"][k] for k in M.COUNTERS} == {k: ref[k] for k in M.COUNTERS}
    r.close()


def test_rendering_state_is_left_alone(ptlib):
    c, m, z = _planes(1)
    probe = scenes.sky_probe(256, 128).BuildCDF()

    def run(with_call):
        r = R.SampleRenderer(scenes.cornell_box())
        r.setProbe(probe)
        r.setOptions(frames_in_flight=3)
        r.resize((W, H))
        r.setCamera(R.make_camera(CAM, W / H))
        r.launchParams.samples_per_launch = 2
        for n in (0, 1):
            r.launchParams.frame.subframe_index = n
            r.render()
        if with_call:
            r.sync()
            before = r.stats()
            b = r.motionBlurPlanes(_upload(c), _upload(m), _upload(z))
            assert b["stats"]["pixels"] == W * H and r.stats() == before
        r.launchParams.frame.subframe_index = 2
        r.render()
        r.sync()
        bufs = [r.download(n) for n in range(5)]
        r.close()
        return bufs

    for n, (x, y) in enumerate(zip(run(True), run(False))):
        assert x.tobytes() == y.tobytes(), f"buffer {n} differs after motionBlurPlanes between the frames"


# ------------------------------------------------------------------ 5. the stream contract
@pytest.mark.parametrize("mode", ["default", "side"])
def test_under_a_busy_torch_stream(ptlib, mode):
    """tests/test_gpu_stream_contract.py's protocol: the inputs are produced, and the outputs sentinel-filled, by work still pending on
    torch's current stream when the call is made; the result equals the synchronous call's, and that equals the reference"""
    from stream_kit import _pin, _res

    r, (c, m, z) = _frame()
    nbytes = r.motionBlurLayout()[1]
    outs = dict(out=filled((H, W, 4)), scratch=torch.zeros((nbytes // 8, 2), dtype=torch.float32, device="cuda:0"))

    def blur(dev, outs, returned):
        res = r.motionBlurPlanes(dev["color"], dev["motion"], dev["depth"], out=outs["out"], scratch=outs["scratch"])
        returned()
        return _res(res, outs)

    sync, got = _pin("motionBlurPlanes", mode, r, dict(color=c, motion=m, depth=z), outs, blur)
    ref = M.motion_blur_ref(c, m, z, _all())
    assert not _differ(got["out"].view(u32).reshape(H, W, 4), ref["out"]).any(), f"out under a busy stream [{mode}]"
    assert not _differ(got["scratch"].view(u32).reshape(-1), ref["scratch"]).any(), f"the scratch under a busy stream [{mode}]"
    assert got["stats"] == {k: ref[k] for k in M.COUNTERS}


# ------------------------------------------------------------------ 6. the example loops with --motion-blur
def _example(name):
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def _main(ex, argv):
    import sys

    old = sys.argv
    sys.argv = argv
    try:
        ex.main()
    finally:
        sys.argv = old


def test_moving_geometry_loop_blurs_the_moved_box(ptlib, tmp_path, capsys):
    ex = _example("moving_geometry_loop")
    _main(ex, ["moving_geometry_loop.py", "--size", "128", "56", "--frames", "3", "--motion-blur", "--shutter", "2.0", "--blur-taps", "8", "--out-dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert out.count("motion blur ") == 3 and "moving_blurred.npy" in out
    filtered, blurred = np.load(tmp_path / "moving_filtered.npy"), np.load(tmp_path / "moving_blurred.npy")
    assert blurred.shape == (56, 128, 4) and (blurred[..., 3] == 1).all() and np.isfinite(blurred).all()
    assert not np.array_equal(blurred[..., 0:3], filtered[..., 0:3])
    frame = np.load(tmp_path / "moving_frame.npy")
    assert frame.shape == (56, 128) and (frame >> 24 == 255).all() and len(np.unique(frame)) > 50


def test_upsampled_loop_with_motion_blur_displays_the_blurred_frame(ptlib):
    """examples/upsampled_svgf_loop.py's UpsampledLoop with motion_blur at 128 x 56, scale 2: the blurred plane is motionBlurPlanes of the
    final one under the full-resolution G-buffer's motion and depth, and the displayed frame is tonemapPlanes of it"""
    import surface_ref as S

    ex = _example("upsampled_svgf_loop")
    w, h = 128, 56
    probe = scenes.sky_probe(256, 128).BuildCDF()
    cam0 = dict(eye=(2.0, 0.35, -3.0), lookat=(0.0, 0.2, 0.5), up=(0.0, 1.0, 0.0), fovY=35.0)
    up = ex.UpsampledLoop(S.textured_scene(), (w, h), 2, probe=probe, motion_blur=True, shutter=2.0, blur_taps=8)
    cam = R.make_camera(cam0, w / h)
    for k in range(3):
        prev, cam = cam, R.make_camera(ex.orbit(cam0, 0.02 * k), w / h)
        x = up.frame(k, prev, cam)
        assert x["pixels"] == w * h and x["motion_blur_ms"] > 0 and x["tonemap_ms"] > 0
    assert x["moving"] > 0
    ref = M.motion_blur_ref(_np(up.final), _np(up.hi_gbuf["motion"]), _np(up.hi_gbuf["depth"]), _all(h, w), shutter=2.0, taps=8)
    assert not _differ(_bits(up.blurred), ref["out"]).any() and x["moving"] == ref["moving"]
    want = up.hi.tonemapPlanes(up.blurred, frame=torch.zeros((h, w), dtype=torch.int32, device="cuda:0"), op="linear", write_out=False)
    assert np.array_equal(_np(up.frame_rgba8), _np(want["frame_rgba8"]))
    up.close()


def test_adaptive_albedo_loop_runs_with_motion_blur(ptlib, tmp_path, capsys):
    ex = _example("adaptive_svgf_albedo_loop")
    _main(ex, ["adaptive_svgf_albedo_loop.py", "--size", "128", "56", "--frames", "3", "--motion-blur", "--shutter", "2.0", "--blur-taps", "8", "--edge-aa", "--bloom",
               "--bloom-levels", "4", "--auto-exposure", "--out-dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert out.count("motion blur ") >= 3 and "tone map" in out
    blurred = np.load(tmp_path / "adaptive_svgf_albedo_blurred.npy")
    assert blurred.shape == (56, 128, 4) and (blurred[..., 3] == 1).all()
    frame = np.load(tmp_path / "adaptive_svgf_albedo_frame.npy")
    assert frame.shape == (56, 128) and (frame >> 24 == 255).all() and len(np.unique(frame)) > 50
