"""Depth of field (pt_dof_layout, pt_dof_planes) on the GPU.  out, every word of the scratch (T and N of every view) and every counter are
compared word for word with tests/dof_ref.py — NumPy evaluating the header's rule — over WHOLE sentinel-filled allocations: out as a whole
plane (a word written outside the pixel set shows as a lost sentinel), the scratch exactly pt_dof_layout's bytes between guard words.  NaN
words compare as NaN (payloads are not specified).  Frames are 131 x 59 and smaller."""
import ctypes as C

import numpy as np
import pytest
import torch

import dof_ref as M
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
GUARD = 2  # sentinel words on either side of the scratch
SENTINEL = M.SENTINEL
CAM = scenes.CORNELL_CAMERA
FOCUS = 3.0
LENS = dict(focus=FOCUS, aperture=3.0)
HOSTILE = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x80000000], u32).view(f32)


def _all(h=H, w=W):
    return np.ones((h, w), bool)


def _scratch(nbytes, offset=False):
    """(the whole allocation as int32, the (floats,) float32 tensor inside it): sentinel-filled, GUARD words on either side (one more in
    front with `offset`: the scratch then starts 4 bytes off an 8-byte boundary)"""
    n = nbytes // 4
    lead = GUARD + (1 if offset else 0)
    buf = torch.full((4 * (n + lead + GUARD),), 0xA5, dtype=torch.uint8, device="cuda:0").view(torch.int32)
    t = buf[lead:lead + n].view(torch.float32)
    assert t.is_contiguous() and t.data_ptr() % 4 == 0
    return buf, t, lead


def _planes(seed, h=H, w=W, hostile=True):
    """hand-made planes: colours over ten stops with a random fourth word, depths spread log-uniformly from 0.1 to 100 times FOCUS with a
    tenth of them exactly in focus; with `hostile`, NaN, +-inf, denormals, +-FLT_MAX and -0 in each plane, and 0, negative and tiny
    depths"""
    rng = np.random.default_rng(seed)
    c = (np.exp2(rng.uniform(-6, 4, (h, w, 1))) * rng.uniform(0.4, 1.0, (h, w, 3))).astype(f32)
    c = np.concatenate([c, rng.uniform(0, 1, (h, w, 1)).astype(f32)], -1)
    z = (FOCUS * np.exp(rng.uniform(np.log(0.1), np.log(100.0), (h, w)))).astype(f32)
    z[rng.random((h, w)) < 0.1] = FOCUS
    if hostile and h * w >= 64:
        pos = rng.permutation(h * w)
        k = len(HOSTILE)
        for n, word in enumerate(HOSTILE):
            c.reshape(-1, 4)[pos[n], n % 3] = word
            z.reshape(-1)[pos[k + n]] = word
        z.reshape(-1)[pos[2 * k:2 * k + 3]] = (0.0, -2.0, 1e-7)
    return c, z


def _dof(r, color, depth, pixels, what, rects=None, mask=None, offset=False, **prm):
    """dofPlanes into a sentinel-filled out plane and a guarded scratch of exactly pt_dof_layout's bytes, against the reference: the
    layout, out over the whole frame, every word of the scratch, the five counters; color and depth are unchanged afterwards.
    Returns (the reference, the scratch's words)"""
    prm = dict(LENS, **prm)
    h, w = depth.shape
    dims, nbytes = r.dofLayout()
    rdims, rbytes = M.layout(rects, h, w)
    assert nbytes == rbytes and np.array_equal(dims, rdims), f"{what}: the layout is {dims.tolist()}, {nbytes} bytes; the reference {rdims.tolist()}, {rbytes}"
    dev, zdev = _upload(color, offset), _upload(depth, offset)
    out = filled((h, w, 4), offset)
    sbuf, scratch, lead = _scratch(nbytes, offset)
    res = r.dofPlanes(dev, zdev, out=out, scratch=scratch, mask=mask, **prm)
    assert res["out"] is out and res["scratch"] is scratch
    ref = M.dof_ref(color, depth, pixels, rects, **prm)
    st = res["stats"]
    print(f"{what}: {({k: st[k] for k in M.COUNTERS})}, {st['kernel_ms']:.4f} ms")
    got = _bits(out)
    neq = _differ(got, ref["out"])
    assert got.shape == ref["out"].shape and not neq.any(), f"{what}: out differs in {int(neq.sum())} words, first at {np.argwhere(neq)[:3].tolist()}"
    words = _np(sbuf).view(u32)
    assert (words[:lead] == SENTINEL).all() and (words[-GUARD:] == SENTINEL).all(), f"{what}: a word outside the scratch was written"
    tn = words[lead:-GUARD]
    neq = _differ(tn, ref["scratch"])
    assert not neq.any(), f"{what}: the scratch differs in {int(neq.sum())} words, first in texel {int(np.argwhere(neq)[0, 0])} (layout {dims.tolist()})"
    assert {k: st[k] for k in M.COUNTERS} == {k: ref[k] for k in M.COUNTERS}, (what, st, {k: ref[k] for k in M.COUNTERS})
    assert np.array_equal(_np(dev).view(u32), np.ascontiguousarray(color, f32).view(u32)), f"{what}: color was written"
    assert np.array_equal(_np(zdev).view(u32), np.ascontiguousarray(depth, f32).view(u32)), f"{what}: depth was written"
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
    c, z = _planes(w * 100 + h, h, w)
    ref, _ = _dof(r, c, z, _all(h, w), f"{w} x {h}")
    assert ref["sources"] == w * h == ref["pixels"]
    if w * h > 64:
        assert 0 < ref["gathered"] and 0 < ref["taps"] and 0 < ref["nonfinite"]
    _dof(r, c, z, _all(h, w), f"{w} x {h}, jitter, 5 taps", taps=5, jitter=True, seed=9)
    r.close()


@pytest.mark.parametrize("prm", [dict(taps=1), dict(taps=2), dict(taps=5), dict(taps=8), dict(taps=16), dict(taps=33), dict(taps=64),
                                 dict(max_radius=1.0), dict(max_radius=4.0), dict(max_radius=7.3), dict(max_radius=16.0, aperture=40.0),
                                 dict(aperture=0.0), dict(aperture=-0.0), dict(aperture=0.3), dict(aperture=4096.0), dict(focus=1e30), dict(focus=1e-3),
                                 dict(jitter=True, seed=1), dict(jitter=True, seed=0xFFFFFFFF)],
                         ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()))
def test_the_parameters(ptlib, prm):
    r, (c, z) = _frame()
    ref, tn = _dof(r, c, z, _all(), f"{prm}", **prm)
    if prm.get("aperture") == 0.0:
        assert ref["gathered"] == 0 and (tn == 0).all()
    if prm.get("aperture") == 0.3:  # the far limit is K = 0.3: with nothing nearer than the focus no radius exceeds 0.5 and no tile gathers
        far = np.where(z < f32(FOCUS), f32(FOCUS), z).astype(f32)  # (a NaN stays: it counts as far)
        ref, tn = _dof(r, c, far, _all(), f"{prm}, nothing nearer than the focus", **prm)
        assert ref["gathered"] == 0 and tn.view(f32).max() == f32(0.3)
    if "seed" in prm:
        other, _ = _dof(r, c, z, _all(), f"{prm}, seed 2", **dict(prm, seed=2))
        assert _differ(other["out"], ref["out"]).any()


def test_every_plane_one_float_into_its_allocation(ptlib):
    r, (c, z) = _frame()
    _dof(r, c, z, _all(), "every plane 4 bytes off a 16-byte boundary, the scratch 4 bytes off an 8-byte one", offset=True)


def test_equal_maxima(ptlib):
    """the same radius at several pixels of a tile and in several tiles of a neighbourhood: the maximum is that radius whatever the order"""
    w, h = 48, 48
    r = _plain((w, h))
    c, _ = _planes(5, h, w, hostile=False)
    z = np.full((h, w), FOCUS, f32)
    for y, x in [(3, 9), (3, 10), (7, 2), (15, 15), (20, 40), (20, 41), (40, 5), (33, 6), (47, 47)]:
        z[y, x] = 0.5
    ref, _ = _dof(r, c, z, _all(h, w), "equal maxima", aperture=1.0)
    T, N = ref["T"][0], ref["N"][0]
    assert T[0, 0] == 5.0 == T[1, 2] == T[2, 0] == T[2, 2] and T[1, 1] == 0 and (N == 5.0).all()
    r.close()


def test_one_far_pixel_in_the_corner_tile(ptlib):
    """the last pixel of a partial corner tile of 33 x 49 is a miss in a frame otherwise in focus: its tile and the three around it gather,
    the rest keeps its colour"""
    w, h = 33, 49
    r = _plain((w, h))
    c, _ = _planes(6, h, w, hostile=False)
    z = np.full((h, w), FOCUS, f32)
    z[48, 32] = np.inf
    ref, tn = _dof(r, c, z, _all(h, w), "one far pixel")
    assert ref["gathered"] == (33 - 16) * (49 - 32) and (ref["T"][0][:3, :2] == 0).all() and (ref["N"][0][:2] == 0).all() and ref["T"][0][3, 2] == 3.0
    r.close()


def _rect_scene(z_rect, z_back):
    c = np.zeros((H, W, 4), f32)
    c[..., 0:3] = (0.0, 0.25, 0.5)
    z = np.full((H, W), z_back, f32)
    rect = np.zeros((H, W), bool)
    rect[12:30, 20:45] = True
    c[rect, 0:3] = (1.0, 0.5, 0.0)
    z[rect] = z_rect
    return c, z, rect


def test_sharp_and_blurred_foreground_rectangles(ptlib):
    """tests/test_dof_cabi.py's two scenes on the GPU: word for word, and the properties derived there"""
    r, _ = _frame()
    c, z, rect = _rect_scene(2.0, 50.0)
    ref, _ = _dof(r, c, z, _all(), "a sharp foreground", focus=2.0, aperture=11.25, taps=16)
    assert np.array_equal(ref["out"][rect][:, 0:3], c[rect][:, 0:3].view(u32)) and ref["gathered"] == W * H
    c, z, rect = _rect_scene(1.0, 10.0)
    ref, _ = _dof(r, c, z, _all(), "a blurred foreground", focus=10.0, aperture=0.7, taps=16)
    near = np.zeros((H, W), bool)
    near[12 - 7:30 + 7, 20 - 7:45 + 7] = True
    red = ref["out"].view(f32)[..., 0]
    assert (red[~near] == 0).all() and (red[12:30, 19] > 0).all() and (red[12:30, 20] < 1).all()


def test_a_constant_colour(ptlib):
    """tests/test_dof_cabi.py's case on the GPU: the word-for-word comparison, and the bound of (2 taps + 3) roundings derived there"""
    r, (_, z) = _frame()
    c = np.empty((H, W, 4), f32)
    c[:] = (0.7310, 1.9125, 0.0421, 1.0)
    ref, _ = _dof(r, c, z, _all(), "constant colour", taps=8, aperture=9.0)
    out = ref["out"].view(f32)[..., 0:3].astype(np.float64)
    assert ref["gathered"] == W * H and (np.abs(out - c[..., 0:3]) <= (2 * 8 + 3) * 2.0 ** -24 * c[..., 0:3]).all()


# ------------------------------------------------------------------ 2. a real frame
def _two_box():
    """the two-box scene of pass_cases.MOTION_INPUTS: the colour from the frame path, the depth from renderGBuffer.  Built once; read-only."""
    if "two_box" not in _CASES:
        make, cam, _, _ = MOTION_INPUTS["two_box"]
        r = R.SampleRenderer(make())
        r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
        r.resize((W, H))
        r.setCamera(R.make_camera(cam, W / H))
        r.launchParams.samples_per_launch = 2
        r.launchParams.frame.subframe_index = 0
        r.render()
        r.sync()
        color = r.download(R.PT_BUF_ACCUM).astype(f32).reshape(H, W, 4)
        g = r.renderGBuffer(("depth",))
        planes = dict(color=color, depth=_np(g["depth"]))
        for a in planes.values():
            a.setflags(write=False)
        _CASES["two_box"] = (r, planes)
    return _CASES["two_box"]


def test_two_box_frame_from_the_real_chain(ptlib):
    r, p = _two_box()
    z = p["depth"]
    assert np.isfinite(p["color"]).all() and np.isfinite(z).any() and (z[np.isfinite(z)] > 0).all()
    near = float(z[np.isfinite(z)].min())
    for prm in (dict(focus=near, aperture=6.0), dict(focus=near, aperture=40.0, taps=24), dict(focus=2.0 * near, aperture=12.0, jitter=True, seed=4, taps=9)):
        ref, _ = _dof(r, p["color"], z, _all(), f"two-box, {prm}", **prm)
        assert ref["sources"] == W * H and 0 < ref["gathered"] and 0 < ref["taps"]


# ------------------------------------------------------------------ 3. views, masks, partitions
def test_two_views_of_odd_sizes_hold_a_standalone_frames_bits(ptlib):
    r = _plain((W, H))
    rects = RECTS[:2]
    inside = _set_views(r, rects, W, H)
    c, z = _planes(11)
    prm = dict(jitter=True, seed=3, taps=9)
    ref, _ = _dof(r, c, z, inside, "two views", rects=rects, **prm)
    assert ref["sources"] == sum(w * h for _, _, w, h in rects) == ref["pixels"]
    focus = [0.7, 40.0]
    per_view, _ = _dof(r, c, z, inside, "two views, view_focus", rects=rects, view_focus=focus, **prm)
    for (x0, y0, wr, hr), F in zip(rects, focus):
        box = (slice(y0, y0 + hr), slice(x0, x0 + wr))
        alone = _plain((wr, hr))
        one, _ = _dof(alone, c[box], z[box], _all(hr, wr), f"a frame of {wr} x {hr}", **prm)
        assert not _differ(ref["out"][box], one["out"]).any()
        one, _ = _dof(alone, c[box], z[box], _all(hr, wr), f"a frame of {wr} x {hr}, focus {F}", **dict(prm, focus=F))
        assert not _differ(per_view["out"][box], one["out"]).any() and _differ(per_view["out"][box], ref["out"][box]).any()
        alone.close()
    r.setViews([])
    r.setCamera(R.make_camera(CAM, W / H))
    _dof(r, c, z, _all(), "views dropped")
    _dof(r, c, z, _all(), "views dropped, view_focus of one", view_focus=[0.7])
    r.close()


def test_sixteen_views(ptlib):
    """16 views of 8 x 8 in a 32 x 32 frame: one launch, blockIdx.y the view, one partial tile each, a focus distance each"""
    r = _plain((32, 32))
    rects = [(8 * i, 8 * j, 8, 8) for j in range(4) for i in range(4)]
    inside = _set_views(r, rects, 32, 32)
    c, z = _planes(13, 32, 32)
    ref, _ = _dof(r, c, z, inside, "16 views", rects=rects, taps=6)
    assert ref["sources"] == 1024
    _dof(r, c, z, inside, "16 views, view_focus", rects=rects, taps=6, view_focus=[0.5 * (v + 1) for v in range(16)])
    r.close()


def test_a_view_puts_nothing_into_its_neighbour(ptlib):
    """tests/test_dof_cabi.py's seam case: the right view's T and N are zero, its pixels come back as they were"""
    h, w = 32, 64
    rects = [(0, 0, 32, 32), (32, 0, 32, 32)]
    r = _plain((w, h))
    inside = _set_views(r, rects, w, h)
    c, _ = _planes(12, h, w, hostile=False)
    z = np.full((h, w), 4.0, f32)
    c[8:24, 24:32, 0:3] = 500.0
    z[8:24, 24:32] = 0.5
    ref, tn = _dof(r, c, z, inside, "the seam", rects=rects, focus=4.0)
    first = int(r.dofLayout()[0][1, 2])
    assert (tn[first:] == 0).all() and (tn[:first] != 0).any()
    assert np.array_equal(ref["out"][:, 32:, 0:3], c[:, 32:, 0:3].view(u32)) and ref["gathered"] > 0
    r.close()


def test_masks_write_their_blocks_and_read_every_pixel(ptlib):
    r, (c, z) = _frame()
    nby, nbx = r.blockGrid()
    _, whole = _dof(r, c, z, _all(), "no mask")
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.5
    mask[0, 0] = mask[nby - 1, nbx - 1] = True
    mask[1, 1] = False
    ref, tn = _dof(r, c, z, pixel_mask(mask, h=H, w=W), "a random block mask", mask=mask)
    assert 0 < ref["pixels"] < W * H and ref["sources"] == W * H and np.array_equal(tn, whole)
    ref, tn = _dof(r, c, z, np.zeros((H, W), bool), "the empty mask", mask=np.zeros((nby, nbx), bool))
    assert ref["pixels"] == 0 and ref["sources"] == W * H and ref["gathered"] == 0 and np.array_equal(tn, whole)


def test_partitions_gather_their_own_pixels(ptlib):
    r, (c, z) = _frame()
    ref, whole = _dof(r, c, z, _all(), "unpartitioned")
    by, bx = np.mgrid[0:H, 0:W] // 8
    union = np.full((H, W, 4), SENTINEL, u32)
    model = scenes.cornell_box()
    for rank in range(3):
        rr = _renderer(model, (W, H), CAM, partition=(rank, 3, 8, 8))
        own = (bx + by) % 3 == rank
        part, tn = _dof(rr, c, z, own, f"rank {rank} of 3")
        assert part["pixels"] == int(own.sum()) and part["sources"] == W * H and np.array_equal(tn, whole)
        assert (union[own] == SENTINEL).all()
        union[own] = part["out"][own]
        rr.close()
    assert not _differ(union, ref["out"]).any()


# ------------------------------------------------------------------ 4. refusals
def test_refusals(ptlib):
    L = _lib.load_library()
    r = R.SampleRenderer(scenes.cornell_box())
    c, z = _planes(1)
    color, depth = _upload(c), _upload(z)
    out = filled((H, W, 4))
    nbytes = M.layout(None, H, W)[1]
    sbuf, scratch, lead = _scratch(nbytes)
    good = dict(color=color.data_ptr(), depth=depth.data_ptr(), out=out.data_ptr(), scratch=scratch.data_ptr(), view_focus=None, focus=FOCUS,
                aperture=3.0, max_radius=16.0, taps=32, seed=0, flags=0)

    def untouched(what):
        assert (_np(sbuf).view(u32) == SENTINEL).all(), f"{what}: the scratch was written"
        assert (_bits(out) == SENTINEL).all(), f"{what}: out was written"

    def refused(what, pattern, **fields):
        d = _lib.DofDesc()
        for n, v in dict(good, **fields).items():
            setattr(d, n, v)
        torch.cuda.synchronize()
        s = _lib.DofStats(7, 7, 7, 7, 7, 7.0)
        rc = L.pt_dof_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_dof_planes") and pattern in msg, f"{what}: {msg!r}"
        assert tuple(getattr(s, n) for n, _ in s._fields_) == (7, 7, 7, 7, 7, 7.0)
        untouched(what)

    def layout_refused(what, pattern, with_bytes=True):
        nb = C.c_size_t(77)
        dims = np.full(4, 9, u32)
        rc = L.pt_dof_layout(r._ctx, dims.ctypes.data, C.byref(nb) if with_bytes else None)
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1 and msg.startswith("pt_dof_layout") and pattern in msg, f"{what}: {rc}, {msg!r}"
        assert nb.value == 77 and (dims == 9).all(), f"{what}: an output was written"

    refused("no resize yet", "pt_resize")
    layout_refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(CAM, W / H))
    layout_refused("bytes null", "bytes is null", with_bytes=False)
    nb = C.c_size_t(0)
    assert L.pt_dof_layout(r._ctx, None, C.byref(nb)) == 0 and nb.value == nbytes  # dims may be NULL
    assert L.pt_dof_planes(r._ctx, None, None) == -1 and "pt_dof_planes: null description" in L.pt_last_error(r._ctx).decode()
    refused("an unknown flag", "unknown flag bits 2", flags=3)
    refused("an unknown flag", "unknown flag bits 2147483648", flags=0x80000000)
    for bad in (0, 65, 0xFFFFFFFF):
        refused(f"taps {bad}", f"taps must be 1..64, not {bad}", taps=bad)
    for bad in (0.0, -1.0, 2e30, float("nan"), float("inf")):
        refused(f"focus {bad}", "focus must be finite and in (0,1e30]", focus=bad)
        vf = np.array([bad], f32)
        refused(f"view_focus {bad}", "view_focus[0] must be finite and in (0,1e30]", view_focus=vf.ctypes.data)
    for bad in (-0.5, 4097.0, float("nan"), float("inf")):
        refused(f"aperture {bad}", "aperture must be finite and in [0,4096]", aperture=bad)
    for bad in (0.5, 16.5, float("nan"), float("inf")):
        refused(f"max_radius {bad}", "max_radius must be finite and in [1,16]", max_radius=bad)
    for name in ("color", "depth", "out", "scratch"):
        refused(f"{name} null", f"{name} is null", **{name: None})
    host = np.zeros((H, W, 4), f32)
    refused("a host pointer", "color is not device memory", color=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "out is not 4-byte aligned", out=good["out"] + 2)
    refused("the scratch 2 bytes off", "scratch is not 4-byte aligned", scratch=good["scratch"] + 2)
    refused("out exactly color", "color and out overlap", out=good["color"])
    big = torch.zeros(2 * H * W * 4 + 8, dtype=torch.float32, device="cuda:0")
    refused("out offset against the colour", "color and out overlap", color=big.data_ptr(), out=big.data_ptr() + 16)
    refused("out inside the depth plane", "depth and out overlap", depth=big.data_ptr() + 64, out=big.data_ptr())
    refused("the scratch inside the colour", "color and scratch overlap", scratch=good["color"] + 16)
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
        r.dofPlanes(color, depth, out=color, **LENS)
    with pytest.raises(ValueError, match=r"scratch: a contiguous torch.float32 tensor of shape \(%d,\) is expected" % (nbytes // 4)):
        r.dofPlanes(color, depth, scratch=torch.zeros((nbytes // 4 + 1,), device="cuda:0"), **LENS)
    with pytest.raises(ValueError, match="view_focus has 2 values, expected 1"):
        r.dofPlanes(color, depth, view_focus=[1.0, 2.0], **LENS)
    res = r.dofPlanes(color, depth, out=out, scratch=scratch, **LENS)
    ref = M.dof_ref(c, z, _all(), **LENS)
    assert not _differ(_bits(out), ref["out"]).any() and not _differ(_np(sbuf).view(u32)[lead:-GUARD], ref["scratch"]).any()
    assert {k: res["stats"][k] for k in M.COUNTERS} == {k: ref[k] for k in M.COUNTERS}
    r.close()


def test_rendering_state_is_left_alone(ptlib):
    c, z = _planes(1)
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
            b = r.dofPlanes(_upload(c), _upload(z), **LENS)
            assert b["stats"]["pixels"] == W * H and r.stats() == before
        r.launchParams.frame.subframe_index = 2
        r.render()
        r.sync()
        bufs = [r.download(n) for n in range(5)]
        r.close()
        return bufs

    for n, (x, y) in enumerate(zip(run(True), run(False))):
        assert x.tobytes() == y.tobytes(), f"buffer {n} differs after dofPlanes between the frames"


# ------------------------------------------------------------------ 5. the stream contract
@pytest.mark.parametrize("mode", ["default", "side"])
def test_under_a_busy_torch_stream(ptlib, mode):
    """tests/test_gpu_stream_contract.py's protocol: the inputs are produced, and the outputs sentinel-filled, by work still pending on
    torch's current stream when the call is made; the result equals the synchronous call's, and that equals the reference"""
    from stream_kit import _pin, _res

    r, (c, z) = _frame()
    nbytes = r.dofLayout()[1]
    outs = dict(out=filled((H, W, 4)), scratch=torch.zeros((nbytes // 4,), dtype=torch.float32, device="cuda:0"))

    def lens(dev, outs, returned):
        res = r.dofPlanes(dev["color"], dev["depth"], out=outs["out"], scratch=outs["scratch"], **LENS)
        returned()
        return _res(res, outs)

    sync, got = _pin("dofPlanes", mode, r, dict(color=c, depth=z), outs, lens)
    ref = M.dof_ref(c, z, _all(), **LENS)
    assert not _differ(got["out"].view(u32).reshape(H, W, 4), ref["out"]).any(), f"out under a busy stream [{mode}]"
    assert not _differ(got["scratch"].view(u32).reshape(-1), ref["scratch"]).any(), f"the scratch under a busy stream [{mode}]"
    assert got["stats"] == {k: ref[k] for k in M.COUNTERS}


# ------------------------------------------------------------------ 6. the example loops with --dof
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


@pytest.mark.parametrize("autofocus", [False, True], ids=["focus", "autofocus"])
def test_upsampled_loop_with_dof_displays_the_lens_frame(ptlib, autofocus):
    """examples/upsampled_svgf_loop.py's UpsampledLoop with dof at 128 x 56, scale 2: the lens plane is dofPlanes of the final one under
    the full-resolution G-buffer's depth, and the displayed frame is tonemapPlanes of it.  With autofocus the first frame focuses on the
    depth under the centre, and later frames approach it by a quarter of the difference."""
    import surface_ref as S

    ex = _example("upsampled_svgf_loop")
    w, h = 128, 56
    probe = scenes.sky_probe(256, 128).BuildCDF()
    cam0 = dict(eye=(2.0, 0.35, -3.0), lookat=(0.0, 0.2, 0.5), up=(0.0, 1.0, 0.0), fovY=35.0)
    up = ex.UpsampledLoop(S.textured_scene(), (w, h), 2, probe=probe, dof=True, focus=2.5, autofocus=autofocus, aperture=5.0, dof_taps=8)
    cam = R.make_camera(cam0, w / h)
    focus = None
    for k in range(3):
        prev, cam = cam, R.make_camera(ex.orbit(cam0, 0.02 * k), w / h)
        x = up.frame(k, prev, cam)
        assert x["pixels"] == w * h and x["dof_ms"] > 0 and x["tonemap_ms"] > 0
        if autofocus:
            d = float(_np(up.hi_gbuf["depth"])[h // 2, w // 2])
            target = d if np.isfinite(d) and d > 0 else 2.5
            focus = target if focus is None else focus + 0.25 * (target - focus)
            assert x["focus"] == focus
        else:
            assert x["focus"] == 2.5
    assert x["gathered"] > 0
    ref = M.dof_ref(_np(up.final), _np(up.hi_gbuf["depth"]), _all(h, w), focus=x["focus"], aperture=5.0, taps=8)
    assert not _differ(_bits(up.lens), ref["out"]).any() and x["gathered"] == ref["gathered"]
    want = up.hi.tonemapPlanes(up.lens, frame=torch.zeros((h, w), dtype=torch.int32, device="cuda:0"), op="linear", write_out=False)
    assert np.array_equal(_np(up.frame_rgba8), _np(want["frame_rgba8"]))
    up.close()


@pytest.mark.parametrize("argv", [["--dof", "--focus", "5.0"], ["--dof", "--autofocus", "--bloom", "--bloom-levels", "4", "--motion-blur", "--blur-taps", "8"]],
                         ids=["focus", "autofocus"])
def test_adaptive_albedo_loop_runs_with_dof(ptlib, tmp_path, capsys, argv):
    ex = _example("adaptive_svgf_albedo_loop")
    _main(ex, ["adaptive_svgf_albedo_loop.py", "--size", "128", "56", "--frames", "3", "--aperture", "5.0", "--dof-taps", "8", "--edge-aa", "--auto-exposure",
               "--out-dir", str(tmp_path)] + argv)
    out = capsys.readouterr().out
    assert out.count("depth of field ") == 3 and "tone map" in out and ("focus 5.000" in out) == ("--focus" in argv)
    final, lens = np.load(tmp_path / "adaptive_svgf_albedo_final.npy"), np.load(tmp_path / "adaptive_svgf_albedo_dof.npy")
    assert lens.shape == (56, 128, 4) and (lens[..., 3] == 1).all() and np.isfinite(lens).all() and not np.array_equal(lens[..., 0:3], final[..., 0:3])
    frame = np.load(tmp_path / "adaptive_svgf_albedo_frame.npy")
    assert frame.shape == (56, 128) and (frame >> 24 == 255).all() and len(np.unique(frame)) > 50
