"""Bloom (pt_bloom_layout, pt_bloom_planes) on the GPU.  out, every level of the scratch pyramid and every counter are compared word for word
with tests/bloom_ref.py — NumPy evaluating the header's rule — over WHOLE sentinel-filled allocations: out as a whole plane (a word written
outside the pixel set shows as a lost sentinel), the scratch exactly pt_bloom_layout's bytes between guard words.  NaN words compare as NaN
(payloads are not specified).  Frames are 131 x 59 and smaller, except the one frame that is large enough to leave two levels to the
per-level kernels in front of the tail (193 x 321)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bloom_ref as B
from gpu_kit import filled, pixel_mask
from gpu_kit import bits3 as _bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from gpu_kit import words_differ as _differ
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from scene_kit import RECTS

pytestmark = pytest.mark.gpu

f32 = np.float32
u32 = np.uint32
W, H = 131, 59
GUARD = 4  # sentinel words on either side of the scratch: 16 bytes, so the pyramid stays 16-byte aligned
SENTINEL = B.SENTINEL
CAM = scenes.CORNELL_CAMERA
PRM = dict(exposure=1.0, threshold=0.5, knee=0.25, clamp=64.0, spread=0.75, intensity=0.5, levels=6)
TAIL_TEXELS = 1024  # csrc/pt_bloom.hip's BLOOM_TAIL_TEXELS: the tail starts at the first level from 2 on with at most this many texels


def _all(h=H, w=W):
    return np.ones((h, w), bool)


def _image(seed, h=H, w=W, lo=-8.0, hi=5.0):
    """colours whose luminance spreads over [2^lo, 2^hi], with a random fourth word"""
    rng = np.random.default_rng(seed)
    c = (np.exp2(rng.uniform(lo, hi, (h, w, 1))) * rng.uniform(0.4, 1.0, (h, w, 3))).astype(f32)
    return np.concatenate([c, rng.uniform(0, 1, (h, w, 1)).astype(f32)], -1)


def _scratch(nbytes):
    """(the whole allocation as int32, the (texels, 4) float32 tensor inside it): sentinel-filled, GUARD words on either side"""
    n = nbytes // 4
    buf = torch.full((4 * (n + 2 * GUARD),), 0xA5, dtype=torch.uint8, device="cuda:0").view(torch.int32)
    t = buf[GUARD:GUARD + n].view(torch.float32).view(n // 4, 4)
    assert t.is_contiguous() and t.data_ptr() % 16 == 0
    return buf, t


def _bloom(r, color, pixels, what, state=None, rects=None, mask=None, offset=False, in_place=False, **prm):
    """bloomPlanes into a sentinel-filled out plane and a guarded scratch of exactly pt_bloom_layout's bytes, against the reference: the
    layout, out over the whole frame, every word of the scratch, the four counters.  Returns (the reference, the scratch's words)"""
    h, w = color.shape[:2]
    prm = dict(PRM, **prm)
    dims, nbytes = r.bloomLayout(prm["levels"])
    rdims, rbytes = B.layout(rects, h, w, prm["levels"])
    assert nbytes == rbytes and np.array_equal(dims, rdims), f"{what}: the layout is {dims.tolist()}, {nbytes} bytes; the reference {rdims.tolist()}, {rbytes}"
    dev = _upload(color, offset)
    out = dev if in_place else filled((h, w, 4), offset)
    sbuf, scratch = _scratch(nbytes)
    res = r.bloomPlanes(dev, state=None if state is None else _upload(state, offset), out=out, scratch=scratch, mask=mask, **prm)
    assert res["out"] is out and res["scratch"] is scratch
    ref = B.bloom_ref(color, pixels, state, rects, out0=color if in_place else None, **prm)
    got = _bits(out)
    neq = _differ(got, ref["out"])
    assert got.shape == ref["out"].shape and not neq.any(), f"{what}: out differs in {int(neq.sum())} words, first at {np.argwhere(neq)[:3].tolist()}"
    words = _np(sbuf).view(u32)
    assert (words[:GUARD] == SENTINEL).all() and (words[-GUARD:] == SENTINEL).all(), f"{what}: a word outside the scratch was written"
    pyr = words[GUARD:-GUARD]
    neq = _differ(pyr, ref["scratch"])
    if neq.any():
        first = int(np.argwhere(neq)[0, 0]) // 4
        level = [(v, k + 1) for v in range(dims.shape[0]) for k in range(prm["levels"]) if dims[v, k, 2] <= first][-1]
        raise AssertionError(f"{what}: the scratch differs in {int(neq.sum())} words, first in texel {first} (view, level {level})")
    st = res["stats"]
    assert {k: st[k] for k in B.COUNTERS} == {k: ref[k] for k in B.COUNTERS}, (what, st, {k: ref[k] for k in B.COUNTERS})
    if not in_place:
        assert np.array_equal(_np(dev).view(u32), np.ascontiguousarray(color, f32).view(u32)), f"{what}: color was written"
    return ref, pyr


class _Case:
    pass


_CASES = {}


def _cornell():
    """the Cornell box at W x H under a sky probe, two subframes: the accumulation buffer as the colour.  Built once; read-only."""
    if "cornell" not in _CASES:
        c = _Case()
        c.model = scenes.cornell_box()
        c.r = R.SampleRenderer(c.model)
        c.r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
        c.r.resize((W, H))
        c.r.setCamera(R.make_camera(CAM, W / H))
        c.r.launchParams.samples_per_launch = 2
        for n in (0, 1):
            c.r.launchParams.frame.subframe_index = n
            c.r.render()
        c.r.sync()
        c.color = c.r.download(R.PT_BUF_ACCUM).astype(f32).reshape(H, W, 4)
        c.color.setflags(write=False)
        _CASES["cornell"] = c
    return _CASES["cornell"]


def _plain(size):
    """a renderer of the given size on the Cornell box; no frame is rendered"""
    return _renderer(scenes.cornell_box(), size, CAM)


def _set_views(r, rects, w, h):
    r.setViews([(x, y, ww, hh, R.make_camera(CAM, ww / hh)) for x, y, ww, hh in rects])
    inside = np.zeros((h, w), bool)
    for x, y, ww, hh in rects:
        inside[y:y + hh, x:x + ww] = True
    return inside


# ------------------------------------------------------------------ 1. frames and level counts
def test_cornell_frame_from_the_real_chain(ptlib):
    c = _cornell()
    assert np.isfinite(c.color).all()
    for levels in (1, 2, 6, 8):
        ref, _ = _bloom(c.r, c.color, _all(), f"cornell, {levels} levels", levels=levels)
        assert 0 < ref["bright"] <= W * H and ref["sources"] == W * H
    _bloom(c.r, c.color, _all(), "cornell, every plane 4 bytes off a 16-byte boundary", offset=True, state=np.array([[0, 1.5, 0, 0]], f32))


@pytest.mark.parametrize("size", [(1, 1), (2, 2), (5, 3), (8, 8), (9, 17), (64, 3)])
def test_small_frames(ptlib, size):
    """levels 1, 2 and 8: at 8 every one of these frames has levels of 1 x 1 several times over"""
    w, h = size
    r = _plain(size)
    color = _image(w * 100 + h, h, w)
    for levels in (1, 2, 8):
        ref, _ = _bloom(r, color, _all(h, w), f"{w} x {h}, {levels} levels", levels=levels)
        assert ref["sources"] == w * h
    dims, _ = r.bloomLayout(8)
    assert (dims[0, 6:, 0:2] == 1).all()
    r.close()


def test_halos_cross_tiles_on_both_axes(ptlib):
    """129 x 33: level 1 is 65 x 17, one texel more than two 32 x 8 tiles of k_bloom_down1 in each direction"""
    w, h = 129, 33
    r = _plain((w, h))
    dims, _ = r.bloomLayout(1)
    assert dims[0, 0, 0:2].tolist() == [65, 17]
    color = _image(7, h, w)
    color[15:18, 62:67, 0:3] = 40.0  # light on the corner the four tiles share
    for levels in (1, 3):
        _bloom(r, color, _all(h, w), f"{w} x {h}, {levels} levels", levels=levels)
    r.close()


def test_two_levels_for_the_per_level_kernels_and_two_for_the_tail(ptlib):
    """193 x 321: level 3 is 25 x 41 = 1025 texels, one more than the cut-off, level 4 is 13 x 21: with 5 levels k_bloom_down writes
    levels 2 and 3, k_bloom_tail levels 4 and 5 (and U_4, U_3), k_bloom_up levels 2 and 1.  25 * 41 is the smallest product above 1024 of
    two level sizes that has a frame, and 8 * 24 + 1, 8 * 40 + 1 the smallest frame that has them."""
    w, h = 193, 321
    r = _plain((w, h))
    dims, _ = r.bloomLayout(5)
    texels = (dims[0, :5, 0] * dims[0, :5, 1]).tolist()
    assert texels[2] == TAIL_TEXELS + 1 and texels[3] <= TAIL_TEXELS
    rng = np.random.default_rng(21)
    color = np.ones((h, w, 4), f32)
    color[..., 0:3] = np.exp2(rng.uniform(-8, 5, (h, w, 1))).astype(f32) * rng.uniform(0.4, 1.0, (h, w, 3)).astype(f32)
    _bloom(r, color, _all(h, w), f"{w} x {h}, 5 levels", levels=5)
    r.close()


# ------------------------------------------------------------------ 2. views, masks, partitions
def test_two_views_of_odd_sizes(ptlib):
    r = _plain((W, H))
    rects = RECTS[:2]
    inside = _set_views(r, rects, W, H)
    color = _image(11)
    state = np.array([[0, 0.5, 0, 0], [0, 4.0, 0, 0]], f32)
    ref, _ = _bloom(r, color, inside, "two views", state=state, rects=rects)
    assert ref["sources"] == sum(w * h for _, _, w, h in rects) == ref["pixels"]
    _bloom(r, color, inside, "two views, 8 levels, state NULL", rects=rects, levels=8)
    r.setViews([])
    r.setCamera(R.make_camera(CAM, W / H))
    _bloom(r, color, _all(), "views dropped")
    r.close()


def test_sixteen_views_for_the_tail(ptlib):
    """16 views of 8 x 8 in a 32 x 32 frame: every level from 2 on is the tail's, one workgroup per view"""
    r = _plain((32, 32))
    rects = [(8 * i, 8 * j, 8, 8) for j in range(4) for i in range(4)]
    inside = _set_views(r, rects, 32, 32)
    color = _image(13, 32, 32)
    state = np.zeros((16, 4), f32)
    state[:, 1] = np.exp2(np.arange(16) - 8)
    for levels in (2, 5):
        ref, _ = _bloom(r, color, inside, f"16 views, {levels} levels", state=state, rects=rects, levels=levels)
    r.close()


def test_a_view_puts_nothing_into_its_neighbour(ptlib):
    """tests/test_bloom_cabi.py's seam case: the right view's pyramid is all zeros, its pixels come back as they were"""
    h, w = 24, 48
    rects = [(0, 0, 24, 24), (24, 0, 24, 24)]
    r = _plain((w, h))
    inside = _set_views(r, rects, w, h)
    color = np.zeros((h, w, 4), f32)
    color[12, 23, 0:3] = 1e6
    ref, pyr = _bloom(r, color, inside, "the seam", rects=rects, threshold=1.0, knee=0.5, clamp=64.0, spread=1.0, intensity=1.0, levels=5)
    first = int(r.bloomLayout(5)[0][1, 0, 2])
    assert (pyr[4 * first:] == 0).all() and (pyr[:4 * first] != 0).any() and ref["bright"] == 1
    r.close()


def test_masks_write_their_blocks_and_see_all_the_light(ptlib):
    c = _cornell()
    nby, nbx = c.r.blockGrid()
    _, whole = _bloom(c.r, c.color, _all(), "no mask")
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.5
    mask[0, 0] = mask[nby - 1, nbx - 1] = True
    mask[1, 1] = False
    ref, pyr = _bloom(c.r, c.color, pixel_mask(mask, h=H, w=W), "a random block mask", mask=mask)
    assert 0 < ref["pixels"] < W * H and ref["sources"] == W * H and np.array_equal(pyr, whole)
    ref, pyr = _bloom(c.r, c.color, np.zeros((H, W), bool), "the empty mask", mask=np.zeros((nby, nbx), bool))
    assert ref["pixels"] == 0 and ref["sources"] == W * H and np.array_equal(pyr, whole)


def test_partitions_composite_their_own_pixels(ptlib):
    c = _cornell()
    ref, whole = _bloom(c.r, c.color, _all(), "unpartitioned")
    by, bx = np.mgrid[0:H, 0:W] // 8
    union = np.full((H, W, 4), SENTINEL, u32)
    for rank in range(3):
        r = _renderer(c.model, (W, H), CAM, partition=(rank, 3, 8, 8))
        own = (bx + by) % 3 == rank
        rr, pyr = _bloom(r, c.color, own, f"rank {rank} of 3")
        assert rr["pixels"] == int(own.sum()) and rr["sources"] == W * H and np.array_equal(pyr, whole)
        assert (union[own] == SENTINEL).all()
        union[own] = rr["out"][own]
        r.close()
    assert not _differ(union, ref["out"]).any()


# ------------------------------------------------------------------ 3. in place, the state, hand-made words, the parameters' ends
def test_out_exactly_color(ptlib):
    c = _cornell()
    nby, nbx = c.r.blockGrid()
    mask = np.random.default_rng(9).random((nby, nbx)) < 0.6
    _bloom(c.r, c.color, _all(), "in place", in_place=True)
    _bloom(c.r, c.color, pixel_mask(mask, h=H, w=W), "in place under a mask", in_place=True, mask=mask)


def test_the_exposure_state(ptlib):
    c = _cornell()
    base, _ = _bloom(c.r, c.color, _all(), "state NULL")
    lit, _ = _bloom(c.r, c.color, _all(), "E = 4", state=np.array([[2.0, 4.0, 0, 0]], f32))
    assert lit["bright"] >= base["bright"] > 0
    for bad in (np.nan, np.inf, 0.0, -2.0):
        ref, _ = _bloom(c.r, c.color, _all(), f"E = {bad}", state=np.array([[0, bad, 0, 0]], f32))
        assert ref["bright"] == base["bright"] and np.array_equal(ref["out"], base["out"])


def test_hand_made_words(ptlib):
    """NaN, +-inf, negatives, denormals and FLT_MAX as whole pixels and as single components: the pyramid stays finite, the counters agree"""
    words = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x807FFFFF, 0x80000000, 0xBF800000, 0x42800000, 0x42800001],
                     u32).view(f32)
    h, w = 24, 40
    color = _image(17, h, w, lo=-3, hi=1)
    flat = color.reshape(-1, 4)
    n = len(words)
    pos = np.random.default_rng(3).permutation(h * w)[:4 * n]
    flat[pos[:n], 0:3] = words[:, None]
    for ch in range(3):
        flat[pos[(ch + 1) * n:(ch + 2) * n], ch] = words
    r = _plain((w, h))
    for prm in (dict(), dict(clamp=1e30, threshold=0.0, knee=0.0), dict(levels=3, spread=1.0)):
        ref, pyr = _bloom(r, color, _all(h, w), f"hand-made words, {prm}", **prm)
        assert ref["nonfinite"] == 16 and np.isfinite(pyr.view(f32)).all()
    r.close()


@pytest.mark.parametrize("prm", [dict(knee=0.0), dict(knee=2.0, threshold=2.0), dict(spread=0.0), dict(spread=1.0), dict(intensity=0.0), dict(threshold=0.0, knee=0.0)],
                         ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()))
def test_the_ends_of_the_parameters(ptlib, prm):
    c = _cornell()
    ref, _ = _bloom(c.r, c.color, _all(), f"{prm}", **prm)
    if prm.get("intensity") == 0.0:
        assert np.array_equal(ref["out"].view(f32)[..., 0:3], c.color[..., 0:3])


def test_a_constant_plane_is_exact(ptlib):
    """tests/test_bloom_cabi.py's exactness case on the GPU: every level is the constant times n_k, out = color + intensity * color"""
    c = _cornell()
    v = f32(1.5 * 2.0 ** -3)
    color = np.full((H, W, 4), v, f32)
    ref, pyr = _bloom(c.r, color, _all(), "a constant plane", threshold=0.0, knee=0.0, spread=0.5, intensity=1.0, levels=6)
    a, n = B.gain(1.0, 0.5, 6)
    dims, _ = c.r.bloomLayout(6)
    lvl1 = pyr.view(f32).reshape(-1, 4)[:int(dims[0, 0, 0] * dims[0, 0, 1])]
    assert (lvl1[:, 0:3] == v * n).all() and (lvl1[:, 3] == 0).all()


def test_rendering_state_is_left_alone(ptlib):
    c = _cornell()
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
            b = r.bloomPlanes(_upload(c.color))
            assert b["stats"]["pixels"] == W * H and r.stats() == before
        r.launchParams.frame.subframe_index = 2
        r.render()
        r.sync()
        bufs = [r.download(n) for n in range(5)]
        r.close()
        return bufs

    for n, (x, y) in enumerate(zip(run(True), run(False))):
        assert x.tobytes() == y.tobytes(), f"buffer {n} differs after bloomPlanes between the frames"


# ------------------------------------------------------------------ 4. refusals
def test_refusals(ptlib):
    c = _cornell()
    L = _lib.load_library()
    r = R.SampleRenderer(c.model)
    color = _upload(c.color)
    state = _upload(np.array([[0.0, 1.0, 0.0, 0.0]], f32))
    out = filled((H, W, 4))
    nbytes = B.layout(None, H, W, 6)[1]
    sbuf, scratch = _scratch(nbytes)
    good = dict(color=color.data_ptr(), state=state.data_ptr(), out=out.data_ptr(), scratch=scratch.data_ptr(), flags=0, **PRM)

    def untouched(what):
        assert (_np(sbuf).view(u32) == SENTINEL).all(), f"{what}: the scratch was written"
        assert (_bits(out) == SENTINEL).all(), f"{what}: out was written"

    def refused(what, pattern, **fields):
        d = _lib.BloomDesc()
        for n, v in dict(good, **fields).items():
            setattr(d, n, v)
        torch.cuda.synchronize()
        s = _lib.BloomStats(7, 7, 7, 7, 7.0)
        rc = L.pt_bloom_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_bloom_planes") and pattern in msg, f"{what}: {msg!r}"
        assert tuple(getattr(s, n) for n, _ in s._fields_) == (7, 7, 7, 7, 7.0)
        untouched(what)

    def layout_refused(what, pattern, levels, with_bytes=True):
        nb = C.c_size_t(77)
        dims = np.full(32, 9, u32)
        rc = L.pt_bloom_layout(r._ctx, levels, dims.ctypes.data, C.byref(nb) if with_bytes else None)
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1 and msg.startswith("pt_bloom_layout") and pattern in msg, f"{what}: {rc}, {msg!r}"
        assert nb.value == 77 and (dims == 9).all(), f"{what}: an output was written"

    refused("no resize yet", "pt_resize")
    layout_refused("no resize yet", "pt_resize", 6)
    r.resize((W, H))
    r.setCamera(R.make_camera(CAM, W / H))
    layout_refused("levels 0", "levels must be 1..8, not 0", 0)
    layout_refused("levels 9", "levels must be 1..8, not 9", 9)
    layout_refused("bytes null", "bytes is null", 6, with_bytes=False)
    assert L.pt_bloom_planes(r._ctx, None, None) == -1 and "pt_bloom_planes: null description" in L.pt_last_error(r._ctx).decode()
    refused("a flag", "unknown flag bits 1", flags=1)
    for bad in (0, 9, 0xFFFFFFFF):
        refused(f"levels {bad}", f"levels must be 1..8, not {bad}", levels=bad)
    for name in ("exposure", "clamp"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(f"{name} {bad}", f"{name} must be finite and > 0", **{name: bad})
    for name in ("threshold", "knee", "intensity"):
        for bad in (-0.5, float("nan"), float("inf")):
            refused(f"{name} {bad}", f"{name} must be finite and >= 0", **{name: bad})
    for bad in (-0.01, 1.5, float("nan"), float("inf")):
        refused(f"spread {bad}", "spread must be in [0,1]", spread=bad)
    for name in ("color", "out", "scratch"):
        refused(f"{name} null", f"{name} is null", **{name: None})
    host = np.zeros((H, W, 4), f32)
    refused("a host pointer", "color is not device memory", color=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "out is not 4-byte aligned", out=good["out"] + 2)
    refused("the scratch 4 bytes off", "scratch is not 16-byte aligned", scratch=good["scratch"] - 12)
    big = torch.zeros(2 * H * W * 4 + 8, dtype=torch.float32, device="cuda:0")
    refused("out offset against the colour", "color and out overlap", color=big.data_ptr(), out=big.data_ptr() + 16)
    refused("the scratch inside the colour", "color and scratch overlap", scratch=good["color"] + 16)
    refused("the scratch inside out", "out and scratch overlap", scratch=good["out"] + 32)
    refused("the state inside out", "state and out overlap", state=good["out"] + 32)
    refused("the state inside the scratch", "state and scratch overlap", state=good["scratch"] + 16)
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
    with pytest.raises(RuntimeError, match="knee must be finite"):
        r.bloomPlanes(color, knee=float("nan"))
    with pytest.raises(ValueError, match=r"scratch: a contiguous torch.float32 tensor of shape \(%d, 4\) is expected" % (nbytes // 16)):
        r.bloomPlanes(color, scratch=torch.zeros((nbytes // 16 + 1, 4), device="cuda:0"))
    res = r.bloomPlanes(color, state=state, out=out, scratch=scratch, **PRM)
    ref = B.bloom_ref(c.color, _all(), _np(state), **PRM)
    assert not _differ(_bits(out), ref["out"]).any() and not _differ(_np(sbuf).view(u32)[GUARD:-GUARD], ref["scratch"]).any()
    assert {k: res["stats"][k] for k in B.COUNTERS} == {k: ref[k] for k in B.COUNTERS}
    r.close()


# ------------------------------------------------------------------ 5. the stream contract
@pytest.mark.parametrize("mode", ["default", "side"])
def test_under_a_busy_torch_stream(ptlib, mode):
    """tests/test_gpu_stream_contract.py's protocol: the inputs are produced, and the outputs sentinel-filled, by work still pending on
    torch's current stream when the call is made; the result equals the synchronous call's, and that equals the reference"""
    from stream_kit import _pin, _res

    c = _cornell()
    state = np.array([[0.5, 1.5, 0.0, 0.0]], f32)
    nbytes = c.r.bloomLayout(PRM["levels"])[1]
    outs = dict(out=filled((H, W, 4)), scratch=torch.zeros((nbytes // 16, 4), dtype=torch.float32, device="cuda:0"))

    def bloom(dev, outs, returned):
        res = c.r.bloomPlanes(dev["color"], state=dev["state"], out=outs["out"], scratch=outs["scratch"], **PRM)
        returned()
        return _res(res, outs)

    sync, got = _pin("bloomPlanes", mode, c.r, dict(color=c.color, state=state), outs, bloom, A=dict(state=np.array([[0, 64.0, 0, 0]], f32)))
    ref = B.bloom_ref(c.color, _all(), state, **PRM)
    assert not _differ(got["out"].view(u32).reshape(H, W, 4), ref["out"]).any(), f"out under a busy stream [{mode}]"
    assert not _differ(got["scratch"].view(u32).reshape(-1), ref["scratch"]).any(), f"the scratch under a busy stream [{mode}]"
    assert got["stats"] == {k: ref[k] for k in B.COUNTERS}


# ------------------------------------------------------------------ 6. the example loops with --bloom --auto-exposure
def _example(name):
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def test_upsampled_loop_with_bloom_displays_the_bloomed_frame(ptlib):
    """examples/upsampled_svgf_loop.py's UpsampledLoop with bloom and auto_exposure at 128 x 56, scale 2: the bloomed plane is bloomPlanes of
    the final one under the PREVIOUS frame's exposure state, and the displayed frame is tonemapPlanes of it under this frame's"""
    import surface_ref as S

    ex = _example("upsampled_svgf_loop")
    w, h = 128, 56
    probe = scenes.sky_probe(256, 128).BuildCDF()
    cam0 = dict(eye=(2.0, 0.35, -3.0), lookat=(0.0, 0.2, 0.5), up=(0.0, 1.0, 0.0), fovY=35.0)
    up = ex.UpsampledLoop(S.textured_scene(), (w, h), 2, auto_exposure=True, tonemap="aces", probe=probe, bloom=True, bloom_threshold=0.75, bloom_levels=4)
    cam = R.make_camera(cam0, w / h)
    for k in range(3):
        prev, cam = cam, R.make_camera(ex.orbit(cam0, 0.01 * k), w / h)
        x = up.frame(k, prev, cam)
        assert x["pixels"] == w * h and x["bloom_ms"] > 0 and x["tonemap_ms"] > 0
    prev_state, state = _np(up.state[up.cur ^ 1]), up.state[up.cur]
    ref = B.bloom_ref(_np(up.final), _all(h, w), prev_state, threshold=0.75, levels=4)
    assert not _differ(_bits(up.bloomed), ref["out"]).any() and x["bright"] == ref["bright"]
    want = up.hi.tonemapPlanes(up.bloomed, state=state, frame=torch.zeros((h, w), dtype=torch.int32, device="cuda:0"), op="aces", write_out=False)
    assert np.array_equal(_np(up.frame_rgba8), _np(want["frame_rgba8"]))
    up.close()


def test_adaptive_albedo_loop_runs_with_bloom(ptlib, tmp_path, capsys):
    ex = _example("adaptive_svgf_albedo_loop")
    import sys

    argv = sys.argv
    sys.argv = ["adaptive_svgf_albedo_loop.py", "--size", "128", "56", "--frames", "3", "--bloom", "--bloom-threshold", "0.75", "--bloom-levels", "4",
                "--auto-exposure", "--out-dir", str(tmp_path)]
    try:
        ex.main()
    finally:
        sys.argv = argv
    out = capsys.readouterr().out
    assert out.count("bloom ") >= 3 and "tone map" in out
    final, bloomed = np.load(tmp_path / "adaptive_svgf_albedo_final.npy"), np.load(tmp_path / "adaptive_svgf_albedo_bloomed.npy")
    assert bloomed.shape == (56, 128, 4) and (bloomed[..., 0:3] >= final[..., 0:3]).all() and (bloomed[..., 3] == 1).all()
    frame = np.load(tmp_path / "adaptive_svgf_albedo_frame.npy")
    assert frame.shape == (56, 128) and (frame >> 24 == 255).all() and len(np.unique(frame)) > 50
