"""Auto exposure and display tone mapping (pt_exposure_planes, pt_tonemap_planes) on the GPU.  hist, state_out, out, frame_rgba8 and every
counter are compared bit for bit with tests/exposure_ref.py — NumPy evaluating the header's rules — over WHOLE sentinel-filled allocations
(guard words around hist and the state, whole planes for out and frame_rgba8: a word written outside the pixel set shows as a lost
sentinel).  NaN words compare as NaN (payloads are not specified).  Frames are 131 x 59 and smaller, except the one frame that is large
enough for a workgroup of the bounded metering grid to walk more than one tile and to change its view on the way."""
import ctypes as C

import numpy as np
import pytest
import torch

import exposure_ref as X
from gpu_kit import filled, pixel_mask, plane_shape
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
GUARD = 4  # sentinel words on either side of hist and of the state
SENTINEL = X.SENTINEL
CAM = scenes.CORNELL_CAMERA
PRM = dict(low_permille=50, high_permille=20, key_log2=-2.4739312, ev_min=-16.0, ev_max=16.0, rate_up=1.0, rate_down=1.0)


def _guarded(rows, width, dtype, offset=False, content=None):
    """(the whole allocation as int32, the (rows, width) tensor inside it): sentinel-filled, GUARD words on either side; offset: the tensor
    starts one word off a 16-byte boundary.  content: what the tensor holds instead of the sentinel"""
    n = rows * width
    buf = torch.full((4 * (n + 2 * GUARD + 1),), 0xA5, dtype=torch.uint8, device="cuda:0").view(torch.int32)
    a = GUARD + (1 if offset else 0)
    t = buf[a:a + n].view(rows, width).view(dtype)
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 if offset else 0)
    if content is not None:
        t.copy_(torch.from_numpy(np.ascontiguousarray(content).view(np.int32 if dtype == torch.int32 else f32)).to("cuda:0"))
    return buf, t


def _guards_intact(buf, t, what):
    words = _np(buf).view(u32)
    a = (t.data_ptr() - buf.data_ptr()) // 4
    assert (words[:a] == SENTINEL).all() and (words[a + t.numel():] == SENTINEL).all(), f"{what}: a word outside the array was written"


def _plane(name, h, w, offset=False):
    """a sentinel-filled output plane of the tone mapper"""
    return filled(plane_shape(h, w, 4 if name == "out" else 1), offset, torch.int32 if name == "frame_rgba8" else torch.float32)


def _all(h=H, w=W):
    return np.ones((h, w), bool)


def _image(seed, h=H, w=W, lo=-9.0, hi=5.0):
    """colours whose luminance spreads over [2^lo, 2^hi]"""
    rng = np.random.default_rng(seed)
    c = (np.exp2(rng.uniform(lo, hi, (h, w, 1))) * rng.uniform(0.4, 1.0, (h, w, 3))).astype(f32)
    return np.concatenate([c, rng.uniform(0, 1, (h, w, 1)).astype(f32)], -1)


def _meter(r, color, pixels, what, hit=None, rects=None, mask=None, offset=False, state_in=None, in_place=False, hist0=None, accumulate=False, **prm):
    """exposurePlanes into guarded arrays against the reference: hist, state_out and the five counters, bit for bit.  in_place: state_out is
    state_in.  hist0: the histogram's content before the call (with accumulate).  Returns (hist, state_out, stats) as arrays"""
    nv = max(1, len(rects or ()))
    prm = dict(PRM, **prm)
    hbuf, hist = _guarded(nv, 256, torch.int32, offset, hist0)
    sin = None
    if state_in is not None:
        sibuf, sin = _guarded(nv, 4, torch.float32, offset, state_in)
    sbuf, sout = (sibuf, sin) if in_place else _guarded(nv, 4, torch.float32, offset)
    res = r.exposurePlanes(_upload(color, offset), None if hit is None else _upload(hit, offset), hist=hist, state_in=sin, state_out=sout, mask=mask,
                           accumulate=accumulate, **prm)
    assert res["hist"] is hist and res["state_out"] is sout
    rh, rs, rc = X.exposure_ref(color, pixels, hit, rects, hist0 if accumulate else None, state_in, **prm)
    gh, gs, st = _np(hist).view(u32), _np(sout), res["stats"]
    assert np.array_equal(gh, rh), f"{what}: hist differs in {int((gh != rh).sum())} bins, first at {np.argwhere(gh != rh)[:3].tolist()}"
    assert not _differ(gs.view(u32), rs.view(u32)).any(), f"{what}: state_out {gs.tolist()} against {rs.tolist()}"
    assert {k: st[k] for k in X.COUNTERS} == rc, (what, st, rc)
    _guards_intact(hbuf, hist, what + ", hist")
    _guards_intact(sbuf, sout, what + ", state_out")
    if state_in is not None and not in_place:
        assert np.array_equal(_np(sin).view(u32), np.ascontiguousarray(state_in, f32).view(u32)), f"{what}: state_in was written"
    return gh, gs, st


def _tone(r, orc, color, pixels, what, state=None, rects=None, mask=None, offset=False, in_place=False, planes=("out", "frame_rgba8"), **prm):
    """tonemapPlanes into sentinel-filled planes against the reference over the whole frame, and both counters"""
    h, w = color.shape[:2]
    dev = _upload(color, offset)
    outs = {n: _plane(n, h, w, offset) for n in planes}
    if in_place:
        outs["out"] = dev
    res = r.tonemapPlanes(dev, state=None if state is None else _upload(state, offset), out=outs.get("out"), frame=outs.get("frame_rgba8"), mask=mask,
                          write_out="out" in planes, **prm)
    assert all(res[n] is outs[n] for n in planes)
    ref = X.tonemap_ref(color, pixels, state, rects, planes=planes, orc=orc, **prm)
    if in_place:  # outside the set the plane keeps the colour
        keep = ~np.asarray(pixels, bool)
        ref["out"][keep] = np.ascontiguousarray(color, f32).view(u32)[keep]
    for n in planes:
        g = _bits(outs[n])
        neq = _differ(g, ref[n]) if n == "out" else g != ref[n]
        assert g.shape == ref[n].shape and not neq.any(), f"{what}: {n} differs in {int(neq.sum())} words, first at {np.argwhere(neq)[:3].tolist()}"
    st = res["stats"]
    assert (st["pixels"], st["clipped"]) == (ref["pixels"], ref["clipped"]) and st["pixels"] == int(np.asarray(pixels).sum()), (what, st, ref["pixels"], ref["clipped"])
    return ref, st


class _Case:
    pass


_CASES = {}


def _cornell():
    """the Cornell box at W x H under a sky probe, two subframes: the accumulation buffer as the colour, the G-buffer's hit plane.  Built once;
    the arrays are read-only."""
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
        c.hit = _np(c.r.renderGBuffer(("hit",))["hit"])
        for a in (c.color, c.hit):
            a.setflags(write=False)
        _CASES["cornell"] = c
    return _CASES["cornell"]


def _plain(size):
    """a renderer of the given size on the Cornell box; no frame is rendered"""
    return _renderer(scenes.cornell_box(), size, CAM)


# ------------------------------------------------------------------ 1. the meter and the adaptation against the reference
def test_cornell_frame_from_the_real_chain(ptlib, orc_det):
    c = _cornell()
    assert np.isfinite(c.color).all() and (c.hit.view(np.int32)[..., 3] < 0).any()
    for hit in (c.hit, None):
        gh, gs, st = _meter(c.r, c.color, _all(), f"cornell, hit {'given' if hit is not None else 'NULL'}", hit=hit)
        print(f"cornell: {st}, state {gs.tolist()}, {int((gh != 0).sum())} bins in use")
        assert (st["skipped"] > 0) == (hit is not None) and gh.sum() == W * H - st["skipped"] - st["nonfinite"] and gs[0, 3] > 0
        assert int((gh != 0).sum()) > 20 and -16 < gs[0, 0] < 16
    state = gs
    for op in X.OPS:
        _tone(c.r, orc_det, c.color, _all(), f"cornell, {op}, metered", state=state, op=op, white=2.0)
        _tone(c.r, orc_det, c.color, _all(), f"cornell, {op}, state NULL", op=op, exposure=1.5)


@pytest.mark.parametrize("size", [(1, 1), (8, 8), (9, 17), (64, 3)])
def test_small_frames(ptlib, orc_det, size):
    w, h = size
    r = _plain(size)
    color = _image(w * 100 + h, h, w)
    hit = np.zeros((h, w, 8), f32)
    hit.view(np.int32)[..., 3] = np.where(np.random.default_rng(1).random((h, w)) < 0.3, -1, 5)
    _, gs, st = _meter(r, color, _all(h, w), f"{w} x {h}", hit=hit)
    assert st["pixels"] == w * h
    _tone(r, orc_det, color, _all(h, w), f"{w} x {h}", state=gs, op="aces")
    r.close()


def test_constant_and_black_frames(ptlib, orc_det):
    r = _plain((W, H))
    const = np.broadcast_to(np.array([0.3, 0.2, 0.1, 1.0], f32), (H, W, 4)).copy()
    gh, gs, st = _meter(r, const, _all(), "a constant frame", low_permille=0, high_permille=0)
    b = int(X.bin_of(X.luminance(const[0:1, 0]))[0])
    assert gh[0, b] == W * H and gh.sum() == W * H and gs[0, 3] == W * H and 1 <= b <= 254
    black = np.zeros((H, W, 4), f32)
    gh, gs, st = _meter(r, black, _all(), "an all-black frame, state_in NULL")
    assert gh[0, 0] == W * H and st["under"] == W * H and gs[0, 0] == 0 and gs[0, 1] == 1 and np.isnan(gs[0, 2]) and gs[0, 3] == 0
    prev = np.array([[2.5, 7.0, -1.25, 10.0]], f32)
    gh, gs, st = _meter(r, black, _all(), "an all-black frame keeps ev_prev", state_in=prev, rate_up=0.5)
    assert gs[0, 0] == f32(2.5) and gs[0, 2] == f32(-1.25) and gs[0, 3] == 0
    _tone(r, orc_det, black, _all(), "black", state=gs, op="reinhard")
    r.close()


def _edge_words():
    """the exact bin edges of tests/test_exposure_cabi.py's (b) and the words outside the scale"""
    v = []
    for e in (-17, -16, -9, -1, 0, 1, 7, 15, 16):
        for j in range(8):
            x = f32(2.0 ** e * (1 + j / 8))
            v += [x, np.nextafter(x, f32(0)), np.nextafter(x, f32(np.inf))]
    words = np.array([0x00000000, 0x80000000, 0xBF800000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F7FFFFE],
                     u32).view(f32)
    return np.concatenate([np.array(v, f32), words, -np.array(v[:12], f32)])


def test_hand_made_words(ptlib, orc_det):
    """NaN, +-inf, negatives, denormals and the exact bin edges, as luminances (grey pixels: the weights sum to 1 within a rounding, so
    neighbours of an edge land on both sides of it) and as single components"""
    vals = _edge_words()
    h, w = 24, 40
    color = np.ones((h, w, 4), f32)
    flat = color.reshape(-1, 4)
    n = len(vals)
    assert 3 * n <= h * w
    flat[:n, 0:3] = vals[:, None]  # grey
    flat[n:2 * n, 0:3] = 0
    flat[n:2 * n, 1] = vals  # green alone
    flat[2 * n:3 * n, 2] = vals  # red and green 1, blue the word
    r = _plain((w, h))
    hit = np.zeros((h, w, 8), f32)
    hit.view(np.int32)[::5, ::3, 3] = np.int32(-2 ** 31)  # misses, NaN colours among them
    for hh in (None, hit):
        gh, gs, st = _meter(r, color, _all(h, w), "hand-made words", hit=hh, low_permille=0, high_permille=0)
        assert st["nonfinite"] > 10 and st["under"] > 30 and st["over"] > 10 and gh[0, 1] > 0 and gh[0, 254] > 0
    for op in X.OPS:
        _tone(r, orc_det, color, _all(h, w), f"hand-made words, {op}", state=np.array([[0, 3.0, 0, 0]], f32), op=op, white=0.75)
    # exposure words that count as 1
    for bad in (np.nan, np.inf, -np.inf, 0.0, -2.0):
        ref, _ = _tone(r, orc_det, color, _all(h, w), f"E = {bad}", state=np.array([[0, bad, 0, 0]], f32), op="linear", exposure=0.5, planes=("out",))
    r.close()


def test_planes_one_float_into_their_allocations(ptlib, orc_det):
    c = _cornell()
    _, gs, _ = _meter(c.r, c.color, _all(), "every array 4 bytes off a 16-byte boundary", hit=c.hit, offset=True, state_in=np.array([[1.0, 2.0, 0.0, 5.0]], f32), rate_up=0.25,
                      rate_down=0.5)
    _tone(c.r, orc_det, c.color, _all(), "every plane 4 bytes off a 16-byte boundary", state=gs, offset=True, op="aces")


# ------------------------------------------------------------------ 2. views, masks, partitions
def _set_views(r, rects, w, h):
    r.setViews([(x, y, ww, hh, R.make_camera(CAM, ww / hh)) for x, y, ww, hh in rects])
    inside = X.view_index(rects, h, w) >= 0
    return inside


def test_two_views_off_the_block_grid_with_different_content(ptlib, orc_det):
    r = _plain((W, H))
    rects = RECTS[:2]
    inside = _set_views(r, rects, W, H)
    color = _image(11)
    x1, y1, w1, h1 = rects[1]
    color[y1:y1 + h1, x1:x1 + w1, 0:3] *= f32(64.0)  # the second view is six stops brighter
    hit = np.zeros((H, W, 8), f32)
    hit.view(np.int32)[10:20, :, 3] = -1
    gh, gs, st = _meter(r, color, inside, "two views", hit=hit, rects=rects)
    assert st["pixels"] == sum(w * h for _, _, w, h in rects) and 5.9 < float(gs[1, 2]) - float(gs[0, 2]) < 6.1
    _tone(r, orc_det, color, inside, "two views", state=gs, rects=rects, op="aces")
    _tone(r, orc_det, color, inside, "two views, state NULL", rects=rects, op="reinhard")
    r.setViews([])
    r.setCamera(R.make_camera(CAM, W / H))
    _meter(r, color, _all(), "views dropped")
    r.close()


def test_sixteen_views_in_one_workgroup(ptlib, orc_det):
    """16 views of 8 x 8 in a 32 x 32 frame: the whole frame is one tile of one workgroup, whose LDS copy serves the first view alone"""
    r = _plain((32, 32))
    rects = [(8 * i, 8 * j, 8, 8) for j in range(4) for i in range(4)]
    inside = _set_views(r, rects, 32, 32)
    color = _image(13, 32, 32)
    for k, (x, y, w, h) in enumerate(rects):
        color[y:y + h, x:x + w, 0:3] *= f32(2.0 ** (k - 8))
    gh, gs, st = _meter(r, color, inside, "16 views", rects=rects)
    assert (gh.sum(1) == 64).all() and len(set(gs[:, 0].tolist())) == 16
    _tone(r, orc_det, color, inside, "16 views", state=gs, rects=rects, op="linear")
    r.close()


def test_a_workgroup_that_walks_several_tiles_and_changes_its_view(ptlib):
    """2048 x 520: 1040 tiles of 1024 pixels, more than four workgroups a CU of a 256-CU device hold, so a workgroup walks two tiles.  Two
    views side by side, the first 129 blocks wide: the ninth tile of every block row starts in the first view and ends in the second (the
    stragglers), the tenth starts in the second (the flush), and the two belong to one workgroup."""
    w, h = 2048, 520
    r = _plain((w, h))
    rng = np.random.default_rng(17)
    color = np.ones((h, w, 4), f32)
    color[..., 0:3] = np.exp2(rng.uniform(-8, 4, (h, w, 1))).astype(f32)
    color[:, 1032:, 0:3] *= f32(8.0)
    _meter(r, color, _all(h, w), "2048 x 520, no views")
    rects = [(0, 0, 1032, h), (1032, 0, 1016, h)]
    inside = _set_views(r, rects, w, h)
    gh, gs, st = _meter(r, color, inside, "2048 x 520, two views", rects=rects)
    assert gh[0].sum() == 1032 * h and gh[1].sum() == 1016 * h and 2.9 < float(gs[1, 2]) - float(gs[0, 2]) < 3.1
    r.close()


def test_block_masks_partitions_and_accumulate(ptlib, orc_det):
    c = _cornell()
    nby, nbx = c.r.blockGrid()
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.5
    mask[0, 0] = mask[nby - 1, nbx - 1] = True
    mask[1, 1] = False
    px = pixel_mask(mask, h=H, w=W)
    gh, gs, st = _meter(c.r, c.color, px, "a random block mask", hit=c.hit, mask=mask)
    assert 0 < st["pixels"] < W * H
    _tone(c.r, orc_det, c.color, px, "a random block mask", state=gs, mask=mask, op="aces")
    # ACCUMULATE over two calls equals one call on the union mask
    other = ~mask
    h1, _, _ = _meter(c.r, c.color, px, "the first half", hit=c.hit, mask=mask)
    h2, s2, _ = _meter(c.r, c.color, pixel_mask(other, h=H, w=W), "the second half, accumulated", hit=c.hit, mask=other, hist0=h1, accumulate=True)
    hw, sw, _ = _meter(c.r, c.color, _all(), "the whole frame", hit=c.hit)
    assert np.array_equal(h2, hw) and np.array_equal(s2.view(u32), sw.view(u32))
    # the empty mask: nothing is metered, the histogram is zeroed, the adaptation runs on it
    empty = np.zeros((nby, nbx), bool)
    gh, gs, st = _meter(c.r, c.color, np.zeros((H, W), bool), "the empty mask", hit=c.hit, mask=empty, state_in=np.array([[1.0, 2.0, 3.0, 4.0]], f32))
    assert not gh.any() and {k: st[k] for k in X.COUNTERS} == {k: 0 for k in X.COUNTERS} and gs[0].tolist() == [1.0, float(X.expf(f32(0.69314718))), 3.0, 0.0]
    ref, st = _tone(c.r, orc_det, c.color, np.zeros((H, W), bool), "the empty mask", mask=empty, op="aces")
    assert st["pixels"] == st["clipped"] == 0
    # rank 1 of 3, and the three ranks' histograms added, through FROM_HISTOGRAM: the unpartitioned call's state
    by, bx = np.mgrid[0:H, 0:W] // 8
    total = np.zeros((1, 256), np.int64)
    for rank in range(3):
        r = _renderer(c.model, (W, H), CAM, partition=(rank, 3, 8, 8))
        own = (bx + by) % 3 == rank
        gh, _, st = _meter(r, c.color, own, f"rank {rank} of 3", hit=c.hit)
        assert st["pixels"] == int(own.sum())
        if rank == 1:
            _tone(r, orc_det, c.color, own, "rank 1 of 3", state=sw, op="reinhard", white=3.0)
        total += gh
        r.close()
    assert np.array_equal(total, hw)
    prev = np.array([[0.5, 1.0, 0.0, 0.0]], f32)
    want = c.r.exposurePlanes(_upload(c.color), _upload(c.hit), state_in=_upload(prev), rate_up=0.5, rate_down=0.25, **{k: PRM[k] for k in ("low_permille", "high_permille")})
    hbuf, hist = _guarded(1, 256, torch.int32, content=total.astype(u32))
    sbuf, sout = _guarded(1, 4, torch.float32)
    res = c.r.exposurePlanes(hist=hist, state_in=_upload(prev), state_out=sout, from_histogram=True, rate_up=0.5, rate_down=0.25,
                             **{k: PRM[k] for k in ("low_permille", "high_permille")})
    assert np.array_equal(_np(sout).view(u32), _np(want["state_out"]).view(u32)) and np.array_equal(_np(hist).view(u32), hw)
    assert np.array_equal(_np(sout).view(u32), X.adapt_ref(hw, prev, **dict(PRM, rate_up=0.5, rate_down=0.25)).view(u32))
    assert {k: res["stats"][k] for k in X.COUNTERS} == {k: 0 for k in X.COUNTERS}
    _guards_intact(hbuf, hist, "FROM_HISTOGRAM, hist")
    _guards_intact(sbuf, sout, "FROM_HISTOGRAM, state_out")


# ------------------------------------------------------------------ 3. the state from frame to frame
def test_three_frames_of_state_ping_pong(ptlib, orc_det):
    c = _cornell()
    frames = [c.color, (c.color * f32(8.0)).astype(f32), (c.color * f32(0.125)).astype(f32)]
    for in_place in (False, True):
        state = np.array([[np.nan, np.nan, np.nan, np.nan]], f32) if in_place else None  # in place: a first state that is not finite
        evs = []
        for k, color in enumerate(frames):
            _, state, _ = _meter(c.r, color, _all(), f"frame {k}, in place {in_place}", hit=c.hit, state_in=state, in_place=in_place and state is not None, rate_up=0.5,
                                 rate_down=0.25)
            evs.append(float(state[0, 0]))
            _tone(c.r, orc_det, color, _all(), f"frame {k}", state=state, op="aces", planes=("frame_rgba8",))
        assert evs[1] < evs[0] and evs[2] > evs[1]  # brighter frame: the exposure falls by a quarter of three stops; then it rises
        # (the target moves by three stops up to the pixels that enter or leave bins 0 and 255: a sanity check beside the bit-exact one)
        assert abs((evs[0] - evs[1]) - 0.75) < 0.05 and abs((evs[2] - evs[1]) - 0.5 * (evs[0] + 3 - evs[1])) < 0.05


def test_out_exactly_color(ptlib, orc_det):
    c = _cornell()
    nby, nbx = c.r.blockGrid()
    mask = np.random.default_rng(9).random((nby, nbx)) < 0.6
    _tone(c.r, orc_det, c.color, _all(), "in place", in_place=True, op="aces", exposure=2.0)
    _tone(c.r, orc_det, c.color, pixel_mask(mask, h=H, w=W), "in place under a mask", in_place=True, mask=mask, op="reinhard")


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
            e = r.exposurePlanes(_upload(c.color), _upload(c.hit))
            t = r.tonemapPlanes(_upload(c.color), state=e["state_out"], frame=_plane("frame_rgba8", H, W))
            assert e["stats"]["pixels"] == t["stats"]["pixels"] == W * H and r.stats() == before
        r.launchParams.frame.subframe_index = 2
        r.render()
        r.sync()
        bufs = [r.download(n) for n in range(5)]
        r.close()
        return bufs

    for n, (x, y) in enumerate(zip(run(True), run(False))):
        assert x.tobytes() == y.tobytes(), f"buffer {n} differs after exposurePlanes and tonemapPlanes between the frames"


# ------------------------------------------------------------------ 4. against the frame path
def test_reinhard_equals_the_frame_paths_own_write(ptlib):
    """pt_render_regions with tonemap = 1, exposure = 4, white = 1 leaves frame_buffer = make_color(reinhard_tonemap(accum * 4, 1)); this pass
    on that accum buffer, with state NULL, must leave the same bytes"""
    w, h = 64, 40
    r = R.SampleRenderer(scenes.cornell_box())
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.resize((w, h))
    r.setCamera(R.make_camera(CAM, w / h))
    frame = np.zeros((h, w), np.uint32)
    r.renderRegions([dict(launch_w=w, launch_h=h, factor_x=1, factor_y=1, fill_size=1, cx=0, cy=0, r_inner=0.0, r_outer=1.0e9, offset_x=0, offset_y=0, redraw=1, spp=2,
                          subframe_index=0)], dict(tonemap=1, exposure=4.0, white=1.0), out=frame)
    accum = r.download(R.PT_BUF_ACCUM).astype(f32).reshape(h, w, 4)
    assert np.isfinite(accum[..., 0:3]).all() and (accum[..., 0:3] >= 0).all() and accum[..., 0:3].max() > 0.3
    got = r.tonemapPlanes(_upload(accum), frame=_plane("frame_rgba8", h, w), op="reinhard", exposure=4.0, white=1.0, write_out=False)
    mine = _np(got["frame_rgba8"]).view(u32)
    assert np.array_equal(mine, frame), f"{int((mine != frame).sum())} of {w * h} pixels differ from the frame path's"
    assert len(np.unique(frame)) > 100
    r.close()


# ------------------------------------------------------------------ 5. refusals
def test_refusals(ptlib):
    c = _cornell()
    L = _lib.load_library()
    r = R.SampleRenderer(c.model)
    color, hit = _upload(c.color), _upload(c.hit)
    hbuf, hist = _guarded(1, 256, torch.int32)
    sbuf, sout = _guarded(1, 4, torch.float32)
    sin = _upload(np.array([[0.0, 1.0, 0.0, 0.0]], f32))
    outs = {n: _plane(n, H, W) for n in ("out", "frame_rgba8")}
    egood = dict(color=color.data_ptr(), hit=hit.data_ptr(), hist=hist.data_ptr(), state_in=sin.data_ptr(), state_out=sout.data_ptr(), flags=0, **PRM)
    tgood = dict(color=color.data_ptr(), state=sin.data_ptr(), out=outs["out"].data_ptr(), frame_rgba8=outs["frame_rgba8"].data_ptr(), exposure=1.0, white=1.0, op=2, flags=0)

    def untouched(what):
        assert (_np(hbuf).view(u32) == SENTINEL).all() and (_np(sbuf).view(u32) == SENTINEL).all(), f"{what}: hist or state_out was written"
        for n, t in outs.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {n} was written"

    def refused(fn, what, pattern, **fields):
        Desc, Stats, good, seven = ((_lib.ExposureDesc, _lib.ExposureStats, egood, (7, 7, 7, 7, 7, 7.0)) if fn == "pt_exposure_planes" else
                                    (_lib.TonemapDesc, _lib.TonemapStats, tgood, (7, 7, 7.0)))
        d = Desc()
        for n, v in dict(good, **fields).items():
            setattr(d, n, v)
        torch.cuda.synchronize()
        s = Stats(*seven)
        rc = getattr(L, fn)(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith(fn) and pattern in msg, f"{what}: {msg!r}"
        assert tuple(getattr(s, n) for n, _ in s._fields_) == seven
        untouched(what)

    E, T = "pt_exposure_planes", "pt_tonemap_planes"
    refused(E, "no resize yet", "pt_resize")
    refused(T, "no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(CAM, W / H))
    for fn in (E, T):
        assert getattr(L, fn)(r._ctx, None, None) == -1 and f"{fn}: null description" in L.pt_last_error(r._ctx).decode()
    # ---- pt_exposure_planes
    refused(E, "a flag", "unknown flag bits 4", flags=4)
    refused(E, "a flag beside the known ones", "unknown flag bits 8", flags=11)
    refused(E, "FROM_HISTOGRAM with a colour", "takes no color, hit or block_mask", flags=2, hit=None)
    refused(E, "FROM_HISTOGRAM with a hit plane", "takes no color, hit or block_mask", flags=2, color=None)
    mask = np.ones(c.r.blockGrid(), np.uint8)
    refused(E, "FROM_HISTOGRAM with a mask", "takes no color, hit or block_mask", flags=3, color=None, hit=None, block_mask=mask.ctypes.data)
    refused(E, "the trims", "low_permille + high_permille must be <= 999", low_permille=500, high_permille=500)
    refused(E, "a huge trim", "low_permille + high_permille must be <= 999", low_permille=0xFFFFFFFF, high_permille=1)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(E, f"key_log2 {bad}", "key_log2 must be finite", key_log2=bad)
    for f in (dict(ev_min=-24.5), dict(ev_max=25.0), dict(ev_min=float("nan")), dict(ev_max=float("nan")), dict(ev_min=2.0, ev_max=1.0), dict(ev_min=-float("inf"))):
        refused(E, f"{f}", "ev_min and ev_max must be in [-24,24] with ev_min <= ev_max", **f)
    for name in ("rate_up", "rate_down"):
        for bad in (-0.01, 1.5, float("nan"), float("inf")):
            refused(E, f"{name} {bad}", "rate_up and rate_down must be in [0,1]", **{name: bad})
    for name in ("color", "hist", "state_out"):
        refused(E, f"{name} null", f"{name} is null", **{name: None})
    host = np.zeros((H, W, 8), f32)
    refused(E, "a host pointer", "hit is not device memory", hit=host.ctypes.data)
    refused(E, "a pointer offset by 2 bytes", "hist is not 4-byte aligned", hist=egood["hist"] + 2)
    refused(E, "hist on the colour", "color and hist overlap", hist=egood["color"] + 64)
    refused(E, "state_out on the colour", "color and state_out overlap", state_out=egood["color"])
    refused(E, "state_out inside hist", "hist and state_out overlap", state_out=egood["hist"] + 512)
    refused(E, "state_in inside hist", "hist and state_in overlap", state_in=egood["hist"] + 16)
    refused(E, "state_out offset against state_in", "state_in and state_out overlap", state_in=egood["state_out"] + 4)
    # ---- pt_tonemap_planes
    refused(T, "a flag", "unknown flag bits 1", flags=1)
    refused(T, "an operator", "unknown operator 3", op=3)
    for name in ("exposure", "white"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(T, f"{name} {bad}", f"{name} must be finite and > 0", **{name: bad})
    refused(T, "no output", "no output asked for", out=None, frame_rgba8=None)
    refused(T, "color null", "color is null", color=None)
    refused(T, "a host pointer", "state is not device memory", state=host.ctypes.data)
    refused(T, "a pointer offset by 1 byte", "out is not 4-byte aligned", out=tgood["out"] + 1)
    big = torch.zeros(2 * H * W * 4 + 8, dtype=torch.float32, device="cuda:0")
    refused(T, "out offset against the colour", "color and out overlap", color=big.data_ptr(), out=big.data_ptr() + 16)
    refused(T, "the frame inside the colour", "color and frame_rgba8 overlap", frame_rgba8=tgood["color"] + 16)
    refused(T, "two outputs", "out and frame_rgba8 overlap", frame_rgba8=tgood["out"])
    refused(T, "the state inside out", "state and out overlap", state=tgood["out"] + 32)
    hip = _hip_runtime()
    for fn, name, nbytes, step in ((E, "hist", 1024, 16), (E, "state_out", 16, 4), (T, "frame_rgba8", H * W * 4, 16), (T, "out", H * W * 16, 16)):
        raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert hip.hipMalloc(C.byref(raw), C.c_size_t(nbytes)) == 0
        try:
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= nbytes
            refused(fn, f"{name} one element too small", f"{name} has fewer than {nbytes} bytes left", **{name: raw.value + size.value - (nbytes - step)})
        finally:
            assert hip.hipFree(raw) == 0
    # the Python facade passes the library's refusals on; valid calls afterwards still work, into the same arrays
    with pytest.raises(RuntimeError, match="key_log2 must be finite"):
        r.exposurePlanes(color, key_log2=float("nan"))
    with pytest.raises(RuntimeError, match="white must be finite"):
        r.tonemapPlanes(color, white=0.0)
    res = r.exposurePlanes(color, hit, hist=hist, state_in=sin, state_out=sout)
    rh, rs, rc = X.exposure_ref(c.color, _all(), c.hit, None, None, _np(sin), **PRM)
    assert np.array_equal(_np(hist).view(u32), rh) and np.array_equal(_np(sout).view(u32), rs.view(u32)) and {k: res["stats"][k] for k in X.COUNTERS} == rc
    r.close()


# ------------------------------------------------------------------ 6. the stream contract
@pytest.mark.parametrize("mode", ["default", "side"])
def test_under_a_busy_torch_stream(ptlib, orc_det, mode):
    """tests/test_gpu_stream_contract.py's protocol for both entry points: the inputs are produced, and the outputs sentinel-filled, by work
    still pending on torch's current stream when the call is made; the result equals the synchronous call's, and that equals the reference"""
    from stream_kit import _pin, _res

    c = _cornell()
    state = np.array([[0.5, 1.5, 0.0, 0.0]], f32)
    outs = dict(hist=torch.zeros((1, 256), dtype=torch.int32, device="cuda:0"), state_out=torch.zeros((1, 4), dtype=torch.float32, device="cuda:0"))

    def meter(dev, outs, returned):
        res = c.r.exposurePlanes(dev["color"], dev["hit"], hist=outs["hist"], state_in=dev["state_in"], state_out=outs["state_out"], rate_up=0.5, rate_down=0.5)
        returned()
        return _res(res, outs)

    sync, got = _pin("exposurePlanes", mode, c.r, dict(color=c.color, hit=c.hit, state_in=state), outs, meter)
    rh, rs, rc = X.exposure_ref(c.color, _all(), c.hit, None, None, state, **dict(PRM, rate_up=0.5, rate_down=0.5))
    assert np.array_equal(got["hist"].view(u32).reshape(1, 256), rh) and np.array_equal(got["state_out"].view(u32).reshape(1, 4), rs.view(u32))
    assert got["stats"] == rc
    outs = {n: _plane(n, H, W) for n in ("out", "frame_rgba8")}

    def tone(dev, outs, returned):
        res = c.r.tonemapPlanes(dev["color"], state=dev["state"], out=outs["out"], frame=outs["frame_rgba8"], op="aces")
        returned()
        return _res(res, outs)

    sync, got = _pin("tonemapPlanes", mode, c.r, dict(color=c.color, state=rs), outs, tone, A=dict(state=np.array([[0, 64.0, 0, 0]], f32)))
    ref = X.tonemap_ref(c.color, _all(), rs, None, op="aces", orc=orc_det)
    for n in ("out", "frame_rgba8"):
        assert not _differ(got[n].view(u32).reshape(H, W, -1), ref[n]).any(), f"{n} under a busy stream [{mode}]"
    assert got["stats"] == dict(pixels=ref["pixels"], clipped=ref["clipped"])


# ------------------------------------------------------------------ 7. the example loops with --auto-exposure
def _example(name):
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def test_upsampled_loop_with_auto_exposure_displays_the_tone_mapped_frame(ptlib):
    """examples/upsampled_svgf_loop.py's UpsampledLoop with auto_exposure at 128 x 56, scale 2, behind edge_aa: the displayed frame is
    tonemapPlanes of the antialiased one under the state the meter left; the state ping-pongs"""
    import surface_ref as S

    ex = _example("upsampled_svgf_loop")
    w, h = 128, 56
    probe = scenes.sky_probe(256, 128).BuildCDF()
    cam0 = dict(eye=(2.0, 0.35, -3.0), lookat=(0.0, 0.2, 0.5), up=(0.0, 1.0, 0.0), fovY=35.0)
    up = ex.UpsampledLoop(S.textured_scene(), (w, h), 2, edge_aa=True, auto_exposure=True, tonemap="aces", probe=probe)
    cam = R.make_camera(cam0, w / h)
    evs = []
    for k in range(3):
        prev, cam = cam, R.make_camera(ex.orbit(cam0, 0.01 * k), w / h)
        x = up.frame(k, prev, cam)
        assert x["pixels"] == w * h and x["exposure_ms"] > 0 and x["tonemap_ms"] > 0 and np.isfinite(x["ev"])
        evs.append(x["ev"])
    state = up.state[up.cur]
    want = up.hi.tonemapPlanes(up.final, state=state, frame=torch.zeros((h, w), dtype=torch.int32, device="cuda:0"), op="aces", write_out=False)
    assert np.array_equal(_np(up.frame_rgba8), _np(want["frame_rgba8"]))
    hist, st = X.meter_ref(_np(up.final), _all(h, w), _np(up.hi_gbuf["hit"]))
    assert np.array_equal(_np(up.hist).view(u32), hist) and float(_np(state)[0, 0]) == evs[-1]
    up.close()
    plain = ex.UpsampledLoop(S.textured_scene(), (w, h), 2, probe=probe)
    assert not plain.auto_exposure
    x = plain.frame(0, cam, cam)
    assert x["exposure_ms"] == 0.0 and x["tonemap_ms"] == 0.0
    plain.close()


def test_adaptive_albedo_loop_runs_with_auto_exposure(ptlib, tmp_path, capsys):
    ex = _example("adaptive_svgf_albedo_loop")
    import sys

    argv = sys.argv
    sys.argv = ["adaptive_svgf_albedo_loop.py", "--size", "128", "56", "--frames", "3", "--edge-aa", "--auto-exposure", "--tonemap", "reinhard", "--out-dir", str(tmp_path)]
    try:
        ex.main()
    finally:
        sys.argv = argv
    out = capsys.readouterr().out
    assert out.count("exposure ") >= 3 and "tone map" in out
    frame = np.load(tmp_path / "adaptive_svgf_albedo_frame.npy")
    assert frame.shape == (56, 128) and (frame >> 24 == 255).all() and len(np.unique(frame)) > 50
