"""Viewports (pt_set_views) on the GPU.  The yardstick is the existing pt_render, which is pinned to the CPU checker and to the reference's own
device programs: a view must hold, bit for bit, what pt_render leaves in a context of the view's own size with the view's camera — in all five
buffers — and a pixel in no view must stay what pt_resize left.  The expectation is built from four separate contexts, one per view, whose
buffers are pasted at the views' origins.  No tolerance anywhere.

Frame 131 x 61 = 17 x 8 blocks, the last column 3 wide, the last row 5 high:
  A  (0, 0)    61 x 37   partial blocks on its right and bottom edges, inside the frame
  B  (64, 0)   67 x 29   ends on the frame's own 3-wide last column
  C  (0, 40)   24 x 21   ends on the frame's 5-high last row
  D  (72, 32)   7 x 5    35 paths: smaller than one block and one packet
Columns 61-63, rows 37-39 and most of the lower right are in no view."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from optixpathtracer_amd import scenes
from parity_kit import _oracle_render
from scene_kit import RECTS, VIEW_H, VIEW_W, _cam_dicts, _rows, _views

pytestmark = pytest.mark.gpu

W, H, SPP, NSUB = VIEW_W, VIEW_H, 2, 3
NBX, NBY = (W + 7) // 8, (H + 7) // 8
CASES = [(False, "0"), (False, "1"), (True, "0"), (True, "1")]
IDS = ["plain-chain", "plain-fused", "catcher-chain", "catcher-fused"]
STAT_SUMS = ("paths", "radiance_rays", "shadow_rays", "shaded_hits")


def _probe():
    return scenes.sky_probe(256, 128).BuildCDF()


def _ctx(monkeypatch, catcher, fused, size=(W, H), cam=None, env=None, partition=None, options=None):
    from optixpathtracer_amd import renderer as R

    env = dict(env or {}, PT_FUSED=fused)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=catcher))
    for k in env:
        monkeypatch.delenv(k)
    r.setProbe(_probe())
    if options:
        r.setOptions(**options)
    if partition:
        r.setPartition(*partition)
    r.resize(size)
    r.setCamera(R.make_camera(cam or scenes.TWO_BOX_CAMERA, size[0] / size[1]))
    r.launchParams.samples_per_launch = SPP
    return r


def _buffers(r):
    return [r.download(k) for k in range(5)]


def _zero():
    return [np.zeros((H, W), np.uint32) if k == 1 else np.zeros((H, W, 4), np.float32) for k in range(5)]


def _same(got, want, what, where=None):
    for k, (x, y) in enumerate(zip(got, want)):
        if where is not None:
            x, y = x[where], y[where]
        if x.dtype == np.uint32:
            assert np.array_equal(x, y), f"{what}: frame buffer differs in {int((x != y).sum())} pixels"
        else:
            assert_bits_equal(x, y, f"{what}: buffer {k}")


_YARDSTICK = {}


def _yardstick(monkeypatch, catcher, fused):
    """(hist, stats): hist[k] = the five expected frame buffers after subframes 0..k — each view's rectangle from a context of the view's own
    size with the view's camera, rendered with the plain pt_render, everything else what pt_resize left (zeros); stats[k] = the sums of the
    four contexts' counters for subframe k.  Computed once per configuration and never modified."""
    key = (catcher, fused)
    if key not in _YARDSTICK:
        hist = [_zero() for _ in range(NSUB)]
        stats = [dict.fromkeys(STAT_SUMS, 0) for _ in range(NSUB)]
        for (x, y, w, h), cam in zip(RECTS, _cam_dicts()):
            r = _ctx(monkeypatch, catcher, fused, size=(w, h), cam=cam)
            assert all(not b.any() for b in _buffers(r))  # what pt_resize leaves
            for k in range(NSUB):
                r.launchParams.frame.subframe_index = k
                r.render()
                for dst, src in zip(hist[k], _buffers(r)):
                    dst[y:y + h, x:x + w] = src
                s = r.stats()
                for name in STAT_SUMS:
                    stats[k][name] += s[name]
            r.close()
        for bufs in hist:
            for b in bufs:
                b.setflags(write=False)
        _YARDSTICK[key] = (hist, stats)
    return _YARDSTICK[key]


def _in_view():
    m = np.zeros((H, W), bool)
    for x, y, w, h in RECTS:
        assert not m[y:y + h, x:x + w].any()
        m[y:y + h, x:x + w] = True
    return m


def _pixel_blocks():
    ys, xs = np.mgrid[0:H, 0:W]
    return (ys // 8) * NBX + xs // 8


def _render_subframes(r, hist=None, stats=None, what=""):
    for k in range(NSUB):
        r.launchParams.frame.subframe_index = k
        r.render()
        if hist is not None:
            _same(_buffers(r), hist[k], f"{what} subframe {k}")
        if stats is not None:
            s = r.stats()
            for name in STAT_SUMS:
                assert s[name] == stats[k][name], (what, k, name, s[name], stats[k][name])


# ------------------------------------------------------------------ 1. views against the yardstick
@pytest.mark.parametrize("catcher,fused", CASES, ids=IDS)
def test_views_hold_the_frames_of_their_own_contexts(ptlib, monkeypatch, catcher, fused):
    hist, stats = _yardstick(monkeypatch, catcher, fused)
    assert stats[0]["paths"] == sum(w * h for _, _, w, h in RECTS) * SPP
    r = _ctx(monkeypatch, catcher, fused)
    r.setViews(_views())
    _render_subframes(r, hist, stats, IDS[CASES.index((catcher, fused))])
    if not catcher:
        assert (r.stats()["fused_passes"] > 0) == (fused == "1")  # both schedules were exercised
    r.close()


# ------------------------------------------------------------------ 2. views against the CPU checker
def test_view_matches_the_cpu_checker(ptlib, orc_det, monkeypatch):
    r = _ctx(monkeypatch, True, "0")
    r.setViews(_views())
    _render_subframes(r)
    got = _buffers(r)
    r.close()
    x, y, w, h = RECTS[0]
    o = _oracle_render(orc_det, scenes.two_box_scene(shadow_catcher=True), _probe(), _cam_dicts()[0], w, h, SPP, subframes=NSUB)
    mine = [g[y:y + h, x:x + w] for g in got]
    want = [np.asarray(o[name]).reshape(g.shape) for name, g in zip(("accum", "frame", "color", "normal", "albedo"), mine)]
    _same(mine, want, "view A against the checker")


# ------------------------------------------------------------------ 3. packets
@pytest.mark.parametrize("env", [{"PT_CAM_PACKETS": "1", "PT_CAM_MIN_PATHS": "0"}, {"PT_CAM_PACKETS": "0"}], ids=["packets", "no-packets"])
def test_views_with_and_without_camera_packets(ptlib, monkeypatch, env):
    """The list's packets mix views here (partial blocks): k_trace8_cam reads origin and direction per lane."""
    hist, stats = _yardstick(monkeypatch, False, "0")
    r = _ctx(monkeypatch, False, "0", env=env)
    r.setViews(_views())
    _render_subframes(r, hist, stats, str(env))
    r.close()


# ------------------------------------------------------------------ 4. batch and frames in flight
def test_views_batch_equals_three_renders(ptlib, monkeypatch):
    hist, _ = _yardstick(monkeypatch, False, "0")
    r = _ctx(monkeypatch, False, "0")
    r.setViews(_views())
    r.launchParams.frame.subframe_index = 0
    r.renderBatch(NSUB)
    _same(_buffers(r), hist[-1], "renderBatch(3)")
    assert r.stats()["paths"] == sum(w * h for _, _, w, h in RECTS) * SPP * NSUB
    r.close()


@pytest.mark.parametrize("inflight", [2, 3])
def test_views_with_frames_in_flight(ptlib, monkeypatch, inflight):
    hist, _ = _yardstick(monkeypatch, False, "0")
    r = _ctx(monkeypatch, False, "0", options=dict(frames_in_flight=inflight))
    r.setViews(_views())
    _render_subframes(r)
    r.sync()
    _same(_buffers(r), hist[-1], f"frames_in_flight={inflight}")
    r.close()


# ------------------------------------------------------------------ 5. one view = the plain frame
@pytest.mark.parametrize("fused", ["0", "1"], ids=["chain", "fused"])
def test_one_full_view_is_the_plain_frame(ptlib, monkeypatch, fused):
    from optixpathtracer_amd import renderer as R

    a, b = _ctx(monkeypatch, False, fused), _ctx(monkeypatch, False, fused)
    b.setViews([(0, 0, W, H, R.make_camera(scenes.TWO_BOX_CAMERA, W / H))])
    names = STAT_SUMS + ("trace_launches", "shadow_launches", "shade_launches", "fused_passes")
    for k in range(NSUB):
        a.launchParams.frame.subframe_index = b.launchParams.frame.subframe_index = k
        a.render()
        b.render()
        _same(_buffers(b), _buffers(a), f"subframe {k}")
        sa, sb = a.stats(), b.stats()
        for name in names:
            assert sa[name] == sb[name], (k, name, sa[name], sb[name])
    a.close()
    b.close()


def test_dropping_the_views_restores_the_single_camera(ptlib, monkeypatch):
    a = _ctx(monkeypatch, False, "0")
    b = _ctx(monkeypatch, False, "0")
    b.setViews(_views())
    _render_subframes(b)
    b.setViews([])
    assert b.views() == []
    b.resize((W, H))  # fresh buffers; the camera of setCamera is in force again
    for k in range(NSUB):
        a.launchParams.frame.subframe_index = b.launchParams.frame.subframe_index = k
        a.render()
        b.render()
        _same(_buffers(b), _buffers(a), f"subframe {k} after setViews([])")
    assert a.stats()["paths"] == b.stats()["paths"] == W * H * SPP
    a.close()
    b.close()


# ------------------------------------------------------------------ 6. partition
def test_views_on_a_partitioned_context(ptlib, monkeypatch):
    hist, _ = _yardstick(monkeypatch, False, "0")
    inview = _in_view()
    by, bx = np.mgrid[0:NBY, 0:NBX]
    union = _zero()
    seen = np.zeros((H, W), bool)
    for rank in (0, 1):
        r = _ctx(monkeypatch, False, "0", partition=(rank, 2, 16, 8))
        r.setViews(_views())
        _render_subframes(r)
        got = _buffers(r)
        mine = ((((bx * 8) // 16 + (by * 8) // 8) % 2) == rank).reshape(-1)[_pixel_blocks()] & inview
        assert mine.any() and r.stats()["paths"] == int(mine.sum()) * SPP
        _same(got, hist[-1], f"rank {rank}: owned view pixels", mine)
        _same(got, _zero(), f"rank {rank}: every other pixel", ~mine)
        for u, g in zip(union, got):
            u[mine] = g[mine]
        assert not (seen & mine).any()
        seen |= mine
        r.close()
    assert np.array_equal(seen, inview)
    _same(union, hist[-1], "union of the ranks")


# ------------------------------------------------------------------ 7. mask
def test_views_under_a_block_mask(ptlib, monkeypatch):
    hist, _ = _yardstick(monkeypatch, False, "0")
    inview = _in_view()
    pb = _pixel_blocks()
    view_px = np.bincount(pb[inview], minlength=NBX * NBY)  # view pixels per block
    mask = np.random.default_rng(23).random(NBX * NBY) < 0.5
    for x, y, w, h in RECTS[:3]:  # the mask leaves out some blocks of every view that has several, and names some
        blocks = np.unique(pb[y:y + h, x:x + w])
        assert mask[blocks].any() and not mask[blocks].all()
    mask[pb[RECTS[3][1], RECTS[3][0]]] = True  # D is a single block: named
    assert (mask & (view_px == 0)).any()  # blocks without view pixels are named too
    named = mask[pb] & inview
    r = _ctx(monkeypatch, False, "0")
    r.setViews(_views())
    for k in range(2):
        r.launchParams.frame.subframe_index = k
        host = np.zeros((H, W), np.uint32)
        got = r.renderMask(mask.reshape(NBY, NBX), host)
        assert got == int(view_px[mask].sum()) == int(named.sum()), got
        assert r.stats()["paths"] == got * SPP
        bufs = _buffers(r)
        _same(bufs, hist[k], f"masked subframe {k}: named blocks' view pixels", named)
        _same(bufs, _zero(), f"masked subframe {k}: everything else", ~named)
        assert np.array_equal(host, bufs[1])
    before = _buffers(r)
    r.launchParams.frame.subframe_index = 2
    assert r.renderMask((view_px == 0).reshape(NBY, NBX)) == 0  # only view-less blocks: nothing to launch, PT_OK
    s = r.stats()
    assert s["paths"] == 0 and s["trace_launches"] == 0 and s["shade_launches"] == 0
    _same(_buffers(r), before, "a mask of view-less blocks")
    r.close()


# ------------------------------------------------------------------ 8. camera setters
def test_view_camera_setters(ptlib, monkeypatch):
    import torch

    hist, stats = _yardstick(monkeypatch, False, "0")
    rows = _rows(_views())
    elsewhere = _views([scenes.TWO_BOX_CAMERA] * 4)  # the rectangles with other cameras
    r = _ctx(monkeypatch, False, "0")
    r.setViews(elsewhere)
    r.setViewCameras(rows)  # a host array
    back = r.views()
    assert [(v["x"], v["y"], v["width"], v["height"]) for v in back] == RECTS
    assert np.array_equal(np.stack([np.concatenate([v["eye"], v["U"], v["V"], v["W"]]) for v in back]), rows)
    _render_subframes(r, hist, stats, "setViewCameras(host array)")
    r.resize((W, H))  # drops the views, fresh buffers
    r.setViews(elsewhere)
    flat = torch.zeros(1 + rows.size + 3, dtype=torch.float32, device="cuda:0")
    t = flat[1:1 + rows.size].view(4, 12)  # offset by one float: only 4-byte aligned
    t.copy_(torch.from_numpy(rows))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    r.setViewCameras(t)
    back = r.views()
    assert np.array_equal(np.stack([np.concatenate([v["eye"], v["U"], v["V"], v["W"]]) for v in back]), rows)
    _render_subframes(r, hist, stats, "setViewCameras(CUDA tensor)")
    r.setViewCameras([v[4] for v in _views()])  # ... and a list of Cameras gives the same rows
    assert np.array_equal(np.stack([np.concatenate([v["eye"], v["U"], v["V"], v["W"]]) for v in r.views()]), rows)
    r.close()


# ------------------------------------------------------------------ 9. multi
def test_views_on_a_multi_renderer(ptlib, monkeypatch):
    from optixpathtracer_amd import renderer as R

    hist, _ = _yardstick(monkeypatch, False, "0")
    m = R.MultiRenderer(scenes.two_box_scene(shadow_catcher=False), devices=(0, 0))
    m.setProbe(_probe())
    m.resize((W, H))
    m.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, W / H))
    m.setViews(_views())
    assert len(m.views()) == 4
    m.launchParams.samples_per_launch = SPP
    m.gather_mask = 0b11111  # all five buffers are assembled on every rank
    for k in range(NSUB):
        m.launchParams.frame.subframe_index = k
        m.render()
        _same([m.download(b, rank=0) for b in range(5)], hist[k], f"multi subframe {k}")
    assert m.stats()["paths"] == sum(w * h for _, _, w, h in RECTS) * SPP
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        m.renderFoveated((60, 30), inner_radius=5, outer_radius=12)
    m.setViewCameras(_rows(_views()))
    m.launchParams.frame.subframe_index = 0
    m.render()
    _same([m.download(b, rank=0) for b in range(5)], hist[0], "multi after setViewCameras and a refused foveated frame")
    m.close()


# ------------------------------------------------------------------ 10. refusals
def test_refusals_change_nothing(ptlib, monkeypatch):
    from optixpathtracer_amd import _lib
    from optixpathtracer_amd import renderer as R

    import torch

    hist, _ = _yardstick(monkeypatch, False, "0")
    L = _lib.load_library()
    good = _views()
    cam = good[0][4]

    fresh = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    with pytest.raises(RuntimeError, match=r"\(-1\).*pt_resize"):
        fresh.setViews(good)  # no pt_resize yet
    assert fresh.views() == []
    fresh.close()

    r = _ctx(monkeypatch, False, "0")
    r.setViews(good)

    def unchanged(what):
        """subframe 0 does not blend with the previous accum value: rendering it again must give the expected first frame"""
        assert [(v["x"], v["y"], v["width"], v["height"]) for v in r.views()] == RECTS, what
        r.launchParams.frame.subframe_index = 0
        r.render()
        _same(_buffers(r), hist[0], f"the frame after {what}")

    def refused(what, call, code=-1):
        with pytest.raises(RuntimeError, match=r"\(%d\)" % code):
            call()
        unchanged(what)

    unchanged("setViews")
    arr = R._view_array(good)
    assert L.pt_set_views(None, arr, 4) == -1  # null context
    unchanged("a null context")
    assert L.pt_set_views(r._ctx, None, 4) == -1 and b"null views" in L.pt_last_error(r._ctx)
    unchanged("null views with n > 0")
    many = (_lib.View * (_lib.PT_MAX_VIEWS + 1))()
    assert L.pt_set_views(r._ctx, many, _lib.PT_MAX_VIEWS + 1) == -1 and b"PT_MAX_VIEWS" in L.pt_last_error(r._ctx)
    unchanged("n > PT_MAX_VIEWS")
    for what, rect in [("negative x", (-8, 0, 16, 16)), ("negative y", (0, -8, 16, 16)), ("x not a multiple of 8", (4, 0, 16, 16)),
                       ("y not a multiple of 8", (0, 12, 16, 16)), ("width < 1", (0, 0, 0, 16)), ("height < 1", (0, 0, 16, -1)),
                       ("a rectangle leaving the frame on the right", (128, 0, 4, 8)), ("a rectangle leaving the frame at the bottom", (0, 56, 8, 6)),
                       ("an origin outside the frame", (136, 0, 8, 8))]:
        refused(what, lambda: r.setViews([good[1], rect + (cam,)]))
    refused("two rectangles sharing a pixel", lambda: r.setViews([(0, 0, 61, 37, cam), (56, 32, 8, 8, cam)]))
    rows = _rows(good)
    refused("a camera setter with the wrong n", lambda: r.setViewCameras(rows[:3]))
    refused("the device setter with the wrong n", lambda: r.setViewCameras(torch.zeros((5, 12), dtype=torch.float32, device="cuda:0")))
    assert L.pt_set_view_cameras_device(r._ctx, rows.ctypes.data, 4) == -1 and b"not device memory" in L.pt_last_error(r._ctx)
    unchanged("a host pointer given to the device setter")
    assert L.pt_set_view_cameras_device(r._ctx, None, 4) == -1 and b"null" in L.pt_last_error(r._ctx)
    unchanged("a null pointer given to the device setter")
    refused("renderRegions", lambda: r.renderFoveated((60, 30), inner_radius=5, outer_radius=12), code=-4)
    refused("adaptiveBegin", lambda: r.adaptiveBegin(), code=-4)
    r.resize((W, H))  # drops the views
    assert r.views() == []
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        r.setViewCameras(rows)
    r.setViews(good)
    unchanged("resize and a new setViews")
    r.close()
