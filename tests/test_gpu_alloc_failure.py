"""Allocation failures at every allocation site of the C ABI (the host-side hook PT_ALLOC_FAIL_AT=k: the k-th device allocation returns
hipErrorOutOfMemory without calling hipMalloc).  Every call that replaces a resource group is run with k = 1, 2, ... until it succeeds — that
count is the number of allocations the call makes, and it must be at least the number of arrays in the group, so a hook that never fires
cannot pass.  A failed call returns PT_ERR_HIP and leaves what a fresh context has: no frame size, "no probe set", no path state, the smaller
query state.  Rendering entry points are reached only behind the host-side asserts that prove the state was reset: no test launches on freed
memory.  With the hook cleared the same call succeeds and the next frame — five buffers, three device-counted totals — equals, bit for
bit, that of a context that never saw a failure; pt_stats.path_state_allocs is that context's plus the failed attempts."""
import functools
import os

import numpy as np
import pytest
import torch

from optixpathtracer_amd import scenes
from optixpathtracer_amd import renderer as R
from parity_kit import _random_rays

pytestmark = pytest.mark.gpu

HOOK = "PT_ALLOC_FAIL_AT"
W, H = 64, 48
BUFFERS = (R.PT_BUF_ACCUM, R.PT_BUF_FRAME, R.PT_BUF_COLOR, R.PT_BUF_NORMAL, R.PT_BUF_ALBEDO)
TOTALS = ("radiance_rays", "shadow_rays", "shaded_hits")
MODELS = {"cornell": (scenes.cornell_box, scenes.CORNELL_CAMERA), "two_box": (scenes.two_box_scene, scenes.TWO_BOX_CAMERA),
          "textured": (scenes.textured_scene, scenes.TWO_BOX_CAMERA)}
# arrays of one batch set (ensure_path_state): 2 x 5 ray streams, 3 shadow records, flags, 4 sums, 3 queues, counters, 2 spill stacks, 4 pixel
# sums = 28; carried sums (no shadow catcher) 5 more; a catcher scene 3 more; asynchronous shadow rays 6 more
SET_ARRAYS = 28


@pytest.fixture(autouse=True)
def fixed_schedule(monkeypatch):
    """launch chains only, no measured trial: the number of batch sets is pt_options.streams"""
    monkeypatch.delenv(HOOK, raising=False)
    monkeypatch.setenv("PT_FUSED", "0")
    monkeypatch.setenv("PT_SCHED_TRIALS", "0")
    yield
    os.environ.pop(HOOK, None)


@functools.lru_cache(maxsize=None)
def _probe(tall):
    """16 x 8, or 32 wide and PT_CDF_BLOCK (64) rows high, so that the coarse row tables are allocated"""
    return scenes.sky_probe(32, 64).BuildCDF() if tall else scenes.sky_probe(16, 8).BuildCDF()


def _set_probe(r, tall=False, image=True):
    r.setProbeImage(_probe(tall).data) if image else r.setProbe(_probe(tall))


def _context(model="cornell", created=None, **opt):
    make, cam = MODELS[model]
    r = created or R.SampleRenderer(make())
    _set_probe(r)
    r.resize((W, H))
    r.setCamera(R.make_camera(cam, W / H))
    r.setOptions(**{"streams": 1, **opt})
    r.launchParams.samples_per_launch = 1
    r.launchParams.frame.subframe_index = 0
    return r


def _frame(r):
    r.render()
    st = r.stats()
    return {**{b: r.download(b) for b in BUFFERS}, **{t: st[t] for t in TOTALS}, "allocs": st["path_state_allocs"]}


@functools.lru_cache(maxsize=None)
def _untroubled(model="cornell", tall=False, image=True, **opt):
    """the frame of a context that never saw a failure (computed once per configuration, with the hook unset)"""
    assert HOOK not in os.environ
    r = _context(model, **opt)
    _set_probe(r, tall, image)
    f = _frame(r)
    r.close()
    return f


def _recovered(r, failed_renders=0, **config):
    """the next frame of a context that has seen failures equals the untroubled context's"""
    assert HOOK not in os.environ
    got, ref = _frame(r), _untroubled(**config)
    for b in BUFFERS:
        assert got[b].tobytes() == ref[b].tobytes(), f"buffer {b} differs after the recovery"
    for t in TOTALS:
        assert got[t] == ref[t], t
    assert got["allocs"] == ref["allocs"] + failed_renders


def _fails_at(k, call):
    """the error of call() with the k-th allocation failing, None if it succeeded; the hook is cleared again either way"""
    os.environ[HOOK] = str(k)
    try:
        call()
        return None
    except RuntimeError as e:
        return str(e)
    finally:
        del os.environ[HOOK]


def _sweep(call, after_failure, before=lambda: None, at_least=1):
    """call() failing at k = 1, 2, ... until it succeeds (before(): what puts the state back that a failed call has unset).  Returns the
    number of failures = the allocations of the call."""
    k = 1
    while True:
        before()
        err = _fails_at(k, call)
        if err is None:
            break
        assert "(-2)" in err and err.split("): ", 1)[1], err  # PT_ERR_HIP and a message
        after_failure()
        k += 1
        assert k < 400, "the call never succeeds"
    assert k - 1 >= at_least, f"{k - 1} allocations failed, the group has {at_least} arrays: the hook did not reach them"
    return k - 1


def _small_query(r):
    rays = torch.from_numpy(_random_rays(np.random.default_rng(3), 64, 0.0, 550.0)).to("cuda:0")
    return r.traceDevice(rays)["record"].cpu().numpy().tobytes()


def test_resize_failure_leaves_no_frame():
    r = _context()
    frames = r.stats()["frames"]

    def unset():
        assert all(not r.deviceBuffer(b) for b in (*BUFFERS, R.PT_BUF_DENOISED))
        assert r.ownedPixels() == (0, 0)
        r.render()  # only behind the asserts above: PT_OK, and nothing is rendered
        assert r.stats()["frames"] == frames

    _sweep(lambda: r.resize((W, H)), unset, before=lambda: r.resize((W, H)), at_least=7)
    _recovered(r)


def _multi():
    """two ranks on one device, two frames in flight and a hand-over of the frame buffer: pt_multi_render takes the overlapped path"""
    m = R.MultiRenderer(scenes.cornell_box(), devices=(0, 0))
    m.setProbe(_probe(False))
    m.setCamera(R.make_camera(scenes.CORNELL_CAMERA, W / H))
    m.setOptions(streams=1, frames_in_flight=2)
    m.launchParams.samples_per_launch = 1
    m.launchParams.frame.subframe_index = 0
    m.gather_mask = 1 << R.PT_BUF_FRAME
    return m


def test_multi_resize_failure_leaves_no_rank_with_a_frame():
    """A pt_multi_resize that fails — in any rank's pt_resize or in the exchange strips — leaves every rank without a frame and the pt_multi
    without strips, so the overlapped hand-off never packs a rank's pixels into strips sized by padded = 0."""
    m = _multi()
    ranks = [m.rank(0), m.rank(1)]

    def unset():
        for v in ranks:
            assert all(not v.deviceBuffer(b) for b in (*BUFFERS, R.PT_BUF_DENOISED))
            assert v.ownedPixels() == (0, 0)
        with pytest.raises(RuntimeError, match=r"\(-1\).*not resized"):
            m.gather(R.PT_BUF_FRAME)
        frames = m.stats()["frames"]
        m.render()  # only behind the asserts above: PT_OK, nothing is rendered and nothing is packed
        st = m.stats()
        assert st["frames"] == frames and st["frames_handed_over"] == 0

    # per rank the frame's 7 arrays, then per rank the 2 strips of the synchronous gather
    _sweep(lambda: m.resize((W, H)), unset, before=lambda: m.resize((W, H)), at_least=2 * 7 + 2 * 2)
    ref = _multi()
    ref.resize((W, H))
    for x in (m, ref):
        x.render()
        x.flush()
    for rank in (0, 1):
        assert m.downloadDisplay(R.PT_BUF_FRAME, rank).tobytes() == ref.downloadDisplay(R.PT_BUF_FRAME, rank).tobytes()
        for b in BUFFERS:
            assert m.download(b, rank).tobytes() == ref.download(b, rank).tobytes(), f"rank {rank}, buffer {b} differs after the recovery"
    assert m.stats()["frames_handed_over"] == ref.stats()["frames_handed_over"] == 1
    for t in TOTALS:
        assert m.stats()[t] == ref.stats()[t], t
    ref.close()
    m.close()


@pytest.mark.parametrize("image", [True, False], ids=["pt_set_probe_image", "pt_set_probe"])
def test_probe_failure_leaves_no_probe(image):
    r = _context()

    def unset():
        with pytest.raises(RuntimeError, match="no probe set"):
            r.probeCDF()
        with pytest.raises(RuntimeError, match=r"\(-1\).*no probe set"):  # only behind the assert above
            r.render()

    _sweep(lambda: _set_probe(r, True, image), unset, before=lambda: _set_probe(r), at_least=9 + image)
    _recovered(r, tall=True, image=image)


@pytest.mark.parametrize("model,opt,arrays", [("cornell", {}, SET_ARRAYS + 5), ("cornell", {"split_shadow": 2}, SET_ARRAYS + 11),
                                              ("two_box", {}, SET_ARRAYS + 3)], ids=["cornell", "async-shadows", "shadow-catcher"])
def test_path_state_failure_one_set(model, opt, arrays):
    r = _context(model, **opt)
    n = _sweep(r.render, r.stats, at_least=arrays)
    _recovered(r, failed_renders=n, model=model, **opt)  # (every failed render counts as a (re-)allocation of the path state)


def test_path_state_failure_three_sets():
    one = _context()
    n1 = _sweep(one.render, one.stats, at_least=SET_ARRAYS + 5)
    one.close()
    r = _context(streams=3)
    n3 = 3 * n1  # (the stream probe's two stamp words are allocated once per context, by the first attempt that gets past them: k = 1 fails there)
    for k in (1, (n3 + 1) // 2, n3):
        err = _fails_at(k, r.render)
        assert err is not None and "(-2)" in err, (k, err)
        r.stats()
    assert _fails_at(n3 + 1, r.render) is None  # n3 was the last
    _recovered(r, failed_renders=3, streams=3)


def test_block_table_adaptive_and_views_failures():
    r = _context()
    _frame(r)  # the path state is there: the sweeps below reach the block table, the adaptive state and the views alone
    hits = _small_query(r)
    nby, nbx = r.blockGrid()
    still = lambda: _small_query(r) == hits or pytest.fail("the small query changed")  # noqa: E731
    _sweep(lambda: r.renderMask(np.ones((nby, nbx), np.uint8)), still, at_least=6)
    _recovered(r)
    # a new frame has no block table: every attempt builds it again (a complete table survives the failure of the adaptive arrays behind it)
    _sweep(r.adaptiveBegin, still, before=lambda: r.resize((W, H)), at_least=6 + 3)
    r.adaptiveEnd()
    _recovered(r)

    def no_views():
        assert r.views() == []
        still()

    view = [(0, 0, 32, 24, R.make_camera(scenes.CORNELL_CAMERA, 32 / 24))]
    _sweep(lambda: r.setViews(view), no_views, at_least=3)
    r.setViews([])
    _recovered(r)


def test_query_and_update_staging_failures():
    r = _context()
    hits = _small_query(r)
    large = torch.from_numpy(_random_rays(np.random.default_rng(4), 256, 0.0, 550.0)).to("cuda:0")
    still = lambda: _small_query(r) == hits or pytest.fail("the small query changed")  # noqa: E731
    _sweep(lambda: r.traceDevice(large), still, at_least=4)
    verts = scenes.cornell_box().meshes[0].vertex
    dev = {0: torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to("cuda:0")}

    def unchanged():
        assert r.downloadVertices(0).tobytes() == np.ascontiguousarray(verts, np.float32).tobytes()
        still()

    _sweep(lambda: r.updateMeshesDevice(dev, rebuild=True), unchanged, at_least=3)
    _recovered(r)


def test_create_failure():
    made = []

    def create():
        made.append(R.SampleRenderer(scenes.textured_scene()))

    # 4 scene arrays, the texcoords per vertex and per primitive, the meshes' textures, 2 textures and their table, 2 side arrays, totals, spill stack
    _sweep(create, lambda: None, at_least=14)
    assert len(made) == 1
    _recovered(_context("textured", created=made[0]), model="textured")
