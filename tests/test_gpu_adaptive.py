"""pt_render_mask and pt_render_adaptive on the GPU.  The yardstick is the existing pt_render, which is pinned to the CPU checker bit for
bit: a pixel's result depends on nothing but (x, y, subframe_index, spp) and its own previous accum value, so rendering a subset of the 8x8
blocks must leave, in those blocks, the bits of the full frames — in all five buffers — and must leave every other pixel alone.  The policy
(per-pixel moments, stopping rule) is checked against the numpy float32 transcription of tests/test_adaptive_cabi.py.  No tolerance anywhere."""
import numpy as np
import pytest

from adaptive_ref import block_slots, rule_sides, stop_rule
from conftest import assert_bits_equal
from optixpathtracer_amd import scenes

pytestmark = pytest.mark.gpu

W, H, SPP = 203, 117, 2  # edge blocks on both sides: 26 x 15 blocks, the last column 3 wide, the last row 5 high
NBX, NBY = (W + 7) // 8, (H + 7) // 8
CASES = [(False, "0"), (False, "1"), (True, "0"), (True, "1")]
IDS = ["plain-chain", "plain-fused", "catcher-chain", "catcher-fused"]


def _ctx(monkeypatch, catcher, fused, env=None, partition=None):
    from optixpathtracer_amd import renderer as R

    env = dict(env or {}, PT_FUSED=fused)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=catcher))
    for k in env:
        monkeypatch.delenv(k)
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    if partition:
        r.setPartition(*partition)
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, W / H))
    r.launchParams.samples_per_launch = SPP
    return r


def _buffers(r):
    return [r.download(k) for k in range(5)]


def _same(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        if x.dtype == np.uint32:
            assert np.array_equal(x, y), f"{what}: frame buffer differs in {int((x != y).sum())} pixels"
        else:
            assert_bits_equal(x, y, f"{what}: buffer {k}")


def _plain_history(r, n):
    """H[k] = the five buffers after plain subframes 0..k"""
    hist = []
    for k in range(n):
        r.launchParams.frame.subframe_index = k
        r.render()
        hist.append(_buffers(r))
    return hist


def _pixel_blocks():
    ys, xs = np.mgrid[0:H, 0:W]
    return (ys // 8) * NBX + xs // 8


def _owned_blocks(partition):
    if not partition:
        return np.ones(NBX * NBY, bool)
    rank, world, tw, th = partition
    by, bx = np.mgrid[0:NBY, 0:NBX]
    return ((((bx * 8) // tw + (by * 8) // th) % world) == rank).reshape(-1)


def _block_pixels():
    return block_slots(np.ones((H, W), bool), False).sum(1)


def _expected(hist, last_block, zero):
    """per pixel: hist[k] where the pixel's block was last rendered at subframe k, what pt_resize left (zeros) where it never was"""
    last = last_block[_pixel_blocks()]
    out = []
    for b in range(5):
        e = zero[b].copy()
        for k in range(len(hist)):
            e[last == k] = hist[k][b][last == k]
        out.append(e)
    return out


def _nested_masks(seed, n):
    u = np.random.default_rng(seed).random(NBX * NBY)
    cuts = np.linspace(0.15, 0.85, n - 1).tolist() + [2.0]  # the first mask already leaves blocks out, the last is empty
    return [u >= c for c in cuts]


@pytest.mark.parametrize("catcher,fused", CASES, ids=IDS)
def test_all_blocks_active_is_the_plain_frame(ptlib, monkeypatch, catcher, fused):
    a, b = _ctx(monkeypatch, catcher, fused), _ctx(monkeypatch, catcher, fused)
    ones = np.ones((NBY, NBX), np.uint8)
    for k in range(4):
        a.launchParams.frame.subframe_index = b.launchParams.frame.subframe_index = k
        a.render()
        host = np.zeros((H, W), np.uint32)
        assert b.renderMask(ones, host) == W * H
        sa, sb = a.stats(), b.stats()
        for name in ("radiance_rays", "shadow_rays", "shaded_hits", "paths"):
            assert sa[name] == sb[name], (k, name, sa[name], sb[name])
        _same(_buffers(a), _buffers(b), f"subframe {k}")
        assert np.array_equal(host, b.downloadPixels())
    a.close()
    b.close()


def _run_nested(monkeypatch, catcher, fused, partition):
    n = 6
    ref = _ctx(monkeypatch, catcher, fused, partition=partition)
    zero = _buffers(ref)
    assert all(not z.any() for z in zero)
    hist = _plain_history(ref, n)
    ref.close()
    r = _ctx(monkeypatch, catcher, fused, partition=partition)
    owned = _owned_blocks(partition)
    masks = _nested_masks(11, n)
    last_block = np.full(NBX * NBY, -1)
    npx = _block_pixels()
    for k, m in enumerate(masks):
        assert k == 0 or not (m & ~masks[k - 1]).any()
        r.launchParams.frame.subframe_index = k
        got = r.renderMask(m.reshape(NBY, NBX))
        assert got == int(npx[m & owned].sum()), (k, got)
        assert r.stats()["paths"] == got * SPP
        last_block[m & owned] = k
        _same(_buffers(r), _expected(hist, last_block, zero), f"after masked subframe {k}")
    assert not masks[-1].any() and r.stats()["trace_launches"] == 0 and r.stats()["shade_launches"] == 0
    assert (last_block[owned] == -1).any() and (last_block[owned] == n - 2).any()
    if partition:  # only owned pixels ever changed
        other = ~owned[_pixel_blocks()]
        for z, g in zip(zero, _buffers(r)):
            assert np.array_equal(z[other], g[other])
    r.close()


@pytest.mark.parametrize("catcher,fused", CASES, ids=IDS)
def test_nested_masks_leave_each_block_at_its_last_subframe(ptlib, monkeypatch, catcher, fused):
    _run_nested(monkeypatch, catcher, fused, None)


@pytest.mark.parametrize("catcher,fused", CASES, ids=IDS)
def test_nested_masks_on_a_partitioned_context(ptlib, monkeypatch, catcher, fused):
    _run_nested(monkeypatch, catcher, fused, (1, 3, 64, 16))


@pytest.mark.parametrize("catcher,fused", CASES, ids=IDS)
def test_masked_frames_leave_schedule_and_path_state_alone(ptlib, monkeypatch, catcher, fused):
    """The measured chain/fused trial (times replaced by constants: PT_SCHED_FAKE) is settled by plain frames; masked frames in between
    neither enter nor restart it and allocate no path state.  The trial only runs for the scene without catcher materials under PT_FUSED=1:
    that case carries the schedule half of the requirement (it asserts the settled choice and its two times); the other three can only
    take the launch chain, so for them this checks the path state (and that the schedule word stays 0)."""
    env = {"PT_SCHED_TRIALS": "3", "PT_SCHED_FAKE": "2.0,1.0", "PT_SCHED_PROBE": "0"}
    r = _ctx(monkeypatch, catcher, fused, env)
    keys = ("schedule", "sched_chain_ms", "sched_fused_ms", "path_state_allocs", "fused_passes")
    for k in range(10):
        r.launchParams.frame.subframe_index = k
        r.render()
    settled = {n: r.stats()[n] for n in keys}
    assert not settled["schedule"] & 0x100
    if not catcher and fused == "1":
        assert settled["schedule"] & 1 and settled["sched_chain_ms"] == 2.0 and settled["sched_fused_ms"] == 1.0
    rng = np.random.default_rng(5)
    for k in range(10, 16):
        m = rng.random(NBX * NBY) < (0.3 if k % 2 else 0.9)
        r.launchParams.frame.subframe_index = k
        r.renderMask(m)
        assert r.stats()["path_state_allocs"] == settled["path_state_allocs"], k
        r.render()  # (blends subframe k twice into the masked blocks: this test compares the context's state, not images)
        assert {n: r.stats()[n] for n in keys} == settled, k
    r.close()


@pytest.mark.parametrize("catcher,fused", CASES, ids=IDS)
def test_small_mask_first_does_not_shrink_later_frames(ptlib, monkeypatch, catcher, fused):
    """A context whose FIRST frame is a one-block mask allocates a small path state; later masked frames must grow it to the full frame's
    shape instead of being cut into chunks of that first frame: same images as render(), and as many launches as the plain frame."""
    ref = _ctx(monkeypatch, catcher, fused)
    hist, plain = [], []
    for k in range(2):
        ref.launchParams.frame.subframe_index = k
        ref.render()
        hist.append(_buffers(ref))
        plain.append(ref.stats())
    ref.close()
    r = _ctx(monkeypatch, catcher, fused)
    one = np.zeros((NBY, NBX), np.uint8)
    one[NBY // 2, NBX // 2] = 1
    ones = np.ones((NBY, NBX), np.uint8)
    r.launchParams.frame.subframe_index = 0
    assert r.renderMask(one) == 64 and r.stats()["path_state_allocs"] == 1
    for k in range(2):  # subframe 0 again for the one block: it does not blend, so the image is plain subframe 0
        r.launchParams.frame.subframe_index = k
        assert r.renderMask(ones) == W * H
        st = r.stats()
        for name in ("trace_launches", "shade_launches", "shadow_launches", "fused_passes", "radiance_rays", "shadow_rays"):
            assert st[name] == plain[k][name], (k, name, st[name], plain[k][name])
        _same(_buffers(r), hist[k], f"all blocks after a one-block first frame, subframe {k}")
    assert r.stats()["path_state_allocs"] == 2  # grown once, to the full frame's shape
    r.adaptiveBegin(threshold=0.0, dark_floor=0.0, min_subframes=1000)
    r.launchParams.frame.subframe_index = 0
    r.renderAdaptive()
    assert r.stats()["trace_launches"] == plain[0]["trace_launches"] and r.stats()["path_state_allocs"] == 2
    r.close()


@pytest.mark.parametrize("catcher,fused", CASES, ids=IDS)
def test_masked_frame_cut_to_the_full_frames_chunks(ptlib, monkeypatch, catcher, fused):
    """The branch in which a masked frame is really limited by the path state of the full frame, against an independent reference: with
    PT_FUSED_MAX_PATHS between the two path counts the full frame is a launch chain on three sets of a third of the pixels each, and a mask of
    half the blocks is small enough for the fused pass but larger than one set: it runs as two fused chunks, allocates nothing, and leaves the
    bits of the plain frames."""
    env = {"PT_FUSED_MAX_PATHS": "30000"}
    ref = _ctx(monkeypatch, catcher, fused, env)
    hist = _plain_history(ref, 3)
    ref.close()
    r = _ctx(monkeypatch, catcher, fused, env)
    r.launchParams.frame.subframe_index = 0
    r.render()
    full = r.stats()
    assert full["fused_passes"] == 0 and full["paths"] == W * H * SPP > 30000
    m = np.random.default_rng(9).random(NBX * NBY) < 0.5
    last_block = np.zeros(NBX * NBY, int)
    for k in (1, 2):
        r.launchParams.frame.subframe_index = k
        got = r.renderMask(m)
        assert (W * H + 2) // 3 < got and got * SPP <= 30000, got  # more than one set's pixels, few enough paths for the fused pass
        st = r.stats()
        assert st["path_state_allocs"] == full["path_state_allocs"]
        if not catcher and fused == "1":
            assert st["fused_passes"] == 2 and st["trace_launches"] == 2, st
        last_block[m] = k
        _same(_buffers(r), _expected(hist, last_block, hist[0]), f"masked subframe {k}")
    r.close()


@pytest.mark.parametrize("catcher,fused", CASES, ids=IDS)
def test_masked_call_is_synchronous_with_frames_in_flight(ptlib, monkeypatch, catcher, fused):
    a, b = _ctx(monkeypatch, catcher, fused), _ctx(monkeypatch, catcher, fused)
    b.setOptions(frames_in_flight=3)
    m = np.random.default_rng(2).random(NBX * NBY) < 0.4
    for k in range(3):
        a.launchParams.frame.subframe_index = b.launchParams.frame.subframe_index = k
        if k < 2:
            a.render()
            b.render()  # enqueued, not waited for
        else:
            na = a.renderMask(m)
            host = np.zeros((H, W), np.uint32)
            nb = b.renderMask(m, host)
            assert na == nb == int(_block_pixels()[m].sum())
            assert np.array_equal(host, a.downloadPixels())
    _same(_buffers(a), _buffers(b), "masked call after two frames in flight")
    a.close()
    b.close()


def _luminance(c):
    f = np.float32
    return ((f(0.2126) * c[..., 0]).astype(f) + (f(0.7152) * c[..., 1]).astype(f)).astype(f) + (f(0.0722) * c[..., 2]).astype(f)


@pytest.mark.parametrize("fused", ["0", "1"], ids=["chain", "fused"])
def test_moments_are_the_sums_of_the_pre_blend_luminance(ptlib, monkeypatch, fused):
    """The pre-blend colour of subframe k comes from the existing product path: one full-image pt_region (factor 1, fill 1, redraw) writes the
    unblended, unclamped accum_color of subframe k; the clamp of k > 0 is applied here."""
    n = 5
    r, q = _ctx(monkeypatch, False, fused), _ctx(monkeypatch, False, fused)
    r.adaptiveBegin(threshold=0.0, dark_floor=0.0, min_subframes=1000)
    want = np.zeros((H, W, 4), np.float32)
    first = None
    for k in range(n):
        r.launchParams.frame.subframe_index = k
        st = r.renderAdaptive()
        assert st["active_pixels"] == W * H and st["active_blocks"] == st["blocks"] == NBX * NBY and st["pixel_subframes"] == (k + 1) * W * H
        if k == 0:
            first = r.download(0)
        q.renderRegions([dict(launch_w=W, launch_h=H, factor_x=1, factor_y=1, fill_size=1, cx=0, cy=0, r_inner=0.0, r_outer=1.0e9,
                              offset_x=0, offset_y=0, redraw=1, spp=SPP, subframe_index=k)])
        c = q.download(0)[..., :3]
        if k == 0:
            assert_bits_equal(c, first[..., :3], "the region route gives subframe 0's own colour")
        else:
            c = np.minimum(np.maximum(c, np.float32(0)), np.float32(10))
        x = _luminance(c)
        want[..., 0] += np.float32(1)
        want[..., 1] += x
        want[..., 2] += (x * x).astype(np.float32)
    mo, active = r.adaptiveArrays()
    assert active.all()
    assert_bits_equal(mo, want, "PT_ADAPT_MOMENTS")
    r.close()
    q.close()


def _median_threshold(mo, dark_floor):
    """the smallest float32 threshold with which the median block (by its critical threshold) passes the rule at the moments `mo`"""
    f = np.float32
    blocks = np.arange(NBX * NBY)
    n, V, M, N = rule_sides(mo, blocks)
    B = (M + (f(dark_floor) * N).astype(f)).astype(np.float64)
    crit = np.sqrt((V * N).astype(np.float64) / ((n.astype(np.float64) - 1.0) * B * B))
    t = f(np.sort(crit)[len(crit) // 2])
    for _ in range(64):  # a few ulps up until the float32 rule itself agrees that the median block passes
        if stop_rule(mo, blocks, t, dark_floor, int(n[0]), 0)[np.argsort(crit, kind="stable")[len(crit) // 2]]:
            break
        t = np.nextafter(t, f(np.inf))
    return float(t)


@pytest.mark.parametrize("catcher,fused", CASES, ids=IDS)
def test_decisions_follow_the_transcribed_rule(ptlib, monkeypatch, catcher, fused):
    nsub, dark = 8, 0.01
    ref = _ctx(monkeypatch, catcher, fused)
    hist = _plain_history(ref, nsub)
    ref.close()
    r = _ctx(monkeypatch, catcher, fused)
    r.adaptiveBegin(threshold=0.0, dark_floor=dark, min_subframes=1000)  # dry run: the moments at n = 3
    for k in range(3):
        r.launchParams.frame.subframe_index = k
        r.renderAdaptive()
    mo3, _ = r.adaptiveArrays()
    threshold = _median_threshold(mo3, dark)
    blocks = np.arange(NBX * NBY)
    first = stop_rule(mo3, blocks, threshold, dark, 3, 0)
    print(f"threshold {threshold:.6g}: {int(first.sum())} of {len(first)} blocks stop at the third call")
    assert first.sum() >= len(first) // 4 and (~first).sum() >= len(first) // 4  # non-vacuous by construction

    r.adaptiveBegin(threshold=threshold, dark_floor=dark, min_subframes=3)  # restart at subframe 0, as after a camera move
    npx = _block_pixels()
    active = np.ones(NBX * NBY, bool)
    last_block = np.full(NBX * NBY, -1)
    total = 0
    stopped_at = []
    for k in range(nsub):
        r.launchParams.frame.subframe_index = k
        st = r.renderAdaptive()
        assert st["active_pixels"] == int(npx[active].sum()), k
        total += int(npx[active].sum())
        last_block[active] = k
        mo, got = r.adaptiveArrays()
        want = active.copy()
        ids = np.flatnonzero(active)
        if len(ids):
            want[ids[stop_rule(mo, ids, threshold, dark, 3, 0)]] = False
        assert np.array_equal(got.reshape(-1) != 0, want), (k, int((got.reshape(-1) != 0).sum()), int(want.sum()))
        assert not (want & ~active).any()  # stopped blocks never come back
        stopped_at.append(int((active & ~want).sum()))
        active = want
        assert st["active_blocks"] == int(active.sum()) and st["pixel_subframes"] == total and st["blocks"] == NBX * NBY
    assert stopped_at[0] == stopped_at[1] == 0 and stopped_at[2] == int(first.sum()), stopped_at
    _same(_buffers(r), _expected(hist, last_block, hist[0]), "every block at its last subframe")
    r.close()


@pytest.mark.parametrize("catcher,fused", CASES, ids=IDS)
def test_max_subframes_stops_everything(ptlib, monkeypatch, catcher, fused):
    r = _ctx(monkeypatch, catcher, fused)
    r.adaptiveBegin(threshold=0.0, dark_floor=0.0, min_subframes=1000, max_subframes=4)
    for k in range(4):
        r.launchParams.frame.subframe_index = k
        st = r.renderAdaptive()
        assert st["active_pixels"] == W * H
        assert st["active_blocks"] == (NBX * NBY if k < 3 else 0), (k, st)
    before = _buffers(r)
    mo_before, act = r.adaptiveArrays()
    assert not act.any()
    r.launchParams.frame.subframe_index = 4
    st = r.renderAdaptive()
    s = r.stats()
    assert st["active_pixels"] == 0 and st["active_blocks"] == 0 and st["pixel_subframes"] == 4 * W * H
    assert s["trace_launches"] == 0 and s["shade_launches"] == 0 and s["shadow_launches"] == 0 and s["paths"] == 0
    _same(before, _buffers(r), "a call with nothing left to render")
    assert_bits_equal(mo_before, r.adaptiveArrays()[0], "moments")
    r.adaptiveEnd()
    r.close()


def test_refusals_have_a_text(ptlib, monkeypatch):
    import ctypes as C

    from optixpathtracer_amd import _lib
    from optixpathtracer_amd import renderer as R

    L = ptlib
    r = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    mask = np.ones(NBX * NBY, np.uint8)
    err = lambda: L.pt_last_error(r._ctx).decode()
    assert L.pt_render_mask(r._ctx, 1, 0, mask.ctypes.data, None, None) == -1 and "pt_render_mask" in err() and "pt_resize" in err()
    prm = _lib.AdaptiveParams(0.01, 0.0, 4, 0)
    assert L.pt_adaptive_begin(r._ctx, C.byref(prm)) == -1 and "pt_resize" in err()
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, W / H))
    assert L.pt_render_mask(r._ctx, 1, 0, None, None, None) == -1 and "null block mask" in err()
    for spp in (0, 4097):
        assert L.pt_render_mask(r._ctx, spp, 0, mask.ctypes.data, None, None) == -1 and "[1,4096]" in err()
    assert L.pt_render_adaptive(r._ctx, 1, 0, None, None) == -1 and "pt_adaptive_begin" in err()
    for bad, word in ((_lib.AdaptiveParams(0.01, 0.0, 1, 0), "min_subframes"), (_lib.AdaptiveParams(-1.0, 0.0, 4, 0), "threshold"),
                      (_lib.AdaptiveParams(float("nan"), 0.0, 4, 0), "threshold"), (_lib.AdaptiveParams(float("inf"), 0.0, 4, 0), "threshold"),
                      (_lib.AdaptiveParams(0.01, -0.5, 4, 0), "dark_floor"), (_lib.AdaptiveParams(0.01, float("nan"), 4, 0), "dark_floor")):
        assert L.pt_adaptive_begin(r._ctx, C.byref(bad)) == -1 and word in err(), word
    assert L.pt_adaptive_begin(r._ctx, C.byref(prm)) == 0
    assert L.pt_render_adaptive(r._ctx, 0, 0, None, None) == -1 and "[1,4096]" in err()
    r.resize((W + 8, H))  # implies pt_adaptive_end
    assert L.pt_render_adaptive(r._ctx, 1, 0, None, None) == -1 and "pt_adaptive_begin" in err()
    r.close()
