"""Adaptive sampling in the reprojection chain (pt_sample_plan, pt_temporal_carry) on the GPU.  The plan's mask and every counter of both
passes are compared exactly, and every output plane of the carry bit for bit over the WHOLE plane (so a pixel written outside the chosen set
shows as a lost sentinel), with tests/plan_ref.py: float32 NumPy evaluating the header's arithmetic.  One thing is not compared: which NaN
a NaN is (plan_ref.canon; the header leaves sign and payload open).  No tolerance anywhere.

Frames are 131 x 61: neither side is a multiple of 8, so the last column of blocks is 3 wide, the last row 5 high.  Real-plane inputs: hit,
position and motion from renderGBuffer (pinned by tests/test_gpu_gbuffer.py) of tests/test_gpu_temporal.py's two scenes under a mild move
(plan_ref.real_case), with plan_ref.block_history's histories; tests/test_plan_cabi.py asserts the same coverage conditions on CPU-built
planes (there: two_box 104 of 136 blocks sampled, 1751 pixels carried; terrain 109 of 136, 1447)."""
import ctypes as C

import numpy as np
import pytest
import torch

import plan_ref as PR
import temporal_ref as T
from gpu_kit import filled, plane_shape
from gpu_kit import bits as _bits
from gpu_kit import plane_renderer as _renderer
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from pass_cases import plan_case as _case

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = PR.W, PR.H
SENTINEL = PR.SENTINEL
FRAME = [(0, 0, W, H)]
ALL = np.ones((H, W), bool)


# ------------------------------------------------------------------ GPU helpers
def _filled(name, h, w, offset=False):
    """a sentinel-filled plane of the pass; offset: one float into its allocation (4-byte aligned only)"""
    return filled(plane_shape(h, w, _lib.CARRY_PLANES[name]), offset)


def _dev(planes, offset=False):
    dev = {k: _upload(planes[k], offset) for k in PR.INPUTS}
    for k in ("prev_hit", "prev_position"):  # read-only planes may alias one another
        if planes[k] is planes[k[5:]]:
            dev[k] = dev[k[5:]]
    return dev


def _plan(r, planes, rects, pixels, what, mask=None, offset=False, dev=None, **prm):
    """samplePlan against plan_ref: the mask and all stats exactly; returns (reference, the GPU's mask, stats)"""
    dev = dev or _dev(planes, offset)
    res = r.samplePlan(**dev, mask=mask, **prm)
    ref = PR.plan_ref(planes, rects, pixels, **prm)
    st = res["stats"]
    print(f"{what}: {st}")
    assert res["mask"].dtype == np.uint8 and res["mask"].shape == ref["mask"].shape
    assert np.array_equal(res["mask"], ref["mask"]), f"{what}: the mask differs in {int((res['mask'] != ref['mask']).sum())} blocks"
    assert {k: st[k] for k in PR.PLAN_STATS} == ref["stats"], (what, st, ref["stats"])
    assert st["kernel_ms"] > 0
    return ref, res["mask"], st


def _carry(r, planes, rects, pixels, what, mask=None, offset=False, dev=None, outputs=PR.OUTPUTS, out=None, **prm):
    """temporalCarry into sentinel-filled outputs against carry_ref over the whole frame; returns (reference, the outputs' bits, stats)"""
    h, w = planes["length_in"].shape
    dev = dev or _dev(planes, offset)
    out = out or {k: _filled(k, h, w, offset) for k in outputs}
    res = r.temporalCarry(**dev, **out, variance="variance_out" in outputs, mask=mask, **prm)
    assert all(res[k] is out[k] for k in outputs) and (("variance_out" in outputs) or res["variance_out"] is None)
    ref = PR.carry_ref(planes, rects, pixels, **prm)
    got = {k: _bits(out[k]) for k in outputs}
    for k in outputs:
        a, b = PR.canon(got[k]), PR.canon(ref[k])
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {k} differs from float32 NumPy in {int((a != b).sum())} words"
    st = res["stats"]
    print(f"{what}: {st}")
    assert {k: st[k] for k in PR.CARRY_STATS} == ref["stats"], (what, st, ref["stats"])
    assert st["kernel_ms"] > 0 if st["pixels"] else st["kernel_ms"] >= 0
    return ref, got, st


def _complement(mask, within=None):
    c = np.asarray(mask) == 0
    return c if within is None else c & (np.asarray(within) != 0)


# ------------------------------------------------------------------ 1. the plan on crafted flat planes
def test_plan_on_crafted_planes(ptlib):
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), (W, H), scenes.TWO_BOX_CAMERA)
    planes = PR.crafted_planes()
    dev = _dev(planes)
    # the reference alone meets the conditions, by construction
    ref7 = PR.plan_ref(planes, FRAME, ALL, **PR.CRAFTED)
    counts = PR.crafted_coverage(ref7, "crafted planes")
    print(f"crafted planes: {counts}")
    masks = {}
    for mp in (1, 7, 64):
        ref, masks[mp], _ = _plan(r, planes, FRAME, ALL, f"min_pixels {mp}", dev=dev, **dict(PR.CRAFTED, min_pixels=mp))
        assert ref["stats"]["lost"] == ref["stats"]["by_lost"] == counts["by_lost"]
    assert not np.array_equal(masks[1], masks[7]) and not np.array_equal(masks[7], masks[64])
    # the refresh: every phase of the period, a frame index at the top of its range (the sum passes 2^32), a period of one, none
    for frame in (0, 1, 2, 3, 2**32 - 1):
        _plan(r, planes, FRAME, ALL, f"frame_index {frame}", dev=dev, **dict(PR.CRAFTED, frame_index=frame, refresh_period=5 if frame > 3 else 4))
    ref, _, st = _plan(r, planes, FRAME, ALL, "refresh_period 1", dev=dev, **dict(PR.CRAFTED, refresh_period=1))
    assert st["sampled"] == st["blocks"] == 17 * 8
    ref, _, st = _plan(r, planes, FRAME, ALL, "no refresh, threshold 0", dev=dev, **dict(PR.CRAFTED, refresh_period=0, threshold=0.0, min_pixels=64))
    assert st["by_refresh"] == 0 and st["needy"] == st["pixels"] - st["lost"] and st["by_need"] > 0
    r.close()


# ------------------------------------------------------------------ 2. plan and carry on real planes
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_plan_and_carry_on_real_planes(ptlib, name):
    r, planes, prm = _case(name)
    dev = _dev(planes)
    plan, mask, _ = _plan(r, planes, FRAME, ALL, f"{name}: plan", dev=dev, **dict(PR.REAL_PLAN, **prm))
    comp = _complement(mask)
    carry, _, _ = _carry(r, planes, FRAME, PR.pixel_mask(comp, H, W), f"{name}: carry of the complement", mask=comp, dev=dev, **prm)
    n, s, cp, cv = PR.real_coverage(plan, carry, name)
    print(f"{name}: {s} of {n} blocks sampled, {cv} of {cp} carried pixels valid")
    # the carry of the whole frame does meet lost pixels: the NaN record
    ref, got, st = _carry(r, planes, FRAME, ALL, f"{name}: carry of the whole frame", dev=dev, **prm)
    assert st["lost"] == plan["stats"]["lost"] > 0 and np.array_equal(ref["valid"], plan["valid"])
    lost = ~ref["valid"]
    assert np.isnan(got["history_out"].view(f32)[lost][:, :3]).all() and not got["length_out"][lost].any()


# ------------------------------------------------------------------ 3. the carry with the plan's complement and the plan's parameters
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_carry_completes_what_temporal_moments_leaves(ptlib, name):
    r, planes, prm = _case(name)
    dev = _dev(planes)
    mask = r.samplePlan(**dev, **dict(PR.REAL_PLAN, **prm))["mask"]
    comp = _complement(mask)
    px_m, px_c = PR.pixel_mask(mask, H, W), PR.pixel_mask(comp, H, W)
    assert px_m.any() and px_c.any() and not (px_m & px_c).any() and (px_m | px_c).all()
    out = {k: _filled(k, H, W) for k in PR.OUTPUTS}
    color = _upload(np.random.default_rng(3).random((H, W, 4), dtype=f32))
    t = r.temporalMoments(color, **dev, **out, mask=mask, **prm)
    assert t["stats"]["pixels"] == int(px_m.sum())
    for k in PR.OUTPUTS:  # the masked temporal stage alone leaves the complement unwritten: the ping-pong would break there
        b = _bits(out[k])
        assert (b[px_c] == SENTINEL).all() and not (b[px_m] == SENTINEL).any()
    before = {k: _bits(out[k]) for k in PR.OUTPUTS}
    c = r.temporalCarry(**dev, **out, mask=comp, **prm)
    assert c["stats"]["lost"] == 0 and c["stats"]["pixels"] == c["stats"]["carried"] == int(px_c.sum())
    want = PR.carry_ref(planes, FRAME, px_c, **prm)
    for k in PR.OUTPUTS:
        b = _bits(out[k])
        assert np.array_equal(b[px_m], before[k][px_m]), f"{k}: the carry wrote a pixel of the plan's mask"
        assert np.array_equal(PR.canon(b[px_c]), PR.canon(want[k][px_c])), k
        assert not (b == SENTINEL).any(), f"{k}: a pixel of the frame was left unwritten"
    assert not np.isnan(_np(out["history_out"])[px_c]).any() and (_np(out["length_out"])[px_c] >= 1).all()


# ------------------------------------------------------------------ 4. the carry of a still frame
def test_carry_with_zero_motion_is_the_identity(ptlib):
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), (W, H), scenes.TWO_BOX_CAMERA)
    planes = PR.crafted_planes()
    assert planes["prev_hit"] is planes["hit"] and not planes["motion"].any()
    nby, nbx = r.blockGrid()
    ref, got, st = _carry(r, planes, FRAME, ALL, "zero motion", mask=np.ones((nby, nbx), np.uint8))
    v = ref["valid"]
    assert st["lost"] == 36 and int(v.sum()) == W * H - 36
    for k, src in (("history_out", "history_in"), ("moments_out", "moments_in"), ("length_out", "length_in")):
        a, b = got[k][v], np.ascontiguousarray(planes[src]).view(np.uint32)[v]
        assert np.array_equal(a[..., :3] if k == "history_out" else a, b[..., :3] if k == "history_out" else b), k
    assert (got["history_out"][..., 3] == f32(1).view(np.uint32)).all()
    assert np.isnan(got["history_out"].view(f32)[~v][:, :3]).all()
    assert not got["moments_out"][~v].any() and not got["length_out"][~v].any() and not got["variance_out"][~v].any()
    r.close()


# ------------------------------------------------------------------ 5. the loop
def test_loop_with_every_block_sampled_is_the_unmasked_loop(ptlib):
    """min_length = 65535 and min_pixels = 1: every pixel with a history is short, every other one lost, so every block is sampled, the
    carry has nothing to do, and three frames of the adaptive loop leave the bits of render() + temporalMoments without a mask"""
    probe = scenes.sky_probe(256, 128).BuildCDF()
    nby, nbx = (H + 7) // 8, (W + 7) // 8

    def loop(adaptive):
        r = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
        r.setProbe(probe)
        r.resize((W, H))
        r.launchParams.samples_per_launch = 1
        r.uploadAccum(np.zeros((H, W, 4), f32))
        z = lambda k: torch.zeros((H, W, k) if k > 1 else (H, W), device="cuda:0")  # noqa: E731
        gbuf = [dict(hit=z(8), position=z(4), motion=z(2)) for _ in range(2)]
        hist, mom, ln = [z(4), z(4)], [z(2), z(2)], [z(1), z(1)]
        var, filt, scratch = z(1), z(4), z(4)
        accum = r.deviceBuffer(R.PT_BUF_ACCUM)
        cam = R.make_camera(scenes.TWO_BOX_CAMERA, W / H)
        frames = []
        for k in range(3):
            prev, cam = cam, R.make_camera(T.forward(scenes.TWO_BOX_CAMERA, 0.01 * k, dx=0.02 * k), W / H)
            cur, old, i, o = gbuf[k & 1], gbuf[~k & 1], k & 1, ~k & 1
            r.setCamera(cam)
            r.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev, out=cur)
            r.launchParams.frame.subframe_index = k
            geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], hist[i], mom[i], ln[i])
            outs = dict(history_out=hist[o], moments_out=mom[o], length_out=ln[o], variance_out=var)
            if adaptive:
                plan = r.samplePlan(*geo, min_length=65535, min_pixels=1, frame_index=k)
                mask = plan["mask"]
                assert mask.all() and plan["stats"]["sampled"] == nby * nbx
                assert r.renderMask(mask) == W * H
                r.temporalMoments(accum, *geo, **outs, mask=mask, color_scale=float(k + 1), clear_color=True)
                c = r.temporalCarry(*geo, **outs, mask=_complement(mask))
                assert c["stats"]["pixels"] == 0
            else:
                r.render()
                r.temporalMoments(accum, *geo, **outs, color_scale=float(k + 1), clear_color=True)
            r.filterPlanes(hist[o], cur["hit"], cur["position"], variance=var, length=ln[o], out=filt, scratch=scratch)
            frames.append({n: _bits(t) for n, t in (("history", hist[o]), ("moments", mom[o]), ("length", ln[o]), ("variance", var), ("filtered", filt))})
        r.close()
        return frames

    a, b = loop(True), loop(False)
    for k, (x, y) in enumerate(zip(a, b)):
        for n in x:
            assert np.array_equal(x[n], y[n]), f"frame {k}: {n} differs in {int((x[n] != y[n]).sum())} words"
    assert (a[2]["length"].view(f32) > 1).any() and a[2]["history"].any()


# ------------------------------------------------------------------ 6. variants
def _both(r, planes, rects, pixels, what, prm, in_mask=None, offset=False, outputs=PR.OUTPUTS):
    """the plan on `pixels` (the set of in_mask), then the carry on the plan's complement within the set and on the set itself"""
    dev = _dev(planes, offset)
    plan, mask, _ = _plan(r, planes, rects, pixels, f"{what}: plan", mask=in_mask, dev=dev, **dict(PR.REAL_PLAN, **prm))
    assert 0 < plan["stats"]["sampled"] < plan["stats"]["blocks"]
    comp = _complement(mask, in_mask)
    h, w = pixels.shape
    px_c = PR.pixel_mask(comp, h, w) & pixels
    ref, got, st = _carry(r, planes, rects, px_c, f"{what}: carry of the complement", mask=comp, offset=offset, dev=dev, outputs=outputs, **prm)
    assert st["lost"] == 0 and st["pixels"] > 0 and (got["length_out"][~px_c] == SENTINEL).all()
    _carry(r, planes, rects, pixels, f"{what}: carry of the set", mask=in_mask, offset=offset, dev=dev, outputs=outputs, **prm)
    return plan, mask


def test_two_views(ptlib):
    from scene_kit import RECTS

    _, planes, prm = _case("two_box")
    rects = RECTS[:2]  # (0, 0, 61, 37) and (64, 0, 67, 29): origins on the 8-grid, no side a multiple of 8
    r = _renderer(scenes.two_box_scene(shadow_catcher=False), (W, H), scenes.TWO_BOX_CAMERA)
    r.setViews([(x, y, w, h, R.make_camera(scenes.TWO_BOX_CAMERA, w / h)) for x, y, w, h in rects])
    inside = np.zeros((H, W), bool)
    for x, y, w, h in rects:
        inside[y:y + h, x:x + w] = True
    plan, mask = _both(r, planes, rects, inside, "two views", prm)
    assert plan["stats"]["blocks"] == 8 * 5 + 9 * 4 and not mask[5:].any() and not mask[4, 8:].any()
    r.close()


def test_partition_rank_1_of_3(ptlib):
    _, planes, prm = _case("terrain")
    make, size, cam, _, _, _ = PR.real_case("terrain")
    r = _renderer(make(), size, cam, partition=(1, 3, 8, 8))
    by, bx = np.mgrid[0:H, 0:W] // 8
    own = (bx + by) % 3 == 1
    plan, mask = _both(r, planes, FRAME, own, "rank 1 of 3", prm)
    assert plan["stats"]["pixels"] == int(own.sum()) and not mask[~PR.block_set(own)].any()
    r.close()


def test_input_block_mask(ptlib):
    r, planes, prm = _case("two_box")
    nby, nbx = r.blockGrid()
    in_mask = np.random.default_rng(5).random((nby, nbx)) < 0.6
    in_mask[0, 0] = in_mask[nby - 1, nbx - 1] = in_mask[0, nbx - 1] = in_mask[nby - 1, 3] = True  # corner and edge blocks
    in_mask[1, 1] = False
    plan, mask = _both(r, planes, FRAME, PR.pixel_mask(in_mask, H, W), "an input mask", prm, in_mask=in_mask)
    assert not mask[~in_mask].any() and plan["stats"]["blocks"] == int(in_mask.sum())
    none = np.zeros((nby, nbx), bool)
    _, mask, st = _plan(r, planes, FRAME, np.zeros((H, W), bool), "the empty mask", mask=none, **dict(PR.REAL_PLAN, **prm))
    assert not mask.any() and st["blocks"] == st["pixels"] == 0
    _, got, st = _carry(r, planes, FRAME, np.zeros((H, W), bool), "the empty mask", mask=none, **prm)
    assert st["pixels"] == 0


def test_planes_four_byte_aligned_only(ptlib):
    r, planes, prm = _case("terrain")
    _both(r, planes, FRAME, ALL, "planes one float into their allocations", prm, offset=True)


def test_no_variance_out(ptlib):
    r, planes, prm = _case("two_box")
    _both(r, planes, FRAME, ALL, "variance_out NULL", prm, outputs=PR.OUTPUTS[:3])


# ------------------------------------------------------------------ 7. refusals
def test_refusals(ptlib):
    _, planes, prm = _case("two_box")
    L = _lib.load_library()
    r = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    dev = _dev(planes)
    out = {k: _filled(k, H, W) for k in PR.OUTPUTS}
    nby, nbx = (H + 7) // 8, (W + 7) // 8
    mask_out = np.full(nby * nbx, 0x5A, np.uint8)
    ptr = {k: t.data_ptr() for k, t in list(dev.items()) + list(out.items())}
    gather = dict(normal_cos=0.9, plane_eps=0.01, min_weight=0.25, flags=0)
    good_plan = dict({k: ptr[k] for k in PR.INPUTS}, block_mask_out=mask_out.ctypes.data, threshold=0.1, dark_floor=0.01, min_length=4, min_pixels=4,
                     refresh_period=0, frame_index=0, **gather)
    good_carry = dict(ptr, **gather)

    def refused(fn, what, pattern, **fields):
        plan = fn == "pt_sample_plan"
        d = _lib.PlanDesc() if plan else _lib.CarryDesc()
        for k, v in dict(good_plan if plan else good_carry, **fields).items():
            setattr(d, k, v)
        torch.cuda.synchronize()
        s = _lib.PlanStats(*([7] * 8), 7.0) if plan else _lib.CarryStats(7, 7, 7, 7.0)
        rc = getattr(L, fn)(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith(fn) and pattern in msg, f"{what}: {msg!r}"
        assert all(v in (7, 7.0) for v in s.as_dict().values())
        assert (mask_out == 0x5A).all(), f"{what}: block_mask_out was written"
        for k, t in out.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {k} was written"

    for fn in ("pt_sample_plan", "pt_temporal_carry"):
        refused(fn, "no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, W / H))
    for fn in ("pt_sample_plan", "pt_temporal_carry"):
        assert getattr(L, fn)(r._ctx, None, None) == -1 and "null description" in L.pt_last_error(r._ctx).decode()
        for name in PR.INPUTS:
            refused(fn, f"{name} null", f"{name} is null", **{name: None})
        refused(fn, "a flag", "unknown flag bits 1", flags=1)
        refused(fn, "a host pointer", "hit is not device memory", hit=np.zeros((H, W, 8), f32).ctypes.data)
        refused(fn, "a pointer offset by 2 bytes", "moments_in is not 4-byte aligned", moments_in=ptr["moments_in"] + 2)
        for name, bad, pattern in (("normal_cos", (1.5, -1.5, np.nan), "normal_cos must be in [-1,1]"),
                                   ("plane_eps", (-1.0, np.inf, np.nan), "plane_eps must be finite and >= 0"),
                                   ("min_weight", (-0.1, 1.5, np.nan), "min_weight must be in [0,1]")):
            for v in bad:
                refused(fn, f"{name} = {v}", pattern, **{name: v})
    # the plan's own
    refused("pt_sample_plan", "no block_mask_out", "block_mask_out is null", block_mask_out=None)
    for v in (0, 65):
        refused("pt_sample_plan", f"min_pixels = {v}", "min_pixels must be in [1,64]", min_pixels=v)
    for v in (np.inf, np.nan, -0.5):
        refused("pt_sample_plan", f"threshold = {v}", "threshold must be finite and >= 0", threshold=v)
        refused("pt_sample_plan", f"dark_floor = {v}", "dark_floor must be finite and >= 0", dark_floor=v)
    refused("pt_sample_plan", "min_length = 65536", "min_length must be in [0,65535]", min_length=65536)
    refused("pt_sample_plan", "refresh_period = 65536", "refresh_period must be in [0,65535]", refresh_period=65536)
    # the carry's own: a null output, the overlaps of an output; the read-only planes may alias
    for name in PR.OUTPUTS[:3]:
        refused("pt_temporal_carry", f"{name} null", f"{name} is null", **{name: None})
    refused("pt_temporal_carry", "history in place", "history_in and history_out overlap", history_out=ptr["history_in"])
    refused("pt_temporal_carry", "moments in place", "moments_in and moments_out overlap", moments_out=ptr["moments_in"])
    refused("pt_temporal_carry", "the length on the motion", "motion and length_out overlap", length_out=ptr["motion"])
    refused("pt_temporal_carry", "the variance inside the history", "history_out and variance_out overlap", variance_out=ptr["history_out"] + 16)
    refused("pt_temporal_carry", "an optional output offset by 1 byte", "variance_out is not 4-byte aligned", variance_out=ptr["variance_out"] + 1)
    with pytest.raises(RuntimeError, match="history_in and history_out overlap"):
        r.temporalCarry(**dev, **dict(out, history_out=dev["history_in"]))
    with pytest.raises(RuntimeError, match="min_pixels must be in"):
        r.samplePlan(**dev, min_pixels=0)
    # valid calls afterwards still work; all eight planes of the plan may be one another's aliases where their sizes agree
    _plan(r, planes, FRAME, ALL, "a valid plan after the refusals", dev=dev, **dict(PR.REAL_PLAN, **prm))
    _carry(r, planes, FRAME, ALL, "a valid carry after the refusals", dev=dev, out=out, **prm)
    res = r.temporalCarry(**dev, **prm)  # the facade allocates the outputs, zero-filled
    want = PR.carry_ref(planes, FRAME, ALL, fill=0, **prm)
    for k in PR.OUTPUTS:
        assert np.array_equal(PR.canon(_bits(res[k])), PR.canon(want[k])), k
    r.close()
