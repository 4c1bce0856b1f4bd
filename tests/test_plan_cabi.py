"""Adaptive sampling in the reprojection chain (pt_sample_plan, pt_temporal_carry) without a GPU: the entry points are declared and exported,
the ctypes mirrors match the compiler's layout, the header compiles as C99 and as C++17 and states the arithmetic, a null context and a null
description are refused before any device work, both facades have the methods; and the float32 NumPy reference (tests/plan_ref.py) has the
properties the tests of tests/test_gpu_plan.py lean on: its restated gather agrees with moments_ref.moments_ref's, the carry of a still
frame is the identity, a plan's complement is carried without loss, the refresh formula holds near 2^32, and the inputs take every outcome
often enough."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import moments_ref as MR
import plan_ref as PR
import temporal_ref as T
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_text
from conftest import ROOT
from optixpathtracer_amd import _lib

f32 = np.float32
PLAN_FIELDS = PR.INPUTS + ("block_mask", "block_mask_out", "normal_cos", "plane_eps", "min_weight", "threshold", "dark_floor", "min_length", "min_pixels",
                           "refresh_period", "frame_index", "flags")
CARRY_FIELDS = PR.INPUTS + PR.OUTPUTS + ("block_mask", "normal_cos", "plane_eps", "min_weight", "flags")
NEW = ("pt_sample_plan", "pt_temporal_carry")


# ------------------------------------------------------------------ surface
def test_library_exports_the_entry_points():
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert name in header().split("VERSIONING.")[1].split("*/")[0]  # the note names it among the entry points added at 0.4
        assert name in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_sample_plan\s*\(\s*pt_ctx\s*\*\s*\w*\s*,\s*const\s+pt_plan_desc\s*\*\s*\w*\s*,\s*pt_plan_stats\s*\*", src)
    assert re.search(r"int\s+pt_temporal_carry\s*\(\s*pt_ctx\s*\*\s*\w*\s*,\s*const\s+pt_carry_desc\s*\*\s*\w*\s*,\s*pt_carry_stats\s*\*", src)
    assert L.pt_version().startswith(b"ptamd 0.4")


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.PlanDesc, "pt_plan_desc", PLAN_FIELDS), (_lib.PlanStats, "pt_plan_stats", PR.PLAN_STATS + ("kernel_ms",)),
                            (_lib.CarryDesc, "pt_carry_desc", CARRY_FIELDS), (_lib.CarryStats, "pt_carry_stats", PR.CARRY_STATS + ("kernel_ms",))],
                 [120] + list(range(0, 80, 8)) + list(range(80, 120, 4)) + [72] + list(range(0, 72, 8)) + [120] + list(range(0, 104, 8)) + [104, 108, 112, 116] + [32, 0, 8, 16, 24])
    assert tuple(_lib.PLAN_PLANES) == PR.INPUTS and tuple(_lib.CARRY_PLANES) == PR.INPUTS + PR.OUTPUTS and _lib.CARRY_OUTPUTS == PR.OUTPUTS
    assert {k: _lib.CARRY_PLANES[k] for k in PR.OUTPUTS} == PR.WORDS == {k: _lib.TMOM_PLANES[k] for k in PR.OUTPUTS}
    assert all(_lib.PLAN_PLANES[k] == _lib.TMOM_PLANES[k] for k in PR.INPUTS)


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const float* planes, float* outs, uint8_t* mask) {\n"
            "    pt_plan_desc d = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.9f, 0.01f, 0.25f, 0.05f, 0.01f, 4u, 4u, 0u, 0u, 0u};\n"
            "    pt_carry_desc k = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.9f, 0.01f, 0.25f, 0u};\n"
            "    pt_plan_stats s;\n"
            "    pt_carry_stats ks;\n"
            "    d.motion = planes; d.hit = planes; d.length_in = planes; d.block_mask = mask; d.block_mask_out = mask;\n"
            "    if (pt_sample_plan(c, &d, &s) || s.sampled != s.by_lost + s.by_need + s.by_refresh) return -1;\n"
            "    k.motion = planes; k.hit = planes; k.history_out = outs; k.variance_out = outs; k.block_mask = mask;\n"
            "    if (pt_temporal_carry(c, &k, &ks)) return -1;\n"
            "    return ks.lost == ks.pixels - ks.carried ? 0 : -1;\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_context_and_null_description_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.PlanDesc(), _lib.PlanStats(*([7] * 8), 7.0)
    assert L.pt_sample_plan(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_sample_plan: null context" in L.pt_last_error(None)
    assert L.pt_sample_plan(None, None, None) == -1
    assert s.as_dict() == dict({k: 7 for k in PR.PLAN_STATS}, kernel_ms=7.0)
    k, ks = _lib.CarryDesc(), _lib.CarryStats(7, 7, 7, 7.0)
    assert L.pt_temporal_carry(None, C.byref(k), C.byref(ks)) == -1
    assert b"pt_temporal_carry: null context" in L.pt_last_error(None)
    assert L.pt_temporal_carry(None, None, None) == -1 and ks.as_dict() == dict(pixels=7, carried=7, lost=7, kernel_ms=7.0)
    # a null description is refused before the context is looked at (the text of pt_plan.hip; a live context needs a GPU)
    api = open(os.path.join(ROOT, "optixpathtracer_amd", "csrc", "pt_plan.hip")).read()
    for name in NEW:
        body = api.split(f'extern "C" int {name}(')[1]
        assert body.index("null description") < body.index("ctx->width")


def test_python_facade_checks_its_arguments():
    from optixpathtracer_amd import renderer as R

    for name in ("samplePlan", "temporalCarry"):
        assert callable(getattr(R.SampleRenderer, name, None))
    r = bare_renderer()
    r.blockGrid = lambda: (1, 1)
    with pytest.raises(ValueError, match="samplePlan: motion is required"):
        r.samplePlan(None, 1, 1, 1, 1, 1, 1, 1)
    with pytest.raises(ValueError, match=r"samplePlan: moments_in: a contiguous torch.float32 tensor of shape \(4, 4, 2\) is expected"):
        r.samplePlan(1, 1, 1, 1, 1, 1, fake_cuda((4, 4, 4)), 1)
    with pytest.raises(ValueError, match="samplePlan: the mask needs"):
        r.samplePlan(1, 1, 1, 1, 1, 1, 1, 1, mask=np.ones((2, 2)))
    with pytest.raises(ValueError, match=r"samplePlan: min_pixels must be in \[1,64\]"):
        r.samplePlan(1, 1, 1, 1, 1, 1, 1, 1, min_pixels=-1)
    with pytest.raises(ValueError, match=r"samplePlan: frame_index must be in \[0,4294967295\]"):
        r.samplePlan(1, 1, 1, 1, 1, 1, 1, 1, frame_index=2**32)
    outs = dict(history_out=1, moments_out=1, length_out=1, variance_out=1)
    with pytest.raises(ValueError, match="temporalCarry: length_in is required"):
        r.temporalCarry(1, 1, 1, 1, 1, 1, 1, None, **outs)
    with pytest.raises(ValueError, match=r"temporalCarry: variance_out: a contiguous torch.float32 tensor of shape \(4, 4\) is expected"):
        r.temporalCarry(1, 1, 1, 1, 1, 1, 1, 1, **dict(outs, variance_out=fake_cuda((4, 4, 1))))
    with pytest.raises(ValueError, match="temporalCarry: the mask needs"):
        r.temporalCarry(1, 1, 1, 1, 1, 1, 1, 1, mask=np.ones((2, 2)), **outs)


def test_cxx_facade_compiles(tmp_path):
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t stage(SampleRenderer& sample, pt_plan_desc d, pt_carry_desc k) {\n"
        "    pt_plan_stats s{};\n"
        "    pt_carry_stats ks{};\n"
        "    sample.samplePlan(d, &s);\n"
        "    sample.temporalCarry(k, &ks);\n"
        "    return sample.samplePlan(d).sampled + s.by_lost + sample.temporalCarry(k).carried + ks.lost;\n"
        "}\n"
    )


def test_header_states_the_contract():
    text = header_text()
    for item in ("px = (float)x + motion[p].x; py = (float)y + motion[p].y", "tap weights w_ij = wx_i * wy_j",
                 "the three colour words of history_in[q] and both words of moments_in[q] are finite (exponent-bit test)",
                 "Tap order (0,0), (1,0), (0,1), (1,1)", "Wsum = ((w00 + w10) + w01) + w11",
                 "valid = (at least one tap counts) && Wsum >= min_weight", "H = Hsum / Wsum and M = Msum / Wsum",
                 "lost(p) = !valid", "short(p) = valid && nprev < (float)min_length", "var = sel_max0(M.y - M.x * M.x); B = M.x + dark_floor",
                 "rhs = (((threshold * threshold) * nprev) * B) * B; noisy = !(var <= rhs)", "a NaN makes it noisy",
                 "refresh = refresh_period > 0 && ((uint64)bx + 3 * (uint64)by + frame_index) % refresh_period == 0",
                 "sampled = L >= 1 || S >= min_pixels || refresh", "Every other block of the frame gets 0",
                 "A block with a lost pixel is always sampled", "history_out[p] = (H, 1.0f); moments_out[p] = M; length_out[p] = nprev",
                 "not incremented, not capped", "three NaN words and 1.0f", "moments_out[p] = (0, 0); length_out[p] = 0; variance_out[p] = 0",
                 "GUARANTEE", "lost is 0", "the four outputs may overlap no other plane", "float32 NumPy evaluating this reproduces every output bit for bit",
                 "a NaN is a NaN", "PT_BUF_ALBEDO is written by the render", "it is stale", "examples/adaptive_svgf_loop.py"):
        assert item in text, item


# ------------------------------------------------------------------ inputs shared by the tests below
_REAL = {}


def _real(orc, name):
    """the CPU-built planes of a real input of tests/test_gpu_plan.py with its block history, and its gather parameters"""
    if name not in _REAL:
        make, size, cam, prev, prm, seed = PR.real_case(name)
        planes = PR.with_block_history(T.cpu_planes(orc, make(), size, cam, prev), seed)
        for a in planes.values():
            a.setflags(write=False)
        _REAL[name] = (planes, prm)
    return _REAL[name]


def _frame(planes):
    h, w = planes["length_in"].shape
    return [(0, 0, w, h)], np.ones((h, w), bool)


# ------------------------------------------------------------------ the restated gather against the pinned one
def _same_valid(planes, rects, px, **prm):
    h, w = px.shape
    g = PR.gather(planes, rects, px, **dict(PR.GATHER_DEFAULTS, **prm))
    mine = np.zeros((h, w), bool)
    mine[g["Y"], g["X"]] = g["valid"]
    pinned = MR.moments_ref(dict(planes, color=np.zeros((h, w, 4), f32), albedo=None), rects, px, **prm)
    assert np.array_equal(mine, pinned["valid"]) and int(g["valid"].sum()) == pinned["reprojected"]
    return int(g["valid"].sum())


@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_gather_agrees_with_moments_ref_on_real_planes(orc_det, name):
    planes, prm = _real(orc_det, name)
    rects, px = _frame(planes)
    n = _same_valid(planes, rects, px, **prm)
    assert 0 < n < px.sum()
    # ... and on the harsher inputs of tests/test_gpu_moments.py (the strong move, random_history's holes)
    make, size, cam, prev, tprm, seed = T.real_inputs()[name]
    harsh = MR.with_random_inputs(T.cpu_planes(orc_det, make(), size, cam, prev), seed)
    n = _same_valid({k: harsh[k] for k in PR.INPUTS}, rects, px, **tprm)
    assert 0 < n < px.sum()


@pytest.mark.parametrize("size", [(65, 3), (9, 8), (1, 1)])
def test_gather_agrees_with_moments_ref_on_synthetic_planes(size):
    w, h = size
    planes = dict(T.synthetic_planes(w, h, 7 + w), moments_in=MR.random_moments(np.random.default_rng(w), h, w))
    rects, px = _frame(planes)
    for mw in (0.0, 0.25, 0.6, 1.0):
        _same_valid({k: planes[k] for k in PR.INPUTS}, rects, px, min_weight=mw)
    if w > 16:  # two views side by side: no tap crosses the border
        _same_valid({k: planes[k] for k in PR.INPUTS}, [(0, 0, 32, h), (32, 0, w - 32, h)], px)


def test_carry_equals_the_blend_free_part_of_moments_ref(orc_det):
    """the reprojected colour H of the two references is the same number: handed H itself as this frame's colour, pt_temporal_moments's
    blend H + (d - H) * a returns H exactly, whatever a is"""
    planes, prm = _real(orc_det, "two_box")
    rects, px = _frame(planes)
    carry = PR.carry_ref(planes, rects, px, **prm)
    H = carry["history_out"].view(f32)
    color = np.where(carry["valid"][..., None], H, f32(0)).astype(f32)
    pinned = MR.moments_ref(dict(planes, color=color, albedo=None), rects, px, **prm)
    v = carry["valid"]
    assert np.array_equal(pinned["history_out"][v][:, :3], carry["history_out"][v][:, :3]) and v.any()


# ------------------------------------------------------------------ the carry
def test_carry_of_a_still_frame_is_the_identity():
    planes = PR.crafted_planes()
    rects, px = _frame(planes)
    res = PR.carry_ref(planes, rects, px)
    v = res["valid"]
    assert v.sum() == px.sum() - 36 and res["stats"] == dict(pixels=int(px.sum()), carried=int(v.sum()), lost=36)
    assert np.array_equal(res["history_out"][v][:, :3], planes["history_in"].view(np.uint32)[v][:, :3])
    assert np.array_equal(res["moments_out"][v], planes["moments_in"].view(np.uint32)[v])
    assert np.array_equal(res["length_out"][v], planes["length_in"].view(np.uint32)[v])
    assert (res["history_out"][..., 3] == np.float32(1).view(np.uint32)).all()
    lost = res["history_out"].view(f32)[~v]
    assert np.isnan(lost[:, :3]).all() and not res["moments_out"][~v].any() and not res["length_out"][~v].any() and not res["variance_out"][~v].any()


@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_the_complement_of_a_plan_is_carried_without_loss(orc_det, name):
    planes, prm = _real(orc_det, name)
    rects, px = _frame(planes)
    h, w = px.shape
    plan = PR.plan_ref(planes, rects, px, **dict(PR.REAL_PLAN, **prm))
    comp = PR.pixel_mask(1 - plan["mask"], h, w)
    carry = PR.carry_ref(planes, rects, comp, **prm)
    assert carry["stats"]["lost"] == 0 and (carry["length_out"][~comp] == PR.SENTINEL).all()
    n, s, cp, cv = PR.real_coverage(plan, carry, name)
    print(f"{name}: {s} of {n} blocks sampled ({plan['stats']}), {cv} of {cp} carried pixels valid")
    # with other gather parameters than the plan's the guarantee is gone: the carry does meet pixels it cannot carry
    assert PR.carry_ref(planes, rects, comp, **dict(prm, min_weight=1.0))["stats"]["lost"] > 0


# ------------------------------------------------------------------ the plan
def test_crafted_planes_take_every_outcome():
    planes = PR.crafted_planes()
    rects, px = _frame(planes)
    masks = []
    for mp in (1, 7, 64):
        ref = PR.plan_ref(planes, rects, px, **dict(PR.CRAFTED, min_pixels=mp))
        counts = PR.crafted_coverage(ref, f"min_pixels {mp}") if mp == 7 else None
        print(mp, ref["stats"], counts)
        st = ref["stats"]
        assert st["sampled"] == st["by_lost"] + st["by_need"] + st["by_refresh"] and st["lost"] == 36 == st["by_lost"]
        masks.append(ref["mask"])
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2])
    assert (masks[0] >= masks[1]).all() and (masks[1] >= masks[2]).all()
    # a NaN in the moments of a valid pixel cannot happen (the tap would not count); a NaN variance can: inf - inf needs an inf, likewise
    # rejected.  What remains is threshold = 0: rhs = 0, noisy = !(var <= 0) — every pixel with a positive variance
    ref = PR.plan_ref(planes, rects, px, **dict(PR.CRAFTED, threshold=0.0, min_pixels=64, refresh_period=0))
    assert ref["stats"]["needy"] == ref["stats"]["pixels"] - ref["stats"]["lost"] and ref["stats"]["by_need"] > 0


def test_refresh_formula_near_two_to_the_32():
    """((uint64)bx + 3 * (uint64)by + frame_index) % period, evaluated without wrapping at 2^32: the kernel's split into
    ((bx + 3 by) % period + frame_index % period) % period is the same number"""
    for period in (1, 2, 3, 7, 255, 4096, 65535):
        for frame in (0, 1, 2**31 - 1, 2**31, 2**32 - 70000, 2**32 - 2, 2**32 - 1):
            for bx, by in ((0, 0), (1, 0), (0, 1), (16, 7), (8191, 8191)):
                want = (bx + 3 * by + frame) % period == 0
                assert PR.refresh(bx, by, frame, period) == want
                assert (((bx + 3 * by) % period + frame % period) % period == 0) == want
    assert not PR.refresh(3, 4, 5, 0)
    planes = PR.crafted_planes()
    rects, px = _frame(planes)
    a = PR.plan_ref(planes, rects, px, **dict(PR.CRAFTED, frame_index=2**32 - 1, refresh_period=5))
    b = PR.plan_ref(planes, rects, px, **dict(PR.CRAFTED, frame_index=(2**32 - 1) % 5, refresh_period=5))
    assert np.array_equal(a["mask"], b["mask"]) and a["stats"] == b["stats"] and a["stats"]["by_refresh"] > 0
    # a 32-bit sum would have wrapped for the blocks with bx + 3 by >= 1: 2^32 % 5 = 1 shifts their phase
    wrong = np.array([[((bx + 3 * by + 2**32 - 1) & 0xFFFFFFFF) % 5 == 0 for bx in range(a["mask"].shape[1])] for by in range(a["mask"].shape[0])])
    assert not np.array_equal(wrong & (a["quiet"] | a["by_refresh"]), a["by_refresh"])
