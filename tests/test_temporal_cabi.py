"""Temporal accumulation (pt_temporal_accumulate) without a GPU: the entry point is declared and exported, the ctypes mirrors of
pt_temporal_desc and pt_temporal_stats match the compiler's layout, the header still compiles as C99 and as C++17, a null context and a null
description are refused before any device work, both facades have the method and the Python one checks its arguments before the library
is called; the float32 NumPy reference (tests/temporal_ref.py) has the properties a running mean must have; and the real-plane inputs of
tests/test_gpu_temporal.py, rebuilt here with the CPU checker, exercise every rejection reason."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import temporal_ref as T
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_text
from conftest import ROOT
from optixpathtracer_amd import _lib

f32 = np.float32
DESC_FIELDS = ("color", "motion", "hit", "position", "prev_hit", "prev_position", "history_in", "length_in", "history_out", "length_out",
               "frame_rgba8", "copy_out", "block_mask", "color_scale", "normal_cos", "plane_eps", "min_weight", "max_history", "flags")
STATS_FIELDS = ("pixels", "reprojected", "kernel_ms")


def test_library_exports_the_entry_point():
    L = _lib.load_library()
    assert "pt_temporal_accumulate" in _lib.EXPORTS and hasattr(L, "pt_temporal_accumulate")
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int\s+pt_temporal_accumulate\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_temporal_desc\s*\*\s*\w+\s*,\s*pt_temporal_stats\s*\*", src)
    assert re.search(r"PT_TEMPORAL_CLEAR_COLOR\s*=\s*1\b", src) and _lib.PT_TEMPORAL_CLEAR_COLOR == 1
    assert L.pt_version().startswith(b"ptamd 0.4")
    assert "pt_temporal_accumulate" in header().split("VERSIONING.")[1].split("*/")[0]  # the note names it among the entry points added at 0.4
    assert "pt_temporal_accumulate" in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.TemporalDesc, "pt_temporal_desc", DESC_FIELDS), (_lib.TemporalStats, "pt_temporal_stats", STATS_FIELDS)],
                 [128] + [8 * k for k in range(13)] + [104, 108, 112, 116, 120, 124] + [24, 0, 8, 16])
    assert set(_lib.TEMPORAL_PLANES) == set(DESC_FIELDS[:12]) and set(_lib.TEMPORAL_OUTPUTS) == set(T.OUTPUTS)


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, float* color, const float* motion, float* out) {\n"
            "    pt_temporal_desc d = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0f, 0.9f, 0.01f, 0.25f, 32u, 0u};\n"
            "    pt_temporal_stats s;\n"
            "    d.color = color; d.motion = motion; d.history_out = out; d.flags = PT_TEMPORAL_CLEAR_COLOR;\n"
            "    return pt_temporal_accumulate(c, &d, &s);\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_context_and_null_description_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.TemporalDesc(), _lib.TemporalStats(7, 7, 7.0)
    assert L.pt_temporal_accumulate(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_temporal_accumulate: null context" in L.pt_last_error(None)
    assert L.pt_temporal_accumulate(None, None, None) == -1
    assert (s.pixels, s.reprojected, s.kernel_ms) == (7, 7, 7.0)
    # a null description is refused before the context is looked at (the text of pt_temporal.hip; a live context needs a GPU)
    api = open(os.path.join(ROOT, "optixpathtracer_amd", "csrc", "pt_temporal.hip")).read()
    body = api.split('extern "C" int pt_temporal_accumulate(')[1]
    assert body.index("null description") < body.index("ctx->width")


def test_python_facade_checks_its_arguments():
    import torch

    from optixpathtracer_amd import renderer as R

    assert callable(getattr(R.SampleRenderer, "temporalAccumulate", None))
    with pytest.raises(TypeError, match="color: a torch tensor or a device pointer"):
        R._check_temporal_tensor("color", np.zeros((4, 4, 4), f32), 0, {torch.float32: (4, 4, 4)})
    with pytest.raises(ValueError, match="motion: the tensor is on cpu"):
        R._check_temporal_tensor("motion", torch.zeros((4, 4, 2)), 0, {torch.float32: (4, 4, 2)})
    R._check_temporal_tensor("motion", fake_cuda((4, 4, 2)), 0, {torch.float32: (4, 4, 2)})
    with pytest.raises(ValueError, match="the context on GPU 1"):
        R._check_temporal_tensor("motion", fake_cuda((4, 4, 2)), 1, {torch.float32: (4, 4, 2)})
    with pytest.raises(ValueError, match="frame_rgba8: a contiguous torch.int32 tensor of shape .4, 4. or torch.uint8 tensor of shape .4, 4, 4. is expected"):
        R._check_temporal_tensor("frame_rgba8", fake_cuda((4, 4)), 0, {torch.int32: (4, 4), torch.uint8: (4, 4, 4)})
    with pytest.raises(ValueError, match="hit: a contiguous"):
        R._check_temporal_tensor("hit", fake_cuda((8, 4, 4)).permute(2, 1, 0), 0, {torch.float32: (4, 4, 8)})
    # the method itself, on an object without a context: what it refuses, it refuses before the library is called
    r = bare_renderer()
    with pytest.raises(ValueError, match="motion is required"):
        r.temporalAccumulate(1, None, 1, 1, 1, 1, 1, 1, history_out=1, length_out=1)
    with pytest.raises(ValueError, match=r"length_in: a contiguous torch.float32 tensor of shape \(4, 4\) is expected"):
        r.temporalAccumulate(1, 1, 1, 1, 1, 1, 1, fake_cuda((4, 4, 1)), history_out=1, length_out=1)
    with pytest.raises(ValueError, match="the mask needs"):
        r.blockGrid = lambda: (1, 1)
        r.temporalAccumulate(1, 1, 1, 1, 1, 1, 1, 1, history_out=1, length_out=1, mask=np.ones((2, 2)))


def test_cxx_facade_compiles(tmp_path):
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t reproject(SampleRenderer& sample, pt_temporal_desc d) {\n"
        "    d.flags = PT_TEMPORAL_CLEAR_COLOR;\n"
        "    pt_temporal_stats s{};\n"
        "    sample.temporalAccumulate(d, &s);\n"
        "    return sample.temporalAccumulate(d).reprojected + s.pixels;\n"
        "}\n"
    )


def test_header_states_the_contract():
    text = header_text()
    for item in ("c = color[p].xyz * color_scale", "px >= -1 && px <= wr && py >= -1 && py <= hr", "flx = floorf(px), ix = (int)flx, fx = px - flx",
                 "length_in[q] >= 1", "exponent-bit test", "dot3(ng_p, ng_q) >= normal_cos",
                 "fabsf(dot3(ng_p, prev_position[q].xyz - position[p].xyz)) <= plane_eps * hit[p].t", "Wsum = ((w00 + w10) + w01) + w11",
                 "n = fminf(nprev, (float)(max_history - 1)); a = 1.0f / (n + 1.0f); out = H + (c - H) * a; len = n + 1",
                 "float32 NumPy evaluating this reproduces every output bit for bit", "No other pixel is written in any output",
                 "Zero pixels launch nothing and return PT_OK", "color_scale = (float)(k + 1)", "redraw = 1 is the exact alternative",
                 "unknown flag bits"):
        assert item in text, item


# ------------------------------------------------------------------ properties of the NumPy reference on synthetic planes
def _flat(h, w, color):
    """one surface everywhere (mesh 0, normal +z, z = 0 plane), zero motion, the colour plane given"""
    hit = np.zeros((h, w, 8), f32)
    hit[..., 0] = 5.0
    hit[..., 7] = 1.0  # ng = (0, 0, 1); prim = mesh = 0
    pos = np.zeros((h, w, 4), f32)
    pos[..., 0], pos[..., 1] = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    pos[..., 3] = 1
    return dict(color=color, motion=np.zeros((h, w, 2), f32), hit=hit, position=pos, prev_hit=hit, prev_position=pos)


def test_zero_motion_gives_the_running_mean_and_saturates(orc_det):
    h, w, frames, cap = 5, 9, 8, 5
    rng = np.random.default_rng(3)
    px = np.ones((h, w), bool)
    hist, ln = np.zeros((h, w, 4), f32), np.zeros((h, w), f32)
    colours = rng.random((frames, h, w, 4), dtype=f32)
    mean = np.zeros((h, w, 3), np.float64)
    for k in range(frames):
        ref = T.temporal_ref(orc_det, dict(_flat(h, w, colours[k]), history_in=hist, length_in=ln), [(0, 0, w, h)], px, max_history=cap)
        hist, ln = ref["history_out"].view(f32), ref["length_out"].view(f32)
        n = min(k + 1, cap)
        assert (ln == n).all() and ref["reprojected"] == (w * h if k else 0) and (hist[..., 3] == 1).all()
        # the running mean while the length grows, an exponential average with weight 1 / cap once it has saturated
        mean = mean + (colours[k, ..., :3].astype(np.float64) - mean) / n
        assert np.abs(hist[..., :3] - mean).max() < 1e-6
    assert n == cap and (ref["frame_rgba8"] >> 24 == 255).all()


def test_a_nan_in_the_history_heals_after_one_frame(orc_det):
    h, w = 4, 6
    px = np.ones((h, w), bool)
    hist = np.full((h, w, 4), 0.5, f32)
    hist[2, 3, 1] = np.nan
    hist[1, 1, 0] = np.inf
    ln = np.full((h, w), 4, f32)
    colour = np.full((h, w, 4), 0.25, f32)
    ref = T.temporal_ref(orc_det, dict(_flat(h, w, colour), history_in=hist, length_in=ln), [(0, 0, w, h)], px)
    bad = np.zeros((h, w), bool)
    bad[2, 3] = bad[1, 1] = True
    out, ln1 = ref["history_out"].view(f32), ref["length_out"].view(f32)
    assert np.isfinite(out).all() and np.array_equal(ref["valid"], ~bad)
    assert (ln1[bad] == 1).all() and (ln1[~bad] == 5).all() and (out[bad][:, :3] == 0.25).all()
    # (zero motion: three taps of weight zero, and the one that carries the weight is not finite)
    assert (ref["reason"][bad] == T.BIT["history"] | T.BIT["nolookup"]).all() and not ref["reason"][~bad].any()
    ref2 = T.temporal_ref(orc_det, dict(_flat(h, w, colour), history_in=out, length_in=ln1), [(0, 0, w, h)], px)
    assert ref2["valid"].all() and (ref2["length_out"].view(f32)[bad] == 2).all()


def test_pixels_outside_the_set_keep_the_fill(orc_det):
    h, w = 8, 16
    px = np.zeros((h, w), bool)
    px[:, 8:] = True
    colour = np.full((h, w, 4), 0.25, f32)
    ref = T.temporal_ref(orc_det, dict(_flat(h, w, colour), history_in=colour, length_in=np.ones((h, w), f32)), [(8, 0, 8, h)], px, clear=True)
    for name in T.OUTPUTS:
        assert (ref[name][~px] == T.SENTINEL).all() and not (ref[name][px] == T.SENTINEL).any()
    assert not ref["color"][px].any() and (ref["color"][~px] == f32(0.25).view(np.uint32)).all()
    assert ref["reprojected"] == 8 * h


# ------------------------------------------------------------------ the GPU tests' real-plane inputs exercise every rejection reason
# counts with the CPU-built planes (valid, invalid, pixels showing each reason among the invalid):
COUNTS = {
    "two_box": (1240, 6751, dict(rect=3895, nolookup=102, length=1478, history=160, miss=1835, mesh=213, normal=11, plane=722, min_weight=264)),
    "terrain": (2113, 5878, dict(rect=3385, nolookup=717, length=1031, history=152, miss=1458, mesh=122, normal=186, plane=39, min_weight=299)),
}


@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_real_inputs_cover_every_rejection_reason(orc_det, name):
    make, size, cam, prev, prm, seed = T.real_inputs()[name]
    w, h = size
    planes = T.with_random_history(T.cpu_planes(orc_det, make(), size, cam, prev), seed)
    px = np.ones((h, w), bool)
    ref = T.temporal_ref(orc_det, planes, [(0, 0, w, h)], px, **prm)
    got = T.check_coverage(ref, px, name)
    assert got == COUNTS[name], got
