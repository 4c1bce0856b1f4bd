"""Block masks and adaptive stopping without a GPU: the entry points are declared and exported, the ctypes mirrors of pt_adaptive_params and
pt_adaptive_stats match the compiler's layout, a null context is refused before any device work, the C++ facade methods compile — and the
numpy float32 transcription of the stopping rule (include/pt_amd.h states it operation by operation).  The transcription is the checker of
the policy: tests/test_gpu_adaptive.py compares every decision of the GPU kernel with it."""
import ctypes as C
import re

import numpy as np

from adaptive_ref import block_slots, butterfly, rule_sides, stop_rule
from cabi_kit import check_layout, compile_facade, header
from optixpathtracer_amd import _lib


def _moments(h, w, n, values):
    """n subframes whose luminances are values[k] (each (h, w) or scalar)"""
    mo = np.zeros((h, w, 4), np.float32)
    for k in range(n):
        x = np.broadcast_to(np.asarray(values[k], np.float32), (h, w))
        mo[..., 0] += np.float32(1)
        mo[..., 1] += x
        mo[..., 2] += x * x
    return mo


def test_rule_on_hand_made_moments():
    h, w = 13, 20  # 2 x 3 blocks, the right column and the bottom row are edge blocks
    blocks = np.arange(6)
    rng = np.random.default_rng(7)
    flat = [0.5, 0.5, 0.5, 0.5]
    noisy = [rng.random((h, w)).astype(np.float32) for _ in range(4)]
    # zero variance stops at min_subframes, and not before
    assert stop_rule(_moments(h, w, 3, flat), blocks, 0.01, 0.0, 3, 0).all()
    assert not stop_rule(_moments(h, w, 2, flat), blocks, 0.01, 0.0, 3, 0).any()
    assert not stop_rule(_moments(h, w, 2, flat), blocks, 1e9, 1.0, 3, 0).any()  # n < min_subframes never stops, whatever the threshold
    # max_subframes stops regardless of the variance and of min_subframes
    assert stop_rule(_moments(h, w, 4, noisy), blocks, 0.0, 0.0, 100, 4).all()
    assert not stop_rule(_moments(h, w, 3, noisy), blocks, 0.0, 0.0, 100, 4).any()
    # threshold 0 stops only V == 0: make one block flat in an otherwise noisy image
    vals = [x.copy() for x in noisy]
    for x in vals:
        x[0:8, 8:16] = 0.25
    stop = stop_rule(_moments(h, w, 4, vals), blocks, 0.0, 0.0, 2, 0)
    assert stop.tolist() == [False, True, False, False, False, False]
    # a generous threshold stops the noisy blocks too, a tight one does not; the dark floor only ever helps
    assert stop_rule(_moments(h, w, 4, noisy), blocks, 1.0, 0.0, 2, 0).all()
    assert not stop_rule(_moments(h, w, 4, noisy), blocks, 0.01, 0.0, 2, 0).any()
    assert stop_rule(_moments(h, w, 4, noisy), blocks, 0.01, 100.0, 2, 0).all()


def test_rule_sums_are_the_documented_butterfly():
    """The order of the two sums is part of the contract: a butterfly over 64 slots, zeros outside the image — not a sequential sum."""
    rng = np.random.default_rng(3)
    a = (rng.random((1, 64)) * 1000).astype(np.float32)
    want = a[0].copy()
    for off in (32, 16, 8, 4, 2, 1):
        want = np.array([np.float32(want[l]) + np.float32(want[l ^ off]) for l in range(64)], np.float32)
    assert butterfly(a)[0] == want[0] and (want == want[0]).all()
    h, w = 5, 11  # one full-width block and an edge block 3 wide, both 5 high
    mo = _moments(h, w, 3, [rng.random((h, w)).astype(np.float32) for _ in range(3)])
    n, V, M, N = rule_sides(mo, np.arange(2))
    assert N.tolist() == [40.0, 15.0] and n.tolist() == [3.0, 3.0]
    slots = block_slots(np.arange(h * w).reshape(h, w), -1)
    assert slots[1, 0] == 8 and slots[1, 2] == 10 and slots[1, 3] == -1 and slots[1, 8] == 11 + 8 and slots[0, 63] == -1


# ------------------------------------------------------------------ the C boundary
def test_header_declares_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in ("pt_render_mask", "pt_adaptive_begin", "pt_render_adaptive", "pt_adaptive_end", "pt_download_adaptive"):
        assert re.search(r"int\s+%s\s*\(\s*pt_ctx\s*\*" % name, src), name
        assert name in _lib.EXPORTS
    assert re.search(r"pt_render_mask\s*\([^)]*const\s+uint8_t\s*\*\s*block_mask[^)]*uint32_t\s*\*\s*active_pixels", src)
    assert "PT_ADAPT_MOMENTS = 0" in src and "PT_ADAPT_ACTIVE = 1" in src
    assert (_lib.PT_ADAPT_MOMENTS, _lib.PT_ADAPT_ACTIVE) == (0, 1)
    L = _lib.load_library()
    assert L.pt_version().startswith(b"ptamd 0.4")


def test_adaptive_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.AdaptiveParams, "pt_adaptive_params", ("threshold", "dark_floor", "min_subframes", "max_subframes")),
                            (_lib.AdaptiveStats, "pt_adaptive_stats", ("blocks", "active_blocks", "active_pixels", "pixel_subframes", "decide_ms"))],
                 [16, 0, 4, 8, 12] + [32, 0, 4, 8, 16, 24])


def test_null_context_is_refused_without_a_gpu():
    L = _lib.load_library()
    mask = (C.c_uint8 * 4)(1, 1, 1, 1)
    n = C.c_uint32(77)
    assert L.pt_render_mask(None, 1, 0, mask, None, C.byref(n)) == -1
    assert n.value == 77 and b"pt_render_mask" in L.pt_last_error(None)
    prm = _lib.AdaptiveParams(0.01, 0.0, 4, 0)
    assert L.pt_adaptive_begin(None, C.byref(prm)) == -1
    assert b"pt_adaptive_begin" in L.pt_last_error(None)
    st = _lib.AdaptiveStats()
    assert L.pt_render_adaptive(None, 1, 0, None, C.byref(st)) == -1
    assert b"pt_render_adaptive" in L.pt_last_error(None) and st.blocks == 0
    assert L.pt_adaptive_end(None) == -1
    assert b"pt_adaptive_end" in L.pt_last_error(None)
    buf = (C.c_uint8 * 4)()
    assert L.pt_download_adaptive(None, _lib.PT_ADAPT_ACTIVE, buf, 4) == -1
    assert b"pt_download_adaptive" in L.pt_last_error(None)


def test_facade_mask_and_adaptive_compile(tmp_path):
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t progressive(SampleRenderer& sample, std::vector<uint32_t>& pixels) {\n"
        "    const int2 size = sample.launchParams.frame.size;\n"
        "    std::vector<uint8_t> mask((size_t)((size.x + 7) / 8) * ((size.y + 7) / 8), 1);\n"
        "    sample.launchParams.frame.subframe_index = 0;\n"
        "    uint32_t active = sample.renderMask(mask, pixels.data());\n"
        "    active += sample.renderMask(mask);\n"
        "    pt_adaptive_params prm{0.02f, 0.01f, 8u, 256u};\n"
        "    sample.adaptiveBegin(prm);\n"
        "    pt_adaptive_stats st{};\n"
        "    do {\n"
        "        st = sample.renderAdaptive(pixels.data());\n"
        "        sample.launchParams.frame.subframe_index++;\n"
        "    } while (st.active_blocks > 0);\n"
        "    sample.adaptiveEnd();\n"
        "    return st.pixel_subframes + active;\n"
        "}\n"
    )
