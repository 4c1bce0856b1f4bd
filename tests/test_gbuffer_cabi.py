"""The first-hit G-buffer (pt_render_gbuffer) without a GPU: the entry point is declared and exported, the ctypes mirrors of pt_gbuffer_desc and
pt_gbuffer_stats match the compiler's layout, the header still compiles as C99 and as C++17, a null context and a null description are refused
before any device work, and both facades have the method.

pt_version() stays "ptamd 0.4": five existing tests pin that string, and it names the struct layouts, which this entry point does not change
(include/pt_amd.h, VERSIONING: a caller that may meet an older library looks the symbol up)."""
import ctypes as C
import os
import re

from cabi_kit import check_layout, compile_c99_and_cxx17, compile_facade, header, header_text
from conftest import ROOT
from optixpathtracer_amd import _lib

DESC_FIELDS = ("hit", "depth", "position", "motion", "ray", "prev_cameras", "num_prev_cameras", "block_mask")
STATS_FIELDS = ("pixels", "hits", "kernel_ms")


def test_library_exports_the_entry_point():
    L = _lib.load_library()
    assert "pt_render_gbuffer" in _lib.EXPORTS and hasattr(L, "pt_render_gbuffer")
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int\s+pt_render_gbuffer\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_gbuffer_desc\s*\*\s*\w+\s*,\s*pt_gbuffer_stats\s*\*", src)
    assert L.pt_version().startswith(b"ptamd 0.4")
    assert "pt_render_gbuffer" in header().split("VERSIONING.")[1].split("*/")[0]  # the note names it among the entry points added at 0.4


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.GBufferDesc, "pt_gbuffer_desc", DESC_FIELDS), (_lib.GBufferStats, "pt_gbuffer_stats", STATS_FIELDS)],
                 [64, 0, 8, 16, 24, 32, 40, 48, 56, 24, 0, 8, 16])
    assert _lib.GBUFFER_PLANES == {"hit": 8, "depth": 1, "position": 4, "motion": 2, "ray": 8} and C.sizeof(_lib.Hit) == 4 * _lib.GBUFFER_PLANES["hit"]


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, float* depth, const float* prev) {\n"
            "    pt_gbuffer_desc d = {0, 0, 0, 0, 0, 0, 0, 0};\n"
            "    pt_gbuffer_stats s;\n"
            "    d.depth = depth; d.prev_cameras = prev; d.num_prev_cameras = 1;\n"
            "    return pt_render_gbuffer(c, &d, &s);\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_context_and_null_description_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.GBufferDesc(), _lib.GBufferStats(7, 7, 7.0)
    assert L.pt_render_gbuffer(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_render_gbuffer: null context" in L.pt_last_error(None)
    assert L.pt_render_gbuffer(None, None, None) == -1
    assert (s.pixels, s.hits, s.kernel_ms) == (7, 7, 7.0)
    # a null description is refused before the context is looked at (the text of pt_gbuffer.hip; a live context needs a GPU: tests/test_gpu_gbuffer.py)
    api = open(os.path.join(ROOT, "optixpathtracer_amd", "csrc", "pt_gbuffer.hip")).read()
    body = api.split('extern "C" int pt_render_gbuffer(')[1]
    assert body.index("null description") < body.index("ctx->width")


def test_python_facade_has_the_method():
    from optixpathtracer_amd import renderer as R

    assert callable(getattr(R.SampleRenderer, "renderGBuffer", None))
    assert callable(getattr(R, "_check_temporal_tensor", None))  # the one plane checker of the facade


def test_cxx_facade_compiles(tmp_path):
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t first_hits(SampleRenderer& sample, float* d_depth, float* d_motion, const float* prev) {\n"
        "    pt_gbuffer_desc d{};\n"
        "    d.depth = d_depth;\n"
        "    d.motion = d_motion;\n"
        "    d.prev_cameras = prev;\n"
        "    d.num_prev_cameras = 1;\n"
        "    pt_gbuffer_stats s{};\n"
        "    sample.renderGBuffer(d, &s);\n"
        "    return sample.renderGBuffer(d).hits + s.pixels;\n"
        "}\n"
    )


def test_header_states_the_contract():
    text = header_text()
    for item in ("dx = 2 * ((x + 0.5f) / width) - 1", "tmin 0.001f, tmax 1e16f", "t * dot3(dir, normalize3(W))", "a miss holds +inf (0x7f800000)",
                 "px = (((a / c) + 1) * 0.5f) * width - 0.5f", "both words are 0x7fc00000", "A pixel outside that set is not written in any plane",
                 "Zero active pixels launch nothing and return PT_OK", "all five planes NULL", "motion without prev_cameras",
                 "a non-finite previous camera value", "PT_ERR_UNSUPPORTED"):
        assert item in text, item
