"""Viewports (pt_set_views) without a GPU: the six entry points are declared and exported, the ctypes mirror of pt_view matches the compiler's
layout, the header still compiles as C99 and as C++17, a null context is refused before any device work, both facades have the new methods —
and the header carries the contract tests/test_gpu_views.py checks on the GPU (what a view pixel holds, the refusal list)."""
import ctypes as C
import re

from cabi_kit import check_layout, compile_c99_and_cxx17, compile_facade, header, header_text
from optixpathtracer_amd import _lib

NAMES = ("pt_set_views", "pt_get_views", "pt_set_view_cameras", "pt_set_view_cameras_device", "pt_multi_set_views", "pt_multi_set_view_cameras")


def test_library_exports_the_entry_points():
    L = _lib.load_library()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NAMES:
        first = "pt_multi" if name.startswith("pt_multi") else "pt_ctx"
        assert re.search(r"int\s+%s\s*\(\s*(const\s+)?%s\s*\*" % (name, first), src), name
    assert re.search(r"#define\s+PT_MAX_VIEWS\s+4096\b", src) and _lib.PT_MAX_VIEWS == 4096
    assert L.pt_version().startswith(b"ptamd 0.4")


def test_view_struct_layout_matches_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.View, "pt_view", ("x", "y", "width", "height", "eye", "U", "V", "W"))], [64, 0, 4, 8, 12, 16, 28, 40, 52])


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = '#include "pt_amd.h"\nint use(pt_ctx* c) { pt_view v = {0, 0, 8, 8, {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}}; return pt_set_views(c, &v, 1); }\n'
    compile_c99_and_cxx17(tmp_path, body)


def test_null_context_is_refused_without_a_gpu():
    L = _lib.load_library()
    v = _lib.View(0, 0, 8, 8)
    assert L.pt_set_views(None, C.byref(v), 1) == -1
    assert b"pt_set_views" in L.pt_last_error(None)
    cams = (C.c_float * 12)()
    assert L.pt_set_view_cameras(None, cams, 1) == -1
    assert b"pt_set_view_cameras" in L.pt_last_error(None)
    assert L.pt_set_view_cameras_device(None, cams, 1) == -1
    assert b"pt_set_view_cameras_device" in L.pt_last_error(None)
    n = C.c_uint32(77)
    assert L.pt_get_views(None, None, 0, C.byref(n)) == -1 and n.value == 77
    assert L.pt_multi_set_views(None, C.byref(v), 1) == -1
    assert L.pt_multi_set_view_cameras(None, cams, 1) == -1


def test_python_facades_have_the_methods():
    from optixpathtracer_amd import renderer as R

    for cls in (R.SampleRenderer, R.MultiRenderer):
        for name in ("setViews", "views", "setViewCameras"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
    cam = R.Camera((0.0, 1.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 2.0)
    arr = R._view_array([(8, 16, 20, 10, cam)])
    U, V, W = cam.UVWFrame()
    assert (arr[0].x, arr[0].y, arr[0].width, arr[0].height) == (8, 16, 20, 10)
    assert list(arr[0].eye) == [0.0, 1.0, 5.0] and list(arr[0].U) == U.tolist() and list(arr[0].V) == V.tolist() and list(arr[0].W) == W.tolist()
    rows = R._camera_rows([cam, cam])
    assert rows.shape == (2, 12) and rows[1].tolist() == [0.0, 1.0, 5.0] + U.tolist() + V.tolist() + W.tolist()


def test_cxx_facades_compile(tmp_path):
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "void stereo(SampleRenderer& sample, MultiSampleRenderer& multi, const Camera& left, const Camera& right) {\n"
        "    const int2 size = sample.launchParams.frame.size;\n"
        "    std::vector<View> views{{0, 0, size.x / 2, size.y, left}, {size.x / 2, 0, size.x / 2, size.y, right}};\n"
        "    sample.setViews(views);\n"
        "    sample.setViewCameras({right, left});\n"
        "    sample.render();\n"
        "    sample.setViews({});\n"
        "    multi.setViews(views);\n"
        "}\n"
    )


def test_header_states_the_contract():
    text = header_text()
    assert "A pixel in no view is not touched in any buffer by any render call" in text
    for item in ("a null context", "null `views` with n > 0", "no pt_resize yet", "n > PT_MAX_VIEWS", "x or y negative or not a multiple of 8",
                 "width or height < 1", "a rectangle leaving the frame", "two rectangles sharing a pixel"):
        assert item in text, item
    for item in ("tea4(y * v.width + x, subframe)", "pt_set_camera is remembered but unused", "wait for the frames in flight first",
                 "n must equal the current view count", "pt_resize and pt_set_partition drop the views", "pt_set_views implies pt_adaptive_end",
                 "PT_ERR_UNSUPPORTED", "does not know about view borders"):
        assert item in text, item
