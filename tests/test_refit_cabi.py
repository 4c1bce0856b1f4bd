"""The in-place vertex update entry points without a GPU: declared in the header, the ctypes mirror of pt_mesh_update matches the
compiler's layout, a null context is refused before any device work, and the C++ facade's updateMeshes compiles."""
import ctypes as C
import re

from cabi_kit import check_layout, compile_facade, header
from optixpathtracer_amd import _lib


def test_header_declares_the_update_entry_points():
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int\s+pt_update_meshes\s*\(\s*pt_ctx\s*\*", src)
    assert re.search(r"int\s+pt_multi_update_meshes\s*\(\s*pt_multi\s*\*", src)
    assert "PT_UPDATE_REFIT = 0" in src and "PT_UPDATE_REBUILD = 1" in src
    assert {"pt_update_meshes", "pt_multi_update_meshes"} <= set(_lib.EXPORTS)
    assert (_lib.PT_UPDATE_REFIT, _lib.PT_UPDATE_REBUILD) == (0, 1)


def test_mesh_update_layout_matches_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.MeshUpdate, "pt_mesh_update", ("mesh", "vertex", "num_vertices"))], [24, 0, 8, 16])


def test_null_context_is_refused_without_a_gpu():
    L = _lib.load_library()
    ups = (_lib.MeshUpdate * 1)()
    ms = C.c_double(-1.0)
    assert L.pt_update_meshes(None, ups, 1, _lib.PT_UPDATE_REFIT, C.byref(ms)) == -1
    assert L.pt_update_meshes(None, None, 0, _lib.PT_UPDATE_REBUILD, None) == -1
    assert L.pt_multi_update_meshes(None, ups, 1, _lib.PT_UPDATE_REFIT, None) == -1
    assert ms.value == -1.0
    assert b"pt_update_meshes" in L.pt_last_error(None)


def test_facade_update_meshes_compiles(tmp_path):
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "double animate(SampleRenderer& sample, MultiSampleRenderer& multi, Model* model) {\n"
        "    for (float3& v : model->meshes[0]->vertex) v.y += 0.5f;\n"
        "    double ms = sample.updateMeshes(model, {0u});\n"
        "    ms += sample.updateMeshes(model, {0u}, /*rebuild=*/true);\n"
        "    ms += multi.updateMeshes(model, std::vector<uint32_t>{0u});\n"
        "    sample.launchParams.frame.subframe_index = 0;\n"
        "    return ms;\n"
        "}\n"
    )
