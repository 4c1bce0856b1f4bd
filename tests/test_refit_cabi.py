"""The in-place vertex update entry points without a GPU: declared in the header, the ctypes mirror of pt_mesh_update matches the
compiler's layout, a null context is refused before any device work, and the C++ facade's updateMeshes compiles."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT
from optixpathtracer_amd import _lib


def _header():
    return open(os.path.join(ROOT, "include", "pt_amd.h")).read()


def test_header_declares_the_update_entry_points():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+pt_update_meshes\s*\(\s*pt_ctx\s*\*", src)
    assert re.search(r"int\s+pt_multi_update_meshes\s*\(\s*pt_multi\s*\*", src)
    assert "PT_UPDATE_REFIT = 0" in src and "PT_UPDATE_REBUILD = 1" in src
    assert {"pt_update_meshes", "pt_multi_update_meshes"} <= set(_lib.EXPORTS)
    assert (_lib.PT_UPDATE_REFIT, _lib.PT_UPDATE_REBUILD) == (0, 1)


def test_mesh_update_layout_matches_the_compiler(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "pt_amd.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(pt_mesh_update), offsetof(pt_mesh_update, mesh), '
        "offsetof(pt_mesh_update, vertex), offsetof(pt_mesh_update, num_vertices)); return 0; }\n"
    )
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, o_mesh, o_vertex, o_nv = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    M = _lib.MeshUpdate
    assert (C.sizeof(M), M.mesh.offset, M.vertex.offset, M.num_vertices.offset) == (size, o_mesh, o_vertex, o_nv)


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
    src = tmp_path / "facade.cpp"
    src.write_text(
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
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", ROOT, "-I", os.path.join(ROOT, "include"), str(src)], check=True)
