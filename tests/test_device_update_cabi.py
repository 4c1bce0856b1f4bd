"""The device-fed update entry points without a GPU: declared in the header and exported, the ctypes mirror of pt_mesh_transform matches
the compiler's layout, a null context is refused before any device work, and the C++ facades' transformMeshes / updateMeshesDevice compile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cabi_kit import compile_facade, header
from conftest import ROOT
from optixpathtracer_amd import _lib

NAMES = ("pt_update_meshes_device", "pt_transform_meshes", "pt_multi_transform_meshes", "pt_download_vertices")


def test_header_declares_the_device_update_entry_points():
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int\s+pt_update_meshes_device\s*\(\s*pt_ctx\s*\*", src)
    assert re.search(r"int\s+pt_transform_meshes\s*\(\s*pt_ctx\s*\*", src)
    assert re.search(r"int\s+pt_multi_transform_meshes\s*\(\s*pt_multi\s*\*", src)
    assert re.search(r"int\s+pt_download_vertices\s*\(\s*pt_ctx\s*\*", src)
    assert "PT_FROM_REST = 0" in src and "PT_FROM_CURRENT = 1" in src
    assert set(NAMES) <= set(_lib.EXPORTS)
    assert (_lib.PT_FROM_REST, _lib.PT_FROM_CURRENT) == (0, 1)
    L = _lib.load_library()
    for n in NAMES:
        assert hasattr(L, n), f"libptamd.so lacks {n}"
    assert L.pt_version().startswith(b"ptamd 0.4")


def test_header_states_the_transform_order():
    """The arithmetic contract NumPy parity rests on is part of the header."""
    text = " ".join(header().split())
    assert "x' = ((m[0]*x + m[1]*y) + m[2]*z) + m[3]" in text
    assert "hipPointerGetAttributes" in text and "4-byte aligned" in text


def test_mesh_transform_layout_matches_the_compiler(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "pt_amd.h"\n'
        'int main(void) { printf("%zu %zu %zu\\n", sizeof(pt_mesh_transform), offsetof(pt_mesh_transform, mesh), '
        "offsetof(pt_mesh_transform, m)); return 0; }\n"
    )
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, o_mesh, o_m = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    M = _lib.MeshTransform
    assert (C.sizeof(M), M.mesh.offset, M.m.offset) == (size, o_mesh, o_m)
    assert C.sizeof(M) == 52


def test_null_context_is_refused_without_a_gpu():
    L = _lib.load_library()
    ups = (_lib.MeshUpdate * 1)()
    xf = (_lib.MeshTransform * 1)()
    buf = (C.c_float * 3)()
    ms = C.c_double(-1.0)
    assert L.pt_update_meshes_device(None, ups, 1, _lib.PT_UPDATE_REFIT, C.byref(ms)) == -1
    assert b"pt_update_meshes_device" in L.pt_last_error(None)
    assert L.pt_transform_meshes(None, xf, 1, _lib.PT_FROM_REST, _lib.PT_UPDATE_REFIT, C.byref(ms)) == -1
    assert b"pt_transform_meshes" in L.pt_last_error(None)
    assert L.pt_multi_transform_meshes(None, xf, 1, _lib.PT_FROM_CURRENT, _lib.PT_UPDATE_REBUILD, C.byref(ms)) == -1
    assert b"pt_multi_transform_meshes" in L.pt_last_error(None)
    assert L.pt_download_vertices(None, 0, 0, buf, 12) == -1
    assert b"pt_download_vertices" in L.pt_last_error(None)
    assert L.pt_update_meshes_device(None, None, 0, _lib.PT_UPDATE_REBUILD, None) == -1
    assert L.pt_transform_meshes(None, None, 0, 7, 7, None) == -1
    assert ms.value == -1.0


def test_python_facade_marshals_matrices():
    from optixpathtracer_amd import renderer as R

    m4 = np.arange(16, dtype=np.float64).reshape(4, 4)
    arr, n = R._mesh_transforms({3: m4, 1: m4[:3] + 0.5})
    assert n == 2 and (arr[0].mesh, arr[1].mesh) == (3, 1)
    assert list(arr[0].m) == [float(x) for x in range(12)]  # the last row of a 4x4 is dropped
    assert list(arr[1].m) == [x + 0.5 for x in range(12)]
    arr, n = R._mesh_transforms([(2, m4), (2, m4)])  # the list form can name a mesh twice (the library refuses it)
    assert n == 2 and arr[1].mesh == 2
    with pytest.raises(ValueError):
        R._mesh_transforms({0: np.zeros((3, 3))})
    for name in ("updateMeshesDevice", "transformMeshes", "downloadVertices"):
        assert callable(getattr(R.SampleRenderer, name))
    assert callable(R.MultiRenderer.transformMeshes)


def test_facade_device_updates_compile(tmp_path):
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "double animate(SampleRenderer& sample, MultiSampleRenderer& multi, const float* d_vertices, uint32_t nv) {\n"
        "    const pt_mesh_transform slide{1u, {1, 0, 0, 0.5f, 0, 1, 0, 0, 0, 0, 1, 0}};\n"
        "    double ms = sample.transformMeshes({slide});\n"
        "    ms += sample.transformMeshes({slide}, /*from_current=*/true, /*rebuild=*/true);\n"
        "    ms += multi.transformMeshes(std::vector<pt_mesh_transform>{slide});\n"
        "    ms += sample.updateMeshesDevice({pt_mesh_update{0u, d_vertices, nv}});\n"
        "    ms += sample.updateMeshesDevice({pt_mesh_update{0u, d_vertices, nv}}, /*rebuild=*/true);\n"
        "    sample.launchParams.frame.subframe_index = 0;\n"
        "    return ms;\n"
        "}\n"
    )
