"""Device ray queries (pt_trace_device, pt_query_wait) without a GPU: declared in the header and exported, pt_hit and pt_query_stats laid out
as the ctypes and NumPy mirrors say, a null context refused before any device work, the Python facade's argument checks, and the C++
facade's traceDevice compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from cabi_kit import compile_facade, header
from conftest import ROOT
from optixpathtracer_amd import _lib

NAMES = ("pt_trace_device", "pt_query_wait")
HIT_FIELDS = ("t", "u", "v", "prim", "mesh", "ng")
STATS_FIELDS = ("rays", "hits", "invalid_rays", "stage_ms", "trace_ms", "attrib_ms", "state_bytes")


def test_header_declares_the_query_entry_points():
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int\s+pt_trace_device\s*\(\s*pt_ctx\s*\*\s*\w*\s*,\s*const\s+float\s*\*", src)
    assert re.search(r"int\s+pt_query_wait\s*\(\s*pt_ctx\s*\*\s*\w*\s*,\s*pt_query_stats\s*\*", src)
    assert "PT_QUERY_CLOSEST = 0" in src and "PT_QUERY_ANY = 1" in src and "PT_QUERY_ASYNC = 2" in src
    assert re.search(r"typedef\s+struct\s+pt_hit\s*\{", src) and re.search(r"typedef\s+struct\s+pt_query_stats\s*\{", src)
    assert set(NAMES) <= set(_lib.EXPORTS)
    assert (_lib.PT_QUERY_CLOSEST, _lib.PT_QUERY_ANY, _lib.PT_QUERY_ASYNC) == (0, 1, 2)
    L = _lib.load_library()
    for n in NAMES:
        assert hasattr(L, n), f"libptamd.so lacks {n}"
    assert L.pt_version().startswith(b"ptamd 0.4")


def test_header_states_the_barycentric_expression():
    """The arithmetic NumPy parity rests on, and the pointer contract, are part of the header."""
    text = " ".join(header().split())
    assert "det = (Uw + Vw) + Ww; u = Vw / det; v = Ww / det" in text
    assert "Uw = dot(d, cross(C, B)), Vw = dot(d, cross(A, C)), Ww = dot(d, cross(B, A))" in text
    assert "pt_trace_device" in text.split("STREAM CONTRACT")[1].split("VERSIONING")[0]


def test_hit_and_stats_layout_match_the_compiler(tmp_path):
    src = tmp_path / "probe.c"
    hit = ", ".join(f"offsetof(pt_hit, {f})" for f in HIT_FIELDS)
    st = ", ".join(f"offsetof(pt_query_stats, {f})" for f in STATS_FIELDS)
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "pt_amd.h"\n'
        "int main(void) {\n"
        f"    size_t v[] = {{sizeof(pt_hit), {hit}, sizeof(pt_query_stats), {st}}};\n"
        '    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]);\n'
        "    return 0;\n}\n"
    )
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    v = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert v[0] == 32 and v[1:7] == [0, 4, 8, 12, 16, 20]  # the documented record
    H, S = _lib.Hit, _lib.QueryStats
    assert [C.sizeof(H)] + [getattr(H, f).offset for f in HIT_FIELDS] == v[:7]
    assert [C.sizeof(S)] + [getattr(S, f).offset for f in STATS_FIELDS] == v[7:]
    D = _lib.HIT_DTYPE
    assert [D.itemsize] + [D.fields[f][1] for f in HIT_FIELDS] == v[:7]
    assert D["prim"] == np.int32 and D["mesh"] == np.int32 and D["ng"].shape == (3,)


def test_null_context_is_refused_without_a_gpu():
    L = _lib.load_library()
    s = _lib.QueryStats()
    s.rays = 77
    assert L.pt_trace_device(None, None, 1, _lib.PT_QUERY_CLOSEST, None, C.byref(s)) == -1
    assert b"pt_trace_device" in L.pt_last_error(None)
    assert L.pt_query_wait(None, C.byref(s)) == -1
    assert b"pt_query_wait" in L.pt_last_error(None)
    assert L.pt_trace_device(None, None, 0, _lib.PT_QUERY_ANY | _lib.PT_QUERY_ASYNC, None, None) == -1
    assert s.rays == 77  # a refused call writes no statistics


class _Elsewhere(torch.Tensor):
    """A tensor that says it lives on another GPU (there is none on this machine): only the facade's checks look at it."""

    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda", 1))


class _NoLibrary:
    """Stands for libptamd.so: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the facade called {name} before checking its arguments")


def test_python_facade_checks_tensors_before_calling_the_library():
    from optixpathtracer_amd import renderer as R

    r = object.__new__(R.SampleRenderer)
    r._device, r._L, r._ctx = 0, _NoLibrary(), None
    good = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="rays: the tensor is on cpu"):
        r.traceDevice(good)
    with pytest.raises(TypeError, match="torch tensor"):
        r.traceDevice(np.zeros((4, 8), np.float32))
    other = torch.Tensor._make_subclass(_Elsewhere, good)
    with pytest.raises(ValueError, match="on cuda:1, the context on GPU 0"):
        r.traceDevice(other)
    r._device = 1  # ... and past the device check, the dtype, the shape and the row stride are looked at
    for bad in (good.double(), torch.zeros(4, 7), torch.zeros(8, 4).t(), torch.zeros(4, 16)[:, :8], torch.zeros(32), torch.zeros(2, 4, 8)):
        with pytest.raises(ValueError, match="rays: a contiguous torch.float32 tensor of shape \\(n, 8\\)"):
            r.traceDevice(torch.Tensor._make_subclass(_Elsewhere, bad))
    rays = torch.Tensor._make_subclass(_Elsewhere, torch.zeros(9)[1:].view(1, 8))  # a storage offset of one float is fine
    with pytest.raises(ValueError, match="out: the tensor is on cpu"):
        r.traceDevice(rays, out=torch.zeros(1, 8))
    with pytest.raises(ValueError, match="out: a contiguous torch.int32 tensor of shape \\(n\\)"):
        r.traceDevice(rays, any_hit=True, out=torch.Tensor._make_subclass(_Elsewhere, torch.zeros(1, 8)))
    with pytest.raises(ValueError, match="out has 2 rows for 1 rays"):
        r.traceDevice(rays, out=torch.Tensor._make_subclass(_Elsewhere, torch.zeros(2, 8)))
    for name in ("traceDevice", "queryWait"):
        assert callable(getattr(R.SampleRenderer, name))


def test_facade_trace_device_compiles(tmp_path):
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t pick(SampleRenderer& sample, const float* d_rays, uint32_t n, pt_hit* d_hits, int32_t* d_occluded) {\n"
        "    const pt_query_stats a = sample.traceDevice(d_rays, n, d_hits);\n"
        "    sample.traceDevice(d_rays, n, d_occluded, /*any_hit=*/true, /*wait=*/false);\n"
        "    sample.traceDevice(d_rays, n / 2, d_hits, false, false);\n"
        "    const pt_query_stats b = sample.queryWait();\n"
        "    static_assert(sizeof(pt_hit) == 32, \"one record per ray\");\n"
        "    return a.hits + b.hits + b.invalid_rays + b.state_bytes;\n"
        "}\n"
    )
