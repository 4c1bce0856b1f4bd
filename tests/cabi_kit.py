"""What every tests/test_<pass>_cabi.py needs and none of them owns: the text of include/pt_amd.h, the two compiler passes over it, the
sizeof / offsetof probe that holds the ctypes mirrors against the compiler, and the stand-ins the facade's argument checks are called on.
No torch at import and nothing that needs a GPU.  pytest does not rewrite the asserts of this module, so each carries its own message."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")


def header():
    """the text of include/pt_amd.h"""
    return open(os.path.join(INCLUDE, "pt_amd.h")).read()


def header_text():
    """the header with the comment stars taken out and every run of whitespace as one blank: what a test_header_states_* searches"""
    return " ".join(re.sub(r"^\s*\*", " ", header(), flags=re.M).split())


def header_section(begin, end):
    """header_text() between the first `begin` and the next `end`; a missing marker raises"""
    text = header_text()
    if begin not in text:
        raise ValueError(f"pt_amd.h has no {begin!r}")
    text = text.split(begin)[1]
    if end not in text:
        raise ValueError(f"pt_amd.h has no {end!r} after {begin!r}")
    return text.split(end)[0]


def compile_c99_and_cxx17(tmp_path, body):
    """`body` as a C99 and as a C++17 translation unit, both pedantic and warning-free; raises CalledProcessError"""
    (tmp_path / "h.c").write_text(body)
    (tmp_path / "h.cpp").write_text(body)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(tmp_path / "h.c")], check=True)
    subprocess.run(["g++", "-std=c++17", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(tmp_path / "h.cpp")], check=True)


def compile_facade(tmp_path, body):
    """`body` as C++17 against csrc/SampleRenderer.h (included by its path from the repository's root)"""
    src = tmp_path / "facade.cpp"
    src.write_text(body)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", ROOT, "-I", INCLUDE, str(src)], check=True)


def check_layout(tmp_path, structs, pinned):
    """structs: [(ctypes class, C type name, field names)].  The ctypes field order is the field names; sizeof and every offsetof, struct
    after struct, are the same numbers from ctypes, from gcc's probe program over pt_amd.h, and in `pinned`."""
    mine, args = [], []
    for cls, ctype, fields in structs:
        have = [n for n, _ in cls._fields_]
        assert have == list(fields), f"{ctype}: the ctypes mirror's fields are {have}, expected {list(fields)}"
        mine += [C.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
        args += [f"sizeof({ctype})"] + [f"offsetof({ctype}, {n})" for n in fields]
    assert mine == list(pinned), f"ctypes lays {[s[1] for s in structs]} out as {mine}, pinned {list(pinned)}"
    fmt = " ".join(["%zu"] * len(mine))
    src = tmp_path / "probe.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "pt_amd.h"\nint main(void) {{ printf("{fmt}\\n", {", ".join(args)}); return 0; }}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == mine, f"the compiler lays {[s[1] for s in structs]} out as {got}, ctypes as {mine}"


def fake_cuda(shape, dtype=None):
    """A CPU tensor that reports CUDA device 0: enough for the checks that run before the library is called."""
    import torch

    class Fake(torch.Tensor):
        @property
        def is_cuda(self):
            return True

        @property
        def device(self):
            return torch.device("cuda", 0)

    return torch.zeros(shape, dtype=dtype or torch.float32).as_subclass(Fake)


def bare_renderer(size=(4, 4), nv=(5, 3)):
    """a SampleRenderer without a context: what a facade method refuses on it, it refuses before the library is called"""
    from optixpathtracer_amd import renderer as R

    r = object.__new__(R.SampleRenderer)
    r._device, r.launchParams, r._nv = 0, R.LaunchParams(), list(nv)
    r.launchParams.frame.size = size
    return r
