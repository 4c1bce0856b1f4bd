"""The overlap routine of the image-space passes (csrc/pt_pass.h, the part that needs no HIP header) without a GPU: a stand-alone host
program, compiled with g++ alone, runs pass_planes_overlap over small plane tables and prints the first offending pair of each."""
import os
import subprocess

from conftest import ROOT

# (what, eq_a, eq_b, rows of (name, address, bytes, required, exclusive)) -> the first offending pair in table order, or None
CASES = [
    ("two planes that touch end to start", -1, -1, [("a", 0x1000, 0x100, 1, 1), ("b", 0x1100, 0x100, 1, 1)], None),
    ("the same two, the later one first in memory", -1, -1, [("a", 0x1100, 0x100, 1, 1), ("b", 0x1000, 0x100, 1, 1)], None),
    ("one byte of overlap", -1, -1, [("a", 0x1000, 0x101, 1, 1), ("b", 0x1100, 0x100, 1, 1)], ("a", "b")),
    ("one byte of overlap, names in table order whatever the addresses", -1, -1, [("hi", 0x1100, 0x100, 1, 1), ("lo", 0x1000, 0x101, 1, 1)], ("hi", "lo")),
    ("the first offending pair of several", -1, -1,
     [("r", 0x5000, 0x10, 1, 0), ("a", 0x1000, 0x100, 1, 1), ("b", 0x2000, 0x100, 1, 1), ("c", 0x10ff, 0x10, 1, 1), ("d", 0x2000, 0x100, 1, 1)], ("a", "c")),
    ("a null plane", -1, -1, [("a", 0, 0x100, 0, 1), ("b", 0x10, 0x100, 1, 1), ("c", 0, 0x100, 0, 1)], None),
    ("two non-exclusive planes alias fully", -1, -1, [("a", 0x1000, 0x100, 1, 0), ("b", 0x1000, 0x100, 1, 0), ("w", 0x3000, 0x100, 1, 1)], None),
    ("an exclusive plane against a non-exclusive one", -1, -1, [("r", 0x1000, 0x100, 1, 0), ("w", 0x1080, 0x100, 0, 1)], ("r", "w")),
    ("a non-exclusive plane behind the exclusive one it overlaps", -1, -1, [("w", 0x1080, 0x100, 0, 1), ("r", 0x1000, 0x100, 1, 0)], ("w", "r")),
    ("the permitted-equal pair, exactly equal", 0, 2, [("color", 0x1000, 0x100, 1, 0), ("albedo", 0x4000, 0x100, 0, 0), ("out", 0x1000, 0x100, 0, 1)], None),
    ("the permitted-equal pair, offset by 4 bytes", 0, 2, [("color", 0x1000, 0x100, 1, 0), ("albedo", 0x4000, 0x100, 0, 0), ("out", 0x1004, 0x100, 0, 1)],
     ("color", "out")),
    ("equal planes that are not the permitted pair", 0, 2, [("color", 0x1000, 0x100, 1, 0), ("out", 0x1000, 0x100, 0, 1), ("frame", 0x8000, 0x40, 0, 1)],
     ("color", "out")),
    ("a zero-byte plane inside another", -1, -1, [("a", 0x1000, 0x100, 1, 1), ("z", 0x1080, 0, 1, 1), ("y", 0x1000, 0, 1, 1)], None),
]


def test_overlap_routine_on_the_host(tmp_path):
    body = ['#include <cstdio>', '#include "pt_pass.h"', "int main() {", "    int i, j;"]
    for k, (_, eq_a, eq_b, rows, _) in enumerate(CASES):
        table = ", ".join(f'{{"{n}", reinterpret_cast<const void*>((uintptr_t){p:#x}), {b:#x}, {bool(r):d} != 0, {bool(x):d} != 0}}' for n, p, b, r, x in rows)
        body += [f"    const PassPlane t{k}[] = {{{table}}};",
                 f'    if (pass_planes_overlap(t{k}, {len(rows)}, &i, &j, {eq_a}, {eq_b})) printf("%s %s\\n", t{k}[i].name, t{k}[j].name); else printf("none\\n");']
    # the default arguments: no pair is permitted to be equal
    body += ['    const PassPlane d[] = {{"a", reinterpret_cast<const void*>((uintptr_t)0x40), 8, true, false}, {"b", reinterpret_cast<const void*>((uintptr_t)0x40), 8, true, true}};',
             '    printf("%d\\n", pass_planes_overlap(d, 2, &i, &j) && i == 0 && j == 1);', "    return 0;", "}"]
    src = tmp_path / "planes.cpp"
    src.write_text("\n".join(body) + "\n")
    exe = tmp_path / "planes"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "optixpathtracer_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    for (what, _, _, _, want), line in zip(CASES, got):
        assert line == ("none" if want is None else " ".join(want)), (what, line)
    assert got[len(CASES)] == "1" and got[len(CASES) + 1:] == [""]
