"""The overlap routine and the tile table of the image-space passes (csrc/pt_pass.h, the part that needs no HIP header) without a GPU:
stand-alone host programs, compiled with g++ alone, run pass_planes_overlap over small plane tables and print the first offending pair of
each, and pass_tile_table over small sets of rectangles and print every view's entry."""
import os
import subprocess

import tile_ref
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


# (frame (h, w), the views' rectangles (x0, y0, wr, hr) or None): one tile, a full tile, a partial column, partial tiles both ways, and two
# views of odd sizes of which one lies off the origin
TILE_CASES = [((1, 1), None), ((16, 16), None), ((16, 17), None), ((49, 33), None), ((64, 64), [(0, 0, 33, 49), (40, 3, 15, 17)])]


def test_tile_table_on_the_host(tmp_path):
    """pass_tile_table, the view table of the tiled passes (motion blur, depth of field), against tests/tile_ref.py's layout: the tile
    grid, where T and N of every view start, the texel total, and the origin packed as x | y << 16; aux is left 0."""
    body = ['#include <cstdio>', '#include <cstring>', '#include "pt_pass.h"', "int main() {",
            '    static_assert(sizeof(TileView) == 32, "the device reads eight words per view");']
    for k, ((h, w), rects) in enumerate(TILE_CASES):
        rs = tile_ref.rectangles(rects, h, w)
        body += [f"    const PassRect r{k}[] = {{{', '.join(f'{{{x}u, {y}u, {wr}u, {hr}u}}' for x, y, wr, hr in rs)}}};",
                 f"    TileView t{k}[{len(rs)}];",
                 f"    memset(t{k}, 0xff, sizeof(t{k}));",
                 f'    printf("%llu\\n", (unsigned long long)pass_tile_table(r{k}, {len(rs)}, PASS_TILE, t{k}));',
                 f'    for (const TileView& t : t{k}) printf("%u %u %u %u %u %u %u %d\\n", t.tw, t.th, t.offT, t.offN, t.org, t.w, t.h, t.aux == 0.0f);']
    body += ["    return 0;", "}"]
    src = tmp_path / "tiles.cpp"
    src.write_text("\n".join(body) + "\n")
    exe = tmp_path / "tiles"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "optixpathtracer_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    want = []
    for (h, w), rects in TILE_CASES:
        dims, nbytes = tile_ref.layout(rects, h, w, 1)  # one byte a texel: the texel total
        want.append(str(nbytes))
        for (x, y, wr, hr), (tw, th, at_t, at_n) in zip(tile_ref.rectangles(rects, h, w), dims.tolist()):
            assert (tw, th) == (-(-wr // tile_ref.TILE), -(-hr // tile_ref.TILE)) and at_n == at_t + tw * th
            want.append(f"{tw} {th} {at_t} {at_n} {x | y << 16} {wr} {hr} 1")
    assert got == want + [""]
    assert want[:2] == ["2", "1 1 0 1 0 1 1 1"] and want[-1] == f"1 2 24 26 {40 | 3 << 16} 15 17 1"  # the reference itself, at both ends
