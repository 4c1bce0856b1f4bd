"""pt_below_horizon and pt_below_horizon_arc (include/pt_detmath.h) on the host: tests/horizon_host.cpp is compiled with the numerics contract's
flags and run.  It walks probes of 32, 128 and 1024 rows, every row and every column, against the axis directions, 30 / 60 degree tilts, 2000
seeded random unit normals and normals with components of +-0 or denormal size — and, against the same normals, the arcs of a row that a
guide cell can span from every first line, which is the predicate the kernel runs — and fails on the first skipped row or arc that has a column whose direction is not at or below the surface in the kernels' float
arithmetic.  The shares it reports are checked too, so that a margin that silently turns the skip off shows up."""
import json
import math
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_skipped_rows_and_arcs_have_no_column_above_the_surface(tmp_path):
    exe = tmp_path / "horizon_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread", "-o", str(exe), os.path.join(ROOT, "tests", "horizon_host.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr
    out = json.loads(p.stdout)
    assert out["violations"] == 0 and out["dots"] > 3 * 10**9
    assert out["max_skipped_dot"] <= 0.0
    # the margin's derivation takes sqrt(sp^2 + cp^2) <= 1 + 4e-7 for the columns' sine and cosine
    assert out["max_unit_excess"] <= 8e-7, out["max_unit_excess"]
    # Normal +y: every row with cos(row / h * pi) < -margin, i.e. all rows past the equator row h / 2 (whose cosine is -4e-8): h / 2 - 1.
    # Normal -y: the h / 2 rows before it.  The four horizontal axes: never (the bound is |sin| >= 0).
    assert out["axes"]["skipped"] == sum(h // 2 - 1 + h // 2 for h in (32, 128, 1024)), out["axes"]
    # A normal at angle a from the vertical (folded into [0, pi / 2]) loses the latitudes further than pi / 2 + a from it: a share of
    # (pi / 2 - a) / pi of the rows.  Uniform normals have E[a] = 1, so the mean share is (pi / 2 - 1) / pi = 0.1817; the standard error over
    # 2000 normals is 0.003 and the rows' granularity below that.
    share = out["random"]["skipped"] / out["random"]["pairs"]
    expect = (math.pi / 2 - 1) / math.pi
    assert abs(share - expect) < 0.012, (share, expect)
    # tilts of 30 and 60 degrees from +-y: (90 - 30) / 180 and (90 - 60) / 180 of the rows, one row of slack per probe height and normal
    tilts = out["tilts"]
    assert abs(tilts["skipped"] / tilts["pairs"] - 0.25) < 0.02, tilts
    assert out["zero_denormal"]["skipped"] > 0.25 * out["zero_denormal"]["pairs"], out["zero_denormal"]
    # Arcs: a plane through the origin has half of the sphere's (row, column) grid below it, whatever its normal; an arc of one to three
    # lines out of width / 6 is lost to the margin and its own width only next to the plane, and the few wide arcs (nine lines, half a row,
    # a whole row: under 1 % of the arcs) only where the circle itself is below.  So just under half of the arcs are skipped.
    for g in ("axes", "tilts", "random", "zero_denormal"):
        s = out[g]["arcs_skipped"] / out[g]["arcs"]
        assert 0.45 < s < 0.5, (g, s)
