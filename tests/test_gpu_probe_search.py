"""ProbeSample's row and column search on the device, queried at chosen random numbers (pt_eval_table 9-11: probe_search_rows and
probe_search_column of pt_device.h, the functions k_shade calls) against the reference's LowerBound (Probe.cuh:119-136) at every edge of
the tables: each CDF entry, each guide-cell edge k / gk, and their float32 neighbours on both sides (probe_search_ref).  Table 9 reads the
marginal arrays in global memory, 10 and 11 the copy a shade workgroup holds in LDS (shade_marg_fill: full and lean layout), so the three
table kernels k_probe_coarse / k_probe_lines / k_probe_guide, both searches and both LDS layouts are compared index for index and texel
for texel.  Every context answers all its queries once; the tests share the answers and leave them unchanged.

Queries per case (row queries + column queries), 178 906 in all:
  sky_13x64 195 + 5520, spots_130x192 476 + 9501, spots_4099x8 24 + 90284, constant_8x64 194 + 4656, constant_5x4 14 + 824,
  spots_7x2048 4692 + 4767, spots_6x2112 4625 + 4725, spots_12x512 987 + 4710, disc_100x50 153 + 11736, black_row0_13x64 168 + 4869,
  dyadic_200x64 98 + 9264, dyadic_65x128 98 + 4656, dyadic_200x64_short 102 + 11568."""
import numpy as np
import pytest

import probe_search_ref as PS
from optixpathtracer_amd import scenes

pytestmark = pytest.mark.gpu

IDS = {9: "global marginals", 10: "LDS copy, full layout", 11: "LDS copy, lean layout"}
_RUNS = {}  # (case, workgroup size or None) -> {9, 10, 11: the table's answers, "stats": pt_stats}


def _run(monkeypatch, name, wg=None):
    if (name, wg) not in _RUNS:
        from optixpathtracer_amd.renderer import SampleRenderer

        monkeypatch.delenv("PT_SHADE_WG", raising=False)
        if wg is not None:
            monkeypatch.setenv("PT_SHADE_WG", str(wg))
        r = SampleRenderer(scenes.cornell_box())  # the switch is read once, at pt_create
        monkeypatch.delenv("PT_SHADE_WG", raising=False)
        c = PS.case(name)
        r.setProbe(c["probe"])
        out = {which: r.evalTable(which, c["q"], 9) for which in IDS}
        out["stats"] = r.stats()
        r.close()
        for which in IDS:
            out[which].setflags(write=False)
        _RUNS[(name, wg)] = out
    return _RUNS[(name, wg)]


def _check(name, got, what):
    c = PS.case(name)
    p, q = c["probe"], c["q"]
    row, lo, hi, col = (got[:, k].view(np.int32).astype(np.int64) for k in range(4))
    bad = np.flatnonzero(row != c["row"])
    assert not len(bad), f"{what}: {len(bad)} rows differ, first r1 = {q[bad[0], 0]!r}: row {row[bad[0]]}, LowerBound {c['row'][bad[0]]}"
    bad = np.flatnonzero(col != c["col"])
    assert not len(bad), (f"{what}: {len(bad)} columns differ, first (r1, r2) = {q[bad[0]].tolist()!r} in row {row[bad[0]]}: column {col[bad[0]]}, "
                          f"LowerBound {c['col'][bad[0]]}, guide counts {lo[bad[0]]} {hi[bad[0]]}")
    lpr = (p.width + PS.LINE_COLS - 1) // PS.LINE_COLS
    line = col // PS.LINE_COLS
    assert (lo >= 0).all() and (lo <= hi).all() and (hi <= lpr).all(), f"{what}: guide counts out of order or past the row's {lpr} lines"
    assert (np.minimum(lo, lpr - 1) <= line).all() and (line <= np.minimum(hi, lpr - 1)).all(), f"{what}: a column outside its guide cell's lines"
    data = np.asarray(p.data, np.float32).reshape(p.height, p.width, 4)
    pdfx = np.asarray(p.pdfValuesX, np.float32).reshape(p.height, p.width)
    want = np.concatenate([data[row, col, :3], pdfx[row, col][:, None], np.asarray(p.pdfValuesY, np.float32)[row][:, None]], 1)
    neq = np.ascontiguousarray(got[:, 4:]).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    assert not neq.any(), f"{what}: texel / pdfX / pdfY words differ in {int(neq.sum())} places, first at query {np.argwhere(neq)[0].tolist()}"


@pytest.mark.parametrize("which", list(IDS))
@pytest.mark.parametrize("name", list(PS.CASES))
def test_search_equals_lower_bound_at_every_edge(ptlib, monkeypatch, name, which):
    run = _run(monkeypatch, name)
    _check(name, run[which], f"{name}, table {which} ({IDS[which]})")
    if which != 9:  # the LDS copy changes where the arrays are read, never what is read
        assert np.array_equal(run[which].view(np.uint32), run[9].view(np.uint32)), f"{name}: table {which} differs from table 9"


@pytest.mark.parametrize("wg", [64, 256])
@pytest.mark.parametrize("name", PS.WG_CASES)
def test_lds_copy_filled_by_the_other_workgroup_sizes(ptlib, monkeypatch, name, wg):
    """shade_marg_fill<WG> strides the copy by the workgroup size: one block, the largest copy, and the first size that has none"""
    run = _run(monkeypatch, name, wg)
    for which in (10, 11):
        _check(name, run[which], f"{name}, PT_SHADE_WG={wg}, table {which} ({IDS[which]})")
        assert np.array_equal(run[which].view(np.uint32), _run(monkeypatch, name)[9].view(np.uint32)), f"{name}, PT_SHADE_WG={wg}: table {which} differs from table 9"


def test_cases_reach_every_branch_of_both_searches(ptlib, monkeypatch):
    """Measured with the guide counts the kernel returned: halving loop 543, second candidate line 5650, third 124, column clamp 2304,
    row clamp 3 (lower_bound_blocked's exit past the last block), all-NaN row 195 (black_row0_13x64: r1 = 0)."""
    total = dict.fromkeys(PS.BRANCHES, 0)
    for name in PS.CASES:
        c = PS.case(name)
        got = _run(monkeypatch, name)[9]
        lo, hi = got[:, 1].view(np.int32), got[:, 2].view(np.int32)
        counts = PS.branch_counts(c["probe"], c["q"], c["lby"], c["lbx"], lo, hi)
        print(name, len(c["q"]), "queries,", c["nrow"], "of them row queries:", counts)
        for k, v in counts.items():
            total[k] += v
    print("all cases:", total)
    assert all(total.values()), total
    words = {n: (_run(monkeypatch, n)["stats"]["marg_lds_words_full"], _run(monkeypatch, n)["stats"]["marg_lds_words_lean"])
             for n in ("spots_7x2048", "spots_6x2112", "disc_100x50")}
    assert words["spots_7x2048"][0] > 0 and words["spots_7x2048"][1] > 0, words  # 2048 rows: the largest copy, in both layouts
    assert words["spots_6x2112"] == (0, 0) and words["disc_100x50"] == (0, 0), words  # 2112 rows / no count tables: tables 10 and 11 read global memory


def test_search_tables_refuse_what_they_cannot_index(ptlib):
    from optixpathtracer_amd.renderer import SampleRenderer

    r = SampleRenderer(scenes.cornell_box())
    for which in IDS:
        with pytest.raises(Exception, match="no probe set"):
            r.evalTable(which, np.float32([[0.5, 0.5]]), 9)
    r.setProbe(PS.case("constant_5x4")["probe"])
    for which in IDS:
        for bad in ([1.0, 0.5], [0.5, 1.0], [-0.25, 0.5], [0.5, np.nan]):
            with pytest.raises(Exception, match=r"must be in \[0,1\)"):
                r.evalTable(which, np.float32([[0.5, 0.5], bad]), 9)
    r.close()
