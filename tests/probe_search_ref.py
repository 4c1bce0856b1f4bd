"""ProbeSample's two searches at the edges of their tables (pt_device.h: lower_bound_blocked for the row, the guide and the 128-byte lines
for the column), for tests/test_gpu_probe_search.py (the device code, pt_eval_table 9-11) and tests/test_oracle_properties.py (numpy models
of the two device structures).  The reference is the literal LowerBound loop (Probe.cuh:119-136), vectorised over the queries; the queries
are every value at which a `<` written as `<=`, a count rounded the other way or an offset off by one changes the answer: the CDF entries
and the guide-cell edges themselves and their float32 neighbours on both sides.  Needs no GPU; everything it hands out is read-only."""
import numpy as np

from optixpathtracer_amd import scenes

f32 = np.float32
LINE_COLS = 6  # PT_LINE_COLS
BLOCK = 64  # PT_CDF_BLOCK
BRANCHES = ("halving", "second_line", "third_line", "column_clamp", "row_clamp", "nan_row")


def lower_bound(a, v, rows=None, le=False):
    """LowerBound(a, 0, n, v) for every v: the reference's loop, one numpy step per halving.  a is (n,), or (h, n) with rows = the row of
    each query.  NaN entries compare false, as in the loop.  le: the loop with `<` written as `<=` (for the tests of the tests)."""
    v = np.asarray(v, f32)
    n = a.shape[-1]
    lo, hi = np.zeros(len(v), np.int64), np.full(len(v), n, np.int64)
    with np.errstate(invalid="ignore"):
        while (lo < hi).any():
            act = lo < hi
            mid = lo + (hi - lo) // 2
            at = np.minimum(mid, n - 1)
            am = a[at] if rows is None else a[rows, at]
            less = (am <= v) if le else (am < v)
            lo = np.where(act & less, mid + 1, lo)
            hi = np.where(act & ~less, mid, hi)
    return lo


def guide_size(w):
    """finish_probe's number of guide cells per row"""
    gk = 64
    while gk < 4096 and gk * 2 < w:
        gk *= 2
    return gk


def value_set(a, gk=None):
    """the float32 values in [0, 1) at which a search of `a` can go wrong: every finite entry and its two neighbours, for a column search
    the guide-cell edges k / gk and theirs, and the ends of the random numbers' range"""
    a = np.asarray(a, f32)
    e = a[np.isfinite(a)]
    if gk is not None:
        e = np.concatenate([e, (np.arange(gk + 1) / gk).astype(f32)])
    special = f32([0.0, np.nextafter(f32(0), f32(1)), 2.0**-24, 1 - 2.0**-24, 1 - 2.0**-23, 0.5])
    v = np.concatenate([e, np.nextafter(e, f32(0)), np.nextafter(e, f32(np.inf)), special]).astype(f32)
    return np.unique(v[(v >= 0) & (v < 1)])


def arrays(probe):
    h, w = probe.height, probe.width
    return np.asarray(probe.cdfValuesY, f32).reshape(h), np.asarray(probe.cdfValuesX, f32).reshape(h, w)


def expected(probe, q, le=False):
    """(row, column) ProbeSample (Probe.cuh:138-169) settles on for the random numbers q = (n, 2), and the two unclamped lower bounds"""
    cdfy, cdfx = arrays(probe)
    lby = lower_bound(cdfy, q[:, 0], le=le)
    row = np.minimum(lby, probe.height - 1)
    lbx = lower_bound(cdfx, q[:, 1], rows=row, le=le)
    return row, np.minimum(lbx, probe.width - 1), lby, lbx


def queries(probe):
    """(q, number of row queries): every r1 of the row value set with r2 = 0.5, then, for at most 24 of the rows those reach (the first,
    the middle and the last eight), one r1 that lands there with every r2 of that row's column value set"""
    cdfy, cdfx = arrays(probe)
    r1 = value_set(cdfy)
    rows = np.minimum(lower_bound(cdfy, r1), probe.height - 1)
    reached = np.unique(rows)
    m = len(reached) // 2
    chosen = np.unique(np.concatenate([reached[:8], reached[max(m - 4, 0):m + 4], reached[-8:]]))
    out = [np.stack([r1, np.full(len(r1), 0.5, f32)], 1)]
    gk = guide_size(probe.width)
    for row in chosen:
        r2 = value_set(cdfx[row], gk)
        out.append(np.stack([np.full(len(r2), r1[np.argmax(rows == row)], f32), r2], 1))
    return np.ascontiguousarray(np.concatenate(out), f32), len(r1)


# ------------------------------------------------------------------ the cases
def _hand_made(w, h, scale=1.0):
    """arrays set directly, as pt_set_probe takes them: dyadic CDFs with exact ties and flat runs (columns in 64ths, rows in 32nds); with
    scale < 1 the last entries lie below the largest random number, which only the clamps of row and column catch"""
    rng = np.random.default_rng(w * 1000 + h)
    p = scenes.ProbeData(w, h, rng.uniform(0.01, 4.0, (h, w, 4)).astype(f32))
    cx = (np.floor((np.arange(w) + 1) * 64 / w) / 64 * scale).astype(f32)
    p.cdfValuesX = np.ascontiguousarray(np.broadcast_to(cx, (h, w)))
    p.cdfValuesY = (np.floor((np.arange(h) + 1) * 32 / h) / 32 * scale).astype(f32)
    p.pdfValuesX = rng.uniform(0.0, 2.0, (h, w)).astype(f32)
    p.pdfValuesY = rng.uniform(0.0, 2.0, h).astype(f32)
    p.valid = True
    return p


def _black_first_row(w, h):
    """A black row's entry of cdfY equals the entry before it, so the lower bound never lands on it — unless it is row 0, where r1 = 0
    does: the one way into an all-NaN row of cdfX."""
    p = scenes.spots_probe(w, h, fill=0.3)
    p.data[0, :, :3] = 0.0
    return p.BuildCDF()


CASES = {
    "sky_13x64": lambda: scenes.sky_probe(13, 64).BuildCDF(),  # one block, c64Y = 1 entry + 7 of padding; 3 lines, the last partly +inf
    "spots_130x192": lambda: scenes.spots_probe(130, 192, fill=0.02).BuildCDF(),  # 3 blocks; gk = 128; NaN rows, plateaus in cdfY
    "spots_4099x8": lambda: scenes.spots_probe(4099, 8, fill=0.002).BuildCDF(),  # no row tables; gk = 4096; flat stretches: the halving loop
    "constant_8x64": lambda: scenes.constant_probe(8, 64).BuildCDF(),  # dyadic column CDF: entries tie with the guide edges
    "constant_5x4": lambda: scenes.constant_probe(5, 4).BuildCDF(),  # less than one line
    "spots_7x2048": lambda: scenes.spots_probe(7, 2048, fill=0.3).BuildCDF(),  # 32 blocks: the largest LDS copy
    "spots_6x2112": lambda: scenes.spots_probe(6, 2112, fill=0.3).BuildCDF(),  # 33 blocks: c64 binary search, marginals stay global
    "spots_12x512": lambda: scenes.spots_probe(12, 512, fill=0.1).BuildCDF(),  # 8 blocks: no padding
    "disc_100x50": lambda: scenes.disc_probe(100, 50).BuildCDF(),  # no row tables: the plain binary search
    "black_row0_13x64": lambda: _black_first_row(13, 64),  # r1 = 0 lands in an all-NaN row: every `<` is false, column 0
    "dyadic_200x64": lambda: _hand_made(200, 64),
    "dyadic_65x128": lambda: _hand_made(65, 128),
    "dyadic_200x64_short": lambda: _hand_made(200, 64, 0.75),  # the column clamp, and the row search's exit past the last block
}
WG_CASES = ("sky_13x64", "spots_7x2048", "spots_6x2112")  # run under the other two workgroup sizes as well
_CACHE = {}


def case(name):
    """{probe, q, nrow, row, col, lby, lbx} of a case, built once"""
    if name not in _CACHE:
        probe = CASES[name]()
        q, nrow = queries(probe)
        row, col, lby, lbx = expected(probe, q)
        for a in (q, row, col, lby, lbx, probe.data, probe.pdfValuesX, probe.cdfValuesX, probe.pdfValuesY, probe.cdfValuesY):
            a.setflags(write=False)
        _CACHE[name] = dict(probe=probe, q=q, nrow=nrow, row=row, col=col, lby=lby, lbx=lbx)
    return _CACHE[name]


# ------------------------------------------------------------------ numpy models of the device structures
def _count_lt8(a, base, v):
    with np.errstate(invalid="ignore"):
        return (a[base[:, None] + np.arange(8)] < v[:, None]).sum(1)


def row_tables(cdfy):
    """k_probe_coarse's two tables: the last entry of every 64-entry block, padded to a multiple of 8 with +inf, and of every 8-entry
    group; None where finish_probe builds none (the row count is no multiple of 64)"""
    h = len(cdfy)
    if h % BLOCK or h < BLOCK:
        return None
    ncy = h // BLOCK
    c64 = np.full((ncy + 7) & ~7, np.inf, f32)
    c64[:ncy] = cdfy[BLOCK - 1::BLOCK]
    return c64, cdfy[7::8].copy(), ncy


def row_model(cdfy, v, pad=np.inf):
    """probe_search_rows' unclamped row: lower_bound_blocked through the count tables, or the plain binary search where there are none.
    pad: what c64Y's padding holds (+inf on the device)."""
    v = np.asarray(v, f32)
    t = row_tables(cdfy)
    if t is None:
        return lower_bound(cdfy, v)
    c64, c8, ncy = t
    c64 = np.where(np.arange(len(c64)) < ncy, c64, f32(pad))
    if ncy <= 32:
        b = sum(_count_lt8(c64, np.full(len(v), k), v) for k in range(0, ncy, 8))
    else:
        b = lower_bound(c64[:ncy], v)
    out = np.full(len(v), len(cdfy), np.int64)
    ok = b < ncy
    bb, vv = b[ok], v[ok]
    g = _count_lt8(c8, bb * 8, vv)
    base = bb * BLOCK + np.minimum(g, 7) * 8
    out[ok] = base + _count_lt8(cdfy, base, vv)
    return out


def column_model(row, v, gk, guide_le=False):
    """probe_search_rows' guide lookup and probe_search_column for one row of cdfX: {col (unclamped), lo, hi (the guide's counts), line,
    halved, second, third}.  guide_le: k_probe_guide's `<` written as `<=`."""
    row, v = np.asarray(row, f32), np.asarray(v, f32)
    w = len(row)
    lpr = (w + LINE_COLS - 1) // LINE_COLS
    cdf = np.full(lpr * LINE_COLS, np.inf, f32)
    cdf[:w] = row
    last = cdf[LINE_COLS - 1::LINE_COLS]
    guide = lower_bound(last, (np.minimum(np.arange(gk + 2), gk) / gk).astype(f32), le=guide_le)  # k_probe_guide
    k = np.minimum((v * f32(gk)).astype(np.int64), gk - 1)
    glo, ghi = guide[k], guide[k + 1]
    lo, hi = np.minimum(glo, lpr - 1), np.minimum(ghi, lpr - 1)
    halved = hi - lo > 2
    with np.errstate(invalid="ignore"):
        while (hi - lo > 2).any():
            act = hi - lo > 2
            mid = lo + (hi - lo) // 2
            less = last[mid] < v
            lo = np.where(act & less, mid + 1, lo)
            hi = np.where(act & ~less, mid, hi)
        i1 = np.minimum(lo + 1, hi)
        second = (i1 > lo) & (last[lo] < v)
        third = second & (hi > i1) & (last[i1] < v)
        line = np.where(third, hi, np.where(second, i1, lo))
        col = line * LINE_COLS + (cdf[line[:, None] * LINE_COLS + np.arange(LINE_COLS)] < v[:, None]).sum(1)
    return dict(col=col, lo=glo, hi=ghi, line=line, halved=halved, second=second & ~third, third=third)


def model(probe, q, pad=np.inf, guide_le=False):
    """(row, col, lo, hi) of the two models for the random numbers q, clamped as the device clamps them"""
    cdfy, cdfx = arrays(probe)
    row = np.minimum(row_model(cdfy, q[:, 0], pad), probe.height - 1)
    col, lo, hi = (np.zeros(len(q), np.int64) for _ in range(3))
    gk = guide_size(probe.width)
    for r in np.unique(row):
        at = row == r
        m = column_model(cdfx[r], q[at, 1], gk, guide_le)
        col[at], lo[at], hi[at] = np.minimum(m["col"], probe.width - 1), m["lo"], m["hi"]
    return row, col, lo, hi


# ------------------------------------------------------------------ which branches a run reached
def branch_counts(probe, q, lby, lbx, lo, hi):
    """how often the queries q reach each branch of the two searches, from the reference's unclamped lower bounds (lby, lbx) and the guide
    counts (lo, hi) a run returned: the halving loop, the second and the third candidate line, the clamps of column and row, an all-NaN row"""
    _, cdfx = arrays(probe)
    h, w = probe.height, probe.width
    lpr = (w + LINE_COLS - 1) // LINE_COLS
    row = np.minimum(lby, h - 1)
    lo, hi = np.minimum(np.asarray(lo, np.int64), lpr - 1), np.minimum(np.asarray(hi, np.int64), lpr - 1)
    halving = hi - lo > 2
    last = np.full((h, lpr * LINE_COLS), np.inf, f32)
    last[:, :w] = cdfx
    last = last[:, LINE_COLS - 1::LINE_COLS]
    v = q[:, 1]
    with np.errstate(invalid="ignore"):
        while (hi - lo > 2).any():
            act = hi - lo > 2
            mid = lo + (hi - lo) // 2
            less = last[row, mid] < v
            lo = np.where(act & less, mid + 1, lo)
            hi = np.where(act & ~less, mid, hi)
    line = np.minimum(lbx // LINE_COLS, lpr - 1)  # the line of the reference's column, where the search has to end
    counts = dict(halving=halving, second_line=line == lo + 1, third_line=line == lo + 2, column_clamp=lbx >= w, row_clamp=lby >= h,
                  nan_row=np.isnan(cdfx).all(1)[row])
    return {k: int(np.count_nonzero(counts[k])) for k in BRANCHES}
