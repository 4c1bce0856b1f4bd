"""float32 NumPy evaluation of pt_sample_plan's and pt_temporal_carry's arithmetic (include/pt_amd.h), shared by tests/test_plan_cabi.py and
tests/test_gpu_plan.py.  A helper, not a test.  Written from the header: step G, the plan and the carry, one rounding per operation, in the
header's order.  It never calls the kernels under test and does not go through moments_ref.moments_ref (that the restated gather agrees with
the pinned one is a test, tests/test_plan_cabi.py, not a definition); canon, SENTINEL and the input builders are moments_ref's and
temporal_ref's."""
import numpy as np

import moments_ref as MR
import temporal_ref as T

f32 = np.float32
SENTINEL = T.SENTINEL
canon = MR.canon
INPUTS = ("motion", "hit", "position", "prev_hit", "prev_position", "history_in", "moments_in", "length_in")
OUTPUTS = ("history_out", "moments_out", "length_out", "variance_out")
WORDS = {"history_out": 4, "moments_out": 2, "length_out": 1, "variance_out": 1}
GATHER_DEFAULTS = dict(normal_cos=0.9, plane_eps=0.01, min_weight=0.25)
PLAN_DEFAULTS = dict(GATHER_DEFAULTS, threshold=0.05, dark_floor=0.01, min_length=4, min_pixels=4, refresh_period=0, frame_index=0)
PLAN_STATS = ("blocks", "sampled", "by_lost", "by_need", "by_refresh", "pixels", "lost", "needy")
CARRY_STATS = ("pixels", "carried", "lost")


def _f(a):
    a = np.ascontiguousarray(a)
    return a.view(f32) if a.dtype == np.uint32 else np.ascontiguousarray(a, f32)


def _finite(a):
    return (np.ascontiguousarray(a, f32).view(np.uint32) & 0x7F800000) != 0x7F800000  # the exponent-bit test


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _max0(v):
    return np.where(v > f32(0), v, f32(0)).astype(f32)  # sel_max0: a NaN gives 0


def block_set(pixels):
    """bool (nby, nbx): the blocks that hold at least one pixel of the set"""
    h, w = pixels.shape
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    pad = np.zeros((nby * 8, nbx * 8), bool)
    pad[:h, :w] = pixels
    return pad.reshape(nby, 8, nbx, 8).any((1, 3))


def pixel_mask(block_mask, h, w):
    """bool (h, w): the pixels of the blocks a mask names"""
    return np.repeat(np.repeat(np.asarray(block_mask) != 0, 8, 0), 8, 1)[:h, :w]


def gather(planes, rects, pixels, normal_cos=0.9, plane_eps=0.01, min_weight=0.25):
    """Step G for every pixel of the set.  planes: the eight INPUTS, float32 or their uint32 bits; rects: [(x0, y0, wr, hr)], the views, or
    [(0, 0, w, h)] without views; pixels: bool (h, w), each inside exactly one rectangle.  Returns {Y, X: the set's pixels in row-major
    order; valid: bool (n,); Wsum, nprev: float32 (n,); Hsum: (n, 3); Msum: (n, 2); H, M: Hsum / Wsum and Msum / Wsum (meaningful where
    valid)}."""
    P = {k: _f(planes[k]) for k in INPUTS}
    pixels = np.asarray(pixels, bool)
    Y, X = np.nonzero(pixels)
    n = len(Y)
    rid = np.full(n, -1)
    for k, (rx, ry, rw, rh) in enumerate(rects):
        inside = (X >= rx) & (X < rx + rw) & (Y >= ry) & (Y < ry + rh)
        assert (rid[inside] == -1).all()
        rid[inside] = k
    assert (rid >= 0).all(), "a pixel of the set lies in no rectangle"
    R = np.asarray(rects, np.int64).reshape(-1, 4)[rid]
    x0, y0, wr, hr = R[:, 0], R[:, 1], R[:, 2], R[:, 3]
    x, y = X - x0, Y - y0
    hitw = P["hit"][Y, X].view(np.int32)
    prim_p, mesh_p = hitw[:, 3], hitw[:, 4]
    t_p, ng_p = P["hit"][Y, X, 0], P["hit"][Y, X, 5:8]
    pos_p = P["position"][Y, X, 0:3]
    with np.errstate(all="ignore"):
        # ---- G1
        mv = P["motion"][Y, X]
        px, py = x.astype(f32) + mv[:, 0], y.astype(f32) + mv[:, 1]
        ok = (px >= f32(-1)) & (px <= wr.astype(f32)) & (py >= f32(-1)) & (py <= hr.astype(f32))
        pxs, pys = np.where(ok, px, f32(0)), np.where(ok, py, f32(0))
        flx, fly = np.floor(pxs), np.floor(pys)
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        fx, fy = pxs - flx, pys - fly
        wx, wy = [f32(1) - fx, fx], [f32(1) - fy, fy]
        plane_max = f32(plane_eps) * t_p
        # ---- G2
        wt, ht, mt, cnt = [], [], [], []
        nprev = np.full(n, np.inf, f32)
        for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
            wij = wx[i] * wy[j]
            tx, ty = ix + i, iy + j
            live = ok & (tx >= 0) & (tx < wr) & (ty >= 0) & (ty < hr) & (wij > 0)
            qx, qy = np.where(live, x0 + tx, 0), np.where(live, y0 + ty, 0)
            ln = P["length_in"][qy, qx]
            live &= ln >= f32(1)
            hq = P["history_in"][qy, qx, 0:3]
            mq = P["moments_in"][qy, qx, 0:2]
            live &= _finite(hq).all(-1) & _finite(mq).all(-1)
            qw = P["prev_hit"][qy, qx].view(np.int32)
            geo = (qw[:, 4] == mesh_p) & (_dot3(ng_p, P["prev_hit"][qy, qx, 5:8]) >= f32(normal_cos))
            geo &= np.abs(_dot3(ng_p, P["prev_position"][qy, qx, 0:3] - pos_p)) <= plane_max
            live &= np.where(prim_p < 0, qw[:, 3] < 0, geo)
            wt.append(np.where(live, wij, f32(0)))
            ht.append(np.where(live[:, None], wij[:, None] * hq, f32(0)))
            mt.append(np.where(live[:, None], wij[:, None] * mq, f32(0)))
            nprev = np.where(live, np.minimum(nprev, ln), nprev)
            cnt.append(live)
        # ---- G3
        wsum = ((wt[0] + wt[1]) + wt[2]) + wt[3]
        hsum = ((ht[0] + ht[1]) + ht[2]) + ht[3]
        msum = ((mt[0] + mt[1]) + mt[2]) + mt[3]
        valid = (cnt[0] | cnt[1] | cnt[2] | cnt[3]) & (wsum >= f32(min_weight))
        H = hsum / wsum[:, None]
        M = msum / wsum[:, None]
    for arr in (wsum, hsum, msum, H, M, nprev):
        assert arr.dtype == f32
    return dict(Y=Y, X=X, valid=valid, Wsum=wsum, Hsum=hsum, Msum=msum, nprev=nprev, H=H, M=M)


def refresh(bx, by, frame_index, period):
    """the header's formula on Python integers (no width to overflow)"""
    return period > 0 and (int(bx) + 3 * int(by) + int(frame_index)) % int(period) == 0


def plan_ref(planes, rects, pixels, **params):
    """pt_sample_plan.  pixels: the call's pixel set (owned, in a view, in a block of the input mask).  Returns {mask: uint8 (nby, nbx);
    stats: {PLAN_STATS}; valid, lost, needy: bool (h, w); L, S: int (nby, nbx); by_lost, by_need, by_refresh, quiet: bool (nby, nbx), the
    four outcomes of a block of the set}."""
    prm = dict(PLAN_DEFAULTS, **params)
    pixels = np.asarray(pixels, bool)
    h, w = pixels.shape
    g = gather(planes, rects, pixels, prm["normal_cos"], prm["plane_eps"], prm["min_weight"])
    valid, nprev, M = g["valid"], g["nprev"], g["M"]
    with np.errstate(all="ignore"):
        lost = ~valid
        short = valid & (nprev < f32(prm["min_length"]))
        var = _max0(M[:, 1] - M[:, 0] * M[:, 0])
        B = M[:, 0] + f32(prm["dark_floor"])
        rhs = (((f32(prm["threshold"]) * f32(prm["threshold"])) * nprev) * B) * B
        assert rhs.dtype == f32 and var.dtype == f32
        noisy = valid & ~short & ~(var <= rhs)
    needy = short | noisy
    Y, X = g["Y"], g["X"]
    inset = block_set(pixels)
    nby, nbx = inset.shape
    L, S = np.zeros((nby, nbx), np.int64), np.zeros((nby, nbx), np.int64)
    np.add.at(L, (Y >> 3, X >> 3), lost)
    np.add.at(S, (Y >> 3, X >> 3), needy)
    ref = np.array([[refresh(bx, by, prm["frame_index"], prm["refresh_period"]) for bx in range(nbx)] for by in range(nby)], bool).reshape(nby, nbx)
    by_lost = inset & (L >= 1)
    by_need = inset & ~by_lost & (S >= prm["min_pixels"])
    by_refresh = inset & ~by_lost & ~by_need & ref
    sampled = by_lost | by_need | by_refresh
    full = {}
    for name, arr in (("valid", valid), ("lost", lost), ("needy", needy)):
        full[name] = np.zeros((h, w), bool)
        full[name][Y, X] = arr
    stats = dict(blocks=int(inset.sum()), sampled=int(sampled.sum()), by_lost=int(by_lost.sum()), by_need=int(by_need.sum()),
                 by_refresh=int(by_refresh.sum()), pixels=len(Y), lost=int(lost.sum()), needy=int(needy.sum()))
    return dict(full, mask=sampled.astype(np.uint8), stats=stats, L=L, S=S, by_lost=by_lost, by_need=by_need, by_refresh=by_refresh,
                quiet=inset & ~sampled)


def carry_ref(planes, rects, pixels, fill=SENTINEL, **params):
    """pt_temporal_carry.  Returns {history_out, moments_out, length_out, variance_out: uint32 bits of the whole plane, `fill` outside the
    set; stats: {CARRY_STATS}; valid: bool (h, w)}."""
    prm = dict(GATHER_DEFAULTS, **params)
    pixels = np.asarray(pixels, bool)
    h, w = pixels.shape
    g = gather(planes, rects, pixels, prm["normal_cos"], prm["plane_eps"], prm["min_weight"])
    Y, X, valid, H, M = g["Y"], g["X"], g["valid"], g["H"], g["M"]
    n = len(Y)
    with np.errstate(all="ignore"):
        var = _max0(M[:, 1] - M[:, 0] * M[:, 0])
    hist = np.where(valid[:, None], H, f32(np.nan)).astype(f32)
    mom = np.where(valid[:, None], M, f32(0)).astype(f32)
    ln = np.where(valid, g["nprev"], f32(0)).astype(f32)
    var = np.where(valid, var, f32(0)).astype(f32)
    res = {}
    res["history_out"] = np.full((h, w, 4), fill, np.uint32)
    res["history_out"][Y, X] = np.concatenate([hist, np.ones((n, 1), f32)], 1).view(np.uint32)
    res["moments_out"] = np.full((h, w, 2), fill, np.uint32)
    res["moments_out"][Y, X] = mom.view(np.uint32)
    res["length_out"] = np.full((h, w), fill, np.uint32)
    res["length_out"][Y, X] = ln.view(np.uint32)
    res["variance_out"] = np.full((h, w), fill, np.uint32)
    res["variance_out"][Y, X] = var.view(np.uint32)
    res["stats"] = dict(pixels=n, carried=int(valid.sum()), lost=int((~valid).sum()))
    res["valid"] = np.zeros((h, w), bool)
    res["valid"][Y, X] = valid
    return res


# ------------------------------------------------------------------ inputs
W, H = 131, 61
CRAFTED = dict(threshold=0.1, dark_floor=0.0, min_length=4, min_pixels=7, refresh_period=4, frame_index=1)


def crafted_planes(w=W, h=H, seed=21):
    """One flat surface, zero motion, prev == cur: every lookup is one tap of weight 1, so a pixel's class is what its own history says.
    A quiet pixel has length 16 and moments (0.5, 0.2525): var = 0.0025 <= rhs = ((0.1 * 0.1 * 16) * 0.5) * 0.5 = 0.04 under CRAFTED.
    Block (bx, by) belongs to class (bx + 2 * by) % 4:
      0  one pixel lost — its length_in 0, a NaN history word or an inf moment, in turn over the class's blocks — the rest quiet;
      1  needy pixels: block k of the class has 1 + k % 12 of them (1..12: below, at and above min_pixels = 7; min_pixels = 1 takes them
         all, 64 none), alternately short (length 2 < min_length = 4) and noisy (moments (0.5, 0.5): var = 0.25 > 0.04);
      2, 3  quiet.
    With refresh_period = 4 the refresh names a quarter of the blocks, among them quiet ones: "by_refresh only"."""
    rng = np.random.default_rng(seed)
    hit = np.zeros((h, w, 8), f32)
    hit[..., 0], hit[..., 7] = 4, 1
    pos = np.zeros((h, w, 4), f32)
    pos[..., 3] = 1
    hist = rng.random((h, w, 4), dtype=f32)
    hist[..., 3] = 1
    ln = np.full((h, w), 16, f32)
    mom = np.zeros((h, w, 2), f32)
    mom[..., 0], mom[..., 1] = 0.5, f32(0.25) + f32(0.0025)
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    k0 = k1 = 0
    for by in range(nby):
        for bx in range(nbx):
            cls = (bx + 2 * by) % 4
            ys, xs = np.mgrid[8 * by:min(8 * by + 8, h), 8 * bx:min(8 * bx + 8, w)]
            ys, xs = ys.reshape(-1), xs.reshape(-1)
            if cls == 0:
                j = int(rng.integers(0, len(ys)))
                if k0 % 3 == 0:
                    ln[ys[j], xs[j]] = 0
                elif k0 % 3 == 1:
                    hist[ys[j], xs[j], k0 % 3] = np.nan
                else:
                    mom[ys[j], xs[j], 1] = np.inf
                k0 += 1
            elif cls == 1:
                m = min(1 + k1 % 12, len(ys))
                for c, j in enumerate(rng.permutation(len(ys))[:m]):
                    if c % 2 == 0:
                        ln[ys[j], xs[j]] = 2
                    else:
                        mom[ys[j], xs[j]] = (0.5, 0.5)
                k1 += 1
    return dict(motion=np.zeros((h, w, 2), f32), hit=hit, position=pos, prev_hit=hit, prev_position=pos, history_in=hist, moments_in=mom,
                length_in=ln)


def crafted_coverage(ref, what):
    """each of the four outcomes holds at least 5 % of the blocks of the set; returns the four counts"""
    n = ref["stats"]["blocks"]
    counts = {k: int(ref[k].sum()) for k in ("by_lost", "by_need", "by_refresh", "quiet")}
    assert sum(counts.values()) == n
    for k, v in counts.items():
        assert v * 20 >= n, f"{what}: only {v} of {n} blocks are {k}"
    return counts


# the mild moves of the real-plane tests: renderGBuffer's planes of temporal_ref.real_inputs()'s scenes, the previous camera
# T.forward(cam, REAL_F, dx=REAL_DX) — chosen on the CPU-built planes (tests/test_plan_cabi.py asserts the coverage there).  The two-box
# scene runs with the default gather parameters (its plane_eps = 0 of tests/test_gpu_temporal.py would let geometry alone decide validity,
# which is what the mild move is there to avoid).  The terrain's triangles are smaller than a pixel at 131 x 61: with the default tests 80
# of its 136 blocks hold a geometrically lost pixel even for a camera that barely moves, so it runs with the tests loosened (any normal in
# the same half-space, five times the plane distance, a tenth of the weight) — the other ends of the parameters' ranges, and the two
# scenes together exercise both.
REAL_F, REAL_DX = 0.02, 0.05
REAL_PLAN = dict(threshold=0.3, dark_floor=0.05, min_length=3, min_pixels=12)
REAL_GATHER = {"two_box": dict(), "terrain": dict(normal_cos=0.0, plane_eps=0.05, min_weight=0.1)}
REAL_SEED = {"two_box": 11, "terrain": 12}


def real_case(name):
    """(model factory, size, current camera, previous camera, gather parameters, seed) with the mild move"""
    make, size, cam, _, _, _ = T.real_inputs()[name]
    return make, size, cam, T.forward(cam, REAL_F, dx=REAL_DX), REAL_GATHER[name], REAL_SEED[name]


def block_history(h, w, seed):
    """Random history_in (h, w, 4), moments_in (h, w, 2), length_in (h, w) whose holes come in blocks, as a plan meets them: every 8x8
    block has a base length 1..12 and its pixels base + 0..2 (so blocks differ in how many pixels are short); in one block in four, pixels
    have temporal_ref.random_history's holes — length 0 for about one in six, a NaN or an inf history word for one in fifty — and one
    moments word in a hundred there is an inf.  The moments elsewhere are moments_ref.random_moments (finite)."""
    rng = np.random.default_rng(seed)
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    up = lambda a: np.repeat(np.repeat(a, 8, 0), 8, 1)[:h, :w]  # noqa: E731
    hist = rng.random((h, w, 4), dtype=f32)
    hist[..., 3] = 1
    ln = (up(rng.integers(1, 13, (nby, nbx))) + rng.integers(0, 3, (h, w))).astype(f32)
    mom = MR.random_moments(rng, h, w)
    holes = up(rng.random((nby, nbx)) < 0.25)
    ln[holes & (rng.random((h, w)) < 0.17)] = 0
    bad = holes & (rng.random((h, w)) < 0.02)
    k = int(bad.sum())
    hist[bad, rng.integers(0, 3, k)] = np.where(np.arange(k) % 3 == 0, f32(np.inf), np.where(np.arange(k) % 3 == 1, f32(-np.inf), f32(np.nan)))
    badm = holes & (rng.random((h, w)) < 0.01)
    mom[badm, rng.integers(0, 2, int(badm.sum()))] = np.inf
    return hist, mom, ln


def with_block_history(planes, seed):
    """the eight INPUTS: a dict of G-buffer planes (motion, hit, position, prev_hit, prev_position) with block_history added"""
    h, w = planes["motion"].shape[:2]
    hist, mom, ln = block_history(h, w, seed)
    return {k: dict(planes, history_in=hist, moments_in=mom, length_in=ln)[k] for k in INPUTS}


def real_coverage(plan, carry, what):
    """at least 10 % of the blocks sampled and 10 % not; at least 10 % of the carried set valid.  Returns the counts."""
    st = plan["stats"]
    n, s = st["blocks"], st["sampled"]
    assert s * 10 >= n and (n - s) * 10 >= n, f"{what}: {s} of {n} blocks are sampled"
    cs = carry["stats"]
    assert cs["pixels"] > 0 and cs["carried"] * 10 >= cs["pixels"], f"{what}: {cs['carried']} of {cs['pixels']} carried pixels are valid"
    return n, s, cs["pixels"], cs["carried"]
