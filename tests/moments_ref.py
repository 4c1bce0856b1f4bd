"""float32 NumPy evaluation of pt_temporal_moments's and pt_modulate_planes's arithmetic (include/pt_amd.h), shared by
tests/test_moments_cabi.py and tests/test_gpu_moments.py.  A helper, not a test.  One rounding per operation, in the header's order; it never
calls the kernels under test and does not go through temporal_ref.temporal_ref (the reduction to the existing pass is a test, not a
definition).  make_color is the CPU checker's, through temporal_ref.make_color_bits."""
import numpy as np

import temporal_ref as T

f32 = np.float32
SENTINEL = T.SENTINEL
QNAN = 0x7FC00000
OUTPUTS = ("history_out", "moments_out", "length_out", "variance_out")
WORDS = {"history_out": 4, "moments_out": 2, "length_out": 1, "variance_out": 1}
DEFAULTS = dict(color_scale=1.0, albedo_min=0.0, normal_cos=0.9, plane_eps=0.01, min_weight=0.25, clamp_k=1.0, max_history=32, clamp=False,
                clear=False)


def canon(bits):
    """uint32 bits with every NaN replaced by one pattern: the header leaves a NaN's sign and payload open (a NaN is a NaN)"""
    bits = np.array(bits, np.uint32)
    bits[((bits & 0x7F800000) == 0x7F800000) & ((bits & 0x007FFFFF) != 0)] = QNAN
    return bits


def _f(a):
    a = np.ascontiguousarray(a)
    return a.view(f32) if a.dtype == np.uint32 else np.ascontiguousarray(a, f32)


def _finite(a):
    return (np.ascontiguousarray(a, f32).view(np.uint32) & 0x7F800000) != 0x7F800000


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def lum(c):
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def max0(v):
    return np.where(v > f32(0), v, f32(0)).astype(f32)  # a NaN gives 0: not fmaxf


def den(albedo, albedo_min, shape):
    """step 0's denominators, (h, w, 3): 1 without an albedo plane, else a > albedo_min ? a : 1"""
    if albedo is None:
        return np.ones(shape, f32)
    a = _f(albedo)[..., 0:3]
    with np.errstate(invalid="ignore"):
        return np.where(a > f32(albedo_min), a, f32(1)).astype(f32)


def demodulated(color, albedo, color_scale, albedo_min):
    """step 0: d(q) for every pixel of the frame, (h, w, 3)"""
    c = _f(color)[..., 0:3]
    with np.errstate(all="ignore"):
        d = (c * f32(color_scale)) / den(albedo, albedo_min, c.shape)
    assert d.dtype == f32
    return d


def moments_ref(planes, rects, pixels, blocks=None, fill=SENTINEL, **params):
    """planes: color (h, w, 4), albedo (h, w, 4) or None, motion (h, w, 2), hit (h, w, 8), position (h, w, 4), prev_hit, prev_position,
    history_in (h, w, 4), moments_in (h, w, 2), length_in (h, w) — float32 or their uint32 bits.  rects: [(x0, y0, wr, hr)], the views, or
    [(0, 0, w, h)] without views.  pixels: bool (h, w), the set the call processes (each inside exactly one rectangle); blocks: bool
    (nby, nbx), the call's block set (default: the blocks that hold a pixel of the set).  params: DEFAULTS; clamp and clear are the two flags.
    Returns {history_out, moments_out, length_out, variance_out, color: uint32 bits of the whole plane, `fill` (for color: the input)
    outside the set; reprojected, clamped: int; valid, clamped_px: bool (h, w); window: int (h, w), the counting window pixels;
    window_rejects: {rect, block, finite: int}, window pixels of valid pixels that did not count, by the first test they fail}."""
    prm = dict(DEFAULTS, **params)
    P = {k: (None if v is None else _f(v)) for k, v in planes.items()}
    h, w = P["length_in"].shape
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
    if blocks is None:
        nby, nbx = (h + 7) // 8, (w + 7) // 8
        pad = np.zeros((nby * 8, nbx * 8), bool)
        pad[:h, :w] = pixels
        blocks = pad.reshape(nby, 8, nbx, 8).any((1, 3))
    blocks = np.asarray(blocks, bool)
    # ---- 0, 1
    D = demodulated(P["color"], P.get("albedo"), prm["color_scale"], prm["albedo_min"])
    d = D[Y, X]
    with np.errstate(all="ignore"):
        l = lum(d)
        m = np.stack([l, l * l], -1)
    hitw = P["hit"][Y, X].view(np.int32)
    prim_p, mesh_p = hitw[:, 3], hitw[:, 4]
    t_p, ng_p = P["hit"][Y, X, 0], P["hit"][Y, X, 5:8]
    pos_p = P["position"][Y, X, 0:3]
    with np.errstate(all="ignore"):
        # ---- 2
        mv = P["motion"][Y, X]
        px, py = x.astype(f32) + mv[:, 0], y.astype(f32) + mv[:, 1]
        ok = (px >= f32(-1)) & (px <= wr.astype(f32)) & (py >= f32(-1)) & (py <= hr.astype(f32))
        pxs, pys = np.where(ok, px, f32(0)), np.where(ok, py, f32(0))
        flx, fly = np.floor(pxs), np.floor(pys)
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        fx, fy = pxs - flx, pys - fly
        wx, wy = [f32(1) - fx, fx], [f32(1) - fy, fy]
        plane_max = f32(prm["plane_eps"]) * t_p
        # ---- 3
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
            pmiss, qmiss = prim_p < 0, qw[:, 3] < 0
            geo = (_dot3(ng_p, P["prev_hit"][qy, qx, 5:8]) >= f32(prm["normal_cos"])) & (qw[:, 4] == mesh_p)
            geo &= np.abs(_dot3(ng_p, P["prev_position"][qy, qx, 0:3] - pos_p)) <= plane_max
            live &= np.where(pmiss, qmiss, geo)
            wt.append(np.where(live, wij, f32(0)))
            ht.append(np.where(live[:, None], wij[:, None] * hq, f32(0)))
            mt.append(np.where(live[:, None], wij[:, None] * mq, f32(0)))
            nprev = np.where(live, np.minimum(nprev, ln), nprev)
            cnt.append(live)
        # ---- 4
        wsum = ((wt[0] + wt[1]) + wt[2]) + wt[3]
        hsum = ((ht[0] + ht[1]) + ht[2]) + ht[3]
        msum = ((mt[0] + mt[1]) + mt[2]) + mt[3]
        anyc = cnt[0] | cnt[1] | cnt[2] | cnt[3]
        valid = anyc & (wsum >= f32(prm["min_weight"]))
        # ---- 5
        Hh = hsum / wsum[:, None]
        M = msum / wsum[:, None]
        nn = np.minimum(nprev, f32(prm["max_history"] - 1))
        a = f32(1) / (nn + f32(1))
        # ---- 5b
        clamped = np.zeros(n, bool)
        wcount = np.zeros(n, np.int64)
        rejects = dict(rect=0, block=0, finite=0)
        if prm["clamp"]:
            k_ = f32(prm["clamp_k"])
            c_ = np.zeros(n, f32)
            s1, s2 = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qx, qy = X + dx, Y + dy
                    inrect = (qx >= x0) & (qx < x0 + wr) & (qy >= y0) & (qy < y0 + hr)
                    qxs, qys = np.where(inrect, qx, 0), np.where(inrect, qy, 0)
                    inblock = blocks[qys >> 3, qxs >> 3]
                    dq = D[qys, qxs]
                    fin = _finite(dq).all(-1)
                    counts = inrect & inblock & fin
                    rejects["rect"] += int((valid & ~inrect).sum())
                    rejects["block"] += int((valid & inrect & ~inblock).sum())
                    rejects["finite"] += int((valid & inrect & inblock & ~fin).sum())
                    c_ = np.where(counts, c_ + f32(1), c_)
                    s1 = np.where(counts[:, None], s1 + dq, s1)
                    s2 = np.where(counts[:, None], s2 + dq * dq, s2)
            some = c_ >= f32(1)
            cs = np.where(some, c_, f32(1))[:, None]
            mu = s1 / cs
            sd = np.sqrt(max0(s2 / cs - mu * mu))
            lo, hi = mu - k_ * sd, mu + k_ * sd
            below, above = Hh < lo, Hh > hi
            Hc = np.where(below, lo, np.where(above, hi, Hh))
            use = valid & some
            clamped = use & (below | above).any(-1)
            Hh = np.where(use[:, None], Hc, Hh)
            wcount = np.where(valid, c_.astype(np.int64), 0)
            for arr in (mu, sd, lo, hi, Hc):
                assert arr.dtype == f32
        # ---- 5c
        out = np.where(valid[:, None], Hh + (d - Hh) * a[:, None], d).astype(f32)
        mo = np.where(valid[:, None], M + (m - M) * a[:, None], m).astype(f32)
        ln_out = np.where(valid, nn + f32(1), f32(1)).astype(f32)
        var = max0(mo[:, 1] - mo[:, 0] * mo[:, 0])
    for arr in (wsum, hsum, msum, Hh, M, a, d, m):
        assert arr.dtype == f32
    res = {}
    res["history_out"] = np.full((h, w, 4), fill, np.uint32)
    res["history_out"][Y, X] = np.concatenate([out, np.ones((n, 1), f32)], 1).view(np.uint32)
    res["moments_out"] = np.full((h, w, 2), fill, np.uint32)
    res["moments_out"][Y, X] = mo.view(np.uint32)
    res["length_out"] = np.full((h, w), fill, np.uint32)
    res["length_out"][Y, X] = ln_out.view(np.uint32)
    res["variance_out"] = np.full((h, w), fill, np.uint32)
    res["variance_out"][Y, X] = var.view(np.uint32)
    res["color"] = P["color"].view(np.uint32).copy()
    if prm["clear"]:
        res["color"][Y, X] = 0
    res["reprojected"] = int(valid.sum())
    res["clamped"] = int(clamped.sum())
    for name, arr, dt in (("valid", valid, bool), ("clamped_px", clamped, bool), ("window", wcount, np.int64)):
        res[name] = np.zeros((h, w), dt)
        res[name][Y, X] = arr
    res["window_rejects"] = rejects
    return res


def modulate_ref(orc, color, albedo, pixels, albedo_min=0.0, fill=SENTINEL):
    """pt_modulate_planes: {out: uint32 (h, w, 4), frame_rgba8: uint32 (h, w)} over the whole frame, `fill` outside the set"""
    c = _f(color)
    h, w = c.shape[:2]
    pixels = np.asarray(pixels, bool)
    Y, X = np.nonzero(pixels)
    with np.errstate(all="ignore"):
        r = (c[..., 0:3] * den(albedo, albedo_min, c[..., 0:3].shape))[Y, X]
    assert r.dtype == f32
    out = np.full((h, w, 4), fill, np.uint32)
    out[Y, X] = np.concatenate([r, c[Y, X, 3:4]], 1).view(np.uint32)
    frame = np.full((h, w), fill, np.uint32)
    frame[Y, X] = T.make_color_bits(orc, r)
    return dict(out=out, frame_rgba8=frame)


# ------------------------------------------------------------------ inputs
ALBEDO_MIN = 0.1


def random_moments(rng, h, w):
    """finite moments (m1, m2) of luminances in [0, 1): m2 >= m1^2 mostly, not always (the variance's sel_max0 is exercised)"""
    m1 = rng.random((h, w), dtype=f32)
    m2 = (m1 * m1 + (rng.random((h, w), dtype=f32) - f32(0.2)) * f32(0.1)).astype(f32)
    return np.stack([m1, m2], -1)


def random_albedo(rng, h, w, albedo_min=ALBEDO_MIN):
    """albedo in [0, 1) with one word in eight below albedo_min (some exactly 0, as a miss leaves them), w = 1"""
    a = (f32(albedo_min) + rng.random((h, w, 4), dtype=f32) * f32(1 - albedo_min)).astype(f32)
    low = rng.random((h, w, 4)) < 0.125
    a[low] = (rng.random(int(low.sum()), dtype=f32) * f32(albedo_min)).astype(f32)
    a[low & (rng.random((h, w, 4)) < 0.25)] = 0
    a[..., 3] = 1
    return a


def with_random_inputs(planes, seed, albedo=True):
    """adds color, history_in, length_in (temporal_ref.with_random_history: NaN and inf history words, length holes), finite moments_in and
    albedo to a dict of G-buffer planes; one colour word in about three hundred is a NaN or an inf (window pixels that do not count)"""
    planes = T.with_random_history(planes, seed)
    h, w = planes["motion"].shape[:2]
    rng = np.random.default_rng(seed + 1000)
    moments, alb = random_moments(rng, h, w), random_albedo(rng, h, w)
    color = planes["color"].copy()
    k = max(2, h * w // 100)
    ys, xs, cs = rng.integers(0, h, k), rng.integers(0, w, k), rng.integers(0, 3, k)
    color[ys, xs, cs] = np.where(np.arange(k) % 3 == 0, f32(np.inf), np.where(np.arange(k) % 3 == 1, f32(-np.inf), f32(np.nan)))
    return dict(planes, color=color, moments_in=moments, albedo=alb if albedo else None)


def real_params(name):
    """the parameters tests/test_gpu_moments.py runs the real inputs with"""
    return dict(T.real_inputs()[name][4], albedo_min=ALBEDO_MIN, clamp_k=1.0)


def check_coverage(planes, ref, pixels, what, albedo_min=ALBEDO_MIN):
    """at least 10 % of the set valid and 10 % invalid; at least 10 % of the valid pixels clamped and 10 % unclamped; both den branches
    taken by at least 5 % of the set's albedo words.  Returns the five counts."""
    pixels = np.asarray(pixels, bool)
    n = int(pixels.sum())
    valid, clamped = ref["reprojected"], ref["clamped"]
    a = _f(planes["albedo"])[..., 0:3][pixels]
    ones = int((~(a > f32(albedo_min))).sum())
    assert valid * 10 >= n and (n - valid) * 10 >= n, f"{what}: {valid} of {n} pixels are valid"
    assert clamped * 10 >= valid and (valid - clamped) * 10 >= valid, f"{what}: {clamped} of {valid} valid pixels are clamped"
    assert ones * 20 >= a.size and (a.size - ones) * 20 >= a.size, f"{what}: {ones} of {a.size} albedo words take den = 1"
    return n, valid, clamped, ones, a.size
