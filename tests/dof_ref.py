"""NumPy evaluation of pt_dof_layout's and pt_dof_planes's rules, written from the text of include/pt_amd.h alone; shared by
tests/test_dof_cabi.py and tests/test_gpu_dof.py.  A helper, not a test; it never calls the kernels under test.  Everything is float32
arrays and float32 scalars, one rounding per operation, in the header's order (NumPy never contracts a product and a sum; its sqrt and its
division are correctly rounded).  Vectorised over the pixels of a rectangle; the only loops are over the taps and the tiles."""
import numpy as np

import tile_ref
from tile_ref import FLT_MAX, SENTINEL, TILE, clamp01, depth_z, finite, hash32, rectangles  # noqa: F401 (kept as this module's names)

f32 = np.float32
u32 = np.uint32
JITTER = 1
PI = f32(3.14159274)
C_BITS, S_BITS = 0xBF3CC435, 0x3F2CECEF
COUNTERS = ("pixels", "sources", "gathered", "taps", "nonfinite")
DEFAULTS = dict(max_radius=16.0, taps=32, seed=0, jitter=False)


def layout(rects, h, w):
    """(dims (nv, 4) uint32: tw, th, first 4-byte texel of T, first of N; bytes)"""
    return tile_ref.layout(rects, h, w, 4)


def directions():
    """D[0 .. 127]: (1, 0), then the header's recurrence — two products and one sum per component, each rounded to float32"""
    C, S = (np.array([b], u32).view(f32)[0] for b in (C_BITS, S_BITS))
    D = np.zeros((128, 2), f32)
    D[0] = (1.0, 0.0)
    for n in range(127):
        x, y = D[n]
        xc, ys, xs, yc = x * C, y * S, x * S, y * C
        assert all(v.dtype == f32 for v in (xc, ys, xs, yc))
        D[n + 1] = (xc - ys, xs + yc)
    return D


def jitter_of(x, y, seed):
    """k0 in 0 .. 63 of the local coordinates"""
    return (hash32(x, y, seed) & u32(63)).astype(np.int64)


def radius(depth, focus, aperture, max_radius):
    """step 1: r of raw depth words"""
    K = f32(aperture) + f32(0.0)
    R = f32(max_radius)
    with np.errstate(all="ignore"):
        r = K * np.abs(f32(1.0) - f32(focus) / depth_z(depth))
        r = np.where(r < R, r, R).astype(f32)
    assert r.dtype == f32
    return r


def area(r):
    with np.errstate(all="ignore"):
        a = (r * r) * PI
        return np.where(a > f32(1.0), a, f32(1.0)).astype(f32)


def tile_max(r):
    """step 2: (hr, wr) -> T (th, tw)"""
    hr, wr = r.shape
    tw, th = (wr + TILE - 1) // TILE, (hr + TILE - 1) // TILE
    T = np.zeros((th, tw), f32)
    for j in range(th):
        for i in range(tw):
            T[j, i] = r[TILE * j:TILE * j + TILE, TILE * i:TILE * i + TILE].max()
    return T


def neighbour_max(T):
    """step 3: the greatest T over the 3 x 3 tiles that exist"""
    th, tw = T.shape
    N = np.zeros_like(T)
    for j in range(th):
        for i in range(tw):
            N[j, i] = T[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2].max()
    return N


def gather(c, z, N, focus, aperture, max_radius, taps, seed, jitter):
    """step 4 for every pixel of one rectangle: c (hr, wr, >=3), z (hr, wr) raw depth, N (th, tw).
    Returns (out (hr, wr, 3) float32, gathered (hr, wr) bool, taps counted (hr, wr) int, taps skipped (hr, wr) int)"""
    hr, wr = z.shape
    c = np.ascontiguousarray(c, f32)[..., 0:3]
    y, x = np.mgrid[0:hr, 0:wr]
    rN = N[y >> 4, x >> 4]
    r = radius(z, focus, aperture, max_radius)
    Z = depth_z(z)
    D = directions()
    cok = finite(c).all(-1)
    with np.errstate(all="ignore"):
        gathered = (rN > f32(0.5)) & cok
        wp = f32(1.0) / area(r)
        At = ((rN * rN) * PI) / f32(taps)
        k0 = jitter_of(x, y, seed) if jitter else np.zeros((hr, wr), np.int64)
        fx, fy = x.astype(f32), y.astype(f32)
        total = np.zeros((hr, wr, 3), f32)
        Wt = np.zeros((hr, wr), f32)
        counted = np.zeros((hr, wr), np.int64)
        skipped = np.zeros((hr, wr), np.int64)
        for i in range(taps):
            rho = np.sqrt((f32(i) + f32(0.5)) / f32(taps))
            d = rN * rho
            Di = D[i + k0]
            qx = np.clip(np.floor((fx + d * Di[..., 0]) + f32(0.5)).astype(np.int64), 0, wr - 1)
            qy = np.clip(np.floor((fy + d * Di[..., 1]) + f32(0.5)).astype(np.int64), 0, hr - 1)
            rq, zq = r[qy, qx], Z[qy, qx]
            re = np.where(zq > Z, r, rq).astype(f32)
            cov = clamp01((re - d) + f32(0.5))
            w = (cov * At) / area(re)
            assert rho.dtype == f32 and d.dtype == f32 and cov.dtype == f32 and w.dtype == f32
            live = w > 0
            ok = live & cok[qy, qx]
            skipped += live & ~ok
            cq = np.where(ok[..., None], c[qy, qx], f32(0)).astype(f32)
            total = np.where(ok[..., None], total + cq * np.where(ok, w, f32(0)).astype(f32)[..., None], total).astype(f32)
            Wt = np.where(ok, Wt + w, Wt).astype(f32)
            counted += ok
        blurred = (c * wp[..., None] + total) / (wp + Wt)[..., None]
        out = np.where((gathered & (Wt != 0))[..., None], blurred, c).astype(f32)
    assert out.dtype == f32 and total.dtype == f32 and Wt.dtype == f32 and At.dtype == f32
    return out, gathered, np.where(gathered, counted, 0), np.where(gathered, skipped, 0)


def dof_ref(color, depth, pixels, rects=None, focus=1.0, aperture=0.0, max_radius=16.0, taps=32, seed=0, jitter=False, view_focus=None,
            fill=SENTINEL):
    """color (h, w, 4), depth (h, w) float32; pixels bool (h, w): the set (what is WRITTEN; the tile pass reads every rectangle pixel).
    Returns {out: (h, w, 4) uint32 bits, `fill` where nothing is written; scratch: (bytes / 4,) uint32 bits; T, N: [view] float32
    (th, tw); r: [view] float32 (hr, wr); pixels, sources, gathered, taps, nonfinite}"""
    color, depth = (np.ascontiguousarray(a, f32) for a in (color, depth))
    h, w = depth.shape
    rs = rectangles(rects, h, w)
    dims, nbytes = layout(rects, h, w)
    scratch = np.zeros(nbytes // 4, f32)
    pixels = np.asarray(pixels, bool)
    out = np.full((h, w, 4), fill, u32)
    res = dict(pixels=int(pixels.sum()), sources=0, gathered=0, taps=0, nonfinite=0, T=[], N=[], r=[])
    covered = np.zeros((h, w), bool)
    for v, (x0, y0, wr, hr) in enumerate(rs):
        box = (slice(y0, y0 + hr), slice(x0, x0 + wr))
        Fv = focus if view_focus is None else view_focus[v]
        r = radius(depth[box], Fv, aperture, max_radius)
        T = tile_max(r)
        N = neighbour_max(T)
        tw, th, at_t, at_n = (int(t) for t in dims[v])
        assert T.shape == (th, tw)
        scratch[at_t:at_t + tw * th] = T.reshape(-1)
        scratch[at_n:at_n + tw * th] = N.reshape(-1)
        o, gathered, counted, skipped = gather(color[box], depth[box], N, Fv, aperture, max_radius, taps, seed, jitter)
        sel = pixels[box]
        res["sources"] += wr * hr
        res["gathered"] += int((gathered & sel).sum())
        res["taps"] += int(counted[sel].sum())
        res["nonfinite"] += int(skipped[sel].sum())
        res["T"].append(T)
        res["N"].append(N)
        res["r"].append(r)
        block = out[box]
        block[sel] = np.concatenate([o, np.ones((hr, wr, 1), f32)], -1).view(u32)[sel]
        covered[box] = True
    assert not (pixels & ~covered).any(), "a pixel of the set lies in no rectangle"
    res["out"] = out
    res["scratch"] = scratch.view(u32).reshape(-1)
    return res
