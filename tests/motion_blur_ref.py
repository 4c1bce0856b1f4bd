"""NumPy evaluation of pt_motion_blur_layout's and pt_motion_blur_planes's rules, written from the text of include/pt_amd.h alone; shared by
tests/test_motion_blur_cabi.py and tests/test_gpu_motion_blur.py.  A helper, not a test; it never calls the kernels under test.  Everything
is float32 arrays and float32 scalars, one rounding per operation, in the header's order (NumPy never contracts a product and a sum; its
sqrt and its division are correctly rounded).  Vectorised over the pixels of a rectangle; the only loops are over the taps and the tiles."""
import numpy as np

import tile_ref
from tile_ref import FLT_MAX, SENTINEL, TILE, clamp01, depth_z, finite, hash32, rectangles  # noqa: F401 (kept as this module's names)

f32 = np.float32
u32 = np.uint32
JITTER = 1
COUNTERS = ("pixels", "sources", "unknown", "moving", "taps", "nonfinite")
DEFAULTS = dict(shutter=0.5, max_blur=16.0, depth_soft=0.05, taps=12, seed=0, jitter=False)


def layout(rects, h, w):
    """(dims (nv, 4) uint32: tw, th, first 8-byte texel of T, first of N; bytes)"""
    return tile_ref.layout(rects, h, w, 8)


def velocity(m, shutter, max_blur):
    """step 1: motion (..., 2) -> (V (..., 2), l2 (...), unknown (...))"""
    m = np.ascontiguousarray(m, f32)
    hs = f32(0.5) * f32(shutter)
    R = f32(max_blur)
    R2 = R * R
    unknown = ~finite(m).all(-1)
    lim = f32(4096.0)
    with np.errstate(all="ignore"):
        V = np.where(unknown[..., None], f32(0), m).astype(f32) * hs
        V = np.where(V < -lim, -lim, V).astype(f32)
        V = np.where(V > lim, lim, V).astype(f32)
        l2 = V[..., 0] * V[..., 0] + V[..., 1] * V[..., 1]
        big = l2 > R2
        s = R / np.sqrt(np.where(big, l2, f32(1)).astype(f32))
        Vs = V * s[..., None]
        l2s = Vs[..., 0] * Vs[..., 0] + Vs[..., 1] * Vs[..., 1]
        V = np.where(big[..., None], Vs, V).astype(f32)
        l2 = np.where(big, l2s, l2).astype(f32)
    assert hs.dtype == f32 and R2.dtype == f32 and V.dtype == f32 and l2.dtype == f32
    return V, l2, unknown


def tile_max(V, l2):
    """step 2: (hr, wr) -> T (th, tw, 2): the V of greatest l2 per tile, the first in row order among equals (argmax's rule; l2 >= 0 is
    never NaN)"""
    hr, wr = l2.shape
    tw, th = (wr + TILE - 1) // TILE, (hr + TILE - 1) // TILE
    T = np.zeros((th, tw, 2), f32)
    for j in range(th):
        for i in range(tw):
            sl = (slice(TILE * j, TILE * j + TILE), slice(TILE * i, TILE * i + TILE))
            k = int(np.argmax(l2[sl].reshape(-1)))
            T[j, i] = V[sl].reshape(-1, 2)[k]
    return T


def neighbour_max(T):
    """step 3: the T of greatest l2 over the 3 x 3 tiles that exist, row order, strict >"""
    th, tw = T.shape[:2]
    with np.errstate(all="ignore"):
        l2 = T[..., 0] * T[..., 0] + T[..., 1] * T[..., 1]
    N = np.zeros_like(T)
    for j in range(th):
        for i in range(tw):
            best = None
            for v in range(max(j - 1, 0), min(j + 2, th)):
                for u in range(max(i - 1, 0), min(i + 2, tw)):
                    if best is None or l2[v, u] > l2[best]:
                        best = (v, u)
            N[j, i] = T[best]
    return N


def jitter_of(x, y, seed):
    """j in [-0.5, 0.5) of the local coordinates"""
    j = (hash32(x, y, seed) >> u32(8)).astype(f32) * f32(2.0 ** -24) - f32(0.5)
    assert j.dtype == f32
    return j


def length(l2):
    with np.errstate(all="ignore"):
        l = np.sqrt(l2)
        return np.where(l > f32(0.5), l, f32(0.5)).astype(f32)


def cone(d, l):
    with np.errstate(all="ignore"):
        return clamp01(f32(1.0) - d / l)


def cyl(d, l):
    with np.errstate(all="ignore"):
        u = clamp01((d - f32(0.95) * l) / (f32(1.05) * l - f32(0.95) * l))
        return f32(1.0) - (u * u) * (f32(3.0) - f32(2.0) * u)


def gather(c, m, z, N, shutter, max_blur, depth_soft, taps, seed, jitter):
    """step 4 for every pixel of one rectangle: c (hr, wr, >=3), m (hr, wr, 2), z (hr, wr) raw depth, N (th, tw, 2).
    Returns (out (hr, wr, 3) float32, moving (hr, wr) bool, taps counted (hr, wr) int, taps skipped (hr, wr) int)"""
    hr, wr = z.shape
    c = np.ascontiguousarray(c, f32)[..., 0:3]
    y, x = np.mgrid[0:hr, 0:wr]
    vN = N[y >> 4, x >> 4]
    _, l2, _ = velocity(m, shutter, max_blur)
    Z = depth_z(z)
    with np.errstate(all="ignore"):
        n2 = vN[..., 0] * vN[..., 0] + vN[..., 1] * vN[..., 1]
        moving = (n2 > f32(0.25)) & finite(c).all(-1)
        lN = np.sqrt(n2)
        lp = length(l2)
        wp = f32(1.0) / lp
        j = jitter_of(x, y, seed) if jitter else np.zeros((hr, wr), f32)
        fx, fy = x.astype(f32), y.astype(f32)
        total = np.zeros((hr, wr, 3), f32)
        Wt = np.zeros((hr, wr), f32)
        counted = np.zeros((hr, wr), np.int64)
        skipped = np.zeros((hr, wr), np.int64)
        for i in range(taps):
            a = (f32(i) + f32(0.5)) + j
            t = (f32(2.0) * a) / f32(taps) - f32(1.0)
            qx = np.clip(np.floor((fx + vN[..., 0] * t) + f32(0.5)).astype(np.int64), 0, wr - 1)
            qy = np.clip(np.floor((fy + vN[..., 1] * t) + f32(0.5)).astype(np.int64), 0, hr - 1)
            cq = c[qy, qx]
            ok = finite(cq).all(-1)
            skipped += ~ok
            d = np.abs(t) * lN
            lq = length(l2[qy, qx])
            zq = Z[qy, qx]
            e = f32(depth_soft) * np.where(Z < zq, Z, zq).astype(f32)
            fg = clamp01(f32(1.0) - (zq - Z) / e)
            bg = clamp01(f32(1.0) - (Z - zq) / e)
            w = (fg * cone(d, lq) + bg * cone(d, lp)) + (cyl(d, lq) * cyl(d, lp)) * f32(2.0)
            assert t.dtype == f32 and d.dtype == f32 and e.dtype == f32 and w.dtype == f32
            w = np.where(ok, w, f32(0)).astype(f32)  # (a skipped tap adds nothing: x + 0 = x for the sums, which are never -0)
            total = np.where(ok[..., None], total + np.where(ok[..., None], cq, f32(0)).astype(f32) * w[..., None], total).astype(f32)
            Wt = np.where(ok, Wt + w, Wt).astype(f32)
            counted += ok & (w > 0)
        blurred = (c * wp[..., None] + total) / (wp + Wt)[..., None]
        out = np.where((moving & (Wt != 0))[..., None], blurred, c).astype(f32)
    assert out.dtype == f32 and total.dtype == f32 and Wt.dtype == f32
    return out, moving, np.where(moving, counted, 0), np.where(moving, skipped, 0)


def motion_blur_ref(color, motion, depth, pixels, rects=None, shutter=0.5, max_blur=16.0, depth_soft=0.05, taps=12, seed=0, jitter=False,
                    fill=SENTINEL):
    """color (h, w, 4), motion (h, w, 2), depth (h, w) float32; pixels bool (h, w): the set (what is WRITTEN; the tile pass reads every
    rectangle pixel).  Returns {out: (h, w, 4) uint32 bits, `fill` where nothing is written; scratch: (bytes / 4,) uint32 bits; T, N:
    [view] float32 (th, tw, 2); pixels, sources, unknown, moving, taps, nonfinite}"""
    color, motion, depth = (np.ascontiguousarray(a, f32) for a in (color, motion, depth))
    h, w = depth.shape
    rs = rectangles(rects, h, w)
    dims, nbytes = layout(rects, h, w)
    scratch = np.zeros((nbytes // 8, 2), f32)
    pixels = np.asarray(pixels, bool)
    out = np.full((h, w, 4), fill, u32)
    res = dict(pixels=int(pixels.sum()), sources=0, unknown=0, moving=0, taps=0, nonfinite=0, T=[], N=[])
    covered = np.zeros((h, w), bool)
    for v, (x0, y0, wr, hr) in enumerate(rs):
        box = (slice(y0, y0 + hr), slice(x0, x0 + wr))
        V, l2, unknown = velocity(motion[box], shutter, max_blur)
        T = tile_max(V, l2)
        N = neighbour_max(T)
        tw, th, at_t, at_n = (int(t) for t in dims[v])
        assert T.shape == (th, tw, 2)
        scratch[at_t:at_t + tw * th] = T.reshape(-1, 2)
        scratch[at_n:at_n + tw * th] = N.reshape(-1, 2)
        o, moving, counted, skipped = gather(color[box], motion[box], depth[box], N, shutter, max_blur, depth_soft, taps, seed, jitter)
        sel = pixels[box]
        res["sources"] += wr * hr
        res["unknown"] += int(unknown.sum())
        res["moving"] += int((moving & sel).sum())
        res["taps"] += int(counted[sel].sum())
        res["nonfinite"] += int(skipped[sel].sum())
        res["T"].append(T)
        res["N"].append(N)
        block = out[box]
        block[sel] = np.concatenate([o, np.ones((hr, wr, 1), f32)], -1).view(u32)[sel]
        covered[box] = True
    assert not (pixels & ~covered).any(), "a pixel of the set lies in no rectangle"
    res["out"] = out
    res["scratch"] = scratch.view(u32).reshape(-1)
    return res
