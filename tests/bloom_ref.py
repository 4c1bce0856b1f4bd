"""NumPy evaluation of pt_bloom_layout's and pt_bloom_planes's rules, written from the text of include/pt_amd.h alone; shared by
tests/test_bloom_cabi.py and tests/test_gpu_bloom.py.  A helper, not a test; it never calls the kernels under test.  Everything is float32
arrays and float32 scalars, one rounding per operation, in the header's order (NumPy never contracts a product and a sum)."""
import numpy as np

from tile_ref import SENTINEL, finite, rectangles  # noqa: F401 (SENTINEL: for the tests)

f32 = np.float32
u32 = np.uint32
MAX_LEVELS = 8
COUNTERS = ("pixels", "sources", "bright", "nonfinite")
DEFAULTS = dict(exposure=1.0, threshold=1.0, knee=0.5, clamp=65504.0, spread=0.7, intensity=0.25, levels=6)


def layout(rects, h, w, levels):
    """(dims (nv, 8, 4) uint32: w_k, h_k, first float4 of the level, 0 — zeros above `levels`; bytes)"""
    rs = rectangles(rects, h, w)
    dims = np.zeros((len(rs), MAX_LEVELS, 4), u32)
    at = 0
    for v, (_, _, wk, hk) in enumerate(rs):
        for k in range(1, levels + 1):
            wk, hk = (wk + 1) // 2, (hk + 1) // 2
            dims[v, k - 1] = (wk, hk, at, 0)
            at += wk * hk
    return dims, 16 * at


def exposure_of(state, view):
    """E_v as pt_tonemap_planes step 1 reads it"""
    if state is None:
        return f32(1.0)
    E = f32(np.ascontiguousarray(state, f32)[view, 1])
    with np.errstate(all="ignore"):
        return E if bool(finite(E)) and E > 0 else f32(1.0)


def weight(Y, threshold, knee):
    """steps 4 .. 8 on an exposed luminance: g"""
    Y = np.ascontiguousarray(Y, f32)
    threshold, knee = f32(threshold), f32(knee)
    with np.errstate(all="ignore"):
        d = Y - threshold
        t = d + knee
        t = np.where(t > 0, t, f32(0)).astype(f32)
        t = np.where(t < f32(2.0) * knee, t, f32(2.0) * knee).astype(f32)
        t = (t * t) / (f32(4.0) * knee + f32(1e-4))
        m = np.where(t > d, t, d).astype(f32)
        m = np.where(m > 0, m, f32(0)).astype(f32)
        g = m / np.where(Y > f32(1e-4), Y, f32(1e-4)).astype(f32)
    assert g.dtype == f32
    return g


def source(c, E=1.0, exposure=1.0, threshold=1.0, knee=0.5, clamp=65504.0):
    """c (h, w, >=3) float32, one rectangle -> (B (h, w, 3), bright, nonfinite)"""
    c = np.ascontiguousarray(c, f32)[..., 0:3]
    bad = ~finite(c).all(-1)
    with np.errstate(all="ignore"):
        x = np.where(c > 0, c, f32(0)).astype(f32)
        x = np.where(x < f32(clamp), x, f32(clamp)).astype(f32)
        s = f32(E) * f32(exposure)
        Y = ((f32(0.2126) * x[..., 0] + f32(0.7152) * x[..., 1]) + f32(0.0722) * x[..., 2]) * s
        g = weight(Y, threshold, knee)
        B = x * g[..., None]
    assert s.dtype == f32 and Y.dtype == f32 and B.dtype == f32
    B[bad] = 0
    with np.errstate(all="ignore"):
        bright = (g > 0) & ~bad
    return B, int(bright.sum()), int(bad.sum())


def _row(s0, s1, s2, s3):
    return ((s0 + f32(3.0) * s1) + f32(3.0) * s2) + s3


def down(D):
    """D_{k-1} (h, w, 3) -> D_k"""
    h, w = D.shape[:2]
    hk, wk = (h + 1) // 2, (w + 1) // 2
    cols = [np.clip(2 * np.arange(wk) - 1 + t, 0, w - 1) for t in range(4)]
    rows = [np.clip(2 * np.arange(hk) - 1 + t, 0, h - 1) for t in range(4)]
    with np.errstate(all="ignore"):
        r = [_row(*(D[rows[u]][:, cols[t]] for t in range(4))) for u in range(4)]
        out = _row(*r) * f32(1.0 / 64.0)
    assert out.dtype == f32 and out.shape == (hk, wk, 3)
    return out


def up(U, h, w):
    """up_k: U_{k+1} (hu, wu, 3) at every texel of a level h x w"""
    hu, wu = U.shape[:2]
    x, y = np.arange(w), np.arange(h)
    i, j = x >> 1, y >> 1
    i2 = np.where(x & 1, np.minimum(i + 1, wu - 1), np.maximum(i - 1, 0))
    j2 = np.where(y & 1, np.minimum(j + 1, hu - 1), np.maximum(j - 1, 0))
    a, b, c, d = U[j][:, i], U[j][:, i2], U[j2][:, i], U[j2][:, i2]
    q, t = f32(0.25), f32(0.75)
    with np.errstate(all="ignore"):
        out = t * (t * a + q * b) + q * (t * c + q * d)
    assert out.dtype == f32
    return out


def pyramid(B, levels, spread):
    """([D_1 .. D_levels], [U_1 .. U_levels]) of one rectangle"""
    D = [B]
    for _ in range(levels):
        D.append(down(D[-1]))
    U = [None] * (levels + 1)
    U[levels] = D[levels]
    with np.errstate(all="ignore"):
        for k in range(levels - 1, 0, -1):
            U[k] = D[k] + f32(spread) * up(U[k + 1], *D[k].shape[:2])
    return D[1:], U[1:]


def gain(intensity, spread, levels):
    """a = intensity * (1 / n) and n"""
    n = f32(1.0)
    for _ in range(levels - 1):
        n = n * f32(spread) + f32(1.0)
    return f32(intensity) * (f32(1.0) / n), n


def bloom_ref(color, pixels, state=None, rects=None, exposure=1.0, threshold=1.0, knee=0.5, clamp=65504.0, spread=0.7, intensity=0.25, levels=6,
              out0=None, fill=SENTINEL):
    """color (h, w, 4) float32; pixels bool (h, w): the set (what is WRITTEN; the pyramid reads every rectangle pixel).  out0: what out
    holds before the call (the colour itself for an in-place call), else `fill`.
    Returns {out: (h, w, 4) uint32 bits; scratch: (bytes / 4,) uint32 bits; U: [view][k - 1] float32 (h_k, w_k, 3); D likewise; pixels,
    sources, bright, nonfinite}"""
    color = np.ascontiguousarray(color, f32)
    h, w = color.shape[:2]
    rs = rectangles(rects, h, w)
    dims, nbytes = layout(rects, h, w, levels)
    scratch = np.zeros((nbytes // 16, 4), f32)
    pixels = np.asarray(pixels, bool)
    out = np.full((h, w, 4), fill, u32) if out0 is None else np.ascontiguousarray(out0, f32).view(u32).copy()
    a, _ = gain(intensity, spread, levels)
    res = dict(pixels=int(pixels.sum()), sources=0, bright=0, nonfinite=0, U=[], D=[], B=[])
    covered = np.zeros((h, w), bool)
    for v, (x0, y0, wr, hr) in enumerate(rs):
        c = color[y0:y0 + hr, x0:x0 + wr]
        B, bright, bad = source(c, exposure_of(state, v), exposure, threshold, knee, clamp)
        D, U = pyramid(B, levels, spread)
        res["sources"] += wr * hr
        res["bright"] += bright
        res["nonfinite"] += bad
        res["U"].append(U)
        res["D"].append(D)
        res["B"].append(B)
        for k in range(levels):
            wk, hk, at, _ = (int(t) for t in dims[v, k])
            assert U[k].shape == (hk, wk, 3)
            scratch[at:at + wk * hk, 0:3] = U[k].reshape(-1, 3)
        with np.errstate(all="ignore"):
            o = c[..., 0:3] + a * up(U[0], hr, wr)
        assert o.dtype == f32
        sel = pixels[y0:y0 + hr, x0:x0 + wr]
        block = out[y0:y0 + hr, x0:x0 + wr]
        block[sel] = np.concatenate([o, np.ones((hr, wr, 1), f32)], -1).view(u32)[sel]
        covered[y0:y0 + hr, x0:x0 + wr] = True
    assert not (pixels & ~covered).any(), "a pixel of the set lies in no rectangle"
    res["out"] = out
    res["scratch"] = scratch.view(u32).reshape(-1)
    return res
