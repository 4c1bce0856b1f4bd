"""NumPy evaluation of pt_exposure_planes' and pt_tonemap_planes' rules, written from the text of include/pt_amd.h alone; shared by
tests/test_exposure_cabi.py and tests/test_gpu_exposure.py.  A helper, not a test; it never calls the kernels under test.  Metering is
integer and bit operations on float32.view(uint32) (the luminance: float32, one rounding per operation); the adaptation is Python integers,
then float32; E is include/pt_detmath.h's pt_expf restated operation by operation in float32; the operators are float32, one rounding per
operation."""
import numpy as np

f32 = np.float32
u32 = np.uint32
BINS = 256
SENTINEL = u32(0xA5A5A5A5)
NAN_BITS = u32(0x7FC00000)
COUNTERS = ("pixels", "skipped", "nonfinite", "under", "over")
OPS = ("linear", "reinhard", "aces")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def finite(a):
    """the exponent-bit test"""
    return (_bits(a) & u32(0x7F800000)) != u32(0x7F800000)


def luminance(c):
    """(..., >=3) float32 -> (...): (0.2126f * x + 0.7152f * y) + 0.0722f * z"""
    c = np.ascontiguousarray(c, f32)
    with np.errstate(all="ignore"):
        Y = (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]
    assert Y.dtype == f32
    return Y


def bin_of(Y):
    """step 3 of the metering: the bin of a float32 luminance, from its bit pattern"""
    Y = np.ascontiguousarray(Y, f32)
    with np.errstate(all="ignore"):
        pos = Y > 0
    k = (_bits(Y) >> u32(20)).astype(np.int64) - 887
    b = np.clip(k, 0, 255)
    b = np.where(finite(Y), b, 255)
    return np.where(pos, b, 0).astype(np.int64)


def view_index(rects, h, w):
    """(h, w) int: the view of each pixel, -1 outside every rectangle; rects None or empty: one view, the frame"""
    if not rects:
        return np.zeros((h, w), np.int64)
    v = np.full((h, w), -1, np.int64)
    for k, (x0, y0, wr, hr) in enumerate(rects):
        v[y0:y0 + hr, x0:x0 + wr] = k
    return v


def meter_ref(color, pixels, hit=None, rects=None, hist=None):
    """color (h, w, 4) float32; pixels bool (h, w): the set; hit (h, w, 8) float32 or None; rects: the views.  hist: (nv, 256) counts to add
    to (ACCUMULATE), or None.  Returns (hist (nv, 256) uint32, {pixels, skipped, nonfinite, under, over})"""
    color = np.ascontiguousarray(color, f32)
    h, w = color.shape[:2]
    nv = max(1, len(rects or ()))
    out = np.zeros((nv, BINS), np.int64) if hist is None else np.asarray(hist).astype(np.int64).copy()
    pixels = np.asarray(pixels, bool)
    view = view_index(rects, h, w)
    assert (view[pixels] >= 0).all(), "a pixel of the set lies in no rectangle"
    skipped = pixels & (np.ascontiguousarray(hit, f32).view(np.int32)[..., 3] < 0) if hit is not None else np.zeros((h, w), bool)
    nonfinite = pixels & ~skipped & ~finite(color[..., 0:3]).all(-1)
    counted = pixels & ~skipped & ~nonfinite
    b = bin_of(luminance(color))
    np.add.at(out, (view[counted], b[counted]), 1)
    return (out & 0xFFFFFFFF).astype(u32), dict(pixels=int(pixels.sum()), skipped=int(skipped.sum()), nonfinite=int(nonfinite.sum()),
                                                under=int((counted & (b == 0)).sum()), over=int((counted & (b == 255)).sum()))


def expf(x):
    """include/pt_detmath.h's pt_expf, operation by operation in float32 (the library is compiled without contraction)"""
    x = f32(x)
    t = f32(f32(1.44269504088896341) * x) + f32(0.5)
    n = int(t)  # truncation, as (int)t
    if f32(n) > t:
        n -= 1
    z = f32(n)
    x = x - z * f32(0.693359375)
    x = x - z * f32(-2.12194440e-4)
    z = x * x
    p = f32(1.9875691500E-4) * x + f32(1.3981999507E-3)
    for coef in (8.3334519073E-3, 4.1665795894E-2, 1.6666665459E-1, 5.0000001201E-1):
        p = p * x + f32(coef)
    z = p * z + x + f32(1.0)
    assert isinstance(z, f32) and isinstance(x, f32)
    return f32(z * np.array((n + 127) << 23, u32).view(f32))


def adapt_ref(hist, state_in=None, low_permille=50, high_permille=20, key_log2=-2.4739312, ev_min=-16.0, ev_max=16.0, rate_up=1.0, rate_down=1.0):
    """hist (nv, 256) counts; state_in (nv, 4) float32 or None.  Returns state_out (nv, 4) float32: ev, E, m, n."""
    hist = np.asarray(hist)
    nv = hist.shape[0]
    out = np.zeros((nv, 4), f32)
    key, lo_ev, hi_ev, up, down = f32(key_log2), f32(ev_min), f32(ev_max), f32(rate_up), f32(rate_down)
    for v in range(nv):
        c = [int(x) for x in hist[v]]
        N = sum(c)
        lo, hi = N * int(low_permille) // 1000, N * int(high_permille) // 1000
        for i in range(BINS):
            take = min(c[i], lo)
            c[i] -= take
            lo -= take
        for i in range(BINS - 1, -1, -1):
            take = min(c[i], hi)
            c[i] -= take
            hi -= take
        n = sum(c[1:255])
        S = sum(c[i] * (2 * i - 1) for i in range(1, 255))
        have = state_in is not None
        ev_prev = f32(state_in[v][0]) if have else f32(0)
        prev_ok = have and bool(finite(ev_prev))
        with np.errstate(all="ignore"):
            if n == 0:
                m = f32(state_in[v][2]) if have else NAN_BITS.view(f32)
                ev = ev_prev if prev_ok else f32(0)
            else:
                q = (S << 12) // n
                assert q < 1 << 21
                m = f32(q) * f32(1.0 / 65536.0) - f32(16.0)
                t = key - m
                t = lo_ev if t < lo_ev else t
                t = hi_ev if t > hi_ev else t
                if not prev_ok:
                    ev = t
                else:
                    r = up if t > ev_prev else down
                    ev = ev_prev + ((t - ev_prev) * r)
            E = expf(f32(ev) * f32(0.69314718))
        out[v] = (ev, E, m, f32(n))
    return out


def exposure_ref(color, pixels, hit=None, rects=None, hist=None, state_in=None, **prm):
    """meter_ref then adapt_ref: (hist, state_out, counters)"""
    hist, counts = meter_ref(color, pixels, hit, rects, hist)
    return hist, adapt_ref(hist, state_in, **prm), counts


def _clamp(x):
    with np.errstate(all="ignore"):
        x = np.where(x > 0, x, f32(0)).astype(f32)  # a NaN gives 0
        return np.where(x < f32(65504.0), x, f32(65504.0)).astype(f32)


def aces(x):
    a = x * (f32(2.51) * x + f32(0.03))
    b = x * (f32(2.43) * x + f32(0.59)) + f32(0.14)
    y = a / b
    assert y.dtype == f32
    return y


def reinhard(x, white):
    """(n, 3): the frame path's operator on the whole colour"""
    L = (f32(0.2126) * x[:, 0] + f32(0.7152) * x[:, 1]) + f32(0.0722) * x[:, 2]
    inv = f32(1.0) / (f32(1.0) + L / f32(white))
    y = (x * f32(1.0)) * inv[:, None]
    assert y.dtype == f32
    return y


def operator_ref(x, op, white=1.0):
    """steps 3's clamp aside: x (n, 3) float32 already scaled and clamped -> y (n, 3)"""
    x = np.ascontiguousarray(x, f32)
    return x if op == "linear" else reinhard(x, white) if op == "reinhard" else aces(x)


def tonemap_ref(color, pixels, state=None, rects=None, op="aces", exposure=1.0, white=1.0, planes=("out", "frame_rgba8"), fill=SENTINEL, orc=None):
    """color (h, w, 4); pixels bool (h, w); state (nv, 4) float32 or None.  orc: the CPU checker, needed by "frame_rgba8" alone (its
    make_color).  Returns {plane: uint32 bits of the whole plane, `fill` outside the set; pixels, clipped: int}"""
    color = np.ascontiguousarray(color, f32)
    h, w = color.shape[:2]
    pixels = np.asarray(pixels, bool)
    Y, X = np.nonzero(pixels)
    n = len(Y)
    view = view_index(rects, h, w)[Y, X]
    E = np.ones(n, f32)
    if state is not None:
        E = np.ascontiguousarray(state, f32)[view, 1]
        with np.errstate(all="ignore"):
            E = np.where(finite(E) & (E > 0), E, f32(1.0)).astype(f32)
    with np.errstate(all="ignore"):
        s = E * f32(exposure)
        x = _clamp(color[Y, X, 0:3] * s[:, None])
        y = operator_ref(x, op, white)
    assert s.dtype == f32 and y.dtype == f32
    res = dict(pixels=n, clipped=int((y > 1).any(-1).sum()), y=y)
    if "out" in planes:
        res["out"] = np.full((h, w, 4), fill, u32)
        res["out"][Y, X] = np.concatenate([y, np.ones((n, 1), f32)], -1).view(u32)
    if "frame_rgba8" in planes:
        import temporal_ref as T

        res["frame_rgba8"] = np.full((h, w, 1), fill, u32)
        if n:
            res["frame_rgba8"][Y, X, 0] = T.make_color_bits(orc, np.ascontiguousarray(y))
    return res
