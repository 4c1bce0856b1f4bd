"""float32 NumPy evaluation of pt_upsample_planes' arithmetic, written from the text of include/pt_amd.h, shared by
tests/test_upsample_cabi.py and tests/test_gpu_upsample.py.  A helper, not a test.  Integers and float32, one rounding per operation, in the
header's order; it never calls the kernel under test."""
import numpy as np

from temporal_ref import SENTINEL

f32 = np.float32
DEFAULTS = dict(normal_cos=0.9, plane_eps=0.01)
# the branch a pixel took
FULL, PARTIAL, RESCUE, ORPHAN, OUTSIDE = 0, 1, 2, 3, -1
# why a tap of the bilinear stage did not count: the first test it fails, in this order (w0: its weight is zero)
REASONS = ("w0", "rect", "kind", "mesh", "normal", "plane", "colour")


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _f(a):
    a = np.ascontiguousarray(a)
    return a.view(f32) if a.dtype == np.uint32 else np.ascontiguousarray(a, f32)


def axis(X, x0, s):
    """step 1 of the header for one axis: (c, i, f) of integer coordinates X in a rectangle that starts at x0"""
    X, x0 = np.asarray(X, np.int64), np.asarray(x0, np.int64)
    a = X - x0
    r = a % s
    c = x0 // s + a // s
    t = (2 * r + 1 - s).astype(f32) / f32(2 * s)
    neg = t < 0
    return c, np.where(neg, c - 1, c), np.where(neg, t + f32(1.0), t).astype(f32)


def upsample_ref(lo, hi, scale, rects, pixels, fill=SENTINEL, guided=True, geometry=True, swap=False, **params):
    """lo: color (lh, lw, 4), hit (lh, lw, 8), position (lh, lw, 4); hi: hit (h, w, 8), position (h, w, 4) — float32 or their uint32 bits.
    rects: [(x0, y0, wr, hr)], the views, or [(0, 0, w, h)] without views.  pixels: bool (h, w), the set the call processes (each inside
    exactly one rectangle).
    Returns {out: uint32 (h, w, 4), weight_out: uint32 (h, w) — bits over the whole frame, `fill` outside the set; pixels, hits, full,
    rescued, orphans: int; branch: int8 (h, w), FULL / PARTIAL / RESCUE / ORPHAN, OUTSIDE outside the set; taps: {reason: int (h, w)}, per
    pixel the taps of the bilinear stage rejected for that reason; counted: int (h, w), those that counted}.
    Not the header's rule, for the tests that show what its parts are for: guided=False lets every tap inside the rectangle with a finite
    colour count (plain bilinear interpolation); geometry=False drops the normal and the plane test; swap=True exchanges fx and fy."""
    prm = dict(DEFAULTS, **params)
    s = int(scale)
    lo_color, lo_hit, lo_pos = _f(lo["color"]), _f(lo["hit"]), _f(lo["position"])
    hit, pos = _f(hi["hit"]), _f(hi["position"])
    h, w = hit.shape[:2]
    lh, lw = lo_hit.shape[:2]
    assert (lw * s, lh * s) == (w, h)
    pixels = np.asarray(pixels, bool)
    YY, XX = np.mgrid[0:h, 0:w]
    x0 = np.zeros((h, w), np.int64)
    y0, x1, y1 = x0.copy(), x0.copy(), x0.copy()
    seen = np.zeros((h, w), bool)
    for rx, ry, rw, rh in rects:
        assert not seen[ry:ry + rh, rx:rx + rw].any() and rx % s == 0 and ry % s == 0 and rw % s == 0 and rh % s == 0
        seen[ry:ry + rh, rx:rx + rw] = True
        x0[ry:ry + rh, rx:rx + rw], y0[ry:ry + rh, rx:rx + rw], x1[ry:ry + rh, rx:rx + rw], y1[ry:ry + rh, rx:rx + rw] = rx, ry, rx + rw, ry + rh
    assert seen[pixels].all(), "a pixel of the set lies in no rectangle"
    lx0, ly0, lx1, ly1 = x0 // s, y0 // s, x1 // s, y1 // s
    words, lo_words = hit.view(np.int32), lo_hit.view(np.int32)
    miss = words[..., 3] < 0
    mesh, ng, P = words[..., 4], hit[..., 5:8], pos[..., 0:3]
    ncos = f32(prm["normal_cos"])
    cx, i, fx = axis(XX, x0, s)
    cy, j, fy = axis(YY, y0, s)
    if swap:
        fx, fy = fy, fx
    taps = {r: np.zeros((h, w), np.int64) for r in REASONS}
    counted = np.zeros((h, w), np.int64)

    with np.errstate(all="ignore"):
        plane_max = f32(prm["plane_eps"]) * hit[..., 0]

        def test(qx, qy, who, book):
            """(counts (h, w), the colour of q (h, w, 4)) for low-res pixel q of the pixels `who`"""
            alive = who.copy()

            def drop(cond, why):
                nonlocal alive
                if book:
                    taps[why][alive & cond] += 1
                alive = alive & ~cond

            drop(~((qx >= lx0) & (qx < lx1) & (qy >= ly0) & (qy < ly1)), "rect")
            qx, qy = np.where(alive, qx, 0), np.where(alive, qy, 0)
            cq = lo_color[qy, qx]
            if guided:
                qmiss = lo_words[qy, qx, 3] < 0
                drop(miss != qmiss, "kind")
                drop(~miss & (lo_words[qy, qx, 4] != mesh), "mesh")
                if geometry:
                    drop(~miss & ~(_dot3(ng, lo_hit[qy, qx, 5:8]) >= ncos), "normal")
                    drop(~miss & ~(np.abs(_dot3(ng, lo_pos[qy, qx, 0:3] - P)) <= plane_max), "plane")
            drop(~((np.ascontiguousarray(cq[..., 0:3]).view(np.uint32) & 0x7F800000) != 0x7F800000).all(-1), "colour")
            return alive, cq

        # ---- 3. the bilinear stage
        S, W = np.zeros((h, w, 4), f32), np.zeros((h, w), f32)
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            wx = fx if dx else f32(1.0) - fx
            wy = fy if dy else f32(1.0) - fy
            wgt = (wx * wy).astype(f32)
            taps["w0"][pixels & (wgt == 0)] += 1
            ok, cq = test(i + dx, j + dy, pixels & (wgt != 0), True)
            S = np.where(ok[..., None], S + cq * wgt[..., None], S)
            W = np.where(ok, W + wgt, W)
            counted[ok] += 1
        assert S.dtype == f32 and W.dtype == f32
        has = pixels & (W > 0)
        out = S / W[..., None]
        weight = W.copy()
        branch = np.full((h, w), OUTSIDE, np.int8)
        branch[has] = np.where(counted[has] == 4, FULL, PARTIAL)
        # ---- 4. the rescue
        need = pixels & ~has
        S4, N = np.zeros((h, w, 4), f32), np.zeros((h, w), f32)
        if need.any():
            for dy in range(-1, 3):
                for dx in range(-1, 3):
                    ok, cq = test(i + dx, j + dy, need, False)
                    S4 = np.where(ok[..., None], S4 + cq, S4)
                    N = np.where(ok, N + f32(1.0), N)
        rescued = need & (N > 0)
        out = np.where(rescued[..., None], S4 / N[..., None], out).astype(f32)
        weight[rescued] = 0.0
        branch[rescued] = RESCUE
        # ---- 5. the orphans
        orphan = need & ~rescued
        weight[orphan] = -1.0
        branch[orphan] = ORPHAN
    bits = out.view(np.uint32).copy()
    bits[orphan] = lo_color.view(np.uint32)[cy[orphan], cx[orphan]]  # the four words as they are
    res = dict(out=np.full((h, w, 4), fill, np.uint32), weight_out=np.full((h, w), fill, np.uint32))
    res["out"][pixels] = bits[pixels]
    res["weight_out"][pixels] = weight.view(np.uint32)[pixels]
    res.update(pixels=int(pixels.sum()), hits=int((pixels & ~miss).sum()), full=int((branch == FULL).sum()), rescued=int(rescued.sum()),
               orphans=int(orphan.sum()), branch=branch, taps=taps, counted=counted)
    return res


def counters(ref):
    return tuple(ref[k] for k in ("pixels", "hits", "full", "rescued", "orphans"))


# ------------------------------------------------------------------ hand-made planes: every branch and every rejection reason on a known pixel
SYNTHETIC_PARAMS = dict(normal_cos=0.9, plane_eps=0.125)
SYNTHETIC_VIEW = 48  # two square views side by side: a multiple of 8 (pt_set_views) and of every scale
# kind -> (mesh, z of its plane, normal); t = 4 everywhere, so plane_eps * t = 0.5 exactly
_Z_BEYOND = float(np.nextafter(f32(0.5), f32(1.0)))
KINDS = {0: (0, 0.0, (0.0, 0.0, 1.0)),        # the background
         1: (0, 0.5, (0.0, 0.0, 1.0)),        # a plane distance EXACTLY on plane_eps * t from kind 0: counts
         2: (1, 0.0, (0.0, 0.0, 1.0)),        # another mesh
         3: (0, 0.0, (0.6, 0.0, 0.8)),        # dot 0.8 < 0.9 with kind 0
         4: (0, _Z_BEYOND, (0.0, 0.0, 1.0)),  # one ulp beyond plane_eps * t from kind 0: does not count
         5: None,                             # a miss
         7: (3, 0.0, (0.0, 0.0, 1.0)),        # the rescued pixel's surface: one low-res pixel has it, in the outer ring
         8: (4, 0.0, (0.0, 0.0, 1.0))}        # the orphans' surface: no low-res pixel has it


def _records(kind):
    """hit (.., 8) and position (.., 4) planes of a map of kinds; every position has x = y = 0, so a plane distance is a difference of z"""
    hit = np.zeros(kind.shape + (8,), f32)
    pos = np.zeros(kind.shape + (4,), f32)
    words = hit.view(np.int32)
    for k, rec in KINDS.items():
        at = kind == k
        if rec is None:
            hit[at, 0] = f32(1e16)
            words[at, 3] = words[at, 4] = -1
        else:
            m, z, n = rec
            hit[at, 0] = 4.0
            words[at, 3], words[at, 4] = 7, m
            hit[at, 5:8] = np.array(n, f32)
            pos[at] = np.array([0.0, 0.0, z, 1.0], f32)
    return hit, pos


def synthetic_planes(scale):
    """Hand-made planes for a 96 x 48 frame of two 48 x 48 views, A at x = 0 and B at x = 48, over a low-resolution frame of 96/s x 48/s.
    Both views are the background surface (kind 0) with random colours (B's are 2 higher); every other low-res pixel named below lies
    in A, at low-res coordinates (u, v) that exist at every scale, and a full-res pixel has the kind of the low-res pixel that contains it
    unless it is one of the three overridden ones.
    Returns dict(lo, hi, rects, size, params, known): known[name] = (X, Y, branch, {reason: rejected taps of the bilinear stage})."""
    s = int(scale)
    V = SYNTHETIC_VIEW
    w, h, lw, lh = 2 * V, V, 2 * V // s, V // s
    rng = np.random.default_rng(40 + s)
    lo_kind = np.zeros((lh, lw), np.int64)
    lo_kind[2, 2], lo_kind[2, 5], lo_kind[2, 8], lo_kind[5, 2], lo_kind[8, 2] = 2, 3, 1, 4, 5
    lo_kind[8:10, 5:7] = 5     # four misses: miss-miss interpolation
    lo_kind[10, 10] = 7        # the only low-res pixel of the rescued pixel's surface
    lo_color = rng.random((lh, lw, 4), dtype=f32)
    lo_color[:, lw // 2:, :3] += f32(2.0)
    lo_color[5, 5, 1] = np.nan
    lo_color[5, 8, 2] = np.inf
    hi_kind = np.repeat(np.repeat(lo_kind, s, 0), s, 1)

    def px(u, v, rx=0, ry=0):
        return u * s + rx, v * s + ry

    known = {}
    # residue (0, 0) of cell (u, v): the taps are (u-1, v-1), (u, v-1), (u-1, v), (u, v), all of weight > 0
    known["mesh"] = px(2, 2) + (PARTIAL, dict(mesh=3))
    known["normal"] = px(5, 2) + (PARTIAL, dict(normal=3))
    known["plane_exactly_on"] = px(8, 2) + (FULL, dict())
    known["plane_one_ulp_beyond"] = px(2, 5) + (PARTIAL, dict(plane=3))
    known["nan_colour_tap"] = px(5, 5) + (PARTIAL, dict(colour=1))
    known["inf_colour_tap"] = px(8, 5) + (PARTIAL, dict(colour=1))
    known["miss_beside_hits"] = px(2, 8) + (PARTIAL, dict(kind=3))
    known["hit_beside_a_miss"] = px(1, 7, s - 1, s - 1) + (PARTIAL, dict(kind=1))  # taps (1,7), (2,7), (1,8), (2,8)
    known["miss_miss"] = px(6, 9) + (FULL, dict())                                 # taps (5,8), (6,8), (5,9), (6,9): four misses
    # the rescue: taps (8..9, 8..9) are the background, the ring (7..10, 7..10) holds (10, 10)
    X, Y = px(9, 9)
    hi_kind[Y, X] = 7
    known["rescue"] = (X, Y, RESCUE, dict(mesh=4))
    # the orphans: no low-res pixel of their surface; the second one lies in the low-res pixel with the NaN colour word
    X, Y = px(9, 5)
    hi_kind[Y, X] = 8
    known["orphan"] = (X, Y, ORPHAN, dict(mesh=4))
    X, Y = px(5, 5, 1, 1)
    hi_kind[Y, X] = 8
    known["orphan_over_nan"] = (X, Y, ORPHAN, dict(mesh=1, w0=3) if s == 3 else dict(mesh=4))
    if s == 3:  # the centre residue: fx = fy = 0, one tap of weight 1
        known["weight_zero_taps"] = px(3, 3, 1, 1) + (PARTIAL, dict(w0=3))
    # taps outside the rectangle: the four borders of A, and A's right border, behind which B's low-res pixels lie (the same surface)
    known["top_left"] = (0, 0, PARTIAL, dict(rect=3))
    known["bottom_right_of_B"] = (w - 1, h - 1, PARTIAL, dict(rect=3))
    known["across_the_view_border"] = (V - 1, 20 * s // 2 + s - 1, PARTIAL, dict(rect=2))
    known["across_the_view_border_from_B"] = (V, 20 * s // 2, PARTIAL, dict(rect=2))
    lo_hit, lo_pos = _records(lo_kind)
    hit, pos = _records(hi_kind)
    return dict(lo=dict(color=lo_color, hit=lo_hit, position=lo_pos), hi=dict(hit=hit, position=pos), rects=[(0, 0, V, V), (V, 0, V, V)],
                size=(w, h), params=dict(SYNTHETIC_PARAMS), known=known)


# ------------------------------------------------------------------ what the plane means: an analytic irradiance on real planes
MEANING_SIZE = (132, 60)


def irradiance(planes):
    """A smooth float64 function of position and normal, (h, w, 3); a miss (position and normal zero) gets the constant 0.5.
    Two terms, one for each guide the rule has.  0.5 + 0.5 * n, the normal as a colour: a crease between two faces of one mesh carries
    as much contrast as a silhouette does, so the normal and plane tests have something to protect that the mesh test does not.
    0.2 * sin(2 * M P), an oscillation inside every surface with a wavelength of about pi scene units, more than ten low-res pixels at
    scale 4 on two_box: bilinear interpolation follows it, wrong weights do not."""
    P = _f(planes["position"])[..., 0:3].astype(np.float64)
    n = _f(planes["hit"])[..., 5:8].astype(np.float64)
    M = np.array([[1.0, 0.3, 0.2], [0.2, 1.0, 0.4], [0.3, 0.2, 1.0]])
    return 0.5 + 0.5 * n + 0.2 * np.sin(2.0 * (P @ M))


def rms(a, b):
    d = np.asarray(a, np.float64)[..., 0:3] - np.asarray(b, np.float64)[..., 0:3]
    return float(np.sqrt((d * d).mean()))
