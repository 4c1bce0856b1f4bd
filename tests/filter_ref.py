"""float32 NumPy evaluation of pt_filter_planes' arithmetic (include/pt_amd.h), shared by tests/test_filter_cabi.py and
tests/test_gpu_filter.py.  A helper, not a test.  One rounding per operation, in the header's order; it never calls the kernel under test.
pt_expf is restated here in float32 NumPy; make_color is the CPU checker's (temporal_ref.make_color_bits)."""
import numpy as np

from temporal_ref import SENTINEL, make_color_bits

f32 = np.float32
DEFAULTS = dict(iterations=5, sigma_lum=4.0, normal_cos=0.9, plane_eps=0.01, min_length=4)
# why a tap did not count: the first test it fails, in the header's order
REASONS = ("rect", "block", "inert", "mesh", "normal", "plane")
QNAN = 0x7FC00000


def canon(bits):
    """uint32 bits of `out` with every NaN of the variance word replaced by one pattern: the header leaves a NaN's sign and payload open
    (0 * inf is 0xffc00000 on x86 and 0x7fc00000 on the GPU), and only the variance can become one (an inf in, times a weight whose
    square underflowed).  The colour words are compared as they are."""
    bits = np.array(bits, np.uint32)
    v = bits[..., 3]
    v[((v & 0x7F800000) == 0x7F800000) & ((v & 0x007FFFFF) != 0)] = QNAN
    return bits


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _lum(c):
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def _f(a):
    a = np.ascontiguousarray(a)
    return a.view(f32) if a.dtype == np.uint32 else np.ascontiguousarray(a, f32)


def pt_expf(x):
    """include/pt_detmath.h's pt_expf on a float32 array, |x| <= 80: the truncating cast, the floor fix-up, the two-step range reduction,
    the polynomial in the header's association, the scale by bits"""
    x = np.asarray(x, f32)
    t = f32(1.44269504088896341) * x + f32(0.5)
    n = t.astype(np.int32)
    n = np.where(n.astype(f32) > t, n - 1, n).astype(np.int32)
    z = n.astype(f32)
    x = x - z * f32(0.693359375)
    x = x - z * f32(-2.12194440e-4)
    z = x * x
    z = (((((f32(1.9875691500e-4) * x + f32(1.3981999507e-3)) * x + f32(8.3334519073e-3)) * x + f32(4.1665795894e-2)) * x + f32(1.6666665459e-1)) * x
         + f32(5.0000001201e-1)) * z + x + f32(1.0)
    assert z.dtype == f32
    return z * ((n + 127).astype(np.uint32) << np.uint32(23)).view(f32)


def block_set_of(pixels):
    """the 8x8 blocks that hold a pixel of the set"""
    h, w = pixels.shape
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    pad = np.zeros((nby * 8, nbx * 8), bool)
    pad[:h, :w] = pixels
    return pad.reshape(nby, 8, nbx, 8).any((1, 3))


def filter_ref(orc, planes, rects, pixels, blocks=None, fill=SENTINEL, stages=False, **params):
    """planes: color (h, w, 4), hit (h, w, 8), position (h, w, 4), variance (h, w) or None, length (h, w) or None — float32 or their uint32
    bits.  rects: [(x0, y0, wr, hr)], the views, or [(0, 0, w, h)] without views.  pixels: bool (h, w), the set the call processes (each
    inside exactly one rectangle); blocks: bool (nby, nbx), the call's block set (default: the blocks that hold a pixel of the set).
    Returns {out: uint32 (h, w, 4), frame_rgba8: uint32 (h, w) — bits over the whole frame, `fill` outside the set; filtered, spatial: int;
    inert, spatial_px: bool (h, w); taps: {reason: int (h, w)}, per pixel the candidate taps of all stages (the 7x7 window where the pixel
    took the spatial estimate, 3x3 + 25 per pass; the pixel itself is no candidate) rejected for that reason; counted: int (h, w), those
    that counted; records: with stages=True the float32 (h, w, 4) records after every stage}."""
    prm = dict(DEFAULTS, **params)
    color, hit, pos = _f(planes["color"]), _f(planes["hit"]), _f(planes["position"])
    var = None if planes.get("variance") is None else _f(planes["variance"])
    length = None if planes.get("length") is None else _f(planes["length"])
    h, w = hit.shape[:2]
    pixels = np.asarray(pixels, bool)
    blocks = block_set_of(pixels) if blocks is None else np.asarray(blocks, bool)
    YY, XX = np.mgrid[0:h, 0:w]
    x0 = np.zeros((h, w), np.int64)
    y0, x1, y1 = x0.copy(), x0.copy(), x0.copy()
    seen = np.zeros((h, w), bool)
    for rx, ry, rw, rh in rects:
        assert not seen[ry:ry + rh, rx:rx + rw].any()
        seen[ry:ry + rh, rx:rx + rw] = True
        x0[ry:ry + rh, rx:rx + rw], y0[ry:ry + rh, rx:rx + rw], x1[ry:ry + rh, rx:rx + rw], y1[ry:ry + rh, rx:rx + rw] = rx, ry, rx + rw, ry + rh
    assert seen[pixels].all(), "a pixel of the set lies in no rectangle"
    words = hit.view(np.int32)
    c3 = color[..., 0:3]
    inert = (words[..., 3] < 0) | ~(((c3.view(np.uint32) & 0x7F800000) != 0x7F800000).all(-1))
    live_p = pixels & ~inert
    mesh, ng, P = words[..., 4], hit[..., 5:8], pos[..., 0:3]
    ncos = f32(prm["normal_cos"])
    taps = {r: np.zeros((h, w), np.int64) for r in REASONS}
    counted = np.zeros((h, w), np.int64)

    with np.errstate(all="ignore"):
        plane_max = f32(prm["plane_eps"]) * hit[..., 0]

        def tap(sx, sy, who):
            """(counts (h, w), qy, qx) for the tap q = p + (sx, sy) of the pixels `who`; books the reasons"""
            qx, qy = XX + sx, YY + sy
            alive = who.copy()
            if sx == 0 and sy == 0:
                return alive, YY, XX

            def drop(cond, why):
                nonlocal alive
                taps[why][alive & cond] += 1
                alive = alive & ~cond

            drop(~((qx >= x0) & (qx < x1) & (qy >= y0) & (qy < y1)), "rect")
            qx, qy = np.where(alive, qx, 0), np.where(alive, qy, 0)
            drop(~blocks[qy >> 3, qx >> 3], "block")
            drop(inert[qy, qx], "inert")
            drop(mesh[qy, qx] != mesh, "mesh")
            drop(~(_dot3(ng, ng[qy, qx]) >= ncos), "normal")
            drop(~(np.abs(_dot3(ng, P[qy, qx] - P)) <= plane_max), "plane")
            counted[alive] += 1
            return alive, qy, qx

        # ---- stage 0
        if var is None:
            spatial = live_p.copy()
            v_in = np.zeros((h, w), f32)
        else:
            spatial = live_p & (length < f32(prm["min_length"])) if length is not None else np.zeros((h, w), bool)
            v_in = np.where(var > 0, var, f32(0)).astype(f32)
        if spatial.any():
            n, s1, s2 = np.zeros((h, w), f32), np.zeros((h, w), f32), np.zeros((h, w), f32)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    ok, qy, qx = tap(dx, dy, spatial)
                    l = _lum(c3[qy, qx])
                    n = np.where(ok, n + f32(1), n)
                    s1 = np.where(ok, s1 + l, s1)
                    s2 = np.where(ok, s2 + l * l, s2)
            m = s1 / n
            est = s2 / n - m * m
            v_in = np.where(spatial, np.where(est > 0, est, f32(0)), v_in).astype(f32)
        rec = np.concatenate([c3, np.where(inert, f32(0), v_in)[..., None]], -1).astype(f32)
        records = [rec.copy()]
        # ---- the passes
        k3 = (f32(0.25), f32(0.5), f32(0.25))
        kern = (f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625))
        sigma = f32(prm["sigma_lum"])
        for it in range(int(prm["iterations"])):
            step = 1 << it
            r3, v = rec[..., 0:3], rec[..., 3]
            G, K = np.zeros((h, w), f32), np.zeros((h, w), f32)
            for j in range(3):
                for i in range(3):
                    kk = k3[j] * k3[i]
                    ok, qy, qx = tap(i - 1, j - 1, live_p)
                    G = np.where(ok, G + kk * v[qy, qx], G)
                    K = np.where(ok, K + kk, K)
            g = G / K
            den = sigma * np.sqrt(g) + f32(1e-6)
            lp = _lum(r3)
            S, V, W = np.zeros((h, w, 3), f32), np.zeros((h, w), f32), np.zeros((h, w), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    kk = kern[dy + 2] * kern[dx + 2]
                    ok, qy, qx = tap(step * dx, step * dy, live_p)
                    rq, vq = r3[qy, qx], v[qy, qx]
                    e = np.abs(lp - _lum(rq)) / den
                    e = np.where(e < f32(80), e, f32(80))
                    wgt = pt_expf(np.where(ok, -e, f32(0))) * kk
                    S = np.where(ok[..., None], S + rq * wgt[..., None], S)
                    V = np.where(ok, V + (wgt * wgt) * vq, V)
                    W = np.where(ok, W + wgt, W)
            for a in (g, den, S, V, W):
                assert a.dtype == f32
            new = np.concatenate([S / W[..., None], (V / (W * W))[..., None]], -1).astype(f32)
            rec = np.where(live_p[..., None], new, rec)
            records.append(rec.copy())
    res = {}
    res["out"] = np.full((h, w, 4), fill, np.uint32)
    res["out"][pixels] = rec.view(np.uint32)[pixels]
    res["frame_rgba8"] = np.full((h, w), fill, np.uint32)
    res["frame_rgba8"][pixels] = make_color_bits(orc, rec[..., 0:3][pixels])
    res["filtered"] = int(live_p.sum())
    res["spatial"] = int(spatial.sum())
    res["inert"] = inert
    res["spatial_px"] = spatial
    res["taps"] = taps
    res["counted"] = counted
    if stages:
        res["records"] = records
    return res


def tap_counts(ref):
    """({reason: rejected candidate taps}, counting taps) over the whole frame"""
    return {r: int(ref["taps"][r].sum()) for r in REASONS}, int(ref["counted"].sum())


# ------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
def random_planes(rng, h, w):
    """colour (h, w, 4) in [0, 1) with a few NaN and inf words, variance (h, w) around 1e-2 with NaN, negative and zero words (with_random_planes adds one inf: five passes spread it
    over a 125 x 125 window), lengths
    (h, w) 0..9 (whole numbers, about four in ten below the default min_length) with a few NaN words"""
    color = rng.random((h, w, 4), dtype=f32)
    k = max(2, h * w // 50)
    ys, xs, cs = rng.integers(0, h, k), rng.integers(0, w, k), rng.integers(0, 3, k)
    color[ys, xs, cs] = np.where(np.arange(k) % 3 == 0, f32(np.inf), np.where(np.arange(k) % 3 == 1, f32(-np.inf), f32(np.nan)))
    var = (rng.random((h, w), dtype=f32) * f32(0.02)).astype(f32)
    ys, xs = rng.integers(0, h, 9), rng.integers(0, w, 9)
    var[ys, xs] = np.array([np.nan, -1.0, 0.0] * 3, f32)
    length = rng.integers(0, 10, (h, w)).astype(f32)
    ys, xs = rng.integers(0, h, max(1, k // 4)), rng.integers(0, w, max(1, k // 4))
    length[ys, xs] = np.nan
    return color, var, length


def cpu_gbuffer(orc, model, size, cam_dict):
    """renderGBuffer's hit and position planes for `cam_dict`, built without a GPU (temporal_ref.cpu_planes)"""
    import temporal_ref as T

    p = T.cpu_planes(orc, model, size, cam_dict, cam_dict)
    return dict(hit=p["hit"], position=p["position"])


def real_inputs():
    """name -> (model factory, size, camera, parameters, seed of the random planes).  The two-box scene has flat faces of distinct meshes:
    its taps fail by mesh and normal, and no tap can fail the plane test at a practical plane_eps, so it runs with plane_eps = 0 (the lower
    end of the range: only a tap whose plane distance rounds to exactly zero survives); the terrain's plane rejections come at the default."""
    from optixpathtracer_amd import scenes

    return {
        "two_box": (lambda: scenes.two_box_scene(shadow_catcher=False), (131, 61), scenes.TWO_BOX_CAMERA, dict(plane_eps=0.0), 31),
        "terrain": (lambda: scenes.voxel_terrain(n=64, target_tris=20000), (131, 61), scenes.TERRAIN_CAMERA, dict(), 32),
    }


def with_random_planes(gb, seed):
    h, w = gb["hit"].shape[:2]
    color, var, length = random_planes(np.random.default_rng(seed), h, w)
    # the inf is put where it is used: on the hit pixel nearest the frame's centre whose colour is finite and whose length is long enough
    ok = (np.ascontiguousarray(gb["hit"]).view(np.int32)[..., 3] >= 0) & np.isfinite(color[..., :3]).all(-1) & (length >= 4)
    ys, xs = np.nonzero(ok)
    k = np.argmin((ys - h // 2) ** 2 + (xs - w // 2) ** 2)
    var[ys[k], xs[k]] = np.inf
    return dict(gb, color=color, variance=var, length=length)


def check_coverage(ref, what):
    """at least 10 % of the candidate taps count and at least 10 % are rejected; at least 10 % of the non-inert pixels take the spatial
    estimate and at least 10 % the given variance; returns (reason counts, counting taps, spatial, filtered)"""
    rej, cnt = tap_counts(ref)
    total = cnt + sum(rej.values())
    assert cnt * 10 >= total and (total - cnt) * 10 >= total, f"{what}: {cnt} of {total} candidate taps count"
    sp, fl = ref["spatial"], ref["filtered"]
    assert sp * 10 >= fl and (fl - sp) * 10 >= fl, f"{what}: {sp} of {fl} pixels take the spatial estimate"
    return rej, cnt, sp, fl


def synthetic_planes(w, h, seed):
    """Planes for a w x h frame made by hand, every reason on a known tap.  Surfaces in columns of three: mesh 0 on the plane z = 0 (t = 4),
    mesh 0 on z = 0.5 — with plane_eps = 0.125 the distance 0.5 lies EXACTLY on plane_eps * t, so these two count for each other —, mesh 1
    on z = 0, mesh 0 on z = 0 with the normal tilted to (0.6, 0, 0.8) (dot 0.8 < 0.9: `normal`; its plane distances to the others are not
    zero), mesh 0 on z = 1 (`plane`), and misses (`inert`); one NaN colour word (`inert`, on a hit).  Every pixel of the frame's border is a
    pixel on a rectangle edge (`rect`)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    kind = (xs // 3 + ys) % 6
    hit = np.zeros((h, w, 8), f32)
    words = hit.view(np.int32)
    miss = kind == 5
    hit[..., 0] = np.where(miss, f32(1e16), f32(4.0))
    words[..., 3] = np.where(miss, -1, xs + w * ys)
    words[..., 4] = np.where(miss, -1, np.where(kind == 2, 1, 0))
    hit[..., 5] = np.where(kind == 3, f32(0.6), f32(0))
    hit[..., 7] = np.where(miss, f32(0), np.where(kind == 3, f32(0.8), f32(1)))
    pos = np.zeros((h, w, 4), f32)
    pos[..., 0], pos[..., 1], pos[..., 3] = xs, ys, 1
    pos[..., 2] = np.choose(kind, [f32(0), f32(0.5), f32(0), f32(0), f32(1), f32(0)])
    pos[miss] = 0
    color = rng.random((h, w, 4), dtype=f32)
    if w * h > 4:
        color[h // 2, w // 2, 1] = np.nan
    var = (rng.random((h, w), dtype=f32) * f32(0.05)).astype(f32)
    length = rng.integers(0, 9, (h, w)).astype(f32)
    return dict(color=color, hit=hit, position=pos, variance=var, length=length)


SYNTHETIC_PARAMS = dict(plane_eps=0.125, iterations=6)


# ------------------------------------------------------------------ the chain end to end: G-buffer -> temporal -> moments -> filter
CHAIN = dict(size=(64, 48), frames=8, spp=1, reference_spp=256)


def moments_plane(colour, scale):
    """(lum, lum * lum, 0, 1) of colour.xyz * scale, float32"""
    c = _f(colour)[..., 0:3] * f32(scale)
    l = _lum(c)
    return np.stack([l, l * l, np.zeros_like(l), np.ones_like(l)], -1).astype(f32)


def chain_ref(orc, colours, hit, position, **filter_params):
    """The static-camera chain in NumPy.  colours: per frame k the accumulation buffer of a 1-spp launch at subframe k over zeros (the
    header's per-frame colour recipe: color_scale = k + 1).  Returns (history (h, w, 4) float32, the filter_ref result of the last frame,
    variance (h, w), length (h, w))."""
    import temporal_ref as T

    h, w = hit.shape[:2]
    rects, px = [(0, 0, w, h)], np.ones((h, w), bool)
    geo = dict(motion=np.zeros((h, w, 2), f32), hit=hit, position=position, prev_hit=hit, prev_position=position)
    hist, mom, ln = np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32), np.zeros((h, w), f32)
    for k, colour in enumerate(colours):
        a = T.temporal_ref(orc, dict(geo, color=colour, history_in=hist, length_in=ln), rects, px, color_scale=float(k + 1))
        b = T.temporal_ref(orc, dict(geo, color=moments_plane(colour, k + 1), history_in=mom, length_in=ln), rects, px)
        assert np.array_equal(a["length_out"], b["length_out"])
        hist, mom, ln = a["history_out"].view(f32), b["history_out"].view(f32), a["length_out"].view(f32)
    with np.errstate(all="ignore"):
        d = mom[..., 1] - mom[..., 0] * mom[..., 0]
        var = np.where(d > 0, d, f32(0)).astype(f32)
    ref = filter_ref(orc, dict(color=hist, hit=hit, position=position, variance=var, length=ln), rects, px, **filter_params)
    return hist, ref, var, ln


def rms(image, reference):
    d = _f(image)[..., 0:3].astype(np.float64) - _f(reference)[..., 0:3].astype(np.float64)
    return float(np.sqrt((d * d).mean()))
