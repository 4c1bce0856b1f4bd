"""float32 NumPy evaluation of pt_temporal_accumulate's arithmetic (include/pt_amd.h), shared by tests/test_temporal_cabi.py and
tests/test_gpu_temporal.py.  A helper, not a test.  One rounding per operation, in the header's order; it never calls the kernel under test.
make_color is the CPU checker's (oracle.orc, 'det' mode: pinned to the device function by the parity tests)."""
import numpy as np

f32 = np.float32
SENTINEL = 0xA5A5A5A5
OUTPUTS = ("history_out", "length_out", "frame_rgba8", "copy_out")
DEFAULTS = dict(color_scale=1.0, normal_cos=0.9, plane_eps=0.01, min_weight=0.25, max_history=32, clear=False)

# why a tap did not count (the first test it fails, in the header's order), or why a pixel with counting taps is still invalid
REASONS = ("rect", "nolookup", "length", "history", "miss", "mesh", "normal", "plane", "min_weight")
# rect: the tap (or the whole lookup) lies outside the pixel's rectangle; nolookup: a NaN motion word, or a tap of weight zero;
# length: length_in < 1; history: a non-finite colour word; miss: a miss against a hit (either way); mesh / normal / plane: the three
# geometry tests of a hit; min_weight: taps count but Wsum < min_weight
BIT = {r: 1 << k for k, r in enumerate(REASONS)}


def make_color_bits(orc, rgb):
    """(n, 3) float32 -> (n,) uint32 through the CPU checker's make_color"""
    rgb = np.ascontiguousarray(rgb, f32).reshape(-1, 3)
    out = np.empty(len(rgb), np.uint32)
    fn = orc.lib.orc_make_color
    for k in range(len(rgb)):
        out[k] = fn(rgb[k])
    return out


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _f(a):
    a = np.ascontiguousarray(a)
    return a.view(f32) if a.dtype == np.uint32 else np.ascontiguousarray(a, f32)


def temporal_ref(orc, planes, rects, pixels, fill=SENTINEL, **params):
    """planes: color (h, w, 4), motion (h, w, 2), hit (h, w, 8), position (h, w, 4), prev_hit, prev_position, history_in (h, w, 4), length_in
    (h, w) — float32 or their uint32 bits.  rects: [(x0, y0, wr, hr)], the views, or [(0, 0, w, h)] without views.  pixels: bool (h, w), the
    set the call processes (each inside exactly one rectangle).  Returns {history_out, length_out, frame_rgba8, copy_out, color: uint32 bits
    of the whole plane, `fill` (for color: the input) outside the set; reprojected: int; valid: bool (h, w); reason: uint16 (h, w), bits BIT}."""
    prm = dict(DEFAULTS, **params)
    P = {k: _f(v) for k, v in planes.items()}
    h, w = P["length_in"].shape
    pixels = np.asarray(pixels, bool)
    Y, X = np.nonzero(pixels)
    n = len(Y)
    rid = np.full(n, -1)
    for k, (x0, y0, wr, hr) in enumerate(rects):
        inside = (X >= x0) & (X < x0 + wr) & (Y >= y0) & (Y < y0 + hr)
        assert (rid[inside] == -1).all()
        rid[inside] = k
    assert (rid >= 0).all(), "a pixel of the set lies in no rectangle"
    R = np.asarray(rects, np.int64).reshape(-1, 4)[rid]
    x0, y0, wr, hr = R[:, 0], R[:, 1], R[:, 2], R[:, 3]
    x, y = X - x0, Y - y0
    scale = f32(prm["color_scale"])
    c = P["color"][Y, X, 0:3] * scale
    hitw = P["hit"][Y, X].view(np.int32)
    prim_p, mesh_p = hitw[:, 3], hitw[:, 4]
    t_p, ng_p = P["hit"][Y, X, 0], P["hit"][Y, X, 5:8]
    pos_p = P["position"][Y, X, 0:3]
    reason = np.zeros(n, np.uint16)
    with np.errstate(all="ignore"):
        mv = P["motion"][Y, X]
        px, py = x.astype(f32) + mv[:, 0], y.astype(f32) + mv[:, 1]
        ok = (px >= f32(-1)) & (px <= wr.astype(f32)) & (py >= f32(-1)) & (py <= hr.astype(f32))
        nan = np.isnan(px) | np.isnan(py)
        reason[~ok & nan] |= BIT["nolookup"]
        reason[~ok & ~nan] |= BIT["rect"]
        pxs, pys = np.where(ok, px, f32(0)), np.where(ok, py, f32(0))
        flx, fly = np.floor(pxs), np.floor(pys)
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        fx, fy = pxs - flx, pys - fly
        wx, wy = [f32(1) - fx, fx], [f32(1) - fy, fy]
        assert fx.dtype == f32 and c.dtype == f32
        plane_max = f32(prm["plane_eps"]) * t_p
        wt, ht, cnt = [], [], []
        nprev = np.full(n, np.inf, f32)
        for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
            wij = wx[i] * wy[j]
            tx, ty = ix + i, iy + j
            live = ok.copy()

            def drop(cond, why):
                nonlocal live
                reason[live & cond] |= BIT[why]
                live = live & ~cond

            drop(~((tx >= 0) & (tx < wr) & (ty >= 0) & (ty < hr)), "rect")
            drop(~(wij > 0), "nolookup")
            qx, qy = np.where(live, x0 + tx, 0), np.where(live, y0 + ty, 0)
            ln = P["length_in"][qy, qx]
            drop(~(ln >= f32(1)), "length")
            hq = P["history_in"][qy, qx, 0:3]
            drop(~(((hq.view(np.uint32) & 0x7F800000) != 0x7F800000).all(-1)), "history")
            qw = P["prev_hit"][qy, qx].view(np.int32)
            pmiss, qmiss = prim_p < 0, qw[:, 3] < 0
            drop((pmiss & ~qmiss) | (~pmiss & qmiss), "miss")
            ishit = ~pmiss
            drop(ishit & (qw[:, 4] != mesh_p), "mesh")
            drop(ishit & ~(_dot3(ng_p, P["prev_hit"][qy, qx, 5:8]) >= f32(prm["normal_cos"])), "normal")
            d = P["prev_position"][qy, qx, 0:3] - pos_p
            drop(ishit & ~(np.abs(_dot3(ng_p, d)) <= plane_max), "plane")
            wt.append(np.where(live, wij, f32(0)))
            ht.append(np.where(live[:, None], wij[:, None] * hq, f32(0)))
            nprev = np.where(live, np.minimum(nprev, ln), nprev)
            cnt.append(live)
        wsum = ((wt[0] + wt[1]) + wt[2]) + wt[3]
        hsum = ((ht[0] + ht[1]) + ht[2]) + ht[3]
        anyc = cnt[0] | cnt[1] | cnt[2] | cnt[3]
        valid = anyc & (wsum >= f32(prm["min_weight"]))
        reason[anyc & ~valid] |= BIT["min_weight"]
        reason[valid] = 0
        H = hsum / wsum[:, None]
        nn = np.minimum(nprev, f32(prm["max_history"] - 1))
        a = f32(1) / (nn + f32(1))
        blended = H + (c - H) * a[:, None]
        out = np.where(valid[:, None], blended, c).astype(f32)
        ln_out = np.where(valid, nn + f32(1), f32(1)).astype(f32)
    for arr in (wsum, hsum, H, a, blended):
        assert arr.dtype == f32
    res = {}
    o4 = np.concatenate([out, np.ones((n, 1), f32)], 1).view(np.uint32)
    for name in ("history_out", "copy_out"):
        res[name] = np.full((h, w, 4), fill, np.uint32)
        res[name][Y, X] = o4
    res["length_out"] = np.full((h, w), fill, np.uint32)
    res["length_out"][Y, X] = ln_out.view(np.uint32)
    res["frame_rgba8"] = np.full((h, w), fill, np.uint32)
    res["frame_rgba8"][Y, X] = make_color_bits(orc, out)
    res["color"] = P["color"].view(np.uint32).copy()
    if prm["clear"]:
        res["color"][Y, X] = 0
    res["reprojected"] = int(valid.sum())
    res["valid"] = np.zeros((h, w), bool)
    res["valid"][Y, X] = valid
    res["reason"] = np.zeros((h, w), np.uint16)
    res["reason"][Y, X] = reason
    return res


def reason_counts(ref, pixels):
    """{reason: pixels of the set, invalid, that show it}"""
    inv = np.asarray(pixels, bool) & ~ref["valid"]
    return {r: int(((ref["reason"][inv] & BIT[r]) != 0).sum()) for r in REASONS}


def random_history(rng, h, w):
    """history (h, w, 4) and lengths (h, w) 0..9 with about one zero in six, a few NaN and inf colour words"""
    hist = rng.random((h, w, 4), dtype=f32)
    hist[..., 3] = 1
    ln = rng.integers(0, 10, (h, w)).astype(f32)
    ln[rng.random((h, w)) < 0.08] = 0
    k = max(2, h * w // 50)
    ys, xs, cs = rng.integers(0, h, k), rng.integers(0, w, k), rng.integers(0, 3, k)
    hist[ys, xs, cs] = np.where(np.arange(k) % 3 == 0, f32(np.inf), np.where(np.arange(k) % 3 == 1, f32(-np.inf), f32(np.nan)))
    return hist, ln


def cpu_planes(orc, model, size, cam_dict, prev_dict):
    """The planes renderGBuffer gives for `cam_dict` (motion against `prev_dict`) and for `prev_dict`, built without a GPU: the CPU checker's
    trace_closest for (t, prim), float32 NumPy for position and motion (the G-buffer formulas of the header, tests/gbuffer_ref.py), the
    mesh from the primitive's place in mesh order, ng = normalize3(cross3(v1 - v0, v2 - v0)).  Good for counting which pixels reproject and
    why the others do not; the GPU tests take their planes from renderGBuffer."""
    import gbuffer_ref as G

    w, h = size
    sc = orc.make_scene(model, use_bvh=True)
    tri_mesh = np.concatenate([np.full(len(m.index), k, np.int32) for k, m in enumerate(model.meshes)])
    tris = np.concatenate([np.asarray(m.vertex, f32)[np.asarray(m.index).reshape(-1, 3)] for m in model.meshes])  # (T, 3, 3)
    nrm = G._normalize(G._cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]))

    def one(cd, pd):
        row, prev = G._row(cd, w / h), G._row(pd, w / h)
        rays = G._np_rays(row, w, h)
        t, prim = orc.trace_closest(sc, rays.reshape(-1, 8))
        t, prim = np.asarray(t, f32).reshape(h, w), np.asarray(prim, np.int32).reshape(h, w)
        hit = prim >= 0
        _, position, motion, _ = G._np_planes(rays, t, hit, row, prev)
        rec = np.zeros((h, w, 8), f32)
        rec[..., 0] = t
        words = rec.view(np.int32)
        words[..., 3] = prim
        words[..., 4] = np.where(hit, tri_mesh[np.maximum(prim, 0)], -1)
        rec[..., 5:8] = np.where(hit[..., None], nrm[np.maximum(prim, 0)], f32(0))
        return dict(hit=rec, position=position.view(f32), motion=motion.view(f32))

    cur, prv = one(cam_dict, prev_dict), one(prev_dict, prev_dict)
    return dict(motion=cur["motion"], hit=cur["hit"], position=cur["position"], prev_hit=prv["hit"], prev_position=prv["position"])


# ------------------------------------------------------------------ the real-plane inputs of tests/test_gpu_temporal.py
def forward(cam_dict, f, dx=0.25):
    """gbuffer_ref._moved (the eye shifted by dx in x) after a dolly of the eye by the fraction f towards the look-at point: the
    current frame then sees more than the previous one did (lookups leave the image), parallax disoccludes, and for f large enough the
    nearest surface points lie behind the previous camera (NaN motion)."""
    e, l = np.asarray(cam_dict["eye"], np.float64), np.asarray(cam_dict["lookat"], np.float64)
    ex, ey, ez = e + f * (l - e)
    return dict(cam_dict, eye=(float(ex) + dx, float(ey), float(ez)))


def real_inputs():
    """name -> (model factory, size, current camera, previous camera, parameters, history seed).  The two-box scene has flat faces of
    distinct meshes only, so no tap can fail the plane test at a practical plane_eps: it runs with plane_eps = 0 (the lower end of the
    range: only a tap whose plane distance rounds to exactly zero survives); misses keep more than 10 % of its pixels valid."""
    from optixpathtracer_amd import scenes

    return {
        "two_box": (lambda: scenes.two_box_scene(shadow_catcher=False), (131, 61), scenes.TWO_BOX_CAMERA, forward(scenes.TWO_BOX_CAMERA, 0.65),
                    dict(plane_eps=0.0), 11),
        "terrain": (lambda: scenes.voxel_terrain(n=64, target_tris=20000), (131, 61), scenes.TERRAIN_CAMERA, forward(scenes.TERRAIN_CAMERA, 0.5),
                    dict(), 12),
    }


def with_random_history(planes, seed):
    """adds color, history_in and length_in (random_history) to a dict of G-buffer planes"""
    h, w = planes["motion"].shape[:2]
    rng = np.random.default_rng(seed)
    hist, ln = random_history(rng, h, w)
    color = rng.random((h, w, 4), dtype=f32)
    return dict(planes, color=color, history_in=hist, length_in=ln)


def check_coverage(ref, pixels, what):
    """at least 10 % of the pixels valid, at least 10 % invalid, every rejection reason at least once; returns (valid, invalid, counts)"""
    n = int(np.asarray(pixels, bool).sum())
    valid = ref["reprojected"]
    counts = reason_counts(ref, pixels)
    assert valid * 10 >= n, f"{what}: only {valid} of {n} pixels are valid"
    assert (n - valid) * 10 >= n, f"{what}: only {n - valid} of {n} pixels are invalid"
    assert all(counts[r] > 0 for r in REASONS), f"{what}: a rejection reason does not occur: {counts}"
    return valid, n - valid, counts


def synthetic_planes(w, h, seed):
    """Planes for a w x h frame made by hand.  Surfaces in bands: mesh 0 on the plane z = 0, mesh 0 on z = 1 (fails the plane test against
    the first), mesh 1 on z = 0, and misses; previous planes = current planes; a random history without holes.  Motion is crafted so that px (and
    py, in another order) take, pixel after pixel, the values -1, wr, x (zero motion: fx = 0), x + 1, -0.5 and wr - 0.5 (one tap column
    outside the rectangle), x + 0.25, -1.5 and wr + 0.5 (just past either end of the accepted range), x - 0.75, wr - 1 and 0.  All are
    exact in float32, and so is (float)x + motion."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    kind = (xs // 3 + ys) % 4
    hit = np.zeros((h, w, 8), f32)
    words = hit.view(np.int32)
    hit[..., 0] = np.where(kind == 3, f32(1e16), f32(4.0))
    words[..., 3] = np.where(kind == 3, -1, xs + w * ys)
    words[..., 4] = np.where(kind == 3, -1, np.where(kind == 2, 1, 0))
    hit[..., 7] = np.where(kind == 3, f32(0), f32(1))
    pos = np.zeros((h, w, 4), f32)
    pos[..., 0], pos[..., 1], pos[..., 2], pos[..., 3] = xs, ys, np.where(kind == 1, f32(1), f32(0)), 1
    pos[kind == 3] = 0

    def crafted(c, size, k):
        c = c.astype(f32)
        s = np.full(c.shape, size, f32)
        table = [0 * c - 1, s, c, c + 1, 0 * c - f32(0.5), s - f32(0.5), c + f32(0.25), 0 * c - f32(1.5), s + f32(0.5), c - f32(0.75), s - 1, 0 * c]
        return (np.choose(k % 12, table) - c).astype(f32)

    k = xs + w * ys
    motion = np.stack([crafted(xs, w, k), crafted(ys, h, 5 * k + 3)], -1)
    return dict(color=rng.random((h, w, 4), dtype=f32), motion=motion, hit=hit, position=pos, prev_hit=hit, prev_position=pos,
                history_in=rng.random((h, w, 4), dtype=f32), length_in=rng.integers(1, 9, (h, w)).astype(f32))
