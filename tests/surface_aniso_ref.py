"""float32 NumPy evaluation of pt_surface_aniso_planes' arithmetic, written from the text of include/pt_amd.h alone; shared by
tests/test_surface_aniso_cabi.py and tests/test_gpu_surface_aniso.py.  A helper, not a test.  One rounding per operation, in the header's
order, no fused multiply-add; it never calls the kernel under test.  The pyramid, tex2D on a level, the rays and the float64 truth are
tests/surface_lod_ref.py's, the point lookup and the classification of a record tests/surface_ref.py's.

Two switches exist for the teeth of the quality check only and are no part of the interface: axis="minor" lays the taps along the minor
axis, force_n=1 sets N to 1 whatever the axis ratio is (which is the isotropic pass)."""
import numpy as np

import surface_lod_ref as SL
import surface_ref as S
from motion_ref import _cross, _dot

f32 = np.float32
SENTINEL = S.SENTINEL
PLANES = ("albedo", "texcoord", "footprint", "lod", "taps")
WORDS = {"albedo": 4, "texcoord": 2, "footprint": 4, "lod": 1, "taps": 1}
COUNTERS = ("hits", "stale", "textured", "minified", "anisotropic", "taps")


def tap_offsets(n):
    """o_i = (float)(2i + 1 - N) / (float)(2N), i = 0 .. N-1, float32"""
    i = np.arange(n)
    o = (2 * i + 1 - n).astype(f32) / f32(2 * n)
    assert o.dtype == f32
    return o


def surface_aniso_ref(hit, scene, verts, idx, rects, cams, pixels, max_aniso=8, scale=1.0, planes=PLANES, fill=SENTINEL, axis="major", force_n=None):
    """Arguments as surface_lod_ref.surface_lod_ref, and max_aniso in 1..16.  Returns {plane: uint32 bits of the whole plane, `fill` outside
    the set; hits, stale, textured, minified, anisotropic, taps_sum: int; kind, mesh: surface_ref's; n: (h, w) int, the taps per pixel}."""
    assert 1 <= int(max_aniso) <= 16 and axis in ("major", "minor")
    base = S.surface_ref(hit, scene, pixels, planes=("albedo", "texcoord"), fill=fill)
    hit = np.ascontiguousarray(hit)
    hit = hit.view(f32) if hit.dtype == np.uint32 else np.ascontiguousarray(hit, f32)
    h, w = hit.shape[:2]
    verts = np.ascontiguousarray(verts, f32).reshape(-1, 3)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    pixels = np.asarray(pixels, bool)
    Y, X = np.nonzero(pixels)
    n = len(Y)
    tex = base["kind"][Y, X] == 4
    rid = np.full(n, -1)
    for k, (x0, y0, wr, hr) in enumerate(rects):
        rid[(X >= x0) & (X < x0 + wr) & (Y >= y0) & (Y < y0 + hr)] = k
    assert (rid >= 0).all(), "a pixel of the set lies in no rectangle"
    R = np.asarray(rects, np.int64).reshape(-1, 4)[rid]
    x, y, wr, hr = (X - R[:, 0]).astype(f32), (Y - R[:, 1]).astype(f32), R[:, 2].astype(f32), R[:, 3].astype(f32)
    cam = np.asarray(cams, f32).reshape(-1, 12)[rid]
    rec = hit[Y, X]
    prim = np.where(tex, rec.view(np.int32)[:, 3], 0).astype(np.int64)
    tid = np.where(tex, scene["mesh_tex"][scene["tri_mesh"][prim]], -1)
    alb = base["albedo"][Y, X].view(f32).copy()
    fp = np.zeros((n, 4), f32)
    lod = np.zeros(n, f32)
    ntap = np.zeros(n, np.int64)
    minified = np.zeros(n, bool)
    scale = f32(scale)
    amax = f32(int(max_aniso))
    with np.errstate(all="ignore"):
        c = scene["uv"][prim]
        tri = idx[prim]
        p0, p1, p2 = verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]]
        eye = cam[:, 0:3]
        st = base["texcoord"][Y, X].view(f32)
        s, t = st[:, 0], st[:, 1]
        half, one5 = f32(0.5), f32(1.5)
        d_c, d_x, d_y = SL._rays(cam, x + half, y + half, wr, hr), SL._rays(cam, x + one5, y + half, wr, hr), SL._rays(cam, x + half, y + one5, wr, hr)
        e1, e2 = p1 - p0, p2 - p0
        nrm = _cross(e1, e2)
        nn, hgt = _dot(nrm, nrm), _dot(nrm, p0 - eye)
        t_c, t_x, t_y = hgt / _dot(nrm, d_c), hgt / _dot(nrm, d_x), hgt / _dot(nrm, d_y)
        P_c, P_x, P_y = d_c * t_c[:, None] + eye, d_x * t_x[:, None] + eye, d_y * t_y[:, None] + eye
        ok = (t_c > 0) & (t_x > 0) & (t_y > 0)
        d = []
        for P_r in (P_x, P_y):
            g = P_r - P_c
            du, dv = _dot(_cross(g, e2), nrm) / nn, _dot(_cross(e1, g), nrm) / nn
            d.append(du * (c[:, 2] - c[:, 0]) + dv * (c[:, 4] - c[:, 0]))
            d.append(du * (c[:, 3] - c[:, 1]) + dv * (c[:, 5] - c[:, 1]))
        foot = np.stack(d, -1)
        assert foot.dtype == f32
        fp[tex] = foot[tex]
        for k, px in enumerate(scene["textures"]):
            sel = np.nonzero(tex & (tid == k))[0]
            if not len(sel):
                continue
            Ht, Wt = px.shape
            Wf, Hf = f32(Wt), f32(Ht)
            f = foot[sel]
            rx = (f[:, 0] * Wf) * (f[:, 0] * Wf) + (f[:, 1] * Hf) * (f[:, 1] * Hf)
            ry = (f[:, 2] * Wf) * (f[:, 2] * Wf) + (f[:, 3] * Hf) * (f[:, 3] * Hf)
            xm = rx > ry
            okk = ok[sel]
            r_maj2, r_min2 = np.where(xm, rx, ry), np.where(xm, ry, rx)
            a_s, a_t = np.where(xm, f[:, 0], f[:, 2]), np.where(xm, f[:, 1], f[:, 3])
            if axis == "minor":
                a_s, a_t = np.where(xm, f[:, 2], f[:, 0]), np.where(xm, f[:, 3], f[:, 1])
            rho_maj = np.where(okk, np.sqrt(r_maj2), f32(np.inf)).astype(f32) * scale
            rho_min = np.sqrt(r_min2) * scale
            one = ~(rho_maj > f32(1.0)) | ~okk
            q = rho_maj / rho_min
            assert q.dtype == f32
            N = np.where(q <= amax, np.ceil(np.where(q <= amax, q, f32(1.0))), amax).astype(np.int64)
            N = np.where(one, 1, N)
            assert (N >= 1).all() and (N <= int(max_aniso)).all()
            if force_n is not None:
                N = np.full_like(N, int(force_n))
            rho = np.where(N == 1, rho_maj, rho_maj / N.astype(f32)).astype(f32)
            minified[sel] = rho_maj > f32(1.0)
            ntap[sel] = N
            Lm = SL.levels_of(Wt, Ht) - 1
            mips = SL.mip_levels(px)
            look = lambda lv, ss, tt: S.tex2d(px, ss, tt) if lv == 0 else SL.tex2d_level(mips[lv - 1], ss, tt)  # noqa: E731
            big = rho > f32(1.0)
            coarse = big & ~(rho < f32(1 << Lm))
            tri_ = big & ~coarse
            bits = rho.view(np.uint32)
            kk = ((bits >> 23) & 0xFF).astype(np.int64) - 127
            frac = ((bits & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(f32) - f32(1.0)
            assert not (tri_ & ((kk < 0) | (kk >= Lm))).any()
            lv = np.where(~big, 0, np.where(coarse, Lm, kk))
            lod[sel] = np.where(~big, f32(0), np.where(coarse, f32(Lm), kk.astype(f32) + frac)).astype(f32)
            ss, tt = s[sel], t[sel]

            def choice(m, level, si, ti):
                """the level choice of the pixels m (all of one kind and lower level) at (si, ti): (len, 4) float32"""
                if tri_[m][0]:
                    ck, cn = look(level, si, ti), look(level + 1, si, ti)
                    return ck + (cn - ck) * frac[m][:, None]
                return look(level, si, ti)

            for nt in np.unique(N):
                offs = tap_offsets(int(nt))
                for level in np.unique(lv[N == nt]):
                    for is_tri in (False, True):
                        m = np.nonzero((N == nt) & (lv == level) & (tri_ == is_tri))[0]
                        if not len(m):
                            continue
                        acc = None
                        for i in range(int(nt)):
                            if nt == 1:
                                si, ti = ss[m], tt[m]
                            else:
                                os_ = offs[i] * scale
                                si, ti = ss[m] + (os_ * a_s[m]), tt[m] + (os_ * a_t[m])
                            ci = choice(m, int(level), si, ti)
                            acc = ci if acc is None else acc + ci
                        out = acc if nt == 1 else acc / f32(int(nt))
                        assert out.dtype == f32
                        alb[sel[m], 0:3] = out[:, 0:3]
    res = {}
    full = dict(albedo=alb, texcoord=base["texcoord"][Y, X].view(f32), footprint=fp, lod=lod[:, None], taps=ntap.astype(f32)[:, None])
    for name in planes:
        res[name] = np.full((h, w, WORDS[name]), fill, np.uint32)
        res[name][Y, X] = np.ascontiguousarray(full[name], f32).view(np.uint32)
    for k in ("hits", "stale", "textured", "kind", "mesh"):
        res[k] = base[k]
    res["minified"] = int(minified.sum())
    res["anisotropic"] = int((ntap > 1).sum())
    res["taps_sum"] = int(ntap.sum())
    res["n"] = np.zeros((h, w), np.int64)
    res["n"][Y, X] = ntap
    return res


# ------------------------------------------------------------------ hand-made hit planes over small textures
# A 16 x 16 frame under the camera eye = 0, U = x, V = y, W = z (set as one view's camera row): the ray through (a, b) is
# (2a/16 - 1, 2b/16 - 1, 1), exactly.  A primitive with the vertices HAND_FP lies in the plane z = 1, facing the camera: every ray meets it at
# t = 1, a pixel step is 1/8 in x or y, and du/dx = dv/dy = 1/16, du/dy = dv/dx = 0 — all powers of two, so the footprint is the same at every
# pixel and exact: (ds_x, dt_x, ds_y, dt_y) = ((c2 - c0), (c3 - c1), (c4 - c0), (c5 - c1)) / 16.  The texcoords of a primitive therefore SET its
# rho_maj, rho_min and q; u, v of a record only move (s, t).  Texture 0 is 16 x 8 (Lm = 4), texture 1 is 5 x 3 (Lm = 2), texture 2 is 1 x 1.
HAND_W = HAND_H = 16
HAND_ROW = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], f32)
HAND_FP = [(-1, -1, 1), (1, -1, 1), (-1, 1, 1)]
HAND_GROUND = [(-4, -1, 0), (4, -1, 0), (0, -1, 8)]  # the plane y = -1: rows 0..6 see it, row 7's lower neighbour ray (b = 8.5) does not
HAND_BEHIND = [(-1, -1, -1), (1, -1, -1), (-1, 1, -1)]  # the plane z = -1: every t is -1
ABOVE_8 = float(np.nextafter(f32(8), f32(9)))
# name: (vertices, texcoords, texture or -1, N expected at max_aniso 8, N at 16, lod expected or None)
HAND_PRIMS = {
    "magnified": (HAND_FP, [(0, 0), (0.5, 0), (0, 0.5)], 0, 1, 1, 0.0),  # rho_maj 0.5
    "two": (HAND_FP, [(0, 0), (3, 0), (0, 4)], 0, 2, 2, 0.5),  # 3 / 2 = 1.5 -> 2; rho 1.5: k 0, frac 0.5
    "q_is_2": (HAND_FP, [(0, 0), (4, 0), (0, 4)], 0, 2, 2, 1.0),  # 4 / 2 = 2 exactly -> 2, not 3; rho 2
    "q_is_3": (HAND_FP, [(0, 0), (6, 0), (0, 4)], 0, 3, 3, 1.0),  # 6 / 2 = 3 exactly -> 3; rho 2: k 1, frac 0
    "q_is_8": (HAND_FP, [(0, 0), (8, 0), (0, 2)], 0, 8, 8, 0.0),  # 8 / 1 = max_aniso exactly: the ceil's branch; rho 1: level 0
    "q_above_8": (HAND_FP, [(0, 0), (ABOVE_8, 0), (0, 2)], 0, 8, 9, None),  # one ulp above 8: the cap at 8, ceil = 9 at 16
    "q_is_8_5": (HAND_FP, [(0, 0), (8.5, 0), (0, 2)], 0, 8, 9, None),  # rho 8.5 / 8 = 1.0625 at 8
    "rho_min_0": (HAND_FP, [(0, 0), (4, 0), (0, 0)], 0, 8, 16, 0.0),  # collinear texcoords (uv2 = uv0): ry = 0, q = +inf; rho 0.5: level 0
    "falls_to_0": (HAND_FP, [(0, 0), (6, 0), (0, 2)], 0, 6, 6, 0.0),  # rho_maj 6 is minified, rho = 6 / 6 = 1 is level 0
    "y_major": (HAND_FP, [(0, 0), (2, 0), (0, 16)], 0, 4, 4, 1.0),  # rho 8 along y, 2 along x: the taps span 0.75 of t and wrap
    "ground": (HAND_GROUND, [(0, 0), (4, 0), (2, 4)], 0, None, None, None),
    "behind": (HAND_BEHIND, [(0, 0), (3, 0), (0, 4)], 0, 1, 1, 4.0),  # ok false: one tap of the coarsest level
    "zero_area": (HAND_FP, [(0, 0), (6, 0), (0, 4)], 0, 1, 1, 4.0),  # collapsed onto a line by the test: n = 0, NaN footprint
    "five_by_three": (HAND_FP, [(0, 0), (16, 0), (0, 8)], 1, 4, 4, None),  # rho 5 and 1.5: q = 3.33 -> 4; rho 1.25: levels 0 and 1 of 3
    "five_by_three_ground": (HAND_GROUND, [(0, 0), (7, 0), (3, 9)], 1, None, None, None),
    "one_texel_5": (HAND_FP, [(0, 0), (40, 0), (0, 8)], 2, 5, 5, 0.0),  # rho 2.5 and 0.5 -> 5; rho 0.5
    "one_texel_coarsest": (HAND_FP, [(0, 0), (64, 0), (0, 32)], 2, 2, 2, 0.0),  # rho 4 / 2 = 2 > 1 with Lm = 0: the coarsest level is level 0
    "untextured": (HAND_FP, None, -1, 0, 0, 0.0),
}
HAND_COLLAPSED = [(-1, 0, 1), (1, 0, 1), (-1, 0, 1)]  # "zero_area" after the scale (1, 0, 0) and the translation (0, 0, 1)


def hand_made_model():
    """one mesh of one triangle per entry of HAND_PRIMS, in its order: primitive k is mesh k"""
    from optixpathtracer_amd import scenes

    rng = np.random.default_rng(11)
    m = scenes.Model()
    for k, (verts, uv, tex, *_) in enumerate(HAND_PRIMS.values()):
        mesh = scenes.TriangleMesh(np.array(verts, f32), np.array([[0, 1, 2]], np.uint32), scenes.Material(color=(0.1 + 0.04 * k, 0.5, 0.9 - 0.04 * k)))
        if uv is not None:
            mesh.texcoord = np.array(uv, f32)
            mesh.diffuseTextureID = tex
        m.meshes.append(mesh)
    m.textures = [scenes.Texture(rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)) for w, h in ((16, 8), (5, 3), (1, 1))]
    return m


def hand_made_hit():
    """(hit (16, 16, 8) float32, where: {name: bool (16, 16)}).  Rows 6 and 7 name the two ground primitives (row 7 is their horizon);
    elsewhere pixel number 16 * y + x names primitive (16 * y + x) % len(HAND_PRIMS), with u, v drawn in [0, 1) — the first record of every
    primitive sits at u = v = 0, so s = t = 0 and taps left of it wrap.  Then: misses, two stale indices, a NaN and an infinite barycentric."""
    rng = np.random.default_rng(12)
    names = list(HAND_PRIMS)
    n = len(names)
    hit = np.zeros((HAND_H, HAND_W, 8), f32)
    words = hit.view(np.int32)
    prim = (np.arange(HAND_W * HAND_H) % n).reshape(HAND_H, HAND_W)
    prim[6, :] = names.index("ground")
    prim[7, :] = np.where(np.arange(HAND_W) % 2, names.index("ground"), names.index("five_by_three_ground"))
    prim[6, 8:] = names.index("five_by_three_ground")
    uv = rng.random((HAND_H, HAND_W, 2)).astype(f32) * f32(0.5)
    uv[0, :, :] = 0  # the first record of every primitive (n > 16: row 1 holds the rest at random u, v)
    hit[..., 0], hit[..., 1:3] = 1.0, uv
    words[..., 3] = prim
    special = {"miss": ((0, 15), -1), "miss_2": ((9, 15), -7), "stale_ntri": ((1, 15), n), "stale_max": ((2, 15), 0x7FFFFFFF)}
    for (x, y), p in special.values():
        words[y, x, 3] = p
    hit[15, 3, 1], words[15, 3, 3] = np.nan, names.index("q_is_3")
    hit[15, 4, 2], words[15, 4, 3] = np.inf, names.index("y_major")
    where = {name: words[..., 3] == k for k, name in enumerate(names)}
    for name, ((x, y), _) in special.items():
        where[name] = np.zeros((HAND_H, HAND_W), bool)
        where[name][y, x] = True
    where["nan_u"], where["inf_v"] = np.zeros((HAND_H, HAND_W), bool), np.zeros((HAND_H, HAND_W), bool)
    where["nan_u"][15, 3] = where["inf_v"][15, 4] = True
    where["q_is_3"][15, 3] = where["y_major"][15, 4] = False
    return hit, where


def hand_made_verts(model):
    """the model's vertices (motion_ref.model_arrays) with "zero_area" collapsed onto a line, and the indices"""
    from motion_ref import model_arrays

    verts, idx = model_arrays(model)
    verts = np.array(verts, f32)
    k = list(HAND_PRIMS).index("zero_area")
    verts[idx[k]] = np.array(HAND_COLLAPSED, f32)
    return verts, idx


# ------------------------------------------------------------------ the inputs, checks and the figure the tests share (tests/test_surface_aniso_cabi.py measures and pins them)
W, H = 131, 59
GRAZING_CAMERA = dict(eye=(2.0, 0.35, -3.0), lookat=(0.0, 0.2, 0.5), up=(0.0, 1.0, 0.0), fovY=35.0)
# measured 0.19391 (rms 0.0122 anisotropic, 0.0627 isotropic, 3081 pixels, N >= 3 on 0.824 of them); the taps along the minor axis give 0.0809
# (1.290 x isotropic), N forced to 1 gives 0.0627 (1.000 x): see test_anisotropic_albedo_of_the_reference_is_closer_to_the_pixel_average.
# Under the non-grazing camera of tests/test_surface_lod_cabi.py (131 x 61): ratio 0.21688 (0.0125 against 0.0578, 2535 pixels), recorded only.
R_ANISO = 0.194


def ground_truth(c, w, h, q):
    """the 16 x 16 float64 supersample of the ground's texture over the pixels q"""
    Y, X = np.nonzero(q)
    tri, uv = c["verts"][c["idx"][0]], c["sc"]["uv"][0].reshape(3, 2)
    return SL.supersample64(c["sc"]["textures"][0], c["row"], w, h, X.astype(np.float64), Y.astype(np.float64), tri, uv, 16)


# ------------------------------------------------------------------ the hand-made inputs of the GPU test
def check_hand_made(n_plane, lod_plane, where, max_aniso):
    """every primitive of surface_aniso_ref.HAND_PRIMS that names an expected N (and lod) shows it on all of its pixels"""
    for name, (_, _, _, n8, n16, lod) in HAND_PRIMS.items():
        want = {8: n8, 16: n16}[max_aniso]
        on = where[name]
        assert on.sum() >= 10, name
        if want is not None:
            assert (n_plane[on] == want).all(), (name, max_aniso, np.unique(n_plane[on]).tolist(), want)
        if lod is not None and max_aniso == 8:
            assert (lod_plane[on] == f32(lod)).all(), (name, np.unique(lod_plane[on]).tolist(), lod)
    assert (n_plane[7] == 1).all() and (n_plane[6] >= 8).all(), ("rows 7 and 6", max_aniso)  # the horizon row: ok is false; the row above it: grazing, q between 8.x and 16.x
    for name in ("miss", "miss_2", "stale_ntri", "stale_max"):
        assert (n_plane[where[name]] == 0).all() and (lod_plane[where[name]] == 0).all(), name
