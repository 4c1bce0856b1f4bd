"""float32 NumPy evaluation of pt_copy_texture_mips_device's pyramid and pt_surface_lod_planes' arithmetic, written from the text of
include/pt_amd.h alone; shared by tests/test_surface_lod_cabi.py and tests/test_gpu_surface_lod.py.  A helper, not a test.  One rounding per
operation, in the header's order, no fused multiply-add; it never calls the kernel under test.  Everything scene-side comes from the
Model's host arrays (surface_ref.scene_arrays, motion_ref.model_arrays); the float64 half at the end (supersample, footprints from
neighbours) uses no expression of the header."""
import numpy as np

import motion_ref as M
import surface_ref as S
from gbuffer_ref import _row
from motion_ref import _cross, _dot

f32 = np.float32
SENTINEL = S.SENTINEL
PLANES = ("albedo", "texcoord", "footprint", "lod")
WORDS = {"albedo": 4, "texcoord": 2, "footprint": 4, "lod": 1}


# ------------------------------------------------------------------ the pyramid
def levels_of(w, h):
    return 1 + int(np.floor(np.log2(max(w, h))))


def layout(sizes):
    """sizes: [(w, h)].  Returns (dims (n, 4) uint32: w, h, levels, first texel of level 1; bytes)"""
    dims, at = [], 0
    for w, h in sizes:
        L = levels_of(w, h)
        dims.append((w, h, L, at))
        at += sum(max(1, w >> k) * max(1, h >> k) for k in range(1, L))
    return np.array(dims, np.uint32).reshape(-1, 4), 16 * at


def _reduce(S_):
    """level k (h_k, w_k, 4) float32 -> level k+1"""
    hk, wk = S_.shape[:2]
    wn, hn = max(1, wk >> 1), max(1, hk >> 1)
    i, j = np.arange(wn), np.arange(hn)
    i0, j0 = 2 * i, 2 * j
    i1, j1 = np.minimum(2 * i + 1, wk - 1), np.minimum(2 * j + 1, hk - 1)
    g = lambda jj, ii: S_[jj[:, None], ii[None, :]]  # noqa: E731
    out = ((g(j0, i0) + g(j0, i1)) + (g(j1, i0) + g(j1, i1))) * f32(0.25)
    assert out.dtype == f32 and out.shape == (hn, wn, 4)
    return out


def mip_levels(pixel):
    """pixel (H, W) uint32 RGBA8 -> [level 1, level 2, ...] as (h_k, w_k, 4) float32"""
    pixel = np.asarray(pixel, np.uint32)
    H, W = pixel.shape
    lv = np.stack([(pixel >> (8 * k)) & 0xFF for k in range(4)], -1).astype(f32) / f32(255.0)
    out = []
    for _ in range(1, levels_of(W, H)):
        lv = _reduce(lv)
        out.append(lv)
    return out


def pyramid(textures):
    """textures: [(H, W) uint32].  Returns (texels, 4) float32: pt_copy_texture_mips_device's memory"""
    parts = [lv.reshape(-1, 4) for px in textures for lv in mip_levels(px)]
    return np.ascontiguousarray(np.concatenate(parts), f32) if parts else np.zeros((0, 4), f32)


def tex2d_level(T_, s, t):
    """the header's tex2D text on a float level T_ (h_k, w_k, 4); s, t float32 (n,).  Returns (n, 4) float32."""
    H, W = T_.shape[:2]
    s, t = np.asarray(s, f32).reshape(-1), np.asarray(t, f32).reshape(-1)
    with np.errstate(all="ignore"):
        x, y = (s - np.floor(s)) * f32(W), (t - np.floor(t)) * f32(H)
        xB, yB = x - f32(0.5), y - f32(0.5)
        fi, fj = np.floor(xB), np.floor(yB)
        alpha = np.floor(((xB - fi) * f32(256.0)) + f32(0.5)) * f32(1.0 / 256.0)
        beta = np.floor(((yB - fj) * f32(256.0)) + f32(0.5)) * f32(1.0 / 256.0)
        ii = np.where(np.isfinite(fi), fi, f32(0)).astype(np.int64)
        jj = np.where(np.isfinite(fj), fj, f32(0)).astype(np.int64)
        i0, i1, j0, j1 = np.mod(ii, W), np.mod(ii + 1, W), np.mod(jj, H), np.mod(jj + 1, H)
        a, b = alpha[:, None], beta[:, None]
        one = f32(1.0)
        out = ((((one - a) * (one - b)) * T_[j0, i0] + (a * (one - b)) * T_[j0, i1]) + ((one - a) * b) * T_[j1, i0]) + (a * b) * T_[j1, i1]
    assert out.dtype == f32
    return out


# ------------------------------------------------------------------ the pass
def _rays(cam, a, b, wr, hr):
    dx = (f32(2.0) * (a / wr)) - f32(1.0)
    dy = (f32(2.0) * (b / hr)) - f32(1.0)
    return (cam[:, 3:6] * dx[:, None] + cam[:, 6:9] * dy[:, None]) + cam[:, 9:12]


def surface_lod_ref(hit, scene, verts, idx, rects, cams, pixels, scale=1.0, planes=PLANES, fill=SENTINEL):
    """hit: (h, w, 8) float32 or its bits; scene: surface_ref.scene_arrays(model); verts (V, 3) the CURRENT vertices, idx (T, 3) global
    (motion_ref.model_arrays); rects: [(x0, y0, wr, hr)], the views, or [(0, 0, w, h)]; cams: (len(rects), 12) rows eye, U, V, W;
    pixels: bool (h, w), the set the call processes.  Returns {plane: uint32 bits of the whole plane, `fill` outside the set;
    hits, stale, textured, minified: int; kind, mesh: surface_ref's; level: (h, w) int, -1 where untextured, the lower level read}."""
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
    level = np.full(n, -1)
    minified = np.zeros(n, bool)
    scale = f32(scale)
    with np.errstate(all="ignore"):
        c = scene["uv"][prim]
        tri = idx[prim]
        p0, p1, p2 = verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]]
        eye = cam[:, 0:3]
        st = base["texcoord"][Y, X].view(f32)
        s, t = st[:, 0], st[:, 1]
        half, one5 = f32(0.5), f32(1.5)
        d_c, d_x, d_y = _rays(cam, x + half, y + half, wr, hr), _rays(cam, x + one5, y + half, wr, hr), _rays(cam, x + half, y + one5, wr, hr)
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
        assert foot.dtype == f32 and P_c.dtype == f32 and nn.dtype == f32
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
            rho2 = np.where(ok[sel], np.where(rx > ry, rx, ry), f32(np.inf)).astype(f32)
            rho = np.sqrt(rho2) * scale
            assert rho.dtype == f32
            Lm = levels_of(Wt, Ht) - 1
            mips = mip_levels(px)
            look = lambda lv, q: S.tex2d(px, s[q], t[q]) if lv == 0 else tex2d_level(mips[lv - 1], s[q], t[q])  # noqa: E731
            big = rho > f32(1.0)
            minified[sel] = big
            level[sel[~big]] = 0  # level 0: the albedo is surface_ref's already
            coarse = big & ~(rho < f32(1 << Lm))
            q = sel[coarse]
            if len(q):
                alb[q, 0:3] = look(Lm, q)[:, 0:3]
                lod[q], level[q] = f32(Lm), Lm
            tri_ = big & ~coarse
            bits = rho.view(np.uint32)
            kk = ((bits >> 23) & 0xFF).astype(np.int64) - 127
            frac = ((bits & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(f32) - f32(1.0)
            for lv in range(Lm):
                m = tri_ & (kk == lv)
                q = sel[m]
                if not len(q):
                    continue
                ck, cn = look(lv, q), look(lv + 1, q)
                o = ck + (cn - ck) * frac[m][:, None]
                assert o.dtype == f32
                alb[q, 0:3] = o[:, 0:3]
                lod[q], level[q] = f32(lv) + frac[m], lv
            assert not (tri_ & ((kk < 0) | (kk >= Lm))).any()
    res = {}
    full = dict(albedo=alb, texcoord=base["texcoord"][Y, X].view(f32), footprint=fp, lod=lod[:, None])
    for name in planes:
        res[name] = np.full((h, w, WORDS[name]), fill, np.uint32)
        res[name][Y, X] = np.ascontiguousarray(full[name], f32).view(np.uint32)
    for k in ("hits", "stale", "textured", "kind", "mesh"):
        res[k] = base[k]
    res["minified"] = int(minified.sum())
    res["level"] = np.full((h, w), -1)
    res["level"][Y, X] = level
    return res


# ------------------------------------------------------------------ float64, no expression of the header
def camera_rays64(row, w, h, ax, ay):
    """float64 ray directions through image points (ax, ay) (pixel units, arrays) of a w x h image under the camera row (12,)"""
    row = np.asarray(row, np.float64)
    U, V, W = row[3:6], row[6:9], row[9:12]
    return np.multiply.outer(2 * ax / w - 1, U) + np.multiply.outer(2 * ay / h - 1, V) + W


def plane_uv64(row, w, h, ax, ay, tri, uv):
    """float64 texcoord where the ray through (ax, ay) meets the plane of the triangle tri (3, 3) with texcoords uv (3, 2); NaN behind the eye"""
    tri, uv = np.asarray(tri, np.float64), np.asarray(uv, np.float64)
    o = np.asarray(row, np.float64)[0:3]
    d = camera_rays64(row, w, h, np.asarray(ax, np.float64), np.asarray(ay, np.float64))
    nrm = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    with np.errstate(all="ignore"):
        tt = np.dot(tri[0] - o, nrm) / (d @ nrm)
    P = o + d * tt[..., None]
    # affine coordinates of P in the triangle by least squares on the 3 x 2 edge matrix
    E = np.stack([tri[1] - tri[0], tri[2] - tri[0]], -1)
    ab = (P - tri[0]) @ np.linalg.pinv(E).T
    out = uv[0] + ab[..., 0:1] * (uv[1] - uv[0]) + ab[..., 1:2] * (uv[2] - uv[0])
    out[~(tt > 0)] = np.nan
    return out


def texel_lookup64(pixel, st):
    """the wrapped RGBA8 texture at texcoords st (..., 2), bilinear between texel centres, float64 rgb in [0, 1] (no 8-bit weights)"""
    pixel = np.asarray(pixel, np.uint32)
    H, W = pixel.shape
    rgb = np.stack([(pixel >> (8 * k)) & 0xFF for k in range(3)], -1).astype(np.float64) / 255.0
    x, y = st[..., 0] * W - 0.5, st[..., 1] * H - 0.5
    i, j = np.floor(x), np.floor(y)
    a, b = (x - i)[..., None], (y - j)[..., None]
    i, j = i.astype(np.int64), j.astype(np.int64)
    g = lambda jj, ii: rgb[jj % H, ii % W]  # noqa: E731
    return (1 - b) * ((1 - a) * g(j, i) + a * g(j, i + 1)) + b * ((1 - a) * g(j + 1, i) + a * g(j + 1, i + 1))


def supersample64(pixel, row, w, h, X, Y, tri, uv, n=16):
    """the mean texture colour over pixel (X, Y)'s square, n x n points, float64: (len(X), 3)"""
    o = (np.arange(n) + 0.5) / n
    ox, oy = np.meshgrid(o, o)
    ax = X[:, None] + ox.reshape(-1)[None, :]
    ay = Y[:, None] + oy.reshape(-1)[None, :]
    st = plane_uv64(row, w, h, ax, ay, tri, uv)
    return texel_lookup64(pixel, st).mean(1)


def neighbour_footprints(texcoord, prim_plane, kind):
    """From a texcoord plane (h, w, 2) alone: where the right (lower) neighbour is a textured hit on the same primitive,
    texcoord[neighbour] - texcoord[p] in float64.  Returns (fx (h, w, 2), okx (h, w) bool, fy, oky)."""
    tc = np.asarray(texcoord, np.float64)
    h, w = prim_plane.shape
    t4 = kind == 4
    okx = np.zeros((h, w), bool)
    oky = np.zeros((h, w), bool)
    okx[:, :-1] = t4[:, :-1] & t4[:, 1:] & (prim_plane[:, :-1] == prim_plane[:, 1:])
    oky[:-1, :] = t4[:-1, :] & t4[1:, :] & (prim_plane[:-1, :] == prim_plane[1:, :])
    fx, fy = np.zeros((h, w, 2)), np.zeros((h, w, 2))
    fx[:, :-1] = tc[:, 1:] - tc[:, :-1]
    fy[:-1, :] = tc[1:, :] - tc[:-1, :]
    return fx, okx, fy, oky


# ------------------------------------------------------------------ the inputs, checks and figures the tests share (tests/test_surface_lod_cabi.py measures and pins them)
W, H = 131, 61
FOOT_MEASURED = 8.35e-7  # measured 8.345e-07 on footprints up to 0.157, see test_footprints_of_the_reference_are_the_neighbour_differences
FOOT_BOUND = 4 * FOOT_MEASURED
R_REF = 0.797  # measured 0.79705 (rms 0.0578 filtered, 0.0725 point, 2535 pixels), see test_filtered_albedo_of_the_reference_is_closer_to_the_pixel_average
_CPU_CASE = {}


def cpu_case(orc):
    """the textured scene's CPU-built planes with the reference's planes at footprint_scale 1 and 0"""
    if "c" not in _CPU_CASE:
        from geometry_cases import textured_case

        c = dict(textured_case(orc))
        c["verts"], c["idx"] = M.model_arrays(c["model"])
        c["row"] = _row(c["cam"], W / H)
        frame = np.ones((H, W), bool)
        c["lod"] = surface_lod_ref(c["hit"], c["sc"], c["verts"], c["idx"], [(0, 0, W, H)], [c["row"]], frame)
        c["point"] = surface_lod_ref(c["hit"], c["sc"], c["verts"], c["idx"], [(0, 0, W, H)], [c["row"]], frame, scale=0.0)
        c["surface"] = S.surface_ref(c["hit"], c["sc"], frame)
        _CPU_CASE["c"] = c
    return _CPU_CASE["c"]


def check_footprints(footprint, texcoord, prim, kind):
    """The footprint plane against the texcoord plane alone, float64: on pixels whose right (lower) neighbour is a textured hit on the same
    primitive, texcoord[neighbour] - texcoord[p] is the x (y) footprint.  Returns dict(err: the largest absolute difference per component;
    nx, ny: pixels compared; size: the largest |footprint| component compared)."""
    fx, okx, fy, oky = neighbour_footprints(texcoord, prim, kind)
    fp = np.asarray(footprint, np.float64)
    ex, ey = np.abs(fp[..., 0:2] - fx)[okx], np.abs(fp[..., 2:4] - fy)[oky]
    return dict(err=float(max(ex.max(), ey.max())), nx=int(okx.sum()), ny=int(oky.sum()), size=float(max(np.abs(fx[okx]).max(), np.abs(fy[oky]).max())))


def ground_pixels(mesh):
    """ground (mesh 0) pixels whose 3 x 3 hit neighbourhood lies on the ground mesh"""
    h, w = mesh.shape
    pad = np.pad(mesh, 1, mode="constant", constant_values=-1)
    q = np.ones((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            q &= pad[dy:dy + h, dx:dx + w] == 0
    return q


def rms_against(albedo_bits, truth, q):
    d = albedo_bits.view(f32)[..., :3][q].astype(np.float64) - truth
    return float(np.sqrt((d * d).mean()))
