"""float32 NumPy evaluation of pt_lens_warp_planes' rule, written from the text of include/pt_amd.h alone; shared by
tests/test_lens_warp_cabi.py and tests/test_gpu_lens_warp.py.  A helper, not a test.  One rounding per operation, in the header's order, no
fused multiply-add; it never calls the kernel under test.  The float64 half at the end (pt_warp_matrix restated, the source point of a
pixel, the turned cameras) shares no code with the library."""
import numpy as np

import conftest  # noqa: F401  (puts the repository's root on sys.path)
import surface_ref as S
from edge_aa_ref import INPUTS, H, W, rms  # noqa: F401  (the inputs and the frame the image-space tests share)

f32 = np.float32
SENTINEL = S.SENTINEL
PLANES = ("out", "frame_rgba8")
WORDS = {"out": 4, "frame_rgba8": 1}
LENS_WORDS = 24  # center 0, inv_radius 2, k 4, warp 13, reserved 22


def lens_row(size, k=(0.0, 0.0, 0.0), center=None, radius=None, warp=None):
    """(24,) float32: a pt_lens_view as renderer.make_lens documents it, written here a second time"""
    w = float(size[0])
    kk = np.asarray(k, f32)
    kk = np.stack([kk] * 3) if kk.shape == (3,) else kk
    row = np.zeros(LENS_WORDS, f32)
    row[0:2] = (0.5 * w, 0.5 * float(size[1])) if center is None else center
    rad = np.broadcast_to(np.asarray(0.5 * w if radius is None else radius, f32), (2,))
    with np.errstate(divide="ignore"):
        row[2:4] = np.where(rad == 0, f32(0), f32(1.0) / rad)
    row[4:13] = kk.reshape(-1)
    row[13:22] = np.eye(3, dtype=f32).reshape(-1) if warp is None else np.asarray(warp, f32).reshape(-1)
    return row


def lens_table(lenses, nv):
    """(nv, 24) float32; None: k = 0 and the identity matrix for every view"""
    if lenses is None:
        t = np.zeros((nv, LENS_WORDS), f32)
        t[:, [13, 17, 21]] = 1.0
        return t
    t = np.stack([np.frombuffer(bytes(v), f32) if not isinstance(v, np.ndarray) else np.asarray(v, f32).reshape(-1) for v in lenses])
    assert t.shape == (nv, LENS_WORDS), t.shape
    return np.ascontiguousarray(t, f32)


def _finite(v):
    return (np.ascontiguousarray(v, f32).view(np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


def _cubic(t):
    w0 = ((f32(-0.5) * t + f32(1.0)) * t - f32(0.5)) * t
    w1 = ((f32(1.5) * t - f32(2.5)) * t) * t + f32(1.0)
    w2 = ((f32(-1.5) * t + f32(2.0)) * t + f32(0.5)) * t
    w3 = ((f32(0.5) * t - f32(0.5)) * t) * t
    return [w.astype(f32) for w in (w0, w1, w2, w3)]


def lens_warp_ref(color, rects, lenses, pixels, border=(0.0, 0.0, 0.0), bicubic=False, planes=("out",), fill=SENTINEL, orc=None):
    """color: (h, w, 4) float32 or its bits; rects: [(x0, y0, wr, hr)], the views, or [(0, 0, w, h)]; lenses: None or one record per
    rectangle (lens_row's, or _lib.LensView); pixels: bool (h, w), the set the call writes.  orc: the CPU checker, needed by "frame_rgba8"
    alone (its make_color).
    Returns {plane: uint32 bits of the whole plane, `fill` outside the set; pixels, outside, nonfinite: int; Y, X, rid: the set's pixels in
    order and their rectangles; inside (n, 3) bool; sx, sy (n, 3) float32: step 5's source point per channel (NaN where c > 0 failed);
    rgb (n, 3) float32}."""
    color = np.ascontiguousarray(color)
    color = color.view(f32) if color.dtype == np.uint32 else np.ascontiguousarray(color, f32)
    h, w = color.shape[:2]
    pixels = np.asarray(pixels, bool)
    Y, X = np.nonzero(pixels)
    n = len(Y)
    rid = np.full(n, -1)
    for k, (x0, y0, wr, hr) in enumerate(rects):
        rid[(X >= x0) & (X < x0 + wr) & (Y >= y0) & (Y < y0 + hr)] = k
    assert (rid >= 0).all(), "a pixel of the set lies in no rectangle"
    R = np.asarray(rects, np.int64).reshape(-1, 4)[rid] if n else np.zeros((0, 4), np.int64)
    x0, y0, wr, hr = R[:, 0], R[:, 1], R[:, 2], R[:, 3]
    x, y = X - x0, Y - y0
    fwr, fhr = wr.astype(f32), hr.astype(f32)
    L = lens_table(lenses, len(rects))[rid] if n else np.zeros((0, LENS_WORDS), f32)
    half, one, zero = f32(0.5), f32(1.0), f32(0.0)
    border = np.asarray(border, f32)
    rgb = np.zeros((n, 3), f32)
    inside = np.zeros((n, 3), bool)
    SX, SY = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    nonfinite = 0

    def tap(ch, use, tx_, ty_):
        """channel word ch at the tap (tx_, ty_) of the rectangle, clamped; 0 where not finite, counted where the channel is inside"""
        nonlocal nonfinite
        v = color[y0 + np.clip(ty_, 0, hr - 1), x0 + np.clip(tx_, 0, wr - 1), ch]
        bad = ~_finite(v)
        nonfinite += int((bad & use).sum())
        return np.where(bad, zero, v).astype(f32)

    with np.errstate(all="ignore"):
        for ch in range(3):
            # ---- 1 .. 3
            px, py = x.astype(f32) + half, y.astype(f32) + half
            qx, qy = px - L[:, 0], py - L[:, 1]
            ax, ay = qx * L[:, 2], qy * L[:, 3]
            r2 = ax * ax + ay * ay
            k1, k2, k3 = L[:, 4 + 3 * ch], L[:, 5 + 3 * ch], L[:, 6 + 3 * ch]
            g = r2 * (k1 + r2 * (k2 + r2 * k3))
            ux, uy = px + qx * g, py + qy * g
            # ---- 4, 5
            M = L[:, 13:22]
            a = (M[:, 0] * ux + M[:, 1] * uy) + M[:, 2]
            b = (M[:, 3] * ux + M[:, 4] * uy) + M[:, 5]
            c = (M[:, 6] * ux + M[:, 7] * uy) + M[:, 8]
            assert all(v.dtype == f32 for v in (g, ux, uy, a, b, c))
            pos = c > 0
            sx = np.where(pos, a / c, f32(np.nan)).astype(f32)
            sy = np.where(pos, b / c, f32(np.nan)).astype(f32)
            ins = pos & (sx >= 0) & (sx <= fwr) & (sy >= 0) & (sy <= fhr)
            SX[:, ch], SY[:, ch], inside[:, ch] = sx, sy, ins
            # ---- 6 (where the channel is outside the values are never used: 0 stands in)
            fx, fy = np.where(ins, sx, half) - half, np.where(ins, sy, half) - half
            flx, fly = np.floor(fx), np.floor(fy)
            ix, iy = flx.astype(np.int64), fly.astype(np.int64)
            tx, ty = (fx - flx).astype(f32), (fy - fly).astype(f32)
            if not bicubic:  # ---- 7
                wx, wy = [one - tx, tx], [one - ty, ty]
                c00, c10, c01, c11 = tap(ch, ins, ix, iy), tap(ch, ins, ix + 1, iy), tap(ch, ins, ix, iy + 1), tap(ch, ins, ix + 1, iy + 1)
                val = ((c00 * (wx[0] * wy[0]) + c10 * (wx[1] * wy[0])) + c01 * (wx[0] * wy[1])) + c11 * (wx[1] * wy[1])
            else:  # ---- 8
                wx, wy = _cubic(tx), _cubic(ty)
                rows = []
                for j in range(4):
                    cj = [tap(ch, ins, ix - 1 + i, iy - 1 + j) for i in range(4)]
                    rows.append(((cj[0] * wx[0] + cj[1] * wx[1]) + cj[2] * wx[2]) + cj[3] * wx[3])
                val = ((rows[0] * wy[0] + rows[1] * wy[1]) + rows[2] * wy[2]) + rows[3] * wy[3]
            assert val.dtype == f32
            rgb[:, ch] = np.where(ins, val, border[ch])  # ---- 9
    all_in = inside.all(1)
    res = {}
    if "out" in planes:
        res["out"] = np.full((h, w, 4), fill, np.uint32)
        res["out"][Y, X] = np.concatenate([rgb, all_in[:, None].astype(f32)], -1).view(np.uint32)
    if "frame_rgba8" in planes:
        import temporal_ref as T

        res["frame_rgba8"] = np.full((h, w, 1), fill, np.uint32)
        if n:
            res["frame_rgba8"][Y, X, 0] = T.make_color_bits(orc, np.ascontiguousarray(rgb))
    res.update(pixels=n, outside=int((~all_in).sum()), nonfinite=nonfinite, Y=Y, X=X, rid=rid, inside=inside, sx=SX, sy=SY, rgb=rgb)
    return res


# ------------------------------------------------------------------ float64, no code of the library
def warp_matrix64(src_row, dst_row, width, height):
    """pt_warp_matrix restated: (3, 3) float64, H = P [U V W]_src^-1 [U' V' W']_dst P^-1 (a linear solve, not an adjugate)"""
    s, d = np.asarray(src_row, np.float64), np.asarray(dst_row, np.float64)
    Ms, Md = s[3:12].reshape(3, 3).T, d[3:12].reshape(3, 3).T  # columns U, V, W
    P = np.array([[width / 2, 0, width / 2], [0, height / 2, height / 2], [0, 0, 1.0]])
    return P @ np.linalg.solve(Ms, Md) @ np.linalg.inv(P)


def source_point64(row, wr, hr, x, y, ch):
    """steps 1 to 5 in float64 for local pixels (x, y) (arrays) of a wr x hr rectangle under the lens row (24,), channel ch: (sx, sy, c)"""
    L = np.asarray(row, np.float64)
    px, py = np.asarray(x, np.float64) + 0.5, np.asarray(y, np.float64) + 0.5
    qx, qy = px - L[0], py - L[1]
    r2 = (qx * L[2]) ** 2 + (qy * L[3]) ** 2
    k1, k2, k3 = L[4 + 3 * ch:7 + 3 * ch]
    g = r2 * (k1 + r2 * (k2 + r2 * k3))
    u = np.stack([px + qx * g, py + qy * g, np.ones_like(px)])
    a, b, c = L[13:22].reshape(3, 3) @ u
    with np.errstate(all="ignore"):
        return a / c, b / c, c


def _rodrigues(v, axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.radians(deg)
    v = np.asarray(v, np.float64)
    return v * np.cos(t) + np.cross(axis, v) * np.sin(t) + axis * np.dot(axis, v) * (1 - np.cos(t))


def turned(cam, yaw=0.0, pitch=0.0, roll=0.0):
    """the camera dict turned about its own eye: yaw about its up vector, pitch about its right vector, roll about its view direction, degrees"""
    eye, look, up = (np.asarray(cam[k], np.float64) for k in ("eye", "lookat", "up"))
    fwd = look - eye
    fwd = _rodrigues(fwd, up, yaw)
    right = np.cross(fwd, up)
    fwd, up = _rodrigues(fwd, right, pitch), _rodrigues(up, right, pitch)
    up = _rodrigues(up, fwd, roll)
    return dict(cam, lookat=tuple(eye + fwd), up=tuple(up))


def affine_ramp(w, h, coef):
    """(h, w, 4) float32: channel ch is a * (i + 0.5) + b * (j + 0.5) + d at pixel (i, j) for coef[ch] = (a, b, d), evaluated in float64
    and rounded once; .w is 1"""
    i, j = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    out = np.ones((h, w, 4), f32)
    for ch, (a, b, d) in enumerate(coef):
        out[..., ch] = (a * i + b * j + d).astype(f32)
    return out


# ------------------------------------------------------------------ the figure the tests share (tests/test_lens_warp_cabi.py measures and pins it)
YAW = 3.0  # degrees: the late turn of the meaning tests
# R_WARP = rms(warp(A) - B) / rms(A - B) over the pixels with .w == 1, bilinear, A the pixel-centre albedo of the textured scene at 131 x 59
# on CPU-built planes, B the same under the camera turned YAW degrees in yaw: measured by
# test_warped_albedo_is_closer_to_the_turned_camera (test_lens_warp_cabi.py), whose line was
#   lens warp, 131 x 59, yaw 3.0: rms(A - B) 0.299504, ratio 0.31673; transposed matrix 1.97638, opposite yaw 1.32405; bound 0.6583;
#   outside 474 of 7729 (6.1 %)
# What is left of the error is the resampling of a texture with hard texel edges and the pixels whose surface the other camera sees at
# another place of a texel.  The two controls are measured over the right rule's inside pixels.
R_WARP = 0.3167
