"""What the NumPy references of the tiled passes (tests/motion_blur_ref.py, tests/dof_ref.py; bloom_ref.py for the first two) have in
common, written from the text of include/pt_amd.h alone: the exponent-bit test, the views' rectangles, the layout of T and N in the
scratch, the hash of the jitter, Z(depth) and the clamp.  A helper, not a test; it never calls the kernels under test.  float32 arrays and
float32 scalars, one rounding per operation."""
import numpy as np

f32 = np.float32
u32 = np.uint32
TILE = 16
SENTINEL = u32(0xA5A5A5A5)
FLT_MAX = np.finfo(f32).max


def finite(a):
    """the exponent-bit test"""
    return (np.ascontiguousarray(a, f32).view(u32) & u32(0x7F800000)) != u32(0x7F800000)


def rectangles(rects, h, w):
    """the views' rectangles (x0, y0, wr, hr), or the frame"""
    return [tuple(int(v) for v in r) for r in rects] if rects else [(0, 0, w, h)]


def layout(rects, h, w, texel_bytes):
    """(dims (nv, 4) uint32: tw, th, first texel of T, first of N; bytes)"""
    rs = rectangles(rects, h, w)
    dims = np.zeros((len(rs), 4), u32)
    at = 0
    for v, (_, _, wr, hr) in enumerate(rs):
        tw, th = (wr + TILE - 1) // TILE, (hr + TILE - 1) // TILE
        dims[v] = (tw, th, at, at + tw * th)
        at += 2 * tw * th
    return dims, texel_bytes * at


def hash32(x, y, seed):
    """the header's hash, in uint64 arithmetic masked to 32 bits"""
    M = np.uint64(0xFFFFFFFF)
    x, y = np.asarray(x, np.uint64), np.asarray(y, np.uint64)
    h = ((x * np.uint64(0x9E3779B1)) & M) ^ ((y * np.uint64(0x85EBCA77)) & M) ^ ((np.uint64(seed) * np.uint64(0xC2B2AE3D)) & M)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & M
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & M
    h ^= h >> np.uint64(16)
    return h.astype(u32)


def depth_z(d):
    d = np.ascontiguousarray(d, f32)
    with np.errstate(all="ignore"):
        return np.where((d > f32(1e-6)) & (d <= FLT_MAX), d, FLT_MAX).astype(f32)


def clamp01(x):
    with np.errstate(all="ignore"):
        x = np.where(x > 0, x, f32(0)).astype(f32)
        return np.where(x < 1, x, f32(1)).astype(f32)
