"""The stopping rule of adaptive sampling in float32 NumPy (include/pt_amd.h states it operation by operation): the checker of the policy.
tests/test_adaptive_cabi.py holds it against hand-made moments, tests/test_gpu_adaptive.py compares every decision of the kernel with it."""
import numpy as np


# ------------------------------------------------------------------ the stopping rule, transcribed
def block_slots(image, fill=0):
    """(h, w, ...) -> (nby * nbx, 64, ...): slot l of block by * nbx + bx is the pixel (8 bx + (l & 7), 8 by + (l >> 3)); `fill` outside the image."""
    h, w = image.shape[:2]
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    pad = np.full((nby * 8, nbx * 8) + image.shape[2:], fill, image.dtype)
    pad[:h, :w] = image
    rest = tuple(range(4, pad.ndim + 2))
    return pad.reshape((nby, 8, nbx, 8) + image.shape[2:]).transpose((0, 2, 1, 3) + rest).reshape((nby * nbx, 64) + image.shape[2:])


def butterfly(a):
    """for off = 32 .. 1: slot[l] += slot[l ^ off], float32, over the last axis of 64 slots"""
    idx = np.arange(64)
    a = a.astype(np.float32)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[:, idx ^ off]
    return a[:, 0]


def rule_sides(moments, blocks):
    """What the rule is built from, for the given block ids, as float32 arrays: n (the block's subframe count), V and M (the butterfly sums of
    the per-pixel variances and means) and N (the block's pixel count)."""
    f = np.float32
    h, w = moments.shape[:2]
    inside = block_slots(np.ones((h, w), bool), False)[blocks]
    mo = block_slots(np.ascontiguousarray(moments, np.float32))[blocks]
    n = mo[:, 0, 0].astype(f)
    with np.errstate(all="ignore"):
        m = (mo[:, :, 1] / n[:, None]).astype(f)
        q = (mo[:, :, 2] / n[:, None]).astype(f)
        mm = (m * m).astype(f)
        v = np.maximum(f(0), (q - mm).astype(f)).astype(f)
    m = np.where(inside, m, f(0)).astype(f)
    v = np.where(inside, v, f(0)).astype(f)
    return n, butterfly(v), butterfly(m), inside.sum(1).astype(f)


def stop_rule(moments, blocks, threshold, dark_floor, min_subframes, max_subframes):
    """True for the blocks (ids in `blocks`, all rendered by the call) that stop.  Every line is one float32 operation."""
    f = np.float32
    n, V, M, N = rule_sides(moments, blocks)
    fl = (f(dark_floor) * N).astype(f)
    B = (M + fl).astype(f)
    lhs = (V * N).astype(f)
    t2 = f(f(threshold) * f(threshold))
    n1 = (n - f(1)).astype(f)
    rhs = (t2 * n1).astype(f)
    rhs = (rhs * B).astype(f)
    rhs = (rhs * B).astype(f)
    stop = (n >= f(min_subframes)) & (lhs <= rhs)
    if max_subframes > 0:
        stop |= n >= f(max_subframes)
    return stop
