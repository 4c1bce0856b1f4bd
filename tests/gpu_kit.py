"""What the tests marked `gpu` share: planes that go up (upload), sentinel-filled planes that come back (filled, bits, bits3), the
word-for-word comparison (differ, same), pixel sets (pixel_mask, whole_frame_mask, whole_frame), a renderer for the image-space passes
(plane_renderer) and the loaded HIP runtime.  Imports torch; differ, same and the pixel sets need no GPU.  The per-pass word tables stay
with the pass: the caller turns a plane's name into a shape (plane_shape) and a dtype.  pytest does not rewrite the asserts of this module,
so each carries its own message."""
import ctypes as C

import numpy as np
import torch

import conftest  # noqa: F401  (puts the repository's root on sys.path)
from optixpathtracer_amd import renderer as R

f32 = np.float32
SENTINEL = 0xA5A5A5A5


def to_numpy(t):
    return t.cpu().numpy()


def bits(t):
    """a tensor's words, in its own shape"""
    return t.cpu().numpy().view(np.uint32)


def bits3(t):
    """a plane's words as (h, w, words per pixel), also where the plane is (h, w)"""
    a = bits(t)
    return a.reshape(a.shape[0], a.shape[1], -1)


def upload(a, offset=False):
    """a float32 array as a CUDA tensor; offset: one float into its allocation (4-byte aligned only)"""
    a = np.array(a, f32)  # (a copy: the shared planes are read-only)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda:0")
    t = (buf[1:] if offset else buf[:-1]).view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 if offset else 0), f"upload: {tuple(a.shape)} lies at {t.data_ptr():#x}, offset={offset}"
    return t


def plane_shape(h, w, words):
    return (h, w) if words == 1 else (h, w, words)


def filled(shape, offset=False, dtype=torch.float32):
    """a plane of 4-byte words, every byte 0xA5; offset: one word into its allocation (4-byte aligned only).  dtype=torch.int32 is the
    form of a frame_rgba8 plane."""
    n = int(np.prod(shape))
    buf = torch.full((4 * (n + 1),), 0xA5, dtype=torch.uint8, device="cuda:0").view(torch.float32)
    t = (buf[1:] if offset else buf[:-1]).view(tuple(shape))
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 if offset else 0), f"filled: {tuple(shape)} lies at {t.data_ptr():#x}, offset={offset}"
    return t if dtype == torch.float32 else t.view(dtype)


def differ(a, b):
    """where two planes differ.  float32 planes are compared as bits, except that two NaNs are equal whatever their payloads (the header
    specifies none); every other dtype (packed pixels, words, records of integers, a block mask) is compared as it is.  +0 and -0 differ:
    this is deliberately not conftest.assert_bits_equal, which calls them equal for the renderer's own buffers."""
    if a.dtype != f32:
        return a != b
    a, b = a.view(np.uint32), b.view(np.uint32)
    with np.errstate(all="ignore"):
        return (a != b) & ~(np.isnan(a.view(f32)) & np.isnan(b.view(f32)))


def words_differ(a, b):
    """differ for the uint32 words of two float32 planes"""
    return differ(a.view(f32), b.view(f32))


def same(got, ref, what):
    """every plane of `got` has its reference's shape and differs from it (differ) nowhere"""
    for name, a in got.items():
        b = ref[name]
        assert a.shape == b.shape, f"{what}: {name} has shape {a.shape}, the reference {b.shape}"
        neq = differ(a, b)
        assert not neq.any(), f"{what}: {name} differs in {int(neq.sum())} words, first at {np.argwhere(neq)[:3].tolist()}"


def same_words(got, ref, what):
    """same for {name: uint32 words}: every plane of `got` as float32 (NaN-aware), but the packed pixels (frame_rgba8) as they are"""
    as_planes = lambda d: {n: d[n] if n == "frame_rgba8" else d[n].view(f32) for n in got}  # noqa: E731
    same(as_planes(got), as_planes(ref), what)


def pixel_mask(block_mask, *, h, w):
    """the (h, w) pixel set of a mask of 8 x 8 blocks"""
    return np.repeat(np.repeat(block_mask, 8, 0), 8, 1)[:h, :w]


def whole_frame_mask(h, w):
    return np.ones((h, w), bool)


def whole_frame(w, h):
    """(rects, pixel set) of one view that covers the frame"""
    return [(0, 0, w, h)], np.ones((h, w), bool)


def plane_renderer(model, size, cam_dict, partition=None):
    r = R.SampleRenderer(model)
    if partition:
        r.setPartition(*partition)
    r.resize(size)
    r.setCamera(R.make_camera(cam_dict, size[0] / size[1]))
    return r


def hip_runtime():
    """the HIP runtime this process already uses, for one allocation of an exact size"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            hip = C.CDLL(line.split()[-1])
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipFree.argtypes = [C.c_void_p]
            hip.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
            return hip
    raise RuntimeError("no HIP runtime is loaded")


def _dev(v):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to("cuda:0")


def _dev_offset(v):
    """The same tensor as a view one float into a larger allocation: 4-byte aligned, not 16-byte aligned."""
    v = np.ascontiguousarray(v, np.float32)
    buf = torch.zeros(v.size + 1, dtype=torch.float32, device="cuda:0")
    t = buf[1:].view(len(v), 3)
    t.copy_(torch.from_numpy(v))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4, f"_dev_offset: the view lies at {t.data_ptr():#x}"
    return t


def _dev_all(verts: dict, offset_mesh=None):
    return {k: (_dev_offset(v) if k == offset_mesh else _dev(v)) for k, v in verts.items()}
