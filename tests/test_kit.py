"""The test support layer itself (tests/cabi_kit.py, tests/gpu_kit.py): every other test leans on these comparisons, pixel sets and
compiler probes, so their own teeth are checked here, on inputs small enough to be read."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import cabi_kit
import gpu_kit as K
from optixpathtracer_amd import _lib

f32 = np.float32
EDGE_AA = [(_lib.EdgeAaDesc, "pt_edge_aa_desc", ("color", "hit", "position", "out", "edge", "frame_rgba8", "block_mask", "normal_cos", "plane_eps", "flags")),
           (_lib.EdgeAaStats, "pt_edge_aa_stats", ("pixels", "hits", "stale", "boundary", "blended", "kernel_ms"))]
EDGE_AA_PINNED = [72, 0, 8, 16, 24, 32, 40, 48, 56, 60, 64] + [48, 0, 8, 16, 24, 32, 40]


# ------------------------------------------------------------------ differ, same
def _plane():
    return np.random.default_rng(1).random((3, 5, 4), dtype=f32)


def test_one_flipped_mantissa_bit_is_reported_with_its_position():
    a = _plane()
    b = a.copy()
    b.view(np.uint32)[2, 1, 3] ^= 1
    assert np.argwhere(K.differ(a, b)).tolist() == [[2, 1, 3]]
    K.same(dict(out=a), dict(out=a.copy()), "equal planes")
    with pytest.raises(AssertionError, match=re.escape("a flipped bit: out differs in 1 words, first at [[2, 1, 3]]")):
        K.same(dict(out=a), dict(out=b), "a flipped bit")


def test_a_shape_mismatch_fails():
    a = _plane()
    with pytest.raises(AssertionError, match=r"shapes: out has shape \(3, 5, 4\), the reference \(3, 20\)"):
        K.same(dict(out=a), dict(out=a.reshape(3, 20)), "shapes")


def test_nans_are_equal_whatever_their_payloads_and_signed_zeros_are_not():
    a, b = _plane(), _plane()
    a.view(np.uint32)[0, 0, 0], b.view(np.uint32)[0, 0, 0] = 0x7FC00000, 0xFFC12345
    assert np.isnan(a[0, 0, 0]) and np.isnan(b[0, 0, 0]) and not K.differ(a, b).any()
    K.same(dict(out=a), dict(out=b), "two NaNs")
    assert not K.words_differ(a.view(np.uint32), b.view(np.uint32)).any()  # the same planes handed over as words
    b[1, 1, 1] = np.nan  # a NaN against a number
    assert np.argwhere(K.differ(a, b)).tolist() == [[1, 1, 1]]
    z, m = np.zeros((3, 5, 4), f32), np.zeros((3, 5, 4), f32)
    m[2, 4, 0] = -0.0
    with pytest.raises(AssertionError, match=re.escape("zeros: out differs in 1 words, first at [[2, 4, 0]]")):
        K.same(dict(out=z), dict(out=m), "zeros")


def test_an_integer_plane_is_compared_as_it_is():
    a = np.arange(15, dtype=np.int32).reshape(3, 5)
    b = a.copy()
    b[1, 2] = 0x7FC00001  # (as floats both words would be NaNs here: an integer plane gets no such allowance)
    a[1, 2] = 0x7FC00000
    with pytest.raises(AssertionError, match=re.escape("packed pixels: frame_rgba8 differs in 1 words, first at [[1, 2]]")):
        K.same(dict(frame_rgba8=a), dict(frame_rgba8=b), "packed pixels")
    # as words: the float plane's NaNs are equal, the packed pixels' are not
    nan_a, nan_b = _plane().view(np.uint32), _plane().view(np.uint32)
    nan_a[0, 0, 0], nan_b[0, 0, 0] = 0x7FC00000, 0x7FC00001
    K.same_words(dict(out=nan_a, frame_rgba8=a.view(np.uint32)), dict(out=nan_b, frame_rgba8=a.view(np.uint32)), "words")
    with pytest.raises(AssertionError, match=re.escape("words: frame_rgba8 differs in 1 words, first at [[1, 2]]")):
        K.same_words(dict(out=nan_a, frame_rgba8=a.view(np.uint32)), dict(out=nan_b, frame_rgba8=b.view(np.uint32)), "words")


# ------------------------------------------------------------------ pixel sets
def test_pixel_mask_takes_its_size_by_keyword_only():
    blocks = np.array([[1, 0, 1], [0, 1, 1]], bool)
    px = K.pixel_mask(blocks, h=13, w=21)
    assert px.shape == (13, 21) and px.dtype == bool
    assert px[0, 0] and not px[0, 8] and px[0, 20] and not px[12, 0] and px[12, 8] and px[12, 20] and px[7, 7] and not px[8, 7]
    assert int(px.sum()) == 8 * 8 + 8 * 5 + 5 * 8 + 5 * 5
    with pytest.raises(TypeError):
        K.pixel_mask(blocks, 13, 21)
    with pytest.raises(TypeError):
        K.pixel_mask(blocks, 13, w=21)
    assert K.whole_frame_mask(13, 21).shape == (13, 21) and K.whole_frame_mask(13, 21).all()
    rects, px = K.whole_frame(21, 13)
    assert rects == [(0, 0, 21, 13)] and px.shape == (13, 21) and px.all()


# ------------------------------------------------------------------ the compiler probes
def test_check_layout_holds_ctypes_the_compiler_and_the_pinned_numbers_together(tmp_path):
    cabi_kit.check_layout(tmp_path, EDGE_AA, EDGE_AA_PINNED)
    moved = list(EDGE_AA_PINNED)
    moved[8] = 52  # normal_cos
    with pytest.raises(AssertionError, match="pinned"):
        cabi_kit.check_layout(tmp_path, EDGE_AA, moved)
    (cls, ctype, fields), stats = EDGE_AA
    swapped = list(fields)
    swapped[7], swapped[8] = swapped[8], swapped[7]  # normal_cos and plane_eps: the same type, so only the order can tell
    with pytest.raises(AssertionError, match="the ctypes mirror's fields are"):
        cabi_kit.check_layout(tmp_path, [(cls, ctype, tuple(swapped)), stats], EDGE_AA_PINNED)
    # a mirror whose layout is not the C type's, pinned as ctypes has it: only the compiler can tell
    class Packed(C.Structure):
        _pack_ = 4
        _fields_ = [("pixels", C.c_uint64), ("hits", C.c_uint64), ("stale", C.c_uint64), ("boundary", C.c_uint64), ("blended", C.c_uint64), ("kernel_ms", C.c_float)]

    assert C.sizeof(Packed) == 44
    with pytest.raises(AssertionError, match="the compiler lays"):
        cabi_kit.check_layout(tmp_path, [(Packed, "pt_edge_aa_stats", stats[2])], [44, 0, 8, 16, 24, 32, 40])


def test_the_c99_pass_is_a_real_one(tmp_path):
    cabi_kit.compile_c99_and_cxx17(tmp_path, '#include "pt_amd.h"\n')
    with pytest.raises(subprocess.CalledProcessError) as e:
        cabi_kit.compile_c99_and_cxx17(tmp_path, '#include "pt_amd.h"\nstatic int f(int& x) { return x; }\nint g(void) { int y = 1; return f(y); }\n')
    assert e.value.cmd[0] == "gcc"  # (valid C++17: it is the C pass that refuses the reference)


def test_header_section_cuts_between_two_markers():
    text = cabi_kit.header_section("GEOMETRIC EDGE ANTIALIASING", "The acceleration structure as the traversal kernels see it")
    assert "stats->boundary counts the pixels with at least one candidate" in text and "\n" not in text and "  " not in text
    assert "GEOMETRIC EDGE ANTIALIASING" in cabi_kit.header_text() and len(text) < len(cabi_kit.header_text())
    with pytest.raises(ValueError, match="no 'NO SUCH SECTION'"):
        cabi_kit.header_section("NO SUCH SECTION", "The acceleration structure")
    with pytest.raises(ValueError, match="after 'GEOMETRIC EDGE ANTIALIASING'"):
        cabi_kit.header_section("GEOMETRIC EDGE ANTIALIASING", "NO SUCH END")


# ------------------------------------------------------------------ planes on the GPU
@pytest.mark.gpu
def test_uploaded_and_filled_planes_lie_where_they_should(ptlib):
    import torch

    h, w = 3, 5
    for words in (1, 2, 4, 8):
        shape = K.plane_shape(h, w, words)
        assert shape == ((h, w) if words == 1 else (h, w, words))
        a = np.random.default_rng(words).random(shape, dtype=f32)
        for offset in (False, True):
            t = K.upload(a, offset)
            assert t.is_contiguous() and t.data_ptr() % 16 == (4 if offset else 0) and t.shape == shape and t.dtype == torch.float32
            assert np.array_equal(K.bits(t), a.view(np.uint32)) and K.bits(t).shape == shape
            assert K.bits3(t).shape == (h, w, words) and np.array_equal(K.bits3(t).reshape(shape), a.view(np.uint32))
            assert np.array_equal(K.to_numpy(t), a)
            f = K.filled(shape, offset)
            assert f.is_contiguous() and f.data_ptr() % 16 == (4 if offset else 0) and f.shape == shape and f.dtype == torch.float32
            assert K.bits(f).shape == shape and (K.bits(f) == K.SENTINEL).all() and K.SENTINEL == 0xA5A5A5A5
            assert K.bits3(f).shape == (h, w, words)
    for offset in (False, True):
        frame = K.filled((h, w), offset, torch.int32)
        assert frame.dtype == torch.int32 and frame.shape == (h, w) and frame.is_contiguous() and frame.data_ptr() % 16 == (4 if offset else 0)
        assert (K.bits(frame) == K.SENTINEL).all()
