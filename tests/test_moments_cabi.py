"""The fused SVGF temporal stage (pt_temporal_moments) and the remodulation pass (pt_modulate_planes) without a GPU: the entry points are
declared and exported, the ctypes mirrors match the compiler's layout, the header compiles as C99 and as C++17 and states the arithmetic, a
null context and a null description are refused before any device work, both facades have the methods and the Python one checks its
arguments before the library is called; and the float32 NumPy reference (tests/moments_ref.py) has the properties the pass exists for: it
reduces to pt_temporal_accumulate's reference on the colour and on the moments plane, a constant albedo is an exact scaling, the clamp
window counts exactly the pixels the header says, and the inputs of tests/test_gpu_moments.py take every branch often enough."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import moments_ref as MR
import temporal_ref as T
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_text
from conftest import ROOT
from optixpathtracer_amd import _lib

f32 = np.float32
DESC_FIELDS = ("color", "albedo", "motion", "hit", "position", "prev_hit", "prev_position", "history_in", "moments_in", "length_in",
               "history_out", "moments_out", "length_out", "variance_out", "block_mask", "color_scale", "albedo_min", "normal_cos", "plane_eps",
               "min_weight", "clamp_k", "max_history", "flags")
STATS_FIELDS = ("pixels", "reprojected", "clamped", "kernel_ms")
MOD_FIELDS = ("color", "albedo", "out", "frame_rgba8", "block_mask", "albedo_min", "flags")
MOD_STATS_FIELDS = ("pixels", "kernel_ms")
NEW = ("pt_temporal_moments", "pt_modulate_planes")


# ------------------------------------------------------------------ surface
def test_library_exports_the_entry_points():
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert name in header().split("VERSIONING.")[1].split("*/")[0]  # the note names it among the entry points added at 0.4
        assert name in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_temporal_moments\s*\(\s*pt_ctx\s*\*\s*\w*\s*,\s*const\s+pt_tmom_desc\s*\*\s*\w*\s*,\s*pt_tmom_stats\s*\*", src)
    assert re.search(r"int\s+pt_modulate_planes\s*\(\s*pt_ctx\s*\*\s*\w*\s*,\s*const\s+pt_modulate_desc\s*\*\s*\w*\s*,\s*pt_modulate_stats\s*\*", src)
    assert re.search(r"enum\s+pt_tmom_flags\s*\{\s*PT_TMOM_CLEAR_COLOR\s*=\s*1\s*,\s*PT_TMOM_CLAMP\s*=\s*2\s*\}", src)
    assert (_lib.PT_TMOM_CLEAR_COLOR, _lib.PT_TMOM_CLAMP) == (1, 2)
    assert L.pt_version().startswith(b"ptamd 0.4")


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.TMomDesc, "pt_tmom_desc", DESC_FIELDS), (_lib.TMomStats, "pt_tmom_stats", STATS_FIELDS),
                            (_lib.ModulateDesc, "pt_modulate_desc", MOD_FIELDS), (_lib.ModulateStats, "pt_modulate_stats", MOD_STATS_FIELDS)],
                 [152] + list(range(0, 120, 8)) + [120, 124, 128, 132, 136, 140, 144, 148] + [32, 0, 8, 16, 24] + [48, 0, 8, 16, 24, 32, 40, 44] + [16, 0, 8])
    assert tuple(_lib.TMOM_PLANES) == DESC_FIELDS[:14] and _lib.TMOM_OUTPUTS == MR.OUTPUTS == DESC_FIELDS[10:14]
    assert {k: _lib.TMOM_PLANES[k] for k in MR.OUTPUTS} == MR.WORDS
    assert tuple(_lib.MODULATE_PLANES) == MOD_FIELDS[:4] and _lib.MODULATE_OUTPUTS == MOD_FIELDS[2:4]


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, float* color, const float* albedo, const float* planes, float* outs, uint32_t* frame) {\n"
            "    pt_tmom_desc d = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0f, 0.01f, 0.9f, 0.01f, 0.25f, 1.0f, 32u, 0u};\n"
            "    pt_modulate_desc m = {0, 0, 0, 0, 0, 0.01f, 0u};\n"
            "    pt_tmom_stats s;\n"
            "    pt_modulate_stats ms;\n"
            "    d.color = color; d.albedo = albedo; d.motion = planes; d.hit = planes; d.history_out = outs; d.variance_out = outs;\n"
            "    d.flags = PT_TMOM_CLEAR_COLOR | PT_TMOM_CLAMP;\n"
            "    if (pt_temporal_moments(c, &d, &s) || s.clamped > s.reprojected) return -1;\n"
            "    m.color = outs; m.albedo = albedo; m.out = outs; m.frame_rgba8 = frame;\n"
            "    return pt_modulate_planes(c, &m, &ms);\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_context_and_null_description_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.TMomDesc(), _lib.TMomStats(7, 7, 7, 7.0)
    assert L.pt_temporal_moments(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_temporal_moments: null context" in L.pt_last_error(None)
    assert L.pt_temporal_moments(None, None, None) == -1
    assert (s.pixels, s.reprojected, s.clamped, s.kernel_ms) == (7, 7, 7, 7.0)
    m, ms = _lib.ModulateDesc(), _lib.ModulateStats(7, 7.0)
    assert L.pt_modulate_planes(None, C.byref(m), C.byref(ms)) == -1
    assert b"pt_modulate_planes: null context" in L.pt_last_error(None)
    assert L.pt_modulate_planes(None, None, None) == -1 and (ms.pixels, ms.kernel_ms) == (7, 7.0)
    # a null description is refused before the context is looked at (the text of pt_moments.hip; a live context needs a GPU)
    api = open(os.path.join(ROOT, "optixpathtracer_amd", "csrc", "pt_moments.hip")).read()
    for name in NEW:
        body = api.split(f'extern "C" int {name}(')[1]
        assert body.index("null description") < body.index("ctx->width")


def test_python_facade_checks_its_arguments():
    import torch

    from optixpathtracer_amd import renderer as R

    for name in ("temporalMoments", "modulatePlanes"):
        assert callable(getattr(R.SampleRenderer, name, None))
    # on an object without a context: what the methods refuse, they refuse before the library is called
    r = bare_renderer()
    outs = dict(history_out=1, moments_out=1, length_out=1, variance_out=1)
    with pytest.raises(ValueError, match="temporalMoments: motion is required"):
        r.temporalMoments(1, None, 1, 1, 1, 1, 1, 1, 1, **outs)
    with pytest.raises(ValueError, match="temporalMoments: moments_in is required"):
        r.temporalMoments(1, 1, 1, 1, 1, 1, 1, None, 1, **outs)
    with pytest.raises(ValueError, match=r"temporalMoments: moments_in: a contiguous torch.float32 tensor of shape \(4, 4, 2\) is expected"):
        r.temporalMoments(1, 1, 1, 1, 1, 1, 1, fake_cuda((4, 4, 4)), 1, **outs)
    with pytest.raises(ValueError, match=r"temporalMoments: albedo: a contiguous torch.float32 tensor of shape \(4, 4, 4\) is expected"):
        r.temporalMoments(1, 1, 1, 1, 1, 1, 1, 1, 1, albedo=fake_cuda((4, 4, 3)), **outs)
    with pytest.raises(ValueError, match=r"variance_out: a contiguous torch.float32 tensor of shape \(4, 4\) is expected"):
        r.temporalMoments(1, 1, 1, 1, 1, 1, 1, 1, 1, **dict(outs, variance_out=fake_cuda((4, 4, 1))))
    with pytest.raises(TypeError, match="temporalMoments: color: a torch tensor or a device pointer"):
        r.temporalMoments(np.zeros((4, 4, 4), f32), 1, 1, 1, 1, 1, 1, 1, 1, **outs)
    with pytest.raises(ValueError, match="temporalMoments: hit: the tensor is on cpu"):
        r.temporalMoments(1, 1, torch.zeros((4, 4, 8)), 1, 1, 1, 1, 1, 1, **outs)
    with pytest.raises(ValueError, match="max_history must be in"):
        r.temporalMoments(1, 1, 1, 1, 1, 1, 1, 1, 1, max_history=-1, **outs)
    r.blockGrid = lambda: (1, 1)
    with pytest.raises(ValueError, match="temporalMoments: the mask needs"):
        r.temporalMoments(1, 1, 1, 1, 1, 1, 1, 1, 1, mask=np.ones((2, 2)), **outs)
    with pytest.raises(ValueError, match="modulatePlanes: no output asked for"):
        r.modulatePlanes(1, write_out=False)
    with pytest.raises(ValueError, match="modulatePlanes: color is required"):
        r.modulatePlanes(None, out=1)
    with pytest.raises(ValueError, match=r"modulatePlanes: albedo: a contiguous torch.float32 tensor of shape \(4, 4, 4\) is expected"):
        r.modulatePlanes(1, albedo=fake_cuda((4, 4)), out=1)
    with pytest.raises(ValueError, match="modulatePlanes: frame_rgba8: a contiguous torch.int32 tensor of shape .4, 4. or torch.uint8"):
        r.modulatePlanes(1, out=1, frame=fake_cuda((4, 4)))
    with pytest.raises(ValueError, match="modulatePlanes: the mask needs"):
        r.modulatePlanes(1, out=1, mask=np.ones((2, 2)))
    with pytest.raises(ValueError, match="the context on GPU 1"):
        r._device = 1
        r.modulatePlanes(fake_cuda((4, 4, 4)), out=1)


def test_cxx_facade_compiles(tmp_path):
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t stage(SampleRenderer& sample, pt_tmom_desc d, pt_modulate_desc m) {\n"
        "    pt_tmom_stats s{};\n"
        "    pt_modulate_stats ms{};\n"
        "    d.flags = PT_TMOM_CLAMP;\n"
        "    sample.temporalMoments(d, &s);\n"
        "    sample.modulatePlanes(m, &ms);\n"
        "    return sample.temporalMoments(d).clamped + s.reprojected + sample.modulatePlanes(m).pixels + ms.pixels;\n"
        "}\n"
    )


def test_header_states_the_contract():
    text = header_text()
    for item in ("den(q).k = 1.0f when albedo == NULL", "den(q).k = a > albedo_min ? a : 1.0f", "a NaN gives 1, a miss's zero gives 1",
                 "d(q).k = (color[q].k * color_scale) / den(q).k", "the multiplication first, then the division",
                 "d_p = d(p); l = lum(d_p); m = (l, l * l)", "both words of moments_in[q] finite (exponent-bit test)",
                 "H = Hsum / Wsum; M = Msum / Wsum", "row-major (dy outer, dx inner)", "cnt += 1; s1.k += d(q).k; s2.k += d(q).k * d(q).k",
                 "mu = s1 / cnt; sd = sqrtf(sel_max0(s2 / cnt - mu * mu)); lo = mu - clamp_k * sd; hi = mu + clamp_k * sd",
                 "H.k = H.k < lo.k ? lo.k : (H.k > hi.k ? hi.k : H.k)", "stats->clamped counts the valid pixels",
                 "The moments are not clamped", "out = H + (d_p - H) * a; mo = M + (m - M) * a; len = n + 1",
                 "Otherwise out = d_p; mo = m; len = 1",
                 "history_out[p] = (out, 1.0f); moments_out[p] = mo; length_out[p] = len; variance_out[p] = sel_max0(mo.y - mo.x * mo.x)",
                 "the clear is a second launch behind the kernel on the same stream", "float32 NumPy evaluating this reproduces every output bit for bit",
                 "a NaN is a NaN", "r.k = color[p].k * den(p).k", "out[p] = (r, color[p].w)", "frame_rgba8[p] = make_color(r)",
                 "out may be exactly the address of color", "clamping of the moments"):
        assert item in text, item


# ------------------------------------------------------------------ inputs shared by the tests below
_REAL = {}


def _real(orc, name):
    """the CPU-built planes of a real input of tests/test_gpu_moments.py, with its random colour, history, moments and albedo"""
    if name not in _REAL:
        make, size, cam, prev, _, seed = T.real_inputs()[name]
        planes = MR.with_random_inputs(T.cpu_planes(orc, make(), size, cam, prev), seed)
        for a in planes.values():
            a.setflags(write=False)
        _REAL[name] = planes
    return _REAL[name]


def _frame(planes):
    h, w = planes["length_in"].shape
    return [(0, 0, w, h)], np.ones((h, w), bool)


def _flat(w, h, seed):
    """one surface, no motion, one frame of history everywhere: every pixel is valid with H = history_in[p] and a = 1/2"""
    rng = np.random.default_rng(seed)
    hit = np.zeros((h, w, 8), f32)
    hit[..., 0], hit[..., 7] = 4, 1
    pos = np.zeros((h, w, 4), f32)
    pos[..., 3] = 1
    return dict(color=rng.random((h, w, 4), dtype=f32), albedo=None, motion=np.zeros((h, w, 2), f32), hit=hit, position=pos, prev_hit=hit,
                prev_position=pos, history_in=rng.random((h, w, 4), dtype=f32), moments_in=MR.random_moments(rng, h, w),
                length_in=np.ones((h, w), f32))


# ------------------------------------------------------------------ reduction to the existing pass
def _reduces(orc, planes, what, **prm):
    """albedo=None, flags 0: colour and length are temporal_ref's on the colour; the moments are temporal_ref's on the plane (l, l*l, 0, 1)
    against the history (moments_in, z, 1).  z is 0 wherever the three colour words of history_in are finite, and the offending word
    elsewhere: the fused pass reads ONE tap set for both, so a tap whose colour history is not finite carries no moments either — with a
    finite colour history (the synthetic planes) the history is (moments_in, 0, 1) as it stands."""
    rects, px = _frame(planes)
    h, w = px.shape
    got = MR.moments_ref(dict(planes, albedo=None), rects, px, **prm)
    col = T.temporal_ref(orc, planes, rects, px, **prm)
    assert np.array_equal(got["history_out"], col["history_out"]) and np.array_equal(got["length_out"], col["length_out"]), what
    assert got["reprojected"] == col["reprojected"] and np.array_equal(got["valid"], col["valid"])
    scale = f32(prm.get("color_scale", 1.0))
    l = MR.lum(planes["color"][..., :3] * scale)
    hist = planes["history_in"][..., :3]
    bad = ~MR._finite(hist)
    z = np.where(bad.any(-1), np.take_along_axis(hist, bad.argmax(-1)[..., None], -1)[..., 0], f32(0)).astype(f32)
    mplane = np.stack([l, l * l, np.zeros_like(l), np.ones_like(l)], -1)
    mhist = np.concatenate([planes["moments_in"], z[..., None], np.ones((h, w, 1), f32)], -1)
    mom = T.temporal_ref(orc, dict(planes, color=mplane, history_in=mhist), rects, px, **dict(prm, color_scale=1.0))
    assert np.array_equal(got["moments_out"], mom["history_out"][..., :2]), what
    assert np.array_equal(mom["length_out"], col["length_out"])
    m = got["moments_out"].view(f32)
    with np.errstate(all="ignore"):
        assert np.array_equal(got["variance_out"], MR.max0(m[..., 1] - m[..., 0] * m[..., 0]).view(np.uint32))
    return got


@pytest.mark.parametrize("size", [(65, 3), (9, 8), (1, 1)])
def test_reduces_to_the_temporal_pass_on_synthetic_planes(orc_det, size):
    w, h = size
    planes = dict(T.synthetic_planes(w, h, 7 + w), moments_in=MR.random_moments(np.random.default_rng(w), h, w))
    assert MR._finite(planes["history_in"]).all()
    got = _reduces(orc_det, planes, f"{w} x {h}", color_scale=3.0)
    if w * h > 1:
        assert 0 < got["reprojected"] < w * h


@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_reduces_to_the_temporal_pass_on_real_planes(orc_det, name):
    planes = _real(orc_det, name)
    assert not MR._finite(planes["history_in"][..., :3]).all() and MR._finite(planes["moments_in"]).all()
    got = _reduces(orc_det, planes, name, **T.real_inputs()[name][4])
    assert got["reprojected"] * 10 >= got["valid"].size


# ------------------------------------------------------------------ exact scaling
def test_a_constant_albedo_is_an_exact_scaling(orc_det):
    planes = _real(orc_det, "terrain")
    rects, px = _frame(planes)
    h, w = px.shape
    half = np.full((h, w, 4), 0.5, f32)
    twice = planes["color"] * f32(2)
    for flags in (dict(), dict(clamp=True, clamp_k=1.0)):
        a = MR.moments_ref(dict(planes, albedo=half), rects, px, albedo_min=0.1, **flags)
        b = MR.moments_ref(dict(planes, albedo=None, color=twice), rects, px, albedo_min=0.1, **flags)
        for name in MR.OUTPUTS:
            assert np.array_equal(a[name], b[name]), name
        assert (a["reprojected"], a["clamped"]) == (b["reprojected"], b["clamped"])
    # no history: history_out is the demodulated colour, and modulating it gives the colour's bits back
    fresh = MR.moments_ref(dict(planes, albedo=half, length_in=np.zeros((h, w), f32)), rects, px, albedo_min=0.1)
    assert fresh["reprojected"] == 0 and np.array_equal(fresh["history_out"][..., :3], twice[..., :3].view(np.uint32))
    back = MR.modulate_ref(orc_det, fresh["history_out"], half, px, albedo_min=0.1)
    assert np.array_equal(back["out"][..., :3], planes["color"][..., :3].view(np.uint32))
    assert np.array_equal(back["frame_rgba8"].reshape(-1), T.make_color_bits(orc_det, planes["color"][..., :3]))


def test_albedo_words_take_the_stated_branch(orc_det):
    amin = f32(0.1)
    above = np.nextafter(amin, f32(1))
    words = np.array([0.0, np.nan, amin, above, -1.0, np.inf, 0.75], f32)
    want = np.array([1.0, 1.0, 1.0, above, 1.0, np.inf, 0.75], f32)
    alb = np.ones((1, len(words), 4), f32)
    alb[0, :, 1] = words
    got = MR.den(alb, amin, (1, len(words), 3))
    assert np.array_equal(got[0, :, 1], want) and (got[0, :, 0] == 1).all()
    color = np.full((1, len(words), 4), 3.0, f32)
    d = MR.demodulated(color, alb, 2.0, amin)
    assert np.array_equal(d[0, :, 1], (f32(3) * f32(2)) / want) and (d[0, :, 0] == 6).all()
    out = MR.modulate_ref(orc_det, color, alb, np.ones((1, len(words)), bool), albedo_min=amin)["out"].view(f32)
    assert np.array_equal(out[0, :, 1], f32(3) * want) and (out[0, :, 3] == 3).all()


# ------------------------------------------------------------------ clamp
def _hand_window(ds, H, k):
    """lo, hi and the clamped H from a list of window colours (float32, the header's order)"""
    cnt, s1, s2 = f32(0), np.zeros(3, f32), np.zeros(3, f32)
    for dq in ds:
        cnt, s1, s2 = cnt + f32(1), s1 + dq, s2 + dq * dq
    mu = s1 / cnt
    sd = np.sqrt(MR.max0(s2 / cnt - mu * mu))
    lo, hi = mu - f32(k) * sd, mu + f32(k) * sd
    return lo, hi, np.where(H < lo, lo, np.where(H > hi, hi, H))


def _window(planes, X, Y, skip=()):
    return [planes["color"][Y + dy, X + dx, :3] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) not in skip]


def test_clamp_brings_a_stale_history_to_the_window(orc_det):
    w, h, X, Y = 12, 10, 5, 4
    planes = _flat(w, h, 3)
    planes["history_in"][Y, X, :3] = 100
    rects, px = _frame(planes)
    off = MR.moments_ref(planes, rects, px, clamp=False, clamp_k=1.0)
    assert np.array_equal(off["history_out"], MR.moments_ref(planes, rects, px, clamp=False, clamp_k=0.0)["history_out"])  # flag off: clamp_k is ignored
    assert np.array_equal(off["history_out"], T.temporal_ref(orc_det, planes, rects, px)["history_out"]) and off["clamped"] == 0
    assert (off["history_out"].view(f32)[Y, X, :3] > 50).all()  # the ghost
    on = MR.moments_ref(planes, rects, px, clamp=True, clamp_k=1.0)
    assert on["reprojected"] == w * h and on["window"][Y, X] == 9 and on["clamped_px"][Y, X]
    lo, hi, Hc = _hand_window(_window(planes, X, Y), np.full(3, 100, f32), 1.0)
    assert np.array_equal(Hc, hi) and (hi < 1.5).all()
    d = planes["color"][Y, X, :3]
    assert np.array_equal(on["history_out"].view(f32)[Y, X, :3], hi + (d - hi) * f32(0.5))
    # the moments are not clamped, and the corner window holds four pixels
    assert np.array_equal(on["moments_out"], off["moments_out"]) and np.array_equal(on["variance_out"], off["variance_out"])
    assert on["window"][0, 0] == 4 and on["window"][0, 1] == 6 and on["window_rejects"]["rect"] == 2 * 3 * (w + h) - 4
    # every pixel against the hand evaluation of its own window
    got = on["history_out"].view(f32)
    for yy, xx in ((1, 1), (h - 2, w - 2), (Y, X + 1)):
        _, _, Hc = _hand_window(_window(planes, xx, yy), planes["history_in"][yy, xx, :3], 1.0)
        assert np.array_equal(got[yy, xx, :3], Hc + (planes["color"][yy, xx, :3] - Hc) * f32(0.5))
    # clamp_k = 0 pins the history to the window's mean; a huge clamp_k clamps nothing
    assert MR.moments_ref(planes, rects, px, clamp=True, clamp_k=1e9)["clamped"] == 0
    assert MR.moments_ref(planes, rects, px, clamp=True, clamp_k=0.0)["clamped"] == w * h


def test_a_window_pixel_counts_only_inside_the_rectangle_the_block_set_and_finite(orc_det):
    w, h = 16, 8
    base = _flat(w, h, 5)
    X, Y = 7, 3  # the last column of block (0, 0); its right-hand neighbours are in block (0, 1)
    H = base["history_in"][Y, X, :3]
    d = base["color"][Y, X, :3]
    right = [(1, -1), (1, 0), (1, 1)]

    def at(res):
        return res["history_out"].view(f32)[Y, X, :3]

    def spiked(value):
        p = dict(base, color=base["color"].copy())
        p["color"][Y, X + 1, :3] = value
        return p

    _, _, H8 = _hand_window(_window(base, X, Y, skip=[(1, 0)]), H, 1.0)
    _, _, H6 = _hand_window(_window(base, X, Y, skip=right), H, 1.0)
    whole = [(0, 0, w, h)]
    px = np.ones((h, w), bool)
    # the neighbour counts when nothing keeps it out: its colour changes the answer
    full = MR.moments_ref(spiked(1e6), whole, px, clamp=True)
    assert full["window"][Y, X] == 9 and not np.array_equal(at(full), at(MR.moments_ref(base, whole, px, clamp=True)))
    # 1. finite: a NaN, an inf in one word of the neighbour's colour
    for bad in (np.nan, np.inf):
        p = spiked(1.0)
        p["color"][Y, X + 1, 1] = bad
        res = MR.moments_ref(p, whole, px, clamp=True)
        assert res["window"][Y, X] == 8 and np.array_equal(at(res), H8 + (d - H8) * f32(0.5))
    # 2. rectangle: two views side by side, the border between x = 7 and x = 8
    views = [(0, 0, 8, h), (8, 0, 8, h)]
    a, b = MR.moments_ref(spiked(1e6), views, px, clamp=True), MR.moments_ref(base, views, px, clamp=True)
    assert a["window"][Y, X] == 6 and np.array_equal(at(a), at(b)) and np.array_equal(at(a), H6 + (d - H6) * f32(0.5))
    assert a["window_rejects"]["rect"] > full["window_rejects"]["rect"]
    # 3. block set: block (0, 1) is not in the call's set (a mask, or another rank's block)
    blocks = np.array([[True, False]])
    own = np.repeat(np.repeat(blocks, 8, 0), 8, 1)
    a, b = MR.moments_ref(spiked(1e6), whole, own, blocks=blocks, clamp=True), MR.moments_ref(base, whole, own, blocks=blocks, clamp=True)
    assert a["window"][Y, X] == 6 and np.array_equal(at(a), at(b)) and np.array_equal(at(a), H6 + (d - H6) * f32(0.5))
    assert a["window_rejects"]["block"] == 3 * h - 2 and (a["history_out"][~own] == MR.SENTINEL).all()
    # ... and the default block set is the set's own blocks
    assert np.array_equal(MR.moments_ref(spiked(1e6), whole, own, clamp=True)["history_out"], a["history_out"])


def test_uniform_inputs_clamp_about_half_of_the_valid_pixels():
    """200 k draws of a fully valid pixel: nine uniform window colours, H the bilinear mix (uniform fractions) of four uniform histories,
    clamp_k = 1.  The fraction with at least one channel outside [mu - sd, mu + sd] is what leaves the coverage bounds of the real inputs
    (10 % of the valid pixels either way) their room: the assertion is those bounds with a margin of two."""
    rng = np.random.default_rng(1)
    n = 200000
    win = rng.random((n, 9, 3), dtype=f32)
    fx, fy = rng.random((n, 1), dtype=f32), rng.random((n, 1), dtype=f32)
    taps = rng.random((n, 4, 3), dtype=f32)
    Hh = (1 - fx) * (1 - fy) * taps[:, 0] + fx * (1 - fy) * taps[:, 1] + (1 - fx) * fy * taps[:, 2] + fx * fy * taps[:, 3]
    mu = win.mean(1)
    sd = np.sqrt(np.maximum((win * win).mean(1) - mu * mu, 0))
    frac = float(((Hh < mu - sd) | (Hh > mu + sd)).any(-1).mean())
    print(f"uniform colours and histories, clamp_k = 1: {frac:.3f} of the fully valid pixels clamped")
    assert 0.2 < frac < 0.8


# ------------------------------------------------------------------ coverage of the GPU test's inputs
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_gpu_inputs_take_every_branch(orc_det, name):
    planes = _real(orc_det, name)
    rects, px = _frame(planes)
    ref = MR.moments_ref(planes, rects, px, clamp=True, **MR.real_params(name))
    n, valid, clamped, ones, words = MR.check_coverage(planes, ref, px, name)
    print(f"{name}: {n} pixels, {valid} valid, {clamped} clamped, {ones} of {words} albedo words take den = 1; window rejects {ref['window_rejects']}")
    assert ref["window_rejects"]["rect"] > 0 and ref["window_rejects"]["finite"] > 0
