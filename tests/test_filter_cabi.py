"""The chain's filter (pt_filter_planes) without a GPU: the entry point is declared and exported, the ctypes mirrors of pt_filter_desc and
pt_filter_stats match the compiler's layout, the header still compiles as C99 and as C++17, a null context and a null description are
refused before any device work, both facades have the method and the Python one checks its arguments before the library is called; the
float32 NumPy reference (tests/filter_ref.py) has the properties an edge-stopping filter must have, and filters each view as a frame of its
own; the real-plane inputs of tests/test_gpu_filter.py, rebuilt here with the CPU checker, exercise every rejection reason; and the chain
G-buffer -> temporal -> moments -> filter brings the checker's 1-spp frames nearer to a 256-spp render than the accumulation alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import filter_ref as F
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_text
from conftest import ROOT
from optixpathtracer_amd import _lib

f32 = np.float32
DESC_FIELDS = ("color", "hit", "position", "variance", "length", "out", "scratch", "frame_rgba8", "block_mask", "iterations", "sigma_lum",
               "normal_cos", "plane_eps", "min_length", "flags")
STATS_FIELDS = ("pixels", "filtered", "spatial", "kernel_ms")


def test_library_exports_the_entry_point():
    L = _lib.load_library()
    assert "pt_filter_planes" in _lib.EXPORTS and hasattr(L, "pt_filter_planes")
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int\s+pt_filter_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_filter_desc\s*\*\s*\w+\s*,\s*pt_filter_stats\s*\*", src)
    assert re.search(r"PT_FILTER_RESERVED\s*=\s*0\b", src)
    assert L.pt_version().startswith(b"ptamd 0.4")
    assert "pt_filter_planes" in header().split("VERSIONING.")[1].split("*/")[0]  # the note names it among the entry points added at 0.4
    assert "pt_filter_planes" in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.FilterDesc, "pt_filter_desc", DESC_FIELDS), (_lib.FilterStats, "pt_filter_stats", STATS_FIELDS)],
                 [96] + [8 * k for k in range(9)] + [72, 76, 80, 84, 88, 92] + [32, 0, 8, 16, 24])
    assert set(_lib.FILTER_PLANES) == set(DESC_FIELDS[:8]) and _lib.FILTER_OUTPUTS == ("out", "scratch", "frame_rgba8")


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const float* color, const void* hit, float* out) {\n"
            "    pt_filter_desc d = {0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 4.0f, 0.9f, 0.01f, 4u, 0u};\n"
            "    pt_filter_stats s;\n"
            "    d.color = color; d.hit = hit; d.out = out; d.flags = PT_FILTER_RESERVED;\n"
            "    return pt_filter_planes(c, &d, &s);\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_null_context_and_null_description_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.FilterDesc(), _lib.FilterStats(7, 7, 7, 7.0)
    assert L.pt_filter_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_filter_planes: null context" in L.pt_last_error(None)
    assert L.pt_filter_planes(None, None, None) == -1
    assert (s.pixels, s.filtered, s.spatial, s.kernel_ms) == (7, 7, 7, 7.0)
    # a null description is refused before the context is looked at (the text of pt_filter.hip; a live context needs a GPU)
    api = open(os.path.join(ROOT, "optixpathtracer_amd", "csrc", "pt_filter.hip")).read()
    body = api.split('extern "C" int pt_filter_planes(')[1]
    assert body.index("null description") < body.index("ctx->width")


def test_python_facade_checks_its_arguments():
    import torch

    from optixpathtracer_amd import renderer as R

    assert callable(getattr(R.SampleRenderer, "filterPlanes", None))
    # the method on an object without a context: what it refuses, it refuses before the library is called
    r = bare_renderer()
    ok = dict(color=fake_cuda((4, 4, 4)), hit=fake_cuda((4, 4, 8)), position=fake_cuda((4, 4, 4)), out=1, scratch=1)
    with pytest.raises(ValueError, match="filterPlanes: hit is required"):
        r.filterPlanes(**dict(ok, hit=None))
    with pytest.raises(TypeError, match="filterPlanes: color: a torch tensor or a device pointer"):
        r.filterPlanes(**dict(ok, color=np.zeros((4, 4, 4), f32)))
    with pytest.raises(ValueError, match="filterPlanes: position: the tensor is on cpu"):
        r.filterPlanes(**dict(ok, position=torch.zeros((4, 4, 4))))
    r._device = 1
    with pytest.raises(ValueError, match="the context on GPU 1"):
        r.filterPlanes(**ok)
    r._device = 0
    with pytest.raises(ValueError, match=r"filterPlanes: variance: a contiguous torch.float32 tensor of shape \(4, 4\) is expected"):
        r.filterPlanes(**ok, variance=fake_cuda((4, 4, 1)))
    with pytest.raises(ValueError, match="filterPlanes: length: a contiguous torch.float32"):
        r.filterPlanes(**ok, length=fake_cuda((4, 4), torch.float64))
    with pytest.raises(ValueError, match="filterPlanes: hit: a contiguous"):
        r.filterPlanes(**dict(ok, hit=fake_cuda((8, 4, 4)).permute(2, 1, 0)))
    with pytest.raises(ValueError, match="frame_rgba8: a contiguous torch.int32 tensor of shape .4, 4. or torch.uint8 tensor of shape .4, 4, 4. is expected"):
        r.filterPlanes(**ok, frame=fake_cuda((4, 4)))
    with pytest.raises(ValueError, match="iterations must be in"):
        r.filterPlanes(**ok, iterations=7)
    with pytest.raises(ValueError, match="the mask needs"):
        r.blockGrid = lambda: (1, 1)
        r.filterPlanes(**ok, mask=np.ones((2, 2)))


def test_cxx_facade_compiles(tmp_path):
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t filter(SampleRenderer& sample, pt_filter_desc d) {\n"
        "    d.iterations = 5;\n"
        "    pt_filter_stats s{};\n"
        "    sample.filterPlanes(d, &s);\n"
        "    return sample.filterPlanes(d).filtered + s.spatial;\n"
        "}\n"
    )


def test_header_states_the_contract():
    text = header_text()
    for item in ("lum(c) = (0.2126f*c.x + 0.7152f*c.y) + 0.0722f*c.z", "sel_max0(v) = v > 0 ? v : 0", "sel_min80(v) = v < 80 ? v : 80",
                 "these are not fmaxf / fminf", "p is inert when hit[p].prim < 0", "exponent-bit test", "p itself always counts",
                 "fabsf(dot3(ng_p, position[q].xyz - position[p].xyz)) <= plane_eps * hit[p].t", "length[p] < (float)min_length",
                 "n += 1, s1 += lum(c_q), s2 += lum(c_q) * lum(c_q)", "v_in = sel_max0(s2 / n - m * m)", "k3 = {0.25f, 0.5f, 0.25f}",
                 "den = sigma_lum * sqrtf(g) + 1e-6f", "kern = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f}", "w = pt_expf(-e) * (kern[dy+2] * kern[dx+2])",
                 "V += (w * w) * v_q", "The new record is (S / W, V / (W * W))", "No other pixel is written in out, scratch or frame_rgba8",
                 "Zero pixels launch nothing and return PT_OK", "variance = max(0, m2 - m1 * m1)", "flags != 0"):
        assert item in text, item


# ------------------------------------------------------------------ pt_expf restated
def test_expf_is_the_library_functions(tmp_path):
    """filter_ref.pt_expf against include/pt_detmath.h's pt_expf compiled for the host without contraction (the library's flags), bit for
    bit on [-80, 0]; and against exp() to the accuracy the polynomial has"""
    x = np.concatenate([-np.linspace(0, 80, 20001).astype(f32), -np.random.default_rng(0).random(20000, dtype=f32) * f32(80),
                        np.array([-0.0, 0.0, -80.0, -1e-30, -0.34657359, -0.34657362], f32)])
    src = tmp_path / "expf.cpp"
    src.write_text('#include <cstdio>\n#include <cstdint>\n#include <cstring>\n#include <cmath>\n#include "pt_detmath.h"\n'
                   "int main() { float x; while (fread(&x, 4, 1, stdin) == 1) { float y = pt_expf(x); fwrite(&y, 4, 1, stdout); } return 0; }\n")
    exe = tmp_path / "expf"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = np.frombuffer(subprocess.run([str(exe)], input=x.tobytes(), check=True, capture_output=True).stdout, f32)
    got = F.pt_expf(x)
    assert got.dtype == f32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    exact = np.exp(x.astype(np.float64))
    assert (np.abs(got - exact) <= 4 * np.spacing(exact.astype(f32))).all()
    assert got[0] == 1.0 and F.pt_expf(np.array([-80.0], f32))[0] > 0


# ------------------------------------------------------------------ properties of the NumPy reference on synthetic planes
def _flat(h, w, color, variance=None, length=None):
    """one surface everywhere (mesh 0, normal +z, z = 0 plane), the colour plane given"""
    hit = np.zeros((h, w, 8), f32)
    hit[..., 0] = 5.0
    hit[..., 7] = 1.0  # ng = (0, 0, 1); prim = mesh = 0
    pos = np.zeros((h, w, 4), f32)
    pos[..., 0], pos[..., 1] = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    pos[..., 3] = 1
    return dict(color=color, hit=hit, position=pos, variance=variance, length=length)


def _whole(h, w):
    return [(0, 0, w, h)], np.ones((h, w), bool)


def test_a_constant_colour_is_a_fixed_point_for_any_variance(orc_det):
    h, w = 11, 19
    rng = np.random.default_rng(1)
    colour = np.broadcast_to(np.array([0.25, 0.5, 0.125, 9.0], f32), (h, w, 4)).copy()
    var = (rng.random((h, w), dtype=f32) * f32(10)).astype(f32)
    var[3, 4], var[0, 0], var[5, 5] = 0.0, 1e30, -2.0
    for v in (var, None, np.zeros((h, w), f32)):
        ref = F.filter_ref(orc_det, _flat(h, w, colour, v), *_whole(h, w), iterations=6)
        out = ref["out"].view(f32)
        # S / W with every r_q the same value c: the sum of c * w_k against the sum of w_k, each rounded: equal to a few ulp
        assert np.abs(out[..., :3] - colour[..., :3]).max() <= 4 * 2.0**-24
        assert (ref["frame_rgba8"] == ref["frame_rgba8"][0, 0]).all() and ref["filtered"] == h * w
        assert ref["spatial"] == (h * w if v is None else 0)
    # the spatial estimate of a constant is zero up to rounding, and then stays: V sums (w * w) * v
    ref = F.filter_ref(orc_det, _flat(h, w, colour), *_whole(h, w), iterations=2)
    assert (ref["out"].view(f32)[..., 3] <= 1e-7).all()


def test_the_output_lies_within_the_counting_taps_and_the_variance_shrinks(orc_det):
    h, w = 24, 40
    rng = np.random.default_rng(2)
    colour = rng.random((h, w, 4), dtype=f32)
    var = np.full((h, w), 0.08, f32)  # about the variance of a uniform [0, 1) luminance
    ref = F.filter_ref(orc_det, _flat(h, w, colour, var), *_whole(h, w), iterations=5, stages=True)
    recs = ref["records"]
    assert len(recs) == 6 and np.array_equal(recs[0][..., :3], colour[..., :3]) and (recs[0][..., 3] == f32(0.08)).all()
    lo, hi = colour[..., :3].min((0, 1)), colour[..., :3].max((0, 1))
    means = []
    for k in range(1, 6):
        step = 1 << (k - 1)
        prev, cur = recs[k - 1][..., :3], recs[k][..., :3]
        # weights are a partition: inside the min / max of the 25 taps of the previous stage (all count here, where they are in the frame)
        pad = np.pad(prev, ((2 * step, 2 * step), (2 * step, 2 * step), (0, 0)), mode="edge")
        win = np.stack([pad[2 * step + dy * step:2 * step + dy * step + h, 2 * step + dx * step:2 * step + dx * step + w]
                        for dy in range(-2, 3) for dx in range(-2, 3)])
        eps = 4 * 2.0**-24
        assert (cur >= win.min(0) - eps).all() and (cur <= win.max(0) + eps).all()
        assert (cur >= lo - eps).all() and (cur <= hi + eps).all()
        means.append(float(recs[k][..., 3].mean()))
        assert (recs[k][..., 3] >= 0).all()
    # the filtered variance of a flat noisy region shrinks from pass to pass
    assert all(b < a for a, b in zip([0.08] + means, means)), means
    assert means[-1] < 0.08 / 20


def test_zero_iterations_return_the_prepared_record(orc_det):
    h, w = 9, 13
    rng = np.random.default_rng(3)
    colour = rng.random((h, w, 4), dtype=f32)
    var = rng.random((h, w), dtype=f32) - f32(0.3)
    ln = rng.integers(0, 9, (h, w)).astype(f32)
    ref = F.filter_ref(orc_det, _flat(h, w, colour, var, ln), *_whole(h, w), iterations=0, min_length=4)
    out = ref["out"].view(f32)
    assert np.array_equal(out[..., :3], colour[..., :3])
    given = ln >= 4
    assert np.array_equal(out[..., 3][given], np.maximum(var, 0)[given]) and ref["spatial"] == int((~given).sum())
    # the spatial estimate of an interior pixel: the population variance of the 49 luminances
    l = F._lum(colour[..., :3]).astype(np.float64)
    ys, xs = np.nonzero(~given & (np.mgrid[0:h, 0:w][0] >= 3) & (np.mgrid[0:h, 0:w][0] < h - 3) & (np.mgrid[0:h, 0:w][1] >= 3) & (np.mgrid[0:h, 0:w][1] < w - 3))
    assert len(ys)
    for y, x in zip(ys, xs):
        assert abs(out[y, x, 3] - l[y - 3:y + 4, x - 3:x + 4].var()) < 1e-5
    # min_length = 0 and no length plane: every pixel takes the given variance
    for planes, prm in ((_flat(h, w, colour, var, ln), dict(min_length=0)), (_flat(h, w, colour, var), dict())):
        ref = F.filter_ref(orc_det, planes, *_whole(h, w), iterations=0, **prm)
        assert ref["spatial"] == 0 and np.array_equal(ref["out"].view(f32)[..., 3], np.maximum(var, 0))


def test_an_inert_pixel_neither_changes_nor_influences_a_neighbour(orc_det):
    h, w = 12, 17
    rng = np.random.default_rng(4)
    colour = rng.random((h, w, 4), dtype=f32)
    var = np.full((h, w), 0.05, f32)
    a = _flat(h, w, colour, var)
    a["hit"].view(np.int32)[5, 7, 3] = -1  # a miss
    a["color"][6, 2, 1] = np.inf           # a non-finite colour word on a hit
    ref = F.filter_ref(orc_det, a, *_whole(h, w), iterations=3)
    out = ref["out"]
    for y, x in ((5, 7), (6, 2)):
        assert ref["inert"][y, x] and np.array_equal(out[y, x, :3], a["color"].view(np.uint32)[y, x, :3]) and out[y, x, 3] == 0
    assert ref["filtered"] == h * w - 2 and ref["taps"]["inert"].sum() > 0
    # whatever the inert pixels hold, the others get the same bits
    b = dict(a, color=a["color"].copy(), variance=var.copy())
    b["color"][5, 7, :3] = (100.0, -3.0, 7.0)
    b["color"][6, 2, 0], b["color"][6, 2, 2] = np.nan, 55.0
    b["variance"][5, 7] = b["variance"][6, 2] = 1e6
    other = F.filter_ref(orc_det, b, *_whole(h, w), iterations=3)["out"]
    keep = ~ref["inert"]
    assert np.array_equal(out[keep], other[keep])


def test_a_nan_variance_word_acts_as_zero(orc_det):
    h, w = 10, 14
    rng = np.random.default_rng(5)
    colour = rng.random((h, w, 4), dtype=f32)
    var = (rng.random((h, w), dtype=f32) * f32(0.1)).astype(f32)
    var[4, 6] = 0.0
    other = var.copy()
    other[4, 6] = np.nan
    a = F.filter_ref(orc_det, _flat(h, w, colour, var), *_whole(h, w), iterations=4)
    b = F.filter_ref(orc_det, _flat(h, w, colour, other), *_whole(h, w), iterations=4)
    assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["frame_rgba8"], b["frame_rgba8"])
    assert not np.isnan(a["out"].view(f32)).any()


# ------------------------------------------------------------------ view independence
@pytest.mark.parametrize("rects", [[(0, 0, 29, 23), (32, 0, 27, 23)],
                                   [(0, 0, 21, 13), (24, 0, 35, 11), (0, 16, 13, 7), (16, 16, 43, 7)]], ids=["two", "four"])
def test_each_view_is_filtered_as_a_frame_of_its_own(orc_det, rects):
    h, w = 23, 59
    planes = F.synthetic_planes(w, h, 17)
    planes["color"] = planes["color"] + np.float32(3.0) * (np.arange(w, dtype=f32)[None, :, None] // 8)  # different colours left and right of any border
    px = np.zeros((h, w), bool)
    for x, y, rw, rh in rects:
        px[y:y + rh, x:x + rw] = True
    prm = dict(F.SYNTHETIC_PARAMS, iterations=5)
    ref = F.filter_ref(orc_det, planes, rects, px, **prm)
    assert (ref["out"][~px] == F.SENTINEL).all() and (ref["frame_rgba8"][~px] == F.SENTINEL).all()
    filtered = spatial = 0
    for x, y, rw, rh in rects:
        own = {k: np.ascontiguousarray(v[y:y + rh, x:x + rw]) for k, v in planes.items()}
        alone = F.filter_ref(orc_det, own, *_whole(rh, rw), **prm)
        assert np.array_equal(F.canon(ref["out"][y:y + rh, x:x + rw]), F.canon(alone["out"]))
        assert np.array_equal(ref["frame_rgba8"][y:y + rh, x:x + rw], alone["frame_rgba8"])
        filtered += alone["filtered"]
        spatial += alone["spatial"]
    assert (filtered, spatial) == (ref["filtered"], ref["spatial"]) and ref["taps"]["rect"].sum() > 0
    # ... and not as part of the whole frame: without views the taps cross the borders
    whole = F.filter_ref(orc_det, planes, *_whole(h, w), **prm)
    assert not np.array_equal(whole["out"][px], ref["out"][px])


def test_synthetic_planes_put_every_reason_on_a_tap(orc_det):
    """the hand-made planes of the GPU test: each reason, a plane distance exactly on plane_eps * t, a pixel on each rectangle edge"""
    w, h = 65, 3
    planes = F.synthetic_planes(w, h, 7 + w)
    ref = F.filter_ref(orc_det, planes, *_whole(h, w), **F.SYNTHETIC_PARAMS)
    rej, cnt = F.tap_counts(ref)
    assert all(rej[r] > 0 for r in ("rect", "inert", "mesh", "normal", "plane")) and rej["block"] == 0 and cnt > 0, rej
    # kind 0 at x = 0..2 and kind 1 at x = 3..5 of row 0: the distance 0.5 equals plane_eps * t = 0.125 * 4 and counts; a hair less does not
    one = F.filter_ref(orc_det, planes, *_whole(h, w), iterations=1, plane_eps=0.125)
    less = F.filter_ref(orc_det, planes, *_whole(h, w), iterations=1, plane_eps=float(np.nextafter(f32(0.125), f32(0))))
    assert one["counted"][0, 2] > less["counted"][0, 2] and less["taps"]["plane"][0, 2] > one["taps"]["plane"][0, 2]


# ------------------------------------------------------------------ the GPU tests' real-plane inputs exercise every rejection reason
# with the CPU-built planes: rejected candidate taps per reason, counting taps, pixels taking the spatial estimate, non-inert pixels
COUNTS = {
    "two_box": (dict(rect=93251, block=0, inert=68922, mesh=34588, normal=9455, plane=406468), 241092, 1897, 4767),
    "terrain": (dict(rect=100640, block=0, inert=69237, mesh=255486, normal=223179, plane=69223), 212779, 2113, 5182),
}


@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_real_inputs_cover_every_rejection_reason(orc_det, name):
    make, size, cam, prm, seed = F.real_inputs()[name]
    w, h = size
    planes = F.with_random_planes(F.cpu_gbuffer(orc_det, make(), size, cam), seed)
    ref = F.filter_ref(orc_det, planes, *_whole(h, w), **prm)
    got = F.check_coverage(ref, name)
    assert got == COUNTS[name], got
    if name == "terrain":  # over the two cases together every reason but `block` occurs (that one belongs to the mask and partition cases)
        total = {r: got[0][r] + COUNTS["two_box"][0][r] for r in F.REASONS}
        assert all(total[r] > 0 for r in ("rect", "inert", "mesh", "normal", "plane")) and total["block"] == 0
    # the words the random planes are there for
    assert np.isnan(planes["variance"]).any() and np.isinf(planes["variance"]).any() and (planes["variance"] < 0).any()
    assert np.isnan(planes["color"]).any() and np.isinf(planes["color"]).any() and np.isnan(planes["length"]).any()
    assert np.isinf(ref["out"].view(f32)[..., 3]).any()
    # a block mask brings the `block` reason
    mask = np.random.default_rng(5).random(((h + 7) // 8, (w + 7) // 8)) < 0.4
    px = np.repeat(np.repeat(mask, 8, 0), 8, 1)[:h, :w]
    masked = F.filter_ref(orc_det, planes, [(0, 0, w, h)], px, blocks=mask, **prm)
    assert masked["taps"]["block"].sum() > 0 and (masked["out"][~px] == F.SENTINEL).all()


# ------------------------------------------------------------------ the chain end to end, on the checker's frames
def chain_inputs(orc):
    """the checker's eight 1-spp frames (subframe k over a zeroed accumulation) of the two-box scene at 64 x 48, its 256-spp frame, and the
    CPU-built G-buffer"""
    from optixpathtracer_amd import scenes

    w, h = F.CHAIN["size"]
    model = scenes.two_box_scene(shadow_catcher=False)
    cam = scenes.TWO_BOX_CAMERA
    uvw = scenes.uvw_frame(**cam, aspect=w / h)
    sc, pr = orc.make_scene(model), orc.make_probe(scenes.sky_probe(256, 128).BuildCDF())
    colours = [orc.render(sc, pr, uvw, cam["eye"], w, h, F.CHAIN["spp"], subframe=k)["accum"] for k in range(F.CHAIN["frames"])]
    reference = orc.render(sc, pr, uvw, cam["eye"], w, h, F.CHAIN["reference_spp"])["accum"]
    return colours, reference, F.cpu_gbuffer(orc, model, (w, h), cam)


def test_the_chain_beats_the_accumulation_alone(orc_det):
    """RMS error against the 256-spp frame, checker's frames, NumPy chain, default parameters: 0.0727 for history_out, 0.0193 filtered."""
    colours, reference, gb = chain_inputs(orc_det)
    hist, ref, var, ln = F.chain_ref(orc_det, colours, gb["hit"], gb["position"])
    plain, filtered = F.rms(hist, reference), F.rms(ref["out"], reference)
    print(f"chain: rms of history_out {plain:.5f}, filtered {filtered:.5f}")
    assert (ln == F.CHAIN["frames"]).all() and ref["spatial"] == 0 and (var[~ref["inert"]] > 0).any()
    assert filtered < plain
