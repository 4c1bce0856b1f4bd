"""Mirror reflections from the G-buffer (pt_reflect_layout, pt_reflect_planes) without a GPU: the entry points are declared and exported,
the ctypes mirrors match the compiler's layout, the header compiles as C99 and C++17 and states the rule, null arguments are refused before
any device work, both facades have the methods; and the float32 NumPy reference (tests/reflect_ref.py) is held against its own geometry:
the reflection identity for every unit normal and eye, and two analytic scenes of quads under a float64 brute-force closest hit where every
mirror ray hits the lid, or escapes."""
import ctypes as C
import re

import numpy as np
import pytest

import reflect_ref as F
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_section
from optixpathtracer_amd import _lib
from optixpathtracer_amd import renderer as R

f32 = np.float32
u32 = np.uint32
DESC_FIELDS = ("hit", "position", "hit2", "position2", "ray", "sky", "scratch", "block_mask", "bias", "max_distance", "max_rays_in_flight", "flags")
STATS_FIELDS = ("pixels", "traced", "skipped", "nonfinite", "invalid", "hits", "escaped", "batches", "kernel_ms", "trace_ms")
NAMES = ("pt_reflect_layout", "pt_reflect_planes")


def test_library_exports_the_entry_points():
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert name in header().split("VERSIONING.")[1].split("*/")[0]
        assert name in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_reflect_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_reflect_desc\s*\*\s*\w+\s*,\s*pt_reflect_stats\s*\*", src)
    assert re.search(r"int\s+pt_reflect_layout\s*\(\s*const\s+pt_ctx\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*size_t\s*\*\s*\w+\s*\)", src)
    assert b"0.4" in L.pt_version()


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.ReflectDesc, "pt_reflect_desc", DESC_FIELDS), (_lib.ReflectStats, "pt_reflect_stats", STATS_FIELDS)],
                 [80, 0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76] + [80, 0, 8, 16, 24, 32, 40, 48, 56, 64, 72])
    assert _lib.REFLECT_PLANES == dict(hit=8, position=4, hit2=8, position2=4, ray=8, sky=4) and _lib.REFLECT_OUTPUTS == F.PLANES
    m = re.search(r"#define\s+PT_REFLECT_DEFAULT_RAYS_IN_FLIGHT\s+(\d+)u", header())
    assert m and int(m.group(1)) == _lib.PT_REFLECT_DEFAULT_RAYS_IN_FLIGHT == F.DEFAULT_RAYS_IN_FLIGHT == 1 << 23


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const void* hit, const float* position, void* hit2, float* position2, float* ray, float* sky, void* scratch) {\n"
            "    pt_reflect_desc d = {0, 0, 0, 0, 0, 0, 0, 0, 1e-3f, 1e16f, 0u, 0u};\n"
            "    pt_reflect_stats s;\n"
            "    size_t bytes = 0;\n"
            "    if (pt_reflect_layout(c, PT_REFLECT_DEFAULT_RAYS_IN_FLIGHT, &bytes)) return 1;\n"
            "    d.hit = hit; d.position = position; d.hit2 = hit2; d.position2 = position2; d.ray = ray; d.sky = sky; d.scratch = scratch;\n"
            "    return pt_reflect_planes(c, &d, &s) || s.traced + s.skipped + s.nonfinite != s.pixels || s.hits + s.escaped + s.invalid != s.traced ||\n"
            "           s.batches == 0 || s.trace_ms > s.kernel_ms;\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_header_states_the_rule():
    text = header_section("MIRROR REFLECTIONS FROM THE G-BUFFER", "int pt_reflect_planes(")
    for item in ("hit2 = {t 0, u 0, v 0, prim -1, mesh -1, ng 0}, position2 = (0, 0, 0, 0)", "the neutral ray (0, 0, 0, 1, 0, 0, 1, -1)",
                 "If h.prim < 0 (a miss): the empty record", "or t > 0 is false", "s = dot3(n0, E - P); n = (s < 0) ? -n0 : n0",
                 "d = normalize3(P - E); c = dot3(d, n); k = 2.0f * c", "r = normalize3((d.x - n.x*k, d.y - n.y*k, d.z - n.z*k))",
                 "O = P + n * (bias * t) per component, the product first and then the sum", "(O, tmin = 0.0f, r, tmax = max_distance)",
                 "hit2 = {t 0, u 0, v 0, prim -2, mesh -1, ng 0}", "ray = its own eight words as computed",
                 "exactly the pt_hit that pt_trace_device(PT_QUERY_CLOSEST) returns", "t = max_distance", "Back faces count",
                 "position2 = (O.x + t2*r.x, O.y + t2*r.y, O.z + t2*r.z, 1.0f)", "pt_eval_table 3", "(texel.x, texel.y, texel.z, 1.0f)",
                 "batches of M pixels", "256 + pixels * 44, rounded up to 16", "The result does not depend on M, bit for bit",
                 "no probe set (setProbe)", "PT_ERR_UNSUPPORTED",
                 "touches neither the context's query state, nor the frame buffers, nor pt_stats", "launches nothing and returns PT_OK"):
        assert item in text, item


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.ReflectDesc(), _lib.ReflectStats(7, 7, 7, 7, 7, 7, 7, 7, 7.0, 7.0)
    assert L.pt_reflect_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_reflect_planes: null context" in L.pt_last_error(None)
    assert L.pt_reflect_planes(None, None, None) == -1
    nb = C.c_size_t(77)
    assert L.pt_reflect_layout(None, 0, C.byref(nb)) == -1 and b"pt_reflect_layout: null context" in L.pt_last_error(None) and nb.value == 77
    assert tuple(getattr(s, n) for n in STATS_FIELDS) == (7, 7, 7, 7, 7, 7, 7, 7, 7.0, 7.0)


def test_facades_have_the_methods(tmp_path):
    import torch  # noqa: F401

    for name in ("reflectLayout", "reflectPlanes"):
        assert callable(getattr(R.SampleRenderer, name, None)) and callable(getattr(R._RankView, name, None))
    r = bare_renderer()
    hit, pos = fake_cuda((4, 4, 8)), fake_cuda((4, 4, 4))
    with pytest.raises(ValueError, match="max_rays_in_flight must be in"):
        r.reflectPlanes(hit, pos, max_rays_in_flight=-1)
    with pytest.raises(ValueError, match="max_rays_in_flight must be in"):
        r.reflectPlanes(hit, pos, max_rays_in_flight=2**32)
    with pytest.raises(ValueError, match="hit is required"):
        r.reflectPlanes(None, pos)
    with pytest.raises(ValueError, match="position is required"):
        r.reflectPlanes(hit, None)
    with pytest.raises(ValueError, match=r"hit2: a contiguous torch.float32 tensor of shape \(4, 4, 8\) is expected"):
        r.reflectPlanes(hit, pos, hit2=fake_cuda((4, 4, 4)))
    with pytest.raises(ValueError, match=r"sky: a contiguous torch.float32 tensor of shape \(4, 4, 4\) is expected"):
        r.reflectPlanes(hit, pos, sky=fake_cuda((4, 4)))
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t reflection(SampleRenderer& sample, pt_reflect_desc d) {\n"
        "    size_t bytes = sample.reflectLayout() + sample.reflectLayout(1u << 20);\n"
        "    pt_reflect_stats s{};\n"
        "    sample.reflectPlanes(d, &s);\n"
        "    return sample.reflectPlanes(d).hits + s.escaped + s.batches + bytes;\n"
        "}\n")


# ------------------------------------------------------------------ the reference alone
def _normals_and_eye_rays():
    """400 random unit normals with random unit eye rays on the normal's far side (dot3(d, n) <= 0, as step 3 leaves them), the axes in both
    signs against oblique rays, head-on rays (d = -n) and grazing ones (c = 0)"""
    rng = np.random.default_rng(11)
    n = rng.normal(size=(400, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = rng.normal(size=(400, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(((d * n).sum(1) > 0)[:, None], -d, d)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    oblique = -axes + 0.5 * np.roll(axes, 1, axis=1)
    oblique /= np.linalg.norm(oblique, axis=1, keepdims=True)
    grazing = np.roll(axes, 1, axis=1)  # perpendicular to the axis: c = 0 exactly
    n = np.concatenate([n, axes, axes, axes])
    d = np.concatenate([d, oblique, -axes, grazing])
    return n.astype(f32), d.astype(f32)


def test_the_reflection_identity():
    """dot3(r, n) == -dot3(d, n) and |r| == 1 within 2e-6 absolute: a dozen float32 roundings (2^-24 each, on values of at most 2) between
    the unit inputs and either side"""
    n, d = _normals_and_eye_rays()
    assert len(n) == 418
    r = F.mirror(d, n)
    assert r.dtype == f32 and F.ray_valid(np.concatenate([np.zeros((len(r), 4), f32), r, np.ones((len(r), 1), f32)], 1)).all()
    r64, n64, d64 = r.astype(np.float64), n.astype(np.float64), d.astype(np.float64)
    err = np.abs((r64 * n64).sum(1) + (d64 * n64).sum(1))
    assert err.max() <= 2e-6, err.max()
    length = np.sqrt((r64 ** 2).sum(1))
    assert np.abs(length - 1).max() <= 2e-6, np.abs(length - 1).max()
    # the tangential part is kept: r - d is parallel to n
    tang = np.cross(r64 - d64, n64)
    assert np.abs(tang).max() <= 4e-6, np.abs(tang).max()
    grazing = slice(len(n) - 6, len(n))
    assert (F.dot3(d[grazing], n[grazing]) == 0).all() and np.array_equal(r[grazing], d[grazing]), "a grazing ray goes on as it came"
    head_on = slice(len(n) - 12, len(n) - 6)
    assert np.array_equal(r[head_on], n[head_on]), "a head-on ray comes back along the normal"


def test_layout_and_batches():
    assert F.layout(40, 64) == 256 + 2560 * 44 and F.layout(40, 64, 1) == (256 + 44 + 15) // 16 * 16 == 304
    assert F.layout(40, 64, 3) == (256 + 132 + 15) // 16 * 16 and F.layout(40, 64, 1 << 30) == F.layout(40, 64) and F.layout(1, 1) == 304
    assert F.batches_of(2560, 40, 64, 1) == 2560 and F.batches_of(2560, 40, 64, 1000) == 3 and F.batches_of(0, 40, 64) == 0 and F.batches_of(2560, 40, 64) == 1


@pytest.mark.parametrize("ceiling", [True, False], ids=["lid", "open"])
def test_two_analytic_scenes(ceiling):
    """a floor under a lid: every floor pixel's mirror ray hits the lid's mesh, and position2 lies on it; the same floor with no lid: every
    ray escapes at max_distance"""
    hit, P, cam = F.analytic_planes()
    h, w = hit.shape[:2]
    pixels = np.ones((h, w), bool)
    Rr = F.rays_of(hit, P, cam, None, pixels, bias=1e-3, max_distance=100.0)
    assert Rr["valid"].all() and len(Rr["pixel"]) == h * w and (Rr["rays"][:, 5] > 0.9).all() and (Rr["rays"][:, 1] > 0).all()
    # the mirror of the eye ray about +y: the same horizontal part, the vertical part turned round (to a few roundings)
    assert np.abs(Rr["rays"][:, 4:7] - Rr["d"] * np.array([1, -1, 1], f32)).max() <= 2e-6
    t, prim, mesh = F.closest_hit_quads(Rr["rays"], F.analytic_quads(ceiling))
    sky_rgb = np.tile(np.array([[0.25, 0.5, 0.75]], f32), (h * w, 1))
    ref = F.scatter(F.records_of(t, prim, mesh), Rr, pixels, sky_rgb)
    hit2, pos2, sky = ref["hit2"], ref["position2"].view(f32), ref["sky"].view(f32)
    assert (ref["pixels"], ref["traced"], ref["skipped"], ref["nonfinite"], ref["invalid"], ref["batches"]) == (h * w, h * w, 0, 0, 0, 1)
    assert np.array_equal(ref["ray"].view(f32).reshape(-1, 8), Rr["rays"])
    if ceiling:
        assert ref["hits"] == h * w and ref["escaped"] == 0
        assert (hit2[..., 4].view(np.int32) == 1).all() and (hit2[..., 3].view(np.int32) >= 2).all(), "every mirror ray hits the lid's mesh"
        assert np.abs(pos2[..., 1] - F.LID).max() <= 1e-5 and (pos2[..., 3] == 1).all() and (sky == 0).all()
        assert (np.abs(pos2[..., [0, 2]] - P[..., [0, 2]]) < 0.7).all()
    else:
        assert ref["hits"] == 0 and ref["escaped"] == h * w
        assert (hit2[..., 3].view(np.int32) == -1).all() and (hit2[..., 4].view(np.int32) == -1).all() and (hit2[..., 0].view(f32) == f32(100.0)).all()
        assert (pos2 == 0).all() and (sky == np.array([0.25, 0.5, 0.75, 1.0], f32)).all()


def test_misses_hostile_records_and_invalid_rays():
    hit, P, cam = F.analytic_planes()
    hit, P = hit.copy(), P.copy()
    hit[0, 0, 3] = np.array([-1], np.int32).view(f32)[0]
    hit[0, 1, 5] = np.nan
    hit[0, 2, 0] = np.inf
    hit[0, 3, 0] = 0.0
    hit[0, 4, 0] = -1.0
    P[0, 5, 2] = -np.inf
    hit[0, 6, 3] = np.array([0x7FFFFFF0], np.int32).view(f32)[0]  # a stale primitive: processed
    hit[1, 0, 5:8] = 0.0  # a zero normal: r = d, a valid ray
    P[1, 1, 0:3] = F.ANALYTIC_EYE  # the eye itself: d = 0 / 0, an invalid ray with its own words in `ray`
    pixels = np.ones(hit.shape[:2], bool)
    Rr = F.rays_of(hit, P, cam, None, pixels)
    assert Rr["skipped"].sum() == 1 and Rr["nonfinite"].sum() == 5 and Rr["traced"][0, 6] and len(Rr["pixel"]) == pixels.size - 6
    assert int((~Rr["valid"]).sum()) == 1
    n = len(Rr["pixel"])
    ref = F.scatter(F.records_of(np.full(n, 1e16), np.full(n, -1), np.full(n, -1)), Rr, pixels, np.ones((n, 3), f32))
    assert (ref["hit2"][0, :6] == F.EMPTY_HIT).all() and (ref["position2"][0, :6] == 0).all() and (ref["sky"][0, :6] == 0).all()
    assert (ref["ray"][0, :6].view(f32) == F.NEUTRAL_RAY).all()
    assert (ref["hit2"][1, 1] == F.INVALID_HIT).all() and (ref["sky"][1, 1] == 0).all() and np.isnan(ref["ray"][1, 1].view(f32)[4:7]).all()
    assert ref["ray"][1, 1].view(f32)[7] == f32(1e16)
    assert (ref["pixels"], ref["skipped"], ref["nonfinite"], ref["traced"], ref["invalid"], ref["hits"], ref["escaped"]) == (35, 1, 5, 29, 1, 0, 28)
    assert tuple(F.EMPTY_HIT.view(np.int32)) == (0, 0, 0, -1, -1, 0, 0, 0) and tuple(F.INVALID_HIT.view(np.int32)) == (0, 0, 0, -2, -1, 0, 0, 0)
