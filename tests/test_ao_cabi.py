"""Ambient occlusion from the G-buffer (pt_ao_layout, pt_ao_planes) without a GPU: the entry points are declared and exported, the ctypes
mirrors match the compiler's layout, the header compiles as C99 and C++17 and states the rule, null arguments are refused before any device
work, both facades have the methods; and the float32 NumPy reference (tests/ao_ref.py) is held against its own geometry: an orthonormal
frame for every unit normal, directions in the upper hemisphere of unit length, a jitter that stays inside the table, and two analytic
scenes of quads under a float64 brute-force any-hit where the occlusion is exactly 1 and exactly 0."""
import ctypes as C
import re

import numpy as np
import pytest

import ao_ref as A
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_section
from dof_ref import directions
from optixpathtracer_amd import _lib
from optixpathtracer_amd import renderer as R

f32 = np.float32
u32 = np.uint32
DESC_FIELDS = ("hit", "position", "ao", "out", "bent", "scratch", "block_mask", "rays", "max_rays_in_flight", "radius", "bias", "seed", "flags")
STATS_FIELDS = ("pixels", "traced", "skipped", "nonfinite", "rays", "occluded", "invalid", "batches", "kernel_ms", "trace_ms")
NAMES = ("pt_ao_layout", "pt_ao_planes")


def test_library_exports_the_entry_points():
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert name in header().split("VERSIONING.")[1].split("*/")[0]
        assert name in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_ao_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_ao_desc\s*\*\s*\w+\s*,\s*pt_ao_stats\s*\*", src)
    assert re.search(r"int\s+pt_ao_layout\s*\(\s*const\s+pt_ctx\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*size_t\s*\*\s*\w+\s*\)", src)
    assert b"0.4" in L.pt_version()


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.AoDesc, "pt_ao_desc", DESC_FIELDS), (_lib.AoStats, "pt_ao_stats", STATS_FIELDS)],
                 [80, 0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72, 76] + [80, 0, 8, 16, 24, 32, 40, 48, 56, 64, 72])
    assert _lib.AO_PLANES == dict(hit=8, position=4, ao=1, out=4, bent=4) and _lib.AO_OUTPUTS == ("ao", "out", "bent")
    assert _lib.PT_AO_JITTER == 1 and _lib.PT_AO_MAX_RAYS == A.MAX_RAYS == 32
    m = re.search(r"#define\s+PT_AO_DEFAULT_RAYS_IN_FLIGHT\s+(\d+)u", header())
    assert m and int(m.group(1)) == _lib.PT_AO_DEFAULT_RAYS_IN_FLIGHT == A.DEFAULT_RAYS_IN_FLIGHT


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const void* hit, const float* position, float* ao, float* out, float* bent, void* scratch) {\n"
            "    pt_ao_desc d = {0, 0, 0, 0, 0, 0, 0, 4u, 0u, 0.5f, 1e-3f, 0u, 0u};\n"
            "    pt_ao_stats s;\n"
            "    size_t bytes = 0;\n"
            "    if (pt_ao_layout(c, d.rays, PT_AO_DEFAULT_RAYS_IN_FLIGHT, &bytes) || d.rays > PT_AO_MAX_RAYS) return 1;\n"
            "    d.hit = hit; d.position = position; d.ao = ao; d.out = out; d.bent = bent; d.scratch = scratch;\n"
            "    d.flags = PT_AO_JITTER;\n"
            "    return pt_ao_planes(c, &d, &s) || s.traced + s.skipped + s.nonfinite != s.pixels || s.occluded > s.rays || s.batches == 0 || s.trace_ms > s.kernel_ms;\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_header_states_the_rule():
    text = header_section("AMBIENT OCCLUSION FROM THE G-BUFFER", "int pt_ao_planes(")
    for item in ("If h.prim < 0 (a miss): ao = 1.0f, out = (1, 1, 1, 1), bent = (0, 0, 0, 1)", "or t > 0 is false",
                 "s = dot3(n0, E - P); n = (s < 0) ? -n0 : n0", "sg = (n.z >= 0) ? 1.0f : -1.0f; a = -1.0f / (sg + n.z); b = (n.x * n.y) * a",
                 "T = (1.0f + (sg * (n.x * n.x)) * a, sg * b, (-sg) * n.x); B = (b, sg + (n.y * n.y) * a, -n.y)",
                 "O = P + n * (bias * t) per component, the product first and then the sum",
                 "rho_k = sqrtf(((float)k + 0.5f) / (float)rays); Dk = D[(k + k0) & 127]", "k0 = h & 63",
                 "c_k = sqrtf(sel_max0(1.0f - (a_k*a_k + b_k*b_k)))", "w = ((T * a_k) + (B * b_k)) + (n * c_k) per component; d_k = normalize3(w)",
                 "(O, tmin = 0.0f, d_k, tmax = radius)", "An invalid ray is not traced; it counts as unoccluded",
                 "exactly what pt_trace_device(PT_QUERY_ANY) returns", "Back faces count", "ao = (float)open / (float)rays",
                 "bent.xyz = S / (float)rays", "for k ascending", "out = (ao, ao, ao, 1.0f)", "batches of floor(M / rays) pixels",
                 "256 + pixels * (40 * rays + 8), rounded up to 16", "The result does not depend on M, bit for bit", "PT_ERR_UNSUPPORTED",
                 "touches neither the context's query state, nor the frame buffers, nor pt_stats", "launches nothing and returns PT_OK"):
        assert item in text, item


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.AoDesc(), _lib.AoStats(7, 7, 7, 7, 7, 7, 7, 7, 7.0, 7.0)
    assert L.pt_ao_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_ao_planes: null context" in L.pt_last_error(None)
    assert L.pt_ao_planes(None, None, None) == -1
    nb = C.c_size_t(77)
    assert L.pt_ao_layout(None, 4, 0, C.byref(nb)) == -1 and b"pt_ao_layout: null context" in L.pt_last_error(None) and nb.value == 77
    assert tuple(getattr(s, n) for n in STATS_FIELDS) == (7, 7, 7, 7, 7, 7, 7, 7, 7.0, 7.0)


def test_facades_have_the_methods(tmp_path):
    import torch  # noqa: F401

    for name in ("aoLayout", "aoPlanes"):
        assert callable(getattr(R.SampleRenderer, name, None)) and callable(getattr(R._RankView, name, None))
    r = bare_renderer()
    hit, pos = fake_cuda((4, 4, 8)), fake_cuda((4, 4, 4))
    with pytest.raises(ValueError, match="radius is required"):
        r.aoPlanes(hit, pos)
    with pytest.raises(ValueError, match="rays must be 1..32, not 33"):
        r.aoPlanes(hit, pos, rays=33, radius=1.0)
    with pytest.raises(ValueError, match="max_rays_in_flight must be 0 or in"):
        r.aoPlanes(hit, pos, rays=4, radius=1.0, max_rays_in_flight=3)
    with pytest.raises(ValueError, match="hit is required"):
        r.aoPlanes(None, pos, radius=1.0)
    with pytest.raises(ValueError, match=r"bent: a contiguous torch.float32 tensor of shape \(4, 4, 4\) is expected"):
        r.aoPlanes(hit, pos, bent=fake_cuda((4, 4)), radius=1.0)
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t occlusion(SampleRenderer& sample, pt_ao_desc d) {\n"
        "    size_t bytes = sample.aoLayout(d.rays) + sample.aoLayout(d.rays, 1u << 20);\n"
        "    pt_ao_stats s{};\n"
        "    sample.aoPlanes(d, &s);\n"
        "    return sample.aoPlanes(d).occluded + s.batches + bytes;\n"
        "}\n")


# ------------------------------------------------------------------ the reference alone
def _unit_normals():
    rng = np.random.default_rng(11)
    v = rng.normal(size=(400, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    tiny, ulp = 1e-4, 2.0 ** -23
    special = [(np.sqrt(1 - (1 - ulp) ** 2), 0, -1 + ulp), (0, np.sqrt(1 - (1 - ulp) ** 2), 1 - ulp), (1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1),
               (np.sqrt(1 - (1 - tiny) ** 2), 0, -1 + tiny), (0, -np.sqrt(1 - (1 - tiny) ** 2), -1 + tiny), (0.0, 0.0, -0.0 + 1.0), (0.6, -0.8, 0.0), (0.6, 0.8, -0.0)]
    n = np.concatenate([v, np.array(special, np.float64)])
    n = np.concatenate([n, -n])
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)


def test_the_frame_is_orthonormal():
    n = _unit_normals()
    T, B = A.frame_of(n)
    T64, B64, n64 = T.astype(np.float64), B.astype(np.float64), n.astype(np.float64)
    for a, b, want in ((T64, T64, 1), (B64, B64, 1), (T64, B64, 0), (T64, n64, 0), (B64, n64, 0)):
        err = np.abs((a * b).sum(1) - want)
        assert err.max() <= 1e-6, err.max()
    assert np.abs(np.cross(T64, B64) - n64).max() <= 2e-6  # right-handed: T x B = n


@pytest.mark.parametrize("rays", [1, 4, 5, 32])
def test_directions_are_unit_and_in_the_upper_hemisphere(rays):
    n = _unit_normals()
    T, B = A.frame_of(n)
    for k0 in (0, 17, 63):
        d = A.sample_dirs(n, T, B, np.full(len(n), k0, np.int64), rays)
        assert d.dtype == f32 and A.ray_valid(np.concatenate([np.zeros((d.size // 3, 4), f32), d.reshape(-1, 3), np.ones((d.size // 3, 1), f32)], 1)).all()
        cosine = A.dot3(d, np.broadcast_to(n[:, None, :], d.shape))
        assert (cosine >= 0).all(), cosine.min()
        length = np.sqrt((d.astype(np.float64) ** 2).sum(-1))
        assert np.abs(length - 1).max() <= 2 * np.finfo(f32).eps, np.abs(length - 1).max()
    # cosine-weighted: the mean of dot(d, n) over the samples of the unjittered pattern approaches 2/3 from the stratified radii
    rho = A.rho_of(rays).astype(np.float64)
    assert abs(np.sqrt(1 - rho ** 2).mean() - 2 / 3) <= 0.2 / np.sqrt(rays) + 0.05


def test_the_jitter_stays_inside_the_table():
    D = directions()
    assert D.shape == (128, 2)
    ys, xs = np.mgrid[0:40, 0:64]
    for seed in (0, 1, 0xFFFFFFFF):
        k0 = A.jitter_of(xs, ys, seed)
        assert k0.min() >= 0 and k0.max() <= 63 and k0.max() + (A.MAX_RAYS - 1) <= 127
        assert len(np.unique(k0)) > 32
    assert A.rho_of(32).max() < 1 and A.rho_of(1)[0] == f32(np.sqrt(f32(0.5)))


def test_layout_and_batches():
    assert A.layout(40, 64, 4) == 256 + 2560 * 168 and A.layout(40, 64, 4, 4) == 256 + 168 + 8  # 432 is a multiple of 16
    assert A.layout(40, 64, 5, 7) == (256 + 208 + 15) // 16 * 16 and A.layout(40, 64, 4, 1 << 30) == A.layout(40, 64, 4)
    assert A.batches_of(2560, 40, 64, 4, 4) == 2560 and A.batches_of(2560, 40, 64, 4, 1000) == 11 and A.batches_of(0, 40, 64, 4) == 0


@pytest.mark.parametrize("rays", [1, 4, 8, 32])
@pytest.mark.parametrize("jitter", [False, True])
def test_two_analytic_scenes_are_exact(rays, jitter):
    """an open floor: ao == 1.0 exactly; a lid closer than the radius and wider than the radius around the probed pixels: ao == 0.0 exactly"""
    hit, P, cam = A.analytic_planes()
    h, w = hit.shape[:2]
    pixels = np.ones((h, w), bool)
    Rr = A.rays_of(hit, P, cam, None, pixels, rays, A.RADIUS, bias=1e-3, seed=3, jitter=jitter)
    assert Rr["valid"].all() and len(Rr["pixel"]) == h * w and (Rr["rays"][:, 4:7] @ np.array([0, 1, 0], f32) > 0).all()
    for ceiling, want in ((False, 1.0), (True, 0.0)):
        occ = A.any_hit_quads(Rr["rays"], A.analytic_quads(ceiling))
        ref = A.reduce(occ, Rr, rays, pixels)
        assert (ref["ao"].view(f32) == f32(want)).all() and (ref["out"].view(f32) == np.array([want, want, want, 1.0], f32)).all()
        assert (ref["bent"].view(f32)[..., 3] == f32(want)).all()
        assert ref["occluded"] == (h * w * rays if ceiling else 0) and ref["rays"] == h * w * rays and ref["traced"] == h * w
        if ceiling:
            assert (ref["bent"].view(f32)[..., 0:3] == 0).all()
        else:  # the mean of a cosine-weighted hemisphere's directions points along the normal
            b = ref["bent"].view(f32)[..., 0:3]
            assert (b[..., 1] > 0.5).all() and (np.abs(b[..., [0, 2]]) < 0.75).all()


def test_misses_and_hostile_records_shoot_no_ray():
    hit, P, cam = A.analytic_planes()
    hit, P = hit.copy(), P.copy()
    hit[0, 0, 3] = np.array([-1], np.int32).view(f32)[0]
    hit[0, 1, 5] = np.nan
    hit[0, 2, 0] = np.inf
    hit[0, 3, 0] = 0.0
    hit[0, 4, 0] = -1.0
    P[0, 5, 2] = -np.inf
    hit[0, 6, 3] = np.array([0x7FFFFFF0], np.int32).view(f32)[0]  # a stale primitive: processed
    pixels = np.ones(hit.shape[:2], bool)
    Rr = A.rays_of(hit, P, cam, None, pixels, 4, A.RADIUS)
    assert Rr["skipped"].sum() == 1 and Rr["nonfinite"].sum() == 5 and Rr["traced"][0, 6] and len(Rr["pixel"]) == pixels.size - 6
    ref = A.reduce(np.zeros(len(Rr["rays"]), np.int32), Rr, 4, pixels)
    one = f32(1).view(u32)
    assert (ref["ao"][0, :6] == one).all() and (ref["bent"][0, :6] == (0, 0, 0, one)).all() and (ref["out"][0, :6] == one).all()
    assert (ref["pixels"], ref["skipped"], ref["nonfinite"], ref["traced"]) == (35, 1, 5, 29)
