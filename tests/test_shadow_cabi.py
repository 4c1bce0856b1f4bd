"""Sun shadows and direct light from the G-buffer (pt_shadow_layout, pt_shadow_planes) without a GPU: the entry points are declared and
exported, the ctypes mirrors match the compiler's layout, the header compiles as C99 and C++17 and states the rule, null arguments are
refused before any device work, both facades have the methods and check their arguments; and the float32 NumPy reference
(tests/shadow_ref.py) is held against its own geometry: every sample inside the light's cone, a point light's samples all the light's
direction, a jitter that changes the spiral's start and nothing else, and ao_ref's floor and lid under a light straight up and straight
down, judged by a float64 brute-force any-hit."""
import ctypes as C
import re

import numpy as np
import pytest

import shadow_ref as S
from cabi_kit import bare_renderer, check_layout, compile_c99_and_cxx17, compile_facade, fake_cuda, header, header_section
from dof_ref import jitter_of
from optixpathtracer_amd import _lib
from optixpathtracer_amd import renderer as R

f32 = np.float32
u32 = np.uint32
LIGHT_FIELDS = ("dir", "spread", "radiance", "rays")
DESC_FIELDS = ("hit", "position", "view_ray", "visibility", "light", "scratch", "block_mask", "lights", "num_lights", "max_rays_in_flight",
               "max_distance", "bias", "seed", "flags")
STATS_FIELDS = ("pixels", "traced", "skipped", "nonfinite", "backfacing", "rays", "occluded", "invalid", "batches", "kernel_ms", "trace_ms")
NAMES = ("pt_shadow_layout", "pt_shadow_planes")
SEVENS = (7, 7, 7, 7, 7, 7, 7, 7, 7, 7.0, 7.0)
UP = ((0.0, 1.0, 0.0), 0.0, (2.0, 1.5, 1.0), 1)
DOWN = ((0.0, -1.0, 0.0), 0.0, (2.0, 1.5, 1.0), 3)


def test_library_exports_the_entry_points():
    L = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert name in header().split("VERSIONING.")[1].split("*/")[0]
        assert name in header().split("STREAM CONTRACT.")[1].split("VERSIONING.")[0]
    assert re.search(r"int\s+pt_shadow_planes\s*\(\s*pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_shadow_desc\s*\*\s*\w+\s*,\s*pt_shadow_stats\s*\*", src)
    assert re.search(r"int\s+pt_shadow_layout\s*\(\s*const\s+pt_ctx\s*\*\s*\w+\s*,\s*const\s+pt_shadow_light\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,"
                     r"\s*uint32_t\s+\w+\s*,\s*size_t\s*\*\s*\w+\s*\)", src)
    assert b"0.4" in L.pt_version()


def test_struct_layouts_match_the_compiler(tmp_path):
    check_layout(tmp_path, [(_lib.ShadowLight, "pt_shadow_light", LIGHT_FIELDS), (_lib.ShadowDesc, "pt_shadow_desc", DESC_FIELDS),
                            (_lib.ShadowStats, "pt_shadow_stats", STATS_FIELDS)],
                 [32, 0, 12, 16, 28] + [88, 0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76, 80, 84] + [88, 0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80])
    assert _lib.SHADOW_PLANES == dict(hit=8, position=4, view_ray=8, visibility=4, light=4) and _lib.SHADOW_OUTPUTS == S.PLANES
    assert _lib.PT_SHADOW_JITTER == 1 and _lib.PT_SHADOW_MAX_RAYS == S.MAX_RAYS == 32 and _lib.PT_SHADOW_MAX_LIGHTS == S.MAX_LIGHTS == 4
    for name, want in (("PT_SHADOW_MAX_LIGHTS", 4), ("PT_SHADOW_MAX_RAYS", 32)):
        m = re.search(r"#define\s+%s\s+(\d+)\b" % name, header())
        assert m and int(m.group(1)) == want, name
    m = re.search(r"#define\s+PT_SHADOW_DEFAULT_RAYS_IN_FLIGHT\s+(\d+)u", header())
    assert m and int(m.group(1)) == _lib.PT_SHADOW_DEFAULT_RAYS_IN_FLIGHT == S.DEFAULT_RAYS_IN_FLIGHT


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    body = ('#include "pt_amd.h"\n'
            "int use(pt_ctx* c, const void* hit, const float* position, const float* ray, float* visibility, float* light, void* scratch) {\n"
            "    pt_shadow_light sun[PT_SHADOW_MAX_LIGHTS] = {{{0.3f, 1.0f, 0.2f}, 0.01f, {3.0f, 2.9f, 2.7f}, 8u}, {{0.0f, 1.0f, 0.0f}, 0.0f, {0.1f, 0.1f, 0.2f}, 1u}};\n"
            "    pt_shadow_desc d = {0, 0, 0, 0, 0, 0, 0, 0, 2u, 0u, 1e16f, 1e-3f, 0u, 0u};\n"
            "    pt_shadow_stats s;\n"
            "    size_t bytes = 0;\n"
            "    if (pt_shadow_layout(c, sun, d.num_lights, PT_SHADOW_DEFAULT_RAYS_IN_FLIGHT, &bytes) || sun[0].rays + sun[1].rays > PT_SHADOW_MAX_RAYS) return 1;\n"
            "    d.hit = hit; d.position = position; d.view_ray = ray; d.visibility = visibility; d.light = light; d.scratch = scratch; d.lights = sun;\n"
            "    d.flags = PT_SHADOW_JITTER;\n"
            "    return pt_shadow_planes(c, &d, &s) || s.traced + s.skipped + s.nonfinite != s.pixels || s.occluded > s.rays || s.backfacing > 4 * s.traced ||\n"
            "           s.invalid > s.rays + s.invalid || s.batches == 0 || s.trace_ms > s.kernel_ms;\n"
            "}\n")
    compile_c99_and_cxx17(tmp_path, body)


def test_header_states_the_rule():
    text = header_section("SUN SHADOWS AND DIRECT LIGHT FROM THE G-BUFFER", "int pt_shadow_planes(")
    for item in ("L_i = normalize3(dir_i)", "the frame of pt_ao_planes's step 4 with L_i in place of n", "visibility = (1, 1, 1, 1), light = (0, 0, 0, 1)",
                 "or t > 0 is false", "one of view_ray[p]'s first three words is not finite", "E = view_ray[p].xyz when view_ray is given",
                 "n = dot3(ng, E - P) < 0 ? -ng : ng", "O = P + n * (bias * t) per component, the product first and then the sum", "c = dot3(n, L_i)",
                 "If c > 0.0f is false", "v_i = 0.0f, no ray is shot", "stats->backfacing counts the pair", "c_i = c > 1.0f ? 1.0f : c",
                 "rho = sqrtf(((float)k + 0.5f) / (float)rays_i)", "Dk = D[(k + k0) & 127]", "k0 = pass_hash(x, y, seed + i) & 63", "it wraps",
                 "a = (rho * Dk.x) * spread_i; b = (rho * Dk.y) * spread_i", "w = (L_i + T_i * a) + B_i * b per component; d = normalize3(w)",
                 "(O, tmin = 0.0f, d, tmax = max_distance)", "an invalid ray is not traced, counts as unoccluded", "exactly what pt_trace_device(PT_QUERY_ANY) returns",
                 "the tree decides", "v_i = (float)open_i / (float)rays_i", "(i >= num_lights) have v_i = 1.0f", "starts at +0 and adds radiance_i * (c_i * v_i) per component",
                 "light.w = 1.0f", "batches of floor(M / R) pixels", "256 + pixels * (40 * R + 32), rounded up to 16", "The result does not depend on M, bit for bit",
                 "PT_ERR_UNSUPPORTED", "dot3(L, L) > 0.5f", "spread not finite or outside [0, 1]", "launches nothing and returns PT_OK"):
        assert item in text, item


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib.load_library()
    d, s = _lib.ShadowDesc(), _lib.ShadowStats(*SEVENS)
    assert L.pt_shadow_planes(None, C.byref(d), C.byref(s)) == -1
    assert b"pt_shadow_planes: null context" in L.pt_last_error(None)
    assert L.pt_shadow_planes(None, None, None) == -1
    nb = C.c_size_t(77)
    sun = (_lib.ShadowLight * 1)()
    assert L.pt_shadow_layout(None, sun, 1, 0, C.byref(nb)) == -1 and b"pt_shadow_layout: null context" in L.pt_last_error(None) and nb.value == 77
    assert L.pt_shadow_layout(None, None, 0, 0, None) == -1
    assert tuple(getattr(s, n) for n in STATS_FIELDS) == SEVENS


def test_facades_have_the_methods_and_check_their_arguments(tmp_path):
    import torch  # noqa: F401

    for name in ("shadowLayout", "shadowPlanes"):
        assert callable(getattr(R.SampleRenderer, name, None)) and callable(getattr(R._RankView, name, None))
    r = bare_renderer()
    hit, pos = fake_cuda((4, 4, 8)), fake_cuda((4, 4, 4))
    sun = dict(dir=(0.0, 1.0, 0.0), spread=0.01, radiance=(1.0, 1.0, 1.0), rays=4)
    with pytest.raises(ValueError, match="lights is required"):
        r.shadowPlanes(hit, pos)
    with pytest.raises(ValueError, match="1..4 lights are expected, not 0"):
        r.shadowPlanes(hit, pos, lights=[])
    with pytest.raises(ValueError, match="1..4 lights are expected, not 5"):
        r.shadowPlanes(hit, pos, lights=[sun] * 5)
    with pytest.raises(ValueError, match="light 1: rays must be >= 1, not 0"):
        r.shadowPlanes(hit, pos, lights=[sun, dict(sun, rays=0)])
    with pytest.raises(ValueError, match="the lights' rays add up to 33, above 32"):
        r.shadowPlanes(hit, pos, lights=[dict(sun, rays=16), dict(sun, rays=17)])
    with pytest.raises(ValueError, match="the lights' rays add up to 33, above 32"):
        r.shadowLayout([((0, 1, 0), 0.0, (1, 1, 1), 33)])
    with pytest.raises(ValueError, match="max_rays_in_flight must be 0 or in"):
        r.shadowPlanes(hit, pos, lights=sun, max_rays_in_flight=3)
    with pytest.raises(ValueError, match="max_rays_in_flight must be 0 or in"):
        r.shadowLayout([sun], 2**32)
    with pytest.raises(ValueError, match="seed must be in"):
        r.shadowPlanes(hit, pos, lights=sun, seed=-1)
    with pytest.raises(ValueError, match="dir and radiance must be three floats"):
        r.shadowPlanes(hit, pos, lights=[((0, 1), 0.0, (1, 1, 1), 1)])
    with pytest.raises(ValueError, match="hit is required"):
        r.shadowPlanes(None, pos, lights=sun)
    with pytest.raises(ValueError, match="position is required"):
        r.shadowPlanes(hit, None, lights=sun)
    with pytest.raises(ValueError, match=r"view_ray: a contiguous torch.float32 tensor of shape \(4, 4, 8\) is expected"):
        r.shadowPlanes(hit, pos, lights=sun, view_ray=fake_cuda((4, 4, 4)))
    with pytest.raises(ValueError, match=r"visibility: a contiguous torch.float32 tensor of shape \(4, 4, 4\) is expected"):
        r.shadowPlanes(hit, pos, lights=sun, visibility=fake_cuda((4, 4)))
    arr = R.SampleRenderer._shadow_lights("shadowPlanes", [sun, _lib.ShadowLight((1.0, 2.0, 3.0), 0.5, (0.0, 1.0, 2.0), 27), ((0, 0, 1), 1.0, (3, 2, 1), 1)])
    assert len(arr) == 3 and tuple(arr[1].dir) == (1.0, 2.0, 3.0) and arr[1].spread == 0.5 and tuple(arr[1].radiance) == (0.0, 1.0, 2.0) and arr[1].rays == 27
    assert arr[0].rays == 4 and arr[0].spread == f32(0.01) and tuple(arr[2].dir) == (0.0, 0.0, 1.0) and arr[2].rays == 1
    lone = R.SampleRenderer._shadow_lights("shadowPlanes", ((0, 0, 1), 1.0, (3, 2, 1), 5))  # one light as a bare tuple, not four lights
    assert len(lone) == 1 and tuple(lone[0].dir) == (0.0, 0.0, 1.0) and lone[0].rays == 5
    four = R.SampleRenderer._shadow_lights("shadowPlanes", tuple(((0, 0, 1), 1.0, (3, 2, 1), k + 1) for k in range(4)))
    assert len(four) == 4 and [l.rays for l in four] == [1, 2, 3, 4]
    compile_facade(
        tmp_path,
        '#include "optixpathtracer_amd/csrc/SampleRenderer.h"\n'
        "using namespace ptamd;\n"
        "uint64_t sun(SampleRenderer& sample, pt_shadow_desc d) {\n"
        "    size_t bytes = sample.shadowLayout(d.lights, d.num_lights) + sample.shadowLayout(d.lights, d.num_lights, 1u << 20);\n"
        "    pt_shadow_stats s{};\n"
        "    sample.shadowPlanes(d, &s);\n"
        "    return sample.shadowPlanes(d).occluded + s.backfacing + s.batches + bytes;\n"
        "}\n")


# ------------------------------------------------------------------ the reference alone
def _unit_dirs():
    rng = np.random.default_rng(12)
    v = rng.normal(size=(400, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


@pytest.mark.parametrize("spread", [0.0, 0.01, 0.3, 1.0])
def test_every_sample_lies_inside_the_lights_cone(spread):
    """dot3(d_k, L) >= 1 / sqrt(1 + spread^2) - 2e-6: |(a, b)| = rho * spread <= spread puts w inside the cone exactly; the margin is a
    dozen float32 roundings (2^-24 each) on unit vectors, as in the reflection's identity"""
    dirs = _unit_dirs()
    assert len(dirs) == 400
    L = S.normalize3(dirs)  # what lights_of makes of a dir
    T, B = S.frame_of(L)
    one = S.lights_of([(tuple(dirs[7]), spread, (1, 1, 1), 3)])
    assert np.array_equal(one["L"][0].view(u32), L[7].view(u32)) and np.array_equal(one["T"][0].view(u32), T[7].view(u32)) and np.array_equal(one["B"][0].view(u32), B[7].view(u32))
    bound = 1.0 / np.sqrt(1.0 + spread * spread) - 2e-6
    for rays in (1, 5, 32):
        for k0 in (0, 17, 63):
            d = S.sample_dirs(L, T, B, spread, rays, np.full(len(L), k0, np.int64))
            assert d.dtype == f32 and d.shape == (400, rays, 3)
            assert S.ray_valid(np.concatenate([np.zeros((d.size // 3, 4), f32), d.reshape(-1, 3), np.ones((d.size // 3, 1), f32)], 1)).all()
            cosine = (d.astype(np.float64) * L.astype(np.float64)[:, None, :]).sum(-1)
            assert (cosine >= bound).all(), (spread, rays, k0, cosine.min())
            if spread == 0.0:
                want = S.normalize3(L)
                assert (d.view(u32) == want.view(u32)[:, None, :]).all(), "a point light's samples are all normalize3(L), bit for bit"
    if spread > 0:  # the widest sample comes close to the cone's edge: the bound is not slack
        widest = (S.sample_dirs(L, T, B, spread, 32, np.zeros(len(L), np.int64)).astype(np.float64) * L.astype(np.float64)[:, None, :]).sum(-1).min()
        assert widest <= 1.0 / np.sqrt(1.0 + (S.rho_of(32)[-1] * spread) ** 2) + 2e-6


LIGHTS = [((0.3, 1.0, 0.2), 0.3, (3.0, 2.5, 2.0), 5), ((-1.0, 0.4, 0.1), 0.05, (0.2, 0.3, 0.5), 3), ((0.0, 1.0, 0.0), 0.0, (1.0, 1.0, 1.0), 1)]


def test_jitter_changes_the_spirals_start_and_nothing_else():
    hit, P, cam = S.analytic_planes()
    h, w = hit.shape[:2]
    pixels = np.ones((h, w), bool)
    plain = S.rays_of(hit, P, cam, None, pixels, LIGHTS, 10.0)
    ys, xs = np.mgrid[0:h, 0:w]
    for seed in (1, 0xFFFFFFFF):
        jit = S.rays_of(hit, P, cam, None, pixels, LIGHTS, 10.0, seed=seed, jitter=True)
        for name in ("pixel", "first", "c", "valid", "O", "n"):
            assert np.array_equal(jit[name], plain[name]), name
        assert np.array_equal(jit["rays"][:, [0, 1, 2, 3, 7]].view(u32), plain["rays"][:, [0, 1, 2, 3, 7]].view(u32))
        Lt = plain["lights"]
        for i, (_, spread, _, rays) in enumerate(LIGHTS):
            assert (plain["first"][:, i] >= 0).all()
            k0 = jitter_of(xs.reshape(-1), ys.reshape(-1), u32((seed + i) & 0xFFFFFFFF))  # (the addition wraps: seed 0xFFFFFFFF, light 1 hashes 0)
            assert k0.min() >= 0 and k0.max() <= 63 and k0.max() + S.MAX_RAYS - 1 <= 127
            want = S.sample_dirs(Lt["L"][i], Lt["T"][i], Lt["B"][i], spread, rays, k0)
            idx = jit["first"][:, i][:, None] + np.arange(rays)[None, :]
            assert np.array_equal(jit["rays"][idx][..., 4:7].view(u32), want.view(u32)), (seed, i)
            moved = (jit["rays"][idx][..., 4:7].view(u32) != plain["rays"][idx][..., 4:7].view(u32)).any()
            assert moved == (spread > 0), "the jitter turns a disc's pattern and leaves a point light's alone"
    assert np.array_equal(jitter_of(xs, ys, u32(0)), jitter_of(xs, ys, u32((0xFFFFFFFF + 1) & 0xFFFFFFFF)))


def test_absent_lights_are_fully_visible():
    hit, P, cam = S.analytic_planes()
    pixels = np.ones(hit.shape[:2], bool)
    for nl in (1, 2, 3):
        Rr = S.rays_of(hit, P, cam, None, pixels, LIGHTS[:nl], 10.0)
        ref = S.reduce(np.ones(len(Rr["rays"]), np.int32), Rr, LIGHTS[:nl], pixels)
        v = ref["visibility"].view(f32)
        assert (v[..., :nl] == 0).all() and (v[..., nl:] == 1).all() and (ref["light"].view(f32) == np.array([0, 0, 0, 1], f32)).all()
        assert ref["occluded"] == ref["rays"] == pixels.sum() * S.total_rays(LIGHTS[:nl]) and ref["backfacing"] == 0


def test_layout_and_batches():
    four, one = [((0, 1, 0), 0, (1, 1, 1), r) for r in (1, 3, 8, 16)], [((0, 1, 0), 0, (1, 1, 1), 1)]
    assert S.total_rays(four) == 28
    assert S.layout(40, 64, four) == 256 + 2560 * (40 * 28 + 32) and S.layout(40, 64, four, 28) == 256 + 1120 + 32
    assert S.layout(40, 64, one, 1) == (256 + 72 + 15) // 16 * 16 == 336 and S.layout(40, 64, four, 1 << 30) == S.layout(40, 64, four)
    assert S.batches_of(2560, 40, 64, four, 28) == 2560 and S.batches_of(2560, 40, 64, four, 28 * 1000) == 3 and S.batches_of(0, 40, 64, four) == 0


# ------------------------------------------------------------------ the analytic scene: ao_ref's floor and lid
def test_a_light_straight_up_sees_the_lids_shadow():
    """floor points under the lid have v = 0, the others v = 1, by a float64 brute force; the frame is chosen so that no point lies within
    1e-3 of the lid's projected edge"""
    hit, P, cam = S.analytic_planes()
    h, w = hit.shape[:2]
    pixels = np.ones((h, w), bool)
    under, undecided = S.under_the_lid(P)
    assert undecided.sum() <= 0.05 * h * w
    assert undecided.sum() == 0, "the frame was chosen to leave none out"
    assert 0.2 * h * w < under.sum() < 0.8 * h * w
    Rr = S.rays_of(hit, P, cam, None, pixels, [UP], 10.0)
    assert Rr["valid"].all() and len(Rr["rays"]) == h * w and (Rr["rays"][:, 4:7] == np.array([0, 1, 0], f32)).all() and (Rr["c"] == 1).all()
    occ = S.any_hit_quads(Rr["rays"], S.analytic_quads(True))
    ref = S.reduce(occ, Rr, [UP], pixels)
    v = ref["visibility"].view(f32)
    keep = ~undecided
    assert (v[..., 0][keep & under] == 0).all() and (v[..., 0][keep & ~under] == 1).all() and (v[..., 1:] == 1).all()
    lit = ref["light"].view(f32)
    assert (lit[~under] == np.array([2.0, 1.5, 1.0, 1.0], f32)).all() and (lit[under] == np.array([0, 0, 0, 1], f32)).all()
    assert (ref["pixels"], ref["traced"], ref["backfacing"], ref["rays"], ref["occluded"], ref["invalid"]) == (h * w, h * w, 0, h * w, int(under.sum()), 0)
    # without the lid nothing is in the way
    open_ = S.reduce(S.any_hit_quads(Rr["rays"], S.analytic_quads(False)), Rr, [UP], pixels)
    assert open_["occluded"] == 0 and (open_["visibility"].view(f32) == 1).all()


def test_a_light_straight_down_is_under_every_horizon():
    hit, P, cam = S.analytic_planes()
    h, w = hit.shape[:2]
    pixels = np.ones((h, w), bool)
    Rr = S.rays_of(hit, P, cam, None, pixels, [DOWN], 10.0)
    assert len(Rr["rays"]) == 0 and (Rr["first"] == -1).all()
    ref = S.reduce(np.zeros(0, np.int32), Rr, [DOWN], pixels)
    assert (ref["backfacing"], ref["rays"], ref["occluded"], ref["traced"]) == (h * w, 0, 0, h * w)
    assert (ref["light"].view(f32) == np.array([0, 0, 0, 1], f32)).all()
    assert (ref["visibility"].view(f32) == np.array([0, 1, 1, 1], f32)).all()


def test_misses_and_hostile_records_shoot_no_ray():
    hit, P, cam = S.analytic_planes()
    hit, P = hit.copy(), P.copy()
    ray = np.zeros(hit.shape, f32)
    ray[..., 0:3] = S.ANALYTIC_EYE
    hit[0, 0, 3] = np.array([-1], np.int32).view(f32)[0]
    hit[0, 1, 5] = np.nan
    hit[0, 2, 0] = np.inf
    hit[0, 3, 0] = 0.0
    P[0, 4, 2] = -np.inf
    ray[0, 5, 1] = np.nan
    ray[0, 6, 3:8] = np.nan  # only the origin counts
    hit[0, 7, 3] = np.array([0x7FFFFFF0], np.int32).view(f32)[0]  # a stale primitive: processed
    pixels = np.ones(hit.shape[:2], bool)
    Rr = S.rays_of(hit, P, cam, None, pixels, [UP], 10.0, view_ray=ray)
    assert Rr["skipped"].sum() == 1 and Rr["nonfinite"].sum() == 5 and Rr["traced"][0, 6] and Rr["traced"][0, 7]
    ref = S.reduce(np.zeros(len(Rr["rays"]), np.int32), Rr, [UP], pixels)
    one = f32(1).view(u32)
    assert (ref["visibility"][0, :6] == one).all() and (ref["light"][0, :6] == (0, 0, 0, one)).all()
    assert (ref["pixels"], ref["skipped"], ref["nonfinite"], ref["traced"]) == (pixels.size, 1, 5, pixels.size - 6)
    # view_ray's origin decides the facing: from under the floor the normal turns down, and the light straight up is behind it
    below = ray.copy()
    below[..., 1] = -6.0
    Rb = S.rays_of(hit, P, cam, None, pixels, [UP], 10.0, view_ray=below)
    assert len(Rb["rays"]) == 0 and (Rb["n"][:, 1] == -1).all()
