"""The cases of tests/test_gpu_horizon.py (its docstring describes the scene and the probes), shared with the generator of their recorded
counts, tests/golden/make_horizon_counts.py.  Rendering needs a GPU; importing the module does not."""
import json
import math
import os

import numpy as np

from conftest import assert_bits_equal
from optixpathtracer_amd import scenes


W, H, SPP, DEPTH = 64, 64, 2, 3
MARGIN = 1.0e-4  # PT_HORIZON_MARGIN
CAMERA = dict(eye=(0.5, 3.0, -8.0), lookat=(0.0, 0.6, 0.0), up=(0.0, 1.0, 0.0), fovY=45.0)
COUNTS = ("radiance_rays", "shadow_rays", "shaded_hits", "total_radiance_rays", "total_shadow_rays")
MATERIALS = {
    "plain": dict(color=(0.7, 0.6, 0.5)),
    "subsurface": dict(color=(0.8, 0.4, 0.3), subsurface=0.5, roughness=0.7),
    "glass": dict(color=(0.9, 0.9, 0.95), transmission=1.0, roughness=0.2),
}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "horizon_counts.json")
DEPTH_CASES = (("plain", 0, "sky"), ("subsurface", 0, "bright_ground"))  # (material, BSDF mode, probe) of the depth 1 / depth 2 test


def quad_scene(material, catcher_ground=False):
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    quads = [
        [(-4, 0, -4), (-4, 0, 4), (0, 0, 4), (0, 0, -4)],  # ground: cross(v1 - v0, v2 - v0) points up
        [(0, 0, -4), (0, 0, 4), (4, 0, 4), (4, 0, -4)][::-1],  # the same kind of quad beside it, reversed winding
        [(-2.5 - c, 1.0 - s, 0.0), (-2.5 - c, 1.0 - s, 2.0), (-2.5 + c, 1.0 + s, 2.0), (-2.5 + c, 1.0 + s, 0.0)],  # tilted by 30 degrees about z
        [(-3, 0, 3), (-3, 3, 3), (3, 3, 3), (3, 0, 3)],  # vertical wall behind them, facing the camera
    ]
    m = scenes.Model()
    for k, q in enumerate(quads):
        mat = scenes.Material(**material)
        if catcher_ground and k < 2:
            mat["flags"] |= scenes.MATERIAL_FLAG_SHADOW_CATCHER
        m.meshes.append(scenes._quads_to_mesh([q], mat))
    return m


def bright_ground_probe():
    data = np.ones((32, 64, 4), np.float32)
    data[:16, :, :3] = (0.15, 0.2, 0.3)  # sky
    data[16:, :, :3] = (1.2, 1.0, 0.8)  # ground
    data[20:24, 10:20, :3] = 6.0  # and a bright patch in it, so that the conditional CDFs are not uniform
    return scenes.ProbeData(64, 32, data)


PROBES = {"sky": lambda: scenes.sky_probe(256, 128), "bright_ground": bright_ground_probe}


def render(monkeypatch, model, probe, fused, bsdf_mode, max_depth=DEPTH, split_shadow=0, carry=True):
    """one context; returns (buffers, counts, stats)"""
    from optixpathtracer_amd import renderer as R

    monkeypatch.setenv("PT_FUSED", "2" if fused else "0")
    monkeypatch.setenv("PT_CARRY_SUMS", "1" if carry else "0")
    r = R.SampleRenderer(model)
    r.setProbe(probe)
    r.setOptions(max_depth=max_depth, bsdf_mode=bsdf_mode, split_shadow=split_shadow)
    r.resize((W, H))
    r.setCamera(R.make_camera(CAMERA, W / H))
    r.launchParams.samples_per_launch = SPP
    r.launchParams.frame.subframe_index = 0
    r.render()
    st = r.stats()
    out = {name: r.download(b).copy() for name, b in (("accum", R.PT_BUF_ACCUM), ("color", R.PT_BUF_COLOR), ("normal", R.PT_BUF_NORMAL), ("albedo", R.PT_BUF_ALBEDO))}
    out["frame"] = r.downloadPixels().copy()
    r.close()
    monkeypatch.delenv("PT_FUSED")
    monkeypatch.delenv("PT_CARRY_SUMS")
    return out, {k: int(st[k]) for k in COUNTS}, st


def checker(orc_det, model, probe, bsdf_mode, max_depth=DEPTH):
    U, V, Wv = scenes.uvw_frame(**CAMERA, aspect=W / H)
    return orc_det.render(orc_det.make_scene(model), orc_det.make_probe(probe), (U, V, Wv), CAMERA["eye"], W, H, SPP, max_depth=max_depth, bsdf_mode=bsdf_mode)


def same_as_checker(g, o, what):
    for k in ("accum", "color", "normal", "albedo"):
        assert_bits_equal(g[0][k], o[k], f"{what}: {k}")
    assert np.array_equal(g[0]["frame"], o["frame"]), f"{what}: frame"
    # (the chain never traces more than the reference's raygen loop: DESIGN.md, ray accounting)
    assert g[1]["radiance_rays"] <= o["radiance_rays"] and g[1]["shadow_rays"] <= o["shadow_rays"], (what, g[1], o["radiance_rays"], o["shadow_rays"])


def golden_counts(key, counts):
    want = json.load(open(GOLDEN))[key]
    assert counts == want, (key, counts, want)


def case_key(material, mode, probe, schedule, max_depth=DEPTH):
    return f"{material}/{'lambert' if mode else 'disney'}/{probe}/{schedule}/d{max_depth}"


def run_case(monkeypatch, orc_det, probes, material, mode, probe_name, max_depth=DEPTH, check=True):
    """the three schedules of one case: launch chain, fused loop, launch chain with the ground as shadow catcher; returns {key: counts}"""
    probe = probes[probe_name]
    model = quad_scene(MATERIALS[material])
    chain = render(monkeypatch, model, probe, False, mode, max_depth)
    fused = render(monkeypatch, model, probe, True, mode, max_depth)
    cmodel = quad_scene(MATERIALS[material], catcher_ground=True)
    catcher = render(monkeypatch, cmodel, probe, False, mode, max_depth)
    assert chain[2]["fused_passes"] == 0 and chain[2]["shade_launches"] >= 1 and catcher[2]["fused_passes"] == 0, (material, mode, probe_name, "the launch chain", chain[2], catcher[2])
    assert fused[2]["fused_passes"] >= 1 and fused[2]["shade_launches"] == 0, (material, mode, probe_name, "the fused loop", fused[2])
    counts = {case_key(material, mode, probe_name, s, max_depth): r[1] for s, r in (("chain", chain), ("fused", fused), ("catcher", catcher))}
    print(counts)
    if check:
        o = checker(orc_det, model, probe, mode, max_depth)
        same_as_checker(chain, o, "launch chain")
        same_as_checker(fused, o, "fused loop")
        same_as_checker(catcher, checker(orc_det, cmodel, probe, mode, max_depth), "shadow-catcher ground")
        assert chain[1] == fused[1], (chain[1], fused[1])
        n = chain[0]["normal"][..., :3].astype(np.float64)
        up = n[..., 1] > 0.99 * np.maximum(np.linalg.norm(n, axis=-1), 1e-30)
        assert up.mean() >= 0.2, up.mean()  # a fifth of the frame's first hits are on the up-facing quads, where the rows below the horizon are skipped
        for k, c in counts.items():
            golden_counts(k, c)
    return counts
