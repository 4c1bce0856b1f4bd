"""Launch shapes of the kernels around the traversal launches: k_shade / k_shade_carry in workgroups of 64, 128 or 256
threads (PT_SHADE_WG), their LDS copy of the probe's marginal arrays with or without pdfY (PT_SHADE_LDS=full|lean), and the generate /
resolve kernels in 64-thread workgroups (PT_SMALL_WG).  A shape only moves where the work runs: grid x workgroup stays the same number of
threads, so every thread shades the entries it shades in the default shape, and only the order of the entries inside a queue changes.
Every case therefore renders once with the default context and once per shape, in this process, as a launch chain (PT_FUSED=0: the fused
loop of a small frame launches none of these kernels), and compares all five buffers word for word and the device-counted totals."""
import itertools

import numpy as np
import pytest

from gpu_kit import same
from optixpathtracer_amd import scenes
from parity_kit import _compare, _gpu_render, _oracle_render, _renderer

pytestmark = pytest.mark.gpu

COUNTS = ("radiance_rays", "shadow_rays", "shaded_hits")
BUFFERS = ("accum", "color", "normal", "albedo", "frame")
SHAPES = [(wg, lds, small) for wg, lds, small in itertools.product((64, 128, 256), ("full", "lean"), (0, 1))]
TEXTURED_CAMERA = dict(eye=(3.0, 2.5, -4.5), lookat=(0.0, 0.6, 0.5), up=(0.0, 1.0, 0.0), fovY=45.0)
DISNEY, LAMBERT = 0, 1


def _case(name):
    """model, probe, camera, (w, h), spp, options, extra environment.  The sky probe (128 rows) has its marginal arrays copied to LDS; the
    disc probe's 50 rows are no multiple of the search block, so it has no count tables and its marginals stay in global memory."""
    sky = lambda: scenes.sky_probe(256, 128).BuildCDF()  # noqa: E731
    if name.startswith("cornell_72x40"):  # 5760 paths, then queues of any length: no multiple of a workgroup, the last wave is partial
        mode = LAMBERT if "lambert" in name else DISNEY
        env = {"PT_CARRY_SUMS": "0"} if "write_back" in name else {}  # k_shade<MODE, false>: a scene without catchers, sums not carried
        return scenes.cornell_box(), sky(), scenes.CORNELL_CAMERA, (72, 40), 2, dict(max_depth=4, bsdf_mode=mode), env
    if name.startswith("cornell_8x8"):  # 64 paths: the later queues hold fewer than 64 entries, most workgroups find no work
        depth = int(name.rsplit("_d", 1)[1])  # 0 and 1: the chain's first launch is also its last
        return scenes.cornell_box(), sky(), scenes.CORNELL_CAMERA, (8, 8), 1, dict(max_depth=depth), {}
    if name == "catcher_64x64":  # k_shade<MODE, true>, and the extra iterations of paths that pass through a catcher
        return scenes.two_box_scene(shadow_catcher=True), sky(), scenes.TWO_BOX_CAMERA, (64, 64), 1, dict(max_depth=3), {}
    if name == "textured_64x64":  # the table of the 256 byte values, filled by workgroups of 64 threads
        return scenes.textured_scene(), sky(), TEXTURED_CAMERA, (64, 64), 1, dict(max_depth=2), {}
    if name == "global_marginals":
        return scenes.cornell_box(), scenes.disc_probe(100, 50).BuildCDF(), scenes.CORNELL_CAMERA, (72, 40), 2, dict(max_depth=3), {}
    raise KeyError(name)


CASES = ["cornell_72x40_disney", "cornell_72x40_lambert", "cornell_72x40_disney_write_back", "cornell_8x8_d0", "cornell_8x8_d1", "cornell_8x8_d2",
         "catcher_64x64", "textured_64x64", "global_marginals"]
_DEFAULT = {}  # case -> the default context's render: computed once, shared by the shapes, never written to


def _render(monkeypatch, name, env):
    model, probe, cam, (w, h), spp, opt, extra = _case(name)
    env = {"PT_FUSED": "0", **extra, **env}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = _renderer(model, probe, cam, w, h, **opt)  # the switches are read once, at pt_create
    for k in env:
        monkeypatch.delenv(k)
    g = _gpu_render(r, spp)
    g = {k: (np.array(v) if k in BUFFERS else v) for k, v in g.items()}
    r.close()
    assert g["stats"]["fused_passes"] == 0 and g["stats"]["shade_launches"] >= 1, g["stats"]
    return g


def _default(monkeypatch, name):
    if name not in _DEFAULT:
        for k in ("PT_SHADE_WG", "PT_SHADE_LDS", "PT_SMALL_WG"):
            monkeypatch.delenv(k, raising=False)
        g = _render(monkeypatch, name, {})
        for k in BUFFERS:
            g[k].setflags(write=False)
        _DEFAULT[name] = g
    return _DEFAULT[name]


@pytest.mark.parametrize("wg,lds,small", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_shape_leaves_the_default_contexts_bits(ptlib, monkeypatch, name, wg, lds, small):
    ref = _default(monkeypatch, name)
    got = _render(monkeypatch, name, {"PT_SHADE_WG": str(wg), "PT_SHADE_LDS": lds, "PT_SMALL_WG": str(small)})
    what = f"{name}: PT_SHADE_WG={wg} PT_SHADE_LDS={lds} PT_SMALL_WG={small} against the default context"
    same({k: got[k] for k in BUFFERS}, ref, what)
    counts = {k: got["stats"][k] for k in COUNTS}
    assert counts == {k: ref["stats"][k] for k in COUNTS}, (what, counts)
    assert got["stats"]["shade_launches"] == ref["stats"]["shade_launches"], what


def test_cases_reach_both_sides_of_their_branches(ptlib, monkeypatch):
    """what the cases are chosen for, checked on the default context's own figures"""
    d = {n: _default(monkeypatch, n)["stats"] for n in CASES}
    assert d["cornell_8x8_d0"]["shade_launches"] == 1 and d["cornell_8x8_d1"]["shade_launches"] == 1  # first launch = last launch
    assert d["cornell_8x8_d0"]["shadow_rays"] == 0 and d["cornell_8x8_d1"]["shadow_rays"] > 0
    assert d["cornell_8x8_d2"]["shade_launches"] == 2 and d["cornell_8x8_d2"]["shaded_hits"] < 2 * 64  # a second queue of fewer than 64 entries
    assert d["cornell_72x40_disney"]["schedule"] & 0x200 and not d["cornell_72x40_disney_write_back"]["schedule"] & 0x200  # carried sums / write-back
    assert not d["catcher_64x64"]["schedule"] & 0x200
    assert d["global_marginals"]["shadow_rays"] > 0  # light samples were drawn from the probe whose marginals stay in global memory


@pytest.mark.parametrize("wg,lds", [(64, "full"), (64, "lean"), (128, "lean")])
def test_textured_scene_against_the_checker(ptlib, orc_det, monkeypatch, wg, lds):
    """workgroups smaller than the 256-entry byte table fill all of it: the texture lookups of the CPU checker, bit for bit"""
    model, probe, cam, (w, h), spp, opt, _ = _case("textured_64x64")
    got = _render(monkeypatch, "textured_64x64", {"PT_SHADE_WG": str(wg), "PT_SHADE_LDS": lds, "PT_SMALL_WG": "1"})
    _compare(got, _oracle_render(orc_det, model, probe, cam, w, h, spp, max_depth=opt["max_depth"], use_bvh=False))


@pytest.mark.parametrize("env", [{"PT_SHADE_WG": "32"}, {"PT_SHADE_WG": "512"}, {"PT_SHADE_LDS": "small"}])
def test_unknown_shape_is_refused(ptlib, monkeypatch, env):
    from optixpathtracer_amd.renderer import SampleRenderer

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(Exception, match="PT_SHADE_"):
        SampleRenderer(scenes.cornell_box())
