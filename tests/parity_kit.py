"""A frame of the renderer beside the same frame of the CPU checker: how the parity tests build a context, render on both sides and
compare all five buffers.  The bodies need a GPU; importing the module does not."""
import numpy as np

from conftest import assert_bits_equal
from optixpathtracer_amd import scenes


def _renderer(model, probe, cam, w, h, **opt):
    from optixpathtracer_amd.renderer import SampleRenderer, make_camera

    r = SampleRenderer(model)
    r.setProbe(probe)
    r.resize((w, h))
    r.setCamera(make_camera(cam, w / h))
    if opt:
        r.setOptions(**opt)
    return r


def _oracle_render(O, model, probe, cam, w, h, spp, subframes=1, max_depth=8, bsdf_mode=0, use_bvh=None):
    sc = O.make_scene(model, use_bvh)
    pr = O.make_probe(probe)
    U, V, W = scenes.uvw_frame(**cam, aspect=w / h)
    out, accum = None, None
    rays = 0
    for sf in range(subframes):
        out = O.render(sc, pr, (U, V, W), cam["eye"], w, h, spp, max_depth, sf, bsdf_mode, accum)
        accum = out["accum"]
        rays += out["radiance_rays"] + out["shadow_rays"]
    return out


def _gpu_render(r, spp, subframes=1):
    from optixpathtracer_amd import renderer as R

    r.launchParams.samples_per_launch = spp
    for sf in range(subframes):
        r.launchParams.frame.subframe_index = sf
        r.render()
    return dict(
        accum=r.download(R.PT_BUF_ACCUM), frame=r.download(R.PT_BUF_FRAME), normal=r.download(R.PT_BUF_NORMAL),
        color=r.download(R.PT_BUF_COLOR), albedo=r.download(R.PT_BUF_ALBEDO), stats=r.stats(),
    )


def _compare(g, o):
    assert_bits_equal(g["accum"], o["accum"], "accum_buffer")
    assert_bits_equal(g["color"], o["color"], "color_buffer")
    assert_bits_equal(g["normal"], o["normal"], "normal_buffer")
    assert_bits_equal(g["albedo"], o["albedo"], "albedo_buffer")
    assert np.array_equal(g["frame"], o["frame"]), "frame_buffer (rgba8)"


def _check_sched(g, sched):
    st = g["stats"]
    if sched == "fused":
        assert st["fused_passes"] >= 1 and st["shade_launches"] == 0, st
    else:
        assert st["fused_passes"] == 0 and st["shade_launches"] >= 1, st


# ---------------------------------------------------------------- ray search
def _random_rays(rng, n, lo, hi, tmin=1e-3):
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, np.full((n, 1), tmin, np.float32), d, np.full((n, 1), 1e16, np.float32)], 1).astype(np.float32)
