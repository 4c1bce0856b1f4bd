"""The HIP kernels against frames the REFERENCE's own device programs computed (tests/golden/ref_frames.npz: <variant>/deviceProgram.cu run on
the host, tests/golden/make_ref_frames.py).  Every other GPU parity test compares with oracle/pt_oracle.c, a restatement written
by the same hands as the kernels; here the sample loop, the RNG stream order, the RadiancePRD state machine, the MIS weight, the
composition, the clamp and lerp of later subframes and the AOVs are the reference's own lines.  The canonical program goes through pt_render
with the launch chain (k_generate / k_shade / k_resolve) and with the fused bounce loop (k_path_loop), the foveated programs through
pt_render_regions (k_generate_region / k_resolve_region) with the matching pt_variant.  Bit for bit, reading only the fixture."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("make_ref_frames", os.path.join(GOLDEN, "make_ref_frames.py"))
MR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MR)
G = np.load(os.path.join(GOLDEN, "ref_frames.npz"))


def _context(case, **opt):
    from optixpathtracer_amd.renderer import SampleRenderer, make_camera

    r = SampleRenderer(case["scene"]())
    r.setProbe(case["probe"]().BuildCDF())
    r.resize((case["w"], case["h"]))
    r.setCamera(make_camera(case["cam"], case["w"] / case["h"]))
    r.setOptions(**opt)
    return r


def _compare(r, name, buffers):
    from optixpathtracer_amd import renderer as R

    which = dict(accum=R.PT_BUF_ACCUM, frame=R.PT_BUF_FRAME, normal=R.PT_BUF_NORMAL, color=R.PT_BUF_COLOR, albedo=R.PT_BUF_ALBEDO)
    for k in buffers:
        got, ref = r.download(which[k]), G[f"{name}.{k}"]
        if k == "frame":
            assert np.array_equal(got, ref), f"{name}: frame_buffer differs in {int((got != ref).sum())} pixels"
        else:
            assert_bits_equal(got, ref.view(np.float32), f"{name}: {k}_buffer")


def _render_original(monkeypatch, name, fused, frames_in_flight=0):
    case = MR.ALL_CASES[name]
    if fused is not None:
        monkeypatch.setenv("PT_FUSED", fused)  # read per context at pt_create
        monkeypatch.setenv("PT_SCHED_TRIALS", "0")
        monkeypatch.setenv("PT_FUSED_MAX_COST", "1e9")
    r = _context(case, max_depth=8, frames_in_flight=frames_in_flight)
    r.launchParams.samples_per_launch = case["spp"]
    for (sf,) in MR.frames_of(case):
        r.launchParams.frame.subframe_index = sf
        r.render()
    _compare(r, name, MR.BUFFERS)
    st = r.stats()
    r.close()
    return st


@pytest.mark.parametrize("fused", ["0", "1"], ids=["chain", "fused"])
@pytest.mark.parametrize("name", list(MR.CASES))
def test_pt_render_equals_reference_program(ptlib, monkeypatch, name, fused):
    """HelloPathtracing_original/deviceProgram.cu: all five buffers after the case's subframes, through both schedules of a frame."""
    st = _render_original(monkeypatch, name, fused)
    # a scene with a shadow-catcher material never takes the fused loop (include/pt_amd.h): PT_FUSED=1 leaves it on the chain
    catcher = any(int(m.material["flags"]) & 1 for m in MR.CASES[name]["scene"]().meshes)
    if fused == "1" and not catcher:
        assert st["fused_passes"] >= 1 and st["shade_launches"] == 0, st
    else:
        assert st["fused_passes"] == 0 and st["shade_launches"] >= 1, st


@pytest.mark.parametrize("name", ["cornell_progressive", "odd_33x9_progressive"])
def test_pt_render_three_frames_in_flight_equals_reference_program(ptlib, monkeypatch, name):
    """The progressive cases (subframes 0..3, each lerping onto the one before) with three frames in flight and nothing read in between."""
    _render_original(monkeypatch, name, None, frames_in_flight=3)


@pytest.mark.parametrize("name", list(MR.VARIANT_CASES))
def test_pt_render_regions_equals_reference_variant_program(ptlib, name):
    """HelloPathtracing_sv, _sv2, _sv3, _sv4_vmv23/deviceProgram.cu: three frames of three launches around a moving gaze point.  sv3 and sv4
    write accum_buffer and frame_buffer; sv and sv2 also the three AOV buffers."""
    case = MR.ALL_CASES[name]
    r = _context(case, max_depth=case["max_depth"])
    variant = MR.variant_of(case)
    for k, gaze in enumerate(case["gazes"]):
        assert r.launchParams.frame.subframe_index == k
        r.renderFoveated(gaze, inner_radius=case["inner_radius"], outer_radius=case["outer_radius"], spp=case["spp"], variant=variant)
    _compare(r, name, MR.written_buffers(case))
    r.close()
