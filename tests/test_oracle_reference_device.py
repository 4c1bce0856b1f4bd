"""Frame orchestration against the REFERENCE's own device programs.  tests/golden/ref_frames.npz holds whole frames computed by
<variant>/deviceProgram.cu itself (raygen, closest-hit, miss, SampleLights, SampleShadow), run on the host through
oracle/ref_build/ref_device.cpp with the checker's ray search underneath; tests/golden/make_ref_frames.py writes it.
Always: the CPU checker reproduces every fixture frame bit for bit and the fixture's inputs are still the ones scenes.py makes.
Where oracle/_ref holds the libraries (the reference tree was there at build time): they still produce the fixture, and on
cameras and subframe indices drawn afresh the live reference equals the checker in both math flavours.  No tolerance anywhere."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal
from oracle import orc

GOLDEN = os.path.join(ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("make_ref_frames", os.path.join(GOLDEN, "make_ref_frames.py"))
MR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MR)
G = np.load(os.path.join(GOLDEN, "ref_frames.npz"))
NAMES = list(MR.ALL_CASES)


def assert_frames_equal(got, ref_bits, what, buffers=MR.BUFFERS):
    """got: dict of buffers; ref_bits: name -> uint32 bits.  Float buffers bit for bit (+-0 equal), frame_buffer exactly."""
    for k in buffers:
        if k == "frame":
            assert np.array_equal(got[k], ref_bits[k]), f"{what}: frame_buffer differs in {int((got[k] != ref_bits[k]).sum())} pixels"
        else:
            assert_bits_equal(got[k], ref_bits[k].view(np.float32), f"{what}: {k}_buffer")


def fixture_of(name):
    return {k: G[f"{name}.{k}"] for k in MR.BUFFERS}


@pytest.fixture(scope="module")
def case_inputs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = MR.inputs_of(MR.ALL_CASES[name])
        return cache[name]

    return get


def test_fixture_holds_every_case_and_every_branch():
    """One record per case of the generator, and, summed over the cases, every branch counter of the reference's run is > 0."""
    assert [str(n) for n in G["counter_names"]] == list(orc.REF_DEVICE_COUNTERS)
    total = np.zeros(len(orc.REF_DEVICE_COUNTERS), np.uint64)
    for name in NAMES:
        total += G[f"{name}.counters"]
    assert {f.split(".")[0] for f in G.files} - {"counter_names"} == set(NAMES)
    assert (total > 0).all(), dict(zip(orc.REF_DEVICE_COUNTERS, total.tolist()))
    # what single cases were chosen for
    c = lambda name, key: int(G[f"{name}.counters"][orc.REF_DEVICE_COUNTERS.index(key)])
    assert c("cornell_progressive", "clamp_active") > 0 and c("cornell_progressive", "emission_primary") > 0
    assert c("two_box_shadow_catcher", "catcher_pass_through") > 0 and c("catcher_stack", "catcher_pass_through") > 0
    assert c("terrain_all_materials", "transmission") > 0 and c("terrain_all_materials", "depth_cutoff") > 0
    assert c("textured", "textured_hit") > 0
    for name in MR.VARIANT_CASES:
        assert c(name, "depth_cutoff") > 0 and c(name, "transmission") > 0
    assert os.path.getsize(os.path.join(GOLDEN, "ref_frames.npz")) < os.path.getsize(os.path.join(GOLDEN, "ref_tables.npz"))


@pytest.mark.parametrize("name", NAMES)
def test_inputs_are_the_fixtures(name, case_inputs):
    """scenes.py, the probes, the camera frame and the launch sequence still produce the bytes the fixture was computed from."""
    assert MR.input_hash(MR.ALL_CASES[name], *case_inputs(name)) == str(G[f"{name}.inputs_sha256"])


@pytest.mark.parametrize("name", NAMES)
def test_checker_reproduces_reference_frames(orc_det, name, case_inputs):
    """oracle/pt_oracle.c (det) against the frame the reference's own programs computed: all five buffers (the two the program writes
    and three untouched ones for sv3 / sv4)."""
    got = MR.render_checker(orc_det, MR.ALL_CASES[name], case_inputs(name))
    assert_frames_equal(got, fixture_of(name), name)


def _devices(O):
    return {v: orc.load_ref_device(v, O) for v in orc.REF_DEVICE_VARIANTS}


def test_reference_device_libraries_built_by_clang(orc_det, orc_libm):
    """The jitter line make_float2(rnd(seed), rnd(seed)) depends on the order in which function arguments are evaluated: only a
    left-to-right compiler (clang) gives the x jitter the first draw, which is what the kernels and the checker assume of nvcc
    (DESIGN.md §3).  A library built by anything else must not pass as the pin.  Either all ten libraries are there or none."""
    devs = [(O, v, d) for O in (orc_det, orc_libm) for v, d in _devices(O).items()]
    present = [d is not None for _, _, d in devs]
    assert all(present) or not any(present), [(O.mode, v) for (O, v, d) in devs if d is None]
    for O, v, d in devs:
        if d is None:
            continue
        assert d.compiler.startswith("clang"), f"{d.path}: built by {d.compiler}"
        assert d.variant == v and d.detmath == (O.mode == "det") and d.foveated == (v != "original")


@pytest.mark.parametrize("name", NAMES)
def test_live_reference_equals_fixture(orc_det, name, case_inputs):
    """Where oracle/_ref holds the libraries: the reference's programs still compute the committed frames and counters."""
    case = MR.ALL_CASES[name]
    dev = orc.load_ref_device(case["program"], orc_det)
    if dev is None:
        return  # no reference tree at build time: test_checker_reproduces_reference_frames stands on the fixture
    assert dev.compiler.startswith("clang"), dev.compiler
    got, counters = MR.render_reference(dev, case, case_inputs(name))
    assert_frames_equal(got, fixture_of(name), f"live {name}")
    assert np.array_equal(counters, G[f"{name}.counters"]), dict(zip(orc.REF_DEVICE_COUNTERS, counters.tolist()))


@pytest.mark.parametrize("flavour", ["det", "libm"])
def test_live_reference_equals_checker_on_fresh_frames(flavour, orc_det, orc_libm, case_inputs):
    """Where oracle/_ref holds the libraries: every case again with a camera, subframe indices and (variants) gaze points drawn in
    the test, the reference's programs against the checker of the same math flavour, bit for bit in all five buffers."""
    O = orc_det if flavour == "det" else orc_libm
    devs = _devices(O)
    if any(d is None for d in devs.values()):
        return
    seed = int.from_bytes(os.urandom(4), "little")
    rng = np.random.default_rng(seed)
    for name, case in MR.ALL_CASES.items():
        model, probe, _ = case_inputs(name)
        cam = dict(case["cam"])
        eye, at = np.array(cam["eye"], np.float64), np.array(cam["lookat"], np.float64)
        dist = np.linalg.norm(eye - at)
        cam["eye"] = tuple(float(x) for x in eye + rng.uniform(-0.15, 0.15, 3) * dist)
        cam["fovY"] = float(cam["fovY"] * rng.uniform(0.7, 1.3))
        fresh = dict(case, cam=cam)
        if case["program"] == "original":
            start = int(rng.integers(0, 1000))
            fresh["subframe_list"] = [start, start + 1] if case["subframes"] > 1 else [start]
        else:
            fresh["gazes"] = [(int(rng.integers(12, 36)), int(rng.integers(12, 20))) for _ in range(2)]
        from optixpathtracer_amd import scenes

        inputs = (model, probe, scenes.uvw_frame(**cam, aspect=case["w"] / case["h"]))
        ref, _ = MR.render_reference(devs[case["program"]], fresh, inputs)
        got = MR.render_checker(O, fresh, inputs)
        assert_frames_equal(got, {k: MR.as_bits(ref[k]) for k in MR.BUFFERS}, f"{flavour} {name} (seed {seed})")
