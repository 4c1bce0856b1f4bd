#!/usr/bin/env python3
"""Generates tests/golden/ref_frames.npz: small whole frames computed by the REFERENCE's own device programs
(<variant>/deviceProgram.cu: raygen, closest-hit, miss, SampleLights, SampleShadow), run on the host through
oracle/_ref/libptref_device_<variant>_det.so (oracle/ref_build/ref_device.cpp; built by `make -C oracle ref` where the reference tree
exists).  The ray search, the barycentrics and the texture filter are the checker's own; the transcendentals are
those of include/pt_detmath.h, so the bits do not depend on the machine.  Per case the file holds the five buffers as uint32 bits,
the branch counters of the run (oracle.orc.REF_DEVICE_COUNTERS) and a SHA-256 of every input byte, so that a later change of
scenes.py is noticed instead of compared silently.

The script refuses to write a file in which a branch counter is zero over all cases, or in which a library was not built by clang
(argument evaluation order of the jitter line).  Run:  python tests/golden/make_ref_frames.py

tests/test_oracle_reference_device.py and tests/test_gpu_reference_frames.py import the case tables and helpers below."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from optixpathtracer_amd import scenes  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_frames.npz")
BUFFERS = ("accum", "frame", "normal", "color", "albedo")
TEXTURED_CAMERA = dict(eye=(3.0, 2.5, -4.5), lookat=(0.0, 0.6, 0.5), up=(0.0, 1.0, 0.0), fovY=45.0)


def _sky():
    return scenes.sky_probe(256, 128)


def _terrain():
    return scenes.voxel_terrain(n=48, target_tris=15000)


# The canonical program (HelloPathtracing_original): plain width x height launches of subframes 0 .. subframes-1, depth cutoff 8.
CASES = {
    # subframes 0..3 under the sky probe: the ceiling light (emission 15 on camera hits) makes the clamp to 10 of subframes > 0 bite
    "cornell_progressive": dict(scene=scenes.cornell_box, cam=scenes.CORNELL_CAMERA, probe=_sky, w=48, h=32, spp=2, subframes=4),
    "two_box_shadow_catcher": dict(scene=lambda: scenes.two_box_scene(shadow_catcher=True), cam=scenes.TWO_BOX_CAMERA, probe=scenes.disc_probe, w=48, h=32, spp=2, subframes=2),
    # secondary rays cross catcher slabs and go on (the --prd->depth pass-through), with ordinary geometry behind
    "catcher_stack": dict(scene=scenes.catcher_stack_scene, cam=scenes.TWO_BOX_CAMERA, probe=scenes.disc_probe, w=40, h=24, spp=1, subframes=1),
    # 15 k triangles through the checker's BVH, all eight material presets (glass: transmission, bsdfPdf <= 0)
    "terrain_all_materials": dict(scene=_terrain, cam=scenes.TERRAIN_CAMERA, probe=_sky, w=40, h=24, spp=2, subframes=2),
    # texcoord interpolation and hasTexture && texcoord, including the mesh with a texture id but no texcoords
    "textured": dict(scene=scenes.textured_scene, cam=TEXTURED_CAMERA, probe=_sky, w=48, h=32, spp=2, subframes=1),
    # odd size, one sample, disc probe, subframes 0..3
    "odd_33x9_progressive": dict(scene=lambda: scenes.two_box_scene(shadow_catcher=False), cam=scenes.TWO_BOX_CAMERA, probe=scenes.disc_probe, w=33, h=9, spp=1, subframes=4),
}

# The foveated programs: per frame the three launches of SampleRenderer.foveatedRegions (periphery 1/4 resolution accumulating,
# annulus 1/2 and fovea 1/1 redrawn) around a moving gaze point.  48 x 32 with radii 4 / 10 is the smallest frame at which all
# three annuli hold pixels and every splat stays inside the image (a splat clamped at the border is a write race of the reference).
_FOV = dict(scene=_terrain, cam=scenes.TERRAIN_CAMERA, probe=_sky, w=48, h=32, gazes=[(24, 16), (26, 14), (18, 20)], inner_radius=4, outer_radius=10, spp=(1, 2, 4))
VARIANT_CASES = {
    # name: program directory, the pt_variant the project renders it with (attribute of SampleRenderer), its depth cutoff
    "sv4_three_launches": dict(_FOV, program="sv4_vmv23", variant="SV4_VARIANT", max_depth=4),
    "sv3_three_launches": dict(_FOV, program="sv3", variant="SV3_VARIANT", max_depth=4),
    "sv_three_launches": dict(_FOV, program="sv", variant="SV_VARIANT", max_depth=3),
    "sv2_three_launches": dict(_FOV, program="sv2", variant="SV_VARIANT", max_depth=3),
}
ALL_CASES = dict({k: dict(v, program="original") for k, v in CASES.items()}, **VARIANT_CASES)


def variant_of(case):
    from optixpathtracer_amd.renderer import SampleRenderer

    return getattr(SampleRenderer, case["variant"])


def frames_of(case):
    """The launch sequence: a list of frames, each a list of launches; a launch is a pt_region dict, or an int (the subframe
    index of a plain width x height launch)."""
    if case["program"] == "original":
        return [[sf] for sf in case.get("subframe_list", range(case["subframes"]))]
    from optixpathtracer_amd.renderer import SampleRenderer

    return [SampleRenderer.foveatedRegions((case["w"], case["h"]), g, k, case["inner_radius"], case["outer_radius"], case["spp"]) for k, g in enumerate(case["gazes"])]


def inputs_of(case):
    model, probe = case["scene"](), case["probe"]().BuildCDF()
    uvw = scenes.uvw_frame(**case["cam"], aspect=case["w"] / case["h"])
    return model, probe, uvw


def input_hash(case, model, probe, uvw):
    h = hashlib.sha256()
    verts, idx, tri_mesh, mats = model.flatten()
    arrs = [verts, idx, tri_mesh, mats]
    if (getattr(model, "textures", []) or []) or any(m.diffuseTextureID >= 0 for m in model.meshes):
        tc, mesh_tex, has_uv = model.flatten_textures()
        arrs += [tc if tc is not None else np.zeros(0, np.float32), mesh_tex, has_uv] + [t.pixel for t in model.textures]
    arrs += [np.asarray(a, np.float32) for a in (probe.data, probe.pdfValuesX, probe.cdfValuesX, probe.pdfValuesY, probe.cdfValuesY)]
    arrs += [np.asarray(case["cam"]["eye"], np.float32)] + [np.asarray(v, np.float32) for v in uvw]
    for a in arrs:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    h.update(repr((case["w"], case["h"], case["spp"], frames_of(case))).encode())
    return h.hexdigest()


def new_buffers(case):
    w, h = case["w"], case["h"]
    return dict(accum=np.zeros((h, w, 4), np.float32), frame=np.zeros((h, w), np.uint32), normal=np.zeros((h, w, 4), np.float32),
                color=np.zeros((h, w, 4), np.float32), albedo=np.zeros((h, w, 4), np.float32))


def render_checker(O, case, inputs=None):
    """The case through the CPU checker (oracle/pt_oracle.c): the five buffers after the last launch."""
    model, probe, uvw = inputs or inputs_of(case)
    sc, pr = O.make_scene(model, None), O.make_probe(probe)
    w, h, eye = case["w"], case["h"], case["cam"]["eye"]
    b = new_buffers(case)
    for frame in frames_of(case):
        if case["program"] == "original":
            out = O.render(sc, pr, uvw, eye, w, h, case["spp"], 8, frame[0], 0, b["accum"], 4)
            b = {k: out[k] for k in BUFFERS}
        else:
            O.render_regions(sc, pr, uvw, eye, w, h, frame, variant_of(case), case["max_depth"], b["accum"], b["frame"], aov=[b["normal"], b["color"], b["albedo"]])
    return b


def render_reference(dev, case, inputs=None):
    """The case through the reference's device programs (orc.RefDevice of the case's program): buffers and branch counters."""
    model, probe, uvw = inputs or inputs_of(case)
    sc, pr = dev.make_scene(model, None), dev.O.make_probe(probe)
    b = new_buffers(case)
    counters = None
    for frame in frames_of(case):
        for launch in frame:
            if case["program"] == "original":
                counters = dev.launch(sc, pr, uvw, case["cam"]["eye"], case["w"], case["h"], case["spp"], launch, b, counters=counters)
            else:
                counters = dev.launch(sc, pr, uvw, case["cam"]["eye"], case["w"], case["h"], 0, 0, b, region=launch, counters=counters)
    return b, counters


def written_buffers(case):
    """sv3 / sv4 write accum_buffer and frame_buffer only; the original, sv and sv2 all five."""
    return BUFFERS if case["program"] == "original" or variant_of(case).get("write_aov") else ("accum", "frame")


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint32 else a.view(np.uint32)


def main():
    from oracle import orc

    O = orc.Oracle("det")
    G, total = {}, np.zeros(len(orc.REF_DEVICE_COUNTERS), np.uint64)
    for name, case in ALL_CASES.items():
        dev = orc.load_ref_device(case["program"], O)
        assert dev is not None, f"oracle/_ref holds no device library for {case['program']}: run make -C oracle ref"
        assert dev.compiler.startswith("clang"), dev.compiler
        inputs = inputs_of(case)
        b, counters = render_reference(dev, case, inputs)
        for k in BUFFERS:
            G[f"{name}.{k}"] = as_bits(b[k])
        G[f"{name}.counters"] = counters
        G[f"{name}.inputs_sha256"] = np.array(input_hash(case, *inputs))
        total += counters
        print(f"{name:28s}", dict(zip(orc.REF_DEVICE_COUNTERS, counters.tolist())))
    G["counter_names"] = np.array(orc.REF_DEVICE_COUNTERS)
    print(f"{'all cases':28s}", dict(zip(orc.REF_DEVICE_COUNTERS, total.tolist())))
    zero = [n for n, c in zip(orc.REF_DEVICE_COUNTERS, total) if c == 0]
    assert not zero, f"no case reaches: {zero} (change a case, not this condition)"
    np.savez_compressed(PATH, **G)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
