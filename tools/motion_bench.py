#!/usr/bin/env python3
"""motion_bench.py — what the object-motion pass costs (pt_motion_planes), beside the temporal pass it feeds and the snapshot it needs.

Scene: the C3 terrain (1 M triangles), 1920 x 1080, the terrain camera; the previous camera is the eye 0.25 to the side.  One step of the
loop is set up once — snapshot, the terrain's largest band turned and shifted with a refit, G-buffer of this frame and of the last — and then,
in ONE run, medians over --reps calls after two warm-up calls:
  (a) kernel_ms of motionPlanes, all three planes — pt_motion_stats.kernel_ms, hipEvents around the kernel — and of each plane alone
  (b) beside it: kernel_ms of temporalAccumulate (k_temporal) fed those planes, on a random history
  (c) copyVerticesDevice, host time of the whole call (a device-to-device copy of vertices * 12 bytes and a stream wait)
  (d) the floor: a plain device-to-device copy that moves the pass's plane bytes — 32 read, 56 written per pixel (the gathered indices and
      vertices come on top and are shared between the pixels of a triangle)
There is no pass/fail ratio: nobody had measured the pass when this tool was written.  Printed as ONE JSON object; --md PATH also writes
the table as markdown with the raw JSON below it, replacing that file's part from "## Timings" on.
  timeout -k 10 300 python3 tools/motion_bench.py [--reps 7] [--md profiles/motion.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
PLANE_BYTES = 32 + 8 + 16 + 32


def copy_ms(torch, nbytes, reps):
    src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda:0").normal_()
    dst = torch.empty_like(src)
    rows = []
    for k in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        if k >= 2:
            rows.append(e0.elapsed_time(e1))
    return float(np.median(rows))


def markdown(res):
    px = res["pixels"]
    md = ["## Timings (`tools/motion_bench.py`)\n",
          f"C3 terrain, {res['triangles']} triangles, {res['vertices']} vertices, {W} x {H} = {px} pixels, {res['hits']} of them hits, one MI355X; medians of "
          f"{res['reps']} after 2 warm-ups, one run.  Device times by hipEvents unless said otherwise.  No pass/fail ratio is attached to these figures.\n",
          "| what | ms |", "|---|---|",
          f"| (a) `motionPlanes`, three planes: `kernel_ms` (`k_motion`) | {res['motion_ms']['all']:.4f} |"]
    for name in ("motion", "prev_point", "prev_surface"):
        md.append(f"| (a) `{name}` alone | {res['motion_ms'][name]:.4f} |")
    md += [f"| (b) `temporalAccumulate` fed those planes: `kernel_ms` (`k_temporal`), {res['reprojected']} pixels reprojected | {res['temporal_ms']:.4f} |",
           f"| (b) the same with the camera-only planes, {res['reprojected_camera_only']} pixels reprojected | {res['temporal_camera_only_ms']:.4f} |",
           f"| (c) `copyVerticesDevice`, {res['vertices'] * 12} bytes: host time of the call | {res['snapshot_host_ms']:.4f} |",
           f"| (d) device-to-device copy of the pass's plane bytes ({PLANE_BYTES} B/pixel read + written) | {res['copy_plane_bytes_ms']:.4f} |",
           f"| (a) / (d) | {res['motion_ms']['all'] / res['copy_plane_bytes_ms']:.2f} |",
           f"| (a) / (b) | {res['motion_ms']['all'] / res['temporal_ms']:.2f} |",
           "", "## Raw output\n", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--md", help="also write the table as markdown to this path")
    args = ap.parse_args()
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    dev = "cuda:0"
    model = scenes.voxel_terrain()
    r = R.SampleRenderer(model)
    r.resize((W, H))
    cam, prev = scenes.TERRAIN_CAMERA, dict(scenes.TERRAIN_CAMERA, eye=(scenes.TERRAIN_CAMERA["eye"][0] + 0.25,) + tuple(scenes.TERRAIN_CAMERA["eye"][1:]))
    prev_cam = R.make_camera(prev, W / H)
    r.setCamera(prev_cam)
    old = r.renderGBuffer(("hit", "position"))
    snapshot = r.copyVerticesDevice()
    rows = []
    for k in range(args.reps + 2):
        t0 = time.perf_counter()
        r.copyVerticesDevice(out=snapshot)
        if k >= 2:
            rows.append((time.perf_counter() - t0) * 1e3)
    snapshot_ms = float(np.median(rows))
    mesh = int(np.argmax([len(m.vertex) for m in model.meshes]))
    c, s = np.cos(0.03), np.sin(0.03)
    r.transformMeshes({mesh: np.array([[c, 0, s, 1.5], [0, 1, 0, 0.8], [-s, 0, c, -1.0]], np.float32)})
    r.setCamera(R.make_camera(cam, W / H))
    g = r.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev_cam)
    out = {k: torch.zeros((H, W, n), device=dev) for k, n in (("motion", 2), ("prev_point", 4), ("prev_surface", 8))}
    motion_ms = {}
    for name, planes in (("all", tuple(out)), ("motion", ("motion",)), ("prev_point", ("prev_point",)), ("prev_surface", ("prev_surface",))):
        rows = []
        for k in range(args.reps + 2):
            st = r.motionPlanes(g["hit"], snapshot, prev_cameras=prev_cam, planes=planes, out={p: out[p] for p in planes})["stats"]
            if k >= 2:
                rows.append(st["kernel_ms"])
        motion_ms[name] = float(np.median(rows))
        if name == "all":
            hits = int(st["hits"])
    gen = torch.Generator(device=dev).manual_seed(1)
    colour, history = torch.rand((H, W, 4), device=dev, generator=gen), torch.rand((H, W, 4), device=dev, generator=gen)
    length = torch.randint(0, 10, (H, W), device=dev, generator=gen).float()
    hist_out, len_out = torch.zeros((H, W, 4), device=dev), torch.zeros((H, W), device=dev)
    temporal = {}
    for name, geo in (("object", (out["motion"], out["prev_surface"], out["prev_point"])), ("camera", (g["motion"], g["hit"], g["position"]))):
        rows = []
        for k in range(args.reps + 2):
            st = r.temporalAccumulate(colour, *geo, old["hit"], old["position"], history, length, history_out=hist_out, length_out=len_out)["stats"]
            if k >= 2:
                rows.append(st["kernel_ms"])
        temporal[name] = (float(np.median(rows)), int(st["reprojected"]))
    nv, nt = r.vertexCount()
    r.close()
    res = dict(triangles=nt, vertices=nv, pixels=W * H, reps=args.reps, hits=hits, moved_mesh=mesh, motion_ms=motion_ms, temporal_ms=temporal["object"][0],
               reprojected=temporal["object"][1], temporal_camera_only_ms=temporal["camera"][0], reprojected_camera_only=temporal["camera"][1],
               snapshot_host_ms=snapshot_ms, plane_bytes_per_pixel=PLANE_BYTES, copy_plane_bytes_ms=copy_ms(torch, PLANE_BYTES * W * H // 2, args.reps))
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Object motion for the chain (`pt_motion_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
