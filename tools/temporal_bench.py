#!/usr/bin/env python3
"""temporal_bench.py — what the temporal accumulation pass costs (pt_temporal_accumulate) against the memory traffic it cannot avoid.

Scene: the C3 terrain (1 M triangles), 1920 x 1080, the terrain camera; the previous camera is the current one moved by 0.25 in x.  The
G-buffer planes of both cameras come from renderGBuffer, the colour is one rendered frame, the history is random with lengths 1..8.  In ONE
run, medians over --reps calls after two warm-up calls:
  (a) kernel_ms of temporalAccumulate with all four outputs and the clear flag — pt_temporal_stats.kernel_ms, hipEvents around the pass
  (b) the yardstick: a plain device-to-device copy that moves the pass's UNIQUE bytes — every plane read once (140 bytes per pixel) and
      every output written once (40 bytes, and 16 for the cleared colour): a copy of half that many bytes reads and writes that much —
      and, beside it, a copy of twice the size, timed with events on the same device
The pass is a gather: a pixel touches up to 368 bytes, neighbours share taps, so (a) / (b) says how much of the sharing the caches deliver.
There is no pass/fail ratio: nobody had measured the pass when this tool was written.  Printed as ONE JSON object; --md PATH also writes
the table as markdown with the raw JSON below it, replacing that file's part from "## Timings" on.
  timeout -k 10 300 python3 tools/temporal_bench.py [--reps 7] [--md profiles/temporal.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
READ_BYTES = 16 + 8 + 32 + 16 + 32 + 16 + 16 + 4  # color, motion, hit, position, prev_hit, prev_position, history_in, length_in
WRITE_BYTES = 16 + 4 + 4 + 16 + 16  # history_out, length_out, frame_rgba8, copy_out, the cleared colour
UNIQUE_BYTES = READ_BYTES + WRITE_BYTES


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
    md = ["## Timings (`tools/temporal_bench.py`)\n",
          f"C3 terrain, {res['triangles']} triangles, {W} x {H} = {res['pixels']} pixels, {res['reprojected']} of them reprojected, one MI355X; medians of "
          f"{res['reps']} after 2 warm-ups.  Device times by hipEvents.  No pass/fail ratio is attached to these figures.\n",
          "| what | ms | GB/s |", "|---|---|---|",
          f"| (a) `temporalAccumulate`, four outputs, clear flag: `kernel_ms` | {res['kernel_ms']:.4f} | {res['unique_bytes'] / res['kernel_ms'] / 1e6:.0f} of unique bytes |",
          f"| (b) device-to-device copy moving the unique bytes ({res['unique_bytes_per_pixel']} B/pixel read + written) | {res['copy_unique_ms']:.4f} | {res['unique_bytes'] / res['copy_unique_ms'] / 1e6:.0f} |",
          f"| (b') copy of twice that | {res['copy_double_ms']:.4f} | {2 * res['unique_bytes'] / res['copy_double_ms'] / 1e6:.0f} |",
          f"| (a) / (b) | {res['kernel_ms'] / res['copy_unique_ms']:.3f} | |",
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
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.resize((W, H))
    cam = R.make_camera(scenes.TERRAIN_CAMERA, W / H)
    ex, ey, ez = scenes.TERRAIN_CAMERA["eye"]
    prev = R.make_camera(dict(scenes.TERRAIN_CAMERA, eye=(ex + 0.25, ey, ez)), W / H)
    r.setCamera(prev)
    old = r.renderGBuffer(("hit", "position"))
    r.setCamera(cam)
    cur = r.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev)
    r.launchParams.samples_per_launch = 1
    r.launchParams.frame.subframe_index = 0
    r.render()
    colour = torch.from_numpy(r.download(R.PT_BUF_ACCUM)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    hist = torch.rand((H, W, 4), device=dev, generator=gen)
    length = torch.randint(1, 9, (H, W), device=dev, generator=gen).float()
    out = dict(history_out=torch.zeros((H, W, 4), device=dev), length_out=torch.zeros((H, W), device=dev),
               frame_rgba8=torch.zeros((H, W), dtype=torch.int32, device=dev), copy_out=torch.zeros((H, W, 4), device=dev))
    rows = []
    for k in range(args.reps + 2):
        c = colour.clone()  # the clear flag zeroes it
        s = r.temporalAccumulate(c, cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], hist, length, **out, clear_color=True)["stats"]
        if k >= 2:
            rows.append(s["kernel_ms"])
    r.close()
    unique = UNIQUE_BYTES * W * H
    res = dict(triangles=model.num_triangles, pixels=W * H, reps=args.reps, reprojected=int(s["reprojected"]), kernel_ms=float(np.median(rows)),
               unique_bytes_per_pixel=UNIQUE_BYTES, unique_bytes=unique, copy_unique_ms=copy_ms(torch, unique // 2 // 4 * 4, args.reps),
               copy_double_ms=copy_ms(torch, unique // 4 * 4, args.reps))
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Temporal accumulation (`pt_temporal_accumulate`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part (the register table) stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
