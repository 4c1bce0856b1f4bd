#!/usr/bin/env python3
"""filter_bench.py — what the chain's filter costs (pt_filter_planes) against pt_denoise on the same frame and against the memory traffic
it cannot avoid.

Scene: the C3 terrain (1 M triangles), 1920 x 1080, the terrain camera.  hit and position come from renderGBuffer, the colour is one
rendered frame (the context's PT_BUF_COLOR, so both filters read the same image), the variance is random around 1e-2, the lengths are
random 0..9 (about four in ten below min_length = 4, so the prepare stage runs both of its paths).  In ONE run, medians over --reps calls
after two warm-up calls:
  (a) kernel_ms of filterPlanes with 0, 1, .. 5 passes — pt_filter_stats.kernel_ms, hipEvents around all stages of a call.  The call with
      0 passes is the prepare stage; pass i is the difference between the calls with i + 1 and with i passes (one event pair per call: the
      split is by differences of medians, not by events inside a call)
  (b) the yardstick: pt_denoise with 5 (and with 1) iterations on the same frame — k_atrous, existing code, the same 25 taps of 48 bytes
  (c) the floor: a plain device-to-device copy that moves one pass's UNIQUE bytes — each plane read once (record 16, second half of the hit
      record 16, position 16) and the record written once (16)
Algorithmic bytes per pixel, written beside the times: the new filter's pass gathers 25 x 48 B + 9 x 4 B and writes 16 B; k_atrous's pass
gathers 25 x 48 B and writes 16 B.  There is no pass/fail ratio: nobody had measured the pass when this tool was written.  Printed as ONE
JSON object; --md PATH also writes the table as markdown with the raw JSON below it, replacing that file's part from "## Timings" on.
  timeout -k 10 300 python3 tools/filter_bench.py [--reps 7] [--md profiles/filter.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
PASSES = 5
FILTER_PASS_BYTES = 25 * 48 + 9 * 4 + 16
ATROUS_PASS_BYTES = 25 * 48 + 16
UNIQUE_PASS_BYTES = 16 + 16 + 16 + 16


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
    gbs = lambda nbytes, ms: f"{nbytes * px / ms / 1e6:.0f}"
    md = ["## Timings (`tools/filter_bench.py`)\n",
          f"C3 terrain, {res['triangles']} triangles, {W} x {H} = {px} pixels, {res['filtered']} of them filtered, {res['spatial']} with the spatial variance "
          f"estimate, one MI355X; medians of {res['reps']} after 2 warm-ups, one run.  Device times by hipEvents.  No pass/fail ratio is attached to these figures.\n",
          "| what | ms | algorithmic B/pixel | GB/s of those |", "|---|---|---|---|",
          f"| (a) `filterPlanes`, {PASSES} passes: `kernel_ms` | {res['filter_ms'][PASSES]:.4f} | | |",
          f"| (a) prepare stage (0 passes) | {res['filter_ms'][0]:.4f} | | |"]
    for i, ms in enumerate(res["pass_ms"]):
        md.append(f"| (a) pass {i}, spacing {1 << i} (difference of medians) | {ms:.4f} | {FILTER_PASS_BYTES} | {gbs(FILTER_PASS_BYTES, ms)} |")
    per = res["denoise_ms"][str(PASSES)] / PASSES
    md += [f"| (b) `pt_denoise`, {PASSES} iterations | {res['denoise_ms'][str(PASSES)]:.4f} | | |",
           f"| (b) per `k_atrous` pass (a fifth of that) | {per:.4f} | {ATROUS_PASS_BYTES} | {gbs(ATROUS_PASS_BYTES, per)} |",
           f"| (b) `pt_denoise`, 1 iteration | {res['denoise_ms']['1']:.4f} | {ATROUS_PASS_BYTES} | {gbs(ATROUS_PASS_BYTES, res['denoise_ms']['1'])} |",
           f"| (c) device-to-device copy of one pass's unique bytes ({UNIQUE_PASS_BYTES} B/pixel read + written) | {res['copy_unique_ms']:.4f} | {UNIQUE_PASS_BYTES} | {gbs(UNIQUE_PASS_BYTES, res['copy_unique_ms'])} |",
           f"| mean pass of (a) / pass of (b); the byte counts' ratio is {FILTER_PASS_BYTES / ATROUS_PASS_BYTES:.3f} | {float(np.mean(res['pass_ms'])) / per:.3f} | | |",
           f"| mean pass of (a) / (c) | {float(np.mean(res['pass_ms'])) / res['copy_unique_ms']:.2f} | | |",
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
    r.setCamera(R.make_camera(scenes.TERRAIN_CAMERA, W / H))
    g = r.renderGBuffer(("hit", "position"))
    r.launchParams.samples_per_launch = 1
    r.launchParams.frame.subframe_index = 0
    r.render()
    gen = torch.Generator(device=dev).manual_seed(1)
    variance = torch.rand((H, W), device=dev, generator=gen) * 0.02
    length = torch.randint(0, 10, (H, W), device=dev, generator=gen).float()
    out, scratch = torch.zeros((H, W, 4), device=dev), torch.zeros((H, W, 4), device=dev)
    colour = r.deviceBuffer(R.PT_BUF_COLOR)
    filter_ms = []
    for its in range(PASSES + 1):
        rows = []
        for k in range(args.reps + 2):
            s = r.filterPlanes(colour, g["hit"], g["position"], variance=variance, length=length, out=out, scratch=scratch, iterations=its)["stats"]
            if k >= 2:
                rows.append(s["kernel_ms"])
        filter_ms.append(float(np.median(rows)))
    denoise_ms = {}
    for its in (1, PASSES):
        rows = []
        for k in range(args.reps + 2):
            _, ms = r.denoise(iterations=its)
            if k >= 2:
                rows.append(ms)
        denoise_ms[str(its)] = float(np.median(rows))
    r.close()
    res = dict(triangles=model.num_triangles, pixels=W * H, reps=args.reps, filtered=int(s["filtered"]), spatial=int(s["spatial"]), filter_ms=filter_ms,
               pass_ms=[filter_ms[i + 1] - filter_ms[i] for i in range(PASSES)], denoise_ms=denoise_ms,
               filter_pass_bytes_per_pixel=FILTER_PASS_BYTES, atrous_pass_bytes_per_pixel=ATROUS_PASS_BYTES, unique_pass_bytes_per_pixel=UNIQUE_PASS_BYTES,
               copy_unique_ms=copy_ms(torch, UNIQUE_PASS_BYTES * W * H // 2, args.reps))
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# The chain's filter (`pt_filter_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part (the register table) stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
