#!/usr/bin/env python3
"""gbuffer_bench.py — what the first-hit G-buffer pass costs (pt_render_gbuffer) against the composition it replaces.

Scene: the C3 terrain (1 M triangles), 1920 x 1080, the terrain camera.  In ONE run, medians over --reps calls after two warm-up calls:
  (a) kernel_ms of renderGBuffer(("hit",)) and of all five planes (previous camera: the current one moved by 0.25 in x), and of each other
      plane alone — pt_gbuffer_stats.kernel_ms, hipEvents around the pass
  (b) the composition that needs no new entry point: traceDevice over the 2 073 600 pixel-centre rays kept in a tensor (the `ray` plane
      itself, image order), timed as stage_ms + trace_ms + attrib_ms of pt_query_stats — and with the rays in the pixel list's 8x8-block
      order, the order the fused pass traverses in
The yardstick of (a) "hit" is (b): both come from this run, neither depends on the other's code path.  Printed as ONE JSON object;
--md PATH also writes the table as markdown with the raw JSON below it.
  timeout -k 10 300 python3 tools/gbuffer_bench.py [--reps 7] [--md profiles/gbuffer.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
PLANES = ("hit", "depth", "position", "motion", "ray")


def median_kernel_ms(r, planes, prev, out, reps):
    rows = []
    for k in range(reps + 2):
        s = r.renderGBuffer(planes, prev_cameras=prev, out={p: out[p] for p in planes})["stats"]
        if k >= 2:
            rows.append(s["kernel_ms"])
    return float(np.median(rows)), s


def median_query_ms(r, rays, out, reps):
    rows = []
    for k in range(reps + 2):
        r.traceDevice(rays, out=out)
        if k >= 2:
            s = r.queryStats
            rows.append((s["stage_ms"], s["trace_ms"], s["attrib_ms"]))
    st, tr, at = (float(x) for x in np.median(np.array(rows), axis=0))
    return dict(stage_ms=st, trace_ms=tr, attrib_ms=at, total_ms=float(np.median(np.array(rows).sum(axis=1))), hits=int(r.queryStats["hits"]))


def block_order(torch, dev):
    """indices of the frame's pixels in the order of the pixel list: 8x8 blocks row by row, rows of a block top to bottom"""
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    key = (((y // 8) * ((W + 7) // 8) + x // 8) * 8 + y % 8) * 8 + x % 8
    return torch.argsort(key.reshape(-1))


def markdown(res):
    a, b, bb = res["gbuffer"], res["composition"], res["composition_block_order"]
    md = ["# First-hit G-buffer (`tools/gbuffer_bench.py`)\n",
          f"C3 terrain, {res['triangles']} triangles, {W} x {H} = {res['pixels']} pixels, {res['hits']} hits, one MI355X; medians of {res['reps']} after 2 warm-ups.  Device times by hipEvents.\n",
          "| what | ms |", "|---|---|"]
    for name in ("hit", "all five planes", "depth", "position", "motion", "ray"):
        md.append(f"| (a) `renderGBuffer`, {name}: `kernel_ms` | {a[name]:.4f} |")
    md.append(f"| (b) `traceDevice` over the pixel-centre rays, image order: stage + trace + attrib | {b['stage_ms']:.4f} + {b['trace_ms']:.4f} + {b['attrib_ms']:.4f} = {b['total_ms']:.4f} |")
    md.append(f"| (b') the same rays in 8x8-block order | {bb['stage_ms']:.4f} + {bb['trace_ms']:.4f} + {bb['attrib_ms']:.4f} = {bb['total_ms']:.4f} |")
    md.append(f"| (a) hit / (b) | {a['hit'] / b['total_ms']:.3f} |")
    md += ["", "## Raw output\n", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--md", help="also write the table as markdown to this path")
    args = ap.parse_args()
    import torch

    from optixpathtracer_amd import _lib
    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    dev = "cuda:0"
    model = scenes.voxel_terrain()
    r = R.SampleRenderer(model)
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.TERRAIN_CAMERA, W / H))
    ex, ey, ez = scenes.TERRAIN_CAMERA["eye"]
    prev = [R.make_camera(dict(scenes.TERRAIN_CAMERA, eye=(ex + 0.25, ey, ez)), W / H)]
    out = {p: torch.zeros((H, W) if p == "depth" else (H, W, _lib.GBUFFER_PLANES[p]), dtype=torch.float32, device=dev) for p in PLANES}
    res = dict(triangles=model.num_triangles, pixels=W * H, reps=args.reps, gbuffer={})
    res["gbuffer"]["hit"], s = median_kernel_ms(r, ("hit",), None, out, args.reps)
    res["hits"] = int(s["hits"])
    res["gbuffer"]["all five planes"], _ = median_kernel_ms(r, PLANES, prev, out, args.reps)
    for p in ("depth", "position", "motion", "ray"):
        res["gbuffer"][p], _ = median_kernel_ms(r, (p,), prev if p == "motion" else None, out, args.reps)
    rays = out["ray"].reshape(-1, 8).clone()
    rec = torch.empty((W * H, 8), dtype=torch.float32, device=dev)
    res["composition"] = median_query_ms(r, rays, rec, args.reps)
    same = bool(torch.equal(rec.view(torch.int32), out["hit"].reshape(-1, 8).view(torch.int32)))
    res["hit_plane_equals_composition"] = same
    res["composition_block_order"] = median_query_ms(r, rays[block_order(torch, dev)].contiguous(), rec, args.reps)
    r.close()
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(markdown(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
