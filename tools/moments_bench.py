#!/usr/bin/env python3
"""moments_bench.py — what the fused SVGF temporal stage costs (pt_temporal_moments) against the three-call recipe it replaces.

Scene: the C3 terrain (1 M triangles), 1920 x 1080, the terrain camera; the previous camera is the current one moved by 0.25 in x.  The
G-buffer planes of both cameras come from renderGBuffer, the colour and the albedo are one rendered frame's (PT_BUF_ACCUM, PT_BUF_ALBEDO),
the history and the moments are random with lengths 1..8.  In ONE run and ONE process, on the same planes, medians over --reps calls
after two warm-up calls:
  (a) kernel_ms of temporalMoments, all four outputs, the clear flag: without albedo and clamp / with the albedo plane / with albedo and clamp
  (b) examples/svgf_loop.py's recipe: three temporalAccumulate calls over the same motion, hit and position planes — the frame's colour
      against an empty history (clear flag), the colour history, the moments plane (lum, lum^2, 0, 1) — as the SUM of their kernel_ms.  The
      torch element-wise kernels between them (luminance, moments plane, variance) are not in the sum.
  (c) kernel_ms of modulatePlanes, albedo, float and RGBA8 outputs
The cost of the albedo plane and of the clamp window are the differences between the three variants of (a).  There is no pass/fail ratio:
nobody had measured the pass when this tool was written.  Printed as ONE JSON object; --md PATH also writes the table as markdown with the
raw JSON below it, replacing that file's part from "## Timings" on.
  timeout -k 10 300 python3 tools/moments_bench.py [--reps 7] [--md profiles/moments.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080


def markdown(res):
    f, rc = res["fused_ms"], res["recipe_ms"]
    md = ["## Timings (`tools/moments_bench.py`)\n",
          f"C3 terrain, {res['triangles']} triangles, {W} x {H} = {res['pixels']} pixels, {res['reprojected']} of them reprojected, {res['clamped']} "
          f"clamped (clamp_k = 1), one MI355X, one process, the same planes; medians of {res['reps']} after 2 warm-ups.  Device times by hipEvents "
          "(`kernel_ms` of the calls' stats).  No pass/fail ratio is attached to these figures.\n",
          "| what | ms |", "|---|---|",
          f"| (a) `temporalMoments`, four outputs, clear flag, no albedo, no clamp | {f['plain']:.4f} |",
          f"| (a) ... with the albedo plane | {f['albedo']:.4f} |",
          f"| (a) ... with albedo and clamp | {f['albedo_clamp']:.4f} |",
          f"| cost of the albedo plane | {f['albedo'] - f['plain']:+.4f} |",
          f"| cost of the clamp window | {f['albedo_clamp'] - f['albedo']:+.4f} |",
          f"| (b) recipe call 1: the frame's colour against an empty history, clear flag | {rc['colour']:.4f} |",
          f"| (b) recipe call 2: the colour history | {rc['history']:.4f} |",
          f"| (b) recipe call 3: the moments plane | {rc['moments']:.4f} |",
          f"| (b) sum of the three | {res['recipe_sum_ms']:.4f} |",
          f"| (a, no albedo, no clamp) / (b) | {f['plain'] / res['recipe_sum_ms']:.3f} |",
          f"| (c) `modulatePlanes`, albedo, float + RGBA8 | {res['modulate_ms']:.4f} |",
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
    albedo = torch.from_numpy(r.download(R.PT_BUF_ALBEDO)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    hist = torch.rand((H, W, 4), device=dev, generator=gen)
    m1 = torch.rand((H, W), device=dev, generator=gen)
    mom = torch.stack([m1, m1 * m1 + 0.01], -1).contiguous()
    mom4 = torch.cat([mom, torch.zeros((H, W, 1), device=dev), torch.ones((H, W, 1), device=dev)], -1).contiguous()
    length = torch.randint(1, 9, (H, W), device=dev, generator=gen).float()
    geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"])

    def planes(k):
        return torch.zeros((H, W, k) if k > 1 else (H, W), device=dev)

    out = dict(history_out=planes(4), moments_out=planes(2), length_out=planes(1), variance_out=planes(1))
    reps = args.reps

    def median(fn):
        rows = [fn() for _ in range(reps + 2)]
        return float(np.median([row[0] for row in rows[2:]])), rows[-1][1]

    def fused(alb, clamp_k):
        def once():
            c = colour.clone()  # the clear flag zeroes it
            s = r.temporalMoments(c, *geo, hist, mom, length, albedo=alb, **out, albedo_min=0.01, clamp_k=clamp_k, clear_color=True)["stats"]
            return s["kernel_ms"], s
        return median(once)

    fused_ms = {}
    fused_ms["plain"], s_plain = fused(None, None)
    fused_ms["albedo"], _ = fused(albedo, None)
    fused_ms["albedo_clamp"], s_clamp = fused(albedo, 1.0)
    # the recipe of examples/svgf_loop.py, call by call
    none4, none1, one = planes(4), planes(1), planes(1)
    frame_colour, hist_out, len_out, mom_out, len_m = planes(4), planes(4), planes(1), planes(4), planes(1)

    def recipe():
        c = colour.clone()
        a = r.temporalAccumulate(c, *geo, none4, none1, history_out=frame_colour, length_out=one, clear_color=True)["stats"]["kernel_ms"]
        b = r.temporalAccumulate(frame_colour, *geo, hist, length, history_out=hist_out, length_out=len_out)["stats"]["kernel_ms"]
        lum = (0.2126 * frame_colour[..., 0] + 0.7152 * frame_colour[..., 1]) + 0.0722 * frame_colour[..., 2]
        mp = torch.stack([lum, lum * lum, torch.zeros_like(lum), torch.ones_like(lum)], -1).contiguous()
        m = r.temporalAccumulate(mp, *geo, mom4, length, history_out=mom_out, length_out=len_m)["stats"]["kernel_ms"]
        return a + b + m, (a, b, m)

    rows = [recipe() for _ in range(reps + 2)][2:]
    recipe_sum = float(np.median([row[0] for row in rows]))
    parts = np.median(np.array([row[1] for row in rows]), 0)
    # the same frame through both routes: the fused pass without albedo and clamp computes what the recipe computes
    r.temporalMoments(colour.clone(), *geo, hist, mom, length, **out, clear_color=True)
    same = bool(torch.equal(out["history_out"], hist_out) and torch.equal(out["length_out"], len_out) and torch.equal(out["moments_out"], mom_out[..., :2]))
    mod_out, mod_frame = planes(4), torch.zeros((H, W), dtype=torch.int32, device=dev)

    def modulate():
        s = r.modulatePlanes(out["history_out"], albedo=albedo, out=mod_out, frame=mod_frame, albedo_min=0.01)["stats"]
        return s["kernel_ms"], s

    modulate_ms, _ = median(modulate)
    r.close()
    res = dict(triangles=model.num_triangles, pixels=W * H, reps=reps, reprojected=int(s_plain["reprojected"]), clamped=int(s_clamp["clamped"]),
               fused_ms=fused_ms, recipe_ms=dict(colour=float(parts[0]), history=float(parts[1]), moments=float(parts[2])), recipe_sum_ms=recipe_sum,
               fused_equals_recipe=same, modulate_ms=modulate_ms)
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# The fused SVGF temporal stage (`pt_temporal_moments`, `pt_modulate_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part (the register table) stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
