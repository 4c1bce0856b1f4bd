#!/usr/bin/env python3
"""plan_bench.py — what adaptive sampling inside the SVGF loop saves and what its two passes cost (pt_sample_plan, pt_temporal_carry).

Scene: the C3 terrain (1 M triangles), 1920 x 1080, 1 sample per pixel, the terrain camera on an orbit of --frames frames (0.01 rad per
frame about the look-at point).  In ONE process, on one GPU, the two loops take turns --rounds times:
  (a) the existing full loop without albedo: renderGBuffer, render(), temporalMoments (no mask), filterPlanes;
  (b) the adaptive loop of examples/adaptive_svgf_loop.py: renderGBuffer, samplePlan, renderMask, temporalMoments on the mask,
      temporalCarry on its complement, filterPlanes on all pixels.
Per stage: the median over the frames after --warmup of the host time around the (synchronous) call, and of the call's own device time
(kernel_ms, render_ms) where it reports one.  For (b) also the share of blocks sampled per frame and the split of the plan's reasons.  The
yardstick is (a) and temporalMoments's time in the same run on the same box — never the code under test; no threshold is attached to any
figure.  Printed as ONE JSON object; --md PATH also writes the tables as markdown with the raw JSON below them, replacing that file's part
from "## Timings" on.
  timeout -k 10 600 python3 tools/plan_bench.py [--frames 32] [--warmup 8] [--rounds 2] [--md profiles/plan.md]
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
FULL_STAGES = ("gbuffer", "render", "temporal", "filter", "frame")
ADAPT_STAGES = ("gbuffer", "plan", "render", "temporal", "carry", "filter", "frame")


def orbit(cam, angle):
    e, l = np.asarray(cam["eye"], np.float64), np.asarray(cam["lookat"], np.float64)
    d = e - l
    c, s = np.cos(angle), np.sin(angle)
    return dict(cam, eye=(float(l[0] + c * d[0] + s * d[2]), float(e[1]), float(l[2] - s * d[0] + c * d[2])))


def markdown(res):
    a, b = res["full"], res["adaptive"]
    md = ["## Timings (`tools/plan_bench.py`)\n",
          f"C3 terrain, {res['triangles']} triangles, {W} x {H}, 1 spp, an orbit of {res['frames']} frames, one MI355X, one process, the two loops "
          f"taking turns {res['rounds']} times; medians over the frames after {res['warmup']} warm-up frames of every round.  Host: the host clock "
          "around the synchronous call.  Device: the call's own `kernel_ms` (`render_ms` for the render).  Plan parameters: "
          f"`{json.dumps(res['plan_params'])}`.  No threshold is attached to any of these figures.\n",
          "| stage | (a) full loop: host ms | device ms | (b) adaptive loop: host ms | device ms |", "|---|---|---|---|---|"]

    def cell(d, st):
        return f"{d[st]:.3f}" if st in d else "–"

    for st in ADAPT_STAGES:
        md.append(f"| {st} | {cell(a['host_ms'], st)} | {cell(a['device_ms'], st)} | {cell(b['host_ms'], st)} | {cell(b['device_ms'], st)} |")
    md += ["",
           f"Share of blocks sampled per frame in (b), after warm-up: median {b['sampled_share']['median']:.3f}, min {b['sampled_share']['min']:.3f}, "
           f"max {b['sampled_share']['max']:.3f}; by reason (medians of blocks per frame): lost {b['by_lost']:.0f}, short or noisy {b['by_need']:.0f}, "
           f"refresh only {b['by_refresh']:.0f} of {b['blocks']} blocks.  The carry lost {b['carry_lost']} pixels over all frames.",
           f"`kernel_ms` of the plan: {b['device_ms']['plan']:.4f}; of the carry: {b['device_ms']['carry']:.4f}; of `temporalMoments` on the whole "
           f"frame in (a), the yardstick: {a['device_ms']['temporal']:.4f}.",
           "", "## Raw output\n", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.25)
    ap.add_argument("--dark-floor", type=float, default=0.05)
    ap.add_argument("--min-length", type=int, default=4)
    ap.add_argument("--min-pixels", type=int, default=8)
    ap.add_argument("--refresh", type=int, default=16)
    ap.add_argument("--md", help="also write the tables as markdown to this path")
    args = ap.parse_args()
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    if not torch.cuda.is_available():
        raise SystemExit("plan_bench: no GPU")
    dev = "cuda:0"
    model = scenes.voxel_terrain()
    r = R.SampleRenderer(model)
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.resize((W, H))
    r.launchParams.samples_per_launch = 1
    plan_params = dict(threshold=args.threshold, dark_floor=args.dark_floor, min_length=args.min_length, min_pixels=args.min_pixels,
                       refresh_period=args.refresh)

    def planes(k):
        return torch.zeros((H, W, k) if k > 1 else (H, W), device=dev)

    gbuf = [dict(hit=planes(8), position=planes(4), motion=planes(2)) for _ in range(2)]
    history, moments, length = [planes(4) for _ in range(2)], [planes(2) for _ in range(2)], [planes(1) for _ in range(2)]
    variance, filtered, scratch = planes(1), planes(4), planes(4)
    accum = r.deviceBuffer(R.PT_BUF_ACCUM)

    def timed(rows, name, fn):
        t0 = time.perf_counter()
        out = fn()
        rows.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        return out

    def loop(adaptive):
        """one orbit from a cold history; returns per-frame rows {host: {stage: ms}, device: {stage: ms}, plan: stats, carry_lost}"""
        r.uploadAccum(np.zeros((H, W, 4), np.float32))
        for t in gbuf[0].values():
            t.zero_()
        for t in gbuf[1].values():
            t.zero_()
        for t in history + moments + length:
            t.zero_()
        rows = []
        cam = R.make_camera(scenes.TERRAIN_CAMERA, W / H)
        for k in range(args.frames):
            prev, cam = cam, R.make_camera(orbit(scenes.TERRAIN_CAMERA, 0.01 * k), W / H)
            cur, old, i, o = gbuf[k & 1], gbuf[~k & 1], k & 1, ~k & 1
            host, device, row = {}, {}, {}
            t_frame = time.perf_counter()
            r.setCamera(cam)
            g = timed(host, "gbuffer", lambda: r.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev, out=cur))
            device["gbuffer"] = g["stats"]["kernel_ms"]
            geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], history[i], moments[i], length[i])
            outs = dict(history_out=history[o], moments_out=moments[o], length_out=length[o], variance_out=variance)
            r.launchParams.frame.subframe_index = k
            if adaptive:
                p = timed(host, "plan", lambda: r.samplePlan(*geo, frame_index=k, **plan_params))
                mask = p["mask"]
                device["plan"] = p["stats"]["kernel_ms"]
                row["plan"] = {n: v for n, v in p["stats"].items() if n != "kernel_ms"}
                timed(host, "render", lambda: r.renderMask(mask))
                device["render"] = r.stats()["render_ms"]
                t = timed(host, "temporal", lambda: r.temporalMoments(accum, *geo, **outs, mask=mask, color_scale=float(k + 1), clear_color=True))
                c = timed(host, "carry", lambda: r.temporalCarry(*geo, **outs, mask=mask == 0))
                device["carry"] = c["stats"]["kernel_ms"]
                row["carry_lost"] = c["stats"]["lost"]
            else:
                timed(host, "render", lambda: (r.render(), r.sync()))
                device["render"] = r.stats()["render_ms"]
                t = timed(host, "temporal", lambda: r.temporalMoments(accum, *geo, **outs, color_scale=float(k + 1), clear_color=True))
            device["temporal"] = t["stats"]["kernel_ms"]
            f = timed(host, "filter", lambda: r.filterPlanes(history[o], cur["hit"], cur["position"], variance=variance, length=length[o], out=filtered,
                                                             scratch=scratch))
            device["filter"] = f["stats"]["kernel_ms"]
            host = {n: v[0] for n, v in host.items()}
            host["frame"] = (time.perf_counter() - t_frame) * 1e3
            rows.append(dict(row, host=host, device=device))
        return rows

    runs = {False: [], True: []}
    for _ in range(args.rounds):
        for adaptive in (False, True):
            runs[adaptive] += loop(adaptive)[args.warmup:]
    r.close()

    def summary(rows, stages):
        out = dict(host_ms={s: float(np.median([row["host"][s] for row in rows])) for s in stages},
                   device_ms={s: float(np.median([row["device"][s] for row in rows])) for s in stages if s in rows[0]["device"]})
        return out

    full, adapt = summary(runs[False], FULL_STAGES), summary(runs[True], ADAPT_STAGES)
    share = [row["plan"]["sampled"] / row["plan"]["blocks"] for row in runs[True]]
    adapt.update(sampled_share=dict(median=float(np.median(share)), min=float(min(share)), max=float(max(share))),
                 blocks=int(runs[True][0]["plan"]["blocks"]), carry_lost=int(sum(row["carry_lost"] for row in runs[True])),
                 **{n: float(np.median([row["plan"][n] for row in runs[True]])) for n in ("by_lost", "by_need", "by_refresh", "lost", "needy")},
                 per_frame_share=[round(s, 4) for s in share[:args.frames - args.warmup]])
    res = dict(triangles=model.num_triangles, pixels=W * H, frames=args.frames, warmup=args.warmup, rounds=args.rounds, plan_params=plan_params,
               full=full, adaptive=adapt)
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Adaptive sampling in the SVGF loop (`pt_sample_plan`, `pt_temporal_carry`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part (the register table) stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
