#!/usr/bin/env python3
"""lens_warp_bench.py — what the lens warp costs (pt_lens_warp_planes, k_lens_warp) in its four variants — bilinear or bicubic taps, one
source point per pixel or one per colour channel — beside geometric edge antialiasing (pt_edge_aa_planes, k_edge_aa) on the same frame.

One MI355X, the textured scene.  Steps, each a process of its own under `timeout`; the first step that fails ends the tool with its status
(nothing is tried twice):
  frame-1080p   1920 x 1080, one rectangle
  frame-stereo  1920 x 1080 as two views of 960 x 1080, each with its own lens centre and matrix
In each: one G-buffer (hit, position), the pixel-centre albedo as the colour; a barrel lens (k1 0.1, k2 0.05; with chroma the red and blue
rows scaled by 0.985 and 1.015) under a late yaw of 1.5 degrees; `out` and the packed frame both written.  The identity (lenses=None)
stands beside them: the same kernel where every tap of a pixel is the pixel's own line.
Kernel times are the calls' own kernel_ms (hipEvents around the launch), medians over --reps calls after --warmup, the calls taking turns;
next to them the host time around the whole Python call, and kernel_ms against the algorithmic bytes: 16 B read and 16 B + 4 B written per
pixel.  No threshold is attached to any figure.  Prints one JSON object; --md PATH also writes the tables as markdown with the raw JSON below
them, replacing that file's part from "## Timings" on.
  python3 tools/lens_warp_bench.py [--reps 50] [--warmup 10] [--md profiles/lens_warp.md]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
BYTES_PER_PIXEL = 16 + 16 + 4
CAMERA = dict(eye=(3.0, 2.5, -4.5), lookat=(0.0, 0.6, 0.5), up=(0.0, 1.0, 0.0), fovY=45.0)
K, CHROMA, LATE_YAW = (0.1, 0.05, 0.0), 0.015, 1.5
STEPS = [("frame-1080p", 300), ("frame-stereo", 300)]  # (step, seconds allowed)


def _late(cam, yaw_deg):
    """the camera turned by yaw_deg about its up vector, around its own eye"""
    from optixpathtracer_amd import renderer as R

    eye, lookat, up = (np.array(v, np.float64) for v in (cam.eye, cam.lookat, cam.up))
    axis, t, d = up / np.linalg.norm(up), np.radians(yaw_deg), lookat - eye
    d = d * np.cos(t) + np.cross(axis, d) * np.sin(t) + axis * np.dot(axis, d) * (1.0 - np.cos(t))
    return R.Camera(cam.eye, tuple(eye + d), cam.up, cam.fovY, cam.aspectRatio)


def step_frame(args, shape):
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    model = scenes.textured_scene()
    r = R.SampleRenderer(model)
    r.resize((W, H))
    if shape == "stereo":
        ew = W // 2
        right = np.cross(np.subtract(CAMERA["lookat"], CAMERA["eye"]), CAMERA["up"])
        right = right / np.linalg.norm(right) * 0.0325
        cams = [R.Camera(tuple(np.add(CAMERA["eye"], s * right)), tuple(np.add(CAMERA["lookat"], s * right)), CAMERA["up"], CAMERA["fovY"], ew / H) for s in (-1.0, 1.0)]
        rects = [(0, 0, ew, H), (ew, 0, ew, H)]
        r.setViews([(x, y, w, h, c) for (x, y, w, h), c in zip(rects, cams)])
    else:
        cams, rects = [R.make_camera(CAMERA, W / H)], [(0, 0, W, H)]
        r.setCamera(cams[0])
    g = r.renderGBuffer(("hit", "position"))
    hit, position = g["hit"], g["position"]
    color = r.surfacePlanes(hit, r.copyTexcoordsDevice(), planes=("albedo",))["albedo"]
    out, frame = torch.zeros((H, W, 4), device="cuda:0"), torch.zeros((H, W), dtype=torch.int32, device="cuda:0")

    def lenses(chroma):
        k = [tuple(c * s for c in K) for s in (1.0 - CHROMA, 1.0, 1.0 + CHROMA)] if chroma else K
        return [R.make_lens((w, h), k=k, warp=R.warpMatrix(c, _late(c, LATE_YAW), (w, h))) for (_, _, w, h), c in zip(rects, cams)]

    mono, chroma = lenses(False), lenses(True)
    warp = lambda **kw: r.lensWarpPlanes(color, out=out, frame=frame, **kw)["stats"]  # noqa: E731
    calls = [("edge_aa+frame", lambda: r.edgeAaPlanes(color, hit, position, out=out, frame=frame)["stats"]),
             ("identity bilinear", lambda: warp()),
             ("bilinear", lambda: warp(lenses=mono)),
             ("bilinear chroma", lambda: warp(lenses=chroma)),
             ("bicubic", lambda: warp(lenses=mono, bicubic=True)),
             ("bicubic chroma", lambda: warp(lenses=chroma, bicubic=True))]
    ms, host, stats = {k: [] for k, _ in calls}, {k: [] for k, _ in calls}, {}
    for k in range(args.warmup + args.reps):  # the kernels take turns
        for name, call in calls:
            t0 = time.perf_counter()
            st = call()
            dt = time.perf_counter() - t0
            stats[name] = st
            if k >= args.warmup:
                ms[name].append(st["kernel_ms"])
                host[name].append(dt * 1e3)
    r.close()
    rows = {}
    for name, _ in calls:
        st = stats[name]
        med = float(np.median(ms[name]))
        rows[name] = dict(kernel_ms=med, kernel_min_ms=float(min(ms[name])), host_ms=float(np.median(host[name])), pixels=st["pixels"], outside=st.get("outside", 0),
                          gb_per_s=BYTES_PER_PIXEL * st["pixels"] / (med * 1e-3) / 1e9)
    return dict(views=len(rects), rows=rows)


def markdown(res):
    md = ["## Timings (`tools/lens_warp_bench.py`)\n",
          f"{W} x {H}, one MI355X, the textured scene; kernel times are the calls' own `kernel_ms`, medians (minima in brackets) over {res['reps']} calls "
          f"after {res['warmup']} warm-up calls, the calls taking turns on the same planes in one process.  Every call writes `out` and the packed "
          f"frame; GB/s is {BYTES_PER_PIXEL} algorithmic bytes a pixel (16 read, 16 + 4 written) over `kernel_ms`.  `outside` is the share of pixels with "
          "a channel outside its rectangle (they skip that channel's taps).  No threshold is attached to any of these figures.\n"]
    for step, _ in STEPS:
        k = res[step]
        md += [f"`{step}` ({k['views']} rectangle{'s' if k['views'] > 1 else ''}):\n", "| call | `kernel_ms` | GB/s (algorithmic) | host ms around the call | outside |",
               "|---|---|---|---|---|"]
        for name, row in k["rows"].items():
            md.append(f"| `{name}` | {row['kernel_ms']:.4f} ({row['kernel_min_ms']:.4f}) | {row['gb_per_s']:.0f} | {row['host_ms']:.4f} | {row['outside'] / max(1, row['pixels']):.4f} |")
        md.append("")
    md += ["## Raw output\n", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--md", help="also write the tables as markdown to this path")
    ap.add_argument("--step", help="run one step in this process and print its JSON line")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("lens_warp_bench: no GPU")
        print("RESULT " + json.dumps(step_frame(args, args.step.split("-", 1)[1])), flush=True)
        return 0
    res = dict(reps=args.reps, warmup=args.warmup)
    passed = ["--reps", str(args.reps), "--warmup", str(args.warmup)]
    for step, seconds in STEPS:  # one attempt each; the first failure ends the tool
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step] + passed, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"lens_warp_bench: step {step} ended with status {p.returncode}", file=sys.stderr)
            return p.returncode
        res[step] = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Lens warp and late reprojection (`pt_lens_warp_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
