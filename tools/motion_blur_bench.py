#!/usr/bin/env python3
"""motion_blur_bench.py — what motion blur costs (pt_motion_blur_planes: k_mblur_tile, k_mblur_neighbour, k_mblur_gather) beside the chain's
cheapest full-frame pass (pt_modulate_planes without an albedo: one plane in, one plane out) on the same tensor.

1920 x 1080, one MI355X.  Steps, each a process of its own under `timeout`; the first step that fails ends the tool with its status (nothing
is tried twice):
  kernels-static      zero motion: every tile leaves early.  Bytes per pixel: 8 (motion, the tile pass) + 16 (colour) + 16 (out) against
                      k_modulate's 32, plus the two small launches.
  kernels-uniform     one colour plane under a uniform motion of 16 pixels of velocity, at 8, 12 and 24 taps.
  kernels-two_box, kernels-c3_terrain
                      the scene's accumulation buffer after two subframes under the sky probe, depth and motion from renderGBuffer after
                      the camera has orbited by --angle radians; 8, 12 and 24 taps.
  modulate-parent     with --parent DIR (a checkout of the parent commit, built): pt_modulate_planes of THAT library on the same shape, in a
                      process of its own — the yardstick as the parent built it, beside the rows above that take turns with this library's.
  trace-static        motion blur alone on the static frame, --reps calls: what a kernel trace is taken of (rocprofv3 --kernel-trace --stats
                      -- python3 tools/motion_blur_bench.py --step trace-static).
Kernel times are the calls' own kernel_ms (hipEvents around the launches; the upload of the view table in front of them excluded), medians
over --reps calls after --warmup, the calls taking turns on the same planes; next to them the host time around the whole Python call.
`gathered GB/s` is moving pixels x taps x 28 bytes (colour 16, motion 8, depth 4) over the call's kernel time; `modulate GB/s` is 32 bytes a
pixel over k_modulate's.  No threshold is attached to any figure.  Prints one JSON object; --md PATH also writes the tables as markdown with
the raw JSON below them, replacing that file's part from "## Timings" on.
  python3 tools/motion_blur_bench.py [--reps 50] [--warmup 10] [--angle 0.02] [--parent DIR] [--md profiles/motion_blur.md]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H = 1920, 1080
TAPS = (8, 12, 24)
CONTENTS = ("static", "uniform", "two_box", "c3_terrain")
STEPS = [(f"kernels-{n}", 300) for n in CONTENTS]  # (step, seconds allowed)


def _orbit(cam, angle):
    e, l = np.asarray(cam["eye"], np.float64), np.asarray(cam["lookat"], np.float64)
    d = e - l
    c, s = np.cos(angle), np.sin(angle)
    return dict(cam, eye=(float(l[0] + c * d[0] + s * d[2]), float(e[1]), float(l[2] - s * d[0] + c * d[2])))


def _setup(content, angle):
    """(renderer, colour, motion, depth) on the device"""
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    real = {"two_box": (lambda: scenes.two_box_scene(shadow_catcher=False), scenes.TWO_BOX_CAMERA), "c3_terrain": (scenes.voxel_terrain, scenes.TERRAIN_CAMERA)}
    make, cam0 = real.get(content, (scenes.cornell_box, scenes.CORNELL_CAMERA))
    model = make()
    r = R.SampleRenderer(model)
    if content in real:
        r.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    r.resize((W, H))
    r.setCamera(R.make_camera(cam0, W / H))
    if content not in real:
        color = torch.tensor([3.0, 2.0, 1.0, 1.0], device="cuda:0").repeat(H, W, 1).contiguous()
        motion = torch.zeros((H, W, 2), device="cuda:0")
        if content == "uniform":
            motion[..., 0] = 64.0  # times hs = 0.25: 16 pixels of velocity
        depth = torch.full((H, W), 3.0, device="cuda:0")
        return r, model, color, motion, depth
    r.launchParams.samples_per_launch = 1
    for n in (0, 1):
        r.launchParams.frame.subframe_index = n
        r.render()
    r.sync()
    color = torch.from_numpy(r.download(R.PT_BUF_ACCUM).astype(np.float32).reshape(H, W, 4)).to("cuda:0")
    g = r.renderGBuffer(("depth", "motion"), prev_cameras=R.make_camera(_orbit(cam0, angle), W / H))
    return r, model, color, g["motion"], g["depth"]


def _timed(args, calls):
    ms, host, stats = {k: [] for k, _ in calls}, {k: [] for k, _ in calls}, {}
    for k in range(args.warmup + args.reps):  # the calls take turns
        for name, call in calls:
            t0 = time.perf_counter()
            st = call()
            dt = time.perf_counter() - t0
            stats[name] = st
            if k >= args.warmup:
                ms[name].append(st["kernel_ms"])
                host[name].append(dt * 1e3)
    return {name: dict(kernel_ms=float(np.median(ms[name])), kernel_min_ms=float(min(ms[name])), host_ms=float(np.median(host[name])),
                       **{k: v for k, v in stats[name].items() if k != "kernel_ms"}) for name, _ in calls}


def step_kernels(args, content):
    import torch

    r, model, color, motion, depth = _setup(content, args.angle)
    out = torch.zeros((H, W, 4), device="cuda:0")
    dims, nbytes = r.motionBlurLayout()
    scratch = torch.zeros((nbytes // 8, 2), device="cuda:0")
    calls = [("modulate", lambda: r.modulatePlanes(color, out=out)["stats"])]
    for taps in (12,) if content == "static" else TAPS:
        calls.append((f"motion blur, {taps} taps", lambda taps=taps: r.motionBlurPlanes(color, motion, depth, out=out, scratch=scratch, taps=taps)["stats"]))
    rows = _timed(args, calls)
    r.close()
    return dict(triangles=model.num_triangles, tiles=[int(dims[0, 0]), int(dims[0, 1])], scratch_bytes=nbytes, rows=rows)


def step_modulate(args, content):
    """pt_modulate_planes of whatever library sys.path leads to (the parent's, under --parent)"""
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    r = R.SampleRenderer(scenes.cornell_box())
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.CORNELL_CAMERA, W / H))
    color = torch.tensor([3.0, 2.0, 1.0, 1.0], device="cuda:0").repeat(H, W, 1).contiguous()
    out = torch.zeros((H, W, 4), device="cuda:0")
    rows = _timed(args, [("modulate", lambda: r.modulatePlanes(color, out=out)["stats"])])
    r.close()
    return dict(library=os.path.dirname(os.path.abspath(R.__file__)), rows=rows)


def step_trace(args, content):
    import torch

    r, _, color, motion, depth = _setup(content, args.angle)
    out = torch.zeros((H, W, 4), device="cuda:0")
    scratch = torch.zeros((r.motionBlurLayout()[1] // 8, 2), device="cuda:0")
    ms = [r.motionBlurPlanes(color, motion, depth, out=out, scratch=scratch)["stats"]["kernel_ms"] for _ in range(args.warmup + args.reps)]
    r.close()
    return dict(kernel_ms=float(np.median(ms[args.warmup:])), calls=len(ms))


def markdown(res):
    md = ["## Timings (`tools/motion_blur_bench.py`)\n",
          f"{W} x {H}, one MI355X; kernel times are the calls' own `kernel_ms`, medians (minima in brackets) over {res['reps']} calls after "
          f"{res['warmup']} warm-up calls, the calls taking turns on the same planes in one process.  `modulate` is `pt_modulate_planes` without an "
          "albedo (32 bytes a pixel).  `x modulate` is the row's `kernel_ms` over `modulate`'s of the same table; `moving` the share of the pixels "
          "that gather; `gathered GB/s` is moving x taps x 28 bytes over `kernel_ms`, `GB/s` beside `modulate` its 32 bytes a pixel over its own.  "
          "No threshold is attached to any of these figures.\n"]
    for content in CONTENTS:
        k = res[f"kernels-{content}"]
        base = k["rows"]["modulate"]["kernel_ms"]
        md += [f"`{content}`: {k['tiles'][0]} x {k['tiles'][1]} tiles, scratch {k['scratch_bytes']} bytes.\n",
               "| call | `kernel_ms` | x modulate | moving | GB/s | host ms around the call | counters |", "|---|---|---|---|---|---|---|"]
        for name, row in k["rows"].items():
            if name == "modulate":
                rate, moving = 32.0 * W * H / (row["kernel_ms"] * 1e-3) / 1e9, ""
            else:
                taps = int(name.split(",")[1].split()[0])
                rate, moving = row["moving"] * taps * 28.0 / (row["kernel_ms"] * 1e-3) / 1e9, f"{100.0 * row['moving'] / max(1, row['pixels']):.1f} %"
            cnt = ", ".join(f"{c} {row[c]}" for c in ("pixels", "sources", "unknown", "moving", "taps", "nonfinite") if c in row)
            md.append(f"| `{name}` | {row['kernel_ms']:.4f} ({row['kernel_min_ms']:.4f}) | {row['kernel_ms'] / base:.2f} | {moving} | {rate:.0f} | {row['host_ms']:.4f} | {cnt} |")
        md.append("")
    if "modulate-parent" in res:
        row = res["modulate-parent"]["rows"]["modulate"]
        md += [f"`pt_modulate_planes` as the parent commit built it, in a process of its own: {row['kernel_ms']:.4f} ({row['kernel_min_ms']:.4f}) ms.\n"]
    md += ["## Raw output\n", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--angle", type=float, default=0.02, help="the camera's orbit between the previous and this frame, radians")
    ap.add_argument("--parent", help="a built checkout of the parent commit: its pt_modulate_planes is timed in a process of its own")
    ap.add_argument("--md", help="also write the tables as markdown to this path")
    ap.add_argument("--step", help="run one step in this process and print its JSON line")
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, os.path.abspath(args.tree))
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("motion_blur_bench: no GPU")
        kind, content = args.step.split("-", 1)
        print("RESULT " + json.dumps(dict(trace=step_trace, modulate=step_modulate).get(kind, step_kernels)(args, content)), flush=True)
        return 0
    res = dict(reps=args.reps, warmup=args.warmup, angle=args.angle)
    passed = ["--reps", str(args.reps), "--warmup", str(args.warmup), "--angle", str(args.angle)]
    steps = [(s, t, ROOT) for s, t in STEPS] + ([("modulate-parent", 120, args.parent)] if args.parent else [])
    for step, seconds, tree in steps:  # one attempt each; the first failure ends the tool
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step, "--tree", tree] + passed,
                           stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"motion_blur_bench: step {step} ended with status {p.returncode}", file=sys.stderr)
            return p.returncode
        res[step] = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Motion blur (`pt_motion_blur_layout`, `pt_motion_blur_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
