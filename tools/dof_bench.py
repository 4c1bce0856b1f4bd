#!/usr/bin/env python3
"""dof_bench.py — what depth of field costs (pt_dof_planes: k_dof_tile, k_dof_neighbour, k_dof_gather) beside two yardsticks timed in the
same process on the same planes: the chain's cheapest full-frame pass (pt_modulate_planes without an albedo: one plane in, one plane out)
and motion blur (pt_motion_blur_planes, whose sources this pass does not touch).

1920 x 1080, one MI355X.  Steps, each a process of its own under `timeout`; the first step that fails ends the tool with its status (nothing
is tried twice):
  kernels-sharp       aperture > 0 and a depth plane equal to the focus: every tile leaves early.  Bytes per pixel: 4 (depth, the tile pass)
                      + 16 (colour) + 16 (out) against motion blur's static 8 + 16 + 16, which takes turns with it (zero motion).
  kernels-uniform     one colour plane, every pixel at twice the focus distance under aperture 24: a uniform radius of 12 pixels; 8, 16, 32
                      and 64 taps.  Motion blur at 12 taps under a uniform 16-pixel velocity takes turns with them.
  kernels-two_box, kernels-c3_terrain
                      the scene's accumulation buffer after two subframes under the sky probe, depth from renderGBuffer, focused on the near
                      object (the 5th percentile of the finite depths), aperture 12; 8, 16, 32 and 64 taps.
  variant-NAME-CONTENT
                      with --variant NAME: the kernels step of CONTENT on optixpathtracer_amd/variants/libptamd_NAME.so (tools/variants.sh),
                      for an A/B of a build flag or of an edited kernel.
  trace-sharp         depth of field alone on the sharp frame, --reps calls: what a kernel trace is taken of (rocprofv3 --kernel-trace --stats
                      -- python3 tools/dof_bench.py --step trace-sharp).
Kernel times are the calls' own kernel_ms (hipEvents around the launches; the uploads of the tables in front of them excluded), medians over
--reps calls after --warmup, the calls taking turns on the same planes; next to them the host time around the whole Python call.
`us per tap` is the slope of kernel_ms between the fewest and the most taps of a table.  `loaded GB/s` is (gathered x taps x 4 bytes of depth
+ counted taps x 16 bytes of colour) over the call's kernel time.  No threshold is attached to any figure.  Prints one JSON object;
--md PATH also writes the tables as markdown with the raw JSON below them, replacing that file's part from "## Timings" on.
  python3 tools/dof_bench.py [--reps 50] [--warmup 10] [--variant NAME] [--md profiles/dof.md]
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
TAPS = (8, 16, 32, 64)
CONTENTS = ("sharp", "uniform", "two_box", "c3_terrain")
STEPS = [(f"kernels-{n}", 300) for n in CONTENTS]  # (step, seconds allowed)
FOCUS = 3.0


def _setup(content):
    """(renderer, model, colour, depth, motion, lens) on the device"""
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
    motion = torch.zeros((H, W, 2), device="cuda:0")
    if content not in real:
        color = torch.tensor([3.0, 2.0, 1.0, 1.0], device="cuda:0").repeat(H, W, 1).contiguous()
        depth = torch.full((H, W), FOCUS if content == "sharp" else 2.0 * FOCUS, device="cuda:0")
        if content == "uniform":
            motion[..., 0] = 64.0  # times hs = 0.25: 16 pixels of velocity, for the motion-blur yardstick
        return r, model, color, depth, motion, dict(focus=FOCUS, aperture=24.0)
    r.launchParams.samples_per_launch = 1
    for n in (0, 1):
        r.launchParams.frame.subframe_index = n
        r.render()
    r.sync()
    color = torch.from_numpy(r.download(R.PT_BUF_ACCUM).astype(np.float32).reshape(H, W, 4)).to("cuda:0")
    depth = r.renderGBuffer(("depth",))["depth"]
    z = depth.cpu().numpy()
    focus = float(np.percentile(z[np.isfinite(z)], 5.0))
    return r, model, color, depth, motion, dict(focus=focus, aperture=12.0)


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
    return {name: dict(kernel_ms=float(np.median(ms[name])), kernel_min_ms=float(min(ms[name])), kernel_max_ms=float(max(ms[name])),
                       host_ms=float(np.median(host[name])), **{k: v for k, v in stats[name].items() if k != "kernel_ms"}) for name, _ in calls}


def step_kernels(args, content):
    import torch

    r, model, color, depth, motion, lens = _setup(content)
    out = torch.zeros((H, W, 4), device="cuda:0")
    dims, nbytes = r.dofLayout()
    scratch = torch.zeros((nbytes // 4,), device="cuda:0")
    tiles = torch.zeros((r.motionBlurLayout()[1] // 8, 2), device="cuda:0")
    calls = [("modulate", lambda: r.modulatePlanes(color, out=out)["stats"])]
    if content in ("sharp", "uniform"):
        calls.append(("motion blur, 12 taps", lambda: r.motionBlurPlanes(color, motion, depth, out=out, scratch=tiles, taps=12)["stats"]))
    for taps in (32,) if content == "sharp" else TAPS:
        calls.append((f"depth of field, {taps} taps", lambda taps=taps: r.dofPlanes(color, depth, out=out, scratch=scratch, taps=taps, **lens)["stats"]))
    rows = _timed(args, calls)
    r.close()
    return dict(triangles=model.num_triangles, tiles=[int(dims[0, 0]), int(dims[0, 1])], scratch_bytes=nbytes, lens=lens, rows=rows)


def step_trace(args, content):
    import torch

    r, _, color, depth, _, lens = _setup(content)
    out = torch.zeros((H, W, 4), device="cuda:0")
    scratch = torch.zeros((r.dofLayout()[1] // 4,), device="cuda:0")
    ms = [r.dofPlanes(color, depth, out=out, scratch=scratch, **lens)["stats"]["kernel_ms"] for _ in range(args.warmup + args.reps)]
    r.close()
    return dict(kernel_ms=float(np.median(ms[args.warmup:])), calls=len(ms))


def _table(name, k):
    base = k["rows"]["modulate"]["kernel_ms"]
    md = [f"`{name}`: {k['tiles'][0]} x {k['tiles'][1]} tiles, scratch {k['scratch_bytes']} bytes, focus {k['lens']['focus']:.4g}, aperture {k['lens']['aperture']:g}.\n",
          "| call | `kernel_ms` median (min .. max) | x modulate | gathered | GB/s | host ms around the call | counters |", "|---|---|---|---|---|---|---|"]
    dof = []
    for call, row in k["rows"].items():
        share = ""
        if call == "modulate":
            rate = 32.0 * W * H / (row["kernel_ms"] * 1e-3) / 1e9
        elif call.startswith("motion blur"):
            rate = row["moving"] * 12 * 28.0 / (row["kernel_ms"] * 1e-3) / 1e9
        else:
            taps = int(call.split(",")[1].split()[0])
            dof.append((taps, row["kernel_ms"]))
            rate = (row["gathered"] * taps * 4.0 + row["taps"] * 16.0) / (row["kernel_ms"] * 1e-3) / 1e9
            share = f"{100.0 * row['gathered'] / max(1, row['pixels']):.1f} %"
        cnt = ", ".join(f"{c} {row[c]}" for c in ("pixels", "sources", "unknown", "moving", "gathered", "taps", "nonfinite") if c in row)
        md.append(f"| `{call}` | {row['kernel_ms']:.4f} ({row['kernel_min_ms']:.4f} .. {row['kernel_max_ms']:.4f}) | {row['kernel_ms'] / base:.2f} | {share} | {rate:.0f} "
                  f"| {row['host_ms']:.4f} | {cnt} |")
    if len(dof) > 1:
        md.append(f"\n{(dof[-1][1] - dof[0][1]) / (dof[-1][0] - dof[0][0]) * 1e3:.2f} us per tap between {dof[0][0]} and {dof[-1][0]} taps.")
    md.append("")
    return md


def markdown(res):
    md = ["## Timings (`tools/dof_bench.py`)\n",
          f"{W} x {H}, one MI355X; kernel times are the calls' own `kernel_ms`, medians (minimum .. maximum) over {res['reps']} calls after "
          f"{res['warmup']} warm-up calls, the calls taking turns on the same planes in one process.  `modulate` is `pt_modulate_planes` without an "
          "albedo (32 bytes a pixel); `motion blur` is `pt_motion_blur_planes` (its sources are the parent commit's).  `x modulate` is the row's "
          "`kernel_ms` over `modulate`'s of the same table; `gathered` the share of the pixels that gather; `GB/s` is what the row's loads and "
          "stores add up to over `kernel_ms` (depth of field: gathered x taps x 4 bytes of depth + counted taps x 16 bytes of colour).  No "
          "threshold is attached to any of these figures.\n"]
    for key, k in res.items():
        if key.startswith("kernels-"):
            md += _table(key[8:], k)
        if key.startswith("variant-"):
            md += _table(key, k)
    md += ["## Raw output\n", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--variant", help="also time `uniform` and `two_box` on optixpathtracer_amd/variants/libptamd_NAME.so")
    ap.add_argument("--md", help="also write the tables as markdown to this path")
    ap.add_argument("--step", help="run one step in this process and print its JSON line")
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, ROOT)
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("dof_bench: no GPU")
        kind, content = args.step.split("-", 1)
        if kind == "variant":
            from optixpathtracer_amd import _lib

            name, content = content.split("-", 1)
            _lib.LIB_PATH = os.path.join(ROOT, "optixpathtracer_amd", "variants", f"libptamd_{name}.so")
        print("RESULT " + json.dumps(dict(trace=step_trace).get(kind, step_kernels)(args, content)), flush=True)
        return 0
    res = dict(reps=args.reps, warmup=args.warmup)
    passed = ["--reps", str(args.reps), "--warmup", str(args.warmup)]
    steps = STEPS + ([(f"variant-{args.variant}-{c}", 300) for c in ("uniform", "two_box")] if args.variant else [])
    for step, seconds in steps:  # one attempt each; the first failure ends the tool
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step] + passed, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"dof_bench: step {step} ended with status {p.returncode}", file=sys.stderr)
            return p.returncode
        res[step] = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Depth of field (`pt_dof_layout`, `pt_dof_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
