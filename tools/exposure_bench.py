#!/usr/bin/env python3
"""exposure_bench.py — what auto exposure and the display tone mapper cost (pt_exposure_planes: k_meter + k_adapt; pt_tonemap_planes:
k_tonemap) beside the chain's cheapest full-frame pass (pt_modulate_planes without an albedo: one plane in, one plane out) on the same
tensor.

1920 x 1080, one MI355X.  Steps, each a process of its own under `timeout`; the first step that fails ends the tool with its status (nothing
is tried twice):
  kernels-<content>  the colour is linear radiance: on the Cornell box and on the C3 scene (voxel_terrain, 1 M triangles, bench.py's camera)
                     the accumulation buffer after two subframes under the sky probe, with the G-buffer's hit plane; `constant` is one
                     colour in every pixel (every pixel in one bin: the contention extreme) and no hit plane.  k_modulate, the meter
                     (without and with the hit plane; under two side-by-side views) and k_tonemap (out, the packed frame, both) take
                     turns; with every time the pass's counters.
Kernel times are the calls' own kernel_ms (hipEvents around the launches: for the meter k_meter and k_adapt together, the clear of the
histogram in front of them excluded), medians over --reps calls after --warmup; next to them the host time around the whole Python call.
No threshold is attached to any figure.  Prints one JSON object; --md PATH also writes the tables as markdown with the raw JSON below them,
replacing that file's part from "## Timings" on.
  python3 tools/exposure_bench.py [--reps 50] [--warmup 10] [--md profiles/exposure.md]
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
CONTENTS = ("cornell", "c3_terrain", "constant")
STEPS = [(f"kernels-{n}", 300) for n in CONTENTS]  # (step, seconds allowed)


def _scene(name):
    from optixpathtracer_amd import scenes

    return {"c3_terrain": (scenes.voxel_terrain, scenes.TERRAIN_CAMERA), "cornell": (scenes.cornell_box, scenes.CORNELL_CAMERA),
            "constant": (scenes.cornell_box, scenes.CORNELL_CAMERA)}[name]


def step_kernels(args, content):
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    make, cam0 = _scene(content)
    model = make()
    r = R.SampleRenderer(model)
    r.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    r.resize((W, H))
    r.setCamera(R.make_camera(cam0, W / H))
    hit = None
    if content == "constant":
        color = torch.tensor([0.3, 0.2, 0.1, 1.0], device="cuda:0").repeat(H, W, 1).contiguous()
    else:
        r.launchParams.samples_per_launch = 1
        for n in (0, 1):
            r.launchParams.frame.subframe_index = n
            r.render()
        r.sync()
        color = torch.from_numpy(r.download(R.PT_BUF_ACCUM).astype(np.float32).reshape(H, W, 4)).to("cuda:0")
        hit = r.renderGBuffer(("hit",))["hit"]
    out, frame = torch.zeros((H, W, 4), device="cuda:0"), torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    hist, state = torch.zeros((1, 256), dtype=torch.int32, device="cuda:0"), torch.zeros((1, 4), device="cuda:0")
    calls = [("modulate", lambda: r.modulatePlanes(color, out=out)["stats"]),
             ("exposure", lambda: r.exposurePlanes(color, hist=hist, state_out=state)["stats"])]
    if hit is not None:
        calls.append(("exposure+hit", lambda: r.exposurePlanes(color, hit, hist=hist, state_out=state)["stats"]))
    calls += [("tonemap", lambda: r.tonemapPlanes(color, state=state, out=out, op="aces")["stats"]),
              ("tonemap, frame alone", lambda: r.tonemapPlanes(color, state=state, frame=frame, op="aces", write_out=False)["stats"]),
              ("tonemap+frame", lambda: r.tonemapPlanes(color, state=state, out=out, frame=frame, op="aces")["stats"])]

    def timed(calls):
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
        rows = {}
        for name, _ in calls:
            st = stats[name]
            rows[name] = dict(kernel_ms=float(np.median(ms[name])), kernel_min_ms=float(min(ms[name])), host_ms=float(np.median(host[name])),
                              **{k: v for k, v in st.items() if k != "kernel_ms"})
        return rows

    rows = timed(calls)
    ev = float(state[0, 0])
    bins = int((hist != 0).sum())
    # two views side by side: the pixel list is in block-raster order, so the views alternate along every block row
    r.setViews([(0, 0, W // 2, H, R.make_camera(cam0, W / 2 / H)), (W // 2, 0, W // 2, H, R.make_camera(cam0, W / 2 / H))])
    hist2, state2 = torch.zeros((2, 256), dtype=torch.int32, device="cuda:0"), torch.zeros((2, 4), device="cuda:0")
    views = timed([("modulate, 2 views", lambda: r.modulatePlanes(color, out=out)["stats"]),
                   ("exposure, 2 views", lambda: r.exposurePlanes(color, hit, hist=hist2, state_out=state2)["stats"]),
                   ("tonemap, 2 views", lambda: r.tonemapPlanes(color, state=state2, out=out, op="aces")["stats"])])
    rows.update(views)
    r.close()
    return dict(triangles=model.num_triangles, ev=ev, bins_in_use=bins, rows=rows)


def markdown(res):
    md = ["## Timings (`tools/exposure_bench.py`)\n",
          f"{W} x {H}, one MI355X; kernel times are the calls' own `kernel_ms`, medians (minima in brackets) over {res['reps']} calls after "
          f"{res['warmup']} warm-up calls, the kernels taking turns on the same planes in one process.  `modulate` is `pt_modulate_planes` "
          "without an albedo: it reads the colour plane and writes `out`.  `exposure` is k_meter and k_adapt together.  `x modulate` is the "
          "row's `kernel_ms` over `modulate`'s (over `modulate, 2 views` for the rows under views).  No threshold is attached to any of "
          "these figures.\n"]
    for content in CONTENTS:
        k = res[f"kernels-{content}"]
        md += [f"`{content}`: {k['bins_in_use']} bins in use, ev {k['ev']:+.3f}.\n",
               "| call | `kernel_ms` | x modulate | host ms around the call | counters |", "|---|---|---|---|---|"]
        for name, row in k["rows"].items():
            base = k["rows"]["modulate, 2 views" if "2 views" in name else "modulate"]["kernel_ms"]
            cnt = ", ".join(f"{c} {row[c]}" for c in ("pixels", "skipped", "nonfinite", "under", "over", "clipped") if c in row)
            md.append(f"| `{name}` | {row['kernel_ms']:.4f} ({row['kernel_min_ms']:.4f}) | {row['kernel_ms'] / base:.2f} | {row['host_ms']:.4f} | {cnt} |")
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
            raise SystemExit("exposure_bench: no GPU")
        print("RESULT " + json.dumps(step_kernels(args, args.step.split("-", 1)[1])), flush=True)
        return 0
    res = dict(reps=args.reps, warmup=args.warmup)
    passed = ["--reps", str(args.reps), "--warmup", str(args.warmup)]
    for step, seconds in STEPS:  # one attempt each; the first failure ends the tool
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step] + passed, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"exposure_bench: step {step} ended with status {p.returncode}", file=sys.stderr)
            return p.returncode
        res[step] = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Auto exposure and tone mapping (`pt_exposure_planes`, `pt_tonemap_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
