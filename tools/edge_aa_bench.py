#!/usr/bin/env python3
"""edge_aa_bench.py — what geometric edge antialiasing costs (pt_edge_aa_planes, k_edge_aa) beside the chain's cheapest full-frame pass
(pt_modulate_planes, k_modulate) on the same frame.

1920 x 1080, one MI355X.  Steps, each a process of its own under `timeout`; the first step that fails ends the tool with its status (nothing
is tried twice):
  kernels-<scene>  on the C3 scene (voxel_terrain, 1 M triangles, bench.py's camera), on the Cornell box and on the textured scene: one
                   G-buffer (hit, position), the pixel-centre albedo as the colour; k_modulate (colour and albedo in, colour out) and
                   k_edge_aa — `out` alone, with the `edge` plane, with `edge` and the packed frame — taking turns; with every time the
                   pass's counters: the share of boundary and of blended pixels.
Kernel times are the calls' own kernel_ms (hipEvents around the launch), medians over --reps calls after --warmup; next to them the host
time around the whole Python call.  No threshold is attached to any figure.  Prints one JSON object; --md PATH also writes the tables as
markdown with the raw JSON below them, replacing that file's part from "## Timings" on.
  python3 tools/edge_aa_bench.py [--reps 50] [--warmup 10] [--md profiles/edge_aa.md]
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
SCENE_NAMES = ("c3_terrain", "cornell", "textured")
STEPS = [(f"kernels-{n}", 300) for n in SCENE_NAMES]  # (step, seconds allowed)


def _scene(name):
    from optixpathtracer_amd import scenes

    return {"c3_terrain": (scenes.voxel_terrain, scenes.TERRAIN_CAMERA), "cornell": (scenes.cornell_box, scenes.CORNELL_CAMERA),
            "textured": (scenes.textured_scene, dict(eye=(3.0, 2.5, -4.5), lookat=(0.0, 0.6, 0.5), up=(0.0, 1.0, 0.0), fovY=45.0))}[name]


def step_kernels(args, scene):
    import torch

    from optixpathtracer_amd import renderer as R

    make, cam0 = _scene(scene)
    model = make()
    r = R.SampleRenderer(model)
    r.resize((W, H))
    r.setCamera(R.make_camera(cam0, W / H))
    g = r.renderGBuffer(("hit", "position"))
    hit, position = g["hit"], g["position"]
    color = r.surfacePlanes(hit, r.copyTexcoordsDevice(), planes=("albedo",))["albedo"]
    zeros = lambda k: torch.zeros((H, W, k), device="cuda:0")  # noqa: E731
    out, edge, frame = zeros(4), zeros(2), torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    calls = [("modulate", lambda: r.modulatePlanes(color, albedo=color, out=out)["stats"]),
             ("edge_aa", lambda: r.edgeAaPlanes(color, hit, position, out=out)["stats"]),
             ("edge_aa+edge", lambda: r.edgeAaPlanes(color, hit, position, out=out, edge=edge)["stats"]),
             ("edge_aa+edge+frame", lambda: r.edgeAaPlanes(color, hit, position, out=out, edge=edge, frame=frame)["stats"])]
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
        rows[name] = dict(kernel_ms=float(np.median(ms[name])), kernel_min_ms=float(min(ms[name])), host_ms=float(np.median(host[name])), pixels=st["pixels"],
                          hits=st.get("hits", 0), boundary=st.get("boundary", 0), blended=st.get("blended", 0))
    return dict(triangles=model.num_triangles, rows=rows)


def markdown(res):
    md = ["## Timings (`tools/edge_aa_bench.py`)\n",
          f"{W} x {H}, one MI355X; kernel times are the calls' own `kernel_ms`, medians (minima in brackets) over {res['reps']} calls after "
          f"{res['warmup']} warm-up calls, the kernels taking turns on the same planes in one process.  The colour is the pixel-centre albedo; "
          "`pt_modulate_planes` reads it twice (as colour and as albedo) and writes `out`.  `boundary` and `blended` are shares of the frame's "
          "pixels.  No threshold is attached to any of these figures.\n"]
    for scene in SCENE_NAMES:
        k = res[f"kernels-{scene}"]
        e = k["rows"]["edge_aa"]
        md += [f"`{scene}` ({k['triangles']} triangles): {e['hits']} hits of {e['pixels']} pixels, {e['boundary']} boundary, {e['blended']} blended.\n",
               "| call | `kernel_ms` | host ms around the call | boundary | blended |", "|---|---|---|---|---|"]
        for name, row in k["rows"].items():
            px = max(1, row["pixels"])
            md.append(f"| `{name}` | {row['kernel_ms']:.4f} ({row['kernel_min_ms']:.4f}) | {row['host_ms']:.4f} | {row['boundary'] / px:.4f} | {row['blended'] / px:.4f} |")
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
            raise SystemExit("edge_aa_bench: no GPU")
        print("RESULT " + json.dumps(step_kernels(args, args.step.split("-", 1)[1])), flush=True)
        return 0
    res = dict(reps=args.reps, warmup=args.warmup)
    passed = ["--reps", str(args.reps), "--warmup", str(args.warmup)]
    for step, seconds in STEPS:  # one attempt each; the first failure ends the tool
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step] + passed, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"edge_aa_bench: step {step} ended with status {p.returncode}", file=sys.stderr)
            return p.returncode
        res[step] = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Geometric edge antialiasing (`pt_edge_aa_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
