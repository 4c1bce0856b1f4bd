#!/usr/bin/env python3
"""device_update_bench.py — what feeding a geometry update from GPU memory saves (tools/refit_bench.py measures the host-fed call alone).

Per scene (C3 terrain and the stadium, 1 M triangles, every mesh named in every call, PT_UPDATE_REFIT), 20 poses, the three variants
taking turns pose by pose (host and device on one context, transforms on a second), printed as ONE JSON object with, per variant,
the median / min / max host time of the whole call (a host clock around the facade call, which returns after the library has waited
for the device) and the median kernel_ms:
  host       pt_update_meshes: host arrays — validated on the host, uploaded, refitted
  device     pt_update_meshes_device: torch tensors the GPU produced (displaced on the GPU, complete before the clock starts)
  transform  pt_transform_meshes: one 3x4 matrix per mesh, from the rest positions
--md PATH also writes the table as markdown with the raw JSON below it.

Every scene runs in a child process of its own under `timeout -k 10`; the first child that fails ends the run (nothing more is started).
  python3 tools/device_update_bench.py [--scenes terrain,stadium] [--timeout 300] [--md device_update.md]
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

POSES = 20
VARIANTS = ("host", "device", "transform")


def _rot_y(angle, lift):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s, 0], [0, 1, 0, lift], [-s, 0, c, 0]], np.float32)


def one(scene_name):
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    model = {"terrain": scenes.voxel_terrain, "stadium": scenes.stadium_scene}[scene_name]()
    r = R.SampleRenderer(model)
    rt = R.SampleRenderer(model)  # transforms on a context of their own: a context that has seen one keeps the rest array current on every explicit update
    base = {i: torch.from_numpy(np.ascontiguousarray(m.vertex, np.float32)).to("cuda:0") for i, m in enumerate(model.meshes)}

    def displaced(phase):  # the pose, computed on the GPU
        out = {}
        for i, v in base.items():
            d = torch.stack([torch.sin(0.05 * v[:, 2] + phase), torch.sin(0.04 * v[:, 0] + 1.3 * phase), torch.cos(0.03 * (v[:, 0] + v[:, 2]) + phase)], 1)
            out[i] = (v + 0.5 * d).contiguous()
        torch.cuda.synchronize()
        return out

    def call(variant, k):
        phase = 0.3 * k
        if variant == "host":
            arg = {i: t.cpu().numpy() for i, t in displaced(phase).items()}
            fn = r.updateMeshes
        elif variant == "device":
            arg = displaced(phase)
            fn = r.updateMeshesDevice
        else:
            arg = {i: _rot_y(0.01 * k, 0.05 * k) for i in base}
            fn = rt.transformMeshes
        t0 = time.perf_counter()
        kernel_ms = fn(arg)
        return (time.perf_counter() - t0) * 1e3, kernel_ms

    for v in VARIANTS:  # the first refit allocates the side arrays, the first transform the rest array, the first launch loads the kernel
        call(v, 0)
        call(v, 0)
    t = {v: [] for v in VARIANTS}
    for k in range(1, POSES + 1):
        for v in VARIANTS:
            t[v].append(call(v, k))
    out = dict(scene=scene_name, triangles=model.num_triangles, vertices=int(sum(len(m.vertex) for m in model.meshes)), meshes=len(model.meshes), poses=POSES)
    for v in VARIANTS:
        h, km = np.array(t[v]).T
        out[v] = dict(host_ms=float(np.median(h)), host_ms_min=float(h.min()), host_ms_max=float(h.max()), kernel_ms=float(np.median(km)))
    r.close()
    rt.close()
    print(json.dumps(out), flush=True)


def markdown(result):
    names = dict(host="`pt_update_meshes` (host arrays)", device="`pt_update_meshes_device` (tensors produced on the GPU)", transform="`pt_transform_meshes` (one matrix per mesh)")
    md = ["# Geometry updates fed from GPU memory (`tools/device_update_bench.py`)\n",
          "Refit of every mesh of the scene, 20 poses, the three variants taking turns pose by pose, one MI355X.  Host time: a host clock",
          "around the whole facade call (it returns after the device has been waited for); `kernel_ms`: the call's own device time",
          "(staging kernel + refit).  Medians, [min, max].\n"]
    for s, o in result.items():
        md += [f"## {s}: {o['triangles']} triangles, {o['vertices']} vertices in {o['meshes']} meshes\n", "| variant | host time of the call, ms | `kernel_ms` |", "|---|---|---|"]
        for v in VARIANTS:
            x = o[v]
            md.append(f"| {names[v]} | {x['host_ms']:.2f} [{x['host_ms_min']:.2f}, {x['host_ms_max']:.2f}] | {x['kernel_ms']:.2f} |")
        md.append("")
    md += ["## Raw output\n", "```json", json.dumps(result, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="terrain,stadium")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per scene")
    ap.add_argument("--md", help="also write the table as markdown to this path")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        one(args.one)
        return 0
    result = {}
    for s in args.scenes.split(","):
        p = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", s], capture_output=True, text=True)
        if p.returncode != 0:
            result[s] = dict(error=f"exit {p.returncode}", stderr=p.stderr[-2000:])
            print(json.dumps(result))
            return 1
        result[s] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(result))
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(markdown(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
