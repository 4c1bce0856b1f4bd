#!/usr/bin/env python3
"""bloom_bench.py — what bloom costs (pt_bloom_planes: k_bloom_down1, k_bloom_down, k_bloom_tail, k_bloom_up, k_bloom_composite) beside the
chain's cheapest full-frame pass (pt_modulate_planes without an albedo: one plane in, one plane out) on the same tensor.

1920 x 1080, 6 levels, one MI355X.  Steps, each a process of its own under `timeout`; the first step that fails ends the tool with its status
(nothing is tried twice):
  kernels-<content>  the colour is linear radiance: on the Cornell box and on the C3 scene (voxel_terrain, 1 M triangles, bench.py's camera)
                     the accumulation buffer after two subframes under the sky probe; `constant` is one colour in every pixel.  k_modulate
                     and bloom take turns — bloom at the library's tail cut-off and at each of --cutoffs (PT_BLOOM_TAIL_TEXELS, read by the
                     library per call: 0 is "no tail") — then both under two side-by-side views.
  views16-constant   where the tail earns its keep: 16 views of 64 x 64 in a 256 x 256 frame, every level from 2 on small — bloom at the
                     library's cut-off (three launches) and without a tail (twelve).
  trace-cornell      bloom alone, --reps calls: what a kernel trace is taken of (rocprofv3 --kernel-trace --stats -- python3
                     tools/bloom_bench.py --step trace-cornell).
Kernel times are the calls' own kernel_ms (hipEvents around the launches; the upload of the level table in front of them excluded), medians
over --reps calls after --warmup; next to them the host time around the whole Python call.  The yardstick is bytes: colour read by
k_bloom_down1 and again by the composite, out written, every level written once and read by its two consumers, and one re-read and
re-write per level for the up pass, over k_modulate's two frame planes — stated from pt_bloom_layout's sizes.  No threshold is attached to
any figure.  Prints one JSON object; --md PATH also writes the tables as markdown with the raw JSON below them, replacing that file's part
from "## Timings" on.
  python3 tools/bloom_bench.py [--reps 50] [--warmup 10] [--cutoffs 0 2048 16384 32768] [--md profiles/bloom.md]
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

W, H, LEVELS = 1920, 1080, 6
CONTENTS = ("cornell", "c3_terrain", "constant")
STEPS = [(f"kernels-{n}", 300) for n in CONTENTS] + [("views16-constant", 120)]  # (step, seconds allowed)
PRM = dict(threshold=1.0, knee=0.5, clamp=65504.0, spread=0.7, intensity=0.25, levels=LEVELS)


def _scene(name):
    from optixpathtracer_amd import scenes

    return {"c3_terrain": (scenes.voxel_terrain, scenes.TERRAIN_CAMERA), "cornell": (scenes.cornell_box, scenes.CORNELL_CAMERA),
            "constant": (scenes.cornell_box, scenes.CORNELL_CAMERA)}[name]


def byte_ratio(dims, pixels):
    """the call's algorithmic traffic over k_modulate's, from the layout: (3 frame planes + 5 x every level) / 2 frame planes"""
    texels = int((dims[..., 0].astype(np.int64) * dims[..., 1]).sum())
    return (3 * pixels + 5 * texels) / (2 * pixels), texels


def _setup(content):
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    make, cam0 = _scene(content)
    model = make()
    r = R.SampleRenderer(model)
    r.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    r.resize((W, H))
    r.setCamera(R.make_camera(cam0, W / H))
    if content == "constant":
        color = torch.tensor([3.0, 2.0, 1.0, 1.0], device="cuda:0").repeat(H, W, 1).contiguous()
    else:
        r.launchParams.samples_per_launch = 1
        for n in (0, 1):
            r.launchParams.frame.subframe_index = n
            r.render()
        r.sync()
        color = torch.from_numpy(r.download(R.PT_BUF_ACCUM).astype(np.float32).reshape(H, W, 4)).to("cuda:0")
    return r, model, cam0, color


def _bloom_at(r, cutoff, **kw):
    """one bloom call with the tail's cut-off set for this call alone (None: the library's own)"""
    if cutoff is None:
        os.environ.pop("PT_BLOOM_TAIL_TEXELS", None)
    else:
        os.environ["PT_BLOOM_TAIL_TEXELS"] = str(cutoff)
    try:
        return r.bloomPlanes(**kw)["stats"]
    finally:
        os.environ.pop("PT_BLOOM_TAIL_TEXELS", None)


def step_kernels(args, content):
    import torch

    from optixpathtracer_amd import renderer as R

    r, model, cam0, color = _setup(content)
    out = torch.zeros((H, W, 4), device="cuda:0")
    dims, nbytes = r.bloomLayout(LEVELS)
    scratch = torch.zeros((nbytes // 16, 4), device="cuda:0")
    ratio, texels = byte_ratio(dims, W * H)
    kw = dict(color=color, out=out, scratch=scratch, **PRM)
    calls = [("modulate", lambda: r.modulatePlanes(color, out=out)["stats"]), ("bloom", lambda: _bloom_at(r, None, **kw))]
    calls += [(f"bloom, tail from {c} texels" if c else "bloom, no tail", lambda c=c: _bloom_at(r, c, **kw)) for c in args.cutoffs]

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
    # two views side by side: two pyramids of half the width, no tap across the seam
    r.setViews([(0, 0, W // 2, H, R.make_camera(cam0, W / 2 / H)), (W // 2, 0, W // 2, H, R.make_camera(cam0, W / 2 / H))])
    dims2, nbytes2 = r.bloomLayout(LEVELS)
    scratch2 = torch.zeros((nbytes2 // 16, 4), device="cuda:0")
    ratio2, texels2 = byte_ratio(dims2, W * H)
    rows.update(timed([("modulate, 2 views", lambda: r.modulatePlanes(color, out=out)["stats"]),
                       ("bloom, 2 views", lambda: _bloom_at(r, None, color=color, out=out, scratch=scratch2, **PRM))]))
    r.close()
    return dict(triangles=model.num_triangles, level_texels=[int(a) * int(b) for a, b, _, _ in dims[0, :LEVELS]], pyramid_texels=texels, byte_ratio=ratio,
                pyramid_texels_2_views=texels2, byte_ratio_2_views=ratio2, rows=rows)


def step_views16(args, content):
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    n = 256
    r = R.SampleRenderer(scenes.cornell_box())
    r.resize((n, n))
    cam = R.make_camera(scenes.CORNELL_CAMERA, 1.0)
    r.setViews([(64 * i, 64 * j, 64, 64, cam) for j in range(4) for i in range(4)])
    color = torch.tensor([3.0, 2.0, 1.0, 1.0], device="cuda:0").repeat(n, n, 1).contiguous()
    out = torch.zeros((n, n, 4), device="cuda:0")
    scratch = torch.zeros((r.bloomLayout(LEVELS)[1] // 16, 4), device="cuda:0")
    kw = dict(color=color, out=out, scratch=scratch, **PRM)
    ms = {"bloom": [], "bloom, no tail": []}
    for k in range(args.warmup + args.reps):
        for name, cut in (("bloom", None), ("bloom, no tail", 0)):
            st = _bloom_at(r, cut, **kw)
            if k >= args.warmup:
                ms[name].append(st["kernel_ms"])
    r.close()
    return dict(frame=[n, n], views=16, rows={k: dict(kernel_ms=float(np.median(v)), kernel_min_ms=float(min(v))) for k, v in ms.items()})


def step_trace(args, content):
    import torch

    r, _, _, color = _setup(content)
    out = torch.zeros((H, W, 4), device="cuda:0")
    scratch = torch.zeros((r.bloomLayout(LEVELS)[1] // 16, 4), device="cuda:0")
    ms = [r.bloomPlanes(color, out=out, scratch=scratch, **PRM)["stats"]["kernel_ms"] for _ in range(args.warmup + args.reps)]
    r.close()
    return dict(kernel_ms=float(np.median(ms[args.warmup:])), calls=len(ms))


def markdown(res):
    md = ["## Timings (`tools/bloom_bench.py`)\n",
          f"{W} x {H}, {LEVELS} levels, one MI355X; kernel times are the calls' own `kernel_ms`, medians (minima in brackets) over {res['reps']} calls "
          f"after {res['warmup']} warm-up calls, the calls taking turns on the same planes in one process.  `modulate` is `pt_modulate_planes` "
          "without an albedo: it reads the colour plane and writes `out`.  `bloom` is the whole of `pt_bloom_planes` at the library's own tail "
          "cut-off; the rows below it set `PT_BLOOM_TAIL_TEXELS` for the call.  `x modulate` is the row's `kernel_ms` over `modulate`'s (over "
          "`modulate, 2 views` for the rows under views); `bytes` is the call's algorithmic traffic over `k_modulate`'s, from the layout.  "
          "No threshold is attached to any of these figures.\n"]
    for content in CONTENTS:
        k = res[f"kernels-{content}"]
        md += [f"`{content}`: levels of {k['level_texels']} texels; bytes over `k_modulate`'s {k['byte_ratio']:.3f} ({k['byte_ratio_2_views']:.3f} under two views).\n",
               "| call | `kernel_ms` | x modulate | bytes | host ms around the call | counters |", "|---|---|---|---|---|---|"]
        for name, row in k["rows"].items():
            two = "2 views" in name
            base = k["rows"]["modulate, 2 views" if two else "modulate"]["kernel_ms"]
            ratio = 1.0 if name.startswith("modulate") else k["byte_ratio_2_views" if two else "byte_ratio"]
            cnt = ", ".join(f"{c} {row[c]}" for c in ("pixels", "sources", "bright", "nonfinite") if c in row)
            md.append(f"| `{name}` | {row['kernel_ms']:.4f} ({row['kernel_min_ms']:.4f}) | {row['kernel_ms'] / base:.2f} | {ratio:.2f} | {row['host_ms']:.4f} | {cnt} |")
        md.append("")
    v = res["views16-constant"]
    md += [f"{v['views']} views of 64 x 64 in a {v['frame'][0]} x {v['frame'][1]} frame, {LEVELS} levels (every level from 2 on is the tail's):\n", "| call | `kernel_ms` |", "|---|---|"]
    md += [f"| `{name}` | {row['kernel_ms']:.4f} ({row['kernel_min_ms']:.4f}) |" for name, row in v["rows"].items()] + [""]
    md += ["## Raw output\n", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cutoffs", type=int, nargs="*", default=[0, 2048, 16384, 32768], help="tail cut-offs to try beside the library's own; 0: no tail")
    ap.add_argument("--md", help="also write the tables as markdown to this path")
    ap.add_argument("--step", help="run one step in this process and print its JSON line")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bloom_bench: no GPU")
        kind, content = args.step.split("-", 1)
        print("RESULT " + json.dumps(dict(trace=step_trace, views16=step_views16).get(kind, step_kernels)(args, content)), flush=True)
        return 0
    res = dict(reps=args.reps, warmup=args.warmup, cutoffs=args.cutoffs)
    passed = ["--reps", str(args.reps), "--warmup", str(args.warmup), "--cutoffs"] + [str(c) for c in args.cutoffs]
    for step, seconds in STEPS:  # one attempt each; the first failure ends the tool
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step] + passed, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"bloom_bench: step {step} ended with status {p.returncode}", file=sys.stderr)
            return p.returncode
        res[step] = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Bloom (`pt_bloom_layout`, `pt_bloom_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
