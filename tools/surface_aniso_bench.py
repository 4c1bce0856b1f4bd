#!/usr/bin/env python3
"""surface_aniso_bench.py — what the anisotropic footprint-filtered albedo pass costs (pt_surface_aniso_planes, k_surface_aniso) beside the
isotropic one (pt_surface_lod_planes, k_surface_lod), and what it does to the upsampled loop end to end.

1920 x 1080, one MI355X.  Steps, each a process of its own under `timeout`; the first step that fails ends the tool with its status (nothing
is tried twice):
  kernels-<scene>  on textured_terrain (1 M triangles, 1024 x 1024 band textures) and on the textured scene: k_surface_lod and
                   k_surface_aniso at max_aniso 1, 2, 4, 8 and 16 taking turns on ONE hit plane, albedo alone; with every time the pass's
                   counters: the share of anisotropic pixels among the textured ones and the mean number of taps;
  loop             the terrain orbit of examples/upsampled_svgf_loop.py --scale 2 --lod, without and with --aniso 8, taking turns --rounds
                   times: host time around a whole frame and the display-resolution surface pass's kernel_ms; then the rms of each variant's
                   final frame against a converged full-resolution frame (--reference-spp samples, PT_BUF_COLOR of a standing camera at the
                   orbit's last position).
Kernel times are the calls' own kernel_ms (hipEvents around the launch), medians over --reps calls after --warmup; next to them the host
time around the whole Python call.  No threshold is attached to any figure.  Prints one JSON object; --md PATH also writes the tables as
markdown with the raw JSON below them, replacing that file's part from "## Timings" on.
  python3 tools/surface_aniso_bench.py [--reps 50] [--warmup 10] [--frames 24] [--rounds 2] [--md profiles/surface_aniso.md]
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
ANISO = (1, 2, 4, 8, 16)
SCENE_NAMES = ("terrain", "textured")
STEPS = [(f"kernels-{n}", 300) for n in SCENE_NAMES] + [("loop", 420)]  # (step, seconds allowed)


def _example():
    spec = importlib.util.spec_from_file_location("upsampled_svgf_loop", os.path.join(ROOT, "examples", "upsampled_svgf_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def step_kernels(args, scene):
    import torch

    from optixpathtracer_amd import renderer as R

    make, cam0 = _example().SCENES[scene]
    model = make()
    r = R.SampleRenderer(model)
    r.resize((W, H))
    r.setCamera(R.make_camera(cam0, W / H))
    hit = r.renderGBuffer(("hit",))["hit"]
    table, mips = r.copyTexcoordsDevice(), r.copyTextureMipsDevice()
    out = dict(albedo=torch.zeros((H, W, 4), device="cuda:0"))
    calls = [("lod", lambda: r.surfaceLodPlanes(hit, table, mips, out=out)["stats"])]
    for n in ANISO:
        calls.append((str(n), lambda n=n: r.surfaceAnisoPlanes(hit, table, mips, max_aniso=n, out=out)["stats"]))
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
                          hits=st["hits"], textured=st["textured"], minified=st["minified"], anisotropic=st.get("anisotropic", 0), taps=st.get("taps", st["textured"]))
    return dict(triangles=model.num_triangles, rows=rows)


def step_loop(args):
    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    ex = _example()
    make, cam0 = ex.SCENES["terrain"]
    model = make()
    probe = scenes.sky_probe(1024, 512).BuildCDF()
    loops = {"lod": ex.UpsampledLoop(model, (W, H), 2, lod=True, probe=probe), "aniso": ex.UpsampledLoop(model, (W, H), 2, lod=True, aniso=8, probe=probe)}
    cams = [R.make_camera(ex.orbit(cam0, 0.01 * k), W / H) for k in range(args.frames)]

    def run(up):
        up.lo.uploadAccum(np.zeros((H // 2, W // 2, 4), np.float32))
        for t in list(up.gbuf[0].values()) + list(up.gbuf[1].values()) + up.history + up.moments + up.length:
            t.zero_()
        rows, cam = [], R.make_camera(cam0, W / H)
        for k in range(args.frames):
            prev, cam = cam, cams[k]
            rows.append(up.frame(k, prev, cam))
        return rows[args.loop_warmup:]

    runs = {k: [] for k in loops}
    for _ in range(args.rounds):
        for which, up in loops.items():
            runs[which] += run(up)
    images = {k: up.final.cpu().numpy()[..., :3].astype(np.float64) for k, up in loops.items()}
    for up in loops.values():
        up.close()
    # the converged frame: a standing camera at the orbit's last position, --reference-spp samples in subframes of 32
    r = R.SampleRenderer(model)
    r.setProbe(probe)
    r.resize((W, H))
    r.setCamera(cams[-1])
    r.uploadAccum(np.zeros((H, W, 4), np.float32))
    r.launchParams.samples_per_launch = 32
    for k in range(max(1, args.reference_spp // 32)):
        r.launchParams.frame.subframe_index = k
        r.render()
    r.sync()
    reference = r.download(R.PT_BUF_COLOR)[..., :3].astype(np.float64)
    r.close()
    med = lambda rows, key: float(np.median([x[key] for x in rows]))  # noqa: E731
    res = dict(triangles=model.num_triangles, frames=args.frames, warmup=args.loop_warmup, rounds=args.rounds, reference_spp=32 * max(1, args.reference_spp // 32))
    for k in loops:
        res[k] = dict(frame_ms=med(runs[k], "frame_ms"), hi_ms=med(runs[k], "hi_ms"), surface_ms=med(runs[k], "surface_ms"), lo_surface_ms=med(runs[k], "lo_surface_ms"),
                      rms=float(np.sqrt(((images[k] - reference) ** 2).mean())))
    return res


def markdown(res):
    md = ["## Timings (`tools/surface_aniso_bench.py`)\n",
          f"{W} x {H}, one MI355X; kernel times are the calls' own `kernel_ms`, medians (minima in brackets) over {res['reps']} calls after "
          f"{res['warmup']} warm-up calls, the kernels taking turns on the same hit plane in one process, albedo alone.  `anisotropic` is the share of "
          "the textured pixels with N > 1, `taps` the mean N over the textured pixels.  No threshold is attached to any of these figures.\n"]
    for scene in SCENE_NAMES:
        k = res[f"kernels-{scene}"]
        any_row = k["rows"]["lod"]
        md += [f"`{scene}` ({k['triangles']} triangles): {any_row['hits']} hits, {any_row['textured']} textured, {any_row['minified']} minified.\n",
               "| kernel | `max_aniso` | `kernel_ms` | host ms around the call | anisotropic | taps |", "|---|---|---|---|---|---|"]
        for name, row in k["rows"].items():
            tex = max(1, row["textured"])
            kernel = "`k_surface_lod<false, true>`" if name == "lod" else "`k_surface_aniso<false, true>`"
            md.append(f"| {kernel} | {'-' if name == 'lod' else name} | {row['kernel_ms']:.4f} ({row['kernel_min_ms']:.4f}) | {row['host_ms']:.4f} | "
                      f"{row['anisotropic'] / tex:.3f} | {row['taps'] / tex:.2f} |")
        md.append("")
    lp = res["loop"]
    md += [f"The upsampled loop end to end (`examples/upsampled_svgf_loop.py --scene terrain --scale 2 --lod`), an orbit of {lp['frames']} frames at 1 spp, "
           f"without and with `--aniso 8` taking turns {lp['rounds']} times, medians after {lp['warmup']} warm-up frames; rms of the final frame's three colour "
           f"words against a converged full-resolution frame ({lp['reference_spp']} spp, `PT_BUF_COLOR` of a standing camera at the orbit's last position).\n",
           "| variant | ms per frame | display-resolution part | its surface pass `kernel_ms` | low-resolution surface pass | rms against the converged frame |",
           "|---|---|---|---|---|---|"]
    for k, label in (("lod", "`--lod`"), ("aniso", "`--lod --aniso 8`")):
        x = lp[k]
        md.append(f"| {label} | {x['frame_ms']:.3f} | {x['hi_ms']:.3f} | {x['surface_ms']:.4f} | {x['lo_surface_ms']:.4f} | {x['rms']:.5f} |")
    md += ["", "## Raw output\n", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--loop-warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reference-spp", type=int, default=256)
    ap.add_argument("--md", help="also write the tables as markdown to this path")
    ap.add_argument("--step", help="run one step in this process and print its JSON line")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("surface_aniso_bench: no GPU")
        out = step_loop(args) if args.step == "loop" else step_kernels(args, args.step.split("-", 1)[1])
        print("RESULT " + json.dumps(out), flush=True)
        return 0
    res = dict(reps=args.reps, warmup=args.warmup)
    passed = ["--reps", str(args.reps), "--warmup", str(args.warmup), "--frames", str(args.frames), "--loop-warmup", str(args.loop_warmup),
              "--rounds", str(args.rounds), "--reference-spp", str(args.reference_spp)]
    for step, seconds in STEPS:  # one attempt each; the first failure ends the tool
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step] + passed,
                           stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"surface_aniso_bench: step {step} ended with status {p.returncode}", file=sys.stderr)
            return p.returncode
        res[step] = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Anisotropic footprint-filtered albedo (`pt_surface_aniso_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
