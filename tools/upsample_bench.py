#!/usr/bin/env python3
"""upsample_bench.py — what guided upsampling costs (pt_upsample_planes, k_upsample), which branches its pixels take, and what the loop
that traces at a fraction of the display resolution gains and loses end to end.

1920 x 1080, one MI355X, `textured_terrain` (1 M triangles) and the textured scene.  The steps, each a process of its own under `timeout`;
the first step that ends abnormally ends the tool with its status (nothing is tried twice):
  kernels-<scene>  k_upsample at scale 2, 3 and 4 on the G-buffers of two contexts over one model, the low-resolution colour being the
                   low-resolution albedo: `kernel_ms` and the host time around the Python call, medians over --reps calls after --warmup;
                   the counter shares at each scale;
  loops-<scene>    an orbit of --frames frames at 1 spp: examples/upsampled_svgf_loop.py at scale 2 against
                   examples/adaptive_svgf_albedo_loop.py --lod at the same size, taking turns --rounds times, host time around a whole
                   frame; then the rms of each loop's final frame against a converged full-resolution frame (--reference-spp samples,
                   PT_BUF_COLOR of a standing camera at the orbit's last position);
  bench            with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1 --steps 20 --warmup 3` in this tree and in
                   that one, taking turns three times, to show that the frame path did not move.
No threshold is attached to any figure.  Prints one JSON object; --md PATH also writes the tables as markdown with the raw JSON below
them, replacing that file's part from "## Timings" on.
  python3 tools/upsample_bench.py [--reps 50] [--warmup 10] [--frames 24] [--rounds 2] [--parent DIR] [--md profiles/upsample.md]
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
SCALES = (2, 3, 4)
SCENE_NAMES = ("terrain", "textured")
STEPS = [(f"kernels-{n}", 300) for n in SCENE_NAMES] + [(f"loops-{n}", 420) for n in SCENE_NAMES]  # (step, seconds allowed)
BENCH_SECONDS = 300


def _example():
    spec = importlib.util.spec_from_file_location("upsampled_svgf_loop", os.path.join(ROOT, "examples", "upsampled_svgf_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _renderer(model, size, cam0, probe=None):
    from optixpathtracer_amd import renderer as R

    r = R.SampleRenderer(model)
    if probe is not None:
        r.setProbe(probe)
    r.resize(size)
    r.setCamera(R.make_camera(cam0, size[0] / size[1]))
    return r


def step_kernels(args, scene):
    make, cam0 = _example().SCENES[scene]
    model = make()
    hi = _renderer(model, (W, H), cam0)
    g = hi.renderGBuffer(("hit", "position"))
    import torch

    out = dict(out=torch.zeros((H, W, 4), device="cuda:0"), weight_out=torch.zeros((H, W), device="cuda:0"))
    rows = {}
    for s in SCALES:
        lo = _renderer(model, (W // s, H // s), cam0)
        lg = lo.renderGBuffer(("hit", "position"))
        colour = lo.surfacePlanes(lg["hit"], lo.copyTexcoordsDevice())["albedo"]
        lo.close()
        ms, host, st = [], [], None
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            st = hi.upsamplePlanes(colour, lg["hit"], lg["position"], g["hit"], g["position"], s, **out)["stats"]
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                ms.append(st["kernel_ms"])
                host.append(dt * 1e3)
        rows[str(s)] = dict(kernel_ms=float(np.median(ms)), kernel_min_ms=float(min(ms)), host_ms=float(np.median(host)), pixels=st["pixels"], hits=st["hits"],
                            full=st["full"], rescued=st["rescued"], orphans=st["orphans"])
    hi.close()
    return dict(triangles=model.num_triangles, scales=rows)


def step_loops(args, scene):
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    ex = _example()
    make, cam0 = ex.SCENES[scene]
    model = make()
    probe = scenes.sky_probe(1024, 512).BuildCDF()
    up = ex.UpsampledLoop(model, (W, H), 2, lod=True, probe=probe)
    # the loop of examples/adaptive_svgf_albedo_loop.py --lod at the display size
    r = _renderer(model, (W, H), cam0, probe)
    r.launchParams.samples_per_launch = 1
    dev = "cuda:0"

    def planes(k):
        return torch.zeros((H, W, k) if k > 1 else (H, W), device=dev)

    gbuf = [dict(hit=planes(8), position=planes(4), motion=planes(2)) for _ in range(2)]
    history, moments, length = [planes(4) for _ in range(2)], [planes(2) for _ in range(2)], [planes(1) for _ in range(2)]
    variance, filtered, scratch, albedo, final = planes(1), planes(4), planes(4), planes(4), planes(4)
    accum = r.deviceBuffer(R.PT_BUF_ACCUM)
    table, mips = r.copyTexcoordsDevice(), r.copyTextureMipsDevice()
    cams = [R.make_camera(ex.orbit(cam0, 0.01 * k), W / H) for k in range(args.frames)]

    def full_frame(k, prev, cam):
        cur, old, i, o = gbuf[k & 1], gbuf[~k & 1], k & 1, ~k & 1
        t0 = time.perf_counter()
        r.setCamera(cam)
        r.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev, out=cur)
        r.surfaceLodPlanes(cur["hit"], table, mips, out=dict(albedo=albedo))
        geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], history[i], moments[i], length[i])
        outs = dict(history_out=history[o], moments_out=moments[o], length_out=length[o], variance_out=variance)
        p = r.samplePlan(*geo, frame_index=k, **ex.PLAN)
        r.launchParams.frame.subframe_index = k
        r.renderMask(p["mask"])
        r.temporalMoments(accum, *geo, albedo=albedo, **outs, mask=p["mask"], color_scale=float(k + 1), clear_color=True)
        r.temporalCarry(*geo, **outs, mask=p["mask"] == 0)
        r.filterPlanes(history[o], cur["hit"], cur["position"], variance=variance, length=length[o], out=filtered, scratch=scratch)
        r.modulatePlanes(filtered, albedo=albedo, out=final)
        return dict(frame_ms=(time.perf_counter() - t0) * 1e3, share=p["stats"]["sampled"] / p["stats"]["blocks"], colour_ms=r.stats()["render_ms"])

    def run(which):
        if which == "native":
            r.uploadAccum(np.zeros((H, W, 4), np.float32))
            state = list(gbuf[0].values()) + list(gbuf[1].values()) + history + moments + length
        else:
            up.lo.uploadAccum(np.zeros((H // 2, W // 2, 4), np.float32))
            state = list(up.gbuf[0].values()) + list(up.gbuf[1].values()) + up.history + up.moments + up.length
        for t in state:
            t.zero_()
        rows, cam = [], R.make_camera(cam0, W / H)
        for k in range(args.frames):
            prev, cam = cam, cams[k]
            rows.append(full_frame(k, prev, cam) if which == "native" else up.frame(k, prev, cam))
        return rows[args.loop_warmup:]

    runs = {"native": [], "upsampled": []}
    for _ in range(args.rounds):
        for which in ("native", "upsampled"):
            runs[which] += run(which)
    images = dict(native=final.cpu().numpy()[..., :3].astype(np.float64), upsampled=up.final.cpu().numpy()[..., :3].astype(np.float64))
    counters = runs["upsampled"][-1]
    # the converged frame: a standing camera at the orbit's last position, --reference-spp samples in subframes of 32
    r.setCamera(cams[-1])
    r.uploadAccum(np.zeros((H, W, 4), np.float32))
    r.launchParams.samples_per_launch = 32
    for k in range(max(1, args.reference_spp // 32)):
        r.launchParams.frame.subframe_index = k
        r.render()
    r.sync()
    reference = r.download(R.PT_BUF_COLOR)[..., :3].astype(np.float64)
    rms = {k: float(np.sqrt(((v - reference) ** 2).mean())) for k, v in images.items()}
    r.close()
    up.close()
    med = lambda rows, key: float(np.median([x[key] for x in rows]))  # noqa: E731
    return dict(triangles=model.num_triangles, frames=args.frames, warmup=args.loop_warmup, rounds=args.rounds, reference_spp=32 * max(1, args.reference_spp // 32),
                native=dict(frame_ms=med(runs["native"], "frame_ms"), sampled_share=med(runs["native"], "share"), colour_ms=med(runs["native"], "colour_ms"), rms=rms["native"]),
                upsampled=dict(frame_ms=med(runs["upsampled"], "frame_ms"), lo_ms=med(runs["upsampled"], "lo_ms"), hi_ms=med(runs["upsampled"], "hi_ms"),
                               sampled_share=float(np.median([x["sampled"] / x["blocks"] for x in runs["upsampled"]])), colour_ms=med(runs["upsampled"], "colour_ms"),
                               gbuffer_ms=med(runs["upsampled"], "gbuffer_ms"), surface_ms=med(runs["upsampled"], "surface_ms"),
                               upsample_ms=med(runs["upsampled"], "upsample_ms"), modulate_ms=med(runs["upsampled"], "modulate_ms"),
                               pixels=counters["pixels"], full=counters["full"], rescued=counters["rescued"], orphans=counters["orphans"], rms=rms["upsampled"]))


def bench_turns(parent):
    """bench.py in this tree and in the parent's, taking turns three times; every run a process of its own under its time limit"""
    rows = []
    for turn in range(3):
        for name, tree in (("this", ROOT), ("parent", os.path.abspath(parent))):
            p = subprocess.run(["timeout", "-k", "10", str(BENCH_SECONDS), sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=tree,
                               stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                print(f"upsample_bench: bench.py in the {name} tree ended with status {p.returncode}", file=sys.stderr)
                return p.returncode, rows
            line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            rows.append(dict(tree=name, turn=turn, ms_per_step=line["ms_per_step"], mrays_per_s=line["value"]))
    return 0, rows


def markdown(res):
    md = ["## Timings (`tools/upsample_bench.py`)\n",
          f"{W} x {H}, one MI355X; kernel times are the calls' own `kernel_ms` (hipEvents around the launch), medians (minima in brackets) over "
          f"{res['reps']} calls after {res['warmup']} warm-up calls; the host time is the Python call's (`upsamplePlanes`): the drain, the pointer "
          "checks, the temporaries, the launch and the final wait.  The low-resolution colour is the low-resolution albedo.  Bytes: the pass's "
          "algorithmic traffic, 64 per full-res pixel (32 of pt_hit and 16 of position read for a hit, 16 of `out` written, 4 more with "
          "`weight_out`) plus 64 / s^2 for the three low-res planes read once, and the bandwidth that makes of `kernel_ms`.  No threshold is "
          "attached to any of these figures.\n"]
    for scene in SCENE_NAMES:
        k = res[f"kernels-{scene}"]
        md += [f"`{scene}` ({k['triangles']} triangles):\n", "| scale | `kernel_ms` | host ms around the call | bytes per pixel | GB/s | full | partial | rescued | orphans |",
               "|---|---|---|---|---|---|---|---|---|"]
        for s in SCALES:
            x = k["scales"][str(s)]
            n = x["pixels"]
            bpp = 68 + 64 / (s * s)
            part = n - x["full"] - x["rescued"] - x["orphans"]
            md.append(f"| {s} | {x['kernel_ms']:.4f} ({x['kernel_min_ms']:.4f}) | {x['host_ms']:.4f} | {bpp:.1f} | {bpp * n / x['kernel_ms'] / 1e6:.0f} | "
                      f"{x['full'] / n:.4f} | {part / n:.4f} | {x['rescued'] / n:.5f} | {x['orphans'] / n:.5f} |")
        md.append("")
    md.append("The loops end to end: `examples/upsampled_svgf_loop.py --scale 2 --lod` against `examples/adaptive_svgf_albedo_loop.py --lod` at the same "
              "size, the same orbit at 1 spp, taking turns; medians of the host time around a whole frame; rms of the final frame's three colour words "
              "against a converged full-resolution frame (`PT_BUF_COLOR` of a standing camera at the orbit's last position).\n")
    md += ["| scene | loop | ms per frame | of which colour (path tracer) | blocks sampled | rms against the converged frame |", "|---|---|---|---|---|---|"]
    for scene in SCENE_NAMES:
        lp = res[f"loops-{scene}"]
        f, u = lp["native"], lp["upsampled"]
        md.append(f"| `{scene}` | full resolution | {f['frame_ms']:.3f} | {f['colour_ms']:.3f} | {f['sampled_share']:.3f} | {f['rms']:.5f} |")
        md.append(f"| `{scene}` | traced at 1/2, upsampled | {u['frame_ms']:.3f} (low-res part {u['lo_ms']:.3f}, full-res part {u['hi_ms']:.3f}: G-buffer "
                  f"{u['gbuffer_ms']:.3f}, surface {u['surface_ms']:.3f}, upsample {u['upsample_ms']:.3f}, modulate {u['modulate_ms']:.3f}) | {u['colour_ms']:.3f} | "
                  f"{u['sampled_share']:.3f} | {u['rms']:.5f} |")
    lp = res[f"loops-{SCENE_NAMES[0]}"]
    md += ["", f"{lp['frames']} frames, {lp['warmup']} warm-up frames left out, {lp['rounds']} rounds; the converged frame has {lp['reference_spp']} spp.  In the last "
           "frame of the upsampled loop: " + "; ".join(f"`{s}` full {res[f'loops-{s}']['upsampled']['full']}, rescued {res[f'loops-{s}']['upsampled']['rescued']}, "
                                                      f"orphans {res[f'loops-{s}']['upsampled']['orphans']} of {res[f'loops-{s}']['upsampled']['pixels']}" for s in SCENE_NAMES) + ".", ""]
    if res.get("bench"):
        md += ["`bench.py --gpus 1 --steps 20 --warmup 3` in this tree and in the parent commit's, taking turns:\n", "| turn | this tree, ms per step | parent, ms per step |", "|---|---|---|"]
        for turn in range(3):
            a = [x for x in res["bench"] if x["turn"] == turn]
            md.append(f"| {turn} | " + " | ".join(f"{x['ms_per_step']:.3f} ({x['mrays_per_s']:.1f} Mrays/s)" for x in sorted(a, key=lambda x: x["tree"] != "this")) + " |")
        md.append("")
    else:
        md += ["The `bench.py` comparison against the parent commit was not run (no `--parent`).", ""]
    md += ["## Raw output\n", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--loop-warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reference-spp", type=int, default=256)
    ap.add_argument("--parent", help="a built checkout of the parent commit: bench.py runs there and here, taking turns")
    ap.add_argument("--md", help="also write the tables as markdown to this path")
    ap.add_argument("--step", help="run one step in this process and print its JSON line")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("upsample_bench: no GPU")
        kind, scene = args.step.split("-")
        fn = dict(kernels=step_kernels, loops=step_loops)[kind]
        print("RESULT " + json.dumps(fn(args, scene)), flush=True)
        return 0
    res = dict(reps=args.reps, warmup=args.warmup)
    passed = ["--reps", str(args.reps), "--warmup", str(args.warmup), "--frames", str(args.frames), "--loop-warmup", str(args.loop_warmup),
              "--rounds", str(args.rounds), "--reference-spp", str(args.reference_spp)]
    for step, seconds in STEPS:  # one attempt each; the first failure ends the tool
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step] + passed,
                           stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"upsample_bench: step {step} ended with status {p.returncode}", file=sys.stderr)
            return p.returncode
        res[step] = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
        print(f"upsample_bench: step {step} done", file=sys.stderr, flush=True)
    if args.parent:
        rc, res["bench"] = bench_turns(args.parent)
        if rc:
            return rc
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Guided upsampling (`pt_upsample_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
