#!/usr/bin/env python3
"""surface_bench.py — what the pixel-centre albedo pass costs (pt_surface_planes, k_surface) and what the demodulating adaptive loop costs
end to end.

1920 x 1080, one MI355X.  Three steps, each a process of its own under `timeout`; the first step that fails ends the tool with its status
(nothing is tried twice):
  kernels textured    textured_terrain (1 M triangles, six 1024 x 1024 band textures): k_surface<true> on renderGBuffer's hit plane, both
                      planes asked for, beside k_motion (all three planes) on the same hit plane — the closest existing kernel in shape;
  kernels untextured  voxel_terrain (1 M triangles, no texture): k_surface<false> beside k_motion;
  loops               textured_terrain, an orbit of --frames frames at 1 spp, the two loops taking turns --rounds times:
                      (a) examples/adaptive_svgf_loop.py (no albedo), (b) examples/adaptive_svgf_albedo_loop.py (surfacePlanes, demodulation,
                      modulatePlanes); host time around the whole frame.
Kernel times are the calls' own kernel_ms (hipEvents around the launch), medians over --reps calls after --warmup.  Bytes are counted from
the shapes: per pixel 16 B of hit, on a hit 4 B of mesh, on the colour path 12 B of colour, on the texture path 4 B of texture id, 24 B of
texcoords and 16 B of texels, and 16 + 8 B written.  The yardstick is k_motion in the same process; no threshold is attached to any figure.
Prints one JSON object; --md PATH also writes the tables as markdown with the raw JSON below them, replacing that file's part from
"## Timings" on.
  python3 tools/surface_bench.py [--reps 50] [--warmup 10] [--frames 24] [--rounds 2] [--md profiles/surface.md]
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
STEPS = (("kernels", "textured", 300), ("kernels", "untextured", 300), ("loops", "textured", 420))  # (step, scene, seconds allowed)


def orbit(cam, angle):
    e, l = np.asarray(cam["eye"], np.float64), np.asarray(cam["lookat"], np.float64)
    d = e - l
    c, s = np.cos(angle), np.sin(angle)
    return dict(cam, eye=(float(l[0] + c * d[0] + s * d[2]), float(e[1]), float(l[2] - s * d[0] + c * d[2])))


def _renderer(scene):
    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    model = scenes.textured_terrain() if scene == "textured" else scenes.voxel_terrain()
    r = R.SampleRenderer(model)
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.TERRAIN_CAMERA, W / H))
    return r, model


def step_kernels(scene, args):
    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    r, model = _renderer(scene)
    hit = r.renderGBuffer(("hit",))["hit"]
    table, verts = r.copyTexcoordsDevice(), r.copyVerticesDevice()
    row = R._camera_rows([R.make_camera(scenes.TERRAIN_CAMERA, W / H)])[0]
    s_out = {k: v for k, v in r.surfacePlanes(hit, table, planes=("albedo", "texcoord")).items() if k != "stats"}
    m_out = {k: v for k, v in r.motionPlanes(hit, verts, prev_cameras=row).items() if k != "stats"}
    surface, motion, st = [], [], None
    for k in range(args.warmup + args.reps):  # the two kernels take turns
        st = r.surfacePlanes(hit, table, planes=("albedo", "texcoord"), out=s_out)["stats"]
        mt = r.motionPlanes(hit, verts, prev_cameras=row, out=m_out)["stats"]
        if k >= args.warmup:
            surface.append(st["kernel_ms"])
            motion.append(mt["kernel_ms"])
    r.close()
    px, hits, tex = st["pixels"], st["hits"], st["textured"]
    read = 16 * px + 4 * hits + 12 * (hits - tex) + (4 + 24 + 16) * tex
    return dict(scene=scene, triangles=model.num_triangles, pixels=px, hits=hits, textured=tex, bytes_read=read, bytes_written=24 * px,
                surface_ms=float(np.median(surface)), surface_min_ms=float(min(surface)), motion_ms=float(np.median(motion)), motion_min_ms=float(min(motion)))


def step_loops(scene, args):
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    r, model = _renderer(scene)
    r.launchParams.samples_per_launch = 1
    dev = "cuda:0"

    def planes(k):
        return torch.zeros((H, W, k) if k > 1 else (H, W), device=dev)

    gbuf = [dict(hit=planes(8), position=planes(4), motion=planes(2)) for _ in range(2)]
    history, moments, length = [planes(4) for _ in range(2)], [planes(2) for _ in range(2)], [planes(1) for _ in range(2)]
    variance, filtered, scratch, albedo, final = planes(1), planes(4), planes(4), planes(4), planes(4)
    accum = r.deviceBuffer(R.PT_BUF_ACCUM)
    table = r.copyTexcoordsDevice()
    plan = dict(threshold=0.25, dark_floor=0.05, min_length=4, min_pixels=8, refresh_period=16)

    def loop(with_albedo):
        r.uploadAccum(np.zeros((H, W, 4), np.float32))
        for t in list(gbuf[0].values()) + list(gbuf[1].values()) + history + moments + length:
            t.zero_()
        rows = []
        cam = R.make_camera(scenes.TERRAIN_CAMERA, W / H)
        for k in range(args.frames):
            prev, cam = cam, R.make_camera(orbit(scenes.TERRAIN_CAMERA, 0.01 * k), W / H)
            cur, old, i, o = gbuf[k & 1], gbuf[~k & 1], k & 1, ~k & 1
            t0 = time.perf_counter()
            r.setCamera(cam)
            r.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev, out=cur)
            alb = None
            surface_ms = 0.0
            if with_albedo:
                surface_ms = r.surfacePlanes(cur["hit"], table, out=dict(albedo=albedo))["stats"]["kernel_ms"]
                alb = albedo
            geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], history[i], moments[i], length[i])
            outs = dict(history_out=history[o], moments_out=moments[o], length_out=length[o], variance_out=variance)
            p = r.samplePlan(*geo, frame_index=k, **plan)
            r.launchParams.frame.subframe_index = k
            r.renderMask(p["mask"])
            r.temporalMoments(accum, *geo, albedo=alb, **outs, mask=p["mask"], color_scale=float(k + 1), clear_color=True)
            r.temporalCarry(*geo, **outs, mask=p["mask"] == 0)
            r.filterPlanes(history[o], cur["hit"], cur["position"], variance=variance, length=length[o], out=filtered, scratch=scratch)
            if with_albedo:
                r.modulatePlanes(filtered, albedo=albedo, out=final)
            rows.append(dict(frame_ms=(time.perf_counter() - t0) * 1e3, surface_ms=surface_ms, share=p["stats"]["sampled"] / p["stats"]["blocks"]))
        return rows[args.loop_warmup:]

    runs = {False: [], True: []}
    for _ in range(args.rounds):
        for with_albedo in (False, True):
            runs[with_albedo] += loop(with_albedo)
    r.close()

    def summary(rows):
        return dict(frame_ms=float(np.median([x["frame_ms"] for x in rows])), surface_ms=float(np.median([x["surface_ms"] for x in rows])),
                    sampled_share=float(np.median([x["share"] for x in rows])))

    return dict(scene=scene, triangles=model.num_triangles, frames=args.frames, warmup=args.loop_warmup, rounds=args.rounds, plan_params=plan,
                without_albedo=summary(runs[False]), with_albedo=summary(runs[True]))


def markdown(res):
    md = ["## Timings (`tools/surface_bench.py`)\n",
          f"{W} x {H}, one MI355X; kernel times are the calls' own `kernel_ms`, medians (minima in brackets) over {res['reps']} calls after "
          f"{res['warmup']} warm-up calls, `k_surface` and `k_motion` taking turns on the same hit plane in one process.  Bytes are counted from "
          "the shapes (the tool's docstring).  No threshold is attached to any of these figures.\n",
          "| scene | triangles | hits | textured | `k_surface` ms | `k_motion` ms | ratio | bytes read + written | GB/s |", "|---|---|---|---|---|---|---|---|---|"]
    for k in res["kernels"]:
        b = k["bytes_read"] + k["bytes_written"]
        md.append(f"| {k['scene']} | {k['triangles']} | {k['hits']} | {k['textured']} | {k['surface_ms']:.4f} ({k['surface_min_ms']:.4f}) | "
                  f"{k['motion_ms']:.4f} ({k['motion_min_ms']:.4f}) | {k['surface_ms'] / k['motion_ms']:.2f} | {b} | {b / k['surface_ms'] / 1e6:.0f} |")
    lp = res["loops"]
    a, b = lp["without_albedo"], lp["with_albedo"]
    md += ["",
           f"The adaptive loop end to end on `textured_terrain`, an orbit of {lp['frames']} frames at 1 spp, the two loops taking turns {lp['rounds']} "
           f"times, medians of the host time around a whole frame after {lp['warmup']} warm-up frames: `examples/adaptive_svgf_loop.py` (no albedo) "
           f"{a['frame_ms']:.3f} ms per frame (share of blocks sampled {a['sampled_share']:.3f}); `examples/adaptive_svgf_albedo_loop.py` "
           f"{b['frame_ms']:.3f} ms (share {b['sampled_share']:.3f}), of which `k_surface` {b['surface_ms']:.4f} ms.",
           "", "## Raw output\n", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--loop-warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--md", help="also write the tables as markdown to this path")
    ap.add_argument("--step", nargs=2, metavar=("STEP", "SCENE"), help="run one step in this process and print its JSON line")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("surface_bench: no GPU")
        fn = dict(kernels=step_kernels, loops=step_loops)[args.step[0]]
        print("RESULT " + json.dumps(fn(args.step[1], args)), flush=True)
        return 0
    res = dict(reps=args.reps, warmup=args.warmup, kernels=[])
    passed = ["--reps", str(args.reps), "--warmup", str(args.warmup), "--frames", str(args.frames), "--loop-warmup", str(args.loop_warmup),
              "--rounds", str(args.rounds)]
    for step, scene, seconds in STEPS:  # one attempt each; the first failure ends the tool
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step, scene] + passed,
                           stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"surface_bench: step {step} {scene} ended with status {p.returncode}", file=sys.stderr)
            return p.returncode
        out = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
        if step == "kernels":
            res["kernels"].append(out)
        else:
            res["loops"] = out
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Pixel-centre albedo from the hit plane (`pt_surface_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part (the register table) stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
