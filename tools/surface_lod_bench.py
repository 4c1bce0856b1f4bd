#!/usr/bin/env python3
"""surface_lod_bench.py — what the footprint-filtered albedo pass costs (pt_surface_lod_planes, k_surface_lod) beside the point lookup
(pt_surface_planes, k_surface), what it costs the demodulating adaptive loop end to end, and what it does to the albedo plane's shimmer.

1920 x 1080, textured_terrain (1 M triangles, 1024 x 1024 band textures), one MI355X.  Three steps, each a process of its own under
`timeout`; the first step that fails ends the tool with its status (nothing is tried twice):
  kernels  k_surface (albedo and texcoord) and k_surface_lod (albedo and texcoord; all four planes) taking turns on ONE hit plane; the
           pyramid's build (pt_copy_texture_mips_device, host time around the call, one launch per level);
  shimmer  two cameras a quarter of a pixel apart (the view turned about the vertical axis by a quarter of the centre pixel's angle): the
           mean |difference| of the two albedo planes, per channel, on pixels whose hit is on the same mesh under both cameras — with the
           point lookup and with the filtered one.  A figure, not asserted anywhere;
  loops    an orbit of --frames frames at 1 spp, examples/adaptive_svgf_albedo_loop.py without and with --lod taking turns --rounds times;
           host time around the whole frame.
Kernel times are the calls' own kernel_ms (hipEvents around the launch), medians over --reps calls after --warmup; next to them the host
time around the whole Python call, which also holds what the pass does in front of its timed span.  No threshold is attached
to any figure.  Prints one JSON object; --md PATH also writes the tables as markdown with the raw JSON below them, replacing that file's
part from "## Timings" on.
  python3 tools/surface_lod_bench.py [--reps 50] [--warmup 10] [--frames 24] [--rounds 2] [--md profiles/surface_lod.md]
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
STEPS = (("kernels", 300), ("shimmer", 300), ("loops", 420))  # (step, seconds allowed)


def orbit(cam, angle):
    e, l = np.asarray(cam["eye"], np.float64), np.asarray(cam["lookat"], np.float64)
    d = e - l
    c, s = np.cos(angle), np.sin(angle)
    return dict(cam, eye=(float(l[0] + c * d[0] + s * d[2]), float(e[1]), float(l[2] - s * d[0] + c * d[2])))


def turned(cam, angle):
    """the camera turned in place by `angle` radians about the vertical axis through its eye"""
    e, l = np.asarray(cam["eye"], np.float64), np.asarray(cam["lookat"], np.float64)
    d = l - e
    c, s = np.cos(angle), np.sin(angle)
    return dict(cam, lookat=(float(e[0] + c * d[0] + s * d[2]), float(l[1]), float(e[2] - s * d[0] + c * d[2])))


def _renderer():
    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    model = scenes.textured_terrain()
    r = R.SampleRenderer(model)
    r.setProbe(scenes.sky_probe(256, 128).BuildCDF())
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.TERRAIN_CAMERA, W / H))
    return r, model


def step_kernels(args):
    r, model = _renderer()
    hit = r.renderGBuffer(("hit",))["hit"]
    table = r.copyTexcoordsDevice()
    dims, nbytes = r.textureMipsLayout()
    mips = r.copyTextureMipsDevice()
    build = []
    for _ in range(5):
        t0 = time.perf_counter()
        r.copyTextureMipsDevice(out=mips)
        build.append((time.perf_counter() - t0) * 1e3)
    two, four = ("albedo", "texcoord"), ("albedo", "texcoord", "footprint", "lod")
    outs = [{k: v for k, v in r.surfacePlanes(hit, table, planes=two).items() if k != "stats"},
            {k: v for k, v in r.surfaceLodPlanes(hit, table, mips, planes=two).items() if k != "stats"},
            {k: v for k, v in r.surfaceLodPlanes(hit, table, mips, planes=four).items() if k != "stats"}]
    ms, host, st = [[], [], []], [[], [], []], None
    for k in range(args.warmup + args.reps):  # the kernels take turns
        t0 = time.perf_counter()
        a = r.surfacePlanes(hit, table, planes=two, out=outs[0])["stats"]
        t1 = time.perf_counter()
        b = r.surfaceLodPlanes(hit, table, mips, planes=two, out=outs[1])["stats"]
        t2 = time.perf_counter()
        st = r.surfaceLodPlanes(hit, table, mips, planes=four, out=outs[2])["stats"]
        t3 = time.perf_counter()
        if k >= args.warmup:
            for row, hrow, s, dt in zip(ms, host, (a, b, st), (t1 - t0, t2 - t1, t3 - t2)):
                row.append(s["kernel_ms"])
                hrow.append(dt * 1e3)
    lod = outs[2]["lod"].cpu().numpy()
    r.close()
    med = lambda v: float(np.median(v))  # noqa: E731
    return dict(triangles=model.num_triangles, textures=dims.tolist(), mips_bytes=nbytes, mips_build_ms=med(build), pixels=st["pixels"], hits=st["hits"],
                textured=st["textured"], minified=st["minified"], lod_mean=float(lod[lod > 0].mean()) if (lod > 0).any() else 0.0, lod_max=float(lod.max()),
                surface_ms=med(ms[0]), surface_min_ms=float(min(ms[0])), lod2_ms=med(ms[1]), lod2_min_ms=float(min(ms[1])),
                lod4_ms=med(ms[2]), lod4_min_ms=float(min(ms[2])), surface_host_ms=med(host[0]), lod2_host_ms=med(host[1]), lod4_host_ms=med(host[2]))


def step_shimmer(args):
    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    r, model = _renderer()
    table, mips = r.copyTexcoordsDevice(), r.copyTextureMipsDevice()
    cam0 = scenes.TERRAIN_CAMERA
    pixel = 2.0 * np.tan(np.radians(cam0["fovY"]) / 2) / H  # the centre pixel's angle
    planes = []
    for cam in (cam0, turned(cam0, 0.25 * pixel)):
        r.setCamera(R.make_camera(cam, W / H))
        hit = r.renderGBuffer(("hit",))["hit"]
        mesh = hit.cpu().numpy().view(np.int32)[..., 4].copy()
        point = r.surfacePlanes(hit, table)["albedo"].cpu().numpy()[..., :3]
        lod = r.surfaceLodPlanes(hit, table, mips)["albedo"].cpu().numpy()[..., :3]
        planes.append((mesh, point, lod))
    r.close()
    (m0, p0, l0), (m1, p1, l1) = planes
    same = (m0 == m1) & (m0 >= 0)
    return dict(step_px=0.25, pixels=int(same.sum()), point=float(np.abs(p1 - p0)[same].mean()), lod=float(np.abs(l1 - l0)[same].mean()))


def step_loops(args):
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    r, model = _renderer()
    r.launchParams.samples_per_launch = 1
    dev = "cuda:0"

    def planes(k):
        return torch.zeros((H, W, k) if k > 1 else (H, W), device=dev)

    gbuf = [dict(hit=planes(8), position=planes(4), motion=planes(2)) for _ in range(2)]
    history, moments, length = [planes(4) for _ in range(2)], [planes(2) for _ in range(2)], [planes(1) for _ in range(2)]
    variance, filtered, scratch, albedo, final = planes(1), planes(4), planes(4), planes(4), planes(4)
    accum = r.deviceBuffer(R.PT_BUF_ACCUM)
    table, mips = r.copyTexcoordsDevice(), r.copyTextureMipsDevice()
    plan = dict(threshold=0.25, dark_floor=0.05, min_length=4, min_pixels=8, refresh_period=16)

    def loop(with_lod):
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
            if with_lod:
                surface_ms = r.surfaceLodPlanes(cur["hit"], table, mips, out=dict(albedo=albedo))["stats"]["kernel_ms"]
            else:
                surface_ms = r.surfacePlanes(cur["hit"], table, out=dict(albedo=albedo))["stats"]["kernel_ms"]
            geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], history[i], moments[i], length[i])
            outs = dict(history_out=history[o], moments_out=moments[o], length_out=length[o], variance_out=variance)
            p = r.samplePlan(*geo, frame_index=k, **plan)
            r.launchParams.frame.subframe_index = k
            r.renderMask(p["mask"])
            r.temporalMoments(accum, *geo, albedo=albedo, **outs, mask=p["mask"], color_scale=float(k + 1), clear_color=True)
            r.temporalCarry(*geo, **outs, mask=p["mask"] == 0)
            r.filterPlanes(history[o], cur["hit"], cur["position"], variance=variance, length=length[o], out=filtered, scratch=scratch)
            r.modulatePlanes(filtered, albedo=albedo, out=final)
            rows.append(dict(frame_ms=(time.perf_counter() - t0) * 1e3, surface_ms=surface_ms, share=p["stats"]["sampled"] / p["stats"]["blocks"]))
        return rows[args.loop_warmup:]

    runs = {False: [], True: []}
    for _ in range(args.rounds):
        for with_lod in (False, True):
            runs[with_lod] += loop(with_lod)
    r.close()

    def summary(rows):
        return dict(frame_ms=float(np.median([x["frame_ms"] for x in rows])), surface_ms=float(np.median([x["surface_ms"] for x in rows])),
                    sampled_share=float(np.median([x["share"] for x in rows])))

    return dict(triangles=model.num_triangles, frames=args.frames, warmup=args.loop_warmup, rounds=args.rounds, plan_params=plan,
                point=summary(runs[False]), lod=summary(runs[True]))


def markdown(res):
    k, s, lp = res["kernels"], res["shimmer"], res["loops"]
    md = ["## Timings (`tools/surface_lod_bench.py`)\n",
          f"{W} x {H}, `textured_terrain` ({k['triangles']} triangles), one MI355X; kernel times are the calls' own `kernel_ms`, medians (minima in "
          f"brackets) over {res['reps']} calls after {res['warmup']} warm-up calls, the kernels taking turns on the same hit plane in one process: "
          f"{k['hits']} hits, {k['textured']} textured, {k['minified']} minified (mean lod of those {k['lod_mean']:.2f}, largest {k['lod_max']:.2f}).  "
          "No threshold is attached to any of these figures.\n",
          "| kernel | planes | `kernel_ms` | host ms around the call |", "|---|---|---|---|",
          f"| `k_surface<true>` | albedo, texcoord | {k['surface_ms']:.4f} ({k['surface_min_ms']:.4f}) | {k['surface_host_ms']:.4f} |",
          f"| `k_surface_lod<false, true>` | albedo, texcoord | {k['lod2_ms']:.4f} ({k['lod2_min_ms']:.4f}) | {k['lod2_host_ms']:.4f} |",
          f"| `k_surface_lod<false, true>` | albedo, texcoord, footprint, lod | {k['lod4_ms']:.4f} ({k['lod4_min_ms']:.4f}) | {k['lod4_host_ms']:.4f} |",
          "",
          "The host time is the Python call's (`surfacePlanes` / `surfaceLodPlanes`): the drain, the pointer checks, the temporaries, the launch "
          "and the final wait; for the LOD pass also the readback of the texture sizes and the upload of the level table, which `kernel_ms` leaves out.",
          "",
          f"The pyramid: {k['mips_bytes']} bytes for {len(k['textures'])} textures, built in {k['mips_build_ms']:.3f} ms (host time around "
          "`pt_copy_texture_mips_device`, one launch per level, the drain and the final wait included); once per scene.",
          "",
          f"Shimmer: across a camera step of {s['step_px']} px (the view turned about the vertical axis), the mean |difference| of the two albedo planes "
          f"per channel over the {s['pixels']} pixels whose hit stays on one mesh: {s['point']:.5f} with the point lookup, {s['lod']:.5f} with the "
          f"filtered one (ratio {s['lod'] / s['point']:.3f}).",
          "",
          f"The adaptive loop end to end (`examples/adaptive_svgf_albedo_loop.py`), an orbit of {lp['frames']} frames at 1 spp, without and with `--lod` "
          f"taking turns {lp['rounds']} times, medians of the host time around a whole frame after {lp['warmup']} warm-up frames: "
          f"{lp['point']['frame_ms']:.3f} ms per frame with `surfacePlanes` (of which `k_surface` {lp['point']['surface_ms']:.4f} ms, share of blocks "
          f"sampled {lp['point']['sampled_share']:.3f}); {lp['lod']['frame_ms']:.3f} ms with `surfaceLodPlanes` (of which `k_surface_lod` "
          f"{lp['lod']['surface_ms']:.4f} ms, share {lp['lod']['sampled_share']:.3f}).",
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
    ap.add_argument("--step", help="run one step in this process and print its JSON line")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("surface_lod_bench: no GPU")
        fn = dict(kernels=step_kernels, shimmer=step_shimmer, loops=step_loops)[args.step]
        print("RESULT " + json.dumps(fn(args)), flush=True)
        return 0
    res = dict(reps=args.reps, warmup=args.warmup)
    passed = ["--reps", str(args.reps), "--warmup", str(args.warmup), "--frames", str(args.frames), "--loop-warmup", str(args.loop_warmup),
              "--rounds", str(args.rounds)]
    for step, seconds in STEPS:  # one attempt each; the first failure ends the tool
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step] + passed,
                           stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"surface_lod_bench: step {step} ended with status {p.returncode}", file=sys.stderr)
            return p.returncode
        res[step] = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Footprint-filtered albedo (`pt_surface_lod_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
