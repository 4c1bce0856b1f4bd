#!/usr/bin/env python3
"""adaptive_bench.py — what rendering a subset of the 8x8 blocks costs and saves (pt_render_mask, pt_render_adaptive) on the C3 workload
(1 M-triangle terrain, 1920x1080, 4 spp, depth 8).  Printed as ONE JSON object:

  masks     plain pt_render and pt_render_mask with all blocks, a random 25 %, a random 5 % and the central 25 % of the blocks, INTERLEAVED on one
            context (plain, all, r25, r5, c25, plain, ...): per configuration the median over `--frames` frames after `--warmup` cycles of
            render_ms (device time between the frame's begin and end events), of the host time of the whole call (compaction, the 4-byte
            readback and the wait included) and the active share of the pixels; `vs_plain` = render_ms / plain render_ms
  adaptive  a progressive loop of `--subframes` calls of pt_render_adaptive at the stated threshold against the same number of plain
            frames: pixel_subframes (samples spent, in pixels x subframes), device time (sum of render_ms, which includes the decision and
            compaction kernels), host time, the median decide_ms, and the active blocks after every 8th call

  python3 tools/adaptive_bench.py [--frames 24] [--warmup 3] [--subframes 64] [--threshold 0.05] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--subframes", type=int, default=64)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--dark-floor", type=float, default=0.01)
    ap.add_argument("--min-subframes", type=int, default=8)
    ap.add_argument("--small", action="store_true", help="rehearsal: a 30 k-triangle terrain at 640x360")
    args = ap.parse_args()

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    w, h, spp, depth = (640, 360, 4, 8) if args.small else (1920, 1080, 4, 8)
    model = scenes.voxel_terrain(n=64, target_tris=30000) if args.small else scenes.voxel_terrain()
    r = R.SampleRenderer(model)
    r.setOptions(max_depth=depth)
    r.setProbe(scenes.sky_probe(2048, 1024).BuildCDF())
    r.resize((w, h))
    r.setCamera(R.make_camera(scenes.TERRAIN_CAMERA, w / h))
    r.launchParams.samples_per_launch = spp
    nby, nbx = r.blockGrid()
    rng = np.random.default_rng(1)
    u = rng.random((nby, nbx))
    by, bx = np.mgrid[0:nby, 0:nbx]
    central = (np.abs(bx - (nbx - 1) / 2) < nbx / 4) & (np.abs(by - (nby - 1) / 2) < nby / 4)
    configs = [("plain", None), ("mask_all", np.ones((nby, nbx), bool)), ("mask_random_25", u < 0.25), ("mask_random_5", u < 0.05), ("mask_central_25", central)]
    rec = {name: {"render_ms": [], "host_ms": [], "pixels": 0} for name, _ in configs}
    k = 0
    for cycle in range(args.warmup + args.frames):
        for name, m in configs:
            r.launchParams.frame.subframe_index = k
            k += 1
            t0 = time.perf_counter()
            n = w * h
            if m is None:
                r.render()
            else:
                n = r.renderMask(m)
            t1 = time.perf_counter()
            if cycle >= args.warmup:
                rec[name]["render_ms"].append(r.stats()["render_ms"])
                rec[name]["host_ms"].append((t1 - t0) * 1e3)
                rec[name]["pixels"] = n
    allocs = r.stats()["path_state_allocs"]
    masks = {}
    plain = float(np.median(rec["plain"]["render_ms"]))
    for name, _ in configs:
        t = np.array(rec[name]["render_ms"])
        masks[name] = {"render_ms": round(float(np.median(t)), 4), "render_ms_min": round(float(t.min()), 4), "render_ms_max": round(float(t.max()), 4),
                       "host_ms": round(float(np.median(rec[name]["host_ms"])), 4), "active_share": round(rec[name]["pixels"] / (w * h), 5),
                       "vs_plain": round(float(np.median(t)) / plain, 4), "frames": len(t)}

    # the progressive loop: plain frames, then the adaptive loop, both from subframe 0
    def loop(adaptive):
        dev = host = 0.0
        decide, active = [], []
        st = None
        for s in range(args.subframes):
            r.launchParams.frame.subframe_index = s
            t0 = time.perf_counter()
            if adaptive:
                st = r.renderAdaptive()
            else:
                r.render()
            host += (time.perf_counter() - t0) * 1e3
            dev += r.stats()["render_ms"]
            if adaptive:
                if st["active_pixels"]:
                    decide.append(st["decide_ms"])
                if s % 8 == 7:
                    active.append(st["active_blocks"])
        return dev, host, decide, active, st

    pdev, phost, _, _, _ = loop(False)
    r.adaptiveBegin(threshold=args.threshold, dark_floor=args.dark_floor, min_subframes=args.min_subframes)
    adev, ahost, decide, active, st = loop(True)
    out = {
        "workload": {"width": w, "height": h, "spp": spp, "max_depth": depth, "triangles": model.num_triangles, "blocks": nbx * nby},
        "masks": masks, "path_state_allocs": allocs,
        "adaptive": {
            "threshold": args.threshold, "dark_floor": args.dark_floor, "min_subframes": args.min_subframes, "subframes": args.subframes,
            "pixel_subframes": st["pixel_subframes"], "plain_pixel_subframes": w * h * args.subframes,
            "device_ms": round(adev, 3), "plain_device_ms": round(pdev, 3), "host_ms": round(ahost, 3), "plain_host_ms": round(phost, 3),
            "decide_ms_median": round(float(np.median(decide)), 4) if decide else None, "decide_ms_max": round(float(np.max(decide)), 4) if decide else None,
            "active_blocks_every_8th_call": active,
        },
    }
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    main()
