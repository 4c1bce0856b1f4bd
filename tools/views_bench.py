#!/usr/bin/env python3
"""views_bench.py — what viewports (pt_set_views) cost and save.  Every frame is synchronous (render() returns when the device is done), every
figure is the median over `--frames` frames after `--warmup`, the two sides of a comparison are interleaved frame by frame.  ONE JSON object:

  stereo   frame 1920x1080 with two 960x1080 views of the C3 scene (1 M-triangle terrain, 4 spp, depth 8) against two 960x1080 contexts
           rendered one after the other: host ms per pair, device ms per pair (render_ms), and the device memory each set-up holds
           (hipMemGetInfo before the set-up and after its warm-up frames)
  array    64 views of 128x128 in a 1024x1024 frame against ONE 128x128 context rendered 64 times with setCamera in between
  headline (--headline PARENT_TREE) bench.py of a built checkout of the parent commit and of this tree, alternating, `--runs` each: ms per step of
           every run, the medians, the parent's max - min, and whether this tree's median stays within parent median + that spread

  python3 tools/views_bench.py [--frames 24] [--warmup 12] [--small] [--headline DIR --runs 5 --steps 30 --bench-warmup 3] [--out FILE]
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


def _free_bytes():
    """free device memory as the HIP runtime reports it (the runtime the library is bound to)"""
    import torch

    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def _median(x):
    return round(float(np.median(np.asarray(x, np.float64))), 4)


def _spread(x):
    return {"median": _median(x), "min": round(float(np.min(x)), 4), "max": round(float(np.max(x)), 4), "n": len(x)}


def _eye_cameras(R, cam, n, aspect, step):
    """n cameras side by side along the camera's right vector, `step` scene units apart"""
    eye, lookat, up = (np.array(cam[k], np.float64) for k in ("eye", "lookat", "up"))
    fwd = (lookat - eye) / np.linalg.norm(lookat - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    out = []
    for i in range(n):
        off = right * ((i - (n - 1) / 2) * step)
        out.append(R.Camera(tuple(eye + off), tuple(lookat + off), tuple(up), cam["fovY"], aspect))
    return out


def _renderer(R, scenes, model, probe, size, depth, spp):
    r = R.SampleRenderer(model)
    r.setOptions(max_depth=depth)
    r.setProbe(probe)
    r.resize(size)
    r.launchParams.samples_per_launch = spp
    return r


def _frame(r, k):
    r.launchParams.frame.subframe_index = k
    t0 = time.perf_counter()
    r.render()
    return (time.perf_counter() - t0) * 1e3, r.stats()["render_ms"]


def stereo(args, R, scenes, model, probe, cam):
    w, h, spp, depth = (640, 360, 4, 8) if args.small else (1920, 1080, 4, 8)
    ew = w // 2
    cams = _eye_cameras(R, cam, 2, ew / h, 0.065)
    free0 = _free_bytes()
    one = _renderer(R, scenes, model, probe, (w, h), depth, spp)
    one.setViews([(0, 0, ew, h, cams[0]), (ew, 0, ew, h, cams[1])])
    for k in range(args.warmup):
        _frame(one, k)
    free1 = _free_bytes()
    two = [_renderer(R, scenes, model, probe, (ew, h), depth, spp) for _ in cams]
    for r, c in zip(two, cams):
        r.setCamera(c)
        for k in range(args.warmup):
            _frame(r, k)
    free2 = _free_bytes()
    rec = {"views": {"host": [], "dev": []}, "contexts": {"host": [], "dev": []}}
    for k in range(args.warmup, args.warmup + args.frames):
        hms, dms = _frame(one, k)
        rec["views"]["host"].append(hms)
        rec["views"]["dev"].append(dms)
        pair = [_frame(r, k) for r in two]
        rec["contexts"]["host"].append(sum(p[0] for p in pair))
        rec["contexts"]["dev"].append(sum(p[1] for p in pair))
    paths = one.stats()["paths"]
    sched = one.stats()["schedule"], two[0].stats()["schedule"]
    one.close()
    for r in two:
        r.close()
    out = {"frame": [w, h], "view": [ew, h], "spp": spp, "max_depth": depth, "paths_per_pair": paths,
           "one_context_two_views": {"host_ms_per_pair": _spread(rec["views"]["host"]), "device_ms_per_pair": _spread(rec["views"]["dev"]),
                                     "device_memory_mb": round((free0 - free1) / 2**20, 1), "schedule": sched[0]},
           "two_contexts": {"host_ms_per_pair": _spread(rec["contexts"]["host"]), "device_ms_per_pair": _spread(rec["contexts"]["dev"]),
                            "device_memory_mb": round((free1 - free2) / 2**20, 1), "schedule": sched[1]}}
    out["views_vs_contexts_host"] = round(out["one_context_two_views"]["host_ms_per_pair"]["median"] / out["two_contexts"]["host_ms_per_pair"]["median"], 4)
    return out


def array(args, R, scenes, model, probe, cam):
    t, n, spp, depth = 128, 64, 4, 8
    cams = _eye_cameras(R, cam, n, 1.0, 0.25)
    atlas = _renderer(R, scenes, model, probe, (8 * t, 8 * t), depth, spp)
    atlas.setViews([((i % 8) * t, (i // 8) * t, t, t, c) for i, c in enumerate(cams)])
    single = _renderer(R, scenes, model, probe, (t, t), depth, spp)
    uvw = [(c.eye,) + tuple(c.UVWFrame()) for c in cams]  # the camera frames are computed once: the loop below times the renderer

    def sixty_four(k):
        t0 = time.perf_counter()
        dev = 0.0
        single.launchParams.frame.subframe_index = k
        for e, U, V, W in uvw:
            single.setCameraUVW(e, U, V, W)
            single.render()
            dev += single.stats()["render_ms"]
        return (time.perf_counter() - t0) * 1e3, dev

    rec = {"views": {"host": [], "dev": []}, "loop": {"host": [], "dev": []}}
    for k in range(args.warmup + args.frames):
        a = _frame(atlas, k)
        b = sixty_four(k)
        if k >= args.warmup:
            rec["views"]["host"].append(a[0])
            rec["views"]["dev"].append(a[1])
            rec["loop"]["host"].append(b[0])
            rec["loop"]["dev"].append(b[1])
    out = {"frame": [8 * t, 8 * t], "views": n, "view": [t, t], "spp": spp, "max_depth": depth, "paths_per_array": atlas.stats()["paths"],
           "one_frame_64_views": {"host_ms_per_array": _spread(rec["views"]["host"]), "device_ms_per_array": _spread(rec["views"]["dev"]), "schedule": atlas.stats()["schedule"]},
           "one_context_64_renders": {"host_ms_per_array": _spread(rec["loop"]["host"]), "device_ms_per_array": _spread(rec["loop"]["dev"]), "schedule": single.stats()["schedule"]}}
    out["views_vs_loop_host"] = round(out["one_frame_64_views"]["host_ms_per_array"]["median"] / out["one_context_64_renders"]["host_ms_per_array"]["median"], 4)
    atlas.close()
    single.close()
    return out


def _bench_ms(tree, steps, warmup):
    """ms per step of one run of the tree's own bench.py (its last JSON line)"""
    p = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=tree, check=True, capture_output=True, text=True, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for key in ("ms_per_step", "step_ms", "ms_per_frame"):
        if key in d:
            return float(d[key]), d
    raise SystemExit(f"bench.py of {tree}: no ms per step in {sorted(d)}")


def headline(args):
    runs = {"parent": [], "this": []}
    trees = {"parent": os.path.abspath(args.headline), "this": ROOT}
    for i in range(args.runs):
        for name in ("parent", "this"):
            ms, _ = _bench_ms(trees[name], args.steps, args.bench_warmup)
            runs[name].append(round(ms, 4))
            print(f"# bench.py {name} run {i}: {ms:.4f} ms per step", file=sys.stderr, flush=True)
    spread = max(runs["parent"]) - min(runs["parent"])
    mp, mt = float(np.median(runs["parent"])), float(np.median(runs["this"]))
    return {"steps": args.steps, "warmup": args.bench_warmup, "parent_ms_per_step": runs["parent"], "this_ms_per_step": runs["this"],
            "parent_median": round(mp, 4), "this_median": round(mt, 4), "parent_max_minus_min": round(spread, 4), "within_parent_spread": bool(mt <= mp + spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=12, help="per context; the on-line schedule trial of a small frame settles within 8 frames")
    ap.add_argument("--small", action="store_true", help="rehearsal: a 30 k-triangle terrain, stereo at 640x360")
    ap.add_argument("--skip-views", action="store_true", help="only the headline comparison")
    ap.add_argument("--headline", metavar="PARENT_TREE", default=None, help="a built checkout of the parent commit: run its bench.py and this tree's alternately")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.frames < 20 and not args.small:
        raise SystemExit("views_bench: medians of at least 20 frames")
    out = {}
    if not args.skip_views:
        from optixpathtracer_amd import renderer as R
        from optixpathtracer_amd import scenes

        model = scenes.voxel_terrain(n=64, target_tris=30000) if args.small else scenes.voxel_terrain()
        probe = scenes.sky_probe(2048, 1024).BuildCDF()
        out["workload"] = {"triangles": model.num_triangles, "frames": args.frames, "warmup": args.warmup}
        out["stereo"] = stereo(args, R, scenes, model, probe, scenes.TERRAIN_CAMERA)
        out["array"] = array(args, R, scenes, model, probe, scenes.TERRAIN_CAMERA)
    if args.headline:
        out["headline"] = headline(args)
    text = json.dumps(out)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
