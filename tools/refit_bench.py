#!/usr/bin/env python3
"""refit_bench.py — cost of moving geometry (pt_update_meshes) on the 1 M-triangle workloads, and what a refitted tree costs per frame.

Per scene (C3 terrain and the stadium, 1920x1080, 4 spp, depth 8), printed as ONE JSON object:
  refit_kernel_ms   median device time of 20 refits under a moving displacement (hipEvents around the kernels, no upload)
  refit_host_ms     median host time of the whole call (validation, the 12 MB upload, kernels, wait)
  rebuild_kernel_ms median of 3 PT_UPDATE_REBUILD calls (build + calibration + side arrays)
  create_ms         pt_create of the deformed scene (pt_stats.create_ms)
  frames            for two displacement amplitudes: frame time (median render_ms of 8 synchronous frames) on the refitted tree and on
                    the tree rebuilt over the same vertices — the tree-quality cost that says when to rebuild.

Every scene runs in a child process of its own under `timeout -k 10`; the first child that fails ends the run (nothing more is started).
  python3 tools/refit_bench.py [--scenes terrain,stadium] [--timeout 600]
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


def _wave(model, amp, phase):
    out = {}
    for i, m in enumerate(model.meshes):
        v = np.asarray(m.vertex, np.float32)
        d = np.stack([np.sin(0.05 * v[:, 2] + phase), np.sin(0.04 * v[:, 0] + 1.3 * phase), np.cos(0.03 * (v[:, 0] + v[:, 2]) + phase)], 1)
        out[i] = (v + np.float32(amp) * d.astype(np.float32)).astype(np.float32)
    return out


def _frame_ms(r, n=8):
    ts = []
    for k in range(n + 2):
        r.launchParams.frame.subframe_index = k
        r.render()
        if k >= 2:
            ts.append(r.stats()["render_ms"])
    return float(np.median(ts))


def one(scene_name):
    import copy

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    model = {"terrain": scenes.voxel_terrain, "stadium": scenes.stadium_scene}[scene_name]()
    cam = {"terrain": scenes.TERRAIN_CAMERA, "stadium": scenes.STADIUM_CAMERA}[scene_name]
    w, h = 1920, 1080
    probe = scenes.sky_probe(2048, 1024).BuildCDF()
    r = R.SampleRenderer(model)
    r.setProbe(probe)
    r.resize((w, h))
    r.setCamera(R.make_camera(cam, w / h))
    r.launchParams.samples_per_launch = 4
    out = dict(scene=scene_name, triangles=model.num_triangles, base_frame_ms=_frame_ms(r))
    poses = [_wave(model, 0.5, 0.3 * k) for k in range(21)]
    kms, hms = [], []
    r.updateMeshes(poses[0])  # first refit allocates the side arrays
    for k in range(1, 21):
        t0 = time.perf_counter()
        kms.append(r.updateMeshes(poses[k]))
        hms.append((time.perf_counter() - t0) * 1e3)
    out["refit_kernel_ms"] = float(np.median(kms))
    out["refit_host_ms"] = float(np.median(hms))
    out["rebuild_kernel_ms"] = float(np.median([r.updateMeshes(poses[k], rebuild=True) for k in range(3)]))
    frames = {}
    for amp in (1.0, 8.0):
        pose = _wave(model, amp, 0.9)
        r.updateMeshes(_wave(model, 0.0, 0.0), rebuild=True)  # the tree of the undeformed scene ...
        r.updateMeshes(pose)  # ... refitted to the pose
        refit_ms = _frame_ms(r)
        r.updateMeshes(pose, rebuild=True)
        frames[str(amp)] = dict(refit_frame_ms=refit_ms, rebuilt_frame_ms=_frame_ms(r))
    out["frames"] = frames
    r.close()
    deformed = copy.deepcopy(model)
    for i, v in _wave(model, 8.0, 0.9).items():
        deformed.meshes[i].vertex = v
    r2 = R.SampleRenderer(deformed)
    out["create_ms"] = r2.stats()["create_ms"]
    r2.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="terrain,stadium")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per scene")
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
    return 0


if __name__ == "__main__":
    sys.exit(main())
