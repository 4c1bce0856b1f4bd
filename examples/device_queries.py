#!/usr/bin/env python3
"""device_queries.py — a lidar sweep over moving geometry in which nothing touches the host: every step turns the box of the two-box scene
with a matrix (transformMeshes: the vertices are transformed and the tree refitted on the GPU), fires a fan of torch-generated rays at the
scene from GPU memory (traceDevice, asynchronous: torch's stream waits for the hits on the device) and reduces the hits with torch — the mean
range, how many beams met the box, and the cosine between each beam and the surface it met, from the hit's geometric normal.  The only host
read is the line printed per step.

  python3 examples/device_queries.py [--steps 8] [--beams 256 64]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from optixpathtracer_amd import renderer as R  # noqa: E402
from optixpathtracer_amd import scenes  # noqa: E402


def fan(torch, origin, n_az, n_el, dev):
    """n_az x n_el beams around `origin`: a full turn in azimuth, -30..+10 degrees in elevation."""
    az = torch.linspace(0.0, 2.0 * math.pi, n_az + 1, device=dev)[:-1]
    el = torch.deg2rad(torch.linspace(-30.0, 10.0, n_el, device=dev))
    d = torch.stack([torch.cos(el)[None, :] * torch.cos(az)[:, None], torch.sin(el)[None, :].expand(n_az, n_el), torch.cos(el)[None, :] * torch.sin(az)[:, None]], 2)
    rays = torch.empty((n_az * n_el, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = torch.tensor(origin, dtype=torch.float32, device=dev)
    rays[:, 3] = 1e-3  # tmin
    rays[:, 4:7] = d.reshape(-1, 3)
    rays[:, 7] = 50.0  # tmax: the sensor's range
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--beams", type=int, nargs=2, default=[256, 64])
    args = ap.parse_args()
    import torch

    dev = "cuda:0"
    sample = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))  # mesh 0: the unit box, mesh 1: the ground
    rays = fan(torch, (2.5, 1.5, 0.0), args.beams[0], args.beams[1], dev)
    hits = torch.empty((len(rays), 8), dtype=torch.float32, device=dev)  # one 32-byte pt_hit per beam, reused every step
    for k in range(args.steps):
        a = 0.2 * k
        turn = np.array([[math.cos(a), 0, math.sin(a), 0], [0, 1, 0, 0.05 * k], [-math.sin(a), 0, math.cos(a), 0]], np.float32)
        sample.transformMeshes({0: turn})  # from the rest positions: the steps do not drift
        res = sample.traceDevice(rays, out=hits, wait=False)  # enqueued; torch's current stream waits for it on the device
        hit = res["prim"] >= 0
        on_box = (res["mesh"] == 0).sum()
        mean_range = torch.where(hit, res["t"], torch.zeros_like(res["t"])).sum() / hit.sum().clamp(min=1)
        cosine = (res["ng"] * rays[:, 4:7]).sum(1).abs()  # ng is not flipped towards the ray
        grazing = (hit & (cosine < 0.2)).sum()
        print(f"step {k}: {int(hit.sum())} of {len(rays)} beams returned, {int(on_box)} from the box, mean range {float(mean_range):.3f}, {int(grazing)} grazing")
    s = sample.queryWait()
    print(f"{s['rays']} rays in {args.steps} queries: staging {s['stage_ms']:.3f} ms, traversal {s['trace_ms']:.3f} ms, attributes {s['attrib_ms']:.3f} ms; "
          f"query state {s['state_bytes']} bytes")
    sample.close()


if __name__ == "__main__":
    main()
