#!/usr/bin/env python3
"""query_bench.py — what a ray query from GPU memory costs (pt_trace_device), kernel by kernel, against pt_trace and a plain copy.

Scene: the C3 terrain (1 M triangles).  Two batches of 1920 x 1080 = 2 073 600 rays, both generated with torch on the GPU:
  coherent    the camera rays of a 1080p frame (pixel centres through the terrain camera)
  incoherent  uniform origins over the scene's box, uniform directions (the generator of the parity tests)
Per batch, medians over --reps synchronous closest-hit queries after two warm-up queries, printed as ONE JSON object:
  stage_ms, trace_ms, attrib_ms   pt_query_stats: device time of k_stage_rays, the traversal launch, k_hit_attributes (hipEvents)
  mrays_s                         rays / (stage + trace + attrib): the whole call on the device
  any_*                           the same for an any-hit query
  off4_stage_ms, off4_attrib_ms   the two new kernels with rays and records one float into their allocations (4-byte aligned, not 16)
  pt_trace_kernel_ms              kernel_ms of pt_trace on the same rays from host memory: the same traversal launch
  copy_ms                         a device-to-device copy of n x 32 bytes (torch's copy_, a hipMemcpyAsync), by events: k_stage_rays' yardstick
  host_async_us                   host time of one PT_QUERY_ASYNC call (perf_counter around the C call; the state is allocated already)
  host_pt_trace_ms                host time of pt_trace for the same rays
--md PATH also writes the table as markdown with the raw JSON below it.
  timeout -k 10 300 python3 tools/query_bench.py [--reps 7] [--md profiles/device_query.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080


def camera_rays(torch, cam, dev):
    from optixpathtracer_amd import scenes

    U, V, Wv = (torch.tensor(np.asarray(a, np.float32), device=dev) for a in scenes.uvw_frame(**cam, aspect=W / H))
    x = (torch.arange(W, device=dev, dtype=torch.float32) + 0.5) / W * 2 - 1
    y = (torch.arange(H, device=dev, dtype=torch.float32) + 0.5) / H * 2 - 1
    d = x[None, :, None] * U + y[:, None, None] * V + Wv
    d = (d / d.norm(dim=2, keepdim=True)).reshape(-1, 3)
    rays = torch.empty((W * H, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = torch.tensor(cam["eye"], dtype=torch.float32, device=dev)
    rays[:, 3] = 1e-3
    rays[:, 4:7] = d
    rays[:, 7] = 1e16
    return rays


def random_rays(torch, n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(10)
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = torch.rand((n, 3), generator=g, device=dev) * 220 - 110
    rays[:, 1] = torch.rand(n, generator=g, device=dev) * 90 - 30
    d = torch.randn((n, 3), generator=g, device=dev)
    rays[:, 4:7] = d / d.norm(dim=1, keepdim=True)
    rays[:, 3] = 1e-3
    rays[:, 7] = 1e16
    return rays


def measure(torch, r, rays, reps):
    from optixpathtracer_amd import _lib

    n = len(rays)
    out = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
    occ = torch.empty(n, dtype=torch.int32, device=rays.device)
    res = {}
    for name, any_hit, o in (("", False, out), ("any_", True, occ)):
        rows = []
        for k in range(reps + 2):
            r.traceDevice(rays, any_hit=any_hit, out=o)
            if k >= 2:
                s = r.queryStats
                rows.append((s["stage_ms"], s["trace_ms"], s["attrib_ms"]))
        st, tr, at = np.median(np.array(rows), axis=0)
        res.update({name + "stage_ms": st, name + "trace_ms": tr, name + "attrib_ms": at, name + "mrays_s": n / (st + tr + at) / 1e3, name + "hits": r.queryStats["hits"]})
    res["state_bytes"] = r.queryStats["state_bytes"]
    # the same rays and records one float into their allocations: 4-byte aligned, not 16
    rbuf = torch.empty(n * 8 + 1, dtype=torch.float32, device=rays.device)
    obuf = torch.empty(n * 8 + 1, dtype=torch.float32, device=rays.device)
    r4, o4 = rbuf[1:].view(n, 8), obuf[1:].view(n, 8)
    r4.copy_(rays)
    rows = []
    for k in range(reps + 2):
        r.traceDevice(r4, out=o4)
        if k >= 2:
            rows.append((r.queryStats["stage_ms"], r.queryStats["attrib_ms"]))
    res["off4_stage_ms"], res["off4_attrib_ms"] = np.median(np.array(rows), axis=0)
    del rbuf, obuf, r4, o4
    # pt_trace on the same rays, in the same run
    host = rays.cpu().numpy()
    kms, hms = [], []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        _, ms = r.trace(host)
        hms.append((time.perf_counter() - t0) * 1e3)
        kms.append(ms)
    res["pt_trace_kernel_ms"] = float(np.median(kms[1:]))
    res["host_pt_trace_ms"] = float(np.median(hms[1:]))
    # the copy
    dst = torch.empty_like(rays)
    cms = []
    for k in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(rays)
        e1.record()
        e1.synchronize()
        cms.append(e0.elapsed_time(e1))
    res["copy_ms"] = float(np.median(cms[2:]))
    # host cost of an asynchronous call
    torch.cuda.synchronize()
    hus = []
    for k in range(reps + 2):
        t0 = time.perf_counter()
        rc = r._L.pt_trace_device(r._ctx, rays.data_ptr(), n, _lib.PT_QUERY_CLOSEST | _lib.PT_QUERY_ASYNC, out.data_ptr(), None)
        hus.append((time.perf_counter() - t0) * 1e6)
        assert rc == 0
        r.queryWait()
    res["host_async_us"] = float(np.median(hus[2:]))
    return {k: (float(v) if isinstance(v, (float, np.floating)) else int(v)) for k, v in res.items()}


def markdown(result):
    md = ["# Ray queries from GPU memory (`tools/query_bench.py`)\n",
          f"C3 terrain, {result['triangles']} triangles, {result['rays']} rays per batch, one MI355X; medians.  Device times by hipEvents.\n",
          "| batch | `stage_ms` | `trace_ms` | `attrib_ms` | Mrays/s (whole call) | `pt_trace` `kernel_ms` | copy of n x 32 B, ms | host: async call, us | host: `pt_trace`, ms |", "|---|---|---|---|---|---|---|---|---|"]
    for b in ("coherent", "incoherent"):
        x = result[b]
        md.append(f"| {b}, closest hit | {x['stage_ms']:.4f} | {x['trace_ms']:.4f} | {x['attrib_ms']:.4f} | {x['mrays_s']:.0f} | {x['pt_trace_kernel_ms']:.4f} | {x['copy_ms']:.4f} | {x['host_async_us']:.1f} | {x['host_pt_trace_ms']:.1f} |")
        md.append(f"| {b}, any hit | {x['any_stage_ms']:.4f} | {x['any_trace_ms']:.4f} | {x['any_attrib_ms']:.4f} | {x['any_mrays_s']:.0f} | | | | |")
        md.append(f"| {b}, closest hit, arrays at a 4-byte offset | {x['off4_stage_ms']:.4f} | | {x['off4_attrib_ms']:.4f} | | | | | |")
    md += ["", "## Raw output\n", "```json", json.dumps(result, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--md", help="also write the table as markdown to this path")
    args = ap.parse_args()
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    dev = "cuda:0"
    model = scenes.voxel_terrain()
    r = R.SampleRenderer(model)
    result = dict(triangles=model.num_triangles, rays=W * H)
    result["coherent"] = measure(torch, r, camera_rays(torch, scenes.TERRAIN_CAMERA, dev), args.reps)
    result["incoherent"] = measure(torch, r, random_rays(torch, W * H, dev), args.reps)
    r.close()
    print(json.dumps(result), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(markdown(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
