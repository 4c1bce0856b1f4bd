#!/usr/bin/env python3
"""shadow_bench.py — what sun shadows from the G-buffer cost (pt_shadow_planes: k_shadow_rays, the any-hit traversal, k_shadow_reduce)
beside the route a caller had before it: the same rays built on the GPU with torch, sent through traceDevice(any_hit=True), and the flags
reduced and scattered back to the frame with torch.

One MI355X, the C3 terrain (1 M triangles) at 1920 x 1080 under bench.py's camera, two lights — one of 1 ray, one of 8 rays, both at spread
0.01 — the default max_distance and bias, no jitter.  One measurement, in this process (run it under `timeout`):
          the pass's kernel_ms and trace_ms writing visibility and light; the existing route's stage_ms + trace_ms (pt_query_stats) with
          the torch time of building the rays and of reducing the flags beside it (events on torch's stream); the share of (pixel, light)
          pairs under the horizon, and the rays the per-light compaction saved against pixels * R
Medians over --reps calls after --warmup, the two routes taking turns.  The torch route evaluates the header's rule with torch's float32
operators; it is not held to the bits (tests/test_gpu_shadow.py does that with NumPy), only its occluded count is printed beside the
pass's.  No threshold is attached to any figure.  Prints one JSON object; --md PATH also writes the table as markdown with the raw JSON
below it, replacing that file's part from "## Timings" on.
  python3 tools/shadow_bench.py [--reps 20] [--warmup 5] [--md profiles/shadow.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
BIAS, MAX_DISTANCE = 1e-3, 1e16
LIGHTS = [dict(dir=(0.4, 1.0, -0.3), spread=0.01, radiance=(3.0, 2.9, 2.7), rays=1), dict(dir=(-0.8, 0.35, 0.5), spread=0.01, radiance=(0.6, 0.7, 0.9), rays=8)]


def light_tables(torch):
    """per light: L, and the (rays, 3) unit directions of the unjittered pattern (the header's frame and spiral, in float32 NumPy)"""
    f = np.float32
    D = np.zeros((128, 2), f)
    D[0] = (1.0, 0.0)
    C, S = f(float.fromhex("-0x1.79886ap-1")), f(float.fromhex("0x1.59d9dep-1"))  # pt_dof_planes's constants, as include/pt_amd.h writes them
    for n in range(127):
        D[n + 1] = (D[n, 0] * C - D[n, 1] * S, D[n, 0] * S + D[n, 1] * C)
    out = []
    for l in LIGHTS:
        L = np.asarray(l["dir"], f)
        L = L / f(np.sqrt((L * L).sum()))
        sg = f(1.0) if L[2] >= 0 else f(-1.0)
        a = f(-1.0) / (sg + L[2])
        b = L[0] * L[1] * a
        T = np.array([f(1.0) + sg * L[0] * L[0] * a, sg * b, -sg * L[0]], f)
        B = np.array([b, sg + L[1] * L[1] * a, -L[1]], f)
        k = np.arange(l["rays"], dtype=f)
        rho = np.sqrt((k + f(0.5)) / f(l["rays"])).astype(f)
        ab = rho[:, None] * D[:l["rays"]] * f(l["spread"])
        w = L[None, :] + T[None, :] * ab[:, 0:1] + B[None, :] * ab[:, 1:2]
        d = w / np.sqrt((w * w).sum(1, keepdims=True))
        out.append((torch.tensor(L, device="cuda:0"), torch.tensor(d.astype(f), device="cuda:0"), torch.tensor(l["radiance"], device="cuda:0")))
    return out


def torch_rays(torch, hit, position, eye, tables):
    """steps 1 to 5 with torch: the (m, 8) rays, light after light, and per light (pixel indices, clamped cosines)"""
    H8, P4 = hit.reshape(-1, 8), position.reshape(-1, 4)
    prim = H8[:, 3].view(torch.int32)
    ok = (prim >= 0) & torch.isfinite(P4[:, 0:3]).all(1) & torch.isfinite(H8[:, 5:8]).all(1) & torch.isfinite(H8[:, 0]) & (H8[:, 0] > 0)
    n0 = H8[:, 5:8]
    s = (n0 * (eye - P4[:, 0:3])).sum(1)
    n = torch.where((s < 0)[:, None], -n0, n0)
    O = P4[:, 0:3] + n * (BIAS * H8[:, 0])[:, None]
    parts, who = [], []
    for L, d, _ in tables:
        c = (n * L).sum(1)
        sel = torch.nonzero(ok & (c > 0)).reshape(-1)
        r = torch.empty((len(sel), d.shape[0], 8), device=hit.device)
        r[:, :, 0:3] = O[sel][:, None, :]
        r[:, :, 3] = 0.0
        r[:, :, 4:7] = d[None, :, :]
        r[:, :, 7] = MAX_DISTANCE
        parts.append(r.reshape(-1, 8))
        who.append((sel, c[sel].clamp(max=1.0)))
    return torch.cat(parts), who, ok


def torch_reduce(torch, occ, who, ok, tables, visibility, light):
    """steps 6 and 7 with torch; ok: the pixels that passed steps 1 and 2"""
    visibility.fill_(1.0)
    light.zero_()
    light[..., 3] = 1.0
    V, Lt = visibility.reshape(-1, 4), light.reshape(-1, 4)
    at = 0
    for i, ((sel, c), (_, d, radiance)) in enumerate(zip(who, tables)):
        rays = d.shape[0]
        m = len(sel) * rays
        v = (occ[at:at + m].reshape(-1, rays) != 1).sum(1).to(torch.float32) / rays
        at += m
        V[:, i] = torch.where(ok, 0.0, 1.0)
        V[sel, i] = v
        Lt[sel, 0:3] += radiance[None, :] * (c * v)[:, None]
    return V


def _context():
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    r = R.SampleRenderer(scenes.voxel_terrain())
    r.resize((W, H))
    r.setCamera(R.make_camera(scenes.TERRAIN_CAMERA, W / H))
    g = r.renderGBuffer(("hit", "position"))
    return torch, r, g["hit"], g["position"], torch.tensor(scenes.TERRAIN_CAMERA["eye"], device="cuda:0")


def med(v):
    return float(np.median(v))


def measure(args):
    torch, r, hit, position, eye = _context()
    tables = light_tables(torch)
    R_ = sum(l["rays"] for l in LIGHTS)
    planes = dict(visibility=torch.zeros((H, W, 4), device="cuda:0"), light=torch.zeros((H, W, 4), device="cuda:0"))
    route = dict(visibility=torch.zeros((H, W, 4), device="cuda:0"), light=torch.zeros((H, W, 4), device="cuda:0"))
    scratch = torch.zeros((r.shadowLayout(LIGHTS) // 4,), device="cuda:0")
    acc = dict(kernel_ms=[], trace_ms=[], q_stage=[], q_trace=[], build_ms=[], reduce_ms=[])
    st = occluded = n = None
    for k in range(args.warmup + args.reps):  # the routes take turns
        st = r.shadowPlanes(hit, position, lights=LIGHTS, scratch=scratch, bias=BIAS, max_distance=MAX_DISTANCE, **planes)["stats"]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        rr, who, ok = torch_rays(torch, hit, position, eye, tables)
        e[1].record()
        occ = r.traceDevice(rr, any_hit=True)
        q = dict(r.queryStats)
        e[2].record()
        torch_reduce(torch, occ, who, ok, tables, route["visibility"], route["light"])
        e[3].record()
        torch.cuda.synchronize()
        occluded, n = int((occ == 1).sum()), int(rr.shape[0])
        del rr, occ, who
        if k >= args.warmup:
            for name, v in (("kernel_ms", st["kernel_ms"]), ("trace_ms", st["trace_ms"]), ("q_stage", q["stage_ms"]), ("q_trace", q["trace_ms"]),
                            ("build_ms", e[0].elapsed_time(e[1])), ("reduce_ms", e[2].elapsed_time(e[3]))):
                acc[name].append(v)
    pairs = st["traced"] * len(LIGHTS)
    row = dict(kernel_ms=med(acc["kernel_ms"]), trace_ms=med(acc["trace_ms"]), route_ms=med(np.add(acc["q_stage"], acc["q_trace"])),
               route_stage_ms=med(acc["q_stage"]), route_trace_ms=med(acc["q_trace"]), torch_build_ms=med(acc["build_ms"]), torch_reduce_ms=med(acc["reduce_ms"]),
               pixels=st["pixels"], traced=st["traced"], backfacing=st["backfacing"], backfacing_share=st["backfacing"] / max(pairs, 1), rays=st["rays"],
               occluded=st["occluded"], invalid=st["invalid"], batches=st["batches"], rays_without_compaction=st["traced"] * R_,
               rays_saved_share=1.0 - (st["rays"] + st["invalid"]) / max(st["traced"] * R_, 1), route_rays=n, route_occluded=occluded,
               scratch_bytes=int(scratch.numel() * 4), route_ray_bytes=n * 64)
    r.close()
    return dict(row=row)


def markdown(res):
    x = res["pass"]["row"]
    md = ["## Timings (`tools/shadow_bench.py`)\n",
          f"{W} x {H}, one MI355X, the C3 terrain, one light of 1 ray and one of 8 rays at spread 0.01; medians over {res['reps']} calls after {res['warmup']} warm-up "
          "calls, the routes taking turns in one process.  `kernel_ms` is the pass's whole span, `trace_ms` its traversal launches; the existing route is "
          "`stage_ms + trace_ms` of `traceDevice(any_hit=True)` over rays built with torch (torch's own time beside it, not in the sum).  No threshold is "
          "attached to any of these figures.\n",
          "| pass `kernel_ms` | pass `trace_ms` | route stage + trace | route stage / trace | torch build / reduce | pixels traced | rays traced | occluded pass / route | "
          "pairs under the horizon | rays saved against pixels * R | pass scratch MB | route ray buffer MB |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|",
          f"| {x['kernel_ms']:.3f} | {x['trace_ms']:.3f} | {x['route_ms']:.3f} | {x['route_stage_ms']:.3f} / {x['route_trace_ms']:.3f} | "
          f"{x['torch_build_ms']:.3f} / {x['torch_reduce_ms']:.3f} | {x['traced']} | {x['rays']} | {x['occluded']} / {x['route_occluded']} | "
          f"{x['backfacing']} ({100 * x['backfacing_share']:.1f} %) | {x['rays_without_compaction'] - x['rays'] - x['invalid']} ({100 * x['rays_saved_share']:.1f} %) | "
          f"{x['scratch_bytes'] / 1e6:.1f} | {x['route_ray_bytes'] / 1e6:.1f} |",
          "", "## Raw output\n", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--md", help="also write the table as markdown to this path")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("shadow_bench: no GPU")
    res = {"reps": args.reps, "warmup": args.warmup, "pass": measure(args)}
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Sun shadows from the G-buffer (`pt_shadow_layout`, `pt_shadow_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
