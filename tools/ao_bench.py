#!/usr/bin/env python3
"""ao_bench.py — what ambient occlusion from the G-buffer costs (pt_ao_planes: k_ao_rays, the any-hit traversal, k_ao_reduce) beside the
route a caller had before it: the same rays built on the GPU with torch, sent through traceDevice(any_hit=True) and reduced with torch.

One MI355X, the C3 terrain (1 M triangles) at 1920 x 1080 under bench.py's camera, rays 1, 4 and 8 a pixel, jitter on (the seed changes
from call to call), radius 2 world units, the default batch.  Steps, each a process of its own under `timeout`; the first step that fails
ends the tool with its status (nothing is tried twice):
  pass    per ray count: the pass's kernel_ms and trace_ms (out written), and the existing route's stage_ms + trace_ms + attrib_ms
          (pt_query_stats) with the torch time of building the rays and of reducing the flags beside it (events on torch's stream)
  batch   8 rays a pixel at max_rays_in_flight 2^19, 2^21, 2^23 (the default) and 2^25 (the whole frame): kernel_ms, trace_ms, batches,
          scratch bytes
Medians over --reps calls after --warmup, the two routes taking turns.  The torch route evaluates the header's rule with torch's float32
operators; it is not held to the bits (tests/test_gpu_ao.py does that with NumPy), only its occluded count is printed beside the pass's.
Traffic, in bytes a ray outside the traversal's own reads: the existing route writes 32 (the caller's rays), reads 32 and writes 32 (the
staging), writes and reads a record of 8, writes and reads a flag of 4: 120, and its ray buffer is unbounded (rays x 36 bytes of the
caller's, rays x 40 of the library's); the pass writes 32, writes and reads a record of 8: 48 (64 with bent, which reads the direction
back), in a scratch of one batch.  No threshold is attached to any figure.  Prints one JSON object; --md PATH also writes the tables as
markdown with the raw JSON below them, replacing that file's part from "## Timings" on.
  python3 tools/ao_bench.py [--reps 20] [--warmup 5] [--md profiles/ao.md]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
RADIUS, BIAS = 2.0, 1e-3
RAYS = (1, 4, 8)
BATCHES = (1 << 19, 1 << 21, 1 << 23, 1 << 25)
STEPS = [("pass", 420), ("batch", 300)]  # (step, seconds allowed)


def spiral():
    """D[0 .. 127] of the header, in float32"""
    f32 = np.float32
    C, S = np.array([0xBF3CC435, 0x3F2CECEF], np.uint32).view(f32)
    D = np.zeros((128, 2), f32)
    D[0] = (1.0, 0.0)
    for n in range(127):
        x, y = D[n]
        D[n + 1] = (x * C - y * S, x * S + y * C)
    return D


def torch_rays(torch, hit, position, eye, D, rays, seed):
    """the header's steps 1 to 6 with torch: (the traced pixels' indices, their (n * rays, 8) rays)"""
    h, w = hit.shape[:2]
    H8, P4 = hit.reshape(-1, 8), position.reshape(-1, 4)
    prim = H8[:, 3].view(torch.int32)
    ok = (prim >= 0) & torch.isfinite(P4[:, 0:3]).all(1) & torch.isfinite(H8[:, 5:8]).all(1) & torch.isfinite(H8[:, 0]) & (H8[:, 0] > 0)
    sel = torch.nonzero(ok).reshape(-1)
    P, n0, t = P4[sel, 0:3], H8[sel, 5:8], H8[sel, 0]
    s = (n0 * (eye - P)).sum(1)
    n = torch.where((s < 0)[:, None], -n0, n0)
    sg = torch.where(n[:, 2] >= 0, 1.0, -1.0).to(torch.float32)
    a = -1.0 / (sg + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    T = torch.stack([1.0 + sg * n[:, 0] * n[:, 0] * a, sg * b, -sg * n[:, 0]], 1)
    B = torch.stack([b, sg + n[:, 1] * n[:, 1] * a, -n[:, 1]], 1)
    O = P + n * (BIAS * t)[:, None]
    x, y = (sel % w).to(torch.int64), (sel // w).to(torch.int64)
    M = 0xFFFFFFFF
    hsh = ((x * 0x9E3779B1) & M) ^ ((y * 0x85EBCA77) & M) ^ ((seed * 0xC2B2AE3D) & M)
    hsh = hsh ^ (hsh >> 16)
    hsh = (hsh * 0x7FEB352D) & M
    hsh = hsh ^ (hsh >> 15)
    hsh = (hsh * 0x846CA68B) & M
    hsh = hsh ^ (hsh >> 16)
    k0 = hsh & 63
    out = torch.empty((len(sel), rays, 8), device=hit.device)
    for k in range(rays):
        rho = float(np.sqrt(np.float32((k + 0.5) / rays)))
        Dk = D[(k0 + k) & 127]
        ak, bk = rho * Dk[:, 0], rho * Dk[:, 1]
        ck = torch.sqrt(torch.clamp(1.0 - (ak * ak + bk * bk), min=0.0))
        d = T * ak[:, None] + B * bk[:, None] + n * ck[:, None]
        out[:, k, 4:7] = d / torch.linalg.norm(d, dim=1, keepdim=True)
    out[:, :, 0:3] = O[:, None, :]
    out[:, :, 3] = 0.0
    out[:, :, 7] = RADIUS
    return sel, out.reshape(-1, 8)


def _context():
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    r = R.SampleRenderer(scenes.voxel_terrain())
    r.resize((W, H))
    cam = R.make_camera(scenes.TERRAIN_CAMERA, W / H)
    r.setCamera(cam)
    g = r.renderGBuffer(("hit", "position"))
    return torch, r, g["hit"], g["position"], torch.tensor(scenes.TERRAIN_CAMERA["eye"], device="cuda:0")


def med(v):
    return float(np.median(v))


def step_pass(args):
    torch, r, hit, position, eye = _context()
    D = torch.from_numpy(spiral()).to("cuda:0")
    out = torch.zeros((H, W, 4), device="cuda:0")
    rows = {}
    for rays in RAYS:
        scratch = torch.zeros((r.aoLayout(rays) // 4,), device="cuda:0")
        acc = dict(kernel_ms=[], trace_ms=[], q_stage=[], q_trace=[], q_attrib=[], build_ms=[], reduce_ms=[])
        st = occ = n = None
        for k in range(args.warmup + args.reps):  # the two routes take turns
            st = r.aoPlanes(hit, position, out=out, scratch=scratch, rays=rays, radius=RADIUS, bias=BIAS, jitter=True, seed=k)["stats"]
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            sel, rr = torch_rays(torch, hit, position, eye, D, rays, k)
            e[1].record()
            flags = r.traceDevice(rr, any_hit=True)
            q = dict(r.queryStats)
            e[2].record()
            ao = 1.0 - (flags.reshape(-1, rays) == 1).to(torch.float32).mean(1)
            e[3].record()
            torch.cuda.synchronize()
            occ, n = int((flags == 1).sum()), int(rr.shape[0])
            del ao, rr, flags, sel
            if k >= args.warmup:
                for name, v in (("kernel_ms", st["kernel_ms"]), ("trace_ms", st["trace_ms"]), ("q_stage", q["stage_ms"]), ("q_trace", q["trace_ms"]),
                                ("q_attrib", q["attrib_ms"]), ("build_ms", e[0].elapsed_time(e[1])), ("reduce_ms", e[2].elapsed_time(e[3]))):
                    acc[name].append(v)
        route = med(np.add(np.add(acc["q_stage"], acc["q_trace"]), acc["q_attrib"]))
        rows[str(rays)] = dict(kernel_ms=med(acc["kernel_ms"]), trace_ms=med(acc["trace_ms"]), route_ms=route, route_stage_ms=med(acc["q_stage"]),
                               route_trace_ms=med(acc["q_trace"]), route_attrib_ms=med(acc["q_attrib"]), torch_build_ms=med(acc["build_ms"]),
                               torch_reduce_ms=med(acc["reduce_ms"]), rays=st["rays"], occluded=st["occluded"], batches=st["batches"], traced=st["traced"],
                               route_rays=n, route_occluded=occ, scratch_bytes=int(scratch.numel() * 4), route_ray_bytes=n * 36, route_state_bytes=n * 40,
                               pass_bytes_per_ray=48, route_bytes_per_ray=120)
        del scratch
    r.close()
    return dict(rows=rows)


def step_batch(args):
    torch, r, hit, position, eye = _context()
    out = torch.zeros((H, W, 4), device="cuda:0")
    rows, rays = {}, 8
    scratch = {M: torch.zeros((r.aoLayout(rays, M) // 4,), device="cuda:0") for M in BATCHES}
    acc = {M: dict(kernel_ms=[], trace_ms=[]) for M in BATCHES}
    st = {}
    for k in range(args.warmup + args.reps):  # the batch sizes take turns
        for M in BATCHES:
            st[M] = r.aoPlanes(hit, position, out=out, scratch=scratch[M], rays=rays, radius=RADIUS, bias=BIAS, jitter=True, seed=k, max_rays_in_flight=M)["stats"]
            if k >= args.warmup:
                acc[M]["kernel_ms"].append(st[M]["kernel_ms"])
                acc[M]["trace_ms"].append(st[M]["trace_ms"])
    for M in BATCHES:
        rows[str(M)] = dict(kernel_ms=med(acc[M]["kernel_ms"]), trace_ms=med(acc[M]["trace_ms"]), batches=st[M]["batches"], scratch_bytes=int(scratch[M].numel() * 4),
                            rays=st[M]["rays"])
    r.close()
    return dict(rows=rows, rays=rays)


def markdown(res):
    md = ["## Timings (`tools/ao_bench.py`)\n",
          f"{W} x {H}, one MI355X, the C3 terrain, radius {RADIUS}, jitter on; medians over {res['reps']} calls after {res['warmup']} warm-up calls, the routes "
          "taking turns in one process.  `kernel_ms` is the pass's whole span, `trace_ms` its traversal launches; the existing route is "
          "`stage_ms + trace_ms + attrib_ms` of `traceDevice(any_hit=True)` over rays built with torch (torch's own time beside it, not in the sum).  "
          "Bytes a ray are ray and result traffic outside the traversal's reads.  No threshold is attached to any of these figures.\n",
          "| rays | pass `kernel_ms` | pass `trace_ms` | route stage + trace + attrib | route stage / trace / attrib | torch build / reduce | rays traced | pass scratch MB | route ray buffers MB | bytes a ray pass / route |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for rays, x in res["pass"]["rows"].items():
        md.append(f"| {rays} | {x['kernel_ms']:.3f} | {x['trace_ms']:.3f} | {x['route_ms']:.3f} | {x['route_stage_ms']:.3f} / {x['route_trace_ms']:.3f} / {x['route_attrib_ms']:.3f} | "
                  f"{x['torch_build_ms']:.3f} / {x['torch_reduce_ms']:.3f} | {x['rays']} | {x['scratch_bytes'] / 1e6:.1f} | {(x['route_ray_bytes'] + x['route_state_bytes']) / 1e6:.1f} | "
                  f"{x['pass_bytes_per_ray']} / {x['route_bytes_per_ray']} |")
    md += ["", f"`max_rays_in_flight`, {res['batch']['rays']} rays a pixel:\n", "| max_rays_in_flight | `kernel_ms` | `trace_ms` | batches | scratch MB |", "|---|---|---|---|---|"]
    for M, x in res["batch"]["rows"].items():
        md.append(f"| {M} | {x['kernel_ms']:.3f} | {x['trace_ms']:.3f} | {x['batches']} | {x['scratch_bytes'] / 1e6:.1f} |")
    md += ["", "## Raw output\n", "```json", json.dumps(res, indent=1), "```", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--md", help="also write the tables as markdown to this path")
    ap.add_argument("--step", help="run one step in this process and print its JSON line")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("ao_bench: no GPU")
        print("RESULT " + json.dumps(dict(STEP_FUNCTIONS)[args.step](args)), flush=True)
        return 0
    res = dict(reps=args.reps, warmup=args.warmup)
    passed = ["--reps", str(args.reps), "--warmup", str(args.warmup)]
    for step, seconds in STEPS:  # one attempt each; the first failure ends the tool
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step] + passed, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"ao_bench: step {step} ended with status {p.returncode}", file=sys.stderr)
            return p.returncode
        res[step] = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Ambient occlusion from the G-buffer (`pt_ao_layout`, `pt_ao_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


STEP_FUNCTIONS = (("pass", step_pass), ("batch", step_batch))

if __name__ == "__main__":
    sys.exit(main())
