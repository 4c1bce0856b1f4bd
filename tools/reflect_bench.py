#!/usr/bin/env python3
"""reflect_bench.py — what mirror reflections from the G-buffer cost (pt_reflect_planes: k_reflect_rays, the closest-hit traversal,
k_reflect_resolve) beside the route a caller had before it: the same rays built on the GPU with torch, sent through
traceDevice(any_hit=False), and the linear records scattered back to the frame with torch.

One MI355X, the C3 terrain (1 M triangles) at 1920 x 1080 under bench.py's camera, a 1024 x 512 sky probe, the default max_distance and
bias.  Steps, each a process of its own under `timeout`; the first step that fails ends the tool with its status (nothing is tried twice):
  pass    the pass's kernel_ms and trace_ms writing hit2 and position2 (what the route produces), and writing all four planes (ray and sky
          as well); the existing route's stage_ms + trace_ms + attrib_ms (pt_query_stats) with the torch time of building the rays and of
          scattering the records and computing position2 beside it (events on torch's stream)
  batch   hit2 and position2 at max_rays_in_flight 2^17, 2^19, 2^21 (the whole frame) and the default: kernel_ms, trace_ms, batches,
          scratch bytes
Medians over --reps calls after --warmup, the two routes taking turns.  The torch route evaluates the header's rule with torch's float32
operators; it is not held to the bits (tests/test_gpu_reflect.py does that with NumPy), only its hit count is printed beside the pass's.
Traffic, in bytes a ray outside the traversal's own reads: the existing route writes 32 (the caller's rays), reads 32 and writes 32 (the
staging), writes and reads a record of 8, reads the staged 32 again and writes a pt_hit of 32, which torch reads and scatters as 32 more,
and 16 of position2: 256, and its ray buffers are unbounded (rays x 64 bytes of the caller's, rays x 40 of the library's); the pass writes
32, writes and reads a record of 8, reads the 32 back, writes 32 of hit2 and 16 of position2: 128, in a scratch of one batch.  No threshold
is attached to any figure.  Prints one JSON object; --md PATH also writes the tables as markdown with the raw JSON below them, replacing
that file's part from "## Timings" on.
  python3 tools/reflect_bench.py [--reps 20] [--warmup 5] [--md profiles/reflect.md]
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
BIAS, MAX_DISTANCE = 1e-3, 1e16
BATCHES = (1 << 17, 1 << 19, 1 << 21, 0)
STEPS = [("pass", 420), ("batch", 300)]  # (step, seconds allowed)


def torch_rays(torch, hit, position, eye):
    """the header's steps 1 to 5 with torch: (the traced pixels' indices, their (n, 8) rays)"""
    H8, P4 = hit.reshape(-1, 8), position.reshape(-1, 4)
    prim = H8[:, 3].view(torch.int32)
    ok = (prim >= 0) & torch.isfinite(P4[:, 0:3]).all(1) & torch.isfinite(H8[:, 5:8]).all(1) & torch.isfinite(H8[:, 0]) & (H8[:, 0] > 0)
    sel = torch.nonzero(ok).reshape(-1)
    P, n0, t = P4[sel, 0:3], H8[sel, 5:8], H8[sel, 0]
    s = (n0 * (eye - P)).sum(1)
    n = torch.where((s < 0)[:, None], -n0, n0)
    d = P - eye
    d = d / torch.linalg.norm(d, dim=1, keepdim=True)
    k = 2.0 * (d * n).sum(1)
    r = d - n * k[:, None]
    r = r / torch.linalg.norm(r, dim=1, keepdim=True)
    out = torch.empty((len(sel), 8), device=hit.device)
    out[:, 0:3] = P + n * (BIAS * t)[:, None]
    out[:, 3] = 0.0
    out[:, 4:7] = r
    out[:, 7] = MAX_DISTANCE
    return sel, out


def torch_scatter(torch, sel, rays, records, hit2, position2):
    """the linear records back to the frame, and step 8"""
    hit2.reshape(-1, 8)[sel] = records
    is_hit = records[:, 3].view(torch.int32) >= 0
    p = rays[:, 0:3] + records[:, 0:1] * rays[:, 4:7]
    position2.reshape(-1, 4)[sel] = torch.where(is_hit[:, None], torch.cat([p, torch.ones_like(p[:, 0:1])], 1), torch.zeros((1, 4), device=p.device))
    return is_hit


def _context():
    import torch

    from optixpathtracer_amd import renderer as R
    from optixpathtracer_amd import scenes

    r = R.SampleRenderer(scenes.voxel_terrain())
    r.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    r.resize((W, H))
    cam = R.make_camera(scenes.TERRAIN_CAMERA, W / H)
    r.setCamera(cam)
    g = r.renderGBuffer(("hit", "position"))
    return torch, r, g["hit"], g["position"], torch.tensor(scenes.TERRAIN_CAMERA["eye"], device="cuda:0")


def med(v):
    return float(np.median(v))


def step_pass(args):
    torch, r, hit, position, eye = _context()
    planes = {n: torch.zeros((H, W, k), device="cuda:0") for n, k in (("hit2", 8), ("position2", 4), ("ray", 8), ("sky", 4))}
    route_hit2, route_position2 = torch.zeros((H, W, 8), device="cuda:0"), torch.zeros((H, W, 4), device="cuda:0")
    scratch = torch.zeros((r.reflectLayout() // 4,), device="cuda:0")
    acc = dict(kernel_ms=[], trace_ms=[], all_kernel_ms=[], all_trace_ms=[], q_stage=[], q_trace=[], q_attrib=[], build_ms=[], scatter_ms=[])
    st = full = hits = n = None
    for k in range(args.warmup + args.reps):  # the routes take turns
        st = r.reflectPlanes(hit, position, hit2=planes["hit2"], position2=planes["position2"], scratch=scratch, bias=BIAS, max_distance=MAX_DISTANCE)["stats"]
        full = r.reflectPlanes(hit, position, scratch=scratch, bias=BIAS, max_distance=MAX_DISTANCE, **planes)["stats"]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        sel, rr = torch_rays(torch, hit, position, eye)
        e[1].record()
        rec = r.traceDevice(rr, any_hit=False)["record"]
        q = dict(r.queryStats)
        e[2].record()
        is_hit = torch_scatter(torch, sel, rr, rec, route_hit2, route_position2)
        e[3].record()
        torch.cuda.synchronize()
        hits, n = int(is_hit.sum()), int(rr.shape[0])
        del rr, rec, sel, is_hit
        if k >= args.warmup:
            for name, v in (("kernel_ms", st["kernel_ms"]), ("trace_ms", st["trace_ms"]), ("all_kernel_ms", full["kernel_ms"]), ("all_trace_ms", full["trace_ms"]),
                            ("q_stage", q["stage_ms"]), ("q_trace", q["trace_ms"]), ("q_attrib", q["attrib_ms"]), ("build_ms", e[0].elapsed_time(e[1])),
                            ("scatter_ms", e[2].elapsed_time(e[3]))):
                acc[name].append(v)
    route = med(np.add(np.add(acc["q_stage"], acc["q_trace"]), acc["q_attrib"]))
    row = dict(kernel_ms=med(acc["kernel_ms"]), trace_ms=med(acc["trace_ms"]), all_kernel_ms=med(acc["all_kernel_ms"]), all_trace_ms=med(acc["all_trace_ms"]),
               route_ms=route, route_stage_ms=med(acc["q_stage"]), route_trace_ms=med(acc["q_trace"]), route_attrib_ms=med(acc["q_attrib"]),
               torch_build_ms=med(acc["build_ms"]), torch_scatter_ms=med(acc["scatter_ms"]), traced=st["traced"], hits=st["hits"], escaped=st["escaped"],
               invalid=st["invalid"], batches=st["batches"], route_rays=n, route_hits=hits, scratch_bytes=int(scratch.numel() * 4), route_ray_bytes=n * 64,
               route_state_bytes=n * 40, pass_bytes_per_ray=128, route_bytes_per_ray=256)
    r.close()
    return dict(row=row)


def step_batch(args):
    torch, r, hit, position, eye = _context()
    hit2, position2 = torch.zeros((H, W, 8), device="cuda:0"), torch.zeros((H, W, 4), device="cuda:0")
    rows = {}
    scratch = {M: torch.zeros((r.reflectLayout(M) // 4,), device="cuda:0") for M in BATCHES}
    acc = {M: dict(kernel_ms=[], trace_ms=[]) for M in BATCHES}
    st = {}
    for k in range(args.warmup + args.reps):  # the batch sizes take turns
        for M in BATCHES:
            st[M] = r.reflectPlanes(hit, position, hit2=hit2, position2=position2, scratch=scratch[M], bias=BIAS, max_distance=MAX_DISTANCE, max_rays_in_flight=M)["stats"]
            if k >= args.warmup:
                acc[M]["kernel_ms"].append(st[M]["kernel_ms"])
                acc[M]["trace_ms"].append(st[M]["trace_ms"])
    for M in BATCHES:
        rows[str(M)] = dict(kernel_ms=med(acc[M]["kernel_ms"]), trace_ms=med(acc[M]["trace_ms"]), batches=st[M]["batches"], scratch_bytes=int(scratch[M].numel() * 4),
                            traced=st[M]["traced"])
    r.close()
    return dict(rows=rows)


def markdown(res):
    x = res["pass"]["row"]
    md = ["## Timings (`tools/reflect_bench.py`)\n",
          f"{W} x {H}, one MI355X, the C3 terrain, a 1024 x 512 probe; medians over {res['reps']} calls after {res['warmup']} warm-up calls, the routes "
          "taking turns in one process.  `kernel_ms` is the pass's whole span, `trace_ms` its traversal launches; the existing route is "
          "`stage_ms + trace_ms + attrib_ms` of `traceDevice(any_hit=False)` over rays built with torch (torch's own time beside it, not in the sum).  "
          "Bytes a ray are ray and result traffic outside the traversal's reads.  No threshold is attached to any of these figures.\n",
          "| outputs | pass `kernel_ms` | pass `trace_ms` | route stage + trace + attrib | route stage / trace / attrib | torch build / scatter | rays traced | hit / escaped | pass scratch MB | route ray buffers MB | bytes a ray pass / route |",
          "|---|---|---|---|---|---|---|---|---|---|---|",
          f"| hit2, position2 | {x['kernel_ms']:.3f} | {x['trace_ms']:.3f} | {x['route_ms']:.3f} | {x['route_stage_ms']:.3f} / {x['route_trace_ms']:.3f} / {x['route_attrib_ms']:.3f} | "
          f"{x['torch_build_ms']:.3f} / {x['torch_scatter_ms']:.3f} | {x['traced']} | {x['hits']} / {x['escaped']} | {x['scratch_bytes'] / 1e6:.1f} | "
          f"{(x['route_ray_bytes'] + x['route_state_bytes']) / 1e6:.1f} | {x['pass_bytes_per_ray']} / {x['route_bytes_per_ray']} |",
          f"| hit2, position2, ray, sky | {x['all_kernel_ms']:.3f} | {x['all_trace_ms']:.3f} | | | | {x['traced']} | {x['hits']} / {x['escaped']} | {x['scratch_bytes'] / 1e6:.1f} | | |",
          "", "`max_rays_in_flight` (0: the default), hit2 and position2:\n", "| max_rays_in_flight | `kernel_ms` | `trace_ms` | batches | scratch MB |", "|---|---|---|---|---|"]
    for M, y in res["batch"]["rows"].items():
        md.append(f"| {M} | {y['kernel_ms']:.3f} | {y['trace_ms']:.3f} | {y['batches']} | {y['scratch_bytes'] / 1e6:.1f} |")
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
            raise SystemExit("reflect_bench: no GPU")
        print("RESULT " + json.dumps(dict(STEP_FUNCTIONS)[args.step](args)), flush=True)
        return 0
    res = dict(reps=args.reps, warmup=args.warmup)
    passed = ["--reps", str(args.reps), "--warmup", str(args.warmup)]
    for step, seconds in STEPS:  # one attempt each; the first failure ends the tool
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step] + passed, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"reflect_bench: step {step} ended with status {p.returncode}", file=sys.stderr)
            return p.returncode
        res[step] = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    print(json.dumps(res), flush=True)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        head = open(args.md).read().split("## Timings")[0] if os.path.exists(args.md) else "# Mirror reflections from the G-buffer (`pt_reflect_layout`, `pt_reflect_planes`)\n\n"
        with open(args.md, "w") as f:  # what the file says above its timing part stays
            f.write(head + markdown(res))
    return 0


STEP_FUNCTIONS = (("pass", step_pass), ("batch", step_batch))

if __name__ == "__main__":
    sys.exit(main())
