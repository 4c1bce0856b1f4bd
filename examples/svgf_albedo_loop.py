#!/usr/bin/env python3
"""svgf_albedo_loop.py — the SVGF loop with the library's own temporal stage: demodulate, reproject colour and moments in one pass, clamp
the history, filter the demodulated colour, modulate the albedo back in.

svgf_loop.py assembles the temporal side from three temporalAccumulate calls and torch kernels; here it is one call.  Per frame, on the
textured scene (a textured ground quad and a textured tilted quad: the detail the filter must not blur):
  1. renderGBuffer: hit, position and motion against LAST frame's camera;
  2. render(): this frame's samples, into the accumulation buffer, and the first-hit albedo (PT_BUF_ALBEDO);
  3. temporalMoments with PT_BUF_ACCUM as the colour (color_scale = k + 1 and the clear flag: the per-frame colour recipe of
     include/pt_amd.h) and PT_BUF_ALBEDO as the albedo: demodulated history, moments, history length and variance, the history clamped to
     the 3x3 neighbourhood of this frame's demodulated colour;
  4. filterPlanes on the demodulated history with that variance and length;
  5. modulatePlanes: the albedo multiplied back in, float and RGBA8.

  python3 examples/svgf_albedo_loop.py [--size 960 540] [--frames 8] [--spp 1] [--clamp-k 1.5] [--out-dir .]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from optixpathtracer_amd import renderer as R  # noqa: E402
from optixpathtracer_amd import scenes  # noqa: E402


def orbit(cam, angle):
    """the camera turned by `angle` radians about the vertical axis through its look-at point"""
    e, l = np.asarray(cam["eye"], np.float64), np.asarray(cam["lookat"], np.float64)
    d = e - l
    c, s = np.cos(angle), np.sin(angle)
    return dict(cam, eye=(float(l[0] + c * d[0] + s * d[2]), float(e[1]), float(l[2] - s * d[0] + c * d[2])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[960, 540])
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--max-history", type=int, default=32)
    ap.add_argument("--clamp-k", type=float, default=1.5, help="half-width of the history clamp in standard deviations of the 3x3 window")
    ap.add_argument("--albedo-min", type=float, default=0.01)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--sigma-lum", type=float, default=4.0)
    ap.add_argument("--min-length", type=int, default=4)
    ap.add_argument("--out-dir", default=".")
    args = ap.parse_args()
    import torch

    dev = "cuda:0"
    w, h = args.size
    sample = R.SampleRenderer(scenes.textured_scene())
    sample.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    sample.launchParams.samples_per_launch = args.spp
    sample.resize((w, h))
    sample.uploadAccum(np.zeros((h, w, 4), np.float32))

    def planes(k):
        return torch.zeros((h, w, k) if k > 1 else (h, w), device=dev)

    # two sets of G-buffer planes (this frame's, last frame's), two of history, moments and length: everything is reused
    gbuf = [dict(hit=planes(8), position=planes(4), motion=planes(2)) for _ in range(2)]
    history, moments, length = [planes(4) for _ in range(2)], [planes(2) for _ in range(2)], [planes(1) for _ in range(2)]
    variance, filtered, scratch, final = planes(1), planes(4), planes(4), planes(4)
    frame = torch.zeros((h, w), dtype=torch.int32, device=dev)
    accum, albedo = sample.deviceBuffer(R.PT_BUF_ACCUM), sample.deviceBuffer(R.PT_BUF_ALBEDO)
    cam = R.make_camera(scenes.TWO_BOX_CAMERA, w / h)
    for k in range(args.frames):
        prev, cam = cam, R.make_camera(orbit(scenes.TWO_BOX_CAMERA, 0.01 * k), w / h)
        cur, old = gbuf[k & 1], gbuf[~k & 1]
        i, o = k & 1, ~k & 1
        sample.setCamera(cam)
        g = sample.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev, out=cur)
        sample.launchParams.frame.subframe_index = k
        sample.render()
        t = sample.temporalMoments(accum, cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], history[i], moments[i], length[i],
                                   albedo=albedo, history_out=history[o], moments_out=moments[o], length_out=length[o], variance_out=variance,
                                   color_scale=float(k + 1), albedo_min=args.albedo_min, clamp_k=args.clamp_k, max_history=args.max_history,
                                   clear_color=True)
        f = sample.filterPlanes(history[o], cur["hit"], cur["position"], variance=variance, length=length[o], out=filtered, scratch=scratch,
                                iterations=args.iterations, sigma_lum=args.sigma_lum, min_length=args.min_length)
        m = sample.modulatePlanes(filtered, albedo=albedo, out=final, frame=frame, albedo_min=args.albedo_min)
        ts, fs, ms = t["stats"], f["stats"], m["stats"]
        print(f"frame {k}: G-buffer {g['stats']['kernel_ms']:.3f} ms, colour {sample.stats()['render_ms']:.2f} ms, temporal {ts['kernel_ms']:.3f} ms, "
              f"filter {fs['kernel_ms']:.3f} ms, modulate {ms['kernel_ms']:.3f} ms; {ts['reprojected']} of {ts['pixels']} pixels kept their history, "
              f"{ts['clamped']} of those were clamped; {fs['filtered']} pixels filtered, {fs['spatial']} with the spatial variance estimate")
    np.save(os.path.join(args.out_dir, "svgf_albedo_history.npy"), history[args.frames & 1].cpu().numpy())
    np.save(os.path.join(args.out_dir, "svgf_albedo_final.npy"), final.cpu().numpy())
    np.save(os.path.join(args.out_dir, "svgf_albedo_frame.npy"), frame.cpu().numpy().view(np.uint32))
    print(f"wrote svgf_albedo_history.npy, svgf_albedo_final.npy and svgf_albedo_frame.npy to {args.out_dir}")
    sample.close()


if __name__ == "__main__":
    main()
