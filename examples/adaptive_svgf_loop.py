#!/usr/bin/env python3
"""adaptive_svgf_loop.py — the SVGF loop of a moving camera that path-traces only the blocks that need samples.

svgf_albedo_loop.py renders every pixel every frame.  After a few frames of an orbit almost every pixel has a long, valid history, and new
samples are needed only where the history was lost, where it is short and where the accumulated estimate is still noisy.  Per frame:
  1. renderGBuffer: hit, position and motion against LAST frame's camera;
  2. samplePlan: the 8x8 blocks that need samples, from the reprojected moments and history lengths (and a slow refresh of all blocks);
  3. renderMask(mask): this frame's samples for those blocks only, into the accumulation buffer;
  4. temporalMoments on the mask with PT_BUF_ACCUM as the colour (color_scale = k + 1 and the clear flag: the per-frame colour recipe of
     include/pt_amd.h): history, moments, length and variance of the sampled blocks;
  5. temporalCarry on the mask's complement: history, moments and length of the other blocks, reprojected and carried unchanged;
  6. filterPlanes on all pixels.
No albedo: PT_BUF_ALBEDO is written by the render, so in a block that was not rendered it holds the first-hit albedo of an older camera;
demodulating or remodulating with it would be wrong (include/pt_amd.h).  The loop therefore filters the colour itself.

  python3 examples/adaptive_svgf_loop.py [--size 960 540] [--frames 16] [--spp 1] [--threshold 0.25] [--refresh 16] [--out-dir .]
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
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--max-history", type=int, default=32)
    ap.add_argument("--threshold", type=float, default=0.25, help="the relative standard error a pixel's accumulated luminance may keep")
    ap.add_argument("--dark-floor", type=float, default=0.05)
    ap.add_argument("--plan-min-length", type=int, default=4, help="a history shorter than this always asks for samples")
    ap.add_argument("--min-pixels", type=int, default=8, help="short or noisy pixels that make a block sampled")
    ap.add_argument("--refresh", type=int, default=16, help="every block is sampled once in this many frames; 0: no refresh")
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--sigma-lum", type=float, default=4.0)
    ap.add_argument("--min-length", type=int, default=4)
    ap.add_argument("--out-dir", default=".")
    args = ap.parse_args()
    import torch

    dev = "cuda:0"
    w, h = args.size
    sample = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    sample.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    sample.launchParams.samples_per_launch = args.spp
    sample.resize((w, h))
    sample.uploadAccum(np.zeros((h, w, 4), np.float32))

    def planes(k):
        return torch.zeros((h, w, k) if k > 1 else (h, w), device=dev)

    # two sets of G-buffer planes (this frame's, last frame's), two of history, moments and length: everything is reused
    gbuf = [dict(hit=planes(8), position=planes(4), motion=planes(2)) for _ in range(2)]
    history, moments, length = [planes(4) for _ in range(2)], [planes(2) for _ in range(2)], [planes(1) for _ in range(2)]
    variance, filtered, scratch = planes(1), planes(4), planes(4)
    frame = torch.zeros((h, w), dtype=torch.int32, device=dev)
    accum = sample.deviceBuffer(R.PT_BUF_ACCUM)
    cam = R.make_camera(scenes.TWO_BOX_CAMERA, w / h)
    for k in range(args.frames):
        prev, cam = cam, R.make_camera(orbit(scenes.TWO_BOX_CAMERA, 0.01 * k), w / h)
        cur, old = gbuf[k & 1], gbuf[~k & 1]
        i, o = k & 1, ~k & 1
        sample.setCamera(cam)
        g = sample.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev, out=cur)
        geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], history[i], moments[i], length[i])
        outs = dict(history_out=history[o], moments_out=moments[o], length_out=length[o], variance_out=variance)
        p = sample.samplePlan(*geo, threshold=args.threshold, dark_floor=args.dark_floor, min_length=args.plan_min_length, min_pixels=args.min_pixels,
                              refresh_period=args.refresh, frame_index=k)
        mask = p["mask"]
        sample.launchParams.frame.subframe_index = k
        rendered = sample.renderMask(mask)
        t = sample.temporalMoments(accum, *geo, **outs, mask=mask, color_scale=float(k + 1), max_history=args.max_history, clear_color=True)
        c = sample.temporalCarry(*geo, **outs, mask=mask == 0)
        assert c["stats"]["lost"] == 0  # the plan samples every block that holds a pixel the carry could not carry
        f = sample.filterPlanes(history[o], cur["hit"], cur["position"], variance=variance, length=length[o], out=filtered, scratch=scratch, frame=frame,
                                iterations=args.iterations, sigma_lum=args.sigma_lum, min_length=args.min_length)
        ps, ts, cs, fs = p["stats"], t["stats"], c["stats"], f["stats"]
        print(f"frame {k}: {ps['sampled']} of {ps['blocks']} blocks sampled ({ps['by_lost']} lost a pixel, {ps['by_need']} short or noisy, "
              f"{ps['by_refresh']} refreshed), {rendered} pixels rendered, {cs['carried']} carried; G-buffer {g['stats']['kernel_ms']:.3f} ms, "
              f"plan {ps['kernel_ms']:.3f} ms, colour {sample.stats()['render_ms']:.2f} ms, temporal {ts['kernel_ms']:.3f} ms, "
              f"carry {cs['kernel_ms']:.3f} ms, filter {fs['kernel_ms']:.3f} ms")
    np.save(os.path.join(args.out_dir, "adaptive_svgf_history.npy"), history[args.frames & 1].cpu().numpy())
    np.save(os.path.join(args.out_dir, "adaptive_svgf_filtered.npy"), filtered.cpu().numpy())
    np.save(os.path.join(args.out_dir, "adaptive_svgf_frame.npy"), frame.cpu().numpy().view(np.uint32))
    print(f"wrote adaptive_svgf_history.npy, adaptive_svgf_filtered.npy and adaptive_svgf_frame.npy to {args.out_dir}")
    sample.close()


if __name__ == "__main__":
    main()
