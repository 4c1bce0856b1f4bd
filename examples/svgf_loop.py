#!/usr/bin/env python3
"""svgf_loop.py — the stereo loop of temporal_loop.py with the chain's own filter at its end: reproject / accumulate / filter, per eye.

Per frame: renderGBuffer gives hit, position and motion against LAST frame's cameras; render() gives this frame's samples.  Three
temporalAccumulate calls follow, all with the same motion, hit and position planes:
  1. the per-frame colour recipe of include/pt_amd.h against an EMPTY history (length 0 everywhere): its history_out is this frame's own
     colour, accumulation * (k + 1), as a tensor; the accumulation buffer is left zeroed for the next frame;
  2. the colour history: that tensor blended into last frame's accumulated colour;
  3. the moments history: the plane (lum, lum^2, 0, 1) of that tensor blended into last frame's moments.
The variance plane is max(0, m2 - m1^2) of the reprojected moments, and filterPlanes filters the accumulated colour with it: guided by the
exact hit and position planes, inside each eye's rectangle only (temporal_loop.py's denoise() lets the left eye bleed into the right at the
seam), and with the 7x7 spatial estimate where a pixel was disoccluded fewer than --min-length frames ago.

  python3 examples/svgf_loop.py [--eye-size 480 540] [--ipd 0.065] [--frames 8] [--spp 1] [--out-dir .]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from optixpathtracer_amd import renderer as R  # noqa: E402
from optixpathtracer_amd import scenes  # noqa: E402

from gbuffer_views import stereo_cameras  # noqa: E402  (examples/gbuffer_views.py: the head on its arc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eye-size", type=int, nargs=2, default=[480, 540], help="one eye's image; the width is rounded up to a multiple of 8")
    ap.add_argument("--ipd", type=float, default=0.065, help="interocular distance in scene units")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--max-history", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--sigma-lum", type=float, default=4.0)
    ap.add_argument("--min-length", type=int, default=4)
    ap.add_argument("--out-dir", default=".")
    args = ap.parse_args()
    import torch

    dev = "cuda:0"
    sample = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    sample.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    sample.launchParams.samples_per_launch = args.spp
    ew, eh = (args.eye_size[0] + 7) // 8 * 8, args.eye_size[1]
    w, h = 2 * ew, eh
    sample.resize((w, h))
    cams = stereo_cameras(scenes.TWO_BOX_CAMERA, 0.0, args.ipd, ew / eh)
    sample.setViews([(i * ew, 0, ew, eh, c) for i, c in enumerate(cams)])
    sample.uploadAccum(np.zeros((h, w, 4), np.float32))

    def planes(k):
        return torch.zeros((h, w, k) if k > 1 else (h, w), device=dev)

    # two sets of G-buffer planes (this frame's, last frame's), two of colour history, two of moments history: everything is reused
    gbuf = [dict(hit=planes(8), position=planes(4), motion=planes(2)) for _ in range(2)]
    history, moments, length = [planes(4) for _ in range(2)], [planes(4) for _ in range(2)], [planes(1) for _ in range(2)]
    colour, one, none4, none1, length_m = planes(4), planes(1), planes(4), planes(1), planes(1)  # none*: the empty history of call 1
    filtered, scratch = planes(4), planes(4)
    frame = torch.zeros((h, w), dtype=torch.int32, device=dev)
    for k in range(args.frames):
        prev, cams = cams, stereo_cameras(scenes.TWO_BOX_CAMERA, 0.01 * k, args.ipd, ew / eh)
        cur, old = gbuf[k & 1], gbuf[~k & 1]
        i, o = k & 1, ~k & 1
        sample.setViewCameras(cams)  # the per-frame call: cameras only
        g = sample.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev, out=cur)
        sample.launchParams.frame.subframe_index = k
        sample.render()
        geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"])
        sample.temporalAccumulate(sample.deviceBuffer(R.PT_BUF_ACCUM), *geo, none4, none1, history_out=colour, length_out=one,
                                  color_scale=float(k + 1), clear_color=True)
        t = sample.temporalAccumulate(colour, *geo, history[i], length[i], history_out=history[o], length_out=length[o], max_history=args.max_history)
        lum = (0.2126 * colour[..., 0] + 0.7152 * colour[..., 1]) + 0.0722 * colour[..., 2]
        mom = torch.stack([lum, lum * lum, torch.zeros_like(lum), torch.ones_like(lum)], -1).contiguous()
        sample.temporalAccumulate(mom, *geo, moments[i], length[i], history_out=moments[o], length_out=length_m, max_history=args.max_history)
        m1, m2 = moments[o][..., 0], moments[o][..., 1]
        variance = torch.clamp_min(m2 - m1 * m1, 0.0).contiguous()
        f = sample.filterPlanes(history[o], cur["hit"], cur["position"], variance=variance, length=length[o], out=filtered, scratch=scratch, frame=frame,
                                iterations=args.iterations, sigma_lum=args.sigma_lum, min_length=args.min_length)
        n = length[o]
        fs, ts = f["stats"], t["stats"]
        print(f"frame {k}: G-buffer {g['stats']['kernel_ms']:.3f} ms, colour {sample.stats()['render_ms']:.2f} ms, temporal {ts['kernel_ms']:.3f} ms, "
              f"filter {fs['kernel_ms']:.3f} ms; {ts['reprojected']} of {ts['pixels']} pixels kept their history, mean length "
              f"{float(n.sum()) / max(1, ts['pixels']):.2f}; {fs['filtered']} pixels filtered, {fs['spatial']} with the spatial variance estimate")
    np.save(os.path.join(args.out_dir, "svgf_history.npy"), history[args.frames & 1].cpu().numpy())
    np.save(os.path.join(args.out_dir, "svgf_filtered.npy"), filtered.cpu().numpy())
    np.save(os.path.join(args.out_dir, "svgf_frame.npy"), frame.cpu().numpy().view(np.uint32))
    print(f"wrote svgf_history.npy, svgf_filtered.npy and svgf_frame.npy to {args.out_dir}")
    sample.close()


if __name__ == "__main__":
    main()
