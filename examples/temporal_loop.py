#!/usr/bin/env python3
"""temporal_loop.py — a stereo pair that moves EVERY frame and still accumulates: reproject / accumulate / filter, all on the GPU.

Per frame: renderGBuffer gives hit, position and motion against LAST frame's cameras; render() gives this frame's samples;
temporalAccumulate reprojects last frame's accumulated colour along the motion plane, keeps it where the surface is the same and blends this
frame in with a per-pixel history length (disoccluded pixels start over, the others keep gaining samples); its copy_out goes straight into
the context's colour buffer, which denoise() filters.  History and length ping-pong between two pairs of tensors the application owns.

The colour handed to the pass is the per-frame colour recipe of include/pt_amd.h: frame k is rendered at subframe k (so the seeds differ
from frame to frame) into an accumulation buffer the previous pass left zeroed, and color_scale = k + 1 undoes the resolve's 1 / (k + 1).

  python3 examples/temporal_loop.py [--eye-size 480 540] [--ipd 0.065] [--frames 8] [--spp 1] [--out-dir .]
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
    # two sets of G-buffer planes (this frame's, last frame's) and two of history: everything is reused
    gbuf = [dict(hit=torch.zeros((h, w, 8), device=dev), position=torch.zeros((h, w, 4), device=dev), motion=torch.zeros((h, w, 2), device=dev)) for _ in range(2)]
    history = [torch.zeros((h, w, 4), device=dev) for _ in range(2)]
    length = [torch.zeros((h, w), device=dev) for _ in range(2)]  # 0 = no history: the first frame starts every pixel over
    for k in range(args.frames):
        prev, cams = cams, stereo_cameras(scenes.TWO_BOX_CAMERA, 0.01 * k, args.ipd, ew / eh)
        cur, old = gbuf[k & 1], gbuf[~k & 1]
        sample.setViewCameras(cams)  # the per-frame call: cameras only
        g = sample.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev, out=cur)
        sample.launchParams.frame.subframe_index = k
        sample.render()
        t = sample.temporalAccumulate(sample.deviceBuffer(R.PT_BUF_ACCUM), cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"],
                                      history[k & 1], length[k & 1], history_out=history[~k & 1], length_out=length[~k & 1],
                                      copy_out=sample.deviceBuffer(R.PT_BUF_COLOR), color_scale=float(k + 1), clear_color=True, max_history=args.max_history)
        _, denoise_ms = sample.denoise(input=R.PT_BUF_COLOR)
        n = length[~k & 1]
        print(f"frame {k}: G-buffer {g['stats']['kernel_ms']:.3f} ms, colour {sample.stats()['render_ms']:.2f} ms, temporal {t['stats']['kernel_ms']:.3f} ms, "
              f"filter {denoise_ms:.3f} ms; {t['stats']['reprojected']} of {t['stats']['pixels']} pixels kept their history, "
              f"mean length {float(n.sum()) / max(1, t['stats']['pixels']):.2f}, longest {int(n.max())}")
    np.save(os.path.join(args.out_dir, "temporal_history.npy"), history[args.frames & 1].cpu().numpy())
    np.save(os.path.join(args.out_dir, "temporal_length.npy"), length[args.frames & 1].cpu().numpy())
    np.save(os.path.join(args.out_dir, "temporal_denoised.npy"), sample.download(R.PT_BUF_DENOISED))
    print(f"wrote temporal_history.npy, temporal_length.npy and temporal_denoised.npy to {args.out_dir}")
    sample.close()


if __name__ == "__main__":
    main()
