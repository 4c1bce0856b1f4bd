#!/usr/bin/env python3
"""gbuffer_views.py — colour AND first-hit data for a stereo pair that moves (setViews + renderGBuffer).  Per frame the head moves along a small
arc; the colour image comes from render(), then depth, ids and screen-space motion against LAST frame's cameras come from renderGBuffer into
GPU tensors — what a reprojection step or a synthetic-data writer consumes.  One context, one copy of the scene, nothing staged on the host.

  python3 examples/gbuffer_views.py [--eye-size 480 540] [--ipd 0.065] [--frames 4] [--spp 2] [--out-dir .]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from optixpathtracer_amd import renderer as R  # noqa: E402
from optixpathtracer_amd import scenes  # noqa: E402


def stereo_cameras(cam, angle, ipd, aspect):
    """both eyes of a head that has turned by `angle` around the look-at point, half the interocular distance to either side"""
    eye, lookat, up = (np.array(cam[k], np.float64) for k in ("eye", "lookat", "up"))
    c, s = math.cos(angle), math.sin(angle)
    d = eye - lookat
    eye = lookat + np.array([c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]])
    fwd = (lookat - eye) / np.linalg.norm(lookat - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    return [R.Camera(tuple(eye + right * (side * ipd)), tuple(lookat + right * (side * ipd)), tuple(up), cam["fovY"], aspect) for side in (-0.5, 0.5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eye-size", type=int, nargs=2, default=[480, 540], help="one eye's image; the width is rounded up to a multiple of 8")
    ap.add_argument("--ipd", type=float, default=0.065, help="interocular distance in scene units")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--out-dir", default=".")
    args = ap.parse_args()
    import torch

    sample = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    sample.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    sample.launchParams.samples_per_launch = args.spp
    ew, eh = (args.eye_size[0] + 7) // 8 * 8, args.eye_size[1]
    sample.resize((2 * ew, eh))
    cams = stereo_cameras(scenes.TWO_BOX_CAMERA, 0.0, args.ipd, ew / eh)
    sample.setViews([(i * ew, 0, ew, eh, c) for i, c in enumerate(cams)])
    # the planes live in tensors the application owns and are reused every frame
    planes = dict(hit=torch.zeros((eh, 2 * ew, 8), device="cuda:0"), depth=torch.zeros((eh, 2 * ew), device="cuda:0"), motion=torch.zeros((eh, 2 * ew, 2), device="cuda:0"))
    for k in range(args.frames):
        prev, cams = cams, stereo_cameras(scenes.TWO_BOX_CAMERA, 0.01 * k, args.ipd, ew / eh)
        sample.setViewCameras(cams)  # the per-frame call: cameras only
        sample.launchParams.frame.subframe_index = 0  # the head moved: the accumulation starts over
        sample.render()
        g = sample.renderGBuffer(("hit", "depth", "motion"), prev_cameras=prev, out=planes)
        ids = planes["hit"].view(torch.int32)
        hit = ids[..., 3] >= 0
        seen = torch.isfinite(planes["motion"][..., 0]) & hit
        speed = planes["motion"][seen].norm(dim=1)
        print(f"frame {k}: {sample.stats()['render_ms']:.2f} ms colour, {g['stats']['kernel_ms']:.3f} ms G-buffer; {g['stats']['hits']} of {g['stats']['pixels']} pixels hit, "
              f"{int(ids[..., 4][hit].unique().numel())} meshes, depth {float(planes['depth'][hit].min()):.2f} .. {float(planes['depth'][hit].max()):.2f}, "
              f"motion mean {float(speed.mean()) if speed.numel() else 0.0:.3f} px, max {float(speed.max()) if speed.numel() else 0.0:.3f} px")
    np.save(os.path.join(args.out_dir, "gbuffer_color.npy"), sample.downloadPixels())
    for name, t in planes.items():
        np.save(os.path.join(args.out_dir, f"gbuffer_{name}.npy"), t.cpu().numpy())
    print(f"wrote gbuffer_color.npy and gbuffer_{{hit,depth,motion}}.npy to {args.out_dir}")
    sample.close()


if __name__ == "__main__":
    main()
