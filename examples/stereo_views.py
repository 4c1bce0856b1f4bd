#!/usr/bin/env python3
"""stereo_views.py — several cameras in ONE frame (setViews): a side-by-side stereo pair whose eyes sit an interocular distance apart, and an
8 x 8 atlas of cameras on an arc around the scene.  Each is one context, one copy of the scene, one wavefront batch per frame, and is written as
one image (binary PPM, or .npy with --npy).

  python3 examples/stereo_views.py [--eye-size 480 540] [--ipd 0.065] [--tile 128] [--spp 4] [--subframes 8] [--out-dir .]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from optixpathtracer_amd import renderer as R  # noqa: E402
from optixpathtracer_amd import scenes  # noqa: E402


def _save(path, rgba8, npy):
    if npy:
        np.save(path + ".npy", rgba8)
        return path + ".npy"
    h, w = rgba8.shape
    rgb = rgba8.view(np.uint8).reshape(h, w, 4)[::-1, :, :3]  # row 0 of the frame buffer is the bottom row of the image
    with open(path + ".ppm", "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(rgb).tobytes())
    return path + ".ppm"


def _accumulate(sample, subframes):
    ms = 0.0
    for k in range(subframes):
        sample.launchParams.frame.subframe_index = k
        sample.render()
        ms += sample.stats()["render_ms"]
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eye-size", type=int, nargs=2, default=[480, 540], help="one eye's image; the width is rounded up to a multiple of 8")
    ap.add_argument("--ipd", type=float, default=0.065, help="interocular distance in scene units")
    ap.add_argument("--tile", type=int, default=128, help="edge of one atlas camera's image (a multiple of 8)")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--subframes", type=int, default=8)
    ap.add_argument("--out-dir", default=".")
    ap.add_argument("--npy", action="store_true")
    args = ap.parse_args()
    sample = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    sample.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    sample.launchParams.samples_per_launch = args.spp
    cam = scenes.TWO_BOX_CAMERA
    eye, lookat, up = (np.array(cam[k], np.float64) for k in ("eye", "lookat", "up"))

    # -- the stereo pair: both eyes look along the same direction, half the interocular distance to either side
    ew, eh = (args.eye_size[0] + 7) // 8 * 8, args.eye_size[1]
    fwd = (lookat - eye) / np.linalg.norm(lookat - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    views = []
    for i, side in enumerate((-0.5, 0.5)):
        off = right * (side * args.ipd)
        views.append((i * ew, 0, ew, eh, R.Camera(tuple(eye + off), tuple(lookat + off), tuple(up), cam["fovY"], ew / eh)))
    sample.resize((2 * ew, eh))
    sample.setViews(views)
    ms = _accumulate(sample, args.subframes)
    path = _save(os.path.join(args.out_dir, "stereo_pair"), sample.downloadPixels(), args.npy)
    print(f"stereo pair {2 * ew} x {eh}: {args.subframes} subframes of {sample.stats()['paths']} paths, {ms:.1f} ms on the device -> {path}")

    # -- the camera atlas: 64 cameras on an arc around the look-at point, each in its own tile (resize drops the views: set them after it)
    t = (args.tile + 7) // 8 * 8
    radius = np.linalg.norm((eye - lookat)[[0, 2]])
    views = []
    for i in range(64):
        a = math.atan2(eye[2] - lookat[2], eye[0] - lookat[0]) + (i / 63.0 - 0.5) * math.pi
        e = (lookat[0] + radius * math.cos(a), eye[1] + 0.5 * (i // 8 - 3.5) * 0.2, lookat[2] + radius * math.sin(a))
        views.append(((i % 8) * t, (i // 8) * t, t, t, R.Camera(e, tuple(lookat), tuple(up), cam["fovY"], 1.0)))
    sample.resize((8 * t, 8 * t))
    sample.setViews(views)
    ms = _accumulate(sample, args.subframes)
    path = _save(os.path.join(args.out_dir, "camera_atlas"), sample.downloadPixels(), args.npy)
    print(f"camera atlas {8 * t} x {8 * t}, 64 views: {args.subframes} subframes of {sample.stats()['paths']} paths, {ms:.1f} ms on the device -> {path}")
    sample.close()


if __name__ == "__main__":
    main()
