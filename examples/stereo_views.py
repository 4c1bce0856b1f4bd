#!/usr/bin/env python3
"""stereo_views.py — several cameras in ONE frame (setViews): a side-by-side stereo pair whose eyes sit an interocular distance apart, and an
8 x 8 atlas of cameras on an arc around the scene.  Each is one context, one copy of the scene, one wavefront batch per frame, and is written as
one image (binary PPM, or .npy with --npy).

  python3 examples/stereo_views.py [--eye-size 480 540] [--ipd 0.065] [--tile 128] [--spp 4] [--subframes 8] [--out-dir .]
                                   [--lens-warp [--k1 0.22 --k2 0.24 --chroma 0.015] [--late-yaw 1.5] [--bicubic]]

With --lens-warp the stereo pair is also written as a head-mounted display would be sent it (stereo_pair_warped): the linear frame is tone
mapped (tonemapPlanes), then lensWarpPlanes pre-distorts each eye around the centre of its own rectangle with the radial coefficients
--k1, --k2 — red and blue scaled by 1 - chroma and 1 + chroma, which is what cancels a lens's lateral colour fringes — and re-aims it from
the head pose it was rendered with to one turned by --late-yaw degrees (warpMatrix: rotational late reprojection).  Without the flag the
example is what it was.
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


def stereo_views(cam, ew, eh, ipd):
    """[(x, y, w, h, Camera)] of a side-by-side pair: both eyes look along the same direction, half the interocular distance to either side"""
    eye, lookat, up = (np.array(cam[k], np.float64) for k in ("eye", "lookat", "up"))
    fwd = (lookat - eye) / np.linalg.norm(lookat - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    views = []
    for i, side in enumerate((-0.5, 0.5)):
        off = right * (side * ipd)
        views.append((i * ew, 0, ew, eh, R.Camera(tuple(eye + off), tuple(lookat + off), tuple(up), cam["fovY"], ew / eh)))
    return views


def late_camera(c, yaw_deg):
    """the camera turned by yaw_deg about its up vector, around its own eye: the head pose at scan-out"""
    eye, lookat, up = (np.array(v, np.float64) for v in (c.eye, c.lookat, c.up))
    axis, t, d = up / np.linalg.norm(up), math.radians(yaw_deg), lookat - eye
    d = d * math.cos(t) + np.cross(axis, d) * math.sin(t) + axis * np.dot(axis, d) * (1.0 - math.cos(t))
    return R.Camera(c.eye, tuple(eye + d), c.up, c.fovY, c.aspectRatio)


def stereo_lenses(views, k1, k2, chroma, late_yaw):
    """one pt_lens_view per eye: the lens centre at the centre of the eye's rectangle, r = 1 at half its width, red and blue coefficients
    scaled by 1 -+ chroma, and the matrix from the rendered camera to the one turned by late_yaw degrees"""
    k = [(k1 * s, k2 * s, 0.0) for s in (1.0 - chroma, 1.0, 1.0 + chroma)]
    return [R.make_lens((w, h), k=k, warp=R.warpMatrix(c, late_camera(c, late_yaw), (w, h))) for _, _, w, h, c in views]


def warp_display(sample, lenses, bicubic=False):
    """the frame a head-mounted display is sent: the context's linear colour, tone mapped, then warped per eye.  Returns {"tonemapped":
    float32 (h, w, 4), "frame_rgba8": int32 (h, w), "stats": lensWarpPlanes's}."""
    import torch

    w, h = sample.launchParams.frame.size
    tonemapped = sample.tonemapPlanes(sample.deviceBuffer(R.PT_BUF_COLOR), op="reinhard")["out"]
    frame = torch.zeros((h, w), dtype=torch.int32, device=tonemapped.device)
    res = sample.lensWarpPlanes(tonemapped, frame=frame, lenses=lenses, bicubic=bicubic)
    return dict(tonemapped=tonemapped, frame_rgba8=frame, stats=res["stats"])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--eye-size", type=int, nargs=2, default=[480, 540], help="one eye's image; the width is rounded up to a multiple of 8")
    ap.add_argument("--ipd", type=float, default=0.065, help="interocular distance in scene units")
    ap.add_argument("--tile", type=int, default=128, help="edge of one atlas camera's image (a multiple of 8)")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--subframes", type=int, default=8)
    ap.add_argument("--out-dir", default=".")
    ap.add_argument("--npy", action="store_true")
    ap.add_argument("--lens-warp", action="store_true", help="also write the pair pre-distorted and late-reprojected for a headset (lensWarpPlanes)")
    ap.add_argument("--k1", type=float, default=0.22, help="radial coefficient of r^2 (r = 1 at half an eye's width)")
    ap.add_argument("--k2", type=float, default=0.24, help="radial coefficient of r^4")
    ap.add_argument("--chroma", type=float, default=0.015, help="red and blue coefficients are scaled by 1 - chroma and 1 + chroma")
    ap.add_argument("--late-yaw", type=float, default=1.5, help="degrees the head has turned between rendering and scan-out")
    ap.add_argument("--bicubic", action="store_true", help="Catmull-Rom taps instead of bilinear ones")
    args = ap.parse_args(argv)
    sample = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    sample.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    sample.launchParams.samples_per_launch = args.spp
    cam = scenes.TWO_BOX_CAMERA
    eye, lookat, up = (np.array(cam[k], np.float64) for k in ("eye", "lookat", "up"))

    # -- the stereo pair
    ew, eh = (args.eye_size[0] + 7) // 8 * 8, args.eye_size[1]
    views = stereo_views(cam, ew, eh, args.ipd)
    sample.resize((2 * ew, eh))
    sample.setViews(views)
    ms = _accumulate(sample, args.subframes)
    path = _save(os.path.join(args.out_dir, "stereo_pair"), sample.downloadPixels(), args.npy)
    print(f"stereo pair {2 * ew} x {eh}: {args.subframes} subframes of {sample.stats()['paths']} paths, {ms:.1f} ms on the device -> {path}")
    if args.lens_warp:
        shown = warp_display(sample, stereo_lenses(views, args.k1, args.k2, args.chroma, args.late_yaw), args.bicubic)
        st = shown["stats"]
        path = _save(os.path.join(args.out_dir, "stereo_pair_warped"), shown["frame_rgba8"].cpu().numpy().view(np.uint32), args.npy)
        print(f"  for the headset: k1 {args.k1}, k2 {args.k2}, chroma {args.chroma}, late yaw {args.late_yaw} deg: {st['outside']} of {st['pixels']} pixels "
              f"take the border colour, {st['kernel_ms']:.3f} ms on the device -> {path}")

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
