#!/usr/bin/env python3
"""moving_geometry_loop.py — the reproject / accumulate / filter chain over geometry that moves: the box of the two-box scene turns and bobs
under transformMeshes while the camera travels on an arc, and the history follows the box.

Per frame, in this order:
  1. snapshot:       copyVerticesDevice — the vertices as the LAST frame saw them (one device-to-device copy, ping-ponged by the caller)
  2. transform:      transformMeshes moves the box from its rest pose (a refit of the tree)
  3. render:         this frame's samples
  4. G-buffer:       hit, position and the camera-only motion against last frame's camera
  5. motion planes:  motionPlanes(hit, snapshot) — where each pixel's surface point was: motion, prev_point, prev_surface
  6. temporal:       temporalAccumulate(hit=prev_surface, position=prev_point, motion=motion), prev_hit / prev_position last frame's G-buffer
  7. filter:         filterPlanes with the CURRENT hit and position
  8. motion blur:    (--motion-blur) motionBlurPlanes(filtered, the motion of step 5, the G-buffer's depth), so the moved box blurs, then
                     tonemapPlanes into the displayed frame
A second history is kept with the camera-only planes of step 4, on the same colour, and the share of pixels that kept their history is
printed for both routes: on the box the camera-only route loses it every frame (the plane test fails where the surface moved along its
normal) or keeps the history of another surface point (a face sliding in its own plane).

  python3 examples/moving_geometry_loop.py [--size 640 360] [--frames 8] [--spp 1] [--out-dir .] [--motion-blur [--shutter 0.5] [--blur-taps 12]]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from optixpathtracer_amd import renderer as R  # noqa: E402
from optixpathtracer_amd import scenes  # noqa: E402


def box_pose(k):
    """the box's 3x4 matrix at frame k: a turn about the vertical axis through its centre and a bob along it"""
    a, lift = 0.06 * k, 0.08 * np.sin(0.7 * k)
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s, 0], [0, 1, 0, lift], [-s, 0, c, 0]], np.float32)


def camera(k, aspect):
    ex, ey, ez = scenes.TWO_BOX_CAMERA["eye"]
    a = 0.01 * k
    return R.make_camera(dict(scenes.TWO_BOX_CAMERA, eye=(ex * np.cos(a) - ez * np.sin(a), ey, ex * np.sin(a) + ez * np.cos(a))), aspect)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[640, 360])
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--max-history", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--out-dir", default=".")
    ap.add_argument("--motion-blur", action="store_true", help="blur the filtered colour along the motion planes' motion (motionBlurPlanes)")
    ap.add_argument("--shutter", type=float, default=0.5, help="the open fraction of the frame interval, in [0, 4]")
    ap.add_argument("--blur-taps", type=int, default=12)
    args = ap.parse_args()
    import torch

    dev = "cuda:0"
    w, h = args.size
    sample = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    sample.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    sample.launchParams.samples_per_launch = args.spp
    sample.resize((w, h))
    sample.uploadAccum(np.zeros((h, w, 4), np.float32))
    box = 0  # the unit box is mesh 0, the ground mesh 1

    def planes(k):
        return torch.zeros((h, w, k) if k > 1 else (h, w), device=dev)

    gplanes = ("hit", "position", "motion") + (("depth",) if args.motion_blur else ())
    gbuf = [dict(hit=planes(8), position=planes(4), motion=planes(2), **(dict(depth=planes(1)) if args.motion_blur else {})) for _ in range(2)]
    blurred = planes(4) if args.motion_blur else None
    blur_scratch = torch.zeros((sample.motionBlurLayout()[1] // 8, 2), device=dev) if args.motion_blur else None
    mot = dict(motion=planes(2), prev_point=planes(4), prev_surface=planes(8))
    snapshot = torch.zeros((sample.vertexCount()[0], 3), device=dev)
    # two histories on the same colour: [0] with the object motion, [1] camera-only
    history = [[planes(4) for _ in range(2)] for _ in range(2)]
    length = [[planes(1) for _ in range(2)] for _ in range(2)]
    colour, one, none4, none1 = planes(4), planes(1), planes(4), planes(1)
    filtered, scratch = planes(4), planes(4)
    frame = torch.zeros((h, w), dtype=torch.int32, device=dev)
    cam = camera(0, w / h)
    for k in range(args.frames):
        prev_cam, cam = cam, camera(k, w / h)
        cur, old = gbuf[k & 1], gbuf[~k & 1]
        i, o = k & 1, ~k & 1
        sample.copyVerticesDevice(out=snapshot)                                         # 1
        refit_ms = sample.transformMeshes({box: box_pose(k)})                           # 2
        sample.setCamera(cam)
        sample.launchParams.frame.subframe_index = k
        sample.render()                                                                 # 3
        g = sample.renderGBuffer(gplanes, prev_cameras=prev_cam, out=cur)               # 4
        m = sample.motionPlanes(cur["hit"], snapshot, prev_cameras=prev_cam, out=mot)   # 5
        # this frame's own colour as a tensor (the per-frame colour recipe of include/pt_amd.h against an empty history)
        sample.temporalAccumulate(sample.deviceBuffer(R.PT_BUF_ACCUM), cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], none4, none1,
                                  history_out=colour, length_out=one, color_scale=float(k + 1), clear_color=True)
        t = sample.temporalAccumulate(colour, mot["motion"], mot["prev_surface"], mot["prev_point"], old["hit"], old["position"], history[0][i], length[0][i],
                                      history_out=history[0][o], length_out=length[0][o], max_history=args.max_history)             # 6
        t0 = sample.temporalAccumulate(colour, cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], history[1][i], length[1][i],
                                       history_out=history[1][o], length_out=length[1][o], max_history=args.max_history)
        f = sample.filterPlanes(history[0][o], cur["hit"], cur["position"], length=length[0][o], out=filtered, scratch=scratch, frame=frame,
                                iterations=args.iterations)                                                                         # 7
        if args.motion_blur:                                                                                                        # 8
            b = sample.motionBlurPlanes(filtered, mot["motion"], cur["depth"], out=blurred, scratch=blur_scratch, shutter=args.shutter, taps=args.blur_taps)
            sample.tonemapPlanes(blurred, frame=frame, op="reinhard", write_out=False)
            bs = b["stats"]
            print(f"frame {k}: motion blur {bs['kernel_ms']:.3f} ms, {100.0 * bs['moving'] / max(1, bs['pixels']):.1f} % of the pixels gather, "
                  f"{bs['taps'] / max(1, bs['moving']):.1f} taps each count, {bs['unknown']} pixels without a motion")
        on_box = cur["hit"].view(torch.int32)[..., 4] == box
        nbox = max(1, int(on_box.sum()))
        kept = [int((length[j][o][on_box] >= 2).sum()) for j in (0, 1)]
        ts, t0s, ms = t["stats"], t0["stats"], m["stats"]
        print(f"frame {k}: refit {refit_ms:.3f} ms, G-buffer {g['stats']['kernel_ms']:.3f} ms, motion planes {ms['kernel_ms']:.3f} ms, temporal {ts['kernel_ms']:.3f} ms, "
              f"filter {f['stats']['kernel_ms']:.3f} ms; reprojected {100.0 * ts['reprojected'] / ts['pixels']:.1f} % of the frame with the motion planes, "
              f"{100.0 * t0s['reprojected'] / t0s['pixels']:.1f} % camera-only; on the box ({nbox} pixels) {100.0 * kept[0] / nbox:.1f} % against {100.0 * kept[1] / nbox:.1f} %")
    np.save(os.path.join(args.out_dir, "moving_history.npy"), history[0][args.frames & 1].cpu().numpy())
    np.save(os.path.join(args.out_dir, "moving_filtered.npy"), filtered.cpu().numpy())
    np.save(os.path.join(args.out_dir, "moving_frame.npy"), frame.cpu().numpy().view(np.uint32))
    if args.motion_blur:
        np.save(os.path.join(args.out_dir, "moving_blurred.npy"), blurred.cpu().numpy())
    print(f"wrote moving_history.npy, moving_filtered.npy{', moving_blurred.npy' if args.motion_blur else ''} and moving_frame.npy to {args.out_dir}")
    sample.close()


if __name__ == "__main__":
    main()
