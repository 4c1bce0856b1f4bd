#!/usr/bin/env python3
"""adaptive_loop.py — the progressive loop of the reference's application (render, display, subframe_index++ until the camera moves) with
adaptive stopping: every 8x8 block stops being rendered once the standard error of its pixels' means is at most `threshold` of the block's mean
luminance, and the loop ends when no block is left (or after --max-subframes).

  python3 examples/adaptive_loop.py [--size 960 540] [--spp 2] [--threshold 0.03] [--max-subframes 256] [--out frame.npy]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from optixpathtracer_amd import renderer as R  # noqa: E402
from optixpathtracer_amd import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[960, 540])
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.03)
    ap.add_argument("--max-subframes", type=int, default=256)
    ap.add_argument("--out", default=None, help="write the rgba8 frame as a .npy file")
    args = ap.parse_args()
    w, h = args.size
    sample = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
    sample.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    sample.resize((w, h))
    sample.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, w / h))
    sample.launchParams.samples_per_launch = args.spp

    # after every camera move: restart the accumulation AND the adaptive state
    sample.launchParams.frame.subframe_index = 0
    sample.adaptiveBegin(threshold=args.threshold, dark_floor=0.01, min_subframes=8, max_subframes=args.max_subframes)
    pixels = np.zeros((h, w), np.uint32)
    device_ms = 0.0
    while True:
        st = sample.renderAdaptive(pixels)  # `pixels` is what a display would show: stopped blocks keep their last value
        device_ms += sample.stats()["render_ms"]
        sample.launchParams.frame.subframe_index += 1
        k = sample.launchParams.frame.subframe_index
        if k % 16 == 0 or st["active_blocks"] == 0:
            print(f"subframe {k:4d}: {st['active_blocks']:6d} of {st['blocks']} blocks active, {st['active_pixels']:8d} pixels rendered, decide {st['decide_ms']:.3f} ms")
        if st["active_blocks"] == 0:
            break
    full = w * h * sample.launchParams.frame.subframe_index
    print(f"converged after {sample.launchParams.frame.subframe_index} subframes: {st['pixel_subframes']} pixel-subframes "
          f"({100.0 * st['pixel_subframes'] / full:.1f} % of a loop that renders every pixel every time), {device_ms:.1f} ms on the device")
    sample.adaptiveEnd()
    if args.out:
        np.save(args.out, pixels)
    sample.close()


if __name__ == "__main__":
    main()
