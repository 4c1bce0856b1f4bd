#!/usr/bin/env python3
"""adaptive_svgf_albedo_loop.py — adaptive_svgf_loop.py with demodulation: the SVGF loop that path-traces only the blocks that need samples
AND filters irradiance rather than colour, so texture detail survives the a-trous filter.

adaptive_svgf_loop.py cannot demodulate: PT_BUF_ALBEDO is written by the render, so in a block the plan left out it holds the first-hit albedo
of an older camera.  surfacePlanes derives the albedo from this frame's hit plane instead — every pixel, this frame's camera, no rays — and
that plane is what temporalMoments divides by and modulatePlanes multiplies back in.  Per frame:
  1. renderGBuffer: hit, position and motion against LAST frame's camera;
  2. surfacePlanes on all pixels: the albedo under every pixel's centre (the texcoord table is taken once, before the loop);
  3. samplePlan: the 8x8 blocks that need samples;
  4. renderMask(mask): this frame's samples for those blocks only, into the accumulation buffer;
  5. temporalMoments on the mask with PT_BUF_ACCUM as the colour and the surface albedo: demodulated history, moments, length, variance;
  6. temporalCarry on the mask's complement: the history is demodulated already and is carried unchanged;
  7. filterPlanes on all pixels, on demodulated colour;
  8. modulatePlanes with the surface albedo: the displayed frame.

With --lod step 2 is surfaceLodPlanes: the albedo filtered over the pixel's footprint in texture space (a trilinear lookup in the mip pyramid,
which is built once, before the loop), so a minified texture does not alias in the plane the loop divides by and multiplies back in.
With --aniso N (which implies --lod) it is surfaceAnisoPlanes: up to N such lookups along the footprint's longer axis, so a ground seen at a
grazing angle is not blurred across that axis.
With --edge-aa a step 9 follows, the last pass before display: edgeAaPlanes blends the silhouettes, creases and depth steps of the displayed
frame — which shows the surface under each pixel's centre alone — by the share of the pixel that the nearer triangle's edge cuts off.
With --auto-exposure [--tonemap aces|reinhard|linear] the displayed frame is tonemapPlanes's, behind --edge-aa when both are given: the
linear frame is metered (exposurePlanes: a histogram of log2 luminance, its trimmed mean, an exposure that adapts from frame to frame) and
shown through the operator under that exposure.  The exposure state ping-pongs between two device arrays and never visits the host on the
way from the meter to the tone mapper (the value printed per frame is read back for the printing alone).
With --bloom [--bloom-threshold T --bloom-levels N] bloomPlanes sits behind modulate / edge AA and in front of the tone map: the part of the
linear frame above T (on luminance exposed by the PREVIOUS frame's exposure state: this frame's is not metered yet) is spread over a pyramid
of N levels and added back.  The meter still reads the frame without bloom, the tone mapper the one with it; without --auto-exposure the
bloomed frame is displayed through the linear operator at exposure 1.
With --motion-blur [--shutter F --blur-taps N] motionBlurPlanes sits behind edge AA and bloom and in front of the tone map: the linear frame
is blurred along the G-buffer's motion plane (the camera's orbit here), depth-aware, over F of the frame interval with N taps a pixel.
With --dof [--focus F | --autofocus] [--aperture K] [--dof-taps N] dofPlanes sits behind edge AA and in front of bloom, motion blur and the
tone map, so that bright out-of-focus points bloom as discs: each pixel gathers N taps of a disc of the largest blur circle around it,
K * |1 - F / depth| pixels, from the G-buffer's depth plane.  With --autofocus F follows the depth under the frame's centre, smoothed over
frames (one float read back per frame); on a miss it returns to --focus.

  python3 examples/adaptive_svgf_albedo_loop.py [--scene textured|two_box] [--size 960 540] [--frames 16] [--spp 1] [--threshold 0.25] [--lod] [--aniso N] [--edge-aa]
                                                [--auto-exposure] [--tonemap aces|reinhard|linear] [--bloom] [--bloom-threshold T]
                                                [--bloom-levels N] [--motion-blur] [--shutter F] [--blur-taps N]
                                                [--dof] [--focus F | --autofocus] [--aperture K] [--dof-taps N] [--out-dir .]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from optixpathtracer_amd import renderer as R  # noqa: E402
from optixpathtracer_amd import scenes  # noqa: E402

SCENES = {
    "textured": (scenes.textured_scene, dict(eye=(3.0, 2.5, -4.5), lookat=(0.0, 0.6, 0.5), up=(0.0, 1.0, 0.0), fovY=45.0)),
    "two_box": (lambda: scenes.two_box_scene(shadow_catcher=False), scenes.TWO_BOX_CAMERA),
}


def orbit(cam, angle):
    """the camera turned by `angle` radians about the vertical axis through its look-at point"""
    e, l = np.asarray(cam["eye"], np.float64), np.asarray(cam["lookat"], np.float64)
    d = e - l
    c, s = np.cos(angle), np.sin(angle)
    return dict(cam, eye=(float(l[0] + c * d[0] + s * d[2]), float(e[1]), float(l[2] - s * d[0] + c * d[2])))


def autofocus(depth, rects, fallback, previous, rate=0.25):
    """The focus distance of each rectangle (x0, y0, w, h) of a depth plane: the depth under its centre — `fallback` where that is a miss —
    approached from `previous` (None: taken at once) by `rate` a frame.  Reads one float per rectangle back."""
    now = []
    for v, (x0, y0, w, h) in enumerate(rects):
        d = float(depth[y0 + h // 2, x0 + w // 2])
        target = d if np.isfinite(d) and d > 0.0 else float(fallback)
        now.append(target if previous is None else previous[v] + rate * (target - previous[v]))
    return now


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=sorted(SCENES), default="textured")
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
    ap.add_argument("--lod", action="store_true", help="footprint-filtered albedo (surfaceLodPlanes) instead of the point lookup of surfacePlanes")
    ap.add_argument("--aniso", type=int, default=0, metavar="N", help="implies --lod: up to N (1..16) lookups along the footprint's longer axis (surfaceAnisoPlanes)")
    ap.add_argument("--footprint-scale", type=float, default=1.0, help="with --lod: 1 = the pixel's own footprint")
    ap.add_argument("--edge-aa", action="store_true", help="geometric edge antialiasing (edgeAaPlanes) as the last pass before display")
    ap.add_argument("--auto-exposure", action="store_true", help="meter the linear frame (exposurePlanes) and display it through tonemapPlanes")
    ap.add_argument("--tonemap", choices=["aces", "reinhard", "linear"], default="aces", help="with --auto-exposure: the display operator")
    ap.add_argument("--bloom", action="store_true", help="bloom (bloomPlanes) behind modulate / edge AA and in front of the tone map")
    ap.add_argument("--bloom-threshold", type=float, default=1.0, metavar="T", help="with --bloom: the exposed luminance above which a pixel blooms")
    ap.add_argument("--bloom-levels", type=int, default=6, metavar="N", help="with --bloom: the levels of the pyramid (1..8)")
    ap.add_argument("--motion-blur", action="store_true", help="motion blur (motionBlurPlanes) behind edge AA / bloom and in front of the tone map")
    ap.add_argument("--shutter", type=float, default=0.5, metavar="F", help="with --motion-blur: the open fraction of the frame interval, in [0, 4]")
    ap.add_argument("--blur-taps", type=int, default=12, metavar="N", help="with --motion-blur: taps per pixel (1..64)")
    ap.add_argument("--dof", action="store_true", help="depth of field (dofPlanes) behind edge AA and in front of bloom, motion blur and the tone map")
    ap.add_argument("--focus", type=float, default=4.0, metavar="F", help="with --dof: the depth that is sharp (with --autofocus: where the centre is a miss)")
    ap.add_argument("--autofocus", action="store_true", help="with --dof: focus on the depth under the frame's centre, smoothed over frames")
    ap.add_argument("--aperture", type=float, default=6.0, metavar="K", help="with --dof: the blur-circle radius in pixels of a point at infinity")
    ap.add_argument("--dof-taps", type=int, default=32, metavar="N", help="with --dof: taps per pixel (1..64)")
    ap.add_argument("--out-dir", default=".")
    args = ap.parse_args()
    args.lod = args.lod or args.aniso > 0
    import torch

    dev = "cuda:0"
    w, h = args.size
    make, cam0 = SCENES[args.scene]
    sample = R.SampleRenderer(make())
    sample.setProbe(scenes.sky_probe(1024, 512).BuildCDF())
    sample.launchParams.samples_per_launch = args.spp
    sample.resize((w, h))
    sample.uploadAccum(np.zeros((h, w, 4), np.float32))

    def planes(k):
        return torch.zeros((h, w, k) if k > 1 else (h, w), device=dev)

    # two sets of G-buffer planes (this frame's, last frame's), two of history, moments and length: everything is reused
    gplanes = ("hit", "position", "motion") + (("depth",) if args.motion_blur or args.dof else ())
    gbuf = [dict(hit=planes(8), position=planes(4), motion=planes(2), **(dict(depth=planes(1)) if args.motion_blur or args.dof else {})) for _ in range(2)]
    history, moments, length = [planes(4) for _ in range(2)], [planes(2) for _ in range(2)], [planes(1) for _ in range(2)]
    variance, filtered, scratch, albedo, final = planes(1), planes(4), planes(4), planes(4), planes(4)
    modulated = planes(4) if args.edge_aa else None  # step 8's output where step 9 follows it
    frame = torch.zeros((h, w), dtype=torch.int32, device=dev)
    hist = torch.zeros((1, 256), dtype=torch.int32, device=dev)  # --auto-exposure: the meter's histogram and the two exposure states
    state = [torch.zeros((1, 4), device=dev) for _ in range(2)]
    bloomed = planes(4) if args.bloom else None  # --bloom: its output and its scratch pyramid
    pyramid = torch.zeros((sample.bloomLayout(args.bloom_levels)[1] // 16, 4), device=dev) if args.bloom else None
    blurred = planes(4) if args.motion_blur else None  # --motion-blur: its output and its scratch (tile and neighbourhood maxima)
    tiles = torch.zeros((sample.motionBlurLayout()[1] // 8, 2), device=dev) if args.motion_blur else None
    lens = planes(4) if args.dof else None  # --dof: its output, its scratch (tile and neighbourhood maxima of the blur radius), the focus
    discs = torch.zeros((sample.dofLayout()[1] // 4,), device=dev) if args.dof else None
    focus = None
    accum = sample.deviceBuffer(R.PT_BUF_ACCUM)
    table = sample.copyTexcoordsDevice()  # the scene's texcoords per primitive: once, whatever moves later
    mips = sample.copyTextureMipsDevice() if args.lod else None  # the mip pyramid of the scene's textures: once, too
    cam = R.make_camera(cam0, w / h)
    for k in range(args.frames):
        prev, cam = cam, R.make_camera(orbit(cam0, 0.01 * k), w / h)
        cur, old = gbuf[k & 1], gbuf[~k & 1]
        i, o = k & 1, ~k & 1
        sample.setCamera(cam)
        g = sample.renderGBuffer(gplanes, prev_cameras=prev, out=cur)
        if args.aniso:
            s = sample.surfaceAnisoPlanes(cur["hit"], table, mips, max_aniso=args.aniso, footprint_scale=args.footprint_scale, out=dict(albedo=albedo))
        elif args.lod:
            s = sample.surfaceLodPlanes(cur["hit"], table, mips, footprint_scale=args.footprint_scale, out=dict(albedo=albedo))
        else:
            s = sample.surfacePlanes(cur["hit"], table, out=dict(albedo=albedo))
        geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], history[i], moments[i], length[i])
        outs = dict(history_out=history[o], moments_out=moments[o], length_out=length[o], variance_out=variance)
        p = sample.samplePlan(*geo, threshold=args.threshold, dark_floor=args.dark_floor, min_length=args.plan_min_length, min_pixels=args.min_pixels,
                              refresh_period=args.refresh, frame_index=k)
        mask = p["mask"]
        sample.launchParams.frame.subframe_index = k
        rendered = sample.renderMask(mask)
        t = sample.temporalMoments(accum, *geo, albedo=albedo, **outs, mask=mask, color_scale=float(k + 1), max_history=args.max_history, clear_color=True)
        c = sample.temporalCarry(*geo, **outs, mask=mask == 0)
        assert c["stats"]["lost"] == 0  # the plan samples every block that holds a pixel the carry could not carry
        f = sample.filterPlanes(history[o], cur["hit"], cur["position"], variance=variance, length=length[o], out=filtered, scratch=scratch,
                                iterations=args.iterations, sigma_lum=args.sigma_lum, min_length=args.min_length)
        # with --auto-exposure, --dof, --bloom or --motion-blur the tone mapper writes the displayed frame
        shown = None if args.auto_exposure or args.dof or args.bloom or args.motion_blur else frame
        if args.edge_aa:
            m = sample.modulatePlanes(filtered, albedo=albedo, out=modulated)
            e = sample.edgeAaPlanes(modulated, cur["hit"], cur["position"], out=final, frame=shown)["stats"]
        else:
            m = sample.modulatePlanes(filtered, albedo=albedo, out=final, frame=shown)
        lit = final
        if args.dof:
            focus = autofocus(cur["depth"], [(0, 0, w, h)], args.focus, focus) if args.autofocus else [args.focus]
            df = sample.dofPlanes(lit, cur["depth"], out=lens, scratch=discs, focus=focus[0], aperture=args.aperture, taps=args.dof_taps)["stats"]
            lit = lens
        if args.bloom:
            b = sample.bloomPlanes(lit, state=state[i] if args.auto_exposure and k else None, out=bloomed, scratch=pyramid, threshold=args.bloom_threshold,
                                   levels=args.bloom_levels)["stats"]
            lit = bloomed
        if args.motion_blur:
            mb = sample.motionBlurPlanes(lit, cur["motion"], cur["depth"], out=blurred, scratch=tiles, shutter=args.shutter, taps=args.blur_taps)["stats"]
            lit = blurred
        if args.auto_exposure:
            x = sample.exposurePlanes(final, cur["hit"], hist=hist, state_in=state[i] if k else None, state_out=state[o], rate_up=0.25, rate_down=0.5)["stats"]
            tm = sample.tonemapPlanes(lit, state=state[o], frame=frame, op=args.tonemap, write_out=False)["stats"]
        elif args.dof or args.bloom or args.motion_blur:
            sample.tonemapPlanes(lit, frame=frame, op="linear", write_out=False)
        ps, ss, ts, cs, fs = p["stats"], s["stats"], t["stats"], c["stats"], f["stats"]
        print(f"frame {k}: {ps['sampled']} of {ps['blocks']} blocks sampled, {rendered} pixels rendered, {cs['carried']} carried, "
              f"{ss['textured']} of {ss['hits']} hits textured{', %d minified' % ss['minified'] if args.lod else ''}{', %d taps' % ss['taps'] if args.aniso else ''}; G-buffer {g['stats']['kernel_ms']:.3f} ms, surface {ss['kernel_ms']:.3f} ms, "
              f"plan {ps['kernel_ms']:.3f} ms, colour {sample.stats()['render_ms']:.2f} ms, temporal {ts['kernel_ms']:.3f} ms, "
              f"carry {cs['kernel_ms']:.3f} ms, filter {fs['kernel_ms']:.3f} ms, modulate {m['stats']['kernel_ms']:.3f} ms"
              + (f", edge aa {e['kernel_ms']:.3f} ms ({e['blended']} of {e['boundary']} boundary pixels blended)" if args.edge_aa else "")
              + (f", depth of field {df['kernel_ms']:.3f} ms ({df['gathered']} of {df['pixels']} pixels gather, focus {focus[0]:.3f})" if args.dof else "")
              + (f", bloom {b['kernel_ms']:.3f} ms ({b['bright']} of {b['sources']} pixels bright)" if args.bloom else "")
              + (f", motion blur {mb['kernel_ms']:.3f} ms ({mb['moving']} of {mb['pixels']} pixels gather)" if args.motion_blur else "")
              + (f", exposure {x['kernel_ms']:.3f} ms (ev {float(state[o][0, 0]):+.3f}, {x['skipped']} misses skipped, {x['under']} under, {x['over']} over), "
                 f"tone map {tm['kernel_ms']:.3f} ms ({tm['clipped']} pixels clipped)" if args.auto_exposure else ""))
    np.save(os.path.join(args.out_dir, "adaptive_svgf_albedo_final.npy"), final.cpu().numpy())
    np.save(os.path.join(args.out_dir, "adaptive_svgf_albedo_frame.npy"), frame.cpu().numpy().view(np.uint32))
    if args.bloom:
        np.save(os.path.join(args.out_dir, "adaptive_svgf_albedo_bloomed.npy"), bloomed.cpu().numpy())
    if args.motion_blur:
        np.save(os.path.join(args.out_dir, "adaptive_svgf_albedo_blurred.npy"), blurred.cpu().numpy())
    if args.dof:
        np.save(os.path.join(args.out_dir, "adaptive_svgf_albedo_dof.npy"), lens.cpu().numpy())
    print(f"wrote adaptive_svgf_albedo_final.npy and adaptive_svgf_albedo_frame.npy to {args.out_dir}")
    sample.close()


if __name__ == "__main__":
    main()
