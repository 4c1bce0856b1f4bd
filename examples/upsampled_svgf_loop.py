#!/usr/bin/env python3
"""upsampled_svgf_loop.py — adaptive_svgf_albedo_loop.py with the path tracer at a fraction of the display resolution: the noisy,
low-frequency part of the image (the demodulated irradiance) is traced, accumulated and filtered at size / scale, and brought to the display
resolution under the guidance of a full-resolution G-buffer (upsamplePlanes).  The high-frequency parts are cheap to make at full
resolution and are made there: the geometry edges by renderGBuffer (one traversal kernel, no shading), the texture detail by
surface[Lod]Planes.

Two SampleRenderers over one model: `lo` at size / scale and `hi` at size.  Per frame, on `lo`, steps 1-7 of adaptive_svgf_albedo_loop.py:
  1. renderGBuffer: hit, position and motion against LAST frame's camera;
  2. surfacePlanes (surfaceLodPlanes with --lod, surfaceAnisoPlanes with --aniso N): the low-resolution albedo the demodulation divides by;
  3. samplePlan;  4. renderMask(mask);  5. temporalMoments on the mask;  6. temporalCarry on its complement;
  7. filterPlanes on all pixels: the filtered irradiance at low resolution.
Per frame, on `hi`:
  8. renderGBuffer: hit and position;
  9. surfacePlanes (surfaceLodPlanes with --lod, surfaceAnisoPlanes with --aniso N): the albedo under every display pixel;
 10. upsamplePlanes: the low-resolution irradiance on the display's pixels — four taps of the same surface where there are four, fewer
     where an edge is near, the ring around them where there is none (rescued), another surface's value where that fails too (orphans);
 11. modulatePlanes with the full-resolution albedo: the displayed frame;
 12. with --edge-aa, edgeAaPlanes as the last pass before display: the silhouettes, creases and depth steps of that frame, which show the
     surface under each pixel's centre alone, blended by the share of the pixel that the nearer triangle's edge cuts off;
 13. with --auto-exposure [--tonemap aces|reinhard|linear], behind step 12 when both are given: exposurePlanes meters the linear frame (a
     histogram of log2 luminance, its trimmed mean, an exposure that adapts from frame to frame) and tonemapPlanes writes the displayed
     frame through the operator under that exposure.  The exposure state ping-pongs between two device arrays and goes from the meter to
     the tone mapper without visiting the host (the value in the printed line is read back for the printing alone).
 14. with --bloom [--bloom-threshold T --bloom-levels N], behind step 12 and in front of step 13's tone map: bloomPlanes spreads the part
     of the linear frame above T (on luminance exposed by the PREVIOUS frame's exposure state: this frame's is not metered yet) over a
     pyramid of N levels and adds it back; the meter still reads the frame without bloom, the tone mapper the one with it.  Without
     --auto-exposure the bloomed frame is displayed through the linear operator at exposure 1.
 15. with --motion-blur [--shutter F --blur-taps N], behind steps 12 and 14 and in front of the tone map: step 7's G-buffer also writes
     depth and motion at the display resolution, and motionBlurPlanes blurs the linear frame along that motion, depth-aware, over F of
     the frame interval with N taps a pixel.
 16. with --dof [--focus F | --autofocus] [--aperture K] [--dof-taps N], behind step 12 and in front of steps 14, 15 and the tone map (so
     that bright out-of-focus points bloom as discs): step 7's G-buffer also writes depth, and dofPlanes gathers each pixel over a disc of
     the largest blur circle around it, K * |1 - F / depth| pixels, with N taps.  With --autofocus F follows the depth under the frame's
     centre, smoothed over frames (one float read back per frame); on a miss it returns to --focus.
 17. with --ao [--ao-rays N --ao-radius R], between steps 10 and 11: step 8's G-buffer also writes motion, and aoPlanes shoots N short
     any-hit rays a pixel through `hi`'s tree, jittered by the frame index — the contact shadows that are smaller than a low-resolution
     pixel and so never arrive through step 10.  The occlusion is a colour (ao, ao, ao, 1): temporalAccumulate and filterPlanes treat it
     as they treat one, and modulatePlanes multiplies it into the upsampled irradiance, before the albedo.  (modulatePlanes reads a
     factor of exactly 0 as 1, its rule for a miss's albedo, so the filtered occlusion is kept above 2^-10.)
 18. with --reflect [--reflect-mesh K --reflectivity F], behind steps 11 and 12 and in front of everything that follows them: `hi` gets the
     probe, reflectPlanes shoots every pixel's mirror ray through `hi`'s tree into a second G-buffer (hit2) and the probe's radiance where
     the ray escapes (sky), and step 9's pass runs once more, on hit2, for the reflected surface's albedo.  The reflection's colour is sky
     where the ray escaped and that albedo times the mean of step 10's irradiance elsewhere; it is blended with weight F into the pixels
     of mesh K — in torch: the composition is this example's, not a rule of the library.  The displayed frame then comes from the tone
     mapper, as with steps 14 to 16.
 19. with --sun [--sun-dir X Y Z --sun-spread S --sun-rays N --sun-radiance R G B], behind steps 11 and 12 and in front of step 18: a
     distant disc light that the probe does not hold.  shadowPlanes shoots N any-hit rays a pixel towards it through `hi`'s tree, jittered
     by the frame index, and writes the direct light (radiance * cosine * visibility); modulatePlanes multiplies it by step 9's albedo, and
     the product is added to the composed frame: shadow edges at the display resolution.  With --reflect, reflectPlanes also writes
     position2 and the mirror ray, a second shadowPlanes call lights the reflected surface (hit2, position2, view_ray = ray), and the
     reflection's colour where the ray hit is that light times the reflected surface's albedo instead of the mean-irradiance stand-in.
     The displayed frame then comes from the tone mapper.
`hi` never renders a colour sample.

  python3 examples/upsampled_svgf_loop.py [--scene textured|two_box] [--scale 2|3|4] [--size 960 540] [--frames 16] [--lod] [--aniso N] [--edge-aa]
                                          [--ao] [--ao-rays N] [--ao-radius R] [--reflect] [--reflect-mesh K] [--reflectivity F]
                                          [--sun] [--sun-dir X Y Z] [--sun-spread S] [--sun-rays N] [--sun-radiance R G B]
                                          [--auto-exposure] [--tonemap aces|reinhard|linear] [--bloom] [--bloom-threshold T]
                                          [--bloom-levels N] [--motion-blur] [--shutter F] [--blur-taps N]
                                          [--dof] [--focus F | --autofocus] [--aperture K] [--dof-taps N] [--out-dir .]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from optixpathtracer_amd import renderer as R  # noqa: E402
from optixpathtracer_amd import scenes  # noqa: E402

SCENES = {
    "textured": (scenes.textured_scene, dict(eye=(3.0, 2.5, -4.5), lookat=(0.0, 0.6, 0.5), up=(0.0, 1.0, 0.0), fovY=45.0)),
    "two_box": (lambda: scenes.two_box_scene(shadow_catcher=False), scenes.TWO_BOX_CAMERA),
    "terrain": (scenes.textured_terrain, scenes.TERRAIN_CAMERA),
}
PLAN = dict(threshold=0.25, dark_floor=0.05, min_length=4, min_pixels=8, refresh_period=16)


def autofocus(depth, rects, fallback, previous, rate=0.25):
    """The focus distance of each rectangle (x0, y0, w, h) of a depth plane: the depth under its centre — `fallback` where that is a miss —
    approached from `previous` (None: taken at once) by `rate` a frame.  Reads one float per rectangle back."""
    now = []
    for v, (x0, y0, w, h) in enumerate(rects):
        d = float(depth[y0 + h // 2, x0 + w // 2])
        target = d if np.isfinite(d) and d > 0.0 else float(fallback)
        now.append(target if previous is None else previous[v] + rate * (target - previous[v]))
    return now


def orbit(cam, angle):
    """the camera turned by `angle` radians about the vertical axis through its look-at point"""
    e, l = np.asarray(cam["eye"], np.float64), np.asarray(cam["lookat"], np.float64)
    d = e - l
    c, s = np.cos(angle), np.sin(angle)
    return dict(cam, eye=(float(l[0] + c * d[0] + s * d[2]), float(e[1]), float(l[2] - s * d[0] + c * d[2])))


class UpsampledLoop:
    """The two renderers and every plane of the loop, allocated once; frame(k, prev, cam) runs one frame and returns its figures."""

    def __init__(self, model, size, scale, lod=False, aniso=0, spp=1, probe=None, plan=None, iterations=5, sigma_lum=4.0, min_length=4, max_history=32,
                 edge_aa=False, auto_exposure=False, tonemap="aces", bloom=False, bloom_threshold=1.0, bloom_levels=6,
                 motion_blur=False, shutter=0.5, blur_taps=12, dof=False, focus=4.0, autofocus=False, aperture=6.0, dof_taps=32,
                 ao=False, ao_rays=4, ao_radius=0.5, reflect=False, reflect_mesh=0, reflectivity=0.5,
                 sun=False, sun_dir=(0.4, 1.0, -0.3), sun_spread=0.01, sun_rays=4, sun_radiance=(3.0, 2.9, 2.7)):
        import torch

        self.sun = bool(sun)
        self.sun_lights = [dict(dir=tuple(sun_dir), spread=float(sun_spread), radiance=tuple(sun_radiance), rays=int(sun_rays))]
        self.ao, self.ao_prm = bool(ao), dict(rays=int(ao_rays), radius=float(ao_radius))
        self.reflect, self.reflect_mesh, self.reflectivity = bool(reflect), int(reflect_mesh), float(reflectivity)
        lod = lod or aniso > 0  # the anisotropic pass uses the pyramid as well
        self.size, self.scale, self.lod, self.aniso = tuple(size), int(scale), lod, int(aniso)
        self.edge_aa = bool(edge_aa)
        self.auto_exposure, self.tonemap = bool(auto_exposure), tonemap
        self.bloom, self.bloom_prm = bool(bloom), dict(threshold=float(bloom_threshold), levels=int(bloom_levels))
        self.motion_blur, self.blur_prm = bool(motion_blur), dict(shutter=float(shutter), taps=int(blur_taps))
        self.dof, self.dof_prm = bool(dof), dict(aperture=float(aperture), taps=int(dof_taps))
        self.focus, self.autofocus, self.focus_now = float(focus), bool(autofocus), None
        w, h = self.size
        if w % self.scale or h % self.scale:
            raise SystemExit(f"--size {w} {h} is not a multiple of --scale {self.scale}")
        self.lo_size = lw, lh = w // self.scale, h // self.scale
        self.plan = dict(PLAN, **(plan or {}))
        self.filter = dict(iterations=iterations, sigma_lum=sigma_lum, min_length=min_length)
        self.max_history = max_history
        probe = probe if probe is not None else scenes.sky_probe(1024, 512).BuildCDF()
        self.lo, self.hi = R.SampleRenderer(model), R.SampleRenderer(model)
        self.lo.setProbe(probe)
        self.lo.launchParams.samples_per_launch = spp
        self.lo.resize(self.lo_size)
        self.lo.uploadAccum(np.zeros((lh, lw, 4), np.float32))
        self.hi.resize(self.size)  # no probe: the full-size renderer never shades
        if self.reflect:
            self.hi.setProbe(probe)  # (but step 18's escaped mirror rays look it up)

        def planes(hh, ww, k):
            return torch.zeros((hh, ww, k) if k > 1 else (hh, ww), device="cuda:0")

        self.gbuf = [dict(hit=planes(lh, lw, 8), position=planes(lh, lw, 4), motion=planes(lh, lw, 2)) for _ in range(2)]
        self.history, self.moments = [planes(lh, lw, 4) for _ in range(2)], [planes(lh, lw, 2) for _ in range(2)]
        self.length = [planes(lh, lw, 1) for _ in range(2)]
        self.variance, self.filtered, self.scratch, self.lo_albedo = planes(lh, lw, 1), planes(lh, lw, 4), planes(lh, lw, 4), planes(lh, lw, 4)
        self.hi_gbuf = dict(hit=planes(h, w, 8), position=planes(h, w, 4), **(dict(depth=planes(h, w, 1)) if self.motion_blur or self.dof else {}),
                            **(dict(motion=planes(h, w, 2)) if self.motion_blur else {}))
        self.albedo, self.upsampled, self.weight, self.final = planes(h, w, 4), planes(h, w, 4), planes(h, w, 1), planes(h, w, 4)
        self.modulated = planes(h, w, 4) if self.edge_aa else None  # step 11's output where step 12 follows it
        self.frame_rgba8 = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
        # step 13's histogram and its two exposure states (ev, E, mean log2 luminance, pixels metered); cur: the one the last frame wrote
        self.hist = torch.zeros((1, 256), dtype=torch.int32, device="cuda:0")
        self.state, self.cur = [torch.zeros((1, 4), device="cuda:0") for _ in range(2)], 0
        # step 14's output and its scratch pyramid
        self.bloomed = planes(h, w, 4) if self.bloom else None
        self.pyramid = torch.zeros((self.hi.bloomLayout(self.bloom_prm["levels"])[1] // 16, 4), device="cuda:0") if self.bloom else None
        # step 15's output and its scratch (tile and neighbourhood maxima)
        self.blurred = planes(h, w, 4) if self.motion_blur else None
        self.tiles = torch.zeros((self.hi.motionBlurLayout()[1] // 8, 2), device="cuda:0") if self.motion_blur else None
        # step 16's output and its scratch (tile and neighbourhood maxima of the blur radius)
        self.lens = planes(h, w, 4) if self.dof else None
        self.discs = torch.zeros((self.hi.dofLayout()[1] // 4,), device="cuda:0") if self.dof else None
        # step 17: the G-buffer ping-pongs (the reprojection needs last frame's hit and position) and carries motion; the raw, the
        # accumulated and the filtered occlusion, the batch of rays, and the irradiance with the occlusion in it
        if self.ao:
            self.hi_gbufs = [dict(self.hi_gbuf, motion=self.hi_gbuf.get("motion", planes(h, w, 2))),
                             dict({n: torch.zeros_like(t) for n, t in self.hi_gbuf.items()}, motion=planes(h, w, 2))]
            self.ao_raw, self.ao_filtered, self.ao_scratch, self.shaded = (planes(h, w, 4) for _ in range(4))
            self.ao_history, self.ao_length = [planes(h, w, 4) for _ in range(2)], [planes(h, w, 1) for _ in range(2)]
            self.ao_batch = torch.zeros((self.hi.aoLayout(self.ao_prm["rays"]) // 4,), device="cuda:0")
        # step 18: the second G-buffer's hit plane, the probe's radiance, the reflected surface's albedo, the reflection's colour, the rays' batch
        if self.reflect:
            self.hit2, self.sky, self.albedo2, self.reflection = planes(h, w, 8), planes(h, w, 4), planes(h, w, 4), planes(h, w, 4)
            self.reflect_batch = torch.zeros((self.hi.reflectLayout() // 4,), device="cuda:0")
        # step 19: the direct light, its product with the albedo, the rays' batch; with step 18 the same for the reflected surface, which
        # also needs where the mirror ray hit and the ray itself
        if self.sun:
            self.sun_light, self.sun_lit = planes(h, w, 4), planes(h, w, 4)
            self.sun_batch = torch.zeros((self.hi.shadowLayout(self.sun_lights) // 4,), device="cuda:0")
            if self.reflect:
                self.position2, self.ray2, self.sun_light2, self.sun_lit2 = planes(h, w, 4), planes(h, w, 8), planes(h, w, 4), planes(h, w, 4)
        self.accum = self.lo.deviceBuffer(R.PT_BUF_ACCUM)
        # per renderer: the scene's texcoords per primitive and, with --lod, the mip pyramid of its textures — once, before the loop
        self.table = {id(r): r.copyTexcoordsDevice() for r in (self.lo, self.hi)}
        self.mips = {id(r): r.copyTextureMipsDevice() if lod else None for r in (self.lo, self.hi)}

    def _albedo(self, r, hit, out):
        if self.aniso:
            return r.surfaceAnisoPlanes(hit, self.table[id(r)], self.mips[id(r)], max_aniso=self.aniso, out=dict(albedo=out))["stats"]
        if self.lod:
            return r.surfaceLodPlanes(hit, self.table[id(r)], self.mips[id(r)], out=dict(albedo=out))["stats"]
        return r.surfacePlanes(hit, self.table[id(r)], out=dict(albedo=out))["stats"]

    def frame(self, k, prev, cam):
        lo, hi = self.lo, self.hi
        cur, old, i, o = self.gbuf[k & 1], self.gbuf[~k & 1], k & 1, ~k & 1
        t0 = time.perf_counter()
        # ---- the low-resolution chain (the aspect ratio is the same: a Camera serves both renderers)
        lo.setCamera(cam)
        g = lo.renderGBuffer(("hit", "position", "motion"), prev_cameras=prev, out=cur)["stats"]
        s = self._albedo(lo, cur["hit"], self.lo_albedo)
        geo = (cur["motion"], cur["hit"], cur["position"], old["hit"], old["position"], self.history[i], self.moments[i], self.length[i])
        outs = dict(history_out=self.history[o], moments_out=self.moments[o], length_out=self.length[o], variance_out=self.variance)
        p = lo.samplePlan(*geo, frame_index=k, **self.plan)
        lo.launchParams.frame.subframe_index = k
        rendered = lo.renderMask(p["mask"])
        t = lo.temporalMoments(self.accum, *geo, albedo=self.lo_albedo, **outs, mask=p["mask"], color_scale=float(k + 1), max_history=self.max_history,
                               clear_color=True)["stats"]
        c = lo.temporalCarry(*geo, **outs, mask=p["mask"] == 0)["stats"]
        assert c["lost"] == 0  # the plan samples every block that holds a pixel the carry could not carry
        f = lo.filterPlanes(self.history[o], cur["hit"], cur["position"], variance=self.variance, length=self.length[o], out=self.filtered,
                            scratch=self.scratch, **self.filter)["stats"]
        t1 = time.perf_counter()
        # ---- the display resolution: geometry, texture detail, the guided upsample, the product
        hi.setCamera(cam)
        if self.ao:
            self.hi_gbuf, hi_old = self.hi_gbufs[i], self.hi_gbufs[o]
            G = hi.renderGBuffer(tuple(self.hi_gbuf), prev_cameras=prev, out=self.hi_gbuf)["stats"]
        elif self.motion_blur:
            G = hi.renderGBuffer(("hit", "position", "depth", "motion"), prev_cameras=prev, out=self.hi_gbuf)["stats"]
        elif self.dof:
            G = hi.renderGBuffer(("hit", "position", "depth"), out=self.hi_gbuf)["stats"]
        else:
            G = hi.renderGBuffer(("hit", "position"), out=self.hi_gbuf)["stats"]
        S = self._albedo(hi, self.hi_gbuf["hit"], self.albedo)
        u = hi.upsamplePlanes(self.filtered, cur["hit"], cur["position"], self.hi_gbuf["hit"], self.hi_gbuf["position"], self.scale, out=self.upsampled,
                              weight_out=self.weight)["stats"]
        irradiance = self.upsampled
        if self.ao:
            hg = self.hi_gbuf
            a = hi.aoPlanes(hg["hit"], hg["position"], out=self.ao_raw, scratch=self.ao_batch, jitter=True, seed=k, **self.ao_prm)["stats"]
            ta = hi.temporalAccumulate(self.ao_raw, hg["motion"], hg["hit"], hg["position"], hi_old["hit"], hi_old["position"], self.ao_history[i],
                                       self.ao_length[i], history_out=self.ao_history[o], length_out=self.ao_length[o], max_history=self.max_history)["stats"]
            fa = hi.filterPlanes(self.ao_history[o], hg["hit"], hg["position"], length=self.ao_length[o], out=self.ao_filtered, scratch=self.ao_scratch,
                                 iterations=3, sigma_lum=self.filter["sigma_lum"], min_length=self.filter["min_length"])["stats"]
            self.ao_filtered[..., 0:3].clamp_(min=2.0 ** -10)  # (modulatePlanes reads a factor of 0 as 1)
            ma = hi.modulatePlanes(self.upsampled, albedo=self.ao_filtered, out=self.shaded)["stats"]
            irradiance = self.shaded
            ao = dict(ao_ms=a["kernel_ms"], ao_trace_ms=a["trace_ms"], ao_rays=a["rays"], ao_occluded=a["occluded"], ao_batches=a["batches"],
                      ao_chain_ms=ta["kernel_ms"] + fa["kernel_ms"] + ma["kernel_ms"])
        else:
            ao = dict(ao_ms=0.0, ao_trace_ms=0.0, ao_rays=0, ao_occluded=0, ao_batches=0, ao_chain_ms=0.0)
        # with auto exposure, depth of field, bloom or motion blur the tone mapper writes the displayed frame
        shown = None if self.auto_exposure or self.dof or self.bloom or self.motion_blur or self.reflect or self.sun else self.frame_rgba8
        if self.edge_aa:
            m = hi.modulatePlanes(irradiance, albedo=self.albedo, out=self.modulated)["stats"]
            e = hi.edgeAaPlanes(self.modulated, self.hi_gbuf["hit"], self.hi_gbuf["position"], out=self.final, frame=shown)["stats"]
        else:
            m = hi.modulatePlanes(irradiance, albedo=self.albedo, out=self.final, frame=shown)["stats"]
            e = dict(kernel_ms=0.0, boundary=0, blended=0)
        sun = dict(sun_ms=0.0, sun_trace_ms=0.0, sun_rays=0, sun_occluded=0, sun_backfacing=0, sun_batches=0, sun_reflected_ms=0.0)
        if self.sun:
            hg = self.hi_gbuf
            sh = hi.shadowPlanes(hg["hit"], hg["position"], lights=self.sun_lights, light=self.sun_light, scratch=self.sun_batch, jitter=True, seed=k)["stats"]
            hi.modulatePlanes(self.sun_light, albedo=self.albedo, out=self.sun_lit)
            self.final[..., 0:3] += self.sun_lit[..., 0:3]
            sun.update(sun_ms=sh["kernel_ms"], sun_trace_ms=sh["trace_ms"], sun_rays=sh["rays"], sun_occluded=sh["occluded"], sun_backfacing=sh["backfacing"],
                       sun_batches=sh["batches"])
        if self.reflect:
            import torch

            hg = self.hi_gbuf
            more = dict(position2=self.position2, ray=self.ray2) if self.sun else {}
            rf = hi.reflectPlanes(hg["hit"], hg["position"], hit2=self.hit2, sky=self.sky, scratch=self.reflect_batch, **more)["stats"]
            rs = self._albedo(hi, self.hit2, self.albedo2)  # every pass that reads a hit plane works on the second G-buffer
            escaped = self.sky[..., 3:4] == 1.0
            seen = escaped | (self.hit2.view(torch.int32)[..., 3:4] >= 0)  # the pixels whose mirror ray was traced
            if self.sun:  # the reflected surface under the sun: facing is judged from the mirror ray's origin, not from the eye
                s2 = hi.shadowPlanes(self.hit2, self.position2, lights=self.sun_lights, view_ray=self.ray2, light=self.sun_light2, scratch=self.sun_batch,
                                     jitter=True, seed=k)["stats"]
                hi.modulatePlanes(self.sun_light2, albedo=self.albedo2, out=self.sun_lit2)
                reflected = self.sun_lit2[..., 0:3]
                sun.update(sun_reflected_ms=s2["kernel_ms"])
            else:
                reflected = self.albedo2[..., 0:3] * irradiance[..., 0:3].mean(dim=(0, 1))
            self.reflection[..., 0:3] = torch.where(escaped, self.sky[..., 0:3], reflected)
            self.reflection[..., 3] = seen[..., 0].to(torch.float32)
            words = hg["hit"].view(torch.int32)
            mirror = (words[..., 3:4] >= 0) & (words[..., 4:5] == self.reflect_mesh) & seen
            F = self.reflectivity
            self.final[..., 0:3] = torch.where(mirror, (1.0 - F) * self.final[..., 0:3] + F * self.reflection[..., 0:3], self.final[..., 0:3])
            self.mirrored = mirror  # (counted by the caller, outside the timed frame)
            rfl = dict(reflect_ms=rf["kernel_ms"], reflect_trace_ms=rf["trace_ms"], reflect_hits=rf["hits"], reflect_escaped=rf["escaped"],
                       reflect_batches=rf["batches"], reflect_surface_ms=rs["kernel_ms"])
        else:
            rfl = dict(reflect_ms=0.0, reflect_trace_ms=0.0, reflect_hits=0, reflect_escaped=0, reflect_batches=0, reflect_surface_ms=0.0)
        lit = self.final
        if self.dof:
            w, h = self.size
            self.focus_now = autofocus(self.hi_gbuf["depth"], [(0, 0, w, h)], self.focus, self.focus_now) if self.autofocus else [self.focus]
            df = hi.dofPlanes(lit, self.hi_gbuf["depth"], out=self.lens, scratch=self.discs, focus=self.focus_now[0], **self.dof_prm)["stats"]
            lit = self.lens
        else:
            df = dict(kernel_ms=0.0, gathered=0)
        if self.bloom:
            b = hi.bloomPlanes(lit, state=self.state[i] if self.auto_exposure and k else None, out=self.bloomed, scratch=self.pyramid,
                               **self.bloom_prm)["stats"]
            lit = self.bloomed
        else:
            b = dict(kernel_ms=0.0, bright=0)
        if self.motion_blur:
            mb = hi.motionBlurPlanes(lit, self.hi_gbuf["motion"], self.hi_gbuf["depth"], out=self.blurred, scratch=self.tiles, **self.blur_prm)["stats"]
            lit = self.blurred
        else:
            mb = dict(kernel_ms=0.0, moving=0)
        if self.auto_exposure:
            x = hi.exposurePlanes(self.final, self.hi_gbuf["hit"], hist=self.hist, state_in=self.state[i] if k else None, state_out=self.state[o],
                                  rate_up=0.25, rate_down=0.5)["stats"]
            tm = hi.tonemapPlanes(lit, state=self.state[o], frame=self.frame_rgba8, op=self.tonemap, write_out=False)["stats"]
            self.cur = o
        else:
            x, tm = dict(kernel_ms=0.0, skipped=0, under=0, over=0), dict(kernel_ms=0.0, clipped=0)
            if self.dof or self.bloom or self.motion_blur or self.reflect or self.sun:
                tm = hi.tonemapPlanes(lit, frame=self.frame_rgba8, op="linear", write_out=False)["stats"]
        t2 = time.perf_counter()
        ev = float(self.state[self.cur][0, 0]) if self.auto_exposure else 0.0  # read back for the caller's printing, outside the timed frame
        return dict(frame_ms=(t2 - t0) * 1e3, lo_ms=(t1 - t0) * 1e3, hi_ms=(t2 - t1) * 1e3, sampled=p["stats"]["sampled"], blocks=p["stats"]["blocks"],
                    rendered=rendered, colour_ms=lo.stats()["render_ms"], lo_gbuffer_ms=g["kernel_ms"], lo_surface_ms=s["kernel_ms"],
                    plan_ms=p["stats"]["kernel_ms"], temporal_ms=t["kernel_ms"], carry_ms=c["kernel_ms"], filter_ms=f["kernel_ms"],
                    gbuffer_ms=G["kernel_ms"], surface_ms=S["kernel_ms"], upsample_ms=u["kernel_ms"], modulate_ms=m["kernel_ms"],
                    pixels=u["pixels"], full=u["full"], rescued=u["rescued"], orphans=u["orphans"], edge_aa_ms=e["kernel_ms"], boundary=e["boundary"],
                    blended=e["blended"], exposure_ms=x["kernel_ms"], tonemap_ms=tm["kernel_ms"], ev=ev, skipped=x["skipped"], under=x["under"],
                    over=x["over"], clipped=tm["clipped"], bloom_ms=b["kernel_ms"], bright=b["bright"],
                    motion_blur_ms=mb["kernel_ms"], moving=mb["moving"], dof_ms=df["kernel_ms"], gathered=df["gathered"],
                    focus=self.focus_now[0] if self.dof else 0.0, **ao, **rfl, **sun, mirrored=int(self.mirrored.sum()) if self.reflect else 0)

    def close(self):
        self.lo.close()
        self.hi.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=sorted(SCENES), default="textured")
    ap.add_argument("--scale", type=int, choices=(2, 3, 4), default=2)
    ap.add_argument("--size", type=int, nargs=2, default=[960, 540], help="the display size; a multiple of --scale")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--lod", action="store_true", help="footprint-filtered albedo (surfaceLodPlanes) at both resolutions")
    ap.add_argument("--aniso", type=int, default=0, metavar="N", help="implies --lod: up to N (1..16) lookups along the footprint's longer axis (surfaceAnisoPlanes)")
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
    ap.add_argument("--ao", action="store_true", help="ray-traced ambient occlusion (aoPlanes) at the display resolution, multiplied into the upsampled irradiance")
    ap.add_argument("--ao-rays", type=int, default=4, metavar="N", help="with --ao: rays per pixel and frame (1..32)")
    ap.add_argument("--ao-radius", type=float, default=0.5, metavar="R", help="with --ao: the rays' length, world units")
    ap.add_argument("--reflect", action="store_true", help="mirror reflections (reflectPlanes) at the display resolution, blended into the pixels of one mesh")
    ap.add_argument("--reflect-mesh", type=int, default=0, metavar="K", help="with --reflect: the mesh that mirrors")
    ap.add_argument("--reflectivity", type=float, default=0.5, metavar="F", help="with --reflect: the reflection's weight in that mesh's pixels, in [0, 1]")
    ap.add_argument("--sun", action="store_true", help="a distant disc light (shadowPlanes) at the display resolution, added to the composed frame; lights --reflect's surface too")
    ap.add_argument("--sun-dir", type=float, nargs=3, default=[0.4, 1.0, -0.3], metavar=("X", "Y", "Z"), help="with --sun: the direction towards the light")
    ap.add_argument("--sun-spread", type=float, default=0.01, metavar="S", help="with --sun: the tangent of the disc's angular radius, in [0, 1]")
    ap.add_argument("--sun-rays", type=int, default=4, metavar="N", help="with --sun: rays per pixel and frame (1..32)")
    ap.add_argument("--sun-radiance", type=float, nargs=3, default=[3.0, 2.9, 2.7], metavar=("R", "G", "B"), help="with --sun: the light's radiance")
    ap.add_argument("--out-dir", default=".")
    args = ap.parse_args(argv)
    w, h = args.size
    make, cam0 = SCENES[args.scene]
    loop = UpsampledLoop(make(), (w, h), args.scale, lod=args.lod, aniso=args.aniso, spp=args.spp, edge_aa=args.edge_aa,
                         auto_exposure=args.auto_exposure, tonemap=args.tonemap, bloom=args.bloom, bloom_threshold=args.bloom_threshold,
                         bloom_levels=args.bloom_levels, motion_blur=args.motion_blur, shutter=args.shutter, blur_taps=args.blur_taps,
                         dof=args.dof, focus=args.focus, autofocus=args.autofocus, aperture=args.aperture, dof_taps=args.dof_taps,
                         ao=args.ao, ao_rays=args.ao_rays, ao_radius=args.ao_radius, reflect=args.reflect, reflect_mesh=args.reflect_mesh,
                         reflectivity=args.reflectivity, sun=args.sun, sun_dir=args.sun_dir, sun_spread=args.sun_spread, sun_rays=args.sun_rays,
                         sun_radiance=args.sun_radiance)
    cam = R.make_camera(cam0, w / h)
    for k in range(args.frames):
        prev, cam = cam, R.make_camera(orbit(cam0, 0.01 * k), w / h)
        x = loop.frame(k, prev, cam)
        print(f"frame {k}: at {loop.lo_size[0]} x {loop.lo_size[1]}: {x['sampled']} of {x['blocks']} blocks sampled, {x['rendered']} pixels rendered; "
              f"G-buffer {x['lo_gbuffer_ms']:.3f} ms, surface {x['lo_surface_ms']:.3f} ms, plan {x['plan_ms']:.3f} ms, colour {x['colour_ms']:.2f} ms, "
              f"temporal {x['temporal_ms']:.3f} ms, carry {x['carry_ms']:.3f} ms, filter {x['filter_ms']:.3f} ms; at {w} x {h}: G-buffer "
              f"{x['gbuffer_ms']:.3f} ms, surface {x['surface_ms']:.3f} ms, upsample {x['upsample_ms']:.3f} ms, modulate {x['modulate_ms']:.3f} ms; "
              f"of {x['pixels']} pixels full {x['full']} rescued {x['rescued']} orphans {x['orphans']}; "
              + (f"occlusion {x['ao_ms']:.3f} ms (traversal {x['ao_trace_ms']:.3f} ms, {x['ao_occluded']} of {x['ao_rays']} rays occluded, {x['ao_batches']} batches), "
                 f"its accumulation, filter and product {x['ao_chain_ms']:.3f} ms; " if loop.ao else "")
              + (f"edge aa {x['edge_aa_ms']:.3f} ms, {x['blended']} of {x['boundary']} boundary pixels blended; " if loop.edge_aa else "")
              + (f"sun {x['sun_ms']:.3f} ms (traversal {x['sun_trace_ms']:.3f} ms, {x['sun_occluded']} of {x['sun_rays']} rays shadowed, {x['sun_backfacing']} pairs "
                 f"under the horizon, {x['sun_batches']} batches)" + (f", on the reflected surface {x['sun_reflected_ms']:.3f} ms; " if loop.reflect else "; ") if loop.sun else "")
              + (f"reflection {x['reflect_ms']:.3f} ms (traversal {x['reflect_trace_ms']:.3f} ms, {x['reflect_hits']} rays hit, {x['reflect_escaped']} escaped, "
                 f"{x['reflect_batches']} batches), its surface pass {x['reflect_surface_ms']:.3f} ms, {x['mirrored']} pixels mirror; " if loop.reflect else "")
              + (f"depth of field {x['dof_ms']:.3f} ms ({x['gathered']} pixels gather, focus {x['focus']:.3f}); " if loop.dof else "")
              + (f"bloom {x['bloom_ms']:.3f} ms ({x['bright']} bright pixels); " if loop.bloom else "")
              + (f"motion blur {x['motion_blur_ms']:.3f} ms ({x['moving']} pixels gather); " if loop.motion_blur else "")
              + (f"exposure {x['exposure_ms']:.3f} ms (ev {x['ev']:+.3f}, {x['skipped']} misses skipped, {x['under']} under, {x['over']} over), "
                 f"tone map {x['tonemap_ms']:.3f} ms ({x['clipped']} pixels clipped); " if loop.auto_exposure else "")
              + f"frame {x['frame_ms']:.2f} ms")
    np.save(os.path.join(args.out_dir, "upsampled_svgf_final.npy"), loop.final.cpu().numpy())
    np.save(os.path.join(args.out_dir, "upsampled_svgf_frame.npy"), loop.frame_rgba8.cpu().numpy().view(np.uint32))
    if loop.motion_blur:
        np.save(os.path.join(args.out_dir, "upsampled_svgf_blurred.npy"), loop.blurred.cpu().numpy())
    if loop.dof:
        np.save(os.path.join(args.out_dir, "upsampled_svgf_dof.npy"), loop.lens.cpu().numpy())
    if loop.ao:
        np.save(os.path.join(args.out_dir, "upsampled_svgf_ao.npy"), loop.ao_filtered.cpu().numpy())
    if loop.reflect:
        np.save(os.path.join(args.out_dir, "upsampled_svgf_reflection.npy"), loop.reflection.cpu().numpy())
    if loop.sun:
        np.save(os.path.join(args.out_dir, "upsampled_svgf_sun.npy"), loop.sun_light.cpu().numpy())
    print(f"wrote upsampled_svgf_final.npy and upsampled_svgf_frame.npy to {args.out_dir}")
    loop.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
