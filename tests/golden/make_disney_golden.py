#!/usr/bin/env python3
"""Generates tests/golden/ref_disney.npz: what the REFERENCE's own Disney BSDF (Disney.cuh:151-426) and ProbeData::BuildCDF
(Probe.h:29-77) return, through oracle/_ref/libptref_disney.so (glibc transcendentals, key prefix 'libm.') and
oracle/_ref/libptref_disney_det.so (include/pt_detmath.h transcendentals, prefix 'det.'), for fixed inputs chosen where a BSDF
goes wrong: grazing and tangent directions, L = +-V, back-side views, a vanishing half vector, non-normalised and zero vectors,
eta pairs up to total internal reflection, roughness 0, black base colour, seeds 0 / 1 / 0xffffffff.  BuildCDF images have
widths and heights around the 64-lane chunks of the GPU build and black, denormal, overflowing, negative and NaN texels.
tests/test_oracle_reference_bsdf.py and tests/test_gpu_reference_pins.py compare against it.  The file is deterministic: a
second run writes the same bytes.
Run where oracle/_ref was built (make -C oracle ref):  python tests/golden/make_disney_golden.py"""
import ctypes as C
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "ref_disney.npz")
SEED = 20261016
ETA_PAIRS = [(1.0, 1.5), (1.5, 1.0), (1.0, 1.0), (2.4, 1.0), (1.0, 1e-3)]
N_RANDOM = 300
N_ALBEDO_GEO = 64  # the albedo != colour table evaluates the first cases of the random block
FLAVOURS = ("libm", "det")


def materials():
    """(names, [MATERIAL_DTYPE scalar]): the presets, the default, a dielectric, then the edge materials."""
    sys.path.insert(0, ROOT)
    from optixpathtracer_amd import scenes

    M = scenes.Material
    mats = [(f"preset{i}", m) for i, m in enumerate(scenes.material_presets())]
    mats += [
        ("default", M()),
        ("glass133", M(transmission=1.0, roughness=0.2, eta=1.33)),
        ("rough0", M(roughness=0.0)),
        ("rough1", M(roughness=1.0, specular=0.7)),
        ("metal1", M(color=(0.9, 0.6, 0.2), metallic=1.0, roughness=0.3)),
        ("black_tint", M(color=(0.0, 0.0, 0.0), specularTint=1.0, sheenTint=1.0, roughness=0.5)),
        ("clearcoat_gloss0", M(clearcoat=1.0, clearcoatGloss=0.0, roughness=0.4)),
        ("clearcoat_gloss1", M(clearcoat=1.0, clearcoatGloss=1.0, roughness=0.4)),
        ("half_transmission_rough0", M(transmission=0.5, roughness=0.0, color=(0.7, 0.8, 0.9))),
        ("subsurface1", M(subsurface=1.0, color=(0.8, 0.3, 0.2), roughness=0.6)),
        ("specular0", M(specular=0.0, roughness=0.3)),
    ]
    return [n for n, _ in mats], [m for _, m in mats]


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def geometry():
    """(N, V, L, eta (G,2), seed (G,)): constructed cases under every eta pair, then a random block."""
    rng = np.random.default_rng(SEED)
    z = np.array([0.0, 0.0, 1.0], np.float32)
    n0 = _unit(rng.standard_normal(3))
    up = lambda n: _unit(rng.standard_normal(3) * 0.5 + n)  # a direction on n's side
    t_exact = np.array([0.6, 0.8, 0.0], np.float32)  # N.L == 0 exactly against N = +z
    tiny = np.float32(1.4e-45)  # the float next to 0
    fmin = np.float32(1.1754944e-38)
    cases = []
    for n in (n0, _unit([0.9, 0.3, -0.2]), _unit([0.1, -0.2, 0.97])):  # BasisFromVector: |x| > |y| and |x| <= |y|
        v = up(n)
        cases += [(n, v, v), (n, v, -v), (n, v, n), (n, n, up(n)), (n, n, n), (n, -v, -v), (n, -v, v), (n, -v, up(n))]
    for lz in (0.0, tiny, -tiny, fmin, -fmin, np.float32(6e-8), np.float32(-6e-8)):  # L in the tangent plane and next to it
        cases.append((z, up(z), np.array([0.6, 0.8, lz], np.float32)))
    cases.append((n0, up(n0), _unit(np.cross(n0, rng.standard_normal(3)))))  # tangent up to rounding, off-axis
    for vz in (1e-2, 1e-4, 1e-8, 1e-15, 1e-30, 0.0):  # grazing views down to N.V = 1e-30
        v = np.array([np.sqrt(1.0 - vz * vz), 0.0, vz], np.float32)
        cases += [(z, v, up(z)), (z, v, -v)]
    cases.append((z, t_exact, t_exact))
    for s in (2.0, 0.5, 1e-3, 1e3):  # non-normalised N
        cases.append(((n0 * np.float32(s)).astype(np.float32), up(n0), up(n0)))
    zero = np.zeros(3, np.float32)
    cases += [(zero, up(z), up(z)), (z, zero, up(z)), (z, up(z), zero), (-z, up(-z), up(-z)), (np.array([1.0, 1.0, 0.0], np.float32), up(z), up(z))]
    N, V, L, eta = [], [], [], []
    for e in ETA_PAIRS:
        for n, v, l in cases:
            N.append(n); V.append(v); L.append(l); eta.append(e)
    k = len(N)
    seeds = [0, 1, 0xFFFFFFFF] + [int(x) for x in rng.integers(0, 2**32, k, dtype=np.uint64)]
    seed = np.array([seeds[i] if i % 4 < 3 else seeds[3 + i] for i in range(k)], np.uint32)
    Nr = _unit(rng.standard_normal((N_RANDOM, 3)))
    Vr = _unit(rng.standard_normal((N_RANDOM, 3)))
    Vr = np.where(((np.sum(Nr * Vr, 1) < 0) & (rng.random(N_RANDOM) < 0.8))[:, None], -Vr, Vr).astype(np.float32)  # mostly above
    Lr = _unit(rng.standard_normal((N_RANDOM, 3)))
    er = np.array([ETA_PAIRS[i] for i in rng.integers(0, len(ETA_PAIRS), N_RANDOM)], np.float32)
    sr = rng.integers(0, 2**32, N_RANDOM, dtype=np.uint64).astype(np.uint32)
    sr[:3] = (0, 1, 0xFFFFFFFF)
    N = np.concatenate([np.array(N, np.float32), Nr]); V = np.concatenate([np.array(V, np.float32), Vr])
    L = np.concatenate([np.array(L, np.float32), Lr]); eta = np.concatenate([np.array(eta, np.float32), er])
    return N, V, L, eta, np.concatenate([seed, sr]), k


def albedo_cases():
    """(material names, albedos): BSDFEval with an albedo other than the material colour (deviceProgram.cu passes the
    texture-modulated colour), over the first N_ALBEDO_GEO random cases."""
    names = ["default", "metal1", "black_tint", "preset7", "glass133", "clearcoat_gloss0"]
    albedos = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.9, 0.1, 0.1], [1e-30, 0.0, 0.0]], np.float32)
    return names, albedos


def cdf_images():
    """[(name, (h, w, 4) float32)] for BuildCDF."""
    rng = np.random.default_rng(SEED + 1)

    def img(w, h, scale=1.0):
        a = (rng.random((h, w, 4)) * scale).astype(np.float32)
        a[rng.random((h, w)) < 0.1, :3] = 0.0
        a[..., 3] = 1.0
        return a

    out = [(f"rand_{w}x{h}", img(w, h)) for w, h in ((1, 1), (63, 2), (64, 2), (65, 2), (127, 1), (128, 1), (129, 2), (2, 63), (1, 64), (2, 65),
                                                     (1, 127), (2, 128), (1, 129), (65, 65))]
    out.append(("scaled_1e30_33x3", img(33, 3, 1e30)))
    a = img(9, 6); a[2, :, :3] = 0.0; out.append(("black_row", a))
    a = img(6, 9); a[:, 3, :3] = 0.0; out.append(("black_column", a))
    a = img(5, 4); a[..., :3] = 0.0; out.append(("all_black", a))
    a = img(70, 3); a[0, :, :3] *= np.float32(1e-39); a[1, ::3, :3] = np.float32(1e-44); out.append(("denormal", a))
    a = img(66, 2); a[0, 10:20, :3] = np.float32(3.0e38); a[1, :, :3] = np.float32(3.4e38); out.append(("near_flt_max", a))
    a = img(7, 5); a[1, 2, 0] = -0.75; a[3, 6, :3] = -2.0; out.append(("negative_texel", a))
    a = img(7, 5); a[2, 4, 1] = np.nan; out.append(("nan_texel", a))
    return out


def bsdf_outputs(pdf_fn, eval_fn, sample_fn, mats, N, V, L, eta, seed):
    """Run one implementation over every (material, case).  pdf_fn(mat_ptr, etaI, etaO, N, V, L) -> float,
    eval_fn(mat_ptr, albedo, etaI, etaO, N, V, L, out3), sample_fn(mat_ptr, etaI, etaO, N, V, seed, L3, c_float_ref, st2)."""
    M, G = len(mats), len(N)
    f = np.zeros((M, G, 3), np.float32); p = np.zeros((M, G), np.float32)
    sl = np.zeros((M, G, 3), np.float32); sp = np.zeros((M, G), np.float32); ss = np.zeros((M, G, 2), np.uint32)
    o3 = np.zeros(3, np.float32); st = np.zeros(2, np.uint32); pdf = C.c_float()
    for m, mat in enumerate(mats):
        mat = np.array(mat)
        mp = mat.ctypes.data
        alb = np.ascontiguousarray(mat["color"], np.float32)
        for i in range(G):
            ei, eo = float(eta[i, 0]), float(eta[i, 1])
            eval_fn(mp, alb, ei, eo, N[i], V[i], L[i], o3)
            f[m, i] = o3
            p[m, i] = pdf_fn(mp, ei, eo, N[i], V[i], L[i])
            sample_fn(mp, ei, eo, N[i], V[i], int(seed[i]), o3, C.byref(pdf), st)
            sl[m, i] = o3; sp[m, i] = pdf.value; ss[m, i] = st
    return dict(eval=f, pdf=p, sample_L=sl, sample_pdf=sp, sample_state=ss)


def albedo_outputs(eval_fn, mats, names, N, V, L, eta, k):
    an, albedos = albedo_cases()
    out = np.zeros((len(an), len(albedos), k, 3), np.float32)
    o3 = np.zeros(3, np.float32)
    for a, name in enumerate(an):
        mat = np.array(mats[names.index(name)])
        for b, alb in enumerate(albedos):
            for i in range(k):
                eval_fn(mat.ctypes.data, alb, float(eta[i, 0]), float(eta[i, 1]), N[i], V[i], L[i], o3)
                out[a, b, i] = o3
    return out


def ref_fns(R):
    return R.ref_bsdf_pdf, R.ref_bsdf_eval, R.ref_bsdf_sample


def orc_fns(L, mode=0):
    """The checker's entry points in ref_fns' shape (mode 0 = Disney)."""
    return ((lambda *a: L.orc_bsdf_pdf(mode, *a)), (lambda *a: L.orc_bsdf_eval(mode, *a)), (lambda *a: L.orc_bsdf_sample(mode, *a)))


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps, so that the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(arrays[key]), allow_pickle=False)
            zi = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue(), compresslevel=9)
    with open(path, "wb") as f:
        f.write(buf.getvalue())


def main():
    sys.path.insert(0, ROOT)
    from oracle import orc

    libs = {fl: orc.load_ref_disney(fl) for fl in FLAVOURS}
    if any(R is None for R in libs.values()):
        raise SystemExit("oracle/_ref/libptref_disney*.so not built (make -C oracle ref, where the reference is present)")
    names, mats = materials()
    N, V, L, eta, seed, n_constructed = geometry()
    G = dict(mat=np.stack([np.frombuffer(np.array(m).tobytes(), np.uint8) for m in mats]), mat_names=np.array(names),
             N=N, V=V, L=L, eta=eta, seed=seed, n_constructed=np.int64(n_constructed),
             albedo_mats=np.array(albedo_cases()[0]), albedos=albedo_cases()[1])
    Ra, Va, La, ea = N[n_constructed:n_constructed + N_ALBEDO_GEO], V[n_constructed:n_constructed + N_ALBEDO_GEO], L[n_constructed:n_constructed + N_ALBEDO_GEO], eta[n_constructed:n_constructed + N_ALBEDO_GEO]
    for fl, R in libs.items():
        for k, v in bsdf_outputs(*ref_fns(R), mats, N, V, L, eta, seed).items():
            G[f"{fl}.{k}"] = v
        G[f"{fl}.albedo_eval"] = albedo_outputs(R.ref_bsdf_eval, mats, names, Ra, Va, La, ea, N_ALBEDO_GEO)
    imgs = cdf_images()
    G["cdf_names"] = np.array([n for n, _ in imgs])
    for name, a in imgs:
        h, w = a.shape[:2]
        outs = []
        for R in libs.values():  # BuildCDF has no transcendental: both flavours must agree, so one copy is kept
            o = (np.zeros((h, w), np.float32), np.zeros((h, w), np.float32), np.zeros(h, np.float32), np.zeros(h, np.float32))
            R.ref_build_cdf(a.reshape(-1), w, h, o[0].reshape(-1), o[1].reshape(-1), o[2], o[3])
            outs.append(o)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(*outs)), name
        G[f"cdf.{name}.data"] = a
        for key, arr in zip(("pdfX", "cdfX", "pdfY", "cdfY"), outs[0]):
            G[f"cdf.{name}.{key}"] = arr
    save_npz(OUT, G)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(mats)} materials x {len(N)} cases, {len(imgs)} images")


if __name__ == "__main__":
    main()
