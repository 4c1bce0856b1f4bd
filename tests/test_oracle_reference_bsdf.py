"""The CPU checker's Disney BSDF and BuildCDF, and the product's host pt_build_cdf, against the REFERENCE's own Disney.cuh and
Probe.h (tests/golden/ref_disney.npz, written by tests/golden/make_disney_golden.py through oracle/_ref/libptref_disney*.so).
The libm checker must equal the glibc build of the reference and the det checker the pt_detmath build, bit for bit: +-0 are
equal, NaN equals NaN whatever its payload.  Where oracle/_ref exists, fresh random inputs also run straight against the
reference libraries."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal
from optixpathtracer_amd import _lib, scenes

GOLDEN = os.path.join(ROOT, "tests", "golden")
G = np.load(os.path.join(GOLDEN, "ref_disney.npz"))
_spec = importlib.util.spec_from_file_location("make_disney_golden", os.path.join(GOLDEN, "make_disney_golden.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

MATS = [np.frombuffer(m.tobytes(), scenes.MATERIAL_DTYPE)[0] for m in G["mat"]]
NAMES = [str(n) for n in G["mat_names"]]
LIBM_TRANSCENDENTAL = re.compile(r"^(__)?(sin|cos|tan|sincos|asin|acos|atan|atan2|exp|exp2|expm1|log|log2|log10|log1p|pow)f?(_finite)?(@.*)?$")


def assert_same(got, ref, what):
    """Bit for bit, +-0 equal, NaN equal to NaN (the reference's NaN payloads are the host's; the checker's need not be)."""
    got = np.asarray(got); ref = np.asarray(ref)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    if got.dtype != np.float32:
        assert np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} differ"
        return
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaN at {np.argwhere(gn != rn)[:5].tolist()}"
    assert_bits_equal(np.where(gn, 0, got), np.where(rn, 0, ref), what)


def where(bad_mask):
    idx = np.argwhere(bad_mask.reshape(bad_mask.shape[0], bad_mask.shape[1], -1).any(-1))
    return [(NAMES[m], int(i)) for m, i in idx[:6]]


@pytest.mark.parametrize("flavour", ["libm", "det"])
def test_bsdf_checker_equals_reference(flavour):
    """BSDFPdf, BSDFEval and BasisFromVector + BSDFSample (L, pdf, RNG state) over every material x case of the fixture."""
    from oracle import orc

    O = orc.Oracle(flavour)
    out = MG.bsdf_outputs(*MG.orc_fns(O.lib), MATS, G["N"], G["V"], G["L"], G["eta"], G["seed"])
    for key, got in out.items():
        ref = G[f"{flavour}.{key}"]
        try:
            assert_same(got, ref, f"{flavour} {key}")
        except AssertionError as e:
            bad = (np.isnan(got) != np.isnan(ref)) if got.dtype == np.float32 else (got != ref)
            if got.dtype == np.float32:
                bad |= ~np.isnan(ref) & (got.view(np.uint32) != ref.view(np.uint32)) & ~((got == 0) & (ref == 0))
            raise AssertionError(f"{e}; (material, case): {where(bad)}") from None


def test_fixture_reaches_the_edges():
    """The fixture's cases do reach what they were chosen for, in the reference's own outputs."""
    f, p = G["det.eval"], G["det.pdf"]
    k = int(G["n_constructed"])
    assert np.isnan(f).any() and np.isinf(f).any() and (p == 0).any()
    black = f[NAMES.index("black_tint")]
    assert np.isfinite(black).all(-1).sum() > k and (black > 0).any()  # Cdlum == 0 takes Ctint = 1, not 0/0 (Disney.cuh:330)
    assert (G["det.sample_pdf"][NAMES.index("glass133")] == 0).any()  # refraction past the critical angle
    assert not np.array_equal(G["libm.sample_L"].view(np.uint32), G["det.sample_L"].view(np.uint32))  # sinf/cosf: the flavours differ
    assert set(map(tuple, G["eta"].tolist())) == set(map(tuple, np.array(MG.ETA_PAIRS, np.float32).tolist()))
    assert {0, 1, 0xFFFFFFFF} <= set(G["seed"].tolist())


@pytest.mark.parametrize("flavour", ["libm", "det"])
def test_bsdf_eval_albedo_not_colour(flavour):
    """BSDFEval with an albedo other than the material colour (Disney.cuh:317 takes it separately)."""
    from oracle import orc

    O = orc.Oracle(flavour)
    k, n0 = MG.N_ALBEDO_GEO, int(G["n_constructed"])
    sl = slice(n0, n0 + k)
    got = MG.albedo_outputs(lambda *a: O.lib.orc_bsdf_eval(0, *a), MATS, NAMES, G["N"][sl], G["V"][sl], G["L"][sl], G["eta"][sl], k)
    assert_same(got, G[f"{flavour}.albedo_eval"], f"{flavour} BSDFEval(albedo)")


def cdf_cases():
    return [str(n) for n in G["cdf_names"]]


@pytest.mark.parametrize("name", cdf_cases())
def test_build_cdf_equals_reference(orc_libm, orc_det, name):
    """orc_build_cdf (both builds) and the product's host pt_build_cdf against the reference's BuildCDF.  Black rows and images,
    negative and NaN texels are not refused: the product computes what the reference computes, NaN and inf included."""
    data = G[f"cdf.{name}.data"]
    h, w = data.shape[:2]
    ref = [G[f"cdf.{name}.{k}"] for k in ("pdfX", "cdfX", "pdfY", "cdfY")]
    for who, got in (("libm checker", orc_libm.build_cdf(data, w, h)), ("det checker", orc_det.build_cdf(data, w, h)),
                     ("pt_build_cdf", _lib.build_cdf(data, w, h))):
        for k, g, r in zip(("pdfX", "cdfX", "pdfY", "cdfY"), got, ref):
            assert_same(g, r, f"{name} {who} {k}")


def test_build_cdf_fixture_reaches_the_edges():
    assert np.isnan(G["cdf.all_black.cdfY"]).all() and np.isnan(G["cdf.black_row.pdfX"][2]).all()
    assert np.isinf(G["cdf.near_flt_max.cdfX"]).any() or np.isnan(G["cdf.near_flt_max.cdfX"]).any()
    d = G["cdf.denormal.pdfX"]
    assert np.isfinite(d[0]).all() and (G["cdf.denormal.cdfY"][0] > 0)
    assert (G["cdf.negative_texel.pdfX"] < 0).any() and np.isnan(G["cdf.nan_texel.cdfY"]).all()
    sizes = {G[f"cdf.{n}.data"].shape[:2] for n in cdf_cases()}
    for edge in (1, 63, 64, 65, 127, 128, 129):
        assert any(edge in s for s in sizes), edge


def _imports(path):
    out = subprocess.run(["nm", "-D", "--undefined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_live_against_reference_disney():
    """Where oracle/_ref exists: the two reference libraries import no optix* / cuda* symbol (the stand-ins define nothing they
    call), the det one no libm transcendental, and fresh random inputs give the checker's bits.  Elsewhere: the fixture's inputs
    are the ones its generator makes, so the fixture and tests/golden/make_disney_golden.py cannot drift apart."""
    from oracle import orc

    libs = {fl: orc.load_ref_disney(fl) for fl in MG.FLAVOURS}
    if any(R is None for R in libs.values()):
        N, V, L, eta, seed, k = MG.geometry()
        for key, a in (("N", N), ("V", V), ("L", L), ("eta", eta), ("seed", seed)):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), G[key].view(np.uint32)), key
        assert k == int(G["n_constructed"]) and MG.materials()[0] == NAMES
        assert all(np.array_equal(G[f"cdf.{n}.data"].view(np.uint32), a.view(np.uint32)) for n, a in MG.cdf_images())
        return
    for fl, R in libs.items():
        syms = _imports(R.path)
        assert not [s for s in syms if s.lower().startswith(("optix", "cuda", "cu"))], f"{fl}: {sorted(syms)}"
        tr = sorted(s for s in syms if LIBM_TRANSCENDENTAL.match(s))
        if fl == "det":
            assert not tr, f"det reference imports libm transcendentals {tr}"
        else:
            assert tr, "the glibc reference imports no transcendental: the symbol check would not see one"
    rng = np.random.default_rng(int.from_bytes(os.urandom(4), "little"))
    n = 400
    N = MG._unit(rng.standard_normal((n, 3))); V = MG._unit(rng.standard_normal((n, 3))); L = MG._unit(rng.standard_normal((n, 3)))
    eta = np.array([MG.ETA_PAIRS[i] for i in rng.integers(0, len(MG.ETA_PAIRS), n)], np.float32)
    seed = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    mats = MATS + [scenes.Material(color=tuple(rng.random(3)), roughness=float(rng.random()), metallic=float(rng.random() < 0.3),
                                   transmission=float(rng.random() < 0.3), subsurface=float(rng.random()), clearcoat=float(rng.random()),
                                   clearcoatGloss=float(rng.random()), specularTint=float(rng.random()), eta=float(rng.choice([0.0, 1.33])))
                   for _ in range(4)]
    for fl, R in libs.items():
        O = orc.Oracle(fl)
        got = MG.bsdf_outputs(*MG.orc_fns(O.lib), mats, N, V, L, eta, seed)
        ref = MG.bsdf_outputs(*MG.ref_fns(R), mats, N, V, L, eta, seed)
        for key in got:
            assert_same(got[key], ref[key], f"live {fl} {key}")
        w, h = (int(x) for x in rng.integers(1, 140, 2))
        img = (rng.random((h, w, 4)) * rng.choice([1e-40, 1.0, 1e30])).astype(np.float32)
        out = [np.zeros((h, w), np.float32), np.zeros((h, w), np.float32), np.zeros(h, np.float32), np.zeros(h, np.float32)]
        R.ref_build_cdf(img.reshape(-1), w, h, out[0].reshape(-1), out[1].reshape(-1), out[2], out[3])
        for g, r in zip(O.build_cdf(img, w, h), out):
            assert_same(g, r, f"live {fl} BuildCDF {w}x{h}")
