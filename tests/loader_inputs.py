"""The seeded random inputs of the live loader tests (tests/test_objloader.py, tests/test_hdrloader.py): OBJ / MTL / PNG sets, boxes, a
file of many quads, RGBE images.  tests/golden/make_live_golden.py records the reference's answers on the very same inputs."""
import os

import numpy as np

import conftest  # noqa: F401  (puts the repository's root on sys.path)
from optixpathtracer_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "obj_fixture")


def _num(rng, v):
    """One number in one of the spellings tryParseDouble accepts."""
    k = rng.integers(0, 6)
    if k == 0:
        return repr(round(float(v), int(rng.integers(0, 12))))
    if k == 1:
        return f"{v:.{int(rng.integers(0, 10))}e}"
    if k == 2:
        return f"{v:+.{int(rng.integers(1, 16))}f}"
    if k == 3:
        return str(int(v))
    if k == 4:
        s = f"{v:.5f}"
        return s.replace("0.", ".", 1) if abs(v) < 1 else s
    return f"{v:.{int(rng.integers(1, 9))}g}".replace("e", "E")


def _random_set(rng, d):
    from PIL import Image

    ntex = int(rng.integers(1, 4))
    for t in range(ntex):
        h, w = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        mode = ["RGB", "RGBA", "L"][int(rng.integers(0, 3))]
        shape = (h, w) if mode == "L" else (h, w, len(mode))
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8), mode).save(os.path.join(d, f"t{t}.png"))
    nmat = int(rng.integers(1, 5))
    mtl = []
    for m in range(nmat):
        mtl.append(f"newmtl m{m}")
        if rng.random() < 0.7:
            mtl.append("Kd " + " ".join(_num(rng, x) for x in rng.random(3)))
        if rng.random() < 0.5:
            mtl.append("Ke " + " ".join(_num(rng, x) for x in rng.random(3) * 5))
        if rng.random() < 0.6:
            mtl.append(f"map_Kd t{int(rng.integers(0, ntex + 1))}.png")  # one id past the end: a missing file
    open(os.path.join(d, "r.mtl"), "w").write("\n".join(mtl) + "\n")
    nv, nvt, nvn = int(rng.integers(4, 40)), int(rng.integers(1, 12)), int(rng.integers(1, 8))
    P = rng.standard_normal((nv, 3)) * np.exp(rng.uniform(-3, 3))
    lines = ["mtllib r.mtl"]
    lines += ["v " + " ".join(_num(rng, x) for x in p) for p in P]
    lines += ["vt " + " ".join(_num(rng, x) for x in rng.random(2)) for _ in range(nvt)]
    lines += ["vn " + " ".join(_num(rng, x) for x in rng.standard_normal(3)) for _ in range(nvn)]
    lines.append("usemtl m0")
    for _ in range(int(rng.integers(3, 30))):
        r = rng.random()
        if r < 0.12:
            lines.append(["o obj", "g grp", "g"][int(rng.integers(0, 3))])
        elif r < 0.3:
            lines.append(f"usemtl m{int(rng.integers(0, nmat))}")
        else:
            n = int(rng.choice([3, 3, 3, 4, 4, 5, 6, 7, 9]))
            style = int(rng.integers(0, 4))
            if rng.random() < 0.5:  # a planar polygon (often concave, sometimes self-intersecting): project random points of a plane
                ids = rng.choice(nv, size=min(n, nv), replace=False)
            else:
                ids = rng.integers(0, nv, n)
            toks = []
            for vi in ids:
                a = int(vi) + 1 if rng.random() < 0.7 else int(vi) - nv
                b = int(rng.integers(1, nvt + 1)) if rng.random() < 0.7 else -int(rng.integers(1, nvt + 1))
                c = int(rng.integers(1, nvn + 1))
                toks.append([f"{a}", f"{a}/{b}", f"{a}//{c}", f"{a}/{b}/{c}"][style if rng.random() < 0.85 else int(rng.integers(0, 4))])
            lines.append("f " + " ".join(toks))
    open(os.path.join(d, "r.obj"), "w").write("\n".join(lines) + "\n")
    return os.path.join(d, "r.obj")


def random_sets(d):
    """The 150 random OBJ / MTL / PNG sets of test_load_obj_live_random, written under d (seeded): the OBJ paths."""
    rng = np.random.default_rng(2024)
    for it in range(150):
        s = os.path.join(d, f"s{it}")
        os.mkdir(s)
        yield _random_set(rng, s)


def live_boxes():
    rng = np.random.default_rng(5)
    return [(scenes.Material(color=rng.random(3), roughness=rng.random()), rng.standard_normal(3) * 10, rng.random(3) * 5) for _ in range(50)]


MANY_QUADS = 3000


def many_quads_file(d):
    """The OBJ (+ MTL) of test_load_obj_live_many_quads, written under d (seeded): its path."""
    rng = np.random.default_rng(12)
    n = MANY_QUADS
    V = (rng.standard_normal((4 * n, 3)) * np.exp(rng.uniform(-2, 2, (4 * n, 1)))).astype(np.float32)
    V[: 4 * 400, 1] = -1.5
    V[4 * 400: 4 * 600] = np.round(V[4 * 400: 4 * 600])
    open(os.path.join(d, "q.mtl"), "w").write("newmtl a\nKd 0.5 0.25 0.125\n")
    lines = ["mtllib q.mtl", "usemtl a"] + ["v %.9g %.9g %.9g" % tuple(p) for p in V] + ["f %d %d %d %d" % tuple(q) for q in np.arange(1, 4 * n + 1).reshape(n, 4)]
    open(os.path.join(d, "q.obj"), "w").write("\n".join(lines) + "\n")
    return os.path.join(d, "q.obj")


def _golden_module(name):
    import importlib.util

    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hdr_live_inputs(d):
    """The 40 random RGBE images of test_load_hdr_live_random, flat and run-length encoded, written under d (seeded): their paths."""
    mod = _golden_module("make_model_golden")
    rng = np.random.default_rng(5)
    for it in range(40):
        h, w = int(rng.integers(1, 12)), int(rng.choice([1, 7, 8, 9, 33, 128, 129, 500]))
        rgbe = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        if it % 3 == 0:
            rgbe[:, : w // 2] = rgbe[:, :1]  # long runs
        if it % 4 == 0:
            rgbe[..., 3] = rng.choice([0, 1, 127, 128, 129, 255], (h, w))
        path = os.path.join(d, f"r{it}.hdr")
        (mod.write_rle_hdr if (it % 2 == 0 and w >= 8) else mod.write_flat_hdr)(path, rgbe)
        yield path
