#!/usr/bin/env python3
"""Generates tests/golden/ref_live.json: SHA-256 digests of what the REFERENCE's own code (oracle/_ref/libptref.so) returns for the
inputs of the *_live tests — tests/test_hdrloader.py::test_load_hdr_live_random, the test_*_live tests of tests/test_objloader.py and
tests/test_oracle_golden.py::test_live_against_reference_headers.  Their inputs are seeded (the header test's at HEADER_SEED), so where
libptref.so is not built the tests check the same inputs against these digests; where it is built they run against the library.
Every array is digested with its dtype and shape, so a digest match is the tests' bit-for-bit comparison.
Run where oracle/_ref/libptref.so was built:  python tests/golden/make_live_golden.py"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
OUT = os.path.join(HERE, "ref_live.json")
HEADER_SEED = 20261015  # test_live_against_reference_headers without the library: these inputs instead of fresh random ones


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape};".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def model_digest(meshes, textures):
    """Digest of ([mesh dict], [texture]) as oracle.orc.ref_model_arrays returns them (model_fields: the same of a scenes.Model)."""
    parts = []
    for m in meshes:
        parts += [m["vertex"], m["index"], m["normal"], m["texcoord"], np.frombuffer(np.array(m["material"]).tobytes(), np.uint8),
                  np.int64(m["diffuseTextureID"])]
    return digest(np.int64(len(meshes)), np.int64(len(textures)), *parts, *textures)


def model_fields(model):
    """A scenes.Model in the reference's layout: absent normals / texcoords are empty arrays (what test_objloader._check_model compares)."""
    meshes = [dict(vertex=m.vertex, index=m.index, normal=m.normal if m.normal is not None else np.zeros((0, 3), np.float32),
                   texcoord=m.texcoord if m.texcoord is not None else np.zeros((0, 2), np.float32), material=m.material,
                   diffuseTextureID=m.diffuseTextureID) for m in model.meshes]
    return meshes, [t.pixel for t in model.textures]


def header_outputs(lib, prefix, seed, n=300):
    """test_live_against_reference_headers' calls on one library — the checker's orc_* or the reference's ref_* — for the inputs of
    `seed`: one tuple of arrays per case (rand state and values, tea4, basis, make_color; -0 as +0, which the test's == does not tell apart)."""
    fn = lambda name: getattr(lib, prefix + name)  # noqa: E731
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        s = int(rng.integers(0, 2**32))
        st = np.zeros(2, np.uint32)
        fn("random_init")(st, s)
        vals, states = [], []
        for _ in range(8):
            vals.append(fn("randf")(st))
            states.append(st.copy())
        tea = fn("tea4")(s, 3)
        d = rng.standard_normal(3).astype(np.float32); d /= np.linalg.norm(d)
        x = np.zeros(3, np.float32); u = np.zeros(3, np.float32)
        fn("basis_from_vector")(d, x, u)
        c = (rng.random(3) * 1.2 - 0.1).astype(np.float32)
        color = fn("make_color")(c)
        out.append((np.array(vals, np.float32) + np.float32(0), np.array(states), np.uint32(tea), x + np.float32(0), u + np.float32(0), np.uint32(color)))
    return out


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    import loader_inputs as T

    from oracle import orc

    R = orc.load_ref()
    if R is None or not hasattr(R, "refm_load_obj") or not hasattr(R, "refm_loadf"):
        raise SystemExit("oracle/_ref/libptref.so with the Model.cpp and stb_image shims is missing: run `make -C oracle ref` where the reference's sources lie")
    G = {"header_seed": HEADER_SEED}
    with tempfile.TemporaryDirectory() as d:
        G["hdr_live"] = [digest(orc.ref_loadf(R, path)) for path in T.hdr_live_inputs(d)]
    G["obj_fixture"] = {}
    for name in ("basic", "concave", "numbers", "quirks"):
        G["obj_fixture"][name] = model_digest(*orc.ref_load_obj(R, os.path.join(T.FIX, name + ".obj")))
    meshes, textures = orc.ref_load_obj(R, os.path.join(T.FIX, "images.obj"))
    G["obj_fixture"]["images"] = model_digest(meshes, textures[:3])  # (the JPEG, texture 3, is compared with a tolerance in the golden test)
    with tempfile.TemporaryDirectory() as d:
        G["obj_random"] = [model_digest(*orc.ref_load_obj(R, path)) for path in T.random_sets(d)]
    G["add_box"] = model_digest(orc.ref_add_boxes(R, T.live_boxes()), [])
    with tempfile.TemporaryDirectory() as d:
        G["many_quads"] = model_digest(*orc.ref_load_obj(R, T.many_quads_file(d)))
    G["headers"] = [digest(*case) for case in header_outputs(R, "ref_", HEADER_SEED)]
    with open(OUT, "w") as f:
        json.dump(G, f, indent=0)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
