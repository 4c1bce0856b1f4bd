"""Scene ingestion pinned to the reference's own code: optixpathtracer_amd/objloader.py (loadOBJ, addVertex, loadTexture) and
scenes.add_box against what HelloPathtracing_original/Model.cpp:51-286 — compiled from where it lies, with the tinyobjloader and
stb_image it vendors, into oracle/_ref/libptref.so — makes of the same files.  Bit for bit, mesh order included.

  * test_*_golden: the committed inputs (tests/golden/obj_fixture/, written by tests/golden/make_model_golden.py) against the
    reference's stored outputs (tests/golden/ref_model.npz) — runs anywhere;
  * test_*_live: seeded random OBJ / MTL / PNG sets against libptref.so directly where the library was built, and against the digests
    of its outputs for the same files (tests/golden/ref_live.json, tests/golden/make_live_golden.py) everywhere else.

Two implementations are held to the reference: the native parser behind the C ABI (pt_load_obj, csrc/pt_objload.cpp — the product's
route, `native=True`, the default) and the line-cited Python restatement it was written from (`native=False`)."""
import os

import numpy as np
import pytest

from loader_inputs import FIX, HERE, MANY_QUADS, live_boxes, many_quads_file, random_sets
from optixpathtracer_amd import objloader, scenes



def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_model(model, meshes, textures, what):
    assert len(model.meshes) == len(meshes), (what, len(model.meshes), len(meshes))
    assert len(model.textures) == len(textures), what
    for i, (m, r) in enumerate(zip(model.meshes, meshes)):
        w = f"{what} mesh {i}"
        assert _same_bits(m.vertex, r["vertex"]), w
        assert _same_bits(m.index, r["index"]), (w, m.index, r["index"])
        nrm = m.normal if m.normal is not None else np.zeros((0, 3), np.float32)
        tc = m.texcoord if m.texcoord is not None else np.zeros((0, 2), np.float32)
        assert _same_bits(nrm, r["normal"]), w
        assert _same_bits(tc, r["texcoord"]), w
        assert np.array(m.material).tobytes() == np.array(r["material"]).tobytes(), (w, m.material, r["material"])
        assert m.diffuseTextureID == r["diffuseTextureID"], w
    for i, (t, r) in enumerate(zip(model.textures, textures)):
        assert _same_bits(t.pixel, r), f"{what} texture {i}"


def _unpack(G, prefix):
    nm, nt = G[prefix + "n"]
    meshes = []
    for i in range(nm):
        mat = np.frombuffer(G[f"{prefix}m{i}_material"].tobytes(), scenes.MATERIAL_DTYPE)[0]
        meshes.append(dict(vertex=G[f"{prefix}m{i}_vertex"], normal=G[f"{prefix}m{i}_normal"], texcoord=G[f"{prefix}m{i}_texcoord"],
                           index=G[f"{prefix}m{i}_index"], material=mat, diffuseTextureID=int(G[f"{prefix}m{i}_tex"])))
    return meshes, [G[f"{prefix}t{i}"] for i in range(nt)]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "ref_model.npz"))


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("name", ["basic", "concave", "numbers", "quirks"])
def test_load_obj_golden(golden, name, native):
    meshes, textures = _unpack(golden, name + "_")
    assert len(meshes) > 0
    _check_model(objloader.load_obj(os.path.join(FIX, name + ".obj"), native=native), meshes, textures, name)


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_load_obj_golden_image_formats(golden, native):
    """loadTexture's other formats: the reference decodes with stb_image, this package with PIL.  TGA — true
    colour, run-length encoded with alpha, grey — is lossless: the texels must equal the reference's bit for bit.  JPEG is not: two conforming
    decoders may differ in a texel's last bits (stb_image has its own IDCT and chroma upsampling); the bound asserted here, 3 of 255 per channel,
    is what INTEGRATION.md states.  (Three of the four materials' meshes are dropped or shrunk by the reference: the shared vertex map.)"""
    meshes, textures = _unpack(golden, "images_")
    assert len(textures) == 4 and len(meshes) == 2
    m = objloader.load_obj(os.path.join(FIX, "images.obj"), native=native)
    _check_model(scenes.Model(meshes=m.meshes, textures=m.textures[:3]), meshes, textures[:3], "images (TGA)")
    assert textures[0].shape == (7, 5) and textures[1].shape == (4, 9) and textures[2].shape == (3, 4)
    assert (textures[0] >> 24 == 255).all() and not (textures[1] >> 24 == 255).all()  # alpha filled in / alpha decoded
    got, ref = m.textures[3].pixel, textures[3]
    assert got.shape == ref.shape == (16, 24)
    diff = np.abs(got.view(np.uint8).astype(np.int32) - ref.view(np.uint8).astype(np.int32))
    assert diff.max() <= 3, diff.max()
    print(f"\n[jpeg] PIL vs stb_image: {int((diff > 0).sum())} of {diff.size} channel values differ, max {int(diff.max())}")


def test_load_obj_golden_covers_the_quirks(golden):
    """What the fixture is there for, read off the reference's stored output (so that an edit of the inputs cannot silently drop a case)."""
    meshes, textures = _unpack(golden, "basic_")
    assert len(textures) == 5  # rgb, rgba, gray, rgb AGAIN (knownTextures is per shape, Model.cpp:177), bmp; the missing file gave none
    assert sum(1 for m in meshes if m["diffuseTextureID"] == -1) >= 3
    lit = meshes[1]  # shape `quad`: red (id 0) first, lit (id 1) second — std::set order, not file order
    assert lit["diffuseTextureID"] == 0 and tuple(int(x) for x in lit["index"][0][:2]) == (5, 4)  # vertex numbers of the RED mesh: the shared knownVertices map (:176)
    assert len(lit["texcoord"]) == len(lit["vertex"]) == len(lit["normal"])  # zero-padded / back-filled (:68-81)
    assert textures[0].shape == (5, 8) and textures[1].shape == (4, 6) and textures[2].shape == (6, 3)
    q, _ = _unpack(golden, "quirks_")
    assert np.allclose(q[0]["material"]["color"], 0.6) and np.allclose(q[2]["material"]["color"], 0.0)  # has_kd is never reset (tiny_obj_loader.h:1703)
    c, _ = _unpack(golden, "concave_")
    assert len(c[0]["index"]) >= 4 + 4 + 6 + 2 + 3 + 5  # ear clipping produced the triangles of the concave polygons


def test_add_box_golden(golden):
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_model_golden", os.path.join(HERE, "golden", "make_model_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    meshes, _ = _unpack(golden, "boxes_")
    model = scenes.Model()
    for kw, pos, ext in mod.BOXES:
        scenes.add_box(model, scenes.Material(**kw), pos, ext)
    _check_model(model, meshes, [], "addBox")
    assert meshes[0]["vertex"].shape == (36, 3) and meshes[0]["index"].shape == (12, 3) and meshes[0]["texcoord"].shape == (36, 2)


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_per_mesh_vertex_map_option(tmp_path, native):
    """The repair of the shared vertex map (what load_model, the product's route for rendering, uses): every mesh indexes its own vertices;
    the shared-map mode does not on this fixture (the reference's out-of-bounds indices, kept for parity)."""
    m = objloader.load_obj(os.path.join(FIX, "basic.obj"), per_mesh_vertex_map=True, native=native)
    for mesh in m.meshes:
        assert mesh.index.max() < len(mesh.vertex)
    v, idx, tri_mesh, mats = m.flatten()
    assert idx.max() < len(v)
    shared = objloader.load_obj(os.path.join(FIX, "basic.obj"), native=native)
    assert any(mesh.index.max() >= len(mesh.vertex) for mesh in shared.meshes)


def test_load_model_is_the_native_per_mesh_route():
    a = objloader.load_model(os.path.join(FIX, "basic.obj"))
    b = objloader.load_obj(os.path.join(FIX, "basic.obj"), per_mesh_vertex_map=True, native=False)
    assert len(a.meshes) == len(b.meshes) and len(a.textures) == len(b.textures)
    for x, y in zip(a.meshes, b.meshes):
        assert _same_bits(x.vertex, y.vertex) and _same_bits(x.index, y.index) and x.diffuseTextureID == y.diffuseTextureID
        assert np.array(x.material).tobytes() == np.array(y.material).tobytes()


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_load_obj_errors(tmp_path, native):
    with pytest.raises(RuntimeError):
        objloader.load_obj(str(tmp_path / "absent.obj"), native=native)
    p = tmp_path / "zero.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n")  # index 0: tinyobj fails the load, loadOBJ throws (Model.cpp:160-162)
    with pytest.raises(RuntimeError):
        objloader.load_obj(str(p), native=native)
    q = tmp_path / "range.obj"
    q.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 7\n")  # a vertex that does not exist: the reference reads past its array, both loaders refuse
    with pytest.raises(ValueError):
        objloader.load_obj(str(q), native=native)


def test_native_loader_speed(tmp_path):
    """the Python restatement needs 26-50 s for the 150 MB OBJ of the textured 1 M-triangle terrain; the native parser
    must do a comparable file in seconds.  Here: 300 k triangles with normals and texcoords (45 MB of text), bound 5 s, both loaders equal."""
    import time

    rng = np.random.default_rng(3)
    n = 100_000
    V = rng.standard_normal((3 * n, 3)).astype(np.float32)
    VT = rng.random((3 * n, 2)).astype(np.float32)
    lines = ["v %.9g %.9g %.9g" % tuple(p) for p in V] + ["vt %.9g %.9g" % tuple(p) for p in VT] + ["vn 0 1 0"]
    lines += ["f %d/%d/1 %d/%d/1 %d/%d/1" % (a, a, b, b, c, c) for a, b, c in np.arange(1, 3 * n + 1).reshape(n, 3)] * 3
    path = tmp_path / "big.obj"
    path.write_text("\n".join(lines) + "\n")
    t0 = time.perf_counter()
    a = objloader.load_obj(str(path), native=True)
    dt = time.perf_counter() - t0
    assert len(a.meshes) == 1 and len(a.meshes[0].index) == 3 * n and len(a.meshes[0].vertex) == 3 * n
    assert dt < 5.0, dt
    print(f"\n[pt_load_obj] {os.path.getsize(path) / 1e6:.0f} MB, {3 * n} triangles in {dt:.2f} s")


# ----------------------------------------------------------------------------------------------------------------- live


def _live_golden():
    import importlib.util
    import json

    spec = importlib.util.spec_from_file_location("make_live_golden", os.path.join(HERE, "golden", "make_live_golden.py"))
    LG = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(LG)
    return LG, json.load(open(LG.OUT))


def _ref():
    """(orc, libptref.so) where the library with the Model.cpp shims is built, else (None, (make_live_golden module, stored digests))."""
    from oracle import orc

    R = orc.load_ref()
    if R is None or not hasattr(R, "refm_load_obj"):
        return None, _live_golden()
    return orc, R


def _check_live(orc, R, model, ref_out, digest_of, what):
    """model against the reference's ([meshes], [textures]): ref_out() from the library, or without it the stored digest digest_of(stored)."""
    if orc is None:
        LG, stored = R
        assert LG.model_digest(*LG.model_fields(model)) == digest_of(stored), what
    else:
        out = ref_out()
        assert out is not None, what
        _check_model(model, out[0], out[1], what)


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_load_obj_live_fixture(native):
    orc, R = _ref()
    for name in ("basic", "concave", "numbers", "quirks"):
        path = os.path.join(FIX, name + ".obj")
        _check_live(orc, R, objloader.load_obj(path, native=native), lambda: orc.ref_load_obj(R, path), lambda G: G["obj_fixture"][name], name)
    # TGA live (the JPEG, texture 3, is compared with a tolerance in the golden test)
    m = objloader.load_obj(os.path.join(FIX, "images.obj"), native=native)
    _check_live(orc, R, scenes.Model(meshes=m.meshes, textures=m.textures[:3]), lambda: (lambda o: (o[0], o[1][:3]))(orc.ref_load_obj(R, os.path.join(FIX, "images.obj"))),
                lambda G: G["obj_fixture"]["images"], "images")


def test_load_obj_live_random(tmp_path):
    """150 random OBJ / MTL / PNG sets through the reference's loadOBJ and through objloader.load_obj."""
    orc, R = _ref()
    total_tris = 0
    for it, path in enumerate(random_sets(str(tmp_path))):
        native = objloader.load_obj(path, native=True)
        _check_live(orc, R, native, lambda: orc.ref_load_obj(R, path), lambda G: G["obj_random"][it], f"random set {it} (native)")
        _check_live(orc, R, objloader.load_obj(path, native=False), lambda: orc.ref_load_obj(R, path), lambda G: G["obj_random"][it], f"random set {it} (python)")
        total_tris += sum(len(m.index) for m in native.meshes)  # (the reference's count: the check above holds the index arrays equal)
    assert total_tris > 1500


def test_add_box_live():
    orc, R = _ref()
    boxes = live_boxes()
    model = scenes.Model()
    for mat, pos, ext in boxes:
        scenes.add_box(model, mat, pos, ext)
    _check_live(orc, R, model, lambda: (orc.ref_add_boxes(R, boxes), []), lambda G: G["add_box"], "addBox live")


def test_batched_quad_triangulation_equals_scalar_ear_clipping():
    """objloader decides for many 4-gons at once whether tinyobjloader's ear clipping yields the plain fan; everything else runs the
    scalar restatement.  Random quads — convex, concave, self-intersecting, degenerate, in arbitrary planes — must come out of both paths
    with the same triangles."""
    rng = np.random.default_rng(11)
    n = 4000
    V = (rng.standard_normal((4 * n, 3)) * np.exp(rng.uniform(-2, 2, (4 * n, 1)))).astype(np.float32)
    V[: 4 * 500, 2] = 0.25                      # planar quads
    V[4 * 500: 4 * 700] = np.round(V[4 * 500: 4 * 700])  # small-integer coordinates: collinear and coincident corners
    V[4 * 700: 4 * 704] = 0.0
    Q = np.arange(4 * n, dtype=np.int64).reshape(n, 4)
    fan = objloader._quads_clip_to_fan(Q, V)
    assert 0.3 < fan.mean() < 0.95
    for i in range(n):
        face = [(int(v), -1, -1) for v in Q[i]]
        tris = objloader._triangulate(face, V)
        want_fan = [(face[0], face[1], face[2]), (face[0], face[2], face[3])]
        if fan[i]:
            assert tris == want_fan, i
    # and end to end: a file of quads goes through the batch path and must equal the reference's stored / live result elsewhere;
    # here: the same file parsed with the batch disabled gives the same model
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        lines = ["v %.9g %.9g %.9g" % tuple(p) for p in V[: 4 * 800]] + ["f %d %d %d %d" % tuple(q + 1) for q in Q[:800]]
        path = os.path.join(d, "q.obj")
        open(path, "w").write("\n".join(lines) + "\n")
        a = objloader.load_obj(path, native=False)
        saved = objloader._quads_clip_to_fan
        try:
            objloader._quads_clip_to_fan = lambda Q, V: np.zeros(len(Q), bool)
            b = objloader.load_obj(path, native=False)
        finally:
            objloader._quads_clip_to_fan = saved
        c = objloader.load_obj(path, native=True)  # the native parser only has the scalar ear clipping
        assert len(a.meshes) == len(b.meshes) == len(c.meshes) == 1
        assert a.meshes[0].index.tobytes() == b.meshes[0].index.tobytes() == c.meshes[0].index.tobytes()
        assert a.meshes[0].vertex.tobytes() == b.meshes[0].vertex.tobytes() == c.meshes[0].vertex.tobytes()


def test_load_obj_live_many_quads(tmp_path):
    """A file with thousands of random 4-gons (the batched triangulation path of objloader) against the reference's loadOBJ."""
    orc, R = _ref()
    path = many_quads_file(str(tmp_path))
    native = objloader.load_obj(path, native=True)
    _check_live(orc, R, native, lambda: orc.ref_load_obj(R, path), lambda G: G["many_quads"], "many quads (native)")
    _check_live(orc, R, objloader.load_obj(path, native=False), lambda: orc.ref_load_obj(R, path), lambda G: G["many_quads"], "many quads (python)")
    assert len(native.meshes[0].index) > 1.5 * MANY_QUADS


def test_native_loader_refuses_a_directory_without_throwing():
    """pt_load_obj itself (not only the Python wrapper's isfile check) must refuse a path that is a directory — fopen opens
    it and ftell reports a huge size — and no C++ exception may cross the C ABI."""
    import ctypes as C

    from optixpathtracer_amd import _lib

    L = _lib.load_library()
    L.pt_load_obj.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    L.pt_obj_last_error.restype = C.c_char_p
    h = C.c_void_p()
    assert L.pt_load_obj(os.fsencode(FIX), 1, C.byref(h)) != 0 and not h.value
    assert b"Cannot open file" in L.pt_obj_last_error()


def test_native_loader_non_ascii_directory(tmp_path):
    """texture paths come back through the file system's codec (os.fsdecode), so a model directory with a non-ASCII name
    keeps its textures."""
    import shutil

    d = tmp_path / "modèle_日本"
    shutil.copytree(FIX, d)
    a = objloader.load_obj(os.path.join(FIX, "basic.obj"), native=True)
    b = objloader.load_obj(str(d / "basic.obj"), native=True)
    assert len(a.textures) == len(b.textures) and len(a.textures) > 0
    assert [m.diffuseTextureID for m in a.meshes] == [m.diffuseTextureID for m in b.meshes]
    assert any(m.diffuseTextureID >= 0 for m in b.meshes)


def test_number_grammar_native_equals_restatement(tmp_path):
    """The decimal-field reader (tinyobjloader's tryParseDouble, restated in pt_objload.cpp and in objloader.py) on the grammar's corners: the native
    parser and the line-cited Python restatement produce the same float32 bits for every field, accepted or defaulted."""
    fields = ["1", "-1", "+1", "0", "-0", ".5", "-.5", "+.5", ".", "-.", "1.", "1.e2", ".e2", "1e", "1e+", "1e-", "1ex", "1x", "1.5x", "x", "e5", "--1", "+", "-",
              "1e5", "1E5", "1e-5", "1e+05", "12345678.123456789012", "0.1234567", "0.12345678", "0.123456789", "3.14159265358979", "1e38", "1e39", "1e-46",
              "1e400", "1e-400", "1e99999999999", "-1e99999999999", "1e-99999999999", "0e99999999999", "123456789012345678901234567890", "1.5e3.2", "7e2e3",
              "00012", "1.0000000000000000000000001", "4.9e-324", "2.2250738585072014e-308", "9007199254740993"]
    lines = [f"v {f} 0 0" for f in fields] + [f"v 0 {f} {f}" for f in fields]
    n = len(lines)
    faces = [f"f {k + 1} {(k + 1) % n + 1} {(k + 2) % n + 1}" for k in range(n)]
    p = tmp_path / "numbers.obj"
    p.write_text("\n".join(lines + faces) + "\n")
    a = objloader.load_obj(str(p), per_mesh_vertex_map=True, native=True)
    b = objloader.load_obj(str(p), per_mesh_vertex_map=True, native=False)
    assert len(a.meshes) == len(b.meshes) == 1
    assert _same_bits(a.meshes[0].vertex, b.meshes[0].vertex) and _same_bits(a.meshes[0].index, b.meshes[0].index)
