"""float32 NumPy evaluation of pt_copy_texcoords_device's table and pt_surface_planes' arithmetic, written from the text of include/pt_amd.h
alone; shared by tests/test_surface_cabi.py and tests/test_gpu_surface.py.  A helper, not a test.  One rounding per operation, in the header's
order, no fused multiply-add; it never calls the kernel under test.  Everything scene-side comes from the Model's host arrays."""
import numpy as np

import temporal_ref as T

f32 = np.float32
SENTINEL = T.SENTINEL
PLANES = ("albedo", "texcoord")
WORDS = {"albedo": 4, "texcoord": 2}
ONE = 0x3F800000
TEX_CAMERA = dict(eye=(2.0, 1.5, -3.0), lookat=(0.0, 0.6, 0.5), up=(0.0, 1.0, 0.0), fovY=35.0)  # the camera the tests put on textured_scene()


def textured_scene():
    """scenes.textured_scene() with what its docstring promises: the box NAMES texture 0 and has NO texcoords, so it keeps its material
    colour (add_box gives every box a zero texcoord array, which would make the box a textured mesh looked up at (0, 0))."""
    from optixpathtracer_amd import scenes

    m = scenes.textured_scene()
    m.meshes[2].texcoord = None
    return m


def scene_arrays(model):
    """What the pass reads of the scene, from the model's host arrays:
    tri_mesh (T,) the mesh of every primitive in global order; color (M, 3) float32; mesh_tex (M,) the texture id of a mesh that has one AND
    texcoords, else -1; uv (T, 6) float32: pt_copy_texcoords_device's table (all zeros when no mesh is textured); textures: [(h, w) uint32]"""
    tri_mesh, uv, mesh_tex = [], [], []
    for mi, m in enumerate(model.meshes):
        idx = np.asarray(m.index, np.int64).reshape(-1, 3)
        tri_mesh.append(np.full(len(idx), mi, np.int64))
        has_uv = m.texcoord is not None and len(m.texcoord) > 0
        mesh_tex.append(int(m.diffuseTextureID) if (has_uv and m.diffuseTextureID >= 0) else -1)
        tc = np.ascontiguousarray(m.texcoord, f32).reshape(-1, 2) if has_uv else np.zeros((len(m.vertex), 2), f32)
        uv.append(tc[idx].reshape(-1, 6))  # uv0.xy, uv1.xy, uv2.xy
    mesh_tex = np.array(mesh_tex, np.int64)
    uv = np.ascontiguousarray(np.concatenate(uv), f32)
    if not (mesh_tex >= 0).any():
        uv = np.zeros_like(uv)
    color = np.array([[f32(c) for c in m.material["color"]] for m in model.meshes], f32).reshape(-1, 3)
    return dict(tri_mesh=np.concatenate(tri_mesh), color=color, mesh_tex=mesh_tex, uv=uv, textures=[np.ascontiguousarray(t.pixel, np.uint32) for t in model.textures])


def tex2d(pixel, s, t):
    """the header's tex2D: pixel (H, W) uint32 RGBA8, row 0 first; s, t float32 arrays (n,).  Returns (n, 4) float32."""
    pixel = np.asarray(pixel, np.uint32)
    H, W = pixel.shape
    s, t = np.asarray(s, f32).reshape(-1), np.asarray(t, f32).reshape(-1)
    with np.errstate(all="ignore"):
        x, y = (s - np.floor(s)) * f32(W), (t - np.floor(t)) * f32(H)
        xB, yB = x - f32(0.5), y - f32(0.5)
        fi, fj = np.floor(xB), np.floor(yB)
        alpha = np.floor(((xB - fi) * f32(256.0)) + f32(0.5)) * f32(1.0 / 256.0)
        beta = np.floor(((yB - fj) * f32(256.0)) + f32(0.5)) * f32(1.0 / 256.0)
        ii = np.where(np.isfinite(fi), fi, f32(0)).astype(np.int64)  # a non-finite coordinate reads texel 0 (and gives NaN weights)
        jj = np.where(np.isfinite(fj), fj, f32(0)).astype(np.int64)
        i0, i1, j0, j1 = np.mod(ii, W), np.mod(ii + 1, W), np.mod(jj, H), np.mod(jj + 1, H)

        def T_(i, j):
            p = pixel[j, i]
            return (np.stack([(p >> (8 * k)) & 0xFF for k in range(4)], -1).astype(f32)) / f32(255.0)

        a, b = alpha[:, None], beta[:, None]
        one = f32(1.0)
        out = ((((one - a) * (one - b)) * T_(i0, j0) + (a * (one - b)) * T_(i1, j0)) + ((one - a) * b) * T_(i0, j1)) + (a * b) * T_(i1, j1)
    for arr in (x, xB, fi, alpha, beta, out):
        assert arr.dtype == f32
    return out


def surface_ref(hit, scene, pixels, planes=PLANES, fill=SENTINEL):
    """hit: (h, w, 8) float32 or its uint32 bits; scene: scene_arrays(model); pixels: bool (h, w), the set the call processes.
    Returns {plane: uint32 bits of the whole plane, `fill` outside the set; hits, stale, textured: int; kind: int8 (h, w): 0 outside the
    set, 1 a hit on the colour path, 2 a miss, 3 stale, 4 a hit on the texture path; st: (h, w, 2) float32 (s, t), 0 where no lookup ran;
    mesh: int (h, w), -1 where there is no hit in range}."""
    hit = np.ascontiguousarray(hit)
    hit = hit.view(f32) if hit.dtype == np.uint32 else np.ascontiguousarray(hit, f32)
    h, w = hit.shape[:2]
    ntri = len(scene["tri_mesh"])
    pixels = np.asarray(pixels, bool)
    Y, X = np.nonzero(pixels)
    n = len(Y)
    rec = hit[Y, X]
    prim = rec.view(np.int32)[:, 3].astype(np.int64)
    miss = prim < 0
    is_hit = ~miss & (prim < ntri)
    stale = ~miss & ~is_hit
    mesh = np.where(is_hit, scene["tri_mesh"][np.where(is_hit, prim, 0)], -1)
    tid = np.where(is_hit, scene["mesh_tex"][np.maximum(mesh, 0)], -1)
    tex = tid >= 0
    alb = np.zeros((n, 4), f32)
    alb[:, 3] = 1
    alb[is_hit, 0:3] = scene["color"][mesh[is_hit]]
    st = np.zeros((n, 2), f32)
    with np.errstate(all="ignore"):
        c = scene["uv"][np.where(tex, prim, 0)]
        u, v = rec[:, 1], rec[:, 2]
        w0 = (f32(1.0) - u) - v
        s = ((w0 * c[:, 0]) + (u * c[:, 2])) + (v * c[:, 4])
        t = ((w0 * c[:, 1]) + (u * c[:, 3])) + (v * c[:, 5])
        assert w0.dtype == f32 and s.dtype == f32 and t.dtype == f32
    for k, px in enumerate(scene["textures"]):
        sel = tex & (tid == k)
        if sel.any():
            alb[sel, 0:3] = tex2d(px, s[sel], t[sel])[:, 0:3]
    st[tex, 0], st[tex, 1] = s[tex], t[tex]
    res = {}
    if "albedo" in planes:
        res["albedo"] = np.full((h, w, 4), fill, np.uint32)
        res["albedo"][Y, X] = alb.view(np.uint32)
    if "texcoord" in planes:
        res["texcoord"] = np.full((h, w, 2), fill, np.uint32)
        res["texcoord"][Y, X] = st.view(np.uint32)
    res["hits"], res["stale"], res["textured"] = int(is_hit.sum()), int(stale.sum()), int(tex.sum())
    res["kind"] = np.zeros((h, w), np.int8)
    res["kind"][Y, X] = np.where(tex, 4, np.where(is_hit, 1, np.where(miss, 2, 3)))
    res["st"] = np.zeros((h, w, 2), f32)
    res["st"][Y, X] = st
    res["mesh"] = np.full((h, w), -1, np.int64)
    res["mesh"][Y, X] = mesh
    return res
