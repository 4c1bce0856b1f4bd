"""The "skylight box" of the depth-limit tests and its frames under the CPU checker: tests/test_depth_limit_scene.py pins the conditions
the scene has to meet (its docstring says why this scene), tests/test_gpu_depth_limit.py renders it on the GPU."""
import numpy as np

import conftest  # noqa: F401  (puts the repository's root on sys.path)
from optixpathtracer_amd import scenes


W, H = 48, 32
CAMERA = dict(eye=(0.0, -0.2, -0.6), lookat=(0.2, -0.3, 1.0), up=(0.0, 1.0, 0.0), fovY=70.0)
LAMBERT = 1
# two sizes of the hole: a narrow one under which paths live longest (the deep cases), a wide one that lets enough light in for a thirtieth
# bounce to change pixels (the cases around the asynchronous-shadow boundary)
S_DEEP, SPP_DEEP = 0.15, 8
S_EDGE, SPP_EDGE = 0.4, 4
EDGE_DEPTHS = (0, 1, 2, 29, 30, 31, 32)
DEEP_DEPTHS = (64, 249, 250)
DISTINCT_DEPTHS = (0, 1, 2, 30, 31, 32)
MIN_ALIVE_249 = 200


def skylight_box(s, catcher=False):
    """A box of half extent 1 about the origin without its two top triangles, and a lid at y = 1 of four quads around a square hole of
    half width s.  catcher: a thin shadow-catcher slab floating inside."""
    m = scenes.Model()
    white = scenes.Material(color=(1.0, 1.0, 1.0))
    scenes.add_box(m, white, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    box = m.meshes[-1]
    box.index = np.ascontiguousarray(np.delete(box.index, (8, 9), axis=0))  # rows 8, 9: the top face (add_box's order)
    lid = [
        [(-1, 1, s), (1, 1, s), (1, 1, 1), (-1, 1, 1)],
        [(-1, 1, -1), (1, 1, -1), (1, 1, -s), (-1, 1, -s)],
        [(-1, 1, -s), (-s, 1, -s), (-s, 1, s), (-1, 1, s)],
        [(s, 1, -s), (1, 1, -s), (1, 1, s), (s, 1, s)],
    ]
    m.meshes.append(scenes._quads_to_mesh(lid, white))
    if catcher:
        cm = scenes.Material()
        cm["flags"] |= scenes.MATERIAL_FLAG_SHADOW_CATCHER
        scenes.add_box(m, cm, (0.0, -0.6, 0.3), (0.5, 0.02, 0.5))
    return m


def sky():
    return scenes.sky_probe(256, 128).BuildCDF()


_FRAMES = {}


def checker_frame(O, s, spp, max_depth, subframes=1, bsdf_mode=LAMBERT, catcher=False):
    """The checker's frame (brute-force ray search) after `subframes` progressive subframes; the ray counts are the LAST subframe's.
    Computed once per configuration (each subframe on top of the cached one before it), shared by every test and read-only."""
    key = (s, spp, max_depth, subframes, bsdf_mode, catcher)
    if key not in _FRAMES:
        prev = checker_frame(O, s, spp, max_depth, subframes - 1, bsdf_mode, catcher)["accum"] if subframes > 1 else None
        sc = O.make_scene(skylight_box(s, catcher), False)
        pr = O.make_probe(sky())
        U, V, Wv = scenes.uvw_frame(**CAMERA, aspect=W / H)
        out = O.render(sc, pr, (U, V, Wv), CAMERA["eye"], W, H, spp, max_depth, subframes - 1, bsdf_mode, prev)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FRAMES[key] = out
    return _FRAMES[key]
