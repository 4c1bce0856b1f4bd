"""The scene of tests/test_gpu_depth_limit.py and the conditions it has to meet, on the CPU checker alone.

pt_set_options takes max_depth in [0, 250], but from the test cameras the paths of the Cornell box and of the terrain all end by depth ~12:
a render at depth 30 and one at depth 250 trace the same rays there, so nothing a test of those scenes compares can tell the two limits
apart.  The "skylight box" keeps paths alive: a closed white room (albedo 1, Lambert) lit through a small square hole in its lid, the
camera inside.  A path ends only when it leaves through the hole, so a share of them is still bouncing at depth 250.

Above depth ~100 the IMAGE no longer changes (the throughput, a product of 2 cos(theta) terms, underflows), so what tells the deep limits
apart is the number of rays traced.  This module pins what the GPU module relies on:
  - radiance_rays of the checker strictly increases from each tested depth to the next, 249 -> 250 included: paths reach the last slot;
  - at least 200 paths are traced at depth 249;
  - the frames at depths 0, 1, 2, 30, 31 and 32 are pairwise different;
  - everything is finite.
The figures are printed (pytest -s).  Measured with the 'det' checker, 48 x 32: narrow hole (s = 0.15, 8 spp, 12288 paths) 10618 paths
traced at depth 30, 10561 at 31, 3261 at 249, 3241 at 250, radiance_rays 12288 / 24576 / 36827 / 345370 / 355988 / 366549 / 377057 /
684420 / 1719812 / 1723053 at max_depth 0 / 1 / 2 / 29 / 30 / 31 / 32 / 64 / 249 / 250; wide hole (s = 0.4, 4 spp) between 73 and 1373
pixels differ between any two of the limits 0, 1, 2, 30, 31, 32 (30 against 31: 73, 31 against 32: 84)."""
import numpy as np

from depth_limit_scene import DEEP_DEPTHS, DISTINCT_DEPTHS, EDGE_DEPTHS, MIN_ALIVE_249, SPP_DEEP, SPP_EDGE, S_DEEP, S_EDGE, H, W, checker_frame, skylight_box


def _finite(o):
    return all(np.isfinite(o[k]).all() for k in ("accum", "color", "normal", "albedo"))


def test_the_lid_closes_the_box():
    m = skylight_box(S_DEEP)
    assert m.num_triangles == 10 + 8
    v = m.meshes[0].vertex[m.meshes[0].index.reshape(-1)]
    assert not (v[:, 1].reshape(-1, 3) == 1.0).all(axis=1).any()  # no triangle of the box lies in the plane of the lid
    lid = m.meshes[1].vertex[m.meshes[1].index].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(lid[:, 1] - lid[:, 0], lid[:, 2] - lid[:, 0]), axis=1).sum()
    assert abs(area - (4.0 - (2 * S_DEEP) ** 2)) < 1e-6  # the lid is the square minus the hole, nothing twice
    assert skylight_box(S_DEEP, catcher=True).num_triangles == 30


def test_paths_reach_the_last_slot(orc_det):
    """the narrow hole, at the size of the deep GPU cases"""
    npaths = W * H * SPP_DEEP
    depths = sorted(set(EDGE_DEPTHS + DEEP_DEPTHS))
    rays = {d: checker_frame(orc_det, S_DEEP, SPP_DEEP, d) for d in depths + [248]}
    assert all(_finite(o) for o in rays.values())
    rr = {d: o["radiance_rays"] for d, o in rays.items()}
    print("radiance_rays by max_depth:", rr)
    assert rr[0] == npaths  # one trace per path
    for a, b in zip(depths, depths[1:]):
        assert rr[a] < rr[b], (a, b, rr[a], rr[b])
    # the rays a limit adds are the traces at that depth: rr(d) - rr(d - 1) paths are still alive there
    alive = {d: rr[d] - rr[d - 1] for d in (30, 31, 249, 250)}
    print("paths traced at depth:", alive, "of", npaths)
    assert alive[249] >= MIN_ALIVE_249 and alive[250] >= MIN_ALIVE_249, alive
    assert alive[31] >= alive[249]
    # the catcher variant of the deep chain case (2 spp): its paths reach the last slot too
    oc = [checker_frame(orc_det, S_DEEP, 2, d, catcher=True) for d in (249, 250)]
    print("with the catcher slab, radiance_rays at 249, 250:", [o["radiance_rays"] for o in oc])
    assert all(_finite(o) for o in oc) and oc[0]["radiance_rays"] + MIN_ALIVE_249 * 2 // SPP_DEEP <= oc[1]["radiance_rays"]


def test_shallow_limits_give_different_frames(orc_det):
    """the wide hole, at the size of the cases around depth 31"""
    frames = {d: checker_frame(orc_det, S_EDGE, SPP_EDGE, d) for d in EDGE_DEPTHS}
    assert all(_finite(o) for o in frames.values())
    rr = [frames[d]["radiance_rays"] for d in EDGE_DEPTHS]
    print("radiance_rays by max_depth:", dict(zip(EDGE_DEPTHS, rr)))
    assert all(a < b for a, b in zip(rr, rr[1:])), rr
    diff = {}
    for i, a in enumerate(DISTINCT_DEPTHS):
        for b in DISTINCT_DEPTHS[i + 1:]:
            x, y = frames[a]["accum"].view(np.uint32), frames[b]["accum"].view(np.uint32)
            diff[(a, b)] = int((x != y).any(axis=-1).sum())
    print("pixels that differ between two limits:", diff)
    assert all(n > 0 for n in diff.values()), diff
    # depth 0: hit pixels are black with their first-hit normal and albedo written (every camera ray hits the room or leaves through the hole)
    o = frames[0]
    hit = (o["normal"][..., :3] != 0).any(axis=-1)
    assert hit.mean() > 0.9 and (o["accum"][hit][:, :3] == 0).all() and (o["albedo"][hit][:, :3] == 1).all()
