"""Ray queries from and to GPU memory (pt_trace_device, pt_query_wait): t and prim are pt_trace's and the CPU checker's bit for bit, the hit
attributes are float32 NumPy's evaluation of the header's expressions, invalid rays are found on the device and never traversed, refused
calls leave nothing behind, asynchronous queries queue up in stream order, and the queries see what the rest of the loop — device-fed mesh
updates, frames in flight, a partition — has done."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import assert_bits_equal
from gpu_kit import _dev_all
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from parity_kit import _compare, _gpu_render, _random_rays, _renderer
from scene_kit import M1, _np_transform, _wave, _with_vertices

pytestmark = pytest.mark.gpu

HIT = _lib.HIT_DTYPE
NEUTRAL = np.array([0, 0, 0, 1, 0, 0, 1, -1], np.float32)  # what an invalid ray is staged as — and, from a caller, a valid ray that misses


# ------------------------------------------------------------------ helpers
def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to("cuda:0")  # (a copy: the shared references are read-only arrays)


def _offset_like(t):
    """A tensor of t's shape and dtype one element into a larger allocation: 4-byte aligned, not 16."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device="cuda:0")
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _records(out):
    return out.cpu().numpy().reshape(-1, 8).view(HIT).reshape(-1)


def _closest(r, rays, offset=False):
    """The facade's synchronous closest-hit query over host rays: (n,) records of HIT."""
    d = _dev(rays)
    out = None
    if offset:
        src, d = d, _offset_like(d)
        d.copy_(src)
        out = _offset_like(torch.empty((len(rays), 8), dtype=torch.float32, device="cuda:0"))
    res = r.traceDevice(d, out=out)
    for k in ("t", "u", "v", "prim", "mesh", "ng"):  # the typed views are the record's columns
        assert np.array_equal(res[k].cpu().numpy().view(np.uint32), _records(res["record"])[k].view(np.uint32))
    return _records(res["record"])


def _any(r, rays, offset=False):
    d = _dev(rays)
    out = None
    if offset:
        src, d = d, _offset_like(d)
        d.copy_(src)
        out = _offset_like(torch.empty(len(rays), dtype=torch.int32, device="cuda:0"))
    return r.traceDevice(d, any_hit=True, out=out).cpu().numpy()


def _same_records(a, b, what=""):
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a.view(np.uint32).reshape(-1, 8) != b.view(np.uint32).reshape(-1, 8)).any(1).sum())} of {len(a)} records differ"


def _aimed(model, rng, eye, spread):
    """test_gpu_parity's adversarial targets: rays aimed exactly at vertices, edge midpoints and centroids (shared edges, ties)."""
    v, idx, _, _ = model.flatten()
    tri = v[idx]
    targets = np.concatenate([tri.reshape(-1, 3), 0.5 * (tri[:, 0] + tri[:, 1]), 0.5 * (tri[:, 1] + tri[:, 2]), tri.mean(1)]).astype(np.float32)
    o = np.asarray(eye, np.float32) + rng.uniform(-spread, spread, (len(targets), 3)).astype(np.float32)
    d = targets - o
    return np.concatenate([o, np.full((len(o), 1), 1e-3, np.float32), d, np.full((len(o), 1), 1e16, np.float32)], 1).astype(np.float32)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]  # (x + y) + z, as dot3


def _np_attributes(model, rays, prim):
    """The header's expressions in float32, one rounding per operation, from the model's own vertices of `prim`: u, v, ng, mesh."""
    v, idx, tri_mesh, _ = model.flatten()
    tri = v[idx[prim]].astype(np.float32)
    v0, v1, v2 = tri[:, 0], tri[:, 1], tri[:, 2]
    o, d = rays[:, 0:3], rays[:, 4:7]
    A, B, Cc = v0 - o, v1 - o, v2 - o
    Uw, Vw, Ww = _dot(d, _cross(Cc, B)), _dot(d, _cross(A, Cc)), _dot(d, _cross(B, A))
    det = (Uw + Vw) + Ww
    u, w = Vw / det, Ww / det
    n = _cross(v1 - v0, v2 - v0)
    ng = n * (np.float32(1.0) / np.sqrt(_dot(n, n)))[:, None]
    for x in (u, w, ng):
        assert x.dtype == np.float32
    return u, w, ng, tri_mesh[prim].astype(np.int32)


def _check_attributes(model, rays, rec):
    hit = rec["prim"] >= 0
    miss = rec["prim"] == -1
    assert hit.any() and miss.any() and (hit | miss).all()
    u, w, ng, mesh = _np_attributes(model, rays[hit], rec["prim"][hit])
    assert np.array_equal(rec["mesh"][hit], mesh)
    assert np.array_equal(rec["u"][hit].view(np.uint32), u.view(np.uint32)), "u differs from float32 NumPy"
    assert np.array_equal(rec["v"][hit].view(np.uint32), w.view(np.uint32)), "v differs from float32 NumPy"
    # the products and sums reproduce exactly; sqrtf, the reciprocal and the last multiply may each differ in the last place of a value <= 1
    assert np.abs(rec["ng"][hit].astype(np.float64) - ng.astype(np.float64)).max() <= 2.0**-22
    m = rec[miss]
    assert np.array_equal(m["t"].view(np.uint32), rays[miss, 7].view(np.uint32)), "a miss reports the ray's own tmax"
    assert (m["mesh"] == -1).all()
    for k in ("u", "v", "ng"):
        assert not m[k].view(np.uint32).any(), f"{k} of a miss is not zero"


# ------------------------------------------------------------------ shared scenes and references (computed once, never changed)
class _Case:
    pass


@pytest.fixture(scope="module")
def cornell(ptlib, orc_det):
    c = _Case()
    c.model = scenes.cornell_box()
    c.r = R.SampleRenderer(c.model)
    rng = np.random.default_rng(9)
    c.rays = np.concatenate([_random_rays(rng, 50000, -100, 700), _aimed(c.model, rng, (278.0, 273.0, -900.0), 50)]).astype(np.float32)
    c.rays.setflags(write=False)
    c.sc = orc_det.make_scene(c.model, use_bvh=False)  # brute force: independent of any tree
    c.t, c.prim = orc_det.trace_closest(c.sc, c.rays)
    c.rec = _closest(c.r, c.rays)
    c.rec.setflags(write=False)
    yield c
    c.r.close()


@pytest.fixture(scope="module")
def terrain(ptlib, orc_det):
    c = _Case()
    c.model = scenes.voxel_terrain(n=96, target_tris=70000)
    c.r = R.SampleRenderer(c.model)
    rng = np.random.default_rng(10)
    rays = _random_rays(rng, 60000, -110, 110)
    rays[:, 1] = rng.uniform(-30, 60, len(rays))
    c.rays = rays
    c.rays.setflags(write=False)
    c.rng = rng
    c.sc = orc_det.make_scene(c.model, use_bvh=True)
    c.t, c.prim = orc_det.trace_closest(c.sc, c.rays)
    c.rec = _closest(c.r, c.rays)
    c.rec.setflags(write=False)
    yield c
    c.r.close()


@pytest.fixture(scope="module")
def probe():
    return scenes.sky_probe(256, 128).BuildCDF()


def _both_branches(prim):
    assert (prim >= 0).mean() >= 0.2 and (prim < 0).mean() >= 0.05, "the rays must exercise hits and misses"


# ------------------------------------------------------------------ 1. parity with the checker and with pt_trace
def test_closest_and_any_equal_checker_and_pt_trace_cornell(orc_det, cornell):
    c = cornell
    _both_branches(c.prim)
    assert np.array_equal(c.rec["prim"], c.prim)
    assert np.array_equal(c.rec["t"].view(np.uint32), np.asarray(c.t, np.float32).view(np.uint32)), "closest-hit t against the checker"
    (t, prim), _ = c.r.trace(c.rays)
    assert np.array_equal(c.rec["prim"], prim) and np.array_equal(c.rec["t"].view(np.uint32), t.view(np.uint32)), "against pt_trace"
    occ = _any(c.r, c.rays)
    assert np.array_equal(occ, orc_det.trace_any(c.sc, c.rays).astype(np.int32))
    assert np.array_equal(occ, c.r.trace(c.rays, any_hit=True)[0].astype(np.int32))
    s = c.r.queryStats
    assert s["rays"] == len(c.rays) and s["hits"] == int((occ == 1).sum()) and s["invalid_rays"] == 0
    assert s["stage_ms"] > 0 and s["trace_ms"] > 0 and s["attrib_ms"] > 0


def test_closest_and_any_equal_checker_and_pt_trace_terrain(orc_det, terrain):
    c = terrain
    _both_branches(c.prim)
    assert np.array_equal(c.rec["prim"], c.prim)
    assert np.array_equal(c.rec["t"].view(np.uint32), np.asarray(c.t, np.float32).view(np.uint32))
    (t, prim), _ = c.r.trace(c.rays)
    assert np.array_equal(c.rec["prim"], prim) and np.array_equal(c.rec["t"].view(np.uint32), t.view(np.uint32))
    # secondary-like rays starting ON surfaces: re-launched from the hit points
    hit = c.rec["prim"] >= 0
    P = c.rays[hit, :3] + c.rec["t"][hit, None] * c.rays[hit, 4:7]
    r2 = _random_rays(np.random.default_rng(11), int(hit.sum()), 0, 1, tmin=1e-2)
    r2[:, :3] = P
    occ = _any(c.r, r2)
    want = orc_det.trace_any(c.sc, r2).astype(np.int32)
    assert np.array_equal(occ, want) and 0 < (want == 1).sum() < len(want)
    rec2 = _closest(c.r, r2)
    t2, p2 = orc_det.trace_closest(c.sc, r2)
    assert np.array_equal(rec2["prim"], p2)
    assert np.array_equal(rec2["t"].view(np.uint32), np.asarray(t2, np.float32).view(np.uint32))
    assert c.r.queryStats["hits"] == int((p2 >= 0).sum())
    _check_attributes(c.model, r2, rec2)


# ------------------------------------------------------------------ 2. attributes
def test_attributes_cornell(cornell):
    _check_attributes(cornell.model, cornell.rays, cornell.rec)


def test_attributes_terrain(terrain):
    _check_attributes(terrain.model, terrain.rays, terrain.rec)
    meshes = np.unique(terrain.rec["mesh"])
    assert meshes[0] == -1 and meshes[-1] < len(terrain.model.meshes) and len(meshes) >= 4  # several of the scene's meshes, and the misses' -1


@pytest.mark.parametrize("scene", ["two_box", "textured"])
def test_attributes_small_scenes(ptlib, orc_det, scene):
    model = scenes.two_box_scene() if scene == "two_box" else scenes.textured_scene()
    rng = np.random.default_rng(21)
    rays = np.concatenate([_random_rays(rng, 20000, -5, 5), _aimed(model, rng, (3.0, 2.5, -4.5), 0.5)]).astype(np.float32)
    r = R.SampleRenderer(model)
    rec = _closest(r, rays)
    t, prim = orc_det.trace_closest(orc_det.make_scene(model, use_bvh=False), rays)
    assert np.array_equal(rec["prim"], prim) and np.array_equal(rec["t"].view(np.uint32), np.asarray(t, np.float32).view(np.uint32))
    _check_attributes(model, rays, rec)
    r.close()


# ------------------------------------------------------------------ 3. sizes and alignment
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_sizes_and_four_byte_alignment(cornell, n):
    c = cornell
    first = 50000 - n // 2  # random rays, then aimed ones
    rays = c.rays[first : first + n]
    want = c.rec[first : first + n]
    _same_records(_closest(c.r, rays), want, "16-byte aligned")
    _same_records(_closest(c.r, rays, offset=True), want, "one float into the allocation")
    occ = _any(c.r, rays)
    assert np.array_equal(occ, _any(c.r, rays, offset=True))
    assert np.array_equal(occ == 1, want["prim"] >= 0)  # tmax is 1e16 for all of them: occluded means a closest hit exists


# ------------------------------------------------------------------ 4. invalid rays
def _invalid_rays(valid):
    """One ray per way of being invalid, each a valid ray with one thing wrong."""
    out = []
    for pos in range(8):
        for val in (np.nan, np.inf, -np.inf):
            x = valid[len(out) % len(valid)].copy()
            x[pos] = val
            out.append(x)
    for d in ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (1e-25, 0.0, 1e-24),  # s = 0: exactly, and by underflow
              (1e-20, 1e-21, 0.0),  # s is subnormal and 1 / s overflows
              (1e20, 0.0, 0.0), (1.2e19, -1.2e19, 1.2e19)):  # s overflows: one square alone, and only the sum
        x = valid[len(out) % len(valid)].copy()
        x[4:7] = d
        out.append(x)
    return np.array(out, np.float32)


def test_invalid_rays_are_found_on_the_device(cornell, probe):
    c = cornell
    r = _renderer(c.model, probe, scenes.CORNELL_CAMERA, 96, 64)
    valid = np.concatenate([c.rays[:3000], NEUTRAL[None], c.rays[50000:50100]]).astype(np.float32)
    base = _closest(r, valid)
    base_any = _any(r, valid)
    k = 3000  # the caller's own neutral ray: valid, and a miss
    assert base["prim"][k] == -1 and base["t"][k] == -1.0 and base_any[k] == 0
    _same_records(base[:3000], c.rec[:3000])
    bad = _invalid_rays(valid)
    rng = np.random.default_rng(5)
    n = len(valid) + len(bad)
    others = np.setdiff1d(np.arange(1, n - 1), [n // 2])
    where = np.concatenate([[0, n // 2, n - 1], rng.choice(others, len(bad) - 3, replace=False)])  # first, middle, last, then anywhere
    is_bad = np.zeros(n, bool)
    is_bad[where] = True
    mixed = np.empty((n, 8), np.float32)
    mixed[is_bad] = bad
    mixed[~is_bad] = valid
    for offset in (False, True):
        rec = _closest(r, mixed, offset=offset)
        s = r.queryStats
        assert s["invalid_rays"] == len(bad) and s["rays"] == n and s["hits"] == int((base["prim"] >= 0).sum())
        _same_records(rec[~is_bad], base, "valid rays next to invalid ones")
        b = rec[is_bad]
        assert (b["prim"] == -2).all() and (b["mesh"] == -1).all()
        for f in ("t", "u", "v", "ng"):
            assert not b[f].view(np.uint32).any()
        occ = _any(r, mixed, offset=offset)
        assert r.queryStats["invalid_rays"] == len(bad)
        assert (occ[is_bad] == -2).all() and np.array_equal(occ[~is_bad], base_any)
    # no fault bit, no stale state: the next frame is a fresh context's
    _compare(_gpu_render(r, 2), _gpu_render(_renderer(c.model, probe, scenes.CORNELL_CAMERA, 96, 64), 2))
    r.close()


# ------------------------------------------------------------------ 5. refusals leave nothing behind
def test_refused_queries_leave_nothing_behind(cornell):
    c = cornell
    r = R.SampleRenderer(c.model)
    L, ctx = r._L, r._ctx
    rays = _dev(c.rays[:1000])
    out = torch.empty((1000, 8), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.traceDevice(rays, out=out)
    before, state = _records(out), r.queryStats["state_bytes"]
    assert state >= 1000 * 40
    host = np.zeros((1000, 8), np.float32)
    stats = _lib.QueryStats()
    stats.rays = 12345
    rp, op = rays.data_ptr(), out.data_ptr()
    both = torch.zeros(2 * 1000 * 8, dtype=torch.float32, device="cuda:0")
    big = torch.zeros((1 << 21, 8), dtype=torch.float32, device="cuda:0")  # 64 MB: room for 2 M rays, which the 32 KB output's block has not
    torch.cuda.synchronize()
    cases = {
        "host rays": (host.ctypes.data, 1000, 0, op, "not device memory"),
        "host output": (rp, 1000, 0, host.ctypes.data, "not device memory"),
        "null rays": (None, 1000, 0, op, "null"),
        "null output": (rp, 1000, 1, None, "null"),
        "odd alignment of the rays": (rp + 2, 999, 0, op, "not 4-byte aligned"),
        "odd alignment of the output": (rp, 999, 1, op + 1, "not 4-byte aligned"),
        "overlap": (both.data_ptr(), 1000, 0, both.data_ptr() + 1000 * 32 - 16, "overlap"),
        "output inside the rays": (both.data_ptr(), 1000, 1, both.data_ptr() + 64, "overlap"),
        "rays longer than their allocation": (rp, 1 << 27, 1, op, "left in its allocation"),
        "output longer than its allocation": (big.data_ptr(), 1 << 21, 0, op, "dev_out has fewer"),
        "unknown flags": (rp, 1000, 4, op, "flag"),
        "unknown flags with known ones": (rp, 1000, 8 | 2, op, "flag"),
    }
    for what, (a, n, flags, o, text) in cases.items():
        assert L.pt_trace_device(ctx, a, n, flags, o, C.byref(stats)) == -1, what
        msg = L.pt_last_error(ctx).decode()
        assert "pt_trace_device" in msg and text in msg, f"{what}: {msg!r}"
    assert stats.rays == 12345  # a refused call writes no statistics
    assert L.pt_trace_device(ctx, None, 0, 0, None, None) == 0  # no rays: nothing to check, nothing to launch
    s = r.queryWait()
    assert s["state_bytes"] == state and s["rays"] == 0
    out.zero_()
    r.traceDevice(rays, out=out)
    _same_records(_records(out), before)
    _same_records(before, c.rec[:1000])
    assert r.queryStats["state_bytes"] == state
    with pytest.raises(ValueError):
        r.traceDevice(rays.cpu())
    with pytest.raises(ValueError):
        r.traceDevice(rays.double())
    with pytest.raises(ValueError):
        r.traceDevice(rays[:, :7])
    r.close()


# ------------------------------------------------------------------ 6. asynchronous
def test_asynchronous_queries_queue_in_stream_order(terrain):
    c = terrain
    r = R.SampleRenderer(c.model)
    L, ctx = r._L, r._ctx
    r.traceDevice(_dev(c.rays[:30000]))  # the state now holds 30000 rays
    state = r.queryStats["state_bytes"]
    sizes = (5000, 777, 20000)
    firsts = (0, 30000, 40000)
    ins = [_dev(c.rays[f : f + n]) for f, n in zip(firsts, sizes)]
    outs = [torch.zeros((n, 8), dtype=torch.float32, device="cuda:0") for n in sizes]
    torch.cuda.synchronize()  # raw pointers: their producer has to be complete
    for a, o, n in zip(ins, outs, sizes):
        assert L.pt_trace_device(ctx, a.data_ptr(), n, _lib.PT_QUERY_CLOSEST | _lib.PT_QUERY_ASYNC, o.data_ptr(), None) == 0
    s = r.queryWait()
    hits = 0
    for f, n, o in zip(firsts, sizes, outs):
        _same_records(_records(o), c.rec[f : f + n], f"asynchronous query of {n}")
        hits += int((c.rec["prim"][f : f + n] >= 0).sum())
    assert s["rays"] == sum(sizes) and s["hits"] == hits and s["invalid_rays"] == 0 and s["state_bytes"] == state
    assert s["stage_ms"] > 0 and s["trace_ms"] > 0 and s["attrib_ms"] > 0
    again = r.queryWait()
    assert again["rays"] == 0 and again["trace_ms"] == 0 and again["state_bytes"] == state  # the sums start over at a wait
    # the facade: torch's current stream waits for the query on the device, so a torch kernel enqueued next reads the results
    rays = _dev(c.rays[:20000])
    res = r.traceDevice(rays, wait=False)
    copy = res["record"].clone()
    occ = r.traceDevice(rays, any_hit=True, wait=False).clone()
    _same_records(_records(copy), c.rec[:20000], "wait=False, then a torch kernel")
    assert np.array_equal(occ.cpu().numpy() == 1, c.rec["prim"][:20000] >= 0)
    s = r.queryWait()
    assert s["rays"] == 40000 and s["state_bytes"] == state
    r.close()  # with nothing pending; a context destroyed with queries queued completes them first (pt_destroy drains)


# ------------------------------------------------------------------ 7. with the rest of the loop
@pytest.mark.parametrize("rebuild", [False, True])
def test_query_after_device_fed_updates_equals_fresh_context(ptlib, terrain, rebuild):
    rays = terrain.rays[:20000]
    # a transform ...
    A = scenes.two_box_scene()
    small = np.concatenate([_random_rays(np.random.default_rng(3), 8000, -5, 5), _aimed(A, np.random.default_rng(4), (3.0, 2.5, -4.5), 0.5)]).astype(np.float32)
    r = R.SampleRenderer(A)
    before = _closest(r, small)
    r.transformMeshes({0: M1}, rebuild=rebuild)
    B = _with_vertices(A, {0: _np_transform(M1, A.meshes[0].vertex)})
    f = R.SampleRenderer(B)
    after = _closest(r, small)
    _same_records(after, _closest(f, small), "after transformMeshes")
    assert after.tobytes() != before.tobytes()
    _check_attributes(B, small, after)
    r.close()
    f.close()
    # ... and vertices a GPU step left in a tensor
    new = _wave(terrain.model, 2.0, 0.7)
    r = R.SampleRenderer(terrain.model)
    _same_records(_closest(r, rays), terrain.rec[:20000])
    r.updateMeshesDevice(_dev_all(new), rebuild=rebuild)
    moved = _with_vertices(terrain.model, new)
    f = R.SampleRenderer(moved)
    after = _closest(r, rays)
    _same_records(after, _closest(f, rays), "after updateMeshesDevice")
    assert np.array_equal(_any(r, rays), _any(f, rays))
    _check_attributes(moved, rays, after)
    r.close()
    f.close()


def test_query_drains_frames_in_flight(cornell, probe):
    c = cornell

    def frames(r, k0, k1):
        r.launchParams.samples_per_launch = 2
        for k in range(k0, k1):
            r.launchParams.frame.subframe_index = k
            r.render()

    u = _renderer(c.model, probe, scenes.CORNELL_CAMERA, 96, 64, frames_in_flight=3)
    frames(u, 0, 5)
    want = u.download(R.PT_BUF_ACCUM)
    r = _renderer(c.model, probe, scenes.CORNELL_CAMERA, 96, 64, frames_in_flight=3)
    frames(r, 0, 3)  # enqueued, two of them not waited for
    rec = _closest(r, c.rays[:5000])
    assert r.stats()["frames"] == 3
    res = r.traceDevice(_dev(c.rays[:5000]), wait=False)  # queued behind nothing the frames need: they go on while it runs
    frames(r, 3, 5)
    assert_bits_equal(r.download(R.PT_BUF_ACCUM), want, "frames around a query")
    assert np.array_equal(r.download(R.PT_BUF_FRAME), u.download(R.PT_BUF_FRAME))
    _same_records(rec, c.rec[:5000])
    _same_records(_records(res["record"]), c.rec[:5000])  # pt_download completed the queued query as well
    assert r.queryWait()["rays"] == 5000
    u.close()
    r.close()


def test_partitioned_context_answers_over_the_whole_scene(cornell, probe):
    c = cornell
    r = R.SampleRenderer(c.model)
    r.setProbe(probe)
    r.setPartition(1, 4)
    r.resize((96, 64))
    _same_records(_closest(r, c.rays[:20000]), c.rec[:20000])
    r.close()
