"""Object motion for the reprojection chain (pt_copy_vertices_device, pt_motion_planes) on the GPU.  Every plane is compared bit for bit, over
the WHOLE plane (a pixel written outside the chosen set shows as a lost sentinel), with tests/motion_ref.py: float32 NumPy evaluating the
header's arithmetic on the hit plane renderGBuffer gave (pinned by tests/test_gpu_gbuffer.py), the previous vertices and the model's own index
arrays.  No tolerance anywhere; the hand-made plane with NaN barycentrics compares NaN words as NaN (payloads are not specified).

Inputs, 131 x 61 (17 x 8 blocks, last column 3 wide, last row 5 high): the two-box scene with its unit box (mesh 0) turned by 0.2 rad about y
and shifted by (0.1, 0.15, -0.05); voxel_terrain(n=64, target_tris=20000) with its largest band (mesh 3) turned by 0.03 rad and shifted by
(1.5, 0.8, -1.0).  Previous camera: the eye 0.25 to the side (gbuffer_ref._moved)."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_ref as M
import temporal_ref as T
from gbuffer_ref import _moved, _row
from gpu_kit import filled, pixel_mask, plane_shape, whole_frame
from gpu_kit import bits as _bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from pass_cases import _vertices
from pass_cases import motion_case as _case
from scene_kit import RECTS, _cam_dicts, _np_transform

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 131, 61
SENTINEL = M.SENTINEL


# ------------------------------------------------------------------ GPU helpers
def _filled(name, h, w, offset=False):
    """a sentinel-filled plane of the pass; offset: one float into its allocation (4-byte aligned only)"""
    return filled(plane_shape(h, w, M.WORDS[name]), offset)


def _same(got, ref, what, nan_aware=False):
    for name, a in got.items():
        b = ref[name]
        neq = a != b
        if nan_aware:
            with np.errstate(all="ignore"):
                neq &= ~(np.isnan(a.view(f32)) & np.isnan(b.view(f32)))
        assert a.shape == b.shape and not neq.any(), f"{what}: {name} differs from float32 NumPy in {int(neq.sum())} words"


def _run(r, idx, hit, prev_vertices, rects, pixels, what, cams=None, prev_cams=None, planes=M.PLANES, mask=None, offset=False, nan_aware=False):
    """uploads hit (a NumPy plane) and prev_vertices, calls motionPlanes into sentinel-filled outputs, compares every output with the NumPy
    reference over the whole frame and the counters with its counts; returns (reference, {plane: bits}, stats)"""
    h, w = hit.shape[:2]
    out = {k: _filled(k, h, w, offset) for k in planes}
    res = r.motionPlanes(_upload(hit, offset), _upload(prev_vertices, offset), prev_cameras=prev_cams if "motion" in planes else None, planes=planes,
                         mask=mask, out=out)
    assert all(res[k] is out[k] for k in planes)
    ref = M.motion_ref(hit, prev_vertices, idx, rects, pixels, cams=cams, prev_cams=prev_cams, planes=planes)
    got = {k: _bits(out[k]) for k in planes}
    _same(got, ref, what, nan_aware)
    st = res["stats"]
    assert (st["pixels"], st["hits"], st["stale"]) == (int(np.asarray(pixels).sum()), ref["hits"], ref["stale"]), (what, st, ref["hits"], ref["stale"])
    assert st["kernel_ms"] > 0 if st["pixels"] else st["kernel_ms"] >= 0
    return ref, got, st


def _frame(w=W, h=H):
    return whole_frame(w, h)


# ------------------------------------------------------------------ 1. the snapshot
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_copy_vertices_device_is_the_concatenated_download(ptlib, name):
    c = _case(name)
    nv, nt = c.r.vertexCount()
    assert (nv, nt) == (len(c.verts0), len(c.idx)) and c.after_create.shape == (nv, 3)
    assert np.array_equal(c.after_create.view(np.uint32), c.verts0.view(np.uint32))  # after create: the model's vertices, mesh after mesh
    first = sum(len(m.vertex) for m in c.model.meshes[:c.mesh])
    moved = _np_transform(c.A, c.model.meshes[c.mesh].vertex)
    want = c.verts0.copy()
    want[first:first + len(moved)] = moved
    assert np.array_equal(c.after_refit.view(np.uint32), want.view(np.uint32)) and np.array_equal(c.after_refit, c.verts1)  # after a refit
    assert not np.array_equal(c.after_refit, c.after_create)
    # after a rebuild, into the caller's tensor one float into its allocation
    r = _renderer(c.model, (W, H), c.cam)
    r.transformMeshes({c.mesh: c.A}, rebuild=True)
    buf = torch.full((3 * nv + 1,), float("nan"), device="cuda:0")
    out = buf[1:].view(nv, 3)
    assert r.copyVerticesDevice(out=out) is out and out.data_ptr() % 16 == 4
    assert np.array_equal(_np(out).view(np.uint32), want.view(np.uint32)) and np.array_equal(_np(out), _vertices(r, c.model))
    assert np.isnan(_np(buf[:1])).all()
    r.close()


# ------------------------------------------------------------------ 2. the three planes after a rotation plus translation of one mesh
@pytest.mark.parametrize("name", ["two_box", "terrain"])
def test_planes_after_a_mesh_moved(ptlib, name):
    c = _case(name)
    rects, px = _frame()
    ref, got, st = _run(c.r, c.idx, c.cur["hit"], c.after_create, rects, px, f"{name}, refit", cams=[c.row], prev_cams=[c.prev_row])
    assert st["hits"] == c.gstats["hits"] and st["stale"] == 0 and 0 < st["hits"] < W * H
    print(f"{name}: pixels {st['pixels']} hits {st['hits']} kernel_ms {st['kernel_ms']:.4f}")
    # misses: renderGBuffer's own motion, bit for bit; hits on the moved mesh: another motion than the camera's
    miss, hit = ref["kind"] == 2, ref["kind"] == 1
    gb = c.cur["motion"].view(np.uint32)
    assert miss.any() and np.array_equal(got["motion"][miss], gb[miss])
    on_mesh = hit & (c.cur["hit"].view(np.int32)[..., 4] == c.mesh)
    with np.errstate(all="ignore"):
        d = np.abs(got["motion"].view(f32) - c.cur["motion"])[on_mesh].max(-1)
    assert on_mesh.sum() > 100 and (d > 0.05).mean() > 0.9, (int(on_mesh.sum()), float(np.nanmedian(d)))
    # prev_point is the moved mesh's point taken back: A applied to it gives the current position again, up to rounding
    back = _np_transform(c.A, got["prev_point"].view(f32)[on_mesh][:, :3])
    scale = float(np.abs(c.cur["position"][on_mesh][:, :3]).max())
    assert np.abs(back - c.cur["position"][on_mesh][:, :3]).max() < 1e-4 * scale
    # a rebuild instead of the refit: the primitive indices survive it, and so do all three planes
    r = _renderer(c.model, (W, H), c.cam)
    snap = r.copyVerticesDevice()
    r.transformMeshes({c.mesh: c.A}, rebuild=True)
    g = r.renderGBuffer(("hit",))
    assert np.array_equal(_bits(g["hit"]), c.cur["hit"].view(np.uint32))
    res = r.motionPlanes(g["hit"], snap, prev_cameras=c.prev_row)
    _same({k: _bits(res[k]) for k in M.PLANES}, ref, f"{name}, rebuild")
    assert res["stats"]["hits"] == st["hits"]
    r.close()


def test_each_plane_alone(ptlib):
    c = _case("two_box")
    rects, px = _frame()
    for plane in M.PLANES:
        _run(c.r, c.idx, c.cur["hit"], c.after_create, rects, px, f"{plane} alone", cams=[c.row], prev_cams=[c.prev_row], planes=(plane,))
    _run(c.r, c.idx, c.cur["hit"], c.after_create, rects, px, "the two without cameras", planes=("prev_point", "prev_surface"))


# ------------------------------------------------------------------ 3. views, masks, partition
def test_two_views_with_different_previous_cameras(ptlib):
    c = _case("two_box")
    r = _renderer(c.model, (W, H), c.cam)
    rects = RECTS[:2]
    cams = [R.make_camera(cd, w / h) for (x, y, w, h), cd in zip(rects, _cam_dicts())]
    rows = R._camera_rows(cams)
    prev = np.stack([_row(_moved(cd, 0.1 * (k + 1)), w / h) for k, ((x, y, w, h), cd) in enumerate(zip(rects, _cam_dicts()))])
    assert not np.array_equal(prev[0], prev[1])
    r.setViews([(x, y, w, h, cam) for (x, y, w, h), cam in zip(rects, cams)])
    snap = _np(r.copyVerticesDevice())
    r.transformMeshes({c.mesh: c.A})
    g = r.renderGBuffer(("hit", "motion"), prev_cameras=prev)
    inside = np.zeros((H, W), bool)
    for x, y, w, h in rects:
        inside[y:y + h, x:x + w] = True
    hit = _np(g["hit"])
    ref, got, st = _run(r, c.idx, hit, snap, rects, inside, "two views", cams=rows, prev_cams=prev)
    assert st["pixels"] == sum(w * h for _, _, w, h in rects) and 0 < st["hits"] < st["pixels"]
    miss = ref["kind"] == 2
    assert miss.any() and np.array_equal(got["motion"][miss], _bits(g["motion"])[miss])
    for name in M.PLANES:  # (the whole-plane comparison already said so)
        assert (got[name][~inside] == SENTINEL).all()
    # each view used its own previous camera: with the two rows swapped the motion plane changes in both views
    swapped = M.motion_ref(hit, snap, c.idx, rects, inside, cams=rows, prev_cams=prev[::-1])
    for x, y, w, h in rects:
        assert (swapped["motion"][y:y + h, x:x + w] != got["motion"][y:y + h, x:x + w]).any()
    # back to the single camera: the whole frame, one rectangle
    r.setViews([])
    r.setCamera(R.make_camera(c.cam, W / H))
    _run(r, c.idx, c.cur["hit"], snap, *_frame(), "views dropped", cams=[c.row], prev_cams=[c.prev_row])
    r.close()


def test_block_mask(ptlib):
    c = _case("terrain")
    nby, nbx = c.r.blockGrid()
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.4
    mask[0, 0] = mask[nby - 1, nbx - 1] = mask[0, nbx - 1] = mask[nby - 1, 3] = True  # corner and edge blocks, the 3-wide column and the 5-high row
    mask[1, 1] = False
    px = pixel_mask(mask, h=H, w=W)
    ref, got, st = _run(c.r, c.idx, c.cur["hit"], c.after_create, [(0, 0, W, H)], px, "a random block mask", cams=[c.row], prev_cams=[c.prev_row], mask=mask)
    assert 0 < st["pixels"] < W * H
    for name in M.PLANES:
        assert (got[name][~px] == SENTINEL).all()
    assert not (got["prev_surface"][px][:, 0] == SENTINEL).any()
    _, _, st = _run(c.r, c.idx, c.cur["hit"], c.after_create, [(0, 0, W, H)], np.zeros((H, W), bool), "the empty mask", cams=[c.row], prev_cams=[c.prev_row],
                    mask=np.zeros((nby, nbx), bool))
    assert st == dict(pixels=0, hits=0, stale=0, kernel_ms=st["kernel_ms"])


def test_partition_of_two_ranks(ptlib):
    c = _case("two_box")
    by, bx = np.mgrid[0:H, 0:W] // 8
    written = np.zeros((H, W), int)
    hits = 0
    for rank in range(2):
        r = _renderer(c.model, (W, H), c.cam, partition=(rank, 2, 8, 8))
        own = (bx + by) % 2 == rank
        _, got, st = _run(r, c.idx, c.cur["hit"], c.after_create, [(0, 0, W, H)], own, f"rank {rank}", cams=[c.row], prev_cams=[c.prev_row])
        assert st["pixels"] == int(own.sum())
        hits += st["hits"]
        written += got["prev_point"][..., 3] != SENTINEL
        r.close()
    assert (written == 1).all() and hits == c.gstats["hits"]  # the union is the frame, overlaps are empty


# ------------------------------------------------------------------ 4. alignment, small frames, hand-made planes
def test_planes_and_vertices_four_byte_aligned_only(ptlib):
    c = _case("terrain")
    _run(c.r, c.idx, c.cur["hit"], c.after_create, *_frame(), "everything one float into its allocation", cams=[c.row], prev_cams=[c.prev_row], offset=True)


@pytest.mark.parametrize("size", [(1, 1), (9, 9)])
def test_small_frames(ptlib, size):
    c = _case("two_box")
    w, h = size
    cam = dict(c.cam, fovY=12.0) if size == (1, 1) else c.cam  # the one pixel looks at the box
    r = _renderer(c.model, size, cam)
    snap = _np(r.copyVerticesDevice())
    r.transformMeshes({c.mesh: c.A})
    g = r.renderGBuffer(("hit", "motion"), prev_cameras=_row(_moved(cam), w / h))
    ref, got, st = _run(r, c.idx, _np(g["hit"]), snap, *_frame(w, h), f"{w} x {h}", cams=[_row(cam, w / h)], prev_cams=[_row(_moved(cam), w / h)])
    assert st["pixels"] == w * h and st["hits"] == g["stats"]["hits"] > 0
    miss = ref["kind"] == 2
    assert np.array_equal(got["motion"][miss], _bits(g["motion"])[miss])
    r.close()


def test_hand_made_hit_planes(ptlib):
    c = _case("two_box")
    w, h = 9, 9
    r = _renderer(c.model, (w, h), c.cam)
    ntri = r.vertexCount()[1]
    assert ntri == len(c.idx) == 24
    rng = np.random.default_rng(17)
    hit = np.zeros((h, w, 8), f32)
    words = hit.view(np.int32)
    hit[..., 0] = rng.random((h, w), dtype=f32) * 5 + 1
    hit[..., 1], hit[..., 2] = rng.random((h, w), dtype=f32) * f32(0.5), rng.random((h, w), dtype=f32) * f32(0.5)
    prim = rng.integers(-2, ntri + 3, (h, w)).astype(np.int32)
    prim[0, :6] = (ntri - 1, ntri, 2**31 - 1, -(2**31), 2**30, 0)  # the last triangle, the first index past it, the extremes
    words[..., 3] = prim
    words[..., 4] = np.where(prim < 0, -1, 1)
    hit[..., 5:8] = rng.random((h, w, 3), dtype=f32)
    hit[4, 4, 1] = hit[5, 5, 2] = np.nan
    prim[4, 4] = prim[5, 5] = words[4, 4, 3] = words[5, 5, 3] = 3  # NaN barycentrics on a triangle in range: a hit, NaN words, no fault
    stale = int((prim >= ntri).sum())
    assert stale >= 4 and (prim < 0).sum() >= 1
    row, prev_row = _row(c.cam, w / h), _row(_moved(c.cam), w / h)
    ref, got, st = _run(r, c.idx, hit, c.verts0, *_frame(w, h), "hand-made", cams=[row], prev_cams=[prev_row], nan_aware=True)
    assert st["stale"] == stale and st["hits"] == int(((prim >= 0) & (prim < ntri)).sum())
    assert (got["motion"][prim >= ntri] == M.QNAN).all() and (got["motion"][4, 4] == M.QNAN).all()
    assert np.isnan(got["prev_point"].view(f32)[4, 4, :3]).all() and got["prev_point"][4, 4, 3] == f32(1).view(np.uint32)
    want = np.zeros(8, np.uint32)
    want[0], want[3], want[4] = hit[0, 1, 0].view(np.uint32), 0xFFFFFFFF, 0xFFFFFFFF
    assert np.array_equal(got["prev_surface"][0, 1], want)
    r.close()


# ------------------------------------------------------------------ 5. the chain
def test_chain_keeps_the_history_of_the_moving_mesh(ptlib, orc_det):
    c = _case("two_box")
    rects, px = _frame()
    res = c.r.motionPlanes(_upload(c.cur["hit"]), c.snapshot, prev_cameras=c.prev_row)
    ref = M.motion_ref(c.cur["hit"], c.after_create, c.idx, rects, px, cams=[c.row], prev_cams=[c.prev_row])
    base = T.with_random_history(dict(motion=c.cur["motion"], hit=c.cur["hit"], position=c.cur["position"], prev_hit=c.old["hit"], prev_position=c.old["position"]), 23)
    prm = dict(plane_eps=0.01)

    def temporal(motion, hit, position):
        out = c.r.temporalAccumulate(_upload(base["color"]), motion, hit, position, _upload(base["prev_hit"]), _upload(base["prev_position"]),
                                     _upload(base["history_in"]), _upload(base["length_in"]), **prm)
        return out, _np(out["length_out"]) >= 2  # a valid pixel leaves len = n + 1 >= 2, every other pixel 1

    # fed the new planes: what temporal_ref gives when fed the reference's
    out, valid = temporal(res["motion"], res["prev_surface"], res["prev_point"])
    want = T.temporal_ref(orc_det, dict(base, motion=ref["motion"].view(f32), hit=ref["prev_surface"].view(f32), position=ref["prev_point"].view(f32)), rects, px,
                          fill=0, **prm)
    for k in ("history_out", "length_out"):
        assert np.array_equal(_bits(out[k]), want[k]), f"{k} differs from temporal_ref fed the reference's planes"
    assert out["stats"]["reprojected"] == want["reprojected"] and np.array_equal(valid, want["valid"])
    # the camera-only route on the same history
    out0, valid0 = temporal(_upload(c.cur["motion"]), _upload(c.cur["hit"]), _upload(c.cur["position"]))
    moving = c.cur["hit"].view(np.int32)[..., 4] == c.mesh
    still = ~moving
    a, b = int(valid[moving].sum()), int(valid0[moving].sum())
    print(f"chain: reprojected on the moving mesh {a} of {int(moving.sum())} with the new planes, {b} camera-only; elsewhere {int(valid[still].sum())} / {int(valid0[still].sum())}")
    assert a > b
    # where nothing moved the two routes see the same surface tests up to the rounding of Q: the counts stay close
    assert abs(int(valid[still].sum()) - int(valid0[still].sum())) * 20 <= int(still.sum())


# ------------------------------------------------------------------ 6. the rendering state is left alone
@pytest.mark.parametrize("frames_in_flight", [0, 3])
def test_rendering_state_is_left_alone(ptlib, frames_in_flight):
    c = _case("two_box")
    probe = scenes.sky_probe(256, 128).BuildCDF()
    rects, px = _frame()

    def run(with_call):
        r = R.SampleRenderer(scenes.two_box_scene(shadow_catcher=False))
        r.setProbe(probe)
        r.setOptions(frames_in_flight=frames_in_flight)
        r.resize((W, H))
        r.setCamera(R.make_camera(scenes.TWO_BOX_CAMERA, W / H))
        r.launchParams.samples_per_launch = 2
        for k in (0, 1):
            r.launchParams.frame.subframe_index = k
            r.render()
        if with_call:
            if frames_in_flight == 0:
                before = r.stats()
            snap = r.copyVerticesDevice()
            assert np.array_equal(_np(snap), c.verts0)
            _run(r, c.idx, c.cur["hit"], c.after_create, rects, px, "between the frames", cams=[c.row], prev_cams=[c.prev_row])
            if frames_in_flight == 0:  # (with frames in flight the calls complete them, and stats() would have, too)
                assert r.stats() == before
        allocs = r.stats()["path_state_allocs"]
        r.launchParams.frame.subframe_index = 2
        r.render()
        r.sync()
        bufs = [r.download(k) for k in range(5)]
        assert r.stats()["path_state_allocs"] == allocs
        r.close()
        return bufs, allocs

    (a, allocs_a), (b, allocs_b) = run(True), run(False)
    assert allocs_a == allocs_b
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), f"buffer {k} differs after copyVerticesDevice and motionPlanes between the frames"


# ------------------------------------------------------------------ 7. refusals
def test_refusals(ptlib):
    c = _case("two_box")
    L = _lib.load_library()
    r = R.SampleRenderer(c.model)
    nv = len(c.verts0)
    dev = dict(hit=_upload(c.cur["hit"]), prev_vertices=_upload(c.after_create))
    out = {k: _filled(k, H, W) for k in M.PLANES}
    ptr = {k: t.data_ptr() for k, t in list(dev.items()) + list(out.items())}
    cams = np.ascontiguousarray(c.prev_row, f32).reshape(1, 12)
    good = dict(ptr, prev_cameras=cams.ctypes.data, num_prev_cameras=1, flags=0)

    def refused(what, pattern, **fields):
        d = _lib.MotionDesc()
        for k, v in dict(good, **fields).items():
            setattr(d, k, v)
        torch.cuda.synchronize()
        s = _lib.MotionStats(7, 7, 7, 7.0)
        rc = L.pt_motion_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_motion_planes") and pattern in msg, f"{what}: {msg!r}"
        assert (s.pixels, s.hits, s.stale, s.kernel_ms) == (7, 7, 7, 7.0)
        for k, t in out.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {k} was written"

    refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(c.cam, W / H))
    assert L.pt_motion_planes(r._ctx, None, None) == -1 and "null description" in L.pt_last_error(r._ctx).decode()
    refused("hit null", "hit is null", hit=None)
    refused("prev_vertices null", "prev_vertices is null", prev_vertices=None)
    refused("no output", "no plane asked for", motion=None, prev_point=None, prev_surface=None)
    host = np.zeros((H, W, 8), f32)
    refused("a host pointer", "hit is not device memory", hit=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "prev_point is not 4-byte aligned", prev_point=ptr["prev_point"] + 2)
    refused("the vertices offset by 1 byte", "prev_vertices is not 4-byte aligned", prev_vertices=ptr["prev_vertices"] + 1)
    # one element too small for what is left of its allocation (an allocation of the runtime's own: torch's allocator hands out parts of larger ones)
    hip = _hip_runtime()
    for name, nbytes in (("prev_vertices", nv * 12), ("motion", H * W * 8)):
        raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert hip.hipMalloc(C.byref(raw), C.c_size_t(nbytes)) == 0
        try:
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= nbytes
            refused(f"{name} one element too small", f"{name} has fewer than {nbytes} bytes left", **{name: raw.value + size.value - (nbytes - 4)})
        finally:
            assert hip.hipFree(raw) == 0
    # an output may overlap no other plane, nor the vertices; hit and prev_vertices are only read
    refused("the surface on the hit plane", "hit and prev_surface overlap", prev_surface=ptr["hit"])
    refused("the motion inside the hit plane", "hit and motion overlap", motion=ptr["hit"] + 4 * (H * W * 6))
    refused("the point on the vertices", "prev_vertices and prev_point overlap", prev_vertices=ptr["prev_point"] + 16)
    refused("two outputs", "motion and prev_point overlap", motion=ptr["prev_point"] + 4 * (H * W * 2))
    refused("motion without cameras", "motion needs prev_cameras", prev_cameras=None)
    refused("two cameras without views", "num_prev_cameras is 2, expected 1 (no views are set)", num_prev_cameras=2)
    refused("no camera", "num_prev_cameras is 0, expected 1", num_prev_cameras=0)
    for bad in (np.nan, np.inf):
        rows = cams.copy()
        rows[0, 7] = bad
        refused(f"a camera value {bad}", "prev_cameras: value 7 is not finite", prev_cameras=rows.ctypes.data)
    refused("a flag", "unknown flag bits 1", flags=1)
    r.setViews([(x, y, w, h, R.make_camera(cd, w / h)) for (x, y, w, h), cd in zip(RECTS[:2], _cam_dicts())])
    refused("one camera for two views", "num_prev_cameras is 1, expected 2 (the view count)")
    r.setViews([])
    r.setCamera(R.make_camera(c.cam, W / H))
    # pt_copy_vertices_device
    dst = torch.full((nv + 1, 3), float("nan"), device="cuda:0")

    def copy_refused(what, pattern, p, nbytes):
        torch.cuda.synchronize()
        rc = L.pt_copy_vertices_device(r._ctx, p, nbytes)
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1 and msg.startswith("pt_copy_vertices_device") and pattern in msg, f"{what}: {rc} {msg!r}"
        assert np.isnan(_np(dst)).all(), f"{what}: the destination was written"

    copy_refused("too few bytes", f"bytes must equal vertices * 12 = {nv * 12}", dst.data_ptr(), nv * 12 - 12)
    copy_refused("too many bytes", "bytes must equal vertices * 12", dst.data_ptr(), nv * 12 + 12)
    copy_refused("a null pointer", "dev_dst is null", None, nv * 12)
    copy_refused("a host pointer", "dev_dst is not device memory", host.ctypes.data, nv * 12)
    copy_refused("a pointer offset by 2 bytes", "dev_dst is not 4-byte aligned", dst.data_ptr() + 2, nv * 12)
    # the Python facade checks dtype, shape and device before the library is called, and passes the library's refusals on
    with pytest.raises(ValueError, match="prev_point.*shape"):
        r.motionPlanes(dev["hit"], dev["prev_vertices"], planes=("prev_point",), out=dict(prev_point=out["motion"]))
    with pytest.raises(ValueError, match="the tensor is on cpu"):
        r.motionPlanes(torch.zeros((H, W, 8)), dev["prev_vertices"], planes=("prev_point",))
    with pytest.raises(RuntimeError, match="hit and prev_surface overlap"):
        r.motionPlanes(dev["hit"], dev["prev_vertices"], planes=("prev_surface",), out=dict(prev_surface=dev["hit"]))
    assert np.array_equal(_bits(dev["hit"]), c.cur["hit"].view(np.uint32))
    # a valid call afterwards still works, into the same planes
    rects, px = _frame()
    res = r.motionPlanes(dev["hit"], dev["prev_vertices"], prev_cameras=c.prev_row, out=out)
    ref = M.motion_ref(c.cur["hit"], c.after_create, c.idx, rects, px, cams=[c.row], prev_cams=[c.prev_row])
    _same({k: _bits(out[k]) for k in M.PLANES}, ref, "a valid call after the refusals")
    assert res["stats"]["hits"] == ref["hits"]
    # ... and so does one that lets the facade allocate its outputs (zero-filled)
    res = r.motionPlanes(dev["hit"], dev["prev_vertices"], planes=("prev_point",))
    assert np.array_equal(_bits(res["prev_point"]), ref["prev_point"]) and set(res) == {"prev_point", "stats"}
    r.close()
