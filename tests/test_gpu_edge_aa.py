"""Geometric edge antialiasing (pt_edge_aa_planes) on the GPU.  Every output is compared bit for bit, over the WHOLE plane (a pixel written
outside the chosen set shows as a lost sentinel), with tests/edge_aa_ref.py: float32 NumPy evaluating the header's rule on the planes
renderGBuffer gave (or hand-made ones), the current vertices and the cameras.  All five counters are compared exactly.  NaN words compare as
NaN (payloads are not specified).  Frames are 131 x 59 and smaller.

One check carries a meaning beyond the reference, with its bound (edge_aa_ref.R_EDGE) measured by tests/test_edge_aa_cabi.py from the references alone: the
output is closer than the input to the 8 x 8 supersampled albedo (R_EDGE)."""
import ctypes as C

import numpy as np
import pytest
import torch

import edge_aa_ref as E
import motion_ref as M
import surface_ref as S
from edge_aa_ref import INPUTS, R_EDGE, SUPER, H, W, supersampled_truth
from gpu_kit import filled, pixel_mask, plane_shape, whole_frame_mask
from gpu_kit import bits3 as _bits
from gpu_kit import hip_runtime as _hip_runtime
from gpu_kit import plane_renderer as _renderer
from gpu_kit import same_words as _same
from gpu_kit import to_numpy as _np
from gpu_kit import upload as _upload
from gpu_kit import words_differ as _differ
from optixpathtracer_amd import _lib, scenes
from optixpathtracer_amd import renderer as R
from scene_kit import RECTS, _affine

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = E.SENTINEL
COUNTERS = ("pixels", "hits", "stale", "boundary", "blended")
NAN, INF = f32(np.nan), f32(np.inf)


def _filled(name, h, w, offset=False):
    """a sentinel-filled plane of the pass; offset: one float into its allocation (4-byte aligned only)"""
    return filled(plane_shape(h, w, E.WORDS[name]), offset, torch.int32 if name == "frame_rgba8" else torch.float32)


class _Case:
    pass


_CASES = {}


def _case(name):
    """the model, its vertices, a renderer under the input's camera at W x H, its hit and position planes and its pixel-centre albedo as the
    colour.  Built once; the arrays are read-only."""
    if name not in _CASES:
        make, cam = INPUTS[name]
        c = _Case()
        c.model, c.cam = make(), cam
        c.verts, c.idx = M.model_arrays(c.model)
        c.r = _renderer(c.model, (W, H), cam)
        c.row = R._camera_rows([R.make_camera(cam, W / H)])[0]
        g = c.r.renderGBuffer(("hit", "position"))
        c.gstats, c.hit, c.position = g["stats"], _np(g["hit"]), _np(g["position"])
        c.table = c.r.copyTexcoordsDevice()
        c.color = _np(c.r.surfacePlanes(g["hit"], c.table, planes=("albedo",))["albedo"])
        for a in (c.hit, c.position, c.color):
            a.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


def _run(r, orc, c, pixels, what, hit=None, position=None, color=None, verts=None, rects=None, cams=None, mask=None, offset=False, planes=E.PLANES, **prm):
    """uploads the planes, calls edgeAaPlanes into sentinel-filled outputs, compares every output with the NumPy reference over the whole
    frame and the five counters with its counts; returns (reference, {plane: bits}, stats)"""
    hit = c.hit if hit is None else hit
    position = c.position if position is None else position
    color = c.color if color is None else color
    h, w = hit.shape[:2]
    out = {n: _filled(n, h, w, offset) for n in planes}
    res = r.edgeAaPlanes(_upload(color, offset), _upload(hit, offset), _upload(position, offset), out=out["out"], edge=out.get("edge"), frame=out.get("frame_rgba8"),
                         mask=mask, **prm)
    assert all(res[n] is out[n] for n in planes)
    ref = E.edge_aa_ref(hit, position, color, c.verts if verts is None else verts, c.idx, rects or [(0, 0, w, h)], [c.row] if cams is None else cams, pixels,
                        planes=planes, orc=orc, **prm)
    got = {n: _bits(out[n]) for n in planes}
    _same(got, ref, what)
    st = res["stats"]
    want = tuple(ref[k] for k in COUNTERS)
    assert tuple(st[k] for k in COUNTERS) == want and want[0] == int(np.asarray(pixels).sum()), (what, st, want)
    return ref, got, st


def _check_edge_plane(got, pixels, what):
    """weights in (0, 0.5] with codes 1..4, or (0, 0); a blended pixel's neighbour lies in the set; out.w is 1"""
    e = got["edge"].view(f32)
    wgt, code = e[..., 0][pixels], e[..., 1][pixels]
    assert set(np.unique(code).tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0}, what
    assert ((wgt == 0) == (code == 0)).all() and (wgt[code > 0] > 0).all() and (wgt <= 0.5).all(), what
    assert (got["out"][..., 3][pixels] == S.ONE).all(), what
    h, w = pixels.shape
    padded = np.zeros((h + 2, w + 2), bool)
    padded[1:-1, 1:-1] = pixels
    full = e[..., 1]
    for k, (dx, dy) in enumerate(E.DIRS):
        neighbour_in_set = padded[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
        assert not (pixels & (full == k + 1) & ~neighbour_in_set).any(), f"{what}: a pixel was blended with a neighbour outside the set (direction {k})"


def _frame(w=W, h=H):
    return whole_frame_mask(h, w)


# ------------------------------------------------------------------ 1. the pass against the reference
@pytest.mark.parametrize("name", ["cornell", "textured"])
def test_real_planes(ptlib, orc_det, name):
    c = _case(name)
    ref, got, st = _run(c.r, orc_det, c, _frame(), name)
    print(f"{name}: " + ", ".join(f"{k} {st[k]}" for k in COUNTERS) + f", kernel_ms {st['kernel_ms']:.4f}")
    assert 0 < st["blended"] <= st["boundary"] < st["pixels"] and st["stale"] == 0 and st["hits"] == c.gstats["hits"]
    _check_edge_plane(got, _frame(), name)
    assert all(int(((got["edge"].view(f32)[..., 1]) == k).sum()) > 0 for k in (1, 2, 3, 4))  # every direction wins somewhere
    # an unblended pixel keeps its colour's bits
    keep = got["edge"][..., 1] == 0
    assert np.array_equal(got["out"][..., 0:3][keep], c.color.view(np.uint32)[..., 0:3][keep])


def test_each_optional_output_may_be_absent(ptlib, orc_det):
    c = _case("cornell")
    for planes in (("out",), ("out", "edge"), ("out", "frame_rgba8")):
        _run(c.r, orc_det, c, _frame(), f"planes {planes}", planes=planes)
    res = c.r.edgeAaPlanes(_upload(c.color), _upload(c.hit), _upload(c.position))  # the facade allocates out
    assert set(res) == {"out", "edge", "frame_rgba8", "stats"} and res["edge"] is None and res["frame_rgba8"] is None
    assert np.array_equal(_bits(res["out"]), E.edge_aa_ref(c.hit, c.position, c.color, c.verts, c.idx, [(0, 0, W, H)], [c.row], _frame())["out"])


def test_planes_one_float_into_their_allocations(ptlib, orc_det):
    c = _case("textured")
    _run(c.r, orc_det, c, _frame(), "every plane 4 bytes off a 16-byte boundary", offset=True)


@pytest.mark.parametrize("size", [(8, 8), (1, 1), (9, 17), (64, 3)])
def test_small_frames(ptlib, orc_det, size):
    c = _case("cornell")
    w, h = size
    r = _renderer(c.model, size, c.cam)
    g = r.renderGBuffer(("hit", "position"))
    color = _np(r.surfacePlanes(g["hit"], c.table, planes=("albedo",))["albedo"])
    row = R._camera_rows([R.make_camera(c.cam, w / h)])
    _, _, st = _run(r, orc_det, c, _frame(w, h), f"{w} x {h}", hit=_np(g["hit"]), position=_np(g["position"]), color=color, cams=row)
    assert st["pixels"] == w * h and st["hits"] == g["stats"]["hits"] > 0
    r.close()


# ------------------------------------------------------------------ 2. hand-made hit planes on real geometry
def _miss_record(c):
    miss = c.hit.view(np.int32)[..., 3] < 0
    assert miss.any()
    return c.hit[miss][0].copy()


def test_hand_made_records_on_real_geometry(ptlib, orc_det):
    """c.hit with records overwritten in vertical bands, so that each band crosses silhouettes and creases: stale primitives, NaN and inf in
    t, u, v and in the colour, misses at the frame's border and a block of hits inside the background"""
    c = _case("cornell")
    ntri = len(c.idx)
    hit, color = c.hit.copy(), c.color.copy()
    words = hit.view(np.int32)
    was_hit = words[..., 3] >= 0
    band = lambda a, b: was_hit & (np.arange(W)[None, :] >= a) & (np.arange(W)[None, :] < b)  # noqa: E731
    words[..., 3][band(38, 41)] = ntri
    words[..., 3][band(41, 43)] = 0x7FFFFFFF
    hit[..., 1][band(45, 48)] = NAN
    hit[..., 2][band(49, 52)] = INF
    hit[..., 1][band(53, 55)] = -INF
    hit[..., 0][band(57, 60)] = NAN
    hit[..., 0][band(61, 64)] = INF
    hit[..., 2][band(65, 67)] = f32(3e38)
    color[:, 70:73, 0] = NAN
    color[:, 75:77, 2] = INF
    color[:, 79:81, 1] = -INF
    hit[0:3, 82:92] = _miss_record(c)  # misses where the frame has hits, along the top and down its right side
    hit[:, 91:94] = _miss_record(c)
    some = c.hit[was_hit][0]
    hit[50:59, 0:6] = some  # hits at the frame's corner and along its lower border: hit / miss borders on the frame's edge
    hit[56:59, 100:131] = some
    ref, got, st = _run(c.r, orc_det, c, _frame(), "hand-made bands", hit=hit, color=color)
    assert st["stale"] == int(band(38, 43).sum()) > 50 and 0 < st["blended"] < st["boundary"]
    _check_edge_plane(got, _frame(), "hand-made bands")
    # a pixel with a non-finite colour is copied, and is nobody's neighbour
    bad = ~np.isfinite(color[..., 0:3]).all(-1)
    assert not got["edge"][bad].any() and bad.sum() > 300
    e = got["edge"].view(f32)[..., 1]
    assert not (e[:, 69] == 2).any() and not (e[:, 73] == 1).any()
    # the bands did cross edges: the reference dropped candidate directions there for each reason
    assert ref["cand"][ref["X"] == 39].any() and ref["cand"][ref["X"] == 46].any() and ref["cand"][ref["X"] == 58].any()


def test_all_miss_and_all_one_primitive_frames(ptlib, orc_det):
    c = _case("cornell")
    rec = {"all miss": _miss_record(c), "one primitive": c.hit[c.hit.view(np.int32)[..., 3] >= 0][0]}
    for what, record in rec.items():
        hit = np.broadcast_to(record, (H, W, 8)).copy()
        ref, got, st = _run(c.r, orc_det, c, _frame(), what, hit=hit)
        assert st["blended"] == st["boundary"] == 0 and st["hits"] == (0 if what == "all miss" else W * H)
        assert np.array_equal(got["out"][..., 0:3], c.color.view(np.uint32)[..., 0:3]) and (got["out"][..., 3] == S.ONE).all() and not got["edge"].any()


def test_a_record_naming_a_zero_area_triangle(ptlib, orc_det):
    """a mesh collapsed onto a line after the G-buffer was made: its records still name its primitives, which now have nn == 0"""
    c = _case("cornell")
    mesh = np.bincount(c.hit.view(np.int32)[..., 4][c.hit.view(np.int32)[..., 3] >= 0]).argmax()  # the mesh with the most pixels
    r = _renderer(c.model, (W, H), c.cam)
    r.transformMeshes({int(mesh): _affine((0.0, 1.0, 0.0), 0.0, (1.0, 0.0, 0.0), (0.0, 0.5, 0.0))})
    verts = _np(r.copyVerticesDevice())
    tri = verts[c.idx[c.hit.view(np.int32)[..., 3][c.hit.view(np.int32)[..., 4] == mesh]]]
    assert not np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).any()
    ref, got, st = _run(r, orc_det, c, _frame(), "zero-area owner", verts=verts)
    own_mesh = c.hit.view(np.int32)[..., 4][ref["Y"], ref["X"]] == mesh
    owned = ref["cand"] & ref["own_p"] & own_mesh[:, None]
    assert owned.sum() > 50 and not ref["good"][owned].any() and st["boundary"] > 0
    r.close()


# ------------------------------------------------------------------ 3. views, masks, partitions
def test_two_views_off_the_block_grid_with_different_cameras(ptlib, orc_det):
    c = _case("cornell")
    r = _renderer(c.model, (W, H), c.cam)
    rects = RECTS[:2]
    cams = [R.make_camera(c.cam, rects[0][2] / rects[0][3]), R.make_camera(dict(c.cam, fovY=c.cam["fovY"] * 1.3), rects[1][2] / rects[1][3])]
    r.setViews([(x, y, w, h, cam) for (x, y, w, h), cam in zip(rects, cams)])
    rows = R._camera_rows(cams)
    inside = np.zeros((H, W), bool)
    for x, y, w, h in rects:
        inside[y:y + h, x:x + w] = True
    zeros = lambda k: _upload(np.zeros((H, W, k), f32))  # noqa: E731
    g = r.renderGBuffer(("hit", "position"), out=dict(hit=zeros(8), position=zeros(4)))
    color = _np(r.surfacePlanes(g["hit"], c.table, planes=("albedo",), out=dict(albedo=zeros(4)))["albedo"])
    ref, got, st = _run(r, orc_det, c, inside, "two views", hit=_np(g["hit"]), position=_np(g["position"]), color=color, rects=rects, cams=rows)
    assert st["pixels"] == sum(w * h for _, _, w, h in rects) and st["blended"] > 50
    for name in E.PLANES:
        assert (got[name][~inside] == SENTINEL).all()
    _check_edge_plane(got, inside, "two views")  # `inside` is two rectangles that do not touch: no blend crosses a view border
    e = got["edge"].view(f32)[..., 1]
    for x, y, w, h in rects:
        assert not (e[y:y + h, x] == 1).any() and not (e[y:y + h, x + w - 1] == 2).any() and not (e[y, x:x + w] == 3).any() and not (e[y + h - 1, x:x + w] == 4).any()
        assert (e[y:y + h, x:x + w] > 0).sum() > 20
    r.setViews([])
    r.setCamera(R.make_camera(c.cam, W / H))
    _run(r, orc_det, c, _frame(), "views dropped")
    r.close()


def test_block_mask_and_rank_1_of_3(ptlib, orc_det):
    c = _case("cornell")
    nby, nbx = c.r.blockGrid()
    mask = np.random.default_rng(5).random((nby, nbx)) < 0.5
    mask[0, 0] = mask[nby - 1, nbx - 1] = mask[0, nbx - 1] = mask[nby - 1, 3] = True
    mask[1, 1] = False
    px = pixel_mask(mask, h=H, w=W)
    ref, got, st = _run(c.r, orc_det, c, px, "a random block mask", mask=mask)
    assert 0 < st["pixels"] < W * H and all((got[n][~px] == SENTINEL).all() for n in E.PLANES)
    _check_edge_plane(got, px, "a random block mask")
    whole = E.edge_aa_ref(c.hit, c.position, c.color, c.verts, c.idx, [(0, 0, W, H)], [c.row], _frame())
    assert (got["edge"][px] != whole["edge"][px]).any()  # some pixel of the set lost its neighbour to the mask
    _, _, st = _run(c.r, orc_det, c, np.zeros((H, W), bool), "the empty mask", mask=np.zeros((nby, nbx), bool))
    assert st == dict({k: 0 for k in COUNTERS}, kernel_ms=st["kernel_ms"])
    by, bx = np.mgrid[0:H, 0:W] // 8
    r = _renderer(c.model, (W, H), c.cam, partition=(1, 3, 8, 8))
    own = (bx + by) % 3 == 1
    _, got, st = _run(r, orc_det, c, own, "rank 1 of 3")
    assert st["pixels"] == int(own.sum()) and all((got[n][~own] == SENTINEL).all() for n in E.PLANES)
    _check_edge_plane(got, own, "rank 1 of 3")
    r.close()


# ------------------------------------------------------------------ 4. state and parameters
def test_after_transform_meshes_the_pass_follows_the_moved_geometry(ptlib, orc_det):
    c = _case("cornell")
    r = _renderer(c.model, (W, H), c.cam)
    r.transformMeshes({0: _affine((0.0, 1.0, 0.0), 0.1, (1.0, 0.95, 1.0), (5.0, 0.0, -5.0)), 2: _affine((0.0, 0.0, 1.0), -0.05, (1.0, 1.1, 1.0), (0.0, 3.0, 0.0))})
    verts = _np(r.copyVerticesDevice())
    assert not np.array_equal(verts, c.verts)
    g = r.renderGBuffer(("hit", "position"))
    hit, position = _np(g["hit"]), _np(g["position"])
    color = _np(r.surfacePlanes(g["hit"], c.table, planes=("albedo",))["albedo"])
    ref, got, st = _run(r, orc_det, c, _frame(), "after transformMeshes", hit=hit, position=position, color=color, verts=verts)
    rest = E.edge_aa_ref(hit, position, color, c.verts, c.idx, [(0, 0, W, H)], [c.row], _frame())
    assert st["blended"] > 0 and not np.array_equal(rest["edge"], got["edge"]) and not np.array_equal(rest["out"], got["out"])
    r.close()


def test_normal_cos_minus_1_and_a_huge_plane_eps_leave_the_mesh_borders(ptlib, orc_det):
    c = _case("cornell")
    base, _, st0 = _run(c.r, orc_det, c, _frame(), "the defaults")
    ref, got, st = _run(c.r, orc_det, c, _frame(), "normal_cos -1, plane_eps 1e30", normal_cos=-1.0, plane_eps=1e30)
    words = c.hit.view(np.int32)
    mesh = np.where(words[..., 3] >= 0, words[..., 4], -1)
    crease = border = 0
    for k, (dx, dy) in enumerate(E.DIRS):
        qx, qy = np.clip(ref["X"] + dx, 0, W - 1), np.clip(ref["Y"] + dy, 0, H - 1)
        differ = mesh[ref["Y"], ref["X"]] != mesh[qy, qx]
        assert not (ref["cand"][:, k] & ~differ).any()  # no candidate inside a mesh
        border += int((ref["cand"][:, k] & differ).sum())
        crease += int((base["cand"][:, k] & ~differ).sum())
    assert crease > 50 and border > 300 and 0 < st["boundary"] < st0["boundary"] and st["blended"] > 0
    _run(c.r, orc_det, c, _frame(), "normal_cos 1, plane_eps 0", normal_cos=1.0, plane_eps=0.0)


def test_rendering_state_is_left_alone(ptlib):
    c = _case("cornell")
    probe = scenes.sky_probe(256, 128).BuildCDF()

    def run(with_call):
        r = R.SampleRenderer(scenes.cornell_box())
        r.setProbe(probe)
        r.setOptions(frames_in_flight=3)
        r.resize((W, H))
        r.setCamera(R.make_camera(c.cam, W / H))
        r.launchParams.samples_per_launch = 2
        for n in (0, 1):
            r.launchParams.frame.subframe_index = n
            r.render()
        if with_call:
            r.sync()
            before = r.stats()
            res = r.edgeAaPlanes(_upload(c.color), _upload(c.hit), _upload(c.position), edge=_filled("edge", H, W))
            assert res["stats"]["blended"] > 0 and r.stats() == before
        r.launchParams.frame.subframe_index = 2
        r.render()
        r.sync()
        bufs = [r.download(n) for n in range(5)]
        r.close()
        return bufs

    for n, (x, y) in enumerate(zip(run(True), run(False))):
        assert x.tobytes() == y.tobytes(), f"buffer {n} differs after edgeAaPlanes between the frames"


# ------------------------------------------------------------------ 5. what the output means
def test_output_is_closer_to_the_supersampled_truth(ptlib):
    c = _case("cornell")
    big = _renderer(c.model, (SUPER * W, SUPER * H), c.cam)
    g = big.renderGBuffer(("hit",))
    truth = supersampled_truth(_np(big.surfacePlanes(g["hit"], c.table, planes=("albedo",))["albedo"]))
    big.close()
    res = c.r.edgeAaPlanes(_upload(c.color), _upload(c.hit), _upload(c.position))
    e0, e1 = E.rms(c.color[..., 0:3], truth), E.rms(_np(res["out"])[..., 0:3], truth)
    bound = (1 + R_EDGE) / 2
    print(f"edge aa: rms colour {e0:.6f}, rms output {e1:.6f}, ratio {e1 / e0:.5f} (the reference: {R_EDGE}; asserted: <= {bound:.4f}); "
          f"boundary {res['stats']['boundary']}, blended {res['stats']['blended']}")
    assert e0 > 0.01 and e1 <= bound * e0


# ------------------------------------------------------------------ 6. refusals
def test_refusals(ptlib, orc_det):
    c = _case("cornell")
    L = _lib.load_library()
    r = R.SampleRenderer(c.model)
    dev = dict(color=_upload(c.color), hit=_upload(c.hit), position=_upload(c.position))
    out = {n: _filled(n, H, W) for n in E.PLANES}
    good = {n: t.data_ptr() for n, t in list(dev.items()) + list(out.items())}
    good.update(flags=0, normal_cos=0.9, plane_eps=0.01)

    def refused(what, pattern, **fields):
        d = _lib.EdgeAaDesc()
        for n, v in dict(good, **fields).items():
            setattr(d, n, v)
        torch.cuda.synchronize()
        s = _lib.EdgeAaStats(7, 7, 7, 7, 7, 7.0)
        rc = L.pt_edge_aa_planes(r._ctx, C.byref(d), C.byref(s))
        msg = L.pt_last_error(r._ctx).decode()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg.startswith("pt_edge_aa_planes") and pattern in msg, f"{what}: {msg!r}"
        assert tuple(getattr(s, n) for n, _ in s._fields_) == (7, 7, 7, 7, 7, 7.0)
        for n, t in out.items():
            assert (_bits(t) == SENTINEL).all(), f"{what}: {n} was written"

    refused("no resize yet", "pt_resize")
    r.resize((W, H))
    r.setCamera(R.make_camera(c.cam, W / H))
    assert L.pt_edge_aa_planes(r._ctx, None, None) == -1 and "pt_edge_aa_planes: null description" in L.pt_last_error(r._ctx).decode()
    refused("a flag", "unknown flag bits 1", flags=1)
    refused("a flag comes before the planes", "unknown flag bits 4", flags=4, hit=None)
    for bad in (-1.5, 1.25, float("nan"), float("inf")):
        refused(f"normal_cos {bad}", "normal_cos must be in [-1,1]", normal_cos=bad)
    for bad in (-1.0, float("nan"), float("inf"), -1e-30):
        refused(f"plane_eps {bad}", "plane_eps must be finite and >= 0", plane_eps=bad)
    for name in ("color", "hit", "position", "out"):
        refused(f"{name} null", f"{name} is null", **{name: None})
    host = np.zeros((H, W, 8), f32)
    refused("a host pointer", "hit is not device memory", hit=host.ctypes.data)
    refused("a pointer offset by 2 bytes", "edge is not 4-byte aligned", edge=good["edge"] + 2)
    refused("a pointer offset by 1 byte", "color is not 4-byte aligned", color=good["color"] + 1)
    hip = _hip_runtime()
    for name, nbytes in (("edge", H * W * 8), ("frame_rgba8", H * W * 4), ("out", H * W * 16)):
        raw, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert hip.hipMalloc(C.byref(raw), C.c_size_t(nbytes)) == 0
        try:
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= nbytes
            refused(f"{name} one element too small", f"{name} has fewer than {nbytes} bytes left", **{name: raw.value + size.value - (nbytes - 16)})
        finally:
            assert hip.hipFree(raw) == 0
    refused("in place", "color and out overlap", out=good["color"])
    refused("out inside the hit plane", "hit and out overlap", out=good["hit"] + 4 * (H * W * 2))
    refused("edge on the position plane", "position and edge overlap", edge=good["position"])
    refused("the frame inside the colour", "color and frame_rgba8 overlap", frame_rgba8=good["color"] + 16)
    refused("two outputs", "out and edge overlap", edge=good["out"] + 4 * (H * W * 2))
    refused("two outputs", "out and frame_rgba8 overlap", frame_rgba8=good["out"])
    refused("two outputs", "edge and frame_rgba8 overlap", frame_rgba8=good["edge"] + 4 * (H * W))
    # the read-only planes may alias one another: colour and position the same plane
    res = r.edgeAaPlanes(dev["position"], dev["hit"], dev["position"], out=out["out"], edge=out["edge"], frame=out["frame_rgba8"])
    ref = E.edge_aa_ref(c.hit, c.position, c.position, c.verts, c.idx, [(0, 0, W, H)], [c.row], _frame(), planes=E.PLANES, orc=orc_det)
    _same({n: _bits(out[n]) for n in E.PLANES}, ref, "colour and position aliased")
    # the Python facade passes the library's refusals on; a valid call afterwards still works, into the same planes
    with pytest.raises(RuntimeError, match="plane_eps must be finite"):
        r.edgeAaPlanes(dev["color"], dev["hit"], dev["position"], plane_eps=-2.0)
    with pytest.raises(RuntimeError, match="color and out overlap"):
        r.edgeAaPlanes(dev["color"], dev["hit"], dev["position"], out=dev["color"])
    res = r.edgeAaPlanes(dev["color"], dev["hit"], dev["position"], out=out["out"], edge=out["edge"], frame=out["frame_rgba8"])
    ref = E.edge_aa_ref(c.hit, c.position, c.color, c.verts, c.idx, [(0, 0, W, H)], [c.row], _frame(), planes=E.PLANES, orc=orc_det)
    _same({n: _bits(out[n]) for n in E.PLANES}, ref, "a valid call after the refusals")
    assert res["stats"]["blended"] == ref["blended"]
    r.close()


# ------------------------------------------------------------------ 7. the stream contract
@pytest.mark.parametrize("mode", ["default", "side"])
def test_under_a_busy_torch_stream(ptlib, orc_det, mode):
    """tests/test_gpu_stream_contract.py's protocol for this entry point: the three inputs are produced, and the three outputs
    sentinel-filled, by work still pending on torch's current stream when the call is made; the result equals the synchronous call's, and
    that equals the reference"""
    from stream_kit import _pin, _res

    c = _case("cornell")
    outs = {n: _filled(n, H, W) for n in E.PLANES}

    def call(dev, outs, returned):
        res = c.r.edgeAaPlanes(dev["color"], dev["hit"], dev["position"], out=outs["out"], edge=outs["edge"], frame=outs["frame_rgba8"])
        returned()
        return _res(res, outs)

    sync, got = _pin("edgeAaPlanes", mode, c.r, dict(color=c.color, hit=c.hit, position=c.position), outs, call)
    ref = E.edge_aa_ref(c.hit, c.position, c.color, c.verts, c.idx, [(0, 0, W, H)], [c.row], _frame(), planes=E.PLANES, orc=orc_det)
    _same({n: got[n].view(np.uint32).reshape(H, W, -1) for n in E.PLANES}, ref, f"under a busy stream [{mode}]")
    assert got["stats"] == {k: ref[k] for k in COUNTERS}


# ------------------------------------------------------------------ 8. the upsampled loop with --edge-aa
def test_upsampled_loop_with_edge_aa_displays_the_antialiased_frame(ptlib):
    """examples/upsampled_svgf_loop.py's UpsampledLoop with edge_aa=True at 128 x 56, scale 2: the displayed frame is edgeAaPlanes of the
    modulated one; without it the class is what it was"""
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location("upsampled_svgf_loop", os.path.join(ROOT, "examples", "upsampled_svgf_loop.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    w, h = 128, 56
    probe = scenes.sky_probe(256, 128).BuildCDF()
    cam0 = INPUTS["textured"][1]
    up = ex.UpsampledLoop(S.textured_scene(), (w, h), 2, edge_aa=True, probe=probe)
    cam = R.make_camera(cam0, w / h)
    for k in range(2):
        prev, cam = cam, R.make_camera(ex.orbit(cam0, 0.01 * k), w / h)
        up.final.view(torch.uint8).fill_(0xA5)
        x = up.frame(k, prev, cam)
        assert x["pixels"] == w * h and 0 < x["blended"] <= x["boundary"] and x["edge_aa_ms"] > 0
        assert not (_bits(up.final) == SENTINEL).any()
    want = up.hi.edgeAaPlanes(up.modulated, up.hi_gbuf["hit"], up.hi_gbuf["position"], frame=torch.zeros((h, w), dtype=torch.int32, device="cuda:0"))
    assert not _differ(_bits(up.final), _bits(want["out"])).any() and np.array_equal(_np(up.frame_rgba8), _np(want["frame_rgba8"]))
    assert _differ(_bits(up.final)[..., 0:3], _bits(up.modulated)[..., 0:3]).any()
    up.close()
    plain = ex.UpsampledLoop(S.textured_scene(), (w, h), 2, probe=probe)
    assert not plain.edge_aa and plain.modulated is None
    x = plain.frame(0, cam, cam)
    assert x["edge_aa_ms"] == 0.0 and x["blended"] == 0
    plain.close()
