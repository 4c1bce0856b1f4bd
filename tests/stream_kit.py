"""The protocol of the stream contract (tests/test_gpu_stream_contract.py states its eight steps): a call is made once synchronously for its
reference, then again behind a pending filler on torch's stream, and must wait for it.  The passes added since pin themselves with _pin."""
import contextlib
import time

import numpy as np
import torch

import busy_stream as busy
from gpu_kit import differ as _differ

f32 = np.float32
SENTINEL = 0xA5A5A5A5


def _snapshot(res):
    """{name: the words of a tensor or an array, "stats": the counters (no times)} of what a call returned"""
    got = {}
    for k, v in res.items():
        if v is None:
            continue
        if k == "stats":
            got[k] = {s: x for s, x in v.items() if not s.endswith("_ms")}
        elif isinstance(v, torch.Tensor):
            got[k] = v.cpu().numpy().copy()
        else:
            got[k] = np.array(v, copy=True)
    return got


def _same(got, ref, what):
    assert got.keys() == ref.keys(), (what, sorted(got), sorted(ref))
    for k, a in got.items():
        if k == "stats":
            assert a == ref[k], f"{what}: counters {a} against the reference call's {ref[k]}"
            continue
        assert a.shape == ref[k].shape and a.dtype == ref[k].dtype, (what, k)
        neq = _differ(a, ref[k])
        if neq.any():
            sent = int((a.view(np.uint32) == SENTINEL).sum()) if a.dtype.itemsize == 4 else 0
            raise AssertionError(f"{what}: {k} differs from the reference call in {int(neq.sum())} of {a.size} words ({sent} words hold the sentinel)")


def _differs(a, b):
    return any(k != "stats" and _differ(v, b[k]).any() for k, v in a.items())


def _sentinel(t):
    t.view(torch.uint8).fill_(0xA5)


def _dev(a):
    """an array's bytes as a CUDA tensor of its shape, 16-byte aligned; uploaded synchronously"""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, f"_dev: 4-byte words are expected, not {a.dtype}"
    t = torch.empty(a.shape, dtype=torch.float32 if a.dtype == f32 else torch.int32, device="cuda:0")
    t.copy_(torch.from_numpy(a.view(f32 if a.dtype == f32 else np.int32).copy()))
    assert t.is_contiguous() and t.data_ptr() % 16 == 0, f"_dev: {tuple(a.shape)} lies at {t.data_ptr():#x}"
    return t


def _raw(shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda:0")


_BESIDE = {}  # case -> {mode: did the library's stream run beside torch's}


@contextlib.contextmanager
def _stream(mode, r, what):
    """default: torch's default stream.  side: a fresh side stream, of up to three the first that runs beside the library's; a case whose
    default run (if it was made) and side run were both behind the library's stream cannot see a lost ordering and fails.  teeth: the first
    of the default stream and three fresh ones that runs beside the library's, which the test needs."""
    lib = r.stream
    seen = _BESIDE.setdefault(what, {})
    if mode == "default":
        seen[mode] = busy.concurrent(lib, what)
        yield
        return
    if mode == "teeth" and busy.concurrent(lib, what):
        yield
        return
    for _ in range(3):
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            beside = busy.concurrent(lib, what)
        if beside:
            break
    if mode == "teeth":
        assert beside, f"{what}: none of torch's default stream and three fresh streams runs beside the library's: a lost ordering cannot show"
    else:
        seen[mode] = beside
        assert any(seen.values()), f"{what}: the library's stream ran behind torch's on every stream tried ({seen}): the case cannot see a lost ordering"
    with torch.cuda.stream(side):
        yield


def _pin(what, mode, r, B, outs, call, A=None, raw=False, broken=False):
    """The eight steps (module docstring).  B: {name: array}, the inputs' content; A: the stale content (zeros where not given); outs:
    {name: tensor}; call(dev, outs, returned) makes the facade call on the tensors of dev and outs, calls returned() as soon as the
    synchronous entry point is back, and returns {name: tensor or array, "stats": dict}.  raw: the call hands raw pointers over, so the
    ordering is pt_wait_event(E), the C-level half of the contract.  broken: the ordering has been taken out (test_the_pin_has_teeth) — no
    pending fill, E still pending after the call, outputs equal S.  Returns (R, what the ordered call gave)."""
    per = busy.repeat_ms()
    dev = {k: _dev(v) for k, v in B.items()}
    staged = {k: _dev(v) for k, v in B.items()}
    stale = {k: _dev((A or {}).get(k, np.zeros_like(v))) for k, v in B.items()}
    flags = []

    def sync_call():
        for t in outs.values():
            _sentinel(t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call(dev, outs, lambda: flags.append(time.perf_counter()))
        return _snapshot(res), flags[-1] - t0  # (the host wall time of the entry point itself: up to returned())

    sync_call()  # (first use of the entry point by this context: allocations, code loading)
    ref, wall = sync_call()  # 1
    S = None
    if B:  # 2
        for k, t in dev.items():
            t.copy_(stale[k])
        S, _ = sync_call()
        assert _differs(S, ref), f"{what}: stale inputs give the reference's outputs: the case cannot tell stale from fresh"
    else:
        assert not broken, f"{what}: a case without inputs has no stale outputs to show a removed ordering"
        for t in outs.values():
            t.zero_()
    assert len(flags) == (3 if B else 2), f"{what}: the case never said when its entry point returned"
    ms = busy.length_ms(wall, what)
    torch.cuda.synchronize()  # 3
    with _stream(mode, r, what):
        if broken:
            for t in outs.values():
                _sentinel(t)
            torch.cuda.synchronize()
        n = busy.filler(ms)  # 4
        for k, t in dev.items():
            t.copy_(staged[k])
        if not broken:
            for t in outs.values():
                _sentinel(t)
        E = torch.cuda.Event()
        E.record()
        pending = not E.query()  # 5
        print(f"{what} [{mode}]: {per:.4f} ms per repeat, reference call {wall * 1e3:.3f} ms on the host, filler {ms:.1f} ms = {n} repeats")
        assert pending, f"{what}: the filler ({n} repeats, {ms:.1f} ms) had ended before the call was made"
        if raw:
            r.waitEvent(E.cuda_event)
        state = []
        res = call(dev, outs, lambda: state.append(E.query()))  # 6
        torch.cuda.synchronize()
        got = _snapshot(res)
    assert len(state) == 1, f"{what}: the case said {len(state)} times that its entry point returned"
    if broken:
        assert not state[0], f"{what}: with the ordering removed the call still ended behind the pending work"
        _same(got, S, f"{what}, ordering removed: stale outputs expected")
    else:
        assert state[0], f"{what}: the call returned while the work it had to wait for was still pending"  # 7
        _same(got, ref, what)  # 8
    return ref, got


def _res(res, outs):
    return dict({k: outs[k] for k in outs}, stats=res["stats"])
