"""Pending GPU work of known length on torch's current stream (a helper of tests/test_gpu_stream_contract.py, not a test).

filler(ms) enqueues repeated `big.add_(1.0)` over one 64 Mi-float tensor, the idiom of
tests/test_gpu_schedule.py::test_wait_event_orders_the_context_behind_the_callers_stream.  Public torch API only: no sleep kernel, no kernel
that waits for the host, no graph.  The cost of one repeat is measured once per process with torch events after a warm-up; the number of
repeats follows from it.  Nothing here waits on the host after the measurement: whoever calls filler() decides when to look."""
import math

import torch

ELEMENTS = 64 << 20  # floats: 256 MiB read and written per repeat
MIN_MS = 10.0        # no filler is shorter
MARGIN = 50.0        # a filler lasts this many times the host wall time of the call it has to outlast
MAX_MS = 200.0       # a case that would need more fails with its numbers instead of running longer
WARMUP, TIMED = 8, 32

_state = {}


def _big():
    if "big" not in _state:
        _state["big"] = torch.zeros(ELEMENTS, dtype=torch.float32, device="cuda:0")
    return _state["big"]


def repeat_ms():
    """Milliseconds of one `big.add_(1.0)`, measured once per process on torch's current stream (which it leaves idle)."""
    if "repeat_ms" not in _state:
        big = _big()
        for _ in range(WARMUP):
            big.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(TIMED):
            big.add_(1.0)
        e1.record()
        e1.synchronize()
        _state["repeat_ms"] = e0.elapsed_time(e1) / TIMED
        assert _state["repeat_ms"] > 0
    return _state["repeat_ms"]


def length_ms(wall_s, what=""):
    """The rule: max(10 ms, 50 x the host wall time of the case's synchronous reference call); more than 200 ms fails the case."""
    ms = max(MIN_MS, MARGIN * wall_s * 1e3)
    if ms > MAX_MS:
        raise AssertionError(f"{what}: the reference call took {wall_s * 1e3:.3f} ms on the host, so the filler would have to last {ms:.1f} ms "
                             f"(> {MAX_MS:.0f} ms): the case is too slow for a timing-based pin")
    return ms


def repeats(ms):
    return int(math.ceil(ms / repeat_ms())) + 1


def filler(ms):
    """Enqueues at least `ms` milliseconds of work on torch's current stream; returns the number of repeats.  Does not wait."""
    n = repeats(ms)  # (measures first, if this is the first call: the measurement ends with a host wait, the filler never does)
    big = _big()
    for _ in range(n):
        big.add_(1.0)
    return n


def concurrent(lib_stream, what=""):
    """Does a kernel on the library's stream (pt_stream as an integer) run while a filler is pending on torch's current stream?  HIP deals
    its streams onto a few hardware queues in creation order (Streams); two streams on one queue serialise although nothing orders
    them.  A stream pair that serialises hides a lost ordering, so a test that wants to SEE one asks first.  One tiny fill goes to the
    library's stream behind no event; when it is done the filler's event says whether the filler was still pending."""
    ext = torch.cuda.ExternalStream(lib_stream, device=0)
    probe = torch.zeros(64, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    filler(MIN_MS)
    pending = torch.cuda.Event()
    pending.record()
    with torch.cuda.stream(ext):
        probe.fill_(1.0)
        done = torch.cuda.Event()
        done.record()
    done.synchronize()
    result = not pending.query()
    torch.cuda.synchronize()
    print(f"{what}: the library's stream runs {'beside' if result else 'BEHIND'} torch's {torch.cuda.current_stream()}")
    return result
