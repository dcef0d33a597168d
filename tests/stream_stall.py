"""A stall of known length on a stream, for tests/test_gpu_stream_order.py: device work that keeps a stream busy while the host goes
on enqueueing behind it, so that work launched on the wrong stream, or a buffer replaced under work still queued, finishes in the
wrong order instead of being saved by timing.

stall(stream) enqueues torch.cuda._sleep for STALL_MS milliseconds (cycles per millisecond calibrated once per process with two
events; if _sleep does not hold the stream for the time asked for, a chain of matrix products sized by the same calibration) and
returns an event recorded right behind it.  No gate the host opens: a library call that waits for the stream -- the documented
behaviour of a setter's next call -- would never return behind one.

STALL_MS.  The slowest warm "call A" of tests/test_gpu_stream_order.py with no stall in front of it is the long-row family's
process_device into the D x H layout (2048 x 8 -> 65536 points, 11 rows), whose host-side enqueue measured 0.05 to 0.06 ms on an MI355X
(time.perf_counter around the call on a drained device, the smallest of three; test_enqueue_times_and_stall_length prints the list
and holds STALL_MS to it).  One hundred times that is 6 ms, below the floor of 10 ms; the 130 calls of the ticket test return in
1.2 to 1.3 ms together.  STALL_MS = 50 leaves a host thread that loses its CPU for a few milliseconds inside the stall, and lies within
the 10 .. 100 ms a stall may take.  (Calibration on that card: torch.cuda._sleep, 2.39 million cycles per millisecond; a stall
asked to last 10 ms measured 9.98 ms.)

Every case that uses a stall asserts with `still_running` that the stall's event is not complete when its call A has returned: a
case where it is complete proves nothing and fails."""
import time

STALL_MS = 50.0
_CAL = {}


def _elapsed_ms(torch, stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        fn()
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def calibration():
    """{'mode': 'sleep' | 'matmul', 'per_ms': cycles (or products) per millisecond, 'check_ms': what a 10 ms stall measured}."""
    if _CAL:
        return _CAL
    import torch
    st = torch.cuda.Stream()
    probe = 20_000_000
    mode, per_ms = "sleep", 0.0
    try:
        torch.cuda._sleep(1_000_000)
        torch.cuda.synchronize()
        ms = _elapsed_ms(torch, st, lambda: torch.cuda._sleep(probe))
        per_ms = probe / ms if ms > 0.5 else 0.0
        if per_ms:
            check = _elapsed_ms(torch, st, lambda: torch.cuda._sleep(int(10 * per_ms)))
            if not 7.0 <= check <= 20.0:
                per_ms = 0.0
    except (AttributeError, RuntimeError):
        per_ms = 0.0
    if not per_ms:   # _sleep is missing or does not keep time on this card: matrix products instead
        mode = "matmul"
        _CAL["m"] = torch.randn(2048, 2048, device="cuda")
        _CAL["m"] /= 64.0

        def products(n):
            x = _CAL["m"]
            for _ in range(n):
                x = torch.mm(_CAL["m"], x)
        torch.cuda.synchronize()
        _elapsed_ms(torch, st, lambda: products(8))
        per_ms = 64 / _elapsed_ms(torch, st, lambda: products(64))
        check = _elapsed_ms(torch, st, lambda: products(max(1, int(10 * per_ms))))
        _CAL["products"] = products
    _CAL.update(mode=mode, per_ms=per_ms, check_ms=check)
    return _CAL


def stall(stream, ms=STALL_MS):
    """Enqueues `ms` milliseconds of device work on `stream`; returns an event recorded right after it."""
    import torch
    cal = calibration()
    n = max(1, int(ms * cal["per_ms"]))
    with torch.cuda.stream(stream):
        if cal["mode"] == "sleep":
            torch.cuda._sleep(n)
        else:
            cal["products"](n)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def still_running(ev, what=""):
    """The condition of every stalled case, to be called when call A has returned."""
    assert not ev.query(), "%s: the stall ended before the call returned: this run proves nothing" % what


def enqueue_ms(fn, repeat=5):
    """The warm host-side time of fn() in milliseconds: the smallest of `repeat` calls, each on a drained device."""
    import torch
    best = float("inf")
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return best
