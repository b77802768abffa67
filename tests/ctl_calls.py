"""What the control-plane GPU tests share beyond their families' harnesses: a harness call taken in three steps, so that
several calls can be queued with no host wait between them, and the two helpers of the stream tests, a delay that keeps
a stream busy and the choice of two streams that really run side by side."""
from __future__ import annotations


class Call:
    """A harness call written as a generator with two yields. Creating the Call runs it to the first yield: the uploads,
    the result fills and everything else that uses the current stream or waits on the host. issue() runs the library
    call itself and nothing else. finish() waits for the device, applies the call to the model and compares; calls on
    one model finish in the order they were issued."""

    def __init__(self, gen):
        self.gen = gen
        next(gen)

    def issue(self) -> None:
        next(self.gen)

    def finish(self):
        try:
            next(self.gen)
        except StopIteration as e:
            return e.value
        raise AssertionError("a harness call has exactly two yields")


def run(gen):
    """The three steps in a row: what a harness method did before it was cut in steps."""
    c = Call(gen)
    c.issue()
    return c.finish()


# ---- streams -------------------------------------------------------------------------------------------------------------
DELAY_MS = 100
_cycles_per_ms = None


def cycles_per_ms() -> float:
    """torch.cuda._sleep counts device clock cycles: one sleep timed with two events, once per process."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        import torch

        torch.cuda._sleep(1_000_000)  # the first launch pays for loading the kernel
        torch.cuda.synchronize()
        probe = 20_000_000
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        _cycles_per_ms = probe / max(a.elapsed_time(b), 1e-3)
    return _cycles_per_ms


def delayed(stream, ms: float = DELAY_MS):
    """About `ms` milliseconds of sleep queued on `stream`; returns an event recorded behind it. The length is a
    condition, not a measurement: a test asserts `not event.query()` after it has issued its calls, which proves that
    the work queued on `stream` before them was still pending."""
    import torch

    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * cycles_per_ms()))
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


_pair = None


def stream_pair():
    """Two streams that run side by side: with one delayed, a fill on the other completes while the delay is pending.
    Two torch streams can share a hardware queue, which serialises them whatever the library does, so up to 8 fresh
    streams are tried. Returns (A, B, (i, j)), their places among the streams made; fails when no pair qualifies."""
    global _pair
    if _pair is None:
        import torch

        streams = [torch.cuda.Stream(device=0) for _ in range(8)]
        x = torch.zeros(64, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        for i, a in enumerate(streams):
            for j, b in enumerate(streams):
                if i == j or _pair is not None:
                    continue
                ev = delayed(a, 30)
                with torch.cuda.stream(b):
                    x.fill_(i * 8 + j)
                    done = torch.cuda.Event()
                    done.record(b)
                done.synchronize()
                if not ev.query():
                    _pair = (a, b, (i, j))
                torch.cuda.synchronize()
        assert _pair is not None, "no two of 8 fresh streams run side by side: a fill always waited for the other's delay"
    return _pair
