"""A busy non-blocking stream for the stream-order tests (tests/test_gpu_stream_order.py).

A real integration issues the `_device` forms on a non-blocking stream that still works on the previous frame.  Busy makes
that state: one torch.cuda.Stream() (torch creates its streams non-blocking, so null-stream work does not order itself
against them — taken from torch's source, not checked here), a delay of ordinary element-wise passes on it, and behind the
delay the copies that give every device input of the call under test its real contents.  Until then the inputs hold
POISON — another valid input of the same kind — and the outputs a finite sentinel, so a read or a write that is not
ordered on the stream gives a wrong answer and never a fault.

    b = Busy()
    rays = b.late(real, poison)              # poison now, `real` behind the delay
    acc = b.out((n, 4), zeroed=True)         # the sentinel now, zeros behind the delay
    b.start()                                # the delay, then the fills
    ctx.render_rays_device(p, rays.ptr, n, acc.ptr, stream=b.ptr)
    b.issued()                               # still_busy, read right after the last library call
    got = b.fetch(acc)                       # a copy on the same stream
    assert b.finish()                        # the only synchronisation; True = the delay outlasted the issue
    got.numpy()

The delay's length: DELAY_REPS passes over DELAY_BYTES; DESIGN.md "Stream order" has the measurement behind it."""
import time

import numpy as np
import torch

MISS = 0xFFFFFFFF
SENTINEL_BYTE = 0xC1  # four of them: -24.219 as float32, 3250700737 as uint32 — finite, and no count or index of these tests
DELAY_BYTES = 1 << 30
# One pass (x *= 1 over DELAY_BYTES of float32) takes 0.358 ms on the MI355X and the longest call sequence of the module
# 0.96 ms of host time to issue (DESIGN.md "Stream order"): 160 passes are 57 ms, sixty times that — ten times is the rule,
# the rest is room for a host thread that loses its core for a while.
DELAY_REPS = 160

_block = None


def _delay_block():
    global _block
    if _block is None:
        _block = torch.zeros(DELAY_BYTES // 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
    return _block


def delay(stream, reps=None):
    """`reps` element-wise passes over one large tensor on `stream`; the event recorded right behind them."""
    x = _delay_block()
    with torch.cuda.stream(stream):
        for _ in range(DELAY_REPS if reps is None else reps):
            x.mul_(1.0)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def still_busy(event):
    return not event.query()


def rep_ms(reps=50):
    """Device time of one delay pass, by events."""
    s = torch.cuda.Stream()
    x = _delay_block()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        x.mul_(1.0)
        e0.record(s)
        for _ in range(reps):
            x.mul_(1.0)
        e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) / reps


def assert_valid(a, limit=None, what="poison"):
    """What a mis-ordered read may meet: every float finite; with `limit`, every integer an index below it or MISS."""
    a = np.asarray(a)
    if a.dtype.names:
        for f in a.dtype.names:
            assert_valid(a[f], limit, "%s.%s" % (what, f))
    elif a.dtype.kind == "f":
        assert np.isfinite(a).all(), "%s holds a non-finite value" % what
    else:
        assert a.dtype.kind in "iu", (what, a.dtype)
        if limit is not None:
            assert ((a.astype(np.int64) >= 0) & ((a.astype(np.int64) < limit) | (a.astype(np.int64) == MISS))).all(), \
                "%s holds an index outside 0..%d" % (what, limit - 1)


class Buf:
    """A device buffer of the harness: .ptr for the library; its bytes mean `dtype` [shape]."""

    def __init__(self, t, dtype, shape):
        self.t, self.dtype, self.shape = t, np.dtype(dtype), tuple(shape)
        self.ptr = t.data_ptr()

    def numpy(self):
        return self.t.cpu().numpy().view(self.dtype).reshape(self.shape)


class Busy:
    def __init__(self):
        self.stream = torch.cuda.Stream()
        self.ptr = self.stream.cuda_stream
        self._late, self._zero, self._keep = [], [], []
        self.event = self.busy = self.issue_ms = None
        self._t0 = None

    def _dev(self, a):
        a = np.ascontiguousarray(a)
        with torch.cuda.stream(self.stream):
            t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        return Buf(t, a.dtype, a.shape)

    def late(self, real, poison, limit=None, distinct=True):
        """A device buffer that holds `poison` now and `real` once the next delay has run.  limit: the arrays hold indices
        below it (or MISS).  distinct=False: a channel that may well agree between two inputs (a mesh map, a hit count)."""
        real, poison = np.ascontiguousarray(real), np.ascontiguousarray(poison)
        assert real.shape == poison.shape and real.dtype == poison.dtype
        assert_valid(poison, limit)
        assert_valid(real, limit, "input")
        assert not distinct or real.tobytes() != poison.tobytes(), "the poison is the input itself"
        dst, src = self._dev(poison), self._dev(real)
        self._late.append((dst, src))
        return dst

    def resident(self, a):
        """A device buffer that holds `a` from the start (no part of the call under test)."""
        b = self._dev(a)
        self._keep.append(b)
        return b

    def out(self, shape, dtype=np.float32, zeroed=False):
        """An output buffer holding the sentinel; zeroed: zeros behind the next delay (a caller-zeroed accumulator)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        with torch.cuda.stream(self.stream):
            t = torch.full((n,), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
        b = Buf(t, dtype, shape)
        self._keep.append(b)
        if zeroed:
            self._zero.append(b)
        return b

    def start(self, reps=None):
        """The delay, then the fills and zeroings registered since the last start."""
        self.stream.synchronize()  # (poison and sentinels are in place before the delay begins)
        self.event = delay(self.stream, reps)
        with torch.cuda.stream(self.stream):
            for dst, src in self._late:
                dst.t.copy_(src.t, non_blocking=True)
            for b in self._zero:
                b.t.zero_()
        self._keep += [x for pair in self._late for x in pair]
        self._late, self._zero = [], []
        self.busy = None
        self._t0 = time.perf_counter()
        return self.event

    def issued(self):
        """Right after the last library call: is the delay still running?  Also the host time since start()."""
        self.busy = still_busy(self.event)
        self.issue_ms = (time.perf_counter() - self._t0) * 1e3
        return self.busy

    def fetch(self, buf):
        """A copy of buf as it is at this point of the stream."""
        with torch.cuda.stream(self.stream):
            return Buf(buf.t.clone(), buf.dtype, buf.shape)

    def finish(self):
        assert self.busy is not None, "issued() was not called"
        self.stream.synchronize()
        return self.busy
