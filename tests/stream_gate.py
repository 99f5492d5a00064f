"""The stream gate: does an entry enqueue ALL its work on the stream it is given?  (A plain module, not a conftest.)

On the legacy null stream a launch that forgot its stream argument, a memset on the wrong stream or a helper that copies
on stream 0 is invisible: the null stream orders itself against everything.  On a non-blocking stream -- what
torch.cuda.Stream() creates -- the same mistake is a silent data race.  A GATED CALL makes the race deterministic:

  1. the real operands are staged in tensors of their own; the device is synchronised;
  2. every operand buffer the entry reads is prefilled with poison (NaN for float data, 0x7FC0 for bf16 storage, ZERO for
     whatever a kernel turns into an address or a bin: a stray launch computes a wrong number, never a wrong address);
     every written buffer is prefilled with the suite's sentinel 0x4B3C2D1E;
  3. on the side stream s: the delay, the event e_gate, then the device-to-device copies of the staged operands;
  4. `not e_gate.query()` is asserted, then the entry is called with s.cuda_stream;
  5. for an entry that does not synchronise, `not e_gate.query()` is asserted again when the call returns: the host did
     not wait;
  6. s is synchronised and the outputs are read.

Work that follows the stream sees the operands.  Work anywhere else runs while the gate is shut, reads poison and writes
NaN, or is overwritten by the sentinel's absence -- the outputs then differ from the EXPECTED bits, which are the outputs
of the same entry on the same staged operands on the null stream (these kernels are atomics-free and bit-reproducible, and
the operator tests hold the null-stream result against float64).  A gate that was already open at step 4 or 5 proves
nothing: the case FAILS as inconclusive, it never passes and nothing retries it.

Argument descriptions (Case.args): In / InOut / Out / Scratch device buffers, HostIn / HostOut host arrays, PtrTable (a host array
of device addresses), STREAM, None (a NULL pointer) and plain ints / floats, converted by the binding's argtypes.
"""
import ctypes as C
import time

import numpy as np
import torch

DEV = "cuda:0"
SENT_U32 = 0x4B3C2D1E
GUARD = 256                      # sentinel bytes in front of and behind every device buffer
MIN_GATE_MS = 20.0
GATE_FACTOR = 5.0
STREAM = object()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _sentinel_bytes(n):
    return np.resize(np.array([SENT_U32], np.uint32).view(np.uint8), n)


def poison_bytes(kind, nbytes):
    if kind == "zero":
        return np.zeros(nbytes, np.uint8)
    if kind == "nan":
        assert nbytes % 4 == 0
        return np.full(nbytes // 4, 0x7FC00000, np.uint32).view(np.uint8)
    if kind == "nan64":
        assert nbytes % 8 == 0
        return np.full(nbytes // 8, 0x7FF8000000000000, np.uint64).view(np.uint8)
    if kind == "bf16nan":
        assert nbytes % 2 == 0
        return np.full(nbytes // 2, 0x7FC0, np.uint16).view(np.uint8)
    raise ValueError(kind)


class In:
    """A device operand the entry only reads.  poison None: by dtype -- NaN for float32 / float64, else zero."""
    written = False

    def __init__(self, data, poison=None):
        self.data = np.ascontiguousarray(data)
        if poison is None:
            poison = {np.dtype(np.float32): "nan", np.dtype(np.float64): "nan64"}.get(self.data.dtype, "zero")
        self.poison = poison
        self.nbytes = self.data.nbytes


class InOut(In):
    """A device operand the entry reads and writes (an accumulator, a dz it adds to)."""
    written = True


class Out:
    """A device buffer the entry writes without reading it; off: the pointer handed over starts off bytes into it."""
    written = True

    def __init__(self, nbytes, off=0):
        self.nbytes, self.off = int(nbytes), off


class Scratch(Out):
    """A device workspace the entry is handed: its guards are held, what it holds afterwards is not compared (the header
    promises nothing about it -- the union-find parents of depgan_eval_cc_label, for one, depend on the order in which
    the atomics land, while every output does not)."""
    compared = False


class HostIn:
    def __init__(self, data):
        self.data = np.ascontiguousarray(data)


class HostOut:
    def __init__(self, dtype, n):
        self.dtype, self.n = np.dtype(dtype), n


class PtrTable:
    """A host array of device addresses: entries are (index of a device argument in `extra`, byte offset) or None."""

    def __init__(self, entries):
        self.entries = entries


class Case:
    """One row: the entry's name, its argument list, whether the entry synchronises its stream (then step 5 is not
    asserted), `extra`: device buffers reached only through a PtrTable."""

    def __init__(self, fn, args, sync, extra=()):
        self.fn, self.args, self.sync, self.extra = fn, list(args), sync, list(extra)


class _Buf:
    def __init__(self, spec):
        self.spec = spec
        self.t = torch.empty(GUARD + spec.nbytes + GUARD, dtype=torch.uint8, device=DEV)
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + GUARD
        if isinstance(spec, In):
            self.staged = torch.from_numpy(_bytes(spec.data).copy()).to(DEV)
            fill = poison_bytes(spec.poison, spec.nbytes)
        else:
            self.staged = None
            fill = _sentinel_bytes(spec.nbytes)
        whole = np.concatenate([_sentinel_bytes(GUARD), fill, _sentinel_bytes(GUARD)])
        self.prefill = torch.from_numpy(whole).to(DEV)

    def body(self):
        return self.t[GUARD:GUARD + self.spec.nbytes]

    def reset(self):
        self.t.copy_(self.prefill)

    def load(self):
        if self.staged is not None:
            self.body().copy_(self.staged, non_blocking=True)


class Bound:
    """A Case with its device buffers allocated and its ctypes arguments built."""

    def __init__(self, lib, case):
        self.case, self.fn = case, getattr(lib, case.fn)
        self.bufs, self.hosts, self.keep = [], [], []
        self.extra = [self._dev(s) for s in case.extra]
        self.cargs, self.stream_at = [], None
        for i, a in enumerate(case.args):
            if a is STREAM:
                self.stream_at = i
                self.cargs.append(None)
            elif isinstance(a, (In, Out)):
                b = self._dev(a)
                self.cargs.append(C.c_void_p(b.ptr + getattr(a, "off", 0)))
            elif isinstance(a, HostIn):
                self.keep.append(a.data)
                self.cargs.append(C.c_void_p(a.data.ctypes.data))
            elif isinstance(a, HostOut):
                h = np.zeros(a.n, a.dtype)
                self.hosts.append(h)
                self.cargs.append(C.c_void_p(h.ctypes.data))
            elif isinstance(a, PtrTable):
                tab = np.array([0 if e is None else self.extra[e[0]].ptr + e[1] for e in a.entries], np.uint64)
                self.keep.append(tab)
                self.cargs.append(C.c_void_p(tab.ctypes.data))
            else:
                self.cargs.append(a)
        assert self.stream_at is not None, case.fn
        assert len(self.cargs) == len(self.fn.argtypes), (case.fn, len(self.cargs), len(self.fn.argtypes))

    def _dev(self, spec):
        b = _Buf(spec)
        self.bufs.append(b)
        return b

    def reset(self):
        for b in self.bufs:
            b.reset()
        for h in self.hosts:
            h.view(np.uint8)[:] = 0xA5

    def call(self, stream_handle):
        args = list(self.cargs)
        args[self.stream_at] = C.c_void_p(stream_handle)
        t0 = time.perf_counter()
        rc = self.fn(*args)
        return rc, time.perf_counter() - t0

    def snapshot(self, rc):
        """status, host outputs, every device buffer whole (guards included), as bytes"""
        dev = [b.t.cpu().numpy() for b in self.bufs]
        for b, a in zip(self.bufs, dev):
            if not getattr(b.spec, "compared", True):
                a[GUARD:-GUARD] = 0
        return [np.array([rc], np.int64).view(np.uint8)] + [h.view(np.uint8).copy() for h in self.hosts] + dev

    def guards_intact(self, snap):
        g = _sentinel_bytes(GUARD)
        dev = snap[1 + len(self.hosts):]
        bad = [i for i, (b, a) in enumerate(zip(self.bufs, dev))
               if not (np.array_equal(a[:GUARD], g) and np.array_equal(a[-GUARD:], g))]
        ro = [i for i, (b, a) in enumerate(zip(self.bufs, dev))
              if not b.spec.written and not np.array_equal(a[GUARD:-GUARD], _bytes(b.spec.data))]
        return bad, ro


def null_run(bound):
    """The expected bits: the entry on the staged operands on the null stream.  Returns (snapshot, host seconds of the
    second call -- the first one pays for loading the code object)."""
    secs = None
    for _ in range(2):
        bound.reset()
        for b in bound.bufs:
            b.load()
        torch.cuda.synchronize()
        rc, secs = bound.call(0)
        torch.cuda.synchronize()
    return bound.snapshot(rc), secs


# ---------------------------------------------------------------------------------------------------------------------
# the delay
# ---------------------------------------------------------------------------------------------------------------------
class Delay:
    """torch.cuda._sleep calibrated once: two lengths timed with events, solved for a duration.  Without _sleep, a chain
    of large matmuls, calibrated the same way."""

    def __init__(self):
        self.sleep = getattr(torch.cuda, "_sleep", None)
        if self.sleep is None:
            self.m = torch.ones(2048, 2048, device=DEV)
        lo, hi = (2_000_000, 20_000_000) if self.sleep is not None else (4, 24)
        self._run(lo)
        torch.cuda.synchronize()
        t_lo, t_hi = self._time(lo), self._time(hi)
        self.per_unit = (t_hi - t_lo) / (hi - lo)
        self.fixed = t_lo - self.per_unit * lo
        assert self.per_unit > 0, (t_lo, t_hi)

    def _run(self, units):
        if self.sleep is not None:
            self.sleep(int(units))
        else:
            a = self.m
            for _ in range(int(units)):
                a = (a @ self.m) * (1.0 / 2048)

    def _time(self, units):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self._run(units)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def enqueue(self, ms):
        """on torch's current stream"""
        self._run(max(1, int(np.ceil((ms - self.fixed) / self.per_unit))))


_DELAY = None


def session_delay():
    """the one calibrated Delay of the session, shared by every test file"""
    global _DELAY
    if _DELAY is None:
        _DELAY = Delay()
    return _DELAY


def gate_ms(longest_call_seconds):
    return max(MIN_GATE_MS, GATE_FACTOR * 1e3 * longest_call_seconds)


class Gate:
    """Steps 3 to 6 around any callable: `load()` enqueues the operand copies on torch's current stream."""

    def __init__(self, delay, ms):
        self.delay, self.ms = delay, ms

    def run(self, s, load, call, sync, what):
        """call() runs at step 4; returns its value after step 6.  s: the side stream the operands become valid on."""
        torch.cuda.synchronize()
        e_gate = torch.cuda.Event()
        with torch.cuda.stream(s):
            self.delay.enqueue(self.ms)
            e_gate.record(s)
            load()
        assert not e_gate.query(), "%s: inconclusive, the gate was open before the call" % what
        r = call()
        if not sync:
            assert not e_gate.query(), "%s: inconclusive, the gate was open when the call returned -- the host waited " \
                                       "(or the gate of %.0f ms is too short)" % (what, self.ms)
        s.synchronize()
        torch.cuda.synchronize()
        return r


def gated_run(bound, gate, s, stream_handle=None, sync=None):
    """The gated call of a Bound case on side stream s; the entry gets s.cuda_stream, or stream_handle (the negative
    control hands it the null stream).  Returns the snapshot."""
    bound.reset()
    torch.cuda.synchronize()

    def load():
        for b in bound.bufs:
            b.load()

    h = s.cuda_stream if stream_handle is None else stream_handle
    rc = gate.run(s, load, lambda: bound.call(h)[0], bound.case.sync if sync is None else sync, bound.case.fn)
    return bound.snapshot(rc)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def first_difference(bound, got, want):
    names = ["status"] + ["host output %d" % i for i in range(len(bound.hosts))] + \
            ["device buffer %d (%s)" % (i, type(b.spec).__name__) for i, b in enumerate(bound.bufs)]
    for n, x, y in zip(names, got, want):
        if not np.array_equal(x, y):
            d = np.flatnonzero(x != y)
            return "%s: %d bytes differ, first at byte %d" % (n, d.size, int(d[0]) - (GUARD if "device" in n else 0))
    return "no difference"
