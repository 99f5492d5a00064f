"""GPU, the stream contract of a context: depgan_set_stream puts ALL the work of every context entry on the stream it
names -- a non-blocking side stream included.

Three contexts with the same weights, noise, inputs and Adam step walk the same list of entries through the C ABI:
  W  a warm-up walk on the null stream (it pays for loading every code object, so the timed walk does not);
  A  stays on the null stream: the expected bits and the host-side duration of every call;
  B  is moved to the side stream s with depgan_set_stream and every call is a GATED CALL (tests/stream_gate.py): x, y2, z,
     ep, the k noises and the labels hold poison and only become valid on s behind the delay (NaN; class codes ZERO).
Every device output, host scalar, depgan_last_sums and status of B equals A's bit for bit, and so do the arenas (params,
BatchNorm statistics, grads, Adam m and v) after every entry that writes one.  depgan_apply_adam has no caller operand:
its operand is the gradient arena, which is poisoned and restored behind the gate in the same way.

The gate is 5 x the longest host-side call of walk A (20 ms at least).  A gate found open is a failure (inconclusive).
Two side streams at most are alive at a time.
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_gate as sg  # noqa: E402

pytestmark = pytest.mark.gpu
NETS = ("G", "D_y2", "D_dem")
IMG, B, K = 64, 2, 2          # the smallest configuration of tests/test_gpu_steps.py; K noises of the best-of-k entries
SENT = np.array(sg.SENT_U32, np.uint32).view(np.float32)[()]


@pytest.fixture(scope="module")
def delay(lib):
    return sg.session_delay()


@pytest.fixture(scope="module")
def side():
    return torch.cuda.Stream()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _weights(nicg, nc_out, seed=57):
    from oracle import depgan_oracle as O
    PG = O.init_generator(seed, nicg=nicg, bias_std=0.05, nc_out=nc_out)
    if nc_out != 1:
        return {"G": PG}
    return {"G": PG, "D_y2": O.init_critic(seed + 1, bias_std=0.05, img=IMG),
            "D_dem": O.init_critic(seed + 2, bias_std=0.05, img=IMG)}


def _operands(nicg, nc_out, seed=57):
    """host arrays of every caller operand of the walk"""
    from oracle import depgan_oracle as O
    x, y2, z, ep = O.synth_batch(seed + 5, B, IMG, IMG, nicg=nicg)
    rng = np.random.default_rng(seed)
    ops = {"x": (x + 0.02 * rng.uniform(size=x.shape)).astype(np.float32),
           "y2": (y2 + 0.02 * rng.uniform(size=y2.shape)).astype(np.float32),
           "z": np.asarray(z, np.float32).reshape(B, 32), "ep": np.asarray(ep, np.float32).reshape(B),
           "zs": rng.standard_normal((K, B, 32)).astype(np.float32)}
    if nc_out != 1:
        codes = rng.integers(0, nc_out, (B, IMG, IMG)).astype(np.uint8)
        ops["codes"] = codes
        ops["onehot"] = np.eye(nc_out, dtype=np.float32)[codes]
    return ops


def _engine(mode, nicg, nc_out, weights):
    import dep_gan_im_amd as dg
    kw = dict(beta1=0.9, beta2=0.999) if nc_out != 1 else {}
    eng = dg.Engine(B, IMG, IMG, nicg, nc_out=nc_out, bf16_mfma=(mode != "float32"), **kw)
    for n, Pm in weights.items():
        eng.set_weights(n, Pm)
    if mode == "fwd_only":
        eng.forward_only_storage = "bfloat16"
    elif mode == "g_update":
        eng.forward_only_storage = "bfloat16"
        eng.g_update_storage = "bfloat16"
    elif mode == "critic16":
        eng.critic16_pipe = "bfloat16"
    torch.cuda.synchronize()
    return eng


class Walker:
    """One context and its own copy of the operands (live: what the entries are handed; staged: the real values)."""

    def __init__(self, eng, ops, nc_out):
        self.eng, self.lib, self.h, self.nc_out = eng, eng.lib, eng.h, nc_out
        self.staged = {k: torch.from_numpy(v).to(sg.DEV) for k, v in ops.items()}
        self.live = {k: v.clone() for k, v in self.staged.items()}
        self.out_g = torch.empty(B, IMG, IMG, nc_out, device=sg.DEV)
        self.out_d = torch.empty(B, device=sg.DEV)
        torch.cuda.synchronize()

    # -- operand handling -------------------------------------------------------------------------------------------
    def poison(self):
        for t in self.live.values():
            t.fill_(float("nan") if t.is_floating_point() else 0)

    def load(self):
        for k, t in self.live.items():
            t.copy_(self.staged[k], non_blocking=True)

    def prefill_outputs(self):
        self.out_g.fill_(float(SENT))
        self.out_d.fill_(float(SENT))

    def arenas(self, net):
        from dep_gan_im_amd import _lib
        return [self.eng.get_arena(net, a).view(np.uint32) for a in
                (_lib.ARENA_PARAMS, _lib.ARENA_NONTRAINABLE, _lib.ARENA_GRADS, _lib.ARENA_ADAM_M, _lib.ARENA_ADAM_V)]

    def last_sums(self):
        s = (C.c_float * 8)()
        assert self.lib.depgan_last_sums(self.h, s) == 0
        return np.array(s[:], np.float32).view(np.uint32)

    # -- the entries: each returns (status, host values as uint32 bits, device outputs read after the walk's sync) ------
    def step(self, name):
        L, h, v = self.lib, self.h, self.live
        from dep_gan_im_amd import _lib
        nid = {"y2": _lib.NET_D_Y2, "dem": _lib.NET_D_DEM}
        host, dev = None, []
        if name in ("g_forward", "g_forward_bf16s"):
            rc = getattr(L, "depgan_" + name)(h, P(v["x"]), P(v["z"]), P(self.out_g), B)
            dev = [self.out_g]
        elif name.startswith("d_forward_"):
            rc = L.depgan_d_forward(h, nid[name.rsplit("_", 1)[1]], P(v["y2"]), P(self.out_d), B)
            dev = [self.out_d]
        elif name.startswith(("critic_grads_", "critic_step_")):
            host = (C.c_float * 2)()
            entry, which = name.rsplit("_", 1)
            rc = getattr(L, "depgan_" + entry)(h, nid[which], P(v["y2"]), P(v["x"]), P(v["z"]), P(v["ep"]), host)
        elif name.startswith("apply_adam_"):
            rc = L.depgan_apply_adam(h, nid[name.rsplit("_", 1)[1]])
        elif name in ("g_eval", "g_grads", "g_step"):
            host = (C.c_float * 6)()
            rc = getattr(L, "depgan_" + name)(h, P(v["x"]), P(v["y2"]), P(v["z"]), host)
        elif name == "g_eval_multi":
            host, sums = (C.c_float * (6 * K))(), (C.c_float * (8 * K))()
            rc = L.depgan_g_eval_multi(h, P(v["x"]), P(v["y2"]), P(v["zs"]), K, host, sums)
            host = list(host) + list(sums)
        elif name == "gen_iteration":
            host, best = (C.c_float * (2 + 2 + 6 * K + 6))(), C.c_int(-1)
            rc = L.depgan_gen_iteration(h, P(v["x"]), P(v["y2"]), P(v["z"]), P(v["ep"]), 1, P(v["x"]), P(v["y2"]),
                                        P(v["z"]), P(v["ep"]), 1, B, P(v["x"]), P(v["y2"]), P(v["zs"]), K, host,
                                        C.byref(best))
            host = list(host) + [float(best.value)]
        else:
            kind, sparse = name[len("uresnet_"):].split("-")
            lab = v["codes"] if sparse == "sparse" else v["onehot"]
            host = C.c_float()
            fn = getattr(L, "depgan_uresnet_" + kind + ("_sparse" if sparse == "sparse" else ""))
            if kind == "eval":
                rc = fn(h, P(v["x"]), P(v["z"]), P(lab), B, C.byref(host))
            else:
                rc = fn(h, P(v["x"]), P(v["z"]), P(lab), B, C.c_uint(7), C.byref(host))
            host = [host.value]
        bits = np.zeros(0, np.uint32) if host is None else np.array(list(host), np.float32).view(np.uint32)
        return rc, bits, dev


# name -> (the entry synchronises the stream, the networks whose arenas it writes)
GAN_STEPS = [("g_forward", False, ()), ("d_forward_y2", False, ()), ("d_forward_dem", False, ()),
             ("critic_grads_y2", True, ("D_y2",)), ("apply_adam_y2", False, ("D_y2",)), ("critic_step_dem", True, ("D_dem",)),
             ("g_eval", True, ()), ("g_grads", True, ("G",)), ("g_step", True, ("G",)), ("g_eval_multi", True, ()),
             ("gen_iteration", True, NETS)]
URESNET_STEPS = [("uresnet_%s-%s" % (k, s), True, ("G",)) for s in ("onehot", "sparse") for k in ("grads", "step", "eval")]


def _walk_null(w, steps):
    """the walk on the null stream: [(status, host bits, device outputs, last_sums, arenas)], host seconds per call"""
    res, secs = [], []
    for name, sync, writes in steps:
        w.prefill_outputs()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc, bits, dev = w.step(name)
        secs.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        res.append(_collect(w, rc, bits, dev, sync, writes))
    return res, secs


def _collect(w, rc, bits, dev, sync, writes):
    assert rc == 0, (rc, w.lib.depgan_last_error())
    return (rc, bits, [t.cpu().numpy().view(np.uint32) for t in dev], w.last_sums() if sync else None,
            {n: w.arenas(n) for n in writes})


def _same(got, want, what):
    assert got[0] == want[0], "%s: status %d, %d on the null stream" % (what, got[0], want[0])
    assert np.array_equal(got[1], want[1]), "%s: host values differ: %s vs %s" % (what, got[1].view(np.float32), want[1].view(np.float32))
    for g, x in zip(got[2], want[2]):
        assert np.array_equal(g, x), "%s: %d words of the device output differ" % (what, int((g != x).sum()))
    assert (got[3] is None) == (want[3] is None) and (got[3] is None or np.array_equal(got[3], want[3])), what + ": last_sums"
    for n in want[4]:
        for i, (g, x) in enumerate(zip(got[4][n], want[4][n])):
            assert np.array_equal(g, x), "%s: arena %d of %s differs in %d words" % (what, i, n, int((g != x).sum()))


def _hip_async():
    from dep_gan_im_amd import _lib
    hip = _lib.hip()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return hip


def _walk_gated(w, steps, want, gate, s):
    from dep_gan_im_amd import _lib
    assert w.lib.depgan_set_stream(w.h, C.c_void_p(s.cuda_stream)) == 0
    for (name, sync, writes), exp in zip(steps, want):
        w.prefill_outputs()
        w.poison()
        grad = None
        if name.startswith("apply_adam_"):
            # the operand of depgan_apply_adam is the gradient arena: poison it, restore it behind the gate
            ptr, n = w.eng.arena(writes[0], _lib.ARENA_GRADS)
            grad = (ptr, torch.from_numpy(w.eng.get_arena(writes[0], _lib.ARENA_GRADS)).to(sg.DEV))
            nan = torch.full((n,), float("nan"), device=sg.DEV)
            torch.cuda.synchronize()
            _lib.memcpy(ptr, nan.data_ptr(), 4 * n, _lib.D2D)

        def load():
            w.load()
            if grad is not None:
                assert _hip_async().hipMemcpyAsync(C.c_void_p(grad[0]), P(grad[1]), 4 * grad[1].numel(), _lib.D2D,
                                                   C.c_void_p(s.cuda_stream)) == 0
        rc, bits, dev = gate.run(s, load, lambda: w.step(name), sync, name)
        _same(_collect(w, rc, bits, dev, sync, writes), exp, name + " on the side stream")


def _three_walks(mode, nicg, nc_out, steps, delay, side):
    weights, ops = _weights(nicg, nc_out), _operands(nicg, nc_out)
    engines = [_engine(mode, nicg, nc_out, weights) for _ in range(3)]
    try:
        warm, a, b = (Walker(e, ops, nc_out) for e in engines)
        _walk_null(warm, steps)
        want, secs = _walk_null(a, steps)
        ms = sg.gate_ms(max(secs))
        print("stream ctx %s: host-side call durations (ms) %s -> gate %.1f ms" %
              (mode, ", ".join("%s %.2f" % (st[0], 1e3 * t) for st, t in zip(steps, secs)), ms))
        _walk_gated(b, steps, want, sg.Gate(delay, ms), side)
    finally:
        torch.cuda.synchronize()
        for e in engines:
            e.close()


@pytest.mark.parametrize("mode", ["float32", "fwd_only", "g_update", "critic16"])
def test_every_closure_of_a_context_on_a_side_stream(lib, delay, side, mode):
    steps = list(GAN_STEPS)
    if mode != "float32":
        steps.insert(3, ("g_forward_bf16s", False, ()))
    _three_walks(mode, 1 if mode == "float32" else 2, 1, steps, delay, side)


def test_every_supervised_entry_of_a_context_on_a_side_stream(lib, delay, side):
    _three_walks("float32", 1, 4, URESNET_STEPS, delay, side)


def test_a_stream_switch_equals_four_calls_on_the_null_stream(lib, side):
    """null stream, then s, then a second side stream, then the null stream again, the device synchronised between the
    switches (ordering across a switch is the caller's job: include/depgan.h)."""
    weights, ops = _weights(1, 1), _operands(1, 1)
    engines = [_engine("float32", 1, 1, weights) for _ in range(2)]
    second = torch.cuda.Stream()
    try:
        a, b = (Walker(e, ops, 1) for e in engines)
        steps = [("g_step", True, ("G",)), ("critic_step_y2", True, ("D_y2",)), ("g_step", True, ("G",)),
                 ("critic_step_dem", True, ("D_dem",))]
        want, _ = _walk_null(a, steps)
        for (name, sync, writes), exp, handle in zip(steps, want, (0, side.cuda_stream, second.cuda_stream, 0)):
            assert b.lib.depgan_set_stream(b.h, C.c_void_p(handle)) == 0
            b.prefill_outputs()
            torch.cuda.synchronize()
            rc, bits, dev = b.step(name)
            torch.cuda.synchronize()
            _same(_collect(b, rc, bits, dev, sync, writes), exp, "%s after the switch to stream %#x" % (name, handle))
    finally:
        torch.cuda.synchronize()
        for e in engines:
            e.close()
        del second


def test_the_engine_follows_torchs_current_stream(lib, delay, side):
    """Engine methods under `with torch.cuda.stream(s)`: the engine re-reads torch's current stream before every call.
    depgan_set_stream has no getter, so the result bits are the check: gated operands, as above."""
    weights, ops = _weights(1, 1), _operands(1, 1)
    engines = [_engine("float32", 1, 1, weights) for _ in range(3)]
    try:
        warm, a, b = (Walker(e, ops, 1) for e in engines)

        def calls(w):
            v, e = w.live, w.eng
            return [("g_forward", False, lambda: e.g_forward(v["x"], v["z"])),
                    ("critic", True, lambda: e.critic("D_y2", v["y2"], v["x"], v["z"], v["ep"])),
                    ("generator", True, lambda: e.generator(v["x"], v["y2"], v["z"], "step"))]

        def bits(r):          # after the stream has been synchronised
            r = r.cpu().numpy() if isinstance(r, torch.Tensor) else np.array(r, np.float32)
            return r.view(np.uint32)
        for _, _, f in calls(warm):
            f()
        want, secs = [], []
        for _, _, f in calls(a):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = f()
            secs.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            want.append(bits(r))
        gate = sg.Gate(delay, sg.gate_ms(max(secs)))
        for (name, sync, f), exp in zip(calls(b), want):
            b.poison()

            def call():
                with torch.cuda.stream(side):
                    return f()
            got = gate.run(side, b.load, call, sync, "Engine." + name)
            assert np.array_equal(bits(got), exp), "Engine.%s under torch.cuda.stream(s) differs from the null stream" % name
        torch.cuda.synchronize()
        for n in NETS:
            for g, x in zip(b.arenas(n), a.arenas(n)):
                assert np.array_equal(g, x), n
    finally:
        torch.cuda.synchronize()
        for e in engines:
            e.close()
