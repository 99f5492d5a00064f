"""GPU, operator level: the epilogue classes of the 5x5 kernels -- igemm_ws5_kernel<32,8> / <16,16> (operator path 9)
and the workgroup-tile kernels igemm_conv_kernel<32,5,8,25,.> / <16,5,16,25,.> (path 1; the persistent form, which
holds the class bodies, from 513 pixel tiles up) -- through depgan_op_conv2d_fused.

A class is an item loop inside the one kernel whose epilogue flags are compile-time constants; the same statements as
the run-time-flag body, so there is no tolerance anywhere:
  real operands    the same call with the switch on and with it off (every launch then takes the run-time-flag body):
                   every written buffer bitwise equal, its sentinel frame included; what is only read unchanged.
  exact operands   small integers, switch on, against a float64 evaluation of the contract: equal.

Feature sets: the four flag sets model.hip launches on these kernels, the mask set in both of its roles.
Shapes (B, H, W), the smallest that can still go wrong:
  2 x 8 x 16     one pixel tile, every wave block on the border (the pool sets also 2 x 4 x 16: one wave block)
  3 x 20 x 36    partial blocks right and bottom
  2 x 64 x 64    several wave items per wave of the weight-stationary kernel (32 wave blocks per sample, 12 ... 16 waves)
  BIG            256 x 256 at a batch of two wave items per wave slot of the chip and more (16 waves per CU at the most):
                 the weight-stationary kernel walks several groups per workgroup, and with over 512 pixel tiles path 1
                 takes the persistent tile kernel.  Dense tensors, compared on the device; float64 on the device too
                 (25 shifted matrix products), once per (pair, direction), shared by the feature sets.
Channel pairs of the launch: 16 -> 16, 16 -> 32, 32 -> 16, 32 -> 32; the big launch for one pair per kernel: Cout 16, 32.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_ref as fr  # noqa: E402
import test_gpu_fused_ops as fo  # noqa: E402  (Win, dev, P, bits, SENT, NONE: the windows and frames of that file)

pytestmark = pytest.mark.gpu

# name: (class id, make_ops keywords + pool)
FEATS = {
    "critic": (1, dict(bias=1, relu=1)),
    "critic_pool": (2, dict(bias=1, relu=1, pool=1)),
    "u_fwd_mask": (3, dict(mask=1)),                    # the critics' u-forward: forward weights
    "bwd_mask": (3, dict(mask=1, bwd=1)),
    "bwd_plain": (4, dict(bwd=1)),
}
PAIRS = [(16, 16), (16, 32), (32, 16), (32, 32)]        # channels of the LAUNCH (cin, cout)
SMALL = [(2, 8, 16), (3, 20, 36), (2, 64, 64)]
POOL_ONLY = (2, 4, 16)
BIG_PAIRS = [(16, 16), (16, 32)]
PATHS = (1, 9)
CASES = [(p, f, pair, s) for p in PATHS for f in FEATS for pair in PAIRS
         for s in SMALL + ([POOL_ONLY] if "pool" in f else [])]
BIG_CASES = [(p, f, pair) for p in PATHS for f in FEATS for pair in BIG_PAIRS]
_id = lambda c: "p%d-%s-%dto%d" % (c[0], c[1], c[2][0], c[2][1]) + ("-" + "x".join(map(str, c[3])) if len(c) > 3 else "")   # noqa: E731


def flags_of(feat):
    from dep_gan_im_amd import _lib
    names = {"bias": "BIAS", "relu": "RELU", "mask": "MASK", "pool": "POOL"}
    return sum(_lib._K["DEPGAN_EPF_" + names[k]] for k, v in FEATS[feat][1].items() if v and k in names)


@pytest.fixture()
def switch(lib):
    before = lib.depgan_get_epilogue_classes()
    yield lib
    assert lib.depgan_set_epilogue_classes(before) == 0


def set_switch(lib, on, feat):
    assert lib.depgan_set_epilogue_classes(on) == 0
    assert lib.depgan_conv5_epilogue_class(flags_of(feat)) == (FEATS[feat][0] if on else 0)


def run(lib, path, feat, pair, size, kind):
    """One depgan_op_conv2d_fused call, every operand a window of a wider buffer.  Returns (ops, windows, pool)."""
    from dep_gan_im_amd import _lib
    B, H, W = size
    cin, cout = pair
    f = dict(FEATS[feat][1])
    pool = f.pop("pool", 0)
    ci, co = (cout, cin) if f.get("bwd") else (cin, cout)          # the layer's: backward-data runs co -> ci
    rng = np.random.default_rng(sum(size) * 131 + cin * 7 + cout * 3 + sum(map(ord, feat)))
    o = fr.make_ops(kind, rng, B, H, W, ci, co, 5, **f)
    nan = np.float32("nan")
    w = {"in": fo.Win((B, H, W, cin), 12, 4, nan, o.x), "out": fo.Win((B, H, W, cout), 20, 8, fo.SENT)}
    if o.mask is not None:
        w["mask"] = fo.Win((B, H, W, cout), 44, 20, nan, o.mask)
    if pool:
        w["pool"] = fo.Win((B, H // 2, W // 2, cout), 52, 24, fo.SENT)
    d = {n: fo.dev(getattr(o, n)) for n in ("w", "bias")}
    arg = lambda n: w[n].args() if n in w else fo.NONE   # noqa: E731
    P = fo.P
    rc = lib.depgan_op_conv2d_fused(
        *w["in"].args(), P(d["w"]), P(d["bias"]), None, None, None, None, 0, *w["out"].args(), *fo.NONE, *fo.NONE,
        *arg("mask"), *arg("pool"), None, None, None, 0, 0, B, H, W, ci, co, 5, o.relu, 0, path, o.bwd, None)
    torch.cuda.synchronize()
    _lib.check(rc, "op_conv2d_fused path %d" % path)
    return o, w, pool


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_class_real_operands_equal_the_run_time_body_bit_for_bit(switch, case):
    lib = switch
    path, feat, pair, size = case
    got = {}
    for on in (1, 0):
        set_switch(lib, on, feat)
        _, w, _ = run(lib, path, feat, pair, size, "real")
        got[on] = {n: (fo.bits(win.t.cpu().numpy()), fo.bits(win.full0)) for n, win in w.items()}
    assert set(got[1]) == set(got[0]) and "out" in got[1]
    for n in got[1]:
        now1, before1 = got[1][n]
        now0, before0 = got[0][n]
        assert np.array_equal(before1, before0), n                      # the two runs started from the same buffers
        assert np.array_equal(now1, now0), "%s: class and run-time body differ in %d words" % (n, (now1 != now0).sum())
        if n in ("in", "mask"):
            assert np.array_equal(now1, before1), n                     # read-only operands
    assert not np.array_equal(got[1]["out"][0], got[1]["out"][1])       # something was written


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_class_exact_operands_equal_float64(switch, case):
    lib = switch
    path, feat, pair, size = case
    set_switch(lib, 1, feat)
    o, w, pool = run(lib, path, feat, pair, size, "exact")
    ref = fr.reference(o)                               # float64: the one correct bit pattern (test_fused_ref_cpu.py)
    assert fr.bounds_hold(ref["stages"])
    got = w["out"].read()
    assert np.array_equal(got, ref["out"]), "out: %d wrong, first at %s" % (
        (got != ref["out"]).sum(), np.argwhere(got != ref["out"])[:1].tolist())
    assert w["out"].outside_unchanged()
    if pool:
        got = w["pool"].read()
        assert np.array_equal(got, ref["pool"]), "pool: first wrong at %s" % np.argwhere(got != ref["pool"])[:1].tolist()
        assert w["pool"].outside_unchanged()
    for n in ("in", "mask"):
        assert n not in w or w[n].unchanged()


# ---- the big launch: dense device tensors, small-integer operands (every fp32 operation on the way is exact) ----
FRAME = 64      # sentinel floats in front of and behind every written tensor


def big_size():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per = (256 // 4) * (256 // 16)
    B = -(-2 * 16 * cus // per)
    assert B * per >= 2 * 16 * cus and B * 256 > 2 * cus        # two items per wave slot; more pixel tiles than 2 per CU
    return B, 256, 256


@functools.lru_cache(maxsize=None)
def big_operands(pair, bwd):
    """x, w (the layer's HWIO), bias, mask and the float64 contraction, once per (pair, direction); never written to"""
    B, H, W = big_size()
    cin, cout = pair
    ci, co = (cout, cin) if bwd else (cin, cout)
    g = torch.Generator(device="cuda:0").manual_seed(1000 * cin + 10 * cout + bwd)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, device="cuda:0", generator=g).float()   # noqa: E731
    x, wt = ri(-2, 2, (B, H, W, cin)), ri(-1, 1, (5, 5, ci, co))
    bias = ri(-16, 16, (cout,)) / 8
    mask = ri(-1, 2, (B, H, W, cout)) / 2                      # a quarter each: negative, zero, two positive values
    xd = torch.nn.functional.pad(x.double(), (0, 0, 2, 2, 2, 2))
    acc = torch.zeros((B, H, W, cout), dtype=torch.float64, device="cuda:0")
    for ty in range(5):
        for tx in range(5):
            if bwd:         # dx[q] = sum_t dy[q - (t - 2)] w[t]^T
                acc += xd[:, 4 - ty:4 - ty + H, 4 - tx:4 - tx + W, :] @ wt[ty, tx].double().t()
            else:           # y[p] = sum_t x[p + t - 2] w[t]
                acc += xd[:, ty:ty + H, tx:tx + W, :] @ wt[ty, tx].double()
    assert float(acc.abs().max()) < 2 ** 20                    # far inside fp32's exact integers, in eighths as well
    return x, wt, bias, mask, acc


def framed(n):
    t = torch.full((n + 2 * FRAME,), float(fo.SENT), device="cuda:0")
    return t, t[FRAME:FRAME + n]


def big_launch(lib, path, feat, pair):
    from dep_gan_im_amd import _lib
    import ctypes as C
    B, H, W = big_size()
    cin, cout = pair
    f = FEATS[feat][1]
    bwd = int(bool(f.get("bwd")))
    ci, co = (cout, cin) if bwd else (cin, cout)
    x, wt, bias, mask, _ = big_operands(pair, bwd)
    out_full, out = framed(B * H * W * cout)
    pool_full, pool = framed(B * (H // 2) * (W // 2) * cout) if f.get("pool") else (None, None)
    v = lambda t, h, w, c: (C.c_void_p(t.data_ptr()), h * w * c, w * c, c)   # noqa: E731
    rc = lib.depgan_op_conv2d_fused(
        *v(x, H, W, cin), fo.P(wt), fo.P(bias) if f.get("bias") else None, None, None, None, None, 0, *v(out, H, W, cout),
        *fo.NONE, *fo.NONE, *(v(mask, H, W, cout) if f.get("mask") else fo.NONE),
        *(v(pool, H // 2, W // 2, cout) if pool is not None else fo.NONE), None, None, None, 0, 0, B, H, W, ci, co, 5,
        int(bool(f.get("relu"))), 0, path, bwd, None)
    torch.cuda.synchronize()
    _lib.check(rc, "op_conv2d_fused path %d" % path)
    return out_full, pool_full


@pytest.mark.parametrize("case", BIG_CASES, ids=_id)
def test_big_launch_classes_equal_the_run_time_body_and_float64(switch, case):
    lib = switch
    path, feat, pair = case
    B, H, W = big_size()
    cout = pair[1]
    f = FEATS[feat][1]
    bwd = int(bool(f.get("bwd")))
    x, wt, bias, mask, acc = big_operands(pair, bwd)
    before = [t.clone() for t in (x, wt, bias, mask)]
    got = {}
    for on in (1, 0):
        set_switch(lib, on, feat)
        got[on] = big_launch(lib, path, feat, pair)
    for a, b in zip(got[1], got[0]):
        assert (a is None) == (b is None)
        if a is not None:                                   # frames included
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            for t in (a[:FRAME], a[-FRAME:]):
                assert bool((t == float(fo.SENT)).all())
    for t, t0 in zip((x, wt, bias, mask), before):
        assert torch.equal(t, t0)
    # float64: the contract on exact operands
    v = acc + bias.double() if f.get("bias") else acc.clone()
    if f.get("relu"):
        v = v.clamp_min(0)
    if f.get("mask"):
        v = torch.where(mask > 0, v, torch.zeros_like(v))
    out = got[1][0][FRAME:-FRAME].view(B, H, W, cout)
    assert torch.equal(out.double(), v), "out: %d wrong" % int((out.double() != v).sum())
    if f.get("pool"):
        want = v.view(B, H // 2, 2, W // 2, 2, cout).amax(dim=(2, 4))
        assert torch.equal(got[1][1][FRAME:-FRAME].view(B, H // 2, W // 2, cout).double(), want)
