"""GPU, operator level: the epilogue classes of the Winograd 3x3 kernel (csrc/igemm_wino.hip, igemm_epilogue.inc
EPI_CLASS) -- instantiations whose epilogue flags are compile-time constants, one per flag set the model launches --
through depgan_op_conv2d_fused on path 8.

Method of tests/test_gpu_fused_ops.py (its windows, frames and operands; tests/fused_ref.py for the references):
  exact operands   each class, switch on, against the float64 evaluation of the contract: np.array_equal.
  real operands    the same call with the switch on and with it off (the generic kernel): every written tensor (out,
                   out_pre, pool, head_out) bitwise equal, its sentinel frame included; every operand that is only
                   read bitwise unchanged, its NaN frame included.
No tolerance anywhere: the classes hold the generic kernel's statements, so they compute its bits.

Shapes (B, H, W, launch Cin, launch Cout), the smallest that reach each path of the per-item code:
  2 x 22 x 18   border items (EPI_FULL false: 22 = 2 x 8 + 6 rows, 18 = 16 + 2 columns)
  2 x 16 x 32   full tiles only
  Cin 8 (the item's first chunk is also its last) and 24 (three chunks: an odd count)
  Cout 32 and 64 (a second channel tile: the n0 offsets of bias / scale / FiLM rows)
  32 x 64 x 64, Cin 8: more items than resident workgroups -- the persistent instantiation of every class
  the head class: 2 x 22 x 18, Cin 16, stored and head_skip_out; 32 x 64 x 96 for its persistent instantiation
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_ref as fr  # noqa: E402
import test_gpu_fused_ops as fo  # noqa: E402  (Win, Flat, dev, P, bits, SENT, NONE: the windows and frames of that file)

pytestmark = pytest.mark.gpu

# feature sets of this file (make_ops keywords + pre, pool, head as in test_gpu_fused_ops.FEATS, which stays as it is):
# the flag sets model.hip launches on the Winograd kernel, and the class id igemm_wino.hip gives each
FEATS = {
    "g_conv": (1, dict(bias=1, affine=1, relu=1)),
    "g_conv_pool": (2, dict(bias=1, affine=1, relu=1, pool=1)),
    "film": (3, dict(bias=1, affine=1, film=1, relu=1, res=1)),
    "film_pre": (4, dict(bias=1, affine=1, film=1, relu=1, res=1, pre=1)),
    "bwd_join": (5, dict(res=1, mask=1, bwd=1)),
    "bwd_mask": (6, dict(mask=1, bwd=1)),
    "u_fwd_mask": (6, dict(mask=1)),                    # the critics' u-forward: the same flag set, forward weights
    "bwd_plain": (7, dict(bwd=1)),
    "critic": (8, dict(bias=1, relu=1)),
    "critic_pool": (9, dict(bias=1, relu=1, pool=1)),
    "head": (10, dict(bias=1, affine=1, relu=1, head=1)),
    "head_skip": (10, dict(bias=1, affine=1, relu=1, head=2)),
}
HEADS = ("head", "head_skip")
# every pair of (border / full, Cin 8 / 24, Cout 32 / 64) occurs
SMALL = [(2, 22, 18, 8, 32), (2, 22, 18, 24, 64), (2, 16, 32, 8, 64), (2, 16, 32, 24, 32)]
PERSIST = (32, 64, 64, 8, 32)
HEAD_SMALL = (2, 22, 18, 16, 32)
HEAD_PERSIST = (32, 64, 96, 8, 32)
CASES = ([(f, s) for f in FEATS if f not in HEADS for s in SMALL + [PERSIST]] +
         [(f, s) for f in HEADS for s in (HEAD_SMALL, HEAD_PERSIST)])
_id = lambda c: "%s-%s" % (c[0], "x".join(map(str, c[1])))   # noqa: E731


def flags_of(feat):
    from dep_gan_im_amd import _lib
    K = _lib._K
    f = FEATS[feat][1]
    names = {"bias": "BIAS", "affine": "AFFINE", "film": "FILM", "relu": "RELU", "pre": "PRE", "res": "RES", "mask": "MASK",
             "pool": "POOL", "acc": "ACCUM", "head": "HEAD"}
    return sum(K["DEPGAN_EPF_" + names[k]] for k, v in f.items() if v and k in names)


def persistent(feat, shape):
    """more items than resident workgroups: three per CU at 8-row tiles, two at the head kernel's 16-row tiles"""
    B, H, W, _, co = shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows, per_cu = (16, 2) if feat in HEADS else (8, 3)
    return B * (-(-H // rows)) * (-(-W // 16)) * (co // 32) > per_cu * cus


@pytest.fixture()
def switch(lib):
    before = lib.depgan_get_epilogue_classes()
    yield lib
    assert lib.depgan_set_epilogue_classes(before) == 0


def run(lib, feat, shape, kind):
    """One depgan_op_conv2d_fused call on path 8, every operand a window of a wider buffer.  Returns (ops, windows)."""
    from dep_gan_im_amd import _lib
    B, H, W, cin, cout = shape                          # channels of the LAUNCH
    f = dict(FEATS[feat][1])
    pre, pool, head = f.pop("pre", 0), f.pop("pool", 0), f.pop("head", 0)
    ci, co = (cout, cin) if f.get("bwd") else (cin, cout)          # the layer's: backward-data runs co -> ci
    rng = np.random.default_rng(sum(shape) * 131 + len(feat) * 7 + sum(map(ord, feat)))
    o = fr.make_ops(kind, rng, B, H, W, ci, co, 3, head=bool(head), head_tanh=(kind == "real"), **f)
    nan = np.float32("nan")
    w = {"in": fo.Win((B, H, W, cin), 12, 4, nan, o.x), "out": fo.Win((B, H, W, cout), 20, 8, fo.SENT, o.old)}
    if pre:
        w["pre"] = fo.Win((B, H, W, cout), 28, 12, fo.SENT)
    if o.res is not None:
        w["res"] = fo.Win((B, H, W, cout), 36, 16, nan, o.res)
    if o.mask is not None:
        w["mask"] = fo.Win((B, H, W, cout), 44, 20, nan, o.mask)
    if pool:
        w["pool"] = fo.Win((B, H // 2, W // 2, cout), 52, 24, fo.SENT)
    if head:
        w["head"] = fo.Flat(B * H * W)
    d = {n: fo.dev(getattr(o, n)) for n in ("w", "bias", "scale", "shift", "head_w", "head_b")}
    ld = cout + 12                                       # FiLM rows at their own pitch, NaN between them
    for n in ("fmul", "fadd"):
        a = getattr(o, n)
        if a is not None:
            full = np.full((B, ld), nan, np.float32)
            full[:, :cout] = a
            a = full
        d[n] = fo.dev(a)
    arg = lambda n: w[n].args() if n in w else fo.NONE   # noqa: E731
    P = fo.P
    rc = lib.depgan_op_conv2d_fused(
        *w["in"].args(), P(d["w"]), P(d["bias"]), P(d["scale"]), P(d["shift"]), P(d["fmul"]), P(d["fadd"]), ld,
        *w["out"].args(), *arg("pre"), *arg("res"), *arg("mask"), *arg("pool"), P(d["head_w"]), P(d["head_b"]),
        w["head"].ptr() if head else None, o.head_tanh, int(head == 2), B, H, W, ci, co, 3, o.relu,
        int(o.old is not None), 8, o.bwd, None)
    torch.cuda.synchronize()
    _lib.check(rc, "op_conv2d_fused")
    return o, w, (pre, pool, head)


def kernel_name(lib, feat, shape):
    from dep_gan_im_amd import _lib
    B, H, W, cin, cout = shape
    buf = C.create_string_buffer(64)
    _lib.check(lib.depgan_op_conv3x3_wino_kernel_name(flags_of(feat), B, H, W, cin, cout, buf, 64), "kernel_name")
    return buf.value.decode()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_launch_takes_its_class_and_the_generic_kernel_with_the_switch_off(switch, case):
    """The name comes from the table entry the launcher starts (igemm_wino.hip wino_pick): form, persistence, class."""
    lib = switch
    feat, shape = case
    pers = persistent(feat, shape)
    assert pers == (shape in (PERSIST, HEAD_PERSIST))
    stem = "wino_conv_head_kernel<%s," if feat in HEADS else "wino_conv_kernel<1,%s,"
    stem %= "true" if pers else "false"
    assert lib.depgan_set_epilogue_classes(1) == 0
    assert lib.depgan_wino_epilogue_class(flags_of(feat), int(feat in HEADS)) == FEATS[feat][0]
    assert kernel_name(lib, feat, shape) == stem + "%d>" % FEATS[feat][0]
    assert lib.depgan_set_epilogue_classes(0) == 0
    assert kernel_name(lib, feat, shape) == stem + "0>"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_class_exact_operands_equal_float64(switch, case):
    lib = switch
    feat, shape = case
    assert lib.depgan_set_epilogue_classes(1) == 0
    assert kernel_name(lib, feat, shape).endswith(",%d>" % FEATS[feat][0])
    o, w, (pre, pool, head) = run(lib, feat, shape, "exact")
    ref = fr.reference(o)                               # float64: the one correct bit pattern (test_fused_ref_cpu.py)
    assert fr.bounds_hold(ref["stages"])
    if head == 2:
        assert w["out"].unchanged()                     # head_skip_out: the 32-channel output is not stored
    else:
        got = w["out"].read()
        assert np.array_equal(got, ref["out"]), "out: %d wrong, first at %s" % (
            (got != ref["out"]).sum(), np.argwhere(got != ref["out"])[:1].tolist())
        assert w["out"].outside_unchanged()
    if pre:
        assert np.array_equal(w["pre"].read(), ref["out_pre"]) and w["pre"].outside_unchanged()
    if pool:
        got = w["pool"].read()
        assert np.array_equal(got, ref["pool"]), "pool: first wrong at %s" % np.argwhere(got != ref["pool"])[:1].tolist()
        assert w["pool"].outside_unchanged()
    if head:
        assert np.array_equal(w["head"].read().reshape(ref["head"].shape), ref["head"])     # identity activation
        assert w["head"].outside_unchanged()
    for n in ("in", "res", "mask"):
        if n in w:
            assert w[n].unchanged()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_class_real_operands_equal_the_generic_kernel_bit_for_bit(switch, case):
    lib = switch
    feat, shape = case
    got = {}
    for on in (1, 0):
        assert lib.depgan_set_epilogue_classes(on) == 0
        assert kernel_name(lib, feat, shape).endswith(",%d>" % (FEATS[feat][0] if on else 0))
        _, w, _ = run(lib, feat, shape, "real")
        got[on] = {n: (fo.bits(win.t.cpu().numpy()), fo.bits(win.full0)) for n, win in w.items()}
    assert set(got[1]) == set(got[0]) and "out" in got[1]
    for n in got[1]:
        now1, before1 = got[1][n]
        now0, before0 = got[0][n]
        assert np.array_equal(before1, before0), n                      # the two runs started from the same buffers
        assert np.array_equal(now1, now0), "%s: class and generic kernel differ in %d words" % (n, (now1 != now0).sum())
        if n in ("in", "res", "mask"):
            assert np.array_equal(now1, before1), n                     # read-only operands
    if feat != "head_skip":
        assert not np.array_equal(got[1]["out"][0], got[1]["out"][1])   # something was written
