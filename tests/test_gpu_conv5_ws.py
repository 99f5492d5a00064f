"""GPU, operator level: the weight-stationary, wave-private 5x5 kernel (csrc/igemm_wp.hip, igemm_ws5_kernel; operator
path 9) against the workgroup-tile kernel igemm_conv_kernel<., 5, ., 25> (path 1).

The kernel reads the tile kernel's packed panel, walks K in its order (chunk -> tap -> four MFMAs) at the plan's chunk
width for all four channel pairs (16 channels for Cout = 16, 8 for Cout = 32) and runs the same epilogue text, so every
comparison with path 1 here is np.array_equal -- no pair needed the tolerance form.

Method, windows and sentinels are those of tests/test_gpu_fused_ops.py (imported, not copied): every operand is a strided
window of a wider buffer, NaN around what is read, sentinels around what is written.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_ref as fr  # noqa: E402
import test_gpu_fused_ops as tfo  # noqa: E402
from test_gpu_fused_ops import FEATS, NONE, SENT, Flat, P, Win, bits, dev  # noqa: E402

pytestmark = pytest.mark.gpu

PAIRS = [(16, 16), (16, 32), (32, 16), (32, 32)]
SIZES = [(1, 4, 16),     # exactly one wave block
         (3, 6, 20),     # a partial second block in both directions
         (2, 18, 70),    # crosses the 16-row band and the 64-column borders; even sizes: the pool variant runs
         (1, 2, 2)]      # image smaller than the halo
FSETS = ["bias", "affine_relu", "film", "pool", "join", "acc", "negpool"]
assert all(f in tfo.ACCEPTS[1] for f in FSETS)


def make(kind, seed, shape, feat, bwd):
    B, H, W, ci, co = shape
    f = dict(FEATS[feat])
    pre, pool = f.pop("pre", 0), f.pop("pool", 0)
    f["bwd"] = 1 if (bwd or f.get("bwd")) else 0
    rng = np.random.default_rng(seed)
    o = fr.make_ops(kind, rng, B, H, W, ci, co, 5, **f)
    if kind == "real":
        o.w = (rng.standard_normal((5, 5, ci, co)) * 0.05).astype(np.float32)
    return o, pre, pool


def launch(lib, path, o, shape, pre, pool):
    """One depgan_op_conv2d_fused call on fresh windows of wider buffers.  Returns (status, windows)."""
    B, H, W, ci, co = shape
    cin, cout = (co, ci) if o.bwd else (ci, co)
    nan = np.float32("nan")
    w = {"in": Win((B, H, W, cin), 12, 4, nan, o.x), "out": Win((B, H, W, cout), 20, 8, SENT, o.old)}
    if pre:
        w["pre"] = Win((B, H, W, cout), 28, 12, SENT)
    if o.res is not None:
        w["res"] = Win((B, H, W, cout), 36, 16, nan, o.res)
    if o.mask is not None:
        w["mask"] = Win((B, H, W, cout), 44, 20, nan, o.mask)
    if pool:
        w["pool"] = Win((B, H // 2, W // 2, cout), 52, 24, SENT)
    d = {n: dev(getattr(o, n)) for n in ("w", "bias", "scale", "shift")}
    ld = cout + 12
    for n in ("fmul", "fadd"):
        a = getattr(o, n)
        if a is not None:
            full = np.full((B, ld), nan, np.float32)
            full[:, :cout] = a
            a = full
        d[n] = dev(a)
    arg = lambda n: w[n].args() if n in w else NONE   # noqa: E731
    rc = lib.depgan_op_conv2d_fused(
        *w["in"].args(), P(d["w"]), P(d["bias"]), P(d["scale"]), P(d["shift"]), P(d["fmul"]), P(d["fadd"]), ld,
        *w["out"].args(), *arg("pre"), *arg("res"), *arg("mask"), *arg("pool"), None, None, None, 0, 0,
        B, H, W, ci, co, 5, o.relu, int(o.old is not None), path, o.bwd, None)
    torch.cuda.synchronize()
    return rc, w


_id3 = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)   # noqa: E731


@pytest.mark.parametrize("bwd", [0, 1])
@pytest.mark.parametrize("size", SIZES, ids=_id3)
@pytest.mark.parametrize("pair", PAIRS, ids=_id3)
def test_bit_identical_to_the_tile_kernel_on_real_operands(lib, pair, size, bwd):
    from dep_gan_im_amd import _lib
    shape = size + pair
    for feat in FSETS:
        o, _, pool = make("real", sum(shape) * 131 + len(feat) + bwd, shape, feat, bwd)
        got = {}
        for path in (1, 9):
            rc, w = launch(lib, path, o, shape, True, pool)      # out_pre requested throughout
            _lib.check(rc, "op_conv2d_fused path %d %s" % (path, feat))
            got[path] = {n: w[n].read() for n in ("out", "pre") + (("pool",) if pool else ())}
            for n in got[path]:
                assert w[n].outside_unchanged(), (feat, path, n)
            for n in ("in", "res", "mask"):
                assert n not in w or w[n].unchanged(), (feat, path, n)
        for n in got[1]:
            assert np.isfinite(got[1][n]).all(), (feat, n)
            assert np.array_equal(bits(got[9][n]), bits(got[1][n])), "%s %s: %d values differ" % (
                feat, n, (bits(got[9][n]) != bits(got[1][n])).sum())


@pytest.mark.parametrize("feat", FSETS)
@pytest.mark.parametrize("pair", PAIRS, ids=_id3)
def test_exact_operands_give_the_one_correct_bit_pattern(lib, pair, feat):
    from dep_gan_im_amd import _lib
    shape = (3, 6, 20) + pair
    o, pre, pool = make("exact", sum(shape) * 17 + len(feat), shape, feat, 0)
    rc, w = launch(lib, 9, o, shape, pre, pool)
    _lib.check(rc, "op_conv2d_fused")
    ref = fr.reference(o)
    assert fr.bounds_hold(ref["stages"])
    got = w["out"].read()
    assert np.array_equal(got, ref["out"]), "out: %d wrong, first at %s" % (
        (got != ref["out"]).sum(), np.argwhere(got != ref["out"])[:1].tolist())
    assert w["out"].outside_unchanged()
    if pre:
        assert np.array_equal(w["pre"].read(), ref["out_pre"]) and w["pre"].outside_unchanged()
    if pool:
        assert np.array_equal(w["pool"].read(), ref["pool"]) and w["pool"].outside_unchanged()
        if "neg" in FEATS[feat]:
            assert ref["pool"].max() < 0
    for n in ("in", "res", "mask"):
        assert n not in w or w[n].unchanged()


def _dense_pool_launch(lib, path, x, wt, bias, B, H, W, ci, co):
    out = torch.full((B, H, W, co), float(SENT), device="cuda:0")
    pool = torch.full((B, H // 2, W // 2, co), float(SENT), device="cuda:0")
    v = lambda t, h, w, c: (C.c_void_p(t.data_ptr()), h * w * c, w * c, c)   # noqa: E731
    rc = lib.depgan_op_conv2d_fused(
        *v(x, H, W, ci), P(wt), P(bias), None, None, None, None, 0, *v(out, H, W, co), *NONE, *NONE, *NONE,
        *v(pool, H // 2, W // 2, co), None, None, None, 0, 0, B, H, W, ci, co, 5, 1, 0, path, 0, None)
    torch.cuda.synchronize()
    return rc, out, pool


def _persistent_case(lib, pair, B, H, W):
    from dep_gan_im_amd import _lib
    ci, co = pair
    g = torch.Generator(device="cuda:0").manual_seed(ci * 64 + co + W)
    x = torch.randn((B, H, W, ci), device="cuda:0", generator=g)
    wt = torch.randn((5, 5, ci, co), device="cuda:0", generator=g) * 0.05
    bias = torch.randn((co,), device="cuda:0", generator=g)
    res = {}
    for path in (1, 9):
        rc, out, pool = _dense_pool_launch(lib, path, x, wt, bias, B, H, W, ci, co)
        _lib.check(rc, "op_conv2d_fused path %d" % path)
        res[path] = (out, pool)
    for a, b in zip(res[1], res[9]):
        assert bool(torch.isfinite(a).all()) and float(a.max()) > 0 and float(a.max()) < 1e6    # no sentinel left
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("pair", PAIRS, ids=_id3)
def test_persistent_workgroups_every_wave_takes_several_items(lib, pair):
    """Bias + ReLU + pool at a size with more than twice as many wave items as the chip has wave slots (16 per CU at the
    most), bit for bit against path 1 on the GPU."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    H, W = (256, 256) if pair == (16, 16) else (128, 128)
    per = (H // 4) * (W // 16)
    B = (2 * 16 * cus) // per + 1
    assert B * per > 2 * 16 * cus
    _persistent_case(lib, pair, B, H, W)


@pytest.mark.parametrize("pair", [(16, 16), (32, 16)], ids=_id3)
def test_persistent_group_count_that_is_no_multiple_of_eight(lib, pair):
    """5 x 256 x 208: 4160 wave items -- 347 groups of 12 waves, 379 of 11: more than one per CU, odd (the plain
    group numbering instead of the one dealt over the XCDs)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, H, W = 5, 256, 208
    items = B * (H // 4) * (W // 16)
    for nw in (11, 12):
        assert (-(-items // nw)) % 8 != 0
    assert items // 12 > min(cus, 256)
    _persistent_case(lib, pair, B, H, W)


def test_plain_operator_entries_take_path_9(lib):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = 2, 18, 70, 16, 32
    rng = np.random.default_rng(7)
    x = dev(rng.standard_normal((B, H, W, ci)))
    dy = dev(rng.standard_normal((B, H, W, co)))
    wt = dev(rng.standard_normal((5, 5, ci, co)) * 0.05)
    bias = dev(rng.standard_normal(co))
    out, dx = {}, {}
    for path in (1, 9):
        out[path] = torch.empty((B, H, W, co), device="cuda:0")
        dx[path] = torch.empty((B, H, W, ci), device="cuda:0")
        _lib.check(lib.depgan_op_conv2d(P(x), P(wt), P(bias), P(out[path]), B, H, W, ci, co, 5, 1, path, None))
        _lib.check(lib.depgan_op_conv2d_bwd_data(P(dy), P(wt), P(dx[path]), B, H, W, ci, co, 5, path, None))
    torch.cuda.synchronize()
    assert torch.equal(out[1].view(torch.int32), out[9].view(torch.int32))
    assert torch.equal(dx[1].view(torch.int32), dx[9].view(torch.int32))
    # path 9 with another kernel size is a bad argument (status 1, tests/test_fused_ref_cpu.py); nothing written
    o3 = Flat(B * H * W * co)
    assert lib.depgan_op_conv2d(P(x), P(wt), P(bias), o3.ptr(), B, H, W, ci, co, 3, 1, 9, None) == 1
    torch.cuda.synchronize()
    assert o3.unchanged()


REFUSED = [("bias", (2, 6, 20, 16, 16, 3)),      # KS = 3
           ("bias", (2, 6, 20, 64, 32, 5)),      # Cin = 64
           ("head", (2, 6, 20, 32, 32, 5)),      # the fused head
           ("pool", (2, 7, 20, 16, 16, 5))]      # odd H under a pool request


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: "%s-%s" % (c[0], _id3(c[1])))
def test_refusals_return_a_status_and_write_nothing(lib, case):
    feat, shape = case
    rc, o, w, _ = tfo.run_fused(lib, 9, feat, shape, "exact")
    assert rc != 0 and lib.depgan_last_error()
    for win in w.values():
        assert win.unchanged()
