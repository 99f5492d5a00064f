"""GPU, operator level: the weight-gradient kernels PAST ONE TILE PER WORKGROUP.

Every weight-gradient kernel hands a workgroup a contiguous range of pixel tiles (the transposed-convolution kernel: of
k-steps), prefetches the next one under the MFMAs of the current one and writes one partial slab at the end; the host
sizes the range so that a launch is one round of resident workgroups.  At the shapes of the other operator tests that
range is the minimum (one tile; one round of the fragment ring), so the loops these kernels were written for -- the
counted wait with the next tile's DMA in flight, the reuse of an LDS buffer by the third tile, the incremental
tile / row / sample advance, the sample tag that gates the column sums, a border tile staged after an interior one, a
shorter last chunk, a refilled ring stage that is multiplied -- ran only inside the full-size model tests, whose
tolerances absorb one stale 16-byte piece in one of hundreds of tiles.

The cases are the rows of tests/wgrad_plan_cases.py; each names the plan properties it is there for, and every test
reads the plan from depgan_debug_wgrad_plan (the launchers' own chunking functions) on the device and asserts them, so a
later change of the chunking fails here instead of quietly emptying the file.  tests/test_wgrad_plan_cpu.py proves on
the CPU that these operands see the faults in question.

Method, as tests/test_gpu_fused_ops.py::test_wgrad_extras: every read-only operand is a window of a wider NaN-filled
buffer, every written buffer lies between sentinels that must stay bitwise unchanged, every call is made twice and the
two results must have the same bits.
  exact operands   small integers (bf16-representable), every partial sum below 2^24 (asserted): dw, raw, colraw and
                   colout are the integers of the float64 contraction -> np.array_equal.
  real operands    fp32 kernels against float64 at TOL; the bf16 kernel against float64 of the rounded operands at TOL;
                   the bf16-staging kernel bit-equal to the fp32-staging one on the widened operand.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_ref as fr  # noqa: E402
import wgrad_plan_cases as wc  # noqa: E402
from test_gpu_bf16s_exact import NAN_H, NANF, TOL, Flat, P, Win, dev, same  # noqa: E402

pytestmark = pytest.mark.gpu
_ids = lambda c: c.name   # noqa: E731
EX_CASES = [c for c in wc.CASES if c.kernel in (wc.K_F32, wc.K_EDGE, wc.K_BF16)]
BF16S_CASES = [c for c in wc.CASES if c.kernel == wc.K_BF16S]


def device_plan(lib, c):
    """The plan of the row's launch on this device, with the property the row exists for asserted on it."""
    from dep_gan_im_amd import _lib
    B, H, W, ci, co, k = c.shape
    out = (C.c_int * 4)()
    _lib.check(lib.depgan_debug_wgrad_plan(c.kernel, k, B, H, W, ci, co, out), "debug_wgrad_plan")
    wc.check_plan(c, tuple(out))
    print("%s: %s tiles %d, per workgroup %d, chunks %d, gridDim.y %d" % ((c.name, wc.variant(c.kernel, k, ci, co)) + tuple(out)))
    return tuple(out)


def _case_ref(c, kind):
    """operands and float64 references of a row (every (row, kind) pair belongs to exactly one test)"""
    x, dyf, dy = wc.operands(c, kind)
    if kind == "exact":
        assert fr.is_bf16(x) and fr.is_bf16(dyf) and wc.sum_bound(x, dy) < wc.SUM_BOUND
    if c.kernel == wc.K_DECONV:
        return x, dyf, dy, wc.deconv_ref(x, dy)
    rounded = kind == "real" and c.kernel in (wc.K_BF16, wc.K_BF16S)      # x of the bf16-staging kernel is bf16 already
    if kind == "real" and c.kernel == wc.K_BF16S:
        x = fr.rne_bf16(x)
    g = fr.wgrad(fr.bf16_round(x) if rounded else x, fr.bf16_round(dy) if rounded else dy, c.shape[5])
    col = dy[:c.colB].astype(np.float64).sum(axis=(0, 1, 2)) if c.colB else None
    return x, dyf, dy, (g, col)


def rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _f32_exact(a):
    """every value of the float64 array is a float32 value (an fp32 operation that yields it does not round)"""
    return np.array_equal(np.asarray(a, np.float64).astype(np.float32).astype(np.float64), a)


def _twice(call, written):
    """run `call` on fresh buffers twice; the results must have the same bits and the sentinels must be untouched"""
    outs = []
    for rep in range(2):
        bufs = written()
        call(bufs)
        torch.cuda.synchronize()
        outs.append({n: (None if f is None else f.read()) for n, f in bufs.items()})
        for n, f in bufs.items():
            assert f is None or f.outside_unchanged(), n
    for n in outs[0]:
        assert outs[0][n] is None or np.array_equal(outs[0][n].view(np.uint32), outs[1][n].view(np.uint32)), n
    return outs[0]


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("case", EX_CASES, ids=_ids)
def test_wgrad_ex_past_one_tile_per_workgroup(lib, case, kind):
    """depgan_op_conv2d_wgrad_ex with bf16 = 0 (fp32 MFMA and edge kernels) and 1 (bf16 pipe, fp32 staging), with the
    row's scale / raw / accumulate / OI / strided-grid extras and column sums over the samples b < colB."""
    from dep_gan_im_amd import _lib
    c = case
    B, H, W, ci, co, k = c.shape
    device_plan(lib, c)
    assert (c.kernel == wc.K_EDGE) == (not (ci % 4 == 0 and co % 4 == 0 and ci >= 8))      # the entry's own dispatch
    bf16, ex = int(c.kernel == wc.K_BF16), kind == "exact"
    x, dyf, dy, (g, col) = _case_ref(c, kind)
    rng = np.random.default_rng(ci * 100 + co + k + B)
    scale = (rng.choice(fr.SCALES, co) if ex else rng.uniform(0.5, 1.5, co)).astype(np.float32) if c.scale else None
    cscale = (rng.choice(fr.SCALES, co) if ex else rng.uniform(0.5, 1.5, co)).astype(np.float32) if c.colB else None
    old = ((rng.integers(-32, 33, (k, k, ci, co)) / 8.0) if ex else rng.standard_normal((k, k, ci, co))).astype(np.float32)
    lay = (lambda a: np.ascontiguousarray(a.transpose(0, 1, 3, 2))) if c.oi else (lambda a: a)
    scaled = g * (scale.astype(np.float64) if c.scale else 1.0)
    ref_dw = lay(scaled + (old if c.acc else 0.0))
    if ex:      # the finish launch's multiply and add do not round either
        assert _f32_exact(scaled) and _f32_exact(ref_dw) and (not c.colB or _f32_exact(col * cscale.astype(np.float64)))
    wx = Win((B, H, W, ci), 12 + (-ci % 4), 4, "f", NANF, x)
    wdy = Win(dyf.shape, 20 + (-co % 4), 8, "f", NANF, dyf)
    dyargs = wdy.args(c.grid[0] * wdy.strides[1] + c.grid[1] * wdy.strides[2], (1, 2, 2)) if c.grid else wdy.args()
    sd, csd = dev(scale), dev(cscale)
    n = k * k * ci * co

    def written():
        return {"dw": Flat(n, "f", lay(old) if c.acc else None), "raw": Flat(n, "f") if c.raw else None,
                "colout": Flat(co, "f") if c.colB else None, "colraw": Flat(co, "f") if c.colB else None}

    def call(b):
        ptr = lambda f: None if f is None else f.ptr()   # noqa: E731
        _lib.check(lib.depgan_op_conv2d_wgrad_ex(*wx.args(), *dyargs, P(sd), b["dw"].ptr(), ptr(b["raw"]), c.acc, c.oi,
                                                 c.colB, P(csd), ptr(b["colout"]), ptr(b["colraw"]), B, H, W, ci, co, k,
                                                 bf16, None), "op_conv2d_wgrad_ex")

    r = _twice(call, written)
    assert wx.unchanged() and wdy.unchanged()
    want = {"dw": ref_dw, "raw": lay(g) if c.raw else None, "colraw": col,
            "colout": col * cscale.astype(np.float64) if c.colB else None}
    for key, w in want.items():
        if w is None:
            continue
        if ex:
            same(r[key], np.asarray(w).ravel(), key)
        else:
            e = rel(r[key], w)
            print("%s %s rel err %.3g" % (c.name, key, e))
            assert e < TOL, (key, e)


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("case", BF16S_CASES, ids=_ids)
def test_wgrad_bf16s_past_one_tile_per_workgroup(lib, case, kind):
    """depgan_op_conv2d_wgrad_bf16s.  exact: the integers of the float64 contraction.  real: dw bit-equal to
    depgan_op_conv2d_wgrad_bf16 on the widened dense operand, which must run the same plan; the column sums (unrounded
    dy, an order of their own) against float64 at TOL."""
    from dep_gan_im_amd import _lib
    c = case
    B, H, W, ci, co, k = c.shape
    pl = device_plan(lib, c)
    x, dyf, dy, (g, col) = _case_ref(c, kind)
    lay = (lambda a: np.ascontiguousarray(a.transpose(0, 1, 3, 2))) if c.oi else (lambda a: a)
    wx = Win((B, H, W, ci), 16, 8, "h", NAN_H, x)
    wdy = Win(dyf.shape, 20, 8, "f", NANF, dyf)
    dyargs = wdy.args(c.grid[0] * wdy.strides[1] + c.grid[1] * wdy.strides[2], (1, 2, 2)) if c.grid else wdy.args()

    def call(b):
        _lib.check(lib.depgan_op_conv2d_wgrad_bf16s(*wx.args(), *dyargs, b["dw"].ptr(), b["col"].ptr(), B, H, W, ci, co, k,
                                                    c.oi, None), "op_conv2d_wgrad_bf16s")

    r = _twice(call, lambda: {"dw": Flat(k * k * ci * co, "f"), "col": Flat(co, "f")})
    assert wx.unchanged() and wdy.unchanged()
    if kind == "exact":
        same(r["dw"], lay(g).ravel(), "dw")
        same(r["col"], col, "colsum")
        return
    out = (C.c_int * 4)()
    _lib.check(lib.depgan_debug_wgrad_plan(wc.K_BF16, k, B, H, W, ci, co, out))
    assert tuple(out) == pl                                   # the fp32-staging twin walks the same chunks
    xd, dyd = dev(x), dev(dy)
    twin = torch.full((k, k, ci, co), float("nan"), device="cuda:0")
    _lib.check(lib.depgan_op_conv2d_wgrad_bf16(P(xd), P(dyd), P(twin), B, H, W, ci, co, k, None))
    torch.cuda.synchronize()
    same(r["dw"], lay(twin.cpu().numpy()).ravel(), "dw vs depgan_op_conv2d_wgrad_bf16")
    e_dw, e_col = rel(r["dw"], lay(g)), rel(r["col"], col)
    print("%s dw rel err %.3g, colsum rel err %.3g" % (c.name, e_dw, e_col))
    assert e_dw < TOL and e_col < TOL


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("case", wc.DECONV_CASES, ids=_ids)
def test_deconv_wgrad_past_one_ring_round(lib, case, kind):
    """depgan_op_deconv2x2_wgrad, dw and the column sums, with two and with three or more rounds of the fragment ring
    per workgroup.  Its operands are dense (the entry knows no other form): each lies between NaNs."""
    from dep_gan_im_amd import _lib
    c = case
    B, H, W, ci, co, _ = c.shape
    device_plan(lib, c)
    x, _, dout, (gw, col) = _case_ref(c, kind)
    fx, fd = Flat(x.size, "f", x, fill=NANF), Flat(dout.size, "f", dout, fill=NANF)

    def call(b):
        _lib.check(lib.depgan_op_deconv2x2_wgrad(fx.ptr(), fd.ptr(), b["dw"].ptr(), b["col"].ptr(), B, H, W, ci, co, None),
                   "op_deconv2x2_wgrad")

    r = _twice(call, lambda: {"dw": Flat(4 * ci * co, "f"), "col": Flat(co, "f")})
    assert fx.unchanged() and fd.unchanged()
    if kind == "exact":
        same(r["dw"], gw.ravel(), "dw")
        same(r["col"], col, "colsum")
    else:
        e_dw, e_col = rel(r["dw"], gw), rel(r["col"], col)
        print("%s dw rel err %.3g, colsum rel err %.3g" % (c.name, e_dw, e_col))
        assert e_dw < TOL and e_col < TOL
