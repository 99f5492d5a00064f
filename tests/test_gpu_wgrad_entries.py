"""GPU: every weight-gradient operator entry runs the one driver (wgrad_run of model.hip, through op_wgrad).

depgan_op_conv2d_wgrad, depgan_op_conv2d_wgrad_bf16 and depgan_op_conv2d_wgrad_bf16s used to launch their slab kernel
and its finish themselves; depgan_op_conv2d_wgrad_ex always went through the model's driver.  Here each of them equals
depgan_op_conv2d_wgrad_ex bit for bit at the smallest shape of its kernel family (the values themselves are held against
float64 in test_gpu_ops.py, test_gpu_wgrad_tiles.py and test_gpu_bf16s_exact.py).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _operands(shape):
    B, H, W, ci, co, k = shape
    g = torch.Generator().manual_seed(1000 * ci + 10 * co + k)
    x = torch.randn(B, H, W, ci, generator=g).to("cuda:0")
    dy = torch.randn(B, H, W, co, generator=g).to("cuda:0")
    return x, dy


def _dense(t):
    B, H, W, c = t.shape
    return (P(t), H * W * c, W * c, c)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda:0")


def _same_bits(a, b, what):
    torch.cuda.synchronize()
    assert not torch.isnan(a).any() and not torch.isnan(b).any(), what
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


def _ex(lib, x, dy, shape, bf16, col=None):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co, k = shape
    dw = _nan(k, k, ci, co)
    _lib.check(lib.depgan_op_conv2d_wgrad_ex(*_dense(x), *_dense(dy), None, P(dw), None, 0, 0, B if col is not None else 0,
                                             None, P(col), None, B, H, W, ci, co, k, bf16, None), "op_conv2d_wgrad_ex")
    return dw


@pytest.mark.parametrize("shape,bf16", [((2, 21, 19, 40, 96, 3), 0),          # fp32 MFMA kernel
                                        ((2, 8, 8, 1, 16, 5), 0), ((2, 8, 8, 2, 32, 3), 0),      # edge kernels
                                        ((2, 16, 16, 8, 32, 3), 1)],          # bf16 pipe, fp32 staging
                         ids=["f32", "edge-k5", "edge-k3", "bf16"])
def test_dense_entries_equal_the_ex_entry(lib, shape, bf16):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co, k = shape
    x, dy = _operands(shape)
    got = _nan(k, k, ci, co)
    entry = lib.depgan_op_conv2d_wgrad_bf16 if bf16 else lib.depgan_op_conv2d_wgrad
    _lib.check(entry(P(x), P(dy), P(got), B, H, W, ci, co, k, None), "op_conv2d_wgrad" + ("_bf16" if bf16 else ""))
    _same_bits(got, _ex(lib, x, dy, shape, bf16), "dw")


@pytest.mark.parametrize("k", [1, 3])
def test_bf16s_entry_equals_the_ex_entry_on_the_widened_operand(lib, k):
    from dep_gan_im_amd import _lib
    shape = (2, 16, 16, 8, 32, k)
    B, H, W, ci, co, _ = shape
    x, dy = _operands(shape)
    xh = x.to(torch.bfloat16)                                   # round to nearest even
    got, col = _nan(k, k, ci, co), _nan(co)
    _lib.check(lib.depgan_op_conv2d_wgrad_bf16s(*_dense(xh), *_dense(dy), P(got), P(col), B, H, W, ci, co, k, 0, None),
               "op_conv2d_wgrad_bf16s")
    ref_col = _nan(co)
    _same_bits(got, _ex(lib, xh.float(), dy, shape, 1, ref_col), "dw")
    _same_bits(col, ref_col, "column sums")
