"""GPU, operator level: the Winograd 3x3 kernel with V in registers (csrc/igemm_wino.hip; operator path 8), at the
smallest shapes at which its lane mapping, its raw-image swizzle or its staging can still be wrong.  The mapping itself
is enumerated on the CPU by tests/test_wino_regmap_cpu.py; this file runs it.

Method, windows and sentinels are those of tests/test_gpu_fused_ops.py (imported, not copied): exact operands (small
integers and dyadic fractions, tests/fused_ref.py) compare with np.array_equal against float64; every operand is a
window of a wider buffer, NaN around what is read, sentinels around what is written.

  case  B, H, W, Cin -> Cout         what it exercises
  1     1, 8, 16, 8 -> 32            one item, one chunk (only the zero-C first MFMA), every tile on the border
  2     2, 24, 48, 24 -> 64          interior and border items, three chunks (both raw buffers, an odd count), two
                                     output-channel tiles
  3     1, 10, 18, 16 -> 32          ragged bottom and right tiles, out-of-tile sentinel pieces, partial epilogue
  4     2, 24, 48, gathered -> 64    ConvArgs::cpt > 0 (depgan_op_conv3x3_wino_gathered): the runs of the K axis come from
                                     separate windows.  Runs are whole 8-channel chunks, so case 2's 24 channels are three
                                     runs of one chunk; two runs of two chunks (32 channels) walk inside a run as well
  5     8, 64, 96, 16 -> 96          1152 items > 768 resident workgroups: the persistent loop takes a second item
  6     1, 32, 32 and 1, 18, 32, 16 -> 32 with the fused one-channel head: the 16-row form (two transform tasks per lane),
                                     selected by the head itself, not by the environment
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
from test_gpu_fused_ops import SENT, TOL, P, Win, bits, dev, rel  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT = [
    ("bias", (1, 8, 16, 8, 32, 3)), ("film_pool", (1, 8, 16, 8, 32, 3)),                     # 1
    ("affine_relu", (2, 24, 48, 24, 64, 3)), ("film_pool", (2, 24, 48, 24, 64, 3)),          # 2
    ("bias", (1, 10, 18, 16, 32, 3)), ("film_pool", (1, 10, 18, 16, 32, 3)),                 # 3
    ("bias", (8, 64, 96, 16, 96, 3)),                                                        # 5
    ("head", (1, 32, 32, 16, 32, 3)), ("head", (1, 18, 32, 16, 32, 3)),                      # 6
    ("head_skip", (1, 18, 32, 16, 32, 3)),
]
_id = lambda c: "%s-%s" % (c[0], "x".join(map(str, c[1])))   # noqa: E731


@pytest.mark.parametrize("case", EXACT, ids=_id)
def test_exact_operands_are_bit_exact(lib, case):
    feat, shape = case
    assert feat in tfo.ACCEPTS[8]
    tfo.test_fused_epilogue_exact_operands_are_bit_exact(lib, (8, feat, shape))


def test_case_5_is_persistent(lib):
    """the shape of case 5 has more items than workgroups can be resident (three per CU at 8-row tiles)"""
    B, H, W, _, co, _ = EXACT[6][1]
    items = B * (H // 8) * (W // 16) * (co // 32)
    assert items == 1152 > 3 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("runs,cin", [(3, 24), (2, 32)])
def test_gathered_k_exact(lib, runs, cin):
    """case 4: run t of the K axis is a window of its own (another channel offset, NaN all around), all in one
    allocation; the reference convolves the concatenated channels"""
    from dep_gan_im_amd import _lib
    B, H, W, co = 2, 24, 48, 64
    rl = cin // runs
    rng = np.random.default_rng(cin * 7 + runs)
    x = rng.integers(-2, 3, (B, H, W, cin)).astype(np.float32)
    w = rng.integers(-1, 2, (3, 3, cin, co)).astype(np.float32)
    bias = (rng.integers(-16, 17, co) / 8.0).astype(np.float32)
    Ct = rl + 12
    full = np.full((runs, B + 3, H + 2, W + 3, Ct), np.float32("nan"), np.float32)
    strides = ((H + 2) * (W + 3) * Ct, (W + 3) * Ct, Ct)
    offs = []
    for t in range(runs):
        c0 = 4 + 4 * (t & 1)
        full[t, 1:1 + B, 1:1 + H, 2:2 + W, c0:c0 + rl] = x[..., t * rl:(t + 1) * rl]
        offs.append(t * (B + 3) * strides[0] + strides[0] + strides[1] + 2 * strides[2] + c0)
    buf = torch.from_numpy(full).to("cuda:0")
    run_off = (C.c_long * 4)(*[o - offs[0] for o in offs])
    out = Win((B, H, W, co), 20, 8, SENT)
    dw, db = dev(w), dev(bias)
    _lib.check(lib.depgan_op_conv3x3_wino_gathered(C.c_void_p(buf.data_ptr() + 4 * offs[0]), *strides, run_off, runs, P(dw), P(db),
                                                   *out.args(), B, H, W, cin, co, None), "op_conv3x3_wino_gathered")
    torch.cuda.synchronize()
    ref = fr.conv_acc(x, w) + bias.astype(np.float64)
    got = out.read()
    assert np.array_equal(got, ref), "%d wrong, first at %s" % ((got != ref).sum(), np.argwhere(got != ref)[:1].tolist())
    assert out.outside_unchanged()
    assert np.array_equal(bits(buf.cpu().numpy()), bits(full))


def test_gathered_k_refusals(lib):
    """runs that are no whole chunks, and a run offset off its 16 bytes: a status, nothing written"""
    x = torch.zeros(1 * 8 * 16 * 64, device="cuda:0")
    w = torch.zeros(3 * 3 * 24 * 32, device="cuda:0")
    out = Win((1, 8, 16, 32), 20, 8, SENT)
    for runs, cin, off1 in ((2, 24, 16), (2, 16, 6), (5, 40, 16)):
        run_off = (C.c_long * 4)(0, off1, 0, 0)
        rc = lib.depgan_op_conv3x3_wino_gathered(P(x), 8 * 16 * 64, 16 * 64, 64, run_off, runs, P(w), None, *out.args(),
                                                 1, 8, 16, cin, 32, None)
        torch.cuda.synchronize()
        assert rc != 0 and lib.depgan_last_error(), (runs, cin, off1)
        assert out.unchanged()


# one real-operand case per tile form: 8-row tiles (case 2's shape, FiLM layer) and 16-row tiles (the fused head)
REAL = [("film", (2, 24, 48, 24, 64, 3)), ("head", (1, 18, 32, 16, 32, 3))]


@pytest.mark.parametrize("case", REAL, ids=_id)
def test_real_operands_within_tol_and_repeatable(lib, case):
    """out_pre within 1e-4 of float64 (the bound of tests/test_gpu_fused_ops.py and test_gpu_ops.py), the chain after it
    bit for bit from the kernel's own out_pre, two runs equal bits, surroundings untouched"""
    from dep_gan_im_amd import _lib
    feat, shape = case
    runs = []
    for _ in range(2):
        rc, o, w, (pre, pool, head) = tfo.run_fused(lib, 8, feat, shape, "real", want_pre=True)
        _lib.check(rc, "op_conv2d_fused")
        got = {n: w[n].read() for n in w if n in ("out", "pre", "pool", "head")}
        for n in got:
            assert w[n].outside_unchanged(), n
        for n in ("in", "res", "mask"):
            assert n not in w or w[n].unchanged(), n
        runs.append((o, got))
    o, got = runs[0]
    for n in got:
        assert np.array_equal(bits(got[n]), bits(runs[1][1][n])), n
    ref = fr.reference(o)
    e = rel(got["pre"], ref["out_pre"])
    print("out_pre rel err %.3g" % e)
    assert e < TOL
    out, _ = fr.post_chain(got["pre"], o)
    assert np.array_equal(got["out"], out)
    if head:
        h = np.tanh(fr.head(out, o))
        e = rel(got["head"].reshape(h.shape), h)
        print("head rel err %.3g" % e)
        assert e < TOL
