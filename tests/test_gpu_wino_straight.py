"""GPU, operator level: the straight-line chunk loop of the Winograd 3x3 kernel (csrc/igemm_wino.hip; operator path 8).

An item's chunks (8 input channels each) are walked as: the first chunk; a steady state unrolled by two, whose bodies
carry the ring slot as an immediate (slot 1, then slot 0); one more slot-1 chunk when the count is odd; the last chunk,
which issues no DMA.  The DMA's scalar offset and the weight-fragment base advance by one addition per chunk, whether a
DMA piece lies in the image is decided once per item, and gathered K (ConvArgs::cpt) is a kernel of its own that forms a
run's offset when the run starts.  A wrong immediate, a wrong peel or an offset carried over from the previous item reads
the wrong raw image or the wrong weights: wrong values, no fault.  The cases are the smallest that reach each of these
paths and are not already in tests/test_gpu_wino_ring.py, whose method this file uses (exact operands, np.array_equal
against float64, NaN-framed input windows and sentinel-framed outputs; imported from tests/test_gpu_fused_ops.py).

  chunk counts   Cin = 48, 64, 72 -> 32: 6, 8 and 9 chunks -- the unrolled pair is entered, runs for more than one round
                 and is left at both parities of the count; on a single-tile image and on 2 x 22 x 18 (border tiles)
  persistent     32 x 64 x 64 at Cin = 16, 48: a workgroup's items alternate between border and interior tiles, so the
                 per-item piece offsets change from item to item
  gathered K     run length 24 channels = three chunks a run (Cin = 96, 12 chunks): run boundaries at odd chunk
                 positions, inside the unrolled pair; run length 8 with 64 output channels: the second channel tile
                 starts the run walk again
  16-row form    the fused head selects it; it has the same loop: Cin = 16 and 48 on 2 x 22 x 18
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
from test_gpu_fused_ops import PERSIST, SENT, P, Win, dev  # noqa: E402

pytestmark = pytest.mark.gpu

CINS = [48, 64, 72]                              # 6, 8, 9 chunks
SIZES = [(2, 8, 16), (2, 22, 18)]
CHUNKS = [("bias", s + (ci, 32, 3)) for s in SIZES for ci in CINS]
PERS = [(f, PERSIST[:3] + (ci, co, 3)) for ci in (16, 48) for co in (32, 64) for f in ("bias", "film_pool")]
HEAD = [("head", (2, 22, 18, ci, 32, 3)) for ci in (16, 48)]
_id = lambda c: "%s-%s" % (c[0], "x".join(map(str, c[1])))   # noqa: E731


def _exact(lib, case):
    feat, shape = case
    assert feat in tfo.ACCEPTS[8]
    tfo.test_fused_epilogue_exact_operands_are_bit_exact(lib, (8, feat, shape))     # asserts on the whole tensors


@pytest.mark.parametrize("case", CHUNKS, ids=_id)
def test_unrolled_pair_and_peeled_last_chunk(lib, case):
    _exact(lib, case)


@pytest.mark.parametrize("case", PERS, ids=_id)
def test_persistent_items_alternate_border_and_interior(lib, case):
    B, H, W, _, co, _ = case[1]
    items = B * (H // 8) * (W // 16) * (co // 32)
    assert items > 3 * torch.cuda.get_device_properties(0).multi_processor_count      # three workgroups per CU at the most
    assert H // 8 > 2 and W // 16 > 2                                                  # interior tiles exist next to border ones
    _exact(lib, case)


@pytest.mark.parametrize("case", HEAD, ids=_id)
def test_sixteen_row_form(lib, case):
    _exact(lib, case)


@pytest.mark.parametrize("rl,co", [(24, 32), (8, 64)])
def test_gathered_k_runs_across_the_unrolled_pair(lib, rl, co):
    """The gather of tests/test_gpu_wino_ring.py (the four pixel grids of a gradient at twice the size feed the 3x3
    kernel, run t = 2 di + dj reads dy[:, 2i + di, 2j + dj, :]) with rl = 24: three chunks a run, boundaries behind
    chunks 2, 5 and 8 -- the first and third between the two bodies of a round, the second at its back edge; and with
    rl = 8 at two channel tiles: every chunk starts a run, and the second tile's items start again at run 0."""
    from dep_gan_im_amd import _lib
    B, H, W = 2, 22, 18
    cin = 4 * rl
    rng = np.random.default_rng(100 * rl + co)
    dy = rng.integers(-2, 3, (B, 2 * H, 2 * W, rl)).astype(np.float32)
    w = rng.integers(-1, 2, (3, 3, cin, co)).astype(np.float32)
    bias = (rng.integers(-16, 17, co) / 8.0).astype(np.float32)
    wdy = Win((B, 2 * H, 2 * W, rl), 12, 4, np.float32("nan"), dy)
    ptr, sB, sY, sX = wdy.args()
    run_off = (C.c_long * 4)(*[(t // 2) * sY + (t % 2) * sX for t in range(4)])
    out = Win((B, H, W, co), 20, 8, SENT)
    dw, db = dev(w), dev(bias)
    _lib.check(lib.depgan_op_conv3x3_wino_gathered(ptr, sB, 2 * sY, 2 * sX, run_off, 4, P(dw), P(db), *out.args(),
                                                   B, H, W, cin, co, None), "op_conv3x3_wino_gathered")
    torch.cuda.synchronize()
    x = np.concatenate([dy[:, t // 2::2, t % 2::2, :] for t in range(4)], axis=-1)
    ref = fr.conv_acc(x, w) + bias.astype(np.float64)
    assert np.abs(ref).max() < fr.VALUE_BOUND and np.array_equal(ref, np.round(ref / fr.QUANTUM) * fr.QUANTUM)
    got = out.read()
    assert np.array_equal(got, ref), "%d wrong, first at %s" % ((got != ref).sum(), np.argwhere(got != ref)[:1].tolist())
    assert out.outside_unchanged() and wdy.unchanged()
