"""GPU, operator level: the ring of raw halo buffers of the Winograd 3x3 kernel (csrc/igemm_wino.hip; operator path 8).

Chunk c of an item (8 input channels) is copied into ring slot c % NBUF by a DMA issued NBUF - 1 chunks ahead (NBUF = 2
in the product kernel, 3 a valid value the cases are chosen for), and a wave waits for it by COUNT: vmcnt(younger DMA
instructions + 4 weight-fragment loads), fewer at the end of an item; the fragment loads themselves are counted by hand.  A
wrong count, a wrong slot or a DMA left in flight across an item boundary reads a stale or half-written raw image: wrong
values, no fault.  The cases are the smallest at which that can happen.

Method, windows and sentinels are those of tests/test_gpu_fused_ops.py (imported, not copied): exact operands (small
integers and dyadic fractions, tests/fused_ref.py) compare with np.array_equal against float64 -- the one correct bit
pattern -- and every operand is a window of a wider buffer, NaN around what is read, sentinels around what is written.

  chunk counts   Cin = 8, 16, 24, 32, 40, 56 -> 32: 1, 2, 3, 4, 5 and 7 chunks -- an item shorter than the ring's depth,
                 equal to it, every residue of the count modulo 3, the ring wrapping more than once; on a single-tile
                 image and on 2 x 22 x 18 (border tiles in both directions: the bounds-checked staging branch in every
                 slot)
  persistent     32 x 64 x 64 at Cin = 8, 24, 40: more items than resident workgroups, so a workgroup's second and later
                 items start on a ring (and on Z planes over it) the previous item left behind; interior tiles
  16-row form    the fused head selects it: three DMA instructions per chunk, its own counts; one persistent shape
  gathered K     ConvArgs::cpt > 0 in the geometry of the transposed convolution's backward-data: the four runs are the
                 four pixel grids of a gradient at twice the size; a run boundary falls between two chunks in flight
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

CINS = [8, 16, 24, 32, 40, 56]                   # 1, 2, 3, 4, 5, 7 chunks
SIZES = [(2, 8, 16), (2, 22, 18)]
CHUNKS = [("bias", s + (ci, 32, 3)) for s in SIZES for ci in CINS]
PERS = [(f, PERSIST[:3] + (ci, co, 3)) for ci in (8, 24, 40) for co in (32, 64) for f in ("film_pool", "bias")]
HEAD = [("head", (2, 22, 18, ci, 32, 3)) for ci in (8, 24, 32)]
HEAD_PERS = ("head", (9, 128, 128, 24, 32, 3))
_id = lambda c: "%s-%s" % (c[0], "x".join(map(str, c[1])))   # noqa: E731


def _exact(lib, case):
    feat, shape = case
    assert feat in tfo.ACCEPTS[8]
    tfo.test_fused_epilogue_exact_operands_are_bit_exact(lib, (8, feat, shape))     # asserts on the whole tensors


@pytest.mark.parametrize("case", CHUNKS, ids=_id)
def test_every_chunk_count_against_the_ring(lib, case):
    _exact(lib, case)


@pytest.mark.parametrize("case", PERS, ids=_id)
def test_persistent_items_start_on_a_used_ring(lib, case):
    B, H, W, _, co, _ = case[1]
    items = B * (H // 8) * (W // 16) * (co // 32)
    assert items > 3 * torch.cuda.get_device_properties(0).multi_processor_count      # three workgroups per CU at the most
    _exact(lib, case)


@pytest.mark.parametrize("case", HEAD, ids=_id)
def test_sixteen_row_form(lib, case):
    _exact(lib, case)


def test_sixteen_row_form_persistent(lib):
    B, H, W = HEAD_PERS[1][:3]
    assert B * (H // 16) * (W // 16) > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    _exact(lib, HEAD_PERS)


@pytest.mark.parametrize("rl", [8, 16])
def test_gathered_k_run_boundary_between_chunks_in_flight(lib, rl):
    """The backward-data of the 2x2 / stride-2 transposed convolution gathers its K axis from the four pixel grids
    (di, dj) of the upstream gradient (tests/test_gpu_fused_ops.py, test_deconv_backward_data_gathered_and_accumulated);
    here that gather feeds the 3x3 kernel: run t = 2 di + dj reads dy[:, 2i + di, 2j + dj, :], rl channels each.  rl = 8:
    four chunks, a run boundary between every two; rl = 16: eight chunks, boundaries behind chunks 1, 3 and 5 -- with two
    chunks in flight the DMAs on either side of a boundary are always outstanding together."""
    from dep_gan_im_amd import _lib
    B, H, W, co = 2, 22, 18, 32
    cin = 4 * rl
    rng = np.random.default_rng(rl)
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
