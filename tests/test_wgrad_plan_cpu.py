"""CPU: the case table of tests/test_gpu_wgrad_tiles.py can see the faults it is there for.

tests/wgrad_plan_cases.py restates the launchers' chunking for 256 compute units; here every row's plan property is
asserted on that restatement (on the device test_gpu_wgrad_tiles.py asserts it on depgan_debug_wgrad_plan, which is the
authority), the restatement is held against the export where the export sees 256 compute units, and a numpy emulation
that walks the tiles chunk by chunk is (1) equal to fused_ref.wgrad on the exact operands of every row and (2) changed
by every mutant on every row whose property the mutant targets:

  skip_last            the last tile of every chunk is not multiplied
  stale_dy             tile t is multiplied with the dy of tile t - 2 (an LDS buffer that was not refilled)
  prev_sample_tag      a tile's column sums are gated by the sample of the tile before it
  border_as_interior   the first border tile after an interior one is staged without its bounds tests
  last_step_twice      transposed kernel: the clamped re-read of a chunk's last k-step is multiplied
  drop_second_round    transposed kernel: the second round of the fragment ring is not multiplied
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_ref as fr  # noqa: E402
import wgrad_plan_cases as wc  # noqa: E402

_ids = lambda c: c.name   # noqa: E731


def test_every_variant_and_family_has_its_rows():
    t3 = {wc.variant(c.kernel, c.shape[5], c.shape[3], c.shape[4]) for c in wc.TILE_CASES if "t3" in c.props}
    assert t3 == set(wc.TILE_VARIANTS)
    for fam, kernels in wc.FAMILIES.items():
        have = set().union(*(c.props for c in wc.TILE_CASES if c.kernel in kernels))
        assert {"a", "b", "c", "d"} <= have, (fam, sorted(have))
    for ch in (64, 96, 128):
        have = set().union(*(c.props for c in wc.DECONV_CASES if c.shape[3] == ch))
        assert {"r2", "r3"} <= have, (ch, sorted(have))
    # the extras of depgan_op_conv2d_wgrad_ex, each on a multi-tile row of the fp32 and of the bf16 kernel
    for kernel in (wc.K_F32, wc.K_BF16):
        rows = [c for c in wc.TILE_CASES if c.kernel == kernel and "t3" in c.props]
        for extra in ("scale", "raw", "acc", "oi", "grid"):
            assert any(getattr(c, extra) for c in rows), (kernel, extra)
    assert len({c.name for c in wc.CASES}) == len(wc.CASES)


@pytest.mark.parametrize("case", wc.CASES, ids=_ids)
def test_row_has_its_property_at_256_compute_units(case):
    wc.check_plan(case, wc.case_plan_cpu(case))


def _export_cus():
    """compute units the export's chunking sees: the current device's, 256 without one (common.h, dg_cu_count)"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def test_export_agrees_with_the_restatement_and_returns_the_launchers_refusals(lib):
    out = (C.c_int * 4)(-7, -7, -7, -7)
    if _export_cus() == wc.CUS:
        for c in wc.CASES:
            B, H, W, ci, co, k = c.shape
            assert lib.depgan_debug_wgrad_plan(c.kernel, k, B, H, W, ci, co, out) == 0, c.name
            assert tuple(out) == wc.case_plan_cpu(c), c.name
        # the smallest shapes: one tile per workgroup, as the older operator cases have it
        assert lib.depgan_debug_wgrad_plan(wc.K_F32, 3, 2, 21, 19, 40, 96, out) == 0 and out[1] == 1
        assert lib.depgan_debug_wgrad_plan(wc.K_DECONV, 1, 2, 32, 32, 64, 64, out) == 0 and out[1] == wc.DEPTH
    out[:] = [-7] * 4
    refused = [(wc.K_F32, 3, 2, 8, 8, 6, 16, 1), (wc.K_F32, 7, 2, 8, 8, 16, 16, 3), (wc.K_EDGE, 3, 2, 8, 8, 16, 16, 3),
               (wc.K_EDGE, 1, 2, 8, 8, 1, 16, 3), (wc.K_BF16, 3, 2, 8, 8, 4, 16, 3), (wc.K_BF16S, 5, 2, 8, 8, 32, 32, 3),
               (wc.K_BF16S, 3, 2, 8, 8, 36, 32, 3), (wc.K_DECONV, 1, 2, 8, 8, 48, 48, 3), (wc.K_DECONV, 1, 2, 12, 8, 64, 64, 3),
               (5, 3, 2, 8, 8, 32, 32, 1), (-1, 3, 2, 8, 8, 32, 32, 1), (wc.K_F32, 3, 0, 8, 8, 32, 32, 1)]
    for kernel, k, B, H, W, ci, co, status in refused:
        assert lib.depgan_debug_wgrad_plan(kernel, k, B, H, W, ci, co, out) == status, (kernel, k, ci, co)
        assert lib.depgan_last_error()
    assert lib.depgan_debug_wgrad_plan(wc.K_F32, 3, 2, 8, 8, 32, 32, None) == 1
    assert list(out) == [-7] * 4                       # a refusal writes nothing


def _differs(got, ref):
    return not (np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]))


@pytest.mark.parametrize("case", wc.TILE_CASES, ids=_ids)
def test_tile_walk_equals_the_reference_and_every_targeted_mutant_changes_it(case):
    B, H, W, ci, co, k = case.shape
    x, _, dy = wc.operands(case, "exact")
    assert fr.is_bf16(x) and fr.is_bf16(dy) and wc.sum_bound(x, dy) < wc.SUM_BOUND
    nT, tpc, nch, gy = wc.case_plan_cpu(case)
    th = wc.tile_h(case.kernel, k, ci, co)
    ref = (fr.wgrad(x, dy, k), dy[:case.colB].astype(np.float64).sum(axis=(0, 1, 2)))
    got = wc.emulate_tiles(x, dy, k, th, tpc, case.colB)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    for mutant, targets in wc.MUTANTS_TILE.items():
        if targets & case.props:
            assert _differs(wc.emulate_tiles(x, dy, k, th, tpc, case.colB, mutant), ref), mutant


@pytest.mark.parametrize("case", wc.DECONV_CASES, ids=_ids)
def test_step_walk_equals_the_reference_and_every_mutant_changes_it(case):
    x, _, dout = wc.operands(case, "exact")
    assert wc.sum_bound(x, dout) < wc.SUM_BOUND
    steps = wc.case_plan_cpu(case)[1]
    ref = wc.deconv_ref(x, dout)
    # the reference itself against autograd of the transposed convolution, once per channel count
    if "r2" in case.props:
        import torch
        import torch.nn.functional as F
        wt = torch.zeros(x.shape[3], dout.shape[3], 2, 2, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose2d(torch.from_numpy(x).permute(0, 3, 1, 2).double(), wt, stride=2)
        (gw,) = torch.autograd.grad(y, wt, torch.from_numpy(dout).permute(0, 3, 1, 2).double())
        assert np.array_equal(ref[0], gw.permute(2, 3, 1, 0).numpy())
    got = wc.emulate_deconv(x, dout, steps)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    for mutant, targets in wc.MUTANTS_DECONV.items():
        assert targets & case.props
        assert _differs(wc.emulate_deconv(x, dout, steps, mutant), ref), mutant
