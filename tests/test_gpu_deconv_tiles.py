"""GPU, operator level: the fused forward transposed-convolution kernel (csrc/deconv_fwd.hip) PAST ONE TILE PER WORKGROUP.

The kernel is persistent: a workgroup keeps its weights in registers and walks the 32-pixel tiles blockIdx.x,
blockIdx.x + gridDim.x, ...  Its first tile runs the plain body; every later one runs the body with the hand-placed slot
schedule, which inside the MFMA stream of tile t reads tile t - 1 back from the wave's LDS blocks, applies the ReLU, stores
it and stages tile t + 1 into the other half of the double buffer -- and which alone takes the WIDE shortcut for the pass
origins.  The launches of tests/test_gpu_ops.py (DECONV_CASES) and tests/test_gpu_stream_ops.py have at most as many tiles
as workgroups, so that body, the second round of the double buffer, the uneven end of the loop (`nld`, the tail store)
and a strided output view ran only inside the whole-network tests, whose tolerances absorb one stale 16-byte piece.

Launch sizes come from the DEVICE: depgan_debug_deconv_fwd_plan reports the grid the launcher itself computes, and
tests/deconv_tile_cases.py turns it into the smallest batches with tiles = gridDim.x + 1 (or + 2), 2 gridDim.x and
>= 3 gridDim.x + 1 with uneven trip counts, for each of the six instantiations (Cin 64 / 96 / 128, WIDE and narrow), an
image smaller than a tile, and Cin != Cout with gridDim.y of 2 and 3.  No CU count and no occupancy is written down
here; test_case_table_reaches_every_loop_form asserts on the plan's numbers that nothing of this got lost.

Per launch, for exact and real operands (tests/fused_ref.py), the epilogues {bias + scale/shift + ReLU, bias, none} and
the outputs {dense through depgan_op_deconv2x2, a channel slice of a wider sentinel-filled buffer (Win) through
depgan_op_deconv2x2_ex}:
  exact    equal to the float64 contract (tests/test_deconv_tiles_cpu.py proves the folded form exact on these operands)
  real     max |got - ref| / max |ref| < TOL, taken per tile, the worst tile printed;
           bit-equal to the same input run as sub-batches of at most gridDim.x tiles (one tile per workgroup, the path
           the other files check): a pixel's summation order does not depend on the trip that computes it
  always   the slice equals the dense result bit for bit, every float outside it and the input are unchanged, and a
           second run repeats the first bit for bit.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deconv_tile_cases as dc  # noqa: E402
import fused_ref as fr  # noqa: E402
from test_gpu_fused_ops import SENT, TOL, Win, P, _deconv_ops, dev  # noqa: E402

pytestmark = pytest.mark.gpu
EPILOGUES = {"affine_relu": dict(bias=1, affine=1, relu=1), "bias": dict(bias=1), "none": {}}
GUARD = 64                      # floats on either side of a dense buffer (256 bytes: the pointer stays 16-byte aligned)
_GRID = {}


def plan(lib, r, B):
    """(tiles, gridDim.x, gridDim.y, workgroups per CU) of the row's launch at batch B on this device"""
    from dep_gan_im_amd import _lib
    out = (C.c_long * 4)()
    _lib.check(lib.depgan_debug_deconv_fwd_plan(B, r.H, r.W, r.Cin, r.Cout, out), "debug_deconv_fwd_plan")
    return tuple(out)


def grid_of(lib, r):
    """the row's uncapped grid: the plan of a batch with more tiles than any device has workgroups"""
    if r.name not in _GRID:
        tiles, gx, gy, per_cu = plan(lib, r, dc.BIG_B)
        assert tiles == dc.tiles_of(dc.BIG_B, r.H, r.W) and 2 <= gx < tiles, (tiles, gx)
        assert gy == dc.grid_y(r) and per_cu >= 1
        _GRID[r.name] = (gx, gy, per_cu)
    return _GRID[r.name]


def launch_of(lib, r, name):
    """batch and plan of one of the row's three launches, with the property it exists for asserted on the plan"""
    gx, gy, per_cu = grid_of(lib, r)
    B = dc.batches(gx, gy, r.H, r.W)[name]
    tiles, pgx, pgy, _ = plan(lib, r, B)
    assert (tiles, pgx, pgy) == (dc.tiles_of(B, r.H, r.W), gx, gy)
    lo, hi = dc.trips(tiles, gx)
    assert {"one_extra": (lo, hi) == (1, 2), "two_each": lo == 2, "uneven": lo >= 3 and hi == lo + 1}[name], (tiles, gx)
    print("%s %s: B %d, tiles %d, grid (%d, %d), %d workgroups per CU, %d..%d tiles per workgroup"
          % (r.name, name, B, tiles, gx, gy, per_cu, lo, hi))
    return B, tiles, gx, gy


def ibits(t):
    return t.contiguous().view(torch.int32)


class Dense:
    """n floats between two guards, on the device; `fill` everywhere, `data` in the middle"""

    def __init__(self, n, fill, data=None):
        self.n = n
        self.t0 = torch.full((n + 2 * GUARD,), float(fill), dtype=torch.float32, device="cuda:0")
        if data is not None:
            self.t0[GUARD:GUARD + n] = torch.from_numpy(np.ascontiguousarray(data, np.float32).ravel()).to("cuda:0")
        self.t = self.t0.clone()

    def reset(self):
        self.t.copy_(self.t0)

    def ptr(self, off=0):
        return C.c_void_p(self.t.data_ptr() + 4 * (GUARD + off))

    def body(self):
        return self.t[GUARD:GUARD + self.n]

    def guards_unchanged(self):
        return (torch.equal(ibits(self.t[:GUARD]), ibits(self.t0[:GUARD])) and
                torch.equal(ibits(self.t[-GUARD:]), ibits(self.t0[-GUARD:])))

    def unchanged(self):
        return torch.equal(ibits(self.t), ibits(self.t0))


def tile_major(a, B, H, W, co):
    """(B, 2H, 2W, co) -> (tiles, 32 * 4 * co): the output floats of every 32-pixel input tile"""
    return a.view(B, H, 2, W, 2, co).permute(0, 1, 3, 2, 4, 5).reshape(B * H * W // 32, -1)


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("launch", dc.LAUNCHES)
@pytest.mark.parametrize("row", dc.ROWS, ids=lambda r: r.name)
def test_deconv_forward_past_one_tile_per_workgroup(lib, row, launch, kind):
    from dep_gan_im_amd import _lib
    r = row
    H, W, ci, co = r.H, r.W, r.Cin, r.Cout
    B, tiles, gx, gy = launch_of(lib, r, launch)
    x, _, wt = _deconv_ops(kind, (B, H, W, ci, co), ci + co + W + tiles)
    acc = fr.deconv2x2(x, wt)                                                   # float64, (B, 2H, 2W, co)
    shape, n = (B, 2 * H, 2 * W, co), B * 4 * H * W * co
    xin, wd = Dense(x.size, float("nan"), x), dev(wt)
    dense, split = Dense(n, SENT), Dense(n, SENT)
    wout = Win(shape, 20, 8, SENT)                                              # the layer's slice of a concat buffer
    wout0 = wout.t.clone()
    sub = dc.sub_batch(gx, H, W)

    for ename, feats in EPILOGUES.items():
        o = fr.make_ops(kind, np.random.default_rng(len(ename) + co), 1, 1, 1, ci, co, 1, **feats)
        ref = fr.affine(acc, o, np.float64)
        if o.relu:
            ref = np.maximum(ref, 0)
        ref_d = torch.from_numpy(ref).to("cuda:0")
        d = [dev(a) for a in (o.bias, o.scale, o.shift)]

        def run_dense(buf, b0=0, nb=B):
            _lib.check(lib.depgan_op_deconv2x2(xin.ptr(b0 * H * W * ci), P(wd), *map(P, d), buf.ptr(b0 * 4 * H * W * co),
                                               nb, H, W, ci, co, o.relu, None), "op_deconv2x2")

        def run_sliced():
            wout.t.copy_(wout0)
            _lib.check(lib.depgan_op_deconv2x2_ex(xin.ptr(), P(wd), *map(P, d), *wout.args(), B, H, W, ci, co, o.relu, None),
                       "op_deconv2x2_ex")
            torch.cuda.synchronize()
            got = wout.t[wout.sl].contiguous()
            wout.t[wout.sl] = wout0[wout.sl]
            assert torch.equal(ibits(wout.t), ibits(wout0)), "%s: a float outside the slice changed" % ename
            return got

        outs = []
        for rep in range(2):
            dense.reset()
            run_dense(dense)
            torch.cuda.synchronize()
            assert dense.guards_unchanged(), ename
            outs.append(dense.body().view(shape).clone())
        outs += [run_sliced(), run_sliced()]
        for i, what in ((1, "dense, second run"), (2, "slice"), (3, "slice, second run")):
            assert torch.equal(ibits(outs[0]), ibits(outs[i])), "%s: %s differs from the first dense run" % (ename, what)
        got = outs[0]
        if kind == "exact":
            assert torch.equal(ref_d.float().double(), ref_d)                   # the contract's values are float32 values
            bad = (got.double() != ref_d).nonzero()
            assert bad.shape[0] == 0, (ename, "first of %d: (b, y, x, c) = %s" % (bad.shape[0], bad[0].tolist()))
        else:
            err = tile_major((got.double() - ref_d).abs(), B, H, W, co).amax(dim=1)
            worst = int(err.argmax())
            e = float(err[worst] / ref_d.abs().max())
            print("%s %s %s: rel err %.3g, worst tile %d of %d (trip %d of workgroup %d)"
                  % (r.name, launch, ename, e, worst, tiles, worst // gx, worst % gx))
            assert e < TOL, (ename, e, worst)
            # the same input as launches of at most gridDim.x tiles: one tile per workgroup
            split.reset()
            for b0 in range(0, B, sub):
                nb = min(sub, B - b0)
                st, sgx, _, _ = plan(lib, r, nb)
                assert st == sgx <= gx
                run_dense(split, b0, nb)
            torch.cuda.synchronize()
            assert split.guards_unchanged()
            diff = (ibits(tile_major(split.body(), B, H, W, co)) != ibits(tile_major(got, B, H, W, co))).any(dim=1).nonzero()
            assert diff.shape[0] == 0, (ename, "tiles that differ from the one-tile-per-workgroup launches: %s"
                                        % diff[:8].ravel().tolist())
    assert xin.unchanged()


def test_case_table_reaches_every_loop_form(lib):
    """From the plan's numbers on THIS device: each of the six instantiations with 2 tiles per workgroup and with at
    least 3, with uneven trip counts, on dense and sliced outputs; an image smaller than a tile; gridDim.y of 1, 2, 3."""
    launches = []
    for r in dc.ROWS:
        for name in dc.LAUNCHES:
            B, tiles, gx, gy = launch_of(lib, r, name)
            assert tiles > gx                                   # none of them is the one-tile path of the other files
            launches += [(r, tiles, gx, gy, sliced) for sliced in (0, 1)]      # every launch runs both outputs
    dc.check_coverage(dc.coverage(launches))


REFUSALS = {
    "pixel_stride_not_multiple_of_4": lambda w: (0, (w.strides[0], w.strides[1], w.strides[2] - 2), 2),
    "pointer_4_bytes_off": lambda w: (4, w.strides, 2),
    "batch_stride_past_32_bit_offsets": lambda w: (0, (2 ** 30, w.strides[1], w.strides[2]), 2),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_ex_refusals_return_status_3_and_write_nothing(lib, name):
    H, W, ci, co = 4, 16, 64, 64
    wout = Win((2, 2 * H, 2 * W, co), 20, 8, SENT)
    off, strides, B = REFUSALS[name](wout)
    assert B * strides[0] > 2 ** 31 - 1 or name != "batch_stride_past_32_bit_offsets"
    x, _, wt = _deconv_ops("exact", (B, H, W, ci, co), 5)
    xd, wd = dev(x), dev(wt)
    ptr = C.c_void_p(wout.args()[0].value + off)
    rc = lib.depgan_op_deconv2x2_ex(P(xd), P(wd), None, None, None, ptr, *strides, B, H, W, ci, co, 1, None)
    torch.cuda.synchronize()
    assert rc == 3 and lib.depgan_last_error()
    assert wout.unchanged()
    # the control: the same call with the window's own pointer and strides is taken
    assert lib.depgan_op_deconv2x2_ex(P(xd), P(wd), None, None, None, *wout.args(), B, H, W, ci, co, 1, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(wout.read(), np.maximum(fr.deconv2x2(x, wt), 0)) and wout.outside_unchanged()
