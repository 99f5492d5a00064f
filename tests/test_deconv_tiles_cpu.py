"""CPU: what tests/test_gpu_deconv_tiles.py rests on.

(1) The fused forward transposed-convolution kernel (csrc/deconv_fwd.hip) folds its affine epilogue into the
contraction: it computes sum_k (s w_k) x_k + (b s + t), with the constant as the start value of the accumulators, not
(sum_k w_k x_k + b) s + t.  On the exact operand sets of tests/fused_ref.py every stage of THAT form -- the scaled weights,
every partial sum in any K order, the constant -- is a multiple of fused_ref.QUANTUM below fused_ref.VALUE_BOUND at
K = 128, the largest Cin the kernel takes: no float32 operation rounds, and the float32 evaluation equals the float64
evaluation of the contract as it is written.  That is what lets the GPU test ask for np.array_equal.

(2) The case builder tests/deconv_tile_cases.py is a pure function of the grid: for the grids of several devices it
yields whole batches that reach every loop form the GPU file exists for.

(3) The two entries refuse on their arguments before any HIP call.
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deconv_tile_cases as dc  # noqa: E402
import fused_ref as fr  # noqa: E402
from test_gpu_fused_ops import _deconv_ops  # noqa: E402

FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments
K = 128


def kernel_k_order(cin):
    """The order in which a lane of the kernel meets the channels: k-step s of K group q multiplies channels
    8 q + s and 8 q + 4 + s (the two halves of the 32x32x2 MFMA's K pair)."""
    return np.array([8 * q + 4 * h + s for q in range(cin // 8) for s in range(4) for h in range(2)])


def folded_stages(x, wt, o, order, dt):
    """sum (s w) x + (b s + t) in dtype dt, the constant first and the products added in `order`: (result
    [P][4 Cout], list of stages).  x: (P, Cin); wt: (2, 2, Cout, Cin)."""
    co, ci = wt.shape[2], wt.shape[3]
    one = np.ones(co, dt)
    s = one if o.scale is None else o.scale.astype(dt)
    b = 0 * one if o.bias is None else o.bias.astype(dt)
    t = 0 * one if o.scale is None else o.shift.astype(dt)
    sw = (wt.astype(dt) * s[None, None, :, None]).astype(dt).reshape(4 * co, ci)
    bs = (b * s).astype(dt)
    const = np.tile((bs + t).astype(dt), 4)
    prod = (x.astype(dt)[:, None, order] * sw[None, :, order]).astype(dt)                 # [P][4 Cout][K]
    part = np.cumsum(np.concatenate([np.broadcast_to(const[None, :, None], prod.shape[:2] + (1,)), prod], axis=2),
                     axis=2, dtype=dt)
    assert part.dtype == dt and prod.dtype == dt
    return part[:, :, -1], [sw, bs, const, prod, part]


def test_folded_affine_is_exact_on_the_exact_operands_in_every_k_order():
    rng = np.random.default_rng(2)
    orders = [np.arange(K), kernel_k_order(K), np.arange(K)[::-1], rng.permutation(K)]
    assert sorted(orders[1].tolist()) == list(range(K)) and orders[1][:4].tolist() == [0, 4, 1, 5]
    for co, feats in ((128, dict(bias=1, affine=1, relu=1)), (64, dict(bias=1)), (192, dict())):
        x, _, wt = _deconv_ops("exact", (1, 4, 16, K, co), K + co)
        o = fr.make_ops("exact", np.random.default_rng(co), 1, 1, 1, K, co, 1, **feats)
        xf = x.reshape(-1, K)
        direct = fr.affine(fr.deconv2x2(x, wt), o, np.float64)                               # the contract as written
        direct = direct.reshape(1, 4, 2, 16, 2, co).transpose(0, 1, 3, 2, 4, 5).reshape(-1, 4 * co)   # [pixel][tap][co]
        for order in orders:
            r64, st64 = folded_stages(xf, wt, o, order, np.float64)
            r32, st32 = folded_stages(xf, wt, o, order, np.float32)
            assert fr.bounds_hold(st64)
            for a32, a64 in zip(st32, st64):
                assert a32.dtype == np.float32 and np.array_equal(a32.astype(np.float64), a64)
            assert np.array_equal(r64, direct) and np.array_equal(r32.astype(np.float64), direct)
        assert np.abs(direct).max() > 8            # the sums are not trivially small


def test_folded_affine_rounds_on_real_operands():
    """the control: with real operands the folded float32 form differs from float64 (the GPU file compares at TOL there)"""
    x, _, wt = _deconv_ops("real", (1, 4, 16, K, 64), 1)
    o = fr.make_ops("real", np.random.default_rng(1), 1, 1, 1, K, 64, 1, bias=1, affine=1)
    r64, _ = folded_stages(x.reshape(-1, K), wt, o, np.arange(K), np.float64)
    r32, _ = folded_stages(x.reshape(-1, K), wt, o, np.arange(K), np.float32)
    assert (r32.astype(np.float64) != r64).any() and np.abs(r32 - r64).max() < 1e-4 * np.abs(r64).max()


def test_rows_cover_the_six_instantiations_every_grid_y_and_a_small_image():
    assert {dc.instantiation(r) for r in dc.ROWS if r.Cin == r.Cout} == dc.ALL_SIX
    assert {dc.grid_y(r) for r in dc.ROWS} == {1, 2, 3}
    assert {(r.Cin, r.Cout) for r in dc.ROWS if r.Cin != r.Cout} == {(64, 128), (64, 192), (96, 192), (128, 64)}
    assert all(dc.grid_y(r) > 1 or r.Cin == 128 for r in dc.ROWS if r.Cin != r.Cout)
    assert any(r.H * r.W < 32 and r.W < 32 for r in dc.ROWS)
    for r in dc.ROWS:
        assert r.H & (r.H - 1) == 0 and r.W & (r.W - 1) == 0 and r.W >= 8 and r.Cout % 32 == 0
        assert (4 * r.Cout) % (128 * dc.MT[r.Cin]) == 0
        assert dc.BIG_B * 4 * r.H * r.W * r.Cout < 2 ** 31          # the uncapped query is a launch the kernel covers
        assert len(set(n.name for n in dc.ROWS)) == len(dc.ROWS)


def test_case_builder_reaches_every_loop_form_on_every_grid():
    for cus_times_per_cu in (104, 256, 304, 512):
        launches = []
        for r in dc.ROWS:
            gy = dc.grid_y(r)
            for g in (1, 2, 3):                     # the builder itself, for every gridDim.y
                b = dc.batches(cus_times_per_cu, g, r.H, r.W)
                assert b == dc.batches(cus_times_per_cu, g, r.H, r.W)
            gx = cus_times_per_cu // gy
            b = dc.batches(gx, gy, r.H, r.W)
            t = {k: dc.tiles_of(v, r.H, r.W) for k, v in b.items()}
            step = dc.batch_step(r.H, r.W)
            assert all(v % step == 0 and (v * r.H * r.W) % 32 == 0 for v in b.values())
            assert gx < t["one_extra"] <= gx + 2 and dc.trips(t["one_extra"], gx) == (1, 2)
            assert t["two_each"] == 2 * gx and dc.trips(t["two_each"], gx) == (2, 2)
            lo, hi = dc.trips(t["uneven"], gx)
            assert t["uneven"] >= 3 * gx + 1 and t["uneven"] % gx and (lo, hi) == (3, 4)
            assert t["uneven"] <= 3 * gx + 3                                    # and no larger than it has to be
            assert t["uneven"] * 32 <= 50000                   # the largest launch: under 50 k input pixels at the widest grid
            sb = dc.sub_batch(gx, r.H, r.W)
            assert sb % step == 0 and dc.tiles_of(sb, r.H, r.W) <= gx < dc.tiles_of(sb + step, r.H, r.W)
            for name in dc.LAUNCHES:
                launches += [(r, t[name], gx, gy, sliced) for sliced in (0, 1)]
        dc.check_coverage(dc.coverage(launches))
    # the coverage check sees a table that lost a form
    cov = dc.coverage([(r, 2 * 64, 64, dc.grid_y(r), s) for r in dc.ROWS for s in (0, 1)])
    assert cov["two"] == dc.ALL_SIX and not cov["three"] and not cov["uneven"]


def test_entries_refuse_on_their_arguments_before_any_hip_call(lib):
    out = (C.c_long * 4)(-7, -7, -7, -7)

    def plan(B=64, H=4, W=16, ci=64, co=64, o=out):
        return lib.depgan_debug_deconv_fwd_plan(B, H, W, ci, co, o)
    for kw in ({"o": None}, {"B": 0}, {"H": 0}, {"W": -8}, {"ci": 0}, {"co": -64}):
        assert plan(**kw) == 1, kw
        assert lib.depgan_last_error()
    for kw in ({"ci": 32}, {"ci": 80}, {"co": 48}, {"ci": 96, "co": 64}, {"W": 4}, {"W": 24}, {"H": 3}, {"B": 1, "H": 1, "W": 16},
               {"B": 2 ** 20, "H": 64, "W": 64}):
        assert plan(**kw) == 3, kw
        assert lib.depgan_last_error()
    assert list(out) == [-7] * 4                                # a refusal writes nothing

    d = (4 * 4 * 16 * 64, 2 * 16 * 64, 64)                       # dense strides of the (2H, 2W) = (8, 32) grid

    def ex(i=FAKE, w=FAKE, o=FAKE, s=d, B=2, H=4, W=16, ci=64, co=64, bias=None, scale=None, shift=None):
        return lib.depgan_op_deconv2x2_ex(i, w, bias, scale, shift, o, *s, B, H, W, ci, co, 1, None)
    for kw in ({"i": None}, {"w": None}, {"o": None}, {"B": 0}, {"H": 0}, {"W": 0}):
        assert ex(**kw) == 1, kw
    for kw in ({"ci": 32}, {"co": 48}, {"W": 24}, {"B": 1, "H": 1}, {"s": (d[0], d[1], 66)}, {"s": (d[0], d[1] + 2, 64)},
               {"s": (d[0] + 1, d[1], 64)}, {"o": C.c_void_p(0x1004)}, {"i": C.c_void_p(0x1008)},
               {"s": (2 ** 30, d[1], 64)}, {"s": (d[0], 2 ** 29, 64)}, {"s": (d[0], d[1], 32)}, {"s": (d[0], -d[1], 64)},
               {"s": (-d[0], d[1], 64)}):
        assert ex(**kw) == 3, kw
        assert lib.depgan_last_error()
    # weights / bias / scale / shift that are not 16-byte aligned, a scale without its shift: status 1
    for kw in ({"w": C.c_void_p(0x1004)}, {"bias": C.c_void_p(0x1004)}, {"scale": FAKE}, {"scale": FAKE, "shift": C.c_void_p(0x1008)}):
        assert ex(**kw) == 1, kw
