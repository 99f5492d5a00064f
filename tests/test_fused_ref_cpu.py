"""CPU: (1) the exact-operand method of tests/fused_ref.py proved rather than assumed -- with its operand ranges every
stage of the fused-epilogue contract, in both affine forms, through the Winograd transforms and through the weight
gradient, has the same bits in float32 as in float64, and the magnitude bounds the argument rests on hold at the
largest K of the GPU case table; (2) the argument checks of the three operator entries of
tests/test_gpu_fused_ops.py, which come before any HIP call."""
import ctypes as C
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_ref as fr  # noqa: E402
from test_winograd_cpu import AT, BT, G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["depgan_op_conv2d_fused", "depgan_op_deconv2x2_igemm", "depgan_op_conv2d_wgrad_ex"]
FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments

# the largest contractions of the GPU case table: 3x3 at 224 input channels, 5x5 at 32, and the backward-data form
LARGEST = [(1, 12, 10, 224, 32, 3, False), (2, 9, 11, 32, 32, 5, False), (1, 10, 12, 32, 224, 3, True)]
ALL = dict(bias=True, affine=True, film=True, relu=True, res=True, mask=True, acc=True)


def same_bits(a32, a64):
    return a32.dtype == np.float32 and np.array_equal(a32.astype(np.float64), a64)


def test_exact_operands_every_stage_has_the_same_bits_in_float32_and_float64():
    for i, (B, H, W, ci, co, k, bwd) in enumerate(LARGEST):
        for feats in (ALL, dict(ALL, relu=False), dict(bias=True, affine=True, relu=True, head=True)):
            o = fr.make_ops("exact", np.random.default_rng(i), B, H, W, ci, co, k, bwd=bwd, **feats)
            r64 = fr.reference(o, np.float64, "direct")
            assert np.abs(r64["acc"]).max() <= 2 * k * k * (co if bwd else ci) <= fr.ACC_BOUND
            assert fr.bounds_hold(r64["stages"])
            for form in ("direct", "mfma"):          # two roundings (epilogue.h) and one FMA (igemm_epilogue.inc)
                r32 = fr.reference(o, np.float32, form)
                assert len(r32["stages"]) == len(r64["stages"])
                for s32, s64 in zip(r32["stages"], r64["stages"]):
                    assert same_bits(s32, s64)
                for key in ("out_pre", "out", "pool", "head"):
                    if key in r64:
                        assert same_bits(r32[key], r64[key]), (key, form)
            # the MFMA form's constant bias * scale + shift and product acc * scale are exact too: the FMA rounds nothing
            c64 = o.bias.astype(np.float64) * o.scale + o.shift
            assert same_bits((o.bias * o.scale).astype(np.float32) + o.shift, c64)
            assert fr.bounds_hold([c64, r64["acc"] * o.scale.astype(np.float64)])


def test_negative_shift_makes_every_output_negative_and_stays_exact():
    for kind in ("exact", "real"):
        o = fr.make_ops(kind, np.random.default_rng(3), 2, 8, 6, 8, 32, 3, bias=True, neg=True)
        r = fr.reference(o, np.float64)
        assert r["out"].max() < 0 and r["pool"].max() < 0
        if kind == "exact":
            assert fr.bounds_hold(r["stages"])


def winograd32(x, w):
    """F(2x2, 3x3) of test_winograd_cpu.py with EVERY operation in float32: panel G g G^T, input transform B^T d B, the
    sixteen products summed over the channels, the two halves of the output transform."""
    f = np.float32
    g, bt, at = G.astype(f), BT.astype(f), AT.astype(f)
    H, W, Cc = x.shape
    K = w.shape[3]
    xp = np.zeros((H + 2, W + 2, Cc), f)
    xp[1:-1, 1:-1] = x
    U = np.einsum("ai,ijck,bj->abck", g, w.astype(f), g).astype(f).reshape(16, Cc, K)
    th, tw = H // 2, W // 2
    d = np.stack([[xp[i:i + H:2, j:j + W:2][:th, :tw] for j in range(4)] for i in range(4)])
    V = np.einsum("ai,ijtuc,bj->abtuc", bt, d, bt).astype(f).reshape(16, th, tw, Cc)
    M = np.stack([V[q].reshape(-1, Cc).dot(U[q]).reshape(th, tw, K) for q in range(16)]).astype(f).reshape(4, 4, th, tw, K)
    Z = np.einsum("qb,abtuk->aqtuk", at, M).astype(f)
    Y = np.einsum("pa,aqtuk->pqtuk", at, Z).astype(f)
    out = np.zeros((H, W, K), f)
    for p in range(2):
        for q in range(2):
            out[p::2, q::2] = Y[p, q]
    assert U.dtype == V.dtype == M.dtype == Y.dtype == f
    # the intermediates the argument names: multiples of 1/4 below 2^22
    for s in (U, V, M, Z, Y):
        assert np.abs(s).max() < 2.0 ** 22 and np.array_equal(s * 4, np.round(s * 4))
    return out


def test_exact_operands_through_the_winograd_transforms_in_float32_equal_the_direct_float64_convolution():
    for bwd in (False, True):
        o = fr.make_ops("exact", np.random.default_rng(7), 1, 8, 12, 32 if bwd else 224, 224 if bwd else 32, 3, bwd=bwd)
        w = np.ascontiguousarray(o.w[::-1, ::-1].transpose(0, 1, 3, 2)) if bwd else o.w    # flipped, roles swapped
        y = winograd32(o.x[0], w)
        assert same_bits(y, fr.conv_acc(o.x, o.w, int(bwd))[0])


def test_exact_operands_are_exact_in_bf16_and_through_the_weight_gradient():
    o = fr.make_ops("exact", np.random.default_rng(9), 3, 22, 18, 48, 40, 3, **ALL)
    for a in (o.x, o.w):
        assert np.array_equal(fr.bf16_round(a), a)           # the bf16 and split pipes multiply the same numbers
    dy = np.random.default_rng(10).integers(-2, 3, (3, 22, 18, 40)).astype(np.float32)
    dy[2] = np.random.default_rng(11).integers(-8, 9, dy[2].shape) * 64.0      # the "large" samples beyond colB
    assert np.array_equal(fr.bf16_round(dy), dy)
    g64, g32 = fr.wgrad(o.x, dy, 3), fr.wgrad(o.x, dy, 3, torch.float32)
    assert same_bits(g32, g64)
    scaled = g64 * o.scale.astype(np.float64) + 0.125
    assert np.abs(scaled).max() < 2.0 ** 21 and np.array_equal(scaled * 8, np.round(scaled * 8))   # 24 bits
    assert same_bits((g32 * o.scale).astype(np.float32) + np.float32(0.125), scaled)
    col = dy[:2].astype(np.float64).sum(axis=(0, 1, 2))
    assert same_bits(dy[:2].sum(axis=(0, 1, 2), dtype=np.float32), col)


def test_float32_chain_equals_float64_where_both_are_exact_and_rounds_once_per_step_elsewhere():
    o = fr.make_ops("exact", np.random.default_rng(5), 2, 6, 8, 16, 32, 3, **ALL)
    pre = fr.reference(o)["out_pre"]
    out32, _ = fr.post_chain(pre.astype(np.float32), o, np.float32)
    out64, _ = fr.post_chain(pre, o, np.float64)
    assert same_bits(out32, out64)
    # real operands: the chain rounds after the FiLM multiply AND after the add -- a contracted FMA gives other bits
    o = fr.make_ops("real", np.random.default_rng(6), 2, 6, 8, 16, 32, 3, film=True)
    pre = np.random.default_rng(8).standard_normal((2, 6, 8, 32)).astype(np.float32)
    out32, _ = fr.post_chain(pre, o)
    fma = (pre.astype(np.float64) * o.fmul[:, None, None, :] + o.fadd[:, None, None, :]).astype(np.float32)
    assert out32.dtype == np.float32 and (out32 != fma).any()
    assert np.abs(out32 - fma).max() <= np.abs(fma).max() * 2.0 ** -23


def test_entries_are_exported_declared_and_bound(lib):
    from dep_gan_im_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    declared = set(re.findall(r"\b(depgan_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in _lib.EXPORTS and name in declared, name
        assert getattr(lib, name).argtypes, name
    assert "DEPGAN_ABI_VERSION 3" in hdr                      # a new entry point is not a new ABI


def test_operators_refuse_null_and_non_positive_arguments_before_any_hip_call(lib):
    s = (64 * 32, 8 * 32, 32)
    N = (None, 0, 0, 0)

    def conv(i=FAKE, w=FAKE, o=FAKE, B=1, H=8, W=8, ci=32, co=32, k=3, os_=s, scale=None, shift=None, fm=None, fa=None,
             ld=32, pre=N, res=N, mask=N, pool=N, hw=None, hb=None, ho=None, skip=0, path=1):
        return lib.depgan_op_conv2d_fused(i, *s, w, None, scale, shift, fm, fa, ld, o, *os_, *pre, *res, *mask, *pool,
                                          hw, hb, ho, 0, skip, B, H, W, ci, co, k, 1, 0, path, 0, None)
    for kw in ({"i": None}, {"w": None}, {"o": None}, {"B": 0}, {"H": 0}, {"W": -1}, {"ci": 0}, {"co": 0}, {"k": 2},
               {"k": 7}, {"os_": (0, 0, 0)}, {"scale": FAKE}, {"shift": FAKE}, {"fm": FAKE}, {"fa": FAKE},
               {"fm": FAKE, "fa": FAKE, "ld": 16}, {"pre": (FAKE, 0, 8, 32)}, {"res": (FAKE, 64, 0, 32)},
               {"mask": (FAKE, 64, 8, 0)}, {"pool": (FAKE, -1, 8, 32)}, {"hw": FAKE}, {"hw": FAKE, "hb": FAKE},
               {"ho": FAKE}, {"skip": 1}, {"path": 0}, {"path": 9}):
        assert conv(**kw) == 1, kw
        assert lib.depgan_last_error()
    # what the chosen kernel does not cover: status 3, still before any HIP call
    assert conv(ci=6, path=1) == 3 and conv(co=16, path=6) == 3 and conv(k=5, path=8) == 3 and conv(H=7, path=8) == 3
    assert conv(co=16, path=3) == 3 and conv(co=16, path=7) == 3

    def dec(form=0, i=FAKE, w=FAKE, o=FAKE, B=1, H=8, ci=64, co=64, bias=None, scale=None, shift=None, mask=N, relu=0,
            path=1):
        return lib.depgan_op_deconv2x2_igemm(form, i, *s, w, bias, scale, shift, o, 4 * 64 * 64, 16 * 64, 64, *mask,
                                             B, H, 8, ci, co, relu, path, None)
    for kw in ({"i": None}, {"w": None}, {"o": None}, {"B": 0}, {"H": 0}, {"ci": 0}, {"co": -1}, {"form": 3}, {"form": -1},
               {"path": 2}, {"scale": FAKE}, {"mask": (FAKE, 64, 8, 32)}, {"form": 1, "bias": FAKE}, {"form": 2, "relu": 1},
               {"form": 1, "mask": (FAKE, 0, 8, 32)}):
        assert dec(**kw) == 1, kw
        assert lib.depgan_last_error()
    assert dec(path=8) == 3 and dec(ci=6) == 3 and dec(form=1, co=6) == 3 and dec(form=1, co=40, ci=64) == 3

    def wg(x=FAKE, dy=FAKE, dw=FAKE, B=2, H=8, ci=32, co=32, k=3, xs=s, colB=0, cscale=None, cout=None, craw=None, bf16=0):
        return lib.depgan_op_conv2d_wgrad_ex(x, *xs, dy, *s, None, dw, None, 0, 0, colB, cscale, cout, craw, B, H, 8, ci,
                                             co, k, bf16, None)
    for kw in ({"x": None}, {"dy": None}, {"dw": None}, {"B": 0}, {"H": 0}, {"ci": 0}, {"co": 0}, {"k": 4},
               {"xs": (64, 8, 0)}, {"bf16": 2}, {"colB": 1}, {"cscale": FAKE}, {"cout": FAKE}, {"cout": FAKE, "colB": 3},
               {"craw": FAKE, "colB": -1}):
        assert wg(**kw) == 1, kw
        assert lib.depgan_last_error()
    assert wg(ci=2, bf16=1) == 3 and wg(co=6, bf16=1) == 3
