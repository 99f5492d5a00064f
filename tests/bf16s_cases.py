"""The case table of tests/test_gpu_bf16s_exact.py and the operands of every case, numpy only: shared with
tests/test_bf16s_ref_cpu.py, which proves on the CPU that the exact operands are exact for every case listed here and
that the table covers COVERAGE.  Shapes are the smallest at which each mechanism of the bf16-storage kernels is still
exercised: pixel tiles are 16 x 16 (a wave owns 4 rows), channel tiles 32, K chunks 32.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_ref as fr  # noqa: E402

# ---- depgan_op_conv2d_bf16s / _head_bf16s / _film_train_bf16s -------------------------------------------------------
# feature sets: make_ops keywords + pool, head (1: stored output, 2: skip_out)
FEATS = {
    "bias": dict(bias=1),
    "affine_relu": dict(bias=1, affine=1, relu=1),
    "film": dict(bias=1, affine=1, film=1, relu=1, res=1),
    "res": dict(bias=1, affine=1, relu=1, res=1),
    "pool": dict(bias=1, affine=1, relu=1, pool=1),
    "film_pool": dict(bias=1, affine=1, film=1, relu=1, res=1, pool=1),
    "negpool": dict(bias=1, neg=1, pool=1),
    "head": dict(bias=1, affine=1, relu=1, head=1),
    "head_skip": dict(bias=1, affine=1, relu=1, head=2),
    "film_head": dict(bias=1, affine=1, film=1, relu=1, res=1, head=1),
}
TILE = (2, 16, 16, 32, 32, 3)          # one exact tile
RAGGED = (2, 21, 19, 40, 96, 3)        # ragged in both directions, a K tail, three channel tiles
RAGGED_EVEN = (2, 22, 18, 40, 96, 3)   # its pooled form
CIN8 = (2, 22, 18, 8, 32, 3)
K224 = (1, 16, 16, 224, 64, 3)         # the largest K inside fused_ref.ACC_BOUND
# item order (igemm_bf16_main.inc): a pixel-tile count that is a multiple of 8 takes the XCD-aware order (RAGGED, CIN8: 8
# tiles), any other the plain one -- REMAP has 18 tiles: more than 8 and no multiple of 8
REMAP = (3, 33, 31, 8, 32, 3)
REMAP_EVEN = (3, 34, 30, 8, 32, 3)     # 18 pixel tiles as well
ONE_A = (2, 21, 19, 48, 96, 1)
ONE_B = (2, 22, 18, 128, 32, 1)
HEAD_A = (2, 21, 19, 32, 32, 3)

# (feature, shape, view): view "" = every operand a window with its own pitch; "in_sB0" / "res_sB0": that view has
# sample stride 0 (ONE sample read for every batch index) while the FiLM rows stay per sample
CONV_CASES = [("bias", s, "") for s in (TILE, RAGGED, CIN8, REMAP, ONE_A)] + \
             [("affine_relu", s, "") for s in (RAGGED, K224)] + \
             [("film", s, "") for s in (TILE, RAGGED, K224, REMAP, ONE_A)] + \
             [("res", s, "") for s in (RAGGED, CIN8)] + \
             [("pool", s, "") for s in (TILE, CIN8, RAGGED_EVEN, ONE_B)] + \
             [("film_pool", s, "") for s in (RAGGED_EVEN, K224, REMAP_EVEN)] + \
             [("negpool", CIN8, "")] + \
             [("film", RAGGED, "in_sB0"), ("film", RAGGED, "res_sB0")]
HEAD_CASES = [("head", HEAD_A, ""), ("head", CIN8, ""), ("head_skip", HEAD_A, ""), ("head_skip", CIN8, ""),
              ("film_head", CIN8, "")]
TRAIN_CASES = [(2, 16, 16, 32, 32), (2, 21, 19, 40, 96), (1, 16, 16, 224, 64)]        # B, H, W, Cin, Cout; 3x3
DECONV_CASES = [(2, 8, 8, 64, 64), (2, 12, 20, 64, 96), (1, 9, 7, 8, 32)]           # B, H, W, Cin, Cout
EDGE_CASES = [(B, H, W, ci, co) for (B, H, W) in ((2, 21, 19), (1, 16, 16), (1, 5, 3)) for ci in (1, 2)
              for co in (8, 16, 24, 32)]
# B, H, W, Cin of dx, Cout of dy, res, mask
BWD_CASES = [s + (r, m) for s in ((1, 16, 16, 32, 32), (3, 21, 19, 96, 128), (2, 22, 18, 64, 40)) for r in (0, 1)
             for m in (0, 1)]
BWD_DECONV_CASES = [s + rm for s in ((2, 8, 8, 64, 64), (2, 6, 10, 96, 64)) for rm in ((0, 0), (1, 1))]
# B, H, W, Cin, Cout, KS, oi, grid (dy = that (1, 2, 2)-strided grid of a (2H, 2W) buffer), colsum
WGRAD_CASES = [s + (c,) for s in ((3, 22, 18, 48, 40, 3, 0, None), (2, 21, 19, 8, 4, 3, 1, None),
                                  (2, 12, 10, 64, 96, 1, 1, (1, 0))) for c in (0, 1)]
UNPOOL_CASES = [s + (k,) for s in ((3, 9, 7, 32), (2, 4, 6, 8)) for k in (0, 1)]     # B, Ho, Wo, C, skip
REFUSALS = ["pointer_8_bytes_off", "row_stride_not_multiple_of_8", "pool_odd_h", "head_cout_64", "ks_5", "cin_12",
            "film_mul_without_add", "gathered_cout_not_multiple_of_32"]

# what the table must hold (the issue's coverage list); test_bf16s_ref_cpu.py::test_the_case_table_covers_the_coverage_list
COVERAGE = {
    "conv_feats": ["bias", "affine_relu", "film", "res", "pool", "film_pool", "negpool"],
    "conv_shapes": [TILE, RAGGED, CIN8, K224, REMAP, ONE_A, ONE_B],
    "conv_views": ["in_sB0", "res_sB0"],
    "head_feats": ["head", "head_skip"],
    "head_shapes": [HEAD_A, CIN8],
    "train_shapes": [(2, 16, 16, 32, 32), (2, 21, 19, 40, 96), (1, 16, 16, 224, 64)],
    "deconv_shapes": [(2, 8, 8, 64, 64), (2, 12, 20, 64, 96), (1, 9, 7, 8, 32)],
    "edge_cin": [1, 2], "edge_cout": [8, 16, 24, 32], "edge_sizes": [(2, 21, 19), (1, 16, 16), (1, 5, 3)],
    "bwd_shapes": [(1, 16, 16, 32, 32), (3, 21, 19, 96, 128), (2, 22, 18, 64, 40)],
    "bwd_deconv_shapes": [(2, 8, 8, 64, 64), (2, 6, 10, 96, 64)],
    "wgrad_shapes": [(3, 22, 18, 48, 40, 3), (2, 21, 19, 8, 4, 3), (2, 12, 10, 64, 96, 1)],
    "unpool_shapes": [(3, 9, 7, 32), (2, 4, 6, 8)],
    "refusals": ["pointer_8_bytes_off", "row_stride_not_multiple_of_8", "pool_odd_h", "head_cout_64", "ks_5", "cin_12",
                 "film_mul_without_add", "gathered_cout_not_multiple_of_32"],
}


def cid(c):
    return "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in c if p != "")


# ---- operands -------------------------------------------------------------------------------------------------------
def conv_ops(case, kind):
    """Operands of one conv / head / train case: (ops, pool, head).  With a view of sample stride 0 that operand holds
    ONE sample, repeated in `ops` for the references."""
    feat, shape, view = case
    B, H, W, ci, co, k = shape
    f = dict(FEATS[feat])
    pool, head = f.pop("pool", 0), f.pop("head", 0)
    rng = np.random.default_rng(sum(shape) * 131 + 7 * len(feat) + len(view))
    o = fr.make_ops_bf16s(kind, rng, B, H, W, ci, co, k, head=bool(head), head_tanh=(kind == "real"), **f)
    if view == "in_sB0":
        o.x = np.repeat(o.x[:1], B, axis=0)
    if view == "res_sB0":
        o.res = np.repeat(o.res[:1], B, axis=0)
    return o, pool, head


def affine_ops(kind, co, seed):
    """bias, scale, shift of the transposed and the edge convolution (with ReLU)"""
    return fr.make_ops(kind, np.random.default_rng(seed), 1, 1, 1, 8, co, 1, bias=1, affine=1, relu=1)


def deconv_ops(case, kind):
    B, H, W, ci, co = case
    rng = np.random.default_rng(ci + 3 * co + H)
    ex = kind == "exact"
    x = rng.integers(-2, 3, (B, H, W, ci)).astype(np.float32) if ex else fr.rne_bf16(rng.standard_normal((B, H, W, ci)).astype(np.float32))
    wt = (rng.integers(-1, 2, (2, 2, co, ci)) if ex else rng.standard_normal((2, 2, co, ci)) / np.sqrt(ci)).astype(np.float32)
    return x, wt, affine_ops(kind, co, H + co)


def edge_ops(case, kind):
    B, H, W, ci, co = case
    rng = np.random.default_rng(100 * H + 10 * ci + co)
    ex = kind == "exact"
    x = (rng.integers(-2, 3, (B, H, W, ci)) if ex else rng.standard_normal((B, H, W, ci))).astype(np.float32)
    w = (rng.integers(-1, 2, (3, 3, ci, co)) if ex else rng.standard_normal((3, 3, ci, co)) / 3.0).astype(np.float32)
    return x, w, affine_ops(kind, co, W + co)


def bwd_ops(case, kind):
    """make_ops(bwd=1): o.x is dy (Cout channels), o.w HWIO (Cin, Cout), o.res / o.mask have Cin channels."""
    B, H, W, ci, co, res, mask = case
    rng = np.random.default_rng(ci * 100 + co + H + 2 * res + mask)
    o = fr.make_ops_bf16s(kind, rng, B, H, W, ci, co, 3, res=bool(res), mask=bool(mask), bwd=True)
    if kind == "real":
        o.x = rng.standard_normal(o.x.shape).astype(np.float32)     # dy is fp32, rounded while staged: not a stored tensor
        if o.res is not None:
            o.res = rng.standard_normal(o.res.shape).astype(np.float32)
    return o


def bwd_deconv_ops(case, kind):
    """dy (B, 2H, 2W, Cout), w (2, 2, Cout, Cin), res and mask (B, H, W, Cin) or None"""
    B, H, W, ci, co, res, mask = case
    rng = np.random.default_rng(ci * 10 + co + W + res)
    ex = kind == "exact"
    dy = (rng.integers(-2, 3, (B, 2 * H, 2 * W, co)) if ex else rng.standard_normal((B, 2 * H, 2 * W, co))).astype(np.float32)
    wt = (rng.integers(-1, 2, (2, 2, co, ci)) if ex else rng.standard_normal((2, 2, co, ci)) / np.sqrt(ci)).astype(np.float32)
    r = m = None
    if res:
        r = ((rng.integers(-32, 33, (B, H, W, ci)) / 8.0) if ex else rng.standard_normal((B, H, W, ci))).astype(np.float32)
    if mask:
        m = rng.choice(fr.MASKS_BF16, (B, H, W, ci)).astype(np.float32)
    return dy, wt, r, m


def wgrad_ops(case, kind):
    """x (B, H, W, Cin) bf16-valued, dyf the fp32 buffer dy is a view of, dy that view"""
    B, H, W, ci, co, k, oi, grid, colsum = case
    rng = np.random.default_rng(ci * 100 + co + k + B)
    ex = kind == "exact"
    gen = (lambda s: rng.integers(-2, 3, s).astype(np.float32)) if ex else (lambda s: rng.standard_normal(s).astype(np.float32))
    x = gen((B, H, W, ci))
    if not ex:
        x = fr.rne_bf16(x)
    dyf = gen((B, 2 * H, 2 * W, co) if grid else (B, H, W, co))
    dy = dyf[:, grid[0]::2, grid[1]::2] if grid else dyf
    return x, dyf, dy


def unpool_ops(case):
    """Small integers: a in [-1, 2] has equal maxima in most windows."""
    B, Ho, Wo, Cc, skip = case
    rng = np.random.default_rng(Ho * 10 + Cc + skip)
    a = rng.integers(-1, 3, (B, 2 * Ho, 2 * Wo, Cc)).astype(np.float32)
    dpool = rng.integers(-4, 5, (B, Ho, Wo, Cc)).astype(np.float32)
    sk = (rng.integers(-16, 17, (B, 2 * Ho, 2 * Wo, Cc)) / 8.0).astype(np.float32) if skip else None
    return dpool, a, sk
