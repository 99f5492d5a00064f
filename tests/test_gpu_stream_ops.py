"""GPU, the stream contract of the stateless entries: every entry of include/depgan.h that takes a `stream` / `hip_stream`
argument, run as a GATED CALL (tests/stream_gate.py) on a non-blocking side stream and compared bit for bit with the same
call on the null stream: device outputs, host outputs and the status.

ONE table: ROWS, a row per entry (some entries have several) with the smallest case of the entry's own test file that
still reaches its real launcher.  tests/test_stream_table_cpu.py holds the table against the header: a new entry fails
there until it gets a row.  `sync` says whether the entry synchronises its stream before it returns (it returns host
values, or frees a device temporary of the call): for the others the gate must still be shut when the call returns.

Poison (stream_gate.In): float data NaN, bf16 storage 0x7FC0; whatever a kernel turns into an address or a bin -- label
codes, the gather index of depgan_data_augment, the set / label volumes of the component and distance entries -- is ZERO.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_gate as sg  # noqa: E402
from stream_gate import STREAM, Case, HostIn, HostOut, In, InOut, Out, PtrTable, Scratch  # noqa: E402

ROWS = []          # (case id, entry name, builder(lib) -> Case)
EXCLUDED = {
    "depgan_op_conv2d_stamps": "a timing aid: its output is per-workgroup clock stamps, which no two runs share",
}
# Entries that report a launcher's plan and enqueue nothing: they take no stream, so they are no rows of this table.
# tests/test_stream_table_cpu.py holds the list against the header (none of them has a stream parameter or a row).
HOST_ONLY = ["depgan_debug_wgrad_plan", "depgan_debug_wgrad_choice", "depgan_debug_conv_choice",
             "depgan_debug_deconv_fwd_plan"]


def row(fn, tag=""):
    def deco(build):
        ROWS.append((fn[len("depgan_"):] + ("-" + tag if tag else ""), fn, build))
        return build
    return deco


def rng_of(name):
    return np.random.default_rng(sum(name.encode()))


def f32(r, *shape):
    return r.standard_normal(shape, dtype=np.float32)


def h16(r, *shape):
    """bf16 storage: the upper halves of float32 normals, as uint16"""
    return (f32(r, *shape).view(np.uint32) >> 16).astype(np.uint16)


def bf(a):
    return In(a, "bf16nan")


def F(n):
    return Out(4 * int(n))


def dense(H, W, Cc):
    return (H * W * Cc, W * Cc, Cc)


NOVIEW = (None, 0, 0, 0)
MFMA = (2, 32, 32, 32, 32, 3)          # B, H, W, Cin, Cout, KS: the MFMA convolutions (paths 1, 3, 6, 7, 8)
DIRECT = (2, 30, 18, 1, 16, 5)         # the direct kernels
DECONV = (4, 8, 8, 64, 64)             # the transposed convolution


# ---------------------------------------------------------------------------------------------------------------------
# convolutions, weight gradients, transposed convolution
# ---------------------------------------------------------------------------------------------------------------------
def _conv2d(shape, path, name):
    B, H, W, ci, co, k = shape
    r = rng_of(name)
    return Case("depgan_op_conv2d", [In(f32(r, B, H, W, ci)), In(f32(r, k, k, ci, co)), In(f32(r, co)), F(B * H * W * co),
                                     B, H, W, ci, co, k, 1, path, STREAM], sync=(path != 2))


for _p, _s in ((1, MFMA), (3, MFMA), (8, MFMA), (2, DIRECT)):
    row("depgan_op_conv2d", "path%d" % _p)(lambda lib, p=_p, s=_s: _conv2d(s, p, "conv2d%d" % p))


@row("depgan_op_conv2d_bwd_data")
def _(lib):
    B, H, W, ci, co, k = MFMA
    r = rng_of("bwd_data")
    return Case("depgan_op_conv2d_bwd_data", [In(f32(r, B, H, W, co)), In(f32(r, k, k, ci, co)), F(B * H * W * ci),
                                              B, H, W, ci, co, k, 1, STREAM], sync=True)


def _wgrad(fn, shape):
    B, H, W, ci, co, k = shape
    r = rng_of(fn)
    return Case(fn, [In(f32(r, B, H, W, ci)), In(f32(r, B, H, W, co)), F(k * k * ci * co), B, H, W, ci, co, k, STREAM],
                sync=True)


row("depgan_op_conv2d_wgrad", "mfma")(lambda lib: _wgrad("depgan_op_conv2d_wgrad", (2, 16, 16, 32, 32, 3)))
row("depgan_op_conv2d_wgrad", "edge")(lambda lib: _wgrad("depgan_op_conv2d_wgrad", DIRECT))
row("depgan_op_conv2d_wgrad_bf16")(lambda lib: _wgrad("depgan_op_conv2d_wgrad_bf16", (2, 16, 16, 32, 32, 3)))


@row("depgan_op_maxpool")
def _(lib):
    B, Ho, Wo, Cc = 2, 5, 7, 8
    return Case("depgan_op_maxpool", [In(f32(rng_of("maxpool"), B, 2 * Ho, 2 * Wo, Cc)), F(B * Ho * Wo * Cc),
                                      B, Ho, Wo, Cc, STREAM], sync=False)


@row("depgan_op_deconv2x2")
def _(lib):
    B, H, W, ci, co = DECONV
    r = rng_of("deconv2x2")
    return Case("depgan_op_deconv2x2", [In(f32(r, B, H, W, ci)), In(f32(r, 2, 2, co, ci)), In(f32(r, co)), In(f32(r, co)),
                                        In(f32(r, co)), F(B * 4 * H * W * co), B, H, W, ci, co, 1, STREAM], sync=False)


@row("depgan_op_deconv2x2_ex")
def _(lib):
    B, H, W, ci, co = DECONV
    Ct = co + 32                           # the first co channels of a wider concat buffer
    r = rng_of("deconv2x2_ex")
    return Case("depgan_op_deconv2x2_ex", [In(f32(r, B, H, W, ci)), In(f32(r, 2, 2, co, ci)), In(f32(r, co)), In(f32(r, co)),
                                           In(f32(r, co)), F(B * 4 * H * W * Ct), *dense(2 * H, 2 * W, Ct), B, H, W, ci, co, 1,
                                           STREAM], sync=False)


@row("depgan_op_deconv2x2_wgrad")
def _(lib):
    B, H, W, ci, co = DECONV
    r = rng_of("deconv2x2_wgrad")
    return Case("depgan_op_deconv2x2_wgrad", [In(f32(r, B, H, W, ci)), In(f32(r, B, 2 * H, 2 * W, co)), F(4 * co * ci),
                                              F(co), B, H, W, ci, co, STREAM], sync=True)


def _fused(shape, path, name, full=False, bwd=0):
    """depgan_op_conv2d_fused on dense views; full: every operand of the epilogue that path 1 takes"""
    B, H, W, ci, co, k = shape
    r = rng_of(name)
    cin_l, cout_l = (co, ci) if bwd else (ci, co)          # channels of `in` and of `out`
    vo = dense(H, W, cout_l)
    a = [In(f32(r, B, H, W, cin_l)), *dense(H, W, cin_l), In(f32(r, k, k, ci, co)), In(f32(r, cout_l))]
    if full:
        a += [In(f32(r, cout_l)), In(f32(r, cout_l)), In(f32(r, B, cout_l)), In(f32(r, B, cout_l)), cout_l,
              F(B * H * W * cout_l), *vo, F(B * H * W * cout_l), *vo, In(f32(r, B, H, W, cout_l)), *vo,
              In(f32(r, B, H, W, cout_l)), *vo, F(B * (H // 2) * (W // 2) * cout_l), *dense(H // 2, W // 2, cout_l)]
    else:
        a += [None, None, None, None, 0, F(B * H * W * cout_l), *vo, *NOVIEW, *NOVIEW, *NOVIEW, *NOVIEW]
    a += [None, None, None, 0, 0, B, H, W, ci, co, k, 1, 0, path, bwd, STREAM]
    return Case("depgan_op_conv2d_fused", a, sync=(path != 2))


row("depgan_op_conv2d_fused", "path1_full")(lambda lib: _fused(MFMA, 1, "fused1", full=True))
row("depgan_op_conv2d_fused", "path1_bwd")(lambda lib: _fused(MFMA, 1, "fused1b", bwd=1))
row("depgan_op_conv2d_fused", "path2")(lambda lib: _fused(DIRECT, 2, "fused2"))
row("depgan_op_conv2d_fused", "path6")(lambda lib: _fused(MFMA, 6, "fused6"))
row("depgan_op_conv2d_fused", "path7")(lambda lib: _fused(MFMA, 7, "fused7"))
row("depgan_op_conv2d_fused", "path8_full")(lambda lib: _fused(MFMA, 8, "fused8", full=True))
row("depgan_op_conv2d_fused", "path9")(lambda lib: _fused((2, 32, 32, 16, 16, 5), 9, "fused9"))
row("depgan_op_conv2d_fused", "path10")(lambda lib: _fused((2, 32, 32, 16, 16, 5), 10, "fused10"))


@row("depgan_op_conv3x3_wino_gathered")
def _(lib):
    B, H, W, ci, co, Ct = 2, 32, 32, 32, 32, 48          # two runs of 16 channels at channels 0 and 32 of a 48-wide buffer
    r = rng_of("gathered")
    return Case("depgan_op_conv3x3_wino_gathered",
                [In(f32(r, B, H, W, Ct)), *dense(H, W, Ct), HostIn(np.array([0, 32], np.int64)), 2,
                 In(f32(r, 3, 3, ci, co)), In(f32(r, co)), F(B * H * W * co), *dense(H, W, co), B, H, W, ci, co, STREAM],
                sync=True)


def _deconv_igemm(form, path):
    B, H, W, ci, co = DECONV
    r = rng_of("deconv_igemm%d" % form)
    if form == 0:
        a = [0, In(f32(r, B, H, W, ci)), *dense(H, W, ci), In(f32(r, 2, 2, co, ci)), In(f32(r, co)), In(f32(r, co)),
             In(f32(r, co)), F(B * 4 * H * W * co), *dense(2 * H, 2 * W, co), *NOVIEW, B, H, W, ci, co, 1, path, STREAM]
    else:
        a = [form, In(f32(r, B, 2 * H, 2 * W, co)), *dense(2 * H, 2 * W, co), In(f32(r, 2, 2, co, ci)), None, None, None,
             F(B * H * W * ci), *dense(H, W, ci), In(f32(r, B, H, W, ci)), *dense(H, W, ci), B, H, W, ci, co, 0, path,
             STREAM]
    return Case("depgan_op_deconv2x2_igemm", a, sync=True)


row("depgan_op_deconv2x2_igemm", "form0")(lambda lib: _deconv_igemm(0, 1))
row("depgan_op_deconv2x2_igemm", "form1_bf16")(lambda lib: _deconv_igemm(1, 3))
row("depgan_op_deconv2x2_igemm", "form2")(lambda lib: _deconv_igemm(2, 1))


def _wgrad_ex(bf16):
    B, H, W, ci, co, k = 2, 16, 16, 32, 32, 3
    r = rng_of("wgrad_ex%d" % bf16)
    return Case("depgan_op_conv2d_wgrad_ex",
                [In(f32(r, B, H, W, ci)), *dense(H, W, ci), In(f32(r, B, H, W, co)), *dense(H, W, co), In(f32(r, co)),
                 F(k * k * ci * co), F(k * k * ci * co), 0, 0, B, None, F(co), F(co), B, H, W, ci, co, k, bf16, STREAM],
                sync=True)


row("depgan_op_conv2d_wgrad_ex", "fp32")(lambda lib: _wgrad_ex(0))
row("depgan_op_conv2d_wgrad_ex", "bf16")(lambda lib: _wgrad_ex(1))


# ---------------------------------------------------------------------------------------------------------------------
# learning-phase-1 operators
# ---------------------------------------------------------------------------------------------------------------------
@row("depgan_op_bn_moments")
def _(lib):
    B, H, W, Cc = 2, 9, 7, 8
    return Case("depgan_op_bn_moments", [In(f32(rng_of("moments"), B, H, W, Cc)), *dense(H, W, Cc), B, H, W, Cc, F(Cc), F(Cc),
                                         0, STREAM], sync=True)


@row("depgan_op_bn_backward")
def _(lib):
    B, H, W, Cc = 2, 9, 7, 8
    r = rng_of("bn_backward")
    var = np.abs(f32(r, Cc)) + 0.5
    return Case("depgan_op_bn_backward",
                [In(f32(r, B, H, W, Cc)), In(f32(r, B, H, W, Cc)), F(B * H * W * Cc), *dense(H, W, Cc), B, H, W, Cc,
                 In(f32(r, Cc)), In(f32(r, Cc)), In(var), 1e-3, 1.0 / (B * H * W), 0.5, F(Cc), F(Cc), 0, STREAM], sync=True)


@row("depgan_op_affine_act")
def _(lib):
    B, H, W, Cc = 2, 9, 7, 8
    r = rng_of("affine_act")
    n = B * H * W * Cc
    return Case("depgan_op_affine_act",
                [In(f32(r, B, H, W, Cc)), F(n), F(n), In(f32(r, B, H, W, Cc)), *dense(H, W, Cc), In(f32(r, Cc)),
                 In(f32(r, Cc)), In(f32(r, B, Cc)), In(f32(r, B, Cc)), Cc, 1, B, H, W, Cc, 12345, 0.25, STREAM], sync=False)


def _labels(r, Pn, Cc, codes):
    lab = r.integers(0, Cc, Pn).astype(np.uint8)
    if codes:
        return None, In(lab, "zero")
    return In(np.eye(Cc, dtype=np.float32)[lab]), None


def _ce(fn, Cc, codes, name, labels=True):
    Pn = 1000
    r = rng_of(name)
    oh, cd = _labels(r, Pn, Cc, codes) if labels else (None, None)
    logits, outs = In(3 * f32(r, Pn, Cc)), [F(Pn * Cc), F(Pn * Cc), F(4)]
    w = HostIn((0.5 + r.random(Cc)).astype(np.float32))
    cen, cnt = HostOut(np.int64, Cc * Cc), HostOut(np.int64, Cc + 3)
    if fn == "depgan_op_softmax_ce4":
        return Case(fn, [logits, oh, *outs, Pn, STREAM], sync=True)
    if fn == "depgan_op_softmax_ce":
        return Case(fn, [logits, oh, cd, *outs, Pn, Cc, STREAM], sync=labels)
    if fn == "depgan_op_softmax_ce_census":
        return Case(fn, [logits, oh, cd, *outs, cen, Pn, Cc, STREAM], sync=True)
    if fn == "depgan_op_softmax_ce_weighted":
        return Case(fn, [logits, oh, cd, w, Cc, -1, *outs, cen, cnt, Pn, Cc, STREAM], sync=True)
    return Case(fn, [logits, oh, cd, w, Cc, -1, 2.0, 0.1, *outs, cen, cnt, Pn, Cc, STREAM], sync=True)


row("depgan_op_softmax_ce4")(lambda lib: _ce("depgan_op_softmax_ce4", 4, False, "ce4"))
row("depgan_op_softmax_ce", "probs_only")(lambda lib: _ce("depgan_op_softmax_ce", 3, False, "ce_p", labels=False))
for _fn in ("depgan_op_softmax_ce", "depgan_op_softmax_ce_census", "depgan_op_softmax_ce_weighted",
            "depgan_op_softmax_ce_focal"):
    for _codes in (False, True):
        row(_fn, "codes" if _codes else "onehot")(lambda lib, fn=_fn, c=_codes: _ce(fn, 3, c, fn + str(c)))


def _label_counts(codes):
    Pn, Cc = 1000, 3
    oh, cd = _labels(rng_of("label_counts"), Pn, Cc, codes)
    return Case("depgan_op_label_counts", [oh, cd, Pn, Cc, -1, HostOut(np.int64, Cc + 3), STREAM], sync=True)


row("depgan_op_label_counts", "onehot")(lambda lib: _label_counts(False))
row("depgan_op_label_counts", "codes")(lambda lib: _label_counts(True))


def _dice(codes):
    Pn, Cc = 1000, 3
    r = rng_of("dice")
    e = np.exp(f32(r, Pn, Cc))
    oh, cd = _labels(r, Pn, Cc, codes)
    return Case("depgan_op_dice_loss",
                [In((e / e.sum(1, keepdims=True)).astype(np.float32)), oh, cd, -1, 2, None, 0, 1.0, 0.5, 1.0,
                 InOut(f32(r, Pn, Cc)), HostOut(np.float64, 3 * Cc), HostOut(np.float32, 1), Pn, Cc, STREAM], sync=True)


row("depgan_op_dice_loss", "onehot")(lambda lib: _dice(False))
row("depgan_op_dice_loss", "codes")(lambda lib: _dice(True))


@row("depgan_op_head_k_fwd")
def _(lib):
    Pn, Cc, K = 100, 32, 3
    r = rng_of("head_k_fwd")
    return Case("depgan_op_head_k_fwd", [In(f32(r, Pn, Cc)), Cc, In(f32(r, Cc, K)), In(f32(r, K)), F(Pn * K), Pn, Cc, K,
                                         STREAM], sync=False)


@row("depgan_op_head_k_bwd")
def _(lib):
    Pn, Cc, K = 100, 32, 3
    r = rng_of("head_k_bwd")
    return Case("depgan_op_head_k_bwd", [In(f32(r, Pn, K)), In(f32(r, Cc, K)), In(f32(r, Pn, Cc)), Cc, F(Pn * Cc), Cc, Pn,
                                         Cc, K, STREAM], sync=False)


@row("depgan_op_head_k_wgrad")
def _(lib):
    Pn, Cc, K = 100, 32, 3
    r = rng_of("head_k_wgrad")
    return Case("depgan_op_head_k_wgrad", [In(f32(r, Pn, Cc)), Cc, In(f32(r, Pn, K)), F(Cc * K), F(K), Pn, Cc, K, 0, STREAM],
                sync=True)


@row("depgan_op_bn_rows_fwd")
def _(lib):
    R, Cc, ld = 3, 32, 1024
    r = rng_of("bn_rows_fwd")
    return Case("depgan_op_bn_rows_fwd",
                [In(f32(r, R, ld)), F(R * ld), R, Cc, ld, In(f32(r, Cc)), In(f32(r, Cc)), 1e-3, 0.99, 1.5,
                 InOut(f32(r, Cc)), InOut(np.abs(f32(r, Cc))), F(Cc), F(Cc), 1, STREAM], sync=False)


@row("depgan_op_bn_rows_bwd")
def _(lib):
    R, Cc, ld = 3, 32, 1024
    r = rng_of("bn_rows_bwd")
    return Case("depgan_op_bn_rows_bwd",
                [In(f32(r, R, ld)), In(f32(r, R, ld)), In(f32(r, R, ld)), F(R * ld), R, Cc, ld, In(f32(r, Cc)),
                 In(f32(r, Cc)), In(np.abs(f32(r, Cc)) + 0.5), F(Cc), F(Cc), STREAM], sync=False)


@row("depgan_op_small_gemm")
def _(lib):
    M, K, N = 3, 32, 32
    r = rng_of("small_gemm")
    return Case("depgan_op_small_gemm", [0, In(f32(r, M, K)), In(f32(r, K, N)), In(f32(r, N)), F(M * N), M, K, N, STREAM],
                sync=False)


# ---------------------------------------------------------------------------------------------------------------------
# the two-critic step's operators and the noise MLP
# ---------------------------------------------------------------------------------------------------------------------
@row("depgan_op_unpool_mask")
def _(lib):
    B, Ho, Wo, Cc = 2, 5, 7, 8
    r = rng_of("unpool")
    full = dense(2 * Ho, 2 * Wo, Cc)
    return Case("depgan_op_unpool_mask",
                [In(f32(r, B, Ho, Wo, Cc)), *dense(Ho, Wo, Cc), In(f32(r, B, 2 * Ho, 2 * Wo, Cc)), *full,
                 In(f32(r, B, 2 * Ho, 2 * Wo, Cc)), *full, F(B * 4 * Ho * Wo * Cc), *full, B, Ho, Wo, Cc, STREAM], sync=False)


@row("depgan_op_gather_pool")
def _(lib):
    B, Ho, Wo, Cc = 2, 5, 7, 8
    r = rng_of("gather_pool")
    full = dense(2 * Ho, 2 * Wo, Cc)
    return Case("depgan_op_gather_pool",
                [In(f32(r, B, 2 * Ho, 2 * Wo, Cc)), *full, In(f32(r, B, 2 * Ho, 2 * Wo, Cc)), *full, F(B * Ho * Wo * Cc),
                 *dense(Ho, Wo, Cc), B, Ho, Wo, Cc, STREAM], sync=False)


@row("depgan_op_head", "fwd")
def _(lib):
    Pn, Cc = 1000, 32
    r = rng_of("head")
    return Case("depgan_op_head", [0, In(f32(r, Pn, Cc)), In(f32(r, Cc)), In(f32(r, 1)), None, F(Pn), Pn, Cc, 1, STREAM],
                sync=False)


@row("depgan_op_head", "bwd")
def _(lib):
    Pn, Cc = 1000, 32
    r = rng_of("headb")
    return Case("depgan_op_head", [1, In(f32(r, Pn, Cc)), In(f32(r, Cc)), None, In(f32(r, Pn)), F(Pn * Cc), Pn, Cc, 0,
                                   STREAM], sync=False)


TAIL = (3, 17, 100)          # N, HW, C


@row("depgan_op_critic_tail_fwd")
def _(lib):
    N, HW, Cc = TAIL
    r = rng_of("tail_fwd")
    return Case("depgan_op_critic_tail_fwd", [In(f32(r, N, HW, Cc)), In(f32(r, Cc)), In(f32(r, 1)), In(f32(r, HW)),
                                              In(f32(r, 1)), F(N * HW), F(N), N, HW, Cc, STREAM], sync=False)


@row("depgan_op_critic_tail_bwd")
def _(lib):
    N, HW, Cc = TAIL
    r = rng_of("tail_bwd")
    return Case("depgan_op_critic_tail_bwd", [In(f32(r, N, HW, Cc)), In(f32(r, Cc)), In(f32(r, HW)), In(f32(r, 1)), N,
                                              F(N * HW * Cc), N, HW, Cc, STREAM], sync=False)


@row("depgan_op_critic_tail_wgrad")
def _(lib):
    N, HW, Cc = TAIL
    r = rng_of("tail_wgrad")
    return Case("depgan_op_critic_tail_wgrad",
                [In(f32(r, N, HW, Cc)), In(f32(r, Cc)), In(f32(r, 1)), In(f32(r, HW)), In(f32(r, 1)), N, 1, 0, F(Cc), F(1),
                 F(HW), F(1), N, HW, Cc, 0, STREAM], sync=True)


@row("depgan_op_colsum")
def _(lib):
    B, H, W, Cc = 1, 10, 10, 4
    r = rng_of("colsum")
    return Case("depgan_op_colsum", [In(f32(r, B, H, W, Cc)), *dense(H, W, Cc), B, H, W, Cc, In(f32(r, Cc)), F(Cc), F(Cc), 0,
                                     None, 0, STREAM], sync=True)


@row("depgan_op_sum")
def _(lib):
    return Case("depgan_op_sum", [In(f32(rng_of("sum"), 1000)), 1000, F(1), 0, STREAM], sync=True)


@row("depgan_op_critic_inputs")
def _(lib):
    B, HW, nicg = 3, 1000, 2
    r = rng_of("critic_inputs")
    return Case("depgan_op_critic_inputs", [In(f32(r, B, HW)), In(f32(r, B, HW, nicg)), nicg, In(f32(r, B, HW)),
                                            In(np.float32([0.0, 1.0, 0.3137])), F(3 * B * HW), B, HW, 0, STREAM], sync=False)


@row("depgan_op_gp_u0")
def _(lib):
    B, HW = 3, 65
    return Case("depgan_op_gp_u0", [In(f32(rng_of("gp_u0"), B, HW)), F(B * HW), F(B), F(1), 10.0, B, HW, 0, STREAM], sync=True)


@row("depgan_op_critic_stats")
def _(lib):
    B = 3
    r = rng_of("critic_stats")
    return Case("depgan_op_critic_stats", [In(f32(r, 2 * B)), In(np.abs(f32(r, B))), F(4), B, STREAM], sync=False)


@row("depgan_op_gloss_sums")
def _(lib):
    Pn, nicg = 1000, 2
    r = rng_of("gloss")
    return Case("depgan_op_gloss_sums", [In(f32(r, Pn, nicg)), nicg, In(f32(r, Pn)), In(np.tanh(f32(r, Pn))), 0.5, F(4), Pn, 0,
                                         STREAM], sync=True)


@row("depgan_op_g_dpre")
def _(lib):
    B, nicg = 3, 2
    Pn = B * 333
    r = rng_of("g_dpre")
    return Case("depgan_op_g_dpre", [In(f32(r, Pn, nicg)), nicg, In(f32(r, Pn)), In(np.tanh(f32(r, Pn))), In(f32(r, Pn)),
                                     In(f32(r, Pn)), F(Pn), B, Pn, STREAM], sync=False)


@row("depgan_op_film_bwd")
def _(lib):
    B, HW, Cc = 2, 63, 12
    r = rng_of("film_bwd")
    return Case("depgan_op_film_bwd", [In(f32(r, B, HW, Cc)), In(f32(r, B, HW, Cc)), In(f32(r, B, Cc)), In(f32(r, B, Cc)), Cc,
                                       F(B * HW * Cc), F(B * Cc), F(B * Cc), B, HW, Cc, 0, STREAM], sync=True)


@row("depgan_op_bn_prepare_batch")
def _(lib):
    r = rng_of("bn_prepare")
    extra, tab, Cs = [], [], [32, 7]
    for j, Cc in enumerate(Cs):
        ins = [In(f32(r, Cc)), In(f32(r, Cc)), In(f32(r, Cc)), In(np.abs(f32(r, Cc)) + 0.01)]
        outs = [F(Cc) for _ in range(3 + j)]              # mean_copy on the second job
        tab += [(len(extra) + i, 0) for i in range(len(ins) + len(outs))] + [None] * (1 - j)
        extra += ins + outs
    return Case("depgan_op_bn_prepare_batch", [PtrTable(tab), HostIn(np.array(Cs, np.int32)), len(Cs), 1e-3, STREAM],
                sync=True, extra=extra)


@row("depgan_op_bn_gamma_grad_batch")
def _(lib):
    r = rng_of("bn_gamma")
    extra, tab, dims = [], [], []
    for oi, K, Cout, Cin in ((0, 100, 7, 1), (1, 9 * 8, 16, 8)):
        ins = [In(f32(r, K * Cout)), In(f32(r, K * Cout)), In(f32(r, Cout)), In(f32(r, Cout)), In(f32(r, Cout)),
               In(f32(r, Cout))]
        tab += [(len(extra) + i, 0) for i in range(7)]
        extra += ins + [F(Cout)]
        dims += [K, Cout, oi, Cin]
    return Case("depgan_op_bn_gamma_grad_batch", [PtrTable(tab), HostIn(np.array(dims, np.int32)), 2, STREAM], sync=True,
                extra=extra)


NCOL = np.array([96, 96, 64, 64, 32, 32, 128, 128, 96, 96, 64, 64, 32, 32], np.int32)     # the generator's 14 FiLM heads


def _noise_params(r):
    return [In(0.2 * f32(r, 1376)), In(0.05 * f32(r, 1024 * 1024)), In(0.2 * f32(r, 5 * 1024)), HostIn(NCOL)]


@row("depgan_op_noise_fwd")
def _(lib):
    B = 3
    r = rng_of("noise_fwd")
    return Case("depgan_op_noise_fwd", [*_noise_params(r), In(f32(r, B, 32)), F(6 * B * 1024), B, STREAM], sync=False)


@row("depgan_op_noise_bwd")
def _(lib):
    B = 3
    r = rng_of("noise_bwd")
    return Case("depgan_op_noise_bwd", [*_noise_params(r), In(f32(r, B, 32)), InOut(f32(r, 6, B, 1024)), In(f32(r, B, 1024)),
                                        F(1248), F(1024 * 1024), F(3072), B, 0, STREAM], sync=True)


@row("depgan_op_best_noise")
def _(lib):
    k, zf = 4, 96
    r = rng_of("best_noise")
    st = np.abs(f32(r, k, 8)) + 1.0
    return Case("depgan_op_best_noise", [In(st), k, In(f32(r, k, zf)), zf, Out(4), F(zf), STREAM], sync=False)


@row("depgan_op_round_bf16_masked")
def _(lib):
    n = 1000
    r = rng_of("round_bf16")
    return Case("depgan_op_round_bf16_masked", [In(f32(r, n)), In((r.random(n) < 0.7).astype(np.uint8)), F(n), n, STREAM],
                sync=False)


@row("depgan_op_grad_sqnorm")
def _(lib):
    return Case("depgan_op_grad_sqnorm", [In(f32(rng_of("sqnorm"), 1000)), 1000, 0.5, HostOut(np.float64, 1), STREAM],
                sync=True)


@row("depgan_op_adam_opts")
def _(lib):
    n = 1000
    r = rng_of("adam_opts")
    return Case("depgan_op_adam_opts",
                [InOut(f32(r, n)), In(f32(r, n)), InOut(f32(r, n)), InOut(np.abs(f32(r, n))), n, 1e-3, 1e-3, 0.5, 0.9, 1e-7,
                 1.0, 1.0, 0.5, 0.01, HostIn(np.array([400, 1000], np.int64)), HostIn(np.array([1, 0], np.int32)), 2,
                 HostOut(np.float64, 2), STREAM], sync=True)


# ---------------------------------------------------------------------------------------------------------------------
# the operators on bf16 activation storage (strides in ELEMENTS, every bf16 view 16-byte aligned)
# ---------------------------------------------------------------------------------------------------------------------
TILE = (2, 16, 16, 32, 32, 3)


def _conv_bf16s(fn):
    B, H, W, ci, co, k = TILE
    r = rng_of(fn)
    vo = dense(H, W, co)
    a = [bf(h16(r, B, H, W, ci)), *dense(H, W, ci), In(f32(r, k, k, ci, co)), In(f32(r, co)), In(f32(r, co)), In(f32(r, co)),
         In(f32(r, B, co)), In(f32(r, B, co)), co, bf(h16(r, B, H, W, co)), *vo, Out(2 * B * H * W * co), *vo]
    if fn == "depgan_op_conv2d_film_train_bf16s":
        return Case(fn, a + [Out(2 * B * H * W * co), Out(B * H * W * co // 8), B, H, W, ci, co, 1, STREAM], sync=True)
    a += [Out(2 * B * (H // 2) * (W // 2) * co), B, H, W, ci, co, k, 1]
    if fn == "depgan_op_conv2d_head_bf16s":
        a[-8] = None                                        # the fused head has no pool
        a += [In(f32(r, co)), In(f32(r, 1)), F(B * H * W), 1, 0]
    return Case(fn, a + [STREAM], sync=True)


for _fn in ("depgan_op_conv2d_bf16s", "depgan_op_conv2d_head_bf16s", "depgan_op_conv2d_film_train_bf16s"):
    row(_fn)(lambda lib, fn=_fn: _conv_bf16s(fn))


@row("depgan_op_deconv2x2_bf16s")
def _(lib):
    B, H, W, ci, co = 2, 8, 8, 64, 64
    r = rng_of("deconv_bf16s")
    return Case("depgan_op_deconv2x2_bf16s",
                [bf(h16(r, B, H, W, ci)), *dense(H, W, ci), In(f32(r, 2, 2, co, ci)), In(f32(r, co)), In(f32(r, co)),
                 In(f32(r, co)), Out(2 * B * 4 * H * W * co), *dense(2 * H, 2 * W, co), B, H, W, ci, co, 1, STREAM], sync=True)


@row("depgan_op_edge_conv_bf16s")
def _(lib):
    B, H, W, ci, co = 1, 16, 16, 1, 8
    r = rng_of("edge_bf16s")
    return Case("depgan_op_edge_conv_bf16s",
                [In(f32(r, B, H, W, ci)), In(f32(r, 3, 3, ci, co)), In(f32(r, co)), In(f32(r, co)), In(f32(r, co)),
                 Out(2 * B * H * W * co), *dense(H, W, co), B, H, W, ci, co, 1, STREAM], sync=False)


@row("depgan_op_head_bf16s")
def _(lib):
    Pn, Cc = 1000, 32
    r = rng_of("head_bf16s")
    return Case("depgan_op_head_bf16s", [bf(h16(r, Pn, Cc)), In(f32(r, Cc)), In(f32(r, 1)), F(Pn), Pn, Cc, 1, STREAM],
                sync=False)


@row("depgan_op_head_softmax_bf16s")
def _(lib):
    Pn, Cc = 1000, 32
    r = rng_of("head_softmax_bf16s")
    return Case("depgan_op_head_softmax_bf16s", [bf(h16(r, Pn, Cc)), Cc, In(f32(r, Cc, 4)), In(f32(r, 4)), F(Pn * 4),
                                                 F(Pn * 4), Pn, Cc, STREAM], sync=False)


@row("depgan_op_head_softmax_k_bf16s")
def _(lib):
    Pn, Cc, K = 1000, 32, 3
    r = rng_of("head_softmax_k_bf16s")
    return Case("depgan_op_head_softmax_k_bf16s", [bf(h16(r, Pn, Cc)), Cc, In(f32(r, Cc, K)), In(f32(r, K)), F(Pn * K),
                                                   F(Pn * K), Pn, Cc, K, STREAM], sync=False)


@row("depgan_op_conv2d_wgrad_bf16s")
def _(lib):
    B, H, W, ci, co, k = 2, 21, 19, 8, 4, 3
    r = rng_of("wgrad_bf16s")
    return Case("depgan_op_conv2d_wgrad_bf16s",
                [bf(h16(r, B, H, W, ci)), *dense(H, W, ci), In(f32(r, B, H, W, co)), *dense(H, W, co), F(k * k * ci * co),
                 F(co), B, H, W, ci, co, k, 1, STREAM], sync=True)


def _bwd_bf16s(deconv):
    B, H, W, ci, co = (2, 8, 8, 64, 64) if deconv else (1, 16, 16, 32, 32)
    r = rng_of("bwd_bf16s%d" % deconv)
    up = 2 if deconv else 1
    vi = dense(H, W, ci)
    w = f32(r, 2, 2, co, ci) if deconv else f32(r, 3, 3, ci, co)
    return Case("depgan_op_conv2d_bwd_data_bf16s",
                [In(f32(r, B, up * H, up * W, co)), *dense(up * H, up * W, co), In(w), In(f32(r, B, H, W, ci)), *vi,
                 bf(h16(r, B, H, W, ci)), *vi, F(B * H * W * ci), *vi, B, H, W, ci, co, deconv, STREAM], sync=True)


row("depgan_op_conv2d_bwd_data_bf16s", "3x3")(lambda lib: _bwd_bf16s(0))
row("depgan_op_conv2d_bwd_data_bf16s", "deconv")(lambda lib: _bwd_bf16s(1))


@row("depgan_op_unpool_mask_bf16s")
def _(lib):
    B, Ho, Wo, Cc = 2, 4, 6, 8
    r = rng_of("unpool_bf16s")
    full = dense(2 * Ho, 2 * Wo, Cc)
    return Case("depgan_op_unpool_mask_bf16s",
                [In(f32(r, B, Ho, Wo, Cc)), *dense(Ho, Wo, Cc), bf(h16(r, B, 2 * Ho, 2 * Wo, Cc)), *full,
                 In(f32(r, B, 2 * Ho, 2 * Wo, Cc)), *full, F(B * 4 * Ho * Wo * Cc), *full, B, Ho, Wo, Cc, STREAM], sync=False)


@row("depgan_op_film_bwd_bf16s")
def _(lib):
    B, HW, Cc = 2, 63, 32
    r = rng_of("film_bwd_bf16s")
    bits = r.integers(0, 256, -(-B * HW * Cc // 8 // 4) * 4).astype(np.uint8)
    return Case("depgan_op_film_bwd_bf16s",
                [In(f32(r, B, HW, Cc)), bf(h16(r, B, HW, Cc)), In(bits), In(f32(r, B, Cc)), Cc, F(B * HW * Cc), F(B * Cc),
                 F(B * Cc), B, HW, Cc, STREAM], sync=True)


@row("depgan_op_head_bwd_bf16s", "wgrad")
def _(lib):
    Pn, Cc = 1000, 32
    r = rng_of("head_bwd_bf16s0")
    return Case("depgan_op_head_bwd_bf16s", [0, bf(h16(r, Pn, Cc)), Cc, None, In(f32(r, Pn)), F(Cc), Pn, Cc, STREAM],
                sync=True)


@row("depgan_op_head_bwd_bf16s", "data")
def _(lib):
    Pn, Cc = 1000, 32
    r = rng_of("head_bwd_bf16s1")
    return Case("depgan_op_head_bwd_bf16s", [1, bf(h16(r, Pn, Cc)), Cc, In(f32(r, Cc)), In(f32(r, Pn)), F(Pn * Cc), Pn, Cc,
                                             STREAM], sync=False)


# ---------------------------------------------------------------------------------------------------------------------
# the data step and the evaluation step
# ---------------------------------------------------------------------------------------------------------------------
VOL = (20, 18, 3)          # X, Y, Z


def _mask01(r, n, p=0.7):
    return (r.random(n) < p).astype(np.float32)


@row("depgan_eval_accumulate")
def _(lib):
    n = 1000
    r = rng_of("eval_acc")
    return Case("depgan_eval_accumulate", [In(f32(r, n)), In(_mask01(r, n)), InOut(r.standard_normal(n)), n, STREAM],
                sync=False)


@row("depgan_eval_divide")
def _(lib):
    return Case("depgan_eval_divide", [InOut(rng_of("eval_div").standard_normal(1000)), 1000, 10.0, STREAM], sync=False)


@row("depgan_eval_counts")
def _(lib):
    n, nicg = 1000, 2
    r = rng_of("eval_counts")
    return Case("depgan_eval_counts",
                [In(r.random((n, nicg)).astype(np.float32)), nicg, In(r.standard_normal(n) * 0.3),
                 In(r.integers(0, 4, n).astype(np.float32), "zero"), In(_mask01(r, n)), In(_mask01(r, n, 0.3)),
                 In(_mask01(r, n)), In(_mask01(r, n, 0.3)), In(r.random(n).astype(np.float32)), n, 0.5,
                 HostOut(np.int64, 20), STREAM], sync=True)


@row("depgan_data_prep_subject")
def _(lib):
    X, Y, Z = VOL
    n, nicg = X * Y * Z, 2
    r = rng_of("prep_subject")
    vols = [In(r.random(n).astype(np.float32)), In(100 * r.random(n).astype(np.float32)), In(_mask01(r, n)),
            In(_mask01(r, n, 0.1)), In(r.random(n).astype(np.float32)), In(_mask01(r, n)), In(_mask01(r, n, 0.1))]
    scratch = max(4, int(lib.depgan_data_prep_scratch_floats(X, Y, Z)))
    return Case("depgan_data_prep_subject", [*vols, X, Y, Z, nicg, F(n * nicg), F(n), Scratch(4 * scratch), STREAM], sync=False)


@row("depgan_data_prep_zscore")
def _(lib):
    X, Y, Z = VOL
    n = X * Y * Z
    r = rng_of("zscore")
    scratch = max(4, int(lib.depgan_data_zscore_scratch_floats(X, Y, Z)))
    return Case("depgan_data_prep_zscore", [In(100 * r.random(n).astype(np.float32)), In(_mask01(r, n)),
                                            In(_mask01(r, n, 0.1)), X, Y, Z, F(n), F(2), Scratch(4 * scratch), STREAM], sync=False)


@row("depgan_data_mask_slices")
def _(lib):
    X, Y, Z = VOL
    n = X * Y * Z
    r = rng_of("mask_slices")
    return Case("depgan_data_mask_slices", [In(f32(r, n)), In(_mask01(r, n)), In(_mask01(r, n, 0.1)), X, Y, Z, F(n), STREAM],
                sync=False)


@row("depgan_labels_to_onehot")
def _(lib):
    n, Cc = 1000, 4
    return Case("depgan_labels_to_onehot", [In(rng_of("onehot").integers(0, Cc, n).astype(np.float32), "zero"), n, Cc,
                                            F(n * Cc), STREAM], sync=True)


@row("depgan_data_augment")
def _(lib):
    n_src, n, H, W, nicg = 3, 2, 9, 7, 1
    r = rng_of("augment")
    params = np.float32([[1, 0, 0.5, 0, 1, -1.25, 1.5, 0.1], [0.9, 0.1, 0, -0.1, 0.9, 1, 1, 0]])
    return Case("depgan_data_augment",
                [In(f32(r, n_src, H, W, nicg)), nicg, In(r.integers(0, 4, (n_src, H, W)).astype(np.uint8), "zero"), 1, 4,
                 In(np.array([2, 0], np.int64), "zero"), n_src, In(params), n, H, W, 1, -1.0, 3, F(n * H * W * nicg),
                 Out(n * H * W), STREAM], sync=False)


@row("depgan_eval_accumulate_channels")
def _(lib):
    n, Cc = 500, 4
    r = rng_of("acc_channels")
    return Case("depgan_eval_accumulate_channels", [In(f32(r, n, Cc)), In(_mask01(r, n)), InOut(r.standard_normal((n, Cc))),
                                                    n, Cc, STREAM], sync=False)


@row("depgan_eval_label_counts")
def _(lib):
    n, Cc = 1000, 4
    r = rng_of("label_counts_eval")
    return Case("depgan_eval_label_counts",
                [In(r.random((n, Cc))), Cc, In(r.integers(0, 4, n).astype(np.float32), "zero"), In(_mask01(r, n)),
                 In(_mask01(r, n, 0.3)), In(_mask01(r, n)), In(_mask01(r, n, 0.3)), n, Out(n), HostOut(np.int64, 18),
                 STREAM], sync=True)


STATS = (1, 6, 5, 3)          # n, H, W, C


@row("depgan_eval_accumulate_stats")
def _(lib):
    n, H, W, Cc = STATS
    npix = n * H * W
    r = rng_of("acc_stats")
    return Case("depgan_eval_accumulate_stats",
                [In(r.random((npix, Cc)).astype(np.float32)), In(_mask01(r, npix)), None, 0, n, H, W, Cc,
                 InOut(np.zeros((npix, Cc))), InOut(np.zeros((npix, Cc))), InOut(np.zeros(npix)),
                 InOut(np.zeros((npix, Cc), np.uint8)), InOut(np.zeros(npix, np.uint8)), STREAM], sync=False)


@row("depgan_eval_finish_stats")
def _(lib):
    n, H, W, Cc = STATS
    npix = n * H * W
    r = rng_of("finish_stats")
    return Case("depgan_eval_finish_stats",
                [InOut(r.random((npix, Cc)) * 3), InOut(r.random((npix, Cc)) * 9 + 1), InOut(-r.random(npix)),
                 In(r.integers(0, 4, npix).astype(np.uint8), "zero"), Out(8 * npix), Out(8 * npix), npix, Cc, 3, 1,
                 STREAM], sync=False)


BOX = (3, 10, 12)          # D, H, W


def _set(r):
    return (r.random(BOX) < 0.3).astype(np.uint8)


@row("depgan_eval_surface_mask")
def _(lib):
    D, H, W = BOX
    return Case("depgan_eval_surface_mask", [In(_set(rng_of("surface_mask")), "zero"), D, H, W, 0, Out(D * H * W), STREAM],
                sync=False)


@row("depgan_eval_edt_sq")
def _(lib):
    D, H, W = BOX
    scratch = max(8, int(lib.depgan_eval_edt_scratch_bytes(D, H, W)))
    return Case("depgan_eval_edt_sq", [In(_set(rng_of("edt")), "zero"), D, H, W, 4.0, 1.0, 1.0, Out(8 * D * H * W),
                                       Scratch(scratch), STREAM], sync=False)


@row("depgan_eval_surface_sums")
def _(lib):
    n = BOX[0] * BOX[1] * BOX[2]
    r = rng_of("surface_sums")
    scratch = max(8, int(lib.depgan_eval_surface_sums_scratch_bytes(n)))
    return Case("depgan_eval_surface_sums", [In(r.integers(0, 50, n).astype(np.float64)), In(_set(r), "zero"), n,
                                             Scratch(scratch), HostOut(np.float64, 4), STREAM], sync=True)


@row("depgan_eval_cc_label")
def _(lib):
    D, H, W = BOX
    scratch = max(8, int(lib.depgan_eval_cc_scratch_bytes(D, H, W)))
    return Case("depgan_eval_cc_label", [In(_set(rng_of("cc_label")), "zero"), D, H, W, 1, 0, Out(4 * D * H * W),
                                         Scratch(scratch), HostOut(np.int64, 1), STREAM], sync=True)


@row("depgan_eval_cc_overlap")
def _(lib):
    n, ncomp = BOX[0] * BOX[1] * BOX[2], 5
    r = rng_of("cc_overlap")
    return Case("depgan_eval_cc_overlap", [In(r.integers(0, ncomp + 1, n).astype(np.int32), "zero"), In(_set(r), "zero"), n,
                                           ncomp, Out(4 * ncomp), Out(4 * ncomp), STREAM], sync=False)


IDS = [r[0] for r in ROWS]
NEGATIVE_CONTROL = ["op_maxpool", "op_conv2d-path1", "op_softmax_ce-onehot"]


# ---------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------
class Table:
    """every row bound to its buffers, the expected (null-stream) snapshots, the measured host-side call durations, the
    gate chosen from them and the one side stream of the module"""

    def __init__(self, lib):
        import torch
        self.bound, self.want, self.secs = {}, {}, {}
        for cid, fn, build in ROWS:
            self.bound[cid] = b = sg.Bound(lib, build(lib))
            self.want[cid], self.secs[cid] = sg.null_run(b)
        self.longest = max(self.secs, key=self.secs.get)
        self.ms = sg.gate_ms(self.secs[self.longest])
        self.gate = sg.Gate(sg.session_delay(), self.ms)
        self.s = torch.cuda.Stream()
        print("stream gate: longest host-side call %s %.3f ms -> gate %.1f ms" %
              (self.longest, 1e3 * self.secs[self.longest], self.ms))


@pytest.fixture(scope="module")
def table(lib):
    return Table(lib)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_entry_enqueues_everything_on_the_stream_it_is_given(table, cid):
    b, want = table.bound[cid], table.want[cid]
    assert int(want[0].view(np.int64)[0]) == 0, "%s: status %d on the null stream" % (cid, int(want[0].view(np.int64)[0]))
    got = sg.gated_run(b, table.gate, table.s)
    assert sg.same(got, want), "%s on a side stream differs from the null stream: %s" % (cid, sg.first_difference(b, got, want))
    bad, ro = b.guards_intact(got)
    assert not bad and not ro, "%s: wrote outside its outputs (guards of buffers %s, read-only buffers %s)" % (cid, bad, ro)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", NEGATIVE_CONTROL)
def test_the_gate_detects_a_call_on_the_wrong_stream(table, cid):
    """The method's own test: the gated call, but the entry is handed the NULL stream.  Its work then runs while the gate
    is shut, on poison: the outputs must differ from the expected bits, or the gate proves nothing."""
    import torch
    b = table.bound[cid]
    b.reset()
    torch.cuda.synchronize()
    e_gate = torch.cuda.Event()
    with torch.cuda.stream(table.s):
        table.gate.delay.enqueue(table.ms)
        e_gate.record(table.s)
        for buf in b.bufs:
            buf.load()
    assert not e_gate.query(), "inconclusive: the gate was open before the call"
    rc, _ = b.call(0)
    table.s.synchronize()
    torch.cuda.synchronize()
    got = b.snapshot(rc)
    assert not sg.same(got, table.want[cid]), "%s on the wrong stream went unnoticed: the gate proves nothing" % cid


def _wrapper_case(table, poisoned, staged, run):
    """a Python wrapper under `with torch.cuda.stream(s)`: the wrapper reads torch's current stream itself"""
    import torch
    want = run()
    torch.cuda.synchronize()
    want = [w.cpu().numpy() for w in want]
    for p in poisoned:
        p.fill_(float("nan") if p.is_floating_point() else 0)

    def load():
        for p, st in zip(poisoned, staged):
            p.copy_(st, non_blocking=True)

    def call():
        with torch.cuda.stream(table.s):
            return run()
    got = table.gate.run(table.s, load, call, False, "wrapper")
    got = [g.cpu().numpy() for g in got]
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))


@pytest.mark.gpu
def test_data_wrapper_follows_torchs_current_stream(table):
    import torch
    from dep_gan_im_amd import data
    X, Y, Z = VOL
    r = rng_of("wrapper_data")
    staged = [torch.from_numpy(a).to(sg.DEV) for a in (f32(r, X * Y * Z), _mask01(r, X * Y * Z), _mask01(r, X * Y * Z, 0.1))]
    ops = [torch.empty_like(t) for t in staged]
    for o, t in zip(ops, staged):
        o.copy_(t)
    _wrapper_case(table, ops, staged, lambda: [data.mask_slices_flat(*ops, (X, Y, Z), torch.device(sg.DEV))])


@pytest.mark.gpu
def test_evaluate_wrapper_follows_torchs_current_stream(table):
    import torch
    from dep_gan_im_amd import evaluate
    staged = [torch.from_numpy(_set(rng_of("wrapper_eval"))).to(sg.DEV)]
    ops = [staged[0].clone()]
    _wrapper_case(table, ops, staged, lambda: [evaluate.distance_transform(ops[0], spacing=(2, 1, 1), squared=True)])
