"""Plain float64 restatements of the fp32 head to K = 2..8 class logits (csrc/train_ops.hip, dg_head_k_fwd / _bwd /
_wgrad), the two kinds of operands they are tested with, and the case table of tests/test_gpu_head_k.py.  Shared by
tests/test_head_k_ref_cpu.py (which checks the restatement, the exact-operand bound and the table's coverage without a
GPU) and tests/test_gpu_head_k.py (which runs the kernels).

The operations, on P pixel rows; a row of a strided operand is buf[p * ld + c0 : p * ld + c0 + C]:

    logits = a[:, :C] @ w + b                                   w (C, K), b (K)
    din    = (mask > 0 or no mask) ? dz @ w.T : +0              dz (P, K)
    dW     = a.T @ dz,  db = dz.sum(0)

Two kinds of operands (the method of tests/fused_ref.py and tests/test_gpu_bf16s_exact.py):

exact   a integers in [-2, 2]; w multiples of 1/2 in [-1, 1]; dz multiples of 1/4 in [-1, 1]; b multiples of 1/8 in
        [-2, 2]; mask from {-1, -0.0, +0.0, 1e-30, 1}.  Every product and every partial sum of the three kernels is then
        a multiple of 2^-3 (forward, backward) or 2^-2 (weight gradient), and in those units the sum of the absolute
        terms stays below 2^24 (exact_units() for any case, checked at generation on the drawn values): no fp32 product,
        fma or partial sum rounds in any order, so the float64 result is THE bit pattern.
real    standard normal a, dz, b; w normal / sqrt(C); the mask normal with a tenth of it exactly +0.0 and a tenth
        exactly -0.0.  Compared at gamma_L * sum|terms|, L the longest chain of roundings of the kernel's order.

The sign of a zero: the forward adds b (never -0.0 here) last and the weight gradient accumulates from +0, so a zero
result is +0.0 there, which `+ 0.0` states below.  The backward sums dz0 w0, then k = 1..K-1 left to right from that
first product, so -0.0 is a possible value and bwd() follows the same order.
"""
import collections
import math

import numpy as np

U = 2.0 ** -24
MASKS = np.array([-1.0, -0.0, 0.0, 1e-30, 1.0], np.float32)
# the launch constants of train_ops.hip, restated: threads per block, the forward/backward grid cap (head_k_blocks) and
# the weight gradient's cap on pixel blocks (t_pix_grid)
THREADS, FB_CAP, PIX_CAP = 256, 2048, 1024
KS = tuple(range(2, 9))
CS = (4, 8, 16, 32, 64, 128, 256)

Case = collections.namedtuple("Case", "P C K lda c0a ldm c0m ldd c0d")


def case(P, C, K, windowed=False):
    """dense: every row stride is C.  windowed: a, mask and din are channel windows of three wider buffers, each with
    its own stride and its own offset (a multiple of 4), ldm != ldd."""
    if not windowed:
        return Case(P, C, K, C, 0, C, 0, C, 0)
    return Case(P, C, K, C + 8, 4, C + 4, 4, C + 16, 8)


def case_id(c):
    return "P%d_C%d_K%d_%s" % (c.P, c.C, c.K, "dense" if c.lda == c.C else "win")


def _table():
    t = []
    # every (K, C) pair at a P that is no multiple of 4: ragged forward/backward tail, short last weight-gradient block
    for i, K in enumerate(KS):
        for j, C in enumerate(CS):
            t.append(case(1003, C, K, windowed=(i + j) % 2 == 1))
    t += [case(1, 4, 2), case(1, 32, 5, True), case(1, 256, 8), case(1, 128, 4, True)]                # one pixel
    t += [case(5, 4, 2, True), case(5, 4, 7), case(5, 4, 8), case(3, 32, 3), case(2, 256, 8, True)]   # P < 256 / (C/4)
    t += [case(257, 4, 3), case(259, 256, 8, True), case(258, 32, 2, True)]                           # tails, two blocks
    # past the 2048-block cap of the forward and the backward, with a remainder
    t += [case(8192 + 37, 256, 2, True), case(8192 + 37, 256, 8), case(8192 + 37, 256, 5)]
    t += [case(65536 + 5, 32, 5, True), case(65536 + 5, 32, 8), case(65536 + 5, 32, 2)]
    t += [case(524288 + 3, 4, 2), case(524288 + 3, 4, 7, True), case(524288 + 3, 4, 8)]
    # more than 256 pixels per weight-gradient block, not a multiple of the 256 / (C/4) pixel rows
    t += [case(262144 + 7, 4, 2, True), case(262144 + 7, 4, 8), case(262144 + 7, 32, 3), case(262144 + 7, 32, 8)]
    return t


CASES = _table()


def find(P, C, K):
    """The table's case of that size."""
    return next(c for c in CASES if (c.P, c.C, c.K) == (P, C, K))


# ---------------------------------------------------------------------------------------------------------------------
# the launch grids, restated from P and C
# ---------------------------------------------------------------------------------------------------------------------
def pix_grid(P):
    """(nb, ppb) of the weight gradient: at most PIX_CAP blocks of ppb pixels, the last one may be short."""
    nb = min((P + THREADS - 1) // THREADS, PIX_CAP)
    ppb = (P + nb - 1) // nb
    return (P + ppb - 1) // ppb, ppb


def forms(c):
    """The launch forms one case reaches, as a set of names."""
    LP = c.C // 4
    PP = THREADS // LP
    items = c.P * LP                                     # threads' worth of work in the forward and the backward
    nb, ppb = pix_grid(c.P)
    f = {"K%d" % c.K, "C%d" % c.C}
    if c.P == 1003:
        f.add("cross/K%d/C%d" % (c.K, c.C))
    if c.P == 1:
        f.add("one-pixel")
    if c.P < PP:
        f.add("below-row-group/C%d" % c.C)
    if items % THREADS:
        f.add("tail/C%d" % c.C)
    if items > FB_CAP * THREADS and items % (FB_CAP * THREADS):
        f.add("past-cap/C%d" % c.C)
    if nb < 256 and nb > 1 and c.P % ppb:
        f.add("wgrad/short-last-block")
    if 256 < nb <= PIX_CAP:
        f.add("wgrad/over-256-partials")
    if ppb > 256 and ppb % PP:
        f.add("wgrad/ppb-over-256/C%d" % c.C)
    f.add("ld=C" if c.lda == c.C else "ld>C")
    if c.lda > c.C:
        assert c.c0a > 0 and c.c0m > 0 and c.c0d > 0 and not (c.c0a % 4 or c.c0m % 4 or c.c0d % 4)
        assert c.c0a + c.C <= c.lda and c.c0m + c.C <= c.ldm and c.c0d + c.C <= c.ldd
        if len({c.lda, c.ldm, c.ldd}) == 3:
            f.add("own-strides")
    return f


def required_forms():
    req = {"K%d" % K for K in KS} | {"C%d" % C for C in CS} | {"cross/K%d/C%d" % (K, C) for K in KS for C in CS}
    req |= {"one-pixel", "below-row-group/C4", "tail/C4", "tail/C256", "past-cap/C256", "past-cap/C32", "past-cap/C4",
            "wgrad/short-last-block", "wgrad/over-256-partials", "wgrad/ppb-over-256/C4", "wgrad/ppb-over-256/C32",
            "ld=C", "ld>C", "own-strides"}
    return req


def check_table(cases=None):
    """The table reaches every required form; beyond the full cross, the cases still span K = 2, K = 8, an odd K and
    C = 4, 32, 256.  Raises AssertionError naming what is missing."""
    cases = CASES if cases is None else cases
    reached = set().union(*(forms(c) for c in cases))
    missing = required_forms() - reached
    assert not missing, sorted(missing)
    rest = [c for c in cases if c.P != 1003]
    assert {2, 8} <= {c.K for c in rest} and any(c.K % 2 for c in rest)
    assert {4, 32, 256} <= {c.C for c in rest}
    assert 1003 % 256 and 1003 % 4
    # the sizes named for the grids are the ones the restated grids give
    assert pix_grid(1003) == (4, 251) and pix_grid(65536 + 5) == (257, 256) and pix_grid(262144 + 7) == (1021, 257)
    assert pix_grid(524288 + 3) == (1023, 513) and pix_grid(1) == (1, 1)
    return reached


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
class Ops:
    """a, mask (P, C), w (C, K), b (K), dz (P, K), float32."""


def exact_units(P, C, K):
    """Worst case of the sum of absolute terms of any output, in units of the smallest product of its kernel:
    (forward: 2^-3 with the bias, backward: 2^-3, weight and bias gradient: 2^-2)."""
    return ((C * 2 * 1 + 2) * 8, K * 1 * 1 * 8, max(P * 2 * 1, P * 1) * 4)


def make_ops(kind, rng, P, C, K):
    o = Ops()
    if kind == "exact":
        assert max(exact_units(P, C, K)) < 2 ** 24, (P, C, K)
        o.a = rng.integers(-2, 3, (P, C)).astype(np.float32)
        o.w = (rng.integers(-2, 3, (C, K)) / 2.0).astype(np.float32)
        o.b = (rng.integers(-16, 17, K) / 8.0).astype(np.float32)
        o.dz = (rng.integers(-4, 5, (P, K)) / 4.0).astype(np.float32)
        o.mask = rng.choice(MASKS, (P, C)).astype(np.float32)
        o.mask.reshape(-1)[:4] = (-0.0, 1.0, 0.0, -1.0)                  # both decisions are present at every size
        # the bound on the values actually drawn
        assert (fwd_mag(o.a, o.w, o.b) * 8).max() < 2 ** 24 and (bwd_mag(o.dz, o.w) * 8).max() < 2 ** 24
        mw, mb = wgrad_mag(o.a, o.dz)
        assert (mw * 4).max() < 2 ** 24 and (mb * 4).max() < 2 ** 24
    else:
        assert kind == "real"
        nrm = lambda *s: rng.standard_normal(s, dtype=np.float32)      # noqa: E731
        o.a, o.dz, o.b = nrm(P, C), nrm(P, K), nrm(K)
        o.w = (nrm(C, K) / np.float32(math.sqrt(C))).astype(np.float32)
        o.mask = nrm(P, C)
        r = rng.random((P, C))
        o.mask[r < 0.1] = 0.0
        o.mask[r > 0.9] = -0.0
        if o.mask.size >= 4:                                             # the four kinds are present at every size
            o.mask.reshape(-1)[:4] = (0.0, -0.0, -1.5, 0.75)
    assert not np.signbit(o.b[o.b == 0]).any()
    return o


def window(values, P, ld, c0, fill):
    """A (P, ld) float32 buffer holding `fill` with values (P, C) at channel offset c0."""
    buf = np.full((P, ld), fill, np.float32)
    buf[:, c0:c0 + values.shape[1]] = values
    return buf


def rows(buf, P, ld, c0, C):
    """The (P, C) pixel rows of a flat buffer: row p is buf[p * ld + c0 : p * ld + c0 + C]."""
    flat = np.asarray(buf).reshape(-1)
    return np.lib.stride_tricks.as_strided(flat[c0:], (P, C), (ld * flat.itemsize, flat.itemsize), writeable=False)


# ---------------------------------------------------------------------------------------------------------------------
# the restatements (float64) and the sums of absolute terms their bounds use
# ---------------------------------------------------------------------------------------------------------------------
def _d(x):
    return np.asarray(x, np.float64)


def fwd(a, w, b):
    return (_d(a) @ _d(w) + _d(b)) + 0.0


def fwd_mag(a, w, b):
    return np.abs(_d(a)) @ np.abs(_d(w)) + np.abs(_d(b))


def bwd(dz, w, mask=None):
    dz, w = _d(dz), _d(w)
    v = dz[:, 0:1] * w[None, :, 0]
    for k in range(1, dz.shape[1]):
        v = v + dz[:, k:k + 1] * w[None, :, k]
    return v if mask is None else np.where(np.asarray(mask) > 0, v, 0.0)


def bwd_mag(dz, w):
    return np.abs(_d(dz)) @ np.abs(_d(w)).T


def wgrad(a, dz):
    a, dz = _d(a), _d(dz)
    return (a.T @ dz) + 0.0, dz.sum(0) + 0.0


def wgrad_mag(a, dz):
    a, dz = np.abs(_d(a)), np.abs(_d(dz))
    return a.T @ dz, dz.sum(0)


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 error bounds: |err| <= gamma_L * sum|terms|, L the longest chain of roundings a term can pass through
# ---------------------------------------------------------------------------------------------------------------------
def gamma(L):
    return L * U / (1.0 - L * U)


def chain_fwd(C):
    """one product and three fmaf per 4-channel part (4 = 3 + 1), log2(C/4) butterfly steps, the bias (+ 1)"""
    return 3 + int(math.log2(C // 4)) + 2


def chain_bwd(K):
    """one product and K - 1 fmaf"""
    return K


def chain_wgrad(P, C):
    """a thread's ceil(ppb / PP) fmaf, the PP pixel rows added through LDS, a thread's ceil(nb / 256) partials and the
    8 steps of the block sum (6 in a wave, 2 across the 4 waves)"""
    PP = THREADS // (C // 4)
    nb, ppb = pix_grid(P)
    return -(-ppb // PP) + PP + -(-nb // 256) + 8
