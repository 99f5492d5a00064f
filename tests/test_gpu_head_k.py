"""GPU: the fp32 head to K = 2..8 class logits at operator level (depgan_op_head_k_fwd / _bwd / _wgrad: the kernels
head_k_fwd_kernel, head_k_bwd_kernel, head_k_wgrad_partial / _final of csrc/train_ops.hip), against the float64
restatement of tests/head_k_ref.py, over one case table: every K and every width C, pixel counts that leave ragged
tails, run past the forward's 2048-block cap, give the weight gradient short blocks, more than 256 pixels per block and
more than 256 block partials, and channel windows of wider buffers with a stride of their own per operand.

exact operands   no fp32 operation of the kernels can round (head_k_ref.py states the bound, test_head_k_ref_cpu.py checks
                 it for this table): logits, din, dW and db must equal the float64 result bit for bit, and every float
                 around the written windows keeps its sentinel.
real operands    |err| <= gamma_L * sum|terms| per element, L the longest chain of roundings of the kernel's order
                 (head_k_ref.chain_*), from the restated grid; the masked din is +0.0 wherever the mask is +0.0, -0.0 or
                 negative and the unmasked bits elsewhere.

The first device run printed, worst |err| / bound over the table (a ratio above 1 is a failure to investigate):
    forward          0.618  (P262151_C4_K8, L = 5)
    backward         0.963  (P8229_C256_K2, L = 2; 0.925 at P262151_C4_K2: two roundings over millions of elements
                            come close to their worst case, no chain is longer than stated)
    weight gradient  0.117  (P2_C256_K8, L = 14; below 0.001 where L is in the hundreds)
    bias gradient    0.071  (P2_C256_K8, L = 14)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_k_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENT = 0x7FC5A5A5                  # a quiet NaN with a payload no kernel produces
GUARD = 4                          # guard rows before and after the logits, guard rows after the last din row
NANF = np.float32(np.nan)


def sentinel(n):
    return torch.full((n,), SENT, dtype=torch.int32, device=DEV)


def ptr(t, off=0):
    """Device address of element `off` of a 4-byte tensor."""
    return None if t is None else C.c_void_p(t.data_ptr() + 4 * off)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def words(t):
    """Host copy of a 4-byte device tensor as uint32."""
    return t.cpu().numpy().view(np.uint32)


def same_bits(what, got_words, want):
    want = u32(np.asarray(want, np.float64).astype(np.float32))
    bad = got_words != want
    assert not bad.any(), "%s: %d of %d differ, first at %s: 0x%08x, want 0x%08x" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got_words[bad][0], want[bad][0])


def ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.depgan_last_error())


def test_case_table_covers_every_launch_form():
    """Class counts 2..8, widths 4..256, the full cross at P = 1003, one pixel, fewer pixels than a row group, ragged
    tails at C = 4 and C = 256, the three sizes past the 2048-block cap, the weight gradient's short last block, more than
    256 partials and more than 256 pixels per block at C = 4 and C = 32, dense and windowed rows with distinct strides:
    computed from P and C with the constants 256, 2048 and 1024 restated in head_k_ref.py, not asked of the library."""
    assert (R.THREADS, R.FB_CAP, R.PIX_CAP) == (256, 2048, 1024)
    reached = R.check_table()
    assert R.required_forms() <= reached
    win = [c for c in R.CASES if c.lda > c.C]
    assert win and all(c.ldm != c.ldd and c.lda != c.ldm for c in win)


# ---------------------------------------------------------------------------------------------------------------------
# one call of each operator into sentinel-filled buffers
# ---------------------------------------------------------------------------------------------------------------------
class Operands:
    """The device side of one case: a and the mask as windows of NaN-filled wider buffers, w, b, dz dense."""

    def __init__(self, c, o):
        self.c, self.o = c, o
        self.a = dev(R.window(o.a, c.P, c.lda, c.c0a, NANF))
        self.mask = dev(R.window(o.mask, c.P, c.ldm, c.c0m, NANF))
        self.w, self.b, self.dz = dev(o.w), dev(o.b), dev(o.dz)


def run_fwd(lib, d):
    c = d.c
    z = sentinel((c.P + 2 * GUARD) * c.K)
    ok(lib, lib.depgan_op_head_k_fwd(ptr(d.a, c.c0a), c.lda, ptr(d.w), ptr(d.b), ptr(z, GUARD * c.K), c.P, c.C, c.K, None),
       "head_k_fwd")
    got = words(z).reshape(c.P + 2 * GUARD, c.K)
    assert (got[:GUARD] == SENT).all() and (got[GUARD + c.P:] == SENT).all(), "forward wrote outside its P rows"
    return got[GUARD:GUARD + c.P]


def run_bwd(lib, d, masked):
    c = d.c
    din = sentinel((c.P + GUARD) * c.ldd)
    ok(lib, lib.depgan_op_head_k_bwd(ptr(d.dz), ptr(d.w), ptr(d.mask, c.c0m) if masked else None, c.ldm, ptr(din, c.c0d),
                                     c.ldd, c.P, c.C, c.K, None), "head_k_bwd")
    got = words(din).reshape(c.P + GUARD, c.ldd)
    out = got[:c.P, c.c0d:c.c0d + c.C].copy()
    got[:c.P, c.c0d:c.c0d + c.C] = SENT
    assert (got == SENT).all(), "backward wrote outside its window: %s" % (np.argwhere(got != SENT)[:4],)
    return out


def run_wgrad(lib, d, cap=0):
    """Twice into sentinel-filled outputs: two stages, fixed order, no atomics, so the bits repeat."""
    c = d.c
    res = []
    for _ in range(2):
        dW, db = sentinel(c.C * c.K + 8), sentinel(c.K + 8)
        ok(lib, lib.depgan_op_head_k_wgrad(ptr(d.a, c.c0a), c.lda, ptr(d.dz), ptr(dW), ptr(db), c.P, c.C, c.K, cap, None),
           "head_k_wgrad")
        gw, gb = words(dW), words(db)
        assert (gw[c.C * c.K:] == SENT).all() and (gb[c.K:] == SENT).all(), "weight gradient wrote past dW or db"
        res.append((gw[:c.C * c.K].reshape(c.C, c.K), gb[:c.K]))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]), "second call differs"
    return res[0]


def operands(kind, c):
    rng = np.random.default_rng([c.P, c.C, c.K, int(kind == "real")])
    o = R.make_ops(kind, rng, c.P, c.C, c.K)
    return o, Operands(c, o)


# ---------------------------------------------------------------------------------------------------------------------
# exact operands: bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_exact_operands_bit_for_bit(lib, c):
    o, d = operands("exact", c)
    same_bits("logits", run_fwd(lib, d), R.fwd(o.a, o.w, o.b))
    unmasked = R.bwd(o.dz, o.w)
    got_m, got_u = run_bwd(lib, d, True), run_bwd(lib, d, False)
    same_bits("din without a mask", got_u, unmasked)
    same_bits("din", got_m, R.bwd(o.dz, o.w, o.mask))
    off = ~(o.mask > 0)                                       # +0.0, -0.0 and -1 against 1e-30 and 1
    assert off.any() and (~off).any()
    assert (got_m[off] == 0).all(), "din is not +0.0 under a zero or negative mask"
    assert np.array_equal(got_m[~off], got_u[~off])
    gw, gb = run_wgrad(lib, d)
    rw, rb = R.wgrad(o.a, o.dz)
    same_bits("dW", gw, rw)
    same_bits("db", gb, rb)


# ---------------------------------------------------------------------------------------------------------------------
# real operands: the fp32 bound of each kernel's own summation
# ---------------------------------------------------------------------------------------------------------------------
def within(what, c, got_words, ref, mag, L):
    got = got_words.view(np.float32).astype(np.float64)
    assert np.isfinite(got).all(), what + ": non-finite output"
    bound = R.gamma(L) * mag
    err = np.abs(got - ref)
    dead = bound == 0
    assert (err[dead] == 0).all()
    ratio = float((err[~dead] / bound[~dead]).max()) if (~dead).any() else 0.0
    print("head_k ratio %s %s L=%d: %.4f" % (what, R.case_id(c), L, ratio))
    assert ratio <= 1.0, (what, c, ratio)
    return ratio


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_real_operands_within_the_summation_bound(lib, c):
    o, d = operands("real", c)
    within("fwd", c, run_fwd(lib, d), R.fwd(o.a, o.w, o.b), R.fwd_mag(o.a, o.w, o.b), R.chain_fwd(c.C))
    got_m, got_u = run_bwd(lib, d, True), run_bwd(lib, d, False)
    within("bwd", c, got_u, R.bwd(o.dz, o.w), R.bwd_mag(o.dz, o.w), R.chain_bwd(c.K))
    off = ~(o.mask > 0)
    zeros = o.mask == 0
    assert (zeros & np.signbit(o.mask)).any() and (zeros & ~np.signbit(o.mask)).any() and (o.mask < 0).any()
    assert (got_m[off] == 0).all(), "din is not +0.0 under a zero or negative mask"
    assert np.array_equal(got_m[~off], got_u[~off]), "the mask changed a value it lets through"
    gw, gb = run_wgrad(lib, d)
    rw, rb = R.wgrad(o.a, o.dz)
    mw, mb = R.wgrad_mag(o.a, o.dz)
    L = R.chain_wgrad(c.P, c.C)
    within("wgrad", c, gw, rw, mw, L)
    within("wgrad-bias", c, gb, rb, mb, L)


# ---------------------------------------------------------------------------------------------------------------------
# sample independence: a changed pixel row changes that row of the output and no other
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [R.find(1003, 256, 8), R.find(1003, 4, 7), R.find(1003, 32, 5)], ids=R.case_id)
def test_a_pixel_row_changes_only_its_own_output_row(lib, c):
    o, d = operands("real", c)
    z0, din0 = run_fwd(lib, d), run_bwd(lib, d, True)
    rng = np.random.default_rng(c.C)
    for q in (0, 517, c.P - 1):                              # first, inside a wave shared with other pixels, last
        o2 = R.Ops()
        o2.__dict__.update({k: v.copy() for k, v in o.__dict__.items()})
        o2.a[q] = rng.standard_normal(c.C, dtype=np.float32) + 3.0
        o2.dz[q] = rng.standard_normal(c.K, dtype=np.float32) + 3.0
        o2.mask[q] = -o.mask[q]
        o2.mask[q, :2] = 1.0
        d2 = Operands(c, o2)
        z1, din1 = run_fwd(lib, d2), run_bwd(lib, d2, True)
        others = np.arange(c.P) != q
        assert np.array_equal(z0[others], z1[others]) and np.array_equal(din0[others], din1[others]), q
        assert (z0[q] != z1[q]).all() and (din0[q, :2] != din1[q, :2]).all(), q


# ---------------------------------------------------------------------------------------------------------------------
# refusals: status 1 before any launch, every output untouched
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_return_status_1_and_write_nothing(lib):
    P_, Cc = 300, 32
    # operands large enough for every (C, K) that is named below, though no refused call reads them
    a, mask = torch.zeros(P_ * 512 + 4, device=DEV), torch.ones(P_ * 512 + 4, device=DEV)
    w, b, dz = torch.zeros(512 * 9, device=DEV), torch.zeros(16, device=DEV), torch.zeros(P_ * 9 + 4, device=DEV)
    outs = {"logits": sentinel(P_ * 9 + 4), "din": sentinel(P_ * 512 + 4), "dW": sentinel(512 * 9), "db": sentinel(16)}
    nb = R.pix_grid(P_)[0]
    assert nb == 2

    def fwd(a_=ptr(a), ld=Cc, w_=ptr(w), b_=ptr(b), z=ptr(outs["logits"]), P=P_, C_=Cc, K=3):
        return lib.depgan_op_head_k_fwd(a_, ld, w_, b_, z, P, C_, K, None)

    def bwd(dz_=ptr(dz), w_=ptr(w), m=ptr(mask), ldm=Cc, din=ptr(outs["din"]), ldd=Cc, P=P_, C_=Cc, K=3):
        return lib.depgan_op_head_k_bwd(dz_, w_, m, ldm, din, ldd, P, C_, K, None)

    def wgr(a_=ptr(a), lda=Cc, dz_=ptr(dz), dW=ptr(outs["dW"]), db=ptr(outs["db"]), P=P_, C_=Cc, K=3, cap=0):
        return lib.depgan_op_head_k_wgrad(a_, lda, dz_, dW, db, P, C_, K, cap, None)

    sizes = [{"K": 1}, {"K": 9}, {"P": 0}, {"C_": 12}, {"C_": 512}, {"C_": 2}]
    refused = [(fwd, kw) for kw in sizes + [
        {"ld": 28}, {"ld": 34}, {"a_": ptr(a, 1)}, {"K": 4, "z": ptr(outs["logits"], 1)},
        {"K": 8, "z": ptr(outs["logits"], 1)}, {"a_": None}, {"w_": None}, {"b_": None}, {"z": None}]]
    refused += [(bwd, kw) for kw in sizes + [
        {"ldd": 28}, {"ldd": 34}, {"ldm": 28}, {"ldm": 34}, {"m": ptr(mask, 1)}, {"din": ptr(outs["din"], 1)},
        {"K": 4, "dz_": ptr(dz, 1)}, {"K": 8, "dz_": ptr(dz, 1)}, {"dz_": None}, {"w_": None}, {"din": None}]]
    refused += [(wgr, kw) for kw in sizes + [
        {"lda": 28}, {"lda": 34}, {"a_": ptr(a, 1)}, {"K": 4, "dz_": ptr(dz, 1)}, {"K": 8, "dz_": ptr(dz, 1)},
        {"a_": None}, {"dz_": None}, {"dW": None}, {"db": None}, {"cap": nb * (Cc * 3 + 3) - 1}]]
    for call, kw in refused:
        assert call(**kw) == 1, (call.__name__, kw)
        assert lib.depgan_last_error(), (call.__name__, kw)
    assert b"scratch" in lib.depgan_last_error()             # the last one: a capacity one float short
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert (words(t) == SENT).all(), name + " was written by a refused call"


def test_one_float_offset_is_accepted_for_k3_and_exact_capacity_runs(lib):
    """Dense rows of K = 3 floats need no 16-byte alignment: logits and dz one float into their buffers compute the same
    bits; a weight-gradient scratch of exactly nb (C K + K) floats is accepted."""
    c = R.find(1003, 32, 3)
    o, d = operands("exact", c)
    z = sentinel(c.P * c.K + 2)
    ok(lib, lib.depgan_op_head_k_fwd(ptr(d.a, c.c0a), c.lda, ptr(d.w), ptr(d.b), ptr(z, 1), c.P, c.C, c.K, None), "fwd")
    got = words(z)
    assert got[0] == SENT and got[-1] == SENT
    same_bits("logits one float in", got[1:-1].reshape(c.P, c.K), R.fwd(o.a, o.w, o.b))
    shifted = torch.cat([torch.full((1,), float("nan"), device=DEV), d.dz.reshape(-1)])
    din = sentinel(c.P * c.ldd)
    ok(lib, lib.depgan_op_head_k_bwd(ptr(shifted, 1), ptr(d.w), None, 0, ptr(din, c.c0d), c.ldd, c.P, c.C, c.K, None), "bwd")
    same_bits("din from dz one float in", words(din).reshape(c.P, c.ldd)[:, c.c0d:c.c0d + c.C], R.bwd(o.dz, o.w))
    dW, db = sentinel(c.C * c.K), sentinel(c.K)
    need = R.pix_grid(c.P)[0] * (c.C * c.K + c.K)
    ok(lib, lib.depgan_op_head_k_wgrad(ptr(d.a, c.c0a), c.lda, ptr(shifted, 1), ptr(dW), ptr(db), c.P, c.C, c.K, need, None),
       "wgrad")
    rw, rb = R.wgrad(o.a, o.dz)
    same_bits("dW from dz one float in, exact capacity", words(dW).reshape(c.C, c.K), rw)
    same_bits("db", words(db), rb)
