"""Without a GPU: tests/head_k_ref.py's float64 restatements of the K-class head against a per-element triple loop, the
exact-operand bound for every case of the GPU table (so the table's "bit for bit" rests on something checked here), the
table's coverage of the launch forms, the three prototypes, and the forward's and the backward's refusals, which come
before any HIP call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_k_ref as R  # noqa: E402

FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments
TINY = [R.Case(5, 4, 3, 4, 0, 4, 0, 4, 0), R.Case(7, 8, 2, 16, 4, 12, 4, 24, 8)]


def _loops(o, c, abuf, mbuf):
    """The three operations element by element on the flat strided buffers, Python floats (float64)."""
    a = lambda p, ch: float(abuf.reshape(-1)[p * c.lda + c.c0a + ch])      # noqa: E731
    m = lambda p, ch: float(mbuf.reshape(-1)[p * c.ldm + c.c0m + ch])      # noqa: E731
    z = np.zeros((c.P, c.K))
    din, dnm = np.zeros((c.P, c.C)), np.zeros((c.P, c.C))
    dW, db = np.zeros((c.C, c.K)), np.zeros(c.K)
    for p in range(c.P):
        for k in range(c.K):
            s = 0.0
            for ch in range(c.C):
                s += a(p, ch) * float(o.w[ch, k])
            z[p, k] = s + float(o.b[k])
            db[k] += float(o.dz[p, k])
        for ch in range(c.C):
            s = 0.0
            for k in range(c.K):
                s += float(o.dz[p, k]) * float(o.w[ch, k])
                dW[ch, k] += a(p, ch) * float(o.dz[p, k])
            dnm[p, ch] = s
            din[p, ch] = s if m(p, ch) > 0 else 0.0
    return z, din, dnm, dW, db


@pytest.mark.parametrize("c", TINY, ids=R.case_id)
@pytest.mark.parametrize("kind", ["exact", "real"])
def test_restatement_equals_the_triple_loop(c, kind):
    rng = np.random.default_rng(c.P * 100 + c.C)
    o = R.make_ops(kind, rng, c.P, c.C, c.K)
    abuf = R.window(o.a, c.P, c.lda, c.c0a, np.nan)
    mbuf = R.window(o.mask, c.P, c.ldm, c.c0m, np.nan)
    ar, mr = R.rows(abuf, c.P, c.lda, c.c0a, c.C), R.rows(mbuf, c.P, c.ldm, c.c0m, c.C)
    assert np.array_equal(ar, o.a) and np.array_equal(mr.view(np.uint32), o.mask.view(np.uint32))
    z, din, dnm, dW, db = _loops(o, c, abuf, mbuf)
    gw, gb = R.wgrad(ar, o.dz)
    got = (R.fwd(ar, o.w, o.b), R.bwd(o.dz, o.w, mr), R.bwd(o.dz, o.w), gw, gb)
    for g, want in zip(got, (z, din, dnm, dW, db)):
        assert g.dtype == np.float64 and g.shape == want.shape
        if kind == "exact":
            assert np.array_equal(g, want)                       # no rounding: the order cannot matter
        else:
            np.testing.assert_allclose(g, want, rtol=0, atol=64 * 2.0 ** -53 * (1 + np.abs(want).max()))
    # the mask decides on > 0: +0.0, -0.0 and negatives give +0.0, a denormal-small positive passes
    off = ~(mr > 0)
    assert off.any() and (~off).any()
    assert np.all(got[1][off] == 0) and not np.signbit(got[1][off]).any()
    assert np.array_equal(got[1][~off], got[2][~off])


def test_exact_operands_do_not_round_in_float32_in_any_order():
    """The point of the bound: float32 sums of the exact operands, forwards, backwards and pairwise, are the float64 value."""
    P, Cc, K = 1003, 256, 8
    o = R.make_ops("exact", np.random.default_rng(3), P, Cc, K)
    f32 = np.float32
    z = R.fwd(o.a, o.w, o.b)
    terms = o.a[:, :, None] * o.w[None, :, :]                     # float32 products
    assert terms.dtype == f32
    for order in (slice(None), slice(None, None, -1)):
        s = np.zeros((P, K), f32)
        for ch in range(Cc)[order]:
            s = s + terms[:, ch, :]
        assert np.array_equal((s + o.b).astype(np.float64), z)
    assert np.array_equal((terms.sum(1, dtype=f32) + o.b).astype(np.float64), z)          # numpy's pairwise order
    dW, db = R.wgrad(o.a, o.dz)
    t = o.a[:, :, None] * o.dz[:, None, :]
    assert np.array_equal(t.sum(0, dtype=f32).astype(np.float64), dW)
    assert np.array_equal(np.cumsum(t[::-1], 0, dtype=f32)[-1].astype(np.float64), dW)
    assert np.array_equal(o.dz.sum(0, dtype=f32).astype(np.float64), db)
    d = R.bwd(o.dz, o.w)
    t = o.dz[:, None, :] * o.w[None, :, :]
    assert np.array_equal(np.cumsum(t[..., ::-1], 2, dtype=f32)[..., -1].astype(np.float64), d)


def test_exact_bound_holds_for_every_case_of_the_gpu_table():
    worst = 0
    for c in R.CASES:
        units = R.exact_units(c.P, c.C, c.K)
        assert max(units) < 2 ** 24, (c, units)
        worst = max(worst, *units)
    big = max(R.CASES, key=lambda c: c.P)
    assert big.P == 524288 + 3 and worst == 8 * big.P                # the largest case sets the bound: 2^22, four-fold room
    # the generator checks the drawn values too; here on every case small enough to draw quickly, and on the largest
    for c in [c for c in R.CASES if c.P <= 9000 and c.K in (2, 8)] + [big]:
        o = R.make_ops("exact", np.random.default_rng(c.P + c.C + c.K), c.P, c.C, c.K)
        for x, q in ((o.a, 1), (o.w, 2), (o.dz, 4), (o.b, 8)):
            assert np.array_equal(x * q, np.round(x * q)) and np.abs(x).max() <= (2, 1, 1, 2)[(1, 2, 4, 8).index(q)]
    with pytest.raises(AssertionError):
        R.make_ops("exact", np.random.default_rng(0), 2 ** 22, 4, 2)  # a P the bound does not cover is refused


def test_real_operands_carry_both_zeros_and_negatives_in_the_mask():
    o = R.make_ops("real", np.random.default_rng(1), 1003, 32, 5)
    m = o.mask
    pz, nz = (m == 0) & ~np.signbit(m), (m == 0) & np.signbit(m)
    assert 0.05 < pz.mean() < 0.15 and 0.05 < nz.mean() < 0.15 and (m < 0).mean() > 0.3 and (m > 0).mean() > 0.3
    o = R.make_ops("real", np.random.default_rng(1), 1, 4, 2)        # one pixel still has all four kinds
    assert np.array_equal(o.mask.view(np.uint32)[0, :2], np.array([0, 0x80000000], np.uint32))


def test_case_table_covers_every_launch_form():
    reached = R.check_table()
    assert R.required_forms() <= reached
    assert len(set(R.CASES)) == len(R.CASES)
    for c in R.CASES:                                              # a few tens of MB per operand at the most
        assert c.P * max(c.lda, c.ldm, c.ldd) * 4 <= 48 << 20, c
    # the check notices a missing form
    with pytest.raises(AssertionError):
        R.check_table([c for c in R.CASES if c.P != 1])
    with pytest.raises(AssertionError):
        R.check_table([c for c in R.CASES if not (c.P == 262144 + 7 and c.C == 32)])
    with pytest.raises(AssertionError):
        R.check_table([c for c in R.CASES if c.lda == c.C])


def test_error_bound_chains():
    assert R.chain_fwd(4) == 5 and R.chain_fwd(256) == 11 and R.chain_bwd(8) == 8
    assert R.chain_wgrad(1003, 256) == 63 + 4 + 1 + 8 and R.chain_wgrad(262144 + 7, 4) == 2 + 256 + 4 + 8
    assert R.gamma(8) == 8 * R.U / (1 - 8 * R.U)


def test_header_declares_the_three_entries(lib):
    from dep_gan_im_amd import _lib
    hdr = _lib.parse_header(_lib.read_header())
    for name, nargs in {"depgan_op_head_k_fwd": 9, "depgan_op_head_k_bwd": 10, "depgan_op_head_k_wgrad": 10}.items():
        restype, argtypes = hdr.prototypes[name]
        assert restype is C.c_int and len(argtypes) == nargs and name in _lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == nargs


def test_forward_and_backward_refuse_before_any_hip_call(lib):
    half, odd = C.c_void_p(0x1004), C.c_void_p(0x1002)

    def f(a=FAKE, ld=32, w=FAKE, b=FAKE, z=FAKE, P=64, C_=32, K=3):
        return lib.depgan_op_head_k_fwd(a, ld, w, b, z, P, C_, K, None)

    def g(dz=FAKE, w=FAKE, m=FAKE, ldm=32, din=FAKE, ldd=32, P=64, C_=32, K=3):
        return lib.depgan_op_head_k_bwd(dz, w, m, ldm, din, ldd, P, C_, K, None)
    for kw in ({"a": None}, {"w": None}, {"b": None}, {"z": None}, {"P": 0}, {"K": 1}, {"K": 9}, {"C_": 12}, {"C_": 512},
               {"C_": 2}, {"ld": 28}, {"ld": 34}, {"a": half}, {"z": odd}, {"K": 4, "z": half}, {"K": 8, "z": half}):
        assert f(**kw) == 1 and lib.depgan_last_error(), kw
    for kw in ({"dz": None}, {"w": None}, {"din": None}, {"P": 0}, {"K": 1}, {"K": 9}, {"C_": 12}, {"C_": 512}, {"C_": 2},
               {"ldd": 28}, {"ldd": 34}, {"ldm": 28}, {"ldm": 34}, {"din": half}, {"m": half}, {"K": 4, "dz": half},
               {"K": 8, "dz": half}):
        assert g(**kw) == 1 and lib.depgan_last_error(), kw
    w = lambda **kw: lib.depgan_op_head_k_wgrad(kw.get("a", FAKE), 32, kw.get("dz", FAKE), kw.get("dW", FAKE),      # noqa: E731
                                                kw.get("db", FAKE), kw.get("P", 64), 32, 3, 0, None)
    for kw in ({"a": None}, {"dz": None}, {"dW": None}, {"db": None}, {"P": 0}):
        assert w(**kw) == 1 and lib.depgan_last_error(), kw
