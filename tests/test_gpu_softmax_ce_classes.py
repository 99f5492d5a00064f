"""GPU: the softmax + cross-entropy operator for 2 to 8 classes with one-hot or integer labels (depgan_op_softmax_ce) and
the bf16-storage softmax head for K classes (depgan_op_head_softmax_k_bf16s).

Bit for bit: C = 4 against depgan_op_softmax_ce4, class codes against their one-hot encoding, repeated calls, each logit
column of the head against depgan_op_head_bf16s and its probabilities against depgan_op_softmax_ce of those logits.
Against float64 (torch.softmax, the oracle's keras cross-entropy, autograd) the bounds are the ones test_softmax_ce4
applies to the same formulas: 1e-6 on the probabilities, 1e-5 of max |dz| on the gradient, 1e-5 relative on the loss."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import depgan_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CLASSES = [2, 3, 4, 5, 8]
P_GRID = 262_181      # 37 pixels past the 1024-block cap: the grid-stride loop takes over
P_RAGGED = 3219       # a ragged grid of 13 blocks


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _special_rows(Cc):
    """(row, what) pairs: a tie of the maximum in every position, equal logits, a spread of +-100 in every position."""
    rows = []
    for i in range(Cc):
        r = np.full(Cc, -3.0, np.float32)
        r[i] = r[(i + 1) % Cc] = 2.0
        rows.append((r, "tie"))
    for v in (0.0, 5.0):
        rows.append((np.full(Cc, v, np.float32), "equal"))
    for i in range(Cc):
        r = np.full(Cc, -100.0, np.float32)
        r[i] = 100.0
        rows.append((r, "spread"))
    return rows


def _inputs(rng, P_, Cc):
    """test_gpu_train_ops.py::_softmax_inputs for Cc classes and any P_: random rows, then (as far as P_ has room) the
    special rows under every label and the rows that sit on and beyond both clip bounds.  Returns logits (P_, Cc)
    float32, codes (P_,) uint8 and the kind of every row."""
    z = (3.0 * rng.standard_normal((P_, Cc))).astype(np.float32)
    lab = rng.integers(0, Cc, P_)
    kind = np.array(["random"] * P_, dtype=object)
    n = 0
    for row, what in _special_rows(Cc):
        for k in range(Cc):
            if n < P_:
                z[n], lab[n], kind[n] = row, k, what
                n += 1
    m = min(4000, (P_ - n) // 2)
    if m > 0:
        # the clip's upper bound: gaps g with q0 = 1 / (1 + (Cc - 1) exp(-g)) around 1 - 1e-7, true class 0
        g0 = np.log((Cc - 1) * 1e7)
        g = np.linspace(g0 - 1.75, g0 + 1.75, m, dtype=np.float32)
        z[n:n + m] = 0.0
        z[n:n + m, 0] = g
        lab[n:n + m] = 0
        kind[n:n + m] = "upper"
        n += m
        # the lower bound: the true class 1e-7 below the others
        g1 = np.log(1e7 / (Cc - 1))
        z[n:n + m] = 0.0
        z[n:n + m, Cc - 1] = -np.linspace(g1 - 1.75, g1 + 1.75, m, dtype=np.float32)
        lab[n:n + m] = Cc - 1
        kind[n:n + m] = "lower"
    return z, lab.astype(np.uint8), kind


def _run(lib, zd, P_, Cc, onehot=None, codes=None, bufs=None, expect=0):
    """One call on NaN-filled outputs (or the given buffers); returns (probs, dz, loss_sum) as numpy, dz and the loss
    only with labels."""
    if bufs is None:
        bufs = (torch.full((P_, Cc), float("nan"), device=DEV), torch.full((P_, Cc), float("nan"), device=DEV),
                torch.full((1,), float("nan"), device=DEV))
    p, dz, ls = bufs
    lab = onehot is not None or codes is not None
    rc = lib.depgan_op_softmax_ce(P(zd), P(onehot), P(codes), P(p), P(dz) if lab else None, P(ls) if lab else None, P_,
                                  Cc, None)
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.depgan_last_error())
    return p.cpu().numpy(), (dz.cpu().numpy() if lab else None), (ls.cpu().numpy() if lab else None)


def _same(a, b):
    return all(np.array_equal(_u32(x), _u32(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("P_", [1, 255, P_RAGGED, P_GRID])
def test_four_classes_are_softmax_ce4(lib, P_):
    """1. C = 4 with one-hot labels is depgan_op_softmax_ce4, bit for bit: one thread, a ragged block, a ragged grid, and
    past the block cap."""
    from dep_gan_im_amd import _lib
    z, codes, _ = _inputs(np.random.default_rng(3 + P_), P_, 4)
    zd = torch.from_numpy(z).to(DEV)
    td = torch.from_numpy(np.eye(4, dtype=np.float32)[codes]).to(DEV)
    got = _run(lib, zd, P_, 4, onehot=td)
    p, dz = torch.full_like(zd, float("nan")), torch.full_like(zd, float("nan"))
    ls = torch.full((1,), float("nan"), device=DEV)
    _lib.check(lib.depgan_op_softmax_ce4(P(zd), P(td), P(p), P(dz), P(ls), P_, None), "softmax_ce4")
    torch.cuda.synchronize()
    assert _same(got, (p.cpu().numpy(), dz.cpu().numpy(), ls.cpu().numpy()))
    assert all(np.isfinite(a).all() for a in got)
    p0 = torch.full_like(zd, float("nan"))
    _lib.check(lib.depgan_op_softmax_ce4(P(zd), None, P(p0), None, None, P_, None), "softmax4")
    torch.cuda.synchronize()
    assert np.array_equal(_u32(p0.cpu().numpy()), _u32(got[0]))
    assert np.array_equal(_u32(_run(lib, zd, P_, 4)[0]), _u32(got[0]))               # no labels: probabilities only


@pytest.mark.parametrize("P_", [P_RAGGED, P_GRID])
@pytest.mark.parametrize("Cc", CLASSES)
def test_codes_equal_their_one_hot_encoding(lib, Cc, P_):
    """2. the call with class codes equals the call with np.eye(C)[codes] value for value, and repeats."""
    z, codes, _ = _inputs(np.random.default_rng(11 * Cc + P_), P_, Cc)
    zd = torch.from_numpy(z).to(DEV)
    dense = _run(lib, zd, P_, Cc, onehot=torch.from_numpy(np.eye(Cc, dtype=np.float32)[codes]).to(DEV))
    cd = torch.from_numpy(codes).to(DEV)
    sparse = _run(lib, zd, P_, Cc, codes=cd)
    assert _same(sparse, dense)
    assert _same(_run(lib, zd, P_, Cc, codes=cd), sparse)
    assert all(np.isfinite(a).all() for a in sparse)


@pytest.mark.parametrize("Cc", CLASSES)
def test_against_float64(lib, Cc):
    """3. torch.softmax, the oracle's keras cross-entropy and autograd in float64, at test_softmax_ce4's bounds; exact
    values where the arithmetic has them."""
    P_ = P_RAGGED
    z, codes, kind = _inputs(np.random.default_rng(5 + Cc), P_, Cc)
    assert {"tie", "equal", "spread", "upper", "lower", "random"} <= set(kind)
    t = np.eye(Cc, dtype=np.float32)[codes]
    p, dz, ls = _run(lib, torch.from_numpy(z).to(DEV), P_, Cc, codes=torch.from_numpy(codes).to(DEV))
    zt = torch.from_numpy(z).double().requires_grad_(True)
    p64 = torch.softmax(zt, -1)
    loss = O.keras_categorical_crossentropy_t(p64, torch.from_numpy(t).double())
    (g64,) = torch.autograd.grad(loss, zt)
    p64, g64 = p64.detach().numpy(), g64.numpy()
    e_p, e_g = float(np.abs(p - p64).max()), float(np.abs(dz - g64).max())
    lsum = float(loss.detach()) * P_
    print("C = %d: probs %.3e (1e-6), dz %.3e (%.3e), loss sum %.6f vs %.6f" % (Cc, e_p, e_g, 1e-5 * np.abs(g64).max(),
                                                                              float(ls[0]), lsum))
    assert e_p <= 1e-6
    assert e_g <= 1e-5 * np.abs(g64).max()
    assert abs(float(ls[0]) - lsum) <= 1e-5 * lsum, (float(ls[0]), lsum)
    assert np.abs(p.astype(np.float64).sum(-1) - 1.0).max() <= Cc * 2.0 ** -24
    # a spread of +-100: probabilities exactly 1 and 0, and the whole pixel's dz exactly 0 (the true class's q is beyond
    # the clip on one side or the other)
    sp = kind == "spread"
    assert np.array_equal(p[sp], (z[sp] == 100.0).astype(np.float32))
    assert np.all(dz[sp] == 0.0)
    # equal logits: exactly 1 / C where that is a float
    eq = kind == "equal"
    if Cc in (2, 4, 8):
        assert np.all(p[eq] == np.float32(1.0 / Cc))
    # a tie of the maximum: the two tied classes get the same probability, bit for bit
    for i in range(Cc):
        rows = p[i * Cc:(i + 1) * Cc]
        assert np.array_equal(_u32(rows[:, i]), _u32(rows[:, (i + 1) % Cc])), i
    # beyond the clip [1e-7, 1 - 1e-7] the gradient is cut
    q = p64[np.arange(P_), codes]
    out = (q > 1.0 - 0.5e-7) | (q < 0.5e-7)
    assert out.sum() > 100
    assert np.all(dz[out] == 0.0)


@pytest.mark.parametrize("Cc", [3, 8])
def test_out_of_range_codes_are_counted(lib, Cc):
    """4. three pixels coded C and 255: status 1 with the count; the buffers serve a valid call afterwards."""
    P_ = P_RAGGED
    z, codes, _ = _inputs(np.random.default_rng(17 + Cc), P_, Cc)
    zd = torch.from_numpy(z).to(DEV)
    want = _run(lib, zd, P_, Cc, codes=torch.from_numpy(codes).to(DEV))
    bad = codes.copy()
    bad[[5, 1700, P_ - 1]] = [Cc, 255, Cc]
    bufs = (torch.full((P_, Cc), float("nan"), device=DEV), torch.full((P_, Cc), float("nan"), device=DEV),
            torch.full((1,), float("nan"), device=DEV))
    got = _run(lib, zd, P_, Cc, codes=torch.from_numpy(bad).to(DEV), bufs=bufs, expect=1)
    msg = lib.depgan_last_error()
    assert b"3 of %d" % P_ in msg and b"[0, %d)" % Cc in msg, msg
    ok = np.ones(P_, bool)
    ok[[5, 1700, P_ - 1]] = False
    assert np.array_equal(_u32(got[0]), _u32(want[0]))                          # the probabilities do not read the labels
    assert np.array_equal(_u32(got[1][ok]), _u32(want[1][ok])) and np.all(got[1][~ok] == 0.0)
    assert _same(_run(lib, zd, P_, Cc, codes=torch.from_numpy(codes).to(DEV), bufs=bufs), want)


@pytest.mark.parametrize("Pn", [1, 64, P_RAGGED])
@pytest.mark.parametrize("Cn", [32, 64])
@pytest.mark.parametrize("K", [2, 3, 4, 5, 8])
def test_head_softmax_k(lib, K, Cn, Pn):
    """5. the K-class head on channels [32, 32 + Cn) of 96-element bf16 rows, NaN outside the slice."""
    from dep_gan_im_amd import _lib
    ld, coff = 96, 32
    rng = np.random.default_rng(Pn + 7 * Cn + K)
    bf = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16)   # noqa: E731
    a = bf(rng.standard_normal((Pn, Cn)))
    w = bf(rng.standard_normal((Cn, K)) / 4.0).to(torch.float32).numpy()
    b = rng.standard_normal(K).astype(np.float32)
    wide = torch.full((Pn, ld), float("nan"), dtype=torch.bfloat16)
    wide[:, coff:coff + Cn] = a
    ldw = ld
    ah, wd, bd = wide.to(DEV), torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV)
    probs, logits = torch.full((Pn, K), float("nan"), device=DEV), torch.full((Pn, K), float("nan"), device=DEV)
    _lib.check(lib.depgan_op_head_softmax_k_bf16s(C.c_void_p(ah.data_ptr() + 2 * coff), ldw, P(wd), P(bd), P(probs),
                                                  P(logits), Pn, Cn, K, None), "depgan_op_head_softmax_k_bf16s")
    torch.cuda.synchronize()
    probs, logits = probs.cpu().numpy(), logits.cpu().numpy()
    assert np.isfinite(probs).all() and np.isfinite(logits).all()
    dense = a.contiguous().to(DEV)
    for k in range(K):
        wk = torch.from_numpy(np.ascontiguousarray(w[:, k])).to(DEV)
        bk = torch.from_numpy(b[k:k + 1].copy()).to(DEV)
        out = torch.full((Pn,), float("nan"), device=DEV)
        _lib.check(lib.depgan_op_head_bf16s(P(dense), P(wk), P(bk), P(out), Pn, Cn, 0, None), "depgan_op_head_bf16s")
        torch.cuda.synchronize()
        assert np.array_equal(_u32(logits[:, k]), _u32(out.cpu().numpy())), k
    want = _run(lib, torch.from_numpy(logits).to(DEV), Pn, K)[0]
    assert np.array_equal(_u32(probs), _u32(want))
    if K == 4:
        p4, l4 = torch.full((Pn, 4), float("nan"), device=DEV), torch.full((Pn, 4), float("nan"), device=DEV)
        _lib.check(lib.depgan_op_head_softmax_bf16s(C.c_void_p(ah.data_ptr() + 2 * coff), ldw, P(wd), P(bd), P(p4), P(l4),
                                                    Pn, Cn, None), "depgan_op_head_softmax_bf16s")
        torch.cuda.synchronize()
        assert np.array_equal(_u32(probs), _u32(p4.cpu().numpy())) and np.array_equal(_u32(logits), _u32(l4.cpu().numpy()))
