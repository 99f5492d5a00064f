"""GPU: depgan_op_softmax_ce_weighted and depgan_op_label_counts, the loss-weight mode at operator level.

Exact statements are bit for bit: unit weights against depgan_op_softmax_ce, codes with an ignore code against the
one-hot encoding with all-zero rows, weights that are powers of two against ldexp of the unweighted rows, and half the
pixels ignored (den = P / 2, so 1 / den = 2 / P exactly).  The integer counts are compared with np.bincount / np.add.at.
Against float64 (tests/weighted_ce_ref.py) the bounds are test_softmax_ce4's: probabilities 1e-6, dz 1e-5 max|dz|, the
loss sum 1e-5 relative.  P = 1 is one thread, 255 a ragged block, 3219 a ragged grid of 13 blocks, 262181 is 37 pixels
past the 1024-block cap where the grid-stride loop takes over."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import weighted_ce_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
CLASSES = [2, 3, 4, 5, 8]
PIXELS = [1, 255, 3219, 262181]
NCOUNT = 11


def P_(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _u32(t):
    return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(Cc, P):
    """(logits (P, Cc) float32, codes (P,) uint8): standard-normal rows, every 7th with a tied maximum, every 7th all
    equal, every 7th spread by +-100; one class is rare (about 1 % of the pixels)."""
    rng = np.random.default_rng(2000 * Cc + P % 997)
    z = rng.standard_normal((P, Cc)).astype(np.float32)
    r = np.arange(P)
    tie = r[r % 7 == 1]
    z[tie, 0] = z[tie, Cc - 1] = (z[tie].max(-1) + np.float32(0.75)).astype(np.float32)
    z[r % 7 == 2] = np.float32(0.3125)
    z[r % 7 == 3] *= np.float32(100.0)
    share = np.full(Cc, 0.99 / (Cc - 1))
    share[Cc - 1] = 0.01
    codes = rng.choice(Cc, size=P, p=share).astype(np.uint8)
    return z, codes


def _plain(lib, z, onehot, codes, Cc):
    P = len(z)
    zd = torch.from_numpy(z).cuda()
    od = torch.from_numpy(onehot).cuda() if onehot is not None else None
    cd = torch.from_numpy(codes).cuda() if codes is not None else None
    probs, dz = torch.full((P, Cc), float("nan"), device="cuda:0"), torch.full((P, Cc), float("nan"), device="cuda:0")
    loss = torch.full((1,), float("nan"), device="cuda:0")
    rc = lib.depgan_op_softmax_ce(P_(zd), P_(od), P_(cd), P_(probs), P_(dz), P_(loss), P, Cc, None)
    torch.cuda.synchronize()
    return rc, probs.cpu().numpy(), dz.cpu().numpy(), loss.cpu().numpy()


def _weighted(lib, z, onehot, codes, w, ign, Cc, census=False, n=None):
    """One call into fresh NaN-filled outputs: (rc, probs, dz, loss sum, counts int64 (C + 3), census (C, C) or None)."""
    P = len(z)
    zd = torch.from_numpy(z).cuda()
    od = torch.from_numpy(onehot).cuda() if onehot is not None else None
    cd = torch.from_numpy(codes).cuda() if codes is not None else None
    probs, dz = torch.full((P, Cc), float("nan"), device="cuda:0"), torch.full((P, Cc), float("nan"), device="cuda:0")
    loss = torch.full((1,), float("nan"), device="cuda:0")
    wa = (C.c_float * len(w))(*[float(v) for v in w])
    cnt = (C.c_longlong * NCOUNT)(*([-7] * NCOUNT))
    cen = (C.c_longlong * 64)(*([-7] * 64)) if census else None
    rc = lib.depgan_op_softmax_ce_weighted(P_(zd), P_(od), P_(cd), wa, len(w) if n is None else n, ign, P_(probs), P_(dz),
                                           P_(loss), cen, cnt, P, Cc, None)
    torch.cuda.synchronize()
    if rc == 0 or b"class codes are outside" in lib.depgan_last_error():
        assert list(cnt[Cc + 3:]) == [-7] * (NCOUNT - Cc - 3)                 # nothing is written past C + 3 counts
    table = np.array(cen[:Cc * Cc], np.int64).reshape(Cc, Cc) if census else None
    return rc, probs.cpu().numpy(), dz.cpu().numpy(), loss.cpu().numpy(), np.array(cnt[:Cc + 3], np.int64), table


def _want_counts(codes, w, ign, Cc):
    """[den, ignored, bad, n_0 .. n_{C-1}] of class codes by NumPy."""
    c = codes.astype(np.int64)
    ig = (c == ign) if ign >= 0 else np.zeros(c.shape, bool)
    bad = ~ig & (c >= Cc)
    ok = ~ig & ~bad
    n = np.bincount(c[ok], minlength=Cc)
    den = int(sum(n[k] for k in range(Cc) if w[k] != 0))
    return np.array([den, ig.sum(), bad.sum()] + list(n), np.int64)


@pytest.mark.parametrize("P", PIXELS)
@pytest.mark.parametrize("Cc", CLASSES)
def test_unit_weights_are_the_unweighted_bits(lib, Cc, P):
    """1. unit weights, no ignore code, both label forms: probabilities, dz and the loss sum of depgan_op_softmax_ce."""
    z, codes = _case(Cc, P)
    onehot = np.eye(Cc, dtype=np.float32)[codes]
    for oh, cd in ((None, codes), (onehot, None)):
        rc0, p0, d0, l0 = _plain(lib, z, oh, cd, Cc)
        rc1, p1, d1, l1, cnt, _ = _weighted(lib, z, oh, cd, np.ones(Cc), -1, Cc)
        assert rc0 == 0 and rc1 == 0, lib.depgan_last_error()
        assert np.array_equal(_u32(p0), _u32(p1)) and np.array_equal(_u32(d0), _u32(d1)) and np.array_equal(_u32(l0), _u32(l1))
        assert np.isfinite(d1).all() and np.isfinite(l1).all()
        assert cnt[0] == P and np.array_equal(cnt, _want_counts(codes, np.ones(Cc), -1, Cc)), cnt


@pytest.mark.parametrize("P", [255, 3219, 262181])
@pytest.mark.parametrize("Cc", CLASSES)
def test_ignore_code_equals_zero_rows(lib, Cc, P):
    """2. codes with ignore code 255 against the one-hot encoding whose ignored rows are all zero, the same weights."""
    z, codes = _case(Cc, P)
    rng = np.random.default_rng(Cc + P)
    codes = codes.copy()
    codes[rng.uniform(size=P) < 0.3] = 255
    w = np.array([0.0, 1.25, 0.7, 3.0, 0.5, 1.0, 2.0, 7.25], np.float32)[:Cc]
    w[Cc - 1] = 7.25
    onehot = R.onehot_rows(codes, Cc, 255)
    a = _weighted(lib, z, None, codes, w, 255, Cc, census=True)
    b = _weighted(lib, z, onehot, None, w, -1, Cc, census=True)
    assert a[0] == 0 and b[0] == 0, lib.depgan_last_error()
    for u, v in zip(a[1:4], b[1:4]):
        assert np.array_equal(_u32(u), _u32(v))
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
    assert np.array_equal(a[4], _want_counts(codes, w, 255, Cc)) and 0 < a[4][0] < P
    assert np.all(a[2][codes == 255] == 0.0) and np.isfinite(a[1]).all()


@pytest.mark.parametrize("P", [255, 3219])
@pytest.mark.parametrize("Cc", CLASSES)
def test_power_of_two_weights_scale_rows_exactly(lib, Cc, P):
    """3. cw[k] = 2^e_k: row i of dz is ldexp(the unweighted row, e[code_i]) bit for bit (moderate logits, no denormals:
    the smallest |dz| entry is checked to be normal before and after the scaling)."""
    rng = np.random.default_rng(31 * Cc + P)
    z = (1.5 * rng.standard_normal((P, Cc))).astype(np.float32)
    codes = rng.integers(0, Cc, P).astype(np.uint8)
    e = np.array([-2, 3, 0, 1, -1, 2, -3, 4])[:Cc]
    w = np.ldexp(1.0, e).astype(np.float32)
    rc0, p0, d0, _ = _plain(lib, z, None, codes, Cc)
    rc1, p1, d1, _, cnt, _ = _weighted(lib, z, None, codes, w, -1, Cc)
    assert rc0 == 0 and rc1 == 0, lib.depgan_last_error()
    assert cnt[0] == P
    want = np.ldexp(d0, e[codes][:, None]).astype(np.float32)
    tiny = np.finfo(np.float32).tiny
    assert np.abs(d0[d0 != 0]).min() > 16 * tiny and np.abs(want[want != 0]).min() > 16 * tiny
    assert np.array_equal(_u32(want), _u32(d1)) and np.array_equal(_u32(p0), _u32(p1))


@pytest.mark.parametrize("Cc", CLASSES)
def test_half_the_pixels_ignored_doubles_the_kept_rows(lib, Cc):
    """4. P = 4096 with exactly 2048 pixels ignored: 1 / den = 2 / P exactly, so the kept rows of dz are twice the
    unweighted rows, the ignored rows are 0 and the probabilities keep their bits."""
    P = 4096
    rng = np.random.default_rng(77 + Cc)
    z = (1.5 * rng.standard_normal((P, Cc))).astype(np.float32)
    codes = rng.integers(0, Cc, P).astype(np.uint8)
    ign = np.zeros(P, bool)
    ign[rng.permutation(P)[:2048]] = True
    rc0, p0, d0, _ = _plain(lib, z, None, codes, Cc)
    marked = np.where(ign, 255, codes).astype(np.uint8)
    rc1, p1, d1, _, cnt, _ = _weighted(lib, z, None, marked, np.ones(Cc), 255, Cc)
    assert rc0 == 0 and rc1 == 0, lib.depgan_last_error()
    assert cnt[0] == 2048 and cnt[1] == 2048 and cnt[2] == 0
    assert np.array_equal(_u32(d1[~ign]), _u32(np.float32(2.0) * d0[~ign]))
    assert np.all(d1[ign] == 0.0) and np.abs(d0[ign]).max() > 0
    assert np.array_equal(_u32(p0), _u32(p1))


@functools.lru_cache(maxsize=None)
def _ref_case(Cc, hi):
    """Logits and codes for the float64 comparison: 3 sigma normal rows, ties, all-equal rows, +-100 spreads, and rows on
    either side of both clip bounds (true class `hi` with a gap g: q = 1 / (1 + (C - 1) exp(-g)) around 1 - 1e-7; true
    class C - 1 a gap below the others: q around 1e-7)."""
    rng = np.random.default_rng(500 + Cc)
    P = 12000
    z = (3.0 * rng.standard_normal((P, Cc))).astype(np.float32)
    share = np.full(Cc, 0.99 / (Cc - 1))
    share[Cc - 1] = 0.01
    codes = rng.choice(Cc, size=P, p=share).astype(np.uint8)
    r = np.arange(P)
    tie = r[r % 11 == 1]
    z[tie, 0] = z[tie, Cc - 1] = (z[tie].max(-1) + np.float32(0.75)).astype(np.float32)
    z[r % 11 == 2] = np.float32(0.3125)
    z[r % 11 == 3] *= np.float32(100.0 / 3.0)
    g = np.linspace(14.0, 19.5, 1000, dtype=np.float32)
    z[:1000] = 0.0
    z[:1000, hi] = g
    codes[:1000] = hi
    z[1000:2000] = 0.0
    z[1000:2000, Cc - 1] = -g
    codes[1000:2000] = Cc - 1
    return z, codes


@pytest.mark.parametrize("ign", [255, 0])
@pytest.mark.parametrize("Cc", CLASSES)
def test_against_float64(lib, Cc, ign):
    """5. a zero-weight class and a heavy rare class; ignore code 255 (30 % of the pixels marked) or 0, a real class."""
    z, codes = _ref_case(Cc, Cc - 1 if ign == 255 else 1)
    P = len(z)
    codes = codes.copy()
    if ign == 255:
        w = np.array([0.0, 1.25, 0.7, 3.0, 0.5, 1.0, 2.0, 7.25], np.float32)[:Cc]
        w[Cc - 1] = 7.25
        mark = np.random.default_rng(Cc).uniform(size=P) < 0.3
        mark[:2000:2] = False
        codes[mark] = 255
    else:
        w = np.array([0.5, 1.25, 7.25, 0.0, 3.0, 1.0, 2.0, 7.25], np.float32)[:Cc]
        if Cc > 3:
            w[Cc - 1] = 7.25
    t = R.onehot_rows(codes, Cc, ign)
    rc, p, dz, ls, cnt, _ = _weighted(lib, z, None, codes, w, ign, Cc)
    assert rc == 0, lib.depgan_last_error()
    p64, g64, total, den = R.softmax_ce_weighted_ref(z, t, w)
    assert cnt[0] == den and 0 < den < P
    assert np.isfinite(p).all() and np.isfinite(dz).all() and np.isfinite(ls).all()
    print("C = %d ignore %d: den %d of %d; probabilities %.2e; dz %.2e of max|dz| %.2e; loss sum %.6f (fp64 %.6f)"
          % (Cc, ign, den, P, np.abs(p - p64).max(), np.abs(dz - g64).max(), np.abs(g64).max(), float(ls[0]), total))
    assert np.abs(p - p64).max() <= 1e-6
    assert np.abs(dz - g64).max() <= 1e-5 * np.abs(g64).max()
    assert abs(float(ls[0]) - total) <= 1e-5 * total, (float(ls[0]), total)
    # ignored and zero-weight pixels: a dz row of zeros, whatever the logits
    wi = (t * w).sum(-1)
    assert (wi == 0).sum() > 100 and np.all(dz[wi == 0] == 0.0)
    # outside the clip the true class's gradient is cut: the whole pixel's dz is exactly 0
    q = (p64 * t).sum(-1)
    out = (wi != 0) & ((q > 1.0 - 0.5e-7) | (q < 0.5e-7))
    assert out.sum() > 50 and np.all(dz[out] == 0.0)
    inside = (wi != 0) & (q > 1e-6) & (q < 1.0 - 1e-4)
    assert np.all(np.abs(dz[inside]).max(-1) > 0)


@pytest.mark.parametrize("Cc", [2, 4, 8])
def test_everything_ignored(lib, Cc):
    """5. den = 0: loss sum 0, dz all zero, status 0; the probabilities are still written."""
    z, _ = _case(Cc, 3219)
    codes = np.full(3219, 255, np.uint8)
    rc, p, dz, ls, cnt, cen = _weighted(lib, z, None, codes, np.ones(Cc), 255, Cc, census=True)
    assert rc == 0, lib.depgan_last_error()
    assert cnt[0] == 0 and cnt[1] == 3219 and cnt[2:].sum() == 0 and cen.sum() == 0
    assert float(ls[0]) == 0.0 and np.all(dz == 0.0)
    assert np.array_equal(_u32(p), _u32(_plain(lib, z, None, None, Cc)[1]))
    # a zero-weight class alone fills the batch: den 0 as well, the class keeps its census bin
    codes = np.zeros(3219, np.uint8)
    w = np.ones(Cc, np.float32)
    w[0] = 0.0
    rc, p, dz, ls, cnt, cen = _weighted(lib, z, None, codes, w, -1, Cc, census=True)
    assert rc == 0 and cnt[0] == 0 and cnt[1] == 0 and cnt[3] == 3219 and cen[0].sum() == 3219
    assert float(ls[0]) == 0.0 and np.all(dz == 0.0)


@pytest.mark.parametrize("P", PIXELS)
@pytest.mark.parametrize("Cc", CLASSES)
def test_census_and_label_counts(lib, Cc, P):
    """6. the census under the mode is np.add.at over the pixels with a true class; census on and off give the same
    floats; the label counts are np.bincount for both label forms; a bad code that is not the ignore code is status 1."""
    z, codes = _case(Cc, P)
    rng = np.random.default_rng(9 * Cc + P)
    codes = codes.copy()
    codes[rng.uniform(size=P) < 0.25] = 254                                # the ignore code of this test
    w = np.linspace(0.5, 2.0, Cc).astype(np.float32)
    w[0] = 0.0
    on = _weighted(lib, z, None, codes, w, 254, Cc, census=True)
    off = _weighted(lib, z, None, codes, w, 254, Cc)
    assert on[0] == 0 and off[0] == 0, lib.depgan_last_error()
    for u, v in zip(on[1:4], off[1:4]):
        assert np.array_equal(_u32(u), _u32(v))
    assert np.array_equal(on[4], off[4]) and np.array_equal(on[4], _want_counts(codes, w, 254, Cc))
    keep = codes < Cc
    cm = np.zeros((Cc, Cc), np.int64)
    np.add.at(cm, (codes[keep].astype(np.int64), np.argmax(on[1][keep], -1)), 1)
    assert np.array_equal(on[5], cm)
    assert int(on[5].sum()) + int(on[4][2]) + int(on[4][1]) == P and on[4][2] == 0
    assert np.array_equal(on[5].sum(-1), on[4][3:])                          # a zero-weight class keeps its bin
    # depgan_op_label_counts: codes and their one-hot encoding (zero rows for the ignored)
    out = (C.c_longlong * NCOUNT)(*([-7] * NCOUNT))
    cd = torch.from_numpy(codes).cuda()
    assert lib.depgan_op_label_counts(None, P_(cd), P, Cc, 254, out, None) == 0, lib.depgan_last_error()
    want = _want_counts(codes, np.ones(Cc), 254, Cc)
    assert np.array_equal(np.array(out[:Cc + 3], np.int64), want) and list(out[Cc + 3:]) == [-7] * (NCOUNT - Cc - 3)
    od = torch.from_numpy(R.onehot_rows(codes, Cc, 254)).cuda()
    out2 = (C.c_longlong * NCOUNT)()
    assert lib.depgan_op_label_counts(P_(od), None, P, Cc, -1, out2, None) == 0, lib.depgan_last_error()
    assert np.array_equal(np.array(out2[:Cc + 3], np.int64), want)
    # without the ignore code the same bytes are out of range: counted, not refused by the counting entry
    assert lib.depgan_op_label_counts(None, P_(cd), P, Cc, -1, out2, None) == 0
    assert out2[1] == 0 and out2[2] == want[1] and out2[0] == want[0]
    # a bad code that is not the ignore code: status 1 with its count, everything written
    if P >= 255:
        bad = codes.copy()
        where = rng.choice(P, size=41, replace=False)
        bad[where] = np.array([Cc, Cc + 1, 255], np.uint8)[np.arange(41) % 3]
        rc, p, dz, ls, cnt, cen = _weighted(lib, z, None, bad, w, 254, Cc, census=True)
        assert rc == 1
        msg = lib.depgan_last_error()
        assert b"%d of %d" % (41, P) in msg and b"[0, %d)" % Cc in msg, msg
        assert np.array_equal(cnt, _want_counts(bad, w, 254, Cc)) and cnt[2] == 41
        assert int(cen.sum()) + 41 + int(cnt[1]) == P


@pytest.mark.parametrize("Cc,P", [(4, 3219), (8, 262181), (3, 255)])
def test_a_second_call_into_the_same_buffers_repeats_the_result(lib, Cc, P):
    """6. no stale partial and no dependence on zeroing: the same device buffers, other labels in between."""
    z, codes = _case(Cc, P)
    codes = codes.copy()
    codes[::5] = 255
    zd, cd = torch.from_numpy(z).cuda(), torch.from_numpy(codes).cuda()
    probs, dz, loss = torch.empty((P, Cc), device="cuda:0"), torch.empty((P, Cc), device="cuda:0"), torch.empty(1, device="cuda:0")
    w = (C.c_float * Cc)(*np.linspace(0.5, 2.0, Cc))
    cen, cnt = (C.c_longlong * 64)(), (C.c_longlong * NCOUNT)()

    def call(c_dev):
        rc = lib.depgan_op_softmax_ce_weighted(P_(zd), None, P_(c_dev), w, Cc, 255, P_(probs), P_(dz), P_(loss), cen, cnt, P,
                                               Cc, None)
        torch.cuda.synchronize()
        return rc, _u32(dz).copy(), _u32(loss).copy(), list(cnt), list(cen)

    first = call(cd)
    assert first[0] == 0, lib.depgan_last_error()
    other = call(torch.from_numpy(((codes.astype(np.int64) + 1) % Cc).astype(np.uint8)).cuda())
    assert other[0] == 0 and other[3] != first[3]
    again = call(cd)
    assert again[0] == 0 and all(np.array_equal(u, v) for u, v in zip(first[1:], again[1:]))


@pytest.mark.parametrize("what,w,n,ign", [
    ("negative", [1.0, -0.5, 1.0, 1.0], None, -1), ("nan", [1.0, float("nan"), 1.0, 1.0], None, -1),
    ("inf", [1.0, float("inf"), 1.0, 1.0], None, -1), ("all zero", [0.0, 0.0, 0.0, 0.0], None, -1),
    ("n != C", [1.0, 1.0, 1.0], None, -1), ("n != C", [1.0, 1.0, 1.0, 1.0, 1.0], None, -1),
    ("ignore", [1.0, 1.0, 1.0, 1.0], None, -2), ("ignore", [1.0, 1.0, 1.0, 1.0], None, 256)])
def test_refused_before_any_launch(lib, what, w, n, ign):
    """7. status 1 with a message, and the NaN-filled outputs are untouched."""
    z, codes = _case(4, 255)
    rc, p, dz, ls, cnt, _ = _weighted(lib, z, None, codes, w, ign, 4, n=n)
    assert rc == 1, what
    assert lib.depgan_last_error()
    assert np.isnan(p).all() and np.isnan(dz).all() and np.isnan(ls).all() and list(cnt) == [-7] * 7
    out = (C.c_longlong * NCOUNT)(*([-7] * NCOUNT))
    if what == "ignore":
        cd = torch.from_numpy(codes).cuda()
        assert lib.depgan_op_label_counts(None, P_(cd), 255, 4, ign, out, None) == 1 and list(out) == [-7] * NCOUNT
