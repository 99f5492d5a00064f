"""GPU: depgan_op_softmax_ce_focal, the focal mode (focal cross-entropy and label smoothing) at operator level.

Exact statements are bit for bit: codes with an ignore code against the one-hot encoding with all-zero rows, the census
on against off, the probabilities against depgan_op_softmax_ce, weights that are powers of two against ldexp of the
unit-weight focal rows, and half the pixels ignored (den = P / 2, so 1 / den = 2 / P exactly).  Against float64
(tests/focal_ce_ref.py) the bounds are the kernel's existing ones: probabilities 1e-6, dz 1e-5 max|dz|, the loss sum 1e-5
relative.  P = 1 is one thread, 255 a ragged block, 3219 a ragged grid of 13 blocks, 262181 is 37 pixels past the
1024-block cap where the grid-stride loop takes over.

The first device run printed, the worst over the ten (gamma, eps) settings of test_against_float64 per class count
(probabilities; dz as a fraction of max|dz|; the loss sum relative): C = 2: 8.8e-8, 2.6e-7, 1.5e-7; C = 3: 1.4e-7, 2.8e-7,
1.5e-7; C = 4: 1.6e-7, 3.0e-7, 1.1e-7; C = 5: 2.3e-7, 3.0e-7, 9.0e-8; C = 8: 2.4e-7, 2.7e-7, 1.3e-7."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import focal_ce_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu
CLASSES = [2, 3, 4, 5, 8]
PIXELS = [1, 255, 3219, 262181]
NCOUNT = 11
SETTINGS = [(g, e) for g in (0.5, 1.0, 2.0, 5.0) for e in (0.0, 0.1)] + [(0.0, 0.1), (2.0, 0.0)]
WEIGHTS = np.array([0.0, 1.25, 0.7, 3.0, 0.5, 1.0, 2.0, 7.25], np.float32)


def P_(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _u32(t):
    return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(Cc, P):
    """(logits (P, Cc) float32, codes (P,) uint8): standard-normal rows, every 7th with a tied maximum, every 7th all
    equal, every 7th spread by +-100; one class is rare (about 1 % of the pixels).  Read-only."""
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
    z.setflags(write=False)
    codes.setflags(write=False)
    return z, codes


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda() if a is not None else None


def _outputs(P, Cc):
    return (torch.full((P, Cc), float("nan"), device="cuda:0"), torch.full((P, Cc), float("nan"), device="cuda:0"),
            torch.full((1,), float("nan"), device="cuda:0"))


def _plain(lib, z, Cc):
    """depgan_op_softmax_ce without labels: the probabilities."""
    P = len(z)
    zd = _dev(z)
    probs = torch.full((P, Cc), float("nan"), device="cuda:0")
    assert lib.depgan_op_softmax_ce(P_(zd), None, None, P_(probs), None, None, P, Cc, None) == 0, lib.depgan_last_error()
    torch.cuda.synchronize()
    return probs.cpu().numpy()


def _call(lib, focal, z, onehot, codes, w, ign, Cc, census=False):
    """One call into fresh NaN-filled outputs and sentinel-filled counts; focal = (gamma, eps), or None for
    depgan_op_softmax_ce_weighted: (rc, probs, dz, loss sum, counts int64 (C + 3), census (C, C) or None)."""
    P = len(z)
    zd, od, cd = _dev(z), _dev(onehot), _dev(codes)
    probs, dz, loss = _outputs(P, Cc)
    wa = (C.c_float * len(w))(*[float(v) for v in w]) if w is not None else None
    n = len(w) if w is not None else 0
    cnt = (C.c_longlong * NCOUNT)(*([-7] * NCOUNT))
    cen = (C.c_longlong * 64)(*([-7] * 64)) if census else None
    if focal is None:
        rc = lib.depgan_op_softmax_ce_weighted(P_(zd), P_(od), P_(cd), wa, n, ign, P_(probs), P_(dz), P_(loss), cen, cnt, P,
                                               Cc, None)
    else:
        rc = lib.depgan_op_softmax_ce_focal(P_(zd), P_(od), P_(cd), wa, n, ign, focal[0], focal[1], P_(probs), P_(dz),
                                            P_(loss), cen, cnt, P, Cc, None)
    torch.cuda.synchronize()
    if rc == 0 or b"class codes are outside" in lib.depgan_last_error():
        assert list(cnt[Cc + 3:]) == [-7] * (NCOUNT - Cc - 3)                 # nothing is written past C + 3 counts
        if census:
            assert list(cen[Cc * Cc:]) == [-7] * (64 - Cc * Cc)
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


def _weights(Cc):
    w = WEIGHTS[:Cc].copy()
    w[Cc - 1] = 7.25
    return w


@pytest.mark.parametrize("P", PIXELS)
@pytest.mark.parametrize("Cc", CLASSES)
def test_ignore_code_equals_zero_rows(lib, Cc, P):
    """1. codes with ignore code 255 against the one-hot encoding whose ignored rows are all zero: gamma = 2, eps = 0.1,
    weights with a zero entry."""
    z, codes = _case(Cc, P)
    rng = np.random.default_rng(Cc + P)
    codes = codes.copy()
    codes[rng.uniform(size=P) < 0.3] = 255
    w = _weights(Cc)
    onehot = F.onehot_rows(codes, Cc, 255)
    a = _call(lib, (2.0, 0.1), z, None, codes, w, 255, Cc, census=True)
    b = _call(lib, (2.0, 0.1), z, onehot, None, w, -1, Cc, census=True)
    assert a[0] == 0 and b[0] == 0, lib.depgan_last_error()
    for u, v in zip(a[1:4], b[1:4]):
        assert np.array_equal(_u32(u), _u32(v))
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
    assert np.array_equal(a[4], _want_counts(codes, w, 255, Cc))
    assert np.all(a[2][codes == 255] == 0.0) and np.isfinite(a[1]).all() and np.isfinite(a[2]).all() and np.isfinite(a[3]).all()
    if P >= 255:
        assert 0 < a[4][0] < P and np.abs(a[2]).max() > 0 and float(a[3][0]) > 0


@pytest.mark.parametrize("P", PIXELS)
@pytest.mark.parametrize("Cc", CLASSES)
def test_census_on_and_off_and_the_plain_probabilities(lib, Cc, P):
    """2. census on and off give the same floats; the probabilities are depgan_op_softmax_ce's bits; the census is
    np.add.at over the ORIGINAL codes and the stored probabilities (smoothing does not move the true class)."""
    z, codes = _case(Cc, P)
    rng = np.random.default_rng(9 * Cc + P)
    codes = codes.copy()
    codes[rng.uniform(size=P) < 0.25] = 254                                # the ignore code of this test
    w = np.linspace(0.5, 2.0, Cc).astype(np.float32)
    w[0] = 0.0
    for lab in ("codes", "onehot"):
        oh = F.onehot_rows(codes, Cc, 254) if lab == "onehot" else None
        cd, ign = (None, -1) if lab == "onehot" else (codes, 254)
        on = _call(lib, (2.0, 0.1), z, oh, cd, w, ign, Cc, census=True)
        off = _call(lib, (2.0, 0.1), z, oh, cd, w, ign, Cc)
        assert on[0] == 0 and off[0] == 0, lib.depgan_last_error()
        for u, v in zip(on[1:4], off[1:4]):
            assert np.array_equal(_u32(u), _u32(v))
        assert np.array_equal(on[4], off[4]) and np.array_equal(on[4], _want_counts(codes, w, 254, Cc))
        assert np.array_equal(_u32(on[1]), _u32(_plain(lib, z, Cc)))
        keep = codes < Cc
        cm = np.zeros((Cc, Cc), np.int64)
        np.add.at(cm, (codes[keep].astype(np.int64), np.argmax(on[1][keep], -1)), 1)
        assert np.array_equal(on[5], cm)
        assert int(on[5].sum()) + int(on[4][1]) == P and on[4][2] == 0
        assert np.array_equal(on[5].sum(-1), on[4][3:])                      # a zero-weight class keeps its bin


@pytest.mark.parametrize("P", [255, 3219])
@pytest.mark.parametrize("Cc", CLASSES)
def test_power_of_two_weights_scale_rows_exactly(lib, Cc, P):
    """3. cw[k] = 2^e_k: row i of dz is ldexp(the unit-weight focal row, e[code_i]) bit for bit (moderate logits, no
    denormals: the smallest |dz| entry is checked to be normal before and after the scaling)."""
    rng = np.random.default_rng(31 * Cc + P)
    z = (1.5 * rng.standard_normal((P, Cc))).astype(np.float32)
    codes = rng.integers(0, Cc, P).astype(np.uint8)
    e = np.array([-2, 3, 0, 1, -1, 2, -3, 4])[:Cc]
    w = np.ldexp(1.0, e).astype(np.float32)
    for focal in ((2.0, 0.1), (0.5, 0.0)):
        rc0, p0, d0, _, cnt0, _ = _call(lib, focal, z, None, codes, None, -1, Cc)
        rc1, p1, d1, _, cnt, _ = _call(lib, focal, z, None, codes, w, -1, Cc)
        assert rc0 == 0 and rc1 == 0, lib.depgan_last_error()
        assert cnt[0] == P == cnt0[0]
        want = np.ldexp(d0, e[codes][:, None]).astype(np.float32)
        tiny = np.finfo(np.float32).tiny
        assert np.abs(d0[d0 != 0]).min() > 16 * tiny and np.abs(want[want != 0]).min() > 16 * tiny
        assert np.array_equal(_u32(want), _u32(d1)) and np.array_equal(_u32(p0), _u32(p1))
        assert np.abs(d0).max() > 0


@pytest.mark.parametrize("Cc", CLASSES)
def test_half_the_pixels_ignored_doubles_the_kept_rows(lib, Cc):
    """4. P = 4096 with exactly 2048 pixels ignored: 1 / den = 2 / P exactly, so the kept rows of dz are twice the
    all-kept rows, the ignored rows are 0 and the probabilities keep their bits."""
    P = 4096
    rng = np.random.default_rng(77 + Cc)
    z = (1.5 * rng.standard_normal((P, Cc))).astype(np.float32)
    codes = rng.integers(0, Cc, P).astype(np.uint8)
    ign = np.zeros(P, bool)
    ign[rng.permutation(P)[:2048]] = True
    rc0, p0, d0, _, cnt0, _ = _call(lib, (2.0, 0.1), z, None, codes, None, -1, Cc)
    marked = np.where(ign, 255, codes).astype(np.uint8)
    rc1, p1, d1, _, cnt, _ = _call(lib, (2.0, 0.1), z, None, marked, None, 255, Cc)
    assert rc0 == 0 and rc1 == 0, lib.depgan_last_error()
    assert cnt0[0] == P and cnt[0] == 2048 and cnt[1] == 2048 and cnt[2] == 0
    assert np.array_equal(_u32(d1[~ign]), _u32(np.float32(2.0) * d0[~ign]))
    assert np.all(d1[ign] == 0.0) and np.abs(d0[ign]).max() > 0
    assert np.array_equal(_u32(p0), _u32(p1))


@pytest.mark.parametrize("Cc", CLASSES)
def test_against_float64(lib, Cc):
    """5. the loss-weight test's inputs (clip bounds, ties, +-100 spreads, 30 % ignored, a zero-weight class and a 7.25
    class) under ten (gamma, eps) settings."""
    z, codes, w = F.ref_case(Cc)
    P = len(z)
    t = F.onehot_rows(codes, Cc, 255)
    wi = (t * w).sum(-1)
    assert (wi == 0).sum() > 100
    for gamma, eps in SETTINGS:
        rc, p, dz, ls, cnt, _ = _call(lib, (gamma, eps), z, None, codes, w, 255, Cc)
        assert rc == 0, lib.depgan_last_error()
        p64, g64, total, den = F.softmax_ce_focal_ref(z, t, w, gamma, eps)
        assert cnt[0] == den and 0 < den < P
        assert np.isfinite(p).all() and np.isfinite(dz).all() and np.isfinite(ls).all()
        print("C = %d gamma %.1f eps %.1f: den %d of %d; probabilities %.2e; dz %.2e of max|dz| %.2e (%.2e relative); "
              "loss sum %.6f (fp64 %.6f, %.2e relative)"
              % (Cc, gamma, eps, den, P, np.abs(p - p64).max(), np.abs(dz - g64).max(), np.abs(g64).max(),
                 np.abs(dz - g64).max() / np.abs(g64).max(), float(ls[0]), total, abs(float(ls[0]) - total) / total))
        assert np.abs(p - p64).max() <= 1e-6
        assert np.abs(dz - g64).max() <= 1e-5 * np.abs(g64).max()
        assert abs(float(ls[0]) - total) <= 1e-5 * total, (float(ls[0]), total)
        # ignored and zero-weight pixels: a dz row of zeros, whatever the logits
        assert np.all(dz[wi == 0] == 0.0)
        q = (p64 * t).sum(-1)
        if eps == 0.0:
            # outside the clip the true class's gradient is cut: the whole pixel's dz is exactly 0
            out = (wi != 0) & ((q > 1.0 - 0.5e-7) | (q < 0.5e-7))
            assert out.sum() > 50 and np.all(dz[out] == 0.0)
        inside = (wi != 0) & (q > 1e-6) & (q < 1.0 - 1e-4)
        assert np.all(np.abs(dz[inside]).max(-1) > 0)


@pytest.mark.parametrize("P", [255, 3219, 262181])
@pytest.mark.parametrize("Cc", CLASSES)
def test_gamma_zero_and_no_smoothing_is_the_weighted_loss(lib, Cc, P):
    """6. gamma = 0, eps = 0 through this entry: den, counts, census and probabilities of depgan_op_softmax_ce_weighted;
    dz and the loss sum within the float64 bounds of it (the statements differ: they need not be the same bits)."""
    z, codes = _case(Cc, P)
    codes = codes.copy()
    codes[np.random.default_rng(3 * Cc + P).uniform(size=P) < 0.3] = 255
    w = _weights(Cc)
    a = _call(lib, (0.0, 0.0), z, None, codes, w, 255, Cc, census=True)
    b = _call(lib, None, z, None, codes, w, 255, Cc, census=True)
    assert a[0] == 0 and b[0] == 0, lib.depgan_last_error()
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]) and np.array_equal(_u32(a[1]), _u32(b[1]))
    assert np.abs(b[2]).max() > 0
    assert np.abs(a[2] - b[2]).max() <= 1e-5 * np.abs(b[2]).max()
    assert abs(float(a[3][0]) - float(b[3][0])) <= 1e-5 * float(b[3][0])
    # unit weights by a null pointer
    c = _call(lib, (0.0, 0.0), z, None, codes, None, 255, Cc)
    d = _call(lib, None, z, None, codes, np.ones(Cc), 255, Cc)
    assert c[0] == 0 and d[0] == 0 and np.array_equal(c[4], d[4])
    assert np.abs(c[2] - d[2]).max() <= 1e-5 * np.abs(d[2]).max()


@pytest.mark.parametrize("Cc", [2, 4, 8])
def test_everything_ignored(lib, Cc):
    """7. den = 0: loss sum 0, dz all zero, status 0; the probabilities are still written."""
    z, _ = _case(Cc, 3219)
    codes = np.full(3219, 255, np.uint8)
    rc, p, dz, ls, cnt, cen = _call(lib, (2.0, 0.1), z, None, codes, None, 255, Cc, census=True)
    assert rc == 0, lib.depgan_last_error()
    assert cnt[0] == 0 and cnt[1] == 3219 and cnt[2:].sum() == 0 and cen.sum() == 0
    assert float(ls[0]) == 0.0 and np.all(dz == 0.0)
    assert np.array_equal(_u32(p), _u32(_plain(lib, z, Cc)))
    # all-zero one-hot rows, no weights: the same
    rc, p, dz, ls, cnt, cen = _call(lib, (2.0, 0.1), z, np.zeros((3219, Cc), np.float32), None, None, -1, Cc, census=True)
    assert rc == 0 and cnt[0] == 0 and cnt[1] == 3219 and cen.sum() == 0
    assert float(ls[0]) == 0.0 and np.all(dz == 0.0)
    # a zero-weight class alone fills the batch: den 0 as well, the class keeps its census bin, smoothing adds nothing
    codes = np.zeros(3219, np.uint8)
    w = np.ones(Cc, np.float32)
    w[0] = 0.0
    rc, p, dz, ls, cnt, cen = _call(lib, (2.0, 0.1), z, None, codes, w, -1, Cc, census=True)
    assert rc == 0 and cnt[0] == 0 and cnt[1] == 0 and cnt[3] == 3219 and cen[0].sum() == 3219
    assert float(ls[0]) == 0.0 and np.all(dz == 0.0)


@pytest.mark.parametrize("Cc,P", [(4, 3219), (8, 262181), (3, 255)])
def test_a_second_call_into_the_same_buffers_repeats_the_result(lib, Cc, P):
    """8. no stale partial and no dependence on zeroing: the same device buffers, other labels in between."""
    z, codes = _case(Cc, P)
    codes = codes.copy()
    codes[::5] = 255
    zd, cd = _dev(z), _dev(codes)
    probs, dz, loss = torch.empty((P, Cc), device="cuda:0"), torch.empty((P, Cc), device="cuda:0"), torch.empty(1, device="cuda:0")
    w = (C.c_float * Cc)(*np.linspace(0.5, 2.0, Cc))
    cen, cnt = (C.c_longlong * 64)(), (C.c_longlong * NCOUNT)()

    def call(c_dev):
        rc = lib.depgan_op_softmax_ce_focal(P_(zd), None, P_(c_dev), w, Cc, 255, 2.0, 0.1, P_(probs), P_(dz), P_(loss), cen,
                                            cnt, P, Cc, None)
        torch.cuda.synchronize()
        return rc, _u32(dz).copy(), _u32(loss).copy(), list(cnt), list(cen)

    first = call(cd)
    assert first[0] == 0, lib.depgan_last_error()
    other = call(_dev(((codes.astype(np.int64) + 1) % Cc).astype(np.uint8)))
    assert other[0] == 0 and other[3] != first[3] and not np.array_equal(other[1], first[1])
    again = call(cd)
    assert again[0] == 0 and all(np.array_equal(u, v) for u, v in zip(first[1:], again[1:]))


@pytest.mark.parametrize("Cc,P", [(2, 255), (4, 3219), (5, 262181)])
def test_a_bad_code_is_counted_and_reported(lib, Cc, P):
    """9. a code >= C that is not the ignore code: status 1 with its count, everything written."""
    z, codes = _case(Cc, P)
    rng = np.random.default_rng(5 * Cc + P)
    bad = codes.copy()
    bad[rng.uniform(size=P) < 0.25] = 254                                  # the ignore code
    where = rng.choice(P, size=41, replace=False)
    bad[where] = np.array([Cc, Cc + 1, 255], np.uint8)[np.arange(41) % 3]
    w = _weights(Cc)
    rc, p, dz, ls, cnt, cen = _call(lib, (2.0, 0.1), z, None, bad, w, 254, Cc, census=True)
    assert rc == 1
    msg = lib.depgan_last_error()
    assert b"%d of %d" % (41, P) in msg and b"[0, %d)" % Cc in msg, msg
    assert np.array_equal(cnt, _want_counts(bad, w, 254, Cc)) and cnt[2] == 41
    assert int(cen.sum()) + 41 + int(cnt[1]) == P
    assert np.isfinite(p).all() and np.isfinite(dz).all() and np.isfinite(ls).all() and np.all(dz[where] == 0.0)
    assert np.array_equal(_u32(p), _u32(_plain(lib, z, Cc)))


@pytest.mark.parametrize("what,kw", [
    ("gamma < 0", {"gamma": -1.0}), ("gamma nan", {"gamma": float("nan")}), ("gamma inf", {"gamma": float("inf")}),
    ("eps < 0", {"eps": -0.1}), ("eps = 1", {"eps": 1.0}), ("eps nan", {"eps": float("nan")}),
    ("negative weight", {"w": [1.0, -0.5, 1.0, 1.0]}), ("n != C", {"w": [1.0, 1.0, 1.0]}), ("ignore", {"ign": 256})])
def test_refused_before_any_launch(lib, what, kw):
    """status 1 with a message, and the NaN-filled outputs and the sentinel counts are untouched."""
    z, codes = _case(4, 255)
    a = dict(gamma=2.0, eps=0.1, w=[1.0, 1.0, 1.0, 1.0], ign=-1)
    a.update(kw)
    rc, p, dz, ls, cnt, _ = _call(lib, (a["gamma"], a["eps"]), z, None, codes, a["w"], a["ign"], 4)
    assert rc == 1, what
    assert lib.depgan_last_error()
    assert np.isnan(p).all() and np.isnan(dz).all() and np.isnan(ls).all() and list(cnt) == [-7] * 7
