"""GPU: depgan_op_dice_loss, the soft Dice loss at operator level, on probabilities stored by depgan_op_softmax_ce.

Exact statements are bit for bit: class codes against their one-hot encoding, codes with an ignore code against one-hot
with all-zero rows, a second call into the same buffers, saturated predictions (p exactly one-hot: the sums are the
np.bincount integers, a perfect prediction has loss 0.0 and an all-zero dz), pure Dice into a NaN-filled dz, dice_coef =
2^j against ldexp, and ce_coef = 2^j against the float32 restatement ce_coef * dz + the pure-Dice row (one rounding
either way the compiler contracts it).  Bounds: I_k and P_k against float64 sums of the device's own stored
probabilities, relative 2e-6 (at most 16 float roundings per partial chain, 2^-24 * 16, doubled; the second stage adds
in double); against float64 autograd (tests/dice_ref.py) dz within 1e-5 max|dz| and the loss within 1e-5 relative, the
softmax-CE bounds.  P = 1 is one thread, 255 a ragged block, 3219 a ragged grid of 13 blocks, 262181 is 37 pixels past
the 1024-block cap where the grid-stride loop takes over (and four 256-block chunks in the coefficient stage)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dice_ref as D  # noqa: E402
import weighted_ce_ref as R  # noqa: E402
from test_gpu_softmax_ce_weighted import CLASSES, PIXELS, P_, _case, _u32  # noqa: E402

pytestmark = pytest.mark.gpu
FLAT, CLASS = 1, 2
SMOOTH = 1e-7


@functools.lru_cache(maxsize=None)
def _probs(lib, Cc, P, saturate=None):
    """(probabilities float32 (P, Cc) as depgan_op_softmax_ce stores them, logits, codes).  saturate: None for
    _case's logits; 0 puts +100 on the label's class and -100 elsewhere, j > 0 puts the +100 j classes further on."""
    z, codes = _case(Cc, P)
    if saturate is not None:
        z = np.full((P, Cc), -100.0, np.float32)
        z[np.arange(P), (codes.astype(np.int64) + saturate) % Cc] = 100.0
    zd = torch.from_numpy(z).cuda()
    probs = torch.full((P, Cc), float("nan"), device="cuda:0")
    assert lib.depgan_op_softmax_ce(P_(zd), None, None, P_(probs), None, None, P, Cc, None) == 0, lib.depgan_last_error()
    torch.cuda.synchronize()
    p = probs.cpu().numpy()
    assert np.isfinite(p).all()
    return p, z, codes


def _dice(lib, p, onehot, codes, ign, form, coef, Cc, smooth=SMOOTH, ce=0.0, dw=1.0, dz_in=None, n=None):
    """One call: (rc, dz, sums float64 (3, Cc), loss).  dz starts as dz_in, or NaN-filled."""
    P = len(p)
    pd = torch.from_numpy(p).cuda()
    od = torch.from_numpy(onehot).cuda() if onehot is not None else None
    cd = torch.from_numpy(codes).cuda() if codes is not None else None
    dz = torch.from_numpy(dz_in).cuda() if dz_in is not None else torch.full((P, Cc), float("nan"), device="cuda:0")
    ca = (C.c_float * len(coef))(*[float(v) for v in coef]) if coef is not None else None
    sums, loss = (C.c_double * 24)(*([-7.0] * 24)), C.c_float(-7.0)
    rc = lib.depgan_op_dice_loss(P_(pd), P_(od), P_(cd), ign, form, ca, (len(coef) if coef is not None else 0) if n is None else n,
                                 smooth, ce, dw, P_(dz), sums, C.byref(loss), P, Cc, None)
    torch.cuda.synchronize()
    assert list(sums[3 * Cc:]) == [-7.0] * (24 - 3 * Cc)                       # nothing is written past 3 C sums
    return rc, dz.cpu().numpy(), np.array(sums[:3 * Cc], np.float64).reshape(3, Cc), float(loss.value)


def _same(a, b):
    assert a[0] == 0 and b[0] == 0
    assert np.array_equal(_u32(a[1]), _u32(b[1])) and np.array_equal(a[2], b[2])
    assert np.float32(a[3]).view(np.uint32) == np.float32(b[3]).view(np.uint32)


def _coef(Cc):
    c = np.array([0.0, 1.25, 0.7, 3.0, 0.5, 1.0, 2.0, 0.25], np.float32)[:Cc]
    c[Cc - 1] = 0.25
    return c


@pytest.mark.parametrize("P", PIXELS)
@pytest.mark.parametrize("Cc", CLASSES)
def test_codes_equal_their_one_hot_encoding(lib, Cc, P):
    """Codes give the bits of their one-hot encoding; codes with ignore code 255 the bits of one-hot with all-zero rows;
    T_k are the integer label counts; I_k and P_k are the float64 sums of the stored probabilities to 2e-6."""
    p, _, codes = _probs(lib, Cc, P)
    rng = np.random.default_rng(3 * Cc + P)
    d0 = (rng.standard_normal((P, Cc)) / P).astype(np.float32)
    marked = codes.copy()
    marked[::5] = 255
    for form, coef in ((FLAT, None), (CLASS, _coef(Cc))):
        a = _dice(lib, p, None, codes, -1, form, coef, Cc, ce=1.0, dz_in=d0)
        b = _dice(lib, p, R.onehot_rows(codes, Cc), None, -1, form, coef, Cc, ce=1.0, dz_in=d0)
        assert a[0] == 0, lib.depgan_last_error()
        _same(a, b)
        assert np.array_equal(a[2][2], np.bincount(codes, minlength=Cc)) and np.isfinite(a[1]).all()
        a = _dice(lib, p, None, marked, 255, form, coef, Cc, ce=1.0, dz_in=d0)
        b = _dice(lib, p, R.onehot_rows(marked, Cc, 255), None, 0, form, coef, Cc, ce=1.0, dz_in=d0)
        _same(a, b)
        keep = marked != 255
        assert np.array_equal(a[2][2], np.bincount(marked[keep], minlength=Cc))
        assert np.array_equal(_u32(a[1][~keep]), _u32(d0[~keep]))             # ce_coef = 1: an ignored row keeps its dz
        t = R.onehot_rows(marked, Cc, 255).astype(np.float64)
        p64 = p.astype(np.float64)
        want_i, want_p = (t * p64).sum(0), (p64 * keep[:, None]).sum(0)
        assert np.all(np.abs(a[2][0] - want_i) <= 2e-6 * want_i), (a[2][0], want_i)
        assert np.all(np.abs(a[2][1] - want_p) <= 2e-6 * want_p), (a[2][1], want_p)
        # the same one-hot rows with ignore_code = -1: the all-zero rows take part (they add to P_k alone)
        c = _dice(lib, p, R.onehot_rows(marked, Cc, 255), None, -1, form, coef, Cc, ce=1.0, dz_in=d0)
        assert c[0] == 0 and np.array_equal(c[2][2], a[2][2]) and np.array_equal(c[2][0], a[2][0])
        assert np.all(np.abs(c[2][1] - p64.sum(0)) <= 2e-6 * p64.sum(0))


@pytest.mark.parametrize("P", PIXELS)
@pytest.mark.parametrize("Cc", CLASSES)
def test_saturated_predictions_are_exact(lib, Cc, P):
    """Logits +-100: p is exactly one-hot.  Perfect: loss exactly 0.0 in both forms, dz exactly zero, I = P = T = the
    np.bincount integers.  Wrong (I = 0): the sums are exact integers, the loss within one float32 ulp of the float64
    formula."""
    p, _, codes = _probs(lib, Cc, P, 0)
    n = np.bincount(codes, minlength=Cc).astype(np.float64)
    assert np.array_equal(p, np.eye(Cc, dtype=np.float32)[codes])
    for form, coef in ((FLAT, None), (CLASS, None), (CLASS, _coef(Cc))):
        rc, dz, sums, loss = _dice(lib, p, None, codes, -1, form, coef, Cc)
        assert rc == 0, lib.depgan_last_error()
        assert loss == 0.0 and np.all(dz == 0.0)
        assert np.array_equal(sums, np.stack([n, n, n]))
    pw, _, _ = _probs(lib, Cc, P, 1)
    npred = np.bincount((codes.astype(np.int64) + 1) % Cc, minlength=Cc).astype(np.float64)
    s = float(np.float32(SMOOTH))
    for form, coef in ((FLAT, None), (CLASS, None), (CLASS, _coef(Cc))):
        rc, dz, sums, loss = _dice(lib, pw, None, codes, -1, form, coef, Cc)
        assert rc == 0 and np.isfinite(dz).all()
        assert np.array_equal(sums, np.stack([np.zeros(Cc), npred, n]))
        if form == FLAT:
            want = 1.0 - s / (n.sum() + npred.sum() + s)
        else:
            c = D.class_coef(Cc, coef)
            want = float((c * (1.0 - s / (n + npred + s))).sum())
        assert abs(loss - want) <= float(np.spacing(np.float32(want))), (loss, want)


@pytest.mark.parametrize("P", [255, 3219])
@pytest.mark.parametrize("Cc", CLASSES)
def test_pure_dice_does_not_read_dz_and_coefficients_scale_exactly(lib, Cc, P):
    """ce_coef = 0 into a NaN-filled dz gives finite values; dice_coef = 2^j gives ldexp of the dice_coef = 1 rows;
    ce_coef = 2^j gives float32(ce_coef * dz) + the pure row, one rounding."""
    p, _, codes = _probs(lib, Cc, P)
    marked = codes.copy()
    marked[::5] = 255
    rng = np.random.default_rng(11 * Cc + P)
    d0 = (rng.standard_normal((P, Cc)) / P).astype(np.float32)
    tiny = np.finfo(np.float32).tiny
    for form, coef in ((FLAT, None), (CLASS, _coef(Cc))):
        one = _dice(lib, p, None, marked, 255, form, coef, Cc)                 # dz starts as NaN
        assert one[0] == 0 and np.isfinite(one[1]).all() and np.abs(one[1]).max() > 0
        assert np.all(one[1][marked == 255] == 0.0)
        for j in (-3, 4):
            two = _dice(lib, p, None, marked, 255, form, coef, Cc, dw=2.0 ** j)
            want = np.ldexp(one[1], j).astype(np.float32)
            # the +-100 rows leave a few entries near the denormal range, where a scaling need not be exact (a denormal
            # result is rounded, or flushed): those are held to the smallest normal number instead
            normal = (one[1] == 0) | (np.abs(one[1]) > 256 * tiny)
            assert normal.mean() > 0.8
            assert np.array_equal(_u32(two[1][normal]), _u32(want[normal]))
            assert np.all(np.abs(two[1][~normal] - want[~normal]) <= tiny)
            assert two[3] == one[3] and np.array_equal(two[2], one[2])
        for ce in (1.0, 0.5, 4.0):
            both = _dice(lib, p, None, marked, 255, form, coef, Cc, ce=ce, dz_in=d0)
            want = (np.float32(ce) * d0).astype(np.float32) + one[1]
            assert np.array_equal(_u32(both[1]), _u32(want.astype(np.float32)))


@pytest.mark.parametrize("form,which", [(FLAT, None), (CLASS, None), (CLASS, "foreground")])
@pytest.mark.parametrize("P", [3219, 262181])
@pytest.mark.parametrize("Cc", CLASSES)
def test_against_float64(lib, Cc, P, form, which):
    """Every fifth pixel ignored; the flat form, c_k = 1 / C and the foreground coefficients."""
    p, z, codes = _probs(lib, Cc, P)
    marked = codes.copy()
    marked[::5] = 255
    t = R.onehot_rows(marked, Cc, 255)
    keep = D.keep_rows(t)
    c64 = D.class_coef(Cc, which)
    coef = None if which is None else c64.astype(np.float32)
    rc, dz, sums, loss = _dice(lib, p, None, marked, 255, form, coef, Cc)
    assert rc == 0, lib.depgan_last_error()
    _, g64, L64, s64 = D.dice_ref(z, t, keep, "flat" if form == FLAT else "class", c64, SMOOTH)
    print("C = %d P = %d form %d %s: dz %.2e of max|dz| %.2e; loss %.8f (fp64 %.8f, rel %.2e); sums rel %.2e"
          % (Cc, P, form, which, np.abs(dz - g64).max(), np.abs(g64).max(), loss, L64, abs(loss - L64) / L64,
             np.abs(sums - s64).max() / s64.max()))
    assert np.isfinite(dz).all() and np.abs(g64).max() > 0
    assert np.abs(dz - g64).max() <= 1e-5 * np.abs(g64).max()
    assert abs(loss - L64) <= 1e-5 * abs(L64), (loss, L64)
    assert np.all(dz[keep == 0] == 0.0)
    assert np.array_equal(sums[2], s64[2])


@pytest.mark.parametrize("Cc", [2, 4, 8])
def test_everything_ignored(lib, Cc):
    """No pixel takes part: loss 0.0, a zero Dice gradient, status 0."""
    p, _, _ = _probs(lib, Cc, 3219)
    codes = np.full(3219, 255, np.uint8)
    d0 = np.random.default_rng(Cc).standard_normal((3219, Cc)).astype(np.float32)
    for form in (FLAT, CLASS):
        rc, dz, sums, loss = _dice(lib, p, None, codes, 255, form, None, Cc)
        assert rc == 0 and loss == 0.0 and np.all(dz == 0.0) and np.all(sums == 0.0)
        rc, dz, sums, loss = _dice(lib, p, np.zeros((3219, Cc), np.float32), None, 0, form, None, Cc, ce=1.0, dz_in=d0)
        assert rc == 0 and loss == 0.0 and np.array_equal(_u32(dz), _u32(d0)) and np.all(sums == 0.0)


@pytest.mark.parametrize("Cc,P", [(4, 3219), (8, 262181), (3, 255)])
def test_a_second_call_into_the_same_buffers_repeats_the_result(lib, Cc, P):
    """No stale partial and no dependence on zeroing: the same device buffers, other labels in between."""
    p, _, codes = _probs(lib, Cc, P)
    codes = codes.copy()
    codes[::5] = 255
    pd, cd = torch.from_numpy(p).cuda(), torch.from_numpy(codes).cuda()
    dz = torch.empty((P, Cc), device="cuda:0")
    coef = (C.c_float * Cc)(*_coef(Cc))
    sums, loss = (C.c_double * 24)(), C.c_float()

    def call(c_dev):
        rc = lib.depgan_op_dice_loss(P_(pd), None, P_(c_dev), 255, CLASS, coef, Cc, SMOOTH, 0.0, 1.0, P_(dz), sums,
                                     C.byref(loss), P, Cc, None)
        torch.cuda.synchronize()
        return rc, _u32(dz).copy(), list(sums), np.float32(loss.value).view(np.uint32)

    first = call(cd)
    assert first[0] == 0, lib.depgan_last_error()
    other = call(torch.from_numpy(((codes.astype(np.int64) + 1) % Cc).astype(np.uint8)).cuda())
    assert other[0] == 0 and other[2] != first[2]
    again = call(cd)
    assert again[0] == 0 and np.array_equal(first[1], again[1]) and first[2] == again[2] and first[3] == again[3]


@pytest.mark.parametrize("what,kw", [
    ("form off", {"form": 0}), ("form", {"form": 3}), ("flat with coefficients", {"form": FLAT, "coef": [1.0] * 4}),
    ("n != C", {"coef": [1.0] * 3}), ("n != C", {"coef": [1.0] * 5}), ("negative", {"coef": [1.0, -0.5, 1.0, 1.0]}),
    ("nan", {"coef": [1.0, float("nan"), 1.0, 1.0]}), ("inf", {"coef": [1.0, float("inf"), 1.0, 1.0]}),
    ("all zero", {"coef": [0.0] * 4}), ("smooth", {"smooth": 0.0}), ("smooth", {"smooth": -1.0}),
    ("smooth", {"smooth": float("nan")}), ("dice_coef", {"dw": 0.0}), ("dice_coef", {"dw": float("inf")}),
    ("ce_coef", {"ce": -1.0}), ("ce_coef", {"ce": float("nan")}), ("ignore", {"ign": -2}), ("ignore", {"ign": 256})])
def test_refused_before_any_launch(lib, what, kw):
    """Status 1 with a message; the NaN-filled dz and the host outputs are untouched."""
    p, _, codes = _probs(lib, 4, 255)
    a = dict(form=CLASS, coef=None, smooth=SMOOTH, ce=1.0, dw=1.0, ign=-1)
    a.update(kw)
    rc, dz, sums, loss = _dice(lib, p, None, codes, a["ign"], a["form"], a["coef"], 4, smooth=a["smooth"], ce=a["ce"],
                               dw=a["dw"])
    assert rc == 1, what
    assert lib.depgan_last_error()
    assert np.isnan(dz).all() and np.all(sums == -7.0) and loss == -7.0
