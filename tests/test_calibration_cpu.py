"""CPU: the NumPy restatement of the calibration kernels (tests/calibration_ref.py) against a loop over pixels, the bin
and fixed-point rules at their edges, evaluate.calibration_metrics on hand-made tables, the temperature solver driven by
the restatement's sums, and every ValueError of the four public functions (raised before anything touches a device)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_ref as ref  # noqa: E402
from dep_gan_im_amd import evaluate as ev  # noqa: E402


def _rows(r, n, C, dtype):
    p = r.random((n, C)) ** 3
    return (p / p.sum(1, keepdims=True)).astype(dtype)


@pytest.mark.parametrize("C,bins,dtype", [(2, 1, np.float32), (3, 10, np.float64), (4, 15, np.float64), (8, 64, np.float32)])
def test_the_restatement_is_the_loop_over_pixels(C, bins, dtype):
    r = np.random.default_rng(C * 100 + bins)
    n = 300
    p = _rows(r, n, C, dtype)
    p[5] = 0.0
    p[5, C - 1] = 1.0                                   # exact 0.0 and 1.0
    p[6] = 1.0 / C                                      # a tie: class 0 wins
    p[7, 0] = np.nan
    lab = r.integers(0, C, n).astype(np.uint8)
    lab[5], lab[8], lab[9] = 0, C, 200                  # a true-class probability of 0; a bad code; the ignore code
    mask = (r.random(n) > 0.2).astype(np.float32)
    mask[5:10] = 1
    for m in (None, mask):
        a, asum = ref.census(p, lab, bins, ignore=200, mask=m, eps=1e-7)
        b, bsum = ref.brute_census(p, lab, bins, ignore=200, mask=m, eps=1e-7)
        assert np.array_equal(a, b)
        assert np.array_equal(asum, bsum)
        assert a[-3] == 1 and a[-2] == 1 and a[-1] >= 1   # one NaN row, one bad code, the floored pixel (a draw may add one)
        tab = a[:-4].reshape(1 + C, bins, 3)
        assert (tab[:, :, 0].sum(1) == a[-4]).all()     # every table holds every pixel that takes part


@pytest.mark.parametrize("bins", [1, 10, 15, 64])
def test_the_bin_rule_at_the_edges(bins):
    """The rule rounds ONCE, in the product v * bins.  v = k / bins, the double nearest to the quotient, is in bin k for
    these bin counts (the product rounds back to the integer k); 0.0 is bin 0 and 1.0 is bin bins - 1.  A value a little
    below an edge (a factor 1 - 2^-40) is in the bin below it.  The LAST double below an edge is in the bin below it
    unless its product rounds up to the edge -- nextafter(0.9, 0) * 10 is 9.0 in double -- which is the rule as stated,
    so the expectation is the correctly rounded product formed from exact fractions, truncated."""
    from fractions import Fraction
    ks = np.arange(bins + 1)
    edges = ks / float(bins)
    assert np.array_equal(ref.bin_of(edges, bins), np.minimum(ks, bins - 1))
    assert np.array_equal(ref.bin_of(edges[1:] * (1 - 2.0 ** -40), bins), ks[:-1])
    below = np.nextafter(edges[1:], 0.0)
    want = [int(min(float(Fraction(float(v)) * bins), float(bins - 1))) for v in below]
    got = ref.bin_of(below, bins)
    assert got.tolist() == want and ((got == ks[:-1]) | (got == np.minimum(ks[1:], bins - 1))).all()
    assert ref.bin_of(0.0, bins) == 0 and ref.bin_of(1.0, bins) == bins - 1
    assert ref.bin_of(-0.25, bins) == 0 and ref.bin_of(1.5, bins) == bins - 1 and ref.bin_of(-0.0, bins) == 0


def test_the_fixed_point_rule():
    assert ref.fix(0.0) == 0 and ref.fix(1.0) == 2 ** 32
    assert ref.fix(2.0 ** -32) == 1
    assert ref.fix(2.0 ** -33) == 0                     # a tie: 0.5 goes to the even 0
    assert ref.fix(3 * 2.0 ** -33) == 2                 # a tie: 1.5 goes to the even 2
    assert ref.fix(2.0 ** -34) == 0
    assert ref.fix(np.nextafter(2.0 ** -33, 1.0)) == 1
    v = np.random.default_rng(0).random(1000)
    assert np.max(np.abs(ref.fix(v) / 2.0 ** 32 - v)) <= 2.0 ** -33


def _census(top, klass=None, brier_sum=0.0, nll_sum=0.0, n_nan=0, n_floored=0):
    """a census dict from (count, correct, mean confidence) per top-label bin; the class tables default to one class pair
    that repeats the top table"""
    cnt = np.array([t[0] for t in top], np.int64)
    cor = np.array([t[1] for t in top], np.int64)
    q = np.array([int(round(t[0] * t[2] * 2 ** 32)) for t in top], np.int64)
    k = klass if klass is not None else (np.stack([cnt, cnt]), np.stack([cor, cnt - cor]), np.stack([q, q]))
    return {"top_count": cnt, "top_correct": cor, "top_conf_q": q, "class_count": k[0], "class_pos": k[1],
            "class_prob_q": k[2], "n": int(cnt.sum()), "n_nan": n_nan, "n_bad": 0, "n_floored": n_floored,
            "brier_sum": brier_sum, "nll_sum": nll_sum, "bins": len(top), "n_class": 2, "eps": 1e-7}


def test_metrics_of_a_perfectly_calibrated_table():
    """four bins whose accuracy is their mean confidence (all dyadic, so the fixed point holds them exactly)"""
    m = ev.calibration_metrics(_census([(8, 1, 0.125), (8, 3, 0.375), (16, 10, 0.625), (32, 28, 0.875)]))
    assert m["ece"] == 0.0 and m["mce"] == 0.0
    assert m["accuracy"] == 42 / 64 and m["mean_confidence"] == 42 / 64
    assert np.array_equal(m["bin_accuracy"], [0.125, 0.375, 0.625, 0.875])


def test_metrics_of_a_two_bin_table():
    """bin 0: 40 pixels, 30 right, mean confidence 0.25 -> gap |0.75 - 0.25| = 0.5; bin 1: 60 pixels, 45 right, mean
    confidence 0.875 -> gap |0.75 - 0.875| = 0.125.  ECE = 0.4 * 0.5 + 0.6 * 0.125 = 0.275, MCE = 0.5, accuracy 0.75,
    mean confidence (40 * 0.25 + 60 * 0.875) / 100 = 0.625.  Class 0 repeats the top table (classwise ECE 0.275); class 1
    has pos = count - correct: gaps |0.25 - 0.25| = 0 and |0.25 - 0.875| = 0.625 -> 0.6 * 0.625 = 0.375."""
    m = ev.calibration_metrics(_census([(40, 30, 0.25), (60, 45, 0.875)], brier_sum=50.0, nll_sum=25.0))
    assert m["ece"] == pytest.approx(0.275, abs=1e-15) and m["mce"] == 0.5
    assert m["accuracy"] == 0.75 and m["mean_confidence"] == 0.625
    assert m["classwise_ece"] == pytest.approx([0.275, 0.375], abs=1e-15)
    assert m["classwise_ece_mean"] == pytest.approx(0.325, abs=1e-15)
    assert m["brier"] == 0.5 and m["nll"] == 0.25 and m["n"] == 100


def test_metrics_with_empty_bins_and_without_pixels():
    m = ev.calibration_metrics(_census([(0, 0, 0.0), (10, 5, 0.75), (0, 0, 0.0)]))
    assert m["ece"] == 0.25 and m["mce"] == 0.25                   # the empty bins contribute 0 ...
    assert np.isnan(m["bin_accuracy"][[0, 2]]).all() and np.isnan(m["bin_confidence"][[0, 2]]).all()   # ... and show nan
    assert m["bin_accuracy"][1] == 0.5 and m["bin_count"].tolist() == [0, 10, 0]
    e = ev.calibration_metrics(_census([(0, 0, 0.0)] * 3, n_nan=7))
    assert e["n"] == 0 and e["n_nan"] == 7
    for k in ("ece", "mce", "brier", "nll", "accuracy", "mean_confidence", "classwise_ece_mean"):
        assert math.isnan(e[k]), k
    assert np.isnan(e["classwise_ece"]).all() and np.isnan(e["bin_accuracy"]).all()


def test_metrics_from_the_restatement_are_the_definitions():
    p, lab = ref.softmax_problem(3, 4000)
    counts, sums = ref.census(p, lab, 15)
    m = ev.calibration_metrics(ev.census_from_tables(counts, sums, 4, 15, 1e-7))
    assert m["ece"] == pytest.approx(ref.ece_of(p, lab, 15), abs=1e-9)
    onehot = np.eye(4)[lab]
    assert m["brier"] == pytest.approx(((p - onehot) ** 2).sum(1).mean(), rel=1e-12)
    assert m["nll"] == pytest.approx(-np.log(np.maximum(p[np.arange(len(p)), lab], 1e-7)).mean(), rel=1e-12)
    assert m["accuracy"] == (p.argmax(1) == lab).mean()


def _check_fit(fit, p, lab, tol, eps=1e-7):
    """the three conditions of the issue, evaluated by the restatement: the slope at the returned beta is within tol, the
    NLL there is not above the NLL at 0.99 beta and 1.01 beta, and the ECE falls"""
    beta = fit["beta"]
    assert fit["converged"] and not fit["at_bound"] and fit["T"] == 1.0 / beta
    n, L, L1, _ = ref.temperature_sums(p, lab, beta, eps=eps, exact=True)
    assert abs(L1) / n <= tol
    for f in (0.99, 1.01):
        assert L <= ref.temperature_sums(p, lab, f * beta, eps=eps, exact=True)[1]
    assert fit["nll_after"] == pytest.approx(L / n, rel=1e-12) and fit["nll_after"] < fit["nll_before"]
    scaled, _ = ref.apply(p, beta, eps)
    assert ref.ece_of(scaled, lab) < ref.ece_of(p, lab)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_solver_on_the_restatements_sums(dtype):
    p, lab = ref.softmax_problem(11, 20000)
    p = p.astype(dtype)
    calls = []

    def sums(beta):
        calls.append(beta)
        return ref.temperature_sums(p, lab, beta)

    fit = ev.solve_temperature(sums, tol=1e-6)
    assert fit["iterations"] == len(calls) <= 12 and calls[0] == 1.0
    _check_fit(fit, p, lab, 1e-6)
    assert fit["nll_before"] == pytest.approx(ref.temperature_sums(p, lab, 1.0)[1] / len(p), rel=1e-12)


def test_the_solver_with_a_minimum_beyond_a_bound():
    p, lab = ref.softmax_problem(11, 5000)               # the minimum is near T = 3
    hot = ev.solve_temperature(lambda b: ref.temperature_sums(p, lab, b), bounds=(0.5, 2.0))
    assert hot["at_bound"] and not hot["converged"] and hot["T"] == pytest.approx(2.0, rel=1e-15) and hot["beta"] == 0.5
    cold = ev.solve_temperature(lambda b: ref.temperature_sums(p, lab, b), bounds=(5.0, 10.0))
    assert cold["at_bound"] and not cold["converged"] and cold["T"] == pytest.approx(5.0, rel=1e-15)
    assert cold["nll_before"] == pytest.approx(ref.temperature_sums(p, lab, 1.0)[1] / len(p), rel=1e-12)
    inside = ev.solve_temperature(lambda b: ref.temperature_sums(p, lab, b), bounds=(2.0, 10.0))
    assert inside["converged"] and not inside["at_bound"] and 2.0 < inside["T"] < 10.0
    none = ev.solve_temperature(lambda b: np.zeros(4))
    assert none["n"] == 0 and math.isnan(none["T"]) and not none["converged"] and not none["at_bound"]


P4 = np.full((1, 2, 3, 4), 0.25, np.float32)
L4 = np.zeros((1, 2, 3), np.uint8)


@pytest.mark.parametrize("kw", [
    dict(prob=P4[0]), dict(prob=np.full((1, 2, 3, 1), 1.0, np.float32)), dict(prob=np.full((1, 2, 3, 9), 0.1, np.float32)),
    dict(prob=P4.astype(np.float16)), dict(prob=P4.astype(np.int32)), dict(prob=[[[[0.5, 0.5]]]]),
    dict(labels=L4[0]), dict(labels=L4.astype(np.int64)), dict(labels=np.zeros((1, 2, 4), np.uint8)), dict(labels=None),
    dict(mask=np.ones((1, 2, 4), np.float32)), dict(ignore_label=-1), dict(ignore_label=256), dict(ignore_label=1.0),
    dict(ignore_label=True), dict(eps=-1e-9), dict(eps=1.0), dict(eps=float("nan")), dict(eps="x"),
    dict(bins=0), dict(bins=65), dict(bins=15.0), dict(bins=True)])
def test_calibration_census_value_errors(kw):
    args = dict(prob=P4, labels=L4)
    args.update(kw)
    with pytest.raises(ValueError, match="calibration_census"):
        ev.calibration_census(**args)


@pytest.mark.parametrize("kw", [
    dict(prob=P4[0]), dict(prob=P4.astype(np.float16)), dict(labels=L4.astype(np.int8)), dict(mask=np.ones(6, np.float32)),
    dict(ignore_label=300), dict(eps=0.0), dict(eps=1.0), dict(bounds=(0.0, 2.0)), dict(bounds=(2.0, 1.0)),
    dict(bounds=(1.0, float("inf"))), dict(bounds=3.0), dict(tol=0.0), dict(tol=float("nan")), dict(max_iter=0),
    dict(max_iter=2.5)])
def test_fit_temperature_value_errors(kw):
    args = dict(prob=P4, labels=L4)
    args.update(kw)
    with pytest.raises(ValueError, match="fit_temperature"):
        ev.fit_temperature(**args)


@pytest.mark.parametrize("kw", [
    dict(prob=P4[0]), dict(prob=P4.astype(np.float16)), dict(T=0.0), dict(T=-1.0), dict(T=float("inf")), dict(T=float("nan")),
    dict(T="x"), dict(eps=1.0), dict(eps=-0.5), dict(out=np.empty_like(P4))])
def test_apply_temperature_value_errors(kw):
    args = dict(prob=P4, T=2.0)
    args.update(kw)
    with pytest.raises(ValueError, match="apply_temperature"):
        ev.apply_temperature(**args)


def test_solve_temperature_value_errors():
    for kw in (dict(bounds=(0.0, 1.0)), dict(tol=-1.0), dict(max_iter=0)):
        with pytest.raises(ValueError, match="solve_temperature"):
            ev.solve_temperature(lambda b: np.ones(4), **kw)


def test_a_label_outside_the_classes_raises():
    counts = np.zeros(3 * 2 * 3 + 4, np.int64)
    counts[-2] = 5
    with pytest.raises(ValueError, match="5 labels"):
        ev.census_from_tables(counts, np.zeros(2), 2, 2, 1e-7)
