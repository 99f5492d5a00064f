"""NumPy restatement of csrc/calibration.hip, statement by statement as include/depgan.h words them.  (A plain module.)

census(): the integer tables with np.add.at on int64, the Brier and NLL sums with math.fsum (the bound of the device's
double sums is stated against the exact sum).  temperature_sums(): float64, summed plainly or with math.fsum.
apply(): the temperature-scaled rows in float64, rounded once to the kind of prob.  brute_census(): the same census as a
Python loop over pixels, the check of the vectorised one.
"""
import math

import numpy as np

FIX_SHIFT = 32
SCALARS = ("n", "n_nan", "n_bad", "n_floored")


def bin_of(v, bins):
    """b(v) = (int)min(max(v * bins, 0.0), bins - 1), in double"""
    v = np.asarray(v, np.float64)
    return np.minimum(np.maximum(v * float(bins), 0.0), float(bins - 1)).astype(np.int64)


def fix(v):
    """q(v) = (long long)rint(v * 2^32)"""
    return np.rint(np.asarray(v, np.float64) * 2.0 ** FIX_SHIFT).astype(np.int64)


def classify(prob, lab, ignore, mask):
    """per pixel 0 (masked / ignored), 1 (takes part), 2 (code >= C), 3 (a NaN in the row): the first rule that applies"""
    P, C = prob.shape
    what = np.ones(P, np.int64)
    what[np.isnan(prob).any(1)] = 3
    what[lab.astype(np.int64) >= C] = 2
    what[lab.astype(np.int64) == ignore] = 0
    if mask is not None:
        what[np.asarray(mask, np.float32) == 0] = 0
    return what


def census(prob, lab, bins, ignore=-1, mask=None, eps=1e-7):
    """prob (P, C) float32 / float64, lab (P) uint8.  Returns (counts, sums): the entry's two host tables, counts int64
    of (1 + C) * bins * 3 + 4, sums = [Brier, NLL] by math.fsum."""
    prob = np.asarray(prob)
    P, C = prob.shape
    what = classify(prob, lab, ignore, mask)
    act = what == 1
    p = prob[act].astype(np.float64)
    tc = lab[act].astype(np.int64)
    tab = np.zeros((1 + C, bins, 3), np.int64)
    n = len(p)
    if n:
        pred = np.argmax(p, 1)                         # the first maximum
        conf = p[np.arange(n), pred]
        b = bin_of(conf, bins)
        np.add.at(tab[0, :, 0], b, 1)
        np.add.at(tab[0, :, 1], b, (pred == tc).astype(np.int64))
        np.add.at(tab[0, :, 2], b, fix(conf))
        for k in range(C):
            b = bin_of(p[:, k], bins)
            np.add.at(tab[1 + k, :, 0], b, 1)
            np.add.at(tab[1 + k, :, 1], b, (tc == k).astype(np.int64))
            np.add.at(tab[1 + k, :, 2], b, fix(p[:, k]))
    r = p[np.arange(n), tc] if n else np.zeros(0)
    bs = np.zeros(n)
    for c in range(C):
        d = p[:, c] - (tc == c).astype(np.float64)
        bs = bs + d * d
    with np.errstate(divide="ignore", invalid="ignore"):
        ll = 0.0 - np.log(np.where(r < eps, eps, r))
    scal = [n, int((what == 3).sum()), int((what == 2).sum()), int((r < eps).sum())]
    return (np.concatenate([tab.reshape(-1), np.array(scal, np.int64)]),
            np.array([math.fsum(bs), math.fsum(ll)], np.float64))


def brute_census(prob, lab, bins, ignore=-1, mask=None, eps=1e-7):
    """census() as a loop over pixels with Python integers and floats"""
    prob = np.asarray(prob)
    P, C = prob.shape
    tab = [[[0, 0, 0] for _ in range(bins)] for _ in range(1 + C)]
    n = n_nan = n_bad = n_floored = 0
    bs_all, ll_all = [], []
    for x in range(P):
        if mask is not None and float(mask[x]) == 0.0:
            continue
        code = int(lab[x])
        if code == ignore:
            continue
        if code >= C:
            n_bad += 1
            continue
        row = [float(v) for v in prob[x]]
        if any(v != v for v in row):
            n_nan += 1
            continue
        n += 1
        conf, pred = row[0], 0
        for c in range(1, C):
            if row[c] > conf:
                conf, pred = row[c], c
        for j, v, hit in [(0, conf, pred == code)] + [(1 + k, row[k], code == k) for k in range(C)]:
            b = int(min(max(v * bins, 0.0), float(bins - 1)))
            cell = tab[j][b]
            cell[0] += 1
            cell[1] += int(hit)
            cell[2] += int(round(v * 2.0 ** FIX_SHIFT))      # Python's round: to even, on an exact product
        r = row[code]
        n_floored += r < eps
        bs = 0.0
        for c in range(C):
            d = row[c] - (1.0 if c == code else 0.0)
            bs = bs + d * d
        bs_all.append(bs)
        ll_all.append(0.0 - math.log(max(r, eps)) if max(r, eps) > 0 else math.inf)
    counts = np.array([v for t in tab for cell in t for v in cell] + [n, n_nan, n_bad, n_floored], np.int64)
    return counts, np.array([math.fsum(bs_all), math.fsum(ll_all)], np.float64)


def scaled_terms(p, beta, eps):
    """z, s, lse, pi of the rows p (n, C) float64, as the header states them"""
    z = np.log(np.where(p < eps, eps, p))
    s = beta * z
    m = s[:, 0].copy()
    for c in range(1, s.shape[1]):
        m = np.where(s[:, c] > m, s[:, c], m)
    e = np.exp(s - m[:, None])
    S = np.zeros(len(p))
    for c in range(s.shape[1]):
        S = S + e[:, c]
    return z, s, m + np.log(S), e / S[:, None]


def temperature_sums(prob, lab, beta, ignore=-1, mask=None, eps=1e-7, exact=False):
    """{N, sum L, sum L', sum L''}; exact: math.fsum of the per-pixel terms"""
    prob = np.asarray(prob)
    act = classify(prob, lab, ignore, mask) == 1
    p = prob[act].astype(np.float64)
    tc = lab[act].astype(np.int64)
    n = len(p)
    if not n:
        return np.zeros(4)
    z, s, lse, pi = scaled_terms(p, beta, eps)
    A, B = np.zeros(n), np.zeros(n)
    for c in range(p.shape[1]):
        A = A + pi[:, c] * z[:, c]
        B = B + pi[:, c] * (z[:, c] * z[:, c])
    i = np.arange(n)
    L, L1, L2 = lse - s[i, tc], A - z[i, tc], B - A * A
    add = math.fsum if exact else (lambda v: float(np.sum(v)))
    return np.array([float(n), add(L), add(L1), add(L2)])


def apply(prob, beta, eps=1e-7):
    """out_c = exp(s_c - lse) in float64, rounded once to prob's dtype; also returns the float64 rows"""
    prob = np.asarray(prob)
    _, s, lse, _ = scaled_terms(prob.astype(np.float64), beta, eps)
    with np.errstate(invalid="ignore"):
        out = np.exp(s - lse[:, None])
    return out.astype(prob.dtype), out


def ece_of(prob, lab, bins=15):
    """the expected calibration error from its definition, in float64 (no fixed point)"""
    p = np.asarray(prob, np.float64)
    pred = np.argmax(p, 1)
    conf = p[np.arange(len(p)), pred]
    b = bin_of(conf, bins)
    ece = 0.0
    for k in range(bins):
        sel = b == k
        if sel.any():
            ece += sel.sum() / len(p) * abs(float((pred[sel] == lab[sel]).mean()) - float(conf[sel].mean()))
    return ece


def softmax_problem(seed, n, C=4, sharpen=3.0, sigma=2.0):
    """The over-confident model of the issue: logits z ~ N(0, sigma^2), labels sampled from softmax(z), and
    prob = softmax(sharpen * z), whose calibrating temperature is near `sharpen` (never asserted).  (prob float64, lab)"""
    r = np.random.default_rng(seed)
    z = sigma * r.standard_normal((n, C))
    def sm(a):
        e = np.exp(a - a.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)
    cdf = np.cumsum(sm(z), 1)
    lab = np.minimum((r.random(n)[:, None] > cdf).sum(1), C - 1).astype(np.uint8)
    return sm(sharpen * z), lab
