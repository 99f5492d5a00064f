"""GPU: csrc/calibration.hip against the NumPy restatement (tests/calibration_ref.py).

Every integer of the census -- counts, hits, the fixed-point sums, the scalars -- bit for bit; the Brier and NLL sums
against math.fsum within (n + 3) 2^-52 relative (the bound the surface mean is held to; the per-pixel terms have the
restatement's bits and are not negative, so only the order of n adds differs), the NLL with 1e-12 relative more for the
device's log (the bound of predict_stats' entropy figures).  depgan_eval_temperature_sums within 1e-12 relative of the
float64 restatement; depgan_eval_apply_temperature within 1e-12 (float64) or one float32 ulp of it.

Shapes: (1, 5, 13) = 65 pixels, one full wave and one lane; (3, 37, 53) = 5883, six blocks and a ragged tail; and
(1, 517, 509) = 263153, derived from the launch code: a census block takes 256 * CAL_PER_THREAD = 1024 pixels up to
CAL_MAX_BLOCKS = 1024 blocks, so this size launches ceil(263153 / 1024) = 257 blocks -- one more than the 256 threads
of the finishing block, whose threads therefore bring in more than one partial each and whose fold runs over more
partials than it has threads -- and 257 * 256 = 65792 threads for 263153 pixels, so every thread walks 3 or 4 pixels in
grid-stride order.  (1, 1025, 1024) = 1049600 pixels is the smallest slice stack past the grid cap: ceil(1049600 / 1024) =
1025 blocks are cut to CAL_MAX_BLOCKS = 1024, the finishing launch adds 1024 tables and folds 1024 x 2 double partials
out of an LDS array of exactly that size, and a thread walks 4 or 5 pixels.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {"wave+1": (1, 5, 13), "blocks": (3, 37, 53), "partials": (1, 517, 509), "cap": (1, 1025, 1024)}
SENT = 0x4B3C2D1E


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _scratch(lib, npix, Cc, bins):
    import torch
    nbytes = int(lib.depgan_eval_calibration_scratch_bytes(npix, Cc, bins))
    assert nbytes > 0 and nbytes % 8 == 0
    return torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")


def run_census(lib, prob, lab, bins, ignore=-1, mask=None, eps=1e-7):
    """the entry on host arrays: (counts int64, sums float64)"""
    import torch
    P, Cc = prob.shape
    p, l, m = _t(prob), _t(lab), _t(mask)
    scratch = _scratch(lib, P, Cc, bins)
    counts = np.full((1 + Cc) * bins * 3 + 4, -7, np.int64)
    sums = np.full(2, -7.0)
    rc = lib.depgan_eval_calibration_census(_ptr(p), int(prob.dtype == np.float64), Cc, _ptr(l), ignore, _ptr(m), P, bins,
                                            eps, _ptr(scratch), C.c_void_p(counts.ctypes.data),
                                            C.c_void_p(sums.ctypes.data), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.depgan_last_error()
    return counts, sums


def run_tsums(lib, prob, lab, beta, ignore=-1, mask=None, eps=1e-7):
    import torch
    P, Cc = prob.shape
    p, l, m = _t(prob), _t(lab), _t(mask)
    scratch = _scratch(lib, P, Cc, 1)
    out = np.full(4, -7.0)
    rc = lib.depgan_eval_temperature_sums(_ptr(p), int(prob.dtype == np.float64), Cc, _ptr(l), ignore, _ptr(m), P, beta,
                                          eps, _ptr(scratch), C.c_void_p(out.ctypes.data),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.depgan_last_error()
    return out


def make_case(shape, Cc, dtype, bins, style="mixed", seed=0):
    """(prob (P, C), lab, mask, ignore code).  mixed: random rows, then planted rows -- elements exactly on the bin edges
    k / bins, exact 0.0 and 1.0, ties for the maximum (all equal; two equal leaders), a true-class probability of 0, NaN
    rows, a masked run, ignored pixels.  one_bin: every pixel the same row.  skewed: 97 % of the pixels are class 0 at
    confidence >= 0.99 (the top-label bin bins - 1 and bin 0 of every other class), the rest random."""
    P = int(np.prod(shape))
    r = np.random.default_rng(seed + 1000 * Cc + bins)
    p = r.random((P, Cc)) ** 3 + 1e-3
    p = p / p.sum(1, keepdims=True)
    lab = r.integers(0, Cc, P).astype(np.uint8)
    mask, ignore = None, -1
    if style == "one_bin":
        p[:] = p[0]
    elif style == "skewed":
        hot = r.random(P) < 0.97
        conf = 0.99 + 0.01 * r.random(P)
        row = np.concatenate([conf[:, None], np.repeat(((1 - conf) / (Cc - 1))[:, None], Cc - 1, 1)], 1)
        p[hot], lab[hot] = row[hot], 0
    else:
        ignore = 255
        lab[r.random(P) < 0.05] = ignore
        mask = (r.random(P) > 0.1).astype(np.float32) * r.random(P).astype(np.float32)
        mask[:min(P, 70)] = np.where(np.arange(min(P, 70)) % 3 == 0, 0.0, 1.0)   # zeros inside the first wave
        at = iter(r.permutation(P))

        def plant():
            """the next free pixel, made to take part"""
            x = next(at, None)
            if x is not None:
                mask[x], lab[x] = 1.0, lab[x] % Cc
            return x

        for x in (plant(), plant()):
            p[x] = 0.0
            p[x, int(lab[x])] = 1.0                        # exact 1.0 and 0.0, right
        x = plant()
        p[x], p[x, (int(lab[x]) + 1) % Cc] = 0.0, 1.0       # exact 1.0 on a wrong class: the true class has probability 0
        p[plant()] = 1.0 / Cc                              # every element the maximum: class 0 wins
        x = plant()
        p[x], p[x, Cc - 1], p[x, Cc - 2] = 0.0, 0.5, 0.5    # two leaders: the lower index wins
        for x in (plant(), plant(), plant()):
            p[x, r.integers(0, Cc)] = np.nan
        for k in range(bins + 1):                          # on the edges and next to them, as far as the pixels go
            for v in (k / bins, np.nextafter(k / bins, 0.0), np.nextafter(k / bins, 1.0)):
                x = plant() if 0.0 <= v <= 1.0 else None
                if x is not None:
                    p[x] = (1.0 - v) / (Cc - 1)
                    p[x, k % Cc] = v
    return p.astype(dtype), lab, mask, ignore


def check_census(lib, prob, lab, bins, ignore, mask, eps=1e-7, what=""):
    got, gsum = run_census(lib, prob, lab, bins, ignore, mask, eps)
    want, wsum = ref.census(prob, lab, bins, ignore, mask, eps)
    assert np.array_equal(got, want), "%s: %d integers differ, first at %d" % (
        what, int((got != want).sum()), int(np.flatnonzero(got != want)[0]))
    n = int(want[-4])
    tab = got[:-4].reshape(1 + prob.shape[1], bins, 3)
    assert (tab[:, :, 0].sum(1) == n).all()
    for i, (key, extra) in enumerate((("brier", 0.0), ("nll", 1e-12))):
        err = abs(gsum[i] - wsum[i]) / wsum[i] if wsum[i] else abs(gsum[i])
        print("%s: %s sum %.17g, fsum %.17g, relative error %.3e (bound %.3e), n = %d"
              % (what, key, gsum[i], wsum[i], err, (n + 3) * 2.0 ** -52 + extra, n))
        assert err <= (n + 3) * 2.0 ** -52 + extra, (what, key, err)
    again, asum = run_census(lib, prob, lab, bins, ignore, mask, eps)
    assert np.array_equal(again, got) and again.tobytes() == got.tobytes()
    assert asum.tobytes() == gsum.tobytes(), "%s: a second call gave other bits in the double sums" % what
    return got, gsum


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("bins", [1, 10, 15, 64])
@pytest.mark.parametrize("Cc", [2, 3, 4, 8])
def test_census_is_the_restatement(lib, Cc, bins, dtype):
    for name in ("wave+1", "blocks"):
        prob, lab, mask, ignore = make_case(SHAPES[name], Cc, dtype, bins)
        got, _ = check_census(lib, prob, lab, bins, ignore, mask, what="%s C=%d bins=%d %s" % (name, Cc, bins, dtype.__name__))
        assert got[-3] == 3 and got[-2] == 0 and got[-1] >= 1          # three NaN rows, no bad code, the planted zero


@pytest.mark.parametrize("style", ["mixed", "skewed"])
def test_census_past_one_finishing_block_of_partials(lib, style):
    """the derived size (module docstring): 257 blocks, 3 or 4 pixels per thread"""
    prob, lab, mask, ignore = make_case(SHAPES["partials"], 4, np.float64, 15, style)
    assert math.ceil(len(prob) / 1024) == 257 > 256 and 257 * 256 < len(prob)
    check_census(lib, prob, lab, 15, ignore, mask, what="partials " + style)


def test_census_at_the_grid_cap(lib):
    """the size past CAL_MAX_BLOCKS (module docstring), two classes in float32 to keep it at 8 MB"""
    prob, lab, mask, ignore = make_case(SHAPES["cap"], 2, np.float32, 15)
    assert math.ceil(len(prob) / 1024) == 1025 > 1024
    assert int(lib.depgan_eval_calibration_scratch_bytes(len(prob), 2, 15)) == (1024 + 1) * (3 * 15 * 3 + 4 + 4) * 8
    check_census(lib, prob, lab, 15, ignore, mask, what="cap")


@pytest.mark.parametrize("style", ["one_bin", "skewed"])
@pytest.mark.parametrize("Cc,dtype", [(4, np.float64), (3, np.float32)])
def test_census_with_every_pixel_or_97_percent_in_one_bin(lib, style, Cc, dtype):
    prob, lab, mask, ignore = make_case(SHAPES["blocks"], Cc, dtype, 15, style)
    got, _ = check_census(lib, prob, lab, 15, ignore, mask, what="%s C=%d" % (style, Cc))
    top = got[:15 * 3].reshape(15, 3)[:, 0]
    if style == "one_bin":
        assert (top > 0).sum() == 1 and top.max() == len(prob)
    else:
        assert top[14] >= 0.96 * len(prob)


def test_census_counts_a_bad_code_and_python_raises(lib):
    from dep_gan_im_amd import evaluate
    n, H, W = SHAPES["wave+1"]
    prob, lab, _, _ = make_case((n, H, W), 3, np.float32, 10, "skewed")
    lab[[7, 64]] = [3, 200]
    got, _ = check_census(lib, prob, lab, 10, -1, None, what="bad codes")
    assert got[-2] == 2 and got[-4] == 63
    got, _ = check_census(lib, prob, lab, 10, 200, None, what="one bad code, one ignored")
    assert got[-2] == 1 and got[-4] == 63
    with pytest.raises(ValueError, match="2 labels"):
        evaluate.calibration_census(prob.reshape(n, H, W, 3), lab.reshape(n, H, W), bins=10)
    with pytest.raises(ValueError, match="1 labels"):
        evaluate.fit_temperature(prob.reshape(n, H, W, 3), lab.reshape(n, H, W), ignore_label=200)
    # code 255, the usual "unlabelled" byte, without an ignore label: bad, for both functions and for host and device labels
    import torch
    lab[:] = 0
    lab[[3, 40]] = 255
    for labels in (lab.reshape(n, H, W), torch.from_numpy(lab.reshape(n, H, W)).cuda()):
        with pytest.raises(ValueError, match="2 labels"):
            evaluate.calibration_census(prob.reshape(n, H, W, 3), labels, bins=10)
        with pytest.raises(ValueError, match="2 labels"):
            evaluate.fit_temperature(prob.reshape(n, H, W, 3), labels)
        with pytest.raises(ValueError, match="2 labels"):
            evaluate.fit_temperature(prob.reshape(n, H, W, 3), labels, ignore_label=0)
        assert evaluate.fit_temperature(prob.reshape(n, H, W, 3), labels, ignore_label=255)["n"] == 63
        assert evaluate.calibration_census(prob.reshape(n, H, W, 3), labels, bins=10, ignore_label=255)["n"] == 63


def test_census_with_nothing_taking_part_and_with_eps_zero(lib):
    from dep_gan_im_amd import evaluate
    n, H, W = SHAPES["blocks"]
    prob, lab, _, _ = make_case((n, H, W), 4, np.float64, 15, "skewed")
    lab[:] = 9
    got, gsum = check_census(lib, prob, lab, 15, 9, None, what="all ignored")
    assert not got.any() and gsum.tolist() == [0.0, 0.0]
    got, gsum = check_census(lib, prob, np.zeros_like(lab), 15, -1, np.zeros(len(lab), np.float32), what="all masked")
    assert not got.any() and gsum.tolist() == [0.0, 0.0]
    c = evaluate.calibration_census(prob.reshape(n, H, W, 4), lab.reshape(n, H, W), ignore_label=9)
    m = evaluate.calibration_metrics(c)
    assert c["n"] == 0 and math.isnan(m["ece"]) and math.isnan(m["nll"]) and np.isnan(m["bin_accuracy"]).all()
    fit = evaluate.fit_temperature(prob.reshape(n, H, W, 4), lab.reshape(n, H, W), ignore_label=9)
    assert fit["n"] == 0 and math.isnan(fit["T"]) and not fit["converged"]
    # eps = 0: nothing is floored, and a true-class probability of 0 gives +inf
    lab[:] = 0
    prob[5], prob[5, 1] = 0.0, 1.0
    got, gsum = run_census(lib, prob, lab, 15, eps=0.0)
    want, wsum = ref.census(prob, lab, 15, eps=0.0)
    assert np.array_equal(got, want) and got[-1] == 0 and gsum[1] == math.inf == wsum[1]


def test_the_public_census_takes_host_and_device_arrays_and_a_mask(lib):
    import torch
    from dep_gan_im_amd import evaluate
    n, H, W = SHAPES["blocks"]
    prob, lab, mask, ignore = make_case((n, H, W), 4, np.float32, 15)
    want, wsum = ref.census(prob, lab, 15, ignore, mask)
    p4, l3, m3 = prob.reshape(n, H, W, 4), lab.reshape(n, H, W), mask.reshape(n, H, W)
    for a, b, c in ((p4, l3, m3), (torch.from_numpy(p4).cuda(), torch.from_numpy(l3).cuda(), torch.from_numpy(m3).cuda())):
        cen = evaluate.calibration_census(a, b, bins=15, ignore_label=ignore, mask=c)
        tab = want[:-4].reshape(5, 15, 3)
        assert np.array_equal(cen["top_count"], tab[0, :, 0]) and np.array_equal(cen["top_conf_q"], tab[0, :, 2])
        assert np.array_equal(cen["class_pos"], tab[1:, :, 1]) and np.array_equal(cen["class_prob_q"], tab[1:, :, 2])
        assert [cen[k] for k in ref.SCALARS] == want[-4:].tolist()
        m = evaluate.calibration_metrics(cen)
        keep = ref.classify(prob, lab, ignore, mask) == 1
        assert m["ece"] == pytest.approx(ref.ece_of(prob[keep], lab[keep], 15), abs=1e-9)
        assert m["nll"] == pytest.approx(wsum[1] / want[-4], rel=1e-11)
    # the mask is judged in its own dtype: a float64 value that float32 flushes to zero keeps its pixel
    tiny = np.where(m3 != 0, 1e-300, 0.0)
    assert np.float32(1e-300) == 0
    for c in (tiny, torch.from_numpy(tiny).cuda()):
        assert evaluate.calibration_census(p4, l3, bins=15, ignore_label=ignore, mask=c)["n"] == want[-4]
        assert evaluate.fit_temperature(p4, l3, ignore_label=ignore, mask=c)["n"] == want[-4]


BAD_CENSUS = [dict(npix=0), dict(npix=2 ** 31), dict(Cc=1), dict(Cc=9), dict(bins=0), dict(bins=65), dict(kind=2),
              dict(kind=-1), dict(ignore=-2), dict(ignore=256), dict(eps=-0.1), dict(eps=1.0), dict(eps=float("nan")),
              dict(prob=None), dict(lab=None), dict(scratch=None), dict(counts=None), dict(sums=None),
              dict(prob_off=4), dict(scratch_off=4), dict(mask_off=2), dict(scratch_in_prob=True)]


class _Buffers:
    """sentinel-filled device and host buffers around one small problem"""

    def __init__(self, lib):
        import torch
        self.P, self.Cc, self.bins = 500, 4, 15
        prob, lab, _, _ = make_case((self.P,), self.Cc, np.float64, self.bins, "skewed")
        self.prob, self.lab = _t(prob), _t(lab)
        self.mask = torch.ones(self.P + 4, dtype=torch.float32, device="cuda")
        self.nscr = int(lib.depgan_eval_calibration_scratch_bytes(self.P, self.Cc, self.bins))
        self.scratch = torch.full((self.nscr // 4 + 4,), SENT, dtype=torch.int32, device="cuda")
        self.out = torch.full((self.P * self.Cc * 2 + 8,), SENT, dtype=torch.int32, device="cuda")
        self.counts = np.full((1 + self.Cc) * self.bins * 3 + 4, SENT, np.int64)
        self.sums = np.full(4, float(SENT))
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.scratch == SENT).all()) and bool((self.out == SENT).all()) and \
            (self.counts == SENT).all() and (self.sums == float(SENT)).all()

    def labelled(self, kw):
        """(prob, kind, C, lab, ignore, mask, npix) of a call, one argument made bad"""
        prob = None if "prob" in kw else C.c_void_p(self.prob.data_ptr() + kw.get("prob_off", 0))
        lab = None if "lab" in kw else _ptr(self.lab)
        mask = C.c_void_p(self.mask.data_ptr() + kw["mask_off"]) if "mask_off" in kw else None
        return [prob, kw.get("kind", 1), kw.get("Cc", self.Cc), lab, kw.get("ignore", -1), mask, kw.get("npix", self.P)]

    def scratch_ptr(self, kw):
        if "scratch" in kw:
            return None
        if kw.get("scratch_in_prob"):
            return C.c_void_p(self.prob.data_ptr() + 8 * (self.P * self.Cc - 2))     # its first 16 bytes are prob's last
        return C.c_void_p(self.scratch.data_ptr() + kw.get("scratch_off", 0))


@pytest.fixture(scope="module")
def bufs(lib):
    return _Buffers(lib)


def test_scratch_bytes_outside_the_limits(lib):
    f = lib.depgan_eval_calibration_scratch_bytes
    assert f(1, 2, 1) > 0 and f(2 ** 31 - 1, 8, 64) > 0
    for args in ((0, 4, 15), (2 ** 31, 4, 15), (100, 1, 15), (100, 9, 15), (100, 4, 0), (100, 4, 65)):
        assert f(*args) == 0, args
    assert f(263153, 4, 15) == (257 + 1) * ((1 + 4) * 15 * 3 + 4 + 4) * 8


@pytest.mark.parametrize("kw", BAD_CENSUS, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_census_status_1_leaves_everything_untouched(lib, bufs, kw):
    counts = None if "counts" in kw else C.c_void_p(bufs.counts.ctypes.data)
    sums = None if "sums" in kw else C.c_void_p(bufs.sums.ctypes.data)
    rc = lib.depgan_eval_calibration_census(*bufs.labelled(kw), kw.get("bins", bufs.bins), kw.get("eps", 1e-7),
                                            bufs.scratch_ptr(kw), counts, sums, bufs.stream)
    assert rc == 1 and bufs.untouched()
    assert lib.depgan_last_error()


@pytest.mark.parametrize("kw", [k for k in BAD_CENSUS if not set(k) & {"bins", "counts", "sums"}] +
                         [dict(eps=0.0), dict(beta=0.0), dict(beta=-1.0), dict(beta=float("inf")), dict(beta=float("nan")),
                          dict(out_host=None)], ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_temperature_sums_status_1_leaves_everything_untouched(lib, bufs, kw):
    out = None if "out_host" in kw else C.c_void_p(bufs.sums.ctypes.data)
    rc = lib.depgan_eval_temperature_sums(*bufs.labelled(kw), kw.get("beta", 1.0), kw.get("eps", 1e-7),
                                          bufs.scratch_ptr(kw), out, bufs.stream)
    assert rc == 1 and bufs.untouched()


@pytest.mark.parametrize("kw", [dict(npix=0), dict(npix=2 ** 31), dict(Cc=1), dict(Cc=9), dict(kind=2), dict(eps=-0.1),
                                dict(eps=1.0), dict(beta=0.0), dict(beta=float("inf")), dict(beta=float("nan")),
                                dict(prob=None), dict(out=None), dict(prob_off=8), dict(out_off=8), dict(overlap=True)],
                         ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_apply_status_1_leaves_everything_untouched(lib, bufs, kw):
    import torch
    before = bufs.prob.clone()
    prob = None if "prob" in kw else C.c_void_p(bufs.prob.data_ptr() + kw.get("prob_off", 0))
    out = None if "out" in kw else C.c_void_p(bufs.out.data_ptr() + kw.get("out_off", 0))
    if kw.get("overlap"):
        out = C.c_void_p(bufs.prob.data_ptr() + 32)             # one row further: overlaps prob without being prob
    rc = lib.depgan_eval_apply_temperature(prob, kw.get("kind", 1), kw.get("Cc", bufs.Cc), kw.get("beta", 0.5),
                                           kw.get("eps", 1e-7), out, kw.get("npix", bufs.P - 1 if kw.get("overlap") else bufs.P),
                                           bufs.stream)
    assert rc == 1 and bufs.untouched() and torch.equal(before, bufs.prob)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("beta", [0.2, 1.0, 5.0])
@pytest.mark.parametrize("Cc", [2, 4, 8])
def test_temperature_sums_are_the_restatements(lib, Cc, beta, dtype):
    """random labels, so that no sum cancels; the planted rows hold probabilities below eps (exact zeros)"""
    for name in ("wave+1", "blocks"):
        prob, lab, mask, ignore = make_case(SHAPES[name], Cc, dtype, 10)
        got = run_tsums(lib, prob, lab, beta, ignore, mask)
        want = ref.temperature_sums(prob, lab, beta, ignore, mask)
        assert got[0] == want[0] == (ref.classify(prob, lab, ignore, mask) == 1).sum()
        err = np.abs(got - want) / np.abs(want)
        print("%s C=%d beta=%g %s: relative errors of N, L, L', L'' %s" % (name, Cc, beta, dtype.__name__, err))
        assert (err <= 1e-12).all(), (got, want)
        assert run_tsums(lib, prob, lab, beta, ignore, mask).tobytes() == got.tobytes()


def test_temperature_sums_past_one_finishing_block_of_partials(lib):
    prob, lab, mask, ignore = make_case(SHAPES["partials"], 4, np.float64, 15)
    got, want = run_tsums(lib, prob, lab, 0.5, ignore, mask), ref.temperature_sums(prob, lab, 0.5, ignore, mask)
    err = np.abs(got - want) / np.abs(want)
    print("partials: relative errors of N, L, L', L'' %s" % err)
    assert got[0] == want[0] and (err <= 1e-12).all()
    assert run_tsums(lib, prob, lab, 0.5, ignore, mask).tobytes() == got.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_fit_temperature_on_the_device(lib, dtype):
    """the construction and the three conditions of tests/test_calibration_cpu.py, the sums coming from the device"""
    import torch
    from dep_gan_im_amd import evaluate
    from test_calibration_cpu import _check_fit
    n, H, W = 4, 64, 80
    p, lab = ref.softmax_problem(11, n * H * W)
    p = p.astype(dtype)
    fit = evaluate.fit_temperature(torch.from_numpy(p.reshape(n, H, W, 4)).cuda(), lab.reshape(n, H, W), tol=1e-6)
    print("fit_temperature %s: %s" % (dtype.__name__, fit))
    assert fit["n"] == n * H * W and fit["iterations"] <= 12
    _check_fit(fit, p, lab, 1e-6)
    hot = evaluate.fit_temperature(p.reshape(n, H, W, 4), lab.reshape(n, H, W), bounds=(0.5, 2.0))
    assert hot["at_bound"] and not hot["converged"] and hot["beta"] == 0.5


@pytest.mark.parametrize("T", [0.7, 3.0])
@pytest.mark.parametrize("Cc,dtype", [(2, np.float32), (4, np.float32), (3, np.float64), (4, np.float64), (8, np.float64)])
def test_apply_temperature(lib, Cc, dtype, T):
    import torch
    from dep_gan_im_amd import evaluate
    n, H, W = SHAPES["blocks"]
    prob, _, _, _ = make_case((n, H, W), Cc, dtype, 10)
    prob = prob[~np.isnan(prob).any(1)][:n * H * (W - 1)].reshape(n, H, W - 1, Cc)      # the planted zeros stay
    dev = torch.from_numpy(prob).cuda()
    out = evaluate.apply_temperature(dev, T)
    assert out.dtype == dev.dtype and out.shape == dev.shape and out.data_ptr() != dev.data_ptr()
    got = out.cpu().numpy().reshape(-1, Cc)
    want, want64 = ref.apply(prob.reshape(-1, Cc), 1.0 / T)
    if dtype == np.float64:
        err = float(np.max(np.abs(got - want64) / want64))
        print("apply C=%d float64 T=%g: relative error %.2e" % (Cc, T, err))
        assert err <= 1e-12
        rows = np.array([abs(math.fsum(r) - 1.0) for r in got]).max() / 2.0 ** -52
    else:
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, "float32: %d ulp from the restatement rounded once" % ulps.max()
        rows = np.abs(got.astype(np.float64).sum(1) - 1.0).max() / 2.0 ** -23
    print("apply C=%d %s T=%g: rows sum to 1 within %.2f ulp" % (Cc, dtype.__name__, T, rows))
    assert rows <= 4.0
    same = evaluate.apply_temperature(prob, T)                                 # from the host
    assert torch.equal(same, out)
    into = torch.empty_like(dev)
    assert evaluate.apply_temperature(dev, T, out=into) is into and torch.equal(into, out)
    assert evaluate.apply_temperature(dev, T, out=dev) is dev                  # in place
    assert dev.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()


def test_model_level_census_of_predict_stats(lib):
    """Gen_UNet2D(..., nc_out=4) at 16 x 48, the smallest size of tests/rect_cases.py: the float64 mean of three draws
    goes into the census as it is; every table holds every pixel that takes part"""
    import torch
    import dep_gan_im_amd as dg
    from dep_gan_im_amd import evaluate
    from rect_cases import URESNET_SIZES
    H, W = min(URESNET_SIZES)
    n = 2
    r = np.random.default_rng(5)
    net = dg.Gen_UNet2D((H, W, 1), nc_out=4, seed=3)
    x = r.standard_normal((n, H, W, 1)).astype(np.float32)
    codes = torch.from_numpy(r.integers(0, 4, (n, H, W)).astype(np.uint8)).cuda()
    stats = evaluate.predict_stats(net, x, n_repeat=3, rng=np.random.RandomState(0))
    assert stats["mean"].dtype == torch.float64 and tuple(stats["mean"].shape) == (n, H, W, 4)
    cen = evaluate.calibration_census(stats["mean"], codes)
    assert cen["n"] == n * H * W and cen["n_nan"] == 0
    assert cen["top_count"].sum() == cen["n"] and (cen["class_count"].sum(1) == cen["n"]).all()
    assert cen["class_pos"].sum() == cen["n"]
    want, _ = ref.census(stats["mean"].cpu().numpy().reshape(-1, 4), codes.cpu().numpy().reshape(-1), 15)
    assert np.array_equal(cen["top_conf_q"], want[:45].reshape(15, 3)[:, 2])
    m = evaluate.calibration_metrics(cen)
    assert 0.0 <= m["ece"] <= 1.0 and m["brier"] > 0 and m["nll"] > 0
    fit = evaluate.fit_temperature(stats["mean"], codes)
    assert fit["converged"] or fit["at_bound"]
