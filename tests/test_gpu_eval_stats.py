"""GPU: depgan_eval_accumulate_stats and depgan_eval_finish_stats at operator level, synthetic predictions fed straight
to the entries, against the NumPy restatement (tests/eval_stats_ref.py).

Everything without a log is asserted bit for bit; the three entropy outputs within 1e-12 absolute (a device double log
and NumPy's differ by an ulp or two; each term is at most 1/e, at most 8 terms and 5 draws).  Shapes: 3 x 13 x 19 (H*W
is no multiple of 256, so blocks straddle samples) and 3 x 16 x 16 (every block inside one sample)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_stats_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

N = 3
ENT_TOL = 1e-12
LOG_KEYS = ("entropy", "expected_entropy", "mutual_info")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def make_draws(seed, n_draws, H, W, Cc, nan=True):
    """float32 softmax rows of logits at scales 0.1 .. 20, with the edge cases planted in sample 0, row 0"""
    rng = np.random.default_rng(seed)
    if Cc == 1:
        p = rng.uniform(-1, 1, size=(n_draws, N, H, W, 1)).astype(np.float32)
        p[:, 0, 0, 1] = 0.0
    else:
        logits = rng.standard_normal((n_draws, N, H, W, Cc)) * rng.choice([0.1, 1.0, 5.0, 20.0], size=(1, N, H, W, 1))
        e = np.exp(logits - logits.max(-1, keepdims=True))
        p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
        p[:, 0, 0, 0] = 0.0
        p[:, 0, 0, 0, Cc - 1] = 1.0              # exactly one-hot
        p[:, 0, 0, 1] = 0.0                      # exactly zero: every log edge
        p[:, 0, 0, 2] = np.float32(1.0 / Cc)     # an exact tie of all channels: class 0 wins
        p[:, 0, 0, 3] = 0.0
        p[:, 0, 0, 3, [Cc - 2, Cc - 1]] = 0.5    # a tie of the last two: the first of them wins
    if nan:
        p[1, 1, 2, 3, Cc - 1] = np.nan           # a NaN counts as the maximum ...
        p[0, 1, 2, 4, 0] = np.nan                # ... and the first one wins
        if Cc > 1:
            p[0, 1, 2, 4, 1] = np.nan
    return p


def make_mask(seed, H, W):
    rng = np.random.default_rng(seed)
    m = rng.choice(np.float32([0.0, 1.0, 0.7]), size=(N, H, W), p=[0.3, 0.5, 0.2])
    m[0, 0, :4] = 1.0                            # the planted rows of make_draws keep their values
    return m


class Device:
    """the state of one run on the device"""

    def __init__(self, lib, H, W, Cc):
        import torch
        self.torch, self.lib, self.H, self.W, self.C = torch, lib, H, W, Cc
        dev = torch.device("cuda:0")
        f64 = dict(dtype=torch.float64, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        many = Cc > 1
        self.t = {"sum": torch.zeros((N, H, W, Cc), **f64),
                  "sumsq": torch.zeros((N, H, W, Cc), **f64),
                  "ent_sum": torch.zeros((N, H, W), **f64) if many else None,
                  "votes": torch.zeros((N, H, W, Cc), **u8) if many else None,
                  "count": torch.zeros((N, H, W), **u8)}
        self.stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.dev = dev

    def up(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.dev)

    def accumulate(self, pred, mask=None, params=None, border="edge"):
        t = self.t
        self.keep = [self.up(pred), self.up(mask), self.up(params)]
        return self.lib.depgan_eval_accumulate_stats(
            _p(self.keep[0]), _p(self.keep[1]), _p(self.keep[2]), R.BORDERS[border] * 1, N, self.H, self.W, self.C,
            _p(t["sum"]), _p(t["sumsq"]), _p(t["ent_sum"]), _p(t["votes"]), _p(t["count"]), self.stream)

    def state(self):
        self.torch.cuda.synchronize()
        return {k: (None if v is None else v.cpu().numpy()) for k, v in self.t.items()}

    def finish(self, n_draws, ddof, use_count):
        torch, t = self.torch, self.t
        many = self.C > 1
        ent = torch.full((N, self.H, self.W), -1.0, dtype=torch.float64, device=self.dev) if many else None
        mi = torch.full((N, self.H, self.W), -1.0, dtype=torch.float64, device=self.dev) if many else None
        rc = self.lib.depgan_eval_finish_stats(_p(t["sum"]), _p(t["sumsq"]), _p(t["ent_sum"]),
                                               _p(t["count"]) if use_count else None, _p(ent), _p(mi),
                                               N * self.H * self.W, self.C, n_draws, ddof, self.stream)
        assert rc == 0
        torch.cuda.synchronize()
        out = {"mean": t["sum"].cpu().numpy(), "var": t["sumsq"].cpu().numpy()}
        if many:
            out.update({"expected_entropy": t["ent_sum"].cpu().numpy(), "entropy": ent.cpu().numpy(),
                        "mutual_info": mi.cpu().numpy()})
        return out


def same_bits(got, want, what):
    """bit for bit; a NaN matches a NaN (which payload a NaN carries through an add is the hardware's business)"""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.dtype == np.float64:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        got, want = np.where(nan, 0.0, got).view(np.uint64), np.where(nan, 0.0, want).view(np.uint64)
    assert np.array_equal(got, want), what


def check_state(got, want):
    for k in ("sum", "sumsq", "votes", "count"):
        if got[k] is not None:
            same_bits(got[k], want[k], k)
    if got["ent_sum"] is not None:
        err = float(np.abs(got["ent_sum"] - want["ent_sum"]).max())
        print("ent_sum: worst |device - NumPy| = %.3e" % err)
        assert err <= ENT_TOL


def check_finished(got, want):
    same_bits(got["mean"], want["mean"], "mean")
    same_bits(got["var"], want["var"], "var")
    for k in LOG_KEYS:
        if k in got:
            err = float(np.abs(got[k] - want[k]).max())
            print("%s: worst |device - NumPy| = %.3e" % (k, err))
            assert err <= ENT_TOL, k
    if "mutual_info" in got:
        assert (got["mutual_info"] >= 0).all()


@pytest.mark.parametrize("H,W,Cc,n_draws,ddof,masked", [(13, 19, 1, 3, 0, True), (13, 19, 2, 5, 1, True),
                                                       (13, 19, 4, 3, 1, True), (13, 19, 8, 5, 0, True),
                                                       (13, 19, 4, 5, 0, False), (16, 16, 4, 3, 0, True)])
def test_draw_statistics_against_the_restatement(lib, H, W, Cc, n_draws, ddof, masked):
    import torch
    draws = make_draws(100 + Cc + n_draws, n_draws, H, W, Cc)
    mask = make_mask(7, H, W) if masked else None
    d, ref = Device(lib, H, W, Cc), R.new_state(N, H, W, Cc)
    # the running sum of the existing entry on the same draws, and its mean
    acc = torch.zeros((N, H, W, Cc), dtype=torch.float64, device=d.dev)
    for p in draws:
        assert d.accumulate(p, mask) == 0
        assert lib.depgan_eval_accumulate_channels(_p(d.keep[0]), _p(d.keep[1]), _p(acc), N * H * W, Cc, d.stream) == 0
        R.accumulate(ref, p, mask)
    got = d.state()
    if Cc == 1:
        ref["ent_sum"] = ref["votes"] = None
    check_state(got, ref)
    same_bits(got["sum"], acc.cpu().numpy(), "sum against depgan_eval_accumulate_channels")
    assert (got["count"] == n_draws).all()
    if Cc > 1:
        assert np.array_equal(got["votes"].sum(-1), got["count"])
        assert got["votes"][0, 0, 0, Cc - 1] == n_draws and got["votes"][0, 0, 1, 0] == n_draws
        assert got["votes"][0, 0, 2, 0] == n_draws and got["votes"][0, 0, 3, Cc - 2] == n_draws
        if mask is not None:                     # a pixel the mask zeroed votes for class 0
            zeroed = (mask == 0) & np.isfinite(draws).all((0, 4))
            assert zeroed.sum() > 100 and (got["votes"][zeroed][:, 0] == n_draws).all()
        # NaN * 0 is NaN: the mask does not remove it
        assert got["votes"][1, 2, 4, 0] >= 1 and got["votes"][1, 2, 3, Cc - 1] >= 1
    fin = d.finish(n_draws, ddof, use_count=False)
    check_finished(fin, R.finish(ref, n_draws, ddof))
    assert lib.depgan_eval_divide(_p(acc), acc.numel(), float(n_draws), d.stream) == 0
    torch.cuda.synchronize()
    same_bits(fin["mean"], acc.cpu().numpy(), "mean against depgan_eval_divide")
    # the variance against NumPy's own, two-pass: the formula's error is a few ulp of sumsq / R
    v = draws.astype(np.float64) if mask is None else (draws * mask[None, ..., None]).astype(np.float64)
    ok = np.isfinite(v).all(0)
    want = np.var(np.where(ok, v, 0.0), axis=0, ddof=ddof)
    err = float(np.abs(fin["var"] - want)[ok].max())
    bound = 1e-13 * max(1.0, float((v * v)[:, ok].max()))
    print("var: worst |device - np.var| = %.3e (bound %.1e)" % (err, bound))
    assert err <= bound
    assert np.isnan(fin["var"][~ok]).all() and (~ok).sum() >= 2


def _exact_rows(H, W, kinds):
    from dep_gan_im_amd import data
    return np.stack([data.affine_params(H, W, **k) for k in kinds])


@pytest.mark.parametrize("border", ["edge", "valid"])
@pytest.mark.parametrize("H,W,kinds,views", [
    (13, 19, [dict(flip_lr=True), dict(flip_ud=True), dict(rotate_deg=180.0)],
     [lambda a: a[:, ::-1], lambda a: a[::-1], lambda a: a[::-1, ::-1]]),
    (13, 19, [dict(), dict(), dict()], [lambda a: a] * 3),
    (16, 16, [dict(rotate_deg=90.0), dict(rotate_deg=270.0), dict(rotate_deg=90.0, flip_lr=True)],
     [lambda a: np.rot90(a, 1), lambda a: np.rot90(a, -1), lambda a: np.rot90(a[:, ::-1], 1)])])
def test_tta_exact_maps_are_flips_and_quarter_turns(lib, border, H, W, kinds, views):
    """sample i accumulated through row i is the flipped / turned prediction, and the flipped / turned prediction
    accumulated through the inverse row is the prediction again: bit for bit, and no pixel is lost under 'valid'"""
    from dep_gan_im_amd import data
    Cc, n_draws = 4, 3
    draws = make_draws(31, n_draws, H, W, Cc, nan=False)
    rows = _exact_rows(H, W, kinds)
    inv = data.affine_inverse(rows)
    turned = np.stack([np.stack([views[i](p[i]) for i in range(N)]) for p in draws])
    fwd, back = Device(lib, H, W, Cc), Device(lib, H, W, Cc)
    for p, q in zip(draws, turned):
        assert fwd.accumulate(p, None, rows, border) == 0
        assert back.accumulate(q, None, inv, border) == 0
    got_f, got_b = fwd.state(), back.state()
    same_bits(got_f["sum"], sum_in_order(turned.astype(np.float64)), "sum through the rows")
    same_bits(got_b["sum"], sum_in_order(draws.astype(np.float64)), "sum through the inverse rows")
    assert (got_f["count"] == n_draws).all() and (got_b["count"] == n_draws).all()
    check_state(got_b, ref_run(turned, None, [inv] * n_draws, border, Cc))


def sum_in_order(a):
    s = np.zeros(a.shape[1:])
    for d in a:
        s = s + d
    return s


def ref_run(draws, mask, params, border, Cc):
    H, W = draws.shape[2:4]
    ref = R.new_state(N, H, W, Cc)
    for p, rows in zip(draws, params):
        R.accumulate(ref, p, mask, rows, border)
    if Cc == 1:
        ref["ent_sum"] = ref["votes"] = None
    return ref


@pytest.mark.parametrize("border", ["edge", "valid"])
@pytest.mark.parametrize("H,W,Cc,n_draws", [(13, 19, 4, 3), (13, 19, 1, 5), (16, 16, 8, 3)])
def test_tta_general_map(lib, border, H, W, Cc, n_draws):
    """rotate 10 degrees, scale 1.1, shift (1.5, -2): sample 0 in every draw, sample 1 in the first draw only (identity
    afterwards), sample 2 through the inverse row"""
    from dep_gan_im_amd import data
    gen = data.affine_params(H, W, rotate_deg=10.0, scale=1.1, shift=(1.5, -2.0))
    ident = data.affine_params(H, W)
    params = [np.stack([gen, gen if r == 0 else ident, data.affine_inverse(gen)]) for r in range(n_draws)]
    draws, mask = make_draws(57 + Cc, n_draws, H, W, Cc), make_mask(9, H, W)
    d = Device(lib, H, W, Cc)
    for p, rows in zip(draws, params):
        assert d.accumulate(p, mask, rows, border) == 0
    got, ref = d.state(), ref_run(draws, mask, params, border, Cc)
    check_state(got, ref)
    count = got["count"]
    cy, cx = H // 2, W // 2
    assert (count[:, cy, cx] == n_draws).all()
    corners = count[:, [0, 0, -1, -1], [0, -1, 0, -1]]
    if border == "edge":
        assert (count == n_draws).all()
    else:
        assert (corners[0] < n_draws).any() and (corners[1] < n_draws).any() and (count[0] == 0).any()
        assert count[1].min() == n_draws - 1
    ddof = 1 if Cc == 8 else 0
    fin = d.finish(n_draws, ddof, use_count=True)
    check_finished(fin, R.finish(ref, n_draws, ddof, use_count=True))
    for k, a in fin.items():
        assert not a[count == 0].any(), k


def test_finish_with_count_and_ddof_one(lib):
    """R per pixel from count: where one draw is left and ddof = 1 the variance is 0"""
    from dep_gan_im_amd import data
    H, W, Cc, n_draws = 13, 19, 2, 3
    gen = data.affine_params(H, W, rotate_deg=10.0, scale=1.1, shift=(1.5, -2.0))
    ident = data.affine_params(H, W)
    params = [np.stack([gen, gen if r else ident, ident]) for r in range(n_draws)]
    draws = make_draws(77, n_draws, H, W, Cc, nan=False)
    d = Device(lib, H, W, Cc)
    for p, rows in zip(draws, params):
        assert d.accumulate(p, None, rows, "valid") == 0
    got, ref = d.state(), ref_run(draws, None, params, "valid", Cc)
    check_state(got, ref)
    assert (got["count"] == 1).any() and (got["count"] == 0).any()
    fin = d.finish(n_draws, 1, use_count=True)
    check_finished(fin, R.finish(ref, n_draws, 1, use_count=True))
    assert not fin["var"][got["count"] <= 1].any()


def test_refusals_launch_nothing(lib):
    import torch
    H, W = 13, 19
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    npix = N * H * W

    def call(Cc, pred, sum_, sumsq=None, ent=None, votes=None, count=None, params=None):
        return lib.depgan_eval_accumulate_stats(_p(pred), None, _p(params), 0, N, H, W, Cc, _p(sum_), _p(sumsq),
                                                _p(ent), _p(votes), _p(count), stream)

    pred = torch.ones((N, H, W, 9), dtype=torch.float32, device=dev)
    big = torch.zeros((2 * npix * 9,), dtype=torch.float64, device=dev)
    ent = torch.zeros((npix,), dtype=torch.float64, device=dev)
    votes = torch.zeros((npix * 9,), dtype=torch.uint8, device=dev)
    assert call(9, pred, big) == 1                                         # C = 9
    assert call(0, pred, big) == 1
    assert call(1, pred, big, ent=ent) == 1                                # entropy of one channel
    assert call(1, pred, big, votes=votes) == 1
    assert call(4, pred, big, sumsq=big) == 1                              # two state ranges are one
    assert call(4, pred, big, sumsq=big[npix * 4 - 1:]) == 1               # ... or overlap by one element
    assert call(4, pred, pred.reshape(-1)[:-1].view(torch.float64)) == 1   # the state is the prediction
    assert call(4, pred, big, ent=big[8:]) == 1
    assert call(4, pred, big, params=big.view(torch.float32)) == 1
    assert call(4, pred, None) == 1 and call(4, None, big) == 1
    assert lib.depgan_eval_accumulate_stats(_p(pred), None, None, 2, N, H, W, 4, _p(big), None, None, None, None,
                                            stream) == 1                   # border
    assert lib.depgan_eval_finish_stats(_p(big), _p(big), None, None, None, None, npix, 4, 3, 0, stream) == 1
    assert lib.depgan_eval_finish_stats(_p(big), None, None, None, None, None, npix, 4, 0, 0, stream) == 1
    assert lib.depgan_eval_finish_stats(_p(big), None, None, None, None, None, npix, 4, 256, 0, stream) == 1
    assert lib.depgan_eval_finish_stats(_p(big), None, None, None, None, None, npix, 4, 3, 2, stream) == 1
    assert lib.depgan_eval_finish_stats(_p(big), None, _p(ent), None, None, None, npix, 1, 3, 0, stream) == 1
    assert lib.depgan_eval_finish_stats(_p(big), None, None, None, None, _p(ent), npix, 4, 3, 0, stream) == 1
    torch.cuda.synchronize()
    assert not big.any() and not ent.any() and not votes.any() and bool((pred == 1).all())
    assert b"eval_" in lib.depgan_last_error()
    # the adjacent ranges of one allocation are fine
    assert call(4, pred[..., :4].contiguous(), big, sumsq=big[npix * 4:]) == 0
    torch.cuda.synchronize()
    assert bool((big[:npix * 4] == 1).all()) and bool((big[npix * 4:npix * 8] == 1).all())
