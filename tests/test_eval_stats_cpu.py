"""CPU: the host side of the per-draw prediction statistics -- data.affine_inverse, the NumPy restatement of the two
kernels (tests/eval_stats_ref.py) against direct NumPy formulas, the argument checks of evaluate.predict_stats, and the
C ABI entries."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_stats_ref as R  # noqa: E402

from dep_gan_im_amd import _lib, build, data, evaluate  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("depgan_eval_accumulate_stats", "depgan_eval_finish_stats")
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 1, 0], np.float32)


def compose(a, b):
    """the row of p -> a(b(p)) in float64 (elements 6, 7: 1, 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    A, B = a[[0, 1, 3, 4]].reshape(2, 2), b[[0, 1, 3, 4]].reshape(2, 2)
    M, t = A @ B, A @ b[[2, 5]] + a[[2, 5]]
    return np.array([M[0, 0], M[0, 1], t[0], M[1, 0], M[1, 1], t[1], 1.0, 0.0])


EXACT = [dict(), dict(flip_lr=True), dict(flip_ud=True), dict(rotate_deg=180.0), dict(rotate_deg=90.0),
         dict(rotate_deg=270.0, flip_lr=True), dict(shift=(3.0, -5.0)), dict(shift=(-2.0, 4.0), flip_ud=True)]


@pytest.mark.parametrize("H,W", [(13, 19), (16, 16)])
def test_affine_inverse_of_exact_maps_is_exact(H, W):
    rows = np.stack([data.affine_params(H, W, **kw) for kw in EXACT])
    inv = data.affine_inverse(rows)
    assert inv.dtype == np.float32 and inv.shape == rows.shape
    assert not np.signbit(inv[inv == 0]).any()              # no negative zero
    for r, i in zip(rows, inv):
        assert np.array_equal(compose(r, i), IDENTITY.astype(np.float64))
        assert np.array_equal(compose(i, r), IDENTITY.astype(np.float64))
    assert np.array_equal(data.affine_inverse(IDENTITY), IDENTITY)
    # gain and offset are not inverted
    g = data.affine_params(H, W, flip_lr=True, gain=1.3, offset=-0.2)
    assert np.array_equal(data.affine_inverse(g), data.affine_inverse(data.affine_params(H, W, flip_lr=True)))
    # leading axes are kept
    assert np.array_equal(data.affine_inverse(rows.reshape(2, 4, 8)), inv.reshape(2, 4, 8))


def test_affine_inverse_of_a_general_row_maps_the_grid_back():
    H, W = 13, 19
    rows = np.stack([data.affine_params(H, W, rotate_deg=10.0, scale=1.1, shift=(1.5, -2.0)),
                     data.affine_params(H, W, rotate_deg=-33.0, scale=0.8, shift=(-4.25, 3.0), flip_lr=True)])
    inv = data.affine_inverse(rows)
    oy, ox = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for r, i in zip(rows.astype(np.float64), inv.astype(np.float64)):
        sy, sx = r[0] * oy + r[1] * ox + r[2], r[3] * oy + r[4] * ox + r[5]
        by, bx = i[0] * sy + i[1] * sx + i[2], i[3] * sy + i[4] * sx + i[5]
        assert max(np.abs(by - oy).max(), np.abs(bx - ox).max()) < 1e-3
    assert np.array_equal(inv[:, 6:], np.tile(np.float32([1, 0]), (2, 1)))


@pytest.mark.parametrize("row", [[0, 0, 1, 0, 0, 1, 1, 0], [1, 2, 0, 2, 4, 0, 1, 0], [np.nan, 0, 0, 0, 1, 0, 1, 0],
                                 [1, 0, np.inf, 0, 1, 0, 1, 0]])
def test_affine_inverse_refuses_singular_and_non_finite_rows(row):
    with pytest.raises(ValueError):
        data.affine_inverse(np.array(row, np.float32))
    with pytest.raises(ValueError):
        data.affine_inverse(np.zeros((2, 7), np.float32))


def _draws(seed, R_, n, H, W, C):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((R_, n, H, W, C)) * rng.choice([0.1, 1.0, 5.0, 20.0], size=(1, n, H, W, 1))
    e = np.exp(logits - logits.max(-1, keepdims=True))
    p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    p[:, 0, 0, 0] = 0.0
    p[:, 0, 0, 0, 1] = 1.0                      # one-hot: the log edges
    return p


@pytest.mark.parametrize("ddof", [0, 1])
def test_restatement_against_direct_numpy(ddof):
    R_, n, H, W, C = 5, 2, 5, 7, 4
    p = _draws(3, R_, n, H, W, C)
    mask = (np.random.default_rng(4).uniform(size=(n, H, W)) > 0.3).astype(np.float32)
    st = R.new_state(n, H, W, C)
    for d in p:
        R.accumulate(st, d, mask)
    out = R.finish(st, R_, ddof)
    v = (p * mask[None, ..., None]).astype(np.float64)
    assert np.array_equal(st["count"], np.full((n, H, W), R_, np.uint8))
    assert np.array_equal(st["votes"].sum(-1), st["count"])
    want_votes = sum((np.arange(C) == np.argmax(d, -1)[..., None]).astype(np.uint8) for d in v)
    assert np.array_equal(st["votes"], want_votes)
    np.testing.assert_allclose(out["mean"], v.mean(0), rtol=1e-14, atol=0)
    assert np.abs(out["var"] - np.var(v, axis=0, ddof=ddof)).max() <= 1e-13 * max(1.0, (v * v).max())
    with np.errstate(divide="ignore", invalid="ignore"):
        def H_(q):
            return -np.where(q > 0, q * np.log(q), 0.0).sum(-1)
        ent, exp_ent = H_(v.mean(0)), H_(v).mean(0)
    assert np.abs(out["entropy"] - ent).max() < 1e-12
    assert np.abs(out["expected_entropy"] - exp_ent).max() < 1e-12
    assert np.abs(out["mutual_info"] - np.maximum(ent - exp_ent, 0)).max() < 1e-12
    assert (out["mutual_info"] >= 0).all() and out["mutual_info"].max() > 1e-3
    # one draw and ddof = 1: no degree of freedom is left, the variance is 0
    one = R.finish(R.accumulate(R.new_state(n, H, W, C), p[0]), 1, 1)
    assert not one["var"].any()


def test_restatement_valid_border_and_count():
    """an integer shift under 'valid': the pixels whose source lies outside take no part and finish as 0.0"""
    n, H, W, C = 1, 6, 9, 2
    p = _draws(5, 2, n, H, W, C)
    row = data.affine_params(H, W, shift=(2.0, 0.0))[None]          # source row = oy - 2
    st = R.new_state(n, H, W, C)
    for d in p:
        R.accumulate(st, d, None, row, "valid")
    assert np.array_equal(st["count"][0, :2], np.zeros((2, W), np.uint8)) and (st["count"][0, 2:] == 2).all()
    assert np.array_equal(st["sum"][0, 2:], p[:, 0, :-2].astype(np.float64).sum(0))
    out = R.finish(st, 2, 0, use_count=True)
    for k in ("mean", "var", "entropy", "expected_entropy", "mutual_info"):
        assert not out[k][0, :2].any(), k
    edge = R.new_state(n, H, W, C)
    R.accumulate(edge, p[0], None, row, "edge")
    assert (edge["count"] == 1).all() and np.array_equal(edge["sum"][0, 0], p[0, 0, 0].astype(np.float64))


def test_entry_points_are_declared_bound_and_built(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    declared = set(re.findall(r"\b(depgan_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "eval_stats.hip" in build.SOURCES
    assert len(_lib._HDR.prototypes["depgan_eval_accumulate_stats"][1]) == 14
    assert len(_lib._HDR.prototypes["depgan_eval_finish_stats"][1]) == 11
    assert evaluate.MAX_DRAWS == 255


class _NoDevice:
    """a model whose engine must never be asked for"""
    nc_out = 4

    def _ensure_engine(self, batch):
        raise AssertionError("predict_stats touched the model before it checked its arguments")


@pytest.mark.parametrize("kw", [dict(n_repeat=0), dict(n_repeat=256), dict(n_repeat=2.5), dict(border="wrap"),
                                dict(ddof=2), dict(tta=data.Augmenter(gain=(0.9, 1.1))),
                                dict(tta=data.Augmenter(offset=(-0.1, 0.1))),
                                dict(tta=np.zeros((3, 2, 8), np.float32), n_repeat=4),
                                dict(mask=np.ones((2, 8, 7), np.float32))])
def test_predict_stats_refuses_bad_arguments_before_any_device_call(kw):
    x = np.zeros((2, 8, 8, 1), np.float32)
    with pytest.raises(ValueError):
        evaluate.predict_stats(_NoDevice(), x, **kw)
    with pytest.raises(ValueError):
        evaluate.predict_stats(_NoDevice(), np.zeros((2, 8, 8), np.float32))
