"""CPU: the host side of the elastic / bias-field augmentation (data.Augmenter's elastic, bias, field_grid and
draw_fields, the argument checks of data.augment(fields=...)) and the NumPy restatement of depgan_data_augment_fields
that the GPU tests compare bits with (tests/elastic_ref.py).

The restatement is held against what the spline must do whatever its rounding: zero grids give tests/augment_ref.py's
bits, a constant grid gives the constant, the weights sum to 6 and t stays in [0, 1], and float32 stays within
64 * 2^-24 * max|C| of the identical float64 statements (each of the ~12 roundings on the way to a value contributes at
most a few units of 2^-24 of a partial sum that is at most 36 max|C| before the division; measured worst: 19.2).
A constant grid: the statements give the constant to 1e-7 relative -- held on the float64 yardstick, which gives
4.4e-16.  Their float32 roundings alone leave up to 5 units in the last place (3.1e-7 relative measured, 2.4e-7 for the
constant 1.0), more than 1e-7 whatever the constant, so float32 is held to the float32-against-float64 bound above."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elastic_ref as E  # noqa: E402
from augment_ref import augment_ref  # noqa: E402
from dep_gan_im_amd import data, evaluate  # noqa: E402

SHAPES = [(5, 7, 4, 4), (16, 256, 7, 7), (9, 300, 4, 32), (3, 512, 32, 4), (1, 1, 4, 4), (256, 256, 7, 7),
          (256, 256, 32, 32), (37, 53, 11, 6)]        # H, W, gh, gw


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set(seed, h, w, nicg=2, n_src=3, C=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_src, h, w, nicg)).astype(np.float32)
    codes = rng.integers(0, C, (n_src, h, w)).astype(np.uint8)
    return x, codes, np.eye(C, dtype=np.float32)[codes]


def test_the_header_constant():
    assert data.AUG_MAX_GRID == 32 == E.MAX_GRID


@pytest.mark.parametrize("border", ["edge", "constant"])
def test_zero_fields_give_the_affine_restatements_bits(border):
    H, W = 19, 23
    x, codes, onehot = _set(0, H, W)
    index = [2, 0, 2, 1]
    P = data.Augmenter(rotate=20, scale=(0.8, 1.2), shift=5, flip_lr=True, gain=(0.5, 1.5), offset=(-1, 1), seed=3).draw(4, H, W)
    Z = np.zeros((4, 3, 5, 6), np.float32)
    for labels, fill in ((codes, 7), (onehot, -1), (None, 0)):
        want, wlab = augment_ref(x, labels, P, index, border, -2.5, fill)
        got, lab, dense = E.elastic_ref(x, labels, P, Z, index, border, -2.5, fill)
        assert got.dtype == np.float32 and np.array_equal(_u32(got), _u32(want))
        assert (lab is None and wlab is None) or np.array_equal(lab, wlab)
        assert not dense.any() and not np.signbit(dense).any()


@pytest.mark.parametrize("H,W,gh,gw", SHAPES)
def test_weights_sum_to_six_t_stays_in_the_cell_and_a_constant_grid_is_the_constant(H, W, gh, gw):
    for size, g in ((H, gh), (W, gw)):
        c, B, t = E.spline_axis(size, g, np.float32)
        assert c.min() >= 0 and c.max() <= g - 4 and t.min() >= 0 and t.max() <= 1.0
        assert c[0] == 0 and t[0] == 0 and (size == 1 or (c[-1] == g - 4 and t[-1] > 0.999))
        assert all(b.min() >= 0 for b in B)
        total = B[0].astype(np.float64) + B[1] + B[2] + B[3]
        assert np.abs(total / 6 - 1).max() <= 1e-7
    grid = np.empty((3, gh, gw), np.float32)
    grid[0], grid[1], grid[2] = 2.75, -0.3, 1e-3
    const = grid[:, 0, 0].astype(np.float64)
    d64 = E.dense_fields(grid, H, W, np.float64)
    assert np.abs(d64 / const - 1).max() <= 1e-7                   # the statements themselves: 4.4e-16 measured
    d32 = E.dense_fields(grid, H, W).astype(np.float64)
    assert np.abs(d32 / const - 1).max() <= 64 * 2.0 ** -24        # their float32 roundings: the bound of the next test
    assert not E.dense_fields(np.zeros((3, gh, gw), np.float32), H, W).any()


def test_float32_fields_against_float64():
    worst = 0.0
    for k, (H, W, gh, gw) in enumerate(SHAPES):
        rng = np.random.default_rng(50 + k)
        for _ in range(5):
            grid = (rng.uniform(-1, 1, (3, gh, gw)) * np.array([8.0, 0.5, 100.0])[:, None, None]).astype(np.float32)
            d32, d64 = E.dense_fields(grid, H, W), E.dense_fields(grid, H, W, np.float64)
            assert d32.dtype == np.float32 and d64.dtype == np.float64
            err = np.abs(d32.astype(np.float64) - d64).max(axis=(0, 1)) / np.abs(grid).max(axis=(1, 2)) * 2.0 ** 24
            worst = max(worst, float(err.max()))
            # the spline of values in [-m, m] stays inside it: the weights are non-negative and sum to 1
            assert np.all(np.abs(d64).max(axis=(0, 1)) <= np.abs(grid).max(axis=(1, 2)) * (1 + 1e-6))
    print("float32 fields against float64: worst |difference| = %.1f * 2^-24 * max|C|" % worst)
    assert worst <= 64


def test_the_field_moves_the_picture_and_scales_the_intensity():
    """the sign conventions: a constant displacement grid (2, -3) shows the source 2 rows down and 3 columns left, a
    constant bias grid 0.5 is a gain of 1.5 -- to the few units in the last place the constant is reproduced to"""
    H, W = 12, 17
    x, codes, _ = _set(1, H, W)
    ident = np.tile(np.array([1, 0, 0, 0, 1, 0, 1, 0], np.float32), (3, 1))
    F = np.zeros((3, 3, 4, 5), np.float32)
    F[:, 0], F[:, 1], F[:, 2] = 2.0, -3.0, 0.5
    out, lab, dense = E.elastic_ref(x, codes, ident, F, None, "constant", x_fill=-7.0, label_fill=9)
    assert np.abs(dense - np.float32([2.0, -3.0, 0.5])).max() <= 64 * 2.0 ** -24 * 3
    want = np.full((3, H, W, 2), np.float32(-7.0) * np.float32(1.5), np.float32)
    want[:, :H - 2, 3:] = x[:, 2:, :W - 3] * np.float32(1.5)
    wlab = np.full((3, H, W), 9, np.uint8)
    wlab[:, :H - 2, 3:] = codes[:, 2:, :W - 3]                      # labels move with the picture, the bias skips them
    assert np.abs(out - want).max() <= 1e-4 and np.array_equal(lab, wlab)


def test_the_parameter_rows_of_a_seed_do_not_depend_on_the_fields():
    for s in (0, 5):
        closed = data.Augmenter(seed=s, rotate=10)
        opened = data.Augmenter(seed=s, rotate=10, elastic=3)
        for _ in range(3):
            want = closed.draw(6, 40, 56)
            assert np.array_equal(opened.draw(6, 40, 56), want)
            opened.draw_fields(6)
    # and an Augmenter written without the new arguments draws what it drew before they existed
    a, b = data.Augmenter(seed=4, rotate=10, flip_lr=True), data.Augmenter(seed=4, rotate=10, flip_lr=True, elastic=0.0, bias=0.0)
    assert np.array_equal(a.draw(5, 8, 8), b.draw(5, 8, 8)) and not a.fields_open and not b.fields_open


def test_draw_fields_repeats_for_a_seed_and_respects_its_ranges():
    np.random.seed(9)
    state = np.random.get_state()
    a = data.Augmenter(seed=7, elastic=2.5, bias=0.25, field_grid=(5, 9))
    f1, f2 = a.draw_fields(16), a.draw_fields(16)
    g1 = data.Augmenter(seed=7, elastic=2.5, bias=0.25, field_grid=(5, 9)).draw_fields(16)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert f1.shape == (16, 3, 5, 9) and f1.dtype == np.float32
    assert np.array_equal(f1, g1) and not np.array_equal(f1, f2)
    assert not np.array_equal(f1, data.Augmenter(seed=8, elastic=2.5, bias=0.25, field_grid=(5, 9)).draw_fields(16))
    f = np.concatenate([f1, f2])
    assert np.abs(f[:, :2]).max() <= 2.5 and np.abs(f[:, :2]).max() > 2.0
    assert np.abs(f[:, 2]).max() <= 0.25 and np.abs(f[:, 2]).max() > 0.2
    only = data.Augmenter(seed=7, bias=0.25).draw_fields(4)          # one range open: all three planes are drawn
    assert only.shape == (4, 3, 7, 7) and not only[:, :2].any() and only[:, 2].any()
    assert not data.Augmenter(seed=1).draw_fields(2).any()


def test_identity_and_fields_open_account_for_the_new_ranges():
    assert data.Augmenter().identity and not data.Augmenter().fields_open
    for kw in (dict(elastic=1.0), dict(bias=0.1)):
        a = data.Augmenter(**kw)
        assert a.fields_open and not a.identity
    assert data.Augmenter(field_grid=(4, 32)).identity


def test_argument_errors():
    for kw in (dict(elastic=-1.0), dict(elastic=np.inf), dict(elastic=np.nan), dict(bias=-0.1), dict(bias=1.0),
               dict(bias=np.nan), dict(field_grid=(3, 7)), dict(field_grid=(7, 33)), dict(field_grid=7),
               dict(field_grid=(7, 7, 7)), dict(field_grid=(7.0, 7)), dict(field_grid=(True, 7))):
        with pytest.raises(ValueError):
            data.Augmenter(**kw)
    # data.augment(fields=...): shapes and ranges are refused on the host, before anything touches the device
    x = np.zeros((3, 8, 8, 1), np.float32)
    ok = np.zeros((3, 3, 4, 4), np.float32)
    for kw in (dict(fields=ok[:2]), dict(fields=ok[:, :2]), dict(fields=ok[0, 0]), dict(fields=ok[None]),
               dict(fields=np.zeros((3, 3, 3, 4), np.float32)), dict(fields=np.zeros((3, 3, 4, 33), np.float32)),
               dict(fields=np.zeros((3, 40, 4), np.float32)), dict(fields=ok, index=[0, 1]), dict(return_fields=True),
               dict(fields=ok, index=torch.tensor([0, 1])), dict(fields=torch.zeros((2, 3, 4, 4))),
               dict(fields=torch.zeros((3, 4, 40)))):
        with pytest.raises(ValueError):
            data.augment(x, **kw)
    # predict_stats refuses an Augmenter whose map has no inverse row
    for kw in (dict(elastic=1), dict(bias=0.1)):
        with pytest.raises(ValueError, match="elastic"):
            evaluate._stats_arguments(x, 2, None, data.Augmenter(**kw), "valid", 0)
    assert evaluate._stats_arguments(x, 2, None, data.Augmenter(rotate=5), "valid", 0)[:3] == (3, 8, 8)
