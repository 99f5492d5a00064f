"""CPU: the host side of training-time augmentation (data.affine_params, data.Augmenter.draw) and the NumPy restatement
of depgan_data_augment that the GPU tests compare bits with (tests/augment_ref.py).

The restatement is checked two ways.  Exact cases -- identity, mirror, integer shift with fills, transpose -- against
plain NumPy indexing, bit for bit.  Random warps against the identical float64 statement sequence at the same float32
parameters: images within 2e-4 (three float32 roundings of a coordinate below 64 give <= 1.2e-5 px, times two axes,
times a neighbour difference <= 2 max|x| ~ 9), and at most 0.1 % of the label pixels may differ, since rounding can
flip a nearest-pixel tie; seeds 0..19."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from augment_ref import augment_ref  # noqa: E402
from dep_gan_im_amd import data  # noqa: E402

H, W = 40, 56
INDEX = [3, 0, 3, 4]
IDENT = np.array([1, 0, 0, 0, 1, 0, 1, 0], np.float32)


def _set(seed, h=H, w=W, nicg=2, n_src=5, C=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_src, h, w, nicg)).astype(np.float32)
    codes = rng.integers(0, C, (n_src, h, w)).astype(np.uint8)
    return x, codes, np.eye(C, dtype=np.float32)[codes]


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _src(row, oy, ox):
    return (float(row[0]) * oy + float(row[1]) * ox + float(row[2]), float(row[3]) * oy + float(row[4]) * ox + float(row[5]))


def test_affine_params_defaults_are_the_identity_row():
    row = data.affine_params(H, W)
    assert row.dtype == np.float32 and row.shape == (8,) and data.AUG_NPARAM == 8
    assert np.array_equal(row, IDENT) and not np.signbit(row).any()
    with pytest.raises(ValueError):
        data.affine_params(H, W, scale=0.0)
    with pytest.raises(ValueError):
        data.affine_params(0, W)


def test_affine_params_maps_the_corners():
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    lr = data.affine_params(H, W, flip_lr=True)
    assert np.array_equal(lr, np.array([1, 0, 0, 0, -1, W - 1, 1, 0], np.float32))
    ud = data.affine_params(H, W, flip_ud=True)
    assert [_src(ud, *c) for c in corners] == [(H - 1 - y, x) for y, x in corners]
    both = data.affine_params(H, W, flip_lr=True, flip_ud=True)
    assert np.array_equal(both, data.affine_params(H, W, rotate_deg=180.0))
    assert [_src(both, *c) for c in corners] == [(H - 1 - y, W - 1 - x) for y, x in corners]
    sh = data.affine_params(H, W, shift=(3, -5))                 # the picture moves 3 rows down, 5 columns left
    assert [_src(sh, *c) for c in corners] == [(y - 3, x + 5) for y, x in corners]
    # 90 degrees on a square image is np.rot90: out[i, j] = src[j, N-1-i]; with both flips it is rot90 the other way
    N = 40
    sq = [(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)]
    r90 = data.affine_params(N, N, rotate_deg=90.0)
    assert [_src(r90, *c) for c in sq] == [(x, N - 1 - y) for y, x in sq]
    assert np.array_equal(data.affine_params(N, N, rotate_deg=-270.0), r90)
    assert np.array_equal(data.affine_params(N, N, rotate_deg=90.0, flip_lr=True, flip_ud=True),
                          data.affine_params(N, N, rotate_deg=270.0))
    tr = data.affine_params(N, N, rotate_deg=90.0, flip_lr=True)  # transpose
    assert np.array_equal(tr, np.array([0, 1, 0, 1, 0, 0, 1, 0], np.float32))
    # scale 2 about the centre: the corners show the points half way to the centre; gain / offset pass through
    z2 = data.affine_params(H, W, scale=2.0, gain=1.5, offset=-0.25)
    assert [_src(z2, *c) for c in corners] == [((y + (H - 1) / 2) / 2, (x + (W - 1) / 2) / 2) for y, x in corners]
    assert z2[6] == 1.5 and z2[7] == -0.25
    # composed in float64, rounded once
    t = np.deg2rad(10.0)
    want = np.array([np.cos(t) / 1.1, np.sin(t) / 1.1, 0, -np.sin(t) / 1.1, np.cos(t) / 1.1, 0, 1, 0])
    cy, cx = (H - 1) / 2, (W - 1) / 2
    want[2] = cy - want[0] * (cy + 2.5) - want[1] * (cx - 1.25)
    want[5] = cx - want[3] * (cy + 2.5) - want[4] * (cx - 1.25)
    assert np.array_equal(data.affine_params(H, W, 10.0, 1.1, (2.5, -1.25)), want.astype(np.float32))


def test_augmenter_draw_repeats_stays_in_range_and_leaves_np_random_alone():
    kw = dict(rotate=15, scale=(0.9, 1.1), shift=4, flip_lr=True, flip_ud=True, gain=(0.8, 1.2), offset=(-0.1, 0.3))
    np.random.seed(123)
    state = np.random.get_state()
    a = data.Augmenter(seed=7, **kw)
    p1, p2 = a.draw(64, H, W), a.draw(64, H, W)
    q1 = data.Augmenter(seed=7, **kw).draw(64, H, W)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert p1.shape == (64, 8) and p1.dtype == np.float32
    assert np.array_equal(p1, q1) and not np.array_equal(p1, p2)
    assert not np.array_equal(p1, data.Augmenter(seed=8, **kw).draw(64, H, W))
    p = np.concatenate([p1, p2]).astype(np.float64)
    eps = 1e-6
    assert np.all(p[:, 6] >= 0.8 - eps) and np.all(p[:, 6] <= 1.2 + eps)
    assert np.all(p[:, 7] >= -0.1 - eps) and np.all(p[:, 7] <= 0.3 + eps)
    det = p[:, 0] * p[:, 4] - p[:, 1] * p[:, 3]                  # +-1 / scale^2; the sign is that of the mirrors
    assert np.all(np.abs(det) >= 1 / 1.1 ** 2 - eps) and np.all(np.abs(det) <= 1 / 0.9 ** 2 + eps)
    assert (det < 0).any() and (det > 0).any()
    s = 1.0 / np.sqrt(np.abs(det))
    cos = np.abs(p[:, 0]) * s                                     # |cos| of the angle, whatever the mirrors
    assert np.all(cos >= np.cos(np.deg2rad(15.0)) - eps) and np.all(np.abs(p[:, 1]) * s <= np.sin(np.deg2rad(15.0)) + eps)
    # the centre's source is the centre moved by the shift, turned and scaled: within 4 * sqrt(2) / 0.9 px of it
    cy, cx = (H - 1) / 2, (W - 1) / 2
    sy = p[:, 0] * cy + p[:, 1] * cx + p[:, 2] - cy
    sx = p[:, 3] * cy + p[:, 4] * cx + p[:, 5] - cx
    assert np.all(np.hypot(sy, sx) <= 4 * np.sqrt(2) / 0.9 + 1e-4)
    # identity ranges: every row is the identity row
    ident = data.Augmenter(seed=1)
    assert ident.identity and not a.identity and not data.Augmenter(flip_lr=True).identity
    assert np.array_equal(ident.draw(5, H, W), np.tile(IDENT, (5, 1)))
    with pytest.raises(ValueError):
        data.Augmenter(scale=(1.1, 0.9))
    with pytest.raises(ValueError):
        data.Augmenter(border="wrap")


@pytest.mark.parametrize("border", ["edge", "constant"])
def test_restatement_identity_returns_the_source_bits(border):
    x, codes, onehot = _set(0)
    P = np.tile(IDENT, (4, 1))
    out, lab = augment_ref(x, codes, P, INDEX, border, x_fill=-7.0, label_fill=9)
    assert out.dtype == np.float32 and np.array_equal(_u32(out), _u32(x[INDEX])) and np.array_equal(lab, codes[INDEX])
    out, lab = augment_ref(x, onehot, P, INDEX, border, x_fill=-7.0, label_fill=-1)
    assert np.array_equal(_u32(out), _u32(x[INDEX])) and np.array_equal(_u32(lab), _u32(onehot[INDEX]))


def test_restatement_exact_cases():
    x, codes, onehot = _set(1)
    flip = np.tile(np.array([1, 0, 0, 0, -1, W - 1, 1, 0], np.float32), (4, 1))
    out, lab = augment_ref(x, codes, flip, INDEX)
    assert np.array_equal(_u32(out), _u32(x[INDEX][:, :, ::-1])) and np.array_equal(lab, codes[INDEX][:, :, ::-1])
    # the picture moves 3 rows down and 5 columns left; what comes in from outside is the fill
    shift = np.tile(data.affine_params(H, W, shift=(3, -5)), (4, 1))
    out, lab = augment_ref(x, codes, shift, INDEX, "constant", x_fill=-7.0, label_fill=9)
    want = np.full((4, H, W, 2), -7.0, np.float32)
    want[:, 3:, :W - 5] = x[INDEX][:, :H - 3, 5:]
    wlab = np.full((4, H, W), 9, np.uint8)
    wlab[:, 3:, :W - 5] = codes[INDEX][:, :H - 3, 5:]
    assert np.array_equal(_u32(out), _u32(want)) and np.array_equal(lab, wlab)
    _, lab = augment_ref(x, onehot, shift, INDEX, "constant", label_fill=-1)
    woh = np.zeros((4, H, W, 3), np.float32)
    woh[:, 3:, :W - 5] = onehot[INDEX][:, :H - 3, 5:]
    assert np.array_equal(_u32(lab), _u32(woh))
    # the same shift with the edge border repeats the edge pixels
    out, lab = augment_ref(x, codes, shift, INDEX, "edge")
    yy, xx = np.clip(np.arange(H) - 3, 0, H - 1), np.clip(np.arange(W) + 5, 0, W - 1)
    assert np.array_equal(_u32(out), _u32(x[INDEX][:, yy][:, :, xx])) and np.array_equal(lab, codes[INDEX][:, yy][:, :, xx])
    # transpose on a square image
    xs, cs, _ = _set(2, 40, 40)
    tr = np.tile(np.array([0, 1, 0, 1, 0, 0, 1, 0], np.float32), (4, 1))
    out, lab = augment_ref(xs, cs, tr, INDEX)
    assert np.array_equal(_u32(out), _u32(xs[INDEX].transpose(0, 2, 1, 3))) and np.array_equal(lab, cs[INDEX].transpose(0, 2, 1))
    # an index outside the set: the fill values alone
    out, lab = augment_ref(x, codes, flip, [1, -1, 5, 2], x_fill=2.5, label_fill=4)
    assert np.all(out[1:3] == 2.5) and np.all(lab[1:3] == 4) and np.array_equal(_u32(out[3]), _u32(x[2][:, ::-1]))
    # gain and offset: one multiplication and one addition in float32
    go = np.tile(np.array([1, 0, 0, 0, 1, 0, 1.5, -0.25], np.float32), (4, 1))
    out, _ = augment_ref(x, None, go, INDEX)
    assert np.array_equal(_u32(out), _u32(np.float32(1.5) * x[INDEX] + np.float32(-0.25)))


def test_float32_restatement_against_float64():
    worst, flips, pixels = 0.0, 0, 0
    index = [3, 0, 3, 4, 1, 2, 2, 0]
    for seed in range(20):
        x, codes, _ = _set(100 + seed)
        P = data.Augmenter(rotate=15, scale=(0.9, 1.1), shift=4, flip_lr=True, flip_ud=True, seed=seed).draw(8, H, W)
        o32, l32 = augment_ref(x, codes, P, index)
        o64, l64 = augment_ref(x, codes, P, index, dtype=np.float64)
        assert o32.dtype == np.float32 and o64.dtype == np.float64
        worst = max(worst, float(np.abs(o32.astype(np.float64) - o64).max()))
        flips += int((l32 != l64).sum())
        pixels += l32.size
    print("float32 restatement against float64: max image difference %.3g, %d of %d label pixels differ"
          % (worst, flips, pixels))
    assert pixels == 358400
    assert worst <= 2e-4
    assert flips <= 0.001 * pixels
