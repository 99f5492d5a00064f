"""GPU: training-time augmentation -- depgan_data_augment through data.augment, the C entry and GeneratorModel.fit.

Shapes are the smallest at which the kernel can go wrong: 37 x 53 (H != W, 4 * 37 * 53 = 7844 pixels: 31 blocks, the
last one partly empty), 1 and 2 image channels, class codes and one-hot rows of 3 and 8 classes, a repeated index and
none, both borders.  Exact cases (identity, mirror, integer shift with fills, transpose) are compared with plain NumPy
indexing; random warps, one parameter row per sample, with the float32 restatement tests/augment_ref.py -- images as
uint32 bit patterns, labels equal.  The inputs hold no subnormals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from augment_ref import augment_ref  # noqa: E402
from dep_gan_im_amd import _lib, data  # noqa: E402

pytestmark = pytest.mark.gpu
H, W, N_SRC = 37, 53, 5
INDEX = [3, 0, 3, 4]
IDENT = np.array([1, 0, 0, 0, 1, 0, 1, 0], np.float32)
DEV = "cuda:0"


def _set(seed, h=H, w=W, nicg=2, C=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N_SRC, h, w, nicg)).astype(np.float32)
    assert np.all(np.abs(x) >= np.finfo(np.float32).tiny)           # no subnormals (and no zeros)
    codes = rng.integers(0, C, (N_SRC, h, w)).astype(np.uint8)
    return x, codes, np.eye(C, dtype=np.float32)[codes]


def _u32(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("border", ["edge", "constant"])
@pytest.mark.parametrize("nicg", [1, 2])
def test_identity_returns_the_source_bits(border, nicg):
    x, codes, onehot = _set(0, nicg=nicg)
    P = np.tile(IDENT, (4, 1))
    out, lab = data.augment(x, codes, P, INDEX, border, x_fill=-7.0, label_fill=9)
    assert out.is_cuda and out.dtype == torch.float32 and lab.dtype == torch.uint8 and tuple(lab.shape) == (4, H, W)
    assert np.array_equal(_u32(out), _u32(x[INDEX])) and np.array_equal(_np(lab), codes[INDEX])
    # index=None, a single row for every sample, labels (n, H, W, 1), everything resident on the device
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(codes[..., None]).to(DEV)
    out, lab = data.augment(xd, cd, IDENT, None, border)
    assert tuple(lab.shape) == (N_SRC, H, W, 1)
    assert np.array_equal(_u32(out), _u32(x)) and np.array_equal(_np(lab)[..., 0], codes)
    out, lab = data.augment(xd, onehot, None, torch.tensor(INDEX, device=DEV), border, label_fill=-1)
    assert np.array_equal(_u32(out), _u32(x[INDEX])) and np.array_equal(_u32(lab), _u32(onehot[INDEX]))
    out, lab = data.augment(x)
    assert lab is None and np.array_equal(_u32(out), _u32(x))


def test_exact_cases():
    x, codes, onehot = _set(1)
    flip = np.tile(np.array([1, 0, 0, 0, -1, W - 1, 1, 0], np.float32), (4, 1))
    out, lab = data.augment(x, codes, flip, INDEX)
    assert np.array_equal(_u32(out), _u32(x[INDEX][:, :, ::-1])) and np.array_equal(_np(lab), codes[INDEX][:, :, ::-1])
    # the picture moves 3 rows down and 5 columns left; what comes in from outside is the fill
    shift = data.affine_params(H, W, shift=(3, -5))
    out, lab = data.augment(x, codes, shift, INDEX, "constant", x_fill=-7.0, label_fill=9)
    want = np.full((4, H, W, 2), -7.0, np.float32)
    want[:, 3:, :W - 5] = x[INDEX][:, :H - 3, 5:]
    wlab = np.full((4, H, W), 9, np.uint8)
    wlab[:, 3:, :W - 5] = codes[INDEX][:, :H - 3, 5:]
    assert np.array_equal(_u32(out), _u32(want)) and np.array_equal(_np(lab), wlab)
    out, lab = data.augment(x, codes, shift, INDEX, "edge")
    yy, xx = np.clip(np.arange(H) - 3, 0, H - 1), np.clip(np.arange(W) + 5, 0, W - 1)
    assert np.array_equal(_u32(out), _u32(x[INDEX][:, yy][:, :, xx]))
    assert np.array_equal(_np(lab), codes[INDEX][:, yy][:, :, xx])
    # transpose on a square image
    xs, cs, _ = _set(2, 37, 37)
    out, lab = data.augment(xs, cs, np.array([0, 1, 0, 1, 0, 0, 1, 0], np.float32), INDEX)
    assert np.array_equal(_u32(out), _u32(xs[INDEX].transpose(0, 2, 1, 3)))
    assert np.array_equal(_np(lab), cs[INDEX].transpose(0, 2, 1))
    # gain and offset: one multiplication and one addition in float32
    out, _ = data.augment(x, None, np.array([1, 0, 0, 0, 1, 0, 1.5, -0.25], np.float32), INDEX)
    assert np.array_equal(_u32(out), _u32(np.float32(1.5) * x[INDEX] + np.float32(-0.25)))


def test_one_hot_rows_are_copied_bits_and_fills():
    """Rows of arbitrary float32 bit patterns come out as they went in; outside the image the row is all zero
    (label_fill = -1) or e_2 (label_fill = 2)."""
    x, _, _ = _set(3, nicg=1)
    rng = np.random.default_rng(4)
    for Cc in (3, 8):
        rows = rng.integers(0, 2 ** 32, (N_SRC, H, W, Cc), dtype=np.uint64).astype(np.uint32).view(np.float32)
        shift = data.affine_params(H, W, shift=(-4, 6))            # rows H-4.. and columns ..5 come from outside
        for fill in (-1, 2):
            _, lab = data.augment(x, torch.from_numpy(rows).to(DEV), shift, INDEX, "constant", label_fill=fill)
            got = _np(lab).view(np.uint32)
            want = np.zeros((4, H, W, Cc), np.float32)
            if fill >= 0:
                want[..., fill] = 1.0
            want = want.view(np.uint32)
            want[:, :H - 4, 6:] = rows.view(np.uint32)[INDEX][:, 4:, :W - 6]
            assert np.array_equal(got, want)


CONFIGS = [  # nicg, labels, classes, border, x_fill, label_fill, index
    (1, "codes", 3, "edge", 0.0, 0, None),
    (2, "onehot", 3, "constant", 0.5, -1, INDEX),
    (1, "onehot", 8, "constant", -7.0, 2, INDEX),
    (2, "codes", 3, "constant", 2.0, 9, None),
    (2, "none", 3, "edge", 0.0, 0, INDEX),
]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_warps_match_the_float32_restatement_bit_for_bit(seed):
    for k, (nicg, kind, Cc, border, x_fill, label_fill, index) in enumerate(CONFIGS):
        x, codes, onehot = _set(10 * seed + k, nicg=nicg, C=Cc)
        labels = {"codes": codes, "onehot": onehot, "none": None}[kind]
        n = N_SRC if index is None else len(index)
        aug = data.Augmenter(rotate=25, scale=(0.7, 1.4), shift=10, flip_lr=True, flip_ud=True, gain=(0.5, 1.5),
                             offset=(-1.0, 1.0), seed=100 * seed + k)
        P = aug.draw(n, H, W)
        assert len({tuple(r) for r in P}) == n                       # a different row for each sample
        P[-1, 2] = 3e9 if k % 2 else -3e9                            # one sample entirely outside, far past 2^31
        out, lab = data.augment(x, labels, P, index, border, x_fill, label_fill)
        want, wlab = augment_ref(x, labels, P, index, border, x_fill, label_fill)
        assert want.dtype == np.float32
        assert np.array_equal(_u32(out), _u32(want)), (seed, k)
        if labels is None:
            assert lab is None
        elif kind == "codes":
            assert np.array_equal(_np(lab), wlab), (seed, k)
        else:
            assert np.array_equal(_u32(lab), _u32(wlab)), (seed, k)
        if border == "constant" and kind == "codes":                 # the far sample's labels are the fill
            assert np.all(_np(lab[-1]) == label_fill)


def _entry(x, lab, kind, Cc, index, n_src, params, n, h, w, border, x_fill, label_fill, x_out, lab_out):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _lib.load().depgan_data_augment(p(x), x.shape[3], p(lab), kind, Cc, p(index), n_src, p(params), n, h, w,
                                           border, x_fill, label_fill, p(x_out), p(lab_out), st)


def test_an_index_outside_the_set_gives_the_fill_values():
    """depgan_data_augment itself: index -1 and n_src are samples of x_fill / label_fill, status 0; the samples around
    them are untouched by it."""
    x, codes, onehot = _set(5)
    xd, cd, od = (torch.from_numpy(a).to(DEV) for a in (x, codes, onehot))
    idx = torch.tensor([1, -1, N_SRC, 2], dtype=torch.int64, device=DEV)
    P = torch.from_numpy(np.tile(IDENT, (4, 1))).to(DEV)
    xo = torch.full((4, H, W, 2), np.nan, dtype=torch.float32, device=DEV)
    lo = torch.full((4, H, W), 77, dtype=torch.uint8, device=DEV)
    assert _entry(xd, cd, 1, 0, idx, N_SRC, P, 4, H, W, 0, 2.5, 4, xo, lo) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_u32(xo[[0, 3]]), _u32(x[[1, 2]])) and np.array_equal(_np(lo[[0, 3]]), codes[[1, 2]])
    assert np.all(_np(xo[1:3]) == 2.5) and np.all(_np(lo[1:3]) == 4)
    oo = torch.full((4, H, W, 3), np.nan, dtype=torch.float32, device=DEV)
    assert _entry(xd, od, 2, 3, idx, N_SRC, P, 4, H, W, 1, 2.5, -1, xo, oo) == 0
    torch.cuda.synchronize()
    assert np.all(_np(oo[1:3]) == 0) and np.array_equal(_u32(oo[[0, 3]]), _u32(onehot[[1, 2]]))
    assert np.all(_np(xo[1:3]) == 2.5)


def test_bad_arguments():
    x, codes, onehot = _set(6)
    xd, cd, od = (torch.from_numpy(a).to(DEV) for a in (x, codes, onehot))
    P = torch.from_numpy(np.tile(IDENT, (N_SRC, 1))).to(DEV)
    xo, lo = torch.empty_like(xd), torch.empty_like(cd)
    oo = torch.empty_like(od)
    x3 = torch.zeros((N_SRC, H, W, 3), dtype=torch.float32, device=DEV)
    ok = dict(x=xd, lab=cd, kind=1, Cc=0, index=None, n_src=N_SRC, params=P, n=N_SRC, h=H, w=W, border=0, x_fill=0.0,
              label_fill=0, x_out=xo, lab_out=lo)
    assert _entry(**ok) == 0
    bad = [dict(n=0), dict(h=0), dict(w=-1), dict(x=x3), dict(kind=3), dict(kind=-1), dict(kind=2, lab=od, lab_out=oo, Cc=1),
           dict(kind=2, lab=od, lab_out=oo, Cc=9), dict(lab=None), dict(lab_out=None), dict(params=None), dict(x_out=None),
           dict(n_src=N_SRC - 1),                        # index NULL needs n_src >= n
           dict(x_out=xd), dict(lab_out=cd), dict(x_out=xd[1:]), dict(lab=od, kind=2, Cc=3, lab_out=od)]
    for change in bad:
        assert _entry(**dict(ok, **change)) == 1, change
        assert b"data_augment" in _lib.load().depgan_last_error()
    assert _entry(**dict(ok, kind=0, lab=None, lab_out=None)) == 0
    assert _entry(**dict(ok, kind=2, lab=od, lab_out=oo, Cc=3)) == 0
    torch.cuda.synchronize()
    for kw in (dict(x=x[0]), dict(x=np.zeros((2, H, W, 3), np.float32)), dict(labels=codes[:, :-1]),
               dict(labels=np.zeros((N_SRC, H, W, 9), np.float32)), dict(labels=codes.astype(np.float32) + 0.5),
               dict(labels=codes.astype(np.int32) - 1), dict(index=[0, N_SRC]), dict(index=[-1]), dict(index=[0.5]),
               dict(params=np.zeros((3, 8), np.float32)), dict(params=np.zeros((N_SRC, 7), np.float32)),
               dict(border="wrap"), dict(labels=codes, label_fill=256), dict(labels=onehot, label_fill=3),
               dict(label_fill=1.5)):
        with pytest.raises(ValueError):
            data.augment(**dict(dict(x=x), **kw))


# ---- GeneratorModel.fit(augment=...) at 32 x 32, batch 4, 8 slices, 2 epochs, 3 classes, sparse labels ----

def _fit_set():
    rng = np.random.default_rng(21)
    x = rng.standard_normal((8, 32, 32, 1)).astype(np.float32)
    z = rng.standard_normal((8, 32, 1)).astype(np.float32)
    codes = rng.integers(0, 3, (8, 32, 32)).astype(np.uint8)
    return x, z, codes


def _fit(augment, resident, seed=11):
    from dep_gan_im_amd import Gen_UNet2D
    x, z, codes = _fit_set()
    net = Gen_UNet2D((32, 32, 1), nc_out=3, seed=3).compile(loss="sparse_categorical_crossentropy", metrics=["dice"])
    if resident:
        x, codes = torch.from_numpy(x).to(DEV), torch.from_numpy(codes).to(DEV)
    np.random.seed(seed)
    kw = {} if augment is None else {"augment": augment}
    h = net.fit([x, z], codes, epochs=2, batch_size=4, verbose=0, **kw)
    return h.history, net.get_weights_dict()


def _same(a, b):
    (ha, wa), (hb, wb) = a, b
    return ha == hb and sorted(wa) == sorted(wb) and all(np.array_equal(_u32(wa[k]), _u32(wb[k])) for k in wa)


@pytest.fixture(scope="module")
def plain_fit():
    return _fit(None, resident=False)


def test_fit_with_identity_augmenter_on_the_resident_set_equals_plain_fit(plain_fit):
    """The fused gather (index = the epoch's order) and the unchanged default path together: history and every
    weight, bit for bit."""
    got = _fit(data.Augmenter(), resident=True)
    assert sorted(got[0]) == ["dice", "loss"] and len(got[0]["loss"]) == 2 and np.isfinite(got[0]["loss"]).all()
    assert _same(got, plain_fit)
    assert _same(_fit(data.Augmenter(), resident=False), plain_fit)   # host arrays: sliced, uploaded, augmented


def test_fit_with_augmentation_repeats_and_differs_from_plain_fit(plain_fit):
    a = _fit(data.Augmenter(flip_lr=True, rotate=10, seed=1), resident=True)
    b = _fit(data.Augmenter(flip_lr=True, rotate=10, seed=1), resident=True)
    assert np.isfinite(a[0]["loss"]).all() and _same(a, b)
    assert a[0]["loss"] != plain_fit[0]["loss"] and not _same(a, plain_fit)
    with pytest.raises(TypeError):
        _fit(lambda *args: args, resident=True)
