"""GPU: elastic deformation and bias field in the augmentation launch -- depgan_data_augment_fields through the C entry,
data.augment(fields=...), data.Augmenter(elastic=..., bias=...) and GeneratorModel.fit.

The kernel shares the four collapsed control rows of a block through LDS when the block's 256 pixels lie in one image
row, and evaluates per lane otherwise; both must give the bits of the NumPy restatement tests/elastic_ref.py.  The
shapes sit where the paths differ: 5 x 7 with 3 samples (105 pixels: one block spans the samples), 16 x 256 (every
block is one row), 3 x 512 (two blocks per row), 9 x 300 (blocks span rows; 2700 pixels, the last block partly empty)
and 1 x 1; the grids 4 x 4, 4 x 32, 32 x 4 and 7 x 7 are the smallest, the widest along each axis and the default.
Images are compared as uint32 bit patterns, labels for equality.  The inputs hold no subnormals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_augment as TA  # noqa: E402  (its fit helpers: the same model, set and manner)
from elastic_ref import elastic_ref  # noqa: E402
from dep_gan_im_amd import _lib, data, evaluate  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_SRC = 4
GRIDS = [(4, 4), (4, 32), (32, 4), (7, 7)]


def _u32(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _set(seed, h, w, nicg, Cc):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N_SRC, h, w, nicg)).astype(np.float32)
    assert np.all(np.abs(x) >= np.finfo(np.float32).tiny)
    codes = rng.integers(0, Cc, (N_SRC, h, w)).astype(np.uint8)
    return x, codes, np.eye(Cc, dtype=np.float32)[codes]


def _rows(seed, n, h, w):
    return data.Augmenter(rotate=25, scale=(0.7, 1.4), shift=3, flip_lr=True, flip_ud=True, gain=(0.5, 1.5),
                          offset=(-1.0, 1.0), seed=seed).draw(n, h, w)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _entry(x, lab, kind, Cc, index, n_src, params, fields, gh, gw, n, h, w, border, x_fill, label_fill, x_out, lab_out,
           dense):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _lib.load().depgan_data_augment_fields(_p(x), x.shape[3], _p(lab), kind, Cc, _p(index), n_src, _p(params),
                                                  _p(fields), gh, gw, n, h, w, border, x_fill, label_fill, _p(x_out),
                                                  _p(lab_out), _p(dense), st)


# ---- 1. zero fields against depgan_data_augment, bit for bit ----

@pytest.mark.parametrize("nicg", [1, 2])
@pytest.mark.parametrize("kind,Cc", [(0, 0), (1, 3), (2, 2), (2, 4), (2, 8)])
def test_zero_fields_give_the_bits_of_the_affine_entry(nicg, kind, Cc):
    """through the C entries themselves, with a device index that repeats a slice and leaves the set on both sides;
    37 x 53 evaluates per lane, 4 x 256 through LDS"""
    lib = _lib.load()
    for h, w in ((37, 53), (4, 256)):
        x, codes, onehot = _set(7 * nicg + Cc, h, w, nicg, Cc if kind == 2 else 3)
        xd = torch.from_numpy(x).to(DEV)
        ld = None if kind == 0 else torch.from_numpy(codes if kind == 1 else onehot).to(DEV)
        idx = torch.tensor([2, 0, -1, 2, N_SRC, 3], dtype=torch.int64, device=DEV)
        n = idx.numel()
        P = torch.from_numpy(_rows(11, n, h, w)).to(DEV)
        Z = torch.zeros((n, 3, 5, 9), dtype=torch.float32, device=DEV)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for border in (0, 1):
            fill = (0, 7, -1 if border else 1)[kind]
            lshape = {0: None, 1: (n, h, w), 2: (n, h, w, Cc)}[kind]
            outs = []
            for fields in (False, True):
                xo = torch.full((n, h, w, nicg), np.nan, dtype=torch.float32, device=DEV)
                lo = None if kind == 0 else torch.full(lshape, 77, dtype=ld.dtype, device=DEV)
                if fields:
                    rc = _entry(xd, ld, kind, Cc, idx, N_SRC, P, Z, 5, 9, n, h, w, border, -2.5, fill, xo, lo, None)
                else:
                    rc = lib.depgan_data_augment(_p(xd), nicg, _p(ld), kind, Cc, _p(idx), N_SRC, _p(P), n, h, w, border,
                                                 -2.5, fill, _p(xo), _p(lo), st)
                assert rc == 0, lib.depgan_last_error()
                torch.cuda.synchronize()
                outs.append((xo, lo))
            (xa, la), (xf, lf) = outs
            assert not np.isnan(_np(xa)).any() and np.all(_np(xa[2]) == -2.5) and np.all(_np(xa[4]) == -2.5)
            assert np.array_equal(_u32(xf), _u32(xa)), (h, w, border)
            if kind == 1:
                assert np.array_equal(_np(lf), _np(la)) and np.all(_np(la[2]) == 7)
            if kind == 2:
                assert np.array_equal(_u32(lf), _u32(la)), (h, w, border)


# ---- 2. random rows and fields against the restatement, bit for bit ----

def _fields(seed, n, gh, gw, h, w):
    """displacements up to 0.6 of the image (at least 3 px), so part of every sample comes from outside; bias +-0.5"""
    rng = np.random.default_rng(seed)
    amp = np.array([max(3.0, 0.6 * h), max(3.0, 0.6 * w), 0.5])[None, :, None, None]
    return (rng.uniform(-1, 1, (n, 3, gh, gw)) * amp).astype(np.float32)


@pytest.mark.parametrize("h,w", [(5, 7), (16, 256), (3, 512), (9, 300), (1, 1)])
def test_random_fields_match_the_float32_restatement_bit_for_bit(h, w):
    index = [3, 0, 3]
    k = 0
    for gh, gw in GRIDS:
        for border, x_fill in (("edge", 0.75), ("constant", -7.0)):
            nicg, kind = 1 + k % 2, ("codes", "onehot", "none")[k % 3]
            x, codes, onehot = _set(100 + k, h, w, nicg, 3)
            labels = {"codes": codes, "onehot": onehot, "none": None}[kind]
            label_fill = {"codes": 9, "onehot": (-1, 2)[k % 2], "none": 0}[kind]
            P, F = _rows(200 + k, 3, h, w), _fields(300 + k, 3, gh, gw, h, w)
            out, lab, dense = data.augment(x, labels, P, index, border, x_fill, label_fill, fields=F, return_fields=True)
            want, wlab, wdense = elastic_ref(x, labels, P, F, index, border, x_fill, label_fill)
            assert want.dtype == np.float32 and tuple(dense.shape) == (3, h, w, 3)
            where = (h, w, gh, gw, border)
            assert np.array_equal(_u32(dense), _u32(wdense)), where
            assert np.array_equal(_u32(out), _u32(want)), where
            if kind == "codes":
                assert np.array_equal(_np(lab), wlab), where
                if border == "constant" and h * w > 1:
                    assert (wlab == 9).any(), where                      # the displacement did leave the image
            elif kind == "onehot":
                assert np.array_equal(_u32(lab), _u32(wlab)), where
            else:
                assert lab is None
            k += 1


def test_one_grid_for_all_samples_and_device_tensors():
    h, w = 6, 256
    x, codes, _ = _set(5, h, w, 1, 3)
    F = _fields(6, 1, 7, 7, h, w)[0]
    P = _rows(7, N_SRC, h, w)
    out, lab = data.augment(torch.from_numpy(x).to(DEV), torch.from_numpy(codes).to(DEV), P,
                            fields=torch.from_numpy(F).to(DEV))
    want, wlab, _ = elastic_ref(x, codes, P, np.broadcast_to(F, (N_SRC,) + F.shape))
    assert np.array_equal(_u32(out), _u32(want)) and np.array_equal(_np(lab), wlab)
    # the index a tensor on the device, a grid per output sample
    idx, F5 = [2, 2, 0, 3, 1], _fields(8, 5, 7, 7, h, w)
    out, lab = data.augment(torch.from_numpy(x).to(DEV), codes, _rows(7, 5, h, w), torch.tensor(idx, device=DEV), fields=F5)
    want, wlab, _ = elastic_ref(x, codes, _rows(7, 5, h, w), F5, idx)
    assert np.array_equal(_u32(out), _u32(want)) and np.array_equal(_np(lab), wlab)


# ---- 3. non-finite and huge field values: clamped as floats before they become indices ----

@pytest.mark.parametrize("h,w", [(16, 256), (9, 300)])
@pytest.mark.parametrize("border", ["edge", "constant"])
def test_non_finite_and_huge_field_values_are_clamped(h, w, border):
    x, codes, _ = _set(8, h, w, 2, 3)
    F = _fields(9, N_SRC, 12, 12, h, w) * np.float32(0.2)           # 9 x 9 cells: a control value reaches 4 x 4 of them
    rng = np.random.default_rng(10)
    for i, values in enumerate(((np.nan, 1e30, -np.inf), (np.inf, -1e30, np.nan), (1e30, -1e30, 1e30), (-np.inf, np.inf, np.nan))):
        for v in values:
            F[(i,) + tuple(rng.integers(0, s) for s in F.shape[1:])] = v
    assert np.isnan(F).any() and np.isinf(F).any()
    P = _rows(12, N_SRC, h, w)
    out, lab, dense = data.augment(x, codes, P, None, border, -7.0, 9, fields=F, return_fields=True)   # status 0
    want, wlab, wdense = elastic_ref(x, codes, P, F, None, border, -7.0, 9)
    for got, ref in ((_np(dense), wdense), (_np(out), want)):
        assert np.isnan(ref).any() and not np.isnan(ref).all()
        assert np.array_equal(np.isnan(got), np.isnan(ref))                    # a NaN by its position
        ok = ~np.isnan(ref)
        assert np.array_equal(_u32(got)[ok], _u32(ref)[ok])
    assert np.array_equal(_np(lab), wlab)
    assert set(np.unique(_np(lab))) <= ({0, 1, 2, 9} if border == "constant" else {0, 1, 2})


# ---- 4. dense_out NULL or not: the same x_out ----

def test_dense_out_does_not_change_the_image():
    for h, w in ((16, 256), (9, 300)):
        x, codes, _ = _set(13, h, w, 2, 3)
        P, F = _rows(14, N_SRC, h, w), _fields(15, N_SRC, 7, 7, h, w)
        a, la = data.augment(x, codes, P, fields=F)
        b, lb, dense = data.augment(x, codes, P, fields=F, return_fields=True)
        assert np.array_equal(_u32(a), _u32(b)) and np.array_equal(_np(la), _np(lb)) and _np(dense).any()


def test_bad_arguments():
    h, w = 9, 11
    x, codes, onehot = _set(16, h, w, 2, 3)
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(codes).to(DEV)
    P = torch.from_numpy(np.tile(TA.IDENT, (N_SRC, 1))).to(DEV)
    Fd = torch.zeros((N_SRC, 3, 4, 32), dtype=torch.float32, device=DEV)
    xo, lo = torch.empty_like(xd), torch.empty_like(cd)
    dn = torch.empty((N_SRC, h, w, 3), dtype=torch.float32, device=DEV)
    ok = dict(x=xd, lab=cd, kind=1, Cc=0, index=None, n_src=N_SRC, params=P, fields=Fd, gh=4, gw=32, n=N_SRC, h=h, w=w,
              border=0, x_fill=0.0, label_fill=0, x_out=xo, lab_out=lo, dense=dn)
    assert _entry(**ok) == 0
    assert _entry(**dict(ok, dense=None)) == 0
    torch.cuda.synchronize()
    bad = [dict(fields=None), dict(gh=3), dict(gw=33), dict(gh=0), dict(gw=-4), dict(gh=33),
           dict(n=0), dict(h=0), dict(kind=3), dict(lab=None), dict(params=None), dict(x_out=None), dict(border=2),
           dict(n_src=N_SRC - 1), dict(label_fill=256),
           dict(x_out=xd), dict(lab_out=cd), dict(dense=Fd), dict(dense=xd), dict(dense=xo), dict(x_out=dn),
           dict(x_out=Fd), dict(dense=P)]
    for change in bad:
        assert _entry(**dict(ok, **change)) == 1, change
        assert b"data_augment_fields" in _lib.load().depgan_last_error()


# ---- 5. the Python surface ----

def test_augmenter_with_fields_equals_the_restatement_on_its_own_draws():
    h, w = 20, 256
    x, codes, _ = _set(17, h, w, 1, 3)
    idx = np.array([1, 3, 3, 0, 2])
    kw = dict(rotate=10, flip_lr=True, elastic=2, bias=0.2, border="constant", x_fill=-1.0, label_fill=5)
    out, lab = data.Augmenter(seed=0, **kw)(torch.from_numpy(x).to(DEV), torch.from_numpy(codes).to(DEV), idx)
    twin = data.Augmenter(seed=0, **kw)
    P, F = twin.draw(5, h, w), twin.draw_fields(5)
    assert F.shape == (5, 3, 7, 7) and F[:, :2].any() and F[:, 2].any()
    want, wlab, _ = elastic_ref(x, codes, P, F, idx, "constant", -1.0, 5)
    assert np.array_equal(_u32(out), _u32(want)) and np.array_equal(_np(lab), wlab)
    plain, _ = data.Augmenter(seed=0, **dict(kw, elastic=0, bias=0))(x, codes, idx)
    assert not np.array_equal(_u32(plain), _u32(out))


@pytest.fixture(scope="module")
def closed_fit():
    return TA._fit(data.Augmenter(flip_lr=True, rotate=10, seed=1), resident=True)


def test_fit_with_the_new_ranges_closed_repeats_the_fit_without_them(closed_fit):
    got = TA._fit(data.Augmenter(flip_lr=True, rotate=10, seed=1, elastic=0.0, bias=0.0, field_grid=(9, 5)), resident=True)
    assert TA._same(got, closed_fit)


def test_fit_with_elastic_and_bias_runs_on_both_routes(closed_fit):
    kw = dict(flip_lr=True, rotate=10, seed=1, elastic=2, bias=0.2)
    a = TA._fit(data.Augmenter(**kw), resident=True)
    assert len(a[0]["loss"]) == 2 and np.isfinite(a[0]["loss"]).all()
    assert TA._same(a, TA._fit(data.Augmenter(**kw), resident=False))     # sliced, uploaded and augmented: the same bits
    assert a[0]["loss"] != closed_fit[0]["loss"] and not TA._same(a, closed_fit)


def test_predict_stats_refuses_an_augmenter_with_fields():
    from dep_gan_im_amd import Gen_UNet2D
    net = Gen_UNet2D((32, 32, 1), nc_out=3, seed=3)
    x = np.zeros((2, 32, 32, 1), np.float32)
    for kw in (dict(elastic=1), dict(bias=0.1)):
        with pytest.raises(ValueError, match="elastic"):
            evaluate.predict_stats(net, x, n_repeat=2, tta=data.Augmenter(**kw))
