"""CPU: the host side of the surface distances -- the NumPy restatement (tests/surface_ref.py) against itself and,
where scipy is importable, against scipy; data.prepared_spacing against data_prep; the argument checks of
evaluate.distance_transform / surface_distances / label_surface_metrics; the C ABI entries."""
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_ref as R  # noqa: E402

from dep_gan_im_amd import _lib, build, data, evaluate  # noqa: E402
from oracle import data_oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACINGS = [(1, 1, 1), (3, 0.9375, 0.9375), (2.7, 0.977, 1.013)]
SHAPES = [(1, 1, 1), (1, 9, 70), (5, 37, 70), (3, 3, 300), (3, 300, 3), (70, 5, 9)]
NEW_SYMBOLS = {"depgan_eval_surface_mask": 7, "depgan_eval_edt_scratch_bytes": 3, "depgan_eval_edt_sq": 10,
               "depgan_eval_surface_sums_scratch_bytes": 1, "depgan_eval_surface_sums": 6}


def contents(shape, seed=0):
    """the kinds of volume the GPU test uses: name -> bool (D, H, W)"""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    corners = np.zeros(shape, bool)
    corners[0, 0, 0] = corners[-1, -1, -1] = True
    slab = np.zeros(shape, bool)
    slab[D // 2] = True
    return {"empty": np.zeros(shape, bool), "full": np.ones(shape, bool), "corners": corners, "slab": slab,
            "random_0.01": rng.uniform(size=shape) < 0.01, "random_0.5": rng.uniform(size=shape) < 0.5}


@functools.lru_cache(maxsize=None)
def brute(shape, name, spacing):
    """computed once, shared by the tests below, read-only"""
    out = R.edt_sq_brute(contents(shape)[name], R.weights(spacing))
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_separable_passes_give_the_bits_of_the_brute_force_minimum(shape):
    for name, a in contents(shape).items():
        for sp in SPACINGS:
            w = R.weights(sp)
            want = brute(shape, name, sp)
            assert want.dtype == np.float64 and want.shape == shape
            np.testing.assert_array_equal(R.edt_sq_separable(a, w), want, err_msg="%s %s" % (name, sp))
            if not a.any():
                assert np.isinf(want).all()
            else:
                assert not want[a].any() and (want[~a] > 0).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_against_scipy(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    six = ndimage.generate_binary_structure(3, 1)
    for name, a in contents(shape).items():
        eroded = ndimage.binary_erosion(a, six, border_value=0)
        np.testing.assert_array_equal(R.surface_mask(a, False), (a & ~eroded).astype(np.uint8), err_msg=name)
        planes = np.stack([ndimage.binary_erosion(s, six[1], border_value=0) for s in a])
        np.testing.assert_array_equal(R.surface_mask(a, True), (a & ~planes).astype(np.uint8), err_msg=name)
        if not a.any():
            continue
        for sp in SPACINGS:
            want = ndimage.distance_transform_edt(~a, sampling=sp)
            got = np.sqrt(brute(shape, name, sp))
            assert (np.abs(got - want) <= 2 * np.spacing(np.maximum(got, want))).all(), (name, sp)


def test_metric_algebra_of_the_reference():
    a = np.zeros((3, 9, 9), bool)
    b = np.zeros((3, 9, 9), bool)
    a[1, 2:5, 2:5] = True                       # a 3 x 3 plate: 8 in-plane surface voxels, 9 in the volume
    b[1, 2:5, 4:7] = True                       # the same plate two columns to the right
    m = R.surface_distances(a, b, spacing=(5, 1, 2), in_plane=True)
    assert (m["n_surface_a"], m["n_surface_b"]) == (8, 8)
    assert m["hd_ab"] == m["hd_ba"] == m["hd"] == 4.0 and m["hd95"] == max(m["hd95_ab"], m["hd95_ba"])
    assert m["assd"] == (m["msd_ab"] + m["msd_ba"]) / 2 and 0 < m["msd_ab"] < 4
    assert R.surface_distances(a, b, in_plane=False)["n_surface_a"] == 9
    same = R.surface_distances(a, a)
    assert all(same[k] == 0.0 for k in R.KEYS if not k.startswith("n_"))
    none = R.surface_distances(a, np.zeros_like(a))
    assert none["n_surface_b"] == 0 and all(np.isnan(none[k]) for k in R.KEYS if not k.startswith("n_"))
    assert evaluate.SURFACE_KEYS == R.KEYS


def test_percentile_statement_is_numpys():
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 7, 20, 101, 1000):
        v = np.sort(rng.uniform(size=n))
        for q in (0, 5, 33.3, 50, 95, 95.0, 99.9, 100):
            lo, hi, t = evaluate._percentile_index(n, q)
            assert evaluate._lerp(v[lo], v[hi], t) == np.percentile(v, q), (n, q)


def test_prepared_spacing_follows_data_prep():
    vol = np.zeros((5, 6, 7), np.float32)                # three different dimensions, file order (X, Y, Z)
    prepared = data.data_prep(vol)
    np.testing.assert_array_equal(prepared, data_oracle.data_prep(vol))
    rng = np.random.default_rng(0)
    v = rng.standard_normal((5, 6, 7)).astype(np.float32)
    np.testing.assert_array_equal(data.data_prep(v), data_oracle.data_prep(v))
    pixdim = (0.9375, 0.977, 3.0)                        # spacing along X, Y, Z
    extent = {n: n * p for n, p in zip(vol.shape, pixdim)}
    sz, sy, sx = data.prepared_spacing(pixdim)
    # the physical extent of every prepared axis is the extent of the file axis it came from
    assert [n * s for n, s in zip(prepared.shape[:3], (sz, sy, sx))] == [extent[n] for n in prepared.shape[:3]]
    assert (sz, sy, sx) == (3.0, 0.9375, 0.977)
    # ... and the way back is the same permutation
    assert data.data_prep_save(prepared).shape == vol.shape
    for bad in ((1, 1), (1, 0, 1), (1, np.nan, 1), (1, 2, 3, 4)):
        with pytest.raises(ValueError):
            data.prepared_spacing(bad)


Z = np.zeros((2, 5, 6), np.uint8)


@pytest.mark.parametrize("kw", [dict(b=np.zeros((2, 5, 7), np.uint8)), dict(a=np.zeros((5, 6)), b=np.zeros((5, 6))),
                                dict(a=np.zeros((1, 2, 5, 6)), b=np.zeros((1, 2, 5, 6))), dict(spacing=(1, 1)),
                                dict(spacing=(1, 0, 1)), dict(spacing=(1, -2, 1)), dict(spacing=(1, np.inf, 1)),
                                dict(spacing=(np.nan, 1, 1)), dict(spacing=(1e200, 1, 1)), dict(spacing="abc"),
                                dict(percentile=100.5), dict(percentile=-1), dict(percentile=np.nan)])
def test_surface_distances_refuses_bad_arguments_before_any_device_call(kw, monkeypatch):
    def no_device():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_device)
    args = dict(a=Z, b=Z)
    args.update(kw)
    with pytest.raises(ValueError):
        evaluate.surface_distances(**args)


def test_distance_transform_and_label_metrics_refuse_bad_arguments(monkeypatch):
    def no_device():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_device)
    for kw in (dict(mask=np.zeros((5, 6))), dict(mask=Z, spacing=(1, 1, 0)), dict(mask=Z, spacing=(1, 1))):
        with pytest.raises(ValueError):
            evaluate.distance_transform(**kw)
    lab, real = np.zeros((2, 5, 6), np.int8), np.zeros((2, 5, 6, 1), np.float32)
    for kw in (dict(classes=()), dict(spacing=(0, 1, 1)), dict(code_real=np.zeros((2, 5, 7), np.float32)),
               dict(labels=np.zeros((5, 6), np.int8)), dict(mask=np.ones((2, 5, 5), np.float32))):
        args = dict(labels=lab, code_real=real)
        args.update(kw)
        with pytest.raises(ValueError):
            evaluate.label_surface_metrics(**args)


def test_entry_points_are_declared_bound_and_built(lib):
    """`lib` builds the library for gfx950 with the new source and loads it."""
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "surface_dist.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "surface_dist.hip"))
    for name, count in NEW_SYMBOLS.items():
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        params = re.findall(r"\b%s\s*\(([^()]*)\)\s*;" % name, stripped)
        assert len(params) == 1 and params[0].count(",") + 1 == count, name
        assert len(_lib._HDR.prototypes[name][1]) == count == len(getattr(lib, name).argtypes), name
    import ctypes as C
    assert lib.depgan_eval_edt_scratch_bytes.restype is C.c_size_t
    assert lib.depgan_eval_edt_sq.argtypes[4:7] == [C.c_double] * 3


def test_host_only_entries_and_refusals_without_a_device(lib):
    """The scratch sizes and every status-1 refusal are host code: nothing is launched, so no GPU is needed."""
    import ctypes as C
    assert lib.depgan_eval_edt_scratch_bytes(3, 4, 5) >= 60 * 8 + 60 * 2
    assert lib.depgan_eval_edt_scratch_bytes(0, 4, 5) == 0 and lib.depgan_eval_edt_scratch_bytes(1, 4097, 5) == 0
    assert lib.depgan_eval_edt_scratch_bytes(2048, 1024, 1024) == 0          # D*H*W = 2^31
    assert lib.depgan_eval_surface_sums_scratch_bytes(1) == 2 * 4 * 8
    assert lib.depgan_eval_surface_sums_scratch_bytes(0) == 0 == lib.depgan_eval_surface_sums_scratch_bytes(1 << 31)
    p = [C.c_void_p(4096 * k) for k in range(1, 5)]       # never dereferenced: every call below is refused
    out = (C.c_double * 4)()
    one = (1.0, 1.0, 1.0)
    refused = [
        lib.depgan_eval_surface_mask(p[0], 0, 4, 4, 0, p[1], None),
        lib.depgan_eval_surface_mask(p[0], 2, 4097, 4, 0, p[1], None),
        lib.depgan_eval_surface_mask(p[0], 2048, 1024, 1024, 0, p[1], None),
        lib.depgan_eval_surface_mask(None, 2, 4, 4, 0, p[1], None),
        lib.depgan_eval_surface_mask(p[0], 2, 4, 4, 0, None, None),
        lib.depgan_eval_surface_mask(p[0], 2, 4, 4, 2, p[1], None),
        lib.depgan_eval_surface_mask(p[0], 2, 4, 4, 0, C.c_void_p(4096 + 31), None),      # surf inside set
        lib.depgan_eval_edt_sq(p[0], 2, 4, 0, *one, p[1], p[2], None),
        lib.depgan_eval_edt_sq(p[0], 4097, 4, 4, *one, p[1], p[2], None),
        lib.depgan_eval_edt_sq(None, 2, 4, 4, *one, p[1], p[2], None),
        lib.depgan_eval_edt_sq(p[0], 2, 4, 4, *one, None, p[2], None),
        lib.depgan_eval_edt_sq(p[0], 2, 4, 4, *one, p[1], None, None),
        lib.depgan_eval_edt_sq(p[0], 2, 4, 4, 0.0, 1.0, 1.0, p[1], p[2], None),
        lib.depgan_eval_edt_sq(p[0], 2, 4, 4, 1.0, -1.0, 1.0, p[1], p[2], None),
        lib.depgan_eval_edt_sq(p[0], 2, 4, 4, 1.0, 1.0, float("inf"), p[1], p[2], None),
        lib.depgan_eval_edt_sq(p[0], 2, 4, 4, float("nan"), 1.0, 1.0, p[1], p[2], None),
        lib.depgan_eval_edt_sq(p[0], 2, 4, 4, *one, C.c_void_p(4096 + 24), p[2], None),   # d2 over set
        lib.depgan_eval_edt_sq(p[0], 2, 4, 4, *one, p[1], C.c_void_p(8192 + 8), None),    # scratch over d2
        lib.depgan_eval_surface_sums(p[0], p[1], 0, p[2], out, None),
        lib.depgan_eval_surface_sums(p[0], p[1], 1 << 31, p[2], out, None),
        lib.depgan_eval_surface_sums(None, p[1], 32, p[2], out, None),
        lib.depgan_eval_surface_sums(p[0], None, 32, p[2], out, None),
        lib.depgan_eval_surface_sums(p[0], p[1], 32, None, out, None),
        lib.depgan_eval_surface_sums(p[0], p[1], 32, p[2], None, None),
        lib.depgan_eval_surface_sums(p[0], p[1], 32, C.c_void_p(4096 + 64), out, None),   # partial over d2
    ]
    assert refused == [1] * len(refused)
    assert b"eval_surface_sums" in lib.depgan_last_error()
