"""CPU: the host side of the connected components -- the NumPy restatement (tests/ccl_ref.py) against scipy where it is
importable, the lesion algebra on hand-made cases, the argument checks of evaluate.connected_components /
component_sizes / remove_small_components / lesion_detection / label_lesion_metrics, and the C ABI entries."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ccl_cases as K  # noqa: E402
import ccl_ref as R  # noqa: E402

from dep_gan_im_amd import _lib, build, evaluate  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"depgan_eval_cc_scratch_bytes": 3, "depgan_eval_cc_label": 10, "depgan_eval_cc_overlap": 7}


def test_neighbourhood_sizes():
    assert [len(R.offsets(c, p)) for c, p in K.NEIGHBOURHOODS] == [6, 18, 26, 4, 8]
    assert R.offsets(3, 1) == R.offsets(2, 1)
    for bad in ((0, 0), (4, 0), (1, 2)):
        with pytest.raises(ValueError):
            R.offsets(*bad)


@pytest.mark.parametrize("shape", K.SMALL_SHAPES)
def test_reference_against_scipy(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name in K.CONTENTS:
        a = K.volume(shape, name)
        for c, in_plane in K.NEIGHBOURHOODS:
            got, n = R.label(a, c, in_plane)
            assert got.dtype == np.int32 and got.shape == shape
            if not in_plane:
                want, nw = ndimage.label(a, ndimage.generate_binary_structure(3, c))
            else:                                    # per slice, each slice's numbers after those of the slices before
                want, nw = np.zeros(shape, np.int32), 0
                for z in range(shape[0]):
                    lab, k = ndimage.label(a[z], ndimage.generate_binary_structure(2, c))
                    want[z] = np.where(lab > 0, lab + nw, 0)
                    nw += k
            assert n == nw, (name, c, in_plane)
            np.testing.assert_array_equal(got, want, err_msg="%s %d %d" % (name, c, in_plane))


def test_contents_are_the_cases_they_claim_to_be():
    shape = (5, 37, 70)
    count = lambda name, c, p: R.label(K.volume(shape, name), c, p)[1]      # noqa: E731
    assert count("empty", 1, 0) == 0 and count("full", 1, 0) == 1 and count("corners", 3, 0) == 2
    assert count("checker", 1, 0) == K.volume(shape, "checker").sum() and count("checker", 3, 0) == 1
    assert count("checker", 2, 0) == 1 and count("checker", 2, 1) == 5       # joined through the edge neighbours
    assert [count("diag_plane", c, p) for c, p in K.NEIGHBOURHOODS] == [37, 1, 1, 37, 1]
    assert [count("diag_volume", c, p) for c, p in K.NEIGHBOURHOODS] == [5, 5, 1, 5, 5]
    assert [count("serpentine", c, p) for c, p in K.NEIGHBOURHOODS] == [1, 1, 1, 5, 5]
    assert count("u", 1, 1) == 5 and count("comb", 1, 1) == 5 and count("comb_mirror", 1, 1) == 5
    assert [count("spirals", c, p) for c, p in K.NEIGHBOURHOODS] == [2, 2, 2, 10, 10]
    assert [count("slabs", c, p) for c, p in K.NEIGHBOURHOODS] == [1, 1, 1, 5, 5]
    lab, n = R.label(K.volume(shape, "comb"), 1, 1)
    assert (lab[0, :, ::3] == 1).all() and (lab[0, -1] == 1).all()          # every tooth carries the first tooth's number
    blobs = K.volume(K.BLOBS, "blobs")
    assert 0.02 < blobs.mean() < 0.5 and R.label(blobs, 3, 0)[1] > 3


def test_sizes_hits_and_remove_small():
    a = K.volume((5, 37, 70), "random_0.25")
    other = K.volume((5, 37, 70), "random_0.31")
    lab, n = R.label(a, 1, 0)
    size, hits = R.sizes_hits(lab, n, other)
    assert size.sum() == a.sum() and hits.sum() == (a & other).sum() and (hits <= size).all() and size.min() >= 1
    assert [int(size[k - 1]) for k in (1, n)] == [int((lab == 1).sum()), int((lab == n).sum())]
    assert not R.sizes_hits(lab, n)[1].any()
    np.testing.assert_array_equal(R.remove_small(a * 3.5, 1), a.astype(np.uint8))
    big = R.remove_small(a, 5)
    assert big.dtype == np.uint8 and (big <= a).all()
    assert big.sum() == size[size >= 5].sum() and R.sizes_hits(*R.label(big, 1, 0))[0].min() >= 5


def grid(*boxes):
    a = np.zeros((2, 8, 12), bool)
    for z, y0, y1, x0, x1 in boxes:
        a[z, y0:y1, x0:x1] = True
    return a


def test_lesion_algebra_of_the_reference():
    # one truth lesion touched by two predicted ones, and a third predicted lesion that touches nothing
    truth = grid((0, 1, 4, 1, 9))
    pred = grid((0, 2, 3, 0, 3), (0, 3, 6, 7, 9), (1, 6, 8, 10, 12))
    m = R.lesion_detection(pred, truth, connectivity=1, in_plane=True)
    assert tuple(m)[:len(R.KEYS)] == R.KEYS
    assert (m["n_truth"], m["n_pred"], m["n_truth_detected"], m["n_pred_true"]) == (1, 3, 1, 2)
    assert m["recall"] == 1.0 and m["precision"] == 2 / 3 and m["f1"] == 2 * (2 / 3) * 1.0 / (2 / 3 + 1.0)
    assert (m["voxels_truth"], m["voxels_pred"]) == (24, 3 + 6 + 4) and m["avd_percent"] == 100.0 * 11 / 24
    assert list(m["sizes_truth"]) == [24] and list(m["sizes_pred"]) == [3, 6, 4]
    # one predicted lesion bridging two truth lesions: both detected, the one prediction true
    truth = grid((0, 1, 3, 1, 3), (0, 1, 3, 8, 10), (1, 0, 1, 0, 1))
    pred = grid((0, 2, 3, 2, 9))
    m = R.lesion_detection(pred, truth, connectivity=1)
    assert (m["n_truth"], m["n_pred"], m["n_truth_detected"], m["n_pred_true"]) == (3, 1, 2, 1)
    assert m["recall"] == 2 / 3 and m["precision"] == 1.0
    # min_voxels clears the single truth voxel before anything else; sizes in the unit of voxel_volume
    m = R.lesion_detection(pred, truth, connectivity=1, min_voxels=2, voxel_volume=0.5)
    assert (m["n_truth"], m["n_truth_detected"], m["recall"], m["voxels_truth"]) == (2, 2, 1.0, 8)
    assert list(m["sizes_truth"]) == [2.0, 2.0] and m["sizes_pred"].dtype == np.float64
    # a prediction that lives only on a removed truth lesion is no longer true
    m = R.lesion_detection(grid((1, 0, 2, 0, 2)), truth, connectivity=1, min_voxels=2)
    assert (m["n_pred"], m["n_pred_true"], m["precision"], m["recall"], m["f1"]) == (1, 0, 0.0, 0.0, 0.0)
    # the empty cases: nan where a denominator is 0, and the counts say why
    none = np.zeros_like(truth)
    m = R.lesion_detection(none, truth)
    assert (m["n_truth"], m["n_pred"]) == (2, 0) and m["recall"] == 0.0      # rank 3 joins (1, 0, 0) to (0, 1, 1)
    assert math.isnan(m["precision"]) and math.isnan(m["f1"]) and m["avd_percent"] == 100.0
    m = R.lesion_detection(pred, none)
    assert (m["n_truth"], m["n_pred"], m["precision"]) == (0, 1, 0.0)
    assert math.isnan(m["recall"]) and math.isnan(m["f1"]) and math.isnan(m["avd_percent"])
    m = R.lesion_detection(none, none)
    assert all(math.isnan(m[k]) for k in ("recall", "precision", "f1", "avd_percent"))
    assert all(m[k] == 0 for k in R.KEYS[:4] + ("voxels_truth", "voxels_pred")) and len(m["sizes_truth"]) == 0
    same = R.lesion_detection(truth, truth)
    assert same["recall"] == same["precision"] == same["f1"] == 1.0 and same["avd_percent"] == 0.0
    assert evaluate.LESION_KEYS == R.KEYS


Z = np.zeros((2, 5, 6), np.uint8)


def no_device():
    raise AssertionError("the library was loaded before the arguments were checked")


@pytest.mark.parametrize("kw", [dict(truth=np.zeros((2, 5, 7), np.uint8)), dict(pred=np.zeros((5, 6)), truth=np.zeros((5, 6))),
                                dict(pred=np.zeros((1, 2, 5, 6)), truth=np.zeros((1, 2, 5, 6))),
                                dict(connectivity=0), dict(connectivity=4), dict(connectivity=1.5),
                                dict(connectivity=None), dict(connectivity=True), dict(in_plane=2), dict(in_plane=None),
                                dict(in_plane="yes"), dict(min_voxels=2.5), dict(min_voxels=None), dict(min_voxels="3"),
                                dict(min_voxels=float("nan")), dict(voxel_volume=0), dict(voxel_volume=-1.0),
                                dict(voxel_volume=float("inf")), dict(voxel_volume=float("nan")),
                                dict(voxel_volume="abc")])
def test_lesion_detection_refuses_bad_arguments_before_any_device_call(kw, monkeypatch):
    monkeypatch.setattr(_lib, "load", no_device)
    args = dict(pred=Z, truth=Z)
    args.update(kw)
    with pytest.raises(ValueError):
        evaluate.lesion_detection(**args)


def test_the_other_functions_refuse_bad_arguments(monkeypatch):
    monkeypatch.setattr(_lib, "load", no_device)
    for kw in (dict(mask=np.zeros((5, 6))), dict(mask=Z, connectivity=0), dict(mask=Z, connectivity=4),
               dict(mask=Z, in_plane=2)):
        with pytest.raises(ValueError):
            evaluate.connected_components(**kw)
    for kw in (dict(mask=np.zeros((5, 6)), min_voxels=2), dict(mask=Z, min_voxels=2.5), dict(mask=Z, min_voxels=None),
               dict(mask=Z, min_voxels=2, connectivity=5), dict(mask=Z, min_voxels=2, in_plane=-1)):
        with pytest.raises(ValueError):
            evaluate.remove_small_components(**kw)
    lab = np.zeros((2, 5, 6), np.int32)
    for kw in (dict(labels=np.zeros((5, 6), np.int32), n=0), dict(labels=lab, n=-1), dict(labels=lab, n=61),
               dict(labels=lab, n=1.5), dict(labels=lab, n=None), dict(labels=lab, n=1, other=np.zeros((2, 5, 7))),
               dict(labels=lab, n=1, other=np.zeros((5, 6)))):
        with pytest.raises(ValueError):
            evaluate.component_sizes(**kw)
    labels, real = np.zeros((2, 5, 6), np.int8), np.zeros((2, 5, 6, 1), np.float32)
    for kw in (dict(classes=()), dict(code_real=np.zeros((2, 5, 7), np.float32)), dict(labels=np.zeros((5, 6), np.int8)),
               dict(mask=np.ones((2, 5, 5), np.float32)), dict(connectivity=0), dict(in_plane=3), dict(min_voxels=1.5),
               dict(voxel_volume=0.0), dict(spacing=(1, 1, 1))):
        args = dict(labels=labels, code_real=real)
        args.update(kw)
        with pytest.raises(ValueError):
            evaluate.label_lesion_metrics(**args)


def test_entry_points_are_declared_bound_and_built(lib):
    """`lib` builds the library for gfx950 with the new source and loads it."""
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "components.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "components.hip"))
    for name, count in NEW_SYMBOLS.items():
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        params = re.findall(r"\b%s\s*\(([^()]*)\)\s*;" % name, stripped)
        assert len(params) == 1 and params[0].count(",") + 1 == count, name
        assert len(_lib._HDR.prototypes[name][1]) == count == len(getattr(lib, name).argtypes), name
    assert lib.depgan_eval_cc_scratch_bytes.restype is C.c_size_t
    assert lib.depgan_eval_cc_overlap.argtypes[2:4] == [C.c_long, C.c_int]
    assert lib.depgan_abi_version() == 3 == _lib.ABI_VERSION


def test_host_only_entries_and_refusals_without_a_device(lib):
    """The scratch size and every status-1 refusal are host code: nothing is launched, so no GPU is needed."""
    assert lib.depgan_eval_cc_scratch_bytes(3, 4, 5) >= 60 * 4 + 4 + 8
    assert lib.depgan_eval_cc_scratch_bytes(3, 4, 5) % 8 == 0
    assert lib.depgan_eval_cc_scratch_bytes(0, 4, 5) == 0 == lib.depgan_eval_cc_scratch_bytes(1, 4097, 5)
    assert lib.depgan_eval_cc_scratch_bytes(3, 4, -1) == 0
    assert lib.depgan_eval_cc_scratch_bytes(2048, 1024, 1024) == 0           # D*H*W = 2^31
    assert lib.depgan_eval_cc_scratch_bytes(2047, 1024, 1024) > 0
    p = [C.c_void_p(65536 * k) for k in range(1, 6)]       # never dereferenced: every call below is refused
    out = (C.c_longlong * 1)(-7)
    label, overlap = lib.depgan_eval_cc_label, lib.depgan_eval_cc_overlap
    refused = [
        label(p[0], 0, 4, 4, 1, 0, p[1], p[2], out, None),
        label(p[0], 2, 4097, 4, 1, 0, p[1], p[2], out, None),
        label(p[0], 2, 4, -3, 1, 0, p[1], p[2], out, None),
        label(p[0], 2048, 1024, 1024, 1, 0, p[1], p[2], out, None),
        label(None, 2, 4, 4, 1, 0, p[1], p[2], out, None),
        label(p[0], 2, 4, 4, 1, 0, None, p[2], out, None),
        label(p[0], 2, 4, 4, 1, 0, p[1], None, out, None),
        label(p[0], 2, 4, 4, 1, 0, p[1], p[2], None, None),
        label(p[0], 2, 4, 4, 0, 0, p[1], p[2], out, None),
        label(p[0], 2, 4, 4, 4, 0, p[1], p[2], out, None),
        label(p[0], 2, 4, 4, 1, 2, p[1], p[2], out, None),
        label(p[0], 2, 4, 4, 1, -1, p[1], p[2], out, None),
        label(p[0], 2, 4, 4, 1, 0, C.c_void_p(2 * 65536 + 2), p[2], out, None),      # labels misaligned
        label(p[0], 2, 4, 4, 1, 0, p[1], C.c_void_p(3 * 65536 + 4), out, None),      # scratch misaligned
        label(p[0], 2, 4, 4, 1, 0, C.c_void_p(65536 + 28), p[2], out, None),         # labels over set
        label(p[0], 2, 4, 4, 1, 0, p[1], C.c_void_p(2 * 65536 + 64), out, None),     # scratch over labels
        label(p[0], 2, 4, 4, 1, 0, p[1], C.c_void_p(65536 - 8), out, None),          # scratch over set
        overlap(p[0], p[1], 0, 1, p[2], p[3], None),
        overlap(p[0], p[1], 1 << 31, 1, p[2], p[3], None),
        overlap(p[0], p[1], 32, -1, p[2], p[3], None),
        overlap(p[0], p[1], 32, 33, p[2], p[3], None),
        overlap(None, p[1], 32, 1, p[2], p[3], None),
        overlap(p[0], p[1], 32, 1, None, p[3], None),
        overlap(p[0], p[1], 32, 1, p[2], None, None),
        overlap(C.c_void_p(65536 + 1), p[1], 32, 1, p[2], p[3], None),               # labels misaligned
        overlap(p[0], p[1], 32, 1, C.c_void_p(3 * 65536 + 2), p[3], None),           # size misaligned
        overlap(p[0], p[1], 32, 4, p[2], C.c_void_p(3 * 65536 + 8), None),           # hits over size
        overlap(p[0], p[1], 32, 4, C.c_void_p(65536 + 64), p[3], None),              # size over labels
        overlap(p[0], p[1], 32, 4, p[2], C.c_void_p(2 * 65536 + 16), None),          # hits over other
    ]
    assert refused == [1] * len(refused)
    assert b"eval_cc_overlap" in lib.depgan_last_error()
    assert out[0] == -7
    # n_comp = 0 is allowed and launches nothing, with or without tables
    assert overlap(p[0], None, 32, 0, None, None, None) == 0 == overlap(p[0], p[1], 32, 0, p[2], p[3], None)
