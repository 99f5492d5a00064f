"""No GPU: the focal mode's host side -- the C ABI's declarations, exports and refusals, the float64 reference against a
plain NumPy restatement and against the loss-weight mode's reference, compile's argument validation, and that the
kernel's float64 bounds can be met in float32 with 1 - r formed directly."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dep_gan_im_amd as dg  # noqa: E402
import focal_ce_ref as F  # noqa: E402
import weighted_ce_ref as R  # noqa: E402
from dep_gan_im_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments
ENTRIES = ["depgan_uresnet_set_focal", "depgan_uresnet_get_focal", "depgan_op_softmax_ce_focal",
           "depgan_uresnet_last_label_counts"]


def test_header_declares_and_library_exports_the_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert getattr(lib, name).argtypes, name + " has no argtypes"
    assert _lib._K["DEPGAN_ABI_VERSION"] == 3 and lib.depgan_abi_version() == 3       # new entries, the same ABI
    assert lib.depgan_op_softmax_ce_focal.argtypes[6:8] == [C.c_float, C.c_float]
    assert lib.depgan_uresnet_set_focal.argtypes[1:] == [C.c_float, C.c_float]


def test_operator_entry_refuses_its_arguments_before_any_hip_call(lib):
    cnt = (C.c_longlong * 11)(*([-7] * 11))

    def ce(w=(1.0, 1.0, 1.0), n=None, ign=-1, gamma=2.0, eps=0.1, codes=FAKE, onehot=None, counts=cnt, P=64, C_=3,
           logits=FAKE):
        wa = (C.c_float * len(w))(*w) if w is not None else None
        return lib.depgan_op_softmax_ce_focal(logits, onehot, codes, wa, len(w) if n is None and w else (n or 0), ign,
                                              gamma, eps, FAKE, FAKE, FAKE, None, counts, P, C_, None)
    nan, inf = float("nan"), float("inf")
    for kw in ({"gamma": -0.5}, {"gamma": nan}, {"gamma": inf}, {"gamma": -inf}, {"eps": -0.1}, {"eps": 1.0}, {"eps": 1.5},
               {"eps": nan}, {"eps": inf}, {"w": (1.0, -1.0, 1.0)}, {"w": (1.0, nan, 1.0)}, {"w": (inf, 1.0, 1.0)},
               {"w": (0.0, 0.0, 0.0)}, {"w": (1.0, 1.0)}, {"w": (1.0, 1.0, 1.0, 1.0)}, {"ign": -2}, {"ign": 256},
               {"w": None, "ign": 256}, {"counts": None}, {"codes": None}, {"codes": FAKE, "onehot": FAKE}, {"P": 0},
               {"C_": 9, "w": (1.0,) * 9}, {"C_": 1, "w": None}, {"logits": None}):
        assert ce(**kw) == 1, kw
        assert lib.depgan_last_error(), kw
    assert list(cnt) == [-7] * 11
    assert ce(gamma=-0.5) == 1 and b"focal gamma" in lib.depgan_last_error()
    assert ce(eps=1.0) == 1 and b"label smoothing" in lib.depgan_last_error()
    assert ce(w=(1.0, -1.0, 1.0)) == 1 and b"class weight 1" in lib.depgan_last_error()
    assert ce(ign=300) == 1 and b"ignore code 300" in lib.depgan_last_error()
    # the context entries without a context
    assert lib.depgan_uresnet_set_focal(None, 2.0, 0.1) == 1
    assert lib.depgan_uresnet_get_focal(None, None, None) == 0


def test_reference_loss_equals_a_numpy_restatement_and_the_weighted_reference():
    rng = np.random.default_rng(4)
    for Cc in (2, 4, 7):
        z = (2.0 * rng.standard_normal((5, 9, Cc))).astype(np.float32)
        z[0, 0] = 60.0 * np.eye(Cc)[0]                              # both clip bounds are reached
        codes = rng.integers(0, Cc, (5, 9))
        codes[rng.uniform(size=codes.shape) < 0.3] = 255
        codes[0, 0] = 1
        t = F.onehot_rows(codes, Cc, 255)
        cw = rng.uniform(0.2, 3.0, Cc)
        cw[0] = 0.0
        p = torch.softmax(torch.from_numpy(z).double(), -1)
        tt, cwt = torch.from_numpy(t).double(), torch.from_numpy(cw)
        for gamma, eps in ((2.0, 0.1), (0.5, 0.0), (0.0, 0.25), (5.0, 0.1), (1.0, 0.0)):
            loss, den, total = F.focal_ce_t(p, tt, cwt, gamma, eps)
            want, wden, wtotal = F.focal_ce_np(p.numpy(), t, cw, gamma, eps)
            assert den == wden == int(((codes != 255) & (codes != 0)).sum())
            assert abs(float(loss) - want) <= 1e-12 * abs(want) and abs(float(total) - wtotal) <= 1e-12 * abs(wtotal)
        # gamma = 0 and eps = 0: the loss-weight mode's reference, exactly
        a, b = F.focal_ce_t(p, tt, cwt, 0.0, 0.0), R.weighted_ce_t(p, tt, cwt)
        assert float(a[0]) == float(b[0]) and a[1] == b[1] and float(a[2]) == float(b[2])
        # the focal factor (1 - r)^gamma < 1 shrinks every term
        assert 0 < float(F.focal_ce_t(p, tt, cwt, 2.0, 0.0)[2]) < float(F.focal_ce_t(p, tt, cwt, 0.5, 0.0)[2]) < float(b[2])
        # nothing left: 0.0, not NaN -- an all-zero row is not smoothed
        none, den0, _ = F.focal_ce_t(p, torch.zeros_like(p), cwt, 2.0, 0.1)
        assert float(none) == 0.0 and den0 == 0
    pr, g, total, den = F.softmax_ce_focal_ref(z.reshape(-1, Cc), t.reshape(-1, Cc), cw, 2.0, 0.1)
    assert g.shape == (45, Cc) and np.all(g[(t.reshape(-1, Cc) * cw).sum(-1) == 0] == 0) and np.abs(g.sum(-1)).max() < 1e-12


def test_compile_validates_focal_gamma_and_label_smoothing():
    m = dg.Gen_UNet2D((64, 64, 1), nc_out=3)
    sp = "sparse_categorical_crossentropy"
    assert m._focal is None
    assert m.compile(loss=sp, focal_gamma=2.0, label_smoothing=0.1, class_weight=[1, 2, 0.5], ignore_label=255) is m
    assert m._focal == (2.0, 0.1) and m._ignore_label == 255
    m.compile(focal_gamma=1)
    assert m._focal == (1.0, 0.0) and m._class_weight is None and m._loss == "categorical_crossentropy"
    m.compile(label_smoothing=np.float32(0.25), dice_loss="class", ce_weight=0.0)
    assert m._focal == (0.0, 0.25) and m._dice["ce_weight"] == 0.0
    m.compile()
    assert m._focal is None and m._dice is None
    m.compile(focal_gamma=0.0, label_smoothing=0)
    assert m._focal is None
    m.compile(focal_gamma=0.5)
    nan, inf = float("nan"), float("inf")
    for bad in (-1.0, -1e-9, nan, inf, -inf, True, "2", None, [2.0]):
        with pytest.raises(ValueError, match="focal_gamma"):
            m.compile(focal_gamma=bad)
    for bad in (-0.1, 1.0, 1.5, nan, inf, 1.0 - 1e-9, False, "0.1", None):      # 1 - 1e-9 is 1.0 as float32
        with pytest.raises(ValueError, match="label_smoothing"):
            m.compile(label_smoothing=bad)
    assert m._focal == (0.5, 0.0)                                    # a refused compile leaves the setting
    with pytest.raises(RuntimeError, match="tanh"):
        dg.Gen_UNet2D((64, 64, 1)).compile(focal_gamma=2.0)


GAMMAS, SMOOTH = (0.0, 0.5, 1.0, 2.0, 5.0), (0.0, 0.1)


@pytest.mark.parametrize("Cc", [2, 3, 4, 5, 8])
def test_the_bound_is_attainable_in_float32(Cc):
    """The statements in NumPy float32, 1 - r formed directly, against float64 on the inputs of the operator test: a quarter
    of the kernel's bounds (dz 1e-5 max|dz|, the loss sum 1e-5 relative, probabilities 1e-6)."""
    z, codes, w = F.ref_case(Cc)
    t = F.onehot_rows(codes, Cc, 255)
    worst = [0.0, 0.0]
    for gamma in GAMMAS:
        for eps in SMOOTH:
            p64, g64, total, den = F.softmax_ce_focal_ref(z, t, w, gamma, eps)
            p, dz, ls, den32 = F.softmax_ce_focal_f32(z, t, w, gamma, eps)
            assert den32 == den and 0 < den < len(z)
            assert np.isfinite(dz).all() and np.isfinite(ls)
            e_dz, e_ls = np.abs(dz - g64).max() / np.abs(g64).max(), abs(ls - total) / total
            worst = [max(worst[0], e_dz), max(worst[1], e_ls)]
            assert np.abs(p - p64).max() <= 0.25e-6
            assert e_dz <= 0.25e-5, (gamma, eps, e_dz)
            assert e_ls <= 0.25e-5, (gamma, eps, e_ls)
            wi = (t * w).sum(-1)
            assert np.all(dz[wi == 0] == 0.0) and np.all(g64[wi == 0] == 0.0)
    print("C = %d: worst dz deviation %.2e of max|dz|, worst loss-sum deviation %.2e relative" % (Cc, worst[0], worst[1]))
