"""No GPU: the loss-weight mode's host side -- the float64 reference helper against a plain NumPy restatement,
data.balanced_class_weights, compile's argument validation, and the C ABI's declarations, exports and refusals."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dep_gan_im_amd as dg  # noqa: E402
import weighted_ce_ref as R  # noqa: E402
from dep_gan_im_amd import _lib, data  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments
ENTRIES = ["depgan_uresnet_set_loss_weights", "depgan_uresnet_get_loss_weights", "depgan_uresnet_last_label_counts",
           "depgan_op_softmax_ce_weighted", "depgan_op_label_counts"]


def test_header_declares_and_library_exports_the_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert getattr(lib, name).argtypes, name + " has no argtypes"
    assert _lib._K["DEPGAN_ABI_VERSION"] == 3          # depgan_config did not change
    assert _lib._K["DEPGAN_LABEL_NCOUNT"] == 3 + _lib.MAX_HEAD_CLASSES


def test_operator_entries_refuse_their_arguments_before_any_hip_call(lib):
    cnt = (C.c_longlong * 11)()

    def ce(w=(1.0, 1.0, 1.0), n=None, ign=-1, codes=FAKE, onehot=None, counts=cnt, P=64, C_=3, logits=FAKE):
        wa = (C.c_float * len(w))(*w) if w is not None else None
        return lib.depgan_op_softmax_ce_weighted(logits, onehot, codes, wa, len(w) if n is None and w else (n or 0), ign,
                                                 FAKE, FAKE, FAKE, None, counts, P, C_, None)
    nan, inf = float("nan"), float("inf")
    for kw in ({"w": (1.0, -1.0, 1.0)}, {"w": (1.0, nan, 1.0)}, {"w": (inf, 1.0, 1.0)}, {"w": (0.0, 0.0, 0.0)},
               {"w": (1.0, 1.0)}, {"w": (1.0, 1.0, 1.0, 1.0)}, {"ign": -2}, {"ign": 256}, {"w": None}, {"counts": None},
               {"codes": None}, {"codes": FAKE, "onehot": FAKE}, {"P": 0}, {"C_": 9, "w": (1.0,) * 9}, {"logits": None}):
        assert ce(**kw) == 1, kw
        assert lib.depgan_last_error(), kw
    assert ce(w=(1.0, -1.0, 1.0)) == 1 and b"class weight 1" in lib.depgan_last_error()
    assert ce(w=(0.0, 0.0, 0.0)) == 1 and b"every class weight is 0" in lib.depgan_last_error()
    assert ce(ign=300) == 1 and b"ignore code 300" in lib.depgan_last_error()
    for kw in ({"P": 0}, {"C_": 1}, {"C_": 9}, {"ign": -2}, {"ign": 256}, {"out": None}, {"codes": None},
               {"onehot": FAKE}):
        a = dict(onehot=None, codes=FAKE, P=64, C_=3, ign=-1, out=cnt)
        a.update(kw)
        assert lib.depgan_op_label_counts(a["onehot"], a["codes"], a["P"], a["C_"], a["ign"], a["out"], None) == 1, kw
    assert lib.depgan_uresnet_set_loss_weights(None, None, 0, -1) == 1
    assert lib.depgan_uresnet_get_loss_weights(None, None, None) == 0
    assert lib.depgan_uresnet_last_label_counts(None, cnt, None) == 1


def test_reference_loss_equals_a_numpy_restatement():
    rng = np.random.default_rng(4)
    for Cc in (2, 4, 7):
        z = (2.0 * rng.standard_normal((5, 9, Cc))).astype(np.float32)
        z[0, 0] = 60.0 * np.eye(Cc)[0]                              # both clip bounds are reached
        codes = rng.integers(0, Cc, (5, 9))
        codes[rng.uniform(size=codes.shape) < 0.3] = 255
        codes[0, 0] = 1
        t = R.onehot_rows(codes, Cc, 255)
        assert np.array_equal(t.sum(-1) == 0, codes == 255)
        cw = rng.uniform(0.2, 3.0, Cc)
        cw[0] = 0.0
        p = torch.softmax(torch.from_numpy(z).double(), -1)
        loss, den, total = R.weighted_ce_t(p, torch.from_numpy(t).double(), torch.from_numpy(cw))
        want, wden, wtotal = R.weighted_ce_np(p.numpy(), t, cw)
        assert den == wden == int(((codes != 255) & (codes != 0)).sum())
        assert abs(float(loss) - want) <= 1e-12 * abs(want) and abs(float(total) - wtotal) <= 1e-12 * abs(wtotal)
        # unit weights and nothing ignored: the oracle's own loss
        from oracle import depgan_oracle as O
        full = R.onehot_rows(np.where(codes == 255, 0, codes), Cc)
        loss1, den1, _ = R.weighted_ce_t(p, torch.from_numpy(full).double(), torch.ones(Cc, dtype=torch.float64))
        assert den1 == 45 and abs(float(loss1) - float(O.keras_categorical_crossentropy_t(p, torch.from_numpy(full).double()))) < 1e-12
        # nothing left: 0.0, not NaN
        none, den0, _ = R.weighted_ce_t(p, torch.zeros_like(p), torch.from_numpy(cw))
        assert float(none) == 0.0 and den0 == 0
    pr, g, total, den = R.softmax_ce_weighted_ref(z.reshape(-1, Cc), t.reshape(-1, Cc), cw)
    assert g.shape == (45, Cc) and np.all(g[(t.reshape(-1, Cc) * cw).sum(-1) == 0] == 0) and np.abs(g.sum(-1)).max() < 1e-12


def test_balanced_class_weights():
    n = np.array([600, 30, 0, 270])
    w = data.balanced_class_weights(n)
    assert np.allclose(w, [900 / (4 * 600), 900 / (4 * 30), 0.0, 900 / (4 * 270)]) and w[2] == 0.0
    assert np.allclose(data.balanced_class_weights({"classes": n}, "inverse"), w)
    m = data.balanced_class_weights(n, "median")
    assert np.allclose(m, [270 / 600, 270 / 30, 0.0, 1.0])
    assert np.allclose(data.balanced_class_weights([5, 5, 5]), 1.0) and np.allclose(data.balanced_class_weights([5, 5, 5], "median"), 1.0)
    # the weighted pixel mass of the 'inverse' rule is the same for every class that occurs
    assert np.allclose((w * n)[n > 0], 900 / 4)
    with pytest.raises(ValueError, match="no class occurs"):
        data.balanced_class_weights([0, 0, 0])
    for bad in ([1, -1], [1.0, float("nan")]):
        with pytest.raises(ValueError, match="finite"):
            data.balanced_class_weights(bad)
    with pytest.raises(ValueError, match="rule"):
        data.balanced_class_weights(n, "sqrt")


def test_compile_validates_class_weight_and_ignore_label():
    m = dg.Gen_UNet2D((64, 64, 1), nc_out=3)
    sp = "sparse_categorical_crossentropy"
    assert m.compile(loss=sp, class_weight=[1, 2, 0.5], ignore_label=255) is m
    assert np.array_equal(m._class_weight, np.array([1, 2, 0.5], np.float32)) and m._ignore_label == 255
    m.compile(loss=sp, class_weight={2: 3.0})
    assert np.array_equal(m._class_weight, np.array([1, 1, 3], np.float32)) and m._ignore_label is None
    m.compile(loss=sp, ignore_label=0)
    assert m._class_weight is None and m._ignore_label == 0
    m.compile(class_weight=(0.0, 1.0, 1.0))
    assert m._loss == "categorical_crossentropy" and m._class_weight[0] == 0
    m.compile()
    assert m._class_weight is None and m._ignore_label is None
    with pytest.raises(ValueError, match="all-zero rows"):
        m.compile(loss="categorical_crossentropy", ignore_label=255)
    with pytest.raises(ValueError, match="all-zero rows"):
        m.compile(ignore_label=3)
    for bad in ([1, 2], [1, 2, 3, 4], [1, -1, 1], [1, float("nan"), 1], [1, float("inf"), 1], [0, 0, 0], {3: 1.0},
                {-1: 1.0}, {0: -2.0}, {"a": 1.0}):
        with pytest.raises(ValueError, match="class_weight"):
            m.compile(loss=sp, class_weight=bad)
    for bad in (-1, 256, 1.5, True, "255"):
        with pytest.raises(ValueError, match="ignore_label"):
            m.compile(loss=sp, ignore_label=bad)
    assert m._class_weight is None and m._ignore_label is None          # a refused compile leaves the setting
    with pytest.raises(RuntimeError, match="tanh"):
        dg.Gen_UNet2D((64, 64, 1)).compile(class_weight=[1.0])
    for bad in (-1, 256, 2.5, True):
        with pytest.raises(ValueError, match="ignore_label"):
            data.to_codes(np.zeros((1, 2, 2)), 4, ignore_label=bad)
