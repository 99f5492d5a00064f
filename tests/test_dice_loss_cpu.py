"""No GPU: the soft Dice loss's host side -- the C ABI's declarations, exports and refusals, compile's argument
validation, the float64 reference (autograd against the closed form and against central differences) and
evaluate.soft_dice."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dep_gan_im_amd as dg  # noqa: E402
import dice_ref as D  # noqa: E402
import weighted_ce_ref as R  # noqa: E402
from dep_gan_im_amd import _lib, evaluate  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments
ENTRIES = ["depgan_uresnet_set_dice_loss", "depgan_uresnet_get_dice_loss", "depgan_uresnet_last_dice_sums",
           "depgan_op_dice_loss"]


def test_header_declares_and_library_exports_the_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert getattr(lib, name).argtypes, name + " has no argtypes"
    assert _lib._K["DEPGAN_ABI_VERSION"] == 3 == _lib.ABI_VERSION     # depgan_config did not change
    assert [_lib._K["DEPGAN_DICE_" + n] for n in ("OFF", "FLAT", "CLASS")] == [0, 1, 2]
    assert lib.depgan_uresnet_set_dice_loss.argtypes == [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                                         C.c_int]


def test_operator_entry_refuses_its_arguments_before_any_hip_call(lib):
    sums, loss = (C.c_double * 24)(), C.c_float()

    def op(coef=None, n=None, form=2, smooth=1e-7, ce=1.0, dw=1.0, ign=-1, codes=FAKE, onehot=None, probs=FAKE, dz=FAKE,
           sums_=sums, loss_=C.byref(loss), P=64, C_=3):
        ca = (C.c_float * len(coef))(*coef) if coef is not None else None
        return lib.depgan_op_dice_loss(probs, onehot, codes, ign, form, ca, (len(coef) if coef else 0) if n is None else n,
                                       smooth, ce, dw, dz, sums_, loss_, P, C_, None)
    nan, inf = float("nan"), float("inf")
    for kw in ({"form": 0}, {"form": 3}, {"form": -1}, {"form": 1, "coef": (1.0, 1.0, 1.0)}, {"coef": (1.0, 1.0)},
               {"coef": (1.0, 1.0, 1.0, 1.0)}, {"coef": (1.0, -0.5, 1.0)}, {"coef": (1.0, nan, 1.0)},
               {"coef": (inf, 1.0, 1.0)}, {"coef": (0.0, 0.0, 0.0)}, {"smooth": 0.0}, {"smooth": -1e-7}, {"smooth": nan},
               {"smooth": inf}, {"dw": 0.0}, {"dw": -1.0}, {"dw": nan}, {"dw": inf}, {"ce": -1.0}, {"ce": nan}, {"ce": inf},
               {"ign": -2}, {"ign": 256}, {"codes": None}, {"onehot": FAKE}, {"probs": None}, {"dz": None},
               {"sums_": None}, {"loss_": None}, {"P": 0}, {"C_": 1}, {"C_": 9}, {"probs": C.c_void_p(0x1002)}):
        assert op(**kw) == 1, kw
        assert lib.depgan_last_error(), kw
    assert op(coef=(1.0, -0.5, 1.0)) == 1 and b"class coefficient 1" in lib.depgan_last_error()
    assert op(coef=(0.0, 0.0, 0.0)) == 1 and b"every class coefficient is 0" in lib.depgan_last_error()
    assert op(form=1, coef=(1.0, 1.0, 1.0)) == 1 and b"flat form" in lib.depgan_last_error()
    assert op(smooth=0.0) == 1 and b"smooth" in lib.depgan_last_error()
    assert op(C_=4, probs=C.c_void_p(0x1004)) == 1 and b"16-byte" in lib.depgan_last_error()
    assert lib.depgan_uresnet_set_dice_loss(None, 1, 1.0, 1.0, 1e-7, None, 0) == 1
    assert lib.depgan_uresnet_get_dice_loss(None, None, None, None, None) == 0
    assert lib.depgan_uresnet_last_dice_sums(None, sums, None, None) == 1


def test_compile_validates_the_dice_arguments():
    m = dg.Gen_UNet2D((64, 64, 1), nc_out=3)
    sp = "sparse_categorical_crossentropy"
    assert m._dice is None
    assert m.compile(loss=sp, dice_loss="class", dice_classes="foreground", ignore_label=255) is m
    assert m._dice["form"] == "class" and m._dice["ce_weight"] == 1.0 and m._dice["dice_weight"] == 1.0
    assert m._dice["smooth"] == 1e-7 and m._ignore_label == 255 and m._loss == sp
    assert np.array_equal(m._dice["class_coef"], np.array([0.0, 0.5, 0.5], np.float32))
    m.compile(dice_loss="class", dice_classes=[0.2, 0.0, 3.0], dice_weight=2.0, ce_weight=0.0, dice_smooth=1.0)
    assert np.array_equal(m._dice["class_coef"], np.array([0.2, 0.0, 3.0], np.float32)) and m._ignore_label is None
    assert (m._dice["dice_weight"], m._dice["ce_weight"], m._dice["smooth"]) == (2.0, 0.0, 1.0)
    m.compile(dice_loss="flat", ce_weight=0.5)
    assert m._dice == {"form": "flat", "ce_weight": 0.5, "dice_weight": 1.0, "smooth": 1e-7, "class_coef": None}
    m.compile(dice_loss="class")
    assert m._dice["class_coef"] is None and m._dice["form"] == "class"       # NULL: the library's 1 / C
    m.compile()
    assert m._dice is None and m._loss == "categorical_crossentropy"          # compile() without them: off
    # the reference's own name
    m.compile(loss="dice_coef_loss")
    assert m._dice == {"form": "flat", "ce_weight": 0.0, "dice_weight": 1.0, "smooth": 1e-7, "class_coef": None}
    assert m._loss == "dice_coef_loss"
    m._check_labels(np.zeros((2, 64, 64, 3), np.float32), 2, "test")            # one-hot labels
    with pytest.raises(ValueError, match="one-hot"):
        m._check_labels(np.zeros((2, 64, 64), np.uint8), 2, "test")
    before = dict(m._dice)
    nan, inf = float("nan"), float("inf")
    for kw, word in (({"dice_loss": "tversky"}, "dice_loss"), ({"dice_loss": 1}, "dice_loss"),
                     ({"dice_loss": "flat", "dice_classes": [1.0, 1.0, 1.0]}, "dice_classes"),
                     ({"dice_loss": "flat", "dice_classes": "foreground"}, "dice_classes"),
                     ({"dice_classes": "foreground"}, "dice_classes"),
                     ({"dice_loss": "class", "dice_classes": [1.0, 1.0]}, "dice_classes"),
                     ({"dice_loss": "class", "dice_classes": [1.0, 1.0, 1.0, 1.0]}, "dice_classes"),
                     ({"dice_loss": "class", "dice_classes": [1.0, -0.5, 1.0]}, "dice_classes"),
                     ({"dice_loss": "class", "dice_classes": [1.0, nan, 1.0]}, "dice_classes"),
                     ({"dice_loss": "class", "dice_classes": [1.0, inf, 1.0]}, "dice_classes"),
                     ({"dice_loss": "class", "dice_classes": [0.0, 0.0, 0.0]}, "dice_classes"),
                     ({"dice_loss": "class", "dice_classes": "background"}, "dice_classes"),
                     ({"dice_loss": "class", "dice_smooth": 0.0}, "dice_smooth"),
                     ({"dice_loss": "class", "dice_smooth": -1e-7}, "dice_smooth"),
                     ({"dice_loss": "class", "dice_smooth": nan}, "dice_smooth"),
                     ({"dice_loss": "class", "dice_smooth": 1e-60}, "dice_smooth"),     # 0 as float32
                     ({"dice_loss": "flat", "dice_weight": 0.0}, "dice_weight"),
                     ({"dice_loss": "flat", "dice_weight": -1.0}, "dice_weight"),
                     ({"dice_loss": "flat", "dice_weight": inf}, "dice_weight"),
                     ({"dice_loss": "flat", "dice_weight": "1"}, "dice_weight"),
                     ({"dice_loss": "flat", "ce_weight": -0.5}, "ce_weight"),
                     ({"dice_loss": "flat", "ce_weight": nan}, "ce_weight"),
                     ({"loss": "dice_coef_loss", "dice_loss": "class"}, "dice_coef_loss"),
                     ({"loss": "dice_coef_loss", "dice_classes": "foreground"}, "dice_coef_loss"),
                     ({"loss": "dice_coef_loss", "ignore_label": 255}, "all-zero rows"),
                     ({"loss": "dice_loss"}, "loss must be")):
        with pytest.raises(ValueError, match=word):
            m.compile(**kw)
        assert m._dice == before, kw                                          # a refused compile leaves the setting
    with pytest.raises(RuntimeError, match="tanh"):
        dg.Gen_UNet2D((64, 64, 1)).compile(dice_loss="flat")


@pytest.mark.parametrize("Cc", [2, 3, 4, 5, 8])
def test_reference_autograd_equals_the_closed_form_and_central_differences(Cc):
    rng = np.random.default_rng(40 + Cc)
    P = 37
    z = (2.0 * rng.standard_normal((P, Cc))).astype(np.float32)
    codes = rng.integers(0, Cc, P)
    codes[rng.uniform(size=P) < 0.3] = 255
    codes[:Cc] = np.arange(Cc)
    t = R.onehot_rows(codes, Cc, 255)
    keep = D.keep_rows(t)
    assert np.array_equal(keep == 0, codes == 255) and 0 < keep.sum() < P
    coef = rng.uniform(0.1, 2.0, Cc)
    coef[0] = 0.0
    for form, c, smooth in (("flat", None, 1e-7), ("class", coef, 1e-7), ("class", D.class_coef(Cc), 1.0),
                            ("class", D.class_coef(Cc, "foreground"), 1e-7), ("flat", None, 3.0)):
        p, g, L, sums = D.dice_ref(z, t, keep, form, c, smooth)
        g2, L2, sums2, A, B = D.dice_closed_form(p, t, keep, form, c, smooth)
        assert np.abs(g - g2).max() <= 1e-12 and abs(L - L2) <= 1e-12 and np.abs(sums - sums2).max() <= 1e-12
        assert np.abs(g).max() > 1e-4 and np.all(g[keep == 0] == 0) and np.abs(g.sum(-1)).max() < 1e-12
        assert np.array_equal(sums[2], np.bincount(codes[codes != 255], minlength=Cc))
        if form == "flat":
            assert np.all(A == A[0]) and np.all(B == B[0])                     # equal for every k
        # central differences of the loss in double, on a few logits of kept and ignored pixels
        zt = torch.from_numpy(z).double()

        def loss_at(zz):
            return float(D.dice_t(torch.softmax(zz, -1), torch.from_numpy(t).double(), torch.from_numpy(keep), form,
                                  None if c is None else torch.from_numpy(np.asarray(c, np.float64)), smooth)[0])
        h = 1e-5
        for i, k in ((0, 0), (1, Cc - 1), (5, 1), (P - 1, 0), (int(np.argmax(keep == 0)), 1)):
            zp, zm = zt.clone(), zt.clone()
            zp[i, k] += h
            zm[i, k] -= h
            fd = (loss_at(zp) - loss_at(zm)) / (2 * h)
            assert abs(fd - g[i, k]) <= 1e-8 + 1e-6 * abs(g[i, k]), (form, i, k, fd, g[i, k])
    # no pixel takes part: 0.0 with a zero gradient, in both forms
    none = np.zeros(P)
    for form in D.FORMS:
        _, g, L, sums = D.dice_ref(z, t, none, form, D.class_coef(Cc), 1e-7)
        assert L == 0.0 and np.all(g == 0) and np.all(sums == 0)
    # c_k = 1 / C is one minus the mean class Dice; 'foreground' leaves class 0 out
    p, _, L, sums = D.dice_ref(z, t, keep, "class", np.full(Cc, 1.0 / Cc), 1e-7)
    dice = evaluate.soft_dice({"intersection": sums[0], "pred": sums[1], "true": sums[2]}, float(np.float32(1e-7)))
    assert abs(L - (1.0 - dice["dice"].mean())) < 1e-12
    _, _, Lf, _ = D.dice_ref(z, t, keep, "class", D.class_coef(Cc, "foreground"), 1e-7)
    if Cc > 2:
        assert abs(Lf - (1.0 - dice["mean_dice"])) < 1e-6                      # the coefficients are float32 values
    _, _, Lflat, _ = D.dice_ref(z, t, keep, "flat", None, 1e-7)
    assert abs(Lflat - (1.0 - dice["flat"])) < 1e-12


def test_soft_dice_on_hand_made_sums():
    s = {"intersection": [3.0, 0.0, 1.5], "pred": [4.0, 1.0, 2.0], "true": [5.0, 0.0, 2.0]}
    d = evaluate.soft_dice(s, smooth=1.0)
    assert np.allclose(d["dice"], [7.0 / 10.0, 1.0 / 2.0, 4.0 / 5.0], rtol=0, atol=1e-15)
    assert abs(d["flat"] - 10.0 / 15.0) < 1e-15 and abs(d["mean_dice"] - (0.5 + 0.8) / 2) < 1e-15
    d = evaluate.soft_dice({k: np.array(v) for k, v in s.items()})
    assert abs(d["dice"][0] - (6.0 + 1e-7) / (9.0 + 1e-7)) < 1e-15 and d["dice"][1] == pytest.approx(1e-7 / (1.0 + 1e-7))
    empty = evaluate.soft_dice({"intersection": [0, 0], "pred": [0, 0], "true": [0, 0]})
    assert np.all(empty["dice"] == 1.0) and empty["flat"] == 1.0
    with pytest.raises(ValueError, match="per class"):
        evaluate.soft_dice({"intersection": [1.0], "pred": [1.0], "true": [1.0]})
    with pytest.raises(ValueError, match="per class"):
        evaluate.soft_dice({"intersection": [1.0, 1.0], "pred": [1.0, 1.0, 1.0], "true": [1.0, 1.0]})
    with pytest.raises(ValueError, match="smooth"):
        evaluate.soft_dice(s, smooth=0.0)
