"""No GPU: the boundary loss's host side -- the float64 restatement (against scipy's Euclidean distance transform where
scipy is there, its gradient against torch autograd), compile's and data.signed_distance_maps' argument validation, the
C ABI's declarations and the refusals that need no device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boundary_ref as BR  # noqa: E402
import dep_gan_im_amd as dg  # noqa: E402
import weighted_ce_ref as R  # noqa: E402
from dep_gan_im_amd import _lib, callbacks, data  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments
ENTRIES = {"depgan_op_signed_distance": 13, "depgan_op_boundary_loss": 13, "depgan_uresnet_set_boundary_loss": 8,
           "depgan_uresnet_get_boundary_loss": 6, "depgan_uresnet_last_boundary_loss": 3}


def _codes(rng, n, H, W, Cc, ignore_frac=0.0):
    codes = rng.integers(0, Cc, (n, H, W)).astype(np.uint8)
    if ignore_frac:
        codes[rng.uniform(size=codes.shape) < ignore_frac] = 255
    return codes


def test_restatement_by_hand():
    """one row, unit spacing: S = {2, 3, 4} of 7 pixels"""
    tc = np.array([[[0, 0, 1, 1, 1, 0, 0]]])
    phi = BR.signed_distance(tc, 2)
    assert np.array_equal(phi[0, 0, :, 1], np.array([2, 1, -1, -2, -1, 1, 2], np.float32))
    assert np.array_equal(phi[0, 0, :, 0], -phi[0, 0, :, 1])                 # two classes: complementary sets
    off = BR.signed_distance(tc, 2, inside_offset=1.0)                       # the map of the published code
    assert np.array_equal(off[0, 0, :, 1], np.array([2, 1, 0, -1, 0, 1, 2], np.float32))
    # a class absent from the slice, or filling it: 0 everywhere; slices do not see each other
    two = np.stack([tc[0], np.zeros_like(tc[0])])
    phi = BR.signed_distance(two, 2)
    assert np.all(phi[1] == 0) and np.array_equal(phi[0], BR.signed_distance(tc, 2)[0])
    # a pixel without a class is a member of none: it lies outside every S and ends the inside of its neighbours
    tc = np.array([[[1, 1, BR.NO_CLASS, 1, 1]]])
    phi = BR.signed_distance(tc, 2)
    assert np.array_equal(phi[0, 0, :, 1], np.array([-2, -1, 1, -1, -2], np.float32)) and np.all(phi[..., 0] == 0)
    assert np.all(BR.signed_distance(tc, 2, class_on=[1, 0])[..., 1] == 0)
    # the true class: codes, one-hot rows (first arg-max), all-zero rows with and without an ignore code
    rows = np.array([[[[0, 0, 0], [0.5, 0.5, 0], [0, 0, 1]]]], np.float32)
    assert BR.true_class(rows, 3).tolist() == [[[0, 0, 2]]] and BR.true_class(rows, 3, 0).tolist() == [[[-1, 0, 2]]]
    assert BR.true_class(np.array([[[0, 2, 3, 255]]]), 3, 255).tolist() == [[[0, 2, -1, -1]]]


@pytest.mark.parametrize("spacing", [(1.0, 1.0), (0.977, 1.013)])
def test_restatement_against_scipy(spacing):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    tc = rng.integers(0, 3, (2, 23, 31))
    tc[1][tc[1] == 2] = 0                                                    # class 2 absent from slice 1
    phi = BR.signed_distance(tc, 3, spacing, inside_offset=0.25)
    for s in range(2):
        for k in range(3):
            inside = tc[s] == k
            if not inside.any() or inside.all():
                want = np.zeros(inside.shape)
            else:
                want = np.where(inside, -(ndi.distance_transform_edt(inside, sampling=spacing) - 0.25),
                                ndi.distance_transform_edt(~inside, sampling=spacing))
            # scipy squares the spacing inside its own arithmetic: the last bits of d2 may differ, the float32 rarely
            assert np.abs(phi[s, :, :, k] - want).max() <= 2e-6 * max(1.0, np.abs(want).max()), (s, k)
    assert np.all(phi[1, :, :, 2] == 0)


@pytest.mark.parametrize("Cc", [2, 3, 4, 8])
def test_restatement_gradient_against_autograd(Cc):
    rng = np.random.default_rng(50 + Cc)
    n, H, W = 2, 5, 7
    codes = _codes(rng, n, H, W, Cc, 0.2)
    tc = BR.true_class(codes, Cc, 255)
    phi = BR.signed_distance(tc, Cc, (0.9375, 0.9375)).reshape(-1, Cc)
    keep = (tc.reshape(-1) != BR.NO_CLASS).astype(np.float64)
    z = (2.0 * rng.standard_normal((n * H * W, Cc))).astype(np.float32)
    for coef in (BR.class_coef(Cc), BR.class_coef(Cc, "foreground"), rng.uniform(0.1, 2.0, Cc)):
        zt = torch.from_numpy(z).double().requires_grad_(True)
        p = torch.softmax(zt, -1)
        L = BR.boundary_t(p, torch.from_numpy(phi).double(), torch.from_numpy(keep), torch.from_numpy(np.asarray(coef)))
        (g,) = torch.autograd.grad(L, zt)
        dz, Lnp, M, scale = BR.boundary_np(p.detach().numpy(), phi, keep, coef)
        assert M == keep.sum() > 0 and abs(Lnp - float(L.detach())) <= 1e-12 * max(1.0, scale)
        assert np.abs(dz - g.numpy()).max() <= 1e-14 and np.abs(dz).max() > 1e-4
        assert np.all(dz[keep == 0] == 0) and np.abs(dz.sum(-1)).max() < 1e-15
    # the sign: all the mass inside the true class gives a negative term, all of it far outside a positive one
    onehot = R.onehot_rows(np.where(tc < 0, 0, tc), Cc).reshape(-1, Cc).astype(np.float64)
    _, perfect, _, _ = BR.boundary_np(onehot, phi, keep, BR.class_coef(Cc))
    _, wrong, _, _ = BR.boundary_np(np.roll(onehot, 1, axis=1), phi, keep, BR.class_coef(Cc))
    assert perfect < 0 < wrong
    # no pixel takes part
    dz, L0, M0, _ = BR.boundary_np(onehot, phi, np.zeros_like(keep), BR.class_coef(Cc))
    assert L0 == 0.0 and M0 == 0.0 and np.all(dz == 0)


def test_compile_validates_the_boundary_arguments():
    m = dg.Gen_UNet2D((64, 64, 1), nc_out=3)
    assert m._boundary is None and m.boundary_weight is None
    assert m.compile(boundary_loss=True) is m
    assert m._boundary == {"weight": 1.0, "class_coef": None, "spacing": (1.0, 1.0), "inside_offset": 0.0}
    m.compile(loss="sparse_categorical_crossentropy", ignore_label=255, dice_loss="class", focal_gamma=2.0,
              boundary_loss=True, boundary_weight=0.01, boundary_classes="foreground", boundary_spacing=(0.9375, 1),
              boundary_inside_offset=0.5)
    assert m.boundary_weight == 0.01 and m._boundary["spacing"] == (0.9375, 1.0) and m._boundary["inside_offset"] == 0.5
    assert np.array_equal(m._boundary["class_coef"], np.array([0.0, 0.5, 0.5], np.float32))
    assert m._dice is not None and m._focal is not None and m._ignore_label == 255
    m.set_boundary_weight(0.25)
    assert m.boundary_weight == 0.25
    before = dict(m._boundary)
    nan, inf = float("nan"), float("inf")
    for kw, word in (({"boundary_loss": "yes"}, "boundary_loss"), ({"boundary_loss": 1}, "boundary_loss"),
                     ({"boundary_classes": "foreground"}, "boundary_classes"),
                     ({"boundary_loss": True, "boundary_weight": -1.0}, "boundary_weight"),
                     ({"boundary_loss": True, "boundary_weight": nan}, "boundary_weight"),
                     ({"boundary_loss": True, "boundary_weight": inf}, "boundary_weight"),
                     ({"boundary_loss": True, "boundary_weight": None}, "boundary_weight"),
                     ({"boundary_loss": True, "boundary_weight": "1"}, "boundary_weight"),
                     ({"boundary_loss": True, "boundary_classes": "background"}, "boundary_classes"),
                     ({"boundary_loss": True, "boundary_classes": [1.0, 1.0]}, "boundary_classes"),
                     ({"boundary_loss": True, "boundary_classes": [1.0, -1.0, 1.0]}, "boundary_classes"),
                     ({"boundary_loss": True, "boundary_classes": [1.0, nan, 1.0]}, "boundary_classes"),
                     ({"boundary_loss": True, "boundary_classes": [0.0, 0.0, 0.0]}, "boundary_classes"),
                     ({"boundary_loss": True, "boundary_spacing": 1.0}, "boundary_spacing"),
                     ({"boundary_loss": True, "boundary_spacing": (1.0, 1.0, 1.0)}, "boundary_spacing"),
                     ({"boundary_loss": True, "boundary_spacing": (1.0, 0.0)}, "boundary_spacing"),
                     ({"boundary_loss": True, "boundary_spacing": (inf, 1.0)}, "boundary_spacing"),
                     ({"boundary_loss": True, "boundary_spacing": (1.0, nan)}, "boundary_spacing"),
                     ({"boundary_loss": True, "boundary_inside_offset": -0.1}, "boundary_inside_offset"),
                     ({"boundary_loss": True, "boundary_inside_offset": 1.5}, "boundary_inside_offset"),
                     ({"boundary_loss": True, "boundary_spacing": (0.5, 1.0), "boundary_inside_offset": 0.75},
                      "boundary_inside_offset"),
                     ({"boundary_loss": True, "boundary_inside_offset": nan}, "boundary_inside_offset")):
        with pytest.raises(ValueError, match=word):
            m.compile(**kw)
        assert m._boundary == before or all(np.array_equal(m._boundary[k], before[k]) for k in before), kw
    for w in (-1.0, nan, None, "1"):
        with pytest.raises(ValueError, match="boundary_weight"):
            m.set_boundary_weight(w)
    assert m.boundary_weight == 0.25
    m.compile()
    assert m._boundary is None                                               # compile() without them: off
    with pytest.raises(RuntimeError, match="boundary_loss=True"):
        m.set_boundary_weight(1.0)
    with pytest.raises(RuntimeError, match="tanh"):
        dg.Gen_UNet2D((64, 64, 1)).compile(boundary_loss=True)
    # the scheduler asks for a model compiled with the mode, and for a number
    cb = callbacks.BoundaryWeightScheduler(lambda epoch, w: 0.01 * (epoch + 1))
    cb.set_model(m)
    with pytest.raises(ValueError, match="boundary_loss=True"):
        cb.on_epoch_begin(0)
    m.compile(boundary_loss=True, boundary_weight=0.5)
    cb.on_epoch_begin(2)
    assert m.boundary_weight == pytest.approx(0.03)
    bad = callbacks.BoundaryWeightScheduler(lambda epoch, w: "0.1")
    bad.set_model(m)
    with pytest.raises(ValueError, match="should be float"):
        bad.on_epoch_begin(0)


def test_signed_distance_maps_validates_before_the_library_loads(monkeypatch):
    def no_load():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_load)
    codes = np.zeros((2, 8, 8), np.uint8)
    for kw, word in (({"n_class": 1}, "n_class"), ({"n_class": 9}, "n_class"), ({"n_class": True}, "n_class"),
                     ({"spacing": (1.0,)}, "spacing"), ({"spacing": (0.0, 1.0)}, "spacing"),
                     ({"spacing": (1.0, float("nan"))}, "spacing"), ({"spacing": 2.0}, "spacing"),
                     ({"inside_offset": -1.0}, "inside_offset"), ({"inside_offset": 1.01}, "inside_offset"),
                     ({"spacing": (0.5, 2.0), "inside_offset": 0.6}, "inside_offset"),
                     ({"ignore_label": 256}, "ignore_label"), ({"ignore_label": -1}, "ignore_label"),
                     ({"classes": []}, "classes"), ({"classes": [3]}, "classes"), ({"classes": [0.0]}, "classes")):
        args = dict({"n_class": 3}, **kw)
        with pytest.raises(ValueError, match=word):
            data.signed_distance_maps(codes, **args)
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((2, 8, 8, 2), np.uint8), np.zeros((2, 8, 8, 4), np.float32),
                np.zeros((0, 8, 8), np.uint8), np.zeros((1, 1, 4097), np.uint8)):
        with pytest.raises(ValueError, match="labels"):
            data.signed_distance_maps(bad, 3)
    with pytest.raises(ValueError, match="integral"):
        data.signed_distance_maps(np.full((1, 4, 4), 0.5, np.float32), 3)
    with pytest.raises(AssertionError, match="the library was reached"):
        data.signed_distance_maps(codes, 3)                                  # valid arguments do reach it


def test_header_declares_and_library_exports_the_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    for name, nparam in ENTRIES.items():
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert len(getattr(lib, name).argtypes) == nparam == len(_lib._HDR.prototypes[name][1]), name
    assert _lib._K["DEPGAN_ABI_VERSION"] == 3 == _lib.ABI_VERSION            # depgan_config did not change
    assert lib.depgan_abi_version() == 3
    assert lib.depgan_uresnet_set_boundary_loss.argtypes == [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int,
                                                             C.c_double, C.c_double, C.c_double]
    assert lib.depgan_op_signed_distance.argtypes[8:11] == [C.c_double] * 3


def test_operator_entries_refuse_their_arguments_before_any_hip_call(lib):
    nan, inf = float("nan"), float("inf")

    def sd(onehot=None, codes=FAKE, ign=-1, n=2, H=8, W=8, C_=3, on=None, sy=1.0, sx=1.0, off=0.0, phi=FAKE):
        sw = (C.c_int * len(on))(*on) if on is not None else None
        return lib.depgan_op_signed_distance(onehot, codes, ign, n, H, W, C_, sw, sy, sx, off, phi, None)
    for kw in ({"codes": None}, {"onehot": FAKE}, {"phi": None}, {"phi": C.c_void_p(0x1002)},
               {"onehot": C.c_void_p(0x1001), "codes": None}, {"ign": -2}, {"ign": 256}, {"n": 0}, {"H": 0}, {"W": 0},
               {"H": 4097}, {"W": 4097}, {"n": 1 << 20, "H": 64, "W": 64}, {"n": 1 << 22, "H": 8, "W": 1}, {"C_": 1}, {"C_": 9}, {"on": (0, 0, 0)},
               {"sy": 0.0}, {"sy": -1.0}, {"sy": nan}, {"sy": inf}, {"sx": 0.0}, {"sx": nan}, {"sx": inf},
               {"off": -0.5}, {"off": 1.5}, {"off": nan}, {"sy": 0.5, "off": 0.75}):
        assert sd(**kw) == 1, kw
        assert lib.depgan_last_error(), kw
    assert sd(sy=0.0) == 1 and b"spacings" in lib.depgan_last_error()
    assert sd(off=1.5) == 1 and b"inside_offset" in lib.depgan_last_error()
    assert sd(H=4097) == 1 and b"4096" in lib.depgan_last_error()
    assert sd(on=(0, 0, 0)) == 1 and b"switched off" in lib.depgan_last_error()
    out = (C.c_double * 2)()

    def bl(coef=None, n=None, bc=1.0, ign=-1, codes=FAKE, onehot=None, probs=FAKE, phi=FAKE, dz=FAKE, out_=out, P=64,
           C_=3):
        ca = (C.c_float * len(coef))(*coef) if coef is not None else None
        return lib.depgan_op_boundary_loss(probs, phi, onehot, codes, ign, ca, (len(coef) if coef else 0) if n is None else n,
                                           bc, dz, out_, P, C_, None)
    for kw in ({"coef": (1.0, 1.0)}, {"coef": (1.0, 1.0, 1.0, 1.0)}, {"coef": (1.0, -0.5, 1.0)}, {"coef": (1.0, nan, 1.0)},
               {"coef": (inf, 1.0, 1.0)}, {"coef": (0.0, 0.0, 0.0)}, {"bc": -1.0}, {"bc": nan}, {"bc": inf},
               {"ign": -2}, {"ign": 256}, {"codes": None}, {"onehot": FAKE}, {"probs": None}, {"phi": None},
               {"out_": None}, {"P": 0}, {"P": 1 << 31}, {"C_": 1}, {"C_": 9}, {"probs": C.c_void_p(0x1002)},
               {"phi": C.c_void_p(0x1002)}, {"dz": C.c_void_p(0x1002)}):
        assert bl(**kw) == 1, kw
        assert lib.depgan_last_error(), kw
    assert bl(coef=(1.0, -0.5, 1.0)) == 1 and b"class coefficient 1" in lib.depgan_last_error()
    assert bl(coef=(0.0, 0.0, 0.0)) == 1 and b"every class coefficient is 0" in lib.depgan_last_error()
    assert bl(bc=nan) == 1 and b"boundary_coef" in lib.depgan_last_error()
    assert bl(C_=4, phi=C.c_void_p(0x1004)) == 1 and b"16-byte" in lib.depgan_last_error()
    # the context entries on no context
    assert lib.depgan_uresnet_set_boundary_loss(None, 1, 1.0, None, 0, 1.0, 1.0, 0.0) == 1
    assert lib.depgan_uresnet_get_boundary_loss(None, None, None, None, None, None) == 0
    assert lib.depgan_uresnet_last_boundary_loss(None, out, None) == 1
