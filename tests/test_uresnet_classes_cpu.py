"""What the DEP-UResNet with 2 to 8 classes and integer labels decides without a GPU: the five new prototypes of
include/depgan.h, the constructor's class range and weight table, the inference-context rule, compile's two losses, the
label checks that come before any library call, and the operator entries' argument checks (status 1 before any HIP
call)."""
import ctypes as C

import numpy as np
import pytest

import dep_gan_im_amd as dg
from dep_gan_im_amd import _lib, engine

FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments
NEW = {"depgan_op_softmax_ce": 9, "depgan_op_head_softmax_k_bf16s": 10, "depgan_uresnet_grads_sparse": 7,
       "depgan_uresnet_step_sparse": 7, "depgan_uresnet_eval_sparse": 6}


def test_header_declares_the_five_new_entries():
    hdr = _lib.parse_header(_lib.read_header())
    for name, nargs in NEW.items():
        assert name in hdr.prototypes and name in _lib.EXPORTS, name
        restype, argtypes = hdr.prototypes[name]
        assert restype is C.c_int and len(argtypes) == nargs, (name, len(argtypes))
    assert hdr.constants["DEPGAN_ABI_VERSION"] == 3 and _lib.ABI_VERSION == 3      # new entries are not a new ABI
    assert hdr.constants["DEPGAN_MAX_HEAD_CLASSES"] == 8 == _lib.MAX_HEAD_CLASSES
    # the entries that stay keep their signatures
    assert len(hdr.prototypes["depgan_op_softmax_ce4"][1]) == 7
    assert len(hdr.prototypes["depgan_op_head_softmax_bf16s"][1]) == 9


def test_library_exports_them(lib):
    for name, nargs in NEW.items():
        assert len(getattr(lib, name).argtypes) == nargs


@pytest.mark.parametrize("c", range(2, 9))
def test_constructor_and_weight_table_for_every_class_count(c):
    m = dg.Gen_UNet2D((64, 64, 1), nc_out=c)
    assert m.nc_out == c and m.name == "DEP_UResNet" and m.get_config()["nc_out"] == c
    w = m.get_weights_dict()
    assert w["gen_segmentation/kernel"].shape == (1, 1, 32, c) and w["gen_segmentation/bias"].shape == (c,)
    assert m.count_params() == dg.Gen_UNet2D((64, 64, 1)).count_params() + (c - 1) * 33
    lines = []
    m.summary(print_fn=lines.append)
    assert any("gen_segmentation/kernel" in ln and "(1, 1, 32, %d)" % c in ln for ln in lines)
    twin = m.inference_copy()
    assert twin.inference_only and twin.nc_out == c
    assert twin.get_weights_dict()["gen_segmentation/kernel"].shape == (1, 1, 32, c)


@pytest.mark.parametrize("c", [9, -1, 0, 2.0, True])
def test_constructor_names_the_range(c):
    with pytest.raises(ValueError, match=r"\[2, 8\]"):
        dg.Gen_UNet2D((64, 64, 1), nc_out=c)


def test_weights_round_trip_through_save_and_load(tmp_path):
    m = dg.Gen_UNet2D((64, 64, 1), nc_out=3, seed=5)
    path = str(tmp_path / "w3.npz")
    m.save(path)
    other = dg.Gen_UNet2D((64, 64, 1), nc_out=3, seed=6)
    other.load_weights(path)
    a, b = m.get_weights_dict(), other.get_weights_dict()
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    with pytest.raises(Exception):
        dg.Gen_UNet2D((64, 64, 1), nc_out=5).load_weights(path)      # another head width is another model


def test_keras_h5_lookup_serves_the_head_width():
    m = dg.Gen_UNet2D((64, 64, 1), nc_out=5, seed=2)
    w = m.get_weights_dict()
    f = {"model_weights": {}}
    for n, v in w.items():                 # model.save layout: model_weights/<layer>/<layer>/<weight>:0
        layer, name = n.split("/", 1)
        f["model_weights"].setdefault(layer, {layer: {}})[layer][name + ":0"] = v
    got = dg.models.weights_from_keras_h5(f, list(w))
    assert got["gen_segmentation/kernel"].shape == (1, 1, 32, 5) and all(np.array_equal(got[k], w[k]) for k in w)


def test_inference_only_follows_the_class_count():
    def bare(**kw):                        # a context-less engine: the checks read the configuration only
        eng = engine.Engine.__new__(engine.Engine)
        eng.cfg, eng.h = _lib.Config(**kw), None
        return eng
    eng = bare(bf16_weights=1, bf16_mfma=1, nc_out=3)
    assert eng.inference_only
    eng.forward_storage = "bfloat16"
    with pytest.raises(ValueError, match="inference"):
        eng.uresnet(None, None, None)
    assert not bare(nc_out=3).inference_only
    assert not bare(bf16_weights=1, bf16_mfma=1, nc_out=1).inference_only
    with pytest.raises(ValueError, match="bf16_mfma"):
        bare(nc_out=3).forward_storage = "bfloat16"


def test_compile_takes_the_two_losses():
    m = dg.Gen_UNet2D((64, 64, 1), nc_out=3)
    assert m.compile(loss="categorical_crossentropy") is m
    assert m.compile(loss="sparse_categorical_crossentropy") is m
    with pytest.raises(ValueError, match="sparse_categorical_crossentropy"):
        m.compile(loss="mse")
    with pytest.raises(RuntimeError):
        dg.Gen_UNet2D((64, 64, 1)).compile(loss="sparse_categorical_crossentropy")      # the tanh generator


def test_label_checks_come_before_the_library(monkeypatch):
    """Without a GPU an engine cannot even be created: reaching Engine() here would raise DepganError, not ValueError."""
    def no_engine(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(dg.models.GeneratorModel, "_ensure_engine", no_engine)
    n, H = 2, 64
    x, z = np.zeros((n, H, H, 1), np.float32), np.zeros((n, 32, 1), np.float32)
    codes = np.zeros((n, H, H), np.int64)
    onehot = np.zeros((n, H, H, 3), np.float32)
    calls = lambda m, lab: (lambda: m.train_on_batch([x, z], lab), lambda: m.test_on_batch([x, z], lab),      # noqa: E731
                            lambda: m.evaluate([x, z], lab), lambda: m.fit([x, z], lab, verbose=0),
                            lambda: m.fit([x, z], codes if m._loss.startswith("sparse") else onehot, verbose=0,
                                          validation_data=([x, z], lab)))
    dense = dg.Gen_UNet2D((H, H, 1), nc_out=3).compile(loss="categorical_crossentropy")
    for lab in (codes, codes[..., None], onehot[..., :2]):
        for call in calls(dense, lab):
            with pytest.raises(ValueError, match="one-hot"):
                call()
    sparse = dg.Gen_UNet2D((H, H, 1), nc_out=3).compile(loss="sparse_categorical_crossentropy")
    for lab in (onehot, codes[:, :32], codes[..., None, None]):
        for call in calls(sparse, lab):
            with pytest.raises(ValueError, match="class indices"):
                call()
    frac = codes.astype(np.float32)
    frac[1, 3, 5] = 1.5
    nan = codes.astype(np.float64)
    nan[0, 0, 0] = np.nan
    for lab in (frac, frac[..., None], nan, codes.astype(np.complex64)):
        for call in calls(sparse, lab):
            with pytest.raises(ValueError, match="integ"):
                call()
    # what is accepted gets as far as the engine
    for lab in (codes, codes[..., None].astype(np.uint8), codes.astype(np.float32), codes.astype(np.int8)):
        with pytest.raises(AssertionError, match="library was reached"):
            sparse.train_on_batch([x, z], lab)
    with pytest.raises(AssertionError, match="library was reached"):
        dense.train_on_batch([x, z], onehot)


def test_metrics_are_the_four_code_scheme():
    from dep_gan_im_amd import evaluate
    for c in (3, 5):
        with pytest.raises(ValueError, match="4-code"):
            evaluate.uresnet_metrics(np.zeros((2, 8, 8, c)), None, None, None, None, None, 1.0)
        with pytest.raises(ValueError, match="4-code"):
            evaluate.label_metrics_from_census([0] * 18, 1.0, n_class=c)
    assert evaluate.label_metrics_from_census([0] * 18, 1.0)["census"] == [0] * 18


def test_softmax_ce_refuses_its_arguments_before_any_hip_call(lib):
    def ce(logits=FAKE, onehot=None, codes=None, probs=FAKE, dz=FAKE, ls=FAKE, P=64, C_=3):
        return lib.depgan_op_softmax_ce(logits, onehot, codes, probs, dz, ls, P, C_, None)
    odd = C.c_void_p(0x1002)               # not a float address
    half = C.c_void_p(0x1008)              # a float address, not a 16-byte one
    for kw in ({"logits": None}, {"probs": None}, {"P": 0}, {"P": -5}, {"C_": 1}, {"C_": 9}, {"C_": 0}, {"C_": -4},
               {"onehot": FAKE, "codes": FAKE}, {"onehot": FAKE, "dz": None}, {"codes": FAKE, "ls": None},
               {"logits": odd}, {"probs": odd}, {"onehot": odd}, {"onehot": FAKE, "dz": odd},
               {"C_": 4, "logits": half}, {"C_": 8, "probs": half}, {"C_": 4, "onehot": half},
               {"C_": 8, "codes": FAKE, "dz": half}):
        assert ce(**kw) == 1, kw
        assert lib.depgan_last_error(), kw
    # the four-class entry is a call of the new one
    assert lib.depgan_op_softmax_ce4(None, None, FAKE, None, None, 64, None) == 1
    assert lib.depgan_op_softmax_ce4(half, None, FAKE, None, None, 64, None) == 1


def test_head_softmax_k_refuses_its_arguments_before_any_hip_call(lib):
    def head(a=FAKE, ld=32, w=FAKE, b=FAKE, p=FAKE, lg=None, P=64, C_=32, K=3):
        return lib.depgan_op_head_softmax_k_bf16s(a, ld, w, b, p, lg, P, C_, K, None)
    for kw in ({"a": None}, {"w": None}, {"b": None}, {"p": None}, {"P": 0}, {"C_": 0}, {"C_": 24}, {"C_": 1024},
               {"ld": 24}, {"ld": 36}, {"K": 1}, {"K": 9}, {"K": 0}, {"a": C.c_void_p(0x1008)}, {"w": C.c_void_p(0x1002)},
               {"p": C.c_void_p(0x1002)}, {"lg": C.c_void_p(0x1002)}, {"K": 4, "p": C.c_void_p(0x1008)},
               {"K": 8, "w": C.c_void_p(0x1004)}, {"K": 8, "lg": C.c_void_p(0x1004)}):
        assert head(**kw) == 1, kw
        assert lib.depgan_last_error(), kw


@pytest.mark.parametrize("c", [9, -1, 127])
def test_create_refuses_a_class_count_outside_the_range(lib, c):
    """The range check of depgan_create comes before any allocation: status 1 with the range in the message."""
    cfg = _lib.Config(batch=1, height=16, width=16, nicg=1, first_fm=32, nc_out=c)
    h = C.c_void_p()
    assert lib.depgan_create(C.byref(cfg), C.byref(h)) == 1
    assert b"[2, 8]" in lib.depgan_last_error() and not h.value
