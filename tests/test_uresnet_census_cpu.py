"""No GPU: the class census of the DEP-UResNet path as far as it can be checked on the host -- the header and the exports,
the operator's refusals before any HIP call, evaluate.confusion_metrics against a brute-force count and against the
reference-derived label metrics, and compile(metrics=...)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dep_gan_im_amd as dg
from dep_gan_im_amd import _lib, evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments
ENTRIES = ["depgan_uresnet_set_census", "depgan_uresnet_get_census", "depgan_uresnet_last_census",
           "depgan_op_softmax_ce_census"]


def test_header_declares_and_library_exports_the_census_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert getattr(lib, name).argtypes, name + " has no argtypes"
    assert _lib._K["DEPGAN_ABI_VERSION"] == 3          # depgan_config did not change
    assert '"g/probs"' in hdr


def test_softmax_ce_census_refuses_its_arguments_before_any_hip_call(lib):
    out = (C.c_longlong * 64)()

    def ce(logits=FAKE, onehot=None, codes=FAKE, probs=FAKE, dz=FAKE, ls=FAKE, cen=out, P=64, C_=3):
        return lib.depgan_op_softmax_ce_census(logits, onehot, codes, probs, dz, ls, cen, P, C_, None)
    # the two refusals of its own: no table to write to, no labels to count against
    assert ce(cen=None) == 1 and b"census_host" in lib.depgan_last_error()
    assert ce(codes=None) == 1 and b"labels" in lib.depgan_last_error()
    assert ce(cen=None, onehot=FAKE, codes=None) == 1 and b"census_host" in lib.depgan_last_error()
    # and those of depgan_op_softmax_ce
    for kw in ({"logits": None}, {"probs": None}, {"P": 0}, {"C_": 1}, {"C_": 9}, {"onehot": FAKE}, {"dz": None},
               {"ls": None}, {"logits": C.c_void_p(0x1002)}, {"C_": 4, "probs": C.c_void_p(0x1008)}):
        assert ce(**kw) == 1, kw
        assert lib.depgan_last_error(), kw


def _brute(true, pred, n):
    cm = np.zeros((n, n), np.int64)
    for t, p in zip(true.tolist(), pred.tolist()):
        cm[t, p] += 1
    return cm


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_confusion_metrics_against_a_brute_force_count(n):
    """Seeded random (true, pred) label arrays; class n-1 has no support and class 1 is never predicted (for two classes
    they are the same class), so an empty row and an empty column are both in the table."""
    rng = np.random.default_rng(100 + n)
    true = rng.integers(0, n - 1, 997) if n > 2 else np.zeros(997, np.int64)
    pred = rng.integers(0, n, 997)
    pred[pred == 1] = 0
    cm = _brute(true, pred, n)
    assert cm[n - 1].sum() == 0 and cm[:, 1].sum() == 0 and cm.sum() == 997
    m = evaluate.confusion_metrics(cm)
    assert m["accuracy"] == float((true == pred).sum()) / 997
    s = 1e-7
    for k in range(n):
        both = int(((true == k) & (pred == k)).sum())
        real, fake = int((true == k).sum()), int((pred == k).sum())
        assert m["support"][k] == real
        assert m["dice"][k] == (both * 2.0 + s) / (s + real + fake)
        assert m["iou"][k] == (both + s) / (real + fake - both + s)
        if fake:
            assert m["precision"][k] == both / fake
        else:
            assert np.isnan(m["precision"][k])
        if real:
            assert m["recall"][k] == both / real
        else:
            assert np.isnan(m["recall"][k])
    np.testing.assert_allclose(m["mean_dice"], np.mean(m["dice"][1:]), rtol=1e-15)
    np.testing.assert_allclose(m["mean_iou"], np.mean(m["iou"][1:]), rtol=1e-15)
    # smooth is a parameter
    assert evaluate.confusion_metrics(cm, smooth=1.0)["dice"][0] == (cm[0, 0] * 2.0 + 1.0) / (1.0 + cm[0].sum() + cm[:, 0].sum())


def test_four_classes_reproduce_the_label_metrics():
    """UE:636-652, 697: the per-class Dice of codes 1 to 3 and their mean are label_metrics_from_census of the same
    (#both, #real, #fake) triples."""
    rng = np.random.default_rng(7)
    true, pred = rng.integers(0, 4, 5000), rng.integers(0, 4, 5000)
    pred[rng.uniform(size=5000) < 0.5] = 0
    cm = _brute(true, pred, 4)
    c = [0] * 18
    for k in (1, 2, 3):
        c[3 * k:3 * k + 3] = [int(cm[k, k]), int(cm[k].sum()), int(cm[:, k].sum())]
    ref = evaluate.label_metrics_from_census(c, 1.0)
    m = evaluate.confusion_metrics(cm)
    assert [float(v) for v in m["dice"][1:]] == ref["dice"][:3]
    assert m["mean_dice"] == ref["avg_all_dice"]


def test_an_empty_table_is_refused():
    with pytest.raises(ValueError, match="empty"):
        evaluate.confusion_metrics(np.zeros((4, 4), np.int64))
    with pytest.raises(ValueError):
        evaluate.confusion_metrics(np.ones((3, 4), np.int64))
    with pytest.raises(ValueError):
        evaluate.confusion_metrics(np.ones((3, 3), np.float32))


def test_compile_takes_the_metric_names():
    m = dg.Gen_UNet2D((64, 64, 1), nc_out=3)
    for names in (["acc"], ["accuracy", "dice", "iou"], ["iou", "acc"], [], None):
        assert m.compile(metrics=names) is m
    assert m._metrics == []                                 # None leaves what was compiled
    m.compile(metrics=["dice"])
    m.compile()
    assert m._metrics == ["dice"]
    for bad in (["mse"], ["acc", "f1"], ["acc", "acc"], [3]):
        with pytest.raises(ValueError, match="acc.*accuracy.*dice.*iou"):
            m.compile(metrics=bad)
    with pytest.raises(RuntimeError, match="tanh"):
        dg.Gen_UNet2D((64, 64, 1)).compile(metrics=["acc"])                       # nc_out = 1
    with pytest.raises(RuntimeError, match="inference"):
        dg.Gen_UNet2D((64, 64, 1), nc_out=3).inference_copy().compile(metrics=["acc"])


class _FakeEngine:
    """What fit, evaluate and the batch calls need of an Engine: a loss per call and a census when it is on."""
    batch = 4

    def __init__(self):
        self.census_on, self.calls = False, []

    def set_census(self, on=True):
        self.census_on = bool(on)

    def uresnet(self, x, z, labels, mode="step", drop_seed=0):
        self.calls.append((mode, len(x)))
        return 0.5 + 0.125 * len(self.calls)

    def uresnet_census(self):
        assert self.census_on, "the census was read without being switched on"
        n = self.calls[-1][1]
        return np.array([[5 * n, n, 0], [0, 2 * n, n], [n, 0, n]], np.int64)


def _fit(monkeypatch, metrics):
    eng = _FakeEngine()
    monkeypatch.setattr(dg.models.GeneratorModel, "_ensure_engine", lambda self, batch=32: eng)
    n, H = 7, 64
    x, z = np.zeros((n, H, H, 1), np.float32), np.zeros((n, 32, 1), np.float32)
    codes = np.zeros((n, H, H), np.int64)
    m = dg.Gen_UNet2D((H, H, 1), nc_out=3).compile(loss="sparse_categorical_crossentropy", metrics=metrics)
    if metrics:
        eng.set_census(True)                               # what _bind does on a real engine
    lines = []
    h = m.fit([x, z], codes, epochs=2, batch_size=4, shuffle=False, validation_data=([x[:3], z[:3]], codes[:3]),
              print_fn=lines.append)
    return m, eng, h, lines, (x, z, codes)


def test_fit_without_metrics_keeps_its_history_keys_and_lines(monkeypatch):
    m, eng, h, lines, (x, z, codes) = _fit(monkeypatch, None)
    assert sorted(h.history) == ["loss", "val_loss"] and not hasattr(h, "census")
    assert all(len(v) == 2 for v in h.history.values())
    assert lines[0] == "Epoch 1/2 - loss: %.4f - val_loss: %.4f" % (h.history["loss"][0], h.history["val_loss"][0])
    assert isinstance(m.evaluate([x, z], codes, batch_size=4), float)
    assert isinstance(m.train_on_batch([x[:2], z[:2]], codes[:2]), float)
    assert isinstance(m.test_on_batch([x[:2], z[:2]], codes[:2]), float)
    assert not eng.census_on


def test_fit_with_metrics_records_them_from_the_summed_tables(monkeypatch):
    m, eng, h, lines, (x, z, codes) = _fit(monkeypatch, ["acc", "dice"])
    assert list(h.history) == ["loss", "acc", "dice", "val_loss", "val_acc", "val_dice"]
    assert all(len(v) == 2 for v in h.history.values())
    assert [len(h.census["train"]), len(h.census["val"])] == [2, 2]
    unit = np.array([[5, 1, 0], [0, 2, 1], [1, 0, 1]], np.int64)
    assert np.array_equal(h.census["train"][0], 7 * unit) and np.array_equal(h.census["val"][1], 3 * unit)
    want = evaluate.confusion_metrics(7 * unit)
    assert h.history["acc"] == [want["accuracy"]] * 2 and h.history["dice"] == [want["mean_dice"]] * 2
    assert "val_dice: %.4f" % h.history["val_dice"][0] in lines[0] and "census train" in lines[0]
    out = m.evaluate([x, z], codes, batch_size=4)
    assert isinstance(out, list) and len(out) == 3 and out[1:] == [want["accuracy"], want["mean_dice"]]
    assert len(m.train_on_batch([x[:2], z[:2]], codes[:2])) == 3
    assert len(m.test_on_batch([x[:2], z[:2]], codes[:2])) == 3
