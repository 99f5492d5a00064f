"""No GPU: the optimiser options' host side -- the float64 reference of the update rule against hand-computed elements
and against the oracle's KerasAdam, the callbacks' Keras 2 rules on a stub model, and the refusals of compile, of the
facade's setters and of the library's setters where they return before any HIP call."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dep_gan_im_amd as dg  # noqa: E402
import optim_ref as R  # noqa: E402
from dep_gan_im_amd import _lib, callbacks as cbk  # noqa: E402
from dep_gan_im_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments
ENTRIES = ["depgan_set_lr", "depgan_get_lr", "depgan_set_optimizer", "depgan_get_optimizer", "depgan_last_grad_norm",
           "depgan_op_grad_sqnorm", "depgan_op_adam_opts"]
NAN, INF = float("nan"), float("inf")


# ---- the reference ----

def test_reference_on_three_hand_computed_elements():
    """b1 = 0.5, b2 = 0.75, t = 1: lr_t = lr sqrt(0.25) / 0.5 = lr = 0.125; eps = 0.25.  g = (3, -4, 0): norm 5, clipnorm
    2.5 gives s = 0.5 and g' = (1.5, -2, 0); clipvalue 1.75 gives (1.5, -1.75, 0).  weight_decay 0.5 on elements 0 and
    2: p = (2, 2, -4) -> (2 - 0.0625 * 2, 2, -4 + 0.0625 * 4) = (1.875, 2, -3.75).  m = 0.5 g' = (0.75, -0.875, 0),
    v = 0.25 g'^2 = (0.5625, 0.765625, 0), sqrt v = (0.75, 0.875, 0); displacement 0.125 m / (sqrt v + 0.25) =
    (0.09375, -0.875 / 9, 0)."""
    p, m, v, norm, s = R.adam_opts_step([2.0, 2.0, -4.0], [3.0, -4.0, 0.0], np.zeros(3), np.zeros(3), 1, 0.125, 0.5, 0.75,
                                        eps=0.25, clipnorm=2.5, clipvalue=1.75, weight_decay=0.5, decay=[1, 0, 1])
    assert norm == 5.0 and s == 0.5
    assert m.tolist() == [0.75, -0.875, 0.0] and v.tolist() == [0.5625, 0.765625, 0.0]
    assert p[0] == 1.875 - 0.09375 and p[2] == -3.75
    assert abs(p[1] - (2.0 + 0.875 / 9.0)) <= 1e-15
    # below the threshold nothing is scaled; the supplied scale replaces the computed one
    assert R.adam_opts_step([0.0], [3.0], [0.0], [0.0], 1, 0.125, 0.5, 0.75, clipnorm=3.5)[3:] == (3.0, 1.0)
    assert R.adam_opts_step([0.0], [3.0], [0.0], [0.0], 1, 0.125, 0.5, 0.75, clipnorm=3.0)[4] == 1.0     # c / norm = 1
    assert R.adam_opts_step([0.0], [3.0], [0.0], [0.0], 1, 0.125, 0.5, 0.75, clipnorm=1.5, scale=0.25)[1][0] == 0.375
    # a norm that is not finite: nothing moves, scale 0
    for bad in (NAN, INF, -INF):
        p, m, v, norm, s = R.adam_opts_step([1.0, 2.0], [bad, 1.0], [0.5, 0.5], [0.25, 0.25], 3, 0.125, 0.5, 0.75,
                                            clipnorm=1.0, weight_decay=0.5, decay=[1, 1])
        assert p.tolist() == [1.0, 2.0] and m.tolist() == [0.5, 0.5] and v.tolist() == [0.25, 0.25]
        assert s == 0.0 and not math.isfinite(norm)


@pytest.mark.parametrize("b1,b2", [(0.0, 0.9), (0.9, 0.999)])
def test_reference_equals_the_oracle_s_keras_adam_with_every_option_off(b1, b2):
    from oracle import depgan_oracle as O
    rng = np.random.default_rng(2)
    names = ["a/kernel", "a/bias"]
    shapes = {"a/kernel": (3, 3, 2, 5), "a/bias": (5,)}
    # float64 tensors through KerasAdam with the float32 values of the betas: both sides then hold the same constants
    f32 = lambda x: float(np.float32(x))   # noqa: E731
    P = {n: rng.standard_normal(shapes[n]) for n in names}
    opt = O.KerasAdam(names, f32(1e-4), f32(b1), f32(b2), eps=f32(1e-7))
    flat = np.concatenate([P[n].reshape(-1) for n in names])
    p, m, v = flat.copy(), np.zeros_like(flat), np.zeros_like(flat)
    for t in (1, 2, 3):
        G = {n: (rng.standard_normal(shapes[n]) * 10.0 ** rng.uniform(-6, 0)).astype(np.float32) for n in names}
        before = np.concatenate([P[n].reshape(-1) for n in names])
        opt.apply(P, G)
        g = np.concatenate([G[n].reshape(-1) for n in names])
        p0 = p.copy()
        p, m, v, norm, s = R.adam_opts_step(p, g, m, v, t, 1e-4, b1, b2)
        assert (norm, s) == (0.0, 1.0)
        want = np.concatenate([P[n].reshape(-1) for n in names])
        np.testing.assert_allclose(m, np.concatenate([opt.m[n].reshape(-1) for n in names]), rtol=1e-13, atol=0)
        np.testing.assert_allclose(v, np.concatenate([opt.v[n].reshape(-1) for n in names]), rtol=1e-13, atol=0)
        # the oracle keeps lr_t in double, the library (and the reference) round it to float32: 2^-24 of a displacement
        np.testing.assert_allclose(p - p0, want - before, rtol=1e-7, atol=1e-18)


# ---- the callbacks, on a stub model ----

class Stub:
    """What a callback touches of a model."""

    def __init__(self, lr=1.0):
        self._lr, self.stop_training, self.w, self.saved = lr, False, [np.zeros(2)], []

    lr = property(lambda self: self._lr)

    def set_lr(self, lr):
        self._lr = float(lr)

    def get_weights(self):
        return [w.copy() for w in self.w]

    def set_weights(self, w):
        self.w = [np.array(a) for a in w]

    def save_weights(self, path):
        self.saved.append((path, self.w[0][0]))


def _run(cb, values, key="val_loss", model=None, extra=None):
    """fit's calling sequence on scripted monitor values; returns the model and the lr after every epoch."""
    model = model or Stub()
    cb.set_model(model)
    cb.on_train_begin()
    lrs = []
    for ep, val in enumerate(values):
        cb.on_epoch_begin(ep)
        model.w = [np.full(2, float(ep))]                 # the epoch's training
        logs = {key: val, "lr": model.lr}
        logs.update(extra or {})
        cb.on_epoch_end(ep, logs)
        lrs.append(model.lr)
        if model.stop_training:
            break
    cb.on_train_end()
    return model, lrs


def test_reduce_lr_on_plateau_follows_keras_2():
    """patience 2, cooldown 1, factor 0.5, min_lr 0.2, min_delta 0.1, lr 1.  Keras 2's on_epoch_end: in cooldown the
    counter drops and wait = 0; an improvement (current < best - min_delta) resets wait; otherwise, outside cooldown,
    wait += 1 and at wait >= patience lr = max(lr * factor, min_lr), cooldown restarts, wait = 0.
      epoch value  event
      0     1.00   improves on inf: best 1.00                                      lr 1
      1     0.95   not by 0.1: wait 1                                              lr 1
      2     0.91   wait 2 >= 2: lr 0.5, cooldown 1, wait 0                          lr 0.5
      3     0.92   cooldown 1 -> 0, wait 0; no improvement, out of cooldown: wait 1 lr 0.5
      4     0.80   improves (0.80 < 0.90): best 0.80, wait 0                        lr 0.5
      5     0.80   wait 1                                                          lr 0.5
      6     0.75   not by 0.1: wait 2: lr 0.25, cooldown 1                          lr 0.25
      7     0.75   cooldown -> 0, wait 0, then wait 1                               lr 0.25
      8     0.75   wait 2: lr max(0.125, 0.2) = 0.2, cooldown 1                     lr 0.2
      9     0.75   cooldown -> 0, wait 1                                            lr 0.2
      10    0.75   wait 2, but lr is not above min_lr: nothing                      lr 0.2"""
    cb = cbk.ReduceLROnPlateau(factor=0.5, patience=2, cooldown=1, min_lr=0.2, min_delta=0.1)
    _, lrs = _run(cb, [1.0, 0.95, 0.91, 0.92, 0.80, 0.80, 0.75, 0.75, 0.75, 0.75, 0.75])
    assert lrs == [1, 1, 0.5, 0.5, 0.5, 0.5, 0.25, 0.25, 0.2, 0.2, 0.2]
    # the reference's own setting (UT:584): factor 0.2, patience 5 -- five stagnant epochs after the best one
    _, lrs = _run(cbk.ReduceLROnPlateau(monitor="val_loss", factor=0.2, patience=5), [1.0] * 7, model=Stub(1e-4))
    assert lrs[:5] == [1e-4] * 5 and lrs[5] == pytest.approx(2e-5) and lrs[6] == lrs[5]
    with pytest.raises(ValueError, match="factor"):
        cbk.ReduceLROnPlateau(factor=1.0)


def test_mode_auto_maximises_scores():
    # val_dice rises, then stalls: a maximised monitor sees improvements, a minimised one would see none
    _, lrs = _run(cbk.ReduceLROnPlateau(monitor="val_dice", factor=0.5, patience=1, min_delta=0.0),
                  [0.1, 0.2, 0.3, 0.3, 0.3], key="val_dice")
    assert lrs == [1, 1, 1, 0.5, 0.25]
    for name in ("val_acc", "accuracy", "val_iou", "dice"):
        assert cbk.EarlyStopping(monitor=name)._max and cbk.ModelCheckpoint("x", monitor=name)._max
    assert not cbk.EarlyStopping(monitor="val_loss")._max and not cbk.ReduceLROnPlateau(monitor="loss")._max
    assert not cbk.EarlyStopping(monitor="val_dice", mode="min")._max and cbk.EarlyStopping(monitor="loss", mode="max")._max
    with pytest.raises(ValueError, match="mode"):
        cbk.EarlyStopping(mode="best")


def test_early_stopping_epoch_and_restored_weights():
    # best at epoch 2 (0.5); patience 2: epochs 3 and 4 do not improve, fit ends after epoch 4 (counted from 0)
    cb = cbk.EarlyStopping(patience=2, restore_best_weights=True)
    model, lrs = _run(cb, [1.0, 0.8, 0.5, 0.6, 0.5, 0.1, 0.1])
    assert len(lrs) == 5 and cb.stopped_epoch == 4 and model.stop_training
    assert model.w[0].tolist() == [2.0, 2.0]                              # the weights of the best epoch are back
    model, lrs = _run(cbk.EarlyStopping(patience=2), [1.0, 0.8, 0.5, 0.6, 0.5, 0.1])
    assert len(lrs) == 5 and model.w[0].tolist() == [4.0, 4.0]            # without it the last epoch's stay
    # patience 0: the first epoch that does not improve; min_delta: an improvement smaller than it does not count
    assert len(_run(cbk.EarlyStopping(patience=0), [1.0, 1.0, 0.5])[1]) == 2
    assert len(_run(cbk.EarlyStopping(patience=0, min_delta=0.1), [1.0, 0.95, 0.5])[1]) == 2
    assert len(_run(cbk.EarlyStopping(patience=0, min_delta=0.01), [1.0, 0.95, 0.5, 0.5])[1]) == 4
    # baseline: nothing ever beats it, so patience epochs from the start
    assert len(_run(cbk.EarlyStopping(patience=3, baseline=0.1), [1.0, 0.9, 0.8, 0.7, 0.6])[1]) == 3
    # a second fit starts afresh
    model, lrs = _run(cb, [1.0, 2.0, 3.0])
    assert len(lrs) == 3 and cb.stopped_epoch == 2 and model.w[0].tolist() == [0.0, 0.0]


def test_learning_rate_scheduler_and_model_checkpoint(tmp_path):
    seen = []

    def schedule(epoch, lr):
        seen.append((epoch, lr))
        return lr * 0.5
    model, lrs = _run(cbk.LearningRateScheduler(schedule), [1.0, 1.0, 1.0], model=Stub(0.8))
    assert lrs == [0.4, 0.2, 0.1] and seen == [(0, 0.8), (1, 0.4), (2, 0.2)]
    with pytest.raises(ValueError, match="should be float"):
        _run(cbk.LearningRateScheduler(lambda e, lr: "0.1"), [1.0])
    path = str(tmp_path / "w_{epoch:02d}.npz")
    model, _ = _run(cbk.ModelCheckpoint(path, save_best_only=True), [1.0, 0.5, 0.7, 0.5, 0.4])
    assert model.saved == [(str(tmp_path / "w_01.npz"), 0.0), (str(tmp_path / "w_02.npz"), 1.0),
                           (str(tmp_path / "w_05.npz"), 4.0)]
    model, _ = _run(cbk.ModelCheckpoint("w.npz"), [1.0, 2.0, 3.0])
    assert [s[1] for s in model.saved] == [0.0, 1.0, 2.0] and {s[0] for s in model.saved} == {"w.npz"}
    model, _ = _run(cbk.ModelCheckpoint("w.npz", monitor="val_dice", save_best_only=True), [0.1, 0.3, 0.2], key="val_dice")
    assert [s[1] for s in model.saved] == [0.0, 1.0]


@pytest.mark.parametrize("cb", [cbk.ReduceLROnPlateau(), cbk.EarlyStopping(), cbk.ModelCheckpoint("x", save_best_only=True)])
def test_a_missing_monitor_names_the_available_keys(cb):
    with pytest.raises(ValueError) as e:
        _run(cb, [1.0], key="loss", extra={"dice": 0.5})
    assert "'val_loss'" in str(e.value) and "dice, loss, lr" in str(e.value)


# ---- refusals ----

def test_compile_validates_the_optimizer_options():
    m = dg.Gen_UNet2D((64, 64, 1), nc_out=3)
    assert m._opt is None and m.lr == 1e-4 and m.stop_training is False
    assert m.compile(clipnorm=1.0, weight_decay=1e-4) is m
    assert m._opt == {"clipnorm": 1.0, "clipvalue": 0.0, "weight_decay": 1e-4}
    m.compile(clipvalue=np.float32(0.5))
    assert m._opt == {"clipnorm": 0.0, "clipvalue": 0.5, "weight_decay": 0.0}
    m.compile()
    assert m._opt is None
    m.compile(clipnorm=0, clipvalue=0.0, weight_decay=None)
    assert m._opt is None

    class Opt:
        lr, clipnorm, weight_decay = 3e-4, 2.0, 0.01
    m.compile(optimizer=Opt())
    assert m._opt == {"clipnorm": 2.0, "clipvalue": 0.0, "weight_decay": 0.01} and m.lr == 3e-4
    m.compile(optimizer=Opt(), clipnorm=5.0)                                # an argument wins over the attribute
    assert m._opt["clipnorm"] == 5.0 and m._opt["weight_decay"] == 0.01
    for name in ("clipnorm", "clipvalue", "weight_decay"):
        for bad in (-1.0, -1e-9, NAN, INF, -INF, 1e39, True, "1", [1.0]):   # 1e39 is inf as float32
            with pytest.raises(ValueError, match=name):
                m.compile(**{name: bad})
    assert m._opt["clipnorm"] == 5.0                                        # a refused compile leaves the setting
    with pytest.raises(RuntimeError, match="tanh"):
        dg.Gen_UNet2D((64, 64, 1)).compile(clipnorm=1.0)


def test_set_lr_before_an_engine_exists_and_its_refusals():
    m = dg.Gen_UNet2D((64, 64, 1), nc_out=2)
    m.set_lr(2e-3)
    assert m.lr == 2e-3 and m._lr == 2e-3
    m.compile(lr=5e-4)
    assert m.lr == 5e-4
    for bad in (0.0, -1e-4, NAN, INF, 1e-50, True, "1e-4", None):           # 1e-50 is 0 as float32
        with pytest.raises(ValueError, match="lr"):
            m.set_lr(bad)
    assert m.lr == 5e-4
    with pytest.raises(RuntimeError, match="tanh"):
        dg.Gen_UNet2D((64, 64, 1)).set_lr(1e-3)
    for bad in (-1.0, NAN, INF, False):
        with pytest.raises(ValueError, match="clipvalue"):
            Engine._opt_number(bad, "clipvalue", False)
    assert Engine._opt_number(None, "clipnorm", False) == 0.0 and Engine._opt_number(2, "clipnorm", False) == 2.0


def test_fit_takes_callbacks_and_the_engine_has_the_setters():
    import inspect
    sig = inspect.signature(dg.models.GeneratorModel.fit)
    assert sig.parameters["callbacks"].default is None
    sig = inspect.signature(dg.models.GeneratorModel.compile)
    assert [sig.parameters[n].default for n in ("clipnorm", "clipvalue", "weight_decay")] == [None] * 3
    for name in ("set_lr", "lr", "set_optimizer", "optimizer", "grad_norm"):
        assert callable(getattr(Engine, name)), name
    assert "not recorded" in dg.Trainers.save_state.__doc__


def test_header_declares_and_library_exports_the_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert getattr(lib, name).argtypes, name + " has no argtypes"
    assert _lib._K["DEPGAN_ABI_VERSION"] == 3 and lib.depgan_abi_version() == 3       # new entries, the same ABI
    f, vp = C.c_float, C.c_void_p
    assert lib.depgan_set_optimizer.argtypes == [vp, C.c_int, f, f, f]
    assert lib.depgan_set_lr.argtypes == [vp, C.c_int, f]
    assert lib.depgan_op_grad_sqnorm.argtypes == [vp, C.c_long, f, vp, vp]
    assert lib.depgan_op_adam_opts.argtypes == [vp] * 4 + [C.c_long] + [f] * 9 + [vp, vp, C.c_int, vp, vp]


def test_library_setters_refuse_their_arguments_before_any_hip_call(lib):
    for vals in ((-1.0, 0, 0), (0, -1e-3, 0), (0, 0, -0.5), (NAN, 0, 0), (0, NAN, 0), (0, 0, NAN), (INF, 0, 0),
                 (0, INF, 0), (0, 0, INF), (-INF, 1.0, 1.0)):
        for ctx in (None, FAKE):                                       # the values are looked at before the context
            assert lib.depgan_set_optimizer(ctx, _lib.NET_G, *vals) == 1, vals
            msg = lib.depgan_last_error()
            assert [n for n, v in zip((b"clipnorm", b"clipvalue", b"weight_decay"), vals) if not 0 <= v < INF][0] in msg
    for lr in (0.0, -1e-4, NAN, INF, -INF):
        for ctx in (None, FAKE):
            assert lib.depgan_set_lr(ctx, _lib.NET_G, lr) == 1 and b"lr is" in lib.depgan_last_error()
    # without a context
    assert lib.depgan_set_optimizer(None, _lib.NET_G, 1.0, 0.0, 0.0) == 1
    assert lib.depgan_set_lr(None, _lib.NET_G, 1e-4) == 1
    out = C.c_float(-7.0)
    assert lib.depgan_get_lr(None, _lib.NET_G, C.byref(out)) == 1 and out.value == -7.0
    assert lib.depgan_get_optimizer(None, _lib.NET_G, None, None, None) == 0
    assert lib.depgan_last_grad_norm(None, _lib.NET_G, None, None) == 1
    # the operator entries
    sq = C.c_double(-7.0)
    assert lib.depgan_op_grad_sqnorm(None, 8, 1.0, C.byref(sq), None) == 1
    assert lib.depgan_op_grad_sqnorm(FAKE, 0, 1.0, C.byref(sq), None) == 1
    assert lib.depgan_op_grad_sqnorm(FAKE, 8, 1.0, None, None) == 1 and sq.value == -7.0

    def adam(n=8, cn=0.0, cv=0.0, wd=0.0, ends=(8,), flags=(1,), norm=True, p=FAKE):
        e, fl = (C.c_long * len(ends))(*ends), (C.c_int * len(flags))(*flags)
        nh = (C.c_double * 2)() if norm else None
        return lib.depgan_op_adam_opts(p, FAKE, FAKE, FAKE, n, 1e-4, 1e-4, 0.9, 0.999, 1e-7, 1.0, cn, cv, wd, e, fl,
                                       len(ends), nh, None)
    for kw in ({"p": None}, {"n": 0}, {"cn": -1.0}, {"cv": NAN}, {"wd": -1e-3}, {"ends": (4, 4, 8), "flags": (1, 0, 1)},
               {"ends": (5, 3, 8), "flags": (1, 0, 1)}, {"ends": (4, 9), "flags": (1, 0)}, {"ends": (4, 7), "flags": (1, 0)},
               {"ends": (0, 8), "flags": (1, 0)}, {"cn": 1.0, "norm": False}):
        assert adam(**kw) == 1, kw
        assert lib.depgan_last_error(), kw
