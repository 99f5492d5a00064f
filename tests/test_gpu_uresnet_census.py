"""GPU: the class census of the DEP-UResNet path through the C ABI, the Engine and the Keras-style facade, at 64 x 64 x 1
with batch 4 fed a short batch of 3 (weights and batches as tests/test_gpu_uresnet_classes.py builds them).

Every check is exact: the census is a table of integers counted in the loss kernel, and switching it on must not move a
bit of the loss, of a gradient or of the optimiser's state."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_uresnet_classes import IMG, _arenas, _batch, _engine, _params, _u32  # noqa: E402

pytestmark = pytest.mark.gpu
B, N = 4, 3
NPIX = N * IMG * IMG


def _table(codes, probs, Cc):
    """The NumPy confusion matrix: row = code, column = first arg-max of the probabilities; codes >= Cc are in no bin."""
    codes, probs = np.asarray(codes).reshape(-1), np.asarray(probs).reshape(-1, Cc)
    keep = codes < Cc
    cm = np.zeros((Cc, Cc), np.int64)
    np.add.at(cm, (codes[keep].astype(np.int64), np.argmax(probs[keep], -1)), 1)
    return cm


@pytest.mark.parametrize("Cc,sparse", [(4, False), (3, True)])
def test_the_census_changes_nothing_it_does_not_own(lib, Cc, sparse):
    """Two engines with the same weights, one with the census on: grads, two steps, eval."""
    from dep_gan_im_amd import _lib
    ds = 77
    Pm = _params(5, Cc)
    x, z, codes, onehot = _batch(9, N, Cc)
    lab = codes if sparse else onehot
    plain, cen = _engine(B, Pm, Cc), _engine(B, Pm, Cc)
    assert not cen.census
    cen.set_census(True)
    assert cen.census and not plain.census
    assert cen.uresnet(x, z, lab, "grads", drop_seed=ds) == plain.uresnet(x, z, lab, "grads", drop_seed=ds)
    assert int(cen.uresnet_census().sum()) == NPIX
    ga, gb = plain.get_grads("G"), cen.get_grads("G")
    assert list(ga) == list(gb) and any(float(np.abs(v).max()) > 0 for v in gb.values())
    for k in ga:
        assert np.array_equal(_u32(ga[k]), _u32(gb[k])), k
    for step in range(2):
        assert (cen.uresnet(x, z, lab, "step", drop_seed=ds + step)
                == plain.uresnet(x, z, lab, "step", drop_seed=ds + step)), step
    assert cen.uresnet(x, z, lab, "eval") == plain.uresnet(x, z, lab, "eval")
    for a, b in zip(_arenas(plain), _arenas(cen)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(plain._arena_np("G", _lib.ARENA_NONTRAINABLE).view(np.uint32),
                          cen._arena_np("G", _lib.ARENA_NONTRAINABLE).view(np.uint32))
    assert plain.adam_step("G") == cen.adam_step("G") == 2
    with pytest.raises(_lib.DepganError, match="census"):
        plain.uresnet_census()
    plain.close()
    cen.close()


@pytest.mark.parametrize("Cc,sparse", [(4, True), (3, False), (5, True)])
def test_eval_and_training_census_against_numpy(lib, Cc, sparse):
    from dep_gan_im_amd import evaluate
    Pm = _params(5, Cc)
    x, z, codes, onehot = _batch(9, N, Cc)
    lab = codes if sparse else onehot
    eng = _engine(B, Pm, Cc)
    eng.set_census(True)
    # phase 0: u_eval and the predict path share their forward, so the census is the arg-max of g_forward
    probs0 = eng.g_forward(x, z).cpu().numpy()
    eng.uresnet(x, z, lab, "eval")
    ev = eng.uresnet_census()
    assert ev.dtype == np.int64 and ev.shape == (Cc, Cc)
    assert np.array_equal(ev, _table(codes, probs0, Cc)) and int(ev.sum()) == NPIX
    assert np.array_equal(ev.sum(1), np.bincount(codes.reshape(-1), minlength=Cc))
    if Cc == 4:
        # the reference-derived evaluation on the same probabilities: (#both, #real, #fake) of codes 1, 2, 3
        counts = evaluate.label_census(torch.from_numpy(probs0.astype(np.float64)).cuda(), code_real=codes.astype(np.float32))
        for k in (1, 2, 3):
            assert counts[3 * k:3 * k + 3] == [int(ev[k, k]), int(ev[k].sum()), int(ev[:, k].sum())], k
        m = evaluate.confusion_metrics(ev)
        ref = evaluate.label_metrics_from_census(counts, 1.0)
        assert [float(v) for v in m["dice"][1:]] == ref["dice"][:3] and m["mean_dice"] == ref["avg_all_dice"]
    # phase 1: the probabilities the loss of that very call was taken from
    eng.uresnet(x, z, lab, "grads", drop_seed=77)
    tr = eng.uresnet_census()
    probs1 = eng.debug_tensor("g/probs")
    assert probs1.shape == (B, IMG, IMG, Cc)
    assert np.array_equal(tr, _table(codes, probs1[:N], Cc)) and int(tr.sum()) == NPIX
    assert not np.array_equal(tr, ev)              # a census that ignored the learning phase would repeat the eval table
    assert not np.array_equal(_u32(probs1[:N]), _u32(probs0))
    eng.close()


def test_a_refused_sparse_step_still_reports_its_census(lib):
    from dep_gan_im_amd import _lib
    Cc = 3
    Pm = _params(5, Cc)
    x, z, codes, _ = _batch(7, N, Cc)
    eng = _engine(B, Pm, Cc)
    eng.set_census(True)
    eng.uresnet(x, z, codes, "step", drop_seed=3)
    before, step = _arenas(eng), eng.adam_step("G")
    bad = codes.copy()
    bad[1, 17, 40] = Cc
    with pytest.raises(_lib.DepganError, match="1 of %d" % NPIX):
        eng.uresnet(x, z, bad, "step", drop_seed=4)
    for a, b in zip(before, _arenas(eng)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert eng.adam_step("G") == step == 1
    cm = eng.uresnet_census()
    assert int(cm.sum()) == NPIX - 1
    assert np.array_equal(cm, _table(bad, eng.debug_tensor("g/probs")[:N], Cc))
    eng.close()


def test_last_census_status_and_refusals(lib):
    from dep_gan_im_amd import Engine
    Cc = 3
    x, z, codes, _ = _batch(7, N, Cc)
    eng = _engine(B, _params(5, Cc), Cc)
    out, k = (C.c_longlong * 64)(), C.c_int(0)
    last = lambda: lib.depgan_uresnet_last_census(eng.h, out, C.byref(k))      # noqa: E731
    assert lib.depgan_uresnet_get_census(eng.h) == 0
    assert last() == 1 and b"census" in lib.depgan_last_error()
    eng.uresnet(x, z, codes, "eval")                                           # a call with the census off leaves none
    assert last() == 1
    for v in (2, -1):
        assert lib.depgan_uresnet_set_census(eng.h, v) == 1 and b"depgan_uresnet_set_census" in lib.depgan_last_error()
    assert lib.depgan_uresnet_set_census(eng.h, 1) == 0 and lib.depgan_uresnet_get_census(eng.h) == 1
    assert last() == 1                                                          # on, but no call yet
    eng.uresnet(x, z, codes, "eval")
    assert last() == 0 and k.value == Cc and sum(out[:Cc * Cc]) == NPIX
    assert lib.depgan_uresnet_last_census(eng.h, out, None) == 0
    assert lib.depgan_uresnet_last_census(eng.h, None, C.byref(k)) == 1
    assert lib.depgan_uresnet_set_census(eng.h, 0) == 0 and lib.depgan_uresnet_get_census(eng.h) == 0
    assert last() == 1
    eng.close()
    # the inference context has no labels: status 3 before any launch, the setting named
    inf = Engine(B, IMG, IMG, 1, nc_out=Cc, bf16_mfma=True)
    assert lib.depgan_uresnet_set_census(inf.h, 1) == 3
    msg = lib.depgan_last_error()
    assert b"depgan_uresnet_set_census" in msg and b"inference context" in msg, msg
    assert lib.depgan_uresnet_set_census(inf.h, 0) == 0 and lib.depgan_uresnet_get_census(inf.h) == 0
    with pytest.raises(ValueError, match="inference"):
        inf.set_census(True)
    inf.close()
    # the tanh generator has no softmax head
    gan = Engine(B, IMG, IMG, 1)
    assert lib.depgan_uresnet_set_census(gan.h, 1) == 1
    msg = lib.depgan_last_error()
    assert b"depgan_uresnet_set_census" in msg and b"nc_out" in msg, msg
    shape = (C.c_int * 4)()
    assert lib.depgan_debug_tensor(gan.h, b"g/probs", None, 0, shape) == 1 and b"g/probs" in lib.depgan_last_error()
    gan.close()


def test_facade_metrics_in_float_equality(lib):
    """compile(metrics=['acc', 'dice']) and fit for two epochs of 7 samples at batch 4 with validation data."""
    from dep_gan_im_amd import Gen_UNet2D, evaluate
    Cc = 3
    x, z, codes, _ = _batch(21, 7, Cc)
    vx, vz, vcodes, _ = _batch(22, 3, Cc)

    def run(metrics):
        net = Gen_UNet2D((IMG, IMG, 1), nc_out=Cc, seed=3).compile(loss="sparse_categorical_crossentropy", metrics=metrics)
        np.random.seed(11)
        return net, net.fit([x, z], codes, epochs=2, batch_size=4, shuffle=True, validation_data=([vx, vz], vcodes),
                            verbose=0)

    net, h = run(["acc", "dice"])
    assert list(h.history) == ["loss", "acc", "dice", "val_loss", "val_acc", "val_dice"]
    assert all(len(v) == 2 for v in h.history.values())
    for e in range(2):
        tr, va = h.census["train"][e], h.census["val"][e]
        assert int(tr.sum()) == 7 * IMG * IMG and int(va.sum()) == 3 * IMG * IMG
        assert np.array_equal(tr.sum(1), np.bincount(codes.reshape(-1), minlength=Cc))
        mt, mv = evaluate.confusion_metrics(tr), evaluate.confusion_metrics(va)
        assert h.history["acc"][e] == mt["accuracy"] and h.history["dice"][e] == mt["mean_dice"]
        assert h.history["val_acc"][e] == mv["accuracy"] and h.history["val_dice"][e] == mv["mean_dice"]
    # after the second epoch: the metrics of the NumPy table of predict on the validation set
    want = evaluate.confusion_metrics(_table(vcodes, net.predict([vx, vz], batch_size=4), Cc))
    assert h.history["val_acc"][1] == want["accuracy"] and h.history["val_dice"][1] == want["mean_dice"]
    out = net.evaluate([vx, vz], vcodes, batch_size=4)
    assert out == [h.history["val_loss"][1], want["accuracy"], want["mean_dice"]]
    tb = net.test_on_batch([vx, vz], vcodes)                 # its loss is not weighted and divided again
    assert tb[1:] == out[1:] and abs(tb[0] - out[0]) <= 1e-6 * abs(out[0])
    # without metrics: the history of today, the same losses included
    net0, h0 = run(None)
    assert sorted(h0.history) == ["loss", "val_loss"] and not hasattr(h0, "census")
    assert h0.history["loss"] == h.history["loss"] and h0.history["val_loss"] == h.history["val_loss"]
    assert isinstance(net0.evaluate([vx, vz], vcodes, batch_size=4), float)
    assert all(np.array_equal(_u32(u), _u32(v)) for u, v in zip(net.get_weights(), net0.get_weights()))
