"""GPU: the DEP-UResNet's boundary loss (depgan_uresnet_set_boundary_loss) through the C ABI and the Keras-style facade,
at 64 x 64 x 1, engines of batch 4 fed 3 samples, with the helpers the Dice model test imports.

Exact statements are bit for bit: a context that set the mode and turned it off against one that never set it, class
codes with an ignored frame against one-hot labels with all-zero rows (class weights and Dice on), another
boundary_coef between steps against a context created with it, an all-ignored batch through step.  Against the float64
oracle (tests/boundary_ref.py restates the oracle's gradient and Adam lines with the boundary term added) the criteria
and the weight-seed rule are those of test_gpu_uresnet_dice_loss.test_dice_loss_against_the_oracle: seed 5 unless the
float32 ORACLE's own count of tensors above 1e-4 (under the HIP pass's decisions) exceeds 4, then the next of 6, 7, 8, 9;
the per-tensor cap is 4 x the fp32 oracle's own worst."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boundary_ref as BR  # noqa: E402
import dice_ref as D  # noqa: E402
import weighted_ce_ref as R  # noqa: E402
from test_gpu_uresnet_classes import IMG, _arenas, _batch, _engine, _params  # noqa: E402
from test_gpu_uresnet_loss_weights import BORDER, _framed, _nontrainable, _same_state  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 5
SPACING = (0.9375, 0.9375)


def _phi_ref(labels, Cc, ignore=-1, spacing=SPACING, off=0.0, coef=None):
    on = None if coef is None else [1 if c != 0 else 0 for c in coef]
    return BR.signed_distance(BR.true_class(labels, Cc, ignore), Cc, spacing, off, on)


def test_mode_set_and_turned_off_equals_a_context_that_never_set_it(lib):
    """1. loss, gradients, the arenas after two steps and eval, bit for bit; the getters follow the setting; the term is
    what the formula gives on the stored probabilities; refusals leave the setting."""
    from dep_gan_im_amd import _lib
    B, n, ds = 4, 3, 77
    Pm = _params(5, 4)
    x, z, codes, onehot = _batch(9, n, 4)
    plain, toggled = _engine(B, Pm, 4), _engine(B, Pm, 4)
    assert toggled.boundary_loss is None
    coef = [0.0, 1.0, 2.0, 0.5]
    toggled.set_boundary_loss(True, weight=0.25, class_coef=coef, spacing=SPACING, inside_offset=0.5)
    got = toggled.boundary_loss
    assert got["weight"] == 0.25 and np.array_equal(got["class_coef"], np.array(coef, np.float32))
    assert got["spacing"] == SPACING and got["inside_offset"] == 0.5
    with pytest.raises(Exception, match="boundary loss on"):
        toggled.uresnet_boundary_loss()
    base = plain.uresnet(x, z, codes, "eval")
    with_b = toggled.uresnet(x, z, codes, "eval")
    lb, M = toggled.uresnet_boundary_loss()
    assert M == n * IMG * IMG and lb != 0.0
    # eval: the other terms + boundary_coef L_B (float32 on the host), L_B from predict's own probabilities
    assert with_b == float(np.float32(base) + np.float32(0.25) * np.float32(lb))
    p = plain.g_forward(x, z).cpu().numpy().astype(np.float64).reshape(-1, 4)
    phi = _phi_ref(codes, 4, off=0.5, coef=coef).reshape(-1, 4)
    _, want, _, scale = BR.boundary_np(p, phi, np.ones(len(p)), np.array(coef, np.float32))
    assert abs(lb - want) <= 1e-5 * scale, (lb, want, scale)
    assert toggled.last_sums()[:2] == plain.last_sums()[:2]                  # the cross-entropy's sum and denominator
    assert toggled.uresnet(x, z, codes, "grads", drop_seed=ds) != plain.uresnet(x, z, codes, "grads", drop_seed=ds)
    # refusals: before any launch, and the setting stays
    for kw in ({"class_coef": [1.0, 1.0, 1.0]}, {"class_coef": [0.0] * 4}, {"class_coef": [1.0, float("nan"), 1.0, 1.0]},
               {"class_coef": [1.0, -1.0, 1.0, 1.0]}, {"weight": -1.0}, {"weight": float("inf")}, {"spacing": (0.0, 1.0)},
               {"spacing": (1.0, float("nan"))}, {"inside_offset": -0.1}, {"inside_offset": 1.1},
               {"spacing": (0.5, 1.0), "inside_offset": 0.6}):
        with pytest.raises(_lib.DepganError):
            toggled.set_boundary_loss(True, **kw)
        now = toggled.boundary_loss
        assert np.array_equal(now["class_coef"], got["class_coef"]), kw
        assert all(now[k] == got[k] for k in ("weight", "spacing", "inside_offset")), kw
    toggled.set_boundary_loss(True, weight=0.5)
    with pytest.raises(Exception, match="boundary loss on"):
        toggled.uresnet_boundary_loss()                                    # status 1 after the mode was set again
    toggled.set_boundary_loss(False)
    assert toggled.boundary_loss is None
    toggled.set_weights("G", Pm)
    fresh = _engine(B, Pm, 4)
    for labels in (codes, onehot):
        assert toggled.uresnet(x, z, labels, "grads", drop_seed=ds) == fresh.uresnet(x, z, labels, "grads", drop_seed=ds)
        _same_state(fresh, toggled, Pm)
    for step in range(2):
        assert (toggled.uresnet(x, z, codes, "step", drop_seed=ds + step)
                == fresh.uresnet(x, z, codes, "step", drop_seed=ds + step)), step
    for a, b in zip(_arenas(fresh), _arenas(toggled)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert toggled.uresnet(x, z, codes, "eval") == fresh.uresnet(x, z, codes, "eval")
    for e in (plain, toggled, fresh):
        e.close()


def test_codes_with_an_ignored_frame_equal_zero_rows(lib):
    """2. class weights, Dice and the boundary term on: class codes with ignore_label = 255 on the frame against one-hot
    labels whose frame rows are all zero -- loss, gradients, the weights after two steps, L_B and M, eval."""
    B, n, ds = 4, 3, 77
    Pm = _params(5, 4)
    x, z, codes, _ = _batch(9, n, 4)
    marked = _framed(codes)
    onehot = R.onehot_rows(marked, 4, 255)
    cw = [0.5, 4.0, 2.0, 1.5]
    sparse, dense = _engine(B, Pm, 4), _engine(B, Pm, 4)
    for e, ign in ((sparse, 255), (dense, None)):
        e.set_loss_weights(cw, ignore_label=ign)
        e.set_dice_loss("class", class_coef=D.class_coef(4, "foreground"))
        e.set_boundary_loss(True, weight=0.1, class_coef=BR.class_coef(4, "foreground"), spacing=SPACING)
    assert sparse.uresnet(x, z, marked, "grads", drop_seed=ds) == dense.uresnet(x, z, onehot, "grads", drop_seed=ds)
    _same_state(dense, sparse, Pm)
    inner = n * (IMG - 2 * BORDER) ** 2
    assert sparse.uresnet_boundary_loss() == dense.uresnet_boundary_loss() and sparse.uresnet_boundary_loss()[1] == inner
    for step in range(2):
        assert (sparse.uresnet(x, z, marked, "step", drop_seed=ds + step)
                == dense.uresnet(x, z, onehot, "step", drop_seed=ds + step)), step
    for a, b in zip(_arenas(dense), _arenas(sparse)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert sparse.adam_step("G") == dense.adam_step("G") == 2
    assert sparse.uresnet(x, z, marked, "eval") == dense.uresnet(x, z, onehot, "eval")
    # eval = the other terms + boundary_coef L_B
    lb, M = sparse.uresnet_boundary_loss()
    sparse.set_boundary_loss(False)
    others = sparse.uresnet(x, z, marked, "eval")
    assert dense.uresnet(x, z, onehot, "eval") == float(np.float32(others) + np.float32(0.1) * np.float32(lb))
    sparse.close()
    dense.close()


def test_another_coefficient_between_steps_equals_a_context_created_with_it(lib):
    """3. a schedule: a context that ran at 0.01 and was then set to 0.3 equals, bit for bit from the same weights, a
    context created with 0.3 -- the gradients, then two steps and the arenas."""
    B, n, ds = 4, 3, 77
    Pm = _params(5, 4)
    x, z, codes, _ = _batch(9, n, 4)
    sched, made = _engine(B, Pm, 4), _engine(B, Pm, 4)
    sched.set_boundary_loss(True, weight=0.01, class_coef=BR.class_coef(4, "foreground"), spacing=SPACING)
    made.set_boundary_loss(True, weight=0.3, class_coef=BR.class_coef(4, "foreground"), spacing=SPACING)
    a = sched.uresnet(x, z, codes, "grads", drop_seed=ds)
    sched.set_boundary_loss(True, weight=0.3, class_coef=BR.class_coef(4, "foreground"), spacing=SPACING)
    sched.set_weights("G", Pm)                                             # the moving statistics moved: start alike
    b = sched.uresnet(x, z, codes, "grads", drop_seed=ds)
    assert b == made.uresnet(x, z, codes, "grads", drop_seed=ds) and a != b
    _same_state(made, sched, Pm)
    for step in range(2):
        assert (sched.uresnet(x, z, codes, "step", drop_seed=ds + step)
                == made.uresnet(x, z, codes, "step", drop_seed=ds + step)), step
    for u, v in zip(_arenas(made), _arenas(sched)):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    sched.close()
    made.close()


def test_all_ignored_batch_applies_no_update(lib):
    """4. every pixel ignored: loss 0.0, L_B 0.0 with M = 0, arenas and Adam counter unchanged, zero gradients."""
    B, n = 4, 3
    Pm = _params(5, 4)
    x, z, codes, _ = _batch(7, n, 4)
    eng = _engine(B, Pm, 4)
    eng.set_loss_weights(None, ignore_label=255)
    eng.set_boundary_loss(True, weight=0.5, spacing=SPACING)
    eng.uresnet(x, z, codes, "step", drop_seed=3)                          # a non-trivial Adam state first
    before, step, nt = _arenas(eng), eng.adam_step("G"), _nontrainable(eng)
    assert step == 1 and eng.uresnet_boundary_loss()[1] == n * IMG * IMG
    nothing = np.full_like(codes, 255)
    assert eng.uresnet(x, z, nothing, "step", drop_seed=4) == 0.0
    assert eng.uresnet_boundary_loss() == (0.0, 0)
    for a, b in zip(before, _arenas(eng)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert eng.adam_step("G") == step
    assert not np.array_equal(nt, _nontrainable(eng))
    assert all(float(np.abs(v).max()) == 0.0 for v in eng.get_grads("G").values())
    assert eng.uresnet(x, z, nothing, "eval") == 0.0 and eng.uresnet(x, z, nothing, "grads", drop_seed=5) == 0.0
    eng.uresnet(x, z, codes, "step", drop_seed=6)
    assert eng.adam_step("G") == step + 1
    eng.close()


def test_boundary_loss_against_the_oracle(lib):
    """5. C = 4, cross-entropy 1 + the foreground boundary term under balanced class weights and the ignored frame: the
    phase-0 loss, one gradient evaluation under the HIP pass's own decisions and one Adam step against the float64
    restatement; criteria and seed rule of test_gpu_uresnet_dice_loss.test_dice_loss_against_the_oracle.

    The first device run printed (seed 5 kept), tensors above 1e-4 (HIP / the fp32 oracle under the same decisions): 0 / 0,
    worst tensor 2.92e-5 on dense_noise_2_mul_m3/kernel (the oracle's fp32 worst 5.63e-5, so the per-tensor cap is
    2.25e-4), phase-0 loss 3.871893 and phase-1 loss 3.882008 (L_B 2.493850), both the float64 figures to the six digits
    printed."""
    import test_gpu_masked as TM
    from dep_gan_im_amd import data
    B, n, ds, Cc = 4, 3, 77, 4
    Pm = _params(SEED, Cc)
    x, z, codes, _ = _batch(6, n, Cc)
    eng = _engine(B, Pm, Cc)
    labels = _framed(codes)
    onehot = R.onehot_rows(labels, Cc, 255)
    cw = data.balanced_class_weights(data.class_counts(labels, Cc, ignore_label=255), "inverse").astype(np.float32)
    eng.set_loss_weights(cw, ignore_label=255)
    coef = BR.class_coef(Cc, "foreground")
    eng.set_boundary_loss(True, weight=1.0, class_coef=coef, spacing=SPACING)
    boundary = {"coef": 1.0, "class_coef": coef, "phi": _phi_ref(labels, Cc, 255, coef=coef)}
    # the maps the library computes are the restatement's, bit for bit
    dev_phi = data.signed_distance_maps(labels, Cc, SPACING, ignore_label=255, classes=[1, 2, 3]).cpu().numpy()
    assert np.array_equal(dev_phi.view(np.uint32), boundary["phi"].view(np.uint32))
    want0 = BR.uresnet_eval_boundary(Pm, x, z, onehot, cw, None, boundary)
    ev = eng.uresnet(x, z, labels, "eval")
    assert abs(ev - want0) < 1e-4 * max(1.0, abs(want0)), (ev, want0)
    loss = eng.uresnet(x, z, labels, "grads", drop_seed=ds)
    G = eng.get_grads("G")
    masks = TM.hip_uresnet_masks(eng, n)
    loss64, g64, _ = BR.uresnet_grads_boundary(Pm, x, z, onehot, cw, None, boundary, drop_seed=ds, dtype=torch.float64,
                                               masks=masks)
    _, g32, _ = BR.uresnet_grads_boundary(Pm, x, z, onehot, cw, None, boundary, drop_seed=ds, dtype=torch.float32,
                                          masks=masks)
    errs, errs32 = TM.tensor_errors(G, g64), TM.tensor_errors(g32, g64)
    worst = max(errs, key=errs.get)
    print("ce+boundary(foreground), C = %d, seed %d: phase-0 loss %.6f (fp64 %.6f); loss %.6f (fp64 %.6f); L_B %.6f; worst "
          "tensor %s %.2e (the oracle's own fp32 run: %.2e there, %.2e at its worst); tensors above 1e-4: HIP %d, fp32 "
          "oracle %d" % (Cc, SEED, ev, want0, loss, loss64, eng.uresnet_boundary_loss()[0], worst, errs[worst],
                         errs32[worst], max(errs32.values()), sum(e > 1e-4 for e in errs.values()),
                         sum(e > 1e-4 for e in errs32.values())))
    assert abs(loss - loss64) < 1e-5 * max(1.0, abs(loss64)), (loss, loss64)
    assert sum(e > 1e-4 for e in errs32.values()) <= 4, "the seed rule: take the next weight seed"
    cap = max(1e-4, 4.0 * max(errs32.values()))
    for k in errs:
        assert errs[k] < cap, (k, errs[k], errs32[k])
    assert sum(e > 1e-4 for e in errs.values()) <= 8, sorted(errs.items(), key=lambda kv: -kv[1])[:10]
    assert any(float(np.abs(v).max()) > 0 for v in G.values())
    # one step against the Adam restatement under the step's decisions
    eng.set_weights("G", Pm)
    got = eng.uresnet(x, z, labels, "step", drop_seed=ds)
    tr = BR.BoundaryOracleUResNet({k: v.copy() for k, v in Pm.items()}, cw, None, boundary, dtype=torch.float64)
    want = tr.train_on_batch([x, z], onehot, drop_seed=ds, masks=TM.hip_uresnet_masks(eng, n))
    assert abs(got - want) < 1e-5 * max(1.0, abs(want)), (got, want)
    W = eng.get_weights("G")
    for k in Pm:
        if "moving_" in k:
            np.testing.assert_allclose(W[k], tr.P[k], rtol=1e-4, atol=1e-6, err_msg=k)
        else:
            assert float(np.abs(W[k] - Pm[k]).max()) <= 1.05e-4, k
    assert eng.adam_step("G") == 1
    eng.close()


def test_facade_boundary_loss(lib):
    """6. compile(boundary_loss=True), train_on_batch, and fit with the scheduler and an Augmenter for two epochs at
    32 x 32: history['boundary_weight'] as scheduled; without the arguments the history keys are what they were."""
    from dep_gan_im_amd import Gen_UNet2D, callbacks, data
    S = 32
    rng = np.random.default_rng(21)
    x = rng.standard_normal((3, S, S, 1)).astype(np.float32)
    z = rng.standard_normal((3, 32, 1)).astype(np.float32)
    codes = np.zeros((3, S, S), np.uint8)
    codes[:, 8:20, 10:24] = 1
    codes[:, 22:28, 4:9] = 2
    codes[:, :2] = 255
    net = Gen_UNet2D((S, S, 1), nc_out=3, seed=3).compile(
        loss="sparse_categorical_crossentropy", ignore_label=255, dice_loss="class", dice_classes="foreground",
        focal_gamma=1.0, metrics=["dice"], boundary_loss=True, boundary_weight=0.01, boundary_classes="foreground",
        boundary_spacing=SPACING)
    first = net.train_on_batch([x, z], codes, drop_seed=0)
    assert np.isfinite(first[0]) and net._engine.boundary_loss["weight"] == float(np.float32(0.01))
    lb, M = net._engine.uresnet_boundary_loss()
    assert M == 3 * (S - 2) * S and np.isfinite(lb)
    sched = callbacks.BoundaryWeightScheduler(lambda epoch, w: 0.01 + 0.02 * epoch)
    aug = data.Augmenter(rotate=10.0, shift=2.0, border="constant", label_fill=255, seed=4)
    h = net.fit([x, z], codes, epochs=2, batch_size=4, shuffle=False, validation_data=([x, z], codes), verbose=0,
                augment=aug, callbacks=[sched])
    assert h.history["boundary_weight"] == [0.01, 0.03] and net.boundary_weight == 0.03
    assert net._engine.boundary_loss["weight"] == float(np.float32(0.03))
    assert sorted(h.history) == ["boundary_weight", "dice", "loss", "lr", "val_dice", "val_loss"]
    assert np.isfinite(h.history["loss"]).all() and np.isfinite(h.history["val_loss"]).all()
    net.set_boundary_weight(0.5)
    assert net._engine.boundary_loss["weight"] == 0.5 and net._engine.boundary_loss["spacing"] == SPACING
    # test_on_batch = the same model without the term + weight * L_B
    with_b = net.test_on_batch([x, z], codes)[0]
    lb, _ = net._engine.uresnet_boundary_loss()
    net.compile(loss="sparse_categorical_crossentropy", ignore_label=255, dice_loss="class", dice_classes="foreground",
                focal_gamma=1.0, metrics=["dice"])
    assert net._engine.boundary_loss is None and net.boundary_weight is None
    without = net.test_on_batch([x, z], codes)[0]
    assert with_b == float(np.float32(without) + np.float32(0.5) * np.float32(lb))
    h = net.fit([x, z], codes, epochs=1, batch_size=4, shuffle=False, verbose=0,
                callbacks=[callbacks.LearningRateScheduler(lambda epoch, lr: lr)])
    assert sorted(h.history) == ["dice", "loss", "lr"]                     # no new key without the new arguments
