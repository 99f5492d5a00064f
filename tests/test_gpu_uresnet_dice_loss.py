"""GPU: the DEP-UResNet's soft Dice loss (depgan_uresnet_set_dice_loss) through the C ABI and the Keras-style facade, at
64 x 64 x 1, engines of batch 4 fed 3 samples.

Exact statements are bit for bit: a context that set the mode and turned it off against one that never set it, class
codes with an ignored frame against one-hot labels with all-zero rows (Dice on), an all-ignored batch through step.
Against the float64 oracle (tests/dice_ref.py restates the oracle's gradient and Adam lines with the combined loss) the
criteria and the seed rule are those of test_gpu_uresnet_loss_weights.test_weighted_loss_against_the_oracle.

test_dice_loss_against_the_oracle, the weight seed per setting.  The rule: seed 5 unless the float32 ORACLE's own count of
tensors above 1e-4 (under the HIP pass's decisions) exceeds 4, then the next of 6, 7, 8, 9.  The figures of the first
device run are recorded in that test's docstring."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dice_ref as D  # noqa: E402
import weighted_ce_ref as R  # noqa: E402
from test_gpu_uresnet_classes import IMG, _arenas, _batch, _engine, _params, _u32  # noqa: E402
from test_gpu_uresnet_loss_weights import BORDER, _framed, _nontrainable, _same_state  # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS = {"ce+foreground": 5, "flat": 5}
SMOOTH = 1e-7


def test_mode_set_and_turned_off_equals_a_context_that_never_set_it(lib):
    """1. loss, gradients and the weights after a step, bit for bit; the getters follow the setting."""
    B, n, ds = 4, 3, 77
    Pm = _params(5, 4)
    x, z, codes, onehot = _batch(9, n, 4)
    plain, toggled = _engine(B, Pm, 4), _engine(B, Pm, 4)
    assert toggled.dice_loss is None
    toggled.set_dice_loss("class", ce_weight=0.5, dice_weight=2.0, smooth=1e-3, class_coef=[0.0, 1.0, 2.0, 0.5])
    got = toggled.dice_loss
    assert got["form"] == "class" and got["ce_weight"] == 0.5 and got["dice_weight"] == 2.0
    assert got["smooth"] == float(np.float32(1e-3)) and np.array_equal(got["class_coef"], np.array([0, 1, 2, 0.5], np.float32))
    with pytest.raises(Exception, match="Dice loss on"):
        toggled.uresnet_dice_sums()
    with_dice = toggled.uresnet(x, z, codes, "grads", drop_seed=ds)
    assert with_dice != plain.uresnet(x, z, codes, "grads", drop_seed=ds)
    s = toggled.uresnet_dice_sums()
    assert np.array_equal(s["true"], np.bincount(codes.reshape(-1), minlength=4)) and s["loss"] > 0
    # depgan_last_sums keeps the cross-entropy's sum and denominator
    assert toggled.last_sums()[:2] == plain.last_sums()[:2] and plain.last_sums()[1] == float(n * IMG * IMG)
    ce_mean = np.float32(plain.last_sums()[0]) / np.float32(plain.last_sums()[1])
    assert abs(with_dice - (0.5 * float(ce_mean) + 2.0 * s["loss"])) <= 1e-6 * with_dice
    toggled.set_dice_loss("flat")
    assert toggled.dice_loss["form"] == "flat" and toggled.dice_loss["class_coef"] is None
    with pytest.raises(Exception, match="Dice loss on"):
        toggled.uresnet_dice_sums()                                        # status 1 after the mode was set again
    toggled.set_dice_loss()
    assert toggled.dice_loss is None
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
    # refusals: before any launch, and the setting stays
    from dep_gan_im_amd import _lib
    for kw in ({"form": "class", "class_coef": [1.0, 1.0, 1.0]}, {"form": "flat", "class_coef": [1.0] * 4},
               {"form": "class", "smooth": 0.0}, {"form": "flat", "dice_weight": 0.0}, {"form": "flat", "ce_weight": -1.0},
               {"form": "class", "class_coef": [0.0] * 4}, {"form": "class", "class_coef": [1.0, float("nan"), 1.0, 1.0]}):
        with pytest.raises(_lib.DepganError):
            toggled.set_dice_loss(**kw)
        assert toggled.dice_loss is None
    with pytest.raises(ValueError, match="form"):
        toggled.set_dice_loss("tversky")
    for e in (plain, toggled, fresh):
        e.close()


def test_codes_with_an_ignored_frame_equal_zero_rows(lib):
    """2. Dice on, class weights on the cross-entropy: class codes with ignore_label = 255 on the frame against one-hot
    labels whose frame rows are all zero -- loss, gradients, the weights after two steps, the Dice sums."""
    B, n, ds = 4, 3, 77
    Pm = _params(5, 4)
    x, z, codes, _ = _batch(9, n, 4)
    marked = _framed(codes)
    onehot = R.onehot_rows(marked, 4, 255)
    cw = [0.5, 4.0, 2.0, 1.5]
    for kw in ({"form": "class", "class_coef": D.class_coef(4, "foreground")}, {"form": "flat", "ce_weight": 0.0}):
        sparse, dense = _engine(B, Pm, 4), _engine(B, Pm, 4)
        sparse.set_loss_weights(cw, ignore_label=255)
        dense.set_loss_weights(cw)
        sparse.set_dice_loss(**kw)
        dense.set_dice_loss(**kw)
        assert sparse.uresnet(x, z, marked, "grads", drop_seed=ds) == dense.uresnet(x, z, onehot, "grads", drop_seed=ds)
        _same_state(dense, sparse, Pm)
        ss, sd = sparse.uresnet_dice_sums(), dense.uresnet_dice_sums()
        for k in ("intersection", "pred", "true"):
            assert np.array_equal(ss[k], sd[k]), k
        assert ss["loss"] == sd["loss"] > 0
        inner = n * (IMG - 2 * BORDER) ** 2
        assert ss["true"].sum() == inner and abs(ss["pred"].sum() - inner) < 1e-3 * inner
        assert np.array_equal(ss["true"], sparse.uresnet_label_counts()["classes"])
        for step in range(2):
            assert (sparse.uresnet(x, z, marked, "step", drop_seed=ds + step)
                    == dense.uresnet(x, z, onehot, "step", drop_seed=ds + step)), step
        for a, b in zip(_arenas(dense), _arenas(sparse)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert sparse.adam_step("G") == dense.adam_step("G") == 2
        assert sparse.uresnet(x, z, marked, "eval") == dense.uresnet(x, z, onehot, "eval")
        sparse.close()
        dense.close()


@pytest.mark.parametrize("setting", ["ce+foreground", "flat"])
def test_dice_loss_against_the_oracle(lib, setting):
    """3. 'ce+foreground': C = 4, ce 1 + class-form foreground Dice 1 under balanced class weights and the ignored frame;
    'flat': C = 3, pure flat Dice, every pixel.  The phase-0 loss, one gradient evaluation under the HIP pass's own
    decisions and one Adam step against the float64 restatement.

    The first device run printed (seed 5 kept for both), tensors above 1e-4 (HIP / the fp32 oracle under the same
    decisions): 'ce+foreground': 0 / 0, worst tensor 8.28e-5 on dense_noise_1_add_f0/kernel (the oracle's fp32 worst
    3.90e-5, so the per-tensor cap is 1.56e-4), phase-0 loss 2.349017 and phase-1 loss 2.348728 (Dice term 0.960570),
    both the float64 figures to the six digits printed; 'flat': 0 / 0, worst tensor 5.39e-5 on
    dense_noise_2_mul_m2/kernel (the oracle's fp32 worst 5.04e-5), losses 0.648475 and 0.653460, again the float64
    digits."""
    import test_gpu_masked as TM
    from dep_gan_im_amd import data
    B, n, ds = 4, 3, 77
    Cc = 4 if setting == "ce+foreground" else 3
    Pm = _params(SEEDS[setting], Cc)
    x, z, codes, full = _batch(6, n, Cc)
    eng = _engine(B, Pm, Cc)
    if setting == "ce+foreground":
        labels = _framed(codes)
        onehot = R.onehot_rows(labels, Cc, 255)
        cw = data.balanced_class_weights(data.class_counts(labels, Cc, ignore_label=255), "inverse").astype(np.float32)
        assert cw.min() > 0 and cw.max() / cw.min() > 10
        eng.set_loss_weights(cw, ignore_label=255)
        coef = D.class_coef(Cc, "foreground")
        eng.set_dice_loss("class", ce_weight=1.0, dice_weight=1.0, smooth=SMOOTH, class_coef=coef)
        dice = {"form": "class", "coef": coef, "smooth": SMOOTH, "ce_coef": 1.0, "dice_coef": 1.0}
    else:
        labels, onehot, cw = codes, full, np.ones(Cc, np.float32)
        eng.set_dice_loss("flat", ce_weight=0.0, dice_weight=1.0, smooth=SMOOTH)
        dice = {"form": "flat", "coef": None, "smooth": SMOOTH, "ce_coef": 0.0, "dice_coef": 1.0}
    want0 = D.uresnet_eval_dice(Pm, x, z, onehot, cw, dice)
    ev = eng.uresnet(x, z, labels, "eval")
    assert abs(ev - want0) < 1e-4 * max(1.0, abs(want0)), (ev, want0)
    loss = eng.uresnet(x, z, labels, "grads", drop_seed=ds)
    G = eng.get_grads("G")
    masks = TM.hip_uresnet_masks(eng, n)
    loss64, g64, _ = D.uresnet_grads_dice(Pm, x, z, onehot, cw, dice, drop_seed=ds, dtype=torch.float64, masks=masks)
    _, g32, _ = D.uresnet_grads_dice(Pm, x, z, onehot, cw, dice, drop_seed=ds, dtype=torch.float32, masks=masks)
    errs, errs32 = TM.tensor_errors(G, g64), TM.tensor_errors(g32, g64)
    worst = max(errs, key=errs.get)
    print("%s, C = %d, seed %d: phase-0 loss %.6f (fp64 %.6f); loss %.6f (fp64 %.6f); Dice term %.6f; worst tensor %s "
          "%.2e (the oracle's own fp32 run: %.2e there, %.2e at its worst); tensors above 1e-4: HIP %d, fp32 oracle %d"
          % (setting, Cc, SEEDS[setting], ev, want0, loss, loss64, eng.uresnet_dice_sums()["loss"], worst, errs[worst],
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
    tr = D.DiceOracleUResNet({k: v.copy() for k, v in Pm.items()}, cw, dice, dtype=torch.float64)
    want = tr.train_on_batch([x, z], onehot, drop_seed=ds, masks=TM.hip_uresnet_masks(eng, n))
    assert abs(got - want) < 1e-5 * max(1.0, abs(want)), (got, want)
    W = eng.get_weights("G")
    for k in Pm:
        if "moving_" in k:
            np.testing.assert_allclose(W[k], tr.P[k], rtol=1e-4, atol=1e-6, err_msg=k)
        else:   # Adam's first step is lr g / (|g| + eps): at most lr = 1e-4 per element, plus the rounding of the weight
            assert float(np.abs(W[k] - Pm[k]).max()) <= 1.05e-4, k
    assert eng.adam_step("G") == 1
    eng.close()


@pytest.mark.parametrize("ce_weight", [1.0, 0.0])
def test_all_ignored_batch_applies_no_update(lib, ce_weight):
    """4. every pixel ignored, Dice on: loss 0.0, status 0, arenas and Adam counter unchanged, moving statistics moved;
    a batch whose only pixels belong to a zero-weight class still carries a Dice gradient and is updated."""
    B, n = 4, 3
    Pm = _params(5, 4)
    x, z, codes, _ = _batch(7, n, 4)
    eng = _engine(B, Pm, 4)
    eng.set_loss_weights([0.0, 1.0, 1.0, 1.0], ignore_label=255)
    eng.set_dice_loss("class", ce_weight=ce_weight)
    assert eng.uresnet(x, z, codes, "step", drop_seed=3) > 0               # a non-trivial Adam state first
    before, step, nt = _arenas(eng), eng.adam_step("G"), _nontrainable(eng)
    assert step == 1
    nothing = np.full_like(codes, 255)
    assert eng.uresnet(x, z, nothing, "step", drop_seed=4) == 0.0
    s = eng.uresnet_dice_sums()
    assert s["loss"] == 0.0 and all(np.all(s[k] == 0) for k in ("intersection", "pred", "true"))
    assert eng.uresnet_label_counts()["den"] == 0
    for a, b in zip(before, _arenas(eng)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert eng.adam_step("G") == step
    assert not np.array_equal(nt, _nontrainable(eng))
    assert all(float(np.abs(v).max()) == 0.0 for v in eng.get_grads("G").values())
    assert eng.uresnet(x, z, nothing, "eval") == 0.0 and eng.uresnet(x, z, nothing, "grads", drop_seed=5) == 0.0
    # class 0 alone (weight 0 in the cross-entropy: den == 0), but its pixels take part in the Dice term
    zeros = np.zeros_like(codes)
    assert eng.uresnet(x, z, zeros, "step", drop_seed=6) > 0
    assert eng.uresnet_label_counts()["den"] == 0 and eng.adam_step("G") == step + 1
    assert any(not np.array_equal(a, b) for a, b in zip(before, _arenas(eng)))
    eng.close()


def test_facade_dice_loss(lib):
    """5. compile(dice_loss=...) through fit, train_on_batch, evaluate, test_on_batch; loss='dice_coef_loss'."""
    from dep_gan_im_amd import Gen_UNet2D, evaluate
    x, z, codes, onehot = _batch(12, 3, 4)
    vx, vz, vcodes, vonehot = _batch(13, 3, 4)
    marked, vmarked = _framed(codes), _framed(vcodes)
    net = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(loss="sparse_categorical_crossentropy", dice_loss="class",
                                                                dice_classes="foreground", ignore_label=255)
    h = net.fit([x, z], marked, epochs=2, batch_size=4, shuffle=False, validation_data=([vx, vz], vmarked), verbose=0)
    assert sorted(h.history) == ["loss", "val_loss"]
    assert np.isfinite(h.history["loss"]).all() and np.isfinite(h.history["val_loss"]).all()
    got = net._engine.dice_loss
    assert got["form"] == "class" and np.array_equal(got["class_coef"], D.class_coef(4, "foreground").astype(np.float32))
    assert net._engine.loss_weights[1] == 255
    losses = [net.train_on_batch([x, z], marked, drop_seed=0) for _ in range(4)]          # one batch, dropout off
    assert np.isfinite(losses).all() and all(b <= a for a, b in zip(losses, losses[1:])), losses
    # evaluate is the sample-weighted mean of test_on_batch
    l2, l1 = net.test_on_batch([vx[:2], vz[:2]], vmarked[:2]), net.test_on_batch([vx[2:], vz[2:]], vmarked[2:])
    ev = net.evaluate([vx, vz], vmarked, batch_size=2)
    assert abs(ev - (2.0 * l2 + l1) / 3.0) <= 1e-6 * ev
    # the sums of a call through evaluate.soft_dice against the float64 soft Dice of predict's output
    lv = net.test_on_batch([vx, vz], vmarked)
    sums = net._engine.uresnet_dice_sums()
    p = net.predict([vx, vz]).astype(np.float64).reshape(-1, 4)
    t = R.onehot_rows(vmarked, 4, 255).astype(np.float64).reshape(-1, 4)
    keep = D.keep_rows(t)[:, None]
    want = {"intersection": (keep * t * p).sum(0), "pred": (keep * p).sum(0), "true": (keep * t).sum(0)}
    s32 = float(np.float32(SMOOTH))
    a, b = evaluate.soft_dice(sums, s32), evaluate.soft_dice(want, s32)
    assert np.all(np.abs(a["dice"] - b["dice"]) <= 1e-5 * b["dice"]) and abs(a["mean_dice"] - b["mean_dice"]) <= 1e-5
    ce, den, _ = R.weighted_ce_np(p, t, np.ones(4))
    assert den == 3 * (IMG - 2 * BORDER) ** 2
    assert abs(lv - (ce + 1.0 - b["mean_dice"])) < 1e-5 * max(1.0, lv)
    assert abs(sums["loss"] - (1.0 - b["mean_dice"])) < 1e-5
    # compile() without the arguments: the mode is off
    net.compile(loss="sparse_categorical_crossentropy", ignore_label=255)
    assert net._engine.dice_loss is None
    assert abs(net.test_on_batch([vx, vz], vmarked) - ce) < 1e-5 * max(1.0, ce)
    # the reference's name: one-hot labels, the flat form alone -- depgan_uresnet_eval with the flat form
    ref = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(loss="dice_coef_loss")
    v = ref.test_on_batch([vx, vz], vonehot)
    assert ref._engine.dice_loss == {"form": "flat", "ce_weight": 0.0, "dice_weight": 1.0, "smooth": s32, "class_coef": None}
    eng = _engine(4, ref.get_weights_dict(), 4)
    eng.set_dice_loss("flat", ce_weight=0.0)
    assert eng.uresnet(vx, vz, vonehot, "eval") == v and 0.0 < v < 1.0
    pr = ref.predict([vx, vz]).astype(np.float64)
    flat = evaluate.soft_dice({"intersection": (pr * vonehot).sum((0, 1, 2)), "pred": pr.sum((0, 1, 2)),
                               "true": vonehot.astype(np.float64).sum((0, 1, 2))}, s32)["flat"]
    assert abs(v - (1.0 - flat)) < 1e-5
    assert ref.train_on_batch([x, z], onehot, drop_seed=0) > 0
    eng.close()
