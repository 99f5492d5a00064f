"""GPU: the DEP-UResNet's focal mode (focal cross-entropy, label smoothing) through the C ABI and the Keras-style facade,
at 64 x 64 x 1, engines of batch 4 fed 3 samples.

Exact statements are bit for bit: set_focal(0, 0) against a context that never set it, class codes with an ignore label
against one-hot labels with all-zero rows, an all-ignored batch through step, the Dice sums with the mode on and off.
Against the float64 oracle (tests/focal_ce_ref.py restates the oracle's gradient and Adam lines with the focal loss) the
criteria are those of test_weighted_loss_against_the_oracle: the gradient under the HIP pass's own decisions, per tensor.

test_focal_loss_against_the_oracle, the weight seed per class count.  The rule: seed 5 unless the float32 ORACLE's own
count of tensors above 1e-4 (under the HIP pass's decisions) exceeds 4, then the next of 6, 7, 8, 9.  Kept: seed 5 for
both counts.  The first device run printed, tensors above 1e-4 (HIP / the fp32 oracle under the same decisions): C = 4
(weights 0.268, 10.58, 28.34, 7.557): 0 / 0, worst tensor 9.18e-5 on dense_noise_1_add_f0/kernel (the oracle's fp32 worst
5.19e-5, so the per-tensor cap is 2.08e-4), phase-0 loss 0.782740 and phase-1 loss 0.782129, both the float64 figures to
the six digits printed; C = 3 (weights 0.348, 37.79, 10.08): 0 / 0, worst tensor 1.09e-5 (the oracle's fp32 worst
1.48e-5), losses 0.491821 and 0.491972, again the float64 digits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import focal_ce_ref as F  # noqa: E402
from test_gpu_uresnet_classes import IMG, _arenas, _batch, _engine, _params, _u32  # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS = {4: 5, 3: 5}
BORDER = 9            # the ignored frame, "outside the brain": 9 of 64 pixels on every side
GAMMA, EPS = 2.0, 0.1


def _framed(codes, label=255):
    """The codes with the frame of BORDER pixels set to `label`."""
    out = np.full_like(codes, label)
    out[:, BORDER:-BORDER, BORDER:-BORDER] = codes[:, BORDER:-BORDER, BORDER:-BORDER]
    return out


def _nontrainable(eng):
    from dep_gan_im_amd import _lib
    return eng._arena_np("G", _lib.ARENA_NONTRAINABLE).copy()


def _same_state(a, b, Pm):
    ga, gb = a.get_grads("G"), b.get_grads("G")
    assert list(ga) == list(gb)
    for k in ga:
        assert np.array_equal(_u32(ga[k]), _u32(gb[k])), k
    assert any(float(np.abs(v).max()) > 0 for v in ga.values())
    wa, wb = a.get_weights("G"), b.get_weights("G")
    moved = 0
    for k in wa:
        assert np.array_equal(_u32(wa[k]), _u32(wb[k])), k
        moved += "moving_" in k and not np.array_equal(wa[k], Pm[k])
    assert moved > 0


@pytest.mark.parametrize("weights", [False, True])
def test_focal_off_equals_a_context_that_never_set_it(lib, weights):
    """1. set_focal(0, 0), and the mode on and off again: the loss, every gradient tensor and the arenas after a step, with
    the loss-weight mode off and on."""
    from dep_gan_im_amd import _lib
    B, n, ds = 4, 3, 77
    Pm = _params(5, 4)
    x, z, codes, onehot = _batch(9, n, 4)
    labels = _framed(codes) if weights else codes
    plain, zero, back = _engine(B, Pm, 4), _engine(B, Pm, 4), _engine(B, Pm, 4)
    if weights:
        for e in (plain, zero, back):
            e.set_loss_weights([0.5, 4.0, 2.0, 0.0], ignore_label=255)
    assert zero.focal is None
    zero.set_focal(0.0, 0.0)
    assert zero.focal is None and plain.focal is None
    back.set_focal(GAMMA, EPS)
    assert back.focal == (float(np.float32(GAMMA)), float(np.float32(EPS)))
    assert back.uresnet(x, z, labels, "grads", drop_seed=ds) != plain.uresnet(x, z, labels, "grads", drop_seed=ds)
    back.set_focal()
    assert back.focal is None
    if not weights:
        with pytest.raises(Exception, match="focal mode"):
            back.uresnet_label_counts()
    back.set_weights("G", Pm)
    plain.set_weights("G", Pm)
    for e in (zero, back):
        assert e.uresnet(x, z, labels, "grads", drop_seed=ds) == plain.uresnet(x, z, labels, "grads", drop_seed=ds)
        _same_state(plain, e, Pm)
        plain.set_weights("G", Pm)
    for e in (plain, zero, back):
        e.set_weights("G", Pm)
    for step in range(2):
        want = plain.uresnet(x, z, labels, "step", drop_seed=ds + step)
        assert zero.uresnet(x, z, labels, "step", drop_seed=ds + step) == want, step
        assert back.uresnet(x, z, labels, "step", drop_seed=ds + step) == want, step
    for e in (zero, back):
        for a, b in zip(_arenas(plain), _arenas(e)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert e.adam_step("G") == plain.adam_step("G") == 2
        assert e.uresnet(x, z, labels, "eval") == plain.uresnet(x, z, labels, "eval")
    if not weights:
        assert zero.uresnet(x, z, onehot, "eval") == plain.uresnet(x, z, onehot, "eval")
    # refusals: before any launch, and the setting stays
    back.set_focal(GAMMA, EPS)
    for g, e in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, -0.1), (1.0, 1.0), (1.0, float("nan"))):
        with pytest.raises(_lib.DepganError):
            back.set_focal(g, e)
    with pytest.raises(ValueError):
        back.set_focal(True, 0.0)
    assert back.focal == (float(np.float32(GAMMA)), float(np.float32(EPS)))
    for e in (plain, zero, back):
        e.close()


def test_focal_on_with_no_loss_weights(lib):
    """2. fully labelled data, no loss weights: den == n H W from the label pre-pass, a loss far from the plain one and
    equal to the float64 focal loss of the oracle's phase-0 prediction."""
    B, n = 4, 3
    Pm = _params(5, 4)
    x, z, codes, onehot = _batch(9, n, 4)
    plain, eng = _engine(B, Pm, 4), _engine(B, Pm, 4)
    eng.set_focal(GAMMA, EPS)
    assert eng.loss_weights is None
    ce = plain.uresnet(x, z, codes, "eval")
    want = F.uresnet_eval_focal(Pm, x, z, onehot, np.ones(4), GAMMA, EPS)
    for labels in (codes, onehot):
        got = eng.uresnet(x, z, labels, "eval")
        cnt = eng.uresnet_label_counts()
        assert cnt["den"] == n * IMG * IMG and cnt["ignored"] == 0 and cnt["bad"] == 0
        assert np.array_equal(cnt["classes"], np.bincount(codes.reshape(-1), minlength=4))
        assert eng.last_sums()[1] == float(n * IMG * IMG)
        print("focal (gamma %.1f, eps %.1f) phase-0 loss %.6f (fp64 %.6f); plain cross-entropy %.6f" % (GAMMA, EPS, got, want, ce))
        assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (got, want)
        assert abs(got - ce) > 1e-2 * ce, (got, ce)
    # each half of the mode alone: gamma shrinks the loss, smoothing follows its own float64 figure
    eng.set_focal(GAMMA, 0.0)
    g_only = eng.uresnet(x, z, codes, "eval")
    assert g_only < 0.9 * ce and abs(g_only - F.uresnet_eval_focal(Pm, x, z, onehot, np.ones(4), GAMMA, 0.0)) <= 1e-4
    eng.set_focal(0.0, EPS)
    e_only = eng.uresnet(x, z, codes, "eval")
    assert abs(e_only - F.uresnet_eval_focal(Pm, x, z, onehot, np.ones(4), 0.0, EPS)) <= 1e-4 * max(1.0, e_only)
    # a code that is no class is out of range: the focal mode alone sets no ignore code
    from dep_gan_im_amd import _lib
    with pytest.raises(_lib.DepganError, match="class codes are outside"):
        eng.uresnet(x, z, _framed(codes), "eval")
    plain.close()
    eng.close()


def test_ignore_label_equals_zero_rows(lib):
    """3. class codes with ignore_label = 255 on the frame against one-hot labels whose frame rows are all zero, under
    gamma = 2, eps = 0.1 and balanced class weights: loss, gradients, census."""
    from dep_gan_im_amd import data
    B, n, ds = 4, 3, 77
    Pm = _params(5, 4)
    x, z, codes, _ = _batch(9, n, 4)
    marked = _framed(codes)
    onehot = F.onehot_rows(marked, 4, 255)
    cw = data.balanced_class_weights(data.class_counts(marked, 4, ignore_label=255), "inverse").astype(np.float32)
    sparse, dense = _engine(B, Pm, 4), _engine(B, Pm, 4)
    sparse.set_loss_weights(cw, ignore_label=255)
    dense.set_loss_weights(cw)
    for e in (sparse, dense):
        e.set_focal(GAMMA, EPS)
        e.set_census(True)
    assert sparse.uresnet(x, z, marked, "grads", drop_seed=ds) == dense.uresnet(x, z, onehot, "grads", drop_seed=ds)
    _same_state(dense, sparse, Pm)
    cs, cd = sparse.uresnet_label_counts(), dense.uresnet_label_counts()
    inner = n * (IMG - 2 * BORDER) ** 2
    assert cs["den"] == cd["den"] == inner and cs["ignored"] == cd["ignored"] == n * IMG * IMG - inner
    assert np.array_equal(cs["classes"], cd["classes"]) and cs["bad"] == cd["bad"] == 0
    assert np.array_equal(sparse.uresnet_census(), dense.uresnet_census())
    assert int(sparse.uresnet_census().sum()) == inner
    assert np.array_equal(sparse.uresnet_census().sum(-1), cs["classes"])    # the true class is the original label's
    # one-hot labels and no loss-weight mode: the zero rows are ignored by the focal mode itself
    alone, alone_sparse = _engine(B, Pm, 4), _engine(B, Pm, 4)
    alone.set_focal(GAMMA, EPS)
    alone_sparse.set_focal(GAMMA, EPS)
    alone_sparse.set_loss_weights(ignore_label=255)
    assert alone.uresnet(x, z, onehot, "grads", drop_seed=ds) == alone_sparse.uresnet(x, z, marked, "grads", drop_seed=ds)
    _same_state(alone, alone_sparse, Pm)
    assert alone.uresnet_label_counts()["den"] == inner
    for step in range(2):
        assert (sparse.uresnet(x, z, marked[..., None].astype(np.int64), "step", drop_seed=ds + step)
                == dense.uresnet(x, z, onehot, "step", drop_seed=ds + step)), step
    for a, b in zip(_arenas(dense), _arenas(sparse)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert sparse.uresnet(x, z, marked.astype(np.float32), "eval") == dense.uresnet(x, z, onehot, "eval")
    for e in (sparse, dense, alone, alone_sparse):
        e.close()


@pytest.mark.parametrize("Cc", [4, 3])
def test_focal_loss_against_the_oracle(lib, Cc):
    """4. gamma = 2, eps = 0.1, balanced class weights of the batch's own counts, the frame ignored: the phase-0 loss, one
    gradient evaluation under the HIP pass's own decisions and one Adam step against the float64 restatement."""
    import test_gpu_masked as TM
    from dep_gan_im_amd import data
    B, n, ds = 4, 3, 77
    Pm = _params(SEEDS[Cc], Cc)
    x, z, codes, _ = _batch(6, n, Cc)
    marked = _framed(codes)
    onehot = F.onehot_rows(marked, Cc, 255)
    counts = data.class_counts(marked, Cc, ignore_label=255)
    cw = data.balanced_class_weights(counts, "inverse").astype(np.float32)
    assert cw.min() > 0 and cw.max() / cw.min() > 10                        # a rare class: the weights matter
    eng = _engine(B, Pm, Cc)
    eng.set_loss_weights(cw, ignore_label=255)
    eng.set_focal(GAMMA, EPS)
    want0 = F.uresnet_eval_focal(Pm, x, z, onehot, cw, GAMMA, EPS)
    ev = eng.uresnet(x, z, marked, "eval")
    assert abs(ev - want0) < 1e-4 * max(1.0, abs(want0)), (ev, want0)
    loss = eng.uresnet(x, z, marked, "grads", drop_seed=ds)
    G = eng.get_grads("G")
    masks = TM.hip_uresnet_masks(eng, n)
    loss64, g64, _ = F.uresnet_grads_focal(Pm, x, z, onehot, cw, GAMMA, EPS, drop_seed=ds, dtype=torch.float64, masks=masks)
    _, g32, _ = F.uresnet_grads_focal(Pm, x, z, onehot, cw, GAMMA, EPS, drop_seed=ds, dtype=torch.float32, masks=masks)
    errs, errs32 = TM.tensor_errors(G, g64), TM.tensor_errors(g32, g64)
    worst = max(errs, key=errs.get)
    print("C = %d, seed %d, weights %s: phase-0 loss %.6f (fp64 %.6f); loss %.6f (fp64 %.6f); worst tensor %s %.2e (the "
          "oracle's own fp32 run: %.2e there, %.2e at its worst); tensors above 1e-4: HIP %d, fp32 oracle %d"
          % (Cc, SEEDS[Cc], np.round(cw, 3).tolist(), ev, want0, loss, loss64, worst, errs[worst], errs32[worst],
             max(errs32.values()), sum(e > 1e-4 for e in errs.values()), sum(e > 1e-4 for e in errs32.values())))
    assert abs(loss - loss64) < 1e-5 * max(1.0, abs(loss64)), (loss, loss64)
    assert sum(e > 1e-4 for e in errs32.values()) <= 4, "the seed rule: take the next weight seed"
    cap = max(1e-4, 4.0 * max(errs32.values()))
    for k in errs:
        assert errs[k] < cap, (k, errs[k], errs32[k])
    assert sum(e > 1e-4 for e in errs.values()) <= 8, sorted(errs.items(), key=lambda kv: -kv[1])[:10]
    # one step against the Adam restatement under the step's decisions
    eng.set_weights("G", Pm)
    got = eng.uresnet(x, z, marked, "step", drop_seed=ds)
    tr = F.FocalOracleUResNet({k: v.copy() for k, v in Pm.items()}, cw, GAMMA, EPS, dtype=torch.float64)
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


def test_dice_loss_on_top(lib):
    """5. dice_loss 'class' on top: the reported loss is ce_weight * focal + dice_weight * Dice from depgan_last_sums and
    the Dice sums, and the Dice sums are those of a context without the focal mode, bit for bit."""
    B, n = 4, 3
    Pm = _params(5, 4)
    x, z, codes, _ = _batch(9, n, 4)
    marked = _framed(codes)
    cw = [0.5, 4.0, 2.0, 1.5]
    both, dice_only, focal_only = _engine(B, Pm, 4), _engine(B, Pm, 4), _engine(B, Pm, 4)
    for e in (both, dice_only, focal_only):
        e.set_loss_weights(cw, ignore_label=255)
    for e in (both, dice_only):
        e.set_dice_loss("class", ce_weight=0.5, dice_weight=2.0, smooth=1e-3)
    for e in (both, focal_only):
        e.set_focal(GAMMA, EPS)
    for mode in ("eval", "grads"):
        kw = {"drop_seed": 77} if mode == "grads" else {}
        got, plain_dice, focal = (e.uresnet(x, z, marked, mode, **kw) for e in (both, dice_only, focal_only))
        sb, sd = both.uresnet_dice_sums(), dice_only.uresnet_dice_sums()
        for k in ("intersection", "pred", "true"):
            assert np.array_equal(sb[k], sd[k]), k
        assert sb["loss"] == sd["loss"] > 0
        assert both.last_sums()[:2] == focal_only.last_sums()[:2] != dice_only.last_sums()[:2]
        ce_mean = np.float32(both.last_sums()[0]) / np.float32(both.last_sums()[1])
        assert float(ce_mean) == focal
        assert abs(got - (0.5 * focal + 2.0 * sb["loss"])) <= 1e-6 * got
        assert got != plain_dice
    # the Dice participation follows the loss-weight mode alone: without it every pixel takes part, zero rows included
    alone, ref = _engine(B, Pm, 4), _engine(B, Pm, 4)
    for e in (alone, ref):
        e.set_dice_loss("class", ce_weight=0.5, dice_weight=2.0, smooth=1e-3)
    alone.set_focal(GAMMA, EPS)
    onehot = F.onehot_rows(marked, 4, 255)
    alone.uresnet(x, z, onehot, "eval")
    ref.uresnet(x, z, onehot, "eval")
    sa, sr = alone.uresnet_dice_sums(), ref.uresnet_dice_sums()
    assert all(np.array_equal(sa[k], sr[k]) for k in ("intersection", "pred", "true"))
    assert abs(sa["pred"].sum() - n * IMG * IMG) < 1e-3 * n * IMG * IMG
    for e in (both, dice_only, focal_only, alone, ref):
        e.close()


def test_all_ignored_batch_applies_no_update(lib):
    """6. every pixel without a label, the focal mode on and no loss weights: loss 0.0, status 0, arenas and Adam counter
    unchanged, moving statistics moved; a normal step afterwards works."""
    B, n = 4, 3
    Pm = _params(5, 4)
    x, z, codes, onehot = _batch(7, n, 4)
    eng = _engine(B, Pm, 4)
    eng.set_focal(GAMMA, EPS)
    assert eng.uresnet(x, z, codes, "step", drop_seed=3) > 0               # a non-trivial Adam state first
    before, step, nt = _arenas(eng), eng.adam_step("G"), _nontrainable(eng)
    assert step == 1
    nothing = np.zeros_like(onehot)
    assert eng.uresnet(x, z, nothing, "step", drop_seed=4) == 0.0
    assert eng.uresnet_label_counts()["den"] == 0 and eng.last_sums()[1] == 0.0
    for a, b in zip(before, _arenas(eng)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert eng.adam_step("G") == step
    assert not np.array_equal(nt, _nontrainable(eng))
    assert all(float(np.abs(v).max()) == 0.0 for v in eng.get_grads("G").values())
    assert eng.uresnet(x, z, nothing, "eval") == 0.0 and eng.uresnet(x, z, nothing, "grads", drop_seed=5) == 0.0
    # with an ignore label the same through the sparse entries
    eng.set_loss_weights(ignore_label=255)
    assert eng.uresnet(x, z, np.full_like(codes, 255), "step", drop_seed=6) == 0.0 and eng.adam_step("G") == step
    for a, b in zip(before, _arenas(eng)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert eng.uresnet(x, z, codes, "step", drop_seed=3) > 0 and eng.adam_step("G") == step + 1
    assert any(not np.array_equal(a, b) for a, b in zip(before, _arenas(eng)))
    eng.close()


def test_facade_focal_gamma_and_label_smoothing(lib):
    """7. compile(focal_gamma=2.0, label_smoothing=0.1, class_weight={...}, ignore_label=255, metrics=['dice']) and fit."""
    from dep_gan_im_amd import Gen_UNet2D
    x, z, codes, onehot = _batch(12, 3, 4)
    vx, vz, vcodes, _ = _batch(13, 3, 4)
    marked, vmarked = _framed(codes), _framed(vcodes)
    sp = "sparse_categorical_crossentropy"
    net = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(loss=sp, focal_gamma=GAMMA, label_smoothing=EPS,
                                                                class_weight={1: 4.0, 2: 2.5}, ignore_label=255,
                                                                metrics=["dice"])
    h = net.fit([x, z], marked, epochs=2, batch_size=4, shuffle=False, validation_data=([vx, vz], vmarked), verbose=0)
    assert sorted(h.history) == ["dice", "loss", "val_dice", "val_loss"]
    assert np.isfinite(h.history["loss"]).all() and np.isfinite(h.history["val_loss"]).all()
    assert all(0.0 <= v <= 1.0 for v in h.history["dice"] + h.history["val_dice"])
    inner = 3 * (IMG - 2 * BORDER) ** 2
    assert all(int(cm.sum()) == inner for cm in h.census["train"] + h.census["val"])
    eng = net._engine
    assert eng.focal == (float(np.float32(GAMMA)), float(np.float32(EPS)))
    w, ign = eng.loss_weights
    assert np.array_equal(w, np.array([1.0, 4.0, 2.5, 1.0], np.float32)) and ign == 255
    # the facade's loss is the engine's, and the float64 focal loss of its own prediction
    lv, _ = net.test_on_batch([vx, vz], vmarked)
    want = eng.uresnet(vx, vz, vmarked, "eval")
    assert abs(net.evaluate([vx, vz], vmarked)[0] - want) <= 1e-6 * want and abs(lv - want) <= 1e-6 * want
    p = net.predict([vx, vz])
    ref, den, _ = F.focal_ce_np(p, F.onehot_rows(vmarked, 4, 255), w, GAMMA, EPS)
    assert den == inner and abs(lv - ref) < 1e-5 * max(1.0, ref)
    # one-hot labels with zero rows train the same model
    dense = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(focal_gamma=GAMMA, label_smoothing=EPS,
                                                                  class_weight=[1.0, 4.0, 2.5, 1.0])
    sparse = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(loss=sp, focal_gamma=GAMMA, label_smoothing=EPS,
                                                                   class_weight=[1.0, 4.0, 2.5, 1.0], ignore_label=255)
    assert (dense.train_on_batch([x, z], F.onehot_rows(marked, 4, 255), drop_seed=5)
            == sparse.train_on_batch([x, z], marked, drop_seed=5))
    # compile() without the arguments: the mode is off, the plain context's bits
    plain = _engine(eng.batch, eng.get_weights("G"), 4)
    plain_loss = plain.uresnet(vx, vz, vcodes, "eval")
    plain.close()
    net.compile(loss=sp, metrics=[])
    assert eng.focal is None and eng.loss_weights is None
    assert net.test_on_batch([vx, vz], vcodes) == plain_loss
    # with ce_weight = 0 the Dice replaces the cross-entropy: the arguments are accepted and change no loss bit
    d0 = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(loss=sp, dice_loss="class", ce_weight=0.0)
    d1 = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(loss=sp, dice_loss="class", ce_weight=0.0, focal_gamma=GAMMA,
                                                               label_smoothing=EPS)
    assert d0.train_on_batch([x, z], codes, drop_seed=5) == d1.train_on_batch([x, z], codes, drop_seed=5)
    assert d0.test_on_batch([vx, vz], vcodes) == d1.test_on_batch([vx, vz], vcodes)
    assert d1._engine.last_sums()[0] != d0._engine.last_sums()[0]
    with pytest.raises(RuntimeError):
        net.inference_copy().compile(focal_gamma=GAMMA)
