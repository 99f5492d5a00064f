"""GPU: the DEP-UResNet's loss-weight mode (class weights, ignored pixels) through the C ABI and the Keras-style facade,
at 64 x 64 x 1, engines of batch 4 fed 3 samples.

Exact statements are bit for bit: unit weights against a context that never set them, class codes with an ignore label
against one-hot labels with all-zero rows, an all-ignored batch through step.  Against the float64 oracle
(tests/weighted_ce_ref.py restates the oracle's gradient and Adam lines with the weighted loss) the criteria are those of
test_three_and_five_classes_against_the_oracle: the gradient under the HIP pass's own decisions, per tensor.

test_weighted_loss_against_the_oracle, the weight seed per class count.  The rule: seed 5 unless the float32 ORACLE's own
count of tensors above 1e-4 (under the HIP pass's decisions) exceeds 4, then the next of 6, 7, 8, 9.  Kept: seed 5 for
both counts.  The first device run printed, tensors above 1e-4 (HIP / the fp32 oracle under the same decisions): C = 4
(weights 0.268, 10.58, 28.34, 7.557): 0 / 0, worst tensor 9.06e-5 on dense_noise_1_add_f0/kernel (the oracle's fp32 worst
4.42e-5, so the per-tensor cap is 1.77e-4), phase-0 loss 1.388471 and phase-1 loss 1.388157, both the float64 figures to
the six digits printed; C = 3 (weights 0.348, 37.79, 10.08): 0 / 0, worst tensor 1.13e-5 (the oracle's fp32 worst
1.44e-5), losses 1.101418 and 1.101865, again the float64 digits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import weighted_ce_ref as R  # noqa: E402
from test_gpu_uresnet_classes import IMG, _arenas, _batch, _engine, _params, _u32  # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS = {4: 5, 3: 5}
BORDER = 9            # the ignored frame, "outside the brain": 9 of 64 pixels on every side


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


def test_unit_weights_equal_a_context_that_never_set_them(lib):
    """1. the loss, every gradient tensor, the moving statistics, the arenas after two steps and the phase-0 loss; then
    mode on -> off against a context that never switched."""
    B, n, ds = 4, 3, 77
    Pm = _params(5, 4)
    x, z, codes, onehot = _batch(9, n, 4)
    plain, unit = _engine(B, Pm, 4), _engine(B, Pm, 4)
    assert unit.loss_weights is None
    unit.set_loss_weights(class_weight=[1.0, 1.0, 1.0, 1.0])
    w, ign = unit.loss_weights
    assert np.array_equal(w, np.ones(4, np.float32)) and ign is None and plain.loss_weights is None
    for labels_p, labels_u in ((codes, codes), (onehot, onehot)):
        assert unit.uresnet(x, z, labels_u, "grads", drop_seed=ds) == plain.uresnet(x, z, labels_p, "grads", drop_seed=ds)
        _same_state(plain, unit, Pm)
        cnt = unit.uresnet_label_counts()
        assert cnt["den"] == n * IMG * IMG and cnt["ignored"] == 0 and cnt["bad"] == 0
        assert np.array_equal(cnt["classes"], np.bincount(codes.reshape(-1), minlength=4))
        assert unit.last_sums()[1] == float(n * IMG * IMG) == plain.last_sums()[1]
    for step in range(2):
        assert (unit.uresnet(x, z, codes, "step", drop_seed=ds + step)
                == plain.uresnet(x, z, codes, "step", drop_seed=ds + step)), step
    for a, b in zip(_arenas(plain), _arenas(unit)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert plain.adam_step("G") == unit.adam_step("G") == 2
    assert unit.uresnet(x, z, codes, "eval") == plain.uresnet(x, z, codes, "eval")
    assert unit.uresnet(x, z, onehot, "eval") == plain.uresnet(x, z, onehot, "eval")
    # a weighted step in between, on both; then one engine goes back to the mode off and the other never switched
    heavy = _engine(B, Pm, 4)
    heavy.set_loss_weights(class_weight=[0.5, 4.0, 2.0, 0.0], ignore_label=255)
    assert heavy.uresnet(x, z, _framed(codes), "grads", drop_seed=ds) != plain.uresnet(x, z, codes, "grads", drop_seed=ds)
    heavy.set_loss_weights()
    assert heavy.loss_weights is None
    with pytest.raises(Exception, match="loss-weight mode"):
        heavy.uresnet_label_counts()
    heavy.set_weights("G", Pm)
    fresh = _engine(B, Pm, 4)
    assert heavy.uresnet(x, z, codes, "grads", drop_seed=ds) == fresh.uresnet(x, z, codes, "grads", drop_seed=ds)
    _same_state(fresh, heavy, Pm)
    for e in (plain, unit, heavy, fresh):
        e.close()


def test_ignore_label_equals_zero_rows(lib):
    """2. class codes with ignore_label = 255 on the frame against one-hot labels whose frame rows are all zero."""
    B, n, ds = 4, 3, 77
    Pm = _params(5, 4)
    x, z, codes, _ = _batch(9, n, 4)
    marked = _framed(codes)
    onehot = R.onehot_rows(marked, 4, 255)
    cw = [0.5, 4.0, 2.0, 1.5]
    sparse, dense = _engine(B, Pm, 4), _engine(B, Pm, 4)
    sparse.set_loss_weights(cw, ignore_label=255)
    dense.set_loss_weights(cw)
    sparse.set_census(True)
    dense.set_census(True)
    assert sparse.uresnet(x, z, marked, "grads", drop_seed=ds) == dense.uresnet(x, z, onehot, "grads", drop_seed=ds)
    _same_state(dense, sparse, Pm)
    cs, cd = sparse.uresnet_label_counts(), dense.uresnet_label_counts()
    inner = n * (IMG - 2 * BORDER) ** 2
    assert cs["den"] == cd["den"] == inner and cs["ignored"] == cd["ignored"] == n * IMG * IMG - inner
    assert np.array_equal(cs["classes"], cd["classes"]) and cs["bad"] == cd["bad"] == 0
    assert np.array_equal(sparse.uresnet_census(), dense.uresnet_census())
    assert int(sparse.uresnet_census().sum()) == inner                     # the census leaves the ignored pixels out
    assert sparse.last_sums()[1] == float(inner)
    for step in range(2):
        assert (sparse.uresnet(x, z, marked[..., None].astype(np.int64), "step", drop_seed=ds + step)
                == dense.uresnet(x, z, onehot, "step", drop_seed=ds + step)), step
    for a, b in zip(_arenas(dense), _arenas(sparse)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert sparse.uresnet(x, z, marked.astype(np.float32), "eval") == dense.uresnet(x, z, onehot, "eval")
    # a value that is no byte is still refused with the ignore label at 255: it does not turn into an ignored pixel
    from dep_gan_im_amd import _lib
    wrap = marked.astype(np.int32)
    wrap[0, 20, 20] = 300
    with pytest.raises(_lib.DepganError, match="1 of"):
        sparse.uresnet(x, z, wrap, "eval")
    sparse.close()
    dense.close()


def test_all_ignored_batch_applies_no_update(lib):
    """3. every pixel ignored: loss 0.0, status 0, arenas and Adam counter unchanged, moving statistics moved; a normal
    step afterwards works."""
    B, n = 4, 3
    Pm = _params(5, 4)
    x, z, codes, _ = _batch(7, n, 4)
    eng = _engine(B, Pm, 4)
    eng.set_loss_weights(ignore_label=255)
    assert eng.uresnet(x, z, codes, "step", drop_seed=3) > 0               # a non-trivial Adam state first
    before, step, nt = _arenas(eng), eng.adam_step("G"), _nontrainable(eng)
    assert step == 1
    nothing = np.full_like(codes, 255)
    assert eng.uresnet(x, z, nothing, "step", drop_seed=4) == 0.0
    assert eng.uresnet_label_counts()["den"] == 0 and eng.last_sums()[1] == 0.0
    for a, b in zip(before, _arenas(eng)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert eng.adam_step("G") == step
    assert not np.array_equal(nt, _nontrainable(eng))
    assert all(float(np.abs(v).max()) == 0.0 for v in eng.get_grads("G").values())
    assert eng.uresnet(x, z, nothing, "eval") == 0.0 and eng.uresnet(x, z, nothing, "grads", drop_seed=5) == 0.0
    assert eng.uresnet(x, z, codes, "step", drop_seed=3) > 0 and eng.adam_step("G") == step + 1
    assert any(not np.array_equal(a, b) for a, b in zip(before, _arenas(eng)))
    eng.close()


@pytest.mark.parametrize("Cc", [4, 3])
def test_weighted_loss_against_the_oracle(lib, Cc):
    """4. balanced class weights of the batch's own counts, the frame ignored: the phase-0 loss, one gradient evaluation
    under the HIP pass's own decisions and one Adam step against the float64 restatement."""
    import test_gpu_masked as TM
    from dep_gan_im_amd import data
    B, n, ds = 4, 3, 77
    Pm = _params(SEEDS[Cc], Cc)
    x, z, codes, _ = _batch(6, n, Cc)
    marked = _framed(codes)
    onehot = R.onehot_rows(marked, Cc, 255)
    counts = data.class_counts(marked, Cc, ignore_label=255)
    inner = n * (IMG - 2 * BORDER) ** 2
    assert counts["ignored"] == n * IMG * IMG - inner and counts["bad"] == 0 and counts["total"] == n * IMG * IMG
    assert np.array_equal(counts["classes"], np.bincount(marked[marked != 255].reshape(-1), minlength=Cc))
    assert np.array_equal(data.class_counts(onehot, Cc)["classes"], counts["classes"])
    cw = data.balanced_class_weights(counts, "inverse").astype(np.float32)
    assert cw.min() > 0 and cw.max() / cw.min() > 10                        # a rare class: the weights matter
    eng = _engine(B, Pm, Cc)
    eng.set_loss_weights(cw, ignore_label=255)
    want0 = R.uresnet_eval_weighted(Pm, x, z, onehot, cw)
    ev = eng.uresnet(x, z, marked, "eval")
    assert abs(ev - want0) < 1e-4 * max(1.0, abs(want0)), (ev, want0)
    loss = eng.uresnet(x, z, marked, "grads", drop_seed=ds)
    G = eng.get_grads("G")
    masks = TM.hip_uresnet_masks(eng, n)
    loss64, g64, _ = R.uresnet_grads_weighted(Pm, x, z, onehot, cw, drop_seed=ds, dtype=torch.float64, masks=masks)
    _, g32, _ = R.uresnet_grads_weighted(Pm, x, z, onehot, cw, drop_seed=ds, dtype=torch.float32, masks=masks)
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
    tr = R.WeightedOracleUResNet({k: v.copy() for k, v in Pm.items()}, cw, dtype=torch.float64)
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


def test_facade_class_weight_and_ignore_label(lib):
    """5. compile(class_weight={...}, ignore_label=255, metrics=['dice']) and fit with validation data."""
    from dep_gan_im_amd import Gen_UNet2D
    x, z, codes, onehot = _batch(12, 3, 4)
    vx, vz, vcodes, _ = _batch(13, 3, 4)
    marked, vmarked = _framed(codes), _framed(vcodes)
    net = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(loss="sparse_categorical_crossentropy",
                                                                class_weight={1: 4.0, 2: 2.5}, ignore_label=255,
                                                                metrics=["dice"])
    h = net.fit([x, z], marked, epochs=2, batch_size=4, shuffle=False, validation_data=([vx, vz], vmarked), verbose=0)
    assert sorted(h.history) == ["dice", "loss", "val_dice", "val_loss"]
    assert np.isfinite(h.history["loss"]).all() and np.isfinite(h.history["val_loss"]).all()
    assert all(0.0 <= v <= 1.0 for v in h.history["dice"] + h.history["val_dice"])
    losses = [net.train_on_batch([x, z], marked, drop_seed=11)[0] for _ in range(4)]     # one batch, one dropout mask
    assert np.isfinite(losses).all() and all(b <= a for a, b in zip(losses, losses[1:])), losses
    inner = 3 * (IMG - 2 * BORDER) ** 2
    assert all(int(cm.sum()) == inner for cm in h.census["train"] + h.census["val"])
    w, ign = net._engine.loss_weights
    assert np.array_equal(w, np.array([1.0, 4.0, 2.5, 1.0], np.float32)) and ign == 255
    # the facade's loss is the engine's: test_on_batch against the float64 weighted loss of its own prediction
    lv, _ = net.test_on_batch([vx, vz], vmarked)
    p = net.predict([vx, vz])
    want, den, _ = R.weighted_ce_np(p, R.onehot_rows(vmarked, 4, 255), w)
    assert den == inner and abs(lv - want) < 1e-5 * max(1.0, want)
    assert abs(net.evaluate([vx, vz], vmarked)[0] - lv) <= 1e-6 * lv
    # compile() again without the arguments: the mode is off, an ignore byte is an out-of-range code again
    from dep_gan_im_amd import _lib
    net.compile(loss="sparse_categorical_crossentropy", metrics=[])
    assert net._engine.loss_weights is None
    with pytest.raises(_lib.DepganError, match="class codes are outside"):
        net.test_on_batch([vx, vz], vmarked)
    assert net.test_on_batch([vx, vz], vcodes) > 0
    with pytest.raises(ValueError, match="all-zero rows"):
        net.compile(loss="categorical_crossentropy", ignore_label=255)
    # one-hot labels with zero rows and a weight list
    dense = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(class_weight=[1.0, 4.0, 2.5, 1.0])
    sparse = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(loss="sparse_categorical_crossentropy",
                                                                   class_weight=[1.0, 4.0, 2.5, 1.0], ignore_label=255)
    assert (dense.train_on_batch([x, z], R.onehot_rows(marked, 4, 255), drop_seed=5)
            == sparse.train_on_batch([x, z], marked, drop_seed=5))


def test_data_helpers_keep_the_ignore_label(lib):
    """data.to_codes passes the ignore label through, data.to_one_hot turns it into an all-zero row, both still refuse
    every other out-of-range value; data.class_counts counts both forms in chunks."""
    from dep_gan_im_amd import _lib, data
    _, _, codes, _ = _batch(9, 3, 4)
    marked = _framed(codes)
    coded = marked.astype(np.float32)[..., None] + np.float32(0.25)          # UT:563 truncates toward zero
    got = data.to_codes(coded, 4, ignore_label=255)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), marked)
    oh = data.to_one_hot(coded, 4, ignore_label=255)
    assert np.array_equal(oh.cpu().numpy(), R.onehot_rows(marked, 4, 255))
    for fn in (data.to_codes, data.to_one_hot):
        with pytest.raises(_lib.DepganError):
            fn(coded, 4)                                                     # without the label 255 is out of range
        with pytest.raises(_lib.DepganError):
            fn(np.where(coded > 200, np.float32(77.0), coded), 4, ignore_label=255)
    want = np.bincount(marked[marked != 255], minlength=4)
    for labels, ign in ((marked, 255), (got, 255), (marked.astype(np.int64), 255), (oh, None), (oh.cpu().numpy(), None)):
        for chunk in (1 << 26, 5000):
            c = data.class_counts(labels, 4, ignore_label=ign, chunk=chunk)
            assert np.array_equal(c["classes"], want) and c["bad"] == 0 and c["ignored"] == int((marked == 255).sum())
            assert c["total"] == marked.size
    c = data.class_counts(marked, 4)                                         # no ignore label: 255 is out of range
    assert c["bad"] == int((marked == 255).sum()) and c["ignored"] == 0 and np.array_equal(c["classes"], want)
