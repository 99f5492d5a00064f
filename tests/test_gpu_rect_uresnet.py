"""GPU parity of the DEP-UResNet (nc_out = 4) on non-square, non-power-of-two images: 48x80, 16x48 and 32x128
(tests/rect_cases.py), an engine of batch 4 fed n = 4 and a short batch n = 3.

The supervised path walks the image as rows x columns in more places than the GAN: the batch-statistics BatchNorms over
n x H x W pixels (as few as 2 x 6 x n at the 16x48 bottom), the Dropout keep mask of do_gen_1 at (H/4, W/4), the label
counts, the class census, and the two passes of the distance transform behind the boundary loss.  Every check follows the
square test it restates: test_gpu_uresnet.py::test_short_batch_grads_step_and_eval and test_dropout_mask_is_the_oracles,
the single-option loss tests (weighted_ce_ref, focal_ce_ref, dice_ref, boundary_ref), and the facade tests.

Seeds.  The phase-1 gradient flows through 40 batch-statistics BatchNorms; the rule of the square tests is per tensor
max(1e-4, 4 x the float32 oracle's own worst error under the same masks) and at most 8 tensors above 1e-4.  The oracle's own
float32 run against its float64 one, each under the float32 run's own masks, measured on the CPU before the first GPU run
(weights uresnet_params(5), batch synth_uresnet_batch(22, n), drop_seed 77), tensors above 1e-4 / worst tensor:
    48x80: n = 4: 0 / 7.4e-5, n = 3: 2 / 2.8e-4;  16x48: n = 4: 3 / 1.4e-4, n = 3: 3 / 1.4e-4;
    32x128: n = 4: 1 / 1.5e-4, n = 3: 3 / 3.3e-4
Batch seed 8 + n, which the square test uses, was dropped: at 48x80 with n = 3 the reference alone leaves 18 tensors above
1e-4 (batch seed 21: 14 at 32x128 with n = 3), more than the rule allows the kernel.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boundary_ref as BR  # noqa: E402
import dice_ref as D  # noqa: E402
import focal_ce_ref as F  # noqa: E402
import rect_cases as RC  # noqa: E402
import test_gpu_masked as TM  # noqa: E402
import weighted_ce_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = pytest.mark.parametrize("H,W", RC.URESNET_SIZES, ids=["%dx%d" % s for s in RC.URESNET_SIZES])
PSEED, DSEED, DS = 5, 22, 77
BF16S_E_ROUND_FOUND = 2.22e-2      # test_bf16_storage_predict_48x80: the yardstick as measured on the CPU


def _params(seed=PSEED):
    """tests/golden/make_golden.py::uresnet_params: a head small enough that the softmax is not saturated"""
    from oracle import depgan_oracle as O
    P = O.init_generator(seed, nc_out=4, randomize_bn=True, bias_std=0.05)
    P["gen_segmentation/kernel"] = (P["gen_segmentation/kernel"] * 0.05).astype(np.float32)
    return P


def _engine(H, W, B, P):
    from dep_gan_im_amd import Engine
    eng = Engine(B, H, W, 1, lrG=1e-4, beta1=0.9, beta2=0.999, nc_out=4)
    eng.set_weights("G", P)
    return eng


def _grad_check(what, G, g64, g32):
    errs, errs32 = TM.tensor_errors(G, g64), TM.tensor_errors(g32, g64)
    worst = max(errs, key=errs.get)
    print("%s: worst tensor %s %.2e (CPU fp32 %.2e there, %.2e at its worst); tensors above 1e-4: HIP %d, fp32 oracle %d"
          % (what, worst, errs[worst], errs32[worst], max(errs32.values()), sum(e > 1e-4 for e in errs.values()),
             sum(e > 1e-4 for e in errs32.values())))
    cap = max(1e-4, 4.0 * max(errs32.values()))
    for k in errs:
        assert errs[k] < cap, (k, errs[k], errs32[k])
    assert sum(e > 1e-4 for e in errs.values()) <= 8, sorted(errs.items(), key=lambda kv: -kv[1])[:10]


@SIZES
@pytest.mark.parametrize("n", [4, 3])
def test_grads_step_and_eval(lib, H, W, n):
    """Loss and per-tensor phase-1 gradients (drop_seed 77) against the float64 oracle under the HIP pass's masks, the
    moving statistics of every BatchNorm after the pass (rtol 1e-4, atol 1e-6), the step against
    OracleUResNet.train_on_batch in float64 under the step's masks, and the phase-0 loss after it to 1e-4.

    Measured on an MI355X, tensors above 1e-4 (HIP / the fp32 oracle under the HIP pass's masks), worst tensor:
        48x80:  n = 4: 2 / 0, 1.2e-4 (cap 3.4e-4);  n = 3: 5 / 5, 6.6e-4 (the oracle's fp32 worst 9.8e-4: cap 3.9e-3)
        16x48:  n = 4: 6 / 1, 2.1e-4 (cap 1.1e-3);  n = 3: 4 / 4, 1.8e-4 (cap 1.0e-3)
        32x128: n = 4: 8 / 4, 3.0e-4 (cap 5.3e-4);  n = 3: 2 / 10, 1.4e-4 (cap 3.2e-3)
    Every tensor above 1e-4 is a noise-MLP weight behind the three batch-of-n BatchNorms, as at 64 x 64.  32x128 with
    n = 4 sits at the limit of 8; the batch seed was fixed from the CPU oracle before this was known and stays.
    """
    from oracle import depgan_oracle as O
    B = 4
    P = _params()
    x, z, lab = O.synth_uresnet_batch(DSEED, n, H, W)
    eng = _engine(H, W, B, P)
    loss = eng.uresnet(x, z, lab, "grads", drop_seed=DS)
    G = eng.get_grads("G")
    masks = TM.hip_uresnet_masks(eng, n)
    loss64, g64, stats = O.uresnet_grads(P, x, z, lab, drop_seed=DS, dtype=torch.float64, masks=masks)
    _, g32, _ = O.uresnet_grads(P, x, z, lab, drop_seed=DS, dtype=torch.float32, masks=masks)
    assert abs(loss - loss64) < 1e-5 * max(1.0, abs(loss64)), (loss, loss64)
    _grad_check("%dx%d n = %d" % (H, W, n), G, g64, g32)
    Wt = eng.get_weights("G")
    for name, (mean, var, cnt, fused) in stats.items():
        corr = cnt / (cnt - 1.0) if fused else cnt / (cnt - (1.0 + O.BN_EPS))
        np.testing.assert_allclose(Wt[name + "/moving_mean"], P[name + "/moving_mean"] * 0.99 + mean.numpy() * 0.01,
                                   rtol=1e-4, atol=1e-6, err_msg=name)
        np.testing.assert_allclose(Wt[name + "/moving_variance"],
                                   P[name + "/moving_variance"] * 0.99 + var.numpy() * corr * 0.01,
                                   rtol=1e-4, atol=1e-6, err_msg=name)
    # the step: Adam and the moving statistics, against the fp64 oracle's train_on_batch under the step's masks
    eng.set_weights("G", P)
    got = eng.uresnet(x, z, lab, "step", drop_seed=DS)
    tr = O.OracleUResNet({k: v.copy() for k, v in P.items()}, dtype=torch.float64)
    want = tr.train_on_batch([x, z], lab, drop_seed=DS, masks=TM.hip_uresnet_masks(eng, n))
    assert abs(got - want) < 1e-5 * max(1.0, abs(want)), (got, want)
    Wt = eng.get_weights("G")
    for k in P:
        if "moving_" in k:
            np.testing.assert_allclose(Wt[k], tr.P[k], rtol=1e-4, atol=1e-6, err_msg=k)
    # phase 0 after the step, on the weights the engine holds
    ev = eng.uresnet(x, z, lab, "eval")
    p0 = torch.from_numpy(O.uresnet_predict(Wt, x, z, dtype=torch.float64))
    want0 = float(O.keras_categorical_crossentropy_t(p0, torch.from_numpy(lab).double()))
    assert abs(ev - want0) < 1e-4 * max(1.0, abs(want0)), (ev, want0)
    eng.close()


@SIZES
def test_dropout_mask_is_the_oracles(lib, H, W):
    """drop_seed in (0, 1, 77) gives the oracle's loss to 2e-5 (test_gpu_uresnet.py::test_dropout_mask_is_the_oracles): a
    keep mask of (n, H/4, W/4, 96) indexed with H and W exchanged is another mask"""
    from oracle import depgan_oracle as O
    P = _params()
    x, z, lab = O.synth_uresnet_batch(6, 4, H, W)
    eng = _engine(H, W, 4, P)
    losses = []
    for ds in (0, 1, 77):
        eng.set_weights("G", P)
        got = eng.uresnet(x, z, lab, "grads", drop_seed=ds)
        want, _, _ = O.uresnet_grads(P, x, z, lab, drop_seed=ds or None)
        assert abs(got - want) < 2e-5 * max(1.0, abs(want)), (ds, got, want)
        losses.append(want)
    assert len(set(losses)) == 3                                           # the masks do move the loss
    eng.close()


# ---- every loss option at once, 48x80 ----
BORDER = 5                     # the ignored frame
CW_KIND, GAMMA, EPS = "inverse", 2.0, 0.1
DICE = dict(form="class", ce_coef=0.5, dice_coef=2.0, smooth=1e-3)
SPACING, B_COEF = (0.75, 1.25), 0.1


def _framed(codes, label=255):
    out = np.full_like(codes, label)
    out[:, BORDER:-BORDER, BORDER:-BORDER] = codes[:, BORDER:-BORDER, BORDER:-BORDER]
    return out


def all_options_loss_t(p, lt, cw, dice, boundary, dtype):
    """ce_coef * focal cross-entropy (class weights, label smoothing) + dice_coef * Dice('class') + boundary_coef * L_B of
    probabilities p against one-hot rows lt with all-zero rows for ignored pixels, from the restatements the
    single-option tests use; returns (loss, focal, Dice, L_B)"""
    cwt = torch.as_tensor(np.asarray(cw, np.float64)).to(dtype)
    keep = (lt != 0).any(-1).to(dtype)
    focal, _, _ = F.focal_ce_t(p, lt, cwt, GAMMA, EPS)
    dl, _, _, _ = D.dice_t(p, lt, keep, dice["form"], torch.as_tensor(np.asarray(dice["coef"], np.float64)).to(dtype),
                           dice["smooth"])
    lb = BR.boundary_t(p, torch.as_tensor(np.asarray(boundary["phi"], np.float64)).to(dtype), keep,
                       torch.as_tensor(np.asarray(boundary["class_coef"], np.float64)).to(dtype))
    return dice["ce_coef"] * focal + dice["dice_coef"] * dl + boundary["coef"] * lb, focal, dl, lb


def all_options_grads(P, x, z, onehot, cw, dice, boundary, drop_seed, dtype, masks):
    """O.uresnet_grads with the loss above (the few lines dice_ref / boundary_ref restate)"""
    from oracle import depgan_oracle as O
    T = O.to_torch(P, dtype, requires_grad=True)
    xt, zt, lt = O._t(x, dtype), O._t(z, dtype), O._t(np.asarray(onehot, np.float32), dtype)
    n, H, W, _ = xt.shape
    keep = torch.tensor(O.dropout_keep_mask(drop_seed, (n, H // 4, W // 4, 96)))
    stats = {}
    p = O.uresnet_forward_t(T, xt, zt, phase=1, keep_mask=keep, stats=stats, masks=masks)
    loss = all_options_loss_t(p, lt, cw, dice, boundary, dtype)[0]
    names = O.trainable_names(P)
    gs = torch.autograd.grad(loss, [T[k] for k in names], allow_unused=True)
    return float(loss.detach()), {k: (g.detach().numpy() if g is not None else np.zeros_like(P[k]))
                                  for k, g in zip(names, gs)}


def all_options_case(H=48, W=80, n=3):
    """(P, x, z, integer labels (n, H, W) with the ignored frame, their one-hot rows, class weights, dice, boundary)"""
    from dep_gan_im_amd import data
    from oracle import depgan_oracle as O
    P = _params()
    x, z, lab = O.synth_uresnet_batch(DSEED, n, H, W)
    labels = _framed(lab.argmax(-1).astype(np.int64))
    onehot = R.onehot_rows(labels, 4, 255)
    cw = data.balanced_class_weights(data.class_counts(labels, 4, ignore_label=255), CW_KIND).astype(np.float32)
    coef = BR.class_coef(4, "foreground")
    dice = dict(DICE, coef=D.class_coef(4, "foreground"))
    phi = BR.signed_distance(BR.true_class(labels, 4, 255), 4, SPACING, 0.0, [1 if c != 0 else 0 for c in coef])
    return P, x, z, labels, onehot, cw, dice, {"coef": B_COEF, "class_coef": coef, "phi": phi}


def _all_options_engine(H, W, P, cw, ignore):
    eng = _engine(H, W, 4, P)
    eng.set_loss_weights(cw, ignore_label=ignore)
    eng.set_focal(GAMMA, EPS)
    eng.set_dice_loss("class", ce_weight=DICE["ce_coef"], dice_weight=DICE["dice_coef"], smooth=DICE["smooth"],
                      class_coef=D.class_coef(4, "foreground"))
    eng.set_boundary_loss(True, weight=B_COEF, class_coef=BR.class_coef(4, "foreground"), spacing=SPACING)
    return eng


def test_every_loss_option_at_once_48x80(lib):
    """Integer labels (n, 48, 80) with an ignored frame and balanced class weights, focal (gamma 2) + label smoothing
    (0.1), Dice 'class' on the foreground (0.5 ce + 2 Dice) and the boundary loss with anisotropic spacing (0.75, 1.25),
    all on together, n = 3 of batch 4.  The signed distance maps are the restatement's bit for bit (the two passes of the
    transform walk rows and columns with different weights); the phase-0 loss and its three pieces against the float64
    restatements at the single-option tests' bounds (1e-4; L_B 1e-5 of its scale); the phase-1 loss to 1e-5 and the
    gradient per tensor under the HIP pass's decisions by the rule of those tests; and class codes with the ignored frame
    against one-hot labels with all-zero rows, bit for bit, as each single-option test does for its own option.

    Measured on an MI355X: phase-0 loss 2.844733 (focal 0.782171, Dice 0.985102, L_B 4.834442), each the float64 figure to
    the six digits printed; tensors above 1e-4: HIP 0, the fp32 oracle 0; worst tensor 2.7e-5 (cap 1e-4).
    """
    from dep_gan_im_amd import data
    from oracle import depgan_oracle as O
    H, W, n = 48, 80, 3
    P, x, z, labels, onehot, cw, dice, boundary = all_options_case(H, W, n)
    assert cw.min() > 0 and len(set(np.round(cw, 3))) == 4
    dev_phi = data.signed_distance_maps(labels, 4, SPACING, ignore_label=255, classes=[1, 2, 3]).cpu().numpy()
    assert dev_phi.shape == (n, H, W, 4)
    assert np.array_equal(dev_phi.view(np.uint32), boundary["phi"].view(np.uint32))
    eng = _all_options_engine(H, W, P, cw, 255)
    # phase 0: the loss and its pieces
    p64 = torch.from_numpy(O.uresnet_predict(P, x, z, dtype=torch.float64))
    want0, focal0, dice0, lb0 = (float(v) for v in all_options_loss_t(p64, torch.from_numpy(onehot).double(), cw, dice,
                                                                      boundary, torch.float64))
    ev = eng.uresnet(x, z, labels, "eval")
    kept = int((labels != 255).sum())
    assert kept == n * (H - 2 * BORDER) * (W - 2 * BORDER)
    sums, (lb, M), ds_ = eng.last_sums(), eng.uresnet_boundary_loss(), eng.uresnet_dice_sums()
    print("48x80 all options: phase-0 loss %.6f (fp64 %.6f); focal %.6f (%.6f); Dice %.6f (%.6f); L_B %.6f (%.6f)"
          % (ev, want0, sums[0] / sums[1], focal0, ds_["loss"], dice0, lb, lb0))
    assert abs(ev - want0) < 1e-4 * max(1.0, abs(want0)), (ev, want0)
    assert sums[1] == kept and abs(sums[0] / sums[1] - focal0) < 1e-4 * max(1.0, abs(focal0))
    assert abs(ds_["loss"] - dice0) < 1e-4 * max(1.0, abs(dice0))
    _, _, _, scale = BR.boundary_np(p64.numpy().reshape(-1, 4), boundary["phi"].reshape(-1, 4),
                                    (labels != 255).reshape(-1), boundary["class_coef"])
    assert M == kept and abs(lb - lb0) <= 1e-5 * scale, (lb, lb0, scale)
    true_counts = np.bincount(labels[labels != 255].reshape(-1), minlength=4)
    np.testing.assert_allclose(ds_["true"], true_counts, rtol=0, atol=0)      # the label counts are exact
    # phase 1: the gradient under the HIP pass's decisions
    loss = eng.uresnet(x, z, labels, "grads", drop_seed=DS)
    G = eng.get_grads("G")
    masks = TM.hip_uresnet_masks(eng, n)
    loss64, g64 = all_options_grads(P, x, z, onehot, cw, dice, boundary, DS, torch.float64, masks)
    _, g32 = all_options_grads(P, x, z, onehot, cw, dice, boundary, DS, torch.float32, masks)
    assert abs(loss - loss64) < 1e-5 * max(1.0, abs(loss64)), (loss, loss64)
    _grad_check("48x80 all options", G, g64, g32)
    # class codes with the ignored frame = one-hot rows that are all zero on it, bit for bit
    dense = _all_options_engine(H, W, P, cw, None)
    eng.set_weights("G", P)
    assert eng.uresnet(x, z, labels, "grads", drop_seed=DS) == dense.uresnet(x, z, onehot, "grads", drop_seed=DS)
    ga, gb = eng.get_grads("G"), dense.get_grads("G")
    for k in ga:
        assert np.array_equal(ga[k].view(np.uint32), gb[k].view(np.uint32)), k
    assert eng.uresnet_boundary_loss() == dense.uresnet_boundary_loss()
    eng.close()
    dense.close()


# ---- facade ----
def test_facade_fit_predict_evaluate_round_trip_48x80(lib, tmp_path):
    """Gen_UNet2D((48, 80, 1), nc_out=4).fit with a short last batch, validation data and an Augmenter with elastic and
    bias fields; predict, evaluate, a save / load round trip and evaluate.predict_mean, as
    test_gpu_uresnet.py::test_facade_fit_history_and_short_last_batch at 64 x 64."""
    from dep_gan_im_amd import Gen_UNet2D, data, evaluate
    from oracle import depgan_oracle as O
    H, W = 48, 80
    net = Gen_UNet2D((H, W, 1), (32, 1), 32, 4, seed=3)
    x, z, lab = O.synth_uresnet_batch(12, 7, H, W)
    vx, vz, vlab = O.synth_uresnet_batch(13, 3, H, W)
    np.random.seed(0)
    aug = data.Augmenter(rotate=5.0, shift=2.0, elastic=1.5, bias=0.2, field_grid=(5, 7), seed=4)
    h = net.fit([x, z], lab, epochs=2, batch_size=4, shuffle=True, validation_data=([vx, vz], vlab), verbose=0, augment=aug)
    assert len(h.history["loss"]) == 2 and len(h.history["val_loss"]) == 2
    assert all(np.isfinite(h.history["loss"])) and all(np.isfinite(h.history["val_loss"]))
    assert abs(net.evaluate([vx, vz], vlab, batch_size=4) - h.history["val_loss"][-1]) < 1e-6
    p = net.predict([vx, vz])
    assert p.shape == (3, H, W, 4) and abs(float(p.sum(-1).mean()) - 1.0) < 1e-5
    # phase-0 predict is the oracle's on the weights the model now holds
    np.testing.assert_allclose(p, O.uresnet_predict(net.get_weights_dict(), vx, vz), atol=2e-5)
    path = str(tmp_path / "w.npz")
    net.save_weights(path)
    twin = Gen_UNet2D((H, W, 1), (32, 1), 32, 4, seed=9)
    assert not np.array_equal(twin.predict([vx, vz]), p)
    twin.load_weights(path)
    assert np.array_equal(twin.predict([vx, vz]).view(np.uint32), p.view(np.uint32))
    # predict_mean: the float64 mean of n_repeat masked predictions with the noise of the given generator
    mask = (np.random.default_rng(2).uniform(size=(3, H, W)) > 0.2).astype(np.float32)
    mean = evaluate.predict_mean(net, vx, n_repeat=4, mask=mask, rng=np.random.RandomState(5))
    assert tuple(mean.shape) == (3, H, W, 4) and mean.dtype == torch.float64
    r, acc = np.random.RandomState(5), np.zeros((3, H, W, 4), np.float64)
    for _ in range(4):
        acc += net.predict([vx, r.normal(size=(3, 32, 1)).astype("float32")]).astype(np.float64) * mask[..., None]
    assert np.array_equal(mean.cpu().numpy(), acc / 4.0)


def _dist(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(d.max()), float(d.mean())


def bf16_predict_oracles(H=48, W=80, n=2, seed=61):
    """(P4, x, z, storage-graph oracle, weights-only oracle, float32 oracle), all on the CPU: the yardsticks of
    test_gpu_bf16_store_uresnet.py::test_end_to_end_by_the_modes_own_criterion at this size"""
    from oracle import depgan_oracle as O
    from test_gpu_bf16_store_uresnet import _p4, storage_graph_softmax
    P4 = _p4(seed)
    x, _, z, _ = O.synth_batch(seed + 5, n, H, W, nicg=1)
    x = (x + 0.02 * np.random.default_rng(seed).uniform(size=x.shape)).astype(np.float32)
    PQ = O.round_kernels_bf16(P4)
    with torch.no_grad():
        want_s = storage_graph_softmax(O.to_torch(PQ, torch.float32), torch.from_numpy(x),
                                       torch.from_numpy(np.asarray(z, np.float32)))
    want_w = O.g_predict(PQ, x, z, nicg=1, nc_out=4, head="softmax")
    want_f = O.g_predict(P4, x, z, nicg=1, nc_out=4, head="softmax")
    return P4, x, z, want_s, want_w, want_f


def test_bf16_storage_predict_48x80(lib):
    """inference_copy('bfloat16') (predict on the bf16 pipe with bf16 activation storage) at 48x80, by the criterion
    test_gpu_bf16_store_uresnet.py derives: no farther from the storage-graph oracle than 2.0 times (max) and 1.5 times
    (mean) the distance between two CPU oracle evaluations, storage graph against weights-only rounding -- and against
    the float32 predict of the same model no farther than the same factors of the distance between the storage-graph
    oracle and the float32 oracle.  Both yardsticks re-measured on the CPU at this size (seed 61, n = 2):
    storage graph vs weights-only max 2.22e-2 mean 1.44e-3; storage graph vs float32 max 2.78e-2 mean
    2.09e-3 (64 x 64: 6.72e-3 / 8.06e-4).  The floor asserted is a tenth of what was found, as there."""
    import dep_gan_im_amd as dg
    from test_gpu_bf16_store import TOL
    H, W = 48, 80
    P4, x, z, want_s, want_w, want_f = bf16_predict_oracles(H, W)
    m = dg.Gen_UNet2D((H, W, 1), nc_out=4)
    m.set_weights(P4)
    p32 = m.predict([x, z])
    fast = m.inference_copy("bfloat16")
    p16 = fast.predict([x, z])
    assert p16.shape == p32.shape == (2, H, W, 4) and fast._ensure_engine(2).forward_storage == "bfloat16"
    (e_s, m_s), (e_round, m_round) = _dist(p16, want_s), _dist(want_s, want_w)
    (e_f, m_f), (ef_round, mf_round) = _dist(p16, p32), _dist(want_s, want_f)
    print("48x80 bf16 storage predict vs storage-graph oracle: max %.3e mean %.3e (the rounding's own effect max %.3e mean "
          "%.3e); vs the float32 predict: max %.3e mean %.3e (oracle: max %.3e mean %.3e); float32 predict vs oracle %.2e"
          % (e_s, m_s, e_round, m_round, e_f, m_f, ef_round, mf_round, _dist(p32, want_f)[0]))
    assert _dist(p32, want_f)[0] < 2e-5
    assert e_round > 0.1 * BF16S_E_ROUND_FOUND and e_round > 10 * TOL
    assert e_s < 2.0 * e_round and m_s < 1.5 * m_round, (e_s, e_round, m_s, m_round)
    assert e_f < 2.0 * ef_round and m_f < 1.5 * mf_round, (e_f, ef_round, m_f, mf_round)

