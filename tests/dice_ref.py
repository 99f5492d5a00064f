"""The float64 reference of the soft Dice loss (depgan_uresnet_set_dice_loss), shared by the tests of the mode.

The rule, from include/depgan.h: p the softmax probabilities, t the label row, m = 1 for a pixel that takes part;
I_k = sum m t_k p_k, P_k = sum m p_k, T_k = sum m t_k and, with s = smooth (the float32 value the library is given),
    flat:   L = 1 - (2 sum_k I_k + s) / (sum_k T_k + sum_k P_k + s)
    class:  L = sum_k c_k (1 - (2 I_k + s) / (T_k + P_k + s))
The loss of a call is ce_coef * CE + dice_coef * L with CE the loss-weight mode's cross-entropy (weighted_ce_ref).

The oracle's own uresnet_grads and OracleUResNet.train_on_batch take no loss, so uresnet_grads_dice and
uresnet_eval_dice restate their few lines over O.uresnet_forward_t with this loss, as weighted_ce_ref does."""
import numpy as np
import torch

import weighted_ce_ref as R
from oracle import depgan_oracle as O

FORMS = ("flat", "class")


def class_coef(n_class, which=None):
    """The class form's coefficients as the library rounds them: None -> float32(1) / float32(C) each; 'foreground' ->
    c_0 = 0 and float32(1 / (C - 1)) elsewhere; an array -> its float32 values.  Returned as float64."""
    if which is None:
        c = np.full(n_class, np.float32(1.0) / np.float32(n_class), np.float32)
    elif isinstance(which, str):
        assert which == "foreground"
        c = np.full(n_class, 1.0 / (n_class - 1), np.float64).astype(np.float32)
        c[0] = 0.0
    else:
        c = np.asarray(which, np.float32).reshape(-1)
        assert c.size == n_class
    return c.astype(np.float64)


def dice_t(p, t, keep, form, coef, smooth):
    """The Dice term of probabilities p (..., C) against label rows t (..., C); keep (...) is m as a 0 / 1 tensor, coef
    the C class coefficients (class form; not read for the flat form).  torch tensors of one dtype, differentiable in
    p.  Returns (L, I, P, T) with the sums as (C,) tensors."""
    assert form in FORMS
    C = p.shape[-1]
    m = keep.reshape(-1, 1).to(p.dtype)
    p2, t2 = p.reshape(-1, C), t.reshape(-1, C)
    I, Pk, T = (m * t2 * p2).sum(0), (m * p2).sum(0), (m * t2).sum(0)
    s = float(np.float32(smooth))
    if form == "flat":
        L = 1.0 - (2.0 * I.sum() + s) / (T.sum() + Pk.sum() + s)
    else:
        L = (coef.to(p.dtype) * (1.0 - (2.0 * I + s) / (T + Pk + s))).sum()
    return L, I, Pk, T


def dice_ref(z, t, keep, form, coef, smooth):
    """Operator level, float64 autograd on logits z (P, C): (probabilities, dL/dz, L, sums (3, C) = I, P, T)."""
    zt = torch.from_numpy(np.asarray(z, np.float32)).double().requires_grad_(True)
    p = torch.softmax(zt, -1)
    L, I, Pk, T = dice_t(p, torch.from_numpy(np.asarray(t, np.float32)).double(),
                         torch.from_numpy(np.asarray(keep, np.float64)), form,
                         None if coef is None else torch.from_numpy(np.asarray(coef, np.float64)), smooth)
    (g,) = torch.autograd.grad(L, zt)
    return p.detach().numpy(), g.numpy(), float(L.detach()), np.stack([v.detach().numpy() for v in (I, Pk, T)])


def dice_closed_form(p, t, keep, form, coef, smooth):
    """The same figures in plain NumPy float64 from probabilities p (P, C), by the closed form: dL/dp_k = m (A_k t_k +
    B_k), class form A_k = -2 c_k / Den_k and B_k = c_k Num_k / Den_k^2, flat form the same with the global Num, Den and
    c_k = 1; dL/dz_k = p_k (g_k - sum_j p_j g_j).  Returns (dL/dz, L, sums (3, C), A, B)."""
    assert form in FORMS
    p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
    m = np.asarray(keep, np.float64).reshape(-1, 1)
    C = p.shape[1]
    I, Pk, T = (m * t * p).sum(0), (m * p).sum(0), (m * t).sum(0)
    s = float(np.float32(smooth))
    if form == "flat":
        num, den = 2.0 * I.sum() + s, T.sum() + Pk.sum() + s
        L = 1.0 - num / den
        A, B = np.full(C, -2.0 / den), np.full(C, num / den ** 2)
    else:
        c = np.asarray(coef, np.float64)
        num, den = 2.0 * I + s, T + Pk + s
        L = float((c * (1.0 - num / den)).sum())
        A, B = -2.0 * c / den, c * num / den ** 2
    g = m * (A * t + B)
    dz = p * (g - (p * g).sum(-1, keepdims=True))
    return dz, float(L), np.stack([I, Pk, T]), A, B


def keep_rows(t):
    """m of one-hot rows under the loss-weight mode: a pixel with an all-zero row takes no part."""
    t = np.asarray(t)
    return (t != 0).any(-1).astype(np.float64)


def combined_loss_t(p, lt, cw, dice, dtype):
    """ce_coef * weighted CE + dice_coef * Dice of probabilities p against one-hot rows lt (all-zero rows ignored);
    dice = dict(form, coef, smooth, ce_coef, dice_coef), cw the class weights of the cross-entropy."""
    keep = (lt != 0).any(-1).to(dtype)
    L, _, _, _ = dice_t(p, lt, keep, dice["form"], None if dice["coef"] is None else
                        torch.as_tensor(np.asarray(dice["coef"], np.float64)).to(dtype), dice["smooth"])
    loss = dice["dice_coef"] * L
    if dice["ce_coef"] != 0:
        ce, _, _ = R.weighted_ce_t(p, lt, torch.as_tensor(np.asarray(cw, np.float64)).to(dtype))
        loss = loss + dice["ce_coef"] * ce
    return loss


def uresnet_grads_dice(P, x, z, labels, cw, dice, drop_seed=None, dtype=torch.float32, masks=None):
    """O.uresnet_grads with ce_coef * weighted CE + dice_coef * Dice: labels one-hot (B, H, W, C) with all-zero rows for
    ignored pixels (with the loss-weight mode off no row is zero, every pixel is in the Dice sums and cw is ones).
    Returns (loss, grads dict, batch BN stats dict)."""
    T = O.to_torch(P, dtype, requires_grad=True)
    xt, zt, lt = O._t(x, dtype), O._t(z, dtype), O._t(np.asarray(labels, np.float32), dtype)
    keep = None
    if drop_seed is not None:
        B, H, W, _ = xt.shape
        keep = torch.tensor(O.dropout_keep_mask(drop_seed, (B, H // 4, W // 4, 96)))
    stats = {}
    p = O.uresnet_forward_t(T, xt, zt, phase=1, keep_mask=keep, stats=stats, masks=masks)
    loss = combined_loss_t(p, lt, cw, dice, dtype)
    names = O.trainable_names(P)
    gs = torch.autograd.grad(loss, [T[n] for n in names], allow_unused=True)
    grads = {n: (g.detach().numpy() if g is not None else np.zeros_like(P[n])) for n, g in zip(names, gs)}
    return float(loss.detach()), grads, stats


def uresnet_eval_dice(P, x, z, labels, cw, dice):
    """The phase-0 combined loss in float64."""
    p64 = torch.from_numpy(O.uresnet_predict(P, x, z, dtype=torch.float64))
    lt = torch.from_numpy(np.asarray(labels, np.float32)).double()
    return float(combined_loss_t(p64, lt, cw, dice, torch.float64))


class DiceOracleUResNet(R.WeightedOracleUResNet):
    """O.OracleUResNet whose train_on_batch takes the combined loss: the same Adam and moving-average lines."""

    def __init__(self, P, cw, dice, lr=1e-4, dtype=torch.float32):
        super().__init__(P, cw, lr, dtype)
        self.dice = dice

    def train_on_batch(self, inputs, labels, drop_seed=None, masks=None):
        x, z = inputs
        loss, grads, stats = uresnet_grads_dice(self.P, x, z, labels, self.cw, self.dice, drop_seed, self.dtype, masks)
        self.last_grads = grads
        self.opt.apply(self.P, grads)
        for name, (mean, var, n, fused) in stats.items():
            corr = n / (n - 1.0) if fused else n / (n - (1.0 + O.BN_EPS))
            mm, mv = self.P[name + "/moving_mean"], self.P[name + "/moving_variance"]
            self.P[name + "/moving_mean"] = (mm * O.BN_MOMENTUM + mean.numpy() * (1 - O.BN_MOMENTUM)).astype(mm.dtype)
            self.P[name + "/moving_variance"] = (mv * O.BN_MOMENTUM + var.numpy() * corr * (1 - O.BN_MOMENTUM)).astype(mv.dtype)
        return loss
