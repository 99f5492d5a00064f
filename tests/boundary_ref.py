"""NumPy / float64 restatement of the boundary loss (depgan_uresnet_set_boundary_loss), shared by the tests of the mode.

The rule, from include/depgan.h.  Per slice and class k, S = the pixels whose true class is k; d2 of a pixel in S is
surface_ref.edt_sq_brute of the complement of S on the slice as a (1, H, W) volume, d2 of a pixel outside S that of S,
with the weights (1, sy^2, sx^2).  phi = float32(sqrt(d2)) outside, float32(-(sqrt(d2) - inside_offset)) inside, 0 for an
infinite d2.  L_B = (1/M) sum_x m sum_k c_k phi_k p_k; g_k = m c_k phi_k / M; dz_j += coef p_j (g_j - sum_k p_k g_k).

Following dice_ref: combined_loss_t and the oracle wrappers restate the oracle's gradient and Adam lines with
ce + Dice + boundary_coef L_B."""
import numpy as np
import torch

import dice_ref as D
import surface_ref as S
import weighted_ce_ref as R
from oracle import depgan_oracle as O

NO_CLASS = -1


def true_class(labels, n_class, ignore=-1):
    """(n, H, W) int64 true classes, NO_CLASS for a pixel without one.  labels: class codes (n, H, W) -- the ignore code
    and any code >= n_class have no class -- or one-hot rows (n, H, W, C): the first arg-max, and with ignore >= 0 an
    all-zero row has no class (with ignore < 0 it is class 0)."""
    a = np.asarray(labels)
    if a.ndim == 4:
        tc = np.argmax(a, axis=-1).astype(np.int64)
        if ignore >= 0:
            tc[~(a != 0).any(-1)] = NO_CLASS
        return tc
    tc = a.astype(np.int64)
    return np.where((tc == ignore) | (tc >= n_class), NO_CLASS, tc)


def signed_distance(tc, n_class, spacing=(1.0, 1.0), inside_offset=0.0, class_on=None):
    """phi (n, H, W, C) float32 of true classes tc (n, H, W): per slice, from surface_ref.edt_sq_brute."""
    tc = np.asarray(tc)
    n, H, W = tc.shape
    w = (1.0,) + S.weights(spacing)
    phi = np.zeros((n, H, W, n_class), np.float32)
    for k in range(n_class):
        if class_on is not None and not class_on[k]:
            continue
        for s in range(n):
            inside = tc[s] == k
            to_set = S.edt_sq_brute(inside[None], w)[0]              # for the pixels outside S
            to_rest = S.edt_sq_brute(~inside[None], w)[0]            # for the pixels inside S
            d2 = np.where(inside, to_rest, to_set)
            with np.errstate(invalid="ignore"):
                d = np.sqrt(d2)
                v = np.where(inside, -(d - np.float64(inside_offset)), d)
            phi[s, :, :, k] = np.where(np.isinf(d2), 0.0, v).astype(np.float32)
    return phi


def class_coef(n_class, which=None):
    """the coefficients as the library rounds them (dice_ref.class_coef: None, 'foreground' or an array), float64"""
    return D.class_coef(n_class, which)


def boundary_np(p, phi, keep, coef):
    """Float64, from probabilities p (P, C), phi (P, C), m = keep (P) and the C coefficients:
    (dL_B/dz (P, C), L_B, M, sum |terms| / M) -- the last is the scale the loss's tolerance is taken from."""
    p, phi = np.asarray(p, np.float64), np.asarray(phi, np.float64)
    m = np.asarray(keep, np.float64).reshape(-1, 1)
    c = np.asarray(coef, np.float64)
    M = float(m.sum())
    if M == 0:
        return np.zeros_like(p), 0.0, 0.0, 0.0
    terms = m * c * phi * p
    g = m * c * phi / M
    dz = p * (g - (p * g).sum(-1, keepdims=True))
    return dz, float(terms.sum() / M), M, float(np.abs(terms).sum() / M)


def boundary_t(p, phi, keep, coef):
    """L_B as a torch scalar, differentiable in p: p, phi (..., C), keep (...) and coef (C) tensors of one dtype."""
    C = p.shape[-1]
    m = keep.reshape(-1, 1).to(p.dtype)
    M = m.sum()
    if float(M) == 0:
        return (p * 0.0).sum()
    return (m * coef.to(p.dtype) * phi.reshape(-1, C).to(p.dtype) * p.reshape(-1, C)).sum() / M


def combined_loss_t(p, lt, cw, dice, boundary, dtype):
    """The loss of a call with the boundary mode on: (the weighted cross-entropy, or dice_ref's combination when `dice`
    is given) + boundary['coef'] * L_B.  lt: one-hot rows with all-zero rows for the pixels without a true class;
    boundary = dict(coef, class_coef (C), phi (the float32 maps of these labels, any shape ending in C))."""
    if dice is None:
        loss, _, _ = R.weighted_ce_t(p, lt, torch.as_tensor(np.asarray(cw, np.float64)).to(dtype))
    else:
        loss = D.combined_loss_t(p, lt, cw, dice, dtype)
    keep = (lt != 0).any(-1).to(dtype)
    lb = boundary_t(p, torch.as_tensor(np.asarray(boundary["phi"], np.float64)).to(dtype), keep,
                    torch.as_tensor(np.asarray(boundary["class_coef"], np.float64)).to(dtype))
    return loss + boundary["coef"] * lb


def uresnet_grads_boundary(P, x, z, labels, cw, dice, boundary, drop_seed=None, dtype=torch.float32, masks=None):
    """dice_ref.uresnet_grads_dice with the boundary term added: (loss, grads dict, batch BN stats dict)."""
    T = O.to_torch(P, dtype, requires_grad=True)
    xt, zt, lt = O._t(x, dtype), O._t(z, dtype), O._t(np.asarray(labels, np.float32), dtype)
    keep = None
    if drop_seed is not None:
        B, H, W, _ = xt.shape
        keep = torch.tensor(O.dropout_keep_mask(drop_seed, (B, H // 4, W // 4, 96)))
    stats = {}
    p = O.uresnet_forward_t(T, xt, zt, phase=1, keep_mask=keep, stats=stats, masks=masks)
    loss = combined_loss_t(p, lt, cw, dice, boundary, dtype)
    names = O.trainable_names(P)
    gs = torch.autograd.grad(loss, [T[n] for n in names], allow_unused=True)
    grads = {n: (g.detach().numpy() if g is not None else np.zeros_like(P[n])) for n, g in zip(names, gs)}
    return float(loss.detach()), grads, stats


def uresnet_eval_boundary(P, x, z, labels, cw, dice, boundary):
    """The phase-0 loss with the boundary term, in float64."""
    p64 = torch.from_numpy(O.uresnet_predict(P, x, z, dtype=torch.float64))
    lt = torch.from_numpy(np.asarray(labels, np.float32)).double()
    return float(combined_loss_t(p64, lt, cw, dice, boundary, torch.float64))


class BoundaryOracleUResNet(R.WeightedOracleUResNet):
    """O.OracleUResNet whose train_on_batch takes the loss with the boundary term: the same Adam and moving-average
    lines."""

    def __init__(self, P, cw, dice, boundary, lr=1e-4, dtype=torch.float32):
        super().__init__(P, cw, lr, dtype)
        self.dice, self.boundary = dice, boundary

    def train_on_batch(self, inputs, labels, drop_seed=None, masks=None):
        x, z = inputs
        loss, grads, stats = uresnet_grads_boundary(self.P, x, z, labels, self.cw, self.dice, self.boundary, drop_seed,
                                                    self.dtype, masks)
        self.last_grads = grads
        self.opt.apply(self.P, grads)
        for name, (mean, var, n, fused) in stats.items():
            corr = n / (n - 1.0) if fused else n / (n - (1.0 + O.BN_EPS))
            mm, mv = self.P[name + "/moving_mean"], self.P[name + "/moving_variance"]
            self.P[name + "/moving_mean"] = (mm * O.BN_MOMENTUM + mean.numpy() * (1 - O.BN_MOMENTUM)).astype(mm.dtype)
            self.P[name + "/moving_variance"] = (mv * O.BN_MOMENTUM + var.numpy() * corr * (1 - O.BN_MOMENTUM)).astype(mv.dtype)
        return loss
