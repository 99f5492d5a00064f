"""The float64 reference of the focal mode (depgan_uresnet_set_focal), shared by the tests of the mode.

The rule, from include/depgan.h: label row t (one-hot; a code equal to the ignore label, or an all-zero row, has t = 0),
class weights cw, C classes, q = p / sum(p), r = clip(q, 1e-7, 1 - 1e-7):

    w_i  = sum_k cw[k] t[k]
    has  = any t[k] != 0
    ts_k = w_i ((1 - eps) t[k] + (has ? eps / C : 0))
    L_i  = -sum_k ts_k (1 - r_k)^gamma log r_k
    loss = sum_i L_i / den,  den = the number of pixels with w_i != 0, and 0 for den = 0

focal_ce_t states it in torch (differentiable: the gradient is autograd's, clamp passing on the closed interval),
focal_ce_np pixel by pixel in NumPy float64, softmax_ce_focal_f32 as the float32 statements of the kernel, the gradient
written out.  uresnet_grads_focal, uresnet_eval_focal and FocalOracleUResNet restate the few lines of their
counterparts in weighted_ce_ref.py with this loss."""
import functools

import numpy as np
import torch

from oracle import depgan_oracle as O

from weighted_ce_ref import onehot_rows  # noqa: F401  (the tests of the mode take it from here)


def focal_ce_t(p, t, cw, gamma, eps):
    """(mean loss, den, summed loss) of probabilities p (..., C) against label rows t (..., C) with class weights cw (C),
    all torch tensors of one dtype; gamma and eps Python floats.  Differentiable in p."""
    Cc = p.shape[-1]
    w = (t * cw).sum(dim=-1)
    has = (t != 0).any(dim=-1)
    ts = w[..., None] * ((1.0 - eps) * t + has[..., None].to(p.dtype) * (eps / Cc))
    den = int((w != 0).sum())
    q = p / p.sum(dim=-1, keepdim=True)
    r = torch.clamp(q, 1e-7, 1.0 - 1e-7)
    total = -(ts * (1.0 - r) ** gamma * torch.log(r)).sum()
    return (total / den if den else total * 0.0), den, total


def focal_ce_np(p, t, cw, gamma, eps):
    """The same figures in plain NumPy float64, pixel by pixel sums: (mean loss, den, summed loss)."""
    p, t, cw = (np.asarray(a, np.float64) for a in (p, t, cw))
    p, t = p.reshape(-1, p.shape[-1]), t.reshape(-1, t.shape[-1])
    Cc = p.shape[1]
    total, den = 0.0, 0
    r = np.clip(p / p.sum(-1, keepdims=True), 1e-7, 1.0 - 1e-7)
    for i in range(len(p)):
        w_i, has = 0.0, False
        for k in range(Cc):
            w_i += cw[k] * t[i, k]
            has = has or t[i, k] != 0
        for k in range(Cc):
            ts = w_i * ((1.0 - eps) * t[i, k] + (eps / Cc if has else 0.0))
            total -= ts * (1.0 - r[i, k]) ** gamma * np.log(r[i, k])
        den += w_i != 0
    return (total / den if den else 0.0), den, total


def softmax_ce_focal_ref(z, t, cw, gamma, eps):
    """Operator-level float64 reference on logits z (P, C): (probabilities, dz = d(mean loss)/dz, summed loss, den)."""
    zt = torch.from_numpy(np.array(z, np.float32)).double().requires_grad_(True)
    p = torch.softmax(zt, -1)
    loss, den, total = focal_ce_t(p, torch.from_numpy(np.asarray(t, np.float32)).double(),
                                  torch.from_numpy(np.asarray(cw, np.float64)), float(gamma), float(eps))
    if den:
        (g,) = torch.autograd.grad(loss, zt)
        g = g.numpy()
    else:
        g = np.zeros(zt.shape, np.float64)
    return p.detach().numpy(), g, float(total.detach()), den


def softmax_ce_focal_f32(z, t, cw, gamma, eps):
    """The statements of the rule in NumPy float32, 1 - r formed directly and the gradient written out (dL/dq, q = p / S,
    the softmax Jacobian): (probabilities, dz, summed loss, den).  What float32 can reach: the CPU test holds it to a
    quarter of the kernel's float64 bounds."""
    f = np.float32
    z, t, cw = np.asarray(z, f), np.asarray(t, f), np.asarray(cw, f)
    Cc = z.shape[1]
    gamma, eps = f(gamma), f(eps)
    e = np.exp(z - z.max(-1, keepdims=True))
    S0 = np.zeros(len(z), f)
    for k in range(Cc):
        S0 = S0 + e[:, k]
    p = e / S0[:, None]
    w = np.zeros(len(z), f)
    for k in range(Cc):
        w = w + cw[k] * t[:, k]
    has = (t != 0).any(-1)
    den = int((w != 0).sum())
    inv = f(1.0) / f(den) if den else f(0.0)
    ts = w[:, None] * ((f(1.0) - eps) * t + np.where(has, eps / f(Cc), f(0.0))[:, None])
    S = p[:, 0] + p[:, 1]
    for k in range(2, Cc - 1, 2):
        S = S + (p[:, k] + p[:, k + 1])
    if Cc & 1:
        S = S + p[:, Cc - 1]
    q = p / S[:, None]
    r = np.clip(q, f(1e-7), f(1.0) - f(1e-7))
    om, lg = f(1.0) - r, np.log(r)
    pw = np.power(om, gamma)
    total = float(np.sum(-(ts * pw * lg), dtype=f))
    inside = (q >= f(1e-7)) & (q <= f(1.0) - f(1e-7))
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):     # outside the clip, where the value is dropped
        gq = np.where(inside, -ts * inv * (pw / q - gamma * (pw / om) * lg), f(0.0)).astype(f)
    dot = np.zeros(len(z), f)
    for k in range(Cc):
        dot = dot + gq[:, k] * p[:, k]
    gp = gq / S[:, None] - (dot / (S * S))[:, None]
    pg = np.zeros(len(z), f)
    for k in range(Cc):
        pg = pg + p[:, k] * gp[:, k]
    dz = p * (gp - pg[:, None])
    assert p.dtype == f and dz.dtype == f
    return p, dz, total, den


@functools.lru_cache(maxsize=None)
def ref_case(Cc):
    """The inputs of the float64 comparisons, those of the loss-weight mode's operator test (its `_ref_case(C, C - 1)` with
    ignore code 255): 12000 rows of 3 sigma normal logits with ties, all-equal rows and +-100 spreads, 1000 rows on either
    side of 1 - 1e-7 for the true class C - 1 and 1000 on either side of 1e-7, a rare last class, 30 % of the pixels marked
    255, class 0 at weight 0 and class C - 1 at 7.25.  Returns (logits, codes, class weights); read-only."""
    rng = np.random.default_rng(500 + Cc)
    P, hi = 12000, Cc - 1
    z = (3.0 * rng.standard_normal((P, Cc))).astype(np.float32)
    share = np.full(Cc, 0.99 / (Cc - 1))
    share[Cc - 1] = 0.01
    codes = rng.choice(Cc, size=P, p=share).astype(np.uint8)
    r = np.arange(P)
    tie = r[r % 11 == 1]
    z[tie, 0] = z[tie, Cc - 1] = (z[tie].max(-1) + np.float32(0.75)).astype(np.float32)
    z[r % 11 == 2] = np.float32(0.3125)
    z[r % 11 == 3] *= np.float32(100.0 / 3.0)
    g = np.linspace(14.0, 19.5, 1000, dtype=np.float32)
    z[:1000] = 0.0
    z[:1000, hi] = g
    codes[:1000] = hi
    z[1000:2000] = 0.0
    z[1000:2000, Cc - 1] = -g
    codes[1000:2000] = Cc - 1
    w = np.array([0.0, 1.25, 0.7, 3.0, 0.5, 1.0, 2.0, 7.25], np.float32)[:Cc]
    w[Cc - 1] = 7.25
    mark = np.random.default_rng(Cc).uniform(size=P) < 0.3
    mark[:2000:2] = False
    codes[mark] = 255
    for a in (z, codes, w):
        a.setflags(write=False)
    return z, codes, w


def uresnet_grads_focal(P, x, z, labels, cw, gamma, eps, drop_seed=None, dtype=torch.float32, masks=None):
    """O.uresnet_grads with the focal loss: labels one-hot (B, H, W, C) with all-zero rows for ignored pixels.
    Returns (loss, grads dict, batch BN stats dict)."""
    T = O.to_torch(P, dtype, requires_grad=True)
    xt, zt, lt = O._t(x, dtype), O._t(z, dtype), O._t(np.asarray(labels, np.float32), dtype)
    keep = None
    if drop_seed is not None:
        B, H, W, _ = xt.shape
        keep = torch.tensor(O.dropout_keep_mask(drop_seed, (B, H // 4, W // 4, 96)))
    stats = {}
    p = O.uresnet_forward_t(T, xt, zt, phase=1, keep_mask=keep, stats=stats, masks=masks)
    loss, _, _ = focal_ce_t(p, lt, torch.as_tensor(np.asarray(cw, np.float64)).to(dtype), float(gamma), float(eps))
    names = O.trainable_names(P)
    gs = torch.autograd.grad(loss, [T[n] for n in names], allow_unused=True)
    grads = {n: (g.detach().numpy() if g is not None else np.zeros_like(P[n])) for n, g in zip(names, gs)}
    return float(loss.detach()), grads, stats


def uresnet_eval_focal(P, x, z, labels, cw, gamma, eps):
    """The phase-0 focal loss in float64."""
    p64 = torch.from_numpy(O.uresnet_predict(P, x, z, dtype=torch.float64))
    loss, _, _ = focal_ce_t(p64, torch.from_numpy(np.asarray(labels, np.float32)).double(),
                            torch.as_tensor(np.asarray(cw, np.float64)), float(gamma), float(eps))
    return float(loss)


class FocalOracleUResNet(O.OracleUResNet):
    """O.OracleUResNet whose train_on_batch takes the focal loss: the same Adam and moving-average lines."""

    def __init__(self, P, cw, gamma, eps, lr=1e-4, dtype=torch.float32):
        super().__init__(P, lr, dtype)
        self.cw, self.gamma, self.eps = cw, gamma, eps

    def train_on_batch(self, inputs, labels, drop_seed=None, masks=None):
        x, z = inputs
        loss, grads, stats = uresnet_grads_focal(self.P, x, z, labels, self.cw, self.gamma, self.eps, drop_seed,
                                                 self.dtype, masks)
        self.last_grads = grads
        self.opt.apply(self.P, grads)
        for name, (mean, var, n, fused) in stats.items():
            corr = n / (n - 1.0) if fused else n / (n - (1.0 + O.BN_EPS))
            mm, mv = self.P[name + "/moving_mean"], self.P[name + "/moving_variance"]
            self.P[name + "/moving_mean"] = (mm * O.BN_MOMENTUM + mean.numpy() * (1 - O.BN_MOMENTUM)).astype(mm.dtype)
            self.P[name + "/moving_variance"] = (mv * O.BN_MOMENTUM + var.numpy() * corr * (1 - O.BN_MOMENTUM)).astype(mv.dtype)
        return loss
