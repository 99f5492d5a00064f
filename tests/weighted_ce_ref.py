"""The float64 reference of the loss-weight mode (depgan_uresnet_set_loss_weights), shared by the tests of the mode.

The rule, from include/depgan.h: label row t (one-hot; a code equal to the ignore label, or an all-zero row, has t = 0),
pixel weight w_i = sum_k cw[k] t[k], den = the number of pixels with w_i != 0, loss = -sum_i sum_k cw[k] t[k] log r_k /
den with r = clip(p / sum(p), 1e-7, 1 - 1e-7), and 0 for den = 0: Keras 2's weighted objective.

The oracle's own uresnet_grads and OracleUResNet.train_on_batch take no loss, so uresnet_grads_weighted and
WeightedOracleUResNet restate their few lines over O.uresnet_forward_t with this loss in place of
O.keras_categorical_crossentropy_t."""
import numpy as np
import torch

from oracle import depgan_oracle as O


def onehot_rows(codes, n_class, ignore_label=None):
    """codes (any shape, integers) -> float32 one-hot (..., n_class); the ignore label becomes an all-zero row."""
    codes = np.asarray(codes).astype(np.int64)
    keep = np.ones(codes.shape, bool) if ignore_label is None else codes != ignore_label
    safe = np.where(keep, codes, 0)
    assert safe.min() >= 0 and safe.max() < n_class, "a code outside [0, n_class) that is not the ignore label"
    return (np.eye(n_class, dtype=np.float32)[safe] * keep[..., None]).astype(np.float32)


def weighted_ce_t(p, t, cw):
    """(mean loss, den, summed loss) of probabilities p (..., C) against label rows t (..., C) with class weights cw (C),
    all torch tensors of one dtype.  Differentiable in p."""
    wt = t * cw
    den = int(((wt.sum(dim=-1)) != 0).sum())
    q = p / p.sum(dim=-1, keepdim=True)
    r = torch.clamp(q, 1e-7, 1.0 - 1e-7)
    total = -(wt * torch.log(r)).sum()
    return (total / den if den else total * 0.0), den, total


def weighted_ce_np(p, t, cw):
    """The same figures in plain NumPy float64, pixel by pixel sums: (mean loss, den, summed loss)."""
    p, t, cw = (np.asarray(a, np.float64) for a in (p, t, cw))
    p, t = p.reshape(-1, p.shape[-1]), t.reshape(-1, t.shape[-1])
    total, den = 0.0, 0
    r = np.clip(p / p.sum(-1, keepdims=True), 1e-7, 1.0 - 1e-7)
    for i in range(len(p)):
        w_i = 0.0
        for k in range(p.shape[1]):
            w_i += cw[k] * t[i, k]
            total -= cw[k] * t[i, k] * np.log(r[i, k])
        den += w_i != 0
    return (total / den if den else 0.0), den, total


def softmax_ce_weighted_ref(z, t, cw):
    """Operator-level float64 reference on logits z (P, C): (probabilities, dz = d(mean loss)/dz, summed loss, den)."""
    zt = torch.from_numpy(np.asarray(z, np.float32)).double().requires_grad_(True)
    p = torch.softmax(zt, -1)
    loss, den, total = weighted_ce_t(p, torch.from_numpy(np.asarray(t, np.float32)).double(),
                                     torch.from_numpy(np.asarray(cw, np.float64)))
    if den:
        (g,) = torch.autograd.grad(loss, zt)
        g = g.numpy()
    else:
        g = np.zeros(zt.shape, np.float64)
    return p.detach().numpy(), g, float(total.detach()), den


def uresnet_grads_weighted(P, x, z, labels, cw, drop_seed=None, dtype=torch.float32, masks=None):
    """O.uresnet_grads with the weighted loss: labels one-hot (B, H, W, C) with all-zero rows for ignored pixels.
    Returns (loss, grads dict, batch BN stats dict)."""
    T = O.to_torch(P, dtype, requires_grad=True)
    xt, zt, lt = O._t(x, dtype), O._t(z, dtype), O._t(np.asarray(labels, np.float32), dtype)
    keep = None
    if drop_seed is not None:
        B, H, W, _ = xt.shape
        keep = torch.tensor(O.dropout_keep_mask(drop_seed, (B, H // 4, W // 4, 96)))
    stats = {}
    p = O.uresnet_forward_t(T, xt, zt, phase=1, keep_mask=keep, stats=stats, masks=masks)
    loss, _, _ = weighted_ce_t(p, lt, torch.as_tensor(np.asarray(cw, np.float64)).to(dtype))
    names = O.trainable_names(P)
    gs = torch.autograd.grad(loss, [T[n] for n in names], allow_unused=True)
    grads = {n: (g.detach().numpy() if g is not None else np.zeros_like(P[n])) for n, g in zip(names, gs)}
    return float(loss.detach()), grads, stats


def uresnet_eval_weighted(P, x, z, labels, cw):
    """The phase-0 weighted loss in float64."""
    p64 = torch.from_numpy(O.uresnet_predict(P, x, z, dtype=torch.float64))
    loss, _, _ = weighted_ce_t(p64, torch.from_numpy(np.asarray(labels, np.float32)).double(),
                               torch.as_tensor(np.asarray(cw, np.float64)))
    return float(loss)


class WeightedOracleUResNet(O.OracleUResNet):
    """O.OracleUResNet whose train_on_batch takes the weighted loss: the same Adam and moving-average lines."""

    def __init__(self, P, cw, lr=1e-4, dtype=torch.float32):
        super().__init__(P, lr, dtype)
        self.cw = cw

    def train_on_batch(self, inputs, labels, drop_seed=None, masks=None):
        x, z = inputs
        loss, grads, stats = uresnet_grads_weighted(self.P, x, z, labels, self.cw, drop_seed, self.dtype, masks)
        self.last_grads = grads
        self.opt.apply(self.P, grads)
        for name, (mean, var, n, fused) in stats.items():
            corr = n / (n - 1.0) if fused else n / (n - (1.0 + O.BN_EPS))
            mm, mv = self.P[name + "/moving_mean"], self.P[name + "/moving_variance"]
            self.P[name + "/moving_mean"] = (mm * O.BN_MOMENTUM + mean.numpy() * (1 - O.BN_MOMENTUM)).astype(mm.dtype)
            self.P[name + "/moving_variance"] = (mv * O.BN_MOMENTUM + var.numpy() * corr * (1 - O.BN_MOMENTUM)).astype(mv.dtype)
        return loss
