"""NumPy float64 restatement of the Adam update with options (include/depgan.h, depgan_set_optimizer): global norm,
scale, clipvalue, decoupled decay, then Keras Adam.  Every operation is carried out in float64; the constants are the
float32 values the kernel holds (beta_1, beta_2, 1 - beta in float32 as Keras forms it, eps, lr_t, lr * weight_decay),
so the difference to the kernel is the kernel's float32 rounding alone."""
import math

import numpy as np


def scaled(g, gscale=1.0):
    """g * gscale as the float32 product both kernels form, widened to float64."""
    return (np.asarray(g, np.float32) * np.float32(gscale)).astype(np.float64)


def sqnorm(g, gscale=1.0):
    return float(np.sum(scaled(g, gscale) ** 2))


def clip_scale(norm, clipnorm):
    """Standalone Keras 2's clipnorm: g * c / norm once norm >= c; the factor rounded to float32 as the kernel holds it."""
    if clipnorm > 0 and norm >= np.float32(clipnorm):
        return float(np.float32(float(np.float32(clipnorm)) / norm))
    return 1.0


def lr_t(lr, b1, b2, t):
    """The host's bias-corrected rate, in double from the float32 lr and betas, rounded to float32."""
    lr, b1, b2 = float(np.float32(lr)), float(np.float32(b1)), float(np.float32(b2))
    return float(np.float32(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)))


def adam_opts_step(p, g, m, v, t, lr, b1, b2, eps=1e-7, gscale=1.0, clipnorm=0.0, clipvalue=0.0, weight_decay=0.0,
                   decay=None, scale=None):
    """One update of flat float64 p, m, v (step counter t >= 1) from the gradient g.  decay: boolean mask of the
    decayed elements.  scale: the clip factor to use instead of the one computed here (the float32 value the library
    reports).  Returns (p, m, v, norm, scale); a norm that is not finite returns p, m, v unchanged and scale 0."""
    p, m, v = (np.array(a, np.float64) for a in (p, m, v))
    gi = scaled(g, gscale)
    norm, s = 0.0, 1.0
    if clipnorm > 0:
        with np.errstate(over="ignore", invalid="ignore"):
            sq = float(np.sum(gi ** 2))
        norm = math.sqrt(sq) if sq == sq and sq >= 0 else float("nan")
        if not math.isfinite(sq):
            return p, m, v, norm, 0.0
        s = clip_scale(norm, clipnorm) if scale is None else float(scale)
    gi = gi * s
    if clipvalue > 0:
        a = float(np.float32(clipvalue))
        gi = np.minimum(np.maximum(gi, -a), a)
    if weight_decay > 0:
        lrwd = float(np.float32(lr) * np.float32(weight_decay))
        p = np.where(np.asarray(decay, bool), p - lrwd * p, p)
    b1f, b2f = np.float32(b1), np.float32(b2)
    omb1, omb2 = float(np.float32(1.0) - b1f), float(np.float32(1.0) - b2f)
    m = float(b1f) * m + omb1 * gi
    v = float(b2f) * v + omb2 * gi * gi
    p = p - lr_t(lr, b1, b2, t) * m / (np.sqrt(v) + float(np.float32(eps)))
    return p, m, v, norm, s
