"""NumPy restatement of csrc/surface_dist.hip and of the metric algebra of evaluate.surface_distances.

The squared distance map is defined as the minimum over the set voxels of

    fl(fl(fl(dx^2 wx) + fl(dy^2 wy)) + fl(dz^2 wz))

with the integer squares converted to double exactly and w = (wz, wy, wx) the squared voxel spacings.  NumPy's float64
array arithmetic rounds every product and sum once, so the statements below are that expression tree.
`edt_sq_brute` states it over all set voxels; `edt_sq_separable` is the three-pass form the kernels use, which gives
the same bits because rounding is monotone (tests/test_surface_cpu.py asserts the equality)."""
import math

import numpy as np


def weights(spacing):
    """(wz, wy, wx): the squared spacings as Python floats, the products evaluate.py forms"""
    return tuple(float(s) * float(s) for s in spacing)


def edt_sq_brute(set_, w, chunk=1 << 21):
    """set_: (D, H, W), non-zero = set.  Returns float64 (D, H, W); +inf everywhere when nothing is set."""
    set_ = np.asarray(set_) != 0
    wz, wy, wx = (np.float64(v) for v in w)
    D, H, W = set_.shape
    out = np.full(set_.shape, np.inf, np.float64)
    src = np.argwhere(set_)                                          # (m, 3) in z, y, x
    if not len(src):
        return out
    def term(n, wa):                                                 # [i, i'] = fl((i - i')^2 wa), the square exact
        d = np.arange(n, dtype=np.float64)[:, None] - np.arange(n, dtype=np.float64)[None, :]
        return (d * d) * wa

    tz, ty, tx = term(D, wz), term(H, wy), term(W, wx)
    per = max(1, chunk // set_.size)                                 # set voxels per step: `chunk` candidates
    for i in range(0, len(src), per):
        s = src[i:i + per]
        cz, cy, cx = tz[s[:, 0]], ty[s[:, 1]], tx[s[:, 2]]           # (m, D), (m, H), (m, W): the terms of set voxel m
        cand = (cx[:, None, None, :] + cy[:, None, :, None]) + cz[:, :, None, None]
        np.minimum(out, cand.min(axis=0), out=out)
    return out


def _axis_min(stage, w_axis):
    """stage: (rows, cols) float64.  out[r, c] = min_r' fl(stage[r', c] + fl((r - r')^2 w_axis))"""
    rows = stage.shape[0]
    r = np.arange(rows, dtype=np.float64)
    d = r[:, None] - r[None, :]
    t = (d * d) * np.float64(w_axis)                                 # (r, r')
    out = np.empty_like(stage)
    for i in range(rows):
        out[i] = (stage + t[i][:, None]).min(axis=0)
    return out


def row_distance(set_):
    """Pass 1: per row the distance in voxels to the nearest set voxel of the row, -1 for a row without one."""
    set_ = np.asarray(set_) != 0
    W = set_.shape[-1]
    x = np.arange(W)
    big = 1 << 20
    last = np.maximum.accumulate(np.where(set_, x, -big), axis=-1)
    first = np.minimum.accumulate(np.where(set_, x, big)[..., ::-1], axis=-1)[..., ::-1]
    g = np.minimum(x - last, first - x)
    return np.where(g >= big // 2, -1, g)


def edt_sq_separable(set_, w):
    """The three passes of the kernels: rows, then along H, then along D."""
    wz, wy, wx = (np.float64(v) for v in w)
    g = row_distance(set_)
    D, H, W = g.shape
    gd = g.astype(np.float64)
    stage = np.where(g < 0, np.inf, (gd * gd) * wx)
    F = np.stack([_axis_min(stage[z], wy) for z in range(D)])
    return _axis_min(F.reshape(D, H * W), wz).reshape(D, H, W)


def surface_mask(set_, in_plane):
    """uint8 (D, H, W): set, and a face neighbour (6 in the volume, 4 in the slice) is unset or outside the volume."""
    a = np.asarray(set_) != 0
    p = np.pad(a, 1, constant_values=False)
    c = (slice(1, -1),) * 3
    inner = p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1]
    if not in_plane:
        inner = inner & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1]
    return (p[c] & ~inner).astype(np.uint8)


def surface_sums(d2, surf):
    """What depgan_eval_surface_sums returns, exactly where it is exact: (count, max d2 with 0 for none, the
    math.fsum of the square roots, the number of infinite d2)."""
    v = np.asarray(d2, np.float64)[np.asarray(surf) != 0]
    return (float(v.size), float(v.max()) if v.size else 0.0, math.fsum(np.sqrt(v).tolist()),
            float(np.isinf(v).sum()))


KEYS = ("n_surface_a", "n_surface_b", "hd_ab", "hd_ba", "hd", "msd_ab", "msd_ba", "assd", "hd95_ab", "hd95_ba", "hd95",
        "hd95_pooled")


def surface_distances(a, b, spacing=(1, 1, 1), in_plane=False, percentile=95.0, edt=edt_sq_brute):
    """The metric algebra on the reference distance maps: the dict evaluate.surface_distances returns."""
    w = weights(spacing)
    sa, sb = surface_mask(a, in_plane), surface_mask(b, in_plane)
    na, nb = int(sa.sum()), int(sb.sum())
    out = {k: float("nan") for k in KEYS}
    out["n_surface_a"], out["n_surface_b"] = na, nb
    if na == 0 or nb == 0:
        return out
    s_ab = np.sqrt(edt(sb, w)[sa != 0])
    s_ba = np.sqrt(edt(sa, w)[sb != 0])
    out["hd_ab"], out["hd_ba"] = float(s_ab.max()), float(s_ba.max())
    out["hd"] = max(out["hd_ab"], out["hd_ba"])
    out["msd_ab"], out["msd_ba"] = math.fsum(s_ab.tolist()) / na, math.fsum(s_ba.tolist()) / nb
    out["assd"] = (out["msd_ab"] + out["msd_ba"]) / 2
    out["hd95_ab"], out["hd95_ba"] = float(np.percentile(s_ab, percentile)), float(np.percentile(s_ba, percentile))
    out["hd95"] = max(out["hd95_ab"], out["hd95_ba"])
    out["hd95_pooled"] = float(np.percentile(np.concatenate([s_ab, s_ba]), percentile))
    return out
