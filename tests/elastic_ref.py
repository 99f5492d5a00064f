"""NumPy restatement of depgan_data_augment_fields (include/depgan.h), operation for operation.

elastic_ref(..., dtype=np.float32) casts every operand to float32, so each NumPy operation is the one correctly rounded
float32 operation the kernel performs and the result is expected bit for bit (a NaN by its position: the payload of a
NaN an operation makes is the processor's).  dtype=np.float64 is the identical statement sequence in float64 on the same
float32 parameters, control values and ky / kx: the yardstick for the float32 rounding error.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from augment_ref import augment_ref  # noqa: E402,F401  (the zero-grid yardstick of the tests)

MAX_GRID = 32


def spline_step(g, size):
    """ky / kx of the header: control cells per pixel, computed in double and rounded once to float32"""
    return np.float32((g - 3) / (size - 1)) if size > 1 else np.float32(0)


def spline_axis(size, g, f):
    """cells (size,) int64 and the four weight arrays (six times the B-spline weights) of the pixels 0..size-1"""
    o = np.arange(size).astype(f)
    u = o * f(spline_step(g, size))
    c = np.minimum(np.floor(u), f(g - 4))
    t = u - c
    t2 = t * t
    t3 = t2 * t
    gt = f(1) - t
    B0 = (gt * gt) * gt
    B1 = (f(3) * t3 - f(6) * t2) + f(4)
    B2 = ((f(3) * t2 - f(3) * t3) + f(3) * t) + f(1)
    B3 = t3
    assert t.dtype == f and B2.dtype == f
    return c.astype(np.int64), (B0, B1, B2, B3), t


def dense_fields(grid, H, W, dtype=np.float32):
    """grid (3, gh, gw) float32 -> (H, W, 3) of `dtype`: the three planes at every output pixel"""
    f = dtype
    grid = np.asarray(grid, np.float32)
    _, gh, gw = grid.shape
    assert 4 <= gh <= MAX_GRID and 4 <= gw <= MAX_GRID
    C = grid.astype(f)
    cy, By, _ = spline_axis(H, gh, f)
    cx, Bx, _ = spline_axis(W, gw, f)
    By = [b[:, None] for b in By]
    Bx = [b[None, :] for b in Bx]
    yy, xx = cy[:, None], cx[None, :]
    out = np.empty((H, W, 3), f)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(3):
            Cp = C[p]
            r = [((By[0] * Cp[yy, xx + j] + By[1] * Cp[yy + 1, xx + j]) + By[2] * Cp[yy + 2, xx + j])
                 + By[3] * Cp[yy + 3, xx + j] for j in range(4)]
            val = (((Bx[0] * r[0] + Bx[1] * r[1]) + Bx[2] * r[2]) + Bx[3] * r[3]) * (f(1) / f(36))
            assert val.dtype == f
            out[..., p] = val
    return out


def _tap(fl, n):
    """integral-valued float coordinates (or +-inf / NaN) -> (index clamped into [0, n), inside mask): compared and
    clamped as floats before the cast; a NaN clamps to 0 and is outside, as fminf(fmaxf(f, 0), n - 1) makes it"""
    inside = (fl >= 0) & (fl <= n - 1)
    clamped = np.where(np.isnan(fl), 0, np.clip(fl, 0, n - 1))
    return clamped.astype(np.int64), inside


def elastic_ref(x, labels, params, fields, index=None, border="edge", x_fill=0.0, label_fill=0, dtype=np.float32):
    """x (n_src, H, W, nicg); labels None, codes (n_src, H, W) uint8 or one-hot (n_src, H, W, C) float32;
    params (n, 8) float32; fields (n, 3, gh, gw) float32.
    Returns (x_out (n, H, W, nicg) of `dtype`, labels_out or None, dense (n, H, W, 3) of `dtype`)."""
    f = dtype
    x = np.asarray(x)
    n_src, H, W, nicg = x.shape
    params = np.asarray(params, np.float32)
    fields = np.asarray(fields, np.float32)
    n = len(params)
    assert fields.shape[:2] == (n, 3)
    index = np.arange(n) if index is None else np.asarray(index)
    constant = {"edge": False, "constant": True}[border]
    oy, ox = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    oy, ox = oy.astype(f), ox.astype(f)
    one, half, fill = f(1), f(0.5), f(x_fill)
    out = np.empty((n, H, W, nicg), f)
    dense = np.zeros((n, H, W, 3), f)
    lab_out = None
    if labels is not None:
        labels = np.asarray(labels)
        lab_out = np.empty((n,) + labels.shape[1:], labels.dtype)
        if labels.ndim == 3:
            fill_row = labels.dtype.type(label_fill)
        else:
            fill_row = np.zeros(labels.shape[3], labels.dtype)
            if label_fill >= 0:
                fill_row[label_fill] = 1
    for i in range(n):
        s = int(index[i])
        if not 0 <= s < n_src:
            out[i] = fill
            if labels is not None:
                lab_out[i] = fill_row
            continue
        dense[i] = d = dense_fields(fields[i], H, W, f)
        a00, a01, a02, a10, a11, a12, gain, offset = (f(v) for v in params[i])
        with np.errstate(invalid="ignore", over="ignore"):
            sy = ((a00 * oy + a01 * ox) + a02) + d[..., 0]
            sx = ((a10 * oy + a11 * ox) + a12) + d[..., 1]
            bias = one + d[..., 2]
            y0, x0 = np.floor(sy), np.floor(sx)
            fy, fx = sy - y0, sx - x0
            gy, gx = one - fy, one - fx
            ty0, iy0 = _tap(y0, H)
            ty1, iy1 = _tap(y0 + one, H)
            tx0, ix0 = _tap(x0, W)
            tx1, ix1 = _tap(x0 + one, W)
            img = x[s].astype(f)

            def v(ty, iy, tx, ix):
                val = img[ty, tx]
                return np.where((iy & ix)[..., None], val, fill) if constant else val

            fxc, gxc, fyc, gyc = fx[..., None], gx[..., None], fy[..., None], gy[..., None]
            top = v(ty0, iy0, tx0, ix0) * gxc + v(ty0, iy0, tx1, ix1) * fxc
            bot = v(ty1, iy1, tx0, ix0) * gxc + v(ty1, iy1, tx1, ix1) * fxc
            res = gain * ((top * gyc + bot * fyc) * bias[..., None]) + offset
            assert res.dtype == f
            out[i] = res
            if labels is not None:
                ly, iy = _tap(np.floor(sy + half), H)
                lx, ix = _tap(np.floor(sx + half), W)
                got = labels[s][ly, lx]
                if constant:
                    inside = iy & ix
                    got = np.where(inside if labels.ndim == 3 else inside[..., None], got, fill_row)
                lab_out[i] = got
    return out, lab_out, dense
