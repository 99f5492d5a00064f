"""NumPy restatement of depgan_data_augment (include/depgan.h), operation for operation.

augment_ref(..., dtype=np.float32) casts every operand to float32, so each NumPy operation is the one correctly rounded
float32 operation the kernel performs and the result is expected bit for bit.  dtype=np.float64 is the identical
statement sequence in float64 on the same (float32) parameters: the yardstick for the float32 rounding error.
"""
import numpy as np


def _tap(fl, n):
    """integral-valued float coordinates -> (index clamped into [0, n), inside mask); compared before the cast"""
    inside = (fl >= 0) & (fl <= n - 1)
    return np.clip(fl, 0, n - 1).astype(np.int64), inside


def augment_ref(x, labels, params, index=None, border="edge", x_fill=0.0, label_fill=0, dtype=np.float32):
    """x (n_src, H, W, nicg); labels None, codes (n_src, H, W) uint8 or one-hot (n_src, H, W, C) float32;
    params (n, 8) float32.  Returns (x_out (n, H, W, nicg) of `dtype`, labels_out or None)."""
    f = dtype
    x = np.asarray(x)
    n_src, H, W, nicg = x.shape
    params = np.asarray(params, np.float32)
    n = len(params)
    index = np.arange(n) if index is None else np.asarray(index)
    constant = {"edge": False, "constant": True}[border]
    oy, ox = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    oy, ox = oy.astype(f), ox.astype(f)
    one, half, fill = f(1), f(0.5), f(x_fill)
    out = np.empty((n, H, W, nicg), f)
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
        a00, a01, a02, a10, a11, a12, gain, offset = (f(v) for v in params[i])
        sy = (a00 * oy + a01 * ox) + a02
        sx = (a10 * oy + a11 * ox) + a12
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
        res = gain * (top * gyc + bot * fyc) + offset
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
    return out, lab_out
