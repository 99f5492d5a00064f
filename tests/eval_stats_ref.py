"""NumPy restatement of depgan_eval_accumulate_stats and depgan_eval_finish_stats (include/depgan.h), statement by
statement.  Float32 operands stay float32 and float64 operands float64, so each NumPy operation is the one correctly
rounded operation the kernel performs: everything is expected bit for bit except what passes through a log (the device's
double log and NumPy's differ by an ulp or two)."""
import numpy as np

from augment_ref import _tap

BORDERS = {"edge": False, "valid": True}


def new_state(n, H, W, C):
    """the zeroed state of one run: sum, sumsq (n, H, W, C) float64; ent_sum (n, H, W) float64; votes (n, H, W, C) and
    count (n, H, W) uint8"""
    return {"sum": np.zeros((n, H, W, C)), "sumsq": np.zeros((n, H, W, C)), "ent_sum": np.zeros((n, H, W)),
            "votes": np.zeros((n, H, W, C), np.uint8), "count": np.zeros((n, H, W), np.uint8)}


def _plogp(v):
    """t = v > 0 ? v * log(v) : 0 in float64 (0 for a zero, a negative value and a NaN)"""
    v = np.asarray(v, np.float64)
    pos = v > 0
    return np.where(pos, v * np.log(np.where(pos, v, 1.0)), 0.0)


def entropy_rows(v):
    """h = ((0 - t_0) - t_1) - ... over the last axis, in channel order"""
    t = _plogp(v)
    h = np.zeros(t.shape[:-1])
    for c in range(t.shape[-1]):
        h = h - t[..., c]
    return h


def argmax_first(v):
    """np.argmax: the first maximum; a NaN counts as the maximum (its first occurrence wins)"""
    return np.argmax(v, axis=-1)


def sample(pred, params, border):
    """(u (n, H, W, C) float32, takes_part (n, H, W) bool): the draw's prediction resampled into the original frame by
    the output-to-source rows `params` (n, 8): augment_ref's float32 statements without the gain / offset statement."""
    f = np.float32
    pred = np.asarray(pred, f)
    n, H, W, C = pred.shape
    params = np.asarray(params, f)
    oy, ox = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    oy, ox = oy.astype(f), ox.astype(f)
    one = f(1)
    u = np.empty((n, H, W, C), f)
    part = np.ones((n, H, W), bool)
    for i in range(n):
        a00, a01, a02, a10, a11, a12 = (f(v) for v in params[i, :6])
        with np.errstate(invalid="ignore", over="ignore"):
            sy = (a00 * oy + a01 * ox) + a02
            sx = (a10 * oy + a11 * ox) + a12
            y0, x0 = np.floor(sy), np.floor(sx)
            fy, fx = sy - y0, sx - x0
            gy, gx = one - fy, one - fx
            ty0, iy0 = _tap(y0, H)
            ty1, iy1 = _tap(y0 + one, H)
            tx0, ix0 = _tap(x0, W)
            tx1, ix1 = _tap(x0 + one, W)
            img = pred[i]
            fxc, gxc, fyc, gyc = fx[..., None], gx[..., None], fy[..., None], gy[..., None]
            top = img[ty0, tx0] * gxc + img[ty0, tx1] * fxc
            bot = img[ty1, tx0] * gxc + img[ty1, tx1] * fxc
            res = top * gyc + bot * fyc
        assert res.dtype == f
        u[i] = res
        if BORDERS[border]:
            part[i] = iy0 & ix0 & ((fy == 0) | iy1) & ((fx == 0) | ix1)
    return u, part


def accumulate(state, pred, mask=None, params=None, border="edge"):
    """one draw: updates `state` (any key may be absent or None except 'sum') in place and returns it"""
    pred = np.asarray(pred, np.float32)
    n, H, W, C = pred.shape
    if params is None:
        u, part = pred, np.ones((n, H, W), bool)
    else:
        u, part = sample(pred, params, border)
    with np.errstate(invalid="ignore"):
        v = u if mask is None else u * np.asarray(mask, np.float32).reshape(n, H, W, 1)
    assert v.dtype == np.float32
    v64 = v.astype(np.float64)
    p4 = part[..., None]
    state["sum"][...] = np.where(p4, state["sum"] + v64, state["sum"])
    if state.get("sumsq") is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            state["sumsq"][...] = np.where(p4, state["sumsq"] + v64 * v64, state["sumsq"])
    if state.get("ent_sum") is not None:
        state["ent_sum"][...] = np.where(part, state["ent_sum"] + entropy_rows(v64), state["ent_sum"])
    if state.get("votes") is not None:
        hot = np.arange(C) == argmax_first(v)[..., None]
        state["votes"] += (hot & p4).astype(np.uint8)
    if state.get("count") is not None:
        state["count"] += part.astype(np.uint8)
    return state


def finish(state, n_draws, ddof=0, use_count=False):
    """the finishing pass on a copy of `state`: a dict with mean, var, expected_entropy, entropy, mutual_info (those the
    state has the sums for).  R is n_draws, or count per pixel with use_count."""
    s = np.array(state["sum"], np.float64)
    R = (state["count"].astype(np.float64) if use_count else np.full(s.shape[:-1], float(n_draws)))
    live = R > 0
    Rs = np.where(live, R, 1.0)
    R4, live4 = Rs[..., None], live[..., None]
    out = {}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = s / R4
        out["mean"] = np.where(live4, mean, 0.0)
        if state.get("sumsq") is not None:
            dof = R4 - float(ddof)
            d = state["sumsq"] / R4 - mean * mean
            d = np.where(d < 0, 0.0, d)
            var = d * (R4 / np.where(dof == 0, 1.0, dof))
            out["var"] = np.where(live4 & (dof != 0), var, 0.0)
        h = entropy_rows(mean)
        if s.shape[-1] >= 2:
            out["entropy"] = np.where(live, h, 0.0)
            if state.get("ent_sum") is not None:
                e = state["ent_sum"] / Rs
                out["expected_entropy"] = np.where(live, e, 0.0)
                d = h - e
                out["mutual_info"] = np.where(live, np.where(d < 0, 0.0, d), 0.0)
    return out
