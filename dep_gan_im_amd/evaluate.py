"""Evaluation step after the hot path (DEP-GAN_testing_4fold.py "GE":616-807).

    pred = predict_mean(netG, brain_prob__1tp, n_repeat=10, mask=icv_and_sl_mask_2tp)        # GE:616-628
    m = dem_metrics(brain_prob__1tp, pred, brain_code_2tp, icv_and_sl_mask_1tp, brain_wmh_1tp,
                    icv_and_sl_mask_2tp, brain_wmh_2tp, brain_prob__2tp, voxel_volume, TRSH_VAL) # GE:637-790
    m["vol_dsc"]   # the 18-entry row the script appends per subject (GE:806-808)

The mean over the n_repeat noise draws is accumulated on the device in float64 like the reference's np.zeros
accumulator (GE:617), and the volumes / Dice figures come from one integer census kernel (exact counts) that thresholds
that float64 mean in float64; only the two dozen integers travel to the host, where the reference's own scalar
algebra is applied.

The DEP-UResNet evaluation (DEP-UResNet_testing_4fold.py "UE":553-717) works on the C = 4 class probabilities instead:

    prob = predict_mean(my_network, brain_flair_1tp, n_repeat=10, mask=icv_and_sl_mask_2tp)  # UE:553-564, (n,H,W,4)
    m = uresnet_metrics(prob, brain_cod_2tp, icv_and_sl_mask_1tp, brain_wmh_1tp, icv_and_sl_mask_2tp, brain_wmh_2tp,
                        voxel_volume)                                                           # UE:566-700
    save_uresnet_maps(dirOutData, name, m["labels"], prob, affine)                              # UE:705-717

The label map is np.argmax over the float64 channel means (first index on a tie), and the volumes and Dice figures
come from an 18-count integer census of it (`depgan_eval_label_counts`).

What the noise draws say beyond their mean -- per-pixel variance, entropy, mutual information, votes -- and test-time
augmentation, for both models (csrc/eval_stats.hip):

    stats = predict_stats(my_network, brain_flair_1tp, n_repeat=10, mask=icv_and_sl_mask_2tp, tta=None)
    save_uncertainty_maps(dirOutData, name, stats, affine)

How far the predicted boundaries lie from the true ones -- Hausdorff distance, its 95th percentile, average symmetric
surface distance -- per class, from an exact distance map formed on the device (csrc/surface_dist.hip):

    surf = label_surface_metrics(m["labels"], brain_cod_2tp, classes=(1, 2, 3), spacing=data.prepared_spacing(pixdim))

Which lesions were found at all -- lesion-wise recall, precision, F1 and the absolute volume difference -- per class, from
connected components labelled on the device (csrc/components.hip):

    les = label_lesion_metrics(m["labels"], brain_cod_2tp, classes=(1, 2, 3), voxel_volume=voxel_volume)

Whether the probabilities can be believed -- ECE, MCE, Brier score, NLL, the reliability diagram -- and the temperature
that calibrates them, from an integer census and three double sums formed on the device (csrc/calibration.hip):

    cal = calibration_metrics(calibration_census(stats["mean"], data.to_codes(brain_cod_2tp), bins=15))
    fit = fit_temperature(stats["mean"], codes);  prob_T = apply_temperature(stats["mean"], fit["T"])
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

NCOUNT, NCOUNT_LABEL = _lib.EVAL_NCOUNT, _lib.EVAL_LABEL_NCOUNT      # DEPGAN_EVAL_*NCOUNT of include/depgan.h


def _torch():
    import torch
    return torch


def _dev(a, device, dtype=None):
    torch = _torch()
    if a is None:
        return None
    dtype = dtype or torch.float32
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype).contiguous()
    npdt = np.float64 if dtype == torch.float64 else np.float32
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=npdt)).to(device)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def predict_mean(netG, x, n_repeat=10, mask=None, noise_size=32, rng=None, batch_size=32):
    """Mean of n_repeat generator predictions with fresh N(0,1) noise, each multiplied by `mask` (GE:616-628).
    x: (n, H, W, nicg); mask: (n, H, W) or None.  Returns a float64 CUDA tensor (n, H, W): the reference's running
    sum is float64 and so is the mean it thresholds (GE:617, 628).
    A model with nc_out > 1 (DEP-UResNet, UE:553-564) gets the mask broadcast over its channels and a float64 CUDA
    tensor (n, H, W, nc_out) back."""
    if getattr(netG, "nc_out", 1) != 1:
        return _predict_mean_channels(netG, x, n_repeat, mask, noise_size, rng, batch_size)
    torch = _torch()
    lib = _lib.load()
    rng = rng if rng is not None else np.random
    n = len(x)
    eng = netG._ensure_engine(min(batch_size, n))
    dev = eng.device
    xd = _dev(x, dev)
    md = _dev(mask, dev)
    if md is not None and md.numel() != n * eng.height * eng.width:
        raise ValueError("mask must have one value per output pixel")
    acc = torch.zeros((n, eng.height, eng.width), dtype=torch.float64, device=dev)                  # GE:617
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for _ in range(n_repeat):
        noise = rng.normal(size=(n, noise_size, 1)).astype("float32")               # GE:620
        pred = eng.g_forward(xd, noise)                                               # GE:621
        _lib.check(lib.depgan_eval_accumulate(_p(pred), _p(md), _p(acc), acc.numel(), stream),
                   "depgan_eval_accumulate")                                          # GE:623-624
    _lib.check(lib.depgan_eval_divide(_p(acc), acc.numel(), float(n_repeat), stream), "depgan_eval_divide")  # GE:628
    return acc


def _predict_mean_channels(netG, x, n_repeat, mask, noise_size, rng, batch_size):
    """UE:553-564: output_img_pred_mean (np.zeros, float64) += predict([x, noise]) * icv_and_sl_mask_2tp, the mask
    (n, H, W[, 1]) broadcast over the C channels; then / float(n_repeat)."""
    torch = _torch()
    lib = _lib.load()
    rng = rng if rng is not None else np.random
    n = len(x)
    eng = netG._ensure_engine(min(batch_size, n))
    dev = eng.device
    C_out = int(eng.nc_out)
    xd = _dev(x, dev)
    md = _dev(mask, dev)
    npix = n * eng.height * eng.width
    if md is not None and md.numel() != npix:
        raise ValueError("mask must have one value per output pixel")
    acc = torch.zeros((n, eng.height, eng.width, C_out), dtype=torch.float64, device=dev)        # UE:554
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for _ in range(n_repeat):
        noise = rng.normal(size=(n, noise_size, 1)).astype("float32")               # UE:557
        pred = eng.g_forward(xd, noise)                                               # UE:558
        _lib.check(lib.depgan_eval_accumulate_channels(_p(pred), _p(md), _p(acc), npix, C_out, stream),
                   "depgan_eval_accumulate_channels")                                 # UE:559-560
    _lib.check(lib.depgan_eval_divide(_p(acc), acc.numel(), float(n_repeat), stream), "depgan_eval_divide")  # UE:564
    return acc


_STAT_BORDERS = {"edge": 0, "valid": 1}      # border of depgan_eval_accumulate_stats
MAX_DRAWS = 255                              # votes and count are uint8


def _stats_arguments(x, n_repeat, mask, tta, border, ddof):
    """The host-side checks of predict_stats, before anything touches the device.
    Returns (n, H, W, rows): rows is None, the Augmenter, or the (n_repeat, n, 8) float32 array of parameter rows."""
    from .data import AUG_NPARAM, Augmenter
    if isinstance(n_repeat, bool) or not isinstance(n_repeat, (int, np.integer)) or not 1 <= n_repeat <= MAX_DRAWS:
        raise ValueError("predict_stats: n_repeat must be an integer in 1..%d, got %r" % (MAX_DRAWS, n_repeat))
    if border not in _STAT_BORDERS:
        raise ValueError("predict_stats: border must be 'edge' or 'valid', got %r" % (border,))
    if isinstance(ddof, bool) or ddof not in (0, 1):
        raise ValueError("predict_stats: ddof must be 0 or 1, got %r" % (ddof,))
    shape = tuple(int(d) for d in (x.shape if hasattr(x, "shape") else np.shape(x)))
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError("predict_stats: x must be (n, H, W, nicg), got shape %s" % (shape,))
    n, H, W = shape[:3]
    if mask is not None:
        mshape = tuple(int(d) for d in (mask.shape if hasattr(mask, "shape") else np.shape(mask)))
        if int(np.prod(mshape)) != n * H * W:
            raise ValueError("predict_stats: mask must have one value per output pixel")
    rows = None
    if isinstance(tta, Augmenter):
        if tta.gain != (1.0, 1.0) or tta.offset != (0.0, 0.0):
            raise ValueError("predict_stats: a test-time Augmenter must have gain == (1, 1) and offset == (0, 0): an "
                             "intensity change has no inverse on a probability")
        if tta.fields_open:
            raise ValueError("predict_stats: a test-time Augmenter must have elastic == 0 and bias == 0: an elastic "
                             "map has no inverse row to resample the prediction through")
        rows = tta
    elif tta is not None:
        rows = np.asarray(tta.detach().cpu().numpy() if hasattr(tta, "detach") else tta, np.float32)
        if rows.shape != (n_repeat, n, AUG_NPARAM):
            raise ValueError("predict_stats: tta must be a data.Augmenter or parameter rows (%d, %d, %d), got shape %s"
                             % (n_repeat, n, AUG_NPARAM, rows.shape))
    return n, H, W, rows


def predict_stats(netG, x, n_repeat=10, mask=None, noise_size=32, rng=None, batch_size=32, tta=None, border="valid",
                  ddof=0):
    """What the n_repeat noise draws of predict_mean say beyond their mean, and test-time augmentation.
    x: (n, H, W, nicg); mask: (n, H, W) or None.  Returns a dict of device tensors:
      'mean', 'var'                                 float64 (n, H, W, C), or (n, H, W) for a one-channel model: the mean
                                                    and the variance (ddof 0 or 1) of the masked predictions
      'entropy', 'expected_entropy', 'mutual_info'  float64 (n, H, W), C >= 2: the entropy of the mean row, the mean of
                                                    the draws' entropies, and their difference, the BALD term (nats)
      'votes'                                       uint8 (n, H, W, C), C >= 2: how many draws had their maximum there
      'count'                                       uint8 (n, H, W): how many draws took part at the pixel
    The noise is drawn from `rng` exactly as predict_mean draws it, so with tta=None and the same rng state 'mean' is
    predict_mean's result bit for bit; the forward is eng.g_forward, so an inference_copy("bfloat16") works unchanged.
    tta: a data.Augmenter (gain, offset, elastic and bias closed, else ValueError; it draws n rows per repeat from its
    own generator) or an array (n_repeat, n, 8) of parameter rows.  Repeat r predicts on data.augment(x, params=rows[r])
    and is accumulated in the original frame through data.affine_inverse(rows[r]); the mask applies in the original frame.
    border 'edge' clamps the taps of that resampling, and every draw counts everywhere; 'valid' lets a draw take part
    only where every tap that carries weight lies inside its prediction, so 'count' can fall below n_repeat near the
    corners (a pixel no draw reached holds 0.0 everywhere).  At most 255 draws."""
    n, H, W, rows = _stats_arguments(x, n_repeat, mask, tta, border, ddof)
    from . import data as D
    torch = _torch()
    lib = _lib.load()
    rng = rng if rng is not None else np.random
    eng = netG._ensure_engine(min(batch_size, n))
    dev = eng.device
    if (H, W) != (eng.height, eng.width):
        raise ValueError("predict_stats: x is %d x %d, the model works on %d x %d" % (H, W, eng.height, eng.width))
    C_out = int(getattr(eng, "nc_out", 1))
    xd = _dev(x, dev)
    md = _dev(mask, dev)
    npix = n * H * W
    f64 = dict(dtype=torch.float64, device=dev)
    shape = (n, H, W, C_out) if C_out > 1 else (n, H, W)
    acc, sq = torch.zeros(shape, **f64), torch.zeros(shape, **f64)
    count = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    ent = votes = entropy = mi = None
    if C_out > 1:
        ent, entropy, mi = torch.zeros((n, H, W), **f64), torch.empty((n, H, W), **f64), torch.empty((n, H, W), **f64)
        votes = torch.zeros((n, H, W, C_out), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for r in range(n_repeat):
        noise = rng.normal(size=(n, noise_size, 1)).astype("float32")               # as predict_mean
        xw, inv = xd, None
        if rows is not None:
            fwd = rows.draw(n, H, W) if isinstance(rows, D.Augmenter) else rows[r]
            inv = torch.from_numpy(D.affine_inverse(fwd)).to(dev)                     # ValueError before the forward
            xw, _ = D.augment(xd, params=fwd, border=getattr(tta, "border", "edge"), x_fill=getattr(tta, "x_fill", 0.0))
        pred = eng.g_forward(xw, noise)
        _lib.check(lib.depgan_eval_accumulate_stats(_p(pred), _p(md), _p(inv), _STAT_BORDERS[border], n, H, W, C_out,
                                                    _p(acc), _p(sq), _p(ent), _p(votes), _p(count), stream),
                   "depgan_eval_accumulate_stats")
    _lib.check(lib.depgan_eval_finish_stats(_p(acc), _p(sq), _p(ent), _p(count) if rows is not None else None,
                                            _p(entropy), _p(mi), npix, C_out, int(n_repeat), int(ddof), stream),
               "depgan_eval_finish_stats")
    out = {"mean": acc, "var": sq, "count": count}
    if C_out > 1:
        out.update({"entropy": entropy, "expected_entropy": ent, "mutual_info": mi, "votes": votes})
    return out


def census(x, pred, code_real=None, mask1=None, wmh1=None, mask2=None, wmh2=None, prob2=None, thr=0.5, device=None):
    """The 20 integer counts of depgan_eval_counts (include/depgan.h) as a Python list."""
    torch = _torch()
    lib = _lib.load()
    if device is None:
        device = pred.device if isinstance(pred, torch.Tensor) else torch.device("cuda:%d" % torch.cuda.current_device())
    xd = _dev(x, device)
    if xd.dim() < 2:
        raise ValueError("x must be (..., nicg)")
    nicg = int(xd.shape[-1])
    npix = xd.numel() // nicg
    arrs = [_dev(pred, device, torch.float64)] + [_dev(a, device) for a in (code_real, mask1, wmh1, mask2, wmh2, prob2)]
    for name, a in zip(("pred", "code_real", "mask1", "wmh1", "mask2", "wmh2", "prob2"), arrs):
        if a is not None and a.numel() != npix:
            raise ValueError("%s must have %d elements, got %d" % (name, npix, a.numel()))
    out = (C.c_longlong * NCOUNT)()
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    _lib.check(lib.depgan_eval_counts(_p(xd), nicg, *[_p(a) for a in arrs], npix, float(thr), out, stream),
               "depgan_eval_counts")
    return [int(v) for v in out]


def _dice(both, real, fake, smooth=1e-7):
    return (both * 2.0 + smooth) / (smooth + real + fake)                             # GE:746-748


def confusion_metrics(cm, smooth=1e-7):
    """Accuracy, Dice and IoU from a confusion matrix: cm (C, C) integers, cm[t, p] = pixels of true class t predicted as
    class p -- Engine.uresnet_census() of one call, or the sum of such tables over the batches of an epoch.  Pure NumPy.

    Per class k: both = cm[k, k], real = row sum k, fake = column sum k; dice[k] = _dice(both, real, fake), the
    reference's (2 both + smooth) / (smooth + real + fake), so a 4-class table gives UE:636-652 for codes 1 to 3;
    iou[k] = (both + smooth) / (real + fake - both + smooth); precision = both / fake and recall = both / real (NaN
    for a class never predicted / without support); support = real.  accuracy = trace / sum.  mean_dice and mean_iou
    run over the foreground classes 1..C-1 (four classes: the reference's avg_all_dice, UE:697).

    A table summed over batches gives Keras' sample-weighted accuracy exactly (every sample has H*W pixels) and the
    GLOBAL Dice of the pixels it covers, which is not the mean of the batches' Dice figures.  An empty table is a
    ValueError."""
    cm = np.asarray(cm)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1] or cm.shape[0] < 2 or cm.dtype.kind not in "iu":
        raise ValueError("confusion_metrics: cm must be a (C, C) integer table with C >= 2, got %s %s"
                         % (cm.dtype, cm.shape))
    cm = cm.astype(np.int64)
    total = int(cm.sum())
    if total <= 0 or int(cm.min()) < 0:
        raise ValueError("confusion_metrics: the table is empty (no pixel was counted) or holds a negative count")
    both, real, fake = np.diag(cm), cm.sum(axis=1), cm.sum(axis=0)
    dice = np.array([_dice(int(b), int(r), int(f), smooth) for b, r, f in zip(both, real, fake)], np.float64)
    iou = (both + smooth) / (real + fake - both + smooth)
    with np.errstate(divide="ignore", invalid="ignore"):
        precision, recall = both / fake.astype(np.float64), both / real.astype(np.float64)
    return {"accuracy": float(both.sum()) / total, "dice": dice, "iou": iou, "precision": precision, "recall": recall,
            "support": real, "mean_dice": sum(dice[1:].tolist()) / (len(dice) - 1.0),     # left to right, as UE:697
            "mean_iou": sum(iou[1:].tolist()) / (len(iou) - 1.0)}


def soft_dice(sums, smooth=1e-7):
    """Per-class soft Dice from the sums of a call made with the Dice loss on (Engine.uresnet_dice_sums(): a dict with
    'intersection' I_k = sum t_k p_k, 'pred' P_k = sum p_k and 'true' T_k = sum t_k over the pixels that took part).
    Returns {'dice': (2 I_k + smooth) / (T_k + P_k + smooth) per class (np.float64), 'flat': the reference's dice_coef
    over everything flattened (UT:110-117), 'mean_dice': the mean over the foreground classes 1..C-1}.  Pure NumPy."""
    I, P, T = (np.asarray(sums[k], np.float64).reshape(-1) for k in ("intersection", "pred", "true"))
    if not (I.size == P.size == T.size >= 2):
        raise ValueError("soft_dice: intersection, pred and true must hold one value per class (at least 2 classes)")
    if not smooth > 0:
        raise ValueError("soft_dice: smooth must be > 0, got %r" % (smooth,))
    dice = (2.0 * I + smooth) / (T + P + smooth)
    return {"dice": dice, "flat": float((2.0 * I.sum() + smooth) / (T.sum() + P.sum() + smooth)),
            "mean_dice": sum(dice[1:].tolist()) / (len(dice) - 1.0)}


def metrics_from_census(c, voxel_volume):
    """The reference's scalar algebra on the census (GE:640-808)."""
    vol_1tp__ml = c[0] * voxel_volume / 1000                                          # GE:640-641
    vol_2tp__ml = c[1] * voxel_volume / 1000                                          # GE:650-651
    vol_1tp__ml_iam = c[2] * voxel_volume / 1000                                      # GE:659-660
    vol_2tp__ml_iam = c[3] * voxel_volume / 1000                                      # GE:668-669
    vol_out__ml = c[4] * voxel_volume / 1000                                          # GE:683-684
    err_vol = vol_out__ml - vol_2tp__ml                                               # GE:688
    mse_vol = float(np.mean((vol_2tp__ml - vol_out__ml) ** 2))                        # GE:689
    true_pred = true_prog = true_regg = prog = regg = 0                               # GE:692-707
    if (vol_2tp__ml - vol_1tp__ml) >= 0:
        prog = 1
        if vol_out__ml - vol_1tp__ml >= 0:
            true_pred = true_prog = 1
    else:
        regg = 1
        if vol_out__ml - vol_1tp__ml < 0:
            true_pred = true_regg = 1
    dice_1, dice_2, dice_3 = (_dice(*c[5 + 3 * k:8 + 3 * k]) for k in range(3))       # GE:745-758
    dice_4 = _dice(*c[14:17])                                                         # GE:760-769
    dice_5 = _dice(*c[17:20])                                                         # GE:771-786
    dice_6 = _dice(*c[11:14])                                                         # GE:788-797 (== dice_3)
    avg_all_dice = (dice_1 + dice_2 + dice_3) / 3.0
    avg_dice__56 = (dice_5 + dice_6) / 2.0
    vol_dsc = [true_pred, prog, true_prog, regg, true_regg, vol_1tp__ml, vol_2tp__ml, vol_out__ml, mse_vol, err_vol,
               dice_5, dice_6, avg_dice__56, dice_1, dice_2, dice_3, dice_4, avg_all_dice]
    return {"vol_dsc": vol_dsc, "vol_1tp_ml": vol_1tp__ml, "vol_2tp_ml": vol_2tp__ml, "vol_out_ml": vol_out__ml,
            "vol_1tp_ml_im": vol_1tp__ml_iam, "vol_2tp_ml_im": vol_2tp__ml_iam, "err_vol": err_vol,
            "mse_vol": mse_vol, "true_pred": true_pred, "prog": prog, "true_prog": true_prog, "regg": regg,
            "true_regg": true_regg, "dice": [dice_1, dice_2, dice_3, dice_4, dice_5, dice_6],
            "avg_all_dice": avg_all_dice, "avg_dice_56": avg_dice__56, "census": list(c)}


def dem_metrics(x, pred, code_real, mask1, wmh1, mask2, wmh2, prob2, voxel_volume, thr):
    """All per-subject figures of GE:637-790 for one volume of slices."""
    return metrics_from_census(census(x, pred, code_real, mask1, wmh1, mask2, wmh2, prob2, thr), voxel_volume)


# ---- DEP-UResNet evaluation (UE:566-717) ----

def label_census(pred, code_real=None, mask1=None, wmh1=None, mask2=None, wmh2=None, device=None,
                 return_labels=False):
    """The 18 integer counts of depgan_eval_label_counts (include/depgan.h) as a Python list.
    pred: (..., C) float64 class probabilities (predict_mean of a C-channel model, any C; the counts themselves read the
    reference's 4 codes); the other arrays have one value
    per pixel and may be None.  With return_labels the argmax label map (pred.shape[:-1], int8 CUDA tensor) comes too."""
    torch = _torch()
    lib = _lib.load()
    if device is None:
        device = pred.device if isinstance(pred, torch.Tensor) else torch.device("cuda:%d" % torch.cuda.current_device())
    pd = _dev(pred, device, torch.float64)
    if pd.dim() < 2:
        raise ValueError("pred must be (..., C)")
    n_class = int(pd.shape[-1])
    npix = pd.numel() // n_class
    arrs = [_dev(a, device) for a in (code_real, mask1, wmh1, mask2, wmh2)]
    for name, a in zip(("code_real", "mask1", "wmh1", "mask2", "wmh2"), arrs):
        if a is not None and a.numel() != npix:
            raise ValueError("%s must have %d elements, got %d" % (name, npix, a.numel()))
    labels = torch.empty(tuple(pd.shape[:-1]), dtype=torch.int8, device=device) if return_labels else None
    out = (C.c_longlong * NCOUNT_LABEL)()
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    _lib.check(lib.depgan_eval_label_counts(_p(pd), n_class, *[_p(a) for a in arrs], npix, _p(labels), out, stream),
               "depgan_eval_label_counts")
    counts = [int(v) for v in out]
    return (counts, labels) if return_labels else counts


_FOUR_CODES = ("the DEP-UResNet metrics implement the reference's 4-code change map (UE:566-700); a prediction with %d "
               "classes has no such reading -- predict_mean and label_census(..., return_labels=True) serve any class "
               "count")


def label_metrics_from_census(c, voxel_volume, n_class=4):
    """UE's scalar algebra on the label census (UE:572-700); vol_dsc has GE's 18-entry row order.  The census must come
    from a 4-class prediction (n_class says what it came from): any other count is a ValueError."""
    if int(n_class) != 4:
        raise ValueError(_FOUR_CODES % int(n_class))
    vol_1tp__ml = c[0] * voxel_volume / 1000                                          # UE:575-581
    vol_2tp__ml = c[1] * voxel_volume / 1000                                          # UE:584-591
    vol_out__ml = c[2] * voxel_volume / 1000                                          # UE:594-602
    err_vol = vol_out__ml - vol_2tp__ml                                               # UE:606
    mse_vol = float(np.mean((vol_2tp__ml - vol_out__ml) ** 2))                        # UE:607
    true_pred = true_prog = true_regg = prog = regg = 0                               # UE:609-624
    if (vol_2tp__ml - vol_1tp__ml) >= 0:
        prog = 1
        if vol_out__ml - vol_1tp__ml >= 0:
            true_pred = true_prog = 1
    else:
        regg = 1
        if vol_out__ml - vol_1tp__ml < 0:
            true_pred = true_regg = 1
    dice_1, dice_2, dice_3 = (_dice(*c[3 + 3 * k:6 + 3 * k]) for k in range(3))       # UE:636-652
    dice_4 = _dice(*c[12:15])                                                         # UE:654-662
    dice_5 = _dice(*c[15:18])                                                         # UE:664-679
    dice_6 = _dice(*c[9:12])                                                          # UE:681-690 (== dice_3)
    avg_all_dice = (dice_1 + dice_2 + dice_3) / 3.0                                   # UE:697
    avg_dice__56 = (dice_5 + dice_6) / 2.0                                            # UE:698
    vol_dsc = [true_pred, prog, true_prog, regg, true_regg, vol_1tp__ml, vol_2tp__ml, vol_out__ml, mse_vol, err_vol,
               dice_5, dice_6, avg_dice__56, dice_1, dice_2, dice_3, dice_4, avg_all_dice]    # UE:699-700
    return {"vol_dsc": vol_dsc, "vol_1tp_ml": vol_1tp__ml, "vol_2tp_ml": vol_2tp__ml, "vol_out_ml": vol_out__ml,
            "err_vol": err_vol, "mse_vol": mse_vol, "true_pred": true_pred, "prog": prog, "true_prog": true_prog,
            "regg": regg, "true_regg": true_regg, "dice": [dice_1, dice_2, dice_3, dice_4, dice_5, dice_6],
            "avg_all_dice": avg_all_dice, "avg_dice_56": avg_dice__56, "census": list(c)}


def uresnet_metrics(pred, code_real, mask1, wmh1, mask2, wmh2, voxel_volume):
    """All per-subject figures of UE:566-700 for one volume of slices; "labels" holds the label map (int8 CUDA
    tensor, UE:570 convert_from_1hot) for save_uresnet_maps.  pred must have the reference's 4 channels: any other count is
    a ValueError."""
    n_class = int(pred.shape[-1]) if len(getattr(pred, "shape", ())) else 0
    if n_class != 4:
        raise ValueError(_FOUR_CODES % n_class)
    c, labels = label_census(pred, code_real, mask1, wmh1, mask2, wmh2, return_labels=True)
    m = label_metrics_from_census(c, voxel_volume)
    m["labels"] = labels
    return m


def save_uresnet_maps(directory, name, labels, prob_mean, affine):
    """UE:705-717: <name>_cls_map.nii.gz (the label map, int8) and <name>_prb_map_c<c>.nii.gz (channel c of the mean
    probabilities, float32), each through data_prep_save.  labels: (N, H, W); prob_mean: (N, H, W, C).
    Returns the paths written."""
    import os
    from . import nifti
    from .data import data_prep_save

    def host(a):
        return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)

    lab, prob = host(labels), host(prob_mean)
    paths = [os.path.join(directory, name + "_cls_map.nii.gz")]
    nifti.save(paths[0], data_prep_save(lab).astype("int8"), affine)                                   # UE:705-708
    N, H, W, n_class = prob.shape
    for c in range(n_class):
        pred_prob = prob[:, :, :, c].reshape((N, H, W, 1))                                               # UE:712-713
        paths.append(os.path.join(directory, name + "_prb_map_c" + str(c) + ".nii.gz"))
        nifti.save(paths[-1], data_prep_save(pred_prob).astype("float32"), affine)                      # UE:715-717
    return paths


def save_uncertainty_maps(directory, name, stats, affine):
    """The uncertainty maps of predict_stats as float32 NIfTI volumes, each through data_prep_save like the maps of
    save_uresnet_maps: <name>_unc_entropy.nii.gz and <name>_unc_mutual_info.nii.gz (a model with C >= 2 channels) and
    the variance, <name>_unc_var_c<c>.nii.gz per channel or <name>_unc_var.nii.gz for a one-channel model.
    stats: the dict predict_stats returned (device tensors or arrays).  Returns the paths written."""
    import os
    from . import nifti
    from .data import data_prep_save

    def host(a):
        return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)

    paths = []

    def save(suffix, a):
        paths.append(os.path.join(directory, name + "_unc_" + suffix + ".nii.gz"))
        nifti.save(paths[-1], data_prep_save(a[..., None]).astype("float32"), affine)

    for key in ("entropy", "mutual_info"):
        if stats.get(key) is not None:
            save(key, host(stats[key]))
    var = host(stats["var"])
    if var.ndim == 3:
        save("var", var)
    else:
        for c in range(var.shape[3]):
            save("var_c" + str(c), var[:, :, :, c])
    return paths


# ---- surface distances: HD, HD95, ASSD from an exact on-device distance map (csrc/surface_dist.hip) ----

SURFACE_KEYS = ("n_surface_a", "n_surface_b", "hd_ab", "hd_ba", "hd", "msd_ab", "msd_ba", "assd", "hd95_ab", "hd95_ba",
                "hd95", "hd95_pooled")


def _shape3(a, what):
    shape = tuple(int(d) for d in (a.shape if hasattr(a, "shape") else np.shape(a)))
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("%s must be a three-dimensional (n, H, W) array, got shape %s" % (what, shape))
    return shape


def _spacing_weights(spacing, who):
    """(wz, wy, wx), the squared spacings depgan_eval_edt_sq takes; ValueError unless three finite positive numbers."""
    try:
        s = [float(v) for v in spacing]
    except (TypeError, ValueError):
        s = []
    w = [v * v for v in s]
    if len(s) != 3 or not all(np.isfinite(v) and v > 0 for v in s + w):
        raise ValueError("%s: spacing must hold three finite positive numbers (sz, sy, sx), got %r" % (who, spacing))
    return tuple(w)


def _set_u8(a, device):
    """(n, H, W) uint8 device tensor, 1 where `a` is non-zero (any dtype, host or device)."""
    torch = _torch()
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a) != 0))
    return (t.to(device) != 0).to(torch.uint8).contiguous()


def _surface_device(*arrays):
    torch = _torch()
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    return torch.device("cuda:%d" % torch.cuda.current_device())


def _edt_sq(lib, set_u8, w, stream):
    """float64 device tensor: depgan_eval_edt_sq of a (n, H, W) uint8 device tensor"""
    torch = _torch()
    D, H, W = (int(d) for d in set_u8.shape)
    d2 = torch.empty((D, H, W), dtype=torch.float64, device=set_u8.device)
    scratch = torch.empty((max(1, int(lib.depgan_eval_edt_scratch_bytes(D, H, W)) // 8),), dtype=torch.float64,
                          device=set_u8.device)
    _lib.check(lib.depgan_eval_edt_sq(_p(set_u8), D, H, W, w[0], w[1], w[2], _p(d2), _p(scratch), stream),
               "depgan_eval_edt_sq")
    return d2


def distance_transform(mask, spacing=(1, 1, 1), squared=False):
    """The exact Euclidean distance from every voxel to the nearest non-zero voxel of `mask`, in units of `spacing` =
    (sz, sy, sx) (data.prepared_spacing): a float64 device tensor (n, H, W).  mask: (n, H, W), any dtype, host or
    device; non-zero means set.  squared: the squared distance, which is what the kernels form (include/depgan.h:
    every product and sum of dz^2 sz^2 + dy^2 sy^2 + dx^2 sx^2 rounded once); otherwise its square root.  A mask
    without a set voxel gives +inf everywhere.  Note the sense: scipy.ndimage.distance_transform_edt(~mask, spacing)."""
    _shape3(mask, "distance_transform: mask")
    w = _spacing_weights(spacing, "distance_transform")
    torch = _torch()
    lib = _lib.load()
    dev = _surface_device(mask)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    d2 = _edt_sq(lib, _set_u8(mask, dev), w, stream)
    return d2 if squared else torch.sqrt(d2)


def _percentile_index(n, q):
    """NumPy's linear-interpolation statement for np.percentile(a, q) of n sorted values: (lower index, upper index,
    weight of the upper one)."""
    virtual = (n - 1) * np.true_divide(q, 100.0)
    if virtual >= n - 1:                                 # at or above the last index: the maximum
        return n - 1, n - 1, 0.0
    lo = int(np.floor(virtual))
    return lo, lo + 1, float(virtual - np.floor(virtual))


def _lerp(a, b, t):
    """NumPy's _lerp: a + (b - a) t, taken from the other end for t >= 0.5"""
    d = b - a
    return a + d * t if t < 0.5 else b - d * (1.0 - t)


def surface_distances(a, b, spacing=(1, 1, 1), in_plane=False, percentile=95.0):
    """Distances between the surfaces of two binary volumes a and b, (n, H, W), any dtype, host or device, non-zero =
    set; `spacing` = (sz, sy, sx) of the slices (data.prepared_spacing).  A surface voxel is a set voxel with a face
    neighbour that is unset or outside the volume -- the 6 neighbours in the volume, or with in_plane the 4 in the
    slice (the WMH challenge's convention for thick slices).  With s_ab the distances from a's surface voxels to the
    nearest surface voxel of b and s_ba the reverse, returns a dict of Python numbers:
      n_surface_a, n_surface_b   the surface voxel counts
      hd_ab, hd_ba, hd           the directed maxima and their maximum, the Hausdorff distance
      msd_ab, msd_ba, assd       the directed means and (msd_ab + msd_ba) / 2, medpy's assd
      hd95_ab, hd95_ba, hd95     np.percentile(s, percentile) (linear interpolation) per direction and the maximum of
                                 the two, the WMH challenge's figure
      hd95_pooled                the percentile of the two sets concatenated, medpy's hd95
    If either surface is empty every distance figure is nan and the counts say why; nothing raises.
    The masks, the exact distance maps (depgan_eval_edt_sq), the sums and the sort stay on the device; a handful of
    scalars travel back."""
    shape = _shape3(a, "surface_distances: a")
    if _shape3(b, "surface_distances: b") != shape:
        raise ValueError("surface_distances: a and b must have the same shape, got %s and %s"
                         % (shape, _shape3(b, "surface_distances: b")))
    w = _spacing_weights(spacing, "surface_distances")
    try:
        q = float(percentile)
    except (TypeError, ValueError):
        q = float("nan")
    if not 0.0 <= q <= 100.0:
        raise ValueError("surface_distances: percentile must lie in [0, 100], got %r" % (percentile,))
    torch = _torch()
    lib = _lib.load()
    dev = _surface_device(a, b)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    D, H, W = shape
    n = D * H * W
    partial = torch.empty((max(1, int(lib.depgan_eval_surface_sums_scratch_bytes(n)) // 8),), dtype=torch.float64,
                          device=dev)
    surf, d2 = [], []
    for vol in (a, b):
        s = torch.empty(shape, dtype=torch.uint8, device=dev)
        _lib.check(lib.depgan_eval_surface_mask(_p(_set_u8(vol, dev)), D, H, W, 1 if in_plane else 0, _p(s), stream),
                   "depgan_eval_surface_mask")
        surf.append(s)
        d2.append(_edt_sq(lib, s, w, stream))             # the distance to THIS surface
    sums = []
    for own, other in ((0, 1), (1, 0)):                   # s_ab: a's surface voxels in b's map; then s_ba
        out = (C.c_double * 4)()
        _lib.check(lib.depgan_eval_surface_sums(_p(d2[other]), _p(surf[own]), n, _p(partial), out, stream),
                   "depgan_eval_surface_sums")
        sums.append([float(v) for v in out])
    na, nb = int(sums[0][0]), int(sums[1][0])
    res = {k: float("nan") for k in SURFACE_KEYS}
    res["n_surface_a"], res["n_surface_b"] = na, nb
    if na == 0 or nb == 0:
        return res
    res["hd_ab"], res["hd_ba"] = float(np.sqrt(sums[0][1])), float(np.sqrt(sums[1][1]))
    res["hd"] = max(res["hd_ab"], res["hd_ba"])
    res["msd_ab"], res["msd_ba"] = sums[0][2] / na, sums[1][2] / nb
    res["assd"] = (res["msd_ab"] + res["msd_ba"]) / 2
    # the percentile: the squared distances at the surface voxels, sorted on the device; the square root is monotone,
    # so the order statistics of the distances are the square roots of these
    s_ab = torch.masked_select(d2[1], surf[0] != 0)
    s_ba = torch.masked_select(d2[0], surf[1] != 0)
    picks, where = [], []
    for v in (s_ab, s_ba, torch.cat([s_ab, s_ba])):
        lo, hi, t = _percentile_index(int(v.numel()), q)
        picks.append(torch.sort(v).values[[lo, hi]])
        where.append(t)
    stats = np.sqrt(torch.cat(picks).cpu().numpy())
    for i, key in enumerate(("hd95_ab", "hd95_ba", "hd95_pooled")):
        res[key] = float(_lerp(stats[2 * i], stats[2 * i + 1], where[i]))
    res["hd95"] = max(res["hd95_ab"], res["hd95_ba"])
    return res


def label_surface_metrics(labels, code_real, classes=(1, 2, 3), spacing=(1, 1, 1), mask=None, in_plane=False):
    """surface_distances per class: {k: surface_distances(labels == k, code_real == k, spacing, in_plane)} for k in
    `classes` (any class count).  labels: the int8 label map of uresnet_metrics(...)["labels"]; code_real: the float32
    code volume; both (n, H, W) (a trailing axis of length 1 is dropped), host or device.  mask (same shape, optional):
    both maps are zeroed where it is zero first."""
    classes = [int(k) for k in classes]
    if not classes:
        raise ValueError("label_surface_metrics: classes is empty")
    torch = _torch()

    def vol(v, what):
        shape = tuple(int(d) for d in (v.shape if hasattr(v, "shape") else np.shape(v)))
        if len(shape) == 4 and shape[3] == 1:
            v = v.reshape(shape[:3])
        _shape3(v, "label_surface_metrics: " + what)
        return v

    labels, code_real = vol(labels, "labels"), vol(code_real, "code_real")
    if tuple(labels.shape) != tuple(code_real.shape):
        raise ValueError("label_surface_metrics: labels and code_real must have the same shape, got %s and %s"
                         % (tuple(labels.shape), tuple(code_real.shape)))
    if mask is not None:
        mask = vol(mask, "mask")
        if tuple(mask.shape) != tuple(labels.shape):
            raise ValueError("label_surface_metrics: mask must have the shape of labels")
    _spacing_weights(spacing, "label_surface_metrics")
    dev = _surface_device(labels, code_real, mask)

    def up(v):
        return v.to(dev) if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)).to(dev)

    lab, real = up(labels), up(code_real)
    if mask is not None:
        keep = up(mask) != 0
        lab, real = lab * keep.to(lab.dtype), real * keep.to(real.dtype)
    return {k: surface_distances(lab == k, real == k, spacing, in_plane) for k in classes}


# ---- lesion-wise detection: connected components labelled on the device (csrc/components.hip) ----

LESION_KEYS = ("n_truth", "n_pred", "n_truth_detected", "n_pred_true", "recall", "precision", "f1", "voxels_truth",
               "voxels_pred", "avd_percent")


def _cc_args(who, connectivity=1, in_plane=False, min_voxels=1, voxel_volume=None):
    """(connectivity, in_plane as 0 / 1, min_voxels, voxel_volume or None); ValueError for anything else."""
    if isinstance(connectivity, bool) or connectivity not in (1, 2, 3):
        raise ValueError("%s: connectivity must be 1, 2 or 3 (scipy's generate_binary_structure rank), got %r"
                         % (who, connectivity))
    if isinstance(in_plane, (bool, np.bool_)):
        in_plane = int(in_plane)
    if isinstance(in_plane, (float, str)) or in_plane not in (0, 1):
        raise ValueError("%s: in_plane must be False or True, got %r" % (who, in_plane))
    try:
        mv = int(min_voxels)
        whole = not isinstance(min_voxels, (bool, str)) and mv == min_voxels
    except (TypeError, ValueError, OverflowError):
        mv, whole = 0, False
    if not whole:
        raise ValueError("%s: min_voxels must be an integer, got %r" % (who, min_voxels))
    if voxel_volume is not None:
        try:
            voxel_volume = float(voxel_volume)
        except (TypeError, ValueError):
            voxel_volume = float("nan")
        if not (np.isfinite(voxel_volume) and voxel_volume > 0):
            raise ValueError("%s: voxel_volume must be a finite positive number, got %r" % (who, voxel_volume))
    return int(connectivity), int(in_plane), mv, voxel_volume


def _cc_label(lib, set_u8, connectivity, in_plane, stream):
    """(int32 device tensor, N): depgan_eval_cc_label of a (n, H, W) uint8 device tensor"""
    torch = _torch()
    D, H, W = (int(d) for d in set_u8.shape)
    labels = torch.empty((D, H, W), dtype=torch.int32, device=set_u8.device)
    scratch = torch.empty((max(1, int(lib.depgan_eval_cc_scratch_bytes(D, H, W)) // 8),), dtype=torch.int64,
                          device=set_u8.device)
    n_out = (C.c_longlong * 1)()
    _lib.check(lib.depgan_eval_cc_label(_p(set_u8), D, H, W, connectivity, in_plane, _p(labels), _p(scratch), n_out,
                                        stream), "depgan_eval_cc_label")
    return labels, int(n_out[0])


def _cc_tables(lib, labels, n, other_u8, stream):
    """(size, hits): depgan_eval_cc_overlap of an int32 device tensor with components 1..n"""
    torch = _torch()
    size = torch.empty((n,), dtype=torch.int32, device=labels.device)
    hits = torch.empty((n,), dtype=torch.int32, device=labels.device)
    _lib.check(lib.depgan_eval_cc_overlap(_p(labels), _p(other_u8), int(labels.numel()), n, _p(size) if n else None,
                                          _p(hits) if n else None, stream), "depgan_eval_cc_overlap")
    return size, hits


def _cc_stream(dev):
    return C.c_void_p(_torch().cuda.current_stream(dev).cuda_stream)


def connected_components(mask, connectivity=1, in_plane=False):
    """The connected components of the non-zero voxels of `mask`, (n, H, W), any dtype, host or device: (labels, N) with
    labels an int32 device tensor (n, H, W), 0 where mask is zero and 1..N elsewhere, and N a Python int.  Components
    are numbered in the order of their first voxel in index order, which is scipy.ndimage.label's numbering.
    connectivity is scipy's rank, generate_binary_structure(3, connectivity): 1 (scipy's default) joins the 6 face
    neighbours, 2 the 18 that share a face or an edge, 3 all 26.  With in_plane the neighbours lie in the slice only:
    4 at rank 1, 8 at ranks 2 and 3 (slices several times thicker than pixels, as in surface_distances)."""
    _shape3(mask, "connected_components: mask")
    connectivity, in_plane, _, _ = _cc_args("connected_components", connectivity, in_plane)
    lib = _lib.load()
    dev = _surface_device(mask)
    return _cc_label(lib, _set_u8(mask, dev), connectivity, in_plane, _cc_stream(dev))


def component_sizes(labels, n, other=None):
    """(size, hits), int32 device tensors of length n, for a label volume of connected_components: size[k - 1] is the
    voxel count of component k and hits[k - 1] the number of its voxels where `other` (same shape, any dtype, host or
    device) is non-zero; all zero when other is None.  A label outside 1..n is not counted."""
    shape = _shape3(labels, "component_sizes: labels")
    try:
        whole = not isinstance(n, bool) and int(n) == n
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or not 0 <= int(n) <= shape[0] * shape[1] * shape[2]:
        raise ValueError("component_sizes: n must be an integer from 0 to the number of voxels, got %r" % (n,))
    if other is not None and _shape3(other, "component_sizes: other") != shape:
        raise ValueError("component_sizes: other must have the shape of labels, got %s and %s"
                         % (_shape3(other, "component_sizes: other"), shape))
    torch = _torch()
    lib = _lib.load()
    dev = _surface_device(labels, other)
    lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels))
    lab = lab.to(device=dev, dtype=torch.int32).contiguous()
    return _cc_tables(lib, lab, int(n), None if other is None else _set_u8(other, dev), _cc_stream(dev))


def _keep_large(labels, size, min_voxels):
    """(uint8 mask of the voxels whose component has at least min_voxels voxels, bool table of those components)"""
    torch = _torch()
    keep = size >= min_voxels
    table = torch.cat([keep.new_zeros((1,)), keep])                  # label 0, the background, is never kept
    return table[labels.long()].to(torch.uint8), keep


def remove_small_components(mask, min_voxels, connectivity=1, in_plane=False):
    """`mask` (n, H, W), any dtype, host or device, as a uint8 device tensor of 0 / 1 with every connected component of
    fewer than min_voxels voxels cleared; min_voxels <= 1 returns the binarised mask.  connectivity and in_plane as in
    connected_components."""
    _shape3(mask, "remove_small_components: mask")
    connectivity, in_plane, min_voxels, _ = _cc_args("remove_small_components", connectivity, in_plane, min_voxels)
    dev = _surface_device(mask)
    set_u8 = _set_u8(mask, dev)
    if min_voxels <= 1:
        return set_u8
    lib = _lib.load()
    stream = _cc_stream(dev)
    labels, n = _cc_label(lib, set_u8, connectivity, in_plane, stream)
    size, _ = _cc_tables(lib, labels, n, None, stream)
    return _keep_large(labels, size, min_voxels)[0]


def _ratio(a, b):
    return a / b if b else float("nan")


def lesion_detection(pred, truth, connectivity=3, in_plane=False, min_voxels=1, voxel_volume=None):
    """Lesion-wise detection figures of two binary volumes, (n, H, W), any dtype, host or device, non-zero = set.  A
    lesion is a connected component; connectivity and in_plane as in connected_components.  The default, rank 3, is the
    WMH challenge's fully connected filter; rank 1 is scipy.ndimage.label's default.  Returns a dict of Python numbers
      n_truth, n_pred                the lesion counts
      n_truth_detected               truth lesions with at least one voxel set in pred
      n_pred_true                    predicted lesions with at least one voxel set in truth
      recall, precision, f1          n_truth_detected / n_truth, n_pred_true / n_pred and 2 P R / (P + R)
      voxels_truth, voxels_pred      the set voxels
      avd_percent                    100 |voxels_pred - voxels_truth| / voxels_truth, the absolute volume difference
    followed by sizes_truth and sizes_pred, the lesion sizes as device tensors in label order: int32 voxel counts, or
    with voxel_volume float64 in its unit.  min_voxels > 1 first clears every component of fewer voxels from each
    volume; the lesion lists and the masks the overlaps are taken against are the cleaned ones.  A ratio whose
    denominator is 0 is nan and the counts say why; f1 is nan if either ratio is, and 0.0 if both are 0.  Nothing
    raises.  The labels and tables stay on the device; eight integers travel back."""
    shape = _shape3(pred, "lesion_detection: pred")
    if _shape3(truth, "lesion_detection: truth") != shape:
        raise ValueError("lesion_detection: pred and truth must have the same shape, got %s and %s"
                         % (shape, _shape3(truth, "lesion_detection: truth")))
    connectivity, in_plane, min_voxels, voxel_volume = _cc_args("lesion_detection", connectivity, in_plane, min_voxels,
                                                                voxel_volume)
    torch = _torch()
    lib = _lib.load()
    dev = _surface_device(pred, truth)
    stream = _cc_stream(dev)
    masks = [_set_u8(truth, dev), _set_u8(pred, dev)]
    labelled = [_cc_label(lib, m, connectivity, in_plane, stream) for m in masks]
    keep = [None, None]
    if min_voxels > 1:
        for i, (lab, n) in enumerate(labelled):
            masks[i], keep[i] = _keep_large(lab, _cc_tables(lib, lab, n, None, stream)[0], min_voxels)
    sizes, counts = [], []
    for i, (lab, n) in enumerate(labelled):
        size, hits = _cc_tables(lib, lab, n, masks[1 - i], stream)
        if keep[i] is not None:
            size, hits = size[keep[i]], hits[keep[i]]
        sizes.append(size)
        counts += [torch.tensor(size.numel(), device=dev), (hits > 0).sum(), size.sum()]
    nt, ntd, vt, npd, npt, vp = (int(v) for v in torch.stack([c.to(torch.int64) for c in counts]).cpu())
    recall, precision = _ratio(ntd, nt), _ratio(npt, npd)
    if np.isnan(recall) or np.isnan(precision):
        f1 = float("nan")
    else:
        f1 = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
    res = {"n_truth": nt, "n_pred": npd, "n_truth_detected": ntd, "n_pred_true": npt, "recall": recall,
           "precision": precision, "f1": f1, "voxels_truth": vt, "voxels_pred": vp,
           "avd_percent": _ratio(100.0 * abs(vp - vt), vt)}
    if voxel_volume is not None:
        sizes = [s.to(torch.float64) * voxel_volume for s in sizes]
    res["sizes_truth"], res["sizes_pred"] = sizes
    return res


def label_lesion_metrics(labels, code_real, classes=(1, 2, 3), mask=None, **kw):
    """lesion_detection per class: {k: lesion_detection(labels == k, code_real == k, **kw)} for k in `classes` (any
    class count), kw = connectivity, in_plane, min_voxels, voxel_volume.  labels: the int8 label map of
    uresnet_metrics(...)["labels"], the prediction; code_real: the float32 code volume, the truth; both (n, H, W) (a
    trailing axis of length 1 is dropped), host or device.  mask (same shape, optional): both maps are zeroed where it
    is zero first."""
    classes = [int(k) for k in classes]
    if not classes:
        raise ValueError("label_lesion_metrics: classes is empty")
    torch = _torch()

    def vol(v, what):
        shape = tuple(int(d) for d in (v.shape if hasattr(v, "shape") else np.shape(v)))
        if len(shape) == 4 and shape[3] == 1:
            v = v.reshape(shape[:3])
        _shape3(v, "label_lesion_metrics: " + what)
        return v

    labels, code_real = vol(labels, "labels"), vol(code_real, "code_real")
    if tuple(labels.shape) != tuple(code_real.shape):
        raise ValueError("label_lesion_metrics: labels and code_real must have the same shape, got %s and %s"
                         % (tuple(labels.shape), tuple(code_real.shape)))
    if mask is not None:
        mask = vol(mask, "mask")
        if tuple(mask.shape) != tuple(labels.shape):
            raise ValueError("label_lesion_metrics: mask must have the shape of labels")
    if set(kw) - {"connectivity", "in_plane", "min_voxels", "voxel_volume"}:
        raise ValueError("label_lesion_metrics: unknown argument %s" % sorted(kw))
    _cc_args("label_lesion_metrics", kw.get("connectivity", 3), kw.get("in_plane", False), kw.get("min_voxels", 1),
             kw.get("voxel_volume"))
    dev = _surface_device(labels, code_real, mask)

    def up(v):
        return v.to(dev) if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)).to(dev)

    lab, real = up(labels), up(code_real)
    if mask is not None:
        keep = up(mask) != 0
        lab, real = lab * keep.to(lab.dtype), real * keep.to(real.dtype)
    return {k: lesion_detection(lab == k, real == k, **kw) for k in classes}


# ---- calibration: can the probabilities be believed?  (csrc/calibration.hip) ----

CAL_MAX_BINS, CAL_FIX_SHIFT = _lib._K["DEPGAN_CAL_MAX_BINS"], _lib._K["DEPGAN_CAL_FIX_SHIFT"]
CAL_SCALARS = ("n", "n_nan", "n_bad", "n_floored")


def _float_kind(a, who):
    """0 for float32, 1 for float64 (a NumPy array or a tensor); ValueError for anything else."""
    name = str(getattr(a, "dtype", "")).rpartition(".")[2]
    if name not in ("float32", "float64"):
        raise ValueError("%s: prob must be float32 or float64, got %s" % (who, getattr(a, "dtype", type(a).__name__)))
    return 0 if name == "float32" else 1


def _cal_args(who, prob, labels=None, ignore_label=None, mask=None, eps=1e-7, eps_positive=False, need_labels=True):
    """The argument checks the calibration functions share, before anything touches the device.  Returns
    (shape of prob, prob_kind, ignore code or -1, eps)."""
    shape = tuple(int(d) for d in getattr(prob, "shape", ()))
    if len(shape) != 4 or min(shape) < 1 or not 2 <= shape[3] <= _lib.MAX_HEAD_CLASSES:
        raise ValueError("%s: prob must be (n, H, W, C) with C in 2..%d, got shape %s"
                         % (who, _lib.MAX_HEAD_CLASSES, shape))
    kind = _float_kind(prob, who)
    if shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError("%s: prob has 2^31 pixels or more" % who)
    if need_labels:
        lshape = tuple(int(d) for d in getattr(labels, "shape", ()))
        if lshape != shape[:3] or str(getattr(labels, "dtype", "")).rpartition(".")[2] != "uint8":
            raise ValueError("%s: labels must be uint8 class codes of shape %s (data.to_codes), got %s %s"
                             % (who, shape[:3], getattr(labels, "dtype", type(labels).__name__), lshape))
        if mask is not None and tuple(int(d) for d in getattr(mask, "shape", ())) != shape[:3]:
            raise ValueError("%s: mask must have the shape of labels, %s" % (who, shape[:3]))
    if ignore_label is None:
        ignore = -1
    elif isinstance(ignore_label, bool) or not isinstance(ignore_label, (int, np.integer)) or not 0 <= ignore_label <= 255:
        raise ValueError("%s: ignore_label must be None or an integer in 0..255, got %r" % (who, ignore_label))
    else:
        ignore = int(ignore_label)
    try:
        e = float(eps)
    except (TypeError, ValueError):
        e = float("nan")
    if not (0.0 <= e < 1.0) or (eps_positive and e == 0.0):
        raise ValueError("%s: eps must lie in %s0, 1), got %r" % (who, "(" if eps_positive else "[", eps))
    return shape, kind, ignore, e


def _cal_tensor(a, dev, dtype):
    """contiguous, 16-byte aligned device tensor of `a` (host or device), or None"""
    torch = _torch()
    if a is None:
        return None
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.to(device=dev, dtype=dtype).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _cal_device(prob, kind, labels, mask):
    """the operands on the device.  The mask is judged in its own dtype: the entries get (mask != 0) as float32, so a
    float64 value that float32 would flush to zero keeps its pixel, as NumPy's `mask != 0` does."""
    torch = _torch()
    dev = _surface_device(prob, labels, mask)
    if mask is not None:
        mask = mask != 0 if isinstance(mask, torch.Tensor) else np.asarray(mask) != 0
    return (dev, _cal_tensor(prob, dev, torch.float64 if kind else torch.float32), _cal_tensor(labels, dev, torch.uint8),
            _cal_tensor(mask, dev, torch.float32), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))


def _cal_scratch(lib, dev, npix, Cc, bins):
    return _torch().empty((max(1, int(lib.depgan_eval_calibration_scratch_bytes(npix, Cc, bins)) // 8),),
                          dtype=_torch().float64, device=dev)


def calibration_census(prob, labels, bins=15, ignore_label=None, mask=None, eps=1e-7):
    """The integer tables every calibration figure is formed from, counted on the device in one pass over the pixels
    (depgan_eval_calibration_census; include/depgan.h states every operation).  prob: (n, H, W, C) float32 (predict) or
    float64 (predict_mean, predict_stats(...)['mean']); labels: (n, H, W) uint8 class codes (data.to_codes); mask:
    (n, H, W) or None, a pixel with a zero mask takes no part; ignore_label: a code whose pixels take no part; a row with
    a NaN takes no part and is counted in n_nan.  All host or device.  `bins` equal-width bins, 1..64.  Returns a dict of
    NumPy int64 arrays and Python numbers:
      top_count, top_correct, top_conf_q       (bins): per bin of the top-label confidence its pixels, those of them whose
                                               arg-max (first maximum) is the true class, and the sum of their
                                               confidences in units of 2^-32
      class_count, class_pos, class_prob_q     (C, bins): per class k and bin of p_k the pixels, those of class k, and the
                                               sum of p_k in units of 2^-32
      n, n_nan, n_bad, n_floored               pixels that take part, rows with a NaN, codes >= C (always 0: such a code
                                               raises), pixels whose true-class probability is below eps
      brier_sum, nll_sum                       sums over the pixels of sum_c (p_c - t_c)^2 and of -log(max(p_true, eps))
      bins, n_class, eps
    calibration_metrics turns them into ECE, MCE, Brier, NLL and the reliability diagram."""
    who = "calibration_census"
    shape, kind, ignore, eps = _cal_args(who, prob, labels, ignore_label, mask, eps)
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= CAL_MAX_BINS:
        raise ValueError("%s: bins must be an integer in 1..%d, got %r" % (who, CAL_MAX_BINS, bins))
    bins, Cc, npix = int(bins), shape[3], shape[0] * shape[1] * shape[2]
    lib = _lib.load()
    dev, p, lab, m, stream = _cal_device(prob, kind, labels, mask)
    scratch = _cal_scratch(lib, dev, npix, Cc, bins)
    counts = np.zeros((1 + Cc) * bins * 3 + len(CAL_SCALARS), np.int64)
    sums = np.zeros(2, np.float64)
    _lib.check(lib.depgan_eval_calibration_census(_p(p), kind, Cc, _p(lab), ignore, _p(m), npix, bins, eps, _p(scratch),
                                                  C.c_void_p(counts.ctypes.data), C.c_void_p(sums.ctypes.data), stream),
               "depgan_eval_calibration_census")
    return census_from_tables(counts, sums, Cc, bins, eps)


def census_from_tables(counts, sums, n_class, bins, eps):
    """The dict of calibration_census from the entry's two host tables (counts: (1 + C) * bins * 3 + 4 int64)."""
    tab = np.asarray(counts[:(1 + n_class) * bins * 3], np.int64).reshape(1 + n_class, bins, 3)
    res = {"top_count": tab[0, :, 0].copy(), "top_correct": tab[0, :, 1].copy(), "top_conf_q": tab[0, :, 2].copy(),
           "class_count": tab[1:, :, 0].copy(), "class_pos": tab[1:, :, 1].copy(), "class_prob_q": tab[1:, :, 2].copy()}
    res.update((k, int(v)) for k, v in zip(CAL_SCALARS, counts[-len(CAL_SCALARS):]))
    res.update(brier_sum=float(sums[0]), nll_sum=float(sums[1]), bins=int(bins), n_class=int(n_class), eps=float(eps))
    if res["n_bad"] > 0:
        raise ValueError("calibration_census: %d labels are not below the class count %d (and are not the ignore label)"
                         % (res["n_bad"], n_class))
    return res


def _bin_means(count, hits, q):
    """(share of hits, mean confidence) per bin, nan for an empty bin; any leading axes"""
    count = np.asarray(count, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(hits, np.float64) / count, np.asarray(q, np.float64) / 2.0 ** CAL_FIX_SHIFT / count


def calibration_metrics(census):
    """Calibration figures from the tables of calibration_census; pure NumPy, nothing raises.
      ece                 sum_b n_b / N |acc_b - conf_b| over the top-label bins: the expected calibration error
      mce                 the largest |acc_b - conf_b| of a non-empty bin
      classwise_ece       (C): sum_b n_kb / N |pos_kb / n_kb - mean p_k in bin b| per class k, one against the rest;
      classwise_ece_mean  their mean
      brier, nll          brier_sum / N, nll_sum / N
      accuracy, mean_confidence   of the top label; their difference is the over-confidence
      bin_count, bin_accuracy, bin_confidence   (bins): the reliability diagram, nan in an empty bin
    An empty bin contributes 0.  N = 0 gives nan figures; n, n_nan and n_floored are passed on and say why.  A bin's
    confidence is within 2^-33 of the mean of its values (the fixed point of the device sum)."""
    n = int(census["n"])
    acc, conf = _bin_means(census["top_count"], census["top_correct"], census["top_conf_q"])
    pos, pk = _bin_means(census["class_count"], census["class_pos"], census["class_prob_q"])
    res = {"n": n, "n_nan": int(census["n_nan"]), "n_floored": int(census["n_floored"]),
           "bin_count": np.asarray(census["top_count"], np.int64), "bin_accuracy": acc, "bin_confidence": conf}
    nan = float("nan")
    if n == 0:
        res.update(ece=nan, mce=nan, classwise_ece=np.full(len(pos), nan), classwise_ece_mean=nan, brier=nan, nll=nan,
                   accuracy=nan, mean_confidence=nan)
        return res
    gap = np.where(res["bin_count"] > 0, np.abs(acc - conf), 0.0)
    cgap = np.where(np.asarray(census["class_count"]) > 0, np.abs(pos - pk), 0.0)
    res["ece"] = float(np.sum(res["bin_count"] / n * gap))
    res["mce"] = float(np.max(gap))
    res["classwise_ece"] = np.sum(np.asarray(census["class_count"], np.float64) / n * cgap, axis=1)
    res["classwise_ece_mean"] = float(np.mean(res["classwise_ece"]))
    res["brier"], res["nll"] = float(census["brier_sum"]) / n, float(census["nll_sum"]) / n
    res["accuracy"] = float(np.sum(np.asarray(census["top_correct"], np.int64))) / n
    res["mean_confidence"] = float(int(np.sum(np.asarray(census["top_conf_q"], np.int64)))) / 2.0 ** CAL_FIX_SHIFT / n
    return res


def _temperature_args(who, bounds, tol, max_iter):
    try:
        lo, hi = (float(v) for v in bounds)
    except (TypeError, ValueError):
        lo = hi = float("nan")
    if not (0.0 < lo < hi < float("inf")):
        raise ValueError("%s: bounds must be two temperatures 0 < T_min < T_max, got %r" % (who, bounds))
    try:
        tol = float(tol)
    except (TypeError, ValueError):
        tol = float("nan")
    if not (0.0 < tol < float("inf")):
        raise ValueError("%s: tol must be a finite positive number, got %r" % (who, tol))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError("%s: max_iter must be a positive integer, got %r" % (who, max_iter))
    return (lo, hi), tol, int(max_iter)


def solve_temperature(sums, bounds=(0.05, 20.0), tol=1e-6, max_iter=50):
    """The solver of fit_temperature on any sums function: sums(beta) -> (N, sum L, sum L', sum L'') as
    depgan_eval_temperature_sums states them.  L is convex in beta = 1 / T, so Newton's method on beta is safeguarded by
    a bracket: a step that leaves the bracket goes to the far bound if that has not been looked at yet, else to the
    middle.  Stops when |sum L'| / N <= tol (converged), at a bound whose slope still points outwards (at_bound), or
    after max_iter evaluations besides the one at T = 1.  Returns the dict of fit_temperature."""
    (t_lo, t_hi), tol, max_iter = _temperature_args("solve_temperature", bounds, tol, max_iter)
    lo, hi = 1.0 / t_hi, 1.0 / t_lo
    n, L, g, h = (float(v) for v in sums(1.0))
    calls = 1
    nan = float("nan")
    res = {"T": nan, "beta": nan, "nll_before": nan, "nll_after": nan, "iterations": calls, "converged": False,
           "at_bound": False, "n": int(n)}
    if not n > 0:
        return res
    res["nll_before"] = L / n
    beta = min(max(1.0, lo), hi)
    if beta != 1.0:
        n, L, g, h = (float(v) for v in sums(beta))
        calls += 1
    a, b, a_seen, b_seen = lo, hi, False, False
    while True:
        slope = g / n
        if abs(slope) <= tol:
            res["converged"] = True
            break
        if (slope < 0 and beta >= hi) or (slope > 0 and beta <= lo):
            res["at_bound"] = True
            break
        if calls > max_iter:
            break
        if slope < 0:
            a, a_seen = beta, True
        else:
            b, b_seen = beta, True
        cand = beta - g / h if h > 0 and np.isfinite(h) else nan
        if not a < cand < b:
            cand = b if slope < 0 and not b_seen else a if slope > 0 and not a_seen else 0.5 * (a + b)
        beta = cand
        n, L, g, h = (float(v) for v in sums(beta))
        calls += 1
    res.update(T=1.0 / beta, beta=beta, nll_after=L / n, iterations=calls)
    return res


def fit_temperature(prob, labels, ignore_label=None, mask=None, eps=1e-7, bounds=(0.05, 20.0), tol=1e-6, max_iter=50):
    """The temperature T that minimises the negative log-likelihood of softmax(log(max(prob, eps)) / T) against the
    labels (temperature scaling, Guo et al. 2017), over the pixels that take part (calibration_census's rule).  Arguments
    as calibration_census; bounds = (T_min, T_max).  One device pass and one synchronisation per iteration
    (depgan_eval_temperature_sums returns the loss and its first two derivatives in beta = 1 / T); the probabilities stay
    on the device.  Before the first pass the labels are checked once on the device (a few elementwise launches over the
    codes and one synchronisation for the count): a code >= C that is not the ignore label raises ValueError, as in
    calibration_census.  Returns {'T', 'beta', 'nll_before' (at T = 1), 'nll_after', 'iterations' (device passes),
    'converged' (|dNLL/dbeta| <= tol), 'at_bound' (the minimum lies outside the bounds; T is the bound), 'n'}.  With no
    pixel taking part the figures are nan."""
    who = "fit_temperature"
    shape, kind, ignore, eps = _cal_args(who, prob, labels, ignore_label, mask, eps, eps_positive=True)
    _temperature_args(who, bounds, tol, max_iter)
    Cc, npix = shape[3], shape[0] * shape[1] * shape[2]
    torch = _torch()
    lib = _lib.load()
    dev, p, lab, m, stream = _cal_device(prob, kind, labels, mask)
    bad = lab >= Cc                  # uint8 against a Python int below 256: no wrap-around
    if ignore >= 0:                  # -1 means no ignore label; it is never compared with the uint8 codes
        bad &= lab != ignore
    if m is not None:
        bad &= m != 0
    n_bad = int(bad.sum())
    if n_bad:
        raise ValueError("%s: %d labels are not below the class count %d (and are not the ignore label)" % (who, n_bad, Cc))
    scratch = _cal_scratch(lib, dev, npix, Cc, 1)

    def sums(beta):
        out = (C.c_double * 4)()
        _lib.check(lib.depgan_eval_temperature_sums(_p(p), kind, Cc, _p(lab), ignore, _p(m), npix, float(beta), eps,
                                                    _p(scratch), out, stream), "depgan_eval_temperature_sums")
        return tuple(float(v) for v in out)

    return solve_temperature(sums, bounds, tol, max_iter)


def apply_temperature(prob, T, eps=1e-7, out=None):
    """softmax(log(max(prob, eps)) / T) per pixel, formed in double and rounded once: a device tensor of the shape and
    kind (float32 / float64) of prob, which may be host or device.  out: a contiguous device tensor of that shape and
    kind to write into -- prob itself scales in place.  Enqueued on the current stream; nothing synchronises."""
    who = "apply_temperature"
    shape, kind, _, eps = _cal_args(who, prob, eps=eps, need_labels=False)
    try:
        beta = 1.0 / float(T)
    except (TypeError, ValueError, ZeroDivisionError):
        beta = float("nan")
    if not (0.0 < beta < float("inf")):
        raise ValueError("%s: T must be a finite positive temperature, got %r" % (who, T))
    torch = _torch()
    dtype = torch.float64 if kind else torch.float32
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == dtype and tuple(out.shape) == shape
                and out.is_contiguous() and out.data_ptr() % 16 == 0):
            raise ValueError("%s: out must be a contiguous device tensor of the shape and kind of prob" % who)
    lib = _lib.load()
    dev = out.device if out is not None else _surface_device(prob)
    p = out if out is prob else _cal_tensor(prob, dev, dtype)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.depgan_eval_apply_temperature(_p(p), kind, shape[3], beta, eps, _p(out), shape[0] * shape[1] * shape[2],
                                                 stream), "depgan_eval_apply_temperature")
    return out
