"""NumPy restatement of csrc/components.hip and of the lesion algebra of evaluate.lesion_detection.

`label` is a minimum-index propagation, not the kernels' union-find: every set voxel starts with its own linear index,
takes the minimum over its neighbourhood, and then follows its label (which is the index of a voxel of the same
component) until nothing moves.  At the fixed point every voxel of a component holds the component's smallest index;
numbering those in index order is the canonical numbering, scipy.ndimage.label's.  All of it is whole-array NumPy, so a
(3, 256, 256) volume takes well under a second."""
import itertools

import numpy as np


def offsets(connectivity, in_plane):
    """The neighbour offsets (dz, dy, dx) of scipy's generate_binary_structure(3, connectivity), without the centre;
    in_plane keeps those inside the slice.  6 / 18 / 26 in the volume, 4 / 8 / 8 in the slice."""
    if connectivity not in (1, 2, 3) or in_plane not in (0, 1, False, True):
        raise ValueError((connectivity, in_plane))
    out = []
    for d in itertools.product((-1, 0, 1), repeat=3):
        if any(d) and sum(abs(c) for c in d) <= connectivity and not (in_plane and d[0]):
            out.append(d)
    return out


def label(a, connectivity=1, in_plane=False):
    """a: (D, H, W), non-zero = set.  Returns (int32 labels, N): 0 where unset, components numbered 1..N in the order of
    their smallest linear index."""
    a = np.asarray(a) != 0
    D, H, W = a.shape
    n = a.size
    lab = np.where(a, np.arange(n, dtype=np.int64).reshape(a.shape), n)        # n: unset, larger than any index
    offs = offsets(connectivity, in_plane)
    while True:
        p = np.pad(lab, 1, constant_values=n)
        m = lab
        for dz, dy, dx in offs:
            m = np.minimum(m, p[1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        new = np.append(np.where(a, m, n).ravel(), n)                          # entry n maps to itself
        while True:                                                            # follow the labels to their ends
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        new = new[:n].reshape(a.shape)
        if np.array_equal(new, lab):
            break
        lab = new
    roots = np.unique(lab[a])                                                  # sorted: the order of the first voxels
    out = np.zeros(a.shape, np.int32)
    out[a] = np.searchsorted(roots, lab[a]) + 1
    return out, int(len(roots))


def sizes_hits(labels, n, other=None):
    """(size, hits) of components 1..n, int64: voxel counts, and the voxels where `other` is non-zero (zeros if None)."""
    flat = np.asarray(labels).ravel()
    size = np.bincount(flat, minlength=n + 1)[1:n + 1]
    if other is None:
        return size, np.zeros(n, np.int64)
    return size, np.bincount(flat[np.asarray(other).ravel() != 0], minlength=n + 1)[1:n + 1]


def remove_small(a, min_voxels, connectivity=1, in_plane=False):
    """uint8: `a` binarised, with the components of fewer than min_voxels voxels cleared"""
    a = np.asarray(a) != 0
    if min_voxels <= 1:
        return a.astype(np.uint8)
    lab, n = label(a, connectivity, in_plane)
    keep = np.concatenate([[False], sizes_hits(lab, n)[0] >= min_voxels])
    return keep[lab].astype(np.uint8)


KEYS = ("n_truth", "n_pred", "n_truth_detected", "n_pred_true", "recall", "precision", "f1", "voxels_truth",
        "voxels_pred", "avd_percent")


def ratio(a, b):
    return a / b if b else float("nan")


def lesion_detection(pred, truth, connectivity=3, in_plane=False, min_voxels=1, voxel_volume=None):
    """The dict evaluate.lesion_detection returns, sizes_truth / sizes_pred as NumPy arrays."""
    t = remove_small(truth, min_voxels, connectivity, in_plane)
    p = remove_small(pred, min_voxels, connectivity, in_plane)
    lt, nt = label(t, connectivity, in_plane)
    lp, npd = label(p, connectivity, in_plane)
    size_t, hits_t = sizes_hits(lt, nt, p)
    size_p, hits_p = sizes_hits(lp, npd, t)
    ntd, npt = int((hits_t > 0).sum()), int((hits_p > 0).sum())
    vt, vp = int(size_t.sum()), int(size_p.sum())
    recall, precision = ratio(ntd, nt), ratio(npt, npd)
    if np.isnan(recall) or np.isnan(precision):
        f1 = float("nan")
    else:
        f1 = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
    out = {"n_truth": nt, "n_pred": npd, "n_truth_detected": ntd, "n_pred_true": npt, "recall": recall,
           "precision": precision, "f1": f1, "voxels_truth": vt, "voxels_pred": vp,
           "avd_percent": ratio(100.0 * abs(vp - vt), vt)}
    if voxel_volume is None:
        out["sizes_truth"], out["sizes_pred"] = size_t.astype(np.int32), size_p.astype(np.int32)
    else:
        out["sizes_truth"] = size_t.astype(np.float64) * float(voxel_volume)
        out["sizes_pred"] = size_p.astype(np.float64) * float(voxel_volume)
    return out
