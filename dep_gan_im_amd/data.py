"""Data step in front of the path: NIfTI volumes -> training slices resident in HBM.

Mirrors what DEP-GAN_PROB_IM_twoCritics_training_4fold.py ("GT") does between its file lists and the first
training batch (GT:613-760): read seven lists of volume paths, per subject load the volumes, extract the 2D slices,
mask by the intracranial volume and (when the file exists) the inverted stroke-lesion mask, map the FLAIR channel
to [0, 1], clamp the probability maps at 0, concatenate the channels, stack all subjects, split off 2 % for
validation (train_test_split, random_state 42) and shuffle the rest.

Here the arithmetic of a subject runs on the GPU (`depgan_data_prep_subject`, include/depgan.h) while a host
thread reads and decodes the next subject's files into pinned memory, so a training set is assembled at file-read
speed and never exists on the host as float arrays.  Results are bit-identical to the NumPy statements
(oracle/data_oracle.py restates them for the tests).

The DEP-UResNet training script ("UT", DEP-UResNet-wNoises-training-4fold.py:434-566) prepares its inputs differently:
four lists (`uresnet_file_lists`), FLAIR z-scored over the whole masked volume instead of mapped to [0, 1]
(`depgan_data_prep_zscore`), the coded change map masked like the FLAIR as the target, and 4-class one-hot labels
made from it (`to_one_hot`).  `load_uresnet_training_set` is its counterpart of `load_training_set`; `zscore_flair`
and `mask_slices` also build every array the DEP-UResNet evaluation script ("UE") derives from its volumes.

List pairing: both scripts walk their first list and read the other lists at a counter `id` that advances only for
files that exist (GT:662-733, UT:478-526), so after a missing first-list file every later subject would be read
together with the previous line's other files.  That drift is deliberately not reproduced: here the lists are paired
by line, and a missing first-list file skips its whole line.
"""
from __future__ import annotations

import ctypes as C
import os
import queue
import threading
from collections import namedtuple

import numpy as np

from . import _lib, nifti

SubjectFiles = namedtuple("SubjectFiles", "prob_1tp flair_1tp icv_1tp sl_1tp prob_2tp icv_2tp sl_2tp")

# list-file stems, GT:613-660
_LISTS = (("prob_1tp", "wmh_prob_1tp"), ("flair_1tp", "flair_1tp"), ("icv_1tp", "icv_1tp"),
          ("sl_1tp", "sl_cleaned_1tp"), ("prob_2tp", "wmh_prob_2tp"), ("icv_2tp", "icv_2tp"),
          ("sl_2tp", "sl_cleaned_2tp"))


def read_list(path):
    """GT:614-618: one path per line, trailing newline stripped (nothing else)."""
    with open(path, "r") as f:
        return [line.strip("\n") for line in f]


def training_file_lists(config_dir, fold):
    """The seven lists of GT:613-660 as one SubjectFiles per line index."""
    cols = {k: read_list(os.path.join(config_dir, "%s_fold%s.txt" % (stem, fold))) for k, stem in _LISTS}
    n = len(cols["prob_1tp"])
    for k, v in cols.items():
        if len(v) < n:
            raise ValueError("list %s has %d entries, wmh_prob_1tp has %d" % (k, len(v), n))
    return [SubjectFiles(*[cols[k][i] for k in SubjectFiles._fields]) for i in range(n)]


def _file_order_f32(vol):
    """(X, Y, Z) volume of any dtype -> flat float32 in file order (x fastest); the cast is data_prep's (GT:113)."""
    a = np.asarray(vol)
    if a.ndim != 3:
        raise ValueError("expected a 3-D volume, got shape %s" % (a.shape,))
    a = np.asfortranarray(a, dtype=np.float32)
    if not a.flags.writeable:           # a float32 file decodes to a read-only view of the file buffer
        a = a.copy(order="F")
    return a.reshape(-1, order="F")


def prep_subject(p1, f1, icv1, sl1, p2, icv2, sl2, nicg=2, device=None, stream=None):
    """One subject on the GPU.  Volumes: (X, Y, Z) NumPy arrays of any dtype or flat float32 CUDA tensors already in
    file order together with `shape=` ... (see prep_subject_flat); sl1 / sl2 / f1 may be None.
    Returns (x (Z, X, Y, nicg), y2 (Z, X, Y, 1)) as float32 CUDA tensors."""
    import torch
    dev = torch.device(device if device is not None else "cuda:0")
    shape = tuple(np.shape(p1))
    vols = []
    for v in (p1, f1, icv1, sl1, p2, icv2, sl2):
        if v is None:
            vols.append(None)
            continue
        if tuple(np.shape(v)) != shape:
            raise ValueError("volume shapes differ: %s vs %s" % (np.shape(v), shape))
        vols.append(torch.from_numpy(_file_order_f32(v)).to(dev, non_blocking=True))
    return prep_subject_flat(vols, shape, nicg, dev, stream)


def prep_subject_flat(vols, shape, nicg, dev, stream=None):
    """vols: [p1, f1, icv1, sl1, p2, icv2, sl2] flat float32 CUDA tensors in file order (None where absent)."""
    import torch
    lib = _lib.load()
    X, Y, Z = (int(s) for s in shape)
    if nicg == 2 and vols[1] is None:
        raise ValueError("nicg = 2 needs the FLAIR volume")
    for v in vols:
        if v is not None and (v.dtype != torch.float32 or v.numel() != X * Y * Z or not v.is_cuda):
            raise ValueError("volumes must be float32 CUDA tensors of X*Y*Z elements")
    x = torch.empty((Z, X, Y, nicg), dtype=torch.float32, device=dev)
    y2 = torch.empty((Z, X, Y, 1), dtype=torch.float32, device=dev)
    scratch = torch.empty(int(lib.depgan_data_prep_scratch_floats(X, Y, Z)), dtype=torch.float32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream

    def p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    _lib.check(lib.depgan_data_prep_subject(p(vols[0]), p(vols[1]), p(vols[2]), p(vols[3]), p(vols[4]), p(vols[5]),
                                            p(vols[6]), X, Y, Z, int(nicg), p(x), p(y2), p(scratch),
                                            C.c_void_p(st)), "depgan_data_prep_subject")
    return x, y2


def _read_subject(files, nicg, pin):
    """Host side of one subject: decode the NIfTI files into flat float32 (pinned) tensors.  A missing stroke-lesion
    file means "no mask" (GT:690, 698: os.path.isfile)."""
    import torch
    out, shape = [], None
    for key in SubjectFiles._fields:
        path = getattr(files, key)
        optional = key.startswith("sl_")
        if (key == "flair_1tp" and nicg == 1) or (optional and not os.path.isfile(path)):
            out.append(None)
            continue
        vol = nifti.load(path).image
        if shape is None:
            shape = vol.shape
        elif vol.shape != shape:
            raise ValueError("%s: shape %s differs from %s" % (path, vol.shape, shape))
        t = torch.from_numpy(_file_order_f32(vol))
        out.append(t.pin_memory() if pin else t)
    return out, shape


def _prefetched(items, read, prefetch):
    """Yields (item, read(item)) in order while a reader thread keeps `prefetch` results ahead of the consumer."""
    q = queue.Queue(maxsize=max(1, int(prefetch)))

    def reader():
        try:
            for s in items:
                q.put((s, read(s)))
            q.put(None)
        except BaseException as e:      # surfaced on the consumer side
            q.put(e)

    th = threading.Thread(target=reader, daemon=True)
    th.start()
    while True:
        item = q.get()
        if item is None:
            break
        if isinstance(item, BaseException):
            raise item
        yield item
    th.join()


def load_training_set(subjects, nicg=2, device=None, prefetch=2, progress=None):
    """GT:663-733: every subject whose wmh_prob_1tp file exists, stacked along the slice axis.
    subjects: list of SubjectFiles (training_file_lists).  Returns (x (N, X, Y, nicg), y2 (N, X, Y, 1)) on `device`.
    A reader thread keeps `prefetch` decoded subjects ahead of the GPU."""
    import torch
    dev = torch.device(device if device is not None else "cuda:0")
    todo = [s for s in subjects if os.path.isfile(s.prob_1tp)]
    xs, ys = [], []
    for s, (host, shape) in _prefetched(todo, lambda s: _read_subject(s, nicg, pin=True), prefetch):
        vols = [None if t is None else t.to(dev, non_blocking=True) for t in host]
        x, y2 = prep_subject_flat(vols, shape, nicg, dev)
        xs.append(x)
        ys.append(y2)
        if progress is not None:
            progress(s, tuple(x.shape))
    if not xs:
        raise ValueError("no subject with an existing wmh_prob_1tp file")
    return torch.cat(xs, 0), torch.cat(ys, 0)


def split_and_shuffle(x, y2, rng=None):
    """GT:738-760 on device tensors: train_test_split(test_size=0.02, random_state=42) restated (ShuffleSplit: the
    first ceil(0.02 n) entries of RandomState(42).permutation(n) validate, the rest train), then the training
    indices shuffled with `rng` (np.random.RandomState or module np.random, as the reference's np.random.shuffle).
    Returns x_train, x_val, y2_train, y2_val."""
    import torch
    n = int(x.shape[0])
    n_val = int(np.ceil(0.02 * n))
    perm = np.random.RandomState(42).permutation(n)
    val, train = perm[:n_val], perm[n_val:]
    idx = np.array(range(train.shape[0]))
    (rng if rng is not None else np.random).shuffle(idx)
    train = train[idx]
    tv = torch.from_numpy(val.astype(np.int64)).to(x.device)
    tt = torch.from_numpy(train.astype(np.int64)).to(x.device)
    return x.index_select(0, tt), x.index_select(0, tv), y2.index_select(0, tt), y2.index_select(0, tv)


# ---- DEP-UResNet data step (UT:434-566; the same statements in UE:496-540) ----

UResNetFiles = namedtuple("UResNetFiles", "flair_1tp coded icv_1tp sl_1tp")

# list-file stems, UT:446-468
_URESNET_LISTS = (("flair_1tp", "flair_1tp"), ("coded", "wmh_subtracted_coded_2tp_1tp"), ("icv_1tp", "icv_1tp"),
                  ("sl_1tp", "sl_cleaned_1tp"))


def uresnet_file_lists(config_dir, fold):
    """The four lists of UT:446-468 as one UResNetFiles per line index (FLAIR, coded change map, ICV, stroke lesions)."""
    cols = {k: read_list(os.path.join(config_dir, "%s_fold%s.txt" % (stem, fold))) for k, stem in _URESNET_LISTS}
    n = len(cols["flair_1tp"])
    for k, v in cols.items():
        if len(v) < n:
            raise ValueError("list %s has %d entries, flair_1tp has %d" % (k, len(v), n))
    return [UResNetFiles(*[cols[k][i] for k in UResNetFiles._fields]) for i in range(n)]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev, stream):
    import torch
    return C.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)


def _check_flat(vols, npix):
    import torch
    for v in vols:
        if v is not None and (v.dtype != torch.float32 or v.numel() != npix or not v.is_cuda):
            raise ValueError("volumes must be float32 CUDA tensors of X*Y*Z elements")


def _flat_volumes(vols, device):
    """(X, Y, Z) NumPy volumes (None allowed) -> (flat float32 CUDA tensors in file order, shape, device)."""
    import torch
    dev = torch.device(device if device is not None else "cuda:0")
    shape = None
    out = []
    for v in vols:
        if v is None:
            out.append(None)
            continue
        if shape is None:
            shape = tuple(np.shape(v))
        elif tuple(np.shape(v)) != shape:
            raise ValueError("volume shapes differ: %s vs %s" % (np.shape(v), shape))
        out.append(torch.from_numpy(_file_order_f32(v)).to(dev, non_blocking=True))
    return out, shape, dev


def zscore_flair_flat(f1, icv1, sl1, shape, dev, stream=None, with_stats=False):
    """f1 / icv1 / sl1: flat float32 CUDA tensors in file order (sl1 may be None).  Returns the z-scored brain FLAIR
    (Z, X, Y, 1) of UT:485-512 [and the device's (mean32, std32) as a (2,) float32 CUDA tensor]."""
    import torch
    lib = _lib.load()
    X, Y, Z = (int(s) for s in shape)
    if f1 is None or icv1 is None:
        raise ValueError("the z-score needs the FLAIR and the ICV volume")
    _check_flat((f1, icv1, sl1), X * Y * Z)
    out = torch.empty((Z, X, Y, 1), dtype=torch.float32, device=dev)
    stats = torch.empty(2, dtype=torch.float32, device=dev) if with_stats else None
    scratch = torch.empty(int(lib.depgan_data_zscore_scratch_floats(X, Y, Z)), dtype=torch.float32, device=dev)
    _lib.check(lib.depgan_data_prep_zscore(_p(f1), _p(icv1), _p(sl1), X, Y, Z, _p(out), _p(stats), _p(scratch),
                                           _stream(dev, stream)), "depgan_data_prep_zscore")
    return (out, stats) if with_stats else out


def zscore_flair(f1, icv1, sl1=None, device=None, stream=None, with_stats=False):
    """UT:510-512 / UE:538-540 on (X, Y, Z) volumes of any dtype: brain_flair_1tp = f1*icv1 [*(1 - sl1)], then
    nan_to_num((brain - mean) / std) over the whole volume.  Returns (Z, X, Y, 1) float32 on the GPU."""
    vols, shape, dev = _flat_volumes((f1, icv1, sl1), device)
    return zscore_flair_flat(*vols, shape, dev, stream, with_stats)


def mask_slices_flat(vol, m_a, sl, shape, dev, stream=None):
    """(vol [* m_a]) [* (1 - sl)] as (Z, X, Y, 1) slices; flat float32 CUDA tensors in file order."""
    import torch
    lib = _lib.load()
    X, Y, Z = (int(s) for s in shape)
    if vol is None:
        raise ValueError("mask_slices needs a volume")
    _check_flat((vol, m_a, sl), X * Y * Z)
    out = torch.empty((Z, X, Y, 1), dtype=torch.float32, device=dev)
    _lib.check(lib.depgan_data_mask_slices(_p(vol), _p(m_a), _p(sl), X, Y, Z, _p(out), _stream(dev, stream)),
               "depgan_data_mask_slices")
    return out


def mask_slices(vol, m_a=None, sl=None, device=None, stream=None):
    """np.multiply(vol, m_a) [then np.multiply(., 1 - sl)] on (X, Y, Z) volumes, as the reference's slices
    (Z, X, Y, 1) float32 on the GPU.  UT brain_wsc_1tp = mask_slices(wsc, icv1, sl1); UE brain_wmh_1tp / _2tp likewise,
    brain_cod_2tp = mask_slices(code2, icv2) (no stroke-lesion factor, UE:515), icv_and_sl_mask_1tp =
    mask_slices(icv1, None, sl1)."""
    vols, shape, dev = _flat_volumes((vol, m_a, sl), device)
    return mask_slices_flat(*vols, shape, dev, stream)


def _read_uresnet_subject(files, pin):
    """Host side of one UT subject: [flair, coded, icv, sl or None] as flat float32 (pinned) tensors.  A missing
    stroke-lesion file means "no mask" (UT:500: os.path.isfile)."""
    import torch
    out, shape = [], None
    for key in UResNetFiles._fields:
        path = getattr(files, key)
        if key == "sl_1tp" and not os.path.isfile(path):
            out.append(None)
            continue
        vol = nifti.load(path).image
        if shape is None:
            shape = vol.shape
        elif vol.shape != shape:
            raise ValueError("%s: shape %s differs from %s" % (path, vol.shape, shape))
        t = torch.from_numpy(_file_order_f32(vol))
        out.append(t.pin_memory() if pin else t)
    return out, shape


def load_uresnet_training_set(subjects, device=None, prefetch=2, progress=None):
    """UT:474-531: every subject whose FLAIR file exists, stacked along the slice axis.
    subjects: list of UResNetFiles (uresnet_file_lists).  Returns (flair (N, X, Y, 1), coded (N, X, Y, 1)) on `device`:
    the z-scored brain FLAIR and brain_wsc_1tp = coded*icv1 [*(1 - sl1)].  split_and_shuffle takes them as they are;
    to_one_hot makes the labels, to_codes their 1-byte form for loss='sparse_categorical_crossentropy'.  A reader thread
    keeps `prefetch` decoded subjects ahead of the GPU."""
    import torch
    dev = torch.device(device if device is not None else "cuda:0")
    todo = [s for s in subjects if os.path.isfile(s.flair_1tp)]
    fs, cs = [], []
    for s, (host, shape) in _prefetched(todo, lambda s: _read_uresnet_subject(s, pin=True), prefetch):
        f1, code, icv1, sl1 = [None if t is None else t.to(dev, non_blocking=True) for t in host]
        fs.append(zscore_flair_flat(f1, icv1, sl1, shape, dev))           # UT:494-512
        cs.append(mask_slices_flat(code, icv1, sl1, shape, dev))          # UT:494-502
        if progress is not None:
            progress(s, tuple(fs[-1].shape))
    if not fs:
        raise ValueError("no subject with an existing flair_1tp file")
    return torch.cat(fs, 0), torch.cat(cs, 0)


def _check_ignore_label(ignore_label):
    if ignore_label is None:
        return None
    if isinstance(ignore_label, bool) or not isinstance(ignore_label, (int, np.integer)) or not 0 <= ignore_label <= 255:
        raise ValueError("ignore_label must be an integer in [0, 255], got %r" % (ignore_label,))
    return int(ignore_label)


def to_one_hot(coded, n_class=4, device=None, ignore_label=None):
    """UT:563-568: coded.astype(int) (truncation toward zero), then convert_to_1hot(., n_class) and np.squeeze.
    coded: (N, X, Y, 1) or (N, X, Y) array / tensor.  Returns (N, X, Y, n_class) float32 on the GPU, the layout
    Gen_UNet2D(..., nc_out=4).fit reads.  A value outside [0, n_class) raises DepganError (NumPy would wrap a
    negative index).  ignore_label: the value that truncates to it becomes an all-zero row, the ignored pixel of the
    loss-weight mode (compile(class_weight=...)); every other out-of-range value is refused as before."""
    ignore_label = _check_ignore_label(ignore_label)
    if isinstance(n_class, bool) or not isinstance(n_class, (int, np.integer)) or not 1 <= int(n_class) <= 127:
        raise ValueError("n_class must be an integer in [1, 127], got %r" % (n_class,))
    shape = tuple(int(d) for d in (coded.shape if hasattr(coded, "shape") else np.shape(coded)))
    if len(shape) == 4 and shape[3] == 1:
        shape = shape[:3]
    if len(shape) != 3:
        raise ValueError("coded must be (N, X, Y, 1) or (N, X, Y), got shape %s" % (shape,))
    import torch
    lib = _lib.load()
    if isinstance(coded, torch.Tensor):
        dev = coded.device if device is None and coded.is_cuda else torch.device(device or "cuda:0")
        t = coded.to(device=dev, dtype=torch.float32).contiguous()
    else:
        dev = torch.device(device if device is not None else "cuda:0")
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(coded), dtype=np.float32)).to(dev)
    ign = None
    if ignore_label is not None:
        ign = torch.trunc(t) == float(ignore_label)
        t = torch.where(ign, torch.zeros_like(t), t)
    out = torch.empty(shape + (int(n_class),), dtype=torch.float32, device=dev)
    _lib.check(lib.depgan_labels_to_onehot(_p(t), t.numel(), int(n_class), _p(out), _stream(dev, None)),
               "depgan_labels_to_onehot")
    if ign is not None:
        out[ign.reshape(shape)] = 0.0
    return out


def to_codes(coded, n_class=4, device=None, ignore_label=None):
    """The 1-byte counterpart of to_one_hot: coded.astype(int) (truncation toward zero, UT:563) as class indices.
    coded: (N, X, Y, 1) or (N, X, Y) array / tensor.  Returns (N, X, Y) uint8 on the GPU, the layout
    Gen_UNet2D(..., nc_out=n_class).compile(loss='sparse_categorical_crossentropy').fit reads: 1 byte per pixel where
    the one-hot tensor has 4 * n_class.  A value outside [0, n_class) raises DepganError, as in to_one_hot.
    ignore_label: the value that truncates to it passes through as that byte (compile(ignore_label=...))."""
    ignore_label = _check_ignore_label(ignore_label)
    if isinstance(n_class, bool) or not isinstance(n_class, (int, np.integer)) or not 1 <= int(n_class) <= 127:
        raise ValueError("n_class must be an integer in [1, 127], got %r" % (n_class,))
    shape = tuple(int(d) for d in (coded.shape if hasattr(coded, "shape") else np.shape(coded)))
    if len(shape) == 4 and shape[3] == 1:
        shape = shape[:3]
    if len(shape) != 3:
        raise ValueError("coded must be (N, X, Y, 1) or (N, X, Y), got shape %s" % (shape,))
    import torch
    if isinstance(coded, torch.Tensor):
        dev = coded.device if device is None and coded.is_cuda else torch.device(device or "cuda:0")
        t = coded.to(device=dev, dtype=torch.float32).reshape(shape)
    else:
        dev = torch.device(device if device is not None else "cuda:0")
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(coded), dtype=np.float32)).to(dev).reshape(shape)
    ok = (t > -1.0) & (t < float(n_class))                 # trunc(v) in [0, n_class); False for NaN
    if ignore_label is not None:
        ok = ok | (torch.trunc(t) == float(ignore_label))
    bad = int((~ok).sum())
    if bad:
        raise _lib.DepganError("to_codes: %d of %d values truncate to a class outside [0, %d)"
                               % (bad, t.numel(), int(n_class)))
    return t.to(torch.uint8).contiguous()                  # float -> integer conversion truncates toward zero


def class_counts(labels, n_class, ignore_label=None, device=None, chunk=1 << 26, one_hot=None):
    """Pixels per class of a label set, counted on the device by the loss's label pre-pass (depgan_op_label_counts).
    labels: one-hot (..., n_class) float32, or class indices of any shape (uint8, or anything Engine-style narrowing to a
    byte accepts: integer dtypes and integral floats; a value outside [0, 255] counts as out of range), NumPy or tensor,
    of any size: it goes through in chunks of `chunk` pixels.  The true class of a one-hot row is its first arg-max and
    an all-zero row is ignored.  one_hot: None takes a floating array whose last dimension is n_class for one-hot rows
    and anything else for class indices; True / False says it.  Returns a dict: 'classes' (np.int64, n_class), 'ignored', 'bad' (codes >= n_class that
    are not ignore_label) and 'total'.  n_class in 2..8."""
    ignore_label = _check_ignore_label(ignore_label)
    if isinstance(n_class, bool) or not isinstance(n_class, (int, np.integer)) or not 2 <= int(n_class) <= _lib.MAX_HEAD_CLASSES:
        raise ValueError("n_class must be an integer in [2, %d], got %r" % (_lib.MAX_HEAD_CLASSES, n_class))
    import torch
    K = int(n_class)
    lib = _lib.load()
    tens = isinstance(labels, torch.Tensor)
    a = labels if tens else np.asarray(labels)
    dev = a.device if tens and a.is_cuda and device is None else torch.device(device if device is not None else "cuda:0")
    floating = a.is_floating_point() if tens else a.dtype.kind == "f"
    onehot = (floating and a.ndim >= 2 and int(a.shape[-1]) == K) if one_hot is None else bool(one_hot)
    if onehot and (a.ndim < 2 or int(a.shape[-1]) != K):
        raise ValueError("class_counts: one-hot labels must end in a dimension of n_class = %d, got shape %s" % (K, tuple(a.shape)))
    if onehot:
        flat = a.reshape(-1, K)
    else:
        flat = a.reshape(-1)
    P = int(flat.shape[0])
    if P < 1:
        raise ValueError("class_counts: no labels")
    tot = np.zeros(K + 3, np.int64)
    out = (C.c_longlong * _lib._K["DEPGAN_LABEL_NCOUNT"])()
    for i in range(0, P, int(chunk)):
        part = flat[i:i + int(chunk)]
        if onehot:
            t = (part if tens else torch.from_numpy(np.ascontiguousarray(part, dtype=np.float32)))
            t = t.to(device=dev, dtype=torch.float32).contiguous()
            args = (_p(t), None)
        else:
            if part.dtype != (torch.uint8 if tens else np.uint8):
                xp = torch if tens else np
                if floating and not bool((part == xp.trunc(part)).all()):
                    raise ValueError("class_counts: class indices must hold integral values")
                badv = (part < 0) | (part > 255)
                part = xp.where(badv, xp.full_like(part, 254 if ignore_label == 255 else 255), part)
                part = part.to(torch.uint8) if tens else part.astype(np.uint8)
            t = (part if tens else torch.from_numpy(np.ascontiguousarray(part))).to(dev).contiguous()
            args = (None, _p(t))
        _lib.check(lib.depgan_op_label_counts(args[0], args[1], int(t.shape[0]), K,
                                              -1 if ignore_label is None else ignore_label, out, _stream(dev, None)),
                   "depgan_op_label_counts")
        tot += np.array(out[:K + 3], np.int64)
    return {"classes": tot[3:].copy(), "ignored": int(tot[1]), "bad": int(tot[2]), "total": P}


def _signed_distance_args(shape, floating, n_class, spacing, ignore_label, inside_offset, classes):
    """The checks of signed_distance_maps, before anything touches the library: returns (n, H, W, one-hot?, (sy, sx),
    the ignore code or -1, the offset, the per-class switches or None)."""
    ignore_label = _check_ignore_label(ignore_label)
    if isinstance(n_class, bool) or not isinstance(n_class, (int, np.integer)) or not 2 <= int(n_class) <= _lib.MAX_HEAD_CLASSES:
        raise ValueError("n_class must be an integer in [2, %d], got %r" % (_lib.MAX_HEAD_CLASSES, n_class))
    K = int(n_class)
    onehot = floating and len(shape) == 4 and shape[3] == K
    if not onehot and len(shape) == 4 and shape[3] == 1:
        shape = shape[:3]
    if len(shape) != (4 if onehot else 3):
        raise ValueError("labels must be class indices (n, H, W) or (n, H, W, 1), or float one-hot rows (n, H, W, %d), "
                         "got shape %s" % (K, shape))
    n, H, W = shape[:3]
    if n < 1 or not 1 <= H <= 4096 or not 1 <= W <= 4096 or n * H * W >= 1 << 31:
        raise ValueError("labels: n >= 1 slices of 1..4096 pixels a side and fewer than 2^31 pixels in all, got %s" % (shape,))
    try:
        sp = tuple(spacing)
    except TypeError:
        sp = ()
    if len(sp) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) for v in sp) \
            or not all(np.isfinite(float(v)) and float(v) > 0 for v in sp):
        raise ValueError("spacing must be (sy, sx), two finite numbers > 0, got %r" % (spacing,))
    sp = (float(sp[0]), float(sp[1]))
    if isinstance(inside_offset, bool) or not isinstance(inside_offset, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(inside_offset) <= min(sp):
        raise ValueError("inside_offset must be a number in [0, min(spacing)] = [0, %g], got %r" % (min(sp), inside_offset))
    on = None
    if classes is not None:
        ks = [k for k in classes]
        if not ks or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < K for k in ks):
            raise ValueError("classes must be None or a non-empty list of class indices in [0, %d), got %r" % (K, classes))
        on = [1 if k in ks else 0 for k in range(K)]
    return n, H, W, onehot, sp, -1 if ignore_label is None else ignore_label, float(inside_offset), on


def signed_distance_maps(labels, n_class, spacing=(1, 1), ignore_label=None, inside_offset=0.0, classes=None, device=None):
    """The signed distance maps the boundary loss integrates against (compile(boundary_loss=True) computes them itself
    for every batch; this serves inspection and loops of one's own): depgan_op_signed_distance.
    labels: class indices (n, H, W) or (n, H, W, 1) (uint8, or any integer dtype or integral floats narrowed to a byte),
    or float one-hot rows (n, H, W, n_class), NumPy or tensor.  Per slice and class k, with S the pixels whose true class
    is k (the code, or the first arg-max of the row): phi = +distance to S outside it and -(distance to the complement -
    inside_offset) inside, exact Euclidean distances at pixel spacing (sy, sx), 0 where the class is absent from the slice
    or fills it.  ignore_label: pixels of that code -- or, for one-hot rows and any ignore_label, all-zero rows -- belong
    to no class.  classes: None, or the class indices that get a map (the others are 0).  Slices never see each other.
    Returns (n, H, W, n_class) float32 on the GPU."""
    import torch
    tens = isinstance(labels, torch.Tensor)
    a = labels if tens else np.asarray(labels)
    floating = a.is_floating_point() if tens else a.dtype.kind == "f"
    n, H, W, onehot, sp, ign, off, on = _signed_distance_args(tuple(int(d) for d in a.shape), floating, n_class, spacing,
                                                              ignore_label, inside_offset, classes)
    K = int(n_class)
    if not onehot:
        a = a.reshape(n, H, W)
        if a.dtype != (torch.uint8 if tens else np.uint8):
            xp = torch if tens else np
            if floating and not bool((a == xp.trunc(a)).all()):
                raise ValueError("signed_distance_maps: class indices must hold integral values")
            badv = (a < 0) | (a > 255)
            a = xp.where(badv, xp.full_like(a, 254 if ign == 255 else 255), a)
            a = a.to(torch.uint8) if tens else a.astype(np.uint8)
    lib = _lib.load()
    dev = a.device if tens and a.is_cuda and device is None else torch.device(device if device is not None else "cuda:0")
    if onehot:
        t = (a if tens else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))).to(device=dev, dtype=torch.float32)
        keep = t.contiguous()
        args = (_p(keep), None)
    else:
        keep = (a if tens else torch.from_numpy(np.ascontiguousarray(a))).to(dev).contiguous()
        args = (None, _p(keep))
    out = torch.empty((n, H, W, K), dtype=torch.float32, device=dev)
    sw = None if on is None else (C.c_int * K)(*on)
    _lib.check(lib.depgan_op_signed_distance(args[0], args[1], ign, n, H, W, K, sw, sp[0], sp[1], off, _p(out),
                                             _stream(dev, None)), "depgan_op_signed_distance")
    del keep
    return out


def balanced_class_weights(counts, rule="inverse"):
    """Class weights from pixel counts per class (class_counts(...)['classes']); host only.
    rule 'inverse': total / (C * n_k), scikit-learn's 'balanced'; rule 'median': median(n) / n_k over the classes that
    occur, median-frequency balancing.  A class that never occurs gets weight 0 (it cannot meet the loss); an input
    without any pixel is a ValueError, since all-zero weights are no valid setting.  Returns np.float64 (C,)."""
    if rule not in ("inverse", "median"):
        raise ValueError("rule must be 'inverse' or 'median', got %r" % (rule,))
    n = np.asarray(counts["classes"] if isinstance(counts, dict) else counts, np.float64).reshape(-1)
    if n.size < 1 or not np.all(np.isfinite(n)) or np.any(n < 0):
        raise ValueError("counts must be finite and >= 0, got %r" % (n.tolist(),))
    seen = n > 0
    if not seen.any():
        raise ValueError("balanced_class_weights: no class occurs (every count is 0)")
    w = np.zeros(n.size, np.float64)
    if rule == "inverse":
        w[seen] = n.sum() / (n.size * n[seen])
    else:
        w[seen] = np.median(n[seen]) / n[seen]
    return w


# ---- training-time augmentation (depgan_data_augment, csrc/augment.hip) ----

AUG_NPARAM = _lib._K["DEPGAN_AUG_NPARAM"]
AUG_MAX_GRID = _lib._K["DEPGAN_AUG_MAX_GRID"]        # a control grid of `augment` has 4 .. this many points per axis
_BORDERS = {"edge": 0, "constant": 1}
_ROT90 = np.array(((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)))   # (cos, sin) of 0, 90, 180, 270 degrees, exactly


def _affine_rows(H, W, deg, s, dy, dx, flip_lr, flip_ud, gain, offset):
    """affine_params for arrays of n values each: (n, 8) float32, composed in float64 and rounded once."""
    q = np.floor(deg / 90.0)
    exact = (deg == q * 90.0)[:, None]                # a multiple of 90 degrees: exact sines
    rad = np.deg2rad(deg)
    cs, sn = np.where(exact, _ROT90[q.astype(np.int64) % 4], np.stack([np.cos(rad), np.sin(rad)], 1)).T
    fy, fx = np.where(flip_ud, -1.0, 1.0), np.where(flip_lr, -1.0, 1.0)
    m00, m01, m10, m11 = fy * cs / s, fy * sn / s, -fx * sn / s, fx * cs / s
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    rows = np.stack([m00, m01, cy - m00 * (cy + dy) - m01 * (cx + dx),
                     m10, m11, cx - m10 * (cy + dy) - m11 * (cx + dx), gain, offset], 1)
    return (rows + 0.0).astype(np.float32)          # + 0.0: no negative zero among the coefficients


def affine_params(H, W, rotate_deg=0.0, scale=1.0, shift=(0.0, 0.0), flip_lr=False, flip_ud=False, gain=1.0,
                  offset=0.0):
    """One parameter row of `augment`: a00 a01 a02 a10 a11 a12 gain offset (np.float32, 8 values), the map from an
    output pixel (oy, ox) to its source coordinate sy = a00*oy + a01*ox + a02, sx = a10*oy + a11*ox + a12, taken about
    the image centre ((H-1)/2, (W-1)/2).  The picture turns by rotate_deg counter-clockwise as displayed (90 on a
    square image is np.rot90), grows by `scale`, moves by shift = (rows down, columns right) and is mirrored left-right
    / up-down; gain and offset act on the intensities, out = gain*v + offset.  Composed in float64 and rounded once to
    float32; a multiple of 90 degrees uses exact sines, and with all defaults the row is exactly [1,0,0,0,1,0,1,0]."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("affine_params: H and W must be >= 1, got %r x %r" % (H, W))
    vals = np.array([[float(v)] for v in (rotate_deg, scale, shift[0], shift[1], gain, offset)], np.float64)
    if not np.all(np.isfinite(vals)) or vals[1, 0] <= 0:
        raise ValueError("affine_params: arguments must be finite and scale > 0")
    deg, s, dy, dx, gain, offset = vals
    return _affine_rows(H, W, deg, s, dy, dx, np.array([bool(flip_lr)]), np.array([bool(flip_ud)]), gain, offset)[0]


def affine_inverse(rows):
    """The inverse maps of parameter rows: (..., 8) float32 rows of `affine_params` / `Augmenter.draw` in, rows of the
    same shape out.  A row maps an output pixel p to its source coordinate A p + b; its inverse maps q to
    A^-1 q - A^-1 b, so `augment` with a row followed by `augment` with its inverse brings a picture back to its frame
    (evaluate.predict_stats(tta=...) averages predictions that way).  The 2x2 inverse and the offset are computed in
    float64 from the float32 row and rounded once; the inverse of a flip, a quarter turn or an integer shift is exact.
    Elements 6 and 7 (gain, offset) become 1 and 0: an intensity change is not inverted.  A singular or non-finite row
    is a ValueError.  Pure NumPy."""
    r = np.asarray(rows, np.float32)
    if r.ndim < 1 or r.shape[-1] != AUG_NPARAM:
        raise ValueError("affine_inverse: rows must be (..., %d), got shape %s" % (AUG_NPARAM, r.shape))
    a00, a01, b0, a10, a11, b1 = (r[..., k].astype(np.float64) for k in range(6))
    det = a00 * a11 - a01 * a10
    if not np.all(np.isfinite(r[..., :6])) or not np.all(np.isfinite(det)) or np.any(det == 0):
        raise ValueError("affine_inverse: a row is singular or not finite")
    i00, i01, i10, i11 = a11 / det, -a01 / det, -a10 / det, a00 / det
    one = np.ones_like(det)
    out = np.stack([i00, i01, -(i00 * b0 + i01 * b1), i10, i11, -(i10 * b0 + i11 * b1), one, 0.0 * one], -1)
    out = (out + 0.0).astype(np.float32)              # + 0.0: no negative zero among the coefficients
    if not np.all(np.isfinite(out)):
        raise ValueError("affine_inverse: a row is singular or not finite")
    return out


def _aug_labels(labels, n_src, H, W, dev):
    """labels of `augment` -> (contiguous device tensor or None, lab_kind, C, shape of one output sample)."""
    import torch
    if labels is None:
        return None, 0, 0, None
    shape = tuple(int(d) for d in labels.shape) if hasattr(labels, "shape") else np.shape(labels)
    if shape in ((n_src, H, W), (n_src, H, W, 1)):
        tens = isinstance(labels, torch.Tensor)
        a = labels if tens else np.asarray(labels)
        u8 = torch.uint8 if tens else np.uint8
        if a.dtype != u8:
            from .engine import require_class_indices
            a = require_class_indices(a)
            if a.dtype != (torch.bool if tens else np.bool_) and bool(((a < 0) | (a > 255)).any()):
                raise ValueError("augment: class codes must lie in [0, 255]")
            a = a.to(u8) if tens else a.astype(u8)
        t = (a if tens else torch.from_numpy(np.ascontiguousarray(a))).to(dev).contiguous()
        return t, 1, 0, shape[1:]
    if len(shape) == 4 and shape[:3] == (n_src, H, W) and 2 <= shape[3] <= _lib.MAX_HEAD_CLASSES:
        if isinstance(labels, torch.Tensor):
            t = labels.to(device=dev, dtype=torch.float32).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(labels), dtype=np.float32)).to(dev)
        return t, 2, shape[3], shape[1:]
    raise ValueError("augment: labels must be class codes (%d, %d, %d[, 1]) or one-hot (%d, %d, %d, 2..%d), got shape %s"
                     % (n_src, H, W, n_src, H, W, _lib.MAX_HEAD_CLASSES, shape))


def _aug_fields_shape(fields, n):
    """The host-side check of the control grids of `augment`: (n, 3, gh, gw), or (3, gh, gw) for every sample, with
    gh and gw in [4, AUG_MAX_GRID].  Returns (gh, gw)."""
    shape = tuple(int(d) for d in fields.shape) if hasattr(fields, "shape") else np.shape(fields)
    if len(shape) not in (3, 4) or shape[-3] != 3 or (len(shape) == 4 and shape[0] != n):
        raise ValueError("augment: fields must be (%d, 3, gh, gw) or (3, gh, gw), got shape %s" % (n, shape))
    gh, gw = shape[-2:]
    if not (4 <= gh <= AUG_MAX_GRID and 4 <= gw <= AUG_MAX_GRID):
        raise ValueError("augment: a control grid has 4 to %d points per axis, got %d x %d" % (AUG_MAX_GRID, gh, gw))
    return gh, gw


def augment(x, labels=None, params=None, index=None, border="edge", x_fill=0.0, label_fill=0, device=None,
            stream=None, fields=None, return_fields=False):
    """The batch gather, an affine warp and an intensity change in one launch (depgan_data_augment).
    x: (n_src, H, W, nicg) float32 images, nicg 1 or 2; labels: None, class codes (n_src, H, W) or (n_src, H, W, 1)
    (uint8, or integral values in [0, 255] of another dtype), or one-hot (n_src, H, W, C) float32; NumPy arrays or
    tensors (a tensor on the device is read where it is).  params: (n, 8) float32 rows of `affine_params`, one per
    output sample, or a single row for all of them.  index: the n source slices, output sample i is made from
    x[index[i]] (None: from x[i]); a host index outside [0, n_src) is a ValueError, a device index is not read back
    (an entry outside the range gives a sample of the fill values).  Images are sampled bilinearly, labels by the
    nearest pixel, so a label row is always a copy of a source row.  border 'edge' repeats the edge pixels; 'constant'
    puts x_fill and label_fill outside the image (one-hot: the row with 1.0 at label_fill, all zeros when
    label_fill < 0 -- the ignored pixel of compile(class_weight=...)).  Returns new device tensors (x_out, labels_out)
    of n samples; labels_out is None without labels.  Every value is bit for bit what the float32 formula of
    include/depgan.h gives in NumPy (tests/augment_ref.py).
    fields: None, or control grids (n, 3, gh, gw) float32, one set per output sample, or (3, gh, gw) for all of them,
    gh and gw in [4, AUG_MAX_GRID]; a NumPy array or a tensor.  The same single launch (depgan_data_augment_fields)
    then evaluates each plane as a cubic B-spline over the image and adds plane 0 to the source row and plane 1 to the
    source column of every output pixel (an elastic deformation, in source pixels) and multiplies the interpolated
    intensity by 1 + plane 2 before the gain (a bias field); labels follow the displacement and do not see the bias.
    All-zero grids give the bits of fields=None; tests/elastic_ref.py is the NumPy restatement.  return_fields=True
    (only with fields) returns (x_out, labels_out, dense) with dense (n, H, W, 3) float32, the three planes at every
    output pixel."""
    import torch
    lib = _lib.load()
    if border not in _BORDERS:
        raise ValueError("augment: border must be 'edge' or 'constant', got %r" % (border,))
    shape = tuple(int(d) for d in (x.shape if hasattr(x, "shape") else np.shape(x)))
    if len(shape) != 4 or min(shape) < 1 or shape[3] not in (1, 2):
        raise ValueError("augment: images must be (n_src, H, W, 1 or 2), got shape %s" % (shape,))
    n_src, H, W, nicg = shape
    if fields is None:
        if return_fields:
            raise ValueError("augment: return_fields needs fields")
    else:
        count = int(index.numel()) if isinstance(index, torch.Tensor) else int(np.size(index))
        gh, gw = _aug_fields_shape(fields, n_src if index is None else count)
    if isinstance(x, torch.Tensor):
        dev = x.device if device is None and x.is_cuda else torch.device(device or "cuda:0")
        xs = x.to(device=dev, dtype=torch.float32).contiguous()
    else:
        dev = torch.device(device if device is not None else "cuda:0")
        xs = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32)).to(dev)
    ls, kind, Cc, lshape = _aug_labels(labels, n_src, H, W, dev)
    if isinstance(label_fill, bool) or not isinstance(label_fill, (int, np.integer)):
        raise ValueError("augment: label_fill must be an integer, got %r" % (label_fill,))
    if (kind == 1 and not 0 <= label_fill <= 255) or (kind == 2 and label_fill >= Cc):
        raise ValueError("augment: label_fill = %d does not fit the labels" % label_fill)
    idx = None
    if index is not None:
        if isinstance(index, torch.Tensor) and index.is_cuda:
            idx = index.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        else:
            h = np.asarray(index.numpy() if isinstance(index, torch.Tensor) else index)
            if h.ndim != 1 or h.dtype.kind not in "iu":
                raise ValueError("augment: index must be a 1-D integer array")
            if h.size and (int(h.min()) < 0 or int(h.max()) >= n_src):
                raise ValueError("augment: index outside [0, %d)" % n_src)
            idx = torch.from_numpy(np.ascontiguousarray(h, dtype=np.int64)).to(dev)
    n = n_src if idx is None else int(idx.numel())
    if n < 1:
        raise ValueError("augment: no output samples")
    if params is None:
        params = affine_params(H, W)
    if isinstance(params, torch.Tensor):
        ps = params.to(device=dev, dtype=torch.float32)
    else:
        ps = torch.from_numpy(np.ascontiguousarray(np.asarray(params), dtype=np.float32)).to(dev)
    if tuple(ps.shape) == (AUG_NPARAM,):
        ps = ps.reshape(1, AUG_NPARAM).expand(n, AUG_NPARAM)
    if tuple(ps.shape) != (n, AUG_NPARAM):
        raise ValueError("augment: params must be (%d, %d) or (%d,), got shape %s" % (n, AUG_NPARAM, AUG_NPARAM,
                                                                                   tuple(ps.shape)))
    ps = ps.contiguous()
    x_out = torch.empty((n, H, W, nicg), dtype=torch.float32, device=dev)
    l_out = None if kind == 0 else torch.empty((n,) + tuple(lshape), dtype=ls.dtype, device=dev)
    if fields is None:
        _lib.check(lib.depgan_data_augment(_p(xs), nicg, _p(ls), kind, Cc, _p(idx), n_src, _p(ps), n, H, W,
                                           _BORDERS[border], float(x_fill), int(label_fill), _p(x_out), _p(l_out),
                                           _stream(dev, stream)), "depgan_data_augment")
        return x_out, l_out
    if isinstance(fields, torch.Tensor):
        fs = fields.to(device=dev, dtype=torch.float32)
    else:
        fs = torch.from_numpy(np.ascontiguousarray(np.asarray(fields), dtype=np.float32)).to(dev)
    fs = (fs.expand(n, 3, gh, gw) if fs.dim() == 3 else fs).contiguous()
    dense = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev) if return_fields else None
    _lib.check(lib.depgan_data_augment_fields(_p(xs), nicg, _p(ls), kind, Cc, _p(idx), n_src, _p(ps), _p(fs), gh, gw, n,
                                              H, W, _BORDERS[border], float(x_fill), int(label_fill), _p(x_out),
                                              _p(l_out), _p(dense), _stream(dev, stream)),
               "depgan_data_augment_fields")
    return (x_out, l_out, dense) if return_fields else (x_out, l_out)


class Augmenter:
    """Random affine and intensity augmentation of training batches, drawn per sample and applied by `augment`.
    rotate: degrees, uniform in +-rotate.  scale: (low, high), uniform.  shift: pixels, uniform in +-shift on both axes.
    flip_lr / flip_ud: mirror with probability 1/2.  gain, offset: (low, high), uniform; out = gain*v + offset.
    border, x_fill, label_fill: as in `augment`; with compile(ignore_label=k), border='constant' and label_fill=k keep
    the pixels a warp brings in from outside the image out of the loss.  seed: of the instance's own
    np.random.default_rng -- np.random is never touched, so the shuffle of fit is what it is without augmentation.
    elastic: an elastic deformation; the control displacements of both axes are uniform in +-elastic source pixels.
    bias: a smooth multiplicative intensity field (the bias field of an MR coil), out = gain*(v*(1 + b)) + offset; the
    control values are uniform in +-bias, 0 <= bias < 1, and the spline of them stays inside +-bias (its weights are
    non-negative and sum to 1), so 1 + b stays positive.  field_grid: (gh, gw) control points per axis, 4 to
    AUG_MAX_GRID, evaluated as a cubic B-spline over the image (`augment`, fields).  The grids are drawn only when one
    of the two is open, then all three planes, and from a generator of their own spawned from the seed: the parameter
    rows of a seed are the same with the fields open or closed, and without these arguments nothing changes in any bit
    or draw.  Displacements above about half a control-cell width, (H-1)/(gh-3) pixels, can fold the map (two output
    pixels showing the same source pixel in reversed order); they are not refused.
    GeneratorModel.fit(..., augment=Augmenter(...)) uses it; a hand-written loop calls it: xb, lb = aug(x, labels, idx)."""

    def __init__(self, rotate=0.0, scale=(1.0, 1.0), shift=0.0, flip_lr=False, flip_ud=False, gain=(1.0, 1.0),
                 offset=(0.0, 0.0), border="edge", x_fill=0.0, label_fill=0, seed=None, elastic=0.0, bias=0.0,
                 field_grid=(7, 7)):
        def pair(v, name, positive=False):
            lo, hi = (float(v[0]), float(v[1])) if np.ndim(v) == 1 and len(v) == 2 else (np.nan, np.nan)
            if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi) or (positive and lo <= 0):
                raise ValueError("Augmenter: %s must be a finite (low, high) pair%s, got %r"
                                 % (name, " above 0" if positive else "", v))
            return lo, hi
        self.rotate, self.shift = float(rotate), float(shift)
        if not (np.isfinite(self.rotate) and self.rotate >= 0 and np.isfinite(self.shift) and self.shift >= 0):
            raise ValueError("Augmenter: rotate and shift must be finite and >= 0")
        self.scale, self.gain, self.offset = pair(scale, "scale", True), pair(gain, "gain"), pair(offset, "offset")
        self.flip_lr, self.flip_ud = bool(flip_lr), bool(flip_ud)
        if border not in _BORDERS:
            raise ValueError("Augmenter: border must be 'edge' or 'constant', got %r" % (border,))
        self.border, self.x_fill, self.label_fill = border, float(x_fill), label_fill
        self.rng = np.random.default_rng(seed)
        self.elastic, self.bias = float(elastic), float(bias)
        if not (np.isfinite(self.elastic) and self.elastic >= 0 and 0 <= self.bias < 1):
            raise ValueError("Augmenter: elastic must be finite and >= 0 and bias in [0, 1), got %r and %r"
                             % (elastic, bias))
        grid = tuple(field_grid) if np.ndim(field_grid) == 1 and len(field_grid) == 2 else ()
        if not (grid and all(isinstance(g, (int, np.integer)) and not isinstance(g, bool) and 4 <= g <= AUG_MAX_GRID
                             for g in grid)):
            raise ValueError("Augmenter: field_grid must be two integers in [4, %d], got %r"
                             % (AUG_MAX_GRID, field_grid))
        self.field_grid = (int(grid[0]), int(grid[1]))
        self.field_rng = np.random.default_rng(np.random.SeedSequence(seed).spawn(1)[0])

    @property
    def fields_open(self):
        """True when the elastic or the bias range is open: every call then draws control grids."""
        return self.elastic > 0 or self.bias > 0

    @property
    def identity(self):
        """True when no range can move anything: every draw is the identity row and no field is drawn."""
        return (self.rotate == 0 and self.shift == 0 and self.scale == (1.0, 1.0) and self.gain == (1.0, 1.0)
                and self.offset == (0.0, 0.0) and not self.flip_lr and not self.flip_ud and not self.fields_open)

    def draw(self, n, H, W):
        """(n, 8) float32 parameter rows for n samples of H x W pixels.  Every quantity is drawn for every call, in a
        fixed order, so the stream of a seed does not depend on which ranges are open."""
        n = int(n)
        r = self.rng
        rot = r.uniform(-self.rotate, self.rotate, n)
        sc = r.uniform(self.scale[0], self.scale[1], n)
        dy, dx = r.uniform(-self.shift, self.shift, n), r.uniform(-self.shift, self.shift, n)
        lr, ud = r.random(n) < 0.5, r.random(n) < 0.5
        g = r.uniform(self.gain[0], self.gain[1], n)
        o = r.uniform(self.offset[0], self.offset[1], n)
        return _affine_rows(int(H), int(W), rot, sc, dy, dx, lr & self.flip_lr, ud & self.flip_ud, g, o)

    def draw_fields(self, n):
        """(n, 3, gh, gw) float32 control grids for n samples: the row and the column displacements, uniform in
        +-elastic, and the bias, uniform in +-bias, from the field generator (the parameter rows' stream is not
        touched)."""
        gh, gw = self.field_grid
        r = self.field_rng
        d = r.uniform(-self.elastic, self.elastic, (int(n), 2, gh, gw))
        b = r.uniform(-self.bias, self.bias, (int(n), 1, gh, gw))
        return np.concatenate([d, b], 1).astype(np.float32)

    def __call__(self, x, labels=None, index=None, device=None):
        """Draws one row per output sample -- and, with elastic or bias open, one set of control grids -- and applies
        them in one launch: (x_out, labels_out) device tensors, as `augment`."""
        n = int(x.shape[0]) if index is None else int(len(index))
        rows = self.draw(n, int(x.shape[1]), int(x.shape[2]))
        return augment(x, labels, rows, index, self.border, self.x_fill, self.label_fill, device,
                       fields=self.draw_fields(n) if self.fields_open else None)


def data_prep_save(image_data):
    """GT:121-127: (Z, X, Y, 1) network output -> the orientation the reference saves to NIfTI."""
    a = np.squeeze(np.asarray(image_data))
    a = np.swapaxes(a, 0, 2)
    a = np.rot90(a)
    return a[::-1, ...]


def data_prep(image_data):
    """GT:106-118: an (X, Y, Z) volume as loaded -> the (Z, X, Y, 1) float32 slices the networks work on.  Pure NumPy;
    the device route is prep_subject / mask_slices, which leave their slices in this order."""
    a = np.asarray(image_data)
    if a.ndim != 3:
        raise ValueError("data_prep: expected a 3-D volume, got shape %s" % (a.shape,))
    return np.array([a[:, :, z] for z in range(a.shape[2])], dtype="float32")[..., None]


def prepared_spacing(pixdim):
    """Voxel spacing of the prepared slices.  pixdim: the pixdim[1:4] of a loaded NIfTI (nifti.load(path).header
    ["pixdim"][1:4]), the spacing along the file's three axes.  Returns (sz, sy, sx) as floats, the spacing along the
    axes of the (n, H, W) slices data_prep leaves -- what evaluate.surface_distances takes as `spacing`.  The order is
    read off data_prep itself: a volume whose voxels hold their own file index goes through it, and the file axis
    whose index changes along a prepared axis is that axis' source.  Pure NumPy."""
    p = np.asarray(pixdim, np.float64).reshape(-1)
    if p.size != 3 or not np.isfinite(p).all() or not (p > 0).all():
        raise ValueError("prepared_spacing: pixdim must hold three finite positive spacings, got %r" % (pixdim,))
    index = np.indices((2, 3, 4))                       # index[a][i, j, k] = the voxel's index along file axis a
    moved = [data_prep(index[a])[..., 0] for a in range(3)]
    out = []
    for axis in range(3):                               # prepared axis: which file index changes along it?
        src = [a for a in range(3) if np.diff(moved[a], axis=axis).any()]
        if len(src) != 1:
            raise AssertionError("data_prep no longer permutes the axes of its volume")
        out.append(float(p[src[0]]))
    return tuple(out)
