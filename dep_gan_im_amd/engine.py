"""Engine: one libdepgan context (generator + two critics + optimiser state) on one GPU.

PyTorch-ROCm is used for device buffers of the *inputs* and for the stream
handle only; every FLOP runs in the hand-written HIP kernels behind the C ABI
(include/depgan.h).  Mirrors the slice of the Keras API the reference touches
(GT:513-598): see models.py / trainers.py for the user-facing names.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict

import numpy as np

from . import _lib
from ._lib import (ARENA_ADAM_M, ARENA_ADAM_V, ARENA_GRADS, ARENA_NONTRAINABLE, ARENA_PARAMS, D2H, H2D, NET_D_DEM,
                   NET_D_Y2, NET_G, Config, check, load)

NET_IDS = {"G": NET_G, "D_y2": NET_D_Y2, "D_dem": NET_D_DEM}
_DICE_FORMS = {"flat": _lib._K["DEPGAN_DICE_FLAT"], "class": _lib._K["DEPGAN_DICE_CLASS"]}


def _torch():
    import torch
    return torch


def require_class_indices(labels):
    """ValueError unless `labels` (NumPy array or tensor) has an integer dtype or is float with integral values: what
    the sparse loss accepts.  Reads the array only; no library call."""
    torch = _torch()
    tens = isinstance(labels, torch.Tensor)
    a = labels if tens else np.asarray(labels)
    if (a.is_floating_point() if tens else a.dtype.kind == "f"):
        if not bool((a == (torch if tens else np).trunc(a)).all()):                    # NaN and inf fail here too
            raise ValueError("sparse labels must hold integral values (class indices)")
    elif not tens and a.dtype.kind not in "iub":
        raise ValueError("sparse labels must be an integer or float array, got dtype %s" % a.dtype)
    return a


class Engine:
    def __init__(self, batch, height=256, width=256, nicg=1, first_fm=32, im_thresh=0.5, delta=10.0, lrD=1e-4,
                 lrG=1e-4, beta1=0.0, beta2=0.9, adam_eps=1e-7, device=None, nc_out=1, bf16_weights=False,
                 bf16_mfma=False, f32_split=0):
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.DepganError("dep_gan_im_amd needs a ROCm GPU (MI355X): torch.cuda.is_available() is False")
        self.lib = load()
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        torch.cuda.set_device(self.device)
        if not f32_split and not (bf16_weights or bf16_mfma) and nc_out == 1:
            # DEPGAN_F32_SPLIT=6 (or 3) turns the opt-in split-product convolutions on for contexts that do not ask for
            # anything else: lets the whole parity suite / bench run on them unchanged
            f32_split = int(os.environ.get("DEPGAN_F32_SPLIT", "0") or 0)
        self.f32_split = int(f32_split)
        self.cfg = Config(batch=batch, height=height, width=width, nicg=nicg, first_fm=first_fm, im_thresh=im_thresh,
                          delta=delta, lrD=lrD, lrG=lrG, beta1=beta1, beta2=beta2, adam_eps=adam_eps, nc_out=nc_out,
                          bf16_weights=1 if (bf16_weights or bf16_mfma) else 0, bf16_mfma=1 if bf16_mfma else 0,
                          f32_split=int(f32_split))
        self.batch, self.height, self.width, self.nicg, self.nc_out = batch, height, width, nicg, nc_out
        h = C.c_void_p()
        check(self.lib.depgan_create(C.byref(self.cfg), C.byref(h)), "depgan_create")
        self.h = h
        self._use_current_stream()
        self._tables = {}
        self._ignore_label = None     # set_loss_weights: the label value that takes a pixel out of the loss
        self._ar_cb = None       # keeps the ctypes callback of set_allreduce alive
        self.world = 1
        self._forward_storage = "float32"

    # ---- plumbing ----
    def _use_current_stream(self):
        torch = _torch()
        s = torch.cuda.current_stream(self.device).cuda_stream
        check(self.lib.depgan_set_stream(self.h, C.c_void_p(s)), "depgan_set_stream")

    def close(self):
        if getattr(self, "h", None):
            self.lib.depgan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dev(self, a, shape=None):
        """float32 contiguous CUDA tensor for a numpy array / tensor (cast like Keras' feed)."""
        torch = _torch()
        if isinstance(a, torch.Tensor):
            t = a.to(device=self.device, dtype=torch.float32).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float32)).to(self.device)
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError("expected input of shape %s, got %s" % (tuple(shape), tuple(t.shape)))
        return t

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr())

    # ---- parameter tables ----
    def param_table(self, net):
        nid = NET_IDS[net]
        if nid in self._tables:
            return self._tables[nid]
        n = self.lib.depgan_param_count(self.h, nid)
        out = []
        name = C.create_string_buffer(128)
        shape = (C.c_int * 4)()
        ndim, off, tr = C.c_int(), C.c_long(), C.c_int()
        for i in range(n):
            check(self.lib.depgan_param_info(self.h, nid, i, name, 128, shape, C.byref(ndim), C.byref(off),
                                             C.byref(tr)), "depgan_param_info")
            out.append((name.value.decode(), tuple(shape[:ndim.value]), off.value, bool(tr.value)))
        self._tables[nid] = out
        return out

    def _arena_np(self, net, arena):
        nid = NET_IDS[net]
        n = self.lib.depgan_arena_floats(self.h, nid, arena)
        buf = np.empty(max(n, 1), np.float32)
        ptr = self.lib.depgan_arena_ptr(self.h, nid, arena)
        _torch().cuda.synchronize(self.device)
        if n:
            _lib.memcpy(buf.ctypes.data, ptr, n * 4, D2H)
        return buf

    def _read(self, net, trainable_arena):
        tr = self._arena_np(net, trainable_arena)
        out = OrderedDict()
        nt = None
        for name, shape, off, trainable in self.param_table(net):
            size = int(np.prod(shape))
            if trainable:
                out[name] = tr[off:off + size].reshape(shape).copy()
            elif trainable_arena == ARENA_PARAMS:
                if nt is None:
                    nt = self._arena_np(net, ARENA_NONTRAINABLE)
                out[name] = nt[off:off + size].reshape(shape).copy()
        return out

    def get_weights(self, net):
        """OrderedDict name -> ndarray (Keras layouts), incl. BN moving statistics."""
        return self._read(net, ARENA_PARAMS)

    def get_grads(self, net):
        return self._read(net, ARENA_GRADS)

    def get_adam_state(self, net):
        return self._read(net, ARENA_ADAM_M), self._read(net, ARENA_ADAM_V)

    def set_weights(self, net, weights):
        nid = NET_IDS[net]
        tr = self._arena_np(net, ARENA_PARAMS)
        nt = self._arena_np(net, ARENA_NONTRAINABLE)
        for name, shape, off, trainable in self.param_table(net):
            if name not in weights:
                continue
            v = np.asarray(weights[name], np.float32)
            if tuple(v.shape) != tuple(shape):
                raise ValueError("weight %s: expected shape %s, got %s" % (name, shape, v.shape))
            (tr if trainable else nt)[off:off + v.size] = v.reshape(-1)
        unknown = set(weights) - {p[0] for p in self.param_table(net)}
        if unknown:
            raise ValueError("unknown weight names for %s: %s" % (net, sorted(unknown)[:5]))
        for arena, buf in ((ARENA_PARAMS, tr), (ARENA_NONTRAINABLE, nt)):
            n = self.lib.depgan_arena_floats(self.h, nid, arena)
            if n:
                _lib.memcpy(self.lib.depgan_arena_ptr(self.h, nid, arena), buf.ctypes.data, n * 4, H2D)
        self._use_current_stream()
        check(self.lib.depgan_weights_changed(self.h, nid), "depgan_weights_changed")

    def arena(self, net, arena):
        """(device pointer, number of floats) of one of a network's flat arenas (weights broadcast, checkpoints)."""
        nid = NET_IDS[net]
        return self.lib.depgan_arena_ptr(self.h, nid, arena), self.lib.depgan_arena_floats(self.h, nid, arena)

    def weights_changed(self, net):
        """Call after writing into a PARAMS / NONTRAINABLE arena from outside: rebuilds the derived state."""
        self._use_current_stream()
        check(self.lib.depgan_weights_changed(self.h, NET_IDS[net]), "depgan_weights_changed")

    def set_arena(self, net, arena, values):
        """Overwrites one flat arena from a float32 array of exactly its length (optimiser state on resume)."""
        ptr, n = self.arena(net, arena)
        v = np.ascontiguousarray(values, np.float32).reshape(-1)
        if v.size != n:
            raise ValueError("arena of %s has %d floats, got %d" % (net, n, v.size))
        _torch().cuda.synchronize(self.device)
        if n:
            _lib.memcpy(ptr, v.ctypes.data, n * 4, H2D)

    def get_arena(self, net, arena):
        return self._arena_np(net, arena)[:self.lib.depgan_arena_floats(self.h, NET_IDS[net], arena)].copy()

    def adam_step(self, net, value=None):
        """Adam `iterations` of a network's optimiser; with `value` sets it (resume)."""
        if value is not None:
            check(self.lib.depgan_set_adam_step(self.h, NET_IDS[net], int(value)), "depgan_set_adam_step")
        return int(self.lib.depgan_get_adam_step(self.h, NET_IDS[net]))

    def set_allreduce(self, fn, world):
        """Registers the data-parallel hook: fn(dev_ptr:int, n:int, stream:int) must ENQUEUE an in-place summing
        all-reduce of n device floats on the stream (dist.DataParallel.attach does this).  fn=None removes it."""
        if fn is None:
            self._ar_cb, self.world = None, 1
            check(self.lib.depgan_set_allreduce(self.h, _lib.ALLREDUCE_FN(), None, 1), "depgan_set_allreduce")
            return
        self._ar_err = None

        def _cb(user, ptr, n, stream):
            try:
                fn(int(ptr), int(n), int(stream or 0))
                return 0
            except BaseException as e:   # never let an exception unwind through the C frames
                self._ar_err = e
                return 1

        self._ar_cb = _lib.ALLREDUCE_FN(_cb)
        self.world = int(world)
        check(self.lib.depgan_set_allreduce(self.h, self._ar_cb, None, int(world)), "depgan_set_allreduce")

    # ---- direct RCCL binding (include/depgan.h): the library calls ncclAllReduce itself ----
    def rccl_unique_id(self):
        """The 128-byte ncclUniqueId (rank 0 creates it; the host hands it to every rank)."""
        buf = C.create_string_buffer(_lib.RCCL_ID_BYTES)
        check(self.lib.depgan_rccl_unique_id(buf), "depgan_rccl_unique_id")
        return buf.raw

    def rccl_init(self, uid, rank, world):
        """Collective: ncclCommInitRank on this engine's device.  Every update then all-reduces inside the library."""
        if len(uid) != _lib.RCCL_ID_BYTES:
            raise ValueError("an ncclUniqueId is %d bytes" % _lib.RCCL_ID_BYTES)
        _torch().cuda.set_device(self.device)
        self._ar_cb = None
        check(self.lib.depgan_rccl_init(self.h, C.c_char_p(uid), int(rank), int(world)), "depgan_rccl_init")
        self.world = int(world)

    def rccl_broadcast(self, ptr, n, root=0):
        self._use_current_stream()
        check(self.lib.depgan_rccl_broadcast(self.h, C.c_void_p(ptr), int(n), int(root)), "depgan_rccl_broadcast")

    def rccl_info(self):
        """(nranks, rank) as RCCL reports them, collectives issued by this engine."""
        n, r, k = C.c_int(), C.c_int(), C.c_long()
        check(self.lib.depgan_rccl_info(self.h, C.byref(n), C.byref(r), C.byref(k)), "depgan_rccl_info")
        return n.value, r.value, k.value

    def rccl_shutdown(self):
        check(self.lib.depgan_rccl_shutdown(self.h), "depgan_rccl_shutdown")
        self.world = 1 if self._ar_cb is None else self.world

    def _check(self, rc, what):
        err = getattr(self, "_ar_err", None)
        if err is not None:
            self._ar_err = None
            raise err
        check(rc, what)

    def grad_arena(self, net):
        """(device pointer, number of floats) of a network's flat gradient arena (for the RCCL all-reduce)."""
        return self.arena(net, ARENA_GRADS)

    # ---- the inference context ----
    @property
    def inference_only(self):
        """True for an engine created with bf16_mfma=True and nc_out>=2: the DEP-UResNet in learning phase 0 on the bf16
        matrix pipe.  g_forward (either storage) and the weight surface work; the context holds no critics, gradients or
        optimiser scratch, and every training helper raises ValueError without calling the library."""
        return bool(self.cfg.bf16_mfma and self.cfg.nc_out >= 2)

    def _need_trainable(self, what):
        if self.inference_only:
            raise ValueError("%s: this engine is an inference context (bf16_mfma=True, nc_out>=2), predict-only; train "
                             "on an Engine(..., nc_out=%d) and copy the weights over" % (what, self.cfg.nc_out))

    # ---- forward ----
    @property
    def forward_storage(self):
        """How g_forward stores the activations between the generator's layers: "float32" (default) or "bfloat16"
        (bf16_mfma engines only, the nc_out>=2 inference context included: BASELINE config 4 with bf16 activations,
        depgan_g_forward_bf16s)."""
        return getattr(self, "_forward_storage", "float32")

    @forward_storage.setter
    def forward_storage(self, value):
        self._forward_storage = self._check_storage(value)

    def _check_storage(self, storage):
        if storage not in ("float32", "bfloat16"):
            raise ValueError("forward storage must be 'float32' or 'bfloat16', got %r" % (storage,))
        if storage == "bfloat16" and not (self.cfg.bf16_mfma and 0 <= self.cfg.nc_out <= _lib.MAX_HEAD_CLASSES):
            raise ValueError("bfloat16 activation storage needs an engine created with bf16_mfma=True (nc_out=1, or "
                             "nc_out>=2 for the predict-only inference context); this one has bf16_mfma=%d, nc_out=%d"
                             % (self.cfg.bf16_mfma, self.cfg.nc_out))
        return storage

    def _set_mode(self, attr, entry, value):
        """Tail of the three mode setters: hands an already validated "float32" / "bfloat16" to the library's setter
        `entry` (0 / 1) and remembers it."""
        if getattr(self, "h", None):
            check(getattr(self.lib, entry)(self.h, 1 if value == "bfloat16" else 0), entry)
        setattr(self, "_" + attr, value)

    @property
    def forward_only_storage(self):
        """How the FORWARD-ONLY generator passes of the training closures (the one inside every critic update and
        netG_no_update / the best-of-k evaluations) store their activations: "float32" (default) or "bfloat16"
        (bf16_mfma engines only; depgan_set_fwd_only_storage).  The generator update keeps float32 storage unless
        g_update_storage says otherwise; while it does, netG_no_update(z) and netG_train(z) no longer report identical
        scalars for the same noise.
        Independent of forward_storage, which governs g_forward / predict.  Every rank of a data-parallel job must
        use the same value."""
        return getattr(self, "_forward_only_storage", "float32")

    @forward_only_storage.setter
    def forward_only_storage(self, value):
        value = self._check_storage(value)
        self._need_trainable("forward_only_storage")
        self._set_mode("forward_only_storage", "depgan_set_fwd_only_storage", value)

    @property
    def g_update_storage(self):
        """How the generator UPDATE (g_grads, g_step, the update closing gen_iteration) stores the generator's activations:
        "float32" (default) or "bfloat16" (bf16_mfma engines only; depgan_set_g_update_storage).  With "bfloat16" the
        update runs the forward of the bf16-storage passes (same output bits) and a backward that reads the bf16 buffers;
        gradients stay float32.  Independent of forward_only_storage; with both on netG_no_update(z) and netG_train(z)
        report identical scalars again.  Every rank of a data-parallel job must use the same value."""
        return getattr(self, "_g_update_storage", "float32")

    @g_update_storage.setter
    def g_update_storage(self, value):
        value = self._check_storage(value)
        self._need_trainable("g_update_storage")
        self._set_mode("g_update_storage", "depgan_set_g_update_storage", value)

    @property
    def critic16_pipe(self):
        """The matrix pipe of the critics' 16-channel 5x5 launches (dis_0b forward, its u-forward and backward-data,
        dis_1a backward-data): "float32" (default: the fp32 MFMA kernel, as every bf16_mfma engine ran them before) or
        "bfloat16" (bf16_mfma engines only; depgan_set_critic16_pipe): both operands rounded to bf16 while staged, fp32
        accumulation, like every other convolution of such an engine.  Every rank of a data-parallel job must use the
        same value."""
        return getattr(self, "_critic16_pipe", "float32")

    @critic16_pipe.setter
    def critic16_pipe(self, value):
        if value not in ("float32", "bfloat16"):
            raise ValueError("critic16_pipe must be 'float32' or 'bfloat16', got %r" % (value,))
        self._need_trainable("critic16_pipe")
        if value == "bfloat16" and not (self.cfg.bf16_mfma and self.cfg.nc_out in (0, 1)):
            raise ValueError("critic16_pipe='bfloat16' needs an engine created with bf16_mfma=True (and nc_out=1); "
                             "this one has bf16_mfma=%d, nc_out=%d" % (self.cfg.bf16_mfma, self.cfg.nc_out))
        self._set_mode("critic16_pipe", "depgan_set_critic16_pipe", value)

    def g_forward(self, x, z, storage=None):
        """Model.predict of the generator.  storage: None = self.forward_storage; "bfloat16" keeps every inter-layer
        activation as bf16 (forward only; the input and the output stay float32)."""
        storage = self.forward_storage if storage is None else self._check_storage(storage)
        torch = _torch()
        x = self._dev(x)
        z = self._dev(z).reshape(x.shape[0], -1)
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.height, self.width, self.nicg):
            raise ValueError("generator input must be (N,%d,%d,%d), got %s" % (self.height, self.width, self.nicg,
                                                                                tuple(x.shape)))
        if z.shape[1] != 32:
            raise ValueError("noise input must be (N,32,1)")
        n = x.shape[0]
        out = torch.empty((n, self.height, self.width, self.nc_out), dtype=torch.float32, device=self.device)
        self._use_current_stream()
        fn, what = ((self.lib.depgan_g_forward_bf16s, "depgan_g_forward_bf16s") if storage == "bfloat16"
                    else (self.lib.depgan_g_forward, "depgan_g_forward"))
        for i in range(0, n, self.batch):
            m = min(self.batch, n - i)
            check(fn(self.h, self._p(x[i:i + m]), self._p(z[i:i + m]), self._p(out[i:i + m]), m), what)
        return out

    def d_forward(self, net, img):
        self._need_trainable("d_forward")
        torch = _torch()
        img = self._dev(img)
        if img.dim() != 4 or tuple(img.shape[1:]) != (self.height, self.width, 1):
            raise ValueError("critic input must be (N,%d,%d,1), got %s" % (self.height, self.width, tuple(img.shape)))
        n = img.shape[0]
        out = torch.empty((n, 1), dtype=torch.float32, device=self.device)
        self._use_current_stream()
        cap = 3 * self.batch
        for i in range(0, n, cap):
            m = min(cap, n - i)
            check(self.lib.depgan_d_forward(self.h, NET_IDS[net], self._p(img[i:i + m]), self._p(out[i:i + m]), m),
                  "depgan_d_forward")
        return out

    # ---- closures ----
    def _xy(self, x, y2):
        """One batch of inputs and targets on the device: (B, H, W, nicg) and (B, H, W, 1)."""
        B = self.batch
        return self._dev(x, (B, self.height, self.width, self.nicg)), self._dev(y2, (B, self.height, self.width, 1))

    def _noises(self, zs):
        """k noises for one batch, (k, B, 32[, 1]) or a list of k (B, 32[, 1]), as a contiguous (k, B*32) device
        tensor; returns it and k."""
        B = self.batch
        if isinstance(zs, (list, tuple)):
            zs = _torch().stack([self._dev(z).reshape(B, 32) for z in zs])
        else:
            zs = self._dev(zs)
        k = int(zs.shape[0])
        zs = zs.reshape(k, -1).contiguous()
        if zs.shape[1] != B * 32:
            raise ValueError("noises must be (k,%d,32,1)" % B)
        return zs, k

    def _batch_inputs(self, x, y2, z, ep=None):
        B = self.batch
        x, y2 = self._xy(x, y2)
        z = self._dev(z).reshape(-1)
        if z.numel() != B * 32:
            raise ValueError("noise must be (%d,32,1)" % B)
        if ep is not None:
            ep = self._dev(ep).reshape(-1)
            if ep.numel() != B:
                raise ValueError("ep must be (%d,1,1,1)" % B)
        return x, y2, z, ep

    def critic(self, which, y2, x, z, ep, update=True):
        self._need_trainable("critic")
        x, y2, z, ep = self._batch_inputs(x, y2, z, ep)
        out = (C.c_float * 2)()
        self._use_current_stream()
        fn = self.lib.depgan_critic_step if update else self.lib.depgan_critic_grads
        self._check(fn(self.h, NET_IDS[which], self._p(y2), self._p(x), self._p(z), self._p(ep), out), "critic step")
        return [float(out[0]), float(out[1])]

    def generator(self, x, y2, z, mode="eval"):
        self._need_trainable("generator")
        x, y2, z, _ = self._batch_inputs(x, y2, z)
        out = (C.c_float * 6)()
        self._use_current_stream()
        fn = {"eval": self.lib.depgan_g_eval, "grads": self.lib.depgan_g_grads, "step": self.lib.depgan_g_step}[mode]
        self._check(fn(self.h, self._p(x), self._p(y2), self._p(z), out), "generator " + mode)
        return [float(v) for v in out]

    def generator_eval_multi(self, x, y2, zs):
        """k forward-only loss evaluations on one batch with k noises (GT:868-877), one host sync.
        zs: (k, B, 32, 1) array / tensor or a list of k (B,32,1) noises.  Returns (k x 6 outputs, k x 8 sums)."""
        self._need_trainable("generator_eval_multi")
        x, y2 = self._xy(x, y2)
        zs, k = self._noises(zs)
        out, sums = (C.c_float * (6 * k))(), (C.c_float * (8 * k))()
        self._use_current_stream()
        self._check(self.lib.depgan_g_eval_multi(self.h, self._p(x), self._p(y2), self._p(zs), k, out, sums),
                    "depgan_g_eval_multi")
        return ([[float(out[6 * i + j]) for j in range(6)] for i in range(k)],
                [[float(sums[8 * i + j]) for j in range(8)] for i in range(k)])

    def gen_iteration(self, y2_loop, dem_loop, gen, batch_stride=None):
        """One generator iteration of the reference schedule (GT:791-878) with ONE host synchronisation
        (depgan_gen_iteration).

        y2_loop / dem_loop: (x, y2, z, ep, n) -- n consecutive batches: x (n*stride.., H, W, nicg) and y2 device
        tensors whose batch j starts at sample j*batch_stride, z (n, B, 32[,1]), ep (n, B[,1,1,1]); n may be 0.
        gen: (x, y2, zs) -- one batch and its k noises (k, B, 32[,1]).
        Returns (critic_y2 outs n x 2, critic_dem outs n x 2, eval outs k x 6, train out 6, best index)."""
        self._need_trainable("gen_iteration")
        B = self.batch
        stride = B if batch_stride is None else int(batch_stride)

        def loop(t):
            x, y2, z, ep, n = t
            n = int(n)
            if n == 0:
                return None, None, None, None, 0
            x, y2 = self._dev(x), self._dev(y2)
            need = (n - 1) * stride + B
            if x.shape[0] < need or y2.shape[0] < need or tuple(x.shape[1:]) != (self.height, self.width, self.nicg) \
                    or tuple(y2.shape[1:]) != (self.height, self.width, 1):
                raise ValueError("critic loop: need %d samples of (%d,%d,%d) / (%d,%d,1), got %s / %s"
                                 % (need, self.height, self.width, self.nicg, self.height, self.width,
                                    tuple(x.shape), tuple(y2.shape)))
            z, ep = self._dev(z).reshape(-1), self._dev(ep).reshape(-1)
            if z.numel() != n * B * 32 or ep.numel() != n * B:
                raise ValueError("critic loop: noise must be (%d,%d,32,1) and ep (%d,%d,1,1,1)" % (n, B, n, B))
            return x, y2, z, ep, n

        xa, ya, za, ea, na = loop(y2_loop)
        xb, yb, zb, eb, nb = loop(dem_loop)
        xg, yg, zs = gen
        xg, yg = self._xy(xg, yg)
        zs, k = self._noises(zs)
        if na + nb > _lib.MAX_CRITIC_STEPS or not 1 <= k <= _lib.MAX_MULTI:
            raise ValueError("gen_iteration: at most %d critic updates and %d noises" % (_lib.MAX_CRITIC_STEPS,
                                                                                       _lib.MAX_MULTI))
        nout = 2 * (na + nb) + 6 * k + 6
        out, best = (C.c_float * nout)(), C.c_int(-1)
        p = lambda t: self._p(t) if t is not None else C.c_void_p(0)   # noqa: E731
        self._use_current_stream()
        self._check(self.lib.depgan_gen_iteration(self.h, p(xa), p(ya), p(za), p(ea), na, p(xb), p(yb), p(zb), p(eb),
                                                  nb, stride, self._p(xg), self._p(yg), self._p(zs), k, out,
                                                  C.byref(best)), "depgan_gen_iteration")
        v = [float(t) for t in out]
        o = 0
        cy = [v[o + 2 * j:o + 2 * j + 2] for j in range(na)]
        o += 2 * na
        cd = [v[o + 2 * j:o + 2 * j + 2] for j in range(nb)]
        o += 2 * nb
        ev = [v[o + 6 * i:o + 6 * i + 6] for i in range(k)]
        o += 6 * k
        return cy, cd, ev, v[o:o + 6], int(best.value)

    # ---- DEP-UResNet supervised path (nc_out >= 2) ----
    def _codes(self, labels):
        """(n, H, W) or (n, H, W, 1) class indices of any integer dtype, or float with integral values, as the contiguous
        uint8 CUDA tensor the *_sparse entries read (NumPy arrays are narrowed on the host: 1 byte per pixel crosses the
        bus).  A float that is not integral is a ValueError; a value outside [0, 255] becomes 255, which no class count
        reaches, so the library reports it with the other out-of-range codes.  With an ignore label set
        (set_loss_weights) the value equal to it reaches the device as that byte, and a value outside [0, 255] becomes
        a byte that is neither a class nor the ignore label (254 when the ignore label is 255)."""
        torch = _torch()
        tens = isinstance(labels, torch.Tensor)
        a = labels if tens else np.asarray(labels)
        if a.ndim == 4:
            a = a[..., 0]
        u8 = torch.uint8 if tens else np.uint8
        if a.dtype != u8:
            xp = torch if tens else np
            a = require_class_indices(a)
            if a.dtype == (torch.bool if tens else np.bool_):
                a = a.to(u8) if tens else a.astype(u8)
            else:
                bad = (a < 0) | (a > 255)
                a = xp.where(bad, xp.full_like(a, 254 if self._ignore_label == 255 else 255), a)
                a = a.to(u8) if tens else a.astype(u8)
        t = a if tens else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(self.device).contiguous()

    def uresnet(self, x, z, labels, mode="step", drop_seed=0):
        """mode 'step' = train_on_batch (UT:602-606), 'grads' = gradients only, 'eval' = phase-0 loss.
        The leading dimension may be shorter than the engine batch (Keras' last batch of an epoch).
        labels: one-hot (n, H, W, nc_out), cast to float32 like Keras' feed (depgan_uresnet_*), or class indices
        (n, H, W) / (n, H, W, 1) of an integer dtype or float with integral values (depgan_uresnet_*_sparse, as uint8):
        the shape picks the entry."""
        self._need_trainable("uresnet")
        x = self._dev(x)
        n = int(x.shape[0])
        if n < 1 or n > self.batch or tuple(x.shape[1:]) != (self.height, self.width, self.nicg):
            raise ValueError("images must be (n<=%d,%d,%d,%d), got %s" % (self.batch, self.height, self.width,
                                                                          self.nicg, tuple(x.shape)))
        lshape = tuple(int(d) for d in (labels.shape if hasattr(labels, "shape") else np.shape(labels)))
        sparse = self.nc_out != 1 and lshape in ((n, self.height, self.width), (n, self.height, self.width, 1))
        if sparse:
            labels = self._codes(labels)
        else:
            labels = self._dev(labels, (n, self.height, self.width, self.nc_out))
        sfx = "_sparse" if sparse else ""
        z = self._dev(z).reshape(-1)
        if z.numel() != n * 32:
            raise ValueError("noise must be (%d,32,1)" % n)
        loss = C.c_float()
        self._use_current_stream()
        if mode == "eval":
            fn = getattr(self.lib, "depgan_uresnet_eval" + sfx)
            check(fn(self.h, self._p(x), self._p(z), self._p(labels), n, C.byref(loss)), "depgan_uresnet_eval" + sfx)
        else:
            fn = getattr(self.lib, {"step": "depgan_uresnet_step", "grads": "depgan_uresnet_grads"}[mode] + sfx)
            check(fn(self.h, self._p(x), self._p(z), self._p(labels), n, C.c_uint(int(drop_seed) & 0xFFFFFFFF),
                     C.byref(loss)), "depgan_uresnet_" + mode + sfx)
        return float(loss.value)

    def set_census(self, on=True):
        """depgan_uresnet_set_census: with it on every uresnet() call also counts the (true class, predicted class) pixel
        pairs in the loss kernel; the loss and the gradients keep their bits.  ValueError on an inference context."""
        if on:
            self._need_trainable("set_census")
        check(self.lib.depgan_uresnet_set_census(self.h, 1 if on else 0), "depgan_uresnet_set_census")

    @property
    def census(self):
        return bool(self.lib.depgan_uresnet_get_census(self.h))

    def uresnet_census(self):
        """The (nc_out, nc_out) np.int64 confusion matrix of the last uresnet() call, row = true class, column = the
        arg-max of the probabilities (first index on a tie).  'step' and 'grads' count the phase-1 predictions the loss
        was taken from (batch statistics, dropout, before the update: what Keras' training metrics see), 'eval' the
        phase-0 ones.  It came back with that call's loss; this reads host memory (depgan_uresnet_last_census)."""
        out, k = (C.c_longlong * (_lib.MAX_HEAD_CLASSES ** 2))(), C.c_int()
        check(self.lib.depgan_uresnet_last_census(self.h, out, C.byref(k)), "depgan_uresnet_last_census")
        return np.array(out[:k.value * k.value], np.int64).reshape(k.value, k.value)

    def set_loss_weights(self, class_weight=None, ignore_label=None):
        """depgan_uresnet_set_loss_weights: the loss-weight mode of every uresnet() call.  class_weight: nc_out floats,
        finite and >= 0 with at least one > 0 (None with an ignore_label: unit weights); ignore_label: None, or a label
        value 0..255 whose pixels add no loss and no gradient and are not counted as out of range (class codes only: with
        one-hot labels an ignored pixel is an all-zero row).  The loss is the weighted sum over the number of pixels with
        a non-zero weight (Keras 2's weighted-objective rule).  Both None turns the mode off (the default)."""
        if class_weight is None and ignore_label is None:
            check(self.lib.depgan_uresnet_set_loss_weights(self.h, None, 0, -1), "depgan_uresnet_set_loss_weights")
            self._ignore_label = None
            return
        self._need_trainable("set_loss_weights")
        w = np.ones(self.nc_out, np.float32) if class_weight is None else np.asarray(class_weight, np.float32).reshape(-1)
        if ignore_label is not None and (int(ignore_label) != ignore_label or not 0 <= int(ignore_label) <= 255):
            raise ValueError("ignore_label must be an integer in [0, 255], got %r" % (ignore_label,))
        arr = (C.c_float * len(w))(*[float(v) for v in w])
        check(self.lib.depgan_uresnet_set_loss_weights(self.h, arr, len(w), -1 if ignore_label is None else int(ignore_label)),
              "depgan_uresnet_set_loss_weights")
        self._ignore_label = None if ignore_label is None else int(ignore_label)

    @property
    def loss_weights(self):
        """None with the loss-weight mode off, else (np.float32 class weights, ignore label or None)."""
        w, ign = (C.c_float * _lib.MAX_HEAD_CLASSES)(), C.c_int()
        if not self.lib.depgan_uresnet_get_loss_weights(self.h, w, C.byref(ign)):
            return None
        return np.array(w[:self.nc_out], np.float32), (None if ign.value < 0 else ign.value)

    def uresnet_label_counts(self):
        """The label pre-pass counts of the last uresnet() call made in the loss-weight mode or the focal mode, as a dict: 'den' (pixels
        with a non-zero weight, the loss's denominator), 'ignored' (pixels without a true class), 'bad' (out-of-range
        codes) and 'classes' (np.int64 pixel count per true class).  Host memory (depgan_uresnet_last_label_counts)."""
        out, k = (C.c_longlong * _lib._K["DEPGAN_LABEL_NCOUNT"])(), C.c_int()
        check(self.lib.depgan_uresnet_last_label_counts(self.h, out, C.byref(k)), "depgan_uresnet_last_label_counts")
        return {"den": int(out[0]), "ignored": int(out[1]), "bad": int(out[2]),
                "classes": np.array(out[3:3 + k.value], np.int64)}

    def set_focal(self, gamma=0.0, label_smoothing=0.0):
        """depgan_uresnet_set_focal: the focal mode of every uresnet() call.  gamma: the focal exponent, finite and >= 0
        (each pixel's cross-entropy term is scaled by (1 - r)^gamma); label_smoothing: finite and in [0, 1) (the label
        row becomes (1 - eps) t + eps / nc_out on pixels with a true class).  Both act inside the loss kernel, on top of
        the class weights and the ignore label of set_loss_weights.  The loss is the sum over the number of pixels with
        a non-zero weight, as in the loss-weight mode: with one-hot labels an all-zero row is then an ignored pixel.
        Both 0 turns the mode off (the default)."""
        for v, name in ((gamma, "gamma"), (label_smoothing, "label_smoothing")):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError("%s must be a number, got %r" % (name, v))
        if float(gamma) != 0.0 or float(label_smoothing) != 0.0:
            self._need_trainable("set_focal")
        check(self.lib.depgan_uresnet_set_focal(self.h, float(gamma), float(label_smoothing)), "depgan_uresnet_set_focal")

    @property
    def focal(self):
        """None with the focal mode off, else (gamma, label_smoothing) as the library holds them (float32 values)."""
        g, e = C.c_float(), C.c_float()
        if not self.lib.depgan_uresnet_get_focal(self.h, C.byref(g), C.byref(e)):
            return None
        return g.value, e.value

    def set_dice_loss(self, form=None, ce_weight=1.0, dice_weight=1.0, smooth=1e-7, class_coef=None):
        """depgan_uresnet_set_dice_loss: the soft Dice loss of every uresnet() call, alone or added to the cross-entropy.
        form: None (off, the default), 'flat' (the reference's dice_coef_loss over everything flattened, UT:110-121) or
        'class' (sum_k c_k (1 - Dice_k), class_coef = the nc_out coefficients c_k, None for 1 / nc_out each).  The loss
        of a call is ce_weight * cross-entropy + dice_weight * Dice; ce_weight >= 0, dice_weight > 0, smooth > 0.  With
        the loss-weight mode on, pixels without a true class (the ignore label, an all-zero one-hot row) take no part."""
        if form is None:
            check(self.lib.depgan_uresnet_set_dice_loss(self.h, 0, 1.0, 1.0, 0.0, None, 0), "depgan_uresnet_set_dice_loss")
            return
        self._need_trainable("set_dice_loss")
        if form not in _DICE_FORMS:
            raise ValueError("form must be None, 'flat' or 'class', got %r" % (form,))
        arr, n = None, 0
        if class_coef is not None:
            c = np.asarray(class_coef, np.float32).reshape(-1)
            arr, n = (C.c_float * len(c))(*[float(v) for v in c]), len(c)
        check(self.lib.depgan_uresnet_set_dice_loss(self.h, _DICE_FORMS[form], float(ce_weight), float(dice_weight),
                                                    float(smooth), arr, n), "depgan_uresnet_set_dice_loss")

    @property
    def dice_loss(self):
        """None with the Dice loss off, else a dict: 'form', 'ce_weight', 'dice_weight', 'smooth' and 'class_coef'
        (np.float32, the class form's coefficients; None for the flat form)."""
        ce, dw, sm, cc = C.c_float(), C.c_float(), C.c_float(), (C.c_float * _lib.MAX_HEAD_CLASSES)()
        form = self.lib.depgan_uresnet_get_dice_loss(self.h, C.byref(ce), C.byref(dw), C.byref(sm), cc)
        if not form:
            return None
        name = [k for k, v in _DICE_FORMS.items() if v == form][0]
        return {"form": name, "ce_weight": ce.value, "dice_weight": dw.value, "smooth": sm.value,
                "class_coef": np.array(cc[:self.nc_out], np.float32) if name == "class" else None}

    def uresnet_dice_sums(self):
        """The Dice sums of the last uresnet() call made with the Dice loss on, as a dict of np.float64 arrays (nc_out):
        'intersection' (I_k = sum t_k p_k), 'pred' (P_k = sum p_k), 'true' (T_k = sum t_k) over the pixels that took
        part, and 'loss', the Dice term.  evaluate.soft_dice turns them into per-class soft Dice.  They came back with
        that call's loss; this reads host memory (depgan_uresnet_last_dice_sums)."""
        out, k, loss = (C.c_double * (3 * _lib.MAX_HEAD_CLASSES))(), C.c_int(), C.c_float()
        check(self.lib.depgan_uresnet_last_dice_sums(self.h, out, C.byref(k), C.byref(loss)), "depgan_uresnet_last_dice_sums")
        n = k.value
        return {"intersection": np.array(out[:n], np.float64), "pred": np.array(out[n:2 * n], np.float64),
                "true": np.array(out[2 * n:3 * n], np.float64), "loss": float(loss.value)}

    def set_boundary_loss(self, on=True, weight=1.0, class_coef=None, spacing=(1.0, 1.0), inside_offset=0.0):
        """depgan_uresnet_set_boundary_loss: the boundary loss of every uresnet() call (Kervadec et al.): the softmax
        probabilities integrated against the signed distance map of the call's labels, weight * L_B added to what the
        cross-entropy and the Dice mode compute.  class_coef: the nc_out coefficients c_k >= 0 (None: 1 / nc_out each; a
        class with 0 gets no map); spacing = (sy, sx) > 0; inside_offset in [0, min(spacing)] (0: the symmetric map).
        L_B is negative at a perfect prediction.  The first call allocates the maps; calling again with another weight
        allocates nothing, so a schedule may do it before every epoch.  on=False turns the mode off (the default)."""
        if not on:
            check(self.lib.depgan_uresnet_set_boundary_loss(self.h, 0, 0.0, None, 0, 1.0, 1.0, 0.0),
                  "depgan_uresnet_set_boundary_loss")
            return
        self._need_trainable("set_boundary_loss")
        arr, n = None, 0
        if class_coef is not None:
            c = np.asarray(class_coef, np.float32).reshape(-1)
            arr, n = (C.c_float * len(c))(*[float(v) for v in c]), len(c)
        sy, sx = (float(v) for v in spacing)
        check(self.lib.depgan_uresnet_set_boundary_loss(self.h, 1, float(weight), arr, n, sy, sx, float(inside_offset)),
              "depgan_uresnet_set_boundary_loss")

    @property
    def boundary_loss(self):
        """None with the boundary loss off, else a dict: 'weight', 'class_coef' (np.float32), 'spacing' (sy, sx) and
        'inside_offset' as the library holds them."""
        w, cc = C.c_float(), (C.c_float * _lib.MAX_HEAD_CLASSES)()
        sy, sx, off = C.c_double(), C.c_double(), C.c_double()
        if not self.lib.depgan_uresnet_get_boundary_loss(self.h, C.byref(w), cc, C.byref(sy), C.byref(sx), C.byref(off)):
            return None
        return {"weight": w.value, "class_coef": np.array(cc[:self.nc_out], np.float32),
                "spacing": (sy.value, sx.value), "inside_offset": off.value}

    def uresnet_boundary_loss(self):
        """(L_B, M) of the last uresnet() call made with the boundary loss on: the boundary term before its weight, and
        the number of pixels that took part.  They came back with that call's loss; this reads host memory
        (depgan_uresnet_last_boundary_loss)."""
        lb, m = C.c_double(), C.c_longlong()
        check(self.lib.depgan_uresnet_last_boundary_loss(self.h, C.byref(lb), C.byref(m)),
              "depgan_uresnet_last_boundary_loss")
        return float(lb.value), int(m.value)

    def apply_adam(self, net):
        self._need_trainable("apply_adam")
        self._use_current_stream()
        check(self.lib.depgan_apply_adam(self.h, NET_IDS[net]), "depgan_apply_adam")

    # ---- optimiser options (depgan_set_lr, depgan_set_optimizer) ----
    @staticmethod
    def _opt_number(v, name, positive):
        """`v` as a float that is finite and > 0 (`positive`) or >= 0 once rounded to float32; ValueError otherwise.
        None stands for 0 (off) where 0 is allowed.  No library call."""
        if v is None and not positive:
            return 0.0
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("%s must be a number, got %r" % (name, v))
        with np.errstate(over="ignore"):
            v32 = float(np.float32(v))
        if not np.isfinite(v32) or (v32 <= 0 if positive else v32 < 0):
            raise ValueError("%s must be finite and %s 0 (as float32), got %r" % (name, ">" if positive else ">=", v))
        return float(v)

    def set_lr(self, net, lr):
        """depgan_set_lr: the learning rate of one network's Adam, from the next update on (host only)."""
        check(self.lib.depgan_set_lr(self.h, NET_IDS[net], self._opt_number(lr, "lr", True)), "depgan_set_lr")

    def lr(self, net):
        """The learning rate the next update of `net` uses, as the library holds it (a float32 value)."""
        v = C.c_float()
        check(self.lib.depgan_get_lr(self.h, NET_IDS[net], C.byref(v)), "depgan_get_lr")
        return v.value

    def set_optimizer(self, net, clipnorm=0, clipvalue=0, weight_decay=0):
        """depgan_set_optimizer: options of every Adam update of `net`, each finite and >= 0 with 0 (or None) = off.
        clipnorm: the gradient is scaled by clipnorm / norm when its global L2 norm (over all tensors, taken on the
        device in front of the update) reaches clipnorm -- standalone Keras 2's clipnorm; an update whose norm is not
        finite changes no weight and no Adam moment, though adam_step still counts it.  clipvalue: every gradient
        element is then clamped to +-clipvalue.  weight_decay: decoupled decay (AdamW), p <- p - lr * weight_decay * p
        before the Adam displacement, on the "/kernel" tensors only (never biases or BatchNorm gamma / beta).  All off
        (the default) is the plain update, bit for bit."""
        vals = [self._opt_number(v, n, False) for v, n in ((clipnorm, "clipnorm"), (clipvalue, "clipvalue"),
                                                           (weight_decay, "weight_decay"))]
        if any(vals):
            self._need_trainable("set_optimizer")
        check(self.lib.depgan_set_optimizer(self.h, NET_IDS[net], *vals), "depgan_set_optimizer")

    def optimizer(self, net):
        """None with every option off, else a dict of 'clipnorm', 'clipvalue' and 'weight_decay' (float32 values)."""
        a, b, w = C.c_float(), C.c_float(), C.c_float()
        if not self.lib.depgan_get_optimizer(self.h, NET_IDS[net], C.byref(a), C.byref(b), C.byref(w)):
            return None
        return {"clipnorm": a.value, "clipvalue": b.value, "weight_decay": w.value}

    def grad_norm(self, net):
        """(norm, scale) of the last update of `net` made with clipnorm on: the global L2 norm of the gradient the
        update applied (float64, summed on the device) and the float32 factor it was scaled by (1.0: not clipped; 0.0:
        the norm was not finite and the update was skipped).  Waits for the stream (depgan_last_grad_norm)."""
        norm, scale = C.c_double(), C.c_float()
        check(self.lib.depgan_last_grad_norm(self.h, NET_IDS[net], C.byref(norm), C.byref(scale)),
              "depgan_last_grad_norm")
        return norm.value, scale.value

    def last_sums(self):
        out = (C.c_float * 8)()
        check(self.lib.depgan_last_sums(self.h, out), "depgan_last_sums")
        return [float(v) for v in out]

    # ---- parity-test surface ----
    def debug_capture(self, on=True):
        """Keep a copy of the mixed pass's activations in every critic closure (depgan_debug_capture)."""
        check(self.lib.depgan_debug_capture(self.h, 1 if on else 0), "depgan_debug_capture")

    def _debug_fetch(self, entry, name, dtype):
        """Size-then-fill of the debug surface: asks `entry` for the shape (NULL destination), then for the data."""
        fn, shape = getattr(self.lib, entry), (C.c_int * 4)()
        check(fn(self.h, name.encode(), None, 0, shape), entry)
        out = np.empty(tuple(shape), dtype)
        check(fn(self.h, name.encode(), C.c_void_p(out.ctypes.data), out.size, shape), entry)
        return out

    def debug_tensor(self, name):
        """An internal tensor of the last closure as a dense (N,H,W,C) float32 array (depgan_debug_tensor)."""
        return self._debug_fetch("depgan_debug_tensor", name, np.float32)

    def debug_film_decision_bf16s(self, layer):
        """The FiLM ReLU decisions (uint8, 0 / 1, (N, H, W, C)) the last training forward on bfloat16 storage stored for a
        FiLM layer ("gen_2", ...): what its backward masks with (depgan_debug_film_decision_bf16s)."""
        return self._debug_fetch("depgan_debug_film_decision_bf16s", layer, np.uint8)

    def debug_tensor_bf16s(self, name):
        """"g/out/<layer>" of the last bfloat16-storage g_forward, widened to float32 (depgan_debug_tensor_bf16s)."""
        return self._debug_fetch("depgan_debug_tensor_bf16s", name, np.float32)

    # ---- profiling ----
    def profile(self, on):
        check(self.lib.depgan_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        check(self.lib.depgan_profile_reset(self.h))

    def profile_dump(self, path):
        check(self.lib.depgan_profile_dump(self.h, path.encode()))

    def profile_read(self, klass):
        ms, n, fl = C.c_double(), C.c_long(), C.c_double()
        check(self.lib.depgan_profile_read(self.h, klass, C.byref(ms), C.byref(n), C.byref(fl)))
        return ms.value, n.value, fl.value

    def profile_read_bytes(self, klass):
        by = C.c_double()
        check(self.lib.depgan_profile_read_bytes(self.h, klass, C.byref(by)))
        return by.value
