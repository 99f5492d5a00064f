"""Keras-style model objects over the HIP engine.

Same constructor names and call surface as the reference script
(DEP-GAN_PROB_IM_twoCritics_training_4fold.py, "GT"):
    Gen_UNet2D(input_shape, noiseZ_shape=(32, 1), first_fm=32, nc_out=1)   GT:349
    Dis_C2D_FCN1(input_shape)                                              GT:316
returning objects with .summary() .predict() .trainable_weights .get_weights()
.set_weights() .save() .load_weights() (GT:514-521, 846-848, 892; GE:383).
Weights are keyed by the reference's Keras layer names ('conv2d_gen_0/kernel',
'bn_gen_0/gamma', 'dense_noise_2_mul_m1/kernel', 'deconv2d_de_gen_9/kernel', ...)
in Keras layouts, so an .h5 importer is a pure rename.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np

from ._lib import MAX_HEAD_CLASSES
from .engine import Engine, require_class_indices


class WeightRef:
    """What model.trainable_weights enumerates (name + shape, like a tf.Variable)."""

    def __init__(self, name, shape):
        self.name, self.shape = name, tuple(shape)

    def __repr__(self):
        return "<Weight %s %s>" % (self.name, self.shape)


def _glorot_uniform(rng, shape, fan_in, fan_out):
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=shape).astype(np.float32)


# keras.initializers.he_normal = VarianceScaling(scale=2, mode='fan_in', distribution='normal'): a normal truncated at
# two standard deviations.  From Keras 2.2.3 on the sampled stddev is divided by .87962566103423978 (the standard deviation
# of the truncated unit normal) so that the RESULT has std sqrt(2/fan_in); earlier 2.x releases omit the correction
# (version-sensitive, unverifiable here).  The reference needs Python 2 + TF 1.x, for which 2.2.4 was the
# common release, so the corrected form is used -- the same constant as oracle/depgan_oracle.py::_he_normal.
HE_NORMAL_TRUNC_STD = 0.87962566103423978


def _he_normal(rng, shape, fan_in):
    std = math.sqrt(2.0 / fan_in) / HE_NORMAL_TRUNC_STD
    v = rng.standard_normal(size=shape)
    bad = np.abs(v) > 2
    while bad.any():
        v[bad] = rng.standard_normal(size=int(bad.sum()))
        bad = np.abs(v) > 2
    return (v * std).astype(np.float32)


def _keras_init(name, shape, rng):
    """Keras default initialisers for the layers the reference builds."""
    if name.endswith("/bias") or name.endswith("/beta") or name.endswith("/moving_mean"):
        return np.zeros(shape, np.float32)
    if name.endswith("/gamma") or name.endswith("/moving_variance"):
        return np.ones(shape, np.float32)
    if name.startswith("dense_") or name.startswith("dis_9"):   # he_normal (GT:256, 263, 339, 342)
        fan_in = int(np.prod(shape[:-1]))
        return _he_normal(rng, shape, fan_in)
    if name.startswith("deconv2d_"):                             # (kh,kw,Cout,Cin)
        kh, kw, co, ci = shape
        return _glorot_uniform(rng, shape, kh * kw * co, kh * kw * ci)
    kh, kw, ci, co = shape                                       # Conv2D glorot_uniform
    return _glorot_uniform(rng, shape, kh * kw * ci, kh * kw * co)


class _Model:
    net = None        # engine net id: 'G', 'D_y2', 'D_dem'
    name = "model"

    def __init__(self, input_shape, seed=None):
        self.input_shape = tuple(input_shape)
        self._engine = None
        self._host = None          # OrderedDict while unbound
        self._seed = seed
        self._private_engine = None

    # -- engine binding --
    def _spec_engine(self, batch):
        raise NotImplementedError

    def _bind(self, engine, net):
        host = self._weights_dict()
        self._engine, self.net = engine, net
        self._host = None
        engine.set_weights(net, host)

    def _ensure_engine(self, batch=32):
        if self._engine is None:
            eng = self._spec_engine(batch)
            self._bind(eng, self.net)
            self._private_engine = eng
        return self._engine

    def _table(self):
        if self._engine is not None:
            return self._engine.param_table(self.net)
        return self._static_table()

    def _weights_dict(self):
        if self._engine is not None:
            return self._engine.get_weights(self.net)
        if self._host is None:
            rng = np.random.default_rng(self._seed)
            self._host = OrderedDict((n, _keras_init(n, s, rng)) for n, s, _ in self._static_table())
        return self._host

    # -- keras surface --
    @property
    def trainable_weights(self):
        return [WeightRef(n, s) for n, s, tr in self._named_table() if tr]

    def _named_table(self):
        if self._engine is not None:
            return [(n, s, tr) for n, s, _, tr in self._engine.param_table(self.net)]
        return self._static_table()

    def count_params(self):
        return int(sum(np.prod(s) for _, s, _ in self._named_table()))

    def get_weights(self):
        return list(self._weights_dict().values())

    def get_weights_dict(self):
        return OrderedDict(self._weights_dict())

    def set_weights(self, weights):
        if isinstance(weights, dict):
            new = weights
        else:
            names = [n for n, _, _ in self._named_table()]
            if len(weights) != len(names):
                raise ValueError("set_weights: expected %d arrays, got %d" % (len(names), len(weights)))
            new = OrderedDict(zip(names, weights))
        for (n, s, _) in self._named_table():
            if n in new and tuple(np.shape(new[n])) != tuple(s):
                raise ValueError("weight %s: expected shape %s, got %s" % (n, s, np.shape(new[n])))
        if self._engine is not None:
            self._engine.set_weights(self.net, new)
        else:
            cur = self._weights_dict()
            for n, v in new.items():
                if n not in cur:
                    raise ValueError("unknown weight name %s" % n)
                cur[n] = np.asarray(v, np.float32)

    def save_weights(self, path):
        np.savez(path, **self._weights_dict())

    save = save_weights   # netG.save(...) GT:892 (architecture is code here; the file holds the weights)

    def load_weights(self, path):
        """`.npz` written by save_weights, or a Keras 2.x HDF5 file (`model.save` / `save_weights`: GT:892, GE:383)
        through h5py when it is installed and through dep_gan_im_amd.h5lite otherwise -- the names and layouts here are
        the Keras ones, so that import is a lookup."""
        if str(path).lower().endswith((".h5", ".hdf5")):
            try:
                import h5py as h5
            except ImportError:
                from . import h5lite as h5      # pure-Python reader of the HDF5 subset Keras weight files use
            with h5.File(path, "r") as f:
                self.set_weights(weights_from_keras_h5(f, [n for n, _, _ in self._named_table()]))
            return
        with np.load(path) as f:
            self.set_weights({k: f[k] for k in f.files})

    def summary(self, print_fn=print):
        print_fn('Model: "%s"' % self.name)
        print_fn("%-44s %-22s %10s" % ("Weight (layer/name)", "Shape", "Param #"))
        print_fn("=" * 78)
        tot = tr_tot = 0
        for n, s, tr in self._named_table():
            k = int(np.prod(s))
            tot += k
            tr_tot += k if tr else 0
            print_fn("%-44s %-22s %10d" % (n, str(tuple(s)), k))
        print_fn("=" * 78)
        print_fn("Total params: %d\nTrainable params: %d\nNon-trainable params: %d" % (tot, tr_tot, tot - tr_tot))


def weights_from_keras_h5(f, names):
    """Maps a Keras 2.x HDF5 weight file onto this package's weight names ("<layer>/<weight>").

    f: an open h5py.File (anything indexable the same way).  `model.save` files keep the layers under the group
    "model_weights", `save_weights` files at the root; each layer group holds its tensors at
    "<layer>/<weight>:0" (a nested group named after the layer again).  Layers the file does not have, or extra ones,
    are an error: a silent partial load would pass every shape check and train from a half-initialised model."""
    g = f["model_weights"] if "model_weights" in f else f
    out, missing = OrderedDict(), []
    for n in names:
        layer, w = n.split("/", 1)
        ds = None
        if layer in g:
            lg = g[layer]
            for key in ("%s/%s:0" % (layer, w), "%s:0" % w, "%s/%s" % (layer, w), w):
                node, ok = lg, True
                for part in key.split("/"):
                    if hasattr(node, "keys") and part in node:
                        node = node[part]
                    else:
                        ok = False
                        break
                if ok and not hasattr(node, "keys"):
                    ds = node
                    break
        if ds is None:
            missing.append(n)
        else:
            out[n] = np.asarray(ds[()] if hasattr(ds, "shape") and not isinstance(ds, np.ndarray) else ds, np.float32)
    if missing:
        raise KeyError("Keras HDF5 file lacks %d of %d weights, e.g. %s" % (len(missing), len(names), missing[:3]))
    return out


def _gen_static_table(nicg, fm, nc_out):
    T = []

    def bn(n, c):
        T.extend([(n + "/gamma", (c,), True), (n + "/beta", (c,), True), (n + "/moving_mean", (c,), False),
                  (n + "/moving_variance", (c,), False)])

    def dense(n, fi, fo):
        T.extend([("dense_" + n + "/kernel", (fi, fo), True), ("dense_" + n + "/bias", (fo,), True)])
        bn("dense_bn_" + n, fo)

    dense("noise_1_add_f0", 1, fm)
    dense("noise_1_add_f1", fm, fm)
    for sfx, m in (("add_m3", 3), ("mul_m3", 3), ("add_m2", 2), ("mul_m2", 2), ("add_m1", 1), ("mul_m1", 1),
                   ("add", 4), ("mul", 4), ("add_p3", 3), ("mul_p3", 3), ("add_p2", 2), ("mul_p2", 2),
                   ("add_p1", 1), ("mul_p1", 1)):
        dense("noise_2_" + sfx, 32 * fm, fm * m)
    convs = [("gen_0", nicg, fm), ("gen_noise_m1", fm, fm), ("gen_1", fm, fm), ("gen_2", fm, 2 * fm),
             ("gen_noise_m2", 2 * fm, 2 * fm), ("gen_3", 2 * fm, 2 * fm), ("gen_4", 2 * fm, 3 * fm),
             ("gen_noise_m3", 3 * fm, 3 * fm), ("gen_5", 3 * fm, 3 * fm), ("gen_8", 3 * fm, 4 * fm),
             ("gen_noise_p4", 4 * fm, 4 * fm), ("gen_9", 4 * fm, 4 * fm), ("D:de_gen_9", 4 * fm, 4 * fm),
             ("gen_10", 7 * fm, 3 * fm), ("gen_noise_p3", 3 * fm, 3 * fm), ("gen_11", 3 * fm, 3 * fm),
             ("D:de_gen_11", 3 * fm, 3 * fm), ("gen_14", 5 * fm, 2 * fm), ("gen_noise_p2", 2 * fm, 2 * fm),
             ("gen_15", 2 * fm, 2 * fm), ("D:de_gen_15", 2 * fm, 2 * fm), ("gen_16", 3 * fm, fm),
             ("gen_noise_p1", fm, fm), ("gen_17", fm, fm)]
    for n, ci, co in convs:
        if n.startswith("D:"):
            n = n[2:]
            T.extend([("deconv2d_" + n + "/kernel", (2, 2, co, ci), True), ("deconv2d_" + n + "/bias", (co,), True)])
        else:
            T.extend([("conv2d_" + n + "/kernel", (3, 3, ci, co), True), ("conv2d_" + n + "/bias", (co,), True)])
        bn("bn_" + n, co)
    T.extend([("gen_segmentation/kernel", (1, 1, fm, nc_out), True), ("gen_segmentation/bias", (nc_out,), True)])
    return T


_LOSSES = ("categorical_crossentropy", "sparse_categorical_crossentropy")
# the reference's own loss name (UT:120): one-hot labels, the flat Dice form alone, smooth 1e-7
_DICE_LOSS = "dice_coef_loss"
# compile(metrics=[...]): the name as given is the history key; what it reads out of evaluate.confusion_metrics
_METRICS = {"acc": "accuracy", "accuracy": "accuracy", "dice": "mean_dice", "iou": "mean_iou"}


class History:
    """keras.callbacks.History: .history['loss'] / ['val_loss'] per epoch (UT:609-618).  With compile(metrics=[...])
    also .history[name] / ['val_' + name], and .census = {'train': [...], 'val': [...]}: per epoch the confusion matrix
    (np.int64 (C, C), row = true class) summed over the epoch's training batches / over the validation data."""

    def __init__(self, history, census=None):
        self.history = history
        if census is not None:
            self.census = census


class GeneratorModel(_Model):
    net = "G"
    name = "Gen_UNet2D"

    def __init__(self, input_shape, noiseZ_shape=(32, 1), first_fm=32, nc_out=1, seed=None, inference_dtype="float32",
                 _inference_only=False):
        super().__init__(input_shape, seed)
        if tuple(noiseZ_shape) != (32, 1) or first_fm != 32:
            raise ValueError("the HIP path is built for noiseZ_shape=(32,1), first_fm=32 (GT:520)")
        if isinstance(nc_out, bool) or not isinstance(nc_out, (int, np.integer)) or not 1 <= nc_out <= MAX_HEAD_CLASSES:
            raise ValueError("nc_out must be 1 (DEP-GAN generator, GT:520) or the DEP-UResNet's class count in [2, %d] "
                             "(the reference has 4, UT:573, 583), got %r" % (MAX_HEAD_CLASSES, nc_out))
        nc_out = int(nc_out)
        if inference_dtype not in ("float32", "bfloat16"):
            raise ValueError("inference_dtype must be 'float32' or 'bfloat16', got %r" % (inference_dtype,))
        if inference_dtype == "bfloat16" and nc_out != 1 and not _inference_only:
            raise ValueError("inference_dtype='bfloat16' (bf16 activation storage) with nc_out=%d: the constructor builds "
                             "trainable models and the softmax variant has no training on the bf16 pipe; train the "
                             "float32 model and take model.inference_copy('bfloat16') for predict" % nc_out)
        self.inference_dtype = inference_dtype
        self.inference_only = bool(_inference_only)      # a predict-only copy (inference_copy)
        self.noiseZ_shape, self.first_fm, self.nc_out = tuple(noiseZ_shape), first_fm, nc_out
        if nc_out != 1:
            self.name = "DEP_UResNet"
        # Gen_UNet2D compiles the softmax variant itself: Adam(lr=1e-4), categorical cross-entropy (UT:427)
        self._lr = 1e-4
        self._loss = "categorical_crossentropy"
        self._metrics = []
        self._class_weight, self._ignore_label = None, None      # compile(class_weight=, ignore_label=)
        self._dice = None                                        # compile(dice_loss=...): Engine.set_dice_loss's arguments
        self._focal = None                                       # compile(focal_gamma=, label_smoothing=), None when off
        self._boundary = None                                    # compile(boundary_loss=True, ...): Engine.set_boundary_loss's arguments
        self._opt = None                                         # compile(clipnorm=, clipvalue=, weight_decay=), None when off
        self.stop_training = False                               # a fit callback sets it to end fit after the epoch
        self._drop_rng = np.random.RandomState(seed)

    def _static_table(self):
        return _gen_static_table(self.input_shape[2], self.first_fm, self.nc_out)

    def _spec_engine(self, batch):
        H, W, nicg = self.input_shape
        if self.nc_out == 1 and self.inference_dtype == "bfloat16":
            # predict on the bf16 matrix pipe with bf16 activation storage (BASELINE config 4, forward only)
            eng = Engine(batch, H, W, nicg, bf16_mfma=True)
            eng.forward_storage = "bfloat16"
            return eng
        if self.nc_out == 1:
            return Engine(batch, H, W, nicg)
        if self.inference_only:
            # the inference context: the DEP-UResNet in learning phase 0 on the bf16 matrix pipe, bf16 activation storage
            eng = Engine(batch, H, W, nicg, nc_out=self.nc_out, bf16_mfma=True)
            eng.forward_storage = "bfloat16"
            return eng
        return Engine(batch, H, W, nicg, lrG=self._lr, beta1=0.9, beta2=0.999, nc_out=self.nc_out)

    def _bind(self, engine, net):
        super()._bind(engine, net)
        if self._metrics:
            engine.set_census(True)
        if self._class_weight is not None or self._ignore_label is not None:
            engine.set_loss_weights(self._class_weight, self._ignore_label)
        if self._dice is not None:
            engine.set_dice_loss(**self._dice)
        if self._focal is not None:
            engine.set_focal(*self._focal)
        if self._boundary is not None:
            engine.set_boundary_loss(**self._boundary)
        if self._opt is not None:
            engine.set_optimizer(net, **self._opt)

    def inference_copy(self, dtype="bfloat16"):
        """A new predict-only model with this architecture and a copy of the current weights, whose private engine runs
        predict on the bf16 matrix pipe with bf16 activation storage (for nc_out>=2 the inference context of
        include/depgan.h).  Later changes to this model are not followed.  predict, set_weights, load_weights,
        get_weights and save_weights work on the copy; compile, fit, train_on_batch, test_on_batch and evaluate raise
        RuntimeError.  For nc_out=1 the copy predicts what Gen_UNet2D(..., inference_dtype='bfloat16') with these
        weights predicts.  UE:553-564: evaluate.predict_mean(model.inference_copy(), flair, mask=...)."""
        if dtype != "bfloat16":
            raise ValueError("inference_copy: dtype must be 'bfloat16', got %r" % (dtype,))
        twin = GeneratorModel(self.input_shape, self.noiseZ_shape, self.first_fm, self.nc_out, self._seed, "bfloat16",
                              _inference_only=True)
        twin.set_weights(OrderedDict((n, np.array(v, np.float32)) for n, v in self._weights_dict().items()))
        return twin

    def predict(self, inputs, batch_size=32):
        """netG.predict([x, z])  (GT:848, 859; GE:621; UE:  my_network.predict)."""
        if not isinstance(inputs, (list, tuple)) or len(inputs) != 2:
            raise ValueError("Gen_UNet2D.predict expects [images, noise]")
        x, z = inputs
        eng = self._ensure_engine(min(batch_size, max(1, len(x))))
        return eng.g_forward(x, z, storage=self._predict_storage(eng)).cpu().numpy()

    def _predict_storage(self, eng):
        """The activation storage of predict on `eng`.  A model bound to a trainers' engine follows that engine: its
        weights and kernels live there, so inference_dtype='bfloat16' cannot be honoured on an fp32 engine."""
        if self.inference_dtype != "bfloat16":
            return None                      # the engine's own forward_storage
        if not eng.cfg.bf16_mfma:
            raise ValueError("inference_dtype='bfloat16': this model is bound to an engine without the bf16 matrix pipe "
                             "(build_trainers(..., activations_dtype='bfloat16') or an unbound model gives one)")
        return "bfloat16"

    # ---- supervised surface of the softmax variant (DEP-UResNet, UT:427, 583-618) ----
    def _need_softmax(self, what):
        if self.inference_only:
            raise RuntimeError("%s: this model is a predict-only inference copy (inference_copy); train the model it was "
                               "copied from" % what)
        if self.nc_out == 1:
            raise RuntimeError("%s: the tanh generator is trained through the WGAN-GP closures "
                               "(trainers.build_trainers), not compiled with a loss" % what)

    def _loss_weight_args(self, loss, class_weight, ignore_label):
        """compile's class_weight / ignore_label as (np.float32 weights or None, int or None); ValueError otherwise.
        Needs no engine."""
        C = self.nc_out
        if ignore_label is not None:
            if loss != "sparse_categorical_crossentropy":
                raise ValueError("ignore_label needs loss='sparse_categorical_crossentropy' (class indices); with one-hot "
                                 "labels encode ignored pixels as all-zero rows (data.to_one_hot(..., ignore_label=...))")
            if isinstance(ignore_label, bool) or not isinstance(ignore_label, (int, np.integer)) or not 0 <= ignore_label <= 255:
                raise ValueError("ignore_label must be an integer in [0, 255], got %r" % (ignore_label,))
            ignore_label = int(ignore_label)
        if class_weight is None:
            return None, ignore_label
        if isinstance(class_weight, dict):
            bad = [k for k in class_weight if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < C]
            if bad:
                raise ValueError("class_weight: keys must be class indices in [0, %d), got %r" % (C, bad))
            w = np.ones(C, np.float64)
            for k, v in class_weight.items():
                w[int(k)] = float(v)
        else:
            w = np.asarray(class_weight, np.float64).reshape(-1)
            if w.size != C:
                raise ValueError("class_weight must hold nc_out = %d weights, got %d" % (C, w.size))
        w32 = w.astype(np.float32)
        if not np.all(np.isfinite(w32)) or np.any(w32 < 0) or not np.any(w32 > 0):
            raise ValueError("class_weight: every weight must be finite and >= 0, and at least one > 0, got %r" % (w.tolist(),))
        return w32, ignore_label

    def _focal_args(self, focal_gamma, label_smoothing):
        """compile's focal_gamma / label_smoothing as (gamma, eps) floats, or None with the mode off (both 0);
        ValueError otherwise.  Needs no engine."""
        out = []
        for v, name in ((focal_gamma, "focal_gamma"), (label_smoothing, "label_smoothing")):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError("%s must be a number, got %r" % (name, v))
            v32 = float(np.float32(v))
            if not np.isfinite(v32) or v32 < 0 or (name == "label_smoothing" and v32 >= 1):
                raise ValueError("%s must be finite and %s (as float32), got %r"
                                 % (name, "in [0, 1)" if name == "label_smoothing" else ">= 0", v))
            out.append(float(v))
        return None if out[0] == 0.0 and out[1] == 0.0 else tuple(out)

    def _opt_args(self, optimizer, clipnorm, clipvalue, weight_decay):
        """compile's clipnorm / clipvalue / weight_decay (an argument wins over the optimizer object's attribute of that
        name) as the keyword arguments of Engine.set_optimizer, or None with all of them off; ValueError otherwise.
        Needs no engine."""
        out = {}
        for name, v in (("clipnorm", clipnorm), ("clipvalue", clipvalue), ("weight_decay", weight_decay)):
            if v is None:
                v = getattr(optimizer, name, None)
            out[name] = Engine._opt_number(v, name, False)
        return out if any(out.values()) else None

    def _dice_args(self, loss, dice_loss, dice_weight, ce_weight, dice_smooth, dice_classes):
        """compile's Dice arguments as the keyword arguments of Engine.set_dice_loss, or None with the mode off;
        ValueError otherwise.  Needs no engine."""
        C = self.nc_out
        if loss == _DICE_LOSS:
            if dice_loss not in (None, "flat") or dice_classes is not None:
                raise ValueError("loss='dice_coef_loss' is the flat form alone: leave dice_loss and dice_classes out")
            dice_loss, ce_weight = "flat", 0.0
        if dice_loss is None:
            if dice_classes is not None:
                raise ValueError("dice_classes needs dice_loss='class'")
            return None
        if dice_loss not in ("flat", "class"):
            raise ValueError("dice_loss must be None, 'flat' or 'class', got %r" % (dice_loss,))

        def number(v, name, positive):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError("%s must be a number, got %r" % (name, v))
            v32 = float(np.float32(v))
            if not np.isfinite(v32) or (v32 <= 0 if positive else v32 < 0):
                raise ValueError("%s must be finite and %s 0 (as float32), got %r" % (name, ">" if positive else ">=", v))
            return float(v)
        out = {"form": dice_loss, "ce_weight": number(ce_weight, "ce_weight", False),
               "dice_weight": number(dice_weight, "dice_weight", True), "smooth": number(dice_smooth, "dice_smooth", True),
               "class_coef": None}
        if dice_classes is None:
            return out
        if dice_loss == "flat":
            raise ValueError("dice_classes: the flat form has no class coefficients (dice_loss='class' takes them)")
        if isinstance(dice_classes, str):
            if dice_classes != "foreground":
                raise ValueError("dice_classes must be None, 'foreground' or %d coefficients, got %r" % (C, dice_classes))
            c = np.full(C, 1.0 / (C - 1), np.float64)
            c[0] = 0.0
        else:
            c = np.asarray(dice_classes, np.float64).reshape(-1)
            if c.size != C:
                raise ValueError("dice_classes must hold nc_out = %d coefficients, got %d" % (C, c.size))
        c32 = c.astype(np.float32)
        if not np.all(np.isfinite(c32)) or np.any(c32 < 0) or not np.any(c32 > 0):
            raise ValueError("dice_classes: every coefficient must be finite and >= 0, and at least one > 0, got %r"
                             % (c.tolist(),))
        out["class_coef"] = c32
        return out

    def _boundary_args(self, boundary_loss, boundary_weight, boundary_classes, boundary_spacing, boundary_inside_offset):
        """compile's boundary arguments as the keyword arguments of Engine.set_boundary_loss, or None with the mode
        off; ValueError otherwise.  Needs no engine."""
        C = self.nc_out
        if not isinstance(boundary_loss, (bool, np.bool_)):
            raise ValueError("boundary_loss must be True or False, got %r" % (boundary_loss,))
        if not boundary_loss:
            if boundary_classes is not None:
                raise ValueError("boundary_classes needs boundary_loss=True")
            return None
        H, W, _ = self.input_shape
        if not (1 <= H <= 4096 and 1 <= W <= 4096):
            raise ValueError("boundary_loss: the distance transform takes images of 1..4096 pixels a side, got %dx%d" % (H, W))
        if boundary_weight is None:
            raise ValueError("boundary_weight must be a number, got None")
        weight = Engine._opt_number(boundary_weight, "boundary_weight", False)
        try:
            sp = tuple(boundary_spacing)
        except TypeError:
            sp = ()
        if len(sp) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) for v in sp) \
                or not all(np.isfinite(float(v)) and float(v) > 0 for v in sp):
            raise ValueError("boundary_spacing must be (sy, sx), two finite numbers > 0, got %r" % (boundary_spacing,))
        sp = (float(sp[0]), float(sp[1]))
        off = boundary_inside_offset
        if isinstance(off, bool) or not isinstance(off, (int, float, np.integer, np.floating)) \
                or not 0.0 <= float(off) <= min(sp):
            raise ValueError("boundary_inside_offset must be a number in [0, min(boundary_spacing)] = [0, %g], got %r"
                             % (min(sp), off))
        out = {"weight": weight, "class_coef": None, "spacing": sp, "inside_offset": float(off)}
        if boundary_classes is None:
            return out
        if isinstance(boundary_classes, str):
            if boundary_classes != "foreground":
                raise ValueError("boundary_classes must be None, 'foreground' or %d coefficients, got %r"
                                 % (C, boundary_classes))
            c = np.full(C, 1.0 / (C - 1), np.float64)
            c[0] = 0.0
        else:
            c = np.asarray(boundary_classes, np.float64).reshape(-1)
            if c.size != C:
                raise ValueError("boundary_classes must hold nc_out = %d coefficients, got %d" % (C, c.size))
        c32 = c.astype(np.float32)
        if not np.all(np.isfinite(c32)) or np.any(c32 < 0) or not np.any(c32 > 0):
            raise ValueError("boundary_classes: every coefficient must be finite and >= 0, and at least one > 0, got %r"
                             % (c.tolist(),))
        out["class_coef"] = c32
        return out

    @property
    def boundary_weight(self):
        """The weight of the boundary term in the loss, None with compile(boundary_loss=False)."""
        return None if self._boundary is None else self._boundary["weight"]

    def set_boundary_weight(self, weight):
        """Sets the weight of the boundary term, before or after the first use (finite and >= 0); on an engine it holds
        from the next call on and allocates nothing (Engine.set_boundary_loss).  The schedule the loss is used with
        starts small and rises: callbacks.BoundaryWeightScheduler calls this before every epoch."""
        self._need_softmax("set_boundary_weight")
        if self._boundary is None:
            raise RuntimeError("set_boundary_weight: the model was not compiled with boundary_loss=True")
        if weight is None:
            raise ValueError("boundary_weight must be a number, got None")
        weight = Engine._opt_number(weight, "boundary_weight", False)
        if self._engine is not None:
            self._engine.set_boundary_loss(**dict(self._boundary, weight=weight))
        self._boundary = dict(self._boundary, weight=weight)

    def compile(self, optimizer="adam", loss="categorical_crossentropy", lr=None, metrics=None, class_weight=None,
                ignore_label=None, dice_loss=None, dice_weight=1.0, ce_weight=1.0, dice_smooth=1e-7, dice_classes=None,
                focal_gamma=0.0, label_smoothing=0.0, clipnorm=None, clipvalue=None, weight_decay=None,
                boundary_loss=False, boundary_weight=1.0, boundary_classes=None, boundary_spacing=(1.0, 1.0),
                boundary_inside_offset=0.0, **_):
        """model.compile(optimizer=Adam(lr=1e-4), loss='categorical_crossentropy')  (UT:427).
        metrics: names out of 'acc' / 'accuracy' (pixel accuracy: Keras' categorical_accuracy, arg-max against arg-max),
        'dice' and 'iou' (the means over the foreground classes 1..nc_out-1, evaluate.confusion_metrics).  They come from
        the confusion matrix the loss kernel counts on the device (Engine.set_census), so they cost no second pass and
        change no loss or gradient bit.  train_on_batch / test_on_batch / evaluate then return [loss, m1, ...] in the
        order given and fit records history[name] and history['val_' + name]; a training value is that of the phase-1
        predictions made before the update, as in Keras.  Per epoch the figures come from the table summed over the
        epoch's batches: Keras' sample-weighted accuracy exactly (every sample has H*W pixels), and the global Dice /
        IoU of the epoch rather than a mean of batch figures.  Without metrics nothing changes.
        loss='sparse_categorical_crossentropy' is the same loss on integer labels: train_on_batch, test_on_batch,
        evaluate, fit and its validation_data then take class indices (n, H, W) or (n, H, W, 1) -- any integer dtype, or
        float with integral values (data.to_codes makes them, 1 byte per pixel) -- instead of the one-hot
        (n, H, W, nc_out) tensor, and compute bit for bit what the one-hot encoding of those labels gives.
        class_weight: nc_out floats, or a dict {class: weight} with the missing classes at 1.0 (Keras refuses
        class_weight for targets of 3 or more dimensions; data.balanced_class_weights makes them from pixel counts).
        ignore_label: a label value 0..255 whose pixels add no loss and no gradient (sparse loss only; with one-hot labels
        an all-zero row is the ignored pixel); alone it means unit weights.  Either turns the loss-weight mode on
        (Engine.set_loss_weights): the loss of train_on_batch, test_on_batch, evaluate, fit and its validation data is
        the weighted sum over the number of pixels with a non-zero weight, and the metrics leave ignored pixels out.
        compile() without them turns the mode off; then every result is what it was without the mode.
        dice_loss: None, 'flat' (the reference's dice_coef_loss, UT:110-121: one Dice over everything flattened) or
        'class' (sum_k c_k (1 - Dice_k) with dice_classes = None for c_k = 1 / nc_out, 'foreground' for c_0 = 0 and
        1 / (nc_out - 1) elsewhere -- the Dice metrics=['dice'] reports -- or nc_out coefficients >= 0).  The loss is then
        ce_weight * cross-entropy + dice_weight * Dice on the softmax probabilities (Engine.set_dice_loss); `loss` still
        selects the label format and the cross-entropy, and class_weight acts on the cross-entropy alone, while ignored
        pixels are left out of both.  loss='dice_coef_loss' is the reference's name for one-hot labels, the flat form,
        ce_weight = 0 and smooth 1e-7.  compile() without these arguments turns the Dice loss off.
        focal_gamma: the focal loss's exponent, finite and >= 0 (Keras' CategoricalFocalCrossentropy without its alpha:
        class_weight is the alpha): each pixel's cross-entropy term is scaled by (1 - r)^gamma, so easy pixels stop
        dominating the gradient.  label_smoothing: finite and in [0, 1), Keras' argument of that name: the label row of
        a pixel with a true class becomes (1 - eps) t + eps / nc_out.  Either turns the focal mode on
        (Engine.set_focal), inside the loss kernel; both work with both label formats, with class_weight / ignore_label,
        metrics (which keep reading the original labels) and dice_loss (the Dice term reads the original labels; with
        ce_weight = 0 they change nothing but the reported cross-entropy sums).  The loss is then the sum over the
        number of pixels with a non-zero weight, as with class_weight: with one-hot labels an all-zero row is an
        ignored pixel.  compile() without them turns the mode off; then every result is what it was without the mode.
        clipnorm, clipvalue, weight_decay: options of the Adam update (Engine.set_optimizer), each finite and >= 0 with
        None or 0 = off; they are also read from attributes of those names on an `optimizer` object, as lr is.  clipnorm
        scales the whole gradient by clipnorm / norm once its global L2 norm reaches clipnorm (standalone Keras 2's
        clipnorm; Engine.grad_norm reads the norm back), clipvalue then clamps every element, weight_decay is AdamW's
        decoupled decay on the kernels (not biases, not BatchNorm).  All of it runs inside the update's own launches
        on the device.  compile() without them is the plain Adam update, bit for bit.  The rate itself can change at
        any time: model.set_lr(lr), or fit(callbacks=[...]) with dep_gan_im_amd.callbacks.
        boundary_loss=True adds boundary_weight * L_B to the loss (Kervadec et al.; Engine.set_boundary_loss): the
        softmax probabilities integrated against the signed distance map of each label slice, which the library computes
        on the device for every batch, so it follows fit(augment=...).  boundary_classes: None (1 / nc_out each),
        'foreground' (class 0 out, 1 / (nc_out - 1) elsewhere) or nc_out coefficients >= 0; boundary_spacing = (sy, sx)
        pixel spacings > 0; boundary_inside_offset in [0, min(spacing)] (0: the symmetric map).  L_B is negative at a
        perfect prediction, so the loss reported may be negative.  It works with both label formats, class_weight /
        ignore_label (ignored pixels take no part and belong to no class), dice_loss, focal_gamma / label_smoothing and
        metrics.  The term is used with a weight that starts small and rises: model.set_boundary_weight(w), or
        callbacks.BoundaryWeightScheduler in fit, which then records history['boundary_weight'].  compile() without
        boundary_loss turns the mode off; then every result is what it was without it."""
        self._need_softmax("compile")
        if loss not in _LOSSES + (_DICE_LOSS,):
            raise ValueError("loss must be 'categorical_crossentropy' (UT:427), 'sparse_categorical_crossentropy' or "
                             "'dice_coef_loss' (UT:120), got %r" % (loss,))
        dice = self._dice_args(loss, dice_loss, dice_weight, ce_weight, dice_smooth, dice_classes)
        focal = self._focal_args(focal_gamma, label_smoothing)
        opt = self._opt_args(optimizer, clipnorm, clipvalue, weight_decay)
        boundary = self._boundary_args(boundary_loss, boundary_weight, boundary_classes, boundary_spacing,
                                       boundary_inside_offset)
        was_on = self._class_weight is not None or self._ignore_label is not None
        self._class_weight, self._ignore_label = self._loss_weight_args(loss, class_weight, ignore_label)
        if self._engine is not None and (self._dice is not None or dice is not None):
            self._engine.set_dice_loss(**(dice or {"form": None}))
        self._dice = dice
        if self._engine is not None and (was_on or self._class_weight is not None or self._ignore_label is not None):
            self._engine.set_loss_weights(self._class_weight, self._ignore_label)
        if self._engine is not None and (self._focal is not None or focal is not None):
            self._engine.set_focal(*(focal or (0.0, 0.0)))
        self._focal = focal
        if self._engine is not None and (self._boundary is not None or boundary is not None):
            self._engine.set_boundary_loss(**(boundary or {"on": False}))
        self._boundary = boundary
        if self._engine is not None and (self._opt is not None or opt is not None):
            self._engine.set_optimizer(self.net, **(opt or {}))
        self._opt = opt
        if metrics is not None:
            if isinstance(metrics, str):
                metrics = [metrics]
            bad = [m for m in metrics if not isinstance(m, str) or m not in _METRICS]
            if bad or len(set(metrics)) != len(metrics):
                raise ValueError("metrics must be distinct names out of %s, got %r" % (sorted(_METRICS), list(metrics)))
            metrics = list(metrics)
            if self._engine is not None:
                self._engine.set_census(bool(metrics))
            self._metrics = metrics
        self._loss = loss
        if lr is None:
            lr = getattr(optimizer, "lr", None)
        if lr is not None:
            if self._engine is not None and float(lr) != self._lr:
                raise RuntimeError("compile(lr=...) must come before the first fit / train_on_batch / predict")
            self._lr = float(lr)
        return self

    @property
    def lr(self):
        """The learning rate the next update uses: compile's until an engine exists, then the engine's own (a float32
        value), which set_lr and the callbacks of fit change."""
        return self._lr if self._engine is None else self._engine.lr(self.net)

    def set_lr(self, lr):
        """Sets the learning rate, before or after the first use; on an engine it takes effect at the next update
        (Engine.set_lr).  Finite and > 0."""
        self._need_softmax("set_lr")
        lr = Engine._opt_number(lr, "lr", True)
        if self._engine is not None:
            self._engine.set_lr(self.net, lr)
        self._lr = lr

    def _check_labels(self, labels, n, what):
        """The labels' shape against the compiled loss, before anything reaches the library."""
        H, W, _ = self.input_shape
        shape = tuple(int(d) for d in (labels.shape if hasattr(labels, "shape") else np.shape(labels)))
        if self._loss == "sparse_categorical_crossentropy":
            want = ((n, H, W), (n, H, W, 1))
            text = "class indices of shape (%d, %d, %d) or (%d, %d, %d, 1)" % (n, H, W, n, H, W)
        else:
            want = ((n, H, W, self.nc_out),)
            text = "one-hot labels of shape (%d, %d, %d, %d)" % (n, H, W, self.nc_out)
        if shape not in want:
            raise ValueError("%s: loss=%r takes %s, got shape %s" % (what, self._loss, text, shape))
        if self._loss == "sparse_categorical_crossentropy":
            require_class_indices(labels)

    def _next_drop_seed(self):
        return int(self._drop_rng.randint(1, 2 ** 31 - 1))

    def _metric_values(self, cm):
        """The compiled metrics of one confusion matrix, in the order given to compile."""
        from .evaluate import confusion_metrics
        m = confusion_metrics(cm)
        return [m[_METRICS[name]] for name in self._metrics]

    def _with_metrics(self, eng, loss):
        return [loss] + self._metric_values(eng.uresnet_census()) if self._metrics else loss

    def train_on_batch(self, inputs, labels, drop_seed=None):
        """One learning-phase-1 Adam step; returns the batch loss, or [loss, m1, ...] with compile(metrics=[...])."""
        self._need_softmax("train_on_batch")
        x, z = inputs
        self._check_labels(labels, len(x), "train_on_batch")
        eng = self._ensure_engine(len(x))
        return self._with_metrics(eng, eng.uresnet(x, z, labels, "step",
                                                   self._next_drop_seed() if drop_seed is None else drop_seed))

    def test_on_batch(self, inputs, labels):
        self._need_softmax("test_on_batch")
        x, z = inputs
        self._check_labels(labels, len(x), "test_on_batch")
        eng = self._ensure_engine(len(x))
        return self._with_metrics(eng, eng.uresnet(x, z, labels, "eval"))

    def _evaluate(self, x, z, labels, batch_size):
        """(sample-weighted mean phase-0 loss, the confusion matrix summed over the batches or None without metrics)"""
        eng = self._ensure_engine(min(batch_size, len(x)))
        bs = min(batch_size, eng.batch)
        tot, cm = 0.0, None
        for i in range(0, len(x), bs):
            m = min(bs, len(x) - i)
            tot += m * eng.uresnet(x[i:i + m], z[i:i + m], labels[i:i + m], "eval")
            if self._metrics:
                cm = eng.uresnet_census() if cm is None else cm + eng.uresnet_census()
        return tot / len(x), cm

    def evaluate(self, inputs, labels, batch_size=32, verbose=0):
        """Sample-weighted mean of the phase-0 loss over batches (keras Model.evaluate); with compile(metrics=[...])
        [loss, m1, ...], the metrics from the confusion matrix summed over the batches."""
        self._need_softmax("evaluate")
        x, z = inputs
        self._check_labels(labels, len(x), "evaluate")
        loss, cm = self._evaluate(x, z, labels, batch_size)
        return [loss] + self._metric_values(cm) if self._metrics else loss

    def fit(self, inputs, labels, epochs=1, batch_size=32, shuffle=True, validation_data=None, verbose=1,
            print_fn=print, augment=None, callbacks=None):
        """my_network.fit([flair, noise], onehot, epochs=1, batch_size=nb_samples, shuffle=..., validation_data=...)
        (UT:602-606).  Batches in index order (after an optional np.random shuffle, as keras does), a short last
        batch, per-epoch loss = sample-weighted mean of the batch losses; returns an object with .history.  With
        compile(metrics=[...]) each epoch also records every metric of the confusion matrix summed over its training
        batches and, with validation data, over that data (History.census keeps the tables; the progress line shows
        them).
        augment: a data.Augmenter.  Every training batch is then made by one depgan_data_augment launch: a random affine
        warp of the images (bilinear) and their labels (nearest), and a gain / offset on the intensities, drawn per
        sample from the Augmenter's own generator (np.random, and with it the shuffle, is not touched).  With
        Augmenter(elastic=..., bias=...) the same launch (depgan_data_augment_fields) also bends every sample by a
        smooth random displacement and multiplies it by a smooth random bias field, from control grids drawn per
        sample.  When the
        images (float32) and the labels (uint8 class codes, or float32 one-hot rows) are tensors on the engine's device,
        the launch also does the batch gather: it reads the epoch's order[i:i+bs] as its index and x[idx] / labels[idx]
        are never formed.  Otherwise the batch is sliced as without it, uploaded and augmented.  The noise is gathered
        as before and validation data is never augmented.  With compile(ignore_label=k),
        Augmenter(border='constant', label_fill=k) keeps the pixels a warp brings in from outside the image out of the
        loss (one-hot labels: label_fill=-1, the all-zero row).  None (the default) leaves every batch as it was.
        callbacks: a list of dep_gan_im_amd.callbacks objects (ReduceLROnPlateau, EarlyStopping, LearningRateScheduler,
        ModelCheckpoint, or anything with their hooks).  Each gets on_train_begin(), per epoch on_epoch_begin(epoch)
        and on_epoch_end(epoch, logs) with logs = the epoch's history entries plus 'lr', and on_train_end().
        history['lr'] then records the rate every epoch trained with and the progress line shows it; a callback that
        sets model.stop_training = True ends fit after that epoch.  None (the default) changes nothing."""
        self._need_softmax("fit")
        x, z = inputs
        n = len(x)
        if len(z) != n or len(labels) != n:
            raise ValueError("fit: images, noise and labels must have the same length")
        self._check_labels(labels, n, "fit")
        if validation_data is not None:
            self._check_labels(validation_data[1], len(validation_data[0][0]), "fit(validation_data)")
        eng = self._ensure_engine(min(batch_size, n))
        bs = min(batch_size, eng.batch)
        hist = {"loss": []}
        hist.update((name, []) for name in self._metrics)
        if validation_data is not None:
            hist["val_loss"] = []
            hist.update(("val_" + name, []) for name in self._metrics)
        census = {"train": [], "val": []} if self._metrics else None
        callbacks = list(callbacks) if callbacks is not None else None
        if callbacks is not None:
            hist["lr"] = []
            if self._boundary is not None:
                hist["boundary_weight"] = []
            self.stop_training = False
            for cb in callbacks:
                if hasattr(cb, "set_model"):
                    cb.set_model(self)
                cb.on_train_begin()
        if augment is not None:
            import torch
            from .data import Augmenter
            if not isinstance(augment, Augmenter):
                raise TypeError("fit: augment must be a data.Augmenter or None, got %r" % (augment,))
            # resident: the launch gathers straight from the set, no x[idx] / labels[idx] copy in front of it
            resident = (isinstance(x, torch.Tensor) and isinstance(labels, torch.Tensor) and x.device == eng.device
                        and labels.device == eng.device and x.dtype == torch.float32
                        and labels.dtype == (torch.uint8 if self._loss == "sparse_categorical_crossentropy"
                                             else torch.float32))
        for ep in range(epochs):
            for cb in callbacks or ():
                cb.on_epoch_begin(ep)
            order = np.arange(n)
            if shuffle:
                np.random.shuffle(order)
            tot, cm = 0.0, None
            for i in range(0, n, bs):
                idx = order[i:i + bs]
                if augment is None:
                    xb, lb = x[idx], labels[idx]
                elif resident:
                    xb, lb = augment(x, labels, idx, device=eng.device)
                else:
                    xb, lb = augment(x[idx], labels[idx], device=eng.device)
                tot += len(idx) * eng.uresnet(xb, z[idx], lb, "step", self._next_drop_seed())
                if self._metrics:
                    cm = eng.uresnet_census() if cm is None else cm + eng.uresnet_census()
            hist["loss"].append(tot / n)
            msg = "Epoch %d/%d - loss: %.4f" % (ep + 1, epochs, hist["loss"][-1])
            if self._metrics:
                census["train"].append(cm)
                for name, v in zip(self._metrics, self._metric_values(cm)):
                    hist[name].append(v)
                    msg += " - %s: %.4f" % (name, v)
            if validation_data is not None:
                (vx, vz), vy = validation_data
                vloss, vcm = self._evaluate(vx, vz, vy, bs)
                hist["val_loss"].append(vloss)
                msg += " - val_loss: %.4f" % hist["val_loss"][-1]
                if self._metrics:
                    census["val"].append(vcm)
                    for name, v in zip(self._metrics, self._metric_values(vcm)):
                        hist["val_" + name].append(v)
                        msg += " - val_%s: %.4f" % (name, v)
            if self._metrics and verbose:
                msg += " - census train %s" % cm.tolist() + (" val %s" % vcm.tolist() if validation_data is not None else "")
            if callbacks is not None:
                hist["lr"].append(float(self.lr))
                msg += " - lr: %.4g" % hist["lr"][-1]
                if self._boundary is not None:
                    hist["boundary_weight"].append(float(self.boundary_weight))
                    msg += " - boundary_weight: %.4g" % hist["boundary_weight"][-1]
            if verbose:
                print_fn(msg)
            if callbacks is not None:
                logs = {k: v[-1] for k, v in hist.items()}
                for cb in callbacks:
                    cb.on_epoch_end(ep, logs)
                if self.stop_training:
                    break
        for cb in callbacks or ():
            cb.on_train_end()
        return History(hist, census)

    def get_config(self):
        return {"name": self.name, "input_shape": self.input_shape, "noiseZ_shape": self.noiseZ_shape,
                "first_fm": self.first_fm, "nc_out": self.nc_out}

    def to_json(self):
        import json
        return json.dumps(self.get_config())


_DIS = [("dis_0a", 5, 1, 16), ("dis_0b", 5, 16, 16), ("dis_1a", 5, 16, 32), ("dis_1b", 5, 32, 32),
        ("dis_2", 3, 32, 64), ("dis_3", 3, 64, 64), ("dis_4", 3, 64, 128), ("dis_5", 3, 128, 128),
        ("dis_6", 3, 128, 256), ("dis_7", 3, 256, 256), ("dis_8", 3, 256, 256)]


class CriticModel(_Model):
    net = "D_y2"
    name = "Dis_C2D_FCN1"

    def _static_table(self):
        H, W, _ = self.input_shape
        T = []
        for n, k, ci, co in _DIS:
            T.extend([("conv2d_" + n + "/kernel", (k, k, ci, co), True), ("conv2d_" + n + "/bias", (co,), True)])
        T.extend([("dis_9/kernel", (1, 1, 256, 1), True), ("dis_9/bias", (1,), True),
                  ("dense_1/kernel", ((H // 16) * (W // 16), 1), True), ("dense_1/bias", (1,), True)])
        return T

    def _spec_engine(self, batch):
        H, W, _ = self.input_shape
        return Engine(batch, H, W, 1)

    def predict(self, x, batch_size=32):
        """netD.predict(images)  (GT:846-848)."""
        eng = self._ensure_engine(min(batch_size, max(1, len(x))))
        return eng.d_forward(self.net, x).cpu().numpy()


def Gen_UNet2D(input_shape, noiseZ_shape=(32, 1), first_fm=32, nc_out=1, seed=None, inference_dtype="float32"):
    return GeneratorModel(input_shape, noiseZ_shape, first_fm, nc_out, seed, inference_dtype)


def Dis_C2D_FCN1(input_shape, seed=None):
    if tuple(input_shape)[2] != 1:
        raise ValueError("Dis_C2D_FCN1 takes single-channel images (GT:513)")
    return CriticModel(input_shape, seed)
