"""Keras 2 callbacks for GeneratorModel.fit(callbacks=[...]): ReduceLROnPlateau, EarlyStopping, LearningRateScheduler
and ModelCheckpoint, with Keras 2's rules (the reference's training script carries the first two, UT:583-584).

fit calls on_train_begin(), then per epoch on_epoch_begin(epoch) and on_epoch_end(epoch, logs), then on_train_end().
`epoch` counts from 0.  `logs` holds the epoch's history entries ('loss', the compiled metrics, their 'val_' twins with
validation data) and 'lr', the rate the epoch trained with.  A callback reaches the model as self.model: it reads
model.lr, calls model.set_lr(lr) -- which takes effect at the next update (Engine.set_lr) -- and sets
model.stop_training = True to end fit after the current epoch.  Nothing here touches the GPU.
"""
from __future__ import annotations

import numpy as np

# mode='auto': a monitor with one of these in its name is a score (larger is better), anything else a loss
_MAXIMISED = ("acc", "dice", "iou")


class Callback:
    """Base class: every hook is a no-op."""

    model = None

    def set_model(self, model):
        self.model = model

    def on_train_begin(self):
        pass

    def on_epoch_begin(self, epoch):
        pass

    def on_epoch_end(self, epoch, logs):
        pass

    def on_train_end(self):
        pass


def _monitor_value(who, monitor, logs):
    if monitor not in logs:
        raise ValueError("%s: monitor %r is not in the epoch's logs; available: %s"
                         % (who, monitor, ", ".join(sorted(logs))))
    return float(logs[monitor])


def _maximise(who, monitor, mode):
    if mode not in ("auto", "min", "max"):
        raise ValueError("%s: mode must be 'auto', 'min' or 'max', got %r" % (who, mode))
    return mode == "max" or (mode == "auto" and any(k in monitor for k in _MAXIMISED))


class ReduceLROnPlateau(Callback):
    """keras.callbacks.ReduceLROnPlateau: lr <- max(lr * factor, min_lr) once the monitor has not improved by more
    than min_delta for `patience` epochs; then `cooldown` epochs during which no stagnation is counted."""

    def __init__(self, monitor="val_loss", factor=0.1, patience=10, mode="auto", min_delta=1e-4, cooldown=0, min_lr=0,
                 verbose=0):
        if not factor < 1.0:
            raise ValueError("ReduceLROnPlateau does not support a factor >= 1.0")
        self.monitor, self.factor, self.patience, self.mode = monitor, float(factor), int(patience), mode
        self.min_delta, self.cooldown, self.min_lr, self.verbose = float(min_delta), int(cooldown), float(min_lr), verbose
        self._max = _maximise("ReduceLROnPlateau", monitor, mode)
        self._reset()

    def _reset(self):
        self.best = -np.inf if self._max else np.inf
        self.cooldown_counter = 0
        self.wait = 0

    def _improved(self, current):
        return current > self.best + self.min_delta if self._max else current < self.best - self.min_delta

    def on_train_begin(self):
        self._reset()

    def on_epoch_end(self, epoch, logs):
        current = _monitor_value("ReduceLROnPlateau", self.monitor, logs)
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.wait = 0
        if self._improved(current):
            self.best = current
            self.wait = 0
        elif self.cooldown_counter <= 0:
            self.wait += 1
            if self.wait >= self.patience:
                old = float(self.model.lr)
                if old > self.min_lr:
                    new = max(old * self.factor, self.min_lr)
                    self.model.set_lr(new)
                    if self.verbose:
                        print("Epoch %05d: ReduceLROnPlateau reducing learning rate to %g." % (epoch + 1, new))
                    self.cooldown_counter = self.cooldown
                    self.wait = 0


class EarlyStopping(Callback):
    """keras.callbacks.EarlyStopping: stops once the monitor has not improved by more than min_delta on the best value
    (or on `baseline`) for `patience` epochs; restore_best_weights puts the best epoch's weights back when it stops."""

    def __init__(self, monitor="val_loss", min_delta=0, patience=0, mode="auto", baseline=None,
                 restore_best_weights=False, verbose=0):
        self.monitor, self.patience, self.mode, self.baseline = monitor, int(patience), mode, baseline
        self.min_delta, self.restore_best_weights, self.verbose = abs(float(min_delta)), bool(restore_best_weights), verbose
        self._max = _maximise("EarlyStopping", monitor, mode)
        self.wait, self.stopped_epoch, self.best_weights = 0, 0, None
        self.best = -np.inf if self._max else np.inf

    def on_train_begin(self):
        self.wait, self.stopped_epoch, self.best_weights = 0, 0, None
        if self.baseline is not None:
            self.best = float(self.baseline)
        else:
            self.best = -np.inf if self._max else np.inf

    def on_epoch_end(self, epoch, logs):
        current = _monitor_value("EarlyStopping", self.monitor, logs)
        if (current - self.min_delta > self.best) if self._max else (current + self.min_delta < self.best):
            self.best = current
            self.wait = 0
            if self.restore_best_weights:
                self.best_weights = [np.array(w) for w in self.model.get_weights()]
            return
        self.wait += 1
        if self.wait >= self.patience:
            self.stopped_epoch = epoch
            self.model.stop_training = True
            if self.restore_best_weights and self.best_weights is not None:
                self.model.set_weights(self.best_weights)

    def on_train_end(self):
        if self.stopped_epoch > 0 and self.verbose:
            print("Epoch %05d: early stopping" % (self.stopped_epoch + 1))


class LearningRateScheduler(Callback):
    """keras.callbacks.LearningRateScheduler: at the start of every epoch lr <- schedule(epoch, lr)."""

    def __init__(self, schedule, verbose=0):
        self.schedule, self.verbose = schedule, verbose

    def on_epoch_begin(self, epoch):
        lr = self.schedule(epoch, float(self.model.lr))
        if isinstance(lr, bool) or not isinstance(lr, (int, float, np.integer, np.floating)):
            raise ValueError('The output of the "schedule" function should be float.')
        self.model.set_lr(float(lr))
        if self.verbose:
            print("Epoch %05d: LearningRateScheduler setting learning rate to %g." % (epoch + 1, float(lr)))


class BoundaryWeightScheduler(Callback):
    """At the start of every epoch boundary_weight <- schedule(epoch, boundary_weight), for a model compiled with
    boundary_loss=True: the boundary term is used with a weight that starts small and rises.  fit records the weight
    every epoch trained with in history['boundary_weight']."""

    def __init__(self, schedule, verbose=0):
        self.schedule, self.verbose = schedule, verbose

    def on_epoch_begin(self, epoch):
        if self.model.boundary_weight is None:
            raise ValueError("BoundaryWeightScheduler: the model was not compiled with boundary_loss=True")
        w = self.schedule(epoch, float(self.model.boundary_weight))
        if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)):
            raise ValueError('The output of the "schedule" function should be float.')
        self.model.set_boundary_weight(float(w))
        if self.verbose:
            print("Epoch %05d: BoundaryWeightScheduler setting boundary weight to %g." % (epoch + 1, float(w)))


class ModelCheckpoint(Callback):
    """keras.callbacks.ModelCheckpoint through model.save_weights: after every epoch, or with save_best_only after the
    epochs whose monitor is the best so far.  `path` may hold {epoch} (counted from 1) and the names in logs."""

    def __init__(self, path, monitor="val_loss", save_best_only=False, mode="auto", verbose=0):
        self.path, self.monitor, self.save_best_only, self.mode, self.verbose = str(path), monitor, bool(save_best_only), mode, verbose
        self._max = _maximise("ModelCheckpoint", monitor, mode)
        self.best = -np.inf if self._max else np.inf

    def on_epoch_end(self, epoch, logs):
        path = self.path.format(epoch=epoch + 1, **logs)
        if self.save_best_only:
            current = _monitor_value("ModelCheckpoint", self.monitor, logs)
            if not (current > self.best if self._max else current < self.best):
                return
            self.best = current
        self.model.save_weights(path)
        if self.verbose:
            print("Epoch %05d: saving model to %s" % (epoch + 1, path))
