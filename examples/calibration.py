"""Can the probabilities of a DEP-UResNet be believed?  ECE, Brier score, NLL and the reliability table of one synthetic
subject before and after temperature scaling (needs a GPU).

    python examples/calibration.py [--slices 8] [--size 64] [--sharpen 3.0]

The "prediction" is an over-confident model made on purpose: logits z, labels drawn from softmax(z), and the
probabilities softmax(sharpen * z) -- so the calibrating temperature is near `sharpen` and the figures after scaling are
those of a calibrated model.  In a trained pipeline `prob` is evaluate.predict_stats(my_network, brain_flair_1tp,
...)["mean"] (or predict_mean's result) and `codes` is data.to_codes(brain_cod_2tp)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dep_gan_im_amd import evaluate  # noqa: E402


def softmax(a):
    e = np.exp(a - a.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def report(title, prob, codes):
    m = evaluate.calibration_metrics(evaluate.calibration_census(prob, codes, bins=10))
    print("%s: ece %.4f  mce %.4f  brier %.4f  nll %.4f  accuracy %.4f  mean confidence %.4f"
          % (title, m["ece"], m["mce"], m["brier"], m["nll"], m["accuracy"], m["mean_confidence"]))
    print("    class-wise ece %s" % [round(float(v), 4) for v in m["classwise_ece"]])
    for b, (cnt, acc, conf) in enumerate(zip(m["bin_count"], m["bin_accuracy"], m["bin_confidence"])):
        if cnt:
            print("    bin %2d [%.1f, %.1f): %8d pixels  accuracy %.4f  confidence %.4f" % (b, b / 10, (b + 1) / 10, cnt, acc, conf))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--sharpen", type=float, default=3.0)
    a = ap.parse_args()
    n, s = a.slices, a.size
    r = np.random.default_rng(0)
    z = 2.0 * r.standard_normal((n, s, s, 4))
    z[..., 0] += 3.0                                                          # mostly background, as a brain is
    codes = (r.random((n, s, s, 1)) > np.cumsum(softmax(z), -1)).sum(-1).clip(0, 3).astype(np.uint8)   # brain_cod_2tp
    prob = softmax(a.sharpen * z)                                             # (n, s, s, 4) float64, over-confident
    report("before", prob, codes)
    fit = evaluate.fit_temperature(prob, codes)
    print("temperature %.4f (%d device passes, converged %s, at a bound %s): nll %.4f -> %.4f"
          % (fit["T"], fit["iterations"], fit["converged"], fit["at_bound"], fit["nll_before"], fit["nll_after"]))
    report("after ", evaluate.apply_temperature(prob, fit["T"]), codes)


if __name__ == "__main__":
    main()
