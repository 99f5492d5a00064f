"""DEP-UResNet evaluation of one synthetic subject: the reference's volumes and Dice figures, then how far the
predicted lesion boundaries lie from the true ones, and which lesions were found at all (needs a GPU).

    python examples/surface_metrics.py [--slices 8] [--size 64]

The "prediction" is the one-hot map of the true codes with its lesions moved by a pixel, so the figures are small and
known: in a trained pipeline `prob` comes from evaluate.predict_mean(my_network, brain_flair_1tp, ...)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dep_gan_im_amd import data, evaluate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--size", type=int, default=64)
    a = ap.parse_args()
    n, s = a.slices, a.size
    zz, yy, xx = np.indices((n, s, s))
    code = np.zeros((n, s, s), np.float32)                                   # brain_cod_2tp: codes 0..3
    for k, (cy, cx) in enumerate(((s // 4, s // 4), (s // 2, s // 2), (3 * s // 4, s // 3)), start=1):
        code[(yy - cy) ** 2 + (xx - cx) ** 2 + 9 * (zz - n // 2) ** 2 < (s // 10) ** 2] = k
    ones = np.ones((n, s, s), np.float32)
    prob = np.eye(4)[np.roll(code, 1, axis=2).astype(int)]                   # (n, s, s, 4) float64, lesions one pixel off
    pixdim = (0.9375, 0.9375, 3.0)                                           # loaded_data.header["pixdim"][1:4]
    m = evaluate.uresnet_metrics(prob, code, ones, code > 0, ones, code > 0, float(np.prod(pixdim)))
    surf = evaluate.label_surface_metrics(m["labels"], code, classes=(1, 2, 3), spacing=data.prepared_spacing(pixdim),
                                          in_plane=True)
    les = evaluate.label_lesion_metrics(m["labels"], code, classes=(1, 2, 3), voxel_volume=float(np.prod(pixdim)))
    print("dice 1..3: %s" % [round(d, 4) for d in m["dice"][:3]])
    for k, f in surf.items():
        print("class %d: hd %.3f mm  hd95 %.3f mm  assd %.3f mm  (%d / %d surface voxels)"
              % (k, f["hd"], f["hd95"], f["assd"], f["n_surface_a"], f["n_surface_b"]))
        g = les[k]
        print("         lesions %d true / %d predicted: recall %.3f  precision %.3f  f1 %.3f  avd %.2f %%"
              % (g["n_truth"], g["n_pred"], g["recall"], g["precision"], g["f1"], g["avd_percent"]))


if __name__ == "__main__":
    main()
