"""DEP-UResNet train_on_batch at batch 32, 256x256x1, 4 classes, integer labels, with the soft Dice loss
(depgan_uresnet_set_dice_loss) off or on: the median step time of one process, as one JSON line.

usage: python tools/perf_uresnet_dice_loss.py off|on [codes|onehot] [steps=30] [warmup=5] [classes=4]

`on` adds the class-form Dice (c_k = 1 / C) with weight 1 to the cross-entropy with weight 1: the cross-entropy kernel
runs as before and the three Dice launches follow it (a reduction pass over the stored probabilities and the labels, the
one-block coefficient stage, the gradient pass that reads and rewrites dz); `off` is the step as it was.  A step is timed
from the call to the returned loss (the entry synchronises on the loss fetch, which with the mode on also carries the
Dice sums); labels are on the device before the clock starts, as in tools/perf_uresnet_loss_weights.py.  Run it several
times, alternating off, on and another build of the library (DEPGAN_TREE names a second tree; `off` there needs no
entry that tree lacks), and take the spread of the medians as the noise: profiles/uresnet_dice_loss.json."""
import json
import os
import sys
import time

sys.path.insert(0, os.environ.get("DEPGAN_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dep_gan_im_amd as dg  # noqa: E402

kind = sys.argv[1] if len(sys.argv) > 1 else "off"
form = sys.argv[2] if len(sys.argv) > 2 else "codes"
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
warmup = int(sys.argv[4]) if len(sys.argv) > 4 else 5
Cc = int(sys.argv[5]) if len(sys.argv) > 5 else 4
if kind not in ("off", "on") or form not in ("codes", "onehot"):
    raise SystemExit(__doc__)
B, H = 32, 256
dev = torch.device("cuda:0")
eng = dg.Engine(B, H, H, 1, lrG=1e-4, beta1=0.9, beta2=0.999, nc_out=Cc)
rng = np.random.default_rng(0)
x = torch.from_numpy(rng.standard_normal((B, H, H, 1)).astype(np.float32)).to(dev)
z = torch.from_numpy(rng.standard_normal((B, 32, 1)).astype(np.float32)).to(dev)
# background-dominated labels, as the task's are: class 0 on 97 % of the pixels
codes = rng.choice(Cc, size=(B, H, H), p=[0.97] + [0.03 / (Cc - 1)] * (Cc - 1)).astype(np.uint8)
out = {"mode": kind, "labels": form, "classes": Cc, "batch": B, "image": H, "steps": steps, "warmup": warmup}
if kind == "on":
    eng.set_dice_loss("class", ce_weight=1.0, dice_weight=1.0)
lab = torch.from_numpy(np.eye(Cc, dtype=np.float32)[codes] if form == "onehot" else codes).to(dev)
ms = []
for i in range(warmup + steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = eng.uresnet(x, z, lab, "step", drop_seed=i + 1)
    ms.append((time.perf_counter() - t0) * 1e3)
ms = np.array(ms[warmup:])
out.update({"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
            "max_ms": round(float(ms.max()), 3), "loss": round(float(loss), 6),
            "library_source_hash": dg._lib.load().depgan_source_hash().decode()})
if kind == "on":
    s = eng.uresnet_dice_sums()
    out["dice_term"] = round(s["loss"], 6)
    out["true_pixels"] = int(s["true"].sum())
print(json.dumps(out))
