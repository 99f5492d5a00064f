"""DEP-UResNet train_on_batch at batch 32, 256x256x1, 4 classes, integer labels, with the focal mode (focal cross-entropy
and label smoothing, depgan_uresnet_set_focal) off or on: the median step time of one process, as one JSON line.

usage: python tools/perf_uresnet_focal.py off|on [steps=30] [warmup=5] [gamma=2.0] [label_smoothing=0.1]

`on` sets gamma = 2 and label smoothing 0.1 on fully labelled class codes, with no loss weights: the step then runs the
label pre-pass and the FOCAL instantiation of the softmax + cross-entropy kernel where `off` runs the plain kernel alone.
A step is timed from the call to the returned loss (the entry synchronises on the loss fetch, which with the mode on also
carries the label counts); labels are on the device before the clock starts, as in tools/perf_uresnet_loss_weights.py.
Run it several times, alternating off, on and another build of the library (DEPGAN_TREE names a second tree; `off` there
needs no entry that tree lacks), and take the spread of the medians as the noise: profiles/uresnet_focal.json.  The
kernel's own time comes from a separate run of this tool under a kernel trace (rocprofv3 --kernel-trace --stats), `on`
next to `off`: softmax_ce_kernel<4, 2, false, true, true> and label_count_kernel<4, 2> against
softmax_ce_kernel<4, 2, false, false, false>."""
import json
import os
import sys
import time

sys.path.insert(0, os.environ.get("DEPGAN_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dep_gan_im_amd as dg  # noqa: E402

kind = sys.argv[1] if len(sys.argv) > 1 else "off"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 5
gamma = float(sys.argv[4]) if len(sys.argv) > 4 else 2.0
eps = float(sys.argv[5]) if len(sys.argv) > 5 else 0.1
if kind not in ("off", "on"):
    raise SystemExit(__doc__)
B, H, Cc = 32, 256, 4
dev = torch.device("cuda:0")
eng = dg.Engine(B, H, H, 1, lrG=1e-4, beta1=0.9, beta2=0.999, nc_out=Cc)
rng = np.random.default_rng(0)
x = torch.from_numpy(rng.standard_normal((B, H, H, 1)).astype(np.float32)).to(dev)
z = torch.from_numpy(rng.standard_normal((B, 32, 1)).astype(np.float32)).to(dev)
# background-dominated labels, as the task's are: class 0 on 97 % of the pixels
codes = rng.choice(Cc, size=(B, H, H), p=[0.97] + [0.03 / (Cc - 1)] * (Cc - 1)).astype(np.uint8)
out = {"mode": kind, "labels": "codes", "classes": Cc, "batch": B, "image": H, "steps": steps, "warmup": warmup}
if kind == "on":
    eng.set_focal(gamma, eps)
    out["gamma"], out["label_smoothing"] = gamma, eps
lab = torch.from_numpy(codes).to(dev)
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
    out["den"] = eng.uresnet_label_counts()["den"]
print(json.dumps(out))
