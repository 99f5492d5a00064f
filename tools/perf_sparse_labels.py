"""DEP-UResNet train_on_batch at batch 32, 256x256x1 with one-hot labels (16 bytes per pixel) or integer labels (1 byte
per pixel): the median step time of one process, as one JSON line.

usage: python tools/perf_sparse_labels.py onehot|sparse [steps=30] [warmup=5] [classes=4]

A step is timed from the call to the returned loss (the entry synchronises on the loss fetch); labels are on the device
before the clock starts, as in tools/perf_uresnet.py.  Run it several times, alternating with another build of the library
(a second tree on PYTHONPATH), and take the spread of the medians as the noise: profiles/uresnet_sparse_labels.json."""
import json
import os
import sys
import time

sys.path.insert(0, os.environ.get("DEPGAN_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dep_gan_im_amd as dg  # noqa: E402

kind = sys.argv[1] if len(sys.argv) > 1 else "onehot"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 5
Cc = int(sys.argv[4]) if len(sys.argv) > 4 else 4
if kind not in ("onehot", "sparse"):
    raise SystemExit(__doc__)
B, H = 32, 256
dev = torch.device("cuda:0")
eng = dg.Engine(B, H, H, 1, lrG=1e-4, beta1=0.9, beta2=0.999, nc_out=Cc)
rng = np.random.default_rng(0)
x = torch.from_numpy(rng.standard_normal((B, H, H, 1)).astype(np.float32)).to(dev)
z = torch.from_numpy(rng.standard_normal((B, 32, 1)).astype(np.float32)).to(dev)
codes = rng.integers(0, Cc, (B, H, H)).astype(np.uint8)
lab = torch.from_numpy(codes if kind == "sparse" else np.eye(Cc, dtype=np.float32)[codes]).to(dev)
ms = []
for i in range(warmup + steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = eng.uresnet(x, z, lab, "step", drop_seed=i + 1)
    ms.append((time.perf_counter() - t0) * 1e3)
ms = np.array(ms[warmup:])
print(json.dumps({"labels": kind, "classes": Cc, "batch": B, "image": H, "steps": steps, "warmup": warmup,
                  "label_bytes_per_pixel": int(lab.element_size() * (lab.numel() // (B * H * H))),
                  "median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
                  "max_ms": round(float(ms.max()), 3), "loss": round(float(loss), 6),
                  "library_source_hash": dg._lib.load().depgan_source_hash().decode()}))
