"""DEP-UResNet train_on_batch at batch 32, 256x256x1, 4 classes, integer labels, with the boundary loss
(depgan_uresnet_set_boundary_loss) off or on: the median step time of one process, as one JSON line.

usage: python tools/perf_uresnet_boundary.py off|on [steps=30] [warmup=5] [classes=4]

`on` adds the boundary term over the foreground classes (c_0 = 0, so three maps of the four) with weight 0.01 to the
cross-entropy: the cross-entropy kernel runs as before and four launches follow it -- the row pass and the column pass
of the signed distance maps over all 32 slices and three classes, the pass that reads p, phi, the labels and dz and
rewrites dz, and the one-block sum; `off` is the step as it was.  A step is timed from the call to the returned loss (the
entry synchronises on the loss fetch, which with the mode on also carries L_B and M); labels are on the device before the
clock starts, as in tools/perf_uresnet_dice_loss.py.  The labels are blobs on a background, as the task's are: the maps
of noise labels would be all +-1 and say nothing about the column pass.  Run it several times, alternating off, on and
another build of the library (DEPGAN_TREE names a second tree; `off` there needs no entry that tree lacks), and take the
spread of the medians as the noise: profiles/uresnet_boundary_loss.json.  The kernels' own times come from a separate
rocprofv3 --kernel-trace --stats run of `on` (bl_rows_kernel, bl_cols_kernel, bl_loss_kernel, bl_finish_kernel)."""
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
Cc = int(sys.argv[4]) if len(sys.argv) > 4 else 4
if kind not in ("off", "on"):
    raise SystemExit(__doc__)
B, H = 32, 256
dev = torch.device("cuda:0")
eng = dg.Engine(B, H, H, 1, lrG=1e-4, beta1=0.9, beta2=0.999, nc_out=Cc)
rng = np.random.default_rng(0)
x = torch.from_numpy(rng.standard_normal((B, H, H, 1)).astype(np.float32)).to(dev)
z = torch.from_numpy(rng.standard_normal((B, 32, 1)).astype(np.float32)).to(dev)
# a background with a dozen discs per slice, each of one foreground class: about 2 % foreground
codes = np.zeros((B, H, H), np.uint8)
yy, xx = np.mgrid[:H, :H]
for s in range(B):
    for _ in range(12):
        cy, cx, r = rng.integers(0, H), rng.integers(0, H), rng.uniform(2.0, 9.0)
        codes[s][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(1, Cc)
out = {"mode": kind, "classes": Cc, "batch": B, "image": H, "steps": steps, "warmup": warmup,
       "foreground_share": round(float((codes != 0).mean()), 4)}
if kind == "on":
    c = np.full(Cc, 1.0 / (Cc - 1), np.float32)
    c[0] = 0.0
    eng.set_boundary_loss(True, weight=0.01, class_coef=c, spacing=(0.9375, 0.9375))
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
    lb, M = eng.uresnet_boundary_loss()
    out["boundary_term"] = round(lb, 6)
    out["taking_part"] = M
print(json.dumps(out))
