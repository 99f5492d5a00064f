"""DEP-UResNet training steps at batch 32, 256x256x1, 4 classes, integer labels, drawn from a slice set resident on the
device, with the batch formed by torch gathers (off), by the fused augmentation launch (on) or by that launch with an
elastic deformation and a bias field (elastic): the median step time of one process, as one JSON line.

usage: python tools/perf_uresnet_augment.py off|on|elastic|kernels [steps=30] [warmup=5] [slices=512]

A timed step forms the batch and trains on it, as GeneratorModel.fit does: `off` is x[idx], labels[idx] (two torch gather
copies, each writing the batch once) and the step; `on` is Augmenter(rotate=15, scale=(0.9, 1.1), shift=8, flip_lr=True)
called with the index -- the parameter draw on the host, two small uploads and one depgan_data_augment launch that
gathers, warps and writes the batch -- and the step.  The clock runs from before the batch is formed to the returned
loss (the entry synchronises on the loss fetch).  The launch moves 32 * 65536 * (4 + 4 + 1 + 1) bytes: image and label
in, image and label out ("augment_bytes").  Run it several times, alternating off, on and another build of the library
(DEPGAN_TREE names a second tree; `off` there needs nothing that tree lacks), and take the spread of the medians as the
noise: profiles/uresnet_augment.json.  The kernel's own time comes from a separate rocprofv3 --kernel-trace --stats run
of `on` (augment_kernel) next to `off` (the two index kernels of torch).

`elastic` is `on` with elastic=4, bias=0.2 on a 7 x 7 control grid: the host also draws 32 * 3 * 49 control values and
uploads them (18 816 bytes), and the one launch is depgan_data_augment_fields (profiles/uresnet_elastic.json).
`kernels` trains nothing: it forms `steps` batches with each of the two launches, alternating them in one process, on
the same index, rows and shape, for a rocprofv3 --kernel-trace --stats run that puts augment_fields_kernel next to
augment_kernel; its own figure is the time per launch of `steps` launches enqueued back to back between two device
events, which holds the launch rate as well as the kernel."""
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
N = int(sys.argv[4]) if len(sys.argv) > 4 else 512
if kind not in ("off", "on", "elastic", "kernels"):
    raise SystemExit(__doc__)
B, H, Cc = 32, 256, 4
dev = torch.device("cuda:0")
eng = dg.Engine(B, H, H, 1, lrG=1e-4, beta1=0.9, beta2=0.999, nc_out=Cc)
rng = np.random.default_rng(0)
x = torch.from_numpy(rng.standard_normal((N, H, H, 1), dtype=np.float32)).to(dev)
z = torch.from_numpy(rng.standard_normal((B, 32, 1)).astype(np.float32)).to(dev)
# background-dominated labels, as the task's are: class 0 on 97 % of the pixels
labels = torch.from_numpy(rng.choice(Cc, size=(N, H, H), p=[0.97] + [0.03 / (Cc - 1)] * (Cc - 1)).astype(np.uint8)).to(dev)
out = {"mode": kind, "classes": Cc, "batch": B, "image": H, "slices": N, "steps": steps, "warmup": warmup,
       "augment_bytes": B * H * H * (4 + 4 + 1 + 1)}
AFFINE = dict(rotate=15, scale=(0.9, 1.1), shift=8, flip_lr=True, seed=0)
FIELDS = dict(elastic=4, bias=0.2, field_grid=(7, 7))
aug = None                                               # `off` and `on` need nothing a tree before the fields lacks
if kind != "off":
    aug = dg.data.Augmenter(**AFFINE) if kind == "on" else dg.data.Augmenter(**AFFINE, **FIELDS)
order = np.random.RandomState(0).permutation(N)
if kind == "kernels":
    a = dg.data.Augmenter(**AFFINE, **FIELDS)
    idx = torch.from_numpy(order[:B].copy()).to(dev)
    rows = torch.from_numpy(a.draw(B, H, H)).to(dev)
    fields = torch.from_numpy(a.draw_fields(B)).to(dev)
    out.update({"field_bytes": int(fields.numel()) * 4, "grid": list(a.field_grid)})
    for i in range(warmup + steps):                      # alternating, for the kernel trace
        dg.data.augment(x, labels, rows, idx)
        dg.data.augment(x, labels, rows, idx, fields=fields)
    torch.cuda.synchronize()
    for name, kw in (("augment_kernel", {}), ("augment_fields_kernel", {"fields": fields})):
        per = []
        for rep in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(steps):
                dg.data.augment(x, labels, rows, idx, **kw)
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3 / steps)
        out[name + "_back_to_back_us"] = {"median": round(float(np.median(per)), 2), "min": round(min(per), 2),
                                          "max": round(max(per), 2)}
    out["library_source_hash"] = dg._lib.load().depgan_source_hash().decode()
    print(json.dumps(out))
    raise SystemExit(0)
ms = []
for i in range(warmup + steps):
    idx = order[(i * B) % (N - B + 1):][:B]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if aug is None:
        xb, lb = x[idx], labels[idx]
    else:
        xb, lb = aug(x, labels, idx)
    loss = eng.uresnet(xb, z, lb, "step", drop_seed=i + 1)
    ms.append((time.perf_counter() - t0) * 1e3)
ms = np.array(ms[warmup:])
out.update({"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
            "max_ms": round(float(ms.max()), 3), "loss": round(float(loss), 6),
            "library_source_hash": dg._lib.load().depgan_source_hash().decode()})
print(json.dumps(out))
