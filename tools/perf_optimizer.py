"""DEP-UResNet train_on_batch at batch 32, 256x256x1, 4 classes, integer labels, with the optimiser options
(depgan_set_optimizer) off or on: the median step time of one process as one JSON line, or the alternating comparison
that profiles/optimizer_options.json records.

usage: python tools/perf_optimizer.py off|on [steps=30] [warmup=5] [clipnorm=1.0] [weight_decay=1e-4]
       python tools/perf_optimizer.py collect [rounds=5] [steps=30] [warmup=5] [parent_tree]

`on` sets clipnorm 1.0 and weight_decay 1e-4 on the generator: every update then runs the two launches of the gradient's
squared norm and the option kernel where `off` runs the plain Adam kernel alone.  A step is timed from the call to the
returned loss (the entry synchronises on the loss fetch); the inputs are on the device before the clock starts, as in
tools/perf_uresnet_focal.py.  `off` uses no entry an older build lacks, so DEPGAN_TREE may name a tree of the parent
commit with its own built library.

`collect` starts `rounds` rounds of fresh child processes, each round off, on and (with a parent tree) parent in turn,
and writes profiles/optimizer_options.json: every process's median, and per case the median and the spread (minimum
and maximum) of those medians.  "Inside the noise" is claimed only when the `on` median of medians lies inside the
spread of the parent's (of `off`'s without a parent tree).  It starts no GPU work itself.  The kernels' own times come
from a separate run under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/perf_optimizer.py on):
grad_sqnorm_partial, grad_sqnorm_final and adam_opts_kernel next to adam_kernel of an `off` run."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(kind, steps, warmup, clipnorm, weight_decay):
    sys.path.insert(0, os.environ.get("DEPGAN_TREE") or ROOT)
    import numpy as np
    import torch

    import dep_gan_im_amd as dg
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
        eng.set_optimizer("G", clipnorm=clipnorm, weight_decay=weight_decay)
        out["clipnorm"], out["weight_decay"] = clipnorm, weight_decay
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
        norm, scale = eng.grad_norm("G")
        out["last_grad_norm"], out["last_scale"] = round(norm, 6), round(scale, 6)
    return out


def collect(rounds, steps, warmup, parent_tree):
    import statistics
    cases = [("off", {}), ("on", {})] + ([("parent", {"DEPGAN_TREE": parent_tree})] if parent_tree else [])
    runs = {name: [] for name, _ in cases}
    for r in range(rounds):
        for name, env in cases:
            cmd = [sys.executable, os.path.abspath(__file__), "on" if name == "on" else "off", str(steps), str(warmup)]
            p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("round %d, %s: exit status %d\n%s" % (r, name, p.returncode, p.stderr[-2000:]))
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print("round %d %s: %s" % (r, name, runs[name][-1]["median_ms"]), flush=True)
    out = {"tool": "tools/perf_optimizer.py collect", "rounds": rounds, "order": [n for n, _ in cases],
           "workload": "DEP-UResNet train_on_batch, batch 32, 256x256x1, 4 classes, integer labels",
           "on": "clipnorm 1.0 + weight_decay 1e-4", "runs": runs, "summary": {}}
    for name, rs in runs.items():
        med = [r["median_ms"] for r in rs]
        out["summary"][name] = {"median_of_medians_ms": round(statistics.median(med), 3), "min_ms": min(med),
                                "max_ms": max(med), "library_source_hash": rs[0]["library_source_hash"]}
    base = out["summary"]["parent" if parent_tree else "off"]
    on = out["summary"]["on"]["median_of_medians_ms"]
    out["on_minus_baseline_ms"] = round(on - base["median_of_medians_ms"], 3)
    out["on_inside_baseline_spread"] = bool(base["min_ms"] <= on <= base["max_ms"])
    path = os.path.join(ROOT, "profiles", "optimizer_options.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["summary"]), out["on_minus_baseline_ms"], out["on_inside_baseline_spread"])
    return path


if __name__ == "__main__":
    a = sys.argv[1:]
    kind = a[0] if a else "off"
    if kind == "collect":
        collect(int(a[1]) if len(a) > 1 else 5, int(a[2]) if len(a) > 2 else 30, int(a[3]) if len(a) > 3 else 5,
                a[4] if len(a) > 4 else None)
    elif kind in ("off", "on"):
        print(json.dumps(measure(kind, int(a[1]) if len(a) > 1 else 30, int(a[2]) if len(a) > 2 else 5,
                                 float(a[3]) if len(a) > 3 else 1.0, float(a[4]) if len(a) > 4 else 1e-4)))
    else:
        raise SystemExit(__doc__)
