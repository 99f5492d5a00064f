"""evaluate.predict_stats next to evaluate.predict_mean on one subject of 48 slices, 256x256x1, 4 classes, 10 noise
draws: the median time of one process as one JSON line, or the alternating comparison that profiles/eval_stats.json
records.

usage: python tools/perf_eval_stats.py mean|stats|tta [reps=7] [warmup=2]
       python tools/perf_eval_stats.py collect [rounds=3] [reps=7] [warmup=2] [kernel_stats_csv ...]

`mean` is predict_mean (the float64 running sum alone), `stats` is predict_stats(tta=None) -- every draw goes through
depgan_eval_accumulate_stats where `mean` runs depgan_eval_accumulate_channels, and depgan_eval_finish_stats takes the
place of depgan_eval_divide -- and `tta` is predict_stats with Augmenter(rotate=15, scale=(0.9, 1.1), shift=8,
flip_lr=True): per draw the parameter draw and its inverse on the host, two small uploads, one depgan_data_augment
launch on the input and the resampling inside the accumulate launch.  The clock runs from the call to a device
synchronise after it; the slices and the mask are on the device before it starts.  "stats_bytes" is what one
accumulate launch moves at C = 4 (prediction and mask in; two double rows, the entropy sum, one vote and the count in
and out), "finish_bytes" what the finishing launch moves.

`collect` starts `rounds` rounds of fresh child processes, mean, stats and tta in turn, and writes
profiles/eval_stats.json: every process's median, and per case the median and the spread (minimum and maximum) of those
medians.  It starts no GPU work itself.  The two kernels' own times come from a separate run under a kernel trace,

    rocprofv3 --kernel-trace --stats -d DIR -o r --output-format csv -- python tools/perf_eval_stats.py stats

(and one each of `mean` and `tta`: the kernels `stats` replaces, and the resampling instantiation) whose
DIR/r_kernel_stats.csv files `collect` folds in when they are named: calls, average time and achieved bytes per second
of eval_accumulate_stats_kernel and eval_finish_stats_kernel, of eval_accumulate_channels_kernel and
eval_divide_kernel, and of the augment_kernel launch that warps the input."""
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, CC, REPEAT = 48, 256, 4, 10
STATS_BYTES = N * H * H * (4 * CC + 4 + 2 * (16 * CC + 8 + 1 + 1))
FINISH_BYTES = N * H * H * (2 * (16 * CC + 8) + 16)


def measure(kind, reps, warmup):
    sys.path.insert(0, os.environ.get("DEPGAN_TREE") or ROOT)
    import numpy as np
    import torch

    import dep_gan_im_amd as dg
    from dep_gan_im_amd import evaluate as EV
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    net = dg.Gen_UNet2D((H, H, 1), (32, 1), 32, CC, seed=1)
    x = torch.from_numpy(rng.standard_normal((N, H, H, 1), dtype=np.float32)).to(dev)
    mask = torch.from_numpy((rng.uniform(size=(N, H, H)) > 0.3).astype(np.float32)).to(dev)
    aug = dg.data.Augmenter(rotate=15, scale=(0.9, 1.1), shift=8, flip_lr=True, seed=0) if kind == "tta" else None
    draws = np.random.RandomState(0)
    ms = []
    for _ in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "mean":
            out = EV.predict_mean(net, x, n_repeat=REPEAT, mask=mask, rng=draws)
        else:
            out = EV.predict_stats(net, x, n_repeat=REPEAT, mask=mask, rng=draws, tta=aug)["mean"]
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms[warmup:])
    return {"mode": kind, "slices": N, "image": H, "classes": CC, "n_repeat": REPEAT, "reps": reps, "warmup": warmup,
            "stats_bytes": STATS_BYTES, "finish_bytes": FINISH_BYTES, "median_ms": round(float(np.median(ms)), 3),
            "min_ms": round(float(ms.min()), 3), "max_ms": round(float(ms.max()), 3),
            "mean_of_means": float(out.mean()), "library_source_hash": dg._lib.load().depgan_source_hash().decode()}


KERNELS = (("eval_accumulate_stats_kernel", STATS_BYTES), ("eval_finish_stats_kernel", FINISH_BYTES),
           ("eval_accumulate_channels_kernel", N * H * H * (4 * CC + 4 + 16 * CC)),
           ("eval_divide_kernel", N * H * H * 16 * CC), ("augment_kernel", N * H * H * 8))


def kernel_stats(paths):
    """the evaluation kernels' rows of rocprofv3 r_kernel_stats.csv files, keyed by the traced run's directory name and
    the kernel, with bytes per second from the algorithmic bytes of one launch"""
    out = {}
    for path in paths:
        run = os.path.basename(os.path.dirname(os.path.abspath(path)))
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
        for row in rows:
            for key, nbytes in KERNELS:
                if key in row["Name"]:
                    avg = float(row["AverageNs"])
                    out["%s: %s" % (run, row["Name"])] = {
                        "calls": int(row["Calls"]), "average_us": round(avg / 1e3, 2),
                        "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2),
                        "bytes": nbytes, "tbytes_per_s": round(nbytes / avg / 1e3, 3)}
    return out


def collect(rounds, reps, warmup, stats_csvs):
    import statistics
    cases = ["mean", "stats", "tta"]
    runs = {name: [] for name in cases}
    for r in range(rounds):
        for name in cases:
            cmd = [sys.executable, os.path.abspath(__file__), name, str(reps), str(warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("round %d, %s: exit status %d\n%s" % (r, name, p.returncode, p.stderr[-2000:]))
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print("round %d %s: %s" % (r, name, runs[name][-1]["median_ms"]), flush=True)
    out = {"tool": "tools/perf_eval_stats.py collect", "rounds": rounds, "order": cases,
           "workload": "one subject: 48 slices, 256x256x1, 4 classes, n_repeat 10, mask, fp32 model",
           "tta": "Augmenter(rotate=15, scale=(0.9, 1.1), shift=8, flip_lr=True)", "runs": runs, "summary": {}}
    for name, rs in runs.items():
        med = [r["median_ms"] for r in rs]
        out["summary"][name] = {"median_of_medians_ms": round(statistics.median(med), 3), "min_ms": min(med),
                                "max_ms": max(med), "library_source_hash": rs[0]["library_source_hash"]}
    base = out["summary"]["mean"]["median_of_medians_ms"]
    for name in ("stats", "tta"):
        extra = out["summary"][name]["median_of_medians_ms"] - base
        out[name + "_minus_mean_ms"] = round(extra, 3)
        out[name + "_minus_mean_percent"] = round(100.0 * extra / base, 2)
    out["kernels"] = kernel_stats(stats_csvs) if stats_csvs else "not measured"
    path = os.path.join(ROOT, "profiles", "eval_stats.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["summary"]), json.dumps(out["kernels"]))
    return path


if __name__ == "__main__":
    a = sys.argv[1:]
    kind = a[0] if a else "mean"
    if kind == "collect":
        collect(int(a[1]) if len(a) > 1 else 3, int(a[2]) if len(a) > 2 else 7, int(a[3]) if len(a) > 3 else 2,
                a[4:])
    elif kind in ("mean", "stats", "tta"):
        print(json.dumps(measure(kind, int(a[1]) if len(a) > 1 else 7, int(a[2]) if len(a) > 2 else 2)))
    else:
        raise SystemExit(__doc__)
