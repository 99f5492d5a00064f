"""evaluate.calibration_metrics + fit_temperature next to the host route a user had before them, on one subject of 48
slices of 256x256 with four classes and a float64 mean (what predict_mean leaves on the device), 15 bins: the median time
of one process as one JSON line, or the alternating comparison that profiles/calibration.json records.

usage: python tools/perf_calibration.py device|host [reps=5] [warmup=2]
       python tools/perf_calibration.py census uniform|skewed [calls=20]
       python tools/perf_calibration.py collect [rounds=3] [reps=5] [warmup=2] [uniform=kernel_stats.csv] [skewed=...]

`device` is calibration_metrics(calibration_census(prob, codes, 15)) and fit_temperature(prob, codes) on device tensors;
the clock stops when the Python numbers are there.  `host` copies the probabilities and the labels to the host (100 MB),
forms the same tables with NumPy (np.bincount per table; the fixed-point sums as two exact float64 bincounts of the
halves of q) and finds the temperature with evaluate.solve_temperature, the same solver, over a float64 NumPy statement
of the sums.  The subject is the skewed one: 97 % of the pixels are background at confidence >= 0.99.

`census` calls the census entry `calls` times on one label distribution, for a run under a kernel trace,

    rocprofv3 --kernel-trace --stats -d DIR -o r --output-format csv -- python tools/perf_calibration.py census skewed

whose DIR/r_kernel_stats.csv `collect` folds in when it is named: calls, average, minimum and maximum time of
cal_census_kernel and cal_census_finish_kernel per distribution, and the census launch's rate over the 33 bytes per pixel
it reads.  uniform: labels uniform over the classes, confidences uniform (a wave's lanes spread over all bins, the peel
loop makes many passes); skewed: the subject above (one or two passes per table).

`collect` starts `rounds` rounds of fresh child processes, device and host in turn, and writes
profiles/calibration.json: every process's median, and per mode the median and the spread of those medians.  It starts
no GPU work itself."""
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, CLASSES, BINS = 48, 256, 4, 15
BYTES_PER_PIXEL = CLASSES * 8 + 1
EVAL_STATS_TBPS = 6.1          # eval_accumulate_channels_kernel, profiles/eval_stats.json: the same kind of traffic


def subject(dist, np):
    """(prob (N, H, H, 4) float64, codes (N, H, H) uint8)"""
    r = np.random.default_rng(7)
    P = N * H * H
    lab = r.integers(0, CLASSES, P).astype(np.uint8)
    conf = 1.0 / CLASSES + (1 - 1.0 / CLASSES) * r.random(P)
    if dist == "skewed":
        hot = r.random(P) < 0.97
        lab[hot] = 0
        conf[hot] = 0.99 + 0.01 * r.random(P)[hot]
    top = np.where(r.random(P) < 0.85, lab, r.integers(0, CLASSES, P))
    prob = np.repeat(((1 - conf) / (CLASSES - 1))[:, None], CLASSES, 1)
    prob[np.arange(P), top] = conf
    return prob.reshape(N, H, H, CLASSES), lab.reshape(N, H, H)


def host_tables(prob, lab, np):
    """the census dict of evaluate.calibration_census, with NumPy"""
    p, tc = prob.reshape(-1, CLASSES), lab.reshape(-1).astype(np.int64)
    n = len(p)

    def table(v, hit):
        b = np.minimum(np.maximum(v * float(BINS), 0.0), float(BINS - 1)).astype(np.int64)
        q = np.rint(v * 2.0 ** 32).astype(np.int64)
        hi = np.bincount(b, weights=(q >> 16).astype(np.float64), minlength=BINS).astype(np.int64)
        lo = np.bincount(b, weights=(q & 0xFFFF).astype(np.float64), minlength=BINS).astype(np.int64)
        return (np.bincount(b, minlength=BINS), np.bincount(b, weights=hit, minlength=BINS).astype(np.int64),
                (hi << 16) + lo)

    pred = np.argmax(p, 1)
    idx = np.arange(n)
    top = table(p[idx, pred], (pred == tc).astype(np.float64))
    cls = [table(p[:, k], (tc == k).astype(np.float64)) for k in range(CLASSES)]
    r = p[idx, tc]
    onehot = np.zeros_like(p)
    onehot[idx, tc] = 1.0
    return {"top_count": top[0], "top_correct": top[1], "top_conf_q": top[2],
            "class_count": np.stack([c[0] for c in cls]), "class_pos": np.stack([c[1] for c in cls]),
            "class_prob_q": np.stack([c[2] for c in cls]), "n": n, "n_nan": 0, "n_bad": 0,
            "n_floored": int((r < 1e-7).sum()), "brier_sum": float(((p - onehot) ** 2).sum()),
            "nll_sum": float(-np.log(np.maximum(r, 1e-7)).sum()), "bins": BINS, "n_class": CLASSES, "eps": 1e-7}


def host_sums(prob, lab, np):
    p, tc = prob.reshape(-1, CLASSES), lab.reshape(-1).astype(np.int64)
    z = np.log(np.maximum(p, 1e-7))
    idx = np.arange(len(p))

    def sums(beta):
        s = beta * z
        m = s.max(1)
        e = np.exp(s - m[:, None])
        S = e.sum(1)
        pi = e / S[:, None]
        A, B = (pi * z).sum(1), (pi * z * z).sum(1)
        return (float(len(p)), float((m + np.log(S) - s[idx, tc]).sum()), float((A - z[idx, tc]).sum()),
                float((B - A * A).sum()))
    return sums


def measure(kind, reps, warmup):
    sys.path.insert(0, os.environ.get("DEPGAN_TREE") or ROOT)
    import numpy as np
    import torch

    import dep_gan_im_amd as dg
    from dep_gan_im_amd import evaluate as EV
    dev = torch.device("cuda:0")
    prob_np, lab_np = subject("skewed", np)
    prob, lab = torch.from_numpy(prob_np).to(dev), torch.from_numpy(lab_np).to(dev)
    ms, m, fit = [], None, None
    for _ in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "device":
            m = EV.calibration_metrics(EV.calibration_census(prob, lab, BINS))
            fit = EV.fit_temperature(prob, lab)
        else:
            ph, lh = prob.cpu().numpy(), lab.cpu().numpy()
            m = EV.calibration_metrics(host_tables(ph, lh, np))
            fit = EV.solve_temperature(host_sums(ph, lh, np))
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms[warmup:])
    return {"mode": kind, "slices": N, "image": H, "classes": CLASSES, "bins": BINS, "reps": reps, "warmup": warmup,
            "median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
            "max_ms": round(float(ms.max()), 3),
            "figures": {"ece": m["ece"], "mce": m["mce"], "brier": m["brier"], "nll": m["nll"], "accuracy": m["accuracy"],
                        "T": fit["T"], "nll_after": fit["nll_after"], "iterations": fit["iterations"],
                        "converged": fit["converged"]},
            "library_source_hash": dg._lib.load().depgan_source_hash().decode()}


def census_calls(dist, calls):
    sys.path.insert(0, os.environ.get("DEPGAN_TREE") or ROOT)
    import numpy as np
    import torch

    from dep_gan_im_amd import evaluate as EV
    prob_np, lab_np = subject(dist, np)
    prob, lab = torch.from_numpy(prob_np).cuda(), torch.from_numpy(lab_np).cuda()
    for _ in range(calls):
        c = EV.calibration_census(prob, lab, BINS)
    return {"mode": "census", "distribution": dist, "calls": calls, "n": c["n"],
            "top_bin_share": round(float(c["top_count"].max()) / c["n"], 4)}


KERNELS = ("cal_census_kernel", "cal_census_finish_kernel")


def kernel_stats(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for key in KERNELS:
                if key + "<" in row["Name"] or key + "(" in row["Name"] or row["Name"].endswith(key):
                    out[key] = {"name": row["Name"], "calls": int(row["Calls"]),
                                "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    if "cal_census_kernel" in out:
        k = out["cal_census_kernel"]
        k["bytes_read"] = N * H * H * BYTES_PER_PIXEL
        k["tb_per_s_at_average"] = round(k["bytes_read"] / (k["average_us"] * 1e-6) / 1e12, 3)
        k["share_of_eval_accumulate_channels_rate"] = round(k["tb_per_s_at_average"] / EVAL_STATS_TBPS, 3)
    return out


def collect(rounds, reps, warmup, named):
    import statistics
    cases = ["device", "host"]
    runs = {name: [] for name in cases}
    for r in range(rounds):
        for name in cases:
            cmd = [sys.executable, os.path.abspath(__file__), name, str(reps), str(warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit("round %d, %s: exit status %d\n%s" % (r, name, p.returncode, p.stderr[-2000:]))
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print("round %d %s: %s ms" % (r, name, runs[name][-1]["median_ms"]), flush=True)
    out = {"tool": "tools/perf_calibration.py collect", "rounds": rounds, "order": cases,
           "workload": "one subject: 48 slices of 256x256, 4 classes, float64 mean, 15 bins, 97 % background at "
                       "confidence >= 0.99: calibration_metrics(calibration_census) + fit_temperature",
           "runs": runs, "summary": {}}
    for name, rs in runs.items():
        med = [r["median_ms"] for r in rs]
        out["summary"][name] = {"median_of_medians_ms": round(statistics.median(med), 3), "min_ms": min(med),
                                "max_ms": max(med)}
    out["host_over_device"] = round(out["summary"]["host"]["median_of_medians_ms"]
                                    / out["summary"]["device"]["median_of_medians_ms"], 2)
    d, h = runs["device"][0]["figures"], runs["host"][0]["figures"]
    out["figures_agree"] = {k: abs(d[k] - h[k]) <= 1e-9 * max(1.0, abs(h[k])) for k in ("ece", "mce", "brier", "nll", "T")}
    out["census_launch"] = {"bytes_per_pixel": BYTES_PER_PIXEL, "aggregation": "ballot peel, one LDS add per distinct bin",
                            "reference_rate_tb_per_s": EVAL_STATS_TBPS}
    for item in named:
        dist, _, path = item.partition("=")
        out["census_launch"][dist] = kernel_stats(path)
    path = os.path.join(ROOT, "profiles", "calibration.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["summary"]), json.dumps(out["census_launch"]))
    return path


if __name__ == "__main__":
    a = sys.argv[1:]
    kind = a[0] if a else "device"
    if kind == "collect":
        nums = [v for v in a[1:] if "=" not in v]
        collect(int(nums[0]) if nums else 3, int(nums[1]) if len(nums) > 1 else 5, int(nums[2]) if len(nums) > 2 else 2,
                [v for v in a[1:] if "=" in v])
    elif kind in ("device", "host"):
        print(json.dumps(measure(kind, int(a[1]) if len(a) > 1 else 5, int(a[2]) if len(a) > 2 else 2)))
    elif kind == "census" and len(a) > 1 and a[1] in ("uniform", "skewed"):
        print(json.dumps(census_calls(a[1], int(a[2]) if len(a) > 2 else 20)))
    else:
        raise SystemExit(__doc__)
