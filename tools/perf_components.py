"""evaluate.label_lesion_metrics next to the host route a user had before it, on one subject of 48 slices of 256x256
with three lesion classes at a realistic density (about 0.5 % of the voxels): the median time of one process as one JSON
line, or the alternating comparison that profiles/lesion_metrics.json records.

usage: python tools/perf_components.py device|host [reps=7] [warmup=2]
       python tools/perf_components.py collect [rounds=3] [reps=7] [warmup=2] [kernel_stats_csv ...]

Both modes start from what evaluate.uresnet_metrics leaves: the int8 label map and the float32 code volume on the
device (tools/perf_surface.py's subject).  `device` is label_lesion_metrics(labels, code, (1, 2, 3)) with the defaults
(rank 3, in the volume, no size filter): per class two labellings of six launches each and two overlap tables on the
device, six integers back; the clock stops when the Python numbers are there.  `host` copies the two maps to the host
and does the same per class with scipy.ndimage.label (26 neighbours) and two np.bincount overlaps; where scipy is not
importable the mode reports {"scipy": "absent"} and no time.

`collect` starts `rounds` rounds of fresh child processes, device and host in turn, and writes
profiles/lesion_metrics.json: every process's median, and per mode the median and the spread (minimum and maximum) of
those medians.  It starts no GPU work itself.  The kernels' own times come from a separate run under a kernel trace,

    rocprofv3 --kernel-trace --stats -d DIR -o r --output-format csv -- python tools/perf_components.py device

whose DIR/r_kernel_stats.csv `collect` folds in when it is named: calls, average, minimum and maximum time of
cc_init_kernel, the cc_merge_kernel instantiation, cc_compress_kernel, cc_scan_kernel, cc_rank_kernel,
cc_relabel_kernel and cc_overlap_kernel."""
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from perf_surface import CLASSES, H, N, subject  # noqa: E402

FIGURES = ("n_truth", "n_pred", "n_truth_detected", "n_pred_true", "voxels_truth", "voxels_pred")


def host_metrics(labels, code, ndimage, np):
    full = ndimage.generate_binary_structure(3, 3)
    out = {}
    for k in CLASSES:
        pred, truth = labels == k, code == k
        lt, nt = ndimage.label(truth, full)
        lp, npd = ndimage.label(pred, full)
        hits_t = np.bincount(lt[pred], minlength=nt + 1)[1:]
        hits_p = np.bincount(lp[truth], minlength=npd + 1)[1:]
        out[k] = {"n_truth": int(nt), "n_pred": int(npd), "n_truth_detected": int((hits_t > 0).sum()),
                  "n_pred_true": int((hits_p > 0).sum()), "voxels_truth": int(truth.sum()),
                  "voxels_pred": int(pred.sum())}
    return out


def measure(kind, reps, warmup):
    sys.path.insert(0, os.environ.get("DEPGAN_TREE") or ROOT)
    import numpy as np
    import torch

    import dep_gan_im_amd as dg
    from dep_gan_im_amd import evaluate as EV
    ndimage = None
    if kind == "host":
        try:
            from scipy import ndimage
        except ImportError:
            return {"mode": kind, "scipy": "absent"}
    dev = torch.device("cuda:0")
    lab_np, code_np = subject()
    labels, code = torch.from_numpy(lab_np).to(dev), torch.from_numpy(code_np).to(dev)
    ms, out = [], None
    for _ in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "device":
            out = EV.label_lesion_metrics(labels, code, CLASSES)
        else:
            out = host_metrics(labels.cpu().numpy(), code.cpu().numpy(), ndimage, np)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms[warmup:])
    return {"mode": kind, "slices": N, "image": H, "classes": list(CLASSES), "connectivity": 3, "reps": reps,
            "warmup": warmup, "lesion_fraction": round(float((code_np > 0).mean()), 5),
            "median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
            "max_ms": round(float(ms.max()), 3),
            "figures": {str(k): {f: int(v[f]) for f in FIGURES} for k, v in out.items()},
            "library_source_hash": dg._lib.load().depgan_source_hash().decode()}


KERNELS = ("cc_init_kernel", "cc_merge_kernel", "cc_compress_kernel", "cc_scan_kernel", "cc_rank_kernel",
           "cc_relabel_kernel", "cc_overlap_kernel")


def kernel_stats(paths):
    """the component kernels' rows of rocprofv3 r_kernel_stats.csv files, keyed by the kernel's name"""
    out = {}
    for path in paths:
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
        for row in rows:
            if any(key in row["Name"] for key in KERNELS):
                out[row["Name"]] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                    "min_us": round(float(row["MinNs"]) / 1e3, 2),
                                    "max_us": round(float(row["MaxNs"]) / 1e3, 2),
                                    "total_ms": round(float(row["TotalDurationNs"]) / 1e6, 3)}
    return out


def collect(rounds, reps, warmup, stats_csvs):
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
            print("round %d %s: %s" % (r, name, runs[name][-1].get("median_ms", "scipy absent")), flush=True)
    out = {"tool": "tools/perf_components.py collect", "rounds": rounds, "order": cases,
           "workload": "one subject: 48 slices of 256x256, classes 1..3, label_lesion_metrics defaults (rank 3, volume)",
           "runs": runs, "summary": {}}
    for name, rs in runs.items():
        med = [r["median_ms"] for r in rs if "median_ms" in r]
        out["summary"][name] = ({"median_of_medians_ms": round(statistics.median(med), 3), "min_ms": min(med),
                                 "max_ms": max(med)} if med else "scipy absent")
    if isinstance(out["summary"]["host"], dict):
        out["host_over_device"] = round(out["summary"]["host"]["median_of_medians_ms"]
                                        / out["summary"]["device"]["median_of_medians_ms"], 2)
        out["figures_agree"] = all(d["figures"] == h["figures"] for d, h in zip(runs["device"], runs["host"]))
    out["kernels"] = kernel_stats(stats_csvs) if stats_csvs else "not measured"
    path = os.path.join(ROOT, "profiles", "lesion_metrics.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["summary"]), json.dumps(out["kernels"]))
    return path


if __name__ == "__main__":
    a = sys.argv[1:]
    kind = a[0] if a else "device"
    if kind == "collect":
        collect(int(a[1]) if len(a) > 1 else 3, int(a[2]) if len(a) > 2 else 7, int(a[3]) if len(a) > 3 else 2, a[4:])
    elif kind in ("device", "host"):
        print(json.dumps(measure(kind, int(a[1]) if len(a) > 1 else 7, int(a[2]) if len(a) > 2 else 2)))
    else:
        raise SystemExit(__doc__)
