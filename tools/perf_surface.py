"""evaluate.label_surface_metrics next to the host route a user had before it, on one subject of 48 slices of 256x256
with three lesion classes at a realistic density (about 0.5 % of the voxels): the median time of one process as one JSON
line, or the alternating comparison that profiles/surface_metrics.json records.

usage: python tools/perf_surface.py device|host [reps=7] [warmup=2]
       python tools/perf_surface.py collect [rounds=3] [reps=7] [warmup=2] [kernel_stats_csv ...]

Both modes start from what evaluate.uresnet_metrics leaves: the int8 label map and the float32 code volume on the
device.  `device` is label_surface_metrics(labels, code, (1, 2, 3), spacing, in_plane=True): per class two surface
masks, two exact distance maps, two sums and three sorts on the device, a handful of scalars back; the clock stops when
the Python numbers are there.  `host` copies the two maps to the host and does the same per class with
scipy.ndimage (binary_erosion, distance_transform_edt with `sampling`, np.percentile); where scipy is not importable
the mode reports {"scipy": "absent"} and no time.  The spacing is (3, 0.9375, 0.9375) mm, a WMH FLAIR protocol's.

`collect` starts `rounds` rounds of fresh child processes, device and host in turn, and writes
profiles/surface_metrics.json: every process's median, and per mode the median and the spread (minimum and maximum) of
those medians.  It starts no GPU work itself.  The kernels' own times come from a separate run under a kernel trace,

    rocprofv3 --kernel-trace --stats -d DIR -o r --output-format csv -- python tools/perf_surface.py device

whose DIR/r_kernel_stats.csv `collect` folds in when it is named: calls, average, minimum and maximum time of
surface_mask_kernel, edt_rows_kernel, the two edt_axis_kernel instantiations and the two sums kernels."""
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H = 48, 256
SPACING = (3.0, 0.9375, 0.9375)
CLASSES = (1, 2, 3)


def subject(seed=0):
    """(labels int8, code float32), both (N, H, H): ellipsoid lesions of classes 1..3, about 0.5 % of the voxels, and a
    prediction whose lesions are the true ones moved and resized by a voxel or two."""
    import numpy as np
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.indices((N, H, H), dtype=np.float32)
    code = np.zeros((N, H, H), np.float32)
    labels = np.zeros((N, H, H), np.int8)
    for _ in range(60):
        c = rng.uniform(size=3) * (N, H, H)
        r = rng.uniform(2.0, 9.0)
        k = int(rng.integers(1, 4))
        code[((zz - c[0]) * 3.2) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 < r * r] = k
        c2, r2 = c + rng.uniform(-1.5, 1.5, size=3) * (0.3, 1, 1), r + rng.uniform(-1.0, 1.0)
        labels[((zz - c2[0]) * 3.2) ** 2 + (yy - c2[1]) ** 2 + (xx - c2[2]) ** 2 < r2 * r2] = k
    return labels, code


def host_metrics(labels, code, ndimage, np):
    cross = ndimage.generate_binary_structure(3, 1)
    cross[0] = cross[2] = False                          # the 4 neighbours in the slice
    out = {}
    for k in CLASSES:
        a, b = labels == k, code == k
        sa = a & ~ndimage.binary_erosion(a, cross, border_value=0)
        sb = b & ~ndimage.binary_erosion(b, cross, border_value=0)
        if not sa.any() or not sb.any():
            out[k] = None
            continue
        s_ab = ndimage.distance_transform_edt(~sb, sampling=SPACING)[sa]
        s_ba = ndimage.distance_transform_edt(~sa, sampling=SPACING)[sb]
        out[k] = {"hd": float(max(s_ab.max(), s_ba.max())), "assd": float((s_ab.mean() + s_ba.mean()) / 2),
                  "hd95": float(max(np.percentile(s_ab, 95), np.percentile(s_ba, 95)))}
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
            out = EV.label_surface_metrics(labels, code, CLASSES, SPACING, in_plane=True)
        else:
            out = host_metrics(labels.cpu().numpy(), code.cpu().numpy(), ndimage, np)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms[warmup:])
    return {"mode": kind, "slices": N, "image": H, "classes": list(CLASSES), "spacing": list(SPACING), "reps": reps,
            "warmup": warmup, "lesion_fraction": round(float((code_np > 0).mean()), 5),
            "median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
            "max_ms": round(float(ms.max()), 3),
            "figures": {str(k): (None if v is None else {f: v[f] for f in ("hd", "hd95", "assd")})
                        for k, v in out.items()},
            "library_source_hash": dg._lib.load().depgan_source_hash().decode()}


KERNELS = ("surface_mask_kernel", "edt_rows_kernel", "edt_axis_kernel", "surface_sums_kernel",
           "surface_sums_finish_kernel")


def kernel_stats(paths):
    """the surface kernels' rows of rocprofv3 r_kernel_stats.csv files, keyed by the kernel's name"""
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
    out = {"tool": "tools/perf_surface.py collect", "rounds": rounds, "order": cases,
           "workload": "one subject: 48 slices of 256x256, classes 1..3, spacing (3, 0.9375, 0.9375), in_plane surfaces",
           "runs": runs, "summary": {}}
    for name, rs in runs.items():
        med = [r["median_ms"] for r in rs if "median_ms" in r]
        out["summary"][name] = ({"median_of_medians_ms": round(statistics.median(med), 3), "min_ms": min(med),
                                 "max_ms": max(med)} if med else "scipy absent")
    if isinstance(out["summary"]["host"], dict):
        out["host_over_device"] = round(out["summary"]["host"]["median_of_medians_ms"]
                                        / out["summary"]["device"]["median_of_medians_ms"], 2)
    out["kernels"] = kernel_stats(stats_csvs) if stats_csvs else "not measured"
    path = os.path.join(ROOT, "profiles", "surface_metrics.json")
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
