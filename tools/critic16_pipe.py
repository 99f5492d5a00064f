"""The critics' 16-channel 5x5 launches of a bf16_mfma context at batch 32, 256 x 256 x 2 on the fp32 matrix pipe (mode off:
the baseline) against the bf16 pipe (mode on, depgan_set_critic16_pipe), same process, same context, alternating blocks,
device events around each block:

    (b) the canonical step: critic Y2 + critic DEM + generator update
    (c) one depgan_gen_iteration of the reference schedule, 5 + 5 critic updates, k = 10

Both storage options (depgan_set_fwd_only_storage, depgan_set_g_update_storage) are on in BOTH modes, so the difference
is the four launches'.  Prints ONE JSON object (and writes it to --out): per-block times, medians, spreads (max - min over
the blocks: the noise floor), the saving per workload, and from depgan_profile_dump of one canonical step per mode the
time of every affected launch shape (label, kernel, launches, total ms) with their share of the step's launches.

    python tools/critic16_pipe.py [--batch 32] [--size 256] [--rounds 7] [--out FILE] [--mode-off-only]

--mode-off-only measures the mode-off path alone and touches no entry point newer than depgan_set_g_update_storage, so
it also runs on a build without the mode: the parent's own figure, which mode off of this build is compared with."""
import argparse
import csv
import json
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dep_gan_im_amd as dg

WORK = (("b_canonical_step", 8), ("c_gen_iteration_5_5_k10", 2))
AFFECTED = re.compile(r"^conv(\(bf16\))? k5 b\d+ \d+x\d+ (16->16|32->16)$")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7, help="alternations (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode-off-only", action="store_true")
    a = ap.parse_args()
    B, S, K, ND = a.batch, a.size, 10, 5
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(0, 1, (ND * B, S, S, 2)).astype(np.float32)).to(dev)
    y2 = torch.from_numpy(rng.uniform(0, 1, (ND * B, S, S, 1)).astype(np.float32)).to(dev)
    z = torch.from_numpy(rng.standard_normal((ND, B, 32)).astype(np.float32)).to(dev)
    ep = torch.from_numpy(rng.uniform(0, 1, (ND, B)).astype(np.float32)).to(dev)
    zs = torch.from_numpy(rng.standard_normal((K, B, 32)).astype(np.float32)).to(dev)
    xb, yb = x[:B], y2[:B]
    eng = dg.Engine(B, S, S, 2, bf16_mfma=True)
    eng.set_weights("G", dg.Gen_UNet2D((S, S, 2), seed=1).get_weights_dict())
    eng.set_weights("D_y2", dg.Dis_C2D_FCN1((S, S, 1), seed=2).get_weights_dict())
    eng.set_weights("D_dem", dg.Dis_C2D_FCN1((S, S, 1), seed=3).get_weights_dict())
    eng.forward_only_storage = "bfloat16"
    eng.g_update_storage = "bfloat16"

    def run(what):
        if what == "b_canonical_step":
            eng.critic("D_y2", yb, xb, z[0], ep[0])
            eng.critic("D_dem", yb, xb, z[1], ep[1])
            eng.generator(xb, yb, z[2], "step")
        else:
            eng.gen_iteration((x, y2, z, ep, ND), (x, y2, z, ep, ND), (xb, yb, zs))

    modes = ("float32",) if a.mode_off_only else ("float32", "bfloat16")

    def set_mode(m):
        if not a.mode_off_only:
            eng.critic16_pipe = m

    for _ in range(a.warmup):
        for m in modes:
            set_mode(m)
            for what, _ in WORK:
                run(what)
    torch.cuda.synchronize()
    ms = {(what, m): [] for what, _ in WORK for m in modes}
    for r in range(max(5, a.rounds)):
        for what, reps in WORK:
            for m in (modes if r % 2 == 0 else modes[::-1]):
                set_mode(m)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    run(what)
                e1.record()
                torch.cuda.synchronize()
                ms[(what, m)].append(e0.elapsed_time(e1) / reps)

    def stat(v):
        v = np.array(v)
        return {"mean_ms": round(float(v.mean()), 4), "median_ms": round(float(np.median(v)), 4),
                "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4),
                "spread_ms": round(float(v.max() - v.min()), 4), "blocks_ms": [round(float(t), 4) for t in v]}

    out = {"what": "critics' 16-channel 5x5 launches, bf16_mfma context: fp32 vs bf16 matrix pipe (depgan_set_critic16_pipe)",
           "batch": B, "size": S, "nicg": 2, "k": K, "critic_updates_per_loop": ND, "blocks_per_mode": max(5, a.rounds),
           "reps_per_block": dict(WORK), "device": torch.cuda.get_device_name(0), "mode_off_only": bool(a.mode_off_only),
           "forward_only_storage": eng.forward_only_storage, "g_update_storage": eng.g_update_storage,
           "n16_variant_env": os.environ.get("DEPGAN_BF16_N16_VARIANT", "")}
    for what, _ in WORK:
        d = {"mode_off": stat(ms[(what, "float32")])}
        if not a.mode_off_only:
            d["mode_on"] = stat(ms[(what, "bfloat16")])
            floor = max(d["mode_off"]["spread_ms"], d["mode_on"]["spread_ms"])
            save = d["mode_off"]["median_ms"] - d["mode_on"]["median_ms"]
            d.update(saving_ms=round(save, 4), noise_floor_ms=round(floor, 4),
                     improves_by_more_than_the_spread=bool(save > floor),
                     mode_on_slower_by_more_than_the_spread=bool(-save > floor))
        out[what] = d
    # per-launch times of one canonical step per mode (device events around every launch: the launches serialise, so
    # the sum is longer than the step's wall time; shares are of that sum)
    prof = {}
    for m in modes:
        set_mode(m)
        run("b_canonical_step")
        eng.profile(True)
        eng.profile_reset()
        run("b_canonical_step")
        torch.cuda.synchronize()
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "profile.csv")
            eng.profile_dump(path)
            with open(path, newline="") as fh:
                rows = list(csv.DictReader(fh))
        eng.profile(False)
        eng.profile_reset()
        total = sum(float(r["ms"]) for r in rows)
        shapes = {}
        for r in rows:
            if AFFECTED.match(r["label"]):
                s = shapes.setdefault(r["label"], {"kernel": r["kernel"], "launches": 0, "ms": 0.0, "mbytes": 0.0})
                s["launches"] += 1
                s["ms"] += float(r["ms"])
                s["mbytes"] += float(r["mbytes"])
        for s in shapes.values():
            s["ms"] = round(s["ms"], 4)
            s["ms_per_launch"] = round(s["ms"] / s["launches"], 4)
            s["mbytes"] = round(s["mbytes"], 1)
        aff = sum(s["ms"] for s in shapes.values())
        prof[m] = {"sum_of_launches_ms": round(total, 4), "affected_ms": round(aff, 4),
                   "affected_share": round(aff / total, 4), "shapes": shapes}
    out["one_canonical_step_profile"] = prof
    txt = json.dumps(out)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
