"""Generator update of a bf16_mfma context at batch 32, 256 x 256 x 2 on fp32 activation storage (mode off: the baseline)
against bf16 storage (mode on, depgan_set_g_update_storage), same process, same context, alternating blocks, device
events around each block:

    (a) depgan_g_step                                   the update alone
    (b) the canonical step: critic Y2 + critic DEM + generator update
    (c) one depgan_gen_iteration, 5 + 5 critic updates, k = 10

The forward-only passes of (b) and (c) run with depgan_set_fwd_only_storage on in BOTH modes (that mode is measured by
tools/bf16_store_train_forward.py), so the difference is the update's.
Prints ONE JSON object (and writes it to --out): per-block times, medians, spreads (max - min over the blocks: the noise
floor), the saving per workload, the activation / total algorithmic bytes of one update of each mode from
depgan_profile_read_bytes, and the acceptance rule: mode-on depgan_g_step is not slower than mode-off by more than three
block spreads.

    python tools/bf16_store_g_update.py [--batch 32] [--size 256] [--rounds 7] [--out FILE] [--mode-off-only]

--mode-off-only measures the mode-off path alone (forward-only passes on fp32 storage too) and touches no entry point
newer than depgan_gen_iteration, so it also runs on a build without either mode: the baseline's own figure."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dep_gan_im_amd as dg

WORK = (("a_g_step", 10), ("b_canonical_step", 8), ("c_gen_iteration_5_5_k10", 2))


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
    if not a.mode_off_only:
        eng.forward_only_storage = "bfloat16"

    def run(what):
        if what == "a_g_step":
            eng.generator(xb, yb, z[2], "step")
        elif what == "b_canonical_step":
            eng.critic("D_y2", yb, xb, z[0], ep[0])
            eng.critic("D_dem", yb, xb, z[1], ep[1])
            eng.generator(xb, yb, z[2], "step")
        else:
            eng.gen_iteration((x, y2, z, ep, ND), (x, y2, z, ep, ND), (xb, yb, zs))

    modes = ("float32",) if a.mode_off_only else ("float32", "bfloat16")

    def set_mode(m):
        if not a.mode_off_only:
            eng.g_update_storage = m

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

    out = {"what": "generator update, bf16_mfma context: fp32 vs bf16 activation storage (depgan_set_g_update_storage)",
           "batch": B, "size": S, "nicg": 2, "k": K, "critic_updates_per_loop": ND, "blocks_per_mode": max(5, a.rounds),
           "reps_per_block": dict(WORK), "device": torch.cuda.get_device_name(0), "mode_off_only": bool(a.mode_off_only),
           "forward_only_storage": eng.forward_only_storage if not a.mode_off_only else "float32"}
    for what, _ in WORK:
        d = {"mode_off": stat(ms[(what, "float32")])}
        if not a.mode_off_only:
            d["mode_on"] = stat(ms[(what, "bfloat16")])
            floor = max(d["mode_off"]["spread_ms"], d["mode_on"]["spread_ms"])
            save = d["mode_off"]["median_ms"] - d["mode_on"]["median_ms"]
            d.update(saving_ms=round(save, 4), noise_floor_ms=round(floor, 4),
                     mode_on_slower_by_more_than_3_spreads=bool(-save > 3 * floor),
                     improves_by_more_than_3_spreads=bool(save > 3 * floor))
        out[what] = d
    if not a.mode_off_only:
        out["accepted_g_step_not_slower"] = not out["a_g_step"]["mode_on_slower_by_more_than_3_spreads"]
        # algorithmic bytes of one depgan_g_grads of each mode, per profile class (0 conv, 1 wgrad, 2 the rest); launches
        # that declare no byte count (the fp32-staging weight gradients, the HBM-bound helpers) count as 0
        by = {}
        for m in modes:
            set_mode(m)
            eng.profile(True)
            eng.profile_reset()
            eng.generator(xb, yb, z[2], "grads")
            torch.cuda.synchronize()
            by[m] = {"bytes_class_%d" % k: eng.profile_read_bytes(k) for k in range(3)}
            by[m].update({"ms_class_%d" % k: round(eng.profile_read(k)[0], 4) for k in range(3)})
            by[m].update({"launches_class_%d" % k: eng.profile_read(k)[1] for k in range(3)})
            eng.profile(False)
        out["one_g_grads_profile"] = by
    txt = json.dumps(out)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
