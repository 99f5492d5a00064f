"""Training closures of a bf16_mfma context at batch 32, 256 x 256 x 2 with the forward-only generator passes on fp32
activation storage (mode off: the baseline) against bf16 storage (mode on, depgan_set_fwd_only_storage), same process,
same context, same weights, alternating blocks, device events around each block:

    (a) one critic update                               1 forward-only generator pass
    (b) depgan_g_eval_multi, k = 10                    10
    (c) the canonical step: critic Y2 + critic DEM + generator update      2 (of 3 generator forwards)
    (d) one depgan_gen_iteration, 5 + 5 critic updates, k = 10            20 (of 21)

and the same on a second context created with DEPGAN_BF16S_HEAD_FUSED=0 (read at create), which prices the fused head
alone.  Prints ONE JSON object (and writes it to --out): per-block times, means, medians and spreads (max - min over the
blocks: the noise floor), the saving per workload and per forward-only pass, and the two acceptance rules --
the mode is worth having if (c) and (d) improve by more than three times the larger block spread of the two modes; the
fused head stays default-on if (d) is not slower with it than without by the same rule.

    python tools/bf16_store_train_forward.py [--batch 32] [--size 256] [--rounds 7] [--out FILE] [--mode-off-only]

--mode-off-only measures the mode-off path alone on one context and touches no entry point newer than
depgan_gen_iteration, so it also runs on a build that does not have the mode: the baseline's own figure."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dep_gan_im_amd as dg

WORK = (("a_critic_update", 1, 12), ("b_g_eval_multi_k10", 10, 4), ("c_canonical_step", 2, 10), ("d_gen_iteration_5_5_k10", 20, 2))


def make_engine(B, S, head_fused):
    if not head_fused:
        os.environ["DEPGAN_BF16S_HEAD_FUSED"] = "0"
    try:
        eng = dg.Engine(B, S, S, 2, bf16_mfma=True)
    finally:
        os.environ.pop("DEPGAN_BF16S_HEAD_FUSED", None)
    eng.set_weights("G", dg.Gen_UNet2D((S, S, 2), seed=1).get_weights_dict())
    eng.set_weights("D_y2", dg.Dis_C2D_FCN1((S, S, 1), seed=2).get_weights_dict())
    eng.set_weights("D_dem", dg.Dis_C2D_FCN1((S, S, 1), seed=3).get_weights_dict())
    return eng


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

    def run(eng, what):
        if what == "a_critic_update":
            eng.critic("D_y2", yb, xb, z[0], ep[0])
        elif what == "b_g_eval_multi_k10":
            eng.generator_eval_multi(xb, yb, zs)
        elif what == "c_canonical_step":
            eng.critic("D_y2", yb, xb, z[0], ep[0])
            eng.critic("D_dem", yb, xb, z[1], ep[1])
            eng.generator(xb, yb, z[2], "step")
        else:
            eng.gen_iteration((x, y2, z, ep, ND), (x, y2, z, ep, ND), (xb, yb, zs))

    modes = ("float32",) if a.mode_off_only else ("float32", "bfloat16")
    contexts = (("head_fused", True),) if a.mode_off_only else (("head_fused", True), ("head_two_launches", False))
    engines = {tag: make_engine(B, S, fused) for tag, fused in contexts}

    def set_mode(eng, m):
        if not a.mode_off_only:
            eng.forward_only_storage = m

    for eng in engines.values():
        for _ in range(a.warmup):
            for m in modes:
                set_mode(eng, m)
                for what, _, _ in WORK:
                    run(eng, what)
    torch.cuda.synchronize()
    ms = {(tag, what, m): [] for tag in engines for what, _, _ in WORK for m in modes}
    for r in range(max(5, a.rounds)):
        for what, _, reps in WORK:
            order = [(tag, m) for tag in engines for m in modes]
            for tag, m in (order if r % 2 == 0 else order[::-1]):
                eng = engines[tag]
                set_mode(eng, m)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    run(eng, what)
                e1.record()
                torch.cuda.synchronize()
                ms[(tag, what, m)].append(e0.elapsed_time(e1) / reps)

    def stat(v):
        v = np.array(v)
        return {"mean_ms": round(float(v.mean()), 4), "median_ms": round(float(np.median(v)), 4),
                "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4),
                "spread_ms": round(float(v.max() - v.min()), 4), "blocks_ms": [round(float(t), 4) for t in v]}

    out = {"what": "training closures, bf16_mfma context: forward-only generator passes on fp32 vs bf16 activation storage",
           "batch": B, "size": S, "nicg": 2, "k": K, "critic_updates_per_loop": ND, "blocks_per_mode": max(5, a.rounds),
           "reps_per_block": {w: r for w, _, r in WORK}, "forward_only_passes": {w: n for w, n, _ in WORK},
           "device": torch.cuda.get_device_name(0), "mode_off_only": bool(a.mode_off_only)}
    for tag in engines:
        out[tag] = {}
        for what, npass, _ in WORK:
            d = {"mode_off": stat(ms[(tag, what, "float32")])}
            if not a.mode_off_only:
                d["mode_on"] = stat(ms[(tag, what, "bfloat16")])
                floor = max(d["mode_off"]["spread_ms"], d["mode_on"]["spread_ms"])
                save = d["mode_off"]["median_ms"] - d["mode_on"]["median_ms"]
                d.update(saving_ms=round(save, 4), saving_per_forward_only_pass_ms=round(save / npass, 4),
                         noise_floor_ms=round(floor, 4), improves_by_more_than_3_spreads=bool(save > 3 * floor))
            out[tag][what] = d
    if not a.mode_off_only:
        f, u = out["head_fused"], out["head_two_launches"]
        out["mode_accepted"] = bool(f["c_canonical_step"]["improves_by_more_than_3_spreads"] and
                                    f["d_gen_iteration_5_5_k10"]["improves_by_more_than_3_spreads"])
        head = {}
        for what, npass, _ in WORK:
            d = u[what]["mode_on"]["median_ms"] - f[what]["mode_on"]["median_ms"]
            floor = max(u[what]["mode_on"]["spread_ms"], f[what]["mode_on"]["spread_ms"])
            head[what] = {"fused_saves_ms": round(d, 4), "per_forward_only_pass_ms": round(d / npass, 4),
                          "noise_floor_ms": round(floor, 4), "slower_by_more_than_3_spreads": bool(-d > 3 * floor)}
        out["fused_head_vs_two_launches_mode_on"] = head
        out["fused_head_stays_default_on"] = not head["d_gen_iteration_5_5_k10"]["slower_by_more_than_3_spreads"]
    txt = json.dumps(out)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
