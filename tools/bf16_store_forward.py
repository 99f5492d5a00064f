"""Generator forward of a bf16_mfma context at batch 32, 256 x 256 x 2: fp32 activation storage (depgan_g_forward, the
baseline) against bf16 activation storage (depgan_g_forward_bf16s), same process, same context, alternating blocks,
device events around each block.  Prints ONE JSON object: both medians, both spreads, the activation bytes each mode
reads and writes (computed from the layer shapes) and the implied bytes/s.

    python tools/bf16_store_forward.py [--batch 32] [--size 256] [--reps 10] [--rounds 7] [--profile-csv PREFIX]

--profile-csv PREFIX additionally writes the per-launch profile of one forward of each mode (PREFIX_f32.csv,
PREFIX_bf16s.csv: the library's own event pairs, class / label / ms / GFLOP / algorithmic MB / kernel)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dep_gan_im_amd as dg

FM = 32
# (kind, cin, cout) in units of channels, forward order (GT:398-495); pools halve the size, deconvs double it
TRUNK = [("edge", 2, FM), ("film", FM, FM), ("conv+pool", FM, FM), ("conv", FM, 2 * FM), ("film", 2 * FM, 2 * FM),
         ("conv+pool", 2 * FM, 2 * FM), ("conv", 2 * FM, 3 * FM), ("film", 3 * FM, 3 * FM), ("conv+pool", 3 * FM, 3 * FM),
         ("conv", 3 * FM, 4 * FM), ("film", 4 * FM, 4 * FM), ("conv", 4 * FM, 4 * FM), ("deconv", 4 * FM, 4 * FM),
         ("conv", 7 * FM, 3 * FM), ("film", 3 * FM, 3 * FM), ("conv", 3 * FM, 3 * FM), ("deconv", 3 * FM, 3 * FM),
         ("conv", 5 * FM, 2 * FM), ("film", 2 * FM, 2 * FM), ("conv", 2 * FM, 2 * FM), ("deconv", 2 * FM, 2 * FM),
         ("conv", 3 * FM, FM), ("film", FM, FM), ("conv", FM, FM), ("head", FM, 1)]


def activation_bytes(batch, size, nicg, elem):
    """Bytes of activations one forward reads and writes: every layer input read once (FiLM: the residual once more),
    every output written once (+ the fused pool's quarter); x and the head output are fp32 in both modes."""
    px, rd, wr = size * size, 0.0, 0.0
    for kind, ci, co in TRUNK:
        ci = nicg if kind == "edge" else ci
        ein = 4 if kind == "edge" else elem
        eout = 4 if kind == "head" else elem
        rd += px * ci * ein + (px * co * elem if kind == "film" else 0)
        opx = 4 * px if kind == "deconv" else px
        wr += opx * co * eout + (px // 4 * co * elem if kind == "conv+pool" else 0)
        if kind == "conv+pool":
            px //= 4
        if kind == "deconv":
            px *= 4
    return batch * rd, batch * wr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10, help="forwards per block")
    ap.add_argument("--rounds", type=int, default=7, help="alternations (>= 5)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-csv", default=None)
    a = ap.parse_args()
    B, S = a.batch, a.size
    dev = torch.device("cuda:0")
    eng = dg.Engine(B, S, S, 2, bf16_mfma=True)
    eng.set_weights("G", dg.Gen_UNet2D((S, S, 2), seed=1).get_weights_dict())
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(0, 1, (B, S, S, 2)).astype(np.float32)).to(dev)
    z = torch.from_numpy(rng.standard_normal((B, 32)).astype(np.float32)).to(dev)
    modes = ("float32", "bfloat16")
    for _ in range(a.warmup):
        for m in modes:
            eng.g_forward(x, z, storage=m)
    torch.cuda.synchronize()
    ms = {m: [] for m in modes}
    for r in range(max(5, a.rounds)):
        for m in (modes if r % 2 == 0 else modes[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                eng.g_forward(x, z, storage=m)
            e1.record()
            torch.cuda.synchronize()
            ms[m].append(e0.elapsed_time(e1) / a.reps)
    if a.profile_csv:
        for m, tag in zip(modes, ("f32", "bf16s")):
            eng.profile(True)
            eng.profile_reset()
            eng.g_forward(x, z, storage=m)
            torch.cuda.synchronize()
            eng.profile_dump("%s_%s.csv" % (a.profile_csv, tag))
            eng.profile(False)
    out = {"what": "generator forward, bf16_mfma context: fp32 vs bf16 activation storage", "batch": B, "size": S,
           "nicg": 2, "reps_per_block": a.reps, "blocks_per_mode": len(ms["float32"]),
           "device": torch.cuda.get_device_name(0)}
    for m, tag, elem in (("float32", "f32_storage", 4), ("bfloat16", "bf16_storage", 2)):
        v = np.array(ms[m])
        rd, wr = activation_bytes(B, S, 2, elem)
        med = float(np.median(v))
        out[tag] = {"median_ms": round(med, 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4),
                    "spread_ms": round(float(v.max() - v.min()), 4), "blocks_ms": [round(float(t), 4) for t in v],
                    "activation_bytes_read": rd, "activation_bytes_written": wr,
                    "implied_activation_GB_per_s": round((rd + wr) / med * 1e-6, 1)}
    out["speedup_median"] = round(out["f32_storage"]["median_ms"] / out["bf16_storage"]["median_ms"], 4)
    out["difference_ms"] = round(out["f32_storage"]["median_ms"] - out["bf16_storage"]["median_ms"], 4)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
