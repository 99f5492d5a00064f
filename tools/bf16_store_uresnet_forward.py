"""DEP-UResNet predict (nc_out = 4, learning phase 0) at batch 32, 256 x 256 x 1: milliseconds per forward of
  * a plain fp32 engine (Engine(nc_out=4): fp32 pipe, direct 1x1 head, a softmax launch) -- what predict runs today,
  * the inference context (Engine(nc_out=4, bf16_mfma=True)) with fp32 activation storage (depgan_g_forward),
  * the inference context with bf16 activation storage (depgan_g_forward_bf16s),
same process, alternating blocks, device events around each block; then the head launch alone
(depgan_op_head_softmax_bf16s on a (P, 32) bf16 tensor, device events around a block of launches) and one
evaluate.predict_mean of 48 slices x 10 draws through the facade (host clock around work that ends in a synchronise) on
the plain model and on its inference copy.  Prints ONE JSON object and, with --out, writes it to a file.  Nothing is gated.

    python tools/bf16_store_uresnet_forward.py [--batch 32] [--size 256] [--reps 10] [--rounds 7] [--slices 48]
                                               [--out profiles/bf16_store_uresnet_forward.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dep_gan_im_amd as dg
from dep_gan_im_amd import _lib, evaluate


def stats(v):
    v = np.array(v)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4),
            "max_ms": round(float(v.max()), 4), "spread_ms": round(float(v.max() - v.min()), 4),
            "blocks_ms": [round(float(t), 4) for t in v]}


def timed_block(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10, help="forwards per block")
    ap.add_argument("--rounds", type=int, default=7, help="alternations (>= 5)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slices", type=int, default=48, help="slices of the predict_mean subject")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, S = a.batch, a.size
    dev = torch.device("cuda:0")
    lib = _lib.load()
    model = dg.Gen_UNet2D((S, S, 1), nc_out=4, seed=1)
    W = model.get_weights_dict()
    plain = dg.Engine(B, S, S, 1, nc_out=4, beta1=0.9, beta2=0.999)
    infer = dg.Engine(B, S, S, 1, nc_out=4, bf16_mfma=True)
    plain.set_weights("G", W)
    infer.set_weights("G", W)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(0, 1, (B, S, S, 1)).astype(np.float32)).to(dev)
    z = torch.from_numpy(rng.standard_normal((B, 32)).astype(np.float32)).to(dev)
    paths = (("fp32_engine", lambda: plain.g_forward(x, z)),
             ("inference_f32_storage", lambda: infer.g_forward(x, z, storage="float32")),
             ("inference_bf16_storage", lambda: infer.g_forward(x, z, storage="bfloat16")))
    for _ in range(a.warmup):
        for _, fn in paths:
            fn()
    torch.cuda.synchronize()
    ms = {tag: [] for tag, _ in paths}
    for r in range(max(5, a.rounds)):
        for tag, fn in (paths if r % 2 == 0 else paths[::-1]):
            ms[tag].append(timed_block(fn, a.reps))
    out = {"what": "DEP-UResNet predict forward (nc_out = 4, phase 0): fp32 engine vs the inference context on fp32 and on "
                   "bf16 activation storage", "batch": B, "size": S, "nicg": 1, "reps_per_block": a.reps,
           "blocks_per_path": max(5, a.rounds), "device": torch.cuda.get_device_name(0)}
    for tag, _ in paths:
        out[tag] = stats(ms[tag])
    out["speedup_median_vs_fp32_engine"] = round(out["fp32_engine"]["median_ms"] /
                                                 out["inference_bf16_storage"]["median_ms"], 4)
    out["speedup_median_vs_same_context_f32_storage"] = round(out["inference_f32_storage"]["median_ms"] /
                                                              out["inference_bf16_storage"]["median_ms"], 4)
    # agreement of the three paths on the timed inputs (probabilities; not a gate)
    p0, p1, p2 = (fn().double() for _, fn in paths)
    out["max_abs_diff_vs_fp32_engine"] = {"inference_f32_storage": float((p1 - p0).abs().max()),
                                          "inference_bf16_storage": float((p2 - p0).abs().max())}
    plain.close()
    infer.close()

    # the head launch alone
    Pn, Cn = B * S * S, 32
    a17 = torch.from_numpy(rng.standard_normal((Pn, Cn)).astype(np.float32)).to(torch.bfloat16).to(dev)
    wd = torch.from_numpy(W["gen_segmentation/kernel"].reshape(Cn, 4).copy()).to(dev)
    bd = torch.from_numpy(W["gen_segmentation/bias"].copy()).to(dev)
    probs = torch.empty((Pn, 4), device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def head():
        _lib.check(lib.depgan_op_head_softmax_bf16s(p(a17), Cn, p(wd), p(bd), p(probs), None, Pn, Cn, stream),
                   "depgan_op_head_softmax_bf16s")

    for _ in range(a.warmup):
        head()
    torch.cuda.synchronize()
    hb = [timed_block(head, 10 * a.reps) for _ in range(max(5, a.rounds))]
    nbytes = Pn * (2.0 * Cn + 16.0)
    out["head_softmax_launch"] = dict(stats(hb), pixels=Pn, channels=Cn, algorithmic_bytes=nbytes,
                                      implied_GB_per_s=round(nbytes / float(np.median(hb)) * 1e-6, 1))
    del a17, probs

    # one subject of the evaluation script: predict_mean of `slices` slices x 10 draws (UE:553-564) through the facade
    n = a.slices
    xs = rng.uniform(0, 1, (n, S, S, 1)).astype(np.float32)
    mask = (rng.uniform(size=(n, S, S)) > 0.2).astype(np.float32)
    fast = model.inference_copy("bfloat16")
    pm = {}
    for tag, net in (("fp32_model", model), ("inference_copy_bf16", fast)):
        evaluate.predict_mean(net, xs, n_repeat=1, mask=mask, rng=np.random.RandomState(1))   # builds the engine, warms up
        torch.cuda.synchronize()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            evaluate.predict_mean(net, xs, n_repeat=10, mask=mask, rng=np.random.RandomState(2))
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        pm[tag] = {"median_ms": round(float(np.median(t)), 2), "runs_ms": [round(v, 2) for v in t]}
    out["predict_mean"] = dict(pm, slices=n, draws=10, note="host clock, input upload and noise generation included")
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
