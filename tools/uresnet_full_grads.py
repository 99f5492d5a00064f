"""Per-tensor phase-1 gradient errors of the DEP-UResNet step at its full size (256 x 256, batch 32, drop seed 77;
tests/test_gpu_steps.py::test_config5_full_size_uresnet_batch32): HIP against the fp32 oracle and the fp32 oracle
against the fp64 oracle, all under the HIP pass's ReLU / pool / FiLM decisions.  Prints one line per tensor, worst
first, and a summary; run from the repository root on the GPU box (the fp64 oracle takes a few CPU minutes)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_masked as TM  # noqa: E402
from dep_gan_im_amd import Engine  # noqa: E402
from oracle import depgan_oracle as O  # noqa: E402


def main():
    img, B, ds = 256, 32, 77
    P = O.init_generator(33, nc_out=4, bias_std=0.05)
    x, z, lab = O.synth_uresnet_batch(34, B, img, img)
    eng = Engine(B, img, img, 1, lrG=1e-4, beta1=0.9, beta2=0.999, nc_out=4)
    eng.set_weights("G", P)
    loss = eng.uresnet(x, z, lab, "grads", drop_seed=ds)
    G = eng.get_grads("G")
    masks = TM.hip_uresnet_masks(eng, B)
    eng.close()
    l32, g32, _ = O.uresnet_grads(P, x, z, lab, drop_seed=ds, dtype=torch.float32, masks=masks)
    l64, g64, _ = O.uresnet_grads(P, x, z, lab, drop_seed=ds, dtype=torch.float64, masks=masks)
    h32, h64, o32 = TM.tensor_errors(G, g32), TM.tensor_errors(G, g64), TM.tensor_errors(g32, g64)
    print("loss: HIP %.7f  oracle fp32 %.7f  fp64 %.7f" % (loss, l32, l64))
    print("%-48s %10s %10s %10s" % ("tensor", "HIP-fp32", "HIP-fp64", "fp32-fp64"))
    for k in sorted(h32, key=lambda k: -h32[k]):
        print("%-48s %10.2e %10.2e %10.2e" % (k, h32[k], h64[k], o32[k]))
    for name, e in (("HIP vs fp32", h32), ("HIP vs fp64", h64), ("fp32 vs fp64", o32)):
        v = np.array(list(e.values()))
        print("%-13s worst %.2e  above 1e-4: %d  median %.2e" % (name, v.max(), int((v > 1e-4).sum()), np.median(v)))


if __name__ == "__main__":
    main()
