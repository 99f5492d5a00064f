"""A/B of the epilogue classes of the 5x5 kernels (depgan_set_epilogue_classes 1 against 0: the class body against the
run-time-flag body of the same kernel) on the eight (batch, shape) launches of the critics' 5x5 layers, same process,
interleaved: three rounds, each the best of 3 x 10 launches.  Per shape the kernel the model takes for it (path 9 where
the weight-stationary kernel is the default, path 1 elsewhere), forward {bias, relu} (class 1) and backward-data {}
(class 4).
usage: python tools/ab_conv5.py [--all-paths]     (--all-paths: both kernels for every shape)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from dep_gan_im_amd import _lib  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda:0")


def P(t):
    return C.c_void_p(t.data_ptr())


# (batch, size, Cin, Cout of the LAUNCH, path the model takes for it: dg_conv_igemm_ws5_supported)
SHAPES = [(96, 256, 16, 16, 9), (32, 256, 16, 16, 9), (96, 128, 32, 32, 9), (32, 128, 32, 32, 1),
          (96, 128, 16, 32, 9), (32, 128, 16, 32, 9), (96, 128, 32, 16, 1), (32, 128, 32, 16, 1)]
all_paths = "--all-paths" in sys.argv
for B, S, ci, co, default in SHAPES:
    H = W = S
    x = torch.randn(B, H, W, ci, device=dev)
    w = torch.randn(5, 5, ci, co, device=dev) * 0.05     # forward: the layer ci -> co
    wb = torch.randn(5, 5, co, ci, device=dev) * 0.05    # backward-data of the layer co -> ci: the same ci -> co launch
    b = torch.zeros(co, device=dev)
    out = torch.empty(B, H, W, co, device=dev)
    for path in ((1, 9) if all_paths else (default,)):
        for form in ("fwd", "bwd"):
            def call():
                if form == "fwd":
                    return lib.depgan_op_conv2d(P(x), P(w), P(b), P(out), B, H, W, ci, co, 5, 1, path, None)
                return lib.depgan_op_conv2d_bwd_data(P(x), P(wb), P(out), B, H, W, co, ci, 5, path, None)
            rounds = {1: [], 0: []}
            for rnd in range(3):
                for on in (1, 0):
                    assert lib.depgan_set_epilogue_classes(on) == 0
                    best = 1e30
                    for rep in range(3):
                        _lib.check(call())
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        N = 10
                        for _ in range(N):
                            call()
                        e1.record()
                        torch.cuda.synchronize()
                        best = min(best, e0.elapsed_time(e1) / N * 1e3)
                    rounds[on].append(best)
            lib.depgan_set_epilogue_classes(1)
            fl = 2.0 * B * H * W * ci * co * 25
            t1, t0 = min(rounds[1]), min(rounds[0])
            spread = max(max(rounds[p]) - min(rounds[p]) for p in (1, 0))
            print("b%d %dx%d %d->%d path %d %s: off %s us (%.3f of peak)  on %s us (%.3f)  %+.1f %%  spread %.1f us"
                  % (B, H, W, ci, co, path, form, "/".join("%.1f" % t for t in rounds[0]), fl / t0 / 1e6 / 157.3,
                     "/".join("%.1f" % t for t in rounds[1]), fl / t1 / 1e6 / 157.3, 100 * (t1 - t0) / t0, spread), flush=True)
