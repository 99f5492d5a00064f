"""A/B of the weight-stationary 5x5 kernel (path 9) against the workgroup-tile kernel (path 1) on the eight (batch, shape)
launches of the critics' 5x5 layers, same process, interleaved: three rounds, each the best of 3 x 10 launches.
usage: python tools/ab_ws5.py"""
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


SHAPES = [(b, s, s, ci, co) for (s, ci, co) in ((256, 16, 16), (128, 32, 32), (128, 16, 32), (128, 32, 16)) for b in (96, 32)]
for B, H, W, ci, co in SHAPES:
    x = torch.randn(B, H, W, ci, device=dev)
    w = torch.randn(5, 5, ci, co, device=dev) * 0.05
    b = torch.zeros(co, device=dev)
    out = torch.empty(B, H, W, co, device=dev)
    rounds = {1: [], 9: []}
    for rnd in range(3):
        for path in (1, 9):
            best = 1e30
            for rep in range(3):
                # (the op entry packs the weights on every call: a few microseconds on these shapes, same for both paths)
                _lib.check(lib.depgan_op_conv2d(P(x), P(w), P(b), P(out), B, H, W, ci, co, 5, 1, path, None))
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                N = 10
                for _ in range(N):
                    lib.depgan_op_conv2d(P(x), P(w), P(b), P(out), B, H, W, ci, co, 5, 1, path, None)
                e1.record()
                torch.cuda.synchronize()
                best = min(best, e0.elapsed_time(e1) / N * 1e3)
            rounds[path].append(best)
    fl = 2.0 * B * H * W * ci * co * 25
    t1, t9 = min(rounds[1]), min(rounds[9])
    spread = max(max(rounds[p]) - min(rounds[p]) for p in (1, 9))
    print("b%d %dx%d %d->%d: tile %s us (%.3f of peak)  ws5 %s us (%.3f)  %+.1f %%  spread %.1f us"
          % (B, H, W, ci, co, "/".join("%.1f" % t for t in rounds[1]), fl / t1 / 1e6 / 157.3,
             "/".join("%.1f" % t for t in rounds[9]), fl / t9 / 1e6 / 157.3, 100 * (t9 - t1) / t1, spread), flush=True)
