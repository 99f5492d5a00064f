"""GPU parity, operator level, of the two-critic WGAN-GP step's HBM-bound kernels (csrc/ops.hip) and the noise MLP
(csrc/noise.hip) through the depgan_op_* entries: pooling backward, generator head, critic tail, column sums, critic
inputs, gradient penalty, generator-loss pieces, FiLM backward, the batched BatchNorm jobs, the noise MLP, the best-of-k
noise choice and the bf16 weight rounding.  Each is checked against a float64 restatement of the operation
(oracle/manual.py where it states it: first_argmax_idx, unpool, gather_pool, d_gp_grads, noise_fwd_store, noise_bwd),
at the launch forms the whole-model tests never reach: the 8192- and 2048-block grid caps with ragged tails, both
address paths of the column sums, HW not a multiple of 64, C that does not divide the 256 threads, exact ties and
exact threshold decisions.  Elementwise kernels are compared bitwise with a float32 replay; reductions against
k * 2^-24 * sum|terms| with k written in the test (each case prints its measured error in those units).  Every call
runs twice into NaN-filled outputs and must repeat bit for bit: none of these kernels uses atomics."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import depgan_oracle as O
from oracle import manual as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
NAN = float("nan")


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint8)


def twice(call, outs):
    """Run call() twice, each time into outputs refilled with NaN; both runs must agree bit for bit."""
    res = []
    for _ in range(2):
        for o in outs:
            o.fill_(NAN)
        call()
        torch.cuda.synchronize()
        res.append([host(o) for o in outs])
    for a, b in zip(*res):
        assert np.array_equal(bits(a), bits(b)), "second call differs"
    return res[0]


def ok(rc, what):
    from dep_gan_im_amd import _lib
    _lib.check(rc, what)


def bounded(name, got, ref, mag, k):
    """|got - ref| <= k * 2^-24 * mag elementwise (mag: the sum of the absolute terms); prints the worst ratio."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    mag = np.broadcast_to(np.asarray(mag, np.float64), ref.shape)
    assert np.all(np.isfinite(got)), name + ": non-finite output"
    err = np.abs(got - ref)
    live = mag > 0
    assert np.all(err[~live] == 0), name + ": error on an all-zero reduction"
    worst = float((err[live] / mag[live]).max() / U) if live.any() else 0.0
    print("%s: worst error %.3g x 2^-24 x sum|terms| (bound %d)" % (name, worst, k))
    assert worst <= k, (name, worst)
    return worst


def exact(name, got, ref):
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float32)
    same = bits(got) == bits(ref)
    assert same.all(), "%s: %d of %d differ, first at %s: %r vs %r" % (
        name, (~same).sum(), same.size, np.argwhere(~same)[0], got.flat[np.flatnonzero(~same)[0]],
        ref.flat[np.flatnonzero(~same)[0]])


def nhwc(rng, shape, mode, fill=None):
    """(B,H,W,C) float32 values and a device buffer holding them: 'dense', 'slice' (channels [4, 4+C) of a C+8 wide
    buffer: FLAT address path) or 'gap' (dense rows, sample stride larger than H*sY: the non-FLAT path).
    Returns (x, buffer, view tensor, (sB, sY, sX))."""
    B, H, W, Cc = shape
    x = rng.standard_normal(shape, dtype=np.float32) if fill is None else fill
    if mode == "dense":
        buf = dev(x)
        return x, buf, buf, (H * W * Cc, W * Cc, Cc)
    if mode == "slice":
        buf = torch.full((B, H, W, Cc + 8), NAN, device=DEV)
        buf[..., 4:4 + Cc] = dev(x)
        return x, buf, buf[..., 4:], (H * W * (Cc + 8), W * (Cc + 8), Cc + 8)
    assert mode == "gap"
    buf = torch.full((B, H * W * Cc + 8 * Cc), NAN, device=DEV)
    buf[:, :H * W * Cc] = dev(x.reshape(B, -1))
    return x, buf, buf, (H * W * Cc + 8 * Cc, W * Cc, Cc)


def strides(t):
    return tuple(int(s) for s in t.stride()[:3])


# ---------------------------------------------------------------------------------------------------------------------
# pooling backward: bitwise against the fp32 restatement (select, add one skip term, mask)
# ---------------------------------------------------------------------------------------------------------------------
POOL_CASES = [  # B, Ho, Wo, C, skip, sliced
    (2, 3, 4, 4, True, False),
    (2, 3, 4, 4, False, True),
    (3, 5, 7, 12, True, True),
    (1, 8, 8, 64, False, False),
    (1, 400, 200, 108, True, True),      # 2,160,000 lane tasks: above the 8192 x 256 grid stride
]


def _pool_input(rng, B, Ho, Wo, Cc):
    """values from a small set (exact ties, zeros, negatives), all-zero and all-negative windows, and two equal positive
    maxima in each of the six position pairs of a window"""
    a = rng.integers(-2, 3, size=(B, 2 * Ho, 2 * Wo, Cc)).astype(np.float32) * np.float32(0.75)
    w = a.reshape(B, Ho, 2, Wo, 2, Cc)
    w[0, 0, :, 0, :, 0] = 0.0                                   # all zero (post-ReLU)
    w[-1, -1, :, -1, :, -1] = -1.5                              # all negative: masked everywhere
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    flat = w.transpose(0, 1, 3, 5, 2, 4).reshape(-1, 4)         # windows (b, y, x, c) x position (dy, dx) -- a view
    for k, (i, j) in enumerate(pairs):
        row = flat[Cc + k] if Cc + k < flat.shape[0] else flat[k]
        row[:] = 0.5
        row[i] = row[j] = 2.0
    w[...] = flat.reshape(B, Ho, Wo, Cc, 2, 2).transpose(0, 1, 4, 2, 5, 3)
    return a


@pytest.mark.parametrize("case", POOL_CASES)
def test_unpool_mask_and_gather_pool_bitwise(lib, case):
    B, Ho, Wo, Cc, use_skip, sliced = case
    rng = np.random.default_rng(Ho * 31 + Cc)
    mode = "slice" if sliced else "dense"
    a = _pool_input(rng, B, Ho, Wo, Cc)
    _, abuf, av, ast = nhwc(rng, (B, 2 * Ho, 2 * Wo, Cc), mode, fill=a)
    d = rng.standard_normal((B, Ho, Wo, Cc), dtype=np.float32)
    dd = dev(d)
    skip = rng.standard_normal(a.shape, dtype=np.float32) if use_skip else None
    sbuf = sv = None
    sst = (0, 0, 0)
    if use_skip:
        _, sbuf, sv, sst = nhwc(rng, a.shape, mode, fill=skip)
    obuf = torch.empty((B, 2 * Ho, 2 * Wo, Cc + (8 if sliced else 0)), device=DEV)
    ov = obuf[..., 4:4 + Cc] if sliced else obuf
    (out,) = twice(lambda: ok(lib.depgan_op_unpool_mask(P(dd), *strides(dd), P(av), *ast, P(sv), *sst, P(ov),
                                                        *strides(obuf), B, Ho, Wo, Cc, None), "unpool_mask"), [obuf])
    if sliced:
        assert np.isnan(out[..., :4]).all() and np.isnan(out[..., 4 + Cc:]).all()
        out = out[..., 4:4 + Cc]
    a_nchw = torch.from_numpy(a.transpose(0, 3, 1, 2).copy())
    idx = torch.from_numpy(M.first_argmax_idx(a_nchw.numpy()))
    sel = M.unpool(torch.from_numpy(d.transpose(0, 3, 1, 2).copy()), idx, a_nchw.shape[2:]).numpy().transpose(0, 2, 3, 1)
    v = sel if skip is None else skip + sel          # + 0 off the arg-max, exactly as the kernel adds
    exact("unpool_mask", out, np.where(a > 0, v, np.float32(0)))

    u = rng.standard_normal(a.shape, dtype=np.float32)
    _, ubuf, uv, ust = nhwc(rng, a.shape, mode, fill=u)
    gbuf = torch.empty((B, Ho, Wo, Cc), device=DEV)
    (g,) = twice(lambda: ok(lib.depgan_op_gather_pool(P(uv), *ust, P(av), *ast, P(gbuf), *strides(gbuf), B, Ho, Wo, Cc,
                                                      None), "gather_pool"), [gbuf])
    ref = M.gather_pool(torch.from_numpy(u.transpose(0, 3, 1, 2).copy()), idx).numpy().transpose(0, 2, 3, 1)
    exact("gather_pool", g, ref)


# ---------------------------------------------------------------------------------------------------------------------
# generator head
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [4, 8, 32, 256])
@pytest.mark.parametrize("tanh_act", [0, 1])
def test_head_forward_and_backward(lib, Cc, tanh_act):
    rng = np.random.default_rng(Cc + 7 * tanh_act)
    Pn = 1000 + 37                                   # not a multiple of 64 / LP for any C
    a = np.maximum(rng.standard_normal((Pn, Cc), dtype=np.float32), 0) * np.float32(0.3)
    w = rng.standard_normal(Cc, dtype=np.float32)
    b = np.float32([0.1])
    ad, wd_, bd = dev(a), dev(w), dev(b)
    out = torch.empty(Pn, device=DEV)
    (got,) = twice(lambda: ok(lib.depgan_op_head(0, P(ad), P(wd_), P(bd), None, P(out), Pn, Cc, tanh_act, None),
                              "head fwd"), [out])
    pre = a.astype(np.float64) @ w.astype(np.float64) + float(b[0])
    mag = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)) + abs(float(b[0]))
    # the lane products, a shuffle tree over C/4 lanes and the bias: at most 4 + log2(C/4) + 1 roundings per term;
    # tanhf adds a few ulp of its result
    ref = np.tanh(pre) if tanh_act else pre
    bounded("head fwd C=%d tanh=%d" % (Cc, tanh_act), got, ref, mag + 4 * np.abs(ref), 16)

    dpre = rng.standard_normal(Pn, dtype=np.float32)
    dp = dev(dpre)
    dz = torch.empty(Pn, Cc, device=DEV)
    (gz,) = twice(lambda: ok(lib.depgan_op_head(1, P(ad), P(wd_), None, P(dp), P(dz), Pn, Cc, 0, None), "head bwd"),
                  [dz])
    exact("head bwd", gz, np.where(a > 0, dpre[:, None] * w[None, :], np.float32(0)))


def test_head_refuses_unsupported_widths(lib):
    a = torch.zeros(64, 260, device=DEV)
    w = torch.zeros(260, device=DEV)
    out = torch.zeros(64, device=DEV)
    for Cc in (12, 260):
        assert lib.depgan_op_head(0, P(a), P(w), P(w), None, P(out), 64, Cc, 1, None) == 1
        assert b"power of two" in lib.depgan_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# critic tail
# ---------------------------------------------------------------------------------------------------------------------
TAIL_CASES = [(Cc, HW) for Cc in (4, 100, 256) for HW in (1, 16, 17, 256)]


@pytest.mark.parametrize("Cc,HW", TAIL_CASES)
def test_critic_tail(lib, Cc, HW):
    rng = np.random.default_rng(Cc * 1000 + HW)
    B = 3
    w9 = rng.standard_normal(Cc, dtype=np.float32)
    wd = rng.standard_normal(HW, dtype=np.float32)
    b9, bd = np.float32([0.2]), np.float32([-0.3])
    w9d, wdd, b9d, bdd = dev(w9), dev(wd), dev(b9), dev(bd)
    for N, per, coefs in ((2 * B, B, np.float32([0.7, -1.3])), (B, B, np.float32([-0.45]))):
        a = np.maximum(rng.standard_normal((N, HW, Cc), dtype=np.float32), 0)
        ad = dev(a)
        t9 = torch.empty(N, HW, device=DEV)
        out = torch.empty(N, device=DEV)
        gt9, gout = twice(lambda: ok(lib.depgan_op_critic_tail_fwd(P(ad), P(w9d), P(b9d), P(wdd), P(bdd), P(t9), P(out),
                                                                   N, HW, Cc, None), "tail fwd"), [t9, out])
        a64 = a.astype(np.float64)
        rt9 = a64 @ w9 + float(b9[0])
        mt9 = np.abs(a64) @ np.abs(w9.astype(np.float64)) + abs(float(b9[0]))
        bounded("tail t9 C=%d HW=%d" % (Cc, HW), gt9, rt9, mt9, 16)
        bounded("tail out C=%d HW=%d N=%d" % (Cc, HW, N), gout, rt9 @ wd + float(bd[0]),
                mt9 @ np.abs(wd.astype(np.float64)) + abs(float(bd[0])), 16)

        cd = dev(coefs)
        dz = torch.empty(N, HW, Cc, device=DEV)
        (gdz,) = twice(lambda: ok(lib.depgan_op_critic_tail_bwd(P(ad), P(w9d), P(wdd), P(cd), per, P(dz), N, HW, Cc,
                                                                None), "tail bwd"), [dz])
        k = coefs[np.arange(N) // per][:, None] * wd[None, :]
        exact("tail bwd N=%d" % N, gdz, np.where(a > 0, k[:, :, None] * w9[None, None, :], np.float32(0)))

        src = rng.standard_normal((N, HW, Cc), dtype=np.float32)
        sd = dev(src)
        cn = coefs[np.arange(N) // per].astype(np.float64)
        T = cn[:, None, None] * src.astype(np.float64)
        Tm = np.abs(cn)[:, None, None] * np.abs(src.astype(np.float64))
        rw9, mw9 = np.einsum("npc,p->c", T, wd), np.einsum("npc,p->c", Tm, np.abs(wd))
        rwd, mwd = np.einsum("npc,c->p", T, w9), np.einsum("npc,c->p", Tm, np.abs(w9))
        csum = float(sum(float(coefs[g]) * min(per, N - g * per) for g in range(len(coefs))))
        for add_bias in (0, 1):
            for acc in (0, 1):
                start = [rng.standard_normal(n, dtype=np.float32) for n in (Cc, 1, HW, 1)]
                outs = [torch.empty(len(s), device=DEV) for s in start]

                def run():
                    if acc:
                        for o, s in zip(outs, start):
                            o.copy_(dev(s))
                    ok(lib.depgan_op_critic_tail_wgrad(P(sd), P(w9d), P(b9d), P(wdd), P(cd), per, add_bias, acc,
                                                       *[P(o) for o in outs], N, HW, Cc, 0, None), "tail wgrad")
                res = []
                for _ in range(2):
                    for o in outs:
                        o.fill_(NAN)
                    run()
                    torch.cuda.synchronize()
                    res.append([host(o) for o in outs])
                assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(*res))
                dw9, db9, dwd, dbd = res[0]
                s0 = [s.astype(np.float64) if acc else 0.0 for s in start]
                tag = "tail wgrad C=%d HW=%d N=%d bias=%d acc=%d" % (Cc, HW, N, add_bias, acc)
                bounded(tag + " dw9", dw9, rw9 + s0[0], mw9 + np.abs(s0[0]), 16)
                bdw = float(b9[0]) * csum if add_bias else 0.0
                cabs = float(np.abs(cn).sum())
                bounded(tag + " dwd", dwd, rwd + bdw + s0[2], mwd + abs(float(b9[0])) * cabs + np.abs(s0[2]), 16)
                if add_bias:
                    wsum = float(np.sum(wd.astype(np.float64)))
                    bounded(tag + " db9", db9, csum * wsum + s0[1], cabs * np.abs(wd).sum() + np.abs(s0[1]), 16)
                    bounded(tag + " dbd", dbd, csum + s0[3], cabs + np.abs(s0[3]), 8)
                else:                        # left alone: NaN as filled, or the starting values
                    for got_, st_ in ((db9, start[1]), (dbd, start[3])):
                        assert np.array_equal(bits(got_), bits(st_)) if acc else np.isnan(got_).all()


def test_critic_tail_bias_gradients_cancel_exactly(lib):
    """coefs = (+1/B, -1/B) over N = 2B: the exact db9 and dbd are zero; so must the kernel's be, to the rounding of
    the largest entry (the mean of the two critic outputs, GT:539-541)."""
    B, HW, Cc = 32, 256, 256
    rng = np.random.default_rng(5)
    src = dev(rng.standard_normal((2 * B, HW, Cc), dtype=np.float32))
    w9, wd, b9 = (dev(rng.standard_normal(n, dtype=np.float32)) for n in (Cc, HW, 1))
    coefs = dev(np.float32([1.0 / B, -1.0 / B]))
    outs = [torch.empty(n, device=DEV) for n in (Cc, 1, HW, 1)]
    dw9, db9, dwd, dbd = twice(lambda: ok(lib.depgan_op_critic_tail_wgrad(P(src), P(w9), P(b9), P(wd), P(coefs), B, 1,
                                                                          0, *[P(o) for o in outs], 2 * B, HW, Cc, 0,
                                                                          None), "tail wgrad"), outs)
    scale = float(np.abs(host(wd)).sum()) * 2.0          # |coef| * B * sum|wd| per critic half
    print("tail bias cancellation: db9 %.3g, dbd %.3g" % (db9[0], dbd[0]))
    assert abs(db9[0]) <= 2 * U * scale and abs(dbd[0]) <= 2 * U * 2.0


# ---------------------------------------------------------------------------------------------------------------------
# column sums and the flat sum
# ---------------------------------------------------------------------------------------------------------------------
def colsum_grid(npix):
    nb = max(1, min((npix + 255) // 256, 2048))
    ppb = (npix + nb - 1) // nb
    return (npix + ppb - 1) // ppb, ppb


COLSUM_CASES = [  # B, H, W, C, mode
    (1, 10, 10, 4, "dense"),              # one block, fewer pixels than the 256 / LP per pass
    (1, 10, 10, 12, "gap"),
    (3, 37, 41, 48, "slice"),             # 18 blocks of 253 pixels, the last 247
    (3, 37, 41, 12, "gap"),
    (1, 1, 524289, 48, "slice"),          # the 2048-block cap: 2041 blocks of 257 pixels, the last 25
    (1, 1, 524289, 256, "dense"),
    (1, 1, 524289, 4, "gap"),
    (32, 256, 256, 4, "dense"),           # the model's full size: 2048 blocks of 1024 pixels
    (32, 256, 256, 12, "slice"),
    (32, 256, 256, 4, "gap"),
]


def test_colsum_case_table_covers_every_grid_form():
    forms = set()
    for B, H, W, Cc, mode in COLSUM_CASES:
        nb, ppb = colsum_grid(B * H * W)
        forms.add(("one" if nb == 1 else "cap" if nb * ppb >= 2048 * 256 else "ragged") + "/" + mode)
    assert {"one/dense", "one/gap", "ragged/slice", "ragged/gap", "cap/slice", "cap/dense", "cap/gap"} <= forms
    assert colsum_grid(524289) == (2041, 257) and colsum_grid(32 * 256 * 256) == (2048, 1024)


def _colsum_call(lib, v, st, shape, scale=None, out=None, raw=None, acc=0, rowmul=None, cap=0):
    B, H, W, Cc = shape
    return lib.depgan_op_colsum(P(v), *st, B, H, W, Cc, P(scale), P(out), P(raw), acc, P(rowmul), cap, None)


@pytest.mark.parametrize("case", COLSUM_CASES, ids=lambda c: "%dx%dx%dx%d_%s" % c)
def test_colsum_and_rowmul(lib, case):
    B, H, W, Cc, mode = case
    shape = (B, H, W, Cc)
    npix = B * H * W
    rng = np.random.default_rng(npix + Cc)
    # 1) small integers: every partial sum is exact in fp32 whatever the order, so the result must be the exact sum --
    #    one dropped or doubled pixel anywhere shows
    xi = rng.integers(0, 4, size=shape).astype(np.float32)
    _, buf, v, st = nhwc(rng, shape, mode, fill=xi)
    scale = rng.standard_normal(Cc, dtype=np.float32)
    sc = dev(scale)
    out, raw = torch.empty(Cc, device=DEV), torch.empty(Cc, device=DEV)
    go, gr = twice(lambda: ok(_colsum_call(lib, v, st, shape, sc, out, raw), "colsum"), [out, raw])
    tot = xi.reshape(-1, Cc).astype(np.float64).sum(0)
    assert tot.max() < 2 ** 24
    exact("colsum raw (integers)", gr, tot)
    exact("colsum scaled (integers)", go, tot.astype(np.float32) * scale)
    start = rng.standard_normal(Cc, dtype=np.float32)

    def accumulate():
        out.copy_(dev(start))
        ok(_colsum_call(lib, v, st, shape, None, out, None, 1), "colsum accumulate")
    res = []
    for _ in range(2):
        accumulate()
        torch.cuda.synchronize()
        res.append(host(out))
    assert np.array_equal(bits(res[0]), bits(res[1]))
    exact("colsum accumulate (integers)", res[0], tot.astype(np.float32) + start)
    wi = rng.integers(-3, 4, size=npix).astype(np.float32)      # signed row weights
    rw = dev(wi)
    (gw,) = twice(lambda: ok(_colsum_call(lib, v, st, shape, out=out, rowmul=rw), "colsum_rowmul"), [out])
    exact("colsum rowmul (integers)", gw, (wi[:, None].astype(np.float64) * xi.reshape(-1, Cc)).sum(0))
    del buf, v

    # 2) normal values against fp64
    x, buf, v, st = nhwc(rng, shape, mode)
    x2 = x.reshape(-1, Cc).astype(np.float64)
    (gr,) = twice(lambda: ok(_colsum_call(lib, v, st, shape, raw=raw), "colsum"), [raw])
    bounded("colsum %s" % (case,), gr, x2.sum(0), np.abs(x2).sum(0), 16)
    wf = rng.standard_normal(npix, dtype=np.float32)
    rw = dev(wf)
    (gw,) = twice(lambda: ok(_colsum_call(lib, v, st, shape, out=out, rowmul=rw), "colsum_rowmul"), [out])
    bounded("colsum rowmul %s" % (case,), gw, wf @ x2, np.abs(wf.astype(np.float64)) @ np.abs(x2), 16)


@pytest.mark.parametrize("n", [1, 255, 257, 32 * 256 * 256])
def test_sum(lib, n):
    rng = np.random.default_rng(n)
    out = torch.empty(1, device=DEV)
    xi = rng.integers(-4, 5, size=n).astype(np.float32)
    xd = dev(xi)
    (g,) = twice(lambda: ok(lib.depgan_op_sum(P(xd), n, P(out), 0, None), "sum"), [out])
    exact("sum (integers) n=%d" % n, g, [xi.astype(np.float64).sum()])
    x = rng.standard_normal(n, dtype=np.float32)
    xd = dev(x)
    (g,) = twice(lambda: ok(lib.depgan_op_sum(P(xd), n, P(out), 0, None), "sum"), [out])
    bounded("sum n=%d" % n, g, [x.astype(np.float64).sum()], [np.abs(x.astype(np.float64)).sum()], 16)


def test_reduction_scratch_capacity_is_checked(lib):
    """Every reduction that writes partials into the caller's scratch refuses one float less than its launch needs
    (status 1) and runs with exactly that much."""
    B, H, W, Cc = 32, 256, 256, 12        # colsum at the cap: 2048 blocks x C partials
    x = torch.zeros(B, H, W, Cc, device=DEV)
    out = torch.zeros(1024, device=DEV)
    st = (H * W * Cc, W * Cc, Cc)
    need = colsum_grid(B * H * W)[0] * Cc
    assert need == 2048 * Cc
    assert _colsum_call(lib, x, st, (B, H, W, Cc), out=out, cap=need - 1) == 1
    assert b"scratch" in lib.depgan_last_error()
    assert _colsum_call(lib, x, st, (B, H, W, Cc), out=out, cap=need) == 0
    assert _colsum_call(lib, x, st, (B, H, W, Cc), out=out, rowmul=x, cap=need - 1) == 1
    n = x.numel()
    assert lib.depgan_op_sum(P(x), n, P(out), 1023, None) == 1
    assert lib.depgan_op_sum(P(x), n, P(out), 1024, None) == 0
    assert lib.depgan_op_sum(P(x), 300, P(out), 1, None) == 1       # two blocks
    assert lib.depgan_op_sum(P(x), 300, P(out), 2, None) == 0
    g = x.reshape(-1)
    assert lib.depgan_op_gp_u0(P(g), P(g), P(out), None, 10.0, 3, 4096, 3 * 64 - 1, None) == 1
    assert lib.depgan_op_gp_u0(P(g), P(g), P(out), None, 10.0, 3, 4096, 3 * 64, None) == 0
    nbg = min((B * H * W + 255) // 256, 1024)
    assert lib.depgan_op_gloss_sums(P(g), 1, P(g), P(g), 0.5, P(out), B * H * W, 4 * nbg - 1, None) == 1
    assert lib.depgan_op_gloss_sums(P(g), 1, P(g), P(g), 0.5, P(out), B * H * W, 4 * nbg, None) == 0
    f = torch.zeros(2 * 1024, device=DEV)
    assert lib.depgan_op_film_bwd(P(g), P(g), P(f), P(f), 1024, P(x), P(f), P(f), 2, 64, 32, 2 * 64 * 2 * 32 - 1,
                                  None) == 1
    assert lib.depgan_op_film_bwd(P(g), P(g), P(f), P(f), 1024, P(x), P(f), P(f), 2, 64, 32, 2 * 64 * 2 * 32,
                                  None) == 0
    N, HW, Ct = 6, 16, 256
    tw = [torch.zeros(n, device=DEV) for n in (Ct, 1, HW, 1)]
    args = (P(g), P(g), P(g), P(g), P(g), 3, 1, 0, *[P(t) for t in tw], N, HW, Ct)
    assert lib.depgan_op_critic_tail_wgrad(*args, N * (Ct + HW) - 1, None) == 1
    assert lib.depgan_op_critic_tail_wgrad(*args, N * (Ct + HW), None) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# critic inputs and fake_y2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nicg", [1, 2])
@pytest.mark.parametrize("which", [0, 1])
def test_critic_inputs_and_add_ch0(lib, nicg, which):
    rng = np.random.default_rng(nicg * 10 + which)
    B, HW = 3, 4099
    y2 = rng.standard_normal((B, HW), dtype=np.float32)
    x = rng.standard_normal((B, HW, nicg), dtype=np.float32)
    attr = np.tanh(rng.standard_normal((B, HW))).astype(np.float32)
    ep = np.float32([0.0, 1.0, 0.3137])
    y2d, xd, ad, ed = dev(y2), dev(x), dev(attr), dev(ep)
    out = torch.empty(3, B, HW, device=DEV)
    (g,) = twice(lambda: ok(lib.depgan_op_critic_inputs(P(y2d), P(xd), nicg, P(ad), P(ed), P(out), B, HW, which, None),
                            "critic_inputs"), [out])
    y1 = x[..., 0]
    real = (y2 - y1) if which else y2
    fake = attr if which else y1 + attr
    exact("critic real", g[0], real)
    exact("critic fake", g[1], fake)
    exact("critic mix ep=0", g[2][0], fake[0])
    exact("critic mix ep=1", g[2][1], real[1])
    e = ep[:, None].astype(np.float64)
    ome = (np.float32(1) - ep)[:, None].astype(np.float64)
    bounded("critic mix which=%d nicg=%d" % (which, nicg), g[2], e * real + ome * fake,
            np.abs(e * real) + np.abs(ome * fake), 2)
    f = torch.empty(B, HW, device=DEV)
    (gf,) = twice(lambda: ok(lib.depgan_op_critic_inputs(None, P(xd), nicg, P(ad), None, P(f), B, HW, 2, None),
                             "add_ch0"), [f])
    exact("add_ch0", gf, y1 + attr)


# ---------------------------------------------------------------------------------------------------------------------
# gradient penalty
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", [1, 63, 64, 65, 4096, 65536])
@pytest.mark.parametrize("B", [1, 3, 32])
def test_gp_u0_and_critic_stats(lib, B, HW):
    rng = np.random.default_rng(B * 100000 + HW)
    g0 = rng.standard_normal((B, HW), dtype=np.float32)
    target = np.where(np.arange(B) % 2 == 0, 0.55, 1.8).astype(np.float32)      # norms below and above 1
    g0 *= (target / np.sqrt((g0.astype(np.float64) ** 2).sum(1)))[:, None].astype(np.float32)
    delta = 10.0
    gd = dev(g0)
    u0, norms, gp = torch.empty(B, HW, device=DEV), torch.empty(B, device=DEV), torch.empty(1, device=DEV)
    gu, gn, gg = twice(lambda: ok(lib.depgan_op_gp_u0(P(gd), P(u0), P(norms), P(gp), delta, B, HW, 0, None), "gp_u0"),
                       [u0, norms, gp])
    # d_gp_grads states u0 and the norms in float64 (the per-layer weight gradients it also forms are not needed)
    g64 = torch.from_numpy(g0.astype(np.float64)).view(B, 1, 1, HW)
    norm = torch.sqrt((g64 ** 2).sum((1, 2, 3)))
    ru = ((delta * 2.0 / B) * ((norm - 1.0) / norm).view(B, 1, 1, 1) * g64).view(B, HW).numpy()
    norm = norm.numpy()
    ss = norm ** 2
    bounded("gp norms B=%d HW=%d" % (B, HW), gn ** 2, ss, ss, 32)   # the squared norm is the reduction
    # u0's coefficient (norm - 1) / norm carries the norm's error e as about e / norm
    bounded("gp u0 B=%d HW=%d" % (B, HW), gu, ru, (delta * 2.0 / B) * (1.0 / norm + 1.0)[:, None] * np.abs(g0), 32)
    bounded("gp value B=%d HW=%d" % (B, HW), gg, [((norm - 1) ** 2).mean()],
            [((np.abs(norm - 1) + 1) * (norm + 1)).mean()], 96)

    d_out = rng.standard_normal(2 * B, dtype=np.float32)
    dd = dev(d_out)
    st = torch.empty(4, device=DEV)
    (gs,) = twice(lambda: ok(lib.depgan_op_critic_stats(P(dd), P(norms), P(st), B, None), "critic_stats"), [st])
    d64 = d_out.astype(np.float64)
    bounded("critic_stats sums B=%d" % B, gs[:2], [d64[:B].sum(), d64[B:].sum()],
            [np.abs(d64[:B]).sum(), np.abs(d64[B:]).sum()], 16)
    n64 = gn.astype(np.float64)
    bounded("critic_stats gp B=%d" % B, gs[2:3], [((n64 - 1) ** 2).sum()], [((np.abs(n64 - 1) + 1) ** 2).sum()], 16)
    assert gs[3] == B


# ---------------------------------------------------------------------------------------------------------------------
# generator-loss pieces
# ---------------------------------------------------------------------------------------------------------------------
THR = np.float32(0.5)


def _gloss_inputs(rng, Pn, nicg):
    """y1, y2, attr with y2 == thr and y1 + attr rounding (in fp32) to thr and to the float just below it, in quantity"""
    x = rng.uniform(-1, 1, size=(Pn, nicg)).astype(np.float32)
    attr = np.tanh(rng.standard_normal(Pn)).astype(np.float32)
    y2 = rng.uniform(-1, 1, size=Pn).astype(np.float32)
    below = np.nextafter(THR, np.float32(-1))
    k = Pn // 8
    y2[:k] = THR
    y2[k:2 * k] = below
    # y1 = thr - attr in fp32, nudged by up to two ulps: y1 + attr then lands on thr, below it and above it
    y1 = (THR - attr[2 * k:6 * k]).astype(np.float32)
    steps = rng.integers(-2, 3, size=y1.shape)
    y1 = np.where(steps > 0, np.nextafter(y1, np.float32(9)), np.where(steps < 0, np.nextafter(y1, np.float32(-9)), y1))
    x[2 * k:6 * k, 0] = y1
    s = x[:, 0] + attr
    assert (s == THR).sum() > 0 and (s == below).sum() > 0 and (y2 == THR).sum() > 0
    return x, y2, attr


@pytest.mark.parametrize("Pn", [1000, 256 * 1024 + 3, 32 * 256 * 256])
def test_gloss_sums_counts_are_exact(lib, Pn):
    nicg = 2
    rng = np.random.default_rng(Pn)
    x, y2, attr = _gloss_inputs(rng, Pn, nicg)
    xd, y2d, ad = dev(x), dev(y2), dev(attr)
    sums = torch.empty(4, device=DEV)
    (g,) = twice(lambda: ok(lib.depgan_op_gloss_sums(P(xd), nicg, P(y2d), P(ad), float(THR), P(sums), Pn, 0, None),
                            "gloss_sums"), [sums])
    y1 = x[:, 0]
    wr = y2 >= THR
    wf = (y1 + attr) >= THR                      # fp32 addition, as the kernel and GT:580 (K.greater_equal on floats)
    counts = [np.count_nonzero(wr), np.count_nonzero(wf), np.count_nonzero(wr & wf)]
    print("gloss counts P=%d: %s (kernel %s)" % (Pn, counts, g[1:].tolist()))
    assert g[1:].tolist() == [float(c) for c in counts]
    d = attr.astype(np.float64) - (y2.astype(np.float64) - y1)
    bounded("gloss L1 P=%d" % Pn, g[:1], [np.abs(d).sum()],
            [(np.abs(attr) + np.abs(y2) + np.abs(y1)).astype(np.float64).sum()], 16)


def test_g_dpre(lib):
    nicg, B = 2, 3
    rng = np.random.default_rng(11)
    Pn = B * 4099
    x = rng.uniform(-1, 1, size=(Pn, nicg)).astype(np.float32)
    y2 = rng.uniform(-1, 1, size=Pn).astype(np.float32)
    attr = np.tanh(rng.standard_normal(Pn)).astype(np.float32)
    g1 = rng.standard_normal(Pn, dtype=np.float32)
    g2 = rng.standard_normal(Pn, dtype=np.float32)
    k = Pn // 10
    attr[:k] = (y2[:k] - x[:k, 0]).astype(np.float32)      # attr - (y2 - y1) == 0 exactly: the sign is 0
    g1[:k // 2] = 0.0
    g2[:k // 2] = 0.0
    attr[k:k + 50] = 1.0                                      # the tanh factor vanishes
    attr[k + 50:k + 100] = -1.0
    xd, y2d, ad, g1d, g2d = dev(x), dev(y2), dev(attr), dev(g1), dev(g2)
    dpre = torch.empty(Pn, device=DEV)
    (g,) = twice(lambda: ok(lib.depgan_op_g_dpre(P(xd), nicg, P(y2d), P(ad), P(g1d), P(g2d), P(dpre), B, Pn, None),
                            "g_dpre"), [dpre])
    diff = attr - (y2 - x[:, 0])
    assert (diff[:k] == 0).all()
    m1c = 100.0 / Pn
    a64 = attr.astype(np.float64)
    ref = (-(g1.astype(np.float64) + g2) / B + m1c * np.sign(diff)) * (1 - a64 * a64)
    mag = ((np.abs(g1) + np.abs(g2)).astype(np.float64) / B + m1c) * (1 + a64 * a64)
    bounded("g_dpre", g, ref, mag, 8)
    assert (g[:k // 2] == 0).all(), "sign(0) must be 0"
    assert (g[k:k + 100] == 0).all(), "attr = +-1 must give a zero gradient"


# ---------------------------------------------------------------------------------------------------------------------
# FiLM backward
# ---------------------------------------------------------------------------------------------------------------------
FILM_CASES = [  # B, HW, C
    (1, 1, 4), (32, 63, 12), (1, 4096, 32), (32, 4096, 128), (1, 65536, 12), (32, 65536, 4), (2, 63, 128),
]


@pytest.mark.parametrize("B,HW,Cc", FILM_CASES)
def test_film_bwd(lib, B, HW, Cc):
    rng = np.random.default_rng(B * HW + Cc)
    dr = rng.standard_normal((B, HW, Cc), dtype=np.float32)
    u = rng.standard_normal((B, HW, Cc), dtype=np.float32)
    ld, cm, ca = 1024, 96, 96 + 160                  # rows of the 1024-wide head vector, as the model passes them
    heads = rng.standard_normal((B, ld), dtype=np.float32)
    fm, fa = heads[:, cm:cm + Cc], heads[:, ca:ca + Cc]
    drd, ud, hd = dev(dr), dev(u), dev(heads)
    du = torch.empty(B, HW, Cc, device=DEV)
    dh = torch.empty(B, ld, device=DEV)
    off = lambda t, c: C.c_void_p(t.data_ptr() + 4 * c)   # noqa: E731
    gdu, gdh = twice(lambda: ok(lib.depgan_op_film_bwd(P(drd), P(ud), off(hd, cm), off(hd, ca), ld, P(du), off(dh, cm),
                                                       off(dh, ca), B, HW, Cc, 0, None), "film_bwd"), [du, dh])
    pre = u * fm[:, None, :] + fa[:, None, :]         # fp32 product then sum, not contracted (film_preact)
    dv = np.where(pre > 0, dr, np.float32(0))
    exact("film du", gdu, dv * fm[:, None, :])
    written = np.zeros(ld, bool)
    written[cm:cm + Cc] = written[ca:ca + Cc] = True
    assert np.isnan(gdh[:, ~written]).all(), "film_bwd wrote outside its two column ranges"
    dv64 = dv.astype(np.float64)
    tag = "film B=%d HW=%d C=%d" % (B, HW, Cc)
    bounded(tag + " dmul", gdh[:, cm:cm + Cc], (dv64 * u).sum(1), np.abs(dv64 * u).sum(1), 16)
    bounded(tag + " dadd", gdh[:, ca:ca + Cc], dv64.sum(1), np.abs(dv64).sum(1), 16)


def test_film_bwd_refuses_wide_channels(lib):
    x = torch.zeros(1024, device=DEV)
    assert lib.depgan_op_film_bwd(P(x), P(x), P(x), P(x), 256, P(x), P(x), P(x), 1, 1, 132, 0, None) == 1
    assert b"<= 128" in lib.depgan_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# batched BatchNorm jobs
# ---------------------------------------------------------------------------------------------------------------------
def test_bn_prepare_batch(lib):
    rng = np.random.default_rng(3)
    Cs = [32, 1, 300, 1024, 7, 256]
    jobs, ptrs, keep = [], [], []
    for j, Cc in enumerate(Cs):
        g, b, m = (rng.standard_normal(Cc, dtype=np.float32) for _ in range(3))
        v = rng.uniform(0.01, 3.0, Cc).astype(np.float32)
        ins = [dev(a) for a in (g, b, m, v)]
        outs = [torch.empty(Cc, device=DEV) for _ in range(3 + (j % 2))]      # mean_copy on odd jobs
        keep += ins + outs
        jobs.append((g, b, m, v, outs))
        ptrs += [t.data_ptr() for t in ins + outs] + ([0] if j % 2 == 0 else [])
    arr = (C.c_void_p * len(ptrs))(*ptrs)
    carr = (C.c_int * len(Cs))(*Cs)
    res = []
    for _ in range(2):
        for _, _, _, _, outs in jobs:
            for o in outs:
                o.fill_(NAN)
        ok(lib.depgan_op_bn_prepare_batch(arr, carr, len(Cs), O.BN_EPS, None), "bn_prepare_batch")
        torch.cuda.synchronize()
        res.append([[host(o) for o in outs] for *_, outs in jobs])
    for r0, r1 in zip(*res):
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(r0, r1))
    for (g, b, m, v, _), got in zip(jobs, res[0]):
        r = 1.0 / np.sqrt(v.astype(np.float64) + np.float32(O.BN_EPS))
        s = g * r
        bounded("bn_prepare rstd C=%d" % len(g), got[2], r, r, 6)
        bounded("bn_prepare s C=%d" % len(g), got[0], s, np.abs(s), 8)
        bounded("bn_prepare t C=%d" % len(g), got[1], b - m * s, np.abs(b) + np.abs(m * s), 10)
        if len(got) == 4:
            exact("bn_prepare mean_copy", got[3], m)


def test_bn_gamma_grad_batch(lib):
    """jobs of every form in one launch: oi = 0 and 1 alternating (oi = 1 after oi = 0), K not a multiple of 256,
    Cout = 1 and Cout > 256; the job of each block is found from the blk0 table, so every job boundary is a block"""
    rng = np.random.default_rng(4)
    shapes = [(0, 300, 32, 1), (1, 9 * 37, 64, 37), (0, 1, 1, 1), (1, 9 * 32, 257, 32), (0, 9 * 256, 300, 1),
              (1, 25 * 3, 1, 3), (0, 100, 7, 1)]
    ptrs, dims, refs, outs, keep = [], [], [], [], []
    for oi, K, Cout, Cin in shapes:
        if oi:
            W = rng.standard_normal((K // Cin, Cout, Cin), dtype=np.float32)
            dW = rng.standard_normal((K // Cin, Cout, Cin), dtype=np.float32)
            dot = np.einsum("tci,tci->c", W.astype(np.float64), dW)
            mag = np.einsum("tci,tci->c", np.abs(W.astype(np.float64)), np.abs(dW))
        else:
            W = rng.standard_normal((K, Cout), dtype=np.float32)
            dW = rng.standard_normal((K, Cout), dtype=np.float32)
            dot = (W.astype(np.float64) * dW).sum(0)
            mag = np.abs(W.astype(np.float64) * dW).sum(0)
        bias, mean, S = (rng.standard_normal(Cout, dtype=np.float32) for _ in range(3))
        rstd = rng.uniform(0.5, 2, Cout).astype(np.float32)
        ins = [dev(a) for a in (W, dW, bias, mean, rstd, S)]
        o = torch.empty(Cout, device=DEV)
        keep += ins
        outs.append(o)
        ptrs += [t.data_ptr() for t in ins] + [o.data_ptr()]
        dims += [K, Cout, oi, Cin]
        bm = bias.astype(np.float64) - mean
        refs.append((rstd * (dot + bm * S), rstd * (mag + (np.abs(bias) + np.abs(mean)) * np.abs(S) * 2), oi, K, Cout))
    arr = (C.c_void_p * len(ptrs))(*ptrs)
    darr = (C.c_int * len(dims))(*dims)
    got = twice(lambda: ok(lib.depgan_op_bn_gamma_grad_batch(arr, darr, len(shapes), None), "bn_gamma_grad_batch"),
                outs)
    for g, (ref, mag, oi, K, Cout) in zip(got, refs):
        bounded("bn_gamma_grad oi=%d K=%d Cout=%d" % (oi, K, Cout), g, ref, mag, 24)


# ---------------------------------------------------------------------------------------------------------------------
# noise MLP (inference-mode BatchNorm)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noise_params():
    G = O.init_generator(21)
    G = {k: np.asarray(v, np.float32) for k, v in G.items()}
    heads = ["noise_2_" + sfx for sfx, _ in O.NOISE_HEADS]
    ncol = [G["dense_" + h + "/kernel"].shape[1] for h in heads]
    assert len(ncol) == 14 and sum(ncol) == 1024
    rng = np.random.default_rng(22)
    for nm in ["noise_1_add_f0", "noise_1_add_f1"] + heads:          # biases and BN state away from zero
        G["dense_" + nm + "/bias"] = rng.standard_normal(G["dense_" + nm + "/bias"].shape).astype(np.float32) * 0.1
    return G, heads, ncol


def _bn32(G, nm):
    """the s, t, rstd the model's dg_bn_prepare_batch computes, in float32"""
    g, b, m, v = (G["dense_bn_" + nm + "/" + k] for k in ("gamma", "beta", "moving_mean", "moving_variance"))
    r = (np.float32(1) / np.sqrt(v + np.float32(O.BN_EPS))).astype(np.float32)
    s = (g * r).astype(np.float32)
    return s, (b - m * s).astype(np.float32), r


def _noise_T(G, heads, absval):
    """the oracle's tensor dict in float64, with BN moving statistics that reproduce the float32 s, t, rstd the kernels
    read; absval: every weight, bias and affine term by its absolute value (the sum|terms| pass)"""
    T = {}
    for nm in ["noise_1_add_f0", "noise_1_add_f1"] + heads:
        s, t, r = (a.astype(np.float64) for a in _bn32(G, nm))
        W = G["dense_" + nm + "/kernel"].astype(np.float64)
        b = G["dense_" + nm + "/bias"].astype(np.float64)
        m = G["dense_bn_" + nm + "/moving_mean"].astype(np.float64)
        if absval:
            W, b, s, t, m = np.abs(W), np.abs(b) + np.abs(m), np.abs(s), np.abs(t), 0 * m
        T["dense_" + nm + "/kernel"], T["dense_" + nm + "/bias"] = W, b
        # _bn_st: rstd = 1/sqrt(var + eps), s = gamma * rstd, t = beta - mean * s
        T["dense_bn_" + nm + "/moving_variance"] = 1.0 / (r * r) - O.BN_EPS
        T["dense_bn_" + nm + "/gamma"] = s / r
        T["dense_bn_" + nm + "/moving_mean"] = m
        T["dense_bn_" + nm + "/beta"] = t + m * s
    return {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in T.items()}


@pytest.mark.parametrize("B", [1, 3, 32, 64])
def test_noise_mlp_forward_backward(lib, noise_params, B):
    G, heads, ncol = noise_params
    rng = np.random.default_rng(B)
    s0, t0, r0 = _bn32(G, "noise_1_add_f0")
    s1, t1, r1 = _bn32(G, "noise_1_add_f1")
    g = lambda k: G["dense_" + k].reshape(-1)      # noqa: E731
    trunk = np.concatenate([g("noise_1_add_f0/kernel"), g("noise_1_add_f0/bias"), s0, t0,
                            G["dense_bn_noise_1_add_f0/moving_mean"], r0, g("noise_1_add_f1/kernel"),
                            g("noise_1_add_f1/bias"), s1, t1, G["dense_bn_noise_1_add_f1/moving_mean"], r1])
    assert trunk.size == 1376
    Wh = np.concatenate([G["dense_" + h + "/kernel"].reshape(-1) for h in heads])
    hb = [np.concatenate(a) for a in zip(*[(G["dense_" + h + "/bias"], *_bn32(G, h)[:2],
                                            G["dense_bn_" + h + "/moving_mean"], _bn32(G, h)[2]) for h in heads])]
    hvec = np.concatenate(hb)
    z = rng.standard_normal((B, 32, 1), dtype=np.float32)
    td, whd, hvd, zd = dev(trunk), dev(Wh), dev(hvec), dev(z)
    nc = (C.c_int * 14)(*ncol)
    acts = torch.empty(6, B, 1024, device=DEV)
    (ga,) = twice(lambda: ok(lib.depgan_op_noise_fwd(P(td), P(whd), P(hvd), nc, P(zd), P(acts), B, None), "noise_fwd"),
                  [acts])
    T = _noise_T(G, heads, False)
    Ta = _noise_T(G, heads, True)
    z64 = torch.from_numpy(z.astype(np.float64))
    rh, st = M.noise_fwd_store(T, z64)
    mh, sta = M.noise_fwd_store(Ta, z64.abs(), masks={"noise_a0": st["m0"], "noise_a1": st["m1"]})
    for i, (key, k) in enumerate((("h0", 8), ("a0", 8), ("h1", 16), ("a1", 16))):
        bounded("noise fwd %s B=%d" % (key, B), ga[i].reshape(B, 32, 32), st[key].numpy(), sta[key].numpy(), k)
    cols = np.cumsum([0] + ncol)
    rheads = np.concatenate([rh[h].numpy() for h in heads], 1)
    mheads = np.concatenate([mh[h].numpy() for h in heads], 1)
    bounded("noise fwd heads B=%d" % B, ga[5], rheads, mheads, 24)
    assert cols[-1] == 1024

    dheads = rng.standard_normal((B, 1024), dtype=np.float32)
    dhd = dev(dheads)
    gt, gw, gh = torch.empty(1248, device=DEV), torch.empty(1024 * 1024, device=DEV), torch.empty(3072, device=DEV)
    rt, rw, rhv = twice(lambda: ok(lib.depgan_op_noise_bwd(P(td), P(whd), P(hvd), nc, P(zd), P(acts), P(dhd), P(gt),
                                                           P(gw), P(gh), B, 0, None), "noise_bwd"), [gt, gw, gh])
    dh64 = {h: torch.from_numpy(dheads[:, cols[i]:cols[i + 1]].astype(np.float64)) for i, h in enumerate(heads)}
    R = M.noise_bwd(T, st, dh64)
    Ra = M.noise_bwd(Ta, sta, {h: v.abs() for h, v in dh64.items()})
    tag = " B=%d" % B
    o = 0
    for nm in ("noise_1_add_f0", "noise_1_add_f1"):
        for key, n, k in (("dense_%s/kernel", 32 if nm.endswith("f0") else 1024, 16),
                          ("dense_%s/bias", 32, 16), ("dense_bn_%s/gamma", 32, 16), ("dense_bn_%s/beta", 32, 16)):
            name = key % nm
            bounded("noise bwd " + name + tag, rt[o:o + n], R[name].numpy().reshape(-1),
                    Ra[name].numpy().reshape(-1), k)
            o += n
    for i, h in enumerate(heads):
        a, b = cols[i], cols[i + 1]
        Wn = G["dense_" + h + "/kernel"].size
        woff = 1024 * a
        bounded("noise bwd %s kernel%s" % (h, tag), rw[woff:woff + Wn], R["dense_" + h + "/kernel"].numpy().reshape(-1),
                Ra["dense_" + h + "/kernel"].numpy().reshape(-1), 16)
        for j, key in enumerate(("dense_%s/bias", "dense_bn_%s/gamma", "dense_bn_%s/beta")):
            name = key % h
            bounded("noise bwd " + name + tag, rhv[1024 * j + a:1024 * j + b], R[name].numpy(), Ra[name].numpy(), 24)


# ---------------------------------------------------------------------------------------------------------------------
# best-of-k noise
# ---------------------------------------------------------------------------------------------------------------------
def _g_total(s):
    """g_loss_from_sums' total (model.hip), statement by statement in Python floats (IEEE double, no contraction),
    rounded to float32"""
    s = [float(np.float32(v)) for v in s]
    n, npix = s[6], s[7]

    def div(a, b):
        if b == 0.0:
            return math.nan if a == 0.0 or math.isnan(a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
        return a / b
    lf, lfd = div(s[0], n), div(s[1], n)
    m1 = div(100.0 * s[2], npix)
    dv = s[3] / 1000.0 - s[4] / 1000.0
    m3 = 100.0 * dv * dv
    dice = div(2.0 * s[5] + 1e-7, s[3] + s[4] + 1e-7)
    m4 = 1.0 - dice
    return np.float32(-lf - lfd + m1 + m3 + m4)


def _stats(rng, k):
    st = np.zeros((k, 8), np.float32)
    st[:, 0] = rng.standard_normal(k) * 3
    st[:, 1] = rng.standard_normal(k) * 3
    st[:, 2] = rng.uniform(1e3, 5e4, k)
    st[:, 3] = rng.integers(0, 4000, k)
    st[:, 4] = rng.integers(0, 4000, k)
    st[:, 5] = np.minimum(st[:, 3], st[:, 4]) * rng.uniform(0, 1, k).astype(np.float32)
    st[:, 6] = 3
    st[:, 7] = 3 * 65536
    return st


def _near_ties(rng, k):
    """k candidates whose double totals differ by less than a float32 ulp: after rounding, exact ties and 1-ulp steps"""
    st = np.repeat(_stats(rng, 1), k, 0)
    # m1 = 100 * s2 / npix: a step of one ulp of s2 moves the total by ~1/4 ulp of its float32 value
    s2 = st[0, 2]
    for i in range(k):
        st[i, 2] = s2
        s2 = np.nextafter(s2, np.float32(1e9)) if rng.uniform() < 0.6 else np.nextafter(s2, np.float32(0))
    return st


BEST_CASES = {
    "k1": lambda r: _stats(r, 1),
    "k2": lambda r: _stats(r, 2),
    "k32": lambda r: _stats(r, 32),
    "k32_near_ties": lambda r: _near_ties(r, 32),
    "k2_exact_tie": lambda r: np.repeat(_stats(r, 1), 2, 0),
    "nan_first": lambda r: _with(_stats(r, 32), {0: (0, np.nan)}),
    "nan_later": lambda r: _with(_stats(r, 32), {5: (0, np.nan)}),
    "nan_twice": lambda r: _with(_stats(r, 32), {7: (1, np.nan), 19: (0, np.nan)}),
    "nan_from_zero_n": lambda r: _with(_stats(r, 2), {1: (6, 0.0), 0: (0, 0.0)}),
    "minus_inf": lambda r: _with(_stats(r, 32), {3: (0, np.inf)}),
    "plus_inf_first": lambda r: _with(_stats(r, 2), {0: (0, -np.inf)}),
    "inf_and_nan": lambda r: _with(_stats(r, 32), {4: (0, np.inf), 9: (0, np.nan)}),
}


def _with(st, edits):
    for i, (col, v) in edits.items():
        st[i, col] = v
    return st


@pytest.mark.parametrize("case", list(BEST_CASES))
def test_best_noise_follows_numpy_argmin(lib, case):
    rng = np.random.default_rng(len(case))
    st = BEST_CASES[case](rng)
    k = st.shape[0]
    tot = np.array([_g_total(s) for s in st], np.float32)
    want = int(np.argmin(tot))
    zf = 3 * 32
    z = rng.standard_normal((k, zf), dtype=np.float32)
    sd, zd = dev(st), dev(z)
    best = torch.empty(1, dtype=torch.int32, device=DEV)
    zo = torch.empty(zf, device=DEV)
    res = []
    for _ in range(2):
        best.fill_(-1)
        zo.fill_(NAN)
        ok(lib.depgan_op_best_noise(P(sd), k, P(zd), zf, P(best), P(zo), None), "best_noise")
        torch.cuda.synchronize()
        res.append((int(best.item()), host(zo)))
    assert res[0][0] == res[1][0]
    print("best_noise %s: totals %s -> %d" % (case, tot[:8], res[0][0]))
    assert res[0][0] == want, (case, tot, res[0][0], want)
    exact("best_noise z_out", res[0][1], z[want])
    if case == "k32_near_ties":
        assert len(np.unique(tot)) < k and (tot == tot.min()).sum() >= 1


# ---------------------------------------------------------------------------------------------------------------------
# bf16 rounding of the weights (bf16-weights mode)
# ---------------------------------------------------------------------------------------------------------------------
def test_round_bf16_masked_matches_torch_cast(lib):
    rng = np.random.default_rng(9)
    special = np.array([
        0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF,          # ties to even (down, up), just above / below a tie
        0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7F8000,          # round up to +-inf, and the largest finite below
        0x00000000, 0x80000000, 0x7F800000, 0xFF800000,          # +-0, +-inf
        0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FBFFFFF,          # quiet and signalling NaNs
        0x00000001, 0x00008000, 0x00018000, 0x007FFFFF,          # fp32 subnormals: ties, and up to the normal range
        0x80008001, 0x807F8000, 0x00800000, 0x00C08000,
    ], np.uint32).view(np.float32)
    x = np.concatenate([special, rng.standard_normal(100000).astype(np.float32),
                        rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    mask = (rng.uniform(size=x.size) < 0.7).astype(np.uint8)
    mask[:special.size] = 1
    mask[special.size:special.size + 8] = 0
    x[special.size:special.size + 8] = special[:8]
    xd, md = dev(x), dev(mask)
    out = torch.empty(x.size, device=DEV)
    (g,) = twice(lambda: ok(lib.depgan_op_round_bf16_masked(P(xd), P(md), P(out), x.size, None), "round_bf16"), [out])
    ref = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    m = mask.astype(bool)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(g[m]), nan[m]), "NaN must stay NaN, and nothing else may become NaN"
    exact("round_bf16 masked", g[m & ~nan], ref[m & ~nan])
    exact("round_bf16 pass-through", g[~m], x[~m])
    sub = m & (np.abs(x) < np.float32(1.1754944e-38)) & (x != 0)
    assert sub.sum() >= 6 and (g[sub] != 0).any(), "fp32 subnormals were flushed"
    exact("round_bf16 subnormals", g[sub], ref[sub])
    exact("round_bf16 vs oracle (finite)", g[m & np.isfinite(x) & np.isfinite(ref)],
          O.round_bf16(x[m & np.isfinite(x) & np.isfinite(ref)]))
