"""GPU parity, operator level, of the learning-phase-1 kernels (csrc/train_ops.hip) through the depgan_op_* entries:
batch moments, BatchNorm backward, the fused affine / FiLM / ReLU / dropout / residual pass, softmax + Keras
cross-entropy, the noise MLP's BatchNorm over rows and its small GEMMs.  Each is checked against a float64
restatement of the oracle's formula (oracle/depgan_oracle.py: _bn_train, keras_categorical_crossentropy_t,
dropout_keep_mask), at the shapes where the grid changes form: one block, the 1024-block cap with a ragged last block,
full size, channel counts that do not divide the 256 threads, channel slices of wider buffers (the FLAT = false
address path).  Every call runs twice and must repeat bit for bit: none of these kernels uses float atomics."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import depgan_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = O.BN_EPS


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def grid(npix):
    """moments_partial / colsum2_partial launch: nb blocks of ppb pixels (train_ops.hip t_pix_grid)."""
    nb = min((npix + 255) // 256, 1024)
    ppb = (npix + nb - 1) // nb
    return (npix + ppb - 1) // ppb, ppb


def nhwc_view(rng, B, H, W, C, strided, offset=False, const=False):
    """x as (B,H,W,C) float32 and the device buffer holding it: dense, or channels [4, 4+C) of a (B,H,W,C+8) buffer.
    offset: channels 1 and C-1 sit at 1e3 sigma from zero; const: channel 0 holds one value."""
    x = rng.standard_normal((B, H, W, C), dtype=np.float32)
    x *= (0.5 + np.arange(C, dtype=np.float32) % 3)
    if offset:
        x[..., 1] += 1000.0
        x[..., C - 1] -= 3000.0
    if const:
        x[..., 0] = np.float32(0.3)
    if not strided:
        buf = torch.from_numpy(x).to(DEV)
        return x, buf, buf, (H * W * C, W * C, C)
    Ct = C + 8
    buf = torch.full((B, H, W, Ct), float("nan"), device=DEV)
    buf[..., 4:4 + C] = torch.from_numpy(x).to(DEV)
    return x, buf, buf[..., 4:], (H * W * Ct, W * Ct, Ct)


def like(buf, C):
    """an output buffer shaped as buf (NaN-filled), and its view of the same channels"""
    out = torch.full_like(buf, float("nan"))
    return out, (out if buf.shape[-1] == C else out[..., 4:4 + C])


# B, H, W, C, strided, offset, const
MOMENT_CASES = [
    (1, 8, 8, 32, False, True, True),             # 64 pixels: one block
    (2, 10, 12, 12, True, False, True),           # one block; C = 12: 255 of 256 threads carry a pixel lane
    (1, 1, 256 * 1024 + 1, 4, False, True, True),  # the 1024-block cap, ppb rounded up: 1021 blocks, the last of 5
    (1, 1, 256 * 1024 + 1, 4, True, False, False),
    (3, 317, 331, 4, True, True, False),           # capped, ragged, and a pixel row straddles block boundaries
    (2, 100, 1500, 32, False, False, True),        # capped, 1024 blocks of 293 pixels, the last one 261
    (32, 256, 256, 32, False, True, True),         # the model's full size (256 x 256, batch 32)
    (32, 256, 256, 32, True, False, False),
    (32, 64, 64, 256, False, True, True),          # the 64 x 64 layers at full size, C = 256
    (2, 16, 16, 1020, True, True, False),          # C = 1020: 255 pixel lanes, one pixel per pass
    (2, 16, 16, 1024, False, True, True),          # C = 1024: one pixel lane per block
    (3, 29, 31, 1024, True, False, True),
]


def _case_id(c):
    return "%dx%dx%dx%d%s%s" % (c[0], c[1], c[2], c[3], "_strided" if c[4] else "", "_offset" if c[5] else "")


def test_case_table_covers_every_grid_form():
    """The table cannot lose coverage silently: one block, the cap with ragged per-block counts, a cap whose ppb
    rounding leaves fewer than 1024 blocks, full size, both address paths, every channel form."""
    forms = []
    for B, H, W, Cc, strided, offset, const in MOMENT_CASES:
        npix = B * H * W
        nb, ppb = grid(npix)
        assert (nb - 1) * ppb < npix <= nb * ppb
        forms.append(dict(one=nb == 1, capped=(npix + 255) // 256 > 1024, ragged=npix % ppb != 0, nb=nb,
                          full=(B, H, W) == (32, 256, 256), strided=strided, C=Cc))
    assert any(f["one"] for f in forms)
    assert any(f["capped"] and f["ragged"] for f in forms)
    assert any(f["capped"] and f["nb"] < 1024 for f in forms)
    assert any(f["capped"] and f["nb"] == 1024 and f["ragged"] for f in forms)
    assert any(f["full"] and f["C"] == 32 for f in forms)
    assert all(any(f["strided"] == s for f in forms) for s in (False, True))
    assert {4, 12, 32, 256, 1020, 1024} <= {f["C"] for f in forms}


def _moments(lib, xv, strides, B, H, W, Cc):
    from dep_gan_im_amd import _lib
    res = []
    for _ in range(2):
        mean = torch.full((Cc,), float("nan"), device=DEV)
        var = torch.full((Cc,), float("nan"), device=DEV)
        _lib.check(lib.depgan_op_bn_moments(P(xv), *strides, B, H, W, Cc, P(mean), P(var), 0, None), "bn_moments")
        torch.cuda.synchronize()
        res.append((mean.cpu().numpy(), var.cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    return res[0]


def _ref_moments(x):
    xd = torch.from_numpy(x).reshape(-1, x.shape[-1]).double()
    return xd.mean(0).numpy(), xd.var(0, unbiased=False).numpy()


@pytest.mark.parametrize("case", MOMENT_CASES, ids=_case_id)
def test_bn_moments(lib, case):
    B, H, W, Cc, strided, offset, const = case
    rng = np.random.default_rng(B * 7 + H * 3 + W + Cc)
    x, buf, xv, strides = nhwc_view(rng, B, H, W, Cc, strided, offset, const)
    mean, var = _moments(lib, xv, strides, B, H, W, Cc)
    mu, vr = _ref_moments(x)
    sig = np.sqrt(vr)
    assert np.all(np.abs(mean - mu) <= 1e-6 * (np.abs(mu) + sig)), np.max(np.abs(mean - mu) / (np.abs(mu) + sig))
    live = vr > 0
    assert np.all(np.abs(var[live] - vr[live]) <= 1e-5 * vr[live]), np.max(np.abs(var[live] - vr[live]) / vr[live])
    if const:
        # the first-pixel shift makes every difference of a constant channel exactly zero
        assert var[0] == 0.0 and mean[0] == np.float32(0.3)


def _ref_bn_backward(x, gamma, dy, dyscale):
    Cc = x.shape[-1]
    xd = torch.from_numpy(x).reshape(-1, Cc).double().requires_grad_(True)
    g = torch.from_numpy(gamma).double().requires_grad_(True)
    beta = torch.zeros(Cc, dtype=torch.float64, requires_grad=True)
    mu, var = xd.mean(0), xd.var(0, unbiased=False)
    y = g * (xd - mu) * torch.rsqrt(var + EPS) + beta
    gx, gg, gb = torch.autograd.grad(y, [xd, g, beta], torch.from_numpy(dy).reshape(-1, Cc).double() * dyscale)
    return gx.numpy().reshape(x.shape), gg.numpy(), gb.numpy()


def _bn_backward(lib, x, xv, dyv, buf, strides, gamma, dyscale, B, H, W, Cc, scratch=0):
    from dep_gan_im_amd import _lib
    mu, vr = _ref_moments(x)
    mean_d = torch.from_numpy(mu.astype(np.float32)).to(DEV)
    var_d = torch.from_numpy(vr.astype(np.float32)).to(DEV)
    gam_d = torch.from_numpy(gamma).to(DEV)
    res = []
    for _ in range(2):
        out, ov = like(buf, Cc)
        dgam = torch.full((Cc,), float("nan"), device=DEV)
        dbet = torch.full((Cc,), float("nan"), device=DEV)
        rc = lib.depgan_op_bn_backward(P(dyv), P(xv), P(ov), *strides, B, H, W, Cc, P(gam_d), P(mean_d), P(var_d), EPS,
                                       1.0 / (B * H * W), dyscale, P(dgam), P(dbet), scratch, None)
        _lib.check(rc, "bn_backward")
        torch.cuda.synchronize()
        res.append((ov.cpu().numpy(), dgam.cpu().numpy(), dbet.cpu().numpy()))
        if ov is not out:   # the channels around the slice are untouched
            assert torch.isnan(out[..., :4]).all() and torch.isnan(out[..., 4 + Cc:]).all()
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    return res[0]


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / (np.abs(b).max() + 1e-300))


@pytest.mark.parametrize("case", MOMENT_CASES, ids=_case_id)
def test_bn_backward(lib, case):
    """dRAW, dgamma, dbeta of y = gamma (x - mu) rsqrt(var + eps) + beta, batch statistics differentiated through;
    the exact gradient of a bias in front of the BN (sum of dRAW over the pixels) is zero."""
    B, H, W, Cc, strided, offset, const = case
    rng = np.random.default_rng(B * 5 + H + W * 3 + Cc)
    x, buf, xv, strides = nhwc_view(rng, B, H, W, Cc, strided, offset, const)
    dy, dbuf, dyv, _ = nhwc_view(rng, B, H, W, Cc, strided)
    gamma = (0.5 + rng.random(Cc)).astype(np.float32)
    dyscale = 1.0 / (1.0 - O.DROP_RATE) if Cc % 8 == 0 else 1.0
    draw, dgam, dbet = _bn_backward(lib, x, xv, dyv, buf, strides, gamma, dyscale, B, H, W, Cc)
    gx, gg, gb = _ref_bn_backward(x, gamma, dy, dyscale)
    # The operator is handed the float32 mean, as the model hands it the moments' output: dgamma = rstd sum dy (x - mean)
    # then carries (mu - mean_f32) rstd sum dy exactly, log10(|mu| / sigma) digits of an offset channel (the oracle's
    # fp32 run carries the same).  That term is part of the reference; what is bounded is everything else.
    mu, vr = _ref_moments(x)
    gg = gg + (mu - mu.astype(np.float32)) / np.sqrt(vr + EPS) * gb
    errs = (_rel(draw, gx), _rel(dgam, gg), _rel(dbet, gb))
    assert max(errs) <= 1e-5, errs
    # sum over pixels of dRAW = -gamma rstd^2 dgamma (mu - mean_f32) given the float32 mean, else rounding.  Checked on the
    # channels without an offset: at |mu| = 1e3 sigma the folded coefficient Cc = k mean carries eps |k mean| into every
    # element alike; there the per-element bound above is what holds
    rstd = 1.0 / np.sqrt(vr + EPS)
    given = np.abs(gamma * rstd ** 2 * gg * (mu - mu.astype(np.float32)))
    colsum = np.abs(draw.reshape(-1, Cc).astype(np.float64).sum(0))
    bound = 1e-5 * np.abs(draw).reshape(-1, Cc).astype(np.float64).sum(0) + 1.01 * given + 1e-30
    centred = np.abs(mu) < 100.0 * np.sqrt(vr) + 1.0
    assert centred.sum() >= Cc - 2 and np.all((colsum <= bound)[centred]), colsum[centred].max()


@pytest.mark.parametrize("case", [c for c in MOMENT_CASES if c[0] * c[1] * c[2] * c[3] <= 1 << 22 or c[3] == 32],
                         ids=_case_id)
def test_bn_backward_ill_conditioned(lib, case):
    """dy = a xhat + b + 1e-3 noise: dRAW is the small residual of large terms.  Bound against max |s dy| with a float32
    evaluation of the same formula on the CPU as the yardstick: HIP at most 4x its error."""
    B, H, W, Cc, strided, offset, const = case
    rng = np.random.default_rng(B + H * 5 + W + Cc * 3)
    x, buf, xv, strides = nhwc_view(rng, B, H, W, Cc, strided, offset, False)
    xd = x.reshape(-1, Cc).astype(np.float64)
    xh = (xd - xd.mean(0)) / np.sqrt(xd.var(0) + EPS)
    a, b = rng.uniform(-2, 2, Cc), rng.uniform(-1, 1, Cc)
    dy = (a * xh + b + 1e-3 * rng.standard_normal(xh.shape)).astype(np.float32).reshape(x.shape)
    if strided:
        dbuf = torch.full_like(buf, float("nan"))
        dbuf[..., 4:4 + Cc] = torch.from_numpy(dy).to(DEV)
        dyv = dbuf[..., 4:]
    else:
        dyv = torch.from_numpy(dy).to(DEV)
    gamma = (0.5 + rng.random(Cc)).astype(np.float32)
    draw, _, _ = _bn_backward(lib, x, xv, dyv, buf, strides, gamma, 1.0, B, H, W, Cc)
    gx, _, _ = _ref_bn_backward(x, gamma, dy, 1.0)
    xt = torch.from_numpy(x).reshape(-1, Cc).requires_grad_(True)
    y = torch.from_numpy(gamma) * (xt - xt.mean(0)) * torch.rsqrt(xt.var(0, unbiased=False) + EPS)
    (g32,) = torch.autograd.grad(y, xt, torch.from_numpy(dy).reshape(-1, Cc))
    scale = np.abs(gamma / np.sqrt(xd.var(0) + EPS) * dy.reshape(-1, Cc)).max(0)
    e_hip = (np.abs(draw.reshape(-1, Cc) - gx.reshape(-1, Cc)).max(0) / scale).max()
    e_cpu = (np.abs(g32.numpy() - gx.reshape(-1, Cc)).max(0) / scale).max()
    print("bn backward, ill-conditioned %s: HIP %.2e, CPU fp32 %.2e (of max|s dy|)" % (_case_id(case), e_hip, e_cpu))
    assert e_hip <= 4.0 * e_cpu, (e_hip, e_cpu)


def test_reduction_scratch_capacity_is_checked(lib):
    """moments and the backward column sums refuse a scratch smaller than the grid needs (status 1), as the model's
    call sites do; the grid's need is nb x 3 x C (moments) and nb x 2 x C (sums)."""
    assert grid(256 * 1024)[0] * 3 * 1024 > (1 << 20) + 32 * 20000   # C = 1024 at the cap: more than the model holds
    B, H, W, Cc = 2, 40, 50, 1024
    nb, _ = grid(B * H * W)
    x = torch.randn(B, H, W, Cc, device=DEV)
    mean, var = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    st = (H * W * Cc, W * Cc, Cc)
    need = nb * 3 * Cc
    assert lib.depgan_op_bn_moments(P(x), *st, B, H, W, Cc, P(mean), P(var), need - 1, None) == 1
    assert b"scratch" in lib.depgan_last_error()
    assert lib.depgan_op_bn_moments(P(x), *st, B, H, W, Cc, P(mean), P(var), need, None) == 0
    ones = torch.ones(Cc, device=DEV)
    out = torch.empty_like(x)
    g = torch.empty(Cc, device=DEV)
    args = (P(x), P(x), P(out), *st, B, H, W, Cc, P(ones), P(mean), P(ones), EPS, 1.0 / (B * H * W), 1.0, P(g), P(g))
    assert lib.depgan_op_bn_backward(*args, nb * 2 * Cc - 1, None) == 1
    assert lib.depgan_op_bn_backward(*args, nb * 2 * Cc, None) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# affine / FiLM / ReLU / dropout / residual: bitwise against a float32 replay of the same correctly rounded operations
# ---------------------------------------------------------------------------------------------------------------------
AFFINE_CASES = [  # B, H, W, C, strided, out_pre, film, relu, drop_seed, drop_rate, residual
    (2, 16, 16, 32, False, False, False, True, 0, 0.0, False),      # a plain conv layer's BN + ReLU
    (2, 16, 16, 32, True, True, True, True, 0, 0.0, True),          # the FiLM layer's form (u copy, FiLM, ReLU, residual)
    (3, 20, 12, 96, False, False, False, True, 77, O.DROP_RATE, False),   # the model's dropout layer
    (3, 20, 12, 96, True, True, True, False, 77, O.DROP_RATE, True),
    (2, 9, 7, 12, True, True, True, True, 5, 0.0, False),           # dropout on at rate 0: every element times 1
    (2, 9, 7, 12, False, False, True, False, 0, 0.0, True),
]


@pytest.mark.parametrize("case", AFFINE_CASES)
def test_affine_act_bitwise(lib, case):
    from dep_gan_im_amd import _lib
    B, H, W, Cc, strided, pre, film, relu, seed, rate, resid = case
    rng = np.random.default_rng(B + H + W + Cc + 7 * pre + 11 * film)
    x, buf, xv, strides = nhwc_view(rng, B, H, W, Cc, strided)
    r, rbuf, rv, _ = nhwc_view(rng, B, H, W, Cc, strided)
    s = rng.standard_normal(Cc).astype(np.float32)
    t = rng.standard_normal(Cc).astype(np.float32)
    ld, c0 = 1024, 128                              # per-sample FiLM rows: columns [c0, c0+C) of a [B][1024] buffer
    heads = rng.standard_normal((B, ld)).astype(np.float32)
    fm, fa = heads[:, c0:c0 + Cc], heads[:, c0 + 256:c0 + 256 + Cc]
    sd, td, hd = [torch.from_numpy(a).to(DEV) for a in (s, t, heads)]
    res = []
    for _ in range(2):
        out, ov = like(buf, Cc)
        prebuf, pv = like(buf, Cc) if pre else (None, None)
        rc = lib.depgan_op_affine_act(P(xv), P(ov), P(pv), P(rv) if resid else None, *strides, P(sd), P(td),
                                      P(hd[:, c0:]) if film else None, P(hd[:, c0 + 256:]) if film else None, ld,
                                      int(relu), B, H, W, Cc, seed, rate, None)
        _lib.check(rc, "affine_act")
        torch.cuda.synchronize()
        res.append((ov.cpu().numpy(), pv.cpu().numpy() if pre else None))
    assert np.array_equal(res[0][0], res[1][0])
    f32 = np.float32
    v = x * s                                       # the replay: one rounding per operation, no FMA
    v = v + t
    if pre:
        assert np.array_equal(res[0][1], v)
    if film:
        v = v * fm[:, None, None, :]
        v = v + fa[:, None, None, :]
    if relu:
        v = np.maximum(v, f32(0))
    if seed:
        keep = O.dropout_keep_mask(seed, (B, H, W, Cc), rate)
        v = np.where(keep, v * (f32(1) / (f32(1) - f32(rate))), f32(0))
        assert rate == 0 or 0.2 < 1.0 - keep.mean() < 0.3
    if resid:
        v = v + r
    assert v.dtype == np.float32
    assert np.array_equal(res[0][0], v), np.abs(res[0][0] - v).max()


# ---------------------------------------------------------------------------------------------------------------------
# softmax + Keras categorical cross-entropy
# ---------------------------------------------------------------------------------------------------------------------
def _softmax_inputs(rng, P_):
    z = (3.0 * rng.standard_normal((P_, 4))).astype(np.float32)
    lab = rng.integers(0, 4, P_)
    n = 0
    special = [[80, -80, 0, 0], [-80, 80, 80, -80], [80, 80, 80, 80], [1, 1, 1, 1], [5, 5, -3, -3], [0, 0, 0, 0],
               [-80, -80, -80, -80], [40, 0, 0, 0], [0, 40, 0, 0], [79.5, -79.5, 79.5, -79.5]]
    for row in special:
        for k in range(4):
            z[n], lab[n] = row, k
            n += 1
    # the clip's upper bound: gaps g with q0 = 1/(1 + 3 exp(-g)) around 1 - 1e-7, true class 0
    g = np.linspace(15.0, 18.5, 4000, dtype=np.float32)
    z[n:n + g.size] = 0.0
    z[n:n + g.size, 0] = g
    lab[n:n + g.size] = 0
    n += g.size
    # the lower bound: the true class 1e-7 below the others
    z[n:n + g.size] = 0.0
    z[n:n + g.size, 2] = -g + 1.1
    lab[n:n + g.size] = 2
    return z, np.eye(4, dtype=np.float32)[lab]


def test_softmax_ce4(lib):
    from dep_gan_im_amd import _lib
    rng = np.random.default_rng(3)
    P_ = 2_000_000
    z, t = _softmax_inputs(rng, P_)
    zd, td = torch.from_numpy(z).to(DEV), torch.from_numpy(t).to(DEV)
    res = []
    for _ in range(2):
        p, dz = torch.full_like(zd, float("nan")), torch.full_like(zd, float("nan"))
        ls = torch.full((1,), float("nan"), device=DEV)
        _lib.check(lib.depgan_op_softmax_ce4(P(zd), P(td), P(p), P(dz), P(ls), P_, None), "softmax_ce4")
        torch.cuda.synchronize()
        res.append((p.cpu().numpy(), dz.cpu().numpy(), ls.cpu().numpy()))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    p, dz, ls = res[0]
    assert np.isfinite(p).all() and np.isfinite(dz).all() and np.isfinite(ls).all()
    zt = torch.from_numpy(z).double().requires_grad_(True)
    p64 = torch.softmax(zt, -1)
    loss = O.keras_categorical_crossentropy_t(p64, torch.from_numpy(t).double())
    (g64,) = torch.autograd.grad(loss, zt)
    p64, g64 = p64.detach().numpy(), g64.numpy()
    assert np.abs(p - p64).max() <= 1e-6
    assert np.abs(dz - g64).max() <= 1e-5 * np.abs(g64).max()
    lsum = float(loss.detach()) * P_
    assert abs(float(ls[0]) - lsum) <= 1e-5 * lsum, (float(ls[0]), lsum)
    # outside the clip [1e-7, 1 - 1e-7] the true class's gradient is cut: the whole pixel's dz is exactly 0
    q = p64[np.arange(P_), t.argmax(-1)]
    out = (q > 1.0 - 0.5e-7) | (q < 0.5e-7)
    assert out.sum() > 100
    assert np.all(dz[out] == 0.0)
    # on the bounds themselves the gradient passes (TF clip_by_value, torch.clamp): q as the kernel forms it
    pf = p.astype(np.float32)
    S = (pf[:, 0] + pf[:, 1]) + (pf[:, 2] + pf[:, 3])
    qf = pf[np.arange(P_), t.argmax(-1)] / S
    on = (qf == np.float32(1.0) - np.float32(1e-7)) | (qf == np.float32(1e-7))
    assert on.sum() >= 1
    assert np.any(dz[on] != 0.0)
    # probabilities only (phase 0)
    p0 = torch.full_like(zd, float("nan"))
    _lib.check(lib.depgan_op_softmax_ce4(P(zd), None, P(p0), None, None, P_, None), "softmax4")
    torch.cuda.synchronize()
    assert np.array_equal(p0.cpu().numpy(), p)


# ---------------------------------------------------------------------------------------------------------------------
# noise MLP: BatchNorm over rows, small GEMMs
# ---------------------------------------------------------------------------------------------------------------------
ROWS_CASES = [  # R, C, ld, c0, relu
    (1, 32, 32, 0, True), (2, 32, 32, 0, True), (3, 32, 32, 0, True), (32, 32, 32, 0, True),
    (1, 128, 1024, 96, False), (2, 64, 1024, 480, False), (3, 32, 1024, 992, False), (32, 128, 1024, 0, False),
]


@pytest.mark.parametrize("case", ROWS_CASES)
def test_bn_rows_forward_backward(lib, case):
    from dep_gan_im_amd import _lib
    R, Cc, ld, c0, relu = case
    rng = np.random.default_rng(R * 100 + Cc + c0)
    xb = rng.standard_normal((R, ld)).astype(np.float32) + 0.3
    dyb = rng.standard_normal((R, ld)).astype(np.float32)
    gamma = (0.5 + rng.random(Cc)).astype(np.float32)
    beta = rng.standard_normal(Cc).astype(np.float32)
    mm0 = rng.standard_normal(Cc).astype(np.float32)
    mv0 = (0.5 + rng.random(Cc)).astype(np.float32)
    corr = float(np.float32(R / (R - (1.0 + EPS))))         # uresnet.hip: n / (n - (1 + eps)), -1000 at n = 1
    xd, dyd = torch.from_numpy(xb).to(DEV), torch.from_numpy(dyb).to(DEV)
    gd, bd = torch.from_numpy(gamma).to(DEV), torch.from_numpy(beta).to(DEV)
    res = []
    for _ in range(2):
        y = torch.full_like(xd, float("nan"))
        dx = torch.full_like(xd, float("nan"))
        mm, mv = torch.from_numpy(mm0).to(DEV), torch.from_numpy(mv0).to(DEV)
        mean, rstd, dg, db = [torch.full((Cc,), float("nan"), device=DEV) for _ in range(4)]
        _lib.check(lib.depgan_op_bn_rows_fwd(P(xd[:, c0:]), P(y[:, c0:]), R, Cc, ld, P(gd), P(bd), EPS, O.BN_MOMENTUM,
                                             corr, P(mm), P(mv), P(mean), P(rstd), int(relu), None), "bn_rows_fwd")
        _lib.check(lib.depgan_op_bn_rows_bwd(P(dyd[:, c0:]), P(xd[:, c0:]), P(y[:, c0:]) if relu else None,
                                             P(dx[:, c0:]), R, Cc, ld, P(gd), P(mean), P(rstd), P(dg), P(db), None),
                   "bn_rows_bwd")
        torch.cuda.synchronize()
        yh, dxh = y.cpu().numpy(), dx.cpu().numpy()
        assert np.isnan(np.delete(yh, np.s_[c0:c0 + Cc], 1)).all() and np.isnan(np.delete(dxh, np.s_[c0:c0 + Cc], 1)).all()
        res.append([yh[:, c0:c0 + Cc], dxh[:, c0:c0 + Cc]] + [v.cpu().numpy() for v in (mm, mv, dg, db)])
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    y, dx, mm, mv, dg, db = res[0]
    xt = torch.from_numpy(xb[:, c0:c0 + Cc]).double().requires_grad_(True)
    gt = torch.from_numpy(gamma).double().requires_grad_(True)
    bt = torch.from_numpy(beta).double().requires_grad_(True)
    mu, var = xt.mean(0), xt.var(0, unbiased=False)
    yt = gt * (xt - mu) * torch.rsqrt(var + EPS) + bt
    if relu:
        yt = torch.relu(yt)
    gx, gg, gb = torch.autograd.grad(yt, [xt, gt, bt], torch.from_numpy(dyb[:, c0:c0 + Cc]).double())
    mm_ref = mm0 * O.BN_MOMENTUM + mu.detach().numpy() * (1 - O.BN_MOMENTUM)
    mv_ref = mv0 * O.BN_MOMENTUM + var.detach().numpy() * corr * (1 - O.BN_MOMENTUM)
    for got, want in ((y, yt.detach().numpy()), (mm, mm_ref), (mv, mv_ref), (dx, gx.numpy()), (dg, gg.numpy()),
                      (db, gb.numpy())):
        assert np.all(np.abs(got - want) <= 1e-5 * np.maximum(1.0, np.abs(want))), np.abs(got - want).max()
    if R == 1:
        # one row: x - mean is exactly 0, so y is beta, dx is 0, and the moving variance takes Keras's factor
        # n / (n - (1 + eps)) = -1000 times a zero variance (OracleUResNet.train_on_batch, generic path)
        assert corr == np.float32(-1000.0)
        assert np.array_equal(y[0], np.maximum(beta, 0) if relu else beta)
        assert np.all(dx == 0.0)
        want = (mv0 * O.BN_MOMENTUM + 0.0 * (R / (R - (1.0 + EPS))) * (1 - O.BN_MOMENTUM)).astype(np.float32)
        np.testing.assert_allclose(mv, want, rtol=1e-6)


@pytest.mark.parametrize("M", [1, 3, 32])
@pytest.mark.parametrize("K", [1, 32])
def test_small_gemm_three_forms(lib, M, K):
    from dep_gan_im_amd import _lib
    N = 32
    rng = np.random.default_rng(M * 10 + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    Bm = rng.standard_normal((K, N)).astype(np.float32)
    D = rng.standard_normal((M, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    Ad, Bd, Dd, bd = [torch.from_numpy(a).to(DEV) for a in (A, Bm, D, bias)]
    A64, B64, D64 = A.astype(np.float64), Bm.astype(np.float64), D.astype(np.float64)
    forms = [(0, Ad, Bd, bd, (M, N), A64 @ B64 + bias), (0, Ad, Bd, None, (M, N), A64 @ B64),
             (1, Ad, Dd, None, (K, N), A64.T @ D64), (2, Dd, Bd, None, (M, K), D64 @ B64.T)]
    for form, a, b, bb, shape, want in forms:
        outs = []
        for _ in range(2):
            out = torch.full(shape, float("nan"), device=DEV)
            _lib.check(lib.depgan_op_small_gemm(form, P(a), P(b), P(bb), P(out), M, K, N, None), "small_gemm")
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
        assert np.array_equal(outs[0], outs[1])
        assert _rel(outs[0], want) <= 1e-6, (form, _rel(outs[0], want))
