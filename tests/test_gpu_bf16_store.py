"""GPU: the generator forward with bf16 activation STORAGE (depgan_g_forward_bf16s and its operators).

Bound used throughout (element-wise).  bf16 keeps 8 significand bits, so |RNE_bf16(v) - v| <= 2^-8 |v|; the project's
operator criterion for the bf16 pipe against float64 of the same operands is max|got - ref| < TOL max|ref|, TOL = 1e-4
(tests/test_gpu_ops.py).  Together

    |stored - ref64| <= 2^-8 |ref64| + (1 + 2^-8) TOL S

with S the largest magnitude the contraction's error can be carried to in the epilogue chain of that tensor: max|ref64|
for a plain layer; for a FiLM layer with u the affine result, v = u mul + add and out = relu(v) + res,
S = max(max|u| max(1, max|mul|), max|v|, max|out|).  The half-ulp term dominates: truncation instead of RNE fails it.
The reference is always float64 torch on the CPU of the SAME bf16-valued operands and bf16-rounded weights.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 1e-4
HALF_ULP = 2.0 ** -8


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _bf16(a):
    """float32 -> nearest bf16 (ties to even) -> float32."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _dev_h(a, dev):
    """bf16-valued float32 array -> bf16 device tensor (exact)."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16)
    assert np.array_equal(t.to(torch.float32).numpy(), a)
    return t.to(dev)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def _nan_h(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=dev)


def _strides(t):
    """(sB, sY, sX) in elements of an (B, H, W, Ctot) tensor."""
    return t.stride(0), t.stride(1), t.stride(2)


def _within_bound(got, ref, S, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = HALF_ULP * np.abs(ref) + (1 + HALF_ULP) * TOL * S
    ratio = float((np.abs(got - ref) / bound).max())
    print("bf16 storage: %s error / bound %.3f (S %.3g, max|ref| %.3g)" % (what, ratio, S, float(np.abs(ref).max())))
    assert ratio <= 1.0, (what, ratio)
    return ratio


def _conv64(x, w, k):
    return F.conv2d(torch.from_numpy(np.asarray(x)).permute(0, 3, 1, 2).double(),
                    torch.from_numpy(np.asarray(w)).permute(3, 2, 0, 1).double(), padding=k // 2).permute(0, 2, 3, 1).numpy()


# B, H, W, Cin, Cout, k, opts.  The 3x3 and 1x1 rows of tests/test_gpu_ops.py::BF16_CASES first, then: Cin 96 / 160 / 224
# tails inside a 32-channel chunk, channel slices in and out, ragged 16 x 16 tiles, the fused pool, FiLM + residual.
CONV_CASES = [
    (2, 32, 32, 32, 32, 3, ""), (2, 48, 40, 32, 64, 3, ""), (1, 32, 32, 224, 96, 3, ""), (2, 21, 19, 64, 160, 3, ""),
    (2, 32, 32, 128, 128, 1, ""), (2, 32, 32, 48, 96, 3, ""), (1, 16, 16, 256, 256, 3, ""), (2, 30, 18, 8, 32, 3, ""),
    (2, 32, 32, 384, 96, 1, ""), (9, 112, 120, 32, 64, 3, ""), (16, 64, 64, 64, 96, 1, ""),
    (1, 32, 32, 96, 64, 3, "film"), (1, 32, 32, 160, 96, 3, "affine"), (1, 32, 32, 224, 96, 3, "film slice"),
    (2, 21, 19, 64, 64, 3, "film slice"), (2, 30, 18, 32, 64, 3, "slice"), (2, 21, 19, 96, 32, 1, "slice affine"),
    (2, 32, 32, 32, 32, 3, "pool affine"), (2, 30, 18, 64, 64, 3, "pool slice"), (3, 48, 40, 96, 96, 3, "pool"),
    (2, 64, 64, 32, 32, 3, "film pool"),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_bf16_in_bf16_out(lib, case):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co, k, opts = case
    film, affine, sliced, pool = ("film" in opts), ("affine" in opts or "film" in opts), ("slice" in opts), ("pool" in opts)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(ci * 1000 + co + k + 7 * len(opts))
    x = _bf16(rng.standard_normal((B, H, W, ci)))
    w = (rng.standard_normal((k, k, ci, co)) / np.sqrt(k * k * ci)).astype(np.float32)
    b = rng.standard_normal(co).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, co).astype(np.float32) if affine else None
    sh = rng.standard_normal(co).astype(np.float32) if affine else None
    mul = rng.uniform(-2.0, 2.0, (B, 64 + co)).astype(np.float32) if film else None
    add = rng.standard_normal((B, 64 + co)).astype(np.float32) if film else None
    res = _bf16(rng.standard_normal((B, H, W, co))) if film else None
    relu = 0 if opts == "slice" else 1

    # operands on the device; sliced: input = channels [32, 32 + ci) of a wider buffer, output / residual likewise
    ioff, ooff = (32, 64) if sliced else (0, 0)
    xin_full = _nan_h((B, H, W, ci + ioff + (8 if sliced else 0)), dev)
    xin_full[..., ioff:ioff + ci] = _dev_h(x, dev)
    xin = xin_full[..., ioff:ioff + ci]
    out_full = _nan_h((B, H, W, co + ooff + (32 if sliced else 0)), dev)
    before = _bits(out_full).copy()
    outv = out_full[..., ooff:ooff + co]
    resv = None
    if film:
        res_full = _nan_h((B, H, W, co + ooff), dev)
        res_full[..., ooff:] = _dev_h(res, dev)
        resv = res_full[..., ooff:]
    poolt = _nan_h((B, H // 2, W // 2, co), dev) if pool else None
    wd, bd = torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)
    scd = torch.from_numpy(sc).to(dev) if affine else None
    shd = torch.from_numpy(sh).to(dev) if affine else None
    muld = torch.from_numpy(mul).to(dev) if film else None
    addd = torch.from_numpy(add).to(dev) if film else None

    def run():
        rs = _strides(resv) if film else (0, 0, 0)
        _lib.check(lib.depgan_op_conv2d_bf16s(
            P(xin), *_strides(xin), P(wd), P(bd), P(scd), P(shd),
            C.c_void_p(muld.data_ptr() + 4 * 64) if film else None, C.c_void_p(addd.data_ptr() + 4 * 64) if film else None,
            64 + co, P(resv), *rs, P(outv), *_strides(outv), P(poolt), B, H, W, ci, co, k, relu, None),
            "depgan_op_conv2d_bf16s")
        torch.cuda.synchronize()
        return _bits(out_full).copy(), (_bits(poolt).copy() if pool else None)

    bits1, pool1 = run()
    bits2, pool2 = run()
    assert np.array_equal(bits1, bits2) and (not pool or np.array_equal(pool1, pool2))     # repeatable bit for bit
    # bytes outside the output slice keep the NaN pattern they were filled with
    outside = np.ones(bits1.shape[-1], bool)
    outside[ooff:ooff + co] = False
    assert np.array_equal(bits1[..., outside], before[..., outside])
    got = outv.to(torch.float32).cpu().numpy()

    u = _conv64(x, _bf16(w), k) + b.astype(np.float64)
    if affine:
        u = u * sc.astype(np.float64) + sh.astype(np.float64)
    S = None
    if film:
        m64, a64 = mul[:, 64:].astype(np.float64)[:, None, None, :], add[:, 64:].astype(np.float64)[:, None, None, :]
        v = u * m64 + a64
        ref = np.maximum(v, 0) + res.astype(np.float64)
        S = max(np.abs(u).max() * max(1.0, np.abs(m64).max()), np.abs(v).max(), np.abs(ref).max())
    else:
        ref = np.maximum(u, 0) if relu else u
        S = np.abs(ref).max()
    _within_bound(got, ref, float(S), "conv %s" % (case,))
    if pool:
        want = F.max_pool2d(outv.to(torch.float32).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).to(torch.bfloat16)
        assert np.array_equal(pool1, _bits(want))           # the max of the STORED values, bit for bit


def test_store_rounds_to_nearest_even(lib):
    """Values whose fp32 epilogue result is known exactly and is not a bf16 number.  Through the fp32 bias (x = 0) and
    through sums of two bf16-exact products (1.0 * 1 + 2^-8 * 1 is held exactly by the fp32 accumulator)."""
    from dep_gan_im_amd import _lib
    dev = torch.device("cuda:0")
    B, H, W, ci, co = 1, 16, 16, 8, 32
    u = 2.0 ** -23
    tie = 1.0 + 2.0 ** -8                                  # between 1.0 (even) and 1.0078125 (odd)
    tie_odd = 1.0078125 + 2.0 ** -8                         # between 1.0078125 (odd) and 1.015625 (even): up
    vals = [tie, tie_odd, tie + u, tie - u, tie_odd + u, tie_odd - u, -tie, -tie_odd, -(tie + u), -(tie - u),
            1.99609375, 1.99609375 + 2 * u, 1.99609375 - 2 * u, -1.99609375, 3.0e-3 + 1e-6, 1e-30, 255.5, 257.0, 0.1, -0.3,
            65535.0, 1.0, -2.5, 0.0, 3.14159274, 2.71828175, 1.00390637, 1.00390613, 100.25, 0.33333334, 7.0e5, -9.9e-4]
    bias = np.array(vals, np.float64).astype(np.float32)
    assert len(vals) == co
    wd = torch.zeros((1, 1, ci, co), device=dev)
    out = _nan_h((B, H, W, co), dev)
    x = torch.zeros((B, H, W, ci), dtype=torch.bfloat16, device=dev)
    bd = torch.from_numpy(bias).to(dev)
    args = lambda b_: (P(x), *_strides(x), P(wd), P(b_), None, None, None, None, 0, None, 0, 0, 0, P(out), *_strides(out),  # noqa: E731
                       None, B, H, W, ci, co, 1, 0, None)
    _lib.check(lib.depgan_op_conv2d_bf16s(*args(bd)), "depgan_op_conv2d_bf16s")
    torch.cuda.synchronize()
    want = torch.from_numpy(bias).to(torch.bfloat16)
    assert np.array_equal(_bits(out), np.broadcast_to(_bits(want), (B, H, W, co)))
    assert float(want[0]) == 1.0 and float(want[1]) == 1.015625 and float(want[10]) == 2.0     # the ties went to even
    # through the contraction: out[c] = 1.0 * w0[c] + 2^-8 * w1[c], both products exact, the sum exact in fp32
    w0 = np.array([1.0, 1.0078125, -1.0, -1.0078125, 1.9921875, -1.9921875, 1.0, 1.0078125] * 4, np.float32)
    w1 = np.array([1.0, 1.0, -1.0, -1.0, 1.0, -1.0, 1.0078125, 0.5] * 4, np.float32)
    wn = np.zeros((1, 1, ci, co), np.float32)
    wn[0, 0, 0], wn[0, 0, 1] = w0, w1
    assert np.array_equal(_bf16(wn), wn)
    xn = np.zeros((B, H, W, ci), np.float32)
    xn[..., 0], xn[..., 1] = 1.0, 2.0 ** -8
    exact = w0.astype(np.float64) + 2.0 ** -8 * w1.astype(np.float64)
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)        # fp32 holds the sums exactly
    x.copy_(_dev_h(xn, dev))
    wd.copy_(torch.from_numpy(wn))
    out.fill_(float("nan"))
    _lib.check(lib.depgan_op_conv2d_bf16s(*args(None)), "depgan_op_conv2d_bf16s")
    torch.cuda.synchronize()
    want = torch.from_numpy(exact.astype(np.float32)).to(torch.bfloat16)
    assert np.array_equal(_bits(out), np.broadcast_to(_bits(want), (B, H, W, co)))
    got = want.to(torch.float32).numpy()
    assert got[0] == 1.0 and got[1] == 1.015625 and got[2] == -1.0 and got[3] == -1.015625 and got[4] == 2.0   # next binade


@pytest.mark.parametrize("case", [(2, 32, 32, 32, 32, 3), (2, 21, 19, 64, 160, 3), (1, 32, 32, 224, 96, 3),
                                  (2, 32, 32, 128, 128, 1), (2, 30, 18, 8, 32, 3)])
def test_conv_equals_rounded_fp32_storage_kernel(lib, case):
    """The new kernel keeps igemm_bf16_kernel's K order (chunk, tap, 16-channel sub-chunk) and the epilogue's
    fma(acc, 1, bias): its output is RNE_bf16 of depgan_op_conv2d(path = 3) on the widened operands, bit for bit."""
    from dep_gan_im_amd import _lib
    B, H, W, ci, co, k = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(ci + 31 * co + k)
    x = _bf16(rng.standard_normal((B, H, W, ci)))
    w = (rng.standard_normal((k, k, ci, co)) / np.sqrt(k * k * ci)).astype(np.float32)
    b = rng.standard_normal(co).astype(np.float32)
    xd, wd, bd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)
    o32 = torch.full((B, H, W, co), float("nan"), device=dev)
    _lib.check(lib.depgan_op_conv2d(P(xd), P(wd), P(bd), P(o32), B, H, W, ci, co, k, 1, 3, None))
    xh, oh = _dev_h(x, dev), _nan_h((B, H, W, co), dev)
    _lib.check(lib.depgan_op_conv2d_bf16s(P(xh), *_strides(xh), P(wd), P(bd), None, None, None, None, 0, None, 0, 0, 0,
                                          P(oh), *_strides(oh), None, B, H, W, ci, co, k, 1, None))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(oh), _bits(o32.to(torch.bfloat16)))


@pytest.mark.parametrize("case", [(2, 8, 8, 128, 128), (2, 16, 12, 96, 96), (2, 24, 16, 64, 64)])
def test_deconv2x2_bf16s(lib, case):
    """The generator's three transposed convolutions (reduced spatial size): output into channels [0, C) of a
    2C-channel concat buffer through the grouped launch; the other half keeps its NaN pattern."""
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(ci + co + H)
    x = _bf16(rng.standard_normal((B, H, W, ci)))
    w = (rng.standard_normal((2, 2, co, ci)) / np.sqrt(ci)).astype(np.float32)          # (kh, kw, Cout, Cin)
    b, sc, sh = [rng.standard_normal(co).astype(np.float32) for _ in range(3)]
    sc = np.abs(sc) + 0.5
    xh = _dev_h(x, dev)
    cat = _nan_h((B, 2 * H, 2 * W, 2 * co), dev)
    before = _bits(cat).copy()
    ov = cat[..., :co]
    wd, bd, scd, shd = [torch.from_numpy(a).to(dev) for a in (w, b, sc, sh)]
    outs = []
    for _ in range(2):
        _lib.check(lib.depgan_op_deconv2x2_bf16s(P(xh), *_strides(xh), P(wd), P(bd), P(scd), P(shd), P(ov), *_strides(ov),
                                                 B, H, W, ci, co, 1, None), "depgan_op_deconv2x2_bf16s")
        torch.cuda.synchronize()
        outs.append(_bits(cat).copy())
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0][..., co:], before[..., co:])
    y = F.conv_transpose2d(torch.from_numpy(x).permute(0, 3, 1, 2).double(),
                           torch.from_numpy(_bf16(w)).permute(3, 2, 0, 1).double(), torch.from_numpy(b).double(), stride=2)
    y = y.permute(0, 2, 3, 1).numpy() * sc.astype(np.float64) + sh.astype(np.float64)
    ref = np.maximum(y, 0)
    _within_bound(ov.to(torch.float32).cpu().numpy(), ref, float(np.abs(ref).max()), "deconv %s" % (case,))


@pytest.mark.parametrize("nicg", [1, 2])
def test_edge_conv_bf16s(lib, nicg):
    from dep_gan_im_amd import _lib
    B, H, W, co = 2, 21, 19, 32
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(nicg)
    x = rng.standard_normal((B, H, W, nicg)).astype(np.float32)
    w = _bf16(rng.standard_normal((3, 3, nicg, co)) / 3.0)
    b, sc, sh = [rng.standard_normal(co).astype(np.float32) for _ in range(3)]
    sc = np.abs(sc) + 0.5
    xd, wd, bd, scd, shd = [torch.from_numpy(a).to(dev) for a in (x, w, b, sc, sh)]
    wide = _nan_h((B, H, W, co + 32), dev)
    before = _bits(wide).copy()
    ov = wide[..., 32:]
    outs = []
    for _ in range(2):
        _lib.check(lib.depgan_op_edge_conv_bf16s(P(xd), P(wd), P(bd), P(scd), P(shd), P(ov), *_strides(ov), B, H, W, nicg,
                                                 co, 1, None), "depgan_op_edge_conv_bf16s")
        torch.cuda.synchronize()
        outs.append(_bits(wide).copy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0][..., :32], before[..., :32])
    ref = np.maximum((_conv64(x, w, 3) + b.astype(np.float64)) * sc.astype(np.float64) + sh.astype(np.float64), 0)
    _within_bound(ov.to(torch.float32).cpu().numpy(), ref, float(np.abs(ref).max()), "edge conv nicg %d" % nicg)


@pytest.mark.parametrize("tanh", [0, 1])
def test_head_bf16s(lib, tanh):
    from dep_gan_im_amd import _lib
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11 + tanh)
    Pn, Cn = 3 * 37 * 29, 32
    a = _bf16(rng.standard_normal((Pn, Cn)))
    w = _bf16(rng.standard_normal(Cn) / 4.0)
    b = np.array([0.25], np.float32)
    ah, wd, bd = _dev_h(a, dev), torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)
    out = torch.full((Pn,), float("nan"), device=dev)
    _lib.check(lib.depgan_op_head_bf16s(P(ah), P(wd), P(bd), P(out), Pn, Cn, tanh, None), "depgan_op_head_bf16s")
    torch.cuda.synchronize()
    ref = a.astype(np.float64) @ w.astype(np.float64) + 0.25
    ref = np.tanh(ref) if tanh else ref
    assert rel(out.cpu().numpy(), ref) < TOL


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
def _engine(B, img, PG, **kw):
    import dep_gan_im_amd as dg
    eng = dg.Engine(B, img, img, 2, **kw)
    eng.set_weights("G", PG)
    return eng


def _nchw64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 3, 1, 2)


def _nhwc_np(t):
    return t.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("img,B", [(64, 3), (256, 1)])
def test_layer_by_layer_teacher_forced(lib, img, B):
    """Every layer of oracle.gen_trunk(2, 32, 1) restated ALONE in float64 from the tensors the HIP path stored (its
    input is the captured, bf16-valued output of its producer), so that one flipped rounding cannot spread: conv / FiLM /
    deconv layers within the module's bound, pools bit-equal to max_pool2d of the captured input, the concat is the two
    captured tensors, the head within 1.01 * 2^-8 * sum_c |w_c a_c| + TOL of tanh(ref) (a = the captured gen_17; covers a
    head fed from the stored tensor and a fused one fed from the unrounded value).  No element is left out."""
    from oracle import depgan_oracle as O
    seed = 57
    PG = O.init_generator(seed, nicg=2, bias_std=0.05)
    x, _, z, _ = O.synth_batch(seed + 5, B, img, img, nicg=2)
    rng = np.random.default_rng(seed)
    x = (x + 0.02 * rng.uniform(size=x.shape)).astype(np.float32)
    eng = _engine(B, img, PG, bf16_mfma=True)
    eng.debug_capture(True)
    attr = eng.g_forward(x, z, storage="bfloat16").cpu().numpy()
    cap = {}
    trunk = O.gen_trunk(2, 32, 1)
    for ent in trunk[:-1]:
        cap[ent[1]] = eng.debug_tensor_bf16s("g/out/" + ent[1])
        assert np.array_equal(_bf16(cap[ent[1]]), cap[ent[1]])            # bf16 values, widened exactly
    eng.close()
    with torch.no_grad():
        T = O.to_torch(O.round_kernels_bf16(PG), torch.float64)
        heads = O.noise_mlp(T, torch.from_numpy(np.asarray(z, np.float32)).double())
        cur, skips, worst = _nchw64(x), {}, 0.0
        for ent in trunk:
            kind, name = ent[0], ent[1]
            if kind == "conv":
                ref = torch.relu(O._bn_infer(O._conv_same(cur, T["conv2d_" + name + "/kernel"], T["conv2d_" + name + "/bias"]),
                                             T, "bn_" + name))
                ref = _nhwc_np(ref)
                worst = max(worst, _within_bound(cap[name], ref, float(np.abs(ref).max()), name))
                cur = _nchw64(cap[name])
            elif kind == "film":
                mul_n, add_n = O.film_names(ent[4])
                u = O._bn_infer(O._conv_same(cur, T["conv2d_" + name + "/kernel"], T["conv2d_" + name + "/bias"]), T,
                                "bn_" + name)
                m, a = heads[mul_n][:, :, None, None], heads[add_n][:, :, None, None]
                v = u * m + a
                ref = torch.relu(v) + cur
                S = max(float(u.abs().max()) * max(1.0, float(m.abs().max())), float(v.abs().max()), float(ref.abs().max()))
                worst = max(worst, _within_bound(cap[name], _nhwc_np(ref), S, name))
                cur = _nchw64(cap[name])
            elif kind == "pool":
                skips[name] = cur
                want = _nhwc_np(F.max_pool2d(cur, 2)).astype(np.float32)
                assert np.array_equal(cap[name].view(np.uint32), want.view(np.uint32)), name
                cur = _nchw64(cap[name])
            elif kind == "deconv":
                w = T["deconv2d_" + name + "/kernel"]
                y = F.conv_transpose2d(cur, w.permute(3, 2, 0, 1), T["deconv2d_" + name + "/bias"], stride=2)
                ref = _nhwc_np(torch.relu(O._bn_infer(y, T, "bn_" + name)))
                worst = max(worst, _within_bound(cap[name], ref, float(np.abs(ref).max()), name))
                cur = torch.cat([_nchw64(cap[name]), skips[ent[4]]], dim=1)      # [deconv | skip]: the captured tensors
            elif kind == "head":
                a17 = _nhwc_np(cur)
                wv = T[name + "/kernel"].reshape(-1).numpy()
                ref = a17 @ wv + float(T[name + "/bias"][0])
                slack = 1.01 * HALF_ULP * (np.abs(a17) * np.abs(wv)).sum(axis=-1) + TOL
                err = np.abs(attr[..., 0].astype(np.float64) - np.tanh(ref))
                print("bf16 storage: head error / bound %.3f" % float((err / slack).max()))
                assert (err <= slack).all()
    print("bf16 storage %dx%d batch %d: worst layer error / bound %.3f" % (img, img, B, worst))


def test_batching_repeatability_and_fp32_path_undisturbed(lib):
    from oracle import depgan_oracle as O
    B, img, seed = 3, 64, 61
    PG = O.init_generator(seed, nicg=2, bias_std=0.05)
    n = 2 * B + 1
    x, _, z, _ = O.synth_batch(seed + 5, n, img, img, nicg=2)
    eng = _engine(B, img, PG, bf16_mfma=True)
    f32_before = eng.g_forward(x[:B], z[:B]).cpu().numpy()
    full = eng.g_forward(x, z, storage="bfloat16").cpu().numpy()              # batches of 3, 3 and 1
    again = eng.g_forward(x, z, storage="bfloat16").cpu().numpy()
    assert np.array_equal(full.view(np.uint32), again.view(np.uint32))
    first = eng.g_forward(x[:B], z[:B], storage="bfloat16").cpu().numpy()     # n = batch
    assert np.array_equal(first.view(np.uint32), full[:B].view(np.uint32))
    for i in range(n):                                                         # n = 1
        one = eng.g_forward(x[i:i + 1], z[i:i + 1], storage="bfloat16").cpu().numpy()
        assert np.array_equal(one.view(np.uint32), full[i:i + 1].view(np.uint32)), i
    f32_after = eng.g_forward(x[:B], z[:B]).cpu().numpy()
    assert np.array_equal(f32_before.view(np.uint32), f32_after.view(np.uint32))
    assert not np.array_equal(f32_before, first)                               # it IS another path
    eng.forward_storage = "bfloat16"                                           # the attribute is what storage=None uses
    assert np.array_equal(eng.g_forward(x[:B], z[:B]).cpu().numpy().view(np.uint32), first.view(np.uint32))
    eng.close()


def _storage_graph(T, x, z):
    """oracle.g_forward_t over gen_trunk(2, 32, 1) in fp32 torch, with every layer output rounded to bf16 where the HIP
    path stores it (test_layer_by_layer_teacher_forced is what proves they round at the same points)."""
    from oracle import depgan_oracle as O
    q = lambda t: t.to(torch.bfloat16).to(torch.float32)   # noqa: E731
    heads = O.noise_mlp(T, z)
    a = x.permute(0, 3, 1, 2)
    skips = {}
    for ent in O.gen_trunk(2, 32, 1):
        kind, name = ent[0], ent[1]
        if kind == "conv":
            a = q(torch.relu(O._bn_infer(O._conv_same(a, T["conv2d_" + name + "/kernel"], T["conv2d_" + name + "/bias"]),
                                         T, "bn_" + name)))
        elif kind == "film":
            mul_n, add_n = O.film_names(ent[4])
            u = O._bn_infer(O._conv_same(a, T["conv2d_" + name + "/kernel"], T["conv2d_" + name + "/bias"]), T, "bn_" + name)
            a = q(torch.relu(u * heads[mul_n][:, :, None, None] + heads[add_n][:, :, None, None]) + a)
        elif kind == "pool":
            skips[name] = a
            a = F.max_pool2d(a, 2)
        elif kind == "deconv":
            w = T["deconv2d_" + name + "/kernel"]
            a = F.conv_transpose2d(a, w.permute(3, 2, 0, 1), T["deconv2d_" + name + "/bias"], stride=2)
            a = torch.cat([q(torch.relu(O._bn_infer(a, T, "bn_" + name))), skips[ent[4]]], dim=1)
        elif kind == "head":
            a = torch.tanh(O._conv_same(a, T[name + "/kernel"], T[name + "/bias"]))
    return a.permute(0, 2, 3, 1).numpy()


def test_end_to_end_by_the_modes_own_criterion(lib):
    """The criterion test_config4_bf16_matrix_pipe pins the fp32-storage forward of this mode with, same inputs: no
    farther from the rounded oracle than 2.0 times the rounding's own effect in the maximum, 1.5 times in the mean, the
    rounding's own effect being the distance between two ORACLE evaluations (storage graph vs weights-only rounding)."""
    from oracle import depgan_oracle as O
    img, B, seed = 64, 2, 57
    PG = O.init_generator(seed, nicg=2, bias_std=0.05)
    x, _, z, _ = O.synth_batch(seed + 5, B, img, img, nicg=2)
    rng = np.random.default_rng(seed)
    x = (x + 0.02 * rng.uniform(size=x.shape)).astype(np.float32)
    eng = _engine(B, img, PG, bf16_mfma=True)
    attr = eng.g_forward(x, z, storage="bfloat16").cpu().numpy()
    attr32 = eng.g_forward(x, z).cpu().numpy()
    eng.close()
    PQ = O.round_kernels_bf16(PG)
    with torch.no_grad():
        want_s = _storage_graph(O.to_torch(PQ, torch.float32), torch.from_numpy(x), torch.from_numpy(np.asarray(z, np.float32)))
    want_w = O.g_predict(PQ, x, z, nicg=2)
    with O.bf16_activations():
        want_q = O.g_predict(PQ, x, z, nicg=2)
    e_s, e_round = rel(attr, want_s), rel(want_s, want_w)
    m_s, m_round = float(np.mean(np.abs(attr - want_s))), float(np.mean(np.abs(want_s - want_w)))
    e_q, eq_round = rel(attr32, want_q), rel(want_q, want_w)
    m_q, mq_round = float(np.mean(np.abs(attr32 - want_q))), float(np.mean(np.abs(want_q - want_w)))
    print("bf16 storage forward vs storage-graph oracle: max %.3e mean %.3e; the rounding's own effect max %.3e mean %.3e"
          % (e_s, m_s, e_round, m_round))
    print("fp32 storage forward (same context) vs rounded-operand oracle: max %.3e mean %.3e; the rounding's own effect "
          "max %.3e mean %.3e" % (e_q, m_q, eq_round, mq_round))
    assert e_round > 5e-3
    assert e_s < 2.0 * e_round and m_s < 1.5 * m_round, (e_s, e_round, m_s, m_round)


def test_refusals(lib):
    import dep_gan_im_amd as dg
    dev = torch.device("cuda:0")
    img = 32
    x = torch.zeros((2, img, img, 2), device=dev)
    z = torch.zeros((2, 32), device=dev)
    out = torch.zeros((2, img, img, 1), device=dev)
    for kw in ({}, {"bf16_weights": True}, {"nc_out": 4, "beta1": 0.9, "beta2": 0.999}):
        eng = dg.Engine(2, img, img, 2, **kw)
        eng.profile(True)
        eng.profile_reset()
        assert lib.depgan_g_forward_bf16s(eng.h, P(x), P(z), P(out), 2) == 3, kw
        assert b"bf16_mfma" in lib.depgan_last_error()
        assert sum(eng.profile_read(k)[1] for k in range(3)) == 0            # nothing was launched
        with pytest.raises(ValueError):
            eng.g_forward(x, z, storage="bfloat16")
        with pytest.raises(ValueError):
            eng.forward_storage = "bfloat16"
        shape = (C.c_int * 4)()
        assert lib.depgan_debug_tensor_bf16s(eng.h, b"g/out/gen_0", None, 0, shape) != 0
        eng.close()
    eng = dg.Engine(2, img, img, 2, bf16_mfma=True)
    for n in (0, 3, -1):
        assert lib.depgan_g_forward_bf16s(eng.h, P(x), P(z), P(out), n) == 1, n
    shape = (C.c_int * 4)()
    assert lib.depgan_debug_tensor_bf16s(eng.h, b"g/out/gen_0", None, 0, shape) != 0      # no bf16-storage forward yet
    eng.forward_storage = "bfloat16"
    assert eng.forward_storage == "bfloat16"
    with pytest.raises(ValueError):
        eng.forward_storage = "float16"
    eng.g_forward(x, z)
    assert lib.depgan_debug_tensor_bf16s(eng.h, b"g/out/de_gen_9", None, 0, shape) == 0
    assert tuple(shape) == (2, img // 4, img // 4, 128)
    assert lib.depgan_debug_tensor_bf16s(eng.h, b"g/out/nope", None, 0, shape) != 0
    eng.close()


def test_profile_counts_two_bytes_per_stored_element(lib):
    """Launches go through the profiler with labels that say bf16s and algorithmic bytes at 2 per stored element: the
    convolution class of the bf16-storage forward reads and writes less than 0.55 of what the fp32-storage one does
    (weights are bf16 panels in both)."""
    from oracle import depgan_oracle as O
    B, img = 2, 64
    eng = _engine(B, img, O.init_generator(3, nicg=2), bf16_mfma=True)
    x, _, z, _ = O.synth_batch(4, B, img, img, nicg=2)
    by = {}
    for storage in ("float32", "bfloat16"):
        eng.profile(True)
        eng.profile_reset()
        eng.g_forward(x, z, storage=storage)
        torch.cuda.synchronize()
        by[storage] = eng.profile_read_bytes(0)
        assert eng.profile_read(0)[1] == 23                 # every conv / FiLM / deconv layer but gen_0
    eng.profile(False)
    eng.close()
    assert 0.3 * by["float32"] < by["bfloat16"] < 0.55 * by["float32"], by


def test_predict_mean_uses_the_bf16_storage_forward(lib):
    import dep_gan_im_amd as dg
    from dep_gan_im_amd import evaluate
    from oracle import depgan_oracle as O
    img, n, seed = 32, 3, 9
    PG = O.init_generator(seed, nicg=2, bias_std=0.05)
    x, _, _, _ = O.synth_batch(seed, n, img, img, nicg=2)
    g = dg.Gen_UNet2D((img, img, 2), inference_dtype="bfloat16")
    g.set_weights(PG)
    mean = evaluate.predict_mean(g, x, rng=np.random.RandomState(5)).cpu().numpy()
    eng = g._ensure_engine(n)
    assert eng.cfg.bf16_mfma == 1 and eng.forward_storage == "bfloat16"
    r = np.random.RandomState(5)
    acc = np.zeros((n, img, img), np.float64)
    for _ in range(10):
        noise = r.normal(size=(n, 32, 1)).astype("float32")
        pred = g.predict([x, noise])
        assert np.array_equal(pred, eng.g_forward(x, noise, storage="bfloat16").cpu().numpy())
        acc += pred[..., 0].astype(np.float64)
    assert np.array_equal(mean, acc / 10.0)
    assert not np.array_equal(g.predict([x, noise]), eng.g_forward(x, noise, storage="float32").cpu().numpy())
    # a model bound to an engine without the bf16 matrix pipe cannot honour inference_dtype="bfloat16"
    g2 = dg.Gen_UNet2D((img, img, 2), inference_dtype="bfloat16")
    g2._bind(dg.Engine(n, img, img, 2), "G")
    with pytest.raises(ValueError, match="bf16"):
        g2.predict([x, noise])
