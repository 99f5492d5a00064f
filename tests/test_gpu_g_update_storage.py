"""GPU: the generator update on bf16 activation storage (depgan_set_g_update_storage).

Exact conditions are asserted bit for bit: the update's attr against depgan_g_forward_bf16s, netG_no_update against the
scalars netG_train reports, the fused iteration against the closure schedule, everything after the mode is switched off
against an engine that never switched, the stored u against RNE_bf16 of the fp32-storage kernel's, the stored FiLM
decisions against the stored output.  Operators: |got - ref| <= 1e-4 S, S = max|ref|, against float64 of the same
operands (bf16-valued where the kernel reads bf16, dy rounded where the kernel rounds it).  End to end: the mode's own
criterion, see test_end_to_end_gradient_by_the_modes_own_criterion."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 1e-4
NETS = ("G", "D_y2", "D_dem")
FILMS = ("gen_noise_m1", "gen_noise_m2", "gen_noise_m3", "gen_noise_p4", "gen_noise_p3", "gen_noise_p2", "gen_noise_p1")


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _dev_h(a, dev):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16)
    assert np.array_equal(t.to(torch.float32).numpy(), a)
    return t.to(dev)


def _hbits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def _st(t):
    return t.stride(0), t.stride(1), t.stride(2)


def _gate(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    S = float(np.abs(ref).max())
    e = float(np.abs(got - ref).max())
    print("g-update bf16s: %s max error %.3e = %.3f x 1e-4 S (S %.3g)" % (what, e, e / (TOL * S), S))
    assert np.isfinite(got).all() and e <= TOL * S, (what, e, S)


def _setup(img, B, seed, nb=1):
    """config-4 inputs as test_config4_bf16_matrix_pipe builds them: 2-channel input, tie-free."""
    from oracle import depgan_oracle as O
    PG = O.init_generator(seed, nicg=2, bias_std=0.05)
    PD1 = O.init_critic(seed + 1, bias_std=0.05, img=img)
    PD2 = O.init_critic(seed + 2, bias_std=0.05, img=img)
    x, y2, z, ep = O.synth_batch(seed + 5, B * nb, img, img, nicg=2)
    rng = np.random.default_rng(seed)
    x = (x + 0.02 * rng.uniform(size=x.shape)).astype(np.float32)
    y2 = (y2 + 0.02 * rng.uniform(size=y2.shape)).astype(np.float32)
    return PG, PD1, PD2, x, y2, z, ep


def _engine(img, B, PG, PD1, PD2, fwd=None, upd=None, **kw):
    import dep_gan_im_amd as dg
    kw.setdefault("bf16_mfma", True)
    eng = dg.Engine(B, img, img, 2, **kw)
    for n, Pm in zip(NETS, (PG, PD1, PD2)):
        eng.set_weights(n, Pm)
    if fwd is not None:
        eng.forward_only_storage = fwd
    if upd is not None:
        eng.g_update_storage = upd
    return eng


def _attr(eng):
    return eng.debug_tensor("g/out/gen_segmentation")


def _arenas(eng):
    from dep_gan_im_amd._lib import ARENA_ADAM_M, ARENA_ADAM_V, ARENA_PARAMS
    return [eng.get_arena(n, a) for n in NETS for a in (ARENA_PARAMS, ARENA_ADAM_M, ARENA_ADAM_V)]


def _trainers(img, B, PG, PD1, PD2, **kw):
    import dep_gan_im_amd as dg
    nets = [dg.Gen_UNet2D((img, img, 2)), dg.Dis_C2D_FCN1((img, img, 1)), dg.Dis_C2D_FCN1((img, img, 1))]
    for n, Pm in zip(nets, (PG, PD1, PD2)):
        n.set_weights({k: v.copy() for k, v in Pm.items()})
    return dg.build_trainers(*nets, batchSize=B, weights_dtype="bfloat16", activations_dtype="bfloat16", **kw), nets


# ---------------------------------------------------------------------------
# exact conditions 1, 2, 3, 6
# ---------------------------------------------------------------------------
def test_attr_bits_and_the_wart_is_removed(lib):
    """1. the attr of depgan_g_grads with the mode on IS depgan_g_forward_bf16s's, bit for bit.  2. with both modes on
    netG_no_update(z) and the pre-update scalars of netG_train(z) are the same six floats, for six seeds and through the
    closures of build_trainers; with only the forward-only mode on they differ (the wart this mode removes)."""
    img, B = 64, 2
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 57)
    eng = _engine(img, B, PG, PD1, PD2)
    assert lib.depgan_get_g_update_storage(eng.h) == 0 and eng.g_update_storage == "float32"     # default off
    f32 = eng.g_forward(x, z, storage="float32").cpu().numpy()
    h16 = eng.g_forward(x, z, storage="bfloat16").cpu().numpy()
    assert not same(f32, h16)
    eng.generator(x, y2, z, "grads")
    assert same(_attr(eng), f32)
    eng.g_update_storage = "bfloat16"
    assert lib.depgan_get_g_update_storage(eng.h) == 1 and lib.depgan_get_fwd_only_storage(eng.h) == 0   # independent
    eng.generator(x, y2, z, "grads")
    assert same(_attr(eng), h16)
    eng.generator(x, y2, z, "eval")
    assert same(_attr(eng), f32)                                            # the forward-only passes keep their own mode
    eng.forward_only_storage = "bfloat16"
    for seed in range(6):
        zz = np.random.default_rng(100 + seed).normal(size=(B, 32, 1)).astype(np.float32)
        ev = eng.generator(x, y2, zz, "eval")
        a_ev = _attr(eng).copy()
        gr = eng.generator(x, y2, zz, "grads")
        assert same(_attr(eng), a_ev)
        assert ev == gr and all(np.isfinite(ev)), (seed, ev, gr)
    eng.g_update_storage = "float32"
    assert eng.generator(x, y2, z, "eval") != eng.generator(x, y2, z, "grads")       # the wart, for reference
    eng.close()
    tr, nets = _trainers(img, B, PG, PD1, PD2, forward_only_storage="bfloat16", generator_update_storage="bfloat16")
    assert tr.engine.g_update_storage == "bfloat16" and lib.depgan_get_g_update_storage(tr.engine.h) == 1
    no_up = tr.netG_no_update([x, y2, z])
    trained = tr.netG_train([x, y2, z])
    assert list(no_up) == list(trained), (no_up, trained)
    assert list(tr.netG_no_update([x, y2, z])) != list(no_up)                # and the update moved the weights
    tr.engine.close()


def test_fused_generator_iteration_equals_closure_schedule_in_the_mode(lib):
    """depgan_gen_iteration == the same schedule closure by closure with both storage modes on: scalars, best index,
    weights and Adam state of all three networks, bitwise (test_fused_generator_iteration_equals_closure_schedule's
    comparison)."""
    from dep_gan_im_amd.schedule import ScheduleState, train_epoch
    img, B = 64, 2
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 171, nb=7)
    logs, weights, adam = [], [], []
    for fused in (False, True):
        tr, nets = _trainers(img, B, PG, PD1, PD2, forward_only_storage="bfloat16", generator_update_storage="bfloat16")
        st = ScheduleState()
        st.gen_iterations = 40
        log = []
        xd, yd = (torch.from_numpy(x).cuda(), torch.from_numpy(y2).cuda()) if fused else (x, y2)
        train_epoch(tr, xd, yd, batchSize=B, Diters=3, k_noise=4, state=st, rng=np.random.RandomState(9),
                    on_gen_iteration=log.append, fused=fused)
        logs.append(log)
        weights.append([n.get_weights_dict() for n in nets])
        adam.append([tr.engine.get_adam_state(n) for n in NETS])
        assert [tr.engine.adam_step(n) for n in NETS] == [3, 7, 7]
        tr.engine.close()
    assert len(logs[0]) == len(logs[1]) == 3
    for a, b in zip(*logs):
        assert a["best_noise"] == b["best_noise"] and (a["i"], a["ii"]) == (b["i"], b["ii"])
        for k in ("errD_real", "errD_fake", "errD_real_dem", "errD_fake_dem", "errG", "errG_CY2", "errG_DEM",
                  "errG_MSE", "errG_VOL", "errG_WMH"):
            assert a[k] == b[k] and np.isfinite(a[k]), (k, a[k], b[k])
        assert a["losses_errG"] == b["losses_errG"]
        # the wart is gone inside the schedule too: the best evaluation IS what the update then reports
        assert a["losses_errG"][a["best_noise"]] == a["errG"], (a["losses_errG"], a["best_noise"], a["errG"])
    for wa, wb in zip(*weights):
        for k in wa:
            np.testing.assert_array_equal(wa[k], wb[k])
    for (ma, va), (mb, vb) in zip(*adam):
        for k in ma:
            np.testing.assert_array_equal(ma[k], mb[k])
            np.testing.assert_array_equal(va[k], vb[k])


def test_mode_off_leaves_nothing_behind(lib):
    """3. mode on (a gradient pass in it), then off: every output, gradient and post-Adam weight of depgan_g_step is
    bit-identical to a context that never had the mode on."""
    img, B = 64, 2
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 91)
    a = _engine(img, B, PG, PD1, PD2)
    b = _engine(img, B, PG, PD1, PD2)                       # never switches
    a.g_update_storage = "bfloat16"
    on = a.generator(x, y2, z, "grads")
    g_on = a.get_grads("G")
    a.g_update_storage = "float32"
    assert lib.depgan_get_g_update_storage(a.h) == 0
    res = {}
    for name, e in (("a", a), ("b", b)):
        out = [e.generator(x, y2, z, "grads")]
        grads = e.get_grads("G")
        out.append(e.generator(x, y2, z, "step"))
        out.append(e.generator(x, y2, z, "eval"))
        res[name] = (out, grads, _arenas(e), e.g_forward(x, z).cpu().numpy(), _attr(e))
    assert res["a"][0] == res["b"][0]
    assert on != res["b"][0][0]                                          # the mode was on for a
    assert any(not same(g_on[k], res["b"][1][k]) for k in g_on)
    for k in res["a"][1]:
        assert same(res["a"][1][k], res["b"][1][k]), k
    for u, v in zip(res["a"][2], res["b"][2]):
        assert same(u, v)
    assert same(res["a"][3], res["b"][3]) and same(res["a"][4], res["b"][4])
    a.close()
    b.close()


def test_refusals(lib):
    """6. the setter is refused on fp32, bf16-weights-only and nc_out = 4 contexts, before any launch; g/u/... and the
    decisions are refused before any training forward in the mode."""
    import dep_gan_im_amd as dg
    img = 32
    for kw in ({}, {"bf16_weights": True}, {"nc_out": 4, "beta1": 0.9, "beta2": 0.999}):
        eng = dg.Engine(2, img, img, 2, **kw)
        eng.profile(True)
        eng.profile_reset()
        assert lib.depgan_set_g_update_storage(eng.h, 1) == 3, kw
        msg = lib.depgan_last_error()
        assert b"depgan_set_g_update_storage" in msg and b"bf16_mfma" in msg and b"nc_out" in msg, msg
        assert lib.depgan_get_g_update_storage(eng.h) == 0
        assert lib.depgan_set_g_update_storage(eng.h, 0) == 0
        assert sum(eng.profile_read(k)[1] for k in range(3)) == 0            # nothing was launched
        with pytest.raises(ValueError, match="bf16_mfma"):
            eng.g_update_storage = "bfloat16"
        eng.close()
    PG, PD1, PD2, x, y2, z, ep = _setup(img, 2, 33)
    eng = _engine(img, 2, PG, PD1, PD2)
    for bad in (2, -1):
        assert lib.depgan_set_g_update_storage(eng.h, bad) == 1 and lib.depgan_get_g_update_storage(eng.h) == 0
    shape = (C.c_int * 4)()
    eng.g_update_storage = "bfloat16"
    assert lib.depgan_debug_tensor_bf16s(eng.h, b"g/u/gen_noise_m1", None, 0, shape) == 1       # no training forward yet
    assert lib.depgan_debug_film_decision_bf16s(eng.h, b"gen_noise_m1", None, 0, shape) == 1
    eng.g_forward(x, z, storage="bfloat16")
    eng.generator(x, y2, z, "eval")
    assert lib.depgan_debug_tensor_bf16s(eng.h, b"g/u/gen_noise_m1", None, 0, shape) == 1       # predict / eval keep no u
    eng.generator(x, y2, z, "grads")
    assert lib.depgan_debug_tensor_bf16s(eng.h, b"g/u/gen_noise_m1", None, 0, shape) == 0 and list(shape) == [2, img, img, 32]
    assert lib.depgan_debug_film_decision_bf16s(eng.h, b"gen_noise_m1", None, 0, shape) == 0
    assert lib.depgan_debug_tensor_bf16s(eng.h, b"g/u/gen_1", None, 0, shape) == 1              # not a FiLM layer
    assert lib.depgan_debug_film_decision_bf16s(eng.h, b"nope", None, 0, shape) == 1
    assert lib.depgan_debug_tensor_bf16s(eng.h, b"g/out/gen_17", None, 0, shape) == 0           # the update stores gen_17
    eng.close()


# ---------------------------------------------------------------------------
# 4, 5: the stored u and the stored FiLM decision
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 32, 32, 32, 32), (3, 21, 19, 64, 64), (1, 32, 32, 96, 96), (2, 16, 16, 128, 128)])
def test_film_training_kernel_stores_u_and_the_decision_it_took(lib, case):
    """out has the bits of depgan_op_conv2d_bf16s; u is RNE_bf16 of the pre-FiLM tensor of the fp32-storage kernel
    (depgan_op_conv2d path 3, bias only: fma(acc, 1, bias)) on the widened operands, bit for bit; the decision obeys
    decision 0 => out == res bitwise, and out != res => decision 1 (exact consequences of out = RNE(relu(v) + res) with
    a bf16-valued res), equals (v > 0) in float64 wherever |v| is not within rounding of 0, and is not trivial."""
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(ci + 31 * co + H)
    x = _bf16(rng.standard_normal((B, H, W, ci)))
    w = (rng.standard_normal((3, 3, ci, co)) / np.sqrt(9 * ci)).astype(np.float32)
    b = rng.standard_normal(co).astype(np.float32)
    mul = rng.uniform(-2.0, 2.0, (B, 64 + co)).astype(np.float32)
    add = rng.standard_normal((B, 64 + co)).astype(np.float32)
    res = _bf16(rng.standard_normal((B, H, W, co)))
    xh, rh = _dev_h(x, dev), _dev_h(res, dev)
    wd, bd, md, ad = (torch.from_numpy(a).to(dev) for a in (w, b, mul, add))
    fm, fa = C.c_void_p(md.data_ptr() + 256), C.c_void_p(ad.data_ptr() + 256)
    o_plain = torch.full((B, H, W, co), float("nan"), dtype=torch.bfloat16, device=dev)
    _lib.check(lib.depgan_op_conv2d_bf16s(P(xh), *_st(xh), P(wd), P(bd), None, None, fm, fa, 64 + co, P(rh), *_st(rh),
                                          P(o_plain), *_st(o_plain), None, B, H, W, ci, co, 3, 1, None))
    o = torch.full((B, H, W, co), float("nan"), dtype=torch.bfloat16, device=dev)
    u = torch.full((B, H, W, co), float("nan"), dtype=torch.bfloat16, device=dev)
    dec = torch.full((B * H * W * co // 8,), 0xAA, dtype=torch.uint8, device=dev)
    _lib.check(lib.depgan_op_conv2d_film_train_bf16s(P(xh), *_st(xh), P(wd), P(bd), None, None, fm, fa, 64 + co, P(rh), *_st(rh),
                                                     P(o), *_st(o), P(u), P(dec), B, H, W, ci, co, 1, None))
    u32 = torch.full((B, H, W, co), float("nan"), device=dev)
    xd = torch.from_numpy(x).to(dev)
    _lib.check(lib.depgan_op_conv2d(P(xd), P(wd), P(bd), P(u32), B, H, W, ci, co, 3, 0, 3, None))
    torch.cuda.synchronize()
    assert np.array_equal(_hbits(o), _hbits(o_plain))
    assert np.array_equal(_hbits(u), _hbits(u32.to(torch.bfloat16)))
    d = np.unpackbits(dec.cpu().numpy(), bitorder="little").reshape(B, H, W, co).astype(bool)
    ob, rb = _hbits(o), _hbits(rh)
    assert np.array_equal(ob[~d], rb[~d])                      # decision 0 => out == res, bitwise
    assert d[ob != rb].all()                                   # out != res => decision 1
    v = u32.cpu().numpy().astype(np.float64) * mul[:, None, None, 64:] + add[:, None, None, 64:]
    clear = np.abs(v) > 1e-5 * np.abs(v).max()
    assert np.array_equal(d[clear], v[clear] > 0)
    assert 0.2 < d.mean() < 0.8


def test_stored_u_and_decisions_of_every_film_layer_of_an_update(lib):
    """After depgan_g_grads in the mode, for every element of every FiLM layer: decision 0 => out_stored == res_stored
    bitwise, out_stored != res_stored => decision 1; u is bf16-valued and FiLM of it agrees in sign with the decision
    wherever the FiLM value is not within bf16 rounding of zero."""
    img, B = 64, 2
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 57)
    eng = _engine(img, B, PG, PD1, PD2, upd="bfloat16")
    eng.generator(x, y2, z, "grads")
    heads = eng.debug_tensor("g/heads").reshape(B, 1024)
    from oracle import depgan_oracle as O
    trunk = O.gen_trunk(2, 32, 1)
    for i, ent in enumerate(trunk):
        if ent[0] != "film":
            continue
        name, prev = ent[1], trunk[i - 1][1]
        out = eng.debug_tensor_bf16s("g/out/" + name)
        res = eng.debug_tensor_bf16s("g/out/" + prev)
        u = eng.debug_tensor_bf16s("g/u/" + name)
        d = eng.debug_film_decision_bf16s(name).astype(bool)
        assert d.shape == out.shape == u.shape and np.array_equal(_bf16(u), u)
        assert np.array_equal(bits(out)[~d], bits(res)[~d]), name
        assert d[bits(out) != bits(res)].all(), name
        assert (out[d] >= res[d]).all()
        print("g-update bf16s: %s decisions on %.3f" % (name, d.mean()))
        assert 0.02 < d.mean() < 0.98
    assert heads.shape == (B, 1024)
    eng.close()


# ---------------------------------------------------------------------------
# operators against float64
# ---------------------------------------------------------------------------
# B, H, W, Cin, Cout, sliced.  Every (Cin, Cout) of the generator's 3x3 layers past gen_0; full-size rows on 2 samples,
# odd batches and ragged tiles on small ones; sliced = the operand is a channel slice of a concat buffer
WG3 = [(2, 256, 256, 32, 32, False), (2, 256, 256, 96, 32, False), (2, 128, 128, 32, 64, False), (3, 64, 64, 64, 64, True),
       (2, 128, 128, 160, 64, False), (3, 64, 64, 64, 96, False), (1, 64, 64, 96, 96, True), (2, 64, 64, 224, 96, False),
       (3, 32, 32, 96, 128, False), (3, 21, 19, 128, 128, True)]


def _wgrad64(x, dy, k):
    xi = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    go = torch.from_numpy(dy).double().permute(0, 3, 1, 2)
    g = torch.nn.grad.conv2d_weight(xi, (dy.shape[-1], x.shape[-1], k, k), go, padding=k // 2)
    return g.permute(2, 3, 1, 0).numpy()


@pytest.mark.parametrize("case", WG3)
def test_wgrad_3x3_staged_from_bf16_memory(lib, case):
    """Against float64 of (x bf16-valued, dy rounded to bf16) within 1e-4 S, column sums of the UNROUNDED dy within
    1e-4 S, and bit-equal to depgan_op_conv2d_wgrad_bf16 fed the widened operand (same tiles, chunking and K order)."""
    from dep_gan_im_amd import _lib
    B, H, W, ci, co, sliced = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(ci * 7 + co + H)
    x = _bf16(rng.standard_normal((B, H, W, ci)))
    dy = (rng.standard_normal((B, H, W, co)) * rng.uniform(0.1, 2.0, co)).astype(np.float32)
    off = 32 if sliced else 0
    xfull = torch.full((B, H, W, ci + off + (8 if sliced else 0)), float("nan"), dtype=torch.bfloat16, device=dev)
    xfull[..., off:off + ci] = _dev_h(x, dev)
    xv = xfull[..., off:off + ci]
    dyd = torch.from_numpy(dy).to(dev)
    dw = torch.full((3, 3, ci, co), float("nan"), device=dev)
    cs = torch.full((co,), float("nan"), device=dev)
    _lib.check(lib.depgan_op_conv2d_wgrad_bf16s(P(xv), *_st(xv), P(dyd), *_st(dyd), P(dw), P(cs), B, H, W, ci, co, 3, 0, None))
    xd = torch.from_numpy(x).to(dev)
    dw0 = torch.full((3, 3, ci, co), float("nan"), device=dev)
    _lib.check(lib.depgan_op_conv2d_wgrad_bf16(P(xd), P(dyd), P(dw0), B, H, W, ci, co, 3, None))
    torch.cuda.synchronize()
    _gate(dw.cpu().numpy(), _wgrad64(x, _bf16(dy), 3), "wgrad 3x3 %s" % (case,))
    _gate(cs.cpu().numpy(), dy.astype(np.float64).sum(axis=(0, 1, 2)), "wgrad 3x3 column sums %s" % (case,))
    assert same(dw.cpu().numpy(), dw0.cpu().numpy())


@pytest.mark.parametrize("case", [(2, 32, 32, 128, 128), (3, 16, 12, 96, 96), (2, 128, 128, 64, 64)])
def test_wgrad_of_the_transposed_convolution_form(lib, case):
    """The four taps of Conv2DTranspose(2x2, stride 2): tap t contracts x with the pixel grid (2i + t / 2, 2j + t % 2) of
    the upstream gradient, written (Cout, Cin); float64 within 1e-4 S and bit-equal per tap to the fp32-staging kernel on
    the widened x and the gathered grid."""
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(ci + co + H)
    x = _bf16(rng.standard_normal((B, H, W, ci)))
    dout = rng.standard_normal((B, 2 * H, 2 * W, co)).astype(np.float32)
    xh, xd, dd = _dev_h(x, dev), torch.from_numpy(x).to(dev), torch.from_numpy(dout).to(dev)
    for t in range(4):
        grid = dd[:, t // 2::2, t % 2::2, :]
        dw = torch.full((co, ci), float("nan"), device=dev)
        _lib.check(lib.depgan_op_conv2d_wgrad_bf16s(P(xh), *_st(xh), C.c_void_p(grid.data_ptr()), *_st(grid), P(dw), None,
                                                    B, H, W, ci, co, 1, 1, None))
        gc = grid.contiguous()
        dw0 = torch.full((1, 1, ci, co), float("nan"), device=dev)
        _lib.check(lib.depgan_op_conv2d_wgrad_bf16(P(xd), P(gc), P(dw0), B, H, W, ci, co, 1, None))
        torch.cuda.synchronize()
        ref = np.einsum("bhwi,bhwo->oi", x.astype(np.float64), _bf16(gc.cpu().numpy()).astype(np.float64))
        _gate(dw.cpu().numpy(), ref, "wgrad deconv tap %d %s" % (t, case))
        assert same(dw.cpu().numpy(), dw0.cpu().numpy()[0, 0].T)


# B, H, W, Cin (channels of dx), Cout (channels of dy), res, mask sliced
BD3 = [(2, 256, 256, 32, 32, True, False), (2, 128, 128, 32, 64, False, False), (3, 64, 64, 64, 96, True, True),
       (2, 64, 64, 224, 96, False, False), (3, 21, 19, 96, 128, True, True), (1, 32, 32, 128, 128, True, False),
       (2, 128, 128, 160, 64, False, False), (2, 256, 256, 96, 32, False, False)]


@pytest.mark.parametrize("case", BD3)
def test_backward_data_with_a_bf16_mask(lib, case):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co, has_res, sliced = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(ci * 3 + co + H)
    dy = rng.standard_normal((B, H, W, co)).astype(np.float32)
    w = (rng.standard_normal((3, 3, ci, co)) / np.sqrt(9 * co)).astype(np.float32)
    res = rng.standard_normal((B, H, W, ci)).astype(np.float32) if has_res else None
    mask = _bf16(rng.standard_normal((B, H, W, ci)) * (rng.uniform(size=(B, H, W, ci)) > 0.3))   # zeros included
    off = 32 if sliced else 0
    mfull = torch.full((B, H, W, ci + off), float("nan"), dtype=torch.bfloat16, device=dev)
    mfull[..., off:] = _dev_h(mask, dev)
    mv = mfull[..., off:]
    dyd, wd = torch.from_numpy(dy).to(dev), torch.from_numpy(w).to(dev)
    rd = torch.from_numpy(res).to(dev) if has_res else None
    dx = torch.full((B, H, W, ci), float("nan"), device=dev)
    rs = _st(rd) if has_res else (0, 0, 0)
    _lib.check(lib.depgan_op_conv2d_bwd_data_bf16s(P(dyd), *_st(dyd), P(wd), P(rd), *rs, P(mv), *_st(mv), P(dx), *_st(dx),
                                                   B, H, W, ci, co, 0, None))
    torch.cuda.synchronize()
    g = F.conv_transpose2d(torch.from_numpy(_bf16(dy)).double().permute(0, 3, 1, 2),
                           torch.from_numpy(_bf16(w)).double().permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1).numpy()
    full = g + (res.astype(np.float64) if has_res else 0.0)
    got = dx.cpu().numpy()
    assert (got[mask <= 0] == 0).all()
    _gate(got, np.where(mask > 0, full, 0.0), "bwd-data 3x3 %s" % (case,))
    # without a mask: the plain gradient join
    _lib.check(lib.depgan_op_conv2d_bwd_data_bf16s(P(dyd), *_st(dyd), P(wd), P(rd), *rs, None, 0, 0, 0, P(dx), *_st(dx),
                                                   B, H, W, ci, co, 0, None))
    torch.cuda.synchronize()
    _gate(dx.cpu().numpy(), full, "bwd-data 3x3 no mask %s" % (case,))


# B, H, W, channels of dx, channels of dy: one tile and one chunk; ragged tiles, three channel tiles, four chunks; a K tail
# (the last chunk is partly outside the channels); eight pixel tiles, so the XCD-aware item order is taken
@pytest.mark.parametrize("case", [(1, 16, 16, 32, 32), (3, 21, 19, 96, 128), (2, 32, 32, 64, 40), (8, 16, 16, 32, 64)])
def test_backward_data_equals_the_fp32_mask_kernel_bit_for_bit(lib, case):
    """igemm_bf16_mh_kernel and igemm_bf16_kernel contract with the same included main loop over the same flipped bf16
    panel, and without bias, affine, FiLM and ReLU the shared epilogue leaves the accumulator as it is: the two entries
    agree bit for bit, and a bf16 mask selects those bits or +0.0."""
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7 * ci + co + H)
    dyd = torch.from_numpy(rng.standard_normal((B, H, W, co)).astype(np.float32)).to(dev)
    wd = torch.from_numpy((rng.standard_normal((3, 3, ci, co)) / np.sqrt(9 * co)).astype(np.float32)).to(dev)
    mask = _bf16(rng.standard_normal((B, H, W, ci)) * (rng.uniform(size=(B, H, W, ci)) > 0.3))
    assert (mask == 0).any() and (mask < 0).any() and (mask > 0).any()
    mh = _dev_h(mask, dev)
    ref = torch.full((B, H, W, ci), float("nan"), device=dev)
    _lib.check(lib.depgan_op_conv2d_bwd_data(P(dyd), P(wd), P(ref), B, H, W, ci, co, 3, 3, None))
    dx = torch.full((B, H, W, ci), float("nan"), device=dev)
    _lib.check(lib.depgan_op_conv2d_bwd_data_bf16s(P(dyd), *_st(dyd), P(wd), None, 0, 0, 0, None, 0, 0, 0, P(dx), *_st(dx),
                                                   B, H, W, ci, co, 0, None))
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    assert np.isfinite(ref).all() and same(dx.cpu().numpy(), ref)
    dx.fill_(float("nan"))
    _lib.check(lib.depgan_op_conv2d_bwd_data_bf16s(P(dyd), *_st(dyd), P(wd), None, 0, 0, 0, P(mh), *_st(mh), P(dx), *_st(dx),
                                                   B, H, W, ci, co, 0, None))
    torch.cuda.synchronize()
    assert same(dx.cpu().numpy(), np.where(mask > 0, ref, np.float32(0.0)))


@pytest.mark.parametrize("case", [(2, 32, 32, 128, 128), (3, 16, 12, 96, 96), (2, 128, 128, 64, 64)])
def test_backward_data_of_the_transposed_convolution_with_a_bf16_mask(lib, case):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(ci + 5 * co + H)
    dout = rng.standard_normal((B, 2 * H, 2 * W, co)).astype(np.float32)
    w = (rng.standard_normal((2, 2, co, ci)) / np.sqrt(4 * co)).astype(np.float32)
    mask = _bf16(rng.standard_normal((B, H, W, ci)) * (rng.uniform(size=(B, H, W, ci)) > 0.3))
    # the gradient sits in the lower channels of a concat gradient buffer, the mask is a plain tensor
    dfull = torch.full((B, 2 * H, 2 * W, co + 32), float("nan"), device=dev)
    dfull[..., :co] = torch.from_numpy(dout).to(dev)
    dv = dfull[..., :co]
    wd, mh = torch.from_numpy(w).to(dev), _dev_h(mask, dev)
    dx = torch.full((B, H, W, ci), float("nan"), device=dev)
    _lib.check(lib.depgan_op_conv2d_bwd_data_bf16s(C.c_void_p(dv.data_ptr()), *_st(dv), P(wd), None, 0, 0, 0, P(mh), *_st(mh),
                                                   P(dx), *_st(dx), B, H, W, ci, co, 1, None))
    torch.cuda.synchronize()
    g = F.conv2d(torch.from_numpy(_bf16(dout)).double().permute(0, 3, 1, 2),
                 torch.from_numpy(_bf16(w)).double().permute(3, 2, 0, 1), stride=2).permute(0, 2, 3, 1).numpy()
    got = dx.cpu().numpy()
    assert (got[mask <= 0] == 0).all()
    _gate(got, np.where(mask > 0, g, 0.0), "bwd-data deconv %s" % (case,))


@pytest.mark.parametrize("case", [(2, 128, 128, 32, True), (3, 32, 32, 64, True), (1, 16, 16, 96, False), (3, 9, 7, 32, True)])
def test_unpool_mask_with_ties_is_exact(lib, case):
    """Exact equality with a float64 restatement on inputs with ties (small-integer bf16 values, many zeros).  Tie rule,
    the fp32 kernel's: the arg-max of a window is its FIRST maximum in the order (0,0), (0,1), (1,0), (1,1).  `a` is the
    upper channel slice of a concat buffer, as the skip convolutions store it."""
    from dep_gan_im_amd import _lib
    B, Ho, Wo, Cc, has_skip = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(Cc + Ho)
    a = rng.integers(-1, 3, size=(B, 2 * Ho, 2 * Wo, Cc)).astype(np.float32)          # ties and zeros everywhere
    dpool = rng.standard_normal((B, Ho, Wo, Cc)).astype(np.float32)
    skip = rng.standard_normal((B, 2 * Ho, 2 * Wo, Cc)).astype(np.float32) if has_skip else None
    afull = torch.full((B, 2 * Ho, 2 * Wo, Cc + 64), float("nan"), dtype=torch.bfloat16, device=dev)
    afull[..., 64:] = _dev_h(a, dev)
    av = afull[..., 64:]
    dd = torch.from_numpy(dpool).to(dev)
    sd = torch.from_numpy(skip).to(dev) if has_skip else None
    out = torch.full((B, 2 * Ho, 2 * Wo, Cc), float("nan"), device=dev)
    ss = _st(sd) if has_skip else (0, 0, 0)
    _lib.check(lib.depgan_op_unpool_mask_bf16s(P(dd), *_st(dd), C.c_void_p(av.data_ptr()), *_st(av), P(sd), *ss, P(out), *_st(out),
                                               B, Ho, Wo, Cc, None))
    torch.cuda.synchronize()
    win = np.stack([a[:, 0::2, 0::2], a[:, 0::2, 1::2], a[:, 1::2, 0::2], a[:, 1::2, 1::2]], axis=-1).astype(np.float64)
    am = win.argmax(axis=-1)                                   # numpy: the first maximum
    ref = np.zeros(a.shape, np.float64) if not has_skip else skip.astype(np.float64).copy()
    for t in range(4):
        ref[:, t // 2::2, t % 2::2] += np.where(am == t, dpool.astype(np.float64), 0.0)
    # a float64 sum of two float32 values, rounded to float32, is the kernel's one float32 addition
    ref = np.where(a > 0, ref, 0.0).astype(np.float32)
    assert len(np.unique(am)) == 4 and (win.max(axis=-1, keepdims=True) == win).sum(axis=-1).max() > 1     # ties are there
    assert same(out.cpu().numpy(), ref)


@pytest.mark.parametrize("case", [(2, 64 * 64, 32), (3, 32 * 32, 64), (1, 21 * 19, 96), (2, 16 * 16, 128), (2, 256 * 256, 32)])
def test_film_backward_from_stored_u_and_decisions(lib, case):
    from dep_gan_im_amd import _lib
    B, HW, Cc = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(Cc + HW)
    dr = rng.standard_normal((B, HW, Cc)).astype(np.float32)
    u = _bf16(rng.standard_normal((B, HW, Cc)))
    d = rng.uniform(size=(B, HW, Cc)) > 0.4
    mul = rng.uniform(-2.0, 2.0, (B, 64 + Cc)).astype(np.float32)
    drd, uh, md = torch.from_numpy(dr).to(dev), _dev_h(u, dev), torch.from_numpy(mul).to(dev)
    dbits = torch.from_numpy(np.packbits(d.reshape(-1), bitorder="little")).to(dev)
    du = torch.full((B, HW, Cc), float("nan"), device=dev)
    dm = torch.full((B, 64 + Cc), float("nan"), device=dev)
    da = torch.full((B, 64 + Cc), float("nan"), device=dev)
    _lib.check(lib.depgan_op_film_bwd_bf16s(P(drd), P(uh), P(dbits), C.c_void_p(md.data_ptr() + 256), 64 + Cc, P(du),
                                            C.c_void_p(dm.data_ptr() + 256), C.c_void_p(da.data_ptr() + 256), B, HW, Cc, None))
    torch.cuda.synchronize()
    dv = np.where(d, dr.astype(np.float64), 0.0)
    assert same(du.cpu().numpy(), (np.where(d, dr, np.float32(0)) * mul[:, None, 64:]).astype(np.float32))   # one product
    _gate(dm.cpu().numpy()[:, 64:], (dv * u).sum(axis=1), "film bwd dmul %s" % (case,))
    _gate(da.cpu().numpy()[:, 64:], dv.sum(axis=1), "film bwd dadd %s" % (case,))
    assert np.isnan(dm.cpu().numpy()[:, :64]).all()


@pytest.mark.parametrize("case", [(2 * 256 * 256, 32), (3 * 21 * 19, 32), (64 * 64, 64)])
def test_head_backward_with_a_bf16_activation(lib, case):
    from dep_gan_im_amd import _lib
    Pn, Cc = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(Cc + Pn)
    a = _bf16(np.maximum(rng.standard_normal((Pn, Cc)), 0))
    dpre = rng.standard_normal(Pn).astype(np.float32)
    w = rng.standard_normal(Cc).astype(np.float32)
    ah, dd, wd = _dev_h(a, dev), torch.from_numpy(dpre).to(dev), torch.from_numpy(w).to(dev)
    dw = torch.full((Cc,), float("nan"), device=dev)
    dz = torch.full((Pn, Cc), float("nan"), device=dev)
    _lib.check(lib.depgan_op_head_bwd_bf16s(0, P(ah), Cc, None, P(dd), P(dw), Pn, Cc, None))
    _lib.check(lib.depgan_op_head_bwd_bf16s(1, P(ah), Cc, P(wd), P(dd), P(dz), Pn, Cc, None))
    torch.cuda.synchronize()
    _gate(dw.cpu().numpy(), (a.astype(np.float64) * dpre[:, None]).sum(axis=0), "head dW %s" % (case,))
    assert same(dz.cpu().numpy(), np.where(a > 0, dpre[:, None] * w[None, :], np.float32(0)).astype(np.float32))


# ---------------------------------------------------------------------------
# the mode's own end-to-end criterion
# ---------------------------------------------------------------------------
def _q_st(t):
    """round to bf16 where the HIP path stores, straight-through for the gradient"""
    q = t.detach().to(torch.float32).to(torch.bfloat16).to(t.dtype)
    return t + (q - t.detach())


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 3, 1, 2)


def _pool_pinned(a, stored):
    from oracle import depgan_oracle as O
    _, idx = F.max_pool2d(stored, 2, return_indices=True)      # first maximum in row-major order: the kernels' rule
    return O._pool_gather(a, idx)


def _g_storage_graph(T, x, z, cap, dec):
    """float64 generator with every layer output rounded (straight-through) where the HIP path stores it, evaluated under
    the decisions the HIP path took: ReLU masks = stored > 0, pool arg-max on the stored values, FiLM = stored bits."""
    from oracle import depgan_oracle as O
    heads = O.noise_mlp(T, z)
    a = x.permute(0, 3, 1, 2)
    skips = {}
    prev = None
    for ent in O.gen_trunk(2, 32, 1):
        kind, name = ent[0], ent[1]
        if kind == "conv":
            pre = O._bn_infer(O._conv_same(a, T["conv2d_" + name + "/kernel"], T["conv2d_" + name + "/bias"]), T, "bn_" + name)
            a = _q_st(pre * (_nchw(cap[name]) > 0))
        elif kind == "film":
            mul_n, add_n = O.film_names(ent[4])
            u = O._bn_infer(O._conv_same(a, T["conv2d_" + name + "/kernel"], T["conv2d_" + name + "/bias"]), T, "bn_" + name)
            v = u * heads[mul_n][:, :, None, None] + heads[add_n][:, :, None, None]
            a = _q_st(v * _nchw(dec[name].astype(np.float64)) + a)
        elif kind == "pool":
            skips[name] = a
            a = _pool_pinned(a, _nchw(cap[prev]))
        elif kind == "deconv":
            w = T["deconv2d_" + name + "/kernel"]
            y = F.conv_transpose2d(a, w.permute(3, 2, 0, 1), T["deconv2d_" + name + "/bias"], stride=2)
            y = _q_st(O._bn_infer(y, T, "bn_" + name) * (_nchw(cap[name]) > 0))
            a = torch.cat([y, skips[ent[4]]], dim=1)
        elif kind == "head":
            a = torch.tanh(O._conv_same(a, T[name + "/kernel"], T[name + "/bias"]))
        prev = name
    return a.permute(0, 2, 3, 1)


def _d_pinned(T, img, acts):
    """oracle.d_forward_t (rounded operands where the HIP build rounds them) under the critic's own decisions"""
    from oracle import depgan_oracle as O
    a = img.permute(0, 3, 1, 2)
    with O.bf16_activations():
        for name, k, ci, co, pool in O.DIS_TRUNK:
            s = _nchw(acts[name])
            a = O._conv_same(a, T["conv2d_" + name + "/kernel"], T["conv2d_" + name + "/bias"]) * (s > 0)
            if pool:
                a = _pool_pinned(a, s)
        a = O._conv_same(a, T["dis_9/kernel"], T["dis_9/bias"])
    flat = a.permute(0, 2, 3, 1).reshape(a.shape[0], -1)
    return flat @ T["dense_1/kernel"] + T["dense_1/bias"]


def _rel_l2(a, b):
    n = float(np.sqrt((np.asarray(b, np.float64) ** 2).sum()))
    return float(np.sqrt(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).sum())) / n if n > 0 else 0.0


def test_end_to_end_gradient_by_the_modes_own_criterion(lib):
    """Inputs of test_config4_bf16_matrix_pipe (64 x 64 x 2, batch 2, seed 57).  Oracle: the float64 storage graph of the
    generator and the G loss under the decisions the HIP path took (ReLU, arg-max, FiLM bits, the sign of the L1 term;
    the critics under their own captured ReLU / arg-max decisions).  Yardstick, not the code under test: d_round = the
    per-tensor relative-L2 distance between that oracle's gradient and the rounded-operand oracle's (oracle.g_grads under
    bf16_activations), both float64 -- the size of the storage rounding's own effect.  Gate: HIP mode-on gradient against
    the storage-graph oracle, per tensor, <= 2.0 d_round + 1e-4.  Printed next to it: the mode-off gradient against the
    rounded-operand oracle.  Measured on an MI355X: worst tensor dense_bn_noise_2_mul_p1/gamma, 2.67e-3 against d_round
    2.95e-3 (0.44 of the gate); mode-off against the rounded-operand oracle, decisions not pinned: worst 4.91e-2."""
    from oracle import depgan_oracle as O
    img, B, seed = 64, 2, 57
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, seed)
    eng = _engine(img, B, PG, PD1, PD2, upd="bfloat16", im_thresh=0.5)
    eng.generator(x, y2, z, "grads")
    g_on = eng.get_grads("G")
    trunk = O.gen_trunk(2, 32, 1)
    cap = {e[1]: eng.debug_tensor_bf16s("g/out/" + e[1]) for e in trunk[:-1]}
    dec = {n: eng.debug_film_decision_bf16s(n) for n in FILMS}
    attr = _attr(eng)
    acts1 = {e[0]: eng.debug_tensor("d/act/" + e[0])[:B] for e in O.DIS_TRUNK}
    acts2 = {e[0]: eng.debug_tensor("d/act/" + e[0])[B:2 * B] for e in O.DIS_TRUNK}
    eng.g_update_storage = "float32"
    eng.generator(x, y2, z, "grads")
    g_off = eng.get_grads("G")
    eng.close()

    PQ, PQ1, PQ2 = O.round_kernels_bf16(PG), O.round_kernels_bf16(PD1), O.round_kernels_bf16(PD2)
    TG = O.to_torch(PQ, torch.float64, requires_grad=True)
    T1, T2 = O.to_torch(PQ1, torch.float64), O.to_torch(PQ2, torch.float64)
    xt, yt = torch.from_numpy(x).double(), torch.from_numpy(y2).double()
    zt = torch.from_numpy(np.asarray(z, np.float32)).double()
    a = _g_storage_graph(TG, xt, zt, cap, dec)
    print("g-update bf16s: storage-graph oracle attr vs HIP attr max %.3e" % float((a.detach() - torch.from_numpy(attr).double()).abs().max()))
    y1 = xt[..., 0:1]
    real_dem = yt - y1
    sgn = torch.from_numpy(np.sign(attr.astype(np.float32) - (y2 - x[..., 0:1]).astype(np.float32))).double()
    loss = -_d_pinned(T1, y1 + a, acts1).mean() - _d_pinned(T2, a, acts2).mean() + ((a - real_dem) * sgn).mean() * 100.0
    names = O.trainable_names(PG)
    gs = torch.autograd.grad(loss, [TG[n] for n in names], allow_unused=True)
    g_s = {n: (g.numpy() if g is not None else np.zeros_like(PG[n], np.float64)) for n, g in zip(names, gs)}
    with O.bf16_activations():
        _, g_q = O.g_grads(PQ, PQ1, PQ2, x, y2, z, thr=0.5, nicg=2, dtype=torch.float64)

    worst, worst_off = (0.0, None, 0.0, 0.0), (0.0, None)
    failed = []
    for n in names:
        if not np.any(g_s[n]) and not np.any(g_on[n]):
            continue
        d_round = _rel_l2(g_q[n], g_s[n])
        e_on = _rel_l2(g_on[n], g_s[n])
        e_off = _rel_l2(g_off[n], g_q[n])
        bound = 2.0 * d_round + 1e-4
        if e_on / bound > worst[0]:
            worst = (e_on / bound, n, e_on, d_round)
        if e_off > worst_off[0]:
            worst_off = (e_off, n)
        if not (np.isfinite(g_on[n]).all() and e_on <= bound):
            failed.append((n, e_on, d_round))
    print("g-update bf16s end to end: worst tensor %s: HIP mode-on vs storage-graph oracle rel-L2 %.3e, d_round %.3e "
          "(ratio to 2 d_round + 1e-4: %.3f); mode-off vs rounded-operand oracle worst %.3e (%s)"
          % (worst[1], worst[2], worst[3], worst[0], worst_off[0], worst_off[1]))
    assert not failed, failed


def test_three_steps_in_the_mode_stay_finite_and_near_the_mode_off_trajectory(lib):
    """Three depgan_g_step with the mode on at 64 x 64: losses and weights finite; the loss gap and the weight distance to
    the mode-off trajectory are printed next to each other (test_report_best_of_10... reports the loss gap of the two
    storages: up to 3.2e-3 relative on the total loss)."""
    img, B = 64, 2
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 57)
    on = _engine(img, B, PG, PD1, PD2, upd="bfloat16")
    off = _engine(img, B, PG, PD1, PD2)
    for step in range(3):
        zz = np.random.default_rng(step).normal(size=(B, 32, 1)).astype(np.float32)
        a, b = on.generator(x, y2, zz, "step"), off.generator(x, y2, zz, "step")
        assert all(np.isfinite(a)), a
        print("g-update bf16s trajectory step %d: total loss on %.6f off %.6f (gap %.2e)" % (step, a[0], b[0], abs(a[0] - b[0])))
    wa, wb = on.get_weights("G"), off.get_weights("G")
    num = np.sqrt(sum(((wa[k].astype(np.float64) - wb[k]) ** 2).sum() for k in wa))
    den = np.sqrt(sum((wb[k].astype(np.float64) ** 2).sum() for k in wb))
    dmax = max(float(np.abs(wa[k] - wb[k]).max()) for k in wa)
    print("g-update bf16s trajectory: post-step weights rel-L2 %.3e, max |dw| %.3e (3 Adam steps of 1e-4)" % (num / den, dmax))
    assert all(np.isfinite(wa[k]).all() for k in wa)           # the distances are printed, not gated
    on.close()
    off.close()


def test_full_size_batch_32(lib):
    """256 x 256 x 2 at batch 32 with both modes on: finite, and exact condition 2 (eval == the scalars the update
    reports, the same attr bits).  The layer-wise operator gates at this size run above on 2 samples."""
    img, B = 256, 32
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 57)
    eng = _engine(img, B, PG, PD1, PD2, fwd="bfloat16", upd="bfloat16")
    ev = eng.generator(x, y2, z, "eval")
    a_ev = _attr(eng).copy()
    gr = eng.generator(x, y2, z, "grads")
    assert ev == gr and all(np.isfinite(ev)), (ev, gr)
    assert same(_attr(eng), a_ev)
    g = eng.get_grads("G")
    assert all(np.isfinite(v).all() for v in g.values()) and any(np.any(v) for v in g.values())
    st = eng.generator(x, y2, z, "step")
    assert st == ev
    assert all(np.isfinite(v).all() for v in eng.get_weights("G").values())
    eng.close()
