"""GPU: bf16 activation storage for the FORWARD-ONLY generator passes of the training closures
(depgan_set_fwd_only_storage) and the fused head of the bf16-storage forward (igemm_bf16s_head_kernel).

What is exact here is asserted bit for bit: the routed passes against depgan_g_forward_bf16s, the fused head against
the two launches, the schedule identities, and everything after the mode is switched off against an engine that never
switched.  Bounds against float64 are those of the tests named next to them."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 1e-4
HALF_ULP = 2.0 ** -8
NETS = ("G", "D_y2", "D_dem")


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def srel(got, want):
    return max(abs(a - b) / (abs(b) + 1e-3) for a, b in zip(got, want))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _hbits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def _strides(t):
    return t.stride(0), t.stride(1), t.stride(2)


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


def _engine(img, B, PG, PD1, PD2, mode=None, **kw):
    import dep_gan_im_amd as dg
    kw.setdefault("bf16_mfma", True)
    eng = dg.Engine(B, img, img, 2, **kw)
    for n, Pm in zip(NETS, (PG, PD1, PD2)):
        eng.set_weights(n, Pm)
    if mode is not None:
        eng.forward_only_storage = mode
    return eng


def _attr(eng):
    return eng.debug_tensor("g/out/gen_segmentation")


def _arenas(eng):
    from dep_gan_im_amd._lib import ARENA_ADAM_M, ARENA_ADAM_V, ARENA_PARAMS
    return [eng.get_arena(n, a) for n in NETS for a in (ARENA_PARAMS, ARENA_ADAM_M, ARENA_ADAM_V)]


# ---------------------------------------------------------------------------
# 1. wiring
# ---------------------------------------------------------------------------
def test_wiring_bitwise(lib):
    """The generator pass inside depgan_critic_grads, depgan_g_eval and depgan_g_eval_multi IS the bf16-storage forward
    with the mode on (c->attr bit-equal to depgan_g_forward_bf16s), depgan_g_grads keeps the fp32-storage one; with
    the mode off all of them are the fp32-storage forward.  Repeated after one generator update."""
    img, B = 64, 3
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 57)
    zs = np.random.default_rng(3).normal(size=(3, B, 32, 1)).astype(np.float32)
    eng = _engine(img, B, PG, PD1, PD2)
    assert lib.depgan_get_fwd_only_storage(eng.h) == 0 and eng.forward_only_storage == "float32"

    def check(mode_on):
        f32 = eng.g_forward(x, z, storage="float32").cpu().numpy()
        h16 = eng.g_forward(x, z, storage="bfloat16").cpu().numpy()
        f32_last = eng.g_forward(x, zs[-1], storage="float32").cpu().numpy()
        h16_last = eng.g_forward(x, zs[-1], storage="bfloat16").cpu().numpy()
        assert not same(f32, h16) and not same(f32_last, h16_last)       # the test can tell the paths apart
        want, want_last = (h16, h16_last) if mode_on else (f32, f32_last)
        eng.critic("D_y2", y2, x, z, ep, update=False)
        assert same(_attr(eng), want), "critic_grads D_y2"
        eng.critic("D_dem", y2, x, z, ep, update=False)
        assert same(_attr(eng), want), "critic_grads D_dem"
        eng.generator(x, y2, z, "eval")
        assert same(_attr(eng), want), "g_eval"
        eng.generator_eval_multi(x, y2, zs)
        assert same(_attr(eng), want_last), "g_eval_multi, last pass"
        eng.generator(x, y2, z, "grads")
        assert same(_attr(eng), f32), "g_grads keeps fp32 storage"

    check(False)
    eng.forward_only_storage = "bfloat16"
    assert lib.depgan_get_fwd_only_storage(eng.h) == 1 and eng.forward_only_storage == "bfloat16"
    assert eng.forward_storage == "float32"                                # predict's setting is its own
    check(True)
    w0 = eng.get_weights("G")["conv2d_gen_17/kernel"].copy()
    eng.generator(x, y2, z, "step")                                        # refreshed bf16 panels and BN affines
    assert not np.array_equal(w0, eng.get_weights("G")["conv2d_gen_17/kernel"])
    check(True)
    eng.forward_only_storage = "float32"
    assert lib.depgan_get_fwd_only_storage(eng.h) == 0
    check(False)
    eng.close()


# ---------------------------------------------------------------------------
# 2. loss pieces
# ---------------------------------------------------------------------------
def test_loss_pieces_from_the_bf16_storage_attr(lib):
    """depgan_last_sums after depgan_g_eval with the mode on: the three counts equal the host's, formed in float32 from
    the bf16-storage attr as tests/test_gpu_step_ops.py::test_gloss_sums_counts_are_exact forms them; the L1 piece is
    within that test's bound against float64, 16 * 2^-24 * sum(|attr| + |y2| + |y1|)."""
    img, B = 64, 3
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 57)
    eng = _engine(img, B, PG, PD1, PD2, mode="bfloat16", im_thresh=0.178)
    eng.generator(x, y2, z, "eval")
    sums = eng.last_sums()
    attr = _attr(eng)[..., 0]
    assert same(attr, eng.g_forward(x, z, storage="bfloat16").cpu().numpy()[..., 0])
    eng.close()
    thr = np.float32(0.178)
    y1, y2v = x[..., 0], y2[..., 0]
    wr = y2v >= thr
    wf = (y1 + attr) >= thr                                  # float32 addition, as the kernel
    counts = [float(np.count_nonzero(wr)), float(np.count_nonzero(wf)), float(np.count_nonzero(wr & wf))]
    print("fwd-only bf16: gloss counts host %s kernel %s" % (counts, sums[3:6]))
    assert sums[3:6] == counts and min(counts) > 0
    assert sums[6:] == [float(B), float(B * img * img)]
    l1 = np.abs(attr.astype(np.float64) - (y2v.astype(np.float64) - y1)).sum()
    mag = (np.abs(attr) + np.abs(y2v) + np.abs(y1)).astype(np.float64).sum()
    ratio = abs(sums[2] - l1) / (2.0 ** -24 * mag)
    print("fwd-only bf16: gloss L1 error %.3g x 2^-24 x sum|terms| (bound 16)" % ratio)
    assert ratio <= 16


# ---------------------------------------------------------------------------
# 3. schedule identities in the mode
# ---------------------------------------------------------------------------
def _trainers(img, B, PG, PD1, PD2, **kw):
    import dep_gan_im_amd as dg
    nets = [dg.Gen_UNet2D((img, img, 2)), dg.Dis_C2D_FCN1((img, img, 1)), dg.Dis_C2D_FCN1((img, img, 1))]
    for n, Pm in zip(nets, (PG, PD1, PD2)):
        n.set_weights({k: v.copy() for k, v in Pm.items()})
    return dg.build_trainers(*nets, batchSize=B, weights_dtype="bfloat16", activations_dtype="bfloat16", **kw), nets


def test_schedule_identities_hold_in_the_mode(lib):
    """depgan_g_eval_multi == k single depgan_g_eval calls, and depgan_gen_iteration == the same schedule closure by
    closure: scalars, best index, weights and Adam state of all three networks, bitwise, with the mode on."""
    from dep_gan_im_amd.schedule import ScheduleState, train_epoch
    img, B = 64, 2
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 171, nb=7)
    eng = _engine(img, B, PG, PD1, PD2, mode="bfloat16")
    zs = np.random.default_rng(4).normal(size=(5, B, 32, 1)).astype(np.float32)
    single, sums1 = [], []
    for k in range(5):
        single.append(eng.generator(x[:B], y2[:B], zs[k], "eval"))
        sums1.append(eng.last_sums())
    outs, sums = eng.generator_eval_multi(x[:B], y2[:B], zs)
    assert outs == single and sums == sums1
    eng.forward_only_storage = "float32"
    assert eng.generator_eval_multi(x[:B], y2[:B], zs)[0] != outs          # and the mode is what was evaluated
    eng.close()

    logs, weights, adam = [], [], []
    for fused in (False, True):
        tr, nets = _trainers(img, B, PG, PD1, PD2, forward_only_storage="bfloat16")
        assert tr.engine.forward_only_storage == "bfloat16" and lib.depgan_get_fwd_only_storage(tr.engine.h) == 1
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
            assert a[k] == b[k], (k, a[k], b[k])
        assert a["losses_errG"] == b["losses_errG"]
    for wa, wb in zip(*weights):
        for k in wa:
            np.testing.assert_array_equal(wa[k], wb[k])
    for (ma, va), (mb, vb) in zip(*adam):
        for k in ma:
            np.testing.assert_array_equal(ma[k], mb[k])
            np.testing.assert_array_equal(va[k], vb[k])


# ---------------------------------------------------------------------------
# 4. no leak
# ---------------------------------------------------------------------------
def test_switching_off_leaves_nothing_behind(lib):
    img, B = 64, 2
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 91, nb=3)
    zs = np.random.default_rng(5).normal(size=(4, B, 32, 1)).astype(np.float32)
    xb, yb = x[:B], y2[:B]
    a = _engine(img, B, PG, PD1, PD2)
    b = _engine(img, B, PG, PD1, PD2)                       # never switches
    assert lib.depgan_get_fwd_only_storage(a.h) == 0 and lib.depgan_get_fwd_only_storage(b.h) == 0   # default off
    pred0 = a.g_forward(xb, z[:B]).cpu().numpy()
    a.forward_only_storage = "bfloat16"
    assert lib.depgan_get_fwd_only_storage(a.h) == 1
    res = {}
    for name, e in (("a", a), ("b", b)):                    # the closures that update nothing
        res[name] = [e.critic("D_y2", yb, xb, z[:B], ep[:B], update=False),
                     e.critic("D_dem", yb, xb, z[:B], ep[:B], update=False),
                     e.generator(xb, yb, z[:B], "eval"), e.generator_eval_multi(xb, yb, zs)[0]]
    assert res["a"] != res["b"]                             # the mode was on for a
    a.forward_only_storage = "float32"
    assert lib.depgan_get_fwd_only_storage(a.h) == 0
    assert same(a.g_forward(xb, z[:B]).cpu().numpy(), pred0)
    assert same(b.g_forward(xb, z[:B]).cpu().numpy(), pred0)
    later = {}
    for name, e in (("a", a), ("b", b)):
        out = [e.critic("D_y2", yb, xb, z[:B], ep[:B], update=False), e.generator(xb, yb, z[:B], "eval"),
               e.generator_eval_multi(xb, yb, zs), e.generator(xb, yb, z[:B], "grads"),
               e.critic("D_y2", yb, xb, z[:B], ep[:B]), e.critic("D_dem", yb, xb, z[:B], ep[:B]),
               e.generator(xb, yb, z[:B], "step")]
        zl = np.stack([z[B:2 * B], z[2 * B:3 * B]])
        el = np.stack([ep[B:2 * B], ep[2 * B:3 * B]])
        loop = (torch.from_numpy(x[B:]).cuda(), torch.from_numpy(y2[B:]).cuda(), zl, el, 2)
        out.append(e.gen_iteration(loop, loop, (xb, yb, zs)))
        out.append(e.generator(xb, yb, z[:B], "eval"))
        later[name] = (out, _arenas(e), [e.get_grads(n) for n in NETS], e.g_forward(xb, z[:B]).cpu().numpy())
    assert later["a"][0] == later["b"][0]
    for u, v in zip(later["a"][1], later["b"][1]):
        assert same(u, v)
    for ga, gb in zip(later["a"][2], later["b"][2]):
        for k in ga:
            assert same(ga[k], gb[k]), k
    assert same(later["a"][3], later["b"][3])
    a.close()
    b.close()


# ---------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------
def test_refusals(lib):
    import dep_gan_im_amd as dg
    img = 32
    for kw in ({}, {"bf16_weights": True}, {"nc_out": 4, "beta1": 0.9, "beta2": 0.999}):
        eng = dg.Engine(2, img, img, 2, **kw)
        eng.profile(True)
        eng.profile_reset()
        assert lib.depgan_set_fwd_only_storage(eng.h, 1) == 3, kw
        msg = lib.depgan_last_error()
        assert b"depgan_set_fwd_only_storage" in msg and b"bf16_mfma" in msg and b"nc_out" in msg, msg
        assert lib.depgan_get_fwd_only_storage(eng.h) == 0
        assert lib.depgan_set_fwd_only_storage(eng.h, 0) == 0                 # fp32 is what every context can do
        assert sum(eng.profile_read(k)[1] for k in range(3)) == 0            # nothing was launched
        with pytest.raises(ValueError, match="bf16_mfma"):
            eng.forward_only_storage = "bfloat16"
        assert eng.forward_only_storage == "float32"
        eng.close()
    eng = dg.Engine(2, img, img, 2, bf16_mfma=True)
    eng.profile(True)
    eng.profile_reset()
    for bad in (2, -1, 16):
        assert lib.depgan_set_fwd_only_storage(eng.h, bad) == 1, bad
        assert b"0 (fp32) or 1 (bf16)" in lib.depgan_last_error()
        assert lib.depgan_get_fwd_only_storage(eng.h) == 0
    with pytest.raises(ValueError):
        eng.forward_only_storage = "float16"
    assert lib.depgan_set_fwd_only_storage(eng.h, 1) == 0 and lib.depgan_get_fwd_only_storage(eng.h) == 1
    assert lib.depgan_set_fwd_only_storage(eng.h, 7) == 1 and lib.depgan_get_fwd_only_storage(eng.h) == 1
    assert sum(eng.profile_read(k)[1] for k in range(3)) == 0                # the setter itself launches nothing
    eng.close()


# ---------------------------------------------------------------------------
# 6. fused head
# ---------------------------------------------------------------------------
# B, H, W, Cin, tanh, opts: ragged = H, W not multiples of 16; slice = output is a channel slice of a wider buffer
HEAD_CASES = [(2, 32, 32, 32, 1, "affine"), (2, 21, 19, 64, 1, "affine"), (2, 21, 19, 64, 0, ""),
              (1, 30, 18, 32, 1, "slice affine"), (3, 37, 29, 32, 0, "slice"), (1, 256, 256, 32, 1, "affine")]


@pytest.mark.parametrize("case", HEAD_CASES)
def test_fused_head_operator_equals_the_two_launches(lib, case):
    from dep_gan_im_amd import _lib
    B, H, W, ci, tanh, opts = case
    co = 32
    affine, sliced = "affine" in opts, "slice" in opts
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1000 * H + ci + tanh + len(opts))
    x = _bf16(rng.standard_normal((B, H, W, ci)))
    w = (rng.standard_normal((3, 3, ci, co)) / np.sqrt(9 * ci)).astype(np.float32)
    b = rng.standard_normal(co).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, co).astype(np.float32) if affine else None
    sh = rng.standard_normal(co).astype(np.float32) if affine else None
    hw = (rng.standard_normal(co) / 4.0).astype(np.float32)
    hb = np.array([0.25], np.float32)
    xd = torch.from_numpy(x).to(torch.bfloat16).to(dev)
    wd, bd, hwd, hbd = [torch.from_numpy(t).to(dev) for t in (w, b, hw, hb)]
    scd = torch.from_numpy(sc).to(dev) if affine else None
    shd = torch.from_numpy(sh).to(dev) if affine else None
    ooff, wide = (64, co + 96) if sliced else (0, co)

    def buf():
        return torch.full((B, H, W, wide), float("nan"), dtype=torch.bfloat16, device=dev)

    def conv(out_full, head_out=None, skip=0):
        ov = out_full[..., ooff:ooff + co]
        common = (P(xd), *_strides(xd), P(wd), P(bd), P(scd), P(shd), None, None, 0, None, 0, 0, 0, P(ov), *_strides(ov),
                  None, B, H, W, ci, co, 3, 1)
        if head_out is None:
            _lib.check(lib.depgan_op_conv2d_bf16s(*common, None), "depgan_op_conv2d_bf16s")
        else:
            _lib.check(lib.depgan_op_conv2d_head_bf16s(*common, P(hwd), P(hbd), P(head_out), tanh, skip, None),
                       "depgan_op_conv2d_head_bf16s")
        torch.cuda.synchronize()

    # the two launches
    out_u = buf()
    conv(out_u)
    dense = out_u[..., ooff:ooff + co].contiguous()
    head_u = torch.full((B * H * W,), float("nan"), device=dev)
    _lib.check(lib.depgan_op_head_bf16s(P(dense), P(hwd), P(hbd), P(head_u), B * H * W, co, tanh, None), "depgan_op_head_bf16s")
    # fused, storing
    out_f = buf()
    head_f = torch.full((B, H, W), float("nan"), device=dev)
    conv(out_f, head_f)
    assert np.array_equal(_hbits(out_f), _hbits(out_u))                    # stored tensor (and the NaN outside the slice)
    assert same(head_f.cpu().numpy().reshape(-1), head_u.cpu().numpy())    # bit for bit
    assert np.isfinite(head_f.cpu().numpy()).all()
    # fused, not storing: the sentinel stays
    out_s = buf()
    before = _hbits(out_s).copy()
    head_s = torch.full((B, H, W), float("nan"), device=dev)
    conv(out_s, head_s, skip=1)
    assert np.array_equal(_hbits(out_s), before)
    assert same(head_s.cpu().numpy(), head_f.cpu().numpy())
    # float64 of the same bf16-valued operands: the head bound of test_layer_by_layer_teacher_forced
    a = dense.to(torch.float32).cpu().numpy().astype(np.float64).reshape(B, H, W, co)
    ref = a @ hw.astype(np.float64) + 0.25
    ref = np.tanh(ref) if tanh else ref
    slack = 1.01 * HALF_ULP * (np.abs(a) * np.abs(hw.astype(np.float64))).sum(axis=-1) + TOL
    err = np.abs(head_f.cpu().numpy().astype(np.float64) - ref)
    print("fused bf16s head %s: error / bound %.3g" % (case, float((err / slack).max())))
    assert (err <= slack).all()


def test_fused_head_operator_refuses_what_it_does_not_cover(lib):
    dev = torch.device("cuda:0")
    x = torch.zeros((1, 16, 16, 32), dtype=torch.bfloat16, device=dev)
    out = torch.zeros((1, 16, 16, 64), dtype=torch.bfloat16, device=dev)
    w = torch.zeros((3, 3, 32, 64), device=dev)
    hw, hb, ho = torch.zeros(64, device=dev), torch.zeros(1, device=dev), torch.zeros((1, 16, 16), device=dev)
    rc = lib.depgan_op_conv2d_head_bf16s(P(x), *_strides(x), P(w), None, None, None, None, None, 0, None, 0, 0, 0, P(out),
                                         *_strides(out), None, 1, 16, 16, 32, 64, 3, 1, P(hw), P(hb), P(ho), 1, 0, None)
    assert rc == 3 and b"32 channels" in lib.depgan_last_error()


@pytest.mark.parametrize("img,B", [(64, 3), (256, 1)])
def test_fused_head_in_the_model_and_gen_17_on_the_debug_surface(lib, img, B, tmp_path):
    """The mode-on generator output is bit-equal between the fused head and DEPGAN_BF16S_HEAD_FUSED=0 (read at create);
    the profile shows which kernels ran; gen_17 of the bf16 debug surface errors after a pass that skipped its store,
    works with debug capture on, and predict keeps its two launches."""
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 57)
    shape = (C.c_int * 4)()

    def run(fused):
        os.environ["DEPGAN_BF16S_HEAD_FUSED"] = "1" if fused else "0"
        try:
            eng = _engine(img, B, PG, PD1, PD2, mode="bfloat16")
        finally:
            del os.environ["DEPGAN_BF16S_HEAD_FUSED"]
        eng.generator(x, y2, z, "eval")                      # first use: allocates the bf16 buffers
        eng.profile(True)
        eng.profile_reset()
        eng.critic("D_y2", y2, x, z, ep, update=False)
        eng.profile(False)
        csv = str(tmp_path / ("prof_%d.csv" % fused))
        eng.profile_dump(csv)
        return eng, _attr(eng), open(csv).read()

    e1, a1, k1 = run(True)
    e0, a0, k0 = run(False)
    assert same(a1, a0)
    assert same(a1, e1.g_forward(x, z, storage="bfloat16").cpu().numpy())
    assert "igemm_bf16s_head_kernel" in k1 and "head fwd(bf16s)" not in k1 and "no store" in k1, k1
    assert "igemm_bf16s_head_kernel" not in k0 and "head fwd(bf16s)" in k0, k0
    # predict (two launches, stored gen_17) is the reference for the debug surface
    want17 = e1.debug_tensor_bf16s("g/out/gen_17")
    want16 = e1.debug_tensor_bf16s("g/out/gen_16")
    e1.generator(x, y2, z, "eval")                            # fused, store skipped
    assert lib.depgan_debug_tensor_bf16s(e1.h, b"g/out/gen_17", None, 0, shape) == 1
    assert b"did not store" in lib.depgan_last_error()
    assert same(e1.debug_tensor_bf16s("g/out/gen_16"), want16)             # every other layer stays readable
    e1.debug_capture(True)
    e1.generator(x, y2, z, "eval")                            # fused, stored
    assert same(e1.debug_tensor_bf16s("g/out/gen_17"), want17)
    assert same(_attr(e1), a1)
    e1.debug_capture(False)
    e1.critic("D_dem", y2, x, z, ep, update=False)
    assert lib.depgan_debug_tensor_bf16s(e1.h, b"g/out/gen_17", None, 0, shape) == 1
    e1.g_forward(x, z, storage="bfloat16")                    # predict stores it again
    assert same(e1.debug_tensor_bf16s("g/out/gen_17"), want17)
    # the unfused engine always stores it
    e0.generator(x, y2, z, "eval")
    assert same(e0.debug_tensor_bf16s("g/out/gen_17"), want17)
    e1.close()
    e0.close()


# ---------------------------------------------------------------------------
# 7. parity by the mode's own criterion
# ---------------------------------------------------------------------------
def test_parity_by_the_modes_own_criterion(lib):
    """Inputs and oracle of tests/test_gpu_model.py::test_config4_bf16_matrix_pipe (64x64x2, batch 2, seed 57; the
    float64 oracle with bf16-rounded operands).  netG_no_update, then the two critic closures; every network a closure
    evaluates still holds the initial weights on both sides.  Bounds (SURVEY 8d and that test): 1e-2, 3e-2 where the
    count-based M3 enters (the total loss and M3 itself).  Mode off and mode on are printed side by side."""
    import dep_gan_im_amd as dg  # noqa: F401
    from oracle import depgan_oracle as O
    img, B, seed = 64, 2, 57
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, seed)
    seq = (("netG_no_update", [x, y2, z]), ("netD_y2_train", [y2, x, z, ep]), ("netD_dem_train", [y2, x, z, ep]))
    got = {}
    for mode in ("float32", "bfloat16"):
        tr, _ = _trainers(img, B, PG, PD1, PD2, forward_only_storage=mode)
        got[mode] = [getattr(tr, name)(args) for name, args in seq]
        tr.engine.close()
    # the oracle's training closures update the dictionaries they were given: it gets its own copies, and runs last
    ref = O.OracleTrainers(*[{k: v.copy() for k, v in Pm.items()} for Pm in (PG, PD1, PD2)], nicg=2, dtype=torch.float64,
                           weights_dtype="bfloat16", activations_dtype="bfloat16")
    want = [getattr(ref, name)(args) for name, args in seq]
    dev = {}
    for i, (name, _) in enumerate(seq):
        for mode in ("float32", "bfloat16"):
            g, w = got[mode][i], want[i]
            if len(g) == 6:
                dev[(name, mode)] = (srel(g, w), srel(g[1:4], w[1:4]))
            else:
                dev[(name, mode)] = (srel(g, w), srel(g, w))
        print("fwd-only storage parity %s: oracle %s\n    mode off %s  deviation all %.3e / without M3 %.3e\n"
              "    mode on  %s  deviation all %.3e / without M3 %.3e"
              % (name, [round(v, 5) for v in want[i]], [round(v, 5) for v in got["float32"][i]], *dev[(name, "float32")],
                 [round(v, 5) for v in got["bfloat16"][i]], *dev[(name, "bfloat16")]))
    for (name, mode), (d_all, d_nom3) in dev.items():
        assert d_all < 3e-2, (name, mode, d_all)
        assert d_nom3 < 1e-2, (name, mode, d_nom3)


# ---------------------------------------------------------------------------
# 8. report, no gate
# ---------------------------------------------------------------------------
def test_report_best_of_10_agreement_and_the_no_update_vs_train_gap(lib):
    """No number is fixed for these: how often best-of-10 picks the same noise with the mode on as with it off, and how
    far netG_no_update(z*) (bf16 storage) is from the pre-update scalars netG_train(z*) reports (fp32 storage)."""
    img, B, k = 64, 2, 10
    agree, gaps, gaps_total = 0, [], []
    seeds = (11, 23, 57, 91, 131, 171)
    for seed in seeds:
        PG, PD1, PD2, x, y2, z, ep = _setup(img, B, seed)
        zs = np.random.default_rng(seed).normal(size=(k, B, 32, 1)).astype(np.float32)
        eng = _engine(img, B, PG, PD1, PD2)
        off = [o[0] for o in eng.generator_eval_multi(x, y2, zs)[0]]
        eng.forward_only_storage = "bfloat16"
        outs = eng.generator_eval_multi(x, y2, zs)[0]
        on = [o[0] for o in outs]
        b_off, b_on = int(np.argmin(off)), int(np.argmin(on))
        agree += b_off == b_on
        train = eng.generator(x, y2, zs[b_on], "grads")      # the six scalars netG_train reports, before its update
        gaps.append(srel(outs[b_on], train))
        gaps_total.append(abs(outs[b_on][0] - train[0]) / (abs(train[0]) + 1e-3))
        print("fwd-only storage seed %d: best-of-%d index off %d on %d; netG_no_update(z*) %s vs netG_train(z*) %s"
              % (seed, k, b_off, b_on, [round(v, 5) for v in outs[b_on]], [round(v, 5) for v in train]))
        assert all(np.isfinite(v) for v in on + train)
        eng.close()
    print("fwd-only storage report: best-of-%d index agrees on %d of %d seeds; largest netG_no_update vs netG_train gap "
          "%.3e over the six scalars, %.3e on the total loss" % (k, agree, len(seeds), max(gaps), max(gaps_total)))
