"""GPU parity of the whole DEP-GAN networks on non-square, non-power-of-two images (tests/rect_cases.py).

Every other whole-network test runs a square power-of-two image, where the generator's three transposed convolutions take
the fused four-tap kernels, every 3x3 layer takes Winograd, and height and width can be exchanged anywhere in the layer
tables without a test noticing.  Here the same checks -- forward against the float64 oracle, gradients per tensor against
the float64 manual oracle under the HIP pass's own decisions (tests/test_gpu_masked.py), the modes, the fused schedule,
one update of each network -- run at the sizes that reach the other branches: the grouped deconv forward with colsum + four
per-tap weight gradients for a whole network, direct and Winograd 3x3 layers inside one critic pass, H != W at every level,
a Flatten + Dense tail of 15, 3 and 12 pixels.  tests/test_rect_cases_cpu.py holds the table against the library's own
kernel choice; the kernels a real pass launched are read from the profile here.
"""
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rect_cases as RC
import test_gpu_masked as TM

pytestmark = pytest.mark.gpu
CASE = pytest.mark.parametrize("case", RC.CASES, ids=RC.IDS)
SEED = 131          # penalty in the trained regime (test_gpu_masked.setup); the CPU measurements below are this seed's


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def srel(got, want):
    return max(abs(a - b) / (abs(b) + 1e-3) for a, b in zip(got, want))


def profiled(eng, path, fn):
    """label -> kernel name of the launches fn() made"""
    eng.profile_reset()
    eng.profile(True)
    out = fn()
    eng.profile(False)
    eng.profile_dump(path)
    with open(path) as f:
        rows = list(csv.reader(f))[1:]
    return out, {r[1]: r[5] for r in rows if r[5]}


@CASE
def test_forward_against_the_float64_oracle(lib, case, tmp_path):
    """g_forward and d_forward of both critics against the float64 oracle, at the bounds of
    test_gpu_model.py::test_forward_and_eval_match_golden (generator rtol 1e-3 / atol 1e-4, critic rtol 1e-3 / atol 1e-5),
    over every output element; d_forward again with a Dense kernel whose entries all differ (a transposed Flatten order
    cannot cancel); and the kernels the two passes launched are the ones the table lists."""
    from oracle import depgan_oracle as O
    H, W, B = case.H, case.W, case.B
    PG, PD1, PD2, x, y2, z, ep = TM.setup((H, W), B, SEED)
    eng = TM.engine((H, W), B, PG, PD1, PD2)
    eng.debug_capture(False)
    attr, kg = profiled(eng, str(tmp_path / "g.csv"), lambda: eng.g_forward(x, z).cpu().numpy())
    assert attr.shape == (B, H, W, 1)
    want = O.g_predict(PG, x, z, dtype=torch.float64)
    print("%s: generator forward %.2e of the output range" % (case.name, rel(attr, want)))
    np.testing.assert_allclose(attr, want, rtol=1e-3, atol=1e-4)
    for name in RC.DECONVS:
        div, ch = RC.DECONV_LEVEL[name]
        kernel = kg["conv k1 b%d %dx%d %d->%d x4" % (B, H // div, W // div, ch, ch)]
        if name in case.fused_fwd:
            assert kernel == "deconv_fwd_kernel", (name, kernel)
        else:
            assert kernel.startswith("igemm_conv_kernel<32,1,"), (name, kernel)
    imgs = np.concatenate([y2, attr, y2 - x[..., 0:1]])                  # 3 B images: the batch the closures run
    for which, PD in (("D_y2", PD1), ("D_dem", PD2)):
        got, kd = profiled(eng, str(tmp_path / "d.csv"), lambda: eng.d_forward(which, imgs).cpu().numpy())
        want = O.d_predict(PD, imgs, dtype=torch.float64)
        print("%s: %s forward %.2e" % (case.name, which, rel(got, want)))
        np.testing.assert_allclose(got.reshape(-1), want.reshape(-1), rtol=1e-3, atol=1e-5)
        for name in RC.CRITIC_3X3:
            ci, co, div = RC.CRITIC_LEVEL[name]
            kernel = kd["conv k3 b%d %dx%d %d->%d" % (3 * B, H // div, W // div, ci, co)]
            assert kernel.startswith("wino_conv_kernel<" if name in case.wino else "igemm_conv_kernel<32,3,"), (name, kernel)
    # the Flatten + Dense tail with pixel weights that all differ
    nflat = (H // 16) * (W // 16)
    PD = dict(PD1)
    PD["dense_1/kernel"] = ((1.0 + np.arange(nflat, dtype=np.float32)) / nflat).reshape(nflat, 1)
    eng.set_weights("D_y2", PD)
    got, want = eng.d_forward("D_y2", imgs).cpu().numpy(), O.d_predict(PD, imgs, dtype=torch.float64)
    np.testing.assert_allclose(got.reshape(-1), want.reshape(-1), rtol=1e-3, atol=1e-5)
    if H // 16 > 1:      # and the weights tell the two orders apart: the column-major tail is far outside the bound
        t = dict(PD)
        t["dense_1/kernel"] = PD["dense_1/kernel"].reshape(H // 16, W // 16).T.reshape(nflat, 1).copy()
        assert rel(O.d_predict(t, imgs, dtype=torch.float64), want) > 1e-2
    eng.close()


def _masked_pass(case, split, free):
    from oracle import manual as M
    H, W, B = case.H, case.W, case.B
    PG, PD1, PD2, x, y2, z, ep = TM.setup((H, W), B, SEED, trained_regime=True)
    eng = TM.engine((H, W), B, PG, PD1, PD2, f32_split=split)
    assert eng.f32_split == split
    flips = {}
    for which, PD in (("D_y2", PD1), ("D_dem", PD2)):
        masks, _ = TM.check_critic(eng, which, PD, PG, x, y2, z, ep, B)
        if free:
            real, fake = TM.critic_real_fake(which, x, y2, eng.debug_tensor("g/out/gen_segmentation"))
            _, _, aux = M.critic_grads_manual(PD, real, fake, ep)
            f = [M.count_decision_flips(a, b) for a, b in zip(masks, aux["decisions"])]
            flips[which] = (sum(t[0] for t in f), sum(t[1] for t in f))
    masks, _ = TM.check_generator(eng, PG, PD1, PD2, x, y2, z, B)
    if free:
        dec = {}
        M.g_grads_manual(PG, PD1, PD2, x, y2, z, decisions=dec)
        f = [M.count_decision_flips(a, dec[k]) for a, k in zip(masks, ("G", "D_y2", "D_dem"))]
        flips["G"] = (sum(t[0] for t in f), sum(t[1] for t in f))
    eng.close()
    return flips


@CASE
def test_gradients_under_hip_masks(lib, case):
    """Both critics (first-order and penalty terms) and the generator against the float64 manual oracle under the
    decisions the HIP pass took: per tensor 1e-4, the bound of test_gpu_masked.py at 64 x 64 and 256 x 256.

    At 48x80 and 16x48 the free float64 evaluation is run as well and the decisions the HIP pass took differently are
    counted and held to n <= max(8, 2e-5 * tot).  The oracle's own float32 evaluation against its float64 one, seed 131,
    measured on the CPU before the first GPU run (flips of tot decisions; bound):
        48x80:  D_y2 1 of 1624320 (32), D_dem 0 of 1624320 (32), G 7 of 4470016 (89)
        16x48:  D_y2 0 of  324864 (8),  D_dem 0 of  324864 (8),  G 2 of  897280 (17)
    (seeds 31, 33, 137 at 16x48: 0 / 0 / 1, 0 / 0 / 0, 0 / 0 / 0).  The HIP pass, measured on an MI355X:
        48x80:  D_y2 1 of 1624320, D_dem 0, G 5 of 4470016;   16x48:  D_y2 0, D_dem 0, G 1 of 897280
    and its worst tensor against the masked oracle (D_y2 / D_dem / G; bound 1e-4): 48x80 3.3e-6 / 6.8e-6 / 5.3e-6, 16x48
    6.3e-6 / 8.6e-6 / 4.5e-6, 96x32 3.6e-6 / 5.1e-6 / 6.3e-6, 32x128 3.0e-6 / 4.9e-6 / 4.0e-6, 48x80 batch 3 2.3e-6 /
    3.2e-6 / 1.9e-5 (f32_split = 6 at 48x80: 1.6e-5 / 1.7e-5 / 4.6e-6).
    """
    free = case.name in ("48x80", "16x48")
    flips = _masked_pass(case, 0, free)
    if free:
        print("%s seed %d: decisions taken differently from the free fp64 evaluation: %s" % (case.name, SEED, flips))
        assert set(flips) == {"D_y2", "D_dem", "G"}
        for k, (n, tot) in flips.items():
            assert n <= max(8, 2e-5 * tot), (k, n, tot)


def test_gradients_under_hip_masks_split6_48x80(lib):
    """f32_split = 6 (fp32 operands split exactly into bf16 terms, six products on the bf16 pipe) through the same
    masked check at 48x80: per tensor 1e-4.  This mode keeps its own matrix-pipe kernels for the transposed convolutions
    (deconv_fused() is false in every split context), so at this size it differs from the native mode in the convolutions'
    ragged tiles, not in the deconv branch."""
    _masked_pass(RC.BY_NAME["48x80"], 6, False)


def test_winograd_and_direct_agree_through_the_model_48x80(lib, tmp_path):
    """DEPGAN_WINOGRAD=0 against the default at 48x80, as
    test_gpu_model.py::test_winograd_and_direct_convolutions_agree_through_the_model does at 128 x 128 and at its bounds:
    forward and critic 2e-5, loss scalars 1e-4, gradients 5e-3 in relative L2.  In the default pass of this size dis_6/7/8
    (3x5) are already direct while the rest is Winograd; with the switch off everything is."""
    H, W, B = 48, 80, 2
    PG, PD1, PD2, x, y2, z, ep = TM.setup((H, W), B, 41)

    def run(wino):
        os.environ["DEPGAN_WINOGRAD"] = "1" if wino else "0"
        try:
            eng = TM.engine((H, W), B, PG, PD1, PD2)
        finally:
            del os.environ["DEPGAN_WINOGRAD"]
        eng.debug_capture(False)
        eng.profile(True)
        fwd = eng.g_forward(x, z).cpu().numpy()
        d = eng.d_forward("D_y2", y2).cpu().numpy()
        eng.profile(False)
        csv_ = str(tmp_path / ("prof_w%d.csv" % wino))
        eng.profile_dump(csv_)
        kernels = open(csv_).read()
        gl = eng.generator(x, y2, z, "grads")
        gG = eng.get_grads("G")
        eng.critic("D_y2", y2, x, z, ep, update=False)
        gD = eng.get_grads("D_y2")
        eng.close()
        return fwd, kernels, d, gl, gG, gD

    f1, k1, d1, l1, gG1, gD1 = run(True)
    f0, k0, d0, l0, gG0, gD0 = run(False)
    assert "wino_conv" in k1 and "igemm_conv_kernel<32,3," in k1 and "wino_conv" not in k0, (k1[:300], k0[:300])
    assert "deconv_fwd_kernel" not in k1 and "deconv_fwd_kernel" not in k0
    print("48x80 winograd vs direct: forward %.2e, critic %.2e, loss scalars %.2e" % (rel(f1, f0), rel(d1, d0), srel(l1, l0)))
    assert rel(f1, f0) < 2e-5 and rel(d1, d0) < 2e-5 and srel(l1, l0) < 1e-4
    for name, a_, b_ in (("G", gG1, gG0), ("D_y2", gD1, gD0)):
        num = np.sqrt(sum(((a_[k].astype(np.float64) - b_[k]) ** 2).sum() for k in b_))
        den = np.sqrt(sum((b_[k].astype(np.float64) ** 2).sum() for k in b_))
        print("48x80 winograd vs direct: %s gradient rel-L2 %.2e" % (name, num / den))
        assert num / den < 5e-3, (name, num / den)


def test_bf16_matrix_pipe_48x80(lib):
    """A bf16_mfma context (BASELINE config 4: two-channel input, bf16 weights and activations on the bf16 matrix pipe) at
    48x80: the forward passes and one generator evaluation against the oracle under O.bf16_activations, at the bounds of
    test_gpu_model.py::test_config4_bf16_matrix_pipe.  The forward yardstick of that test is itself a measurement -- the
    effect of the activation rounding, the oracle with and without it -- and is taken here from two CPU oracle
    evaluations at this size (seed 57, measured on the CPU: generator max 1.29e-2 of the output range, mean
    1.54e-3; critic 8.9e-4): the HIP forward may be no farther from the rounded oracle than twice that (mean:
    1.5 times), the critic 2 x + 1e-3; the six loss scalars 3e-2, the critic means and M1 1e-2."""
    from dep_gan_im_amd import Engine
    from oracle import depgan_oracle as O
    H, W, B, seed = 48, 80, 2, 57
    PG, PD1, PD2, x, y2, z, ep = TM.setup((H, W), B, seed, nicg=2)
    eng = Engine(B, H, W, 2, bf16_mfma=True)
    for n, P in (("G", PG), ("D_y2", PD1), ("D_dem", PD2)):
        eng.set_weights(n, P)
    q = O.round_kernels_bf16
    attr = eng.g_forward(x, z).cpu().numpy()
    with O.bf16_activations():
        want_q = O.g_predict(q(PG), x, z, nicg=2)
        d_q = O.d_predict(q(PD1), y2)
    want_w, d_w = O.g_predict(q(PG), x, z, nicg=2), O.d_predict(q(PD1), y2)
    e_q, e_round = rel(attr, want_q), rel(want_q, want_w)
    m_q, m_round = float(np.mean(np.abs(attr - want_q))), float(np.mean(np.abs(want_q - want_w)))
    d_got = eng.d_forward("D_y2", y2).cpu().numpy()
    print("48x80 bf16 pipe: generator vs rounded-operand oracle max %.2e mean %.2e; the rounding's own effect max %.2e mean "
          "%.2e; critic %.2e, the rounding's effect on it %.2e" % (e_q, m_q, e_round, m_round, rel(d_got, d_q), rel(d_q, d_w)))
    assert e_round > 5e-3                                                # the activation rounding is visible ...
    assert e_q < 2.0 * e_round and m_q < 1.5 * m_round, (e_q, e_round, m_q, m_round)   # ... and followed to its own noise
    assert rel(d_got, d_q) < 2.0 * rel(d_q, d_w) + 1e-3, (rel(d_got, d_q), rel(d_q, d_w))
    got = eng.generator(x, y2, z, "eval")
    with O.bf16_activations():
        want = O.g_eval(q(PG), q(PD1), q(PD2), x, y2, z, nicg=2, dtype=torch.float64)
    print("48x80 bf16 pipe netG_no_update: %s vs %s" % ([round(v, 5) for v in got], [round(v, 5) for v in want]))
    assert srel(got, want) < 3e-2, (got, want)
    assert srel(got[1:4], want[1:4]) < 1e-2, (got, want)
    eng.close()


def _trainers(H, W, B, nicg, PG, PD1, PD2):
    import dep_gan_im_amd as dg
    nets = [dg.Gen_UNet2D((H, W, nicg)), dg.Dis_C2D_FCN1((H, W, 1)), dg.Dis_C2D_FCN1((H, W, 1))]
    for n, P in zip(nets, (PG, PD1, PD2)):
        n.set_weights({k: v.copy() for k, v in P.items()})
    return dg.build_trainers(*nets, batchSize=B), nets


def test_fused_generator_iteration_equals_closure_schedule_48x80(lib):
    """depgan_gen_iteration (one enqueue, per-sample strides xs = stride * H * W * nicg and ys = stride * H * W of its
    consecutive batches) against the closure-by-closure schedule at 48x80 with a two-channel generator input, so that the
    two strides differ: scalars, noise choice, weights and Adam state bit for bit, as
    test_gpu_steps.py::test_fused_generator_iteration_equals_closure_schedule at 64 x 64."""
    from dep_gan_im_amd.schedule import ScheduleState, train_epoch
    H, W, B, nb = 48, 80, 2, 7
    PG, PD1, PD2, x, y2, z, ep = TM.setup((H, W), B * nb, 171, nicg=2)
    logs, weights, adam = [], [], []
    for fused in (False, True):
        tr, nets = _trainers(H, W, B, 2, PG, PD1, PD2)
        st = ScheduleState()
        st.gen_iterations = 40                               # steady state: Diters critic steps per loop
        log = []
        xd, yd = (torch.from_numpy(x).cuda(), torch.from_numpy(y2).cuda()) if fused else (x, y2)
        train_epoch(tr, xd, yd, batchSize=B, Diters=3, k_noise=4, state=st, rng=np.random.RandomState(9),
                    on_gen_iteration=log.append, fused=fused)
        logs.append(log)
        weights.append([n.get_weights_dict() for n in nets])
        adam.append([tr.engine.get_adam_state(n) for n in ("G", "D_y2", "D_dem")])
        assert [tr.engine.adam_step(n) for n in ("G", "D_y2", "D_dem")] == [3, 7, 7]
        tr.engine.close()
    assert len(logs[0]) == len(logs[1]) == 3               # 7 batches, Diters 3: critic loops of 3, 3, 1
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


@pytest.mark.parametrize("which", ["D_y2", "D_dem", "G"])
def test_one_update_of_each_network_48x80(lib, which):
    """One update = True step at 48x80 against the float64 oracle's gradient under the step's own decisions and Keras Adam
    (beta_1 = 0: the first step is lr * sign(g)), through test_gpu_steps._masked_weight_check at the bounds of the
    three-step trajectories there: outputs 1e-4 (same weights on both sides), the displacement within 5 % of one step
    wherever the gradient is not rounding-sized and 2e-2 in relative L2."""
    from test_gpu_steps import _masked_weight_check
    from oracle import depgan_oracle as O
    from oracle import manual as M
    H, W, B, lr = 48, 80, 2, 1e-4
    PG, PD1, PD2, x, y2, z, ep = TM.setup((H, W), B, SEED, trained_regime=True)
    eng = TM.engine((H, W), B, PG, PD1, PD2)
    P0 = {"G": PG, "D_y2": PD1, "D_dem": PD2}[which]
    Wref = {k: v.copy() for k, v in P0.items()}
    names = O.trainable_names(P0)
    if which == "G":
        got = eng.generator(x, y2, z, "step")
        want, grads = M.g_grads_manual(PG, PD1, PD2, x, y2, z, masks=TM.hip_generator_masks(eng, x, y2, B))
        cmp = (1, 2, 3)                                      # M3 / M4 are voxel counts at a threshold
    else:
        got = eng.critic(which, y2, x, z, ep, update=True)
        attr = O.g_predict(PG, x, z, dtype=torch.float64)
        real, fake = TM.critic_real_fake(which, x.astype(np.float64), y2.astype(np.float64), attr)
        want, grads, _ = M.critic_grads_manual(P0, real, fake, ep, masks=TM.hip_critic_masks(eng, B))
        cmp = (0, 1)
    assert max(abs(got[i] - want[i]) / (abs(want[i]) + 1e-3) for i in cmp) < 1e-4, (got, want)
    O.KerasAdam(names, lr, 0.0, 0.9).apply(Wref, grads)
    assert eng.adam_step(which) == 1
    Wh = eng.get_weights(which)
    l2, worst = _masked_weight_check({k: Wh[k] for k in names}, P0, {k: Wref[k] for k in names},
                                     [{k: np.asarray(v, np.float64) for k, v in grads.items()}], lr, "48x80 " + which)
    assert worst < 0.05 and l2 < 2e-2, (which, worst, l2)
    eng.close()


@pytest.mark.parametrize("H,W", RC.REFUSED)
def test_sizes_off_the_16_pixel_grid_are_refused(lib, H, W):
    """a height or a width that is no multiple of 16 is status 1 (DEPGAN_ERR_ARG) from depgan_create, and no context is
    left behind: the handle stays null"""
    from dep_gan_im_amd import Engine, _lib
    cfg = _lib.Config(batch=2, height=H, width=W, nicg=1, first_fm=32, im_thresh=0.5, delta=10.0, lrD=1e-4, lrG=1e-4,
                      beta1=0.0, beta2=0.9, adam_eps=1e-7, nc_out=1)
    h = C.c_void_p()
    assert lib.depgan_create(C.byref(cfg), C.byref(h)) == 1
    assert h.value is None and b"multiples of 16" in lib.depgan_last_error()
    with pytest.raises(_lib.DepganError):
        Engine(2, H, W, 1)
