"""GPU: the DEP-UResNet with a class count other than the reference's four, and with integer labels, through the C ABI and
the Keras-style facade, at 64 x 64 x 1.

Exact statements are bit for bit: integer labels against their one-hot encoding (four classes: loss, every gradient
tensor, every moving statistic, the arenas after two steps), the inference context's trunk against the four-class one,
its output against the K-class head operator, batching.  Against the float64 oracle the criteria are those of
tests/test_gpu_uresnet.py for the four-class model: the gradient under the HIP pass's own decisions, per tensor."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
IMG = 64
# test_three_and_five_classes_against_the_oracle: the weight seed per class count.  The rule: seed 5 unless the float32
# ORACLE's own count of tensors above 1e-4 (under the HIP pass's decisions) exceeds 4, then the next of 6, 7, 8, 9.
# Kept: seed 5 for both counts.  The first device run printed, tensors above 1e-4 (HIP / the fp32 oracle under the same
# decisions): C = 3: 0 / 0 (worst tensor 1.96e-5, the oracle's fp32 worst 1.62e-5); C = 5: 1 / 0 (worst 1.06e-4 on
# dense_noise_2_add/kernel, the oracle's fp32 worst 5.22e-5, so the per-tensor cap is 2.09e-4).
SEEDS = {3: 5, 5: 5}


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _params(seed, Cc):
    """tests/golden/make_golden.py::uresnet_params for Cc classes: a head small enough that the softmax is not saturated."""
    from oracle import depgan_oracle as O
    Pm = O.init_generator(seed, nc_out=Cc, randomize_bn=True, bias_std=0.05)
    Pm["gen_segmentation/kernel"] = (Pm["gen_segmentation/kernel"] * 0.05).astype(np.float32)
    return Pm


def _batch(seed, n, Cc):
    """(x, z, codes uint8 (n, H, W), one-hot float32 (n, H, W, Cc)): the synthetic batch with its four codes remapped to
    Cc classes by a seeded map -- every class occurs and one is rare (under 2 % of the pixels), which is asserted."""
    from oracle import depgan_oracle as O
    x, z, lab4 = O.synth_uresnet_batch(seed, n, IMG, IMG)
    c4 = lab4.argmax(-1)
    if Cc == 4:
        codes = c4
    else:
        rng = np.random.default_rng(seed)
        codes = rng.permutation(4)[c4] % min(Cc, 4)
        for extra in range(4, Cc):
            codes[rng.uniform(size=codes.shape) < 0.01] = extra
    share = np.bincount(codes.reshape(-1), minlength=Cc) / codes.size
    assert len(share) == Cc and share.min() > 0 and share.min() < 0.02, share
    codes = codes.astype(np.uint8)
    return x, z, codes, np.eye(Cc, dtype=np.float32)[codes]


def _engine(B, Pm, Cc, **kw):
    from dep_gan_im_amd import Engine
    eng = Engine(B, IMG, IMG, 1, lrG=1e-4, beta1=0.9, beta2=0.999, nc_out=Cc, **kw)
    eng.set_weights("G", Pm)
    return eng


def _arenas(eng):
    from dep_gan_im_amd import _lib
    return [eng._arena_np("G", a).copy() for a in (_lib.ARENA_PARAMS, _lib.ARENA_ADAM_M, _lib.ARENA_ADAM_V)]


def test_four_classes_sparse_equals_one_hot(lib):
    """6. two engines of batch 4 fed a short batch of 3: class codes on one, their one-hot encoding on the other."""
    B, n, ds = 4, 3, 77
    Pm = _params(5, 4)
    x, z, codes, onehot = _batch(9, n, 4)
    dense, sparse = _engine(B, Pm, 4), _engine(B, Pm, 4)
    assert sparse.uresnet(x, z, codes, "grads", drop_seed=ds) == dense.uresnet(x, z, onehot, "grads", drop_seed=ds)
    gd, gs = dense.get_grads("G"), sparse.get_grads("G")
    assert list(gd) == list(gs)
    for k in gd:
        assert np.array_equal(_u32(gd[k]), _u32(gs[k])), k
    assert any(float(np.abs(v).max()) > 0 for v in gs.values())
    wd, ws = dense.get_weights("G"), sparse.get_weights("G")
    moved = 0
    for k in wd:
        assert np.array_equal(_u32(wd[k]), _u32(ws[k])), k
        moved += "moving_" in k and not np.array_equal(wd[k], Pm[k])
    assert moved > 0
    for step in range(2):
        assert (sparse.uresnet(x, z, codes[..., None].astype(np.int64), "step", drop_seed=ds + step)
                == dense.uresnet(x, z, onehot, "step", drop_seed=ds + step)), step
    for a, b in zip(_arenas(dense), _arenas(sparse)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert dense.adam_step("G") == sparse.adam_step("G") == 2
    assert sparse.uresnet(x, z, codes.astype(np.float32), "eval") == dense.uresnet(x, z, onehot, "eval")
    dense.close()
    sparse.close()


@pytest.mark.parametrize("Cc", [3, 5])
def test_three_and_five_classes_against_the_oracle(lib, Cc):
    """7. predict, the phase-0 loss, one gradient evaluation under the HIP pass's own decisions and one Adam step, batch 4,
    by the criteria of test_predict_eval_and_grads_match_golden_and_oracle, test_phase1_gradients_under_hip_masks and
    test_short_batch_grads_step_and_eval."""
    import test_gpu_masked as TM
    from oracle import depgan_oracle as O
    B, ds = 4, 77
    Pm = _params(SEEDS[Cc], Cc)
    x, z, codes, onehot = _batch(6, B, Cc)
    eng = _engine(B, Pm, Cc)
    probs = eng.g_forward(x, z).cpu().numpy()
    assert probs.shape == (B, IMG, IMG, Cc)
    np.testing.assert_allclose(probs.sum(-1), 1.0, atol=1e-5)
    np.testing.assert_allclose(probs, O.uresnet_predict(Pm, x, z), atol=2e-5)
    p64 = torch.from_numpy(O.uresnet_predict(Pm, x, z, dtype=torch.float64))
    want0 = float(O.keras_categorical_crossentropy_t(p64, torch.from_numpy(onehot).double()))
    ev = eng.uresnet(x, z, codes, "eval")
    assert abs(ev - want0) < 1e-4 * max(1.0, abs(want0)), (ev, want0)
    assert eng.uresnet(x, z, onehot, "eval") == ev
    # learning phase 1
    loss = eng.uresnet(x, z, codes, "grads", drop_seed=ds)
    G = eng.get_grads("G")
    assert G["gen_segmentation/kernel"].shape == (1, 1, 32, Cc) and G["gen_segmentation/bias"].shape == (Cc,)
    masks = TM.hip_uresnet_masks(eng, B)
    loss64, g64, _ = O.uresnet_grads(Pm, x, z, onehot, drop_seed=ds, dtype=torch.float64, masks=masks)
    _, g32, _ = O.uresnet_grads(Pm, x, z, onehot, drop_seed=ds, dtype=torch.float32, masks=masks)
    errs, errs32 = TM.tensor_errors(G, g64), TM.tensor_errors(g32, g64)
    worst = max(errs, key=errs.get)
    print("C = %d, seed %d: loss %.6f (fp64 %.6f); worst tensor %s %.2e (the oracle's own fp32 run: %.2e there, %.2e at its "
          "worst); tensors above 1e-4: HIP %d, fp32 oracle %d; head kernel %.2e, head bias %.2e"
          % (Cc, SEEDS[Cc], loss, loss64, worst, errs[worst], errs32[worst], max(errs32.values()),
             sum(e > 1e-4 for e in errs.values()), sum(e > 1e-4 for e in errs32.values()),
             errs["gen_segmentation/kernel"], errs["gen_segmentation/bias"]))
    assert abs(loss - loss64) < 1e-5 * max(1.0, abs(loss64)), (loss, loss64)
    cap = max(1e-4, 4.0 * max(errs32.values()))
    for k in errs:
        assert errs[k] < cap, (k, errs[k], errs32[k])
    assert sum(e > 1e-4 for e in errs.values()) <= 8, sorted(errs.items(), key=lambda kv: -kv[1])[:10]
    # biases feeding a batch-statistics BN: the exact gradient is zero
    scale = max(float(np.abs(v).max()) for v in g64.values())
    dead = [k for k in g64 if float(np.abs(g64[k]).max()) <= 1e-9]
    assert len(dead) >= 24
    for k in dead:
        assert float(np.abs(G[k]).max()) < 1e-5 * scale, k
    # the step with integer labels, against the fp64 oracle's train_on_batch under the step's decisions
    eng.set_weights("G", Pm)
    got = eng.uresnet(x, z, codes, "step", drop_seed=ds)
    tr = O.OracleUResNet({k: v.copy() for k, v in Pm.items()}, dtype=torch.float64)
    want = tr.train_on_batch([x, z], onehot, drop_seed=ds, masks=TM.hip_uresnet_masks(eng, B))
    assert abs(got - want) < 1e-5 * max(1.0, abs(want)), (got, want)
    W = eng.get_weights("G")
    for k in Pm:
        if "moving_" in k:
            np.testing.assert_allclose(W[k], tr.P[k], rtol=1e-4, atol=1e-6, err_msg=k)
        else:   # Adam's first step is lr g / (|g| + eps): at most lr = 1e-4 per element, plus the rounding of the weight
            assert float(np.abs(W[k] - Pm[k]).max()) <= 1.05e-4, k
    assert eng.adam_step("G") == 1
    eng.close()


def test_out_of_range_code_applies_no_update(lib):
    """8. one pixel coded C: step_sparse returns status 1 with the count, no Adam update, the step counter stays."""
    from dep_gan_im_amd import _lib
    Cc, B = 3, 2
    Pm = _params(5, Cc)
    x, z, codes, _ = _batch(7, B, Cc)
    eng = _engine(B, Pm, Cc)
    eng.uresnet(x, z, codes, "step", drop_seed=3)                     # a non-trivial Adam state first
    before, step, nt = _arenas(eng), eng.adam_step("G"), eng._arena_np("G", _lib.ARENA_NONTRAINABLE).copy()
    assert step == 1
    bad = codes.copy()
    bad[1, 17, 40] = Cc
    xd, zd = torch.from_numpy(x).cuda(), torch.from_numpy(z.reshape(B, -1)).cuda().contiguous()
    loss = C.c_float()
    bd = torch.from_numpy(bad).cuda()
    rc = lib.depgan_uresnet_step_sparse(eng.h, P(xd), P(zd), P(bd), B, 3, C.byref(loss))
    assert rc == 1
    msg = lib.depgan_last_error()
    assert b"1 of %d" % (B * IMG * IMG) in msg and b"[0, 3)" in msg, msg
    for a, b in zip(before, _arenas(eng)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert eng.adam_step("G") == step
    # documented: the phase-1 forward moved the BatchNorm moving statistics before the count came back
    assert not np.array_equal(nt, eng._arena_np("G", _lib.ARENA_NONTRAINABLE))
    with pytest.raises(_lib.DepganError, match="1 of"):
        eng.uresnet(x, z, bad, "grads")
    wrap = codes.astype(np.int32)
    wrap[0, 0, 0] = 257                                               # does not wrap into class 1
    with pytest.raises(_lib.DepganError, match="1 of"):
        eng.uresnet(x, z, wrap, "eval")
    assert eng.uresnet(x, z, codes, "step", drop_seed=3) > 0 and eng.adam_step("G") == step + 1
    eng.close()


@pytest.mark.parametrize("K", [3, 5])
def test_inference_context(lib, K):
    """9. bf16_mfma with nc_out = K: the four-class inference context's trunk, the K-class head operator on gen_17."""
    from oracle import depgan_oracle as O
    from test_gpu_bf16_store import _bf16, _dev_h
    B, seed = 3, 57
    P4 = O.init_generator(seed, nicg=1, nc_out=4, bias_std=0.05)
    PK = dict(P4)
    hk = O.init_generator(seed + 1, nicg=1, nc_out=K, bias_std=0.05)
    PK["gen_segmentation/kernel"], PK["gen_segmentation/bias"] = hk["gen_segmentation/kernel"], hk["gen_segmentation/bias"]
    x, _, z, _ = O.synth_batch(seed + 5, B, IMG, IMG, nicg=1)
    x = (x + 0.02 * np.random.default_rng(seed).uniform(size=x.shape)).astype(np.float32)
    names = [ent[1] for ent in O.gen_trunk(1, 32, 4)[:-1]]
    e4 = _engine(B, P4, 4, bf16_mfma=True)
    e4.g_forward(x, z, storage="bfloat16")
    cap4 = {n: e4.debug_tensor_bf16s("g/out/" + n) for n in names}
    e4.close()
    eng = _engine(B, PK, K, bf16_mfma=True)
    assert eng.inference_only
    probs = eng.g_forward(x, z, storage="bfloat16").cpu().numpy()
    assert probs.shape == (B, IMG, IMG, K)
    for n in names:
        assert np.array_equal(_u32(eng.debug_tensor_bf16s("g/out/" + n)), _u32(cap4[n])), n
    # the output is the operator on the captured gen_17 with the context's (bf16-rounded) head weights
    a17 = _dev_h(cap4["gen_17"].reshape(-1, 32), torch.device("cuda:0"))
    wd = torch.from_numpy(_bf16(PK["gen_segmentation/kernel"].reshape(32, K))).cuda()
    bd = torch.from_numpy(PK["gen_segmentation/bias"]).cuda()
    want = torch.full((len(a17), K), float("nan"), device="cuda:0")
    assert lib.depgan_op_head_softmax_k_bf16s(P(a17), 32, P(wd), P(bd), P(want), None, len(a17), 32, K, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_u32(probs.reshape(-1, K)), _u32(want.cpu().numpy()))
    # batches of 2 + 1 are one batch of 3
    two = eng.g_forward(x[:2], z[:2], storage="bfloat16").cpu().numpy()
    one = eng.g_forward(x[2:], z[2:], storage="bfloat16").cpu().numpy()
    assert np.array_equal(_u32(np.concatenate([two, one])), _u32(probs))
    # the fp32-storage forward of the same context ends in the K-class head too
    p32 = eng.g_forward(x, z).cpu().numpy()
    assert p32.shape == probs.shape and np.abs(p32.sum(-1) - 1.0).max() <= 1e-5
    # every training entry, the three with integer labels included, is refused before any launch
    xd, zd = torch.from_numpy(x).cuda(), torch.zeros((B, 32), device="cuda:0")
    lab, cod = torch.zeros((B, IMG, IMG, K), device="cuda:0"), torch.zeros((B, IMG, IMG), dtype=torch.uint8, device="cuda:0")
    loss = C.c_float()
    calls = {
        "depgan_uresnet_grads": lambda: lib.depgan_uresnet_grads(eng.h, P(xd), P(zd), P(lab), B, 0, C.byref(loss)),
        "depgan_uresnet_step": lambda: lib.depgan_uresnet_step(eng.h, P(xd), P(zd), P(lab), B, 0, C.byref(loss)),
        "depgan_uresnet_eval": lambda: lib.depgan_uresnet_eval(eng.h, P(xd), P(zd), P(lab), B, C.byref(loss)),
        "depgan_uresnet_grads_sparse": lambda: lib.depgan_uresnet_grads_sparse(eng.h, P(xd), P(zd), P(cod), B, 0,
                                                                               C.byref(loss)),
        "depgan_uresnet_step_sparse": lambda: lib.depgan_uresnet_step_sparse(eng.h, P(xd), P(zd), P(cod), B, 0,
                                                                             C.byref(loss)),
        "depgan_uresnet_eval_sparse": lambda: lib.depgan_uresnet_eval_sparse(eng.h, P(xd), P(zd), P(cod), B, C.byref(loss)),
        "depgan_apply_adam": lambda: lib.depgan_apply_adam(eng.h, 0),
        "depgan_set_fwd_only_storage": lambda: lib.depgan_set_fwd_only_storage(eng.h, 1),
    }
    eng.profile(True)
    eng.profile_reset()
    for name, call in calls.items():
        assert call() == 3, name
        assert b"inference context" in lib.depgan_last_error(), name
    assert sum(eng.profile_read(k)[1] for k in range(3)) == 0                # nothing was launched
    eng.profile(False)
    with pytest.raises(ValueError, match="inference"):
        eng.uresnet(x, z, cod, "step")
    eng.close()


def test_facade_sparse_fit_and_evaluation(lib):
    """10. Gen_UNet2D(..., nc_out=3).compile(loss='sparse_categorical_crossentropy'): fit with a short last batch and
    sparse validation data is three train_on_batch calls and evaluate; with four classes the two losses train the same
    model; predict_mean and the label map serve three classes, the 4-code metrics refuse them."""
    from dep_gan_im_amd import Gen_UNet2D, evaluate
    x, z, codes, _ = _batch(12, 5, 3)
    vx, vz, vcodes, _ = _batch(13, 3, 3)
    mk = lambda: Gen_UNet2D((IMG, IMG, 1), nc_out=3, seed=3).compile(loss="sparse_categorical_crossentropy")   # noqa: E731
    net = mk()
    h = net.fit([x, z], codes, epochs=1, batch_size=2, shuffle=False, validation_data=([vx, vz], vcodes[..., None]),
                verbose=0)
    twin = mk()
    tot = sum(len(x[i:i + 2]) * twin.train_on_batch([x[i:i + 2], z[i:i + 2]], codes[i:i + 2]) for i in (0, 2, 4))
    assert h.history["loss"] == [tot / 5]
    assert h.history["val_loss"] == [twin.evaluate([vx, vz], vcodes, batch_size=2)]
    a, b = net.get_weights(), twin.get_weights()
    assert all(np.array_equal(_u32(u), _u32(v)) for u, v in zip(a, b))
    assert abs(net.test_on_batch([vx[:2], vz[:2]], torch.from_numpy(vcodes[:2]).cuda().long())
               - twin.test_on_batch([vx[:2], vz[:2]], vcodes[:2].astype(np.float64))) == 0.0
    # prediction and evaluation surface for three classes
    mean = evaluate.predict_mean(net, vx, n_repeat=2, rng=np.random.default_rng(0), batch_size=2)
    assert tuple(mean.shape) == (3, IMG, IMG, 3)
    counts, labels = evaluate.label_census(mean, return_labels=True)
    assert tuple(labels.shape) == (3, IMG, IMG) and 0 <= int(labels.min()) and int(labels.max()) < 3
    with pytest.raises(ValueError, match="4-code"):
        evaluate.uresnet_metrics(mean, None, None, None, None, None, 1.0)
    # four classes: the two losses on two same-seeded models
    x4, z4, codes4, onehot4 = _batch(14, 5, 4)
    dense = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=4).compile(loss="categorical_crossentropy")
    sparse = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=4).compile(loss="sparse_categorical_crossentropy")
    hd = dense.fit([x4, z4], onehot4, epochs=2, batch_size=2, shuffle=False, validation_data=([x4, z4], onehot4), verbose=0)
    hs = sparse.fit([x4, z4], codes4, epochs=2, batch_size=2, shuffle=False, validation_data=([x4, z4], codes4), verbose=0)
    assert hd.history == hs.history
    assert all(np.array_equal(_u32(u), _u32(v)) for u, v in zip(dense.get_weights(), sparse.get_weights()))
