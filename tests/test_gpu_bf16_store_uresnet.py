"""GPU: DEP-UResNet predict on the bf16 pipe with bf16 activation storage -- the softmax head on stored bf16 values
(depgan_op_head_softmax_bf16s), the inference context (Engine(..., nc_out=4, bf16_mfma=True)) and the predict-only model
copy (GeneratorModel.inference_copy).

What is exact is asserted bit for bit: the logits against depgan_op_head_bf16s column by column, the probabilities against
depgan_op_softmax_ce4 of those logits, the trunk against the generator's own bf16-storage forward, batching,
repeatability, the facade.  Against float64 the head is held to the module bound of tests/test_gpu_bf16_store.py
(TOL = 1e-4), the model to that file's end-to-end criterion: no farther from the storage-graph oracle than 2.0 times (max)
and 1.5 times (mean) the distance between two ORACLE evaluations, storage graph against weights-only rounding."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_bf16_store import TOL, P, _bf16, _dev_h  # noqa: E402

pytestmark = pytest.mark.gpu
UNSUPPORTED, ARG = 3, 1
# The yardstick of test_end_to_end_by_the_modes_own_criterion, max |storage graph - weights-only| over the probabilities,
# is two CPU oracle evaluations.  For (seed, head scale) it came out as (57, 1.0): max 5.92e-3, mean 3.03e-4, probabilities
# down to 8e-9; (57, 4.0): max 1.43e-2, mean 6.9e-5 (saturated); (61, 1.0): max 6.72e-3, mean 8.06e-4, probabilities in
# [2.6e-3, 0.897].  The least saturated one is used; its max is 67 TOL.  The floor asserted is a tenth of what was found.
SEED_E2E, HEAD_SCALE, E_ROUND_FOUND = 61, 1.0, 6.72e-3


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _head_softmax(lib, ah, ld, coff, w, b, Pn, Cn, want_logits=True):
    """depgan_op_head_softmax_bf16s on channels [coff, coff + Cn) of the (Pn, ld) bf16 device tensor ah; probs and logits
    prefilled with NaN.  Returns (probs, logits) as numpy."""
    from dep_gan_im_amd import _lib
    dev = ah.device
    wd, bd = torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(dev), torch.from_numpy(b).to(dev)
    probs = torch.full((Pn, 4), float("nan"), device=dev)
    logits = torch.full((Pn, 4), float("nan"), device=dev) if want_logits else None
    _lib.check(lib.depgan_op_head_softmax_bf16s(C.c_void_p(ah.data_ptr() + 2 * coff), ld, P(wd), P(bd), P(probs), P(logits),
                                                Pn, Cn, None), "depgan_op_head_softmax_bf16s")
    torch.cuda.synchronize()
    return probs.cpu().numpy(), (logits.cpu().numpy() if want_logits else None)


def _softmax64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


# Pn, Cn, ld, channel offset
HEAD_CASES = [(3 * 37 * 29, 32, 32, 0), (1, 32, 32, 0), (64, 32, 32, 0), (3 * 37 * 29, 64, 64, 0), (1, 64, 64, 0),
              (64, 64, 64, 0), (3 * 37 * 29, 32, 96, 32)]


@pytest.mark.parametrize("case", HEAD_CASES)
def test_head_operator_exact(lib, case):
    from dep_gan_im_amd import _lib
    Pn, Cn, ld, coff = case
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(Pn + 7 * Cn + ld)
    a = _bf16(rng.standard_normal((Pn, Cn)))
    w = _bf16(rng.standard_normal((Cn, 4)) / 4.0)
    b = rng.standard_normal(4).astype(np.float32)
    wide = np.full((Pn, ld), np.nan, np.float32)               # NaN in the channels outside the slice
    wide[:, coff:coff + Cn] = a
    ah = torch.from_numpy(wide).to(torch.bfloat16).to(dev)
    probs, logits = _head_softmax(lib, ah, ld, coff, w, b, Pn, Cn)
    probs_only, _ = _head_softmax(lib, ah, ld, coff, w, b, Pn, Cn, want_logits=False)
    assert np.array_equal(_u32(probs), _u32(probs_only))
    assert np.isfinite(probs).all() and np.isfinite(logits).all()

    # logit k = depgan_op_head_bf16s(tanh = 0) with column k of w on the same input, bit for bit
    dense = _dev_h(a, dev)
    for k in range(4):
        wk = torch.from_numpy(np.ascontiguousarray(w[:, k])).to(dev)
        bk = torch.from_numpy(b[k:k + 1].copy()).to(dev)
        out = torch.full((Pn,), float("nan"), device=dev)
        _lib.check(lib.depgan_op_head_bf16s(P(dense), P(wk), P(bk), P(out), Pn, Cn, 0, None), "depgan_op_head_bf16s")
        torch.cuda.synchronize()
        assert np.array_equal(_u32(logits[:, k]), _u32(out.cpu().numpy())), k
    # probs = depgan_op_softmax_ce4(onehot = NULL) of those logits, bit for bit
    ld_, pd_ = torch.from_numpy(logits).to(dev), torch.full((Pn, 4), float("nan"), device=dev)
    _lib.check(lib.depgan_op_softmax_ce4(P(ld_), None, P(pd_), None, None, Pn, None), "depgan_op_softmax_ce4")
    torch.cuda.synchronize()
    assert np.array_equal(_u32(probs), _u32(pd_.cpu().numpy()))

    # float64 of the same bf16-valued operands
    ref = a.astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
    zmax = float(np.abs(ref).max())
    e_z = float(np.abs(logits - ref).max())
    e_p = float(np.abs(probs - _softmax64(ref)).max())          # the infinity norm of softmax's Jacobian is <= 1/2
    e_s = float(np.abs(probs.astype(np.float64).sum(axis=-1) - 1.0).max())
    print("head softmax %s: logits %.3e (bound %.3e), probs %.3e (bound %.3e), row sums %.3e"
          % (case, e_z, TOL * zmax, e_p, TOL * max(1.0, zmax), e_s))
    assert e_z <= TOL * zmax
    assert e_p <= TOL * max(1.0, zmax)
    assert e_s <= 4 * 2.0 ** -24


def test_head_operator_constructed_rows(lib):
    """Rows whose logits are exactly representable: a = e_c (one channel set to 1) picks row c of w, b = 0."""
    dev = torch.device("cuda:0")
    Cn = 32
    rows = np.array([[3.0, 3.0, 3.0, 3.0],              # four equal logits
                     [-0.5, -0.5, -0.5, -0.5],
                     [100.0, -100.0, -100.0, -100.0],   # a spread of +-100
                     [-100.0, -100.0, 100.0, -100.0],
                     [2.0, 2.0, -200.0, -200.0],        # ties of the maximum; expf(-101) is a denormal, not 0: -200 here
                     [-200.0, 7.0, -200.0, 7.0],
                     [1.0, 1.0, 1.0, -200.0],
                     [0.0, 0.0, 0.0, 0.0]], np.float32)
    w = np.zeros((Cn, 4), np.float32)
    w[:len(rows)] = rows
    a = np.zeros((len(rows), Cn), np.float32)
    a[np.arange(len(rows)), np.arange(len(rows))] = 1.0
    probs, logits = _head_softmax(lib, _dev_h(a, dev), Cn, 0, w, np.zeros(4, np.float32), len(rows), Cn)
    assert np.array_equal(_u32(logits), _u32(rows))
    q = np.float32(0.25)
    want = np.array([[q, q, q, q], [q, q, q, q], [1, 0, 0, 0], [0, 0, 1, 0], [0.5, 0.5, 0, 0], [0, 0.5, 0, 0.5],
                     [np.float32(1) / np.float32(3)] * 3 + [0], [q, q, q, q]], np.float32)
    assert np.array_equal(_u32(probs), _u32(want)), probs


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
def _inputs(seed, n, img):
    from oracle import depgan_oracle as O
    x, _, z, _ = O.synth_batch(seed + 5, n, img, img, nicg=1)
    rng = np.random.default_rng(seed)
    return (x + 0.02 * rng.uniform(size=x.shape)).astype(np.float32), z


def _p4(seed, head_scale=1.0):
    from oracle import depgan_oracle as O
    P4 = O.init_generator(seed, nicg=1, nc_out=4, bias_std=0.05)
    P4["gen_segmentation/kernel"] = (P4["gen_segmentation/kernel"] * head_scale).astype(np.float32)
    return P4


def _infer_engine(B, img, P4):
    import dep_gan_im_amd as dg
    eng = dg.Engine(B, img, img, 1, nc_out=4, bf16_mfma=True, beta1=0.9, beta2=0.999)
    eng.set_weights("G", P4)
    return eng


@pytest.mark.parametrize("img,B", [(64, 3), (256, 1)])
def test_the_trunk_is_the_pinned_trunk(lib, img, B):
    """Every g/out/<layer> of the inference context equals, bit for bit, the one of the generator's bf16_mfma context with
    the same trunk weights (tests/test_gpu_bf16_store.py pins those layer by layer); the 4-channel output is the operator
    of test_head_operator_exact on the captured gen_17 with the context's (bf16-rounded) head weights."""
    import dep_gan_im_amd as dg
    from oracle import depgan_oracle as O
    seed = 57
    P4 = _p4(seed)
    P1 = dict(P4)
    P1["gen_segmentation/kernel"] = np.ascontiguousarray(P4["gen_segmentation/kernel"][..., :1])
    P1["gen_segmentation/bias"] = np.ascontiguousarray(P4["gen_segmentation/bias"][:1])
    x, z = _inputs(seed, B, img)
    names = [ent[1] for ent in O.gen_trunk(1, 32, 4)[:-1]]
    e1 = dg.Engine(B, img, img, 1, bf16_mfma=True)
    e1.set_weights("G", P1)
    e1.g_forward(x, z, storage="bfloat16")
    cap1 = {n: e1.debug_tensor_bf16s("g/out/" + n) for n in names}
    e1.close()
    e4 = _infer_engine(B, img, P4)
    assert e4.inference_only
    probs = e4.g_forward(x, z, storage="bfloat16").cpu().numpy()
    assert probs.shape == (B, img, img, 4)
    for n in names:
        got = e4.debug_tensor_bf16s("g/out/" + n)
        assert np.array_equal(_u32(got), _u32(cap1[n])), n
    e4.close()
    a17 = cap1["gen_17"].reshape(-1, 32)
    w = _bf16(P4["gen_segmentation/kernel"].reshape(32, 4))
    want, _ = _head_softmax(lib, _dev_h(a17, torch.device("cuda:0")), 32, 0, w, P4["gen_segmentation/bias"], len(a17), 32)
    assert np.array_equal(_u32(probs.reshape(-1, 4)), _u32(want))


def test_batching_repeatability_and_neighbours_undisturbed(lib):
    B, img, seed, n = 3, 64, 61, 7
    x, z = _inputs(seed, n, img)
    eng = _infer_engine(B, img, _p4(seed))
    f32_before = eng.g_forward(x[:B], z[:B]).cpu().numpy()
    full = eng.g_forward(x, z, storage="bfloat16").cpu().numpy()              # batches of 3, 3 and 1
    again = eng.g_forward(x, z, storage="bfloat16").cpu().numpy()
    assert np.array_equal(_u32(full), _u32(again))
    first = eng.g_forward(x[:B], z[:B], storage="bfloat16").cpu().numpy()     # n = batch
    assert np.array_equal(_u32(first), _u32(full[:B]))
    for i in range(n):                                                         # n = 1
        one = eng.g_forward(x[i:i + 1], z[i:i + 1], storage="bfloat16").cpu().numpy()
        assert np.array_equal(_u32(one), _u32(full[i:i + 1])), i
    f32_after = eng.g_forward(x[:B], z[:B]).cpu().numpy()
    assert np.array_equal(_u32(f32_before), _u32(f32_after))
    assert f32_before.shape == first.shape and not np.array_equal(f32_before, first)   # it IS another path
    eng.forward_storage = "bfloat16"                                           # the attribute is what storage=None uses
    assert np.array_equal(_u32(eng.g_forward(x[:B], z[:B]).cpu().numpy()), _u32(first))
    eng.close()


def storage_graph_softmax(T, x, z):
    """oracle.g_forward_t over gen_trunk(1, 32, 4) in fp32 torch with every layer output rounded to bf16 where the HIP path
    stores it (q), and torch.softmax at the head (fed from the stored gen_17)."""
    from oracle import depgan_oracle as O
    q = lambda t: t.to(torch.bfloat16).to(torch.float32)   # noqa: E731
    heads = O.noise_mlp(T, z)
    a = x.permute(0, 3, 1, 2)
    skips = {}
    for ent in O.gen_trunk(1, 32, 4):
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
            a = torch.softmax(O._conv_same(a, T[name + "/kernel"], T[name + "/bias"]), dim=1)
    return a.permute(0, 2, 3, 1).numpy()


def e2e_oracles(seed=SEED_E2E, head_scale=HEAD_SCALE, img=64, B=2):
    """(P4, x, z, storage-graph oracle, weights-only oracle, rounded-operand oracle): all on the CPU."""
    from oracle import depgan_oracle as O
    P4 = _p4(seed, head_scale)
    x, z = _inputs(seed, B, img)
    PQ = O.round_kernels_bf16(P4)
    with torch.no_grad():
        want_s = storage_graph_softmax(O.to_torch(PQ, torch.float32), torch.from_numpy(x),
                                       torch.from_numpy(np.asarray(z, np.float32)))
    want_w = O.g_predict(PQ, x, z, nicg=1, nc_out=4, head="softmax")
    with O.bf16_activations():
        want_q = O.g_predict(PQ, x, z, nicg=1, nc_out=4, head="softmax")
    return P4, x, z, want_s, want_w, want_q


def _dist(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(d.max()), float(d.mean())


def _label_share(a, b):
    return float(np.mean(np.argmax(a, -1) != np.argmax(b, -1)))


def test_end_to_end_by_the_modes_own_criterion(lib):
    P4, x, z, want_s, want_w, want_q = e2e_oracles()
    eng = _infer_engine(2, 64, P4)
    probs = eng.g_forward(x, z, storage="bfloat16").cpu().numpy()
    probs32 = eng.g_forward(x, z).cpu().numpy()
    eng.close()
    (e_s, m_s), (e_round, m_round) = _dist(probs, want_s), _dist(want_s, want_w)
    (e_q, m_q), (eq_round, mq_round) = _dist(probs32, want_q), _dist(want_q, want_w)
    print("bf16 storage softmax forward vs storage-graph oracle: max %.3e mean %.3e; the rounding's own effect max %.3e "
          "mean %.3e" % (e_s, m_s, e_round, m_round))
    print("fp32 storage softmax forward (same context) vs rounded-operand oracle: max %.3e mean %.3e; the rounding's own "
          "effect max %.3e mean %.3e" % (e_q, m_q, eq_round, mq_round))
    print("arg-max labels that differ: HIP vs storage-graph oracle %.5f of the pixels; storage-graph vs weights-only "
          "oracle %.5f" % (_label_share(probs, want_s), _label_share(want_s, want_w)))
    assert e_round > 0.1 * E_ROUND_FOUND and e_round > 10 * TOL
    assert e_s < 2.0 * e_round and m_s < 1.5 * m_round, (e_s, e_round, m_s, m_round)


def test_refusals_and_the_unchanged_surface(lib):
    import dep_gan_im_amd as dg
    dev = torch.device("cuda:0")
    img, B = 32, 2
    x = torch.zeros((B, img, img, 1), device=dev)
    z = torch.zeros((B, 32), device=dev)
    lab = torch.zeros((B, img, img, 4), device=dev)
    y2 = torch.zeros((B, img, img, 1), device=dev)
    ep = torch.zeros((B,), device=dev)
    out = torch.zeros((B, img, img, 4), device=dev)
    eng = dg.Engine(B, img, img, 1, nc_out=4, bf16_mfma=True, beta1=0.9, beta2=0.999)
    loss, o2 = C.c_float(), (C.c_float * 2)()
    calls = {
        "depgan_uresnet_grads": lambda: lib.depgan_uresnet_grads(eng.h, P(x), P(z), P(lab), B, 0, C.byref(loss)),
        "depgan_uresnet_step": lambda: lib.depgan_uresnet_step(eng.h, P(x), P(z), P(lab), B, 0, C.byref(loss)),
        "depgan_uresnet_eval": lambda: lib.depgan_uresnet_eval(eng.h, P(x), P(z), P(lab), B, C.byref(loss)),
        "depgan_apply_adam": lambda: lib.depgan_apply_adam(eng.h, 0),
        "depgan_critic_grads": lambda: lib.depgan_critic_grads(eng.h, 1, P(y2), P(x), P(z), P(ep), o2),
        "depgan_set_fwd_only_storage": lambda: lib.depgan_set_fwd_only_storage(eng.h, 1),
        "depgan_set_g_update_storage": lambda: lib.depgan_set_g_update_storage(eng.h, 1),
        "depgan_set_critic16_pipe": lambda: lib.depgan_set_critic16_pipe(eng.h, 1),
    }
    eng.profile(True)
    eng.profile_reset()
    for name, call in calls.items():
        assert call() == UNSUPPORTED, name
        msg = lib.depgan_last_error()
        assert b"inference context" in msg, (name, msg)
    assert sum(eng.profile_read(k)[1] for k in range(3)) == 0                # nothing was launched
    eng.profile(False)
    with pytest.raises(ValueError, match="inference"):
        eng.uresnet(x, z, lab, "step")
    with pytest.raises(ValueError, match="inference"):
        eng.apply_adam("G")
    with pytest.raises(ValueError, match="inference"):
        eng.forward_only_storage = "bfloat16"
    for n in (0, B + 1, -1):
        assert lib.depgan_g_forward_bf16s(eng.h, P(x), P(z), P(out), n) == ARG, n
    # the weight surface works as on any bf16_weights context
    names = [t[0] for t in eng.param_table("G")]
    assert "gen_segmentation/kernel" in names and eng.get_weights("G")["gen_segmentation/kernel"].shape == (1, 1, 32, 4)
    eng.close()
    # a plain nc_out = 4 engine is refused as before
    plain = dg.Engine(B, img, img, 1, nc_out=4, beta1=0.9, beta2=0.999)
    plain.profile(True)
    plain.profile_reset()
    assert lib.depgan_g_forward_bf16s(plain.h, P(x), P(z), P(out), B) == UNSUPPORTED
    assert b"bf16_mfma" in lib.depgan_last_error()
    assert sum(plain.profile_read(k)[1] for k in range(3)) == 0
    assert not plain.inference_only
    plain.close()


def test_facade_and_evaluation(lib):
    import dep_gan_im_amd as dg
    from dep_gan_im_amd import evaluate
    img, n, seed = 32, 3, 9
    P4 = _p4(seed)
    x, _ = _inputs(seed, n, img)
    rng = np.random.default_rng(seed)
    mask = (rng.uniform(size=(n, img, img)) > 0.2).astype(np.float32)
    m = dg.Gen_UNet2D((img, img, 1), nc_out=4)
    m.set_weights(P4)
    fast = m.inference_copy("bfloat16")
    assert fast.inference_only and fast.nc_out == 4 and not m.inference_only
    mean = evaluate.predict_mean(fast, x, mask=mask, rng=np.random.RandomState(5))
    torch.cuda.synchronize()
    eng = fast._ensure_engine(n)
    assert eng.inference_only and eng.forward_storage == "bfloat16"
    r = np.random.RandomState(5)
    acc = np.zeros((n, img, img, 4), np.float64)
    for _ in range(10):
        noise = r.normal(size=(n, 32, 1)).astype("float32")
        pred = fast.predict([x, noise])
        assert np.array_equal(_u32(pred), _u32(eng.g_forward(x, noise, storage="bfloat16").cpu().numpy()))
        acc += pred.astype(np.float64) * mask[..., None]
    assert mean.dtype == torch.float64 and np.array_equal(mean.cpu().numpy(), acc / 10.0)
    assert not np.array_equal(pred, m.predict([x, noise]))
    code = (rng.uniform(size=(n, img, img)) * 4).astype(np.float32)
    wm = (rng.uniform(size=(n, img, img)) > 0.7).astype(np.float32)
    met = evaluate.uresnet_metrics(mean, code, mask, wm, mask, wm, 3.5)
    assert np.array_equal(met["labels"].cpu().numpy(), np.argmax(acc / 10.0, -1).astype(np.int8))
    assert len(met["vol_dsc"]) == 18
    for call in (lambda: fast.fit([x, noise], None), lambda: fast.train_on_batch([x, noise], None),
                 lambda: fast.compile(), lambda: fast.test_on_batch([x, noise], None),
                 lambda: fast.evaluate([x, noise], None)):
        with pytest.raises(RuntimeError):
            call()
    # the copy does not follow its source; its own weight surface works
    P5 = _p4(seed + 1)
    m.set_weights(P5)
    assert np.array_equal(_u32(fast.predict([x, noise])), _u32(pred))
    got = fast.get_weights_dict()
    assert np.array_equal(got["conv2d_gen_17/kernel"], P4["conv2d_gen_17/kernel"])
    fast.set_weights(P5)
    assert not np.array_equal(fast.predict([x, noise]), pred)
    assert np.array_equal(_u32(fast.predict([x, noise])), _u32(m.inference_copy().predict([x, noise])))


def test_profiler(lib):
    B, img = 2, 64
    x, z = _inputs(3, B, img)
    eng = _infer_engine(B, img, _p4(3))
    eng.profile(True)
    eng.profile_reset()
    eng.g_forward(x, z, storage="bfloat16")
    torch.cuda.synchronize()
    assert eng.profile_read(0)[1] == 23                     # every conv / FiLM / deconv layer but gen_0, as the generator
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "launches.csv")
        eng.profile_dump(path)
        lines = [ln for ln in open(path).read().splitlines() if "head softmax fwd(bf16s)" in ln]
    eng.profile(False)
    eng.close()
    assert len(lines) == 1, lines
    # class, label, ms, GFLOP, algorithmic MB (three decimals), "kernel"
    klass, label, _, _, mb = lines[0].split(",")[:5]
    assert int(klass) == 2 and label == "head softmax fwd(bf16s)"
    assert abs(float(mb) - B * img * img * (2 * 32 + 16) * 1e-6) <= 0.00051, lines[0]
