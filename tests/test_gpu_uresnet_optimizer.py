"""GPU: the optimiser options (depgan_set_lr, depgan_set_optimizer) through the context and the Keras-style facade, at
64 x 64 x 1, engines of batch 4 fed 3 samples.

Exact statements are bit for bit: options set to nothing, or set and cleared, against a context that never set them;
set_lr against a context created with that rate; `step` against `grads` + apply_adam under the same options, for the
DEP-UResNet and for a critic (whose closure launches Adam before the host synchronises, so the norm can only have been
read on the device).  Against float64 (tests/optim_ref.py on the gradients the device produced) the bounds are those of
test_gpu_adam_opts.py's (c)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import optim_ref as R  # noqa: E402
from test_gpu_uresnet_classes import IMG, _arenas, _batch, _engine, _params, _u32  # noqa: E402

pytestmark = pytest.mark.gpu
LR = 1e-4


def _same_arenas(a, b):
    for x, y in zip(_arenas(a), _arenas(b)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def _same_grads(a, b, net="G"):
    ga, gb = a.get_grads(net), b.get_grads(net)
    assert list(ga) == list(gb) and any(float(np.abs(v).max()) > 0 for v in ga.values())
    for k in ga:
        assert np.array_equal(_u32(ga[k]), _u32(gb[k])), k


def _flat(eng, net, arena):
    from dep_gan_im_amd import _lib
    n = eng.arena(net, _lib.ARENA_PARAMS)[1]
    return eng.get_arena(net, arena)[:n]


def _decay_mask(eng, net):
    from dep_gan_im_amd import _lib
    out = np.zeros(eng.arena(net, _lib.ARENA_PARAMS)[1], bool)
    for name, shape, off, tr in eng.param_table(net):
        if tr and name.endswith("/kernel"):
            out[off:off + int(np.prod(shape))] = True
    assert out.any() and not out.all()
    return out


def test_options_off_equal_a_context_that_never_set_them(lib):
    """d. set_optimizer(0, 0, 0) with set_lr(the same lr), and options set and cleared: loss, gradients, arenas."""
    B, n, ds = 4, 3, 77
    Pm = _params(5, 4)
    x, z, codes, _ = _batch(9, n, 4)
    plain, zero, back = _engine(B, Pm, 4), _engine(B, Pm, 4), _engine(B, Pm, 4)
    assert plain.optimizer("G") is None and plain.lr("G") == float(np.float32(LR))
    zero.set_optimizer("G", 0, 0, 0)
    zero.set_lr("G", LR)
    assert zero.optimizer("G") is None and zero.lr("G") == plain.lr("G")
    back.set_optimizer("G", clipnorm=1e-6, clipvalue=1e-4, weight_decay=0.1)
    assert back.optimizer("G") == {"clipnorm": float(np.float32(1e-6)), "clipvalue": float(np.float32(1e-4)),
                                   "weight_decay": float(np.float32(0.1))}
    want = plain.uresnet(x, z, codes, "step", drop_seed=ds)
    assert back.uresnet(x, z, codes, "step", drop_seed=ds) == want          # the loss is taken before the update
    assert any(not np.array_equal(a, b) for a, b in zip(_arenas(plain), _arenas(back)))     # the options acted
    norm, scale = back.grad_norm("G")
    assert norm > 1e-6 and 0 < scale < 1
    back.set_optimizer("G")
    assert back.optimizer("G") is None
    from dep_gan_im_amd import _lib
    for arena in (_lib.ARENA_PARAMS, _lib.ARENA_ADAM_M, _lib.ARENA_ADAM_V, _lib.ARENA_NONTRAINABLE):
        back.set_arena("G", arena, plain.get_arena("G", arena))
    back.weights_changed("G")
    assert zero.uresnet(x, z, codes, "step", drop_seed=ds) == want
    _same_arenas(plain, zero)
    for step in (1, 2):
        want = plain.uresnet(x, z, codes, "step", drop_seed=ds + step)
        assert [e.uresnet(x, z, codes, "step", drop_seed=ds + step) for e in (zero, back)] == [want, want], step
        for e in (zero, back):
            _same_grads(plain, e)
            _same_arenas(plain, e)
    assert plain.adam_step("G") == zero.adam_step("G") == back.adam_step("G") == 3
    # refusals: before any launch, and the setting stays
    back.set_optimizer("G", clipnorm=2.0)
    for kw in ({"clipnorm": -1.0}, {"clipvalue": float("nan")}, {"weight_decay": float("inf")}, {"clipnorm": True}):
        with pytest.raises(ValueError):
            back.set_optimizer("G", **kw)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            back.set_lr("G", bad)
        assert lib.depgan_set_lr(back.h, _lib.NET_G, bad) == 1
    assert lib.depgan_set_optimizer(back.h, _lib.NET_G, -1.0, 0.0, 0.0) == 1
    assert lib.depgan_set_optimizer(back.h, 7, 1.0, 0.0, 0.0) == 1
    assert back.optimizer("G") == {"clipnorm": 2.0, "clipvalue": 0.0, "weight_decay": 0.0} and back.lr("G") == plain.lr("G")
    with pytest.raises(_lib.DepganError, match="clipnorm on"):
        plain.grad_norm("G")
    # an inference context holds no gradients: status 3 from the library, ValueError from the engine; its rate is settable
    from dep_gan_im_amd import Engine
    infer = Engine(B, IMG, IMG, 1, nc_out=4, bf16_mfma=True)
    assert infer.inference_only and lib.depgan_set_optimizer(infer.h, _lib.NET_G, 1.0, 0.0, 0.0) == 3
    assert b"inference context" in lib.depgan_last_error()
    with pytest.raises(ValueError, match="inference"):
        infer.set_optimizer("G", weight_decay=0.1)
    infer.set_lr("G", 2e-4)
    assert infer.lr("G") == float(np.float32(2e-4)) and infer.optimizer("G") is None
    for e in (plain, zero, back, infer):
        e.close()


def test_set_lr_equals_a_context_created_with_that_rate(lib):
    """e. one step at lr1 on both sides' common ancestor, then lr2 by set_lr against a context created with lr2 that was
    given the same weights, statistics, Adam state and step counter."""
    from dep_gan_im_amd import Engine, _lib
    B, n, ds = 4, 3, 77
    lr2 = 3e-4
    Pm = _params(5, 4)
    x, z, codes, _ = _batch(9, n, 4)
    a = _engine(B, Pm, 4)
    a.uresnet(x, z, codes, "step", drop_seed=ds)
    b = Engine(B, IMG, IMG, 1, lrG=lr2, beta1=0.9, beta2=0.999, nc_out=4)
    for arena in (_lib.ARENA_PARAMS, _lib.ARENA_ADAM_M, _lib.ARENA_ADAM_V, _lib.ARENA_NONTRAINABLE):
        b.set_arena("G", arena, a.get_arena("G", arena))
    b.weights_changed("G")
    b.adam_step("G", a.adam_step("G"))
    a.set_lr("G", lr2)
    assert a.lr("G") == b.lr("G") == float(np.float32(lr2))
    before = _arenas(a)[0]
    assert a.uresnet(x, z, codes, "step", drop_seed=ds + 1) == b.uresnet(x, z, codes, "step", drop_seed=ds + 1)
    _same_arenas(a, b)
    # and it is the rate that moved the weights: the second step of Adam moves an element by at most about lr
    moved = float(np.abs(_arenas(a)[0] - before).max())
    assert 1.05e-4 < moved < 1.05 * lr2, moved
    a.close()
    b.close()


def test_step_equals_grads_and_apply_adam_with_options(lib):
    """f. every option on.  The trainable weights are clipped to +-1.9 (the he_normal dense kernel of fan-in 1 reaches 3):
    a decayed weight is rounded twice, by the decay and by the displacement, and below 2 the two half-ulps are
    2 * 2^-24 = 1.2e-3 lr, inside the bound of 2e-3 lr; from 2 on they could reach 2.4e-3 lr whatever the kernel does.
    First device run: norm 1.9239935 (the float64 figure to the digits printed), scale 0.5, 2487 elements cut by
    clipvalue 3.72e-4; worst |p - p64| 1.01e-3 lr, m 5.68e-8 and v 1.17e-7 relative."""
    from dep_gan_im_amd import _lib
    B, n, ds = 4, 3, 77
    Pm = {k: (v if "moving_" in k else np.clip(v, -1.9, 1.9)) for k, v in _params(5, 4).items()}
    x, z, codes, _ = _batch(9, n, 4)
    probe = _engine(B, Pm, 4)
    probe.uresnet(x, z, codes, "grads", drop_seed=ds)
    g = _flat(probe, "G", _lib.ARENA_GRADS)
    p0 = _flat(probe, "G", _lib.ARENA_PARAMS)
    dec = _decay_mask(probe, "G")
    probe.close()
    norm64 = float(np.sqrt(R.sqnorm(g)))
    clipnorm = float(np.float32(0.5 * norm64))
    clipvalue = float(np.float32(np.quantile(np.abs(g) * 0.5, 0.999)))
    wd = 1e-2
    one, two = _engine(B, Pm, 4), _engine(B, Pm, 4)
    for e in (one, two):
        e.set_optimizer("G", clipnorm=clipnorm, clipvalue=clipvalue, weight_decay=wd)
    loss = one.uresnet(x, z, codes, "step", drop_seed=ds)
    assert two.uresnet(x, z, codes, "grads", drop_seed=ds) == loss
    assert np.array_equal(_u32(_flat(two, "G", _lib.ARENA_GRADS)), _u32(g))
    two.apply_adam("G")
    _same_arenas(one, two)
    assert one.adam_step("G") == two.adam_step("G") == 1
    for e in (one, two):
        norm, s = e.grad_norm("G")
        assert abs(norm - norm64) <= 1e-9 * norm64 and s == R.clip_scale(norm, clipnorm) and abs(s - 0.5) < 1e-6
    assert one.uresnet(x, z, codes, "eval") == two.uresnet(x, z, codes, "eval")       # the derived state followed
    p64, m64, v64, _, _ = R.adam_opts_step(p0, g, np.zeros(g.size), np.zeros(g.size), 1, LR, 0.9, 0.999, 1e-7, 1.0,
                                           clipnorm, clipvalue, wd, dec, scale=s)
    P, M, V = _arenas(one)
    e_p = float(np.abs(P - p64).max()) / LR
    e_m = float((np.abs(M - m64) / np.maximum(np.abs(m64), 1e-300)).max())
    e_v = float((np.abs(V - v64) / np.maximum(np.abs(v64), 1e-300)).max())
    print("norm %.9g (float64 %.9g), scale %.9g, %d elements cut by clipvalue %.3g; worst |p - p64| %.2e lr, m %.2e, "
          "v %.2e relative" % (norm, norm64, s, int((np.abs(g) * s > clipvalue).sum()), clipvalue, e_p, e_m, e_v))
    assert (np.abs(g) * s > clipvalue).sum() > 100
    assert e_p <= 2e-3
    np.testing.assert_allclose(V, v64, rtol=2e-6, atol=0)
    np.testing.assert_allclose(M, m64, rtol=2e-6, atol=1e-30)
    # the decay reached the kernels and nothing else: against a step without it, from the same state
    nodecay = _engine(B, Pm, 4)
    nodecay.set_optimizer("G", clipnorm=clipnorm, clipvalue=clipvalue)
    nodecay.uresnet(x, z, codes, "step", drop_seed=ds)
    Pn = _arenas(nodecay)[0]
    assert np.array_equal(_u32(Pn[~dec]), _u32(P[~dec])) and not np.array_equal(_u32(Pn[dec]), _u32(P[dec]))
    for e in (one, two, nodecay):
        e.close()


def test_critic_step_equals_grads_and_apply_adam_with_clipnorm(lib):
    """g. D_y2, clipnorm below the gradient's norm: the closure's update read the norm on the device."""
    from dep_gan_im_amd import Engine, _lib
    from oracle import depgan_oracle as O
    B = 2
    PG, PD = O.init_generator(31, bias_std=0.05), O.init_critic(32, bias_std=0.05, img=IMG)
    x, y2, z, ep = O.synth_batch(36, B, IMG, IMG)
    engs = []
    for _ in range(3):
        e = Engine(B, IMG, IMG, 1)
        e.set_weights("G", PG)
        e.set_weights("D_y2", PD)
        engs.append(e)
    probe, one, two = engs
    probe.critic("D_y2", y2, x, z, ep, update=False)
    norm64 = float(np.sqrt(R.sqnorm(_flat(probe, "D_y2", _lib.ARENA_GRADS))))
    clipnorm = float(np.float32(0.25 * norm64))
    for e in (one, two):
        e.set_optimizer("D_y2", clipnorm=clipnorm)
    out = one.critic("D_y2", y2, x, z, ep, update=True)
    assert two.critic("D_y2", y2, x, z, ep, update=False) == out
    two.apply_adam("D_y2")
    probe.critic("D_y2", y2, x, z, ep, update=True)                    # unclipped
    for arena in (_lib.ARENA_PARAMS, _lib.ARENA_ADAM_M, _lib.ARENA_ADAM_V):
        a, b, c = (e.get_arena("D_y2", arena) for e in (one, two, probe))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        if arena != _lib.ARENA_PARAMS:
            assert not np.array_equal(a, c)                            # the clip acted: m and v are those of g / 4
    for e in (one, two):
        norm, s = e.grad_norm("D_y2")
        assert abs(norm - norm64) <= 1e-9 * norm64 and s == R.clip_scale(norm, clipnorm) and abs(s - 0.25) < 1e-6
    m1, mp = one.get_arena("D_y2", _lib.ARENA_ADAM_M), probe.get_arena("D_y2", _lib.ARENA_ADAM_M)
    np.testing.assert_allclose(m1, mp * np.float32(s), rtol=1e-6, atol=1e-30)
    assert one.optimizer("G") is None and one.optimizer("D_dem") is None     # the options are per network
    for e in engs:
        e.close()


def test_facade_compile_fit_callbacks(lib):
    """h. compile's options reach the engine; LearningRateScheduler halves the rate per epoch; EarlyStopping stops."""
    from dep_gan_im_amd import Gen_UNet2D
    from dep_gan_im_amd.callbacks import EarlyStopping, LearningRateScheduler
    x, z, codes, _ = _batch(12, 3, 4)
    sp = "sparse_categorical_crossentropy"
    net = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(loss=sp, clipnorm=1.5, weight_decay=1e-4)
    ref = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(loss=sp, clipnorm=1.5, weight_decay=1e-4)
    rs = np.random.RandomState(3)
    seeds = [int(rs.randint(1, 2 ** 31 - 1)) for _ in range(2)]            # the model's own dropout seeds
    h = net.fit([x, z], codes, epochs=2, batch_size=4, shuffle=False, verbose=0,
                callbacks=[LearningRateScheduler(lambda e, lr: lr * 0.5)])
    eng = net._engine
    assert eng.optimizer("G") == {"clipnorm": 1.5, "clipvalue": 0.0, "weight_decay": float(np.float32(1e-4))}
    lr0 = float(np.float32(LR))
    assert sorted(h.history) == ["loss", "lr"] and h.history["lr"] == [float(np.float32(lr0 * 0.5)),
                                                                         float(np.float32(lr0 * 0.25))]
    assert net.lr == h.history["lr"][-1] == eng.lr("G")
    losses = []
    for ep, seed in enumerate(seeds):
        ref.set_lr(ref.lr * 0.5)
        losses.append(ref.train_on_batch([x, z], codes, drop_seed=seed))
    assert losses == h.history["loss"]
    _same_arenas(eng, ref._engine)
    assert eng.adam_step("G") == 2 and eng.grad_norm("G")[0] > 0
    # a third model that never halves the rate differs from the second epoch's first update on
    flat = Gen_UNet2D((IMG, IMG, 1), nc_out=4, seed=3).compile(loss=sp, clipnorm=1.5, weight_decay=1e-4)
    flat.set_lr(lr0 * 0.5)
    assert flat.train_on_batch([x, z], codes, drop_seed=seeds[0]) == losses[0]
    flat.train_on_batch([x, z], codes, drop_seed=seeds[1])
    assert not np.array_equal(_arenas(flat._engine)[0], _arenas(eng)[0])
    # EarlyStopping(patience=0) on a monitor that cannot improve: epoch 1 sets the best value, epoch 2 stops
    h = net.fit([x, z], codes, epochs=5, batch_size=4, shuffle=False, verbose=0,
                callbacks=[EarlyStopping(monitor="lr", patience=0)])
    assert len(h.history["loss"]) == 2 and net.stop_training and len(h.history["lr"]) == 2
    # callbacks=None: the keys and the lines of before
    lines = []
    h = net.fit([x, z], codes, epochs=1, batch_size=4, shuffle=False, verbose=1, print_fn=lines.append)
    assert sorted(h.history) == ["loss"] and len(lines) == 1 and " - lr" not in lines[0]
    h = net.fit([x, z], codes, epochs=1, batch_size=4, shuffle=False, validation_data=([x, z], codes), verbose=0)
    assert sorted(h.history) == ["loss", "val_loss"]
    # compile() without the options clears them on the engine; the rate set by the callbacks stays
    net.compile(loss=sp)
    assert eng.optimizer("G") is None and net.lr == eng.lr("G")
    with pytest.raises(RuntimeError):
        net.compile(loss=sp, lr=1e-2)
    with pytest.raises(ValueError, match="monitor"):
        net.fit([x, z], codes, epochs=1, batch_size=4, verbose=0, callbacks=[EarlyStopping()])
