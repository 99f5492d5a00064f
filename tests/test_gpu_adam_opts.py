"""GPU: the kernels behind depgan_set_optimizer at operator level -- depgan_op_grad_sqnorm and depgan_op_adam_opts on
caller-owned arrays.

(a) the squared norm against float64 (the squares are exact in double, n 2^-53 < 3e-10 bounds any summation order, so
    1e-9 relative), bit-identical from run to run, and a NaN or an infinity anywhere comes back as one;
(b) exact statements, compared as uint32: an option that does not act gives the plain kernel's bits;
(c) every option on, three consecutive steps, against tests/optim_ref.py in float64.

The inputs of (b) and (c), one arena-sized draw (the DEP-UResNet's trainable arena): gradients of magnitude 1e-6 to 1
with 5 % exact zeros, as test_adam_kernel_three_steps_on_injected_gradients draws them; weights of magnitude 1e-3 to 1
with a few exact zeros.  |p| < 1 keeps the two float32 roundings of a decayed weight (the decay, then the displacement)
at 2 * 2^-25 = 0.6e-3 lr, inside the project's bound of 2e-3 lr per step; in (c) a gradient element keeps its sign
over the three steps, so m is a sum of like-signed terms and a relative bound on it means something in float32."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import optim_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
LR, EPS = 1e-4, 1e-7
ARENA = 2491969                   # (a)'s arena-sized odd length
LENGTHS = [1, 3, 255, 256, 257, 2047, 2049, 8 * 2048 + 5, ARENA]


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _draw(rng, n):
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
    g[rng.uniform(size=n) < 0.05] = 0.0
    return g


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sqnorm(lib, g_dev, gscale):
    from dep_gan_im_amd._lib import check
    out = C.c_double(-1.0)
    check(lib.depgan_op_grad_sqnorm(C.c_void_p(g_dev.data_ptr()), g_dev.numel(), gscale, C.byref(out), _stream()),
          "depgan_op_grad_sqnorm")
    return out.value


# ---- (a) ----

@pytest.mark.parametrize("n", LENGTHS)
def test_grad_sqnorm_against_float64(lib, n):
    """First device run, worst relative error over the nine lengths and both gscales: 1.94e-16 (n = 16389); 1.71e-16 at
    n = 2 491 969, and exactly the float64 sum at seven of the nine lengths."""
    rng = np.random.default_rng(n)
    g = _draw(rng, n)
    if n <= 3:
        g[:] = np.array([0.37, -1e-6, 0.0], np.float32)[:n]
    dev = torch.from_numpy(g).cuda()
    for gscale in (1.0, 0.125):
        want = float(np.sum((g * np.float32(gscale)).astype(np.float64) ** 2))
        got = _sqnorm(lib, dev, gscale)
        err = abs(got - want) / want
        print("n = %d, gscale %g: squared norm %.17g, relative error %.2e" % (n, gscale, got, err))
        assert err <= 1e-9, (n, gscale, got, want)
        assert _sqnorm(lib, dev, gscale) == got                                   # bit-identical from run to run
    for bad in (np.nan, np.inf, -np.inf):
        h = g.copy()
        h[-1] = bad
        assert not np.isfinite(_sqnorm(lib, torch.from_numpy(h).cuda(), 1.0)), (n, bad)
    # a gradient that overflows float32 only through gscale is an infinity too
    h = g.copy()
    h[-1] = 3e38
    assert not np.isfinite(_sqnorm(lib, torch.from_numpy(h).cuda(), 2.0))
    assert np.isfinite(_sqnorm(lib, torch.from_numpy(h).cuda(), 1.0))


def test_grad_sqnorm_refuses_a_misaligned_gradient(lib):
    dev = torch.zeros(64, device="cuda")
    out = C.c_double(-7.0)
    assert lib.depgan_op_grad_sqnorm(C.c_void_p(dev.data_ptr() + 4), 16, 1.0, C.byref(out), _stream()) == 1
    assert b"aligned" in lib.depgan_last_error() and out.value == -7.0


# ---- (b), (c) ----

@functools.lru_cache(maxsize=None)
def _inputs():
    """(engine-sized n, p, g, m, v) as float32 host arrays; n is the DEP-UResNet's trainable arena at 4 classes."""
    from dep_gan_im_amd import Engine, _lib
    eng = Engine(2, 64, 64, 1, beta1=0.9, beta2=0.999, nc_out=4)
    n = eng.arena("G", _lib.ARENA_PARAMS)[1]
    eng.close()
    rng = np.random.default_rng(11)
    p = (rng.choice([-1.0, 1.0], n) * rng.uniform(1e-3, 1.0, n)).astype(np.float32)
    p[rng.uniform(size=n) < 0.01] = 0.0
    g = _draw(rng, n)
    m = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    v = (rng.uniform(size=n) * 1e-6).astype(np.float32)
    return n, p, g, m, v


def _segments(n):
    """Boundaries that are no multiple of 4, of 64 or of the block's span; flags alternate, the first segment decays."""
    ends = [3, 260, 261, 5000, 5001, 8192 + 7, n]
    return ends, [1, 0, 1, 0, 1, 0, 1]


def _mask(n, ends, flags):
    out, at = np.zeros(n, bool), 0
    for e, f in zip(ends, flags):
        out[at:e] = bool(f)
        at = e
    return out


def _adam_opts(lib, p, g, m, v, t, b1, b2, clipnorm=0.0, clipvalue=0.0, wd=0.0, seg=None, gscale=1.0, lr=LR):
    """One depgan_op_adam_opts call on copies; returns (p, m, v) as host arrays and (norm, scale).  lr is the plain rate
    (it scales weight_decay alone); the bias-corrected rate is always that of LR."""
    from dep_gan_im_amd._lib import check
    n = p.size
    dev = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (p, g, m, v)]
    ends, flags = seg if seg is not None else ([], [])
    e, f = (C.c_long * max(1, len(ends)))(*ends), (C.c_int * max(1, len(flags)))(*flags)
    nh = (C.c_double * 2)(-1.0, -1.0)
    ptr = [C.c_void_p(d.data_ptr()) for d in dev]
    check(lib.depgan_op_adam_opts(ptr[0], ptr[1], ptr[2], ptr[3], n, R.lr_t(LR, b1, b2, t), lr, b1, b2, EPS, gscale,
                                  clipnorm, clipvalue, wd, e, f, len(ends), nh, _stream()), "depgan_op_adam_opts")
    return [dev[i].cpu().numpy() for i in (0, 2, 3)], (nh[0], nh[1])


@functools.lru_cache(maxsize=None)
def _plain(lib):
    """The option kernel with every option 0 on _inputs() at t = 3, (0.9, 0.999): what (b)'s statements compare with."""
    n, p, g, m, v = _inputs()
    return _adam_opts(lib, p, g, m, v, 3, 0.9, 0.999)[0]


def _same(a, b):
    return all(np.array_equal(_u32(x), _u32(y)) for x, y in zip(a, b))


def test_all_options_off_equals_the_plain_kernel(lib):
    """depgan_apply_adam on a context holding the same p, g, m, v at the same step counter."""
    from dep_gan_im_amd import Engine, _lib
    n, p, g, m, v = _inputs()
    eng = Engine(2, 64, 64, 1, lrG=LR, beta1=0.9, beta2=0.999, adam_eps=EPS, nc_out=4)
    assert eng.arena("G", _lib.ARENA_PARAMS)[1] == n
    ng = eng.arena("G", _lib.ARENA_GRADS)[1]
    gg = np.zeros(ng, np.float32)
    gg[:n] = g
    for arena, a in ((_lib.ARENA_PARAMS, p), (_lib.ARENA_GRADS, gg), (_lib.ARENA_ADAM_M, m), (_lib.ARENA_ADAM_V, v)):
        eng.set_arena("G", arena, a)
    eng.adam_step("G", 2)
    assert eng.optimizer("G") is None
    eng.apply_adam("G")
    assert eng.adam_step("G") == 3
    want = [eng.get_arena("G", a)[:n] for a in (_lib.ARENA_PARAMS, _lib.ARENA_ADAM_M, _lib.ARENA_ADAM_V)]
    eng.close()
    got = _plain(lib)
    assert _same(got, want)
    assert not np.array_equal(got[0], p) and not np.array_equal(got[1], m) and not np.array_equal(got[2], v)
    # and the GAN optimiser's betas, against the same context path
    eng = Engine(2, 64, 64, 1, lrG=LR, beta1=0.0, beta2=0.9, adam_eps=EPS, nc_out=4)
    for arena, a in ((_lib.ARENA_PARAMS, p), (_lib.ARENA_GRADS, gg), (_lib.ARENA_ADAM_M, m), (_lib.ARENA_ADAM_V, v)):
        eng.set_arena("G", arena, a)
    eng.apply_adam("G")
    want = [eng.get_arena("G", a)[:n] for a in (_lib.ARENA_PARAMS, _lib.ARENA_ADAM_M, _lib.ARENA_ADAM_V)]
    eng.close()
    assert _same(_adam_opts(lib, p, g, m, v, 1, 0.0, 0.9)[0], want)


def test_options_that_do_not_act_give_the_plain_bits(lib):
    n, p, g, m, v = _inputs()
    plain = _plain(lib)
    norm = np.sqrt(R.sqnorm(g))
    got, (rep, s) = _adam_opts(lib, p, g, m, v, 3, 0.9, 0.999, clipnorm=2.0 * norm)
    assert _same(got, plain) and s == 1.0 and abs(rep - norm) <= 1e-9 * norm
    got, (rep, s) = _adam_opts(lib, p, g, m, v, 3, 0.9, 0.999, clipvalue=float(np.abs(g).max()) * 1.5)
    assert _same(got, plain) and (rep, s) == (0.0, 1.0)
    # weight_decay with no segment, with one segment that is not decayed, and with gscale
    assert _same(_adam_opts(lib, p, g, m, v, 3, 0.9, 0.999, wd=0.5)[0], plain)
    assert _same(_adam_opts(lib, p, g, m, v, 3, 0.9, 0.999, wd=0.5, seg=([n], [0]))[0], plain)
    # clipping does act below the norm and below max|g|
    assert not _same(_adam_opts(lib, p, g, m, v, 3, 0.9, 0.999, clipnorm=0.5 * norm)[0], plain)
    assert not _same(_adam_opts(lib, p, g, m, v, 3, 0.9, 0.999, clipvalue=float(np.abs(g).max()) * 0.5)[0], plain)


@pytest.mark.parametrize("table", ["alternating", "single", "last_element"])
def test_weight_decay_acts_on_the_decayed_segments_alone(lib, table):
    """lr * weight_decay = 0.25: a decayed weight moves by a quarter of itself, far above the rounding of the update."""
    n, p, g, m, v = _inputs()
    seg = {"alternating": _segments(n), "single": ([n], [1]), "last_element": ([n - 1, n], [0, 1])}[table]
    p = p.copy()
    p[-1] = 0.625                                        # the one-element segment at the very end holds a weight
    base = _adam_opts(lib, p, g, m, v, 3, 0.9, 0.999, lr=0.5)[0]
    got, _ = _adam_opts(lib, p, g, m, v, 3, 0.9, 0.999, wd=0.5, seg=seg, lr=0.5)
    dec = _mask(n, *seg)
    assert np.array_equal(_u32(got[1]), _u32(base[1])) and np.array_equal(_u32(got[2]), _u32(base[2]))   # m, v untouched
    assert np.array_equal(_u32(got[0])[~dec], _u32(base[0])[~dec])
    live = dec & (p != 0)
    assert live.sum() == {"alternating": live.sum(), "single": (p != 0).sum(), "last_element": 1}[table] and live[-1]
    assert np.all(_u32(got[0])[live] != _u32(base[0])[live])
    assert (dec & (p == 0)).any() == (table != "last_element")
    assert np.array_equal(_u32(got[0])[dec & (p == 0)], _u32(base[0])[dec & (p == 0)])
    # the decayed weight is fma(-lr wd, p, p) = 0.75 p exactly, then the plain displacement: one float32 rounding of a
    # value below 2 on either side, 2 * 2^-24 = 1.2e-7
    disp = base[0].astype(np.float64) - p
    assert float(np.abs(base[0]).max()) < 2.0
    np.testing.assert_allclose(got[0][live], 0.75 * p[live].astype(np.float64) + disp[live], rtol=0, atol=1.2e-7)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_norm_leaves_everything_as_it_was(lib, bad):
    n, p, g, m, v = _inputs()
    g = g.copy()
    g[n // 3] = bad
    got, (norm, s) = _adam_opts(lib, p, g, m, v, 3, 0.9, 0.999, clipnorm=1.0, clipvalue=0.1, wd=0.01, seg=_segments(n))
    assert _same(got, (p, m, v)) and s == 0.0 and not np.isfinite(norm)
    # without clipnorm there is no norm to test: the update runs (and a NaN stays a NaN through clipvalue)
    got, (norm, s) = _adam_opts(lib, p, g, m, v, 3, 0.9, 0.999, clipvalue=0.1)
    assert (norm, s) == (0.0, 1.0) and not np.array_equal(_u32(got[0]), _u32(p))
    assert np.isnan(got[1][n // 3]) == bool(np.isnan(bad)) and (np.isnan(bad) or abs(got[1][n // 3]) <= 0.1)


@pytest.mark.parametrize("b1,b2", [(0.0, 0.9), (0.9, 0.999)])
def test_every_option_on_against_float64(lib, b1, b2):
    """clipnorm at half the norm (scale near 0.5), clipvalue at the 95th percentile of the scaled |g| (cuts 5 %),
    weight_decay 1e-2, gscale 0.125, three consecutive steps on the device's own state.  Bounds of
    test_adam_kernel_three_steps_on_injected_gradients: |p - p64| <= 2e-3 lr per step (p64 stepped from the device's
    previous p; m and v of the reference run on in float64), m and v at rtol 2e-6; the reference takes the float32
    scale the library reports, and the reported norm is within 1e-9 of float64.
    First device run (n = 2 486 244, norm 293, scale 0.49999997, 5.0 % of the elements cut), worst over the three steps,
    (0, 0.9): |p - p64| 1.06e-3 lr, m 5.96e-8, v 3.36e-7 relative; (0.9, 0.999): |p - p64| 1.06e-3 lr, m 2.50e-7,
    v 3.90e-7; the reported norm within 1.4e-15 of float64."""
    n, p, g0, _, _ = _inputs()
    seg = _segments(n)
    dec = _mask(n, *seg)
    rng = np.random.default_rng(23)
    sign = np.where(g0 < 0, -1.0, 1.0).astype(np.float32)
    gscale, wd = 0.125, 1e-2
    p_dev, m_dev, v_dev = p, np.zeros(n, np.float32), np.zeros(n, np.float32)
    m64, v64 = np.zeros(n), np.zeros(n)
    for t in (1, 2, 3):
        g = (np.abs(_draw(rng, n)) * sign * 8.0).astype(np.float32)
        norm64 = np.sqrt(R.sqnorm(g, gscale))
        clipnorm = float(np.float32(0.5 * norm64))
        clipvalue = float(np.float32(np.quantile(np.abs(R.scaled(g, gscale)) * 0.5, 0.95)))
        (p_new, m_new, v_new), (norm, s) = _adam_opts(lib, p_dev, g, m_dev, v_dev, t, b1, b2, clipnorm=clipnorm,
                                                      clipvalue=clipvalue, wd=wd, seg=seg, gscale=gscale)
        assert abs(norm - norm64) <= 1e-9 * norm64 and abs(s - 0.5) < 1e-6
        assert s == R.clip_scale(norm, clipnorm)
        p64, m64, v64, _, _ = R.adam_opts_step(p_dev, g, m64, v64, t, LR, b1, b2, EPS, gscale, clipnorm, clipvalue, wd,
                                               dec, scale=s)
        cut = float((np.abs(R.scaled(g, gscale) * s) > clipvalue).mean())
        e_p = float(np.abs(p_new - p64).max()) / LR
        e_m = float((np.abs(m_new - m64) / np.maximum(np.abs(m64), 1e-300)).max())
        e_v = float((np.abs(v_new - v64) / np.maximum(np.abs(v64), 1e-300)).max())
        print("(%.1f, %.3f) step %d: norm %.6g (rel. error %.1e), scale %.9g, %.1f %% cut by clipvalue; worst |p - p64| "
              "%.2e lr, m %.2e, v %.2e relative" % (b1, b2, t, norm, abs(norm - norm64) / norm64, s, 100 * cut, e_p, e_m, e_v))
        assert 0.03 < cut < 0.07
        assert e_p <= 2e-3, (t, e_p)
        np.testing.assert_allclose(v_new, v64, rtol=2e-6, atol=0)
        np.testing.assert_allclose(m_new, m64, rtol=2e-6, atol=1e-30)
        p_dev, m_dev, v_dev = p_new, m_new, v_new
