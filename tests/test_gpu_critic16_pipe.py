"""GPU: the critics' 16-channel 5x5 layers on the bf16 matrix pipe -- igemm_bf16_n16_kernel (v_mfma_f32_16x16x32_bf16)
behind operator path 10, and the context switch depgan_set_critic16_pipe that routes dis_0b forward / u-forward /
backward-data and dis_1a backward-data of both critics to it.

What is exact is asserted bit for bit: exact operands through the fused epilogue, sample independence, repeatability,
the teacher-forced wiring, everything after the switch is turned off against a context that never switched, the fused
generator iteration against the closure schedule.  The contraction is held to the project's fp32 tolerance against float64
of the same RNE-rounded operands; the model to config 4's own criterion (tests/test_gpu_model.py::
test_config4_bf16_matrix_pipe) against the oracle under the rounding rule this mode implements."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_ref as fr  # noqa: E402
from test_gpu_fused_ops import NONE, SENT, Win, bits, dev  # noqa: E402  (windows of wider buffers, sentinels)

pytestmark = pytest.mark.gpu
TOL = 1e-4   # tests/test_gpu_ops.py: same rounded operands on both sides, only the summation order differs
NETS = ("G", "D_y2", "D_dem")
PATH = 10


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def srel(got, want):
    return max(abs(a - b) / (abs(b) + 1e-3) for a, b in zip(got, want))


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _bf16(a):
    """float32 -> nearest bf16 (ties to even) -> float32, what v_cvt_pk_bf16_f32 does to both MFMA operands."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


# ---------------------------------------------------------------------------
# 1. contraction
# ---------------------------------------------------------------------------
FWD_CASES = [  # B, H, W, Cin, Cout (KS = 5)
    (2, 32, 32, 16, 16),      # basic
    (2, 17, 33, 32, 16),      # ragged
    (2, 21, 19, 16, 16),      # ragged
    (1, 16, 16, 8, 16),       # Cin below a chunk
    (2, 32, 32, 40, 16),      # chunk tail
    (2, 32, 32, 16, 48),      # three channel tiles
    (16, 128, 128, 16, 16),   # 1024 workgroups, the nPix % 8 == 0 item order
    (3, 48, 40, 16, 16),      # the other item order (27 pixel tiles)
]
BWD_CASES = [  # the LAYER's B, H, W, Cin, Cout: the launch runs Cout -> Cin, so Cin is the multiple of 16
    (2, 32, 32, 16, 16),      # dis_0b backward-data
    (2, 17, 33, 16, 32),      # dis_1a backward-data, ragged
    (2, 32, 32, 16, 40),      # chunk tail in K
]


def _conv64(x, w, b=None, relu=False):
    y = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2).double(), torch.from_numpy(w).permute(3, 2, 0, 1).double(),
                 None if b is None else torch.from_numpy(b).double(), padding=w.shape[0] // 2)
    if relu:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1).numpy()


def _bwd64(dy, w):
    return F.conv_transpose2d(torch.from_numpy(dy).permute(0, 3, 1, 2).double(),
                              torch.from_numpy(w).permute(3, 2, 0, 1).double(), padding=w.shape[0] // 2).permute(0, 2, 3, 1).numpy()


def _launch(lib, x, w, b, co_out, bwd, shape):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = shape
    xd, wd, bd = dev(x), dev(w), dev(b)
    out = torch.full((x.shape[0], H, W, co_out), float("nan"), device="cuda:0")
    if bwd:
        _lib.check(lib.depgan_op_conv2d_bwd_data(P(xd), P(wd), P(out), x.shape[0], H, W, ci, co, 5, PATH, None))
    else:
        _lib.check(lib.depgan_op_conv2d(P(xd), P(wd), P(bd), P(out), x.shape[0], H, W, ci, co, 5, 1, PATH, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", [c + (0,) for c in FWD_CASES] + [c + (1,) for c in BWD_CASES],
                         ids=lambda c: ("bwd-" if c[5] else "fwd-") + "x".join(map(str, c[:5])))
def test_contraction_against_float64_of_the_rounded_operands(lib, case):
    B, H, W, ci, co, bwd = case
    rng = np.random.default_rng(ci * 1000 + co + H + 7 * bwd)
    cin, cout = (co, ci) if bwd else (ci, co)                  # channels of the launch
    x = rng.standard_normal((B, H, W, cin)).astype(np.float32)
    w = (rng.standard_normal((5, 5, ci, co)) / np.sqrt(25 * cin)).astype(np.float32)
    b = None if bwd else rng.standard_normal(co).astype(np.float32)
    got = _launch(lib, x, w, b, cout, bwd, case[:5])
    if bwd:
        ref_q, ref_f = _bwd64(_bf16(x), _bf16(w)), _bwd64(x, w)
    else:
        ref_q, ref_f = _conv64(_bf16(x), _bf16(w), b, True), _conv64(x, w, b, True)
    e_q, e_f = rel(got, ref_q), rel(got, ref_f)
    print("path 10 %s: vs float64 of the rounded operands %.3g, vs the unrounded reference %.3g" % (case, e_q, e_f))
    assert e_q < TOL
    assert e_f > 5 * TOL                                        # the rounding is there (and we follow it)


def test_sample_independence_and_repeatability(lib):
    """A sample's bits do not depend on how many samples share the launch (batch 4 == two launches of batch 2), and two
    launches on the same inputs are bit-equal: the K order is fixed (chunk, then tap), nothing is accumulated atomically."""
    for shape, bwd in (((4, 21, 19, 16, 16), 0), ((4, 32, 32, 40, 16), 0), ((4, 17, 33, 16, 32), 1)):
        B, H, W, ci, co = shape
        rng = np.random.default_rng(ci + co + H)
        cin, cout = (co, ci) if bwd else (ci, co)
        x = rng.standard_normal((B, H, W, cin)).astype(np.float32)
        w = (rng.standard_normal((5, 5, ci, co)) / np.sqrt(25 * cin)).astype(np.float32)
        b = None if bwd else rng.standard_normal(co).astype(np.float32)
        whole = _launch(lib, x, w, b, cout, bwd, shape)
        again = _launch(lib, x, w, b, cout, bwd, shape)
        halves = np.concatenate([_launch(lib, x[:2], w, b, cout, bwd, shape), _launch(lib, x[2:], w, b, cout, bwd, shape)])
        assert np.isfinite(whole).all()
        assert same(whole, again), shape
        assert same(whole, halves), shape


# ---------------------------------------------------------------------------
# 2. fused epilogue, bit for bit
# ---------------------------------------------------------------------------
# make_ops keywords + pre (out_pre requested) and pool.  Every operand of every case is a window of a wider buffer: a
# channel slice at a non-zero offset, samples from 1 of a longer batch, padding rows and columns (test_gpu_fused_ops.Win)
FEATS = {
    "pool": dict(bias=1, relu=1, pool=1),                               # the critics' forward: bias + ReLU + fused pool
    "negpool": dict(bias=1, neg=1, pool=1),                             # every window negative throughout
    "mask_bwd": dict(mask=1, bwd=1),                                    # backward-data and u-forward: the mask alone
    "film": dict(bias=1, affine=1, film=1, relu=1, res=1, pre=1),       # comes with the text, must work
    "acc": dict(bias=1, acc=1),
}
SIZES = [(32, 32), (21, 19)]
CHANNELS = {"pool": (16, 16), "negpool": (16, 16), "mask_bwd": (16, 32), "film": (32, 16), "acc": (16, 48)}
FUSED = [(f, (2, h, w) + CHANNELS[f]) for f in FEATS for (h, w) in SIZES if not ("pool" in FEATS[f] and (h | w) & 1)]
ODD_POOL = [(f, (2, 21, 19) + CHANNELS[f]) for f in FEATS if "pool" in FEATS[f]]
_fid = lambda c: "%s-%s" % (c[0], "x".join(map(str, c[1])))   # noqa: E731


def _run_fused(lib, feat, shape, kind, want_pre=False):
    B, H, W, ci, co = shape
    f = dict(FEATS[feat])
    pre, pool = f.pop("pre", 0) or want_pre, f.pop("pool", 0)
    rng = np.random.default_rng(sum(shape) * 131 + len(feat))
    o = fr.make_ops(kind, rng, B, H, W, ci, co, 5, **f)
    cin, cout = (co, ci) if o.bwd else (ci, co)
    nan = np.float32("nan")
    w = {"in": Win((B, H, W, cin), 12, 4, nan, o.x), "out": Win((B, H, W, cout), 20, 8, SENT, o.old)}
    if pre:
        w["pre"] = Win((B, H, W, cout), 28, 12, SENT)
    if o.res is not None:
        w["res"] = Win((B, H, W, cout), 36, 16, nan, o.res)
    if o.mask is not None:
        w["mask"] = Win((B, H, W, cout), 44, 20, nan, o.mask)
    if pool:
        w["pool"] = Win((B, H // 2, W // 2, cout), 52, 24, SENT)
    d = {n: dev(getattr(o, n)) for n in ("w", "bias", "scale", "shift")}
    ld = cout + 12                                                      # FiLM rows at their own pitch, NaN between them
    for n in ("fmul", "fadd"):
        a = getattr(o, n)
        if a is not None:
            full = np.full((B, ld), nan, np.float32)
            full[:, :cout] = a
            a = full
        d[n] = dev(a)
    arg = lambda n: w[n].args() if n in w else NONE   # noqa: E731
    rc = lib.depgan_op_conv2d_fused(
        *w["in"].args(), P(d["w"]), P(d["bias"]), P(d["scale"]), P(d["shift"]), P(d["fmul"]), P(d["fadd"]), ld,
        *w["out"].args(), *arg("pre"), *arg("res"), *arg("mask"), *arg("pool"), None, None, None, 0, 0, B, H, W, ci, co, 5,
        o.relu, int(o.old is not None), PATH, o.bwd, None)
    torch.cuda.synchronize()
    return rc, o, w, (pre, pool)


@pytest.mark.parametrize("case", FUSED, ids=_fid)
def test_fused_epilogue_exact_operands_are_bit_exact(lib, case):
    """Integers in [-2, 2] and [-1, 1] are bf16-exact, so the float64 evaluation of the contract is THE bit pattern on the
    bf16 pipe as well (tests/fused_ref.py; K = 25 * 32 = 800 products at most, inside its bounds)."""
    from dep_gan_im_amd import _lib
    feat, shape = case
    rc, o, w, (pre, pool) = _run_fused(lib, feat, shape, "exact")
    _lib.check(rc, "op_conv2d_fused")
    assert np.array_equal(fr.bf16_round(o.x), o.x) and np.array_equal(fr.bf16_round(o.w), o.w)
    ref = fr.reference(o)
    assert fr.bounds_hold(ref["stages"])
    got = w["out"].read()
    assert np.array_equal(got, ref["out"]), "out: %d wrong, first at %s" % (
        (got != ref["out"]).sum(), np.argwhere(got != ref["out"])[:1].tolist())
    assert w["out"].outside_unchanged()
    if pre:
        assert np.array_equal(w["pre"].read(), ref["out_pre"])
        assert w["pre"].outside_unchanged()
    if pool:
        got = w["pool"].read()
        assert np.array_equal(got, ref["pool"]), "pool: first wrong at %s" % np.argwhere(got != ref["pool"])[:1].tolist()
        assert w["pool"].outside_unchanged()
        if "neg" in FEATS[feat]:
            assert ref["pool"].max() < 0
    for n in ("in", "res", "mask"):
        if n in w:
            assert w[n].unchanged()


@pytest.mark.parametrize("case", FUSED, ids=_fid)
def test_fused_epilogue_real_operands_contraction_at_tol_and_chain_bit_exact(lib, case):
    from dep_gan_im_amd import _lib
    feat, shape = case
    rc, o, w, (pre, pool) = _run_fused(lib, feat, shape, "real", want_pre=True)
    _lib.check(rc, "op_conv2d_fused")
    ref = fr.reference(o, acc=fr.conv_acc(fr.bf16_round(o.x), fr.bf16_round(o.w), o.bwd))
    got_pre = w["pre"].read()
    e = rel(got_pre, ref["out_pre"])
    print("path 10 %s out_pre rel err %.3g" % (case, e))
    assert e < TOL
    assert w["pre"].outside_unchanged()
    out, _ = fr.post_chain(got_pre, o)         # numpy float32, one operation per step, from the kernel's own out_pre
    got = w["out"].read()
    assert np.array_equal(got, out), "out: %d wrong, first at %s" % ((got != out).sum(), np.argwhere(got != out)[:1].tolist())
    assert w["out"].outside_unchanged()
    if pool:
        assert np.array_equal(w["pool"].read(), fr.pool2(out))
        assert w["pool"].outside_unchanged()


@pytest.mark.parametrize("case", ODD_POOL, ids=_fid)
def test_pool_on_an_odd_size_is_refused_and_nothing_is_written(lib, case):
    rc, o, w, _ = _run_fused(lib, case[0], case[1], "exact")
    assert rc != 0 and lib.depgan_last_error()
    assert all(win.unchanged() for win in w.values())


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
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


def _engine(img, B, PG, PD1, PD2, pipe=None, **kw):
    import dep_gan_im_amd as dg
    kw.setdefault("bf16_mfma", True)
    eng = dg.Engine(B, img, img, 2, **kw)
    for n, Pm in zip(NETS, (PG, PD1, PD2)):
        eng.set_weights(n, Pm)
    if pipe is not None:
        eng.critic16_pipe = pipe
    return eng


def _arenas(eng):
    from dep_gan_im_amd._lib import ARENA_ADAM_M, ARENA_ADAM_V, ARENA_PARAMS
    return [eng.get_arena(n, a) for n in NETS for a in (ARENA_PARAMS, ARENA_ADAM_M, ARENA_ADAM_V)]


# 3. switch semantics
def test_switch_is_refused_without_bf16_mfma_and_leaves_nothing_behind(lib):
    import dep_gan_im_amd as dg
    img, B = 64, 2
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 91)
    for kw in ({"bf16_mfma": False}, {"bf16_mfma": False, "bf16_weights": True}):
        e = _engine(img, B, PG, PD1, PD2, **kw)
        assert lib.depgan_set_critic16_pipe(e.h, 1) == 3, kw
        assert b"bf16_mfma" in lib.depgan_last_error() and b"critic16" in lib.depgan_last_error()
        assert lib.depgan_get_critic16_pipe(e.h) == 0
        assert lib.depgan_set_critic16_pipe(e.h, 0) == 0 and lib.depgan_set_critic16_pipe(e.h, 2) == 1
        with pytest.raises(ValueError, match="bf16_mfma"):
            e.critic16_pipe = "bfloat16"
        e.close()
    a = _engine(img, B, PG, PD1, PD2)
    b = _engine(img, B, PG, PD1, PD2)                       # never switches
    assert lib.depgan_get_critic16_pipe(a.h) == 0 and a.critic16_pipe == "float32"        # default off
    assert lib.depgan_set_critic16_pipe(a.h, 2) == 1 and lib.depgan_set_critic16_pipe(a.h, -1) == 1
    d_off = a.d_forward("D_y2", y2).cpu().numpy()
    a.critic16_pipe = "bfloat16"
    assert lib.depgan_get_critic16_pipe(a.h) == 1 and a.critic16_pipe == "bfloat16"
    d_on = a.d_forward("D_y2", y2).cpu().numpy()
    assert not same(d_on, d_off)                            # another kernel ran
    on = [a.critic("D_y2", y2, x, z, ep, update=False), a.critic("D_dem", y2, x, z, ep, update=False)]
    assert on != [b.critic("D_y2", y2, x, z, ep, update=False), b.critic("D_dem", y2, x, z, ep, update=False)]
    a.generator(x, y2, z, "grads")
    a.critic16_pipe = "float32"
    assert lib.depgan_get_critic16_pipe(a.h) == 0
    later = {}
    for name, e in (("a", a), ("b", b)):
        out = [e.d_forward("D_y2", y2).cpu().numpy(), e.d_forward("D_dem", y2).cpu().numpy()]
        sc = [e.critic("D_y2", y2, x, z, ep, update=False)]
        g = [e.get_grads("D_y2")]
        sc.append(e.critic("D_dem", y2, x, z, ep, update=False))
        g.append(e.get_grads("D_dem"))
        sc.append(e.generator(x, y2, z, "grads"))
        g.append(e.get_grads("G"))
        sc.append(e.critic("D_y2", y2, x, z, ep))          # one depgan_critic_step: post-Adam weights
        later[name] = (out, sc, g, _arenas(e))
    assert same(later["a"][0][0], d_off)
    for u, v in zip(later["a"][0], later["b"][0]):
        assert same(u, v)
    assert later["a"][1] == later["b"][1]
    for ga, gb in zip(later["a"][2], later["b"][2]):
        for k in ga:
            assert same(ga[k], gb[k]), k
    for u, v in zip(later["a"][3], later["b"][3]):
        assert same(u, v)
    a.close()
    b.close()
    with pytest.raises(ValueError):
        dg.Engine(B, img, img, 2).critic16_pipe = "bfloat16"


# 4. wiring, teacher-forced
def test_wiring_dis_0b_is_path_10_on_the_same_call_s_dis_0a(lib):
    """With the mode on, d/act/dis_0b after a critic closure equals, bit for bit, path 10 (bias, ReLU) applied to the
    dis_0a activation the same call produced, with the context's bf16-rounded dis_0b kernel -- for the real and fake
    groups read from d/act, for the mixed group from the capture of the mixed pass (the penalty's u-forward overwrites
    dis_0a's mixed slots in place).  With the mode off the same comparison fails: it is the fp32 kernel then."""
    from dep_gan_im_amd import _lib
    img, B = 64, 2
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 57)
    eng = _engine(img, B, PG, PD1, PD2)
    W = eng.get_weights("D_dem")
    wq, bias = dev(_bf16(W["conv2d_dis_0b/kernel"])), dev(W["conv2d_dis_0b/bias"])
    eng.debug_capture(True)
    for pipe in ("bfloat16", "float32"):
        eng.critic16_pipe = pipe
        eng.critic("D_dem", y2, x, z, ep, update=False)
        a0, a1 = eng.debug_tensor("d/act/dis_0a"), eng.debug_tensor("d/act/dis_0b")
        assert a0.shape == (3 * B, img, img, 16) and a1.shape == (3 * B, img, img, 16)
        a0 = np.concatenate([a0[:2 * B], eng.debug_tensor("d/mixed/dis_0a")])
        assert same(a1[2 * B:], eng.debug_tensor("d/mixed/dis_0b"))       # dis_0b's mixed slots are not overwritten
        src = dev(a0)
        out = torch.full((3 * B, img, img, 16), float("nan"), device="cuda:0")
        _lib.check(lib.depgan_op_conv2d(P(src), P(wq), P(bias), P(out), 3 * B, img, img, 16, 16, 5, 1, PATH, None))
        torch.cuda.synchronize()
        want = out.cpu().numpy()
        for g, name in enumerate(("real", "fake", "mixed")):
            s = slice(g * B, (g + 1) * B)
            assert same(a1[s], want[s]) == (pipe == "bfloat16"), (pipe, name)
    eng.close()


# 5. model against the oracle, by config 4's own criterion
def _patch_oracle_rule(monkeypatch, O):
    """The rounding rule this mode implements: the existing one, or a 5x5 convolution with Cout % 16 == 0, Cin >= 8,
    Cin % 4 == 0.  _conv_same is wrapped to hand the kernel size through; both are module globals looked up at call time."""
    cur = []
    conv_same = O._conv_same

    def conv(x, w_hwio, b):
        cur.append(int(w_hwio.shape[0]))
        try:
            return conv_same(x, w_hwio, b)
        finally:
            cur.pop()

    def act(x, cin, cout):
        k = cur[-1] if cur else 0
        covered = cin >= 8 and cin % 4 == 0 and (cout % 32 == 0 or (k == 5 and cout % 16 == 0))
        if not O._ACT_BF16 or not covered:
            return x
        q = x.detach().to(torch.float32).to(torch.bfloat16).to(x.dtype)
        return x + (q - x.detach())

    monkeypatch.setattr(O, "_conv_same", conv)
    monkeypatch.setattr(O, "_act_operand", act)


CLOSURES = (("netG_no_update", "g"), ("netD_y2_train", "d"), ("netD_dem_train", "d"), ("netG_no_update", "g"),
            ("netG_train", "g"), ("netG_no_update", "g"))


def test_model_against_the_oracle_under_the_mode_s_rounding_rule(lib, monkeypatch):
    """Inputs, sequence of closures and tolerances of test_config4_bf16_matrix_pipe (64 x 64 x 2, batch 2, seed 57).
    Mode on is held to them against the oracle under the patched rule; mode off against the unpatched oracle is printed
    next to it (it is asserted by that test).  The critic gradients at the end are printed, not gated: they are held
    launch by launch, against float64 of the operands each launch stored, by tests/test_gpu_critic_links.py."""
    import dep_gan_im_amd as dg
    from oracle import depgan_oracle as O
    img, B, seed = 64, 2, 57
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, seed)
    args = {"g": [x, y2, z], "d": [y2, x, z, ep]}
    cp = lambda Pm: type(Pm)((k, v.copy()) for k, v in Pm.items())   # noqa: E731  (the oracle updates its dicts in place)

    def oracle():
        with O.bf16_activations():
            d_q = O.d_predict(O.round_kernels_bf16(PD1), y2)
            gp = O.critic_grads(O.round_kernels_bf16(PD1), O.round_kernels_bf16(PG), y2, x, z, ep, "y2", 10.0, 2,
                                torch.float64)[2]["gp"]
        ref = O.OracleTrainers(cp(PG), cp(PD1), cp(PD2), nicg=2, dtype=torch.float64, weights_dtype="bfloat16",
                               activations_dtype="bfloat16")
        return d_q, gp, [getattr(ref, name)(args[kind]) for name, kind in CLOSURES]

    want = {"float32": oracle()}
    _patch_oracle_rule(monkeypatch, O)
    want["bfloat16"] = oracle()
    assert not np.array_equal(want["float32"][0], want["bfloat16"][0])          # the patch is seen
    d_w = O.d_predict(O.round_kernels_bf16(PD1), y2)                             # bf16 weights only
    grads = {}
    for pipe in ("float32", "bfloat16"):
        d_q, gp, outs = want[pipe]
        nets = [dg.Gen_UNet2D((img, img, 2)), dg.Dis_C2D_FCN1((img, img, 1)), dg.Dis_C2D_FCN1((img, img, 1))]
        for n, Pm in zip(nets, (PG, PD1, PD2)):
            n.set_weights(cp(Pm))
        tr = dg.build_trainers(*nets, batchSize=B, weights_dtype="bfloat16", activations_dtype="bfloat16", critic16_pipe=pipe)
        eng = tr.engine
        on = pipe == "bfloat16"
        assert lib.depgan_get_critic16_pipe(eng.h) == int(on)
        d_got = eng.d_forward("D_y2", y2).cpu().numpy()
        e_d, e_round = rel(d_got, d_q), rel(d_q, d_w)
        print("critic16 %s: critic forward vs rounded-operand oracle %.3e (bound 2 x %.3e + 1e-3)" % (pipe, e_d, e_round))
        eng.critic("D_y2", y2, x, z, ep, update=False)
        gp_got = eng.last_sums()[2] / eng.last_sums()[3]
        e_gp = abs(gp_got - gp) / abs(gp)
        print("critic16 %s: penalty %.6f vs oracle %.6f, rel %.3e (bound 1e-2)" % (pipe, gp_got, gp, e_gp))
        grads[pipe] = eng.get_grads("D_y2")
        errs, moved = [], False
        for (name, kind), w_ in zip(CLOSURES, outs):
            got = getattr(tr, name)(args[kind])
            e_all = srel(got, w_)
            e_pin = srel(got[1:4], w_[1:4]) if (len(got) == 6 and not moved) else None
            print("critic16 %s %s: %s vs %s: srel %.3e (bound 3e-2)%s" % (
                pipe, name, [round(v, 5) for v in got], [round(v, 5) for v in w_], e_all,
                "" if e_pin is None else "; critic means and M1 %.3e (bound 1e-2)" % e_pin))
            errs.append((name, e_all, e_pin))
            moved = moved or name.endswith("_train")
        eng.close()
        if on:
            assert e_d < 2.0 * e_round + 1e-3, (e_d, e_round)
            assert e_gp < 1e-2, (gp_got, gp)
            for name, e_all, e_pin in errs:
                assert e_all < 3e-2, (name, e_all)
                assert e_pin is None or e_pin < 1e-2, (name, e_pin)
    # critic gradients, mode on against mode off: printed, not gated (the gradients of bf16 contexts
    # are dominated by ReLU / arg-max decisions that the operand rounding flips)
    for k in grads["float32"]:
        a_, b_ = grads["bfloat16"][k].astype(np.float64), grads["float32"][k].astype(np.float64)
        print("critic16 D_y2 gradient %s: mode on vs off rel-L2 %.3e" % (k, np.sqrt(((a_ - b_) ** 2).sum() / ((b_ ** 2).sum() + 1e-300))))


# 6. three steps
def test_three_steps_and_the_fused_iteration_in_the_mode(lib):
    img, B, lr = 64, 2, 1e-4
    PG, PD1, PD2, x, y2, z, ep = _setup(img, B, 171, nb=3)
    xb, yb = x[:B], y2[:B]
    eng = _engine(img, B, PG, PD1, PD2, pipe="bfloat16")
    steps = {"G": 0, "D_y2": 0, "D_dem": 0}
    for i in range(3):
        for which in ("D_y2", "D_dem"):
            out = eng.critic(which, yb, xb, z[:B], ep[:B])
            steps[which] += 1
            assert np.isfinite(out).all(), (which, i, out)
    zs = np.random.default_rng(5).normal(size=(3, B, 32, 1)).astype(np.float32)
    zl, el = np.stack([z[B:2 * B], z[2 * B:3 * B]]), np.stack([ep[B:2 * B], ep[2 * B:3 * B]])
    xl, yl = torch.from_numpy(x[B:]).cuda(), torch.from_numpy(y2[B:]).cuda()
    before = _arenas(eng)
    fused = eng.gen_iteration((xl, yl, zl, el, 2), (xl, yl, zl, el, 2), (xb, yb, zs))
    for n, s in (("G", 1), ("D_y2", 2), ("D_dem", 2)):
        steps[n] += s
    assert all(np.isfinite(v).all() for v in fused[:4])
    for n, Pm in zip(NETS, (PG, PD1, PD2)):
        Wn = eng.get_weights(n)
        for k in Pm:
            assert float(np.abs(Wn[k] - Pm[k]).max()) <= 2.05 * lr * steps[n], (n, k)
    after = _arenas(eng)
    eng.close()
    # the same schedule closure by closure, from the same state, in the same mode
    ref = _engine(img, B, PG, PD1, PD2, pipe="bfloat16")
    for i in range(3):
        for which in ("D_y2", "D_dem"):
            ref.critic(which, yb, xb, z[:B], ep[:B])
    for u, v in zip(_arenas(ref), before):
        assert same(u, v)
    cy = [ref.critic("D_y2", y2[(j + 1) * B:(j + 2) * B], x[(j + 1) * B:(j + 2) * B], zl[j], el[j]) for j in range(2)]
    cd = [ref.critic("D_dem", y2[(j + 1) * B:(j + 2) * B], x[(j + 1) * B:(j + 2) * B], zl[j], el[j]) for j in range(2)]
    ev = ref.generator_eval_multi(xb, yb, zs)[0]
    best = int(np.argmin([e[0] for e in ev]))
    tr = ref.generator(xb, yb, zs[best], "step")
    assert (cy, cd, ev, tr, best) == tuple(fused)
    for u, v in zip(_arenas(ref), after):
        assert same(u, v)
    ref.close()
