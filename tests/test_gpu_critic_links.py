"""GPU: every launch of the critic closures against float64 links, in fp32 and bf16_mfma contexts.

End to end the critic gradient of a bf16 context cannot be gated tighter than per cent: under identical pinned decisions
a float32-accumulating and a float64 evaluation of the rounding model differ by up to 2e-2 per tensor at 64x64 (a CPU-only
measurement with oracle/manual.py: summation noise moves a few elements across a bf16 rounding boundary and the real / fake
cancellation of the critic loss amplifies it).  Teacher forcing removes that: every launch of critic_enqueue (csrc/model.hip)
reads and writes fp32 tensors that are still there when the closure ends, so each launch is recomputed alone in float64
from the operands the library stored (tests/critic_links_ref.py), rounded to bf16 exactly where that launch's plan is a
bf16 plan (sites(), held against the library's own choice by tests/test_critic_links_cpu.py).  Per link the operator
criterion |got - ref| <= 1e-4 S, S = max|ref|; each link's output is the next link's stored input, so together the links
cover the closure: three forwards, pools, the tail, the backward-data chain, the image gradient, u0, the u-forward through
the mixed pass's masks, one weight gradient per layer over [real | fake | u] with bias sums over the 2B real and fake
samples, and the four tail tensors.  The gate also pins WHERE the library rounds: at a bf16 site the result must be more
than 5e-4 S away from the reference without the operand rounding, at an fp32 site from the one with it.

Measured on an MI355X, worst link per kind in units of S (64x64 batch 2 seed 57, both critics; c16 also 48x80 batch 3):

  context             forward  tail-bwd  bwd-data  image-g  u0       u-fwd    wgrad    bias     tail-grad
  fp32                1.2e-6   4.4e-8    8.1e-7    5.6e-7   1.0e-7   7.4e-7   6.0e-7   4.4e-7   1.5e-6
  bf16                8.7e-7   0         9.0e-7    5.0e-7   1.2e-7   4.7e-7   4.0e-7   6.6e-7   1.3e-6
  bf16-c16            4.6e-7   0         5.8e-7    4.6e-7   9.1e-8   4.8e-7   3.2e-7   4.6e-7   1.3e-6
  bf16-c16 48x80 b3   4.8e-7   6.0e-8    9.5e-7    5.1e-7   1.3e-7   6.0e-7   3.7e-7   2.9e-7   1.3e-6
  bf16-wgrad32        8.7e-7   0         9.0e-7    5.0e-7   1.2e-7   4.7e-7   7.1e-7   8.9e-7   1.3e-6
  c16 after updates   4.5e-7   0         6.9e-7    8.0e-7   1.2e-7   5.0e-7   3.1e-7   3.6e-7   1.4e-6
  generator bf16/c16  7.2e-7   0         6.3e-7    5.0e-7
Every link holds 1e-4 S as stated; none needed a bound of its own (the in-kernel bias column sums included).

Mutants (a scratch build, not committed) and the link that stops each, error in units of S:
  u-forward through the real pass's masks            u-forward dis_0a, 0.76 .. 1.1, every context
  d_panel_b hands the fp32 panel to the 16-ch plan   backward-data into dis_0b, 1.0 .. 1.4, critic16 contexts
  backward panels not repacked after net_adam        backward-data into dis_7, 4.3e-2, test_packed_panels_follow_the_masters
  bias column sums over 3B samples                   bias-gradient dis_0a, 0.59 .. 2.6, every context
  fp32 forward plan for dis_0b under critic16        forward dis_0b, 2.4e-3 .. 3.5e-3 (0.49 .. 0.70 from the wrong side)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_links_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NETS = ("G", "D_y2", "D_dem")
# context name -> (Engine keywords, critic16_pipe, DEPGAN_WGRAD_BF16 at creation, site table)
CONTEXTS = {
    "fp32": ({}, None, None, R.sites(False, False, bf16_mfma=False)),                    # control: no site rounds
    "bf16": ({"bf16_mfma": True}, None, None, R.sites(False, True)),
    "bf16-c16": ({"bf16_mfma": True}, "bfloat16", None, R.sites(True, True)),
    "bf16-wgrad32": ({"bf16_mfma": True}, None, "0", R.sites(False, False)),
}
SIZES = {"64x64-b2": (64, 64, 2, 57), "48x80-b3": (48, 80, 3, 57)}                         # the second: tests/rect_cases.py


def P(t):
    return C.c_void_p(t.data_ptr())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_inputs = {}


def inputs(size):
    if size not in _inputs:
        _inputs[size] = R.case_inputs(*SIZES[size])
    return _inputs[size]


def make_engine(ctx, size):
    import dep_gan_im_amd as dg
    kw, pipe, wg, st = CONTEXTS[ctx]
    H, W, B, _ = SIZES[size]
    PG, PD1, PD2 = inputs(size)[:3]
    saved = os.environ.get("DEPGAN_WGRAD_BF16")
    if wg is not None:
        os.environ["DEPGAN_WGRAD_BF16"] = wg                 # read when the context is created
    try:
        eng = dg.Engine(B, H, W, 2, **kw)
    finally:
        if wg is not None:
            os.environ.pop("DEPGAN_WGRAD_BF16")
            if saved is not None:
                os.environ["DEPGAN_WGRAD_BF16"] = saved
    for n, Pm in zip(NETS, (PG, PD1, PD2)):
        eng.set_weights(n, Pm)
    if pipe is not None:
        eng.critic16_pipe = pipe
    eng.debug_capture(True)
    return eng, st


def read_critic(eng):
    """layer -> the 3B-slot tensors the last critic or generator pass left behind"""
    t = {"act": {n: eng.debug_tensor("d/act/" + n) for n in R.LAYERS},
         "dz": {n: eng.debug_tensor("d/dz/" + n) for n in R.LAYERS},
         "pool": {e[0]: eng.debug_tensor("d/pool/" + e[0]) for e in R.DIS_TRUNK if e[4]},
         "g0": eng.debug_tensor("d/g0")}
    return t


def check_links(links, st, worst, what):
    """the gate of this file, link by link; worst: kind -> largest error seen, in units of S"""
    for ln in links:
        name = "%s: %s %s %s" % (what, ln.kind, ln.layer, ln.tag)
        if ln.exact:
            assert np.array_equal(bits(ln.got), bits(ln.ref_f)), name
            continue
        site, S, e, e_other, d = R.link_errors(ln, st)
        worst[ln.kind] = max(worst.get(ln.kind, 0.0), e)
        assert np.isfinite(np.asarray(ln.got)).all() and e <= R.TOL, (name, "site" if site else "fp32", e, S)
        if site:
            assert e_other > R.SEP, (name, "no operand rounding where the plan is a bf16 plan", e_other, S)
        elif d > R.SEP:
            assert e_other > R.SEP, (name, "an operand rounding where the plan is an fp32 plan", e_other, S)


def audit(eng, which, PD_master, x, y2, z, ep, sites, what=""):
    """One critic closure (gradients only) with the capture on, read back, every link gated.  Returns kind -> worst."""
    lib, B, H, W = eng.lib, eng.batch, eng.height, eng.width
    out = eng.critic(which, y2, x, z, ep, update=False)
    assert np.isfinite(out).all()
    t = read_critic(eng)
    t["in"] = eng.debug_tensor("d/in")
    t["mixed"] = {n: eng.debug_tensor("d/mixed/" + n) for n in R.LAYERS}
    t["grads"] = eng.get_grads(which)
    assert t["in"].shape == (3 * B, H, W, 1) and t["g0"].shape == (2 * B, H, W, 1)
    assert t["dz"]["dis_1b"].shape == (3 * B, H // 2, W // 2, 32) and t["pool"]["dis_1b"].shape == (3 * B, H // 4, W // 4, 32)
    # the mixed image is gone from d/in (u0 took its place): recomputed by the entry the closure calls, same arguments;
    # the real and fake slots must be that entry's output bit for bit
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()   # noqa: E731
    attr = eng.debug_tensor("g/out/gen_segmentation")
    assert attr.shape == (B, H, W, 1)
    ins = torch.full((3 * B, H, W, 1), float("nan"), device="cuda:0")
    hold = [dev(y2), dev(x), dev(attr), dev(np.asarray(ep).reshape(-1))]
    rc = lib.depgan_op_critic_inputs(P(hold[0]), P(hold[1]), eng.nicg, P(hold[2]), P(hold[3]), P(ins), B, H * W,
                                     NETS.index(which) - 1, None)
    assert rc == 0, lib.depgan_last_error()
    torch.cuda.synchronize()
    ins = ins.cpu().numpy()
    assert np.array_equal(bits(t["in"][:2 * B]), bits(ins[:2 * B])), which
    t["mixed_in"] = ins[2 * B:]
    K = R.compute_kernels(PD_master, bool(eng.cfg.bf16_weights))
    worst = {}
    check_links(R.critic_links(K, t, B, delta=float(eng.cfg.delta)), sites, worst, "%s %s" % (what, which))
    print("critic links %s %s: worst per kind, units of S: %s" % (what, which, {k: "%.1e" % v for k, v in worst.items()}))
    return worst


CASES = [(c, s, w) for c in CONTEXTS for s in SIZES for w in NETS[1:] if s == "64x64-b2" or c == "bf16-c16"]


@pytest.mark.parametrize("ctx,size,which", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_every_link_of_a_critic_closure(lib, ctx, size, which):
    PG, PD1, PD2, x, y2, z, ep = inputs(size)
    eng, st = make_engine(ctx, size)
    try:
        audit(eng, which, PD1 if which == "D_y2" else PD2, x, y2, z, ep, st, "%s %s" % (ctx, size))
    finally:
        eng.close()


def test_surface_names_and_refusals(lib):
    """the four names added to depgan_debug_tensor: shapes, and what is no tensor keeps the entry's error"""
    eng, st = make_engine("bf16", "64x64-b2")
    shape = (C.c_int * 4)()
    for name, want in ((b"d/dz/dis_0a", [6, 64, 64, 16]), (b"d/dz/dis_8", [6, 4, 4, 256]), (b"d/pool/dis_0b", [6, 32, 32, 16]),
                       (b"d/pool/dis_5", [6, 4, 4, 128]), (b"d/in", [6, 64, 64, 1]), (b"d/g0", [4, 64, 64, 1])):
        assert lib.depgan_debug_tensor(eng.h, name, None, 0, shape) == 0 and list(shape) == want, name
    for name in (b"d/pool/dis_0a", b"d/pool/dis_8", b"d/dz/nope", b"d/pool/", b"d/in/", b"d/g0x", b"d/dz"):
        assert lib.depgan_debug_tensor(eng.h, name, None, 0, shape) == 1, name
        assert b"unknown tensor" in lib.depgan_last_error(), name
    buf = np.zeros(8, np.float32)
    assert lib.depgan_debug_tensor(eng.h, b"d/in", C.c_void_p(buf.ctypes.data), 8, shape) == 1     # cap too small
    eng.close()


def test_packed_panels_follow_the_masters(lib):
    """Staleness: one update of each critic and one generator step, the critic16 switch off and on, then every link again
    against the masters the context now holds: the forward and backward panels of both plans were repacked by the Adam
    steps (a stale panel is a forward, u-forward or backward-data link off by the weight change, lr = 1e-4 per element
    against a bf16 spacing of 2^-9 relative: measured by the mutant run)."""
    size = "64x64-b2"
    PG, PD1, PD2, x, y2, z, ep = inputs(size)
    eng, st = make_engine("bf16-c16", size)
    try:
        for which in NETS[1:]:
            assert np.isfinite(eng.critic(which, y2, x, z, ep, update=True)).all()
        assert np.isfinite(eng.generator(x, y2, z, "step")).all()
        eng.critic16_pipe = "float32"
        eng.critic16_pipe = "bfloat16"
        for which, P0 in zip(NETS[1:], (PD1, PD2)):
            now = eng.get_weights(which)
            moved = max(float(np.abs(now[k] - P0[k]).max()) for k in P0)
            assert 0.5e-4 < moved < 2.05e-4, (which, moved)                         # one Adam step at lr 1e-4
            audit(eng, which, now, x, y2, z, ep, st, "after updates")
    finally:
        eng.close()


@pytest.mark.parametrize("ctx", ["bf16", "bf16-c16"])
def test_critic_passes_of_the_generator_loss(lib, ctx):
    """After depgan_g_grads: D_y2(fake_y2) in slots [0, B), D_dem(attr) in [B, 2B) -- forward, pool, tail-backward,
    backward-data and image-gradient links of both, both halves of d/g0.  The chain runs with upstream 1 per sample (read
    back from d/dz/dis_8); the -1/B of -loss_fake - loss_fake_dem (GT:592) is applied to both image gradients by
    g_dpre_kernel, dpre = (-(g1 + g2) / B + ...), which tests/test_gpu_step_ops.py holds."""
    size = "64x64-b2"
    PG, PD1, PD2, x, y2, z, ep = inputs(size)
    eng, st = make_engine(ctx, size)
    B = eng.batch
    try:
        assert np.isfinite(eng.generator(x, y2, z, "grads")).all()
        t = read_critic(eng)
        attr = eng.debug_tensor("g/out/gen_segmentation")
        imgs = {"D_y2": (x[..., 0:1] + attr).astype(np.float32), "D_dem": attr}
        worst = {}
        for which, PD, s in (("D_y2", PD1, slice(0, B)), ("D_dem", PD2, slice(B, 2 * B))):
            K = R.compute_kernels(PD, True)
            acts, pools, dz = ({n: v[s] for n, v in t[k].items()} for k in ("act", "pool", "dz"))
            # the upstream the stored dz_10 implies: dz = c * wd[p] * w9[c] where the unit is on
            basis = R.tail_dz_ref(K, acts["dis_8"], np.ones(B))
            c_implied = (dz["dis_8"].astype(np.float64) * basis).sum((1, 2, 3)) / (basis * basis).sum((1, 2, 3))
            assert np.abs(c_implied - 1.0).max() < 1e-6, (which, c_implied)
            check_links(R.pass_links(K, "g-loss", imgs[which], acts, pools, dz, np.ones(B), t["g0"][s]), st, worst,
                        "%s generator %s" % (ctx, which))
        print("critic links %s generator: worst per kind, units of S: %s" % (ctx, {k: "%.1e" % v for k, v in worst.items()}))
    finally:
        eng.close()
