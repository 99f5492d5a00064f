"""Float64 link functions of one critic closure (critic_enqueue, csrc/model.hip), teacher-forced.

Every launch of the closure reads and writes fp32 tensors that stay in memory until the closure ends, so each launch can
be recomputed alone from the operands the library itself stored: same operands on both sides, only the summation order
differs, and the operator criterion |got - ref| <= 1e-4 S, S = max|ref| (tests/test_gpu_ops.py) applies link by link.
Every link's output is the next link's stored input, so all links together cover the closure.

The functions are built from oracle/manual.py (conv_fwd, conv_bwd_data, conv_wgrad, first_argmax_idx, gather_pool, unpool
and the tail formulas of d_forward_store, d_backward, d_gp_grads).  They take NHWC float32 arrays as depgan_debug_tensor
hands them out.  q is RNE float32 -> bf16 -> float32 (O.round_bf16); a launch on the bf16 matrix pipe rounds its activation
operands with it (the kernel operand is the bf16-rounded master in every layer of a bf16 context, whatever the pipe).
Every conv link carries two references, with and without that rounding; sites() says which one the library must meet.

simulate() runs the same site model from the inputs with every convolution in one dtype (float32: the CPU stand-in for
the HIP path, tests/test_critic_links_cpu.py) and returns the tensors in the layout read_back() of the GPU test uses."""
from collections import namedtuple

import numpy as np
import torch

from oracle import depgan_oracle as O
from oracle import manual as M

DIS_TRUNK = O.DIS_TRUNK
LAYERS = [e[0] for e in DIS_TRUNK]
TOL = 1e-4            # the operator criterion, in units of S
SEP = 5e-4            # a misplaced rounding must be at least this far away, in units of S
q = O.round_bf16

# kind: forward / pool / tail-backward / backward-data / image-gradient / u0 / u-forward / weight-gradient /
# bias-gradient / tail-gradient.  launch: the column of sites() that decides the reference (None: never on the bf16 pipe).
# exact: got must equal ref bit for bit.  ref_q == ref_f (the same array) where no operand could have been rounded.
Link = namedtuple("Link", "kind layer tag launch got ref_q ref_f exact")


def sites(critic16, wgrad_bf16, bf16_mfma=True):
    """layer -> {"fwd", "bwd", "wgrad"}: is that launch of the layer on the bf16 matrix pipe?  ("fwd" is the forward and
    the u-forward, one plan; "bwd" of layer l is the launch that turns dz_l into dz_{l-1}.)  Stated from
    dg_plan_conv_bf16 (Cin >= 8, Cin % 4 == 0, Cout % 32 == 0 of the LAUNCH: backward-data exchanges the channels),
    dg_plan_conv_bf16_n16 (5x5, Cout % 16 == 0: taken with critic16 where the first rule does not hold) and
    dg_wgrad_bf16_supported (Cin >= 8, Cin % 4 == 0, Cout % 4 == 0).  dis_0a's backward-data is the image gradient on the
    direct kernel: never.  An fp32 context (bf16_mfma False) has no site."""
    def conv(k, ci, co):
        if not bf16_mfma or ci < 8 or ci % 4:
            return False
        return co % 32 == 0 or (critic16 and k == 5 and co % 16 == 0 and co >= 8)
    out = {}
    for li, (name, k, ci, co, pool) in enumerate(DIS_TRUNK):
        out[name] = {"fwd": conv(k, ci, co), "bwd": li > 0 and conv(k, co, ci),
                     "wgrad": bool(bf16_mfma and wgrad_bf16 and ci >= 8 and ci % 4 == 0 and co % 4 == 0)}
    return out


def case_inputs(H, W, B, seed):
    """config-4 inputs as _setup of tests/test_gpu_g_update_storage.py builds them (2-channel input, tie-free), at any
    H x W"""
    PG = O.init_generator(seed, nicg=2, bias_std=0.05)
    PD1 = O.init_critic(seed + 1, bias_std=0.05, img=(H, W))
    PD2 = O.init_critic(seed + 2, bias_std=0.05, img=(H, W))
    x, y2, z, ep = O.synth_batch(seed + 5, B, H, W, nicg=2)
    rng = np.random.default_rng(seed)
    x = (x + 0.02 * rng.uniform(size=x.shape)).astype(np.float32)
    y2 = (y2 + 0.02 * rng.uniform(size=y2.shape)).astype(np.float32)
    return PG, PD1, PD2, x, y2, z, ep


def compute_kernels(PD, bf16):
    """the weights the launches read: every '/kernel' bf16-rounded in a bf16 context, the masters otherwise"""
    P = O.round_kernels_bf16(PD) if bf16 else PD
    return {k: np.ascontiguousarray(v, np.float32) for k, v in P.items()}


# ----------------------------------------------------------------------------
# primitives: NHWC float32 in, NHWC array of `dt` out
# ----------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _t(a, dt):
    return torch.from_numpy(_f32(a)).to(dt)


def _nchw(a, dt):
    return _t(a, dt).permute(0, 3, 1, 2)


def _out(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _rq(a, rnd):
    return q(_f32(a)) if rnd else _f32(a)


def _wb(K, name, dt):
    return _t(K["conv2d_" + name + "/kernel"], dt), _t(K["conv2d_" + name + "/bias"], dt)


def _tail(K, dt):
    return (_t(K["dis_9/kernel"], dt).reshape(-1), _t(K["dis_9/bias"], dt).reshape(()),
            _t(K["dense_1/kernel"], dt).reshape(-1))


def _nchw_np(a):
    return np.ascontiguousarray(_f32(a).transpose(0, 3, 1, 2))


def pool2(a):
    """2x2 maximum of an NHWC array (exact)"""
    a = _f32(a)
    N, H, W, C = a.shape
    return np.ascontiguousarray(a.reshape(N, H // 2, 2, W // 2, 2, C).max(axis=(2, 4)))


def fwd_ref(K, name, x, rnd, dt=torch.float64):
    w, b = _wb(K, name, dt)
    return _out(torch.relu(M.conv_fwd(_nchw(_rq(x, rnd), dt), w, b)))


def tail_dz_ref(K, a10, coef, dt=torch.float64):
    """dz_10[n, p, c] = coef[n] * wd[p] * w9[c] * (a10 > 0)   (d_backward's first line)"""
    w9, _, wd = _tail(K, dt)
    a = _f32(a10)
    N, h, w, C = a.shape
    d = _t(coef, dt).view(N, 1, 1, 1) * wd.view(1, h, w, 1) * w9.view(1, 1, 1, C)
    return (d * torch.from_numpy(a > 0)).numpy()


def bwd_ref(K, name, dz, act_prev, pool_prev, rnd, dt=torch.float64):
    """backward-data of layer `name`, un-pooled at the first arg-max of act_prev where the previous layer pools, times
    (act_prev > 0): the gradient at the previous layer's conv output"""
    w, _ = _wb(K, name, dt)
    d = M.conv_bwd_data(_nchw(_rq(dz, rnd), dt), w)
    a = _nchw_np(act_prev)
    if pool_prev:
        d = M.unpool(d, torch.from_numpy(M.first_argmax_idx(a)), a.shape[2:])
    return _out(d * torch.from_numpy(a > 0))


def img_grad_ref(K, dz0, rnd, dt=torch.float64):
    w, _ = _wb(K, LAYERS[0], dt)
    return _out(M.conv_bwd_data(_nchw(_rq(dz0, rnd), dt), w))


def u0_ref(g0, delta, dt=torch.float64):
    """u0 = delta * (2 / B) * (norm - 1) / norm * g0   (d_gp_grads)"""
    g = _t(g0, dt)
    B = g.shape[0]
    norm = torch.sqrt((g ** 2).sum((1, 2, 3)))
    return ((delta * 2.0 / B) * ((norm - 1.0) / norm).view(B, 1, 1, 1) * g).numpy()


def ufwd_ref(K, name, u_prev, act_mixed, pool, rnd, dt=torch.float64):
    """conv without bias, times (mixed act > 0), gathered at the mixed pass's arg-max where the layer pools"""
    w, _ = _wb(K, name, dt)
    a = _nchw_np(act_mixed)
    u = M.conv_fwd(_nchw(_rq(u_prev, rnd), dt), w) * torch.from_numpy(a > 0)
    if pool:
        u = M.gather_pool(u, torch.from_numpy(M.first_argmax_idx(a)))
    return _out(u)


def wgrad_ref(x3, dz3, k, rnd, dt=torch.float64):
    return M.conv_wgrad(_nchw(_rq(x3, rnd), dt), _nchw(_rq(dz3, rnd), dt), k).numpy()


def bias_ref(dz3, B, dt=torch.float64):
    """column sums of the unrounded gradient over the real and fake samples only (the penalty has no bias gradient)"""
    return _t(dz3[:2 * B], dt).sum((0, 1, 2)).numpy()


def tail_wgrad_ref(K, a3, B, dt=torch.float64):
    """the four tail tensors from the stored act_10 ([real | fake | u_10]): d_backward's t9 formulas with the upstream
    -1/B, +1/B, and d_gp_grads' two contractions of u_10"""
    w9, b9, wd = _tail(K, dt)
    A = _t(a3, dt)
    N, h, w, C = A.shape
    A = A.reshape(N, h * w, C)
    coef = torch.tensor([-1.0 / B] * B + [1.0 / B] * B + [1.0] * B, dtype=dt)
    c2 = coef[:2 * B]
    return {"dis_9/kernel": torch.einsum("n,p,npc->c", coef, wd, A).reshape(1, 1, C, 1).numpy(),
            "dense_1/kernel": (torch.einsum("n,npc,c->p", coef, A, w9) + b9 * c2.sum()).reshape(-1, 1).numpy(),
            "dis_9/bias": (c2.sum() * wd.sum()).reshape(1).numpy(),
            "dense_1/bias": c2.sum().reshape(1).numpy()}


# ----------------------------------------------------------------------------
# the links
# ----------------------------------------------------------------------------
def _two(fn, single=False):
    if single:
        r = fn(False)
        return r, r
    return fn(True), fn(False)


def pass_links(K, tag, img, acts, pools, dz, coef, g0=None):
    """Forward, pool, tail-backward, backward-data and image-gradient links of one set of N samples that went through the
    critic together.  acts / dz: layer -> (N, ...) stored forward activations / gradients; pools: layer -> stored pooled
    output, or None where it is no longer there (then the exact maximum of acts feeds the next layer and no pool link is
    made); coef: (N,) upstream per sample; g0: the stored image gradient of these samples, or None."""
    x = img
    for name, k, ci, co, pool in DIS_TRUNK:
        rq, rf = _two(lambda r: fwd_ref(K, name, x, r))
        yield Link("forward", name, tag, "fwd", acts[name], rq, rf, False)
        x = acts[name]
        if pool:
            p = pool2(x)
            if pools is not None:
                yield Link("pool", name, tag, None, pools[name], p, p, True)
                x = pools[name]
            else:
                x = p
    last = LAYERS[-1]
    r = tail_dz_ref(K, acts[last], coef)
    yield Link("tail-backward", last, tag, None, dz[last], r, r, False)
    for li in range(len(DIS_TRUNK) - 1, 0, -1):
        name, prev, pool_prev = LAYERS[li], LAYERS[li - 1], DIS_TRUNK[li - 1][4]
        rq, rf = _two(lambda r: bwd_ref(K, name, dz[name], acts[prev], pool_prev, r))
        yield Link("backward-data", prev, tag, ("bwd", name), dz[prev], rq, rf, False)
    if g0 is not None:
        rq, rf = _two(lambda r: img_grad_ref(K, dz[LAYERS[0]], r))
        yield Link("image-gradient", "image", tag, None, g0, rq, rf, False)


def critic_links(K, t, B, delta=10.0):
    """Every link of one critic closure from the tensors it left behind (read_back of the GPU test, or simulate())."""
    rf2, mx = slice(0, 2 * B), slice(2 * B, 3 * B)
    coef = np.array([-1.0 / B] * B + [1.0 / B] * B)
    yield from pass_links(K, "real+fake", t["in"][rf2], {n: t["act"][n][rf2] for n in LAYERS},
                          {n: t["pool"][n][rf2] for n in t["pool"]}, {n: t["dz"][n][rf2] for n in LAYERS}, coef)
    yield from pass_links(K, "mixed", t["mixed_in"], t["mixed"], None, {n: t["dz"][n][mx] for n in LAYERS}, np.ones(B),
                          t["g0"][:B])
    r = u0_ref(t["g0"][:B], delta)
    yield Link("u0", "image", "mixed", None, t["in"][mx], r, r, False)
    u = t["in"][mx]
    for name, k, ci, co, pool in DIS_TRUNK:
        got = (t["pool"] if pool else t["act"])[name][mx]
        rq, rf = _two(lambda r: ufwd_ref(K, name, u, t["mixed"][name], pool, r))
        yield Link("u-forward", name, "mixed", "fwd", got, rq, rf, False)
        u = got
    for li, (name, k, ci, co, pool) in enumerate(DIS_TRUNK):
        x3 = t["in"] if li == 0 else (t["pool"] if DIS_TRUNK[li - 1][4] else t["act"])[LAYERS[li - 1]]
        rq, rf = _two(lambda r: wgrad_ref(x3, t["dz"][name], k, r))
        yield Link("weight-gradient", name, "all", "wgrad", t["grads"]["conv2d_" + name + "/kernel"], rq, rf, False)
        r = bias_ref(t["dz"][name], B)
        yield Link("bias-gradient", name, "real+fake", None, t["grads"]["conv2d_" + name + "/bias"], r, r, False)
    # the tail's weight-gradient inputs were never rounded: one reference
    for n, r in tail_wgrad_ref(K, t["act"][LAYERS[-1]], B).items():
        yield Link("tail-gradient", n, "all", None, t["grads"][n], r, r, False)


def site_of(link, st):
    """does the site table put this link's launch on the bf16 pipe?"""
    if link.launch is None:
        return False
    if isinstance(link.launch, tuple):
        col, layer = link.launch
        return st[layer][col]
    return st[link.layer][link.launch]


def link_errors(link, st):
    """(site, S, |got - chosen ref| / S, |got - other ref| / S, |ref_q - ref_f| / S) of one link; a reference that is
    identically zero (the two tail biases) is measured in absolute terms: S = 1"""
    site = site_of(link, st)
    ref, other = (link.ref_q, link.ref_f) if site else (link.ref_f, link.ref_q)
    ref, other, got = (np.asarray(a, np.float64) for a in (ref, other, link.got))
    assert got.shape == ref.shape, (link.kind, link.layer, got.shape, ref.shape)
    S = float(np.abs(ref).max()) or 1.0
    return site, S, float(np.abs(got - ref).max()) / S, float(np.abs(got - other).max()) / S, \
        float(np.abs(ref - other).max()) / S


# ----------------------------------------------------------------------------
# the site model from the inputs, every convolution in `dt`
# ----------------------------------------------------------------------------
def simulate(K, real, fake, ep, st, delta=10.0, dt=torch.float32):
    """One critic closure under the site table st, each launch computed by the link functions in dtype `dt` from the
    float32 tensors the launches before it stored.  Returns what the library leaves behind, in read_back()'s layout:
    "in" (3B; u0 in the mixed slots), "mixed_in", "act" (u in the mixed slots of the non-pooling layers), "mixed",
    "pool" (u in the mixed slots), "dz", "g0" (B samples), "grads"."""
    B = real.shape[0]
    real, fake = _f32(real), _f32(fake)
    e = _f32(ep).reshape(B, 1, 1, 1)
    mixed_in = (e * real + (np.float32(1.0) - e) * fake).astype(np.float32)
    t = {"in": np.concatenate([real, fake, mixed_in]), "mixed_in": mixed_in, "act": {}, "pool": {}, "dz": {}, "grads": {}}
    x = t["in"]
    for name, k, ci, co, pool in DIS_TRUNK:
        x = t["act"][name] = _f32(fwd_ref(K, name, x, st[name]["fwd"], dt))
        if pool:
            x = t["pool"][name] = pool2(x)
    t["mixed"] = {n: t["act"][n][2 * B:].copy() for n in LAYERS}
    coef = np.array([-1.0 / B] * B + [1.0 / B] * B + [1.0] * B)
    t["dz"][LAYERS[-1]] = _f32(tail_dz_ref(K, t["act"][LAYERS[-1]], coef, dt))
    for li in range(len(DIS_TRUNK) - 1, 0, -1):
        name, prev = LAYERS[li], LAYERS[li - 1]
        t["dz"][prev] = _f32(bwd_ref(K, name, t["dz"][name], t["act"][prev], DIS_TRUNK[li - 1][4], st[name]["bwd"], dt))
    t["g0"] = _f32(img_grad_ref(K, t["dz"][LAYERS[0]][2 * B:], False, dt))
    u = t["in"][2 * B:] = _f32(u0_ref(t["g0"], delta, dt))
    for name, k, ci, co, pool in DIS_TRUNK:
        u = _f32(ufwd_ref(K, name, u, t["mixed"][name], pool, st[name]["fwd"], dt))
        (t["pool"] if pool else t["act"])[name][2 * B:] = u
    for li, (name, k, ci, co, pool) in enumerate(DIS_TRUNK):
        x3 = t["in"] if li == 0 else (t["pool"] if DIS_TRUNK[li - 1][4] else t["act"])[LAYERS[li - 1]]
        t["grads"]["conv2d_" + name + "/kernel"] = _f32(wgrad_ref(x3, t["dz"][name], k, st[name]["wgrad"], dt))
        t["grads"]["conv2d_" + name + "/bias"] = _f32(bias_ref(t["dz"][name], B, dt))
    for n, r in tail_wgrad_ref(K, t["act"][LAYERS[-1]], B, dt).items():
        t["grads"][n] = _f32(r)
    return t
