"""Plain references for the fused epilogue of the fp32 convolution kernels (csrc/common.h `Epilogue`), shared by
tests/test_fused_ref_cpu.py (which proves the exact-operand method) and tests/test_gpu_fused_ops.py (which uses it).

Two kinds of operands:

exact   x, dy integers in [-2, 2]; weights integers in [-1, 1]; bias, shift, film_add, res and the accumulate prefill
        multiples of 1/8; scale in {0.5, 0.75, 1, 1.25, 1.5}; film_mul multiples of 1/4 in [-2, 2]; mask from
        {-1, -0.0, 0, 1e-30, 1}.  Every intermediate of every kernel form is then a multiple of 2^-7 below 2^15 -- 22
        significant bits -- so no fp32 operation rounds, in any summation order, fused or not: the float64 evaluation
        of the contract is THE bit pattern (test_fused_ref_cpu.py asserts the bounds and the float32 == float64
        equality stage by stage, the Winograd transforms included).
real    standard normal operands, weights scaled by 1/sqrt(K).  The contraction and the affine are compared with float64
        at a tolerance; everything after out_pre is ONE fp32 operation per step, so post_chain() recomputes it in numpy
        float32 from the kernel's own out_pre and the result must match bit for bit.
"""
import numpy as np
import torch
import torch.nn.functional as F

SCALES = np.array([0.5, 0.75, 1.0, 1.25, 1.5])
MASKS = np.array([-1.0, -0.0, 0.0, 1e-30, 1.0], np.float32)
# bounds the exactness argument rests on (asserted by bounds_hold() for the largest K of the case table)
ACC_BOUND = 2 * 9 * 224          # |x| <= 2, |w| <= 1, K = 9 * 224 products at most (5x5: 25 * 32 = 800)
QUANTUM = 2.0 ** -7              # every stage is a multiple of this ...
VALUE_BOUND = 2.0 ** 15          # ... and below this in magnitude: 22 bits, fp32 holds 24


class Ops:
    """Operands of one fused convolution; absent ones are None.  The layer is (k, k, ci, co) = w.shape; bwd = 1 runs its
    backward-data form: x then has co channels and every output-side operand ci."""

    def __init__(self, **kw):
        self.x = self.w = self.bias = self.scale = self.shift = self.fmul = self.fadd = None
        self.res = self.mask = self.old = self.head_w = self.head_b = None
        self.relu = self.bwd = self.head_tanh = 0
        self.__dict__.update(kw)


def make_ops(kind, rng, B, H, W, ci, co, k, bias=False, affine=False, film=False, relu=False, res=False, mask=False,
             acc=False, neg=False, head=False, head_tanh=False, bwd=False):
    """kind 'exact' or 'real'.  neg: a shift that makes every output negative (the pooled maximum of a window that never
    sees a positive value).  head: weights of the fused one-channel head (exact: integers in [-1, 1]; the dot product over 32
    outputs of a layer without FiLM stays inside the bounds)."""
    cin, cout = (co, ci) if bwd else (ci, co)          # channels of the launch's input and output
    K = k * k * cin
    ex = kind == "exact"
    o = Ops(relu=int(relu), bwd=int(bwd), head_tanh=int(head_tanh))
    eighth = lambda shape, r: (rng.integers(-8 * r, 8 * r + 1, shape) / 8.0).astype(np.float32)   # noqa: E731
    nrm = lambda shape: rng.standard_normal(shape).astype(np.float32)                              # noqa: E731
    o.x = rng.integers(-2, 3, (B, H, W, cin)).astype(np.float32) if ex else nrm((B, H, W, cin))
    o.w = (rng.integers(-1, 2, (k, k, ci, co)).astype(np.float32) if ex
           else (rng.standard_normal((k, k, ci, co)) / np.sqrt(K)).astype(np.float32))
    if bias:
        o.bias = eighth(cout, 2) if ex else nrm(cout)
    if affine or neg:
        o.scale = rng.choice(SCALES, cout).astype(np.float32) if ex else rng.uniform(0.5, 1.5, cout).astype(np.float32)
        o.shift = eighth(cout, 2) if ex else nrm(cout)
        if neg:
            o.shift = (o.shift - (3 * K + 8 if ex else 24)).astype(np.float32)
    if film:
        o.fmul = (rng.integers(-8, 9, (B, cout)) / 4.0).astype(np.float32) if ex else nrm((B, cout))
        o.fadd = eighth((B, cout), 2) if ex else nrm((B, cout))
        if ex:
            o.fmul[0, :3] = (-1.25, 0.0, 2.0)[:min(3, cout)]   # a negative, a zero and the largest multiplier are always present
    if res:
        o.res = eighth((B, H, W, cout), 4) if ex else nrm((B, H, W, cout))
    if mask:
        o.mask = (rng.choice(MASKS, (B, H, W, cout)) if ex
                  else np.where(rng.random((B, H, W, cout)) < 0.1, 0, rng.standard_normal((B, H, W, cout)))).astype(np.float32)
    if acc:
        o.old = eighth((B, H, W, cout), 4) if ex else nrm((B, H, W, cout))
    if head:
        o.head_w = rng.integers(-1, 2, cout).astype(np.float32) if ex else (nrm(cout) / np.sqrt(cout)).astype(np.float32)
        o.head_b = eighth(1, 1) if ex else nrm(1)
    return o


def _nchw(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).permute(0, 3, 1, 2)


def conv_acc(x, w, bwd=0, dtype=torch.float64):
    """The raw contraction, 'same' padding, cross-correlation (Keras Conv2D); bwd: its backward-data form
    dx = d/dx <conv(x, w), dy> with dy given as x.  NHWC in, NHWC numpy of `dtype` out."""
    k = w.shape[0]
    wt = torch.from_numpy(np.ascontiguousarray(w)).to(dtype).permute(3, 2, 0, 1)       # (co, ci, k, k)
    if bwd:
        y = F.conv_transpose2d(_nchw(x, dtype), wt, padding=k // 2)
    else:
        y = F.conv2d(_nchw(x, dtype), wt, padding=k // 2)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def affine(acc, o, dt, form="direct"):
    """v = (acc + bias) * scale + shift in dtype dt.  form 'direct': as written, two roundings after the bias add
    (epilogue.h); 'mfma': acc * scale + (bias * scale + shift), the MFMA kernels' single FMA with its constant formed by
    one FMA (numpy has no FMA: the product is rounded here, which is the same value whenever the product is exact)."""
    v = acc.astype(dt)
    b = np.zeros(1, dt) if o.bias is None else o.bias.astype(dt)
    if o.scale is None:
        return (v + b).astype(dt)
    s, t = o.scale.astype(dt), o.shift.astype(dt)
    if form == "direct":
        return (((v + b).astype(dt) * s).astype(dt) + t).astype(dt)
    return ((v * s).astype(dt) + ((b * s).astype(dt) + t).astype(dt)).astype(dt)


def post_chain(pre, o, dt=np.float32):
    """Everything after out_pre, one operation of dtype dt per step: FiLM multiply, FiLM add, ReLU, res add, mask
    select, accumulate add.  Returns (out, stages) -- stages lists every intermediate, for the bound checks."""
    v = pre.astype(dt)
    st = [v]
    if o.fmul is not None:
        v = (v * o.fmul.astype(dt)[:, None, None, :]).astype(dt)
        st.append(v)
        v = (v + o.fadd.astype(dt)[:, None, None, :]).astype(dt)
        st.append(v)
    if o.relu:
        v = np.maximum(v, dt(0))
    if o.res is not None:
        v = (v + o.res.astype(dt)).astype(dt)
        st.append(v)
    if o.mask is not None:
        v = np.where(o.mask > 0, v, dt(0)).astype(dt)
    if o.old is not None:
        v = (v + o.old.astype(dt)).astype(dt)
        st.append(v)
    return v, st


def pool2(out):
    """2x2 / stride-2 maximum of an NHWC array with even H and W."""
    B, H, W, C = out.shape
    return out.reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def head(out, o, dt=np.float64):
    """The fused one-channel head before its activation: sum_c out[..., c] head_w[c] + head_b."""
    return (out.astype(dt) * o.head_w.astype(dt)).sum(axis=-1).astype(dt) + dt(o.head_b[0])


def reference(o, dt=np.float64, form="direct", acc=None):
    """The whole contract in dtype dt: dict of acc, out_pre, out, stages (+ pool when H and W are even, head when the
    operands carry one).  acc: a contraction computed elsewhere (bf16-rounded operands, a Winograd evaluation)."""
    if acc is None:
        acc = conv_acc(o.x, o.w, o.bwd, torch.float64 if dt == np.float64 else torch.float32)
    pre = affine(acc, o, dt, form)
    out, st = post_chain(pre, o, dt)
    r = {"acc": acc, "out_pre": pre, "out": out, "stages": [acc.astype(dt)] + st}
    if not (out.shape[1] | out.shape[2]) & 1:
        r["pool"] = pool2(out)
    if o.head_w is not None:
        r["head"] = head(out, o, dt)
        r["stages"].append(r["head"])
    return r


def bounds_hold(stages):
    """Every stage a multiple of QUANTUM below VALUE_BOUND: what makes each fp32 operation on the way exact."""
    for s in stages:
        s = np.asarray(s, np.float64)
        if not (np.abs(s).max() < VALUE_BOUND and np.array_equal(s / QUANTUM, np.round(s / QUANTUM))):
            return False
    return True


def bf16_round(a):
    """float32 -> nearest bf16 (ties to even) -> float32: what the bf16 matrix pipe does to both operands."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def deconv2x2(x, w_hwoi, dtype=torch.float64):
    """Conv2DTranspose 2x2 / stride 2: x (B, H, W, Cin), Keras kernel (2, 2, Cout, Cin) -> (B, 2H, 2W, Cout)."""
    wt = torch.from_numpy(np.ascontiguousarray(w_hwoi)).to(dtype).permute(3, 2, 0, 1)   # (Cin, Cout, 2, 2)
    return F.conv_transpose2d(_nchw(x, dtype), wt, stride=2).permute(0, 2, 3, 1).contiguous().numpy()


def deconv2x2_bwd_data(dy, w_hwoi, dtype=torch.float64):
    """Its backward-data: dy (B, 2H, 2W, Cout) -> (B, H, W, Cin), by autograd of the forward."""
    B, H2, W2, _ = dy.shape
    x = torch.zeros((B, w_hwoi.shape[3], H2 // 2, W2 // 2), dtype=dtype, requires_grad=True)
    wt = torch.from_numpy(np.ascontiguousarray(w_hwoi)).to(dtype).permute(3, 2, 0, 1)
    y = F.conv_transpose2d(x, wt, stride=2)
    (g,) = torch.autograd.grad(y, x, _nchw(dy, dtype))
    return g.permute(0, 2, 3, 1).contiguous().numpy()


def wgrad(x, dy, k, dtype=torch.float64):
    """Weight gradient of the 'same' convolution: (k, k, Cin, Cout), by autograd."""
    ci, co = x.shape[3], dy.shape[3]
    w = torch.zeros((co, ci, k, k), dtype=dtype, requires_grad=True)
    y = F.conv2d(_nchw(x, dtype), w, padding=k // 2)
    (g,) = torch.autograd.grad(y, w, _nchw(dy, dtype))
    return g.permute(2, 3, 1, 0).contiguous().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# bf16 activation STORAGE (depgan_op_*_bf16s): the value in front of the store is known exactly on the exact operands,
# so the stored bf16 is its round-to-nearest-even -- one bit pattern (tests/test_bf16s_ref_cpu.py proves the pieces,
# tests/test_gpu_bf16s_exact.py uses them).  Everything below is numpy on the bits of finite float32 values.
# ---------------------------------------------------------------------------------------------------------------------
def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)


def _f32(b):
    return ((b << np.uint64(16)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)


def rne_bf16(a):
    """float32 -> nearest bf16, ties to even -> float32, by integer arithmetic on the bits (finite values)."""
    b = _u32(a)
    return _f32((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16))


def trunc_bf16(a):
    """MUTANT: the low 16 bits dropped (round toward zero)."""
    return _f32(_u32(a) >> np.uint64(16))


def half_away_bf16(a):
    """MUTANT: round to nearest, ties away from zero (sign-magnitude bits: adding to them grows the magnitude)."""
    return _f32((_u32(a) + np.uint64(0x8000)) >> np.uint64(16))


def is_bf16(a):
    """every value representable in bf16 (low 16 bits of the float32 pattern clear)"""
    return a is None or not (np.ascontiguousarray(a, np.float32).view(np.uint32) & 0xFFFF).any()


MASKS_BF16 = rne_bf16(MASKS)       # {-1, -0.0, 0, RNE_bf16(1e-30), 1}: the mask operand is a bf16 view
ZERO_FILM_CHANNEL = 3              # make_ops_bf16s: FiLM multiplier and addend forced to 0 on this channel


def make_ops_bf16s(kind, rng, *a, **kw):
    """make_ops (same draws, so the cases of the fp32 files keep their operands), then for the bf16-storage kernels:
    exact + FiLM: channel ZERO_FILM_CHANNEL gets fmul = fadd = 0 in every sample, next to the (-1.25, 0, 2) make_ops
    plants -- its FiLM value is exactly 0, its decision 0 and its output the residual; real: x and res rounded to bf16
    first (they are stored activations)."""
    o = make_ops(kind, rng, *a, **kw)
    if kind == "exact":
        if o.fmul is not None:
            o.fmul[:, ZERO_FILM_CHANNEL] = 0.0
            o.fadd[:, ZERO_FILM_CHANNEL] = 0.0
        if o.mask is not None:
            o.mask = rne_bf16(o.mask)
    else:
        o.x = rne_bf16(o.x)
        if o.res is not None:
            o.res = rne_bf16(o.res)
        if o.mask is not None:
            o.mask = rne_bf16(o.mask)
    return o


def pack_dec(dec):
    """(B, H, W, C) booleans -> bytes: bit (c & 7) of byte [pixel * (C / 8) + c / 8] (include/depgan.h)."""
    return np.packbits(np.ascontiguousarray(dec, bool).reshape(-1, 8), axis=-1, bitorder="little").ravel()


def reference_bf16s(o, rnd=rne_bf16):
    """The contract of the bf16-storage convolutions on EXACT operands (every float64 value of reference(o) is then a
    float32 value, so the cast in front of `rnd` does not round): out = rnd(exact out), pool = pool2 of the STORED
    values, head from the stored values, u = rnd(out_pre), dec = (FiLM value > 0) and its packed bytes."""
    r = reference(o)
    f32 = lambda a: a.astype(np.float32)   # noqa: E731
    assert np.array_equal(f32(r["out"]).astype(np.float64), r["out"])
    out = rnd(f32(r["out"]))
    q = {"acc": r["acc"], "out_pre": r["out_pre"], "out_exact": r["out"], "out": out, "stages": list(r["stages"]),
         "u": rnd(f32(r["out_pre"]))}
    if not (out.shape[1] | out.shape[2]) & 1:
        q["pool"] = pool2(out)
    if o.head_w is not None:
        q["stages"].pop()                  # reference()'s head of the unrounded values is not part of this contract
        q["head"] = head(out, o)
        q["stages"].append(q["head"])
    if o.fmul is not None:
        v = r["out_pre"] * o.fmul.astype(np.float64)[:, None, None, :] + o.fadd.astype(np.float64)[:, None, None, :]
        q["dec"] = v > 0
        q["dec_bits"] = pack_dec(q["dec"])
    return q


def unpool_mask(dpool, a, skip=None, last=False):
    """depgan_op_unpool_mask(_bf16s): dpool (B, Ho, Wo, C) goes to the FIRST maximum of each 2x2 window of a
    (B, 2Ho, 2Wo, C) in the order (0,0), (0,1), (1,0), (1,1); then + skip; then * (a > 0).  float64.
    last: MUTANT taking the last maximum."""
    B, Ho, Wo, Cc = dpool.shape
    win = np.asarray(a, np.float64).reshape(B, Ho, 2, Wo, 2, Cc).transpose(0, 1, 3, 5, 2, 4).reshape(B, Ho, Wo, Cc, 4)
    am = 3 - win[..., ::-1].argmax(-1) if last else win.argmax(-1)      # numpy: the first of equal maxima
    g = (np.arange(4) == am[..., None]) * np.asarray(dpool, np.float64)[..., None]
    g = g.reshape(B, Ho, Wo, Cc, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(B, 2 * Ho, 2 * Wo, Cc)
    if skip is not None:
        g = g + np.asarray(skip, np.float64)
    return np.where(np.asarray(a) > 0, g, 0.0)
