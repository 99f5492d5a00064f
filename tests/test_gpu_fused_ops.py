"""GPU, operator level: the fp32 convolution kernels WITH what the model launches them with -- the fused epilogue
(csrc/common.h `Epilogue`: BN scale/shift, out_pre, FiLM, ReLU, res, mask, accumulate, the pooled store, the fused
one-channel head), strided views, the grouped and gathered-K launch forms of the transposed convolution, and the weight
gradient's extras -- through depgan_op_conv2d_fused, depgan_op_deconv2x2_igemm and depgan_op_conv2d_wgrad_ex.
tests/test_gpu_ops.py checks the bare contraction; this file checks everything around it.

Method (tests/fused_ref.py, proved on the CPU by tests/test_fused_ref_cpu.py):
  exact operands   small integers and dyadic fractions: no fp32 operation of any kernel form rounds, so the float64
                   evaluation of the contract is the one correct bit pattern -> np.array_equal, no tolerance.
  real operands    out_pre against float64 at TOL; everything after out_pre is one fp32 operation per step, recomputed
                   in numpy float32 from the kernel's OWN out_pre -> np.array_equal for out and pool.
Every operand is a window of a wider buffer (channel slice at a non-zero offset, a sample window of a longer batch,
padding rows and columns), each with another channel count.  What surrounds a read-only window is NaN (a read that
strays poisons the result), what surrounds a written window is a sentinel that must be bitwise unchanged afterwards.
Everything stays inside its allocation.

What each path accepts, from dg_conv_igemm_check / launch_variant / dg_conv_igemm_head_supported (igemm_conv.hip),
dg_conv_wino_supported (igemm_wino.hip), dg_conv_igemm_wp_supported (igemm_wp.hip) and dg_conv_direct_prepare (direct.hip);
"-" = refused with a non-zero status and nothing written (test_refused_cells_...):

  path                          bias affine out_pre FiLM relu res mask accumulate pool head  shapes
  1  MFMA, 16-ch chunks           x     x      x     x    x    x    x      x       x    -    Cin >= 8, Cin % 4, Cout % 4; 1x1 3x3 5x5
  6  MFMA, 8-ch chunks (tile)     x     x      x     x    x    x    x      x       x    x    3x3, Cin % 8, Cout % 32
  7  wave-private                 x     x      x     x    x    x    x      x       x    -    3x3, Cin % 8 <= 64, Cout % 32
  8  Winograd F(2x2,3x3)          x     x      x     x    x    x    x      x       x    x    3x3, Cin % 8, Cout % 32, even H, W
  3  bf16 matrix pipe             x     x      x     x    x    x    x      x       x    -    Cin >= 8, Cout % 32; 1x1 3x3 5x5
  2  direct (edge kernels)        x     x      x     x    x    x    x      x       -    -    any channels; 1x1 3x3 5x5
  pool needs even H and W and no grouped launch; the head needs Cout = 32, no pool, no accumulate, no gathered K.

ACCEPTS below is this matrix; test_every_accepted_cell_has_a_case checks the case table against it.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4   # tests/test_gpu_ops.py: fp32 MFMA == fmaf chain; only summation order differs from the reference
SENT = np.array(0x4B3C2D1E, np.uint32).view(np.float32)[()]      # 1.2e7, not a NaN: what written buffers are prefilled with
NONE = (None, 0, 0, 0)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Win:
    """A (B, H, W, C) window of a wider device buffer (B + 3, H + 2, W + 3, C + extra): samples from 1, rows from 1,
    columns from 2, channels from c0.  `data` fills the window; everything else holds `fill`."""

    def __init__(self, shape, extra, c0, fill, data=None):
        B, H, W, Cc = shape
        assert c0 % 4 == 0 and 0 < c0 <= extra - 4
        self.full0 = np.full((B + 3, H + 2, W + 3, Cc + extra), fill, np.float32)
        self.sl = (slice(1, 1 + B), slice(1, 1 + H), slice(2, 2 + W), slice(c0, c0 + Cc))
        if data is not None:
            self.full0[self.sl] = data
        self.t = torch.from_numpy(self.full0).to("cuda:0")
        Ct = Cc + extra
        self.strides = ((H + 2) * (W + 3) * Ct, (W + 3) * Ct, Ct)
        self.off = 1 * self.strides[0] + 1 * self.strides[1] + 2 * self.strides[2] + c0

    def args(self, off=0, mul=(1, 1, 1)):
        return (C.c_void_p(self.t.data_ptr() + 4 * (self.off + off)),) + tuple(s * m for s, m in zip(self.strides, mul))

    def read(self):
        self.now = self.t.cpu().numpy()
        return self.now[self.sl].copy()

    def outside_unchanged(self):
        """bitwise; call after read()"""
        a, b = bits(self.now).copy(), bits(self.full0).copy()
        a[self.sl] = 0
        b[self.sl] = 0
        return np.array_equal(a, b)

    def unchanged(self):
        return np.array_equal(bits(self.t.cpu().numpy()), bits(self.full0))


class Flat:
    """n floats with 16 sentinel floats on either side (dw, raw, column sums, head_out)."""

    def __init__(self, n, data=None):
        self.full0 = np.full(n + 32, SENT, np.float32)
        if data is not None:
            self.full0[16:16 + n] = np.asarray(data, np.float32).ravel()
        self.n = n
        self.t = torch.from_numpy(self.full0).to("cuda:0")

    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 64)

    def read(self):
        self.now = self.t.cpu().numpy()
        return self.now[16:16 + self.n].copy()

    def outside_unchanged(self):
        return np.array_equal(bits(self.now[:16]), bits(self.full0[:16])) and np.array_equal(bits(self.now[-16:]), bits(self.full0[-16:]))

    def unchanged(self):
        return np.array_equal(bits(self.t.cpu().numpy()), bits(self.full0))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------------------------
# fused epilogue x path
# ---------------------------------------------------------------------------------------------------------------------
# feature sets: make_ops keywords + pre (out_pre requested), pool, head (1: stored output, 2: head_skip_out)
FEATS = {
    "bias": dict(bias=1),
    "affine_relu": dict(bias=1, affine=1, relu=1),
    "film": dict(bias=1, affine=1, film=1, relu=1, res=1, pre=1),            # the generator's FiLM layer
    "pool": dict(bias=1, affine=1, relu=1, pool=1),
    "film_pool": dict(bias=1, affine=1, film=1, relu=1, res=1, pre=1, pool=1),
    "join": dict(res=1, mask=1, bwd=1),                                      # the backward-data join: no ReLU
    "acc": dict(bias=1, acc=1),
    "negpool": dict(bias=1, neg=1, pool=1),                                  # every window negative throughout
    "head": dict(bias=1, affine=1, relu=1, head=1),
    "head_skip": dict(bias=1, affine=1, relu=1, head=2),
}
_ALL = set(FEATS)
ACCEPTS = {1: _ALL - {"head", "head_skip"}, 6: _ALL, 7: _ALL - {"head", "head_skip"}, 8: _ALL,
           3: _ALL - {"head", "head_skip"}, 2: _ALL - {"pool", "film_pool", "negpool", "head", "head_skip"}}
PERSIST = (32, 64, 64, 32, 64, 3)      # more work items than resident workgroups: per-item constants reloaded per sample


def _mfma_cases(path, odd, k5, k1, ck8):
    """(B, H, W, ci, co, k) per feature; odd: the path takes odd sizes (21 x 19), else 22 x 18."""
    R = (21, 19) if odd else (22, 18)
    t = {
        "bias": [(2, *R, 40, 96, 3), (2, 30, 18, 8, 32, 3)] + ([(2, *R, 8, 40, 3)] if path == 1 else []),   # Cout 40: 16-channel tiles
        "affine_relu": [(2, *R, 40, 160, 3)],
        "film": [(2, *R, 48, 96, 3), (3, 30, 18, 8, 32, 3)],
        "pool": [(2, 48, 40, 8, 32, 3), (2, 30, 18, 48, 160, 3)],
        "film_pool": [(2, 22, 18, 40, 96, 3)] + ([PERSIST] if path in (1, 8) else []),
        "join": [(2, *R, 96, 40, 3), (2, *R, 32, 32, 3)],                    # backward-data: the launch runs co -> ci
        "acc": [(2, *R, 40, 96, 3)],
        "negpool": [(2, 30, 18, 8, 32, 3)],
        "head": [(2, *R, 32, 32, 3), (2, 48, 40, 8, 32, 3)],
        "head_skip": [(2, *R, 32, 32, 3)],
    }
    if k5:   # both MF forms where the path has them: NT = 16 and NT = 32 epilogue geometry
        small = (16, 16) if path == 1 else (16, 32)
        t["bias"] += [(2, 21, 19, *small, 5), (2, 17, 33, 32, 32, 5)]
        t["affine_relu"] += [(2, 17, 33, 32, small[1], 5)]
        t["film"] += [(2, 22, 18, 32, 32, 5), (2, 21, 19, *small, 5)]
        t["pool"] += [(2, 22, 18, *small, 5), (2, 22, 18, 32, 32, 5)]
        t["join"] += [(2, 21, 19, 32, 32, 5)]
        t["acc"] += [(2, 21, 19, *small, 5)]
    if k1:
        t["bias"] += [(2, 21, 19, 48, 96, 1)]
        t["film"] += [(2, 21, 19, 48, 96, 1)]
        t["pool"] += [(2, 22, 18, 128, 32, 1)]
        t["acc"] += [(2, 22, 18, 48, 96, 1)]
    return [(path, f, s) for f, ss in t.items() for s in ss]


DIRECT_CASES = [(2, f, s) for f, ss in {
    # one / two input channels x 16 (vec4 on, the 4 x 4-per-thread kernel), x 6 (vec4 off), x 1; one output channel from
    # >= 4 input channels (the 4-pixels-per-thread kernel) and from 2 (the generic kernel's one-channel form); generic
    "bias": [(2, 21, 19, 1, 16, 3), (2, 21, 19, 2, 16, 5), (2, 21, 19, 2, 6, 3), (2, 33, 31, 16, 1, 5), (2, 21, 19, 2, 1, 3),
             (2, 21, 19, 8, 32, 3), (2, 21, 19, 8, 32, 1)],
    "affine_relu": [(2, 21, 19, 1, 16, 3), (2, 21, 19, 2, 6, 3), (2, 21, 19, 16, 1, 5)],
    "film": [(2, 21, 19, 1, 16, 3), (2, 21, 19, 2, 6, 5), (2, 21, 19, 12, 1, 3), (2, 21, 19, 8, 32, 3)],
    "join": [(2, 33, 31, 1, 16, 5), (2, 21, 19, 6, 2, 3), (2, 21, 19, 16, 2, 3)],      # dD/dx: 16 -> 1; 2 -> 6; 2 -> 16
    "acc": [(2, 21, 19, 2, 16, 3), (2, 21, 19, 2, 6, 3), (2, 21, 19, 8, 1, 3)],
    "pool": [(2, 22, 18, 2, 16, 3)], "film_pool": [(2, 22, 18, 8, 32, 3)], "negpool": [(2, 22, 18, 8, 32, 3)],
    "head": [(2, 22, 18, 8, 32, 3)], "head_skip": [(2, 22, 18, 8, 32, 3)],
}.items() for s in ss]

CASES = (_mfma_cases(1, True, True, True, False) + _mfma_cases(6, True, False, False, True) +
         _mfma_cases(7, True, False, False, True) + _mfma_cases(8, False, False, False, True) +
         _mfma_cases(3, True, True, True, False) + DIRECT_CASES)
ACCEPTED = [c for c in CASES if c[1] in ACCEPTS[c[0]]]
REFUSED = [c for c in CASES if c[1] not in ACCEPTS[c[0]]]
_id = lambda c: "p%d-%s-%s" % (c[0], c[1], "x".join(map(str, c[2])))   # noqa: E731


def test_every_accepted_cell_has_a_case():
    have = {(p, f) for p, f, _ in ACCEPTED}
    for p, feats in ACCEPTS.items():
        for f in feats:
            assert (p, f) in have, (p, f)
        for f in _ALL - feats:
            assert any(c[0] == p and c[1] == f for c in REFUSED), (p, f)
    # the shape list of the issue: channel tiles, K tail and Cin 8, both 5x5 forms, 1x1, the edge forms, persistent grid
    shapes = {(p,) + s for p, _, s in ACCEPTED}
    for need in ((1, 40, 96, 3), (1, 40, 160, 3), (1, 8, 32, 3), (1, 16, 16, 5), (1, 32, 32, 5), (1, 48, 96, 1),
                 (2, 1, 16, 3), (2, 2, 6, 3), (2, 16, 1, 5), (2, 2, 1, 3)):
        assert any(s[0] == need[0] and s[4:] == need[1:] for s in shapes), need
    assert (1,) + PERSIST in shapes and (8,) + PERSIST in shapes


def run_fused(lib, path, feat, shape, kind, want_pre=False):
    """One depgan_op_conv2d_fused call on windows of wider buffers.  Returns (status, ops, windows dict)."""
    B, H, W, ci, co, k = shape
    f = dict(FEATS[feat])
    pre, pool, head = f.pop("pre", 0) or want_pre, f.pop("pool", 0), f.pop("head", 0)
    rng = np.random.default_rng(sum(shape) * 131 + path * 17 + len(feat))
    o = fr.make_ops(kind, rng, B, H, W, ci, co, k, head=bool(head), head_tanh=(kind == "real"), **f)
    cin, cout = (co, ci) if o.bwd else (ci, co)
    nan = np.float32("nan")
    w = {"in": Win((B, H, W, cin), 12, 4, nan, o.x),
         "out": Win((B, H, W, cout), 20, 8, SENT, o.old)}
    if pre:
        w["pre"] = Win((B, H, W, cout), 28, 12, SENT)
    if o.res is not None:
        w["res"] = Win((B, H, W, cout), 36, 16, nan, o.res)
    if o.mask is not None:
        w["mask"] = Win((B, H, W, cout), 44, 20, nan, o.mask)
    if pool:
        w["pool"] = Win((B, H // 2, W // 2, cout), 52, 24, SENT)
    if head:
        w["head"] = Flat(B * H * W)
    d = {n: dev(getattr(o, n)) for n in ("w", "bias", "scale", "shift", "head_w", "head_b")}
    # FiLM rows at their own pitch, NaN between them
    ld = cout + 12
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
        *w["out"].args(), *arg("pre"), *arg("res"), *arg("mask"), *arg("pool"), P(d["head_w"]), P(d["head_b"]),
        w["head"].ptr() if head else None, o.head_tanh, int(head == 2), B, H, W, ci, co, k, o.relu,
        int(o.old is not None), path, o.bwd, None)
    torch.cuda.synchronize()
    return rc, o, w, (pre, pool, head)


def _acc64(o, path, kind):
    if path == 3 and kind == "real":      # the bf16 pipe rounds both operands; the reference multiplies the same numbers
        return fr.conv_acc(fr.bf16_round(o.x), fr.bf16_round(o.w), o.bwd)
    return fr.conv_acc(o.x, o.w, o.bwd)


@pytest.mark.parametrize("case", ACCEPTED, ids=_id)
def test_fused_epilogue_exact_operands_are_bit_exact(lib, case):
    from dep_gan_im_amd import _lib
    path, feat, shape = case
    rc, o, w, (pre, pool, head) = run_fused(lib, path, feat, shape, "exact")
    _lib.check(rc, "op_conv2d_fused")
    ref = fr.reference(o)                      # float64: the one correct bit pattern (test_fused_ref_cpu.py)
    assert fr.bounds_hold(ref["stages"])
    if head == 2:
        assert w["out"].unchanged()            # head_skip_out: the 32-channel output is not stored
    else:
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
    if head:
        assert np.array_equal(w["head"].read().reshape(ref["head"].shape), ref["head"])     # identity activation
        assert w["head"].outside_unchanged()
    for n in ("in", "res", "mask"):
        if n in w:
            assert w[n].unchanged()


@pytest.mark.parametrize("case", ACCEPTED, ids=_id)
def test_fused_epilogue_real_operands_contraction_at_tol_and_chain_bit_exact(lib, case):
    """out_pre is requested in every case here: it is what the float32 chain starts from."""
    from dep_gan_im_amd import _lib
    path, feat, shape = case
    rc, o, w, (pre, pool, head) = run_fused(lib, path, feat, shape, "real", want_pre=True)
    _lib.check(rc, "op_conv2d_fused")
    ref = fr.reference(o, acc=_acc64(o, path, "real"))
    got_pre = w["pre"].read()
    e = rel(got_pre, ref["out_pre"])
    print("out_pre rel err %.3g" % e)
    assert e < TOL
    assert w["pre"].outside_unchanged()
    out, _ = fr.post_chain(got_pre, o)         # numpy float32, one operation per step, from the kernel's own out_pre
    if head == 2:
        assert w["out"].unchanged()
    else:
        got = w["out"].read()
        assert np.array_equal(got, out), "out: %d wrong, first at %s" % ((got != out).sum(), np.argwhere(got != out)[:1].tolist())
        assert w["out"].outside_unchanged()
    if pool:
        assert np.array_equal(w["pool"].read(), fr.pool2(out))
        assert w["pool"].outside_unchanged()
    if head:
        h = np.tanh(fr.head(out, o))
        e = rel(w["head"].read().reshape(h.shape), h)
        print("head rel err %.3g" % e)
        assert e < TOL
        assert w["head"].outside_unchanged()


@pytest.mark.parametrize("case", REFUSED, ids=_id)
def test_refused_cells_return_a_status_and_write_nothing(lib, case):
    path, feat, shape = case
    rc, o, w, _ = run_fused(lib, path, feat, shape, "exact")
    assert rc != 0 and lib.depgan_last_error()
    for win in w.values():
        assert win.unchanged()


def test_pool_on_odd_sizes_is_refused(lib):
    for path in (1, 6, 7, 8, 3):
        rc, o, w, _ = run_fused(lib, path, "pool", (2, 21, 19, 8, 32, 3), "exact")
        assert rc != 0, path
        assert all(win.unchanged() for win in w.values())


# ---------------------------------------------------------------------------------------------------------------------
# the 2x2 / stride-2 transposed convolution on the implicit-GEMM kernels: grouped launch, gathered K, four accumulating
# launches
# ---------------------------------------------------------------------------------------------------------------------
DECONV_CASES = [(2, 16, 16, 64, 64), (2, 8, 8, 96, 96), (2, 8, 8, 128, 128), (2, 12, 20, 64, 96)]   # B, H, W, Cin, Cout


def _deconv_ops(kind, case, seed):
    B, H, W, ci, co = case
    rng = np.random.default_rng(seed)
    ex = kind == "exact"
    x = rng.integers(-2, 3, (B, H, W, ci)).astype(np.float32) if ex else rng.standard_normal((B, H, W, ci)).astype(np.float32)
    dy = (rng.integers(-2, 3, (B, 2 * H, 2 * W, co)).astype(np.float32) if ex
          else rng.standard_normal((B, 2 * H, 2 * W, co)).astype(np.float32))
    wt = (rng.integers(-1, 2, (2, 2, co, ci)).astype(np.float32) if ex
          else (rng.standard_normal((2, 2, co, ci)) / np.sqrt(ci)).astype(np.float32))
    return x, dy, wt


@pytest.mark.parametrize("path", [1, 3])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("case", DECONV_CASES)
def test_deconv_forward_as_grouped_launch(lib, case, kind, path):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = case
    x, _, wt = _deconv_ops(kind, case, ci + co + H)
    o = fr.make_ops(kind, np.random.default_rng(H), 1, 1, 1, ci, co, 1, bias=1, affine=1, relu=1)   # bias, scale, shift
    win = Win((B, H, W, ci), 12, 4, np.float32("nan"), x)
    wout = Win((B, 2 * H, 2 * W, co), 20, 8, SENT)                 # the deconvolution's slice of a concat buffer
    d = [dev(a) for a in (wt, o.bias, o.scale, o.shift)]
    _lib.check(lib.depgan_op_deconv2x2_igemm(0, *win.args(), *map(P, d), *wout.args(), *NONE, B, H, W, ci, co, 1, path, None))
    torch.cuda.synchronize()
    xr, wr = (fr.bf16_round(x), fr.bf16_round(wt)) if (path == 3 and kind == "real") else (x, wt)
    ref = np.maximum(fr.affine(fr.deconv2x2(xr, wr), o, np.float64), 0)
    got = wout.read()
    if kind == "exact":
        assert np.array_equal(got, ref), np.argwhere(got != ref)[:1].tolist()
    else:
        assert rel(got, ref) < TOL
    assert wout.outside_unchanged() and win.unchanged()


@pytest.mark.parametrize("path", [1, 3])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("case", DECONV_CASES)
def test_deconv_backward_data_gathered_and_accumulated(lib, case, kind, path):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = case
    _, dy, wt = _deconv_ops(kind, case, ci + co + W)
    rng = np.random.default_rng(W)
    dyr, wr = (fr.bf16_round(dy), fr.bf16_round(wt)) if (path == 3 and kind == "real") else (dy, wt)
    g = fr.deconv2x2_bwd_data(dyr, wr)
    got = {}
    for masked in (0, 1):
        mask = rng.choice(fr.MASKS, (B, H, W, ci)).astype(np.float32) if masked else None
        ref = np.where(mask > 0, g, 0.0) if masked else g
        for form in (1, 2):
            wdy = Win((B, 2 * H, 2 * W, co), 12, 4, np.float32("nan"), dy)         # the gradient's slice of a concat buffer
            wdx = Win((B, H, W, ci), 20, 8, SENT)
            wm = Win((B, H, W, ci), 44, 20, np.float32("nan"), mask) if masked else None
            wd = dev(wt)
            _lib.check(lib.depgan_op_deconv2x2_igemm(form, *wdy.args(), P(wd), None, None, None, *wdx.args(),
                                                     *(wm.args() if masked else NONE), B, H, W, ci, co, 0, path, None))
            torch.cuda.synchronize()
            got[form] = wdx.read()
            if kind == "exact":
                assert np.array_equal(got[form], ref), (form, masked, np.argwhere(got[form] != ref)[:1].tolist())
            else:
                assert rel(got[form], ref) < TOL, (form, masked)
            assert wdx.outside_unchanged() and wdy.unchanged()
        if kind == "exact":
            assert np.array_equal(bits(got[1]), bits(got[2]))      # the two forms agree bit for bit


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient: strided operands, column sums over the first colB samples, scale / raw / accumulate / OI layout
# ---------------------------------------------------------------------------------------------------------------------
WGRAD_CASES = [  # B, H, W, Cin, Cout, k, colB (0: none), scale, raw, accumulate, oi, grid (None: channel slices)
    (3, 22, 18, 48, 40, 3, 2, 1, 1, 0, 0, None), (2, 21, 19, 40, 96, 3, 2, 0, 0, 1, 0, None),
    (2, 17, 13, 32, 32, 5, 1, 1, 0, 1, 1, None), (3, 21, 19, 64, 64, 3, 1, 1, 1, 0, 1, None),
    (2, 12, 10, 64, 96, 1, 0, 1, 1, 0, 1, (1, 0)), (3, 8, 12, 96, 64, 1, 2, 1, 0, 1, 1, (0, 1)),
    # the edge-layer kernels (Cin 1, 2): their column sums are the separate streaming pass
    (3, 21, 19, 1, 16, 3, 2, 1, 1, 0, 0, None), (2, 21, 19, 2, 16, 5, 1, 0, 0, 1, 0, None), (2, 20, 16, 2, 32, 3, 0, 1, 0, 0, 1, None),
]


# bf16 = 1 where wgrad_bf16.hip has a form: the edge kernels have none (status 3, tests/test_fused_ref_cpu.py)
WGRAD_PARAMS = [(c, kind, bf16) for c in WGRAD_CASES for kind in ("exact", "real") for bf16 in (0, 1) if not (bf16 and c[3] < 8)]


@pytest.mark.parametrize("case,kind,bf16", WGRAD_PARAMS)
def test_wgrad_extras(lib, case, kind, bf16):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co, k, colB, scaled, raw, acc, oi, grid = case
    rng = np.random.default_rng(ci * 100 + co + k + B)
    ex = kind == "exact"
    gen = (lambda s: rng.integers(-2, 3, s).astype(np.float32)) if ex else (lambda s: rng.standard_normal(s).astype(np.float32))
    x = gen((B, H, W, ci))
    gh, gw = (2 * H, 2 * W) if grid else (H, W)
    dyf = gen((B, gh, gw, co))                                     # the buffer dy is a view of
    if colB and colB < B:   # the samples the column sums must ignore hold large values (exact in bf16 as well)
        dyf[colB:] = (rng.integers(-8, 9, dyf[colB:].shape) * 64.0) if ex else dyf[colB:] * 1e4
    dy = dyf[:, grid[0]::2, grid[1]::2] if grid else dyf
    scale = (rng.choice(fr.SCALES, co) if ex else rng.uniform(0.5, 1.5, co)).astype(np.float32) if scaled else None
    cscale = (rng.choice(fr.SCALES, co) if ex else rng.uniform(0.5, 1.5, co)).astype(np.float32) if colB else None
    old = ((rng.integers(-32, 33, (k, k, ci, co)) / 8.0) if ex else rng.standard_normal((k, k, ci, co))).astype(np.float32)
    lay = (lambda a: np.ascontiguousarray(a.transpose(0, 1, 3, 2))) if oi else (lambda a: a)
    xr, dyr = (fr.bf16_round(x), fr.bf16_round(dy)) if (bf16 and not ex) else (x, dy)
    g = fr.wgrad(xr, dyr, k)
    ref_dw = lay(g * (scale.astype(np.float64) if scaled else 1.0) + (old if acc else 0.0))
    col = dy[:colB].astype(np.float64).sum(axis=(0, 1, 2)) if colB else None
    nan = np.float32("nan")
    outs = []
    sd, csd = dev(scale), dev(cscale)        # named: a temporary would be freed, and its memory reused, before the call
    for rep in range(2):
        wx = Win((B, H, W, ci), 12, 4, nan, x)
        wdy = Win((B, gh, gw, co), 20, 8, nan, dyf)
        dyargs = wdy.args(grid[0] * wdy.strides[1] + grid[1] * wdy.strides[2], (1, 2, 2)) if grid else wdy.args()
        fdw = Flat(k * k * ci * co, lay(old) if acc else None)
        fraw = Flat(k * k * ci * co) if raw else None
        fco, fcr = (Flat(co), Flat(co)) if colB else (None, None)
        rc = lib.depgan_op_conv2d_wgrad_ex(*wx.args(), *dyargs, P(sd), fdw.ptr(), fraw.ptr() if raw else None,
                                           acc, oi, colB, P(csd), fco.ptr() if colB else None,
                                           fcr.ptr() if colB else None, B, H, W, ci, co, k, bf16, None)
        _lib.check(rc, "op_conv2d_wgrad_ex")
        torch.cuda.synchronize()
        res = {"dw": fdw.read(), "raw": fraw.read() if raw else None, "colout": fco.read() if colB else None,
               "colraw": fcr.read() if colB else None}
        for fl in (fdw, fraw, fco, fcr):
            assert fl is None or fl.outside_unchanged()
        assert wx.unchanged() and wdy.unchanged()
        outs.append(res)
    for key in outs[0]:      # two runs bitwise equal
        assert outs[0][key] is None or np.array_equal(bits(outs[0][key]), bits(outs[1][key])), key
    r = outs[0]
    cmp = (lambda a, b, what: np.array_equal(a, np.asarray(b).ravel())) if ex else (lambda a, b, what: rel(a, np.asarray(b).ravel()) < TOL)
    assert cmp(r["dw"], ref_dw, "dw")
    if raw:
        assert cmp(r["raw"], lay(g), "raw")
    if colB:
        assert cmp(r["colraw"], col, "colraw"), (r["colraw"][:4], col[:4])
        assert cmp(r["colout"], col * cscale.astype(np.float64), "colout")
