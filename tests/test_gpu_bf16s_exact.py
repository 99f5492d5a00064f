"""GPU, operator level: the bf16-activation-storage kernels (igemm_bf16s_kernel, its head and training variants,
edge_conv_bf16s_kernel, igemm_bf16_mh_kernel, wgrad_bf16s.hip, unpool_mask_bf16s_kernel) through depgan_op_*_bf16s, bit
for bit and on windowed views.  tests/test_gpu_bf16_store.py holds them inside a bound on channel slices of dense
buffers; this file states the one correct bit pattern.

Method (tests/fused_ref.py; proved on the CPU by tests/test_bf16s_ref_cpu.py, case table in tests/bf16s_cases.py):
  exact operands   small integers and dyadic fractions that are bf16 values: no fp32 operation of the kernel rounds, so
                   the float64 evaluation of the contract is THE value in front of the store and the stored bf16 is its
                   round-to-nearest-even (fused_ref.rne_bf16) -> np.array_equal, no tolerance.  7 % to 33 % of the
                   outputs round at the store and about 7 % are exact ties, so ties-to-even is tested on thousands of
                   ties per case.  The pool is pool2 of the stored values, the head is computed from the stored values,
                   u = RNE(out_pre), the decision bits are compared as bytes.
  real operands    standard-normal x and res rounded to bf16 first, weights scaled by 1/sqrt(K): the kernel is compared
                   bit for bit with its fp32-storage sibling on the same widened operands (depgan_op_conv2d_fused path
                   3, depgan_op_deconv2x2_igemm path 3, depgan_op_conv2d_bwd_data path 3, depgan_op_conv2d_wgrad_bf16 --
                   tests/test_gpu_fused_ops.py and tests/test_gpu_ops.py hold those against float64): they share the
                   main loop's text and the epilogue's arithmetic, so out == RNE(sibling out), pool == pool2(stored out),
                   u == RNE(sibling out_pre), dec == (one float32 multiply, one float32 add of the sibling's out_pre > 0),
                   head_out == depgan_op_head_bf16s of the stored output.  No element is left out.
Views: every bf16 operand is a (B, H, W, C) window of a (B + 3, H + 2, W + 3, C + extra) buffer with its origin at sample
1, row 1, column 2, channel c0 (c0 and extra multiples of 8: pointer and strides stay 16-byte aligned); every window of one
call has another `extra`, so no two views share a pitch, no row pitch is W * C and no sample pitch H times the row
pitch.  Around a read window the buffer holds NaN, written windows are prefilled inside and outside with a sentinel that is
not NaN and must be bitwise unchanged outside afterwards (what a ragged tile writes next to the window in the row and
column directions included); dense outputs (pool, u_out, dec_bits, head_out, dw, colsum) have 16 sentinel elements on
either side.  Read-only operands are compared bitwise with their initial contents after the call.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16s_cases as bc  # noqa: E402
import fused_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4   # tests/test_gpu_ops.py: the project's criterion against float64 where only the summation order differs
SENT = np.array(0x4B3C2D1E, np.uint32).view(np.float32)[()]      # tests/test_gpu_fused_ops.py: 1.2e7, not a NaN
SENT_H, NAN_H, SENT_B = 0x4B3C, 0x7FC0, 0xA5                       # bf16 1.2e7; bf16 NaN; a byte
NANF = np.float32("nan")
NONE = (None, 0, 0, 0)
ESIZE = {"f": 4, "h": 2, "b": 1}
NPT = {"f": np.float32, "h": np.uint16, "b": np.uint8}


def h_bits(a):
    """bf16-valued float32 -> the 16 bits"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def h_wide(u16):
    return (np.ascontiguousarray(u16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _raw(a):
    """the bits of a float32 / uint16 / uint8 array"""
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _to_dev(full, dt):
    return torch.from_numpy(full.view(np.int16) if dt == "h" else full).to("cuda:0")


def _to_host(t, dt):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dt == "h" else a


class Win:
    """A (B, H, W, C) window of a wider device buffer (B + 3, H + 2, W + 3, C + extra): samples from 1, rows from 1,
    columns from 2, channels from c0; dt "h" (bf16, as bits) or "f" (fp32).  `data` fills the window, everything else
    holds `fill`.  With a sample stride of 0 (args(sB=0)) the window has ONE sample."""

    def __init__(self, shape, extra, c0, dt, fill, data=None):
        B, H, W, Cc = shape
        q = 8 if dt == "h" else 4
        assert c0 % q == 0 and (Cc + extra) % q == 0 and 0 < c0 <= extra - q
        self.dt = dt
        self.full0 = np.full((B + 3, H + 2, W + 3, Cc + extra), fill, NPT[dt])
        self.sl = (slice(1, 1 + B), slice(1, 1 + H), slice(2, 2 + W), slice(c0, c0 + Cc))
        if data is not None:
            self.full0[self.sl] = h_bits(data) if dt == "h" else data
        self.t = _to_dev(self.full0, dt)
        Ct = Cc + extra
        self.strides = ((H + 2) * (W + 3) * Ct, (W + 3) * Ct, Ct)
        self.off = 1 * self.strides[0] + 1 * self.strides[1] + 2 * self.strides[2] + c0
        assert all(s % q == 0 for s in self.strides) and self.off % q == 0 and self.t.data_ptr() % 16 == 0

    def args(self, off=0, mul=(1, 1, 1), sB=None, dY=0):
        s = [a * m for a, m in zip(self.strides, mul)]
        if sB is not None:
            s[0] = sB
        s[1] += dY
        return (C.c_void_p(self.t.data_ptr() + ESIZE[self.dt] * (self.off + off)),) + tuple(s)

    def read(self):
        self.now = _to_host(self.t, self.dt)
        w = self.now[self.sl].copy()
        return h_wide(w) if self.dt == "h" else w

    def outside_unchanged(self):
        """bitwise; call after read()"""
        a, b = _raw(self.now).copy(), _raw(self.full0).copy()
        a[self.sl] = 0
        b[self.sl] = 0
        return np.array_equal(a, b)

    def unchanged(self):
        return np.array_equal(_raw(_to_host(self.t, self.dt)), _raw(self.full0))


class Flat:
    """n dense elements (dt "f", "h" or "b": bytes) with 16 elements of `fill` on either side."""

    def __init__(self, n, dt, data=None, fill=None):
        self.dt, self.n = dt, n
        fill = {"f": SENT, "h": SENT_H, "b": SENT_B}[dt] if fill is None else fill
        self.full0 = np.full(n + 32, fill, NPT[dt])
        if data is not None:
            d = np.asarray(data).ravel()
            self.full0[16:16 + n] = h_bits(d) if dt == "h" else d
        self.t = _to_dev(self.full0, dt)

    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 16 * ESIZE[self.dt])

    def read(self):
        self.now = _to_host(self.t, self.dt)
        w = self.now[16:16 + self.n].copy()
        return h_wide(w) if self.dt == "h" else w

    def outside_unchanged(self):
        return (np.array_equal(_raw(self.now[:16]), _raw(self.full0[:16])) and
                np.array_equal(_raw(self.now[-16:]), _raw(self.full0[-16:])))

    def unchanged(self):
        return np.array_equal(_raw(_to_host(self.t, self.dt)), _raw(self.full0))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def same(got, want, what):
    """np.array_equal on float32 (like the fp32 file: the sign of zero is not compared), with a useful message"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d of %d wrong, first at %s: got %r, want %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0])


def _film_rows(o, cout):
    """FiLM rows at their own pitch, NaN between them"""
    ld = cout + 12
    d = {}
    for n in ("fmul", "fadd"):
        a = getattr(o, n)
        if a is not None:
            full = np.full((a.shape[0], ld), NANF, np.float32)
            full[:, :cout] = a
            a = full
        d[n] = dev(a)
    return d, ld


# ---------------------------------------------------------------------------------------------------------------------
# depgan_op_conv2d_bf16s, depgan_op_conv2d_head_bf16s, depgan_op_conv2d_film_train_bf16s
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_ref(case):
    """computed once per case and shared (read only)"""
    o, pool, head = bc.conv_ops(case, "exact")
    return o, fr.reference_bf16s(o)


def conv_windows(o, case, pool, head, train):
    feat, shape, view = case
    B, H, W, ci, co, k = shape
    w = {"in": Win((1 if view == "in_sB0" else B, H, W, ci), 16, 8, "h", NAN_H, o.x[:1] if view == "in_sB0" else o.x),
         "out": Win((B, H, W, co), 24, 8, "h", SENT_H)}
    if o.res is not None:
        w["res"] = Win((1 if view == "res_sB0" else B, H, W, co), 40, 16, "h", NAN_H, o.res[:1] if view == "res_sB0" else o.res)
    if pool:
        w["pool"] = Flat(B * (H // 2) * (W // 2) * co, "h")
    if head:
        w["head"] = Flat(B * H * W, "f")
    if train:
        w["u"] = Flat(B * H * W * co, "h")
        w["dec"] = Flat(B * H * W * co // 8, "b")
    return w


def call_conv(lib, o, case, w, entry, d, ld, out="out", skip=0):
    """entry "conv", "head" or "train" on the windows w"""
    feat, shape, view = case
    B, H, W, ci, co, k = shape
    ia = w["in"].args(sB=0 if view == "in_sB0" else None)
    ra = (w["res"].args(sB=0 if view == "res_sB0" else None) if "res" in w else NONE)
    common = (*ia, P(d["w"]), P(d["bias"]), P(d["scale"]), P(d["shift"]), P(d["fmul"]), P(d["fadd"]), ld, *ra, *w[out].args())
    if entry == "train":
        rc = lib.depgan_op_conv2d_film_train_bf16s(*common, w["u"].ptr(), w["dec"].ptr(), B, H, W, ci, co, o.relu, None)
    else:
        tail = (w["pool"].ptr() if "pool" in w else None, B, H, W, ci, co, k, o.relu)
        if entry == "head":
            rc = lib.depgan_op_conv2d_head_bf16s(*common, *tail, P(d["head_w"]), P(d["head_b"]), w["head"].ptr(),
                                                 o.head_tanh, skip, None)
        else:
            rc = lib.depgan_op_conv2d_bf16s(*common, *tail, None)
    torch.cuda.synchronize()
    return rc


def run_conv(lib, case, kind, entry):
    from dep_gan_im_amd import _lib
    if kind == "exact":
        o, ref = _exact_ref(case)
        pool, head = bc.FEATS[case[0]].get("pool", 0), bc.FEATS[case[0]].get("head", 0)
    else:
        (o, pool, head), ref = bc.conv_ops(case, kind), None
    co = case[1][4]
    w = conv_windows(o, case, pool, head, entry == "train")
    d = {n: dev(getattr(o, n)) for n in ("w", "bias", "scale", "shift", "head_w", "head_b")}
    f, ld = _film_rows(o, co)
    d.update(f)
    _lib.check(call_conv(lib, o, case, w, entry, d, ld, skip=int(head == 2)), "depgan_op_conv2d_*_bf16s " + entry)
    return o, ref, w, d, ld, pool, head


def head_of_stored(lib, stored, o, tanh_act):
    """depgan_op_head_bf16s on a dense copy of the stored (bf16-valued) output: the header's contract for head_out"""
    from dep_gan_im_amd import _lib
    a = Flat(stored.size, "h", stored, fill=NAN_H)
    out = Flat(stored.size // 32, "f")
    hw, hb = dev(o.head_w), dev(o.head_b)
    _lib.check(lib.depgan_op_head_bf16s(a.ptr(), P(hw), P(hb), out.ptr(), stored.size // 32, 32, tanh_act, None))
    torch.cuda.synchronize()
    return out.read()


def check_common(w, o, case, stored, pool, head):
    """What every conv test states besides the value of `out`: the pool of the stored values, nothing written outside,
    read-only operands untouched."""
    if head == 2:
        assert w["out"].unchanged()                    # skip_out: the 32-channel output is not stored
    else:
        assert w["out"].outside_unchanged()
    if pool:
        same(w["pool"].read().reshape(fr.pool2(stored).shape), fr.pool2(stored), "pool")
        assert w["pool"].outside_unchanged()
    for n in ("in", "res"):
        if n in w:
            assert w[n].unchanged(), n


_cid = bc.cid


@pytest.mark.parametrize("case", bc.CONV_CASES + bc.HEAD_CASES, ids=_cid)
def test_conv_exact_operands_store_the_one_correct_pattern(lib, case):
    entry = "head" if "head" in case[0] else "conv"
    o, ref, w, d, ld, pool, head = run_conv(lib, case, "exact", entry)
    if head != 2:
        same(w["out"].read(), ref["out"], "out")
    check_common(w, o, case, ref["out"], pool, head)
    if "neg" in bc.FEATS[case[0]]:
        assert ref["pool"].max() < 0
    if case[2]:                                        # one sample read for every batch index: the outputs still differ
        assert not np.array_equal(ref["out"][0], ref["out"][1])
    if head:
        got = w["head"].read()
        same(got.reshape(ref["head"].shape), ref["head"], "head_out")                    # identity activation
        assert w["head"].outside_unchanged()
        assert np.array_equal(got.view(np.uint32), head_of_stored(lib, ref["out"], o, 0).view(np.uint32))


@pytest.mark.parametrize("case", bc.CONV_CASES + bc.HEAD_CASES, ids=_cid)
def test_conv_real_operands_equal_the_rounded_fp32_storage_sibling(lib, case):
    """out == RNE_bf16(depgan_op_conv2d_fused(path 3) on the widened operands), every feature set; the tanh head equals
    depgan_op_head_bf16s of the stored output bit for bit (the header's contract), with skip_out of RNE(sibling out)."""
    entry = "head" if "head" in case[0] else "conv"
    o, _, w, d, ld, pool, head = run_conv(lib, case, "real", entry)
    sib_out, _ = sibling_conv(lib, o, case, d, ld)
    stored = fr.rne_bf16(sib_out)
    if head != 2:
        same(w["out"].read(), stored, "out vs RNE(sibling)")
    check_common(w, o, case, stored, pool, head)
    if head:
        got = w["head"].read()
        assert w["head"].outside_unchanged()
        assert np.array_equal(got.view(np.uint32), head_of_stored(lib, stored, o, 1).view(np.uint32))
        assert np.abs(got).max() <= 1.0 and np.abs(got).max() > 0.1                     # tanh was applied


def sibling_conv(lib, o, case, d, ld):
    """depgan_op_conv2d_fused(path = 3) on the same operands widened to fp32 (exact): (out, out_pre)."""
    from dep_gan_im_amd import _lib
    feat, shape, view = case
    B, H, W, ci, co, k = shape
    s = {"in": Win((B, H, W, ci), 12, 4, "f", NANF, o.x), "out": Win((B, H, W, co), 20, 8, "f", SENT),
         "pre": Win((B, H, W, co), 28, 12, "f", SENT)}
    if o.res is not None:
        s["res"] = Win((B, H, W, co), 36, 16, "f", NANF, o.res)
    _lib.check(lib.depgan_op_conv2d_fused(
        *s["in"].args(), P(d["w"]), P(d["bias"]), P(d["scale"]), P(d["shift"]), P(d["fmul"]), P(d["fadd"]), ld,
        *s["out"].args(), *s["pre"].args(), *(s["res"].args() if "res" in s else NONE), *NONE, *NONE, None, None, None,
        0, 0, B, H, W, ci, co, k, o.relu, 0, 3, 0, None), "op_conv2d_fused")
    torch.cuda.synchronize()
    return s["out"].read(), s["pre"].read()


def _train_case(shape):
    return ("film", shape + (3,), "train")


def _check_train(lib, case, o, w, d, ld, stored, u, dec_bits):
    same(w["out"].read(), stored, "out")
    same(w["u"].read().reshape(u.shape), u, "u_out")
    got = w["dec"].read()
    bad = got != dec_bits
    assert not bad.any(), "dec_bits: %d of %d bytes wrong, first byte %d: got %#x, want %#x" % (
        bad.sum(), bad.size, np.argwhere(bad)[0, 0], got[bad][0], dec_bits[bad][0])
    for n in ("u", "dec"):
        assert w[n].outside_unchanged(), n
    check_common(w, o, case, stored, 0, 0)
    # `out` has the bits of depgan_op_conv2d_bf16s on the same windows
    w["out2"] = Win(stored.shape, 24, 8, "h", SENT_H)
    assert call_conv(lib, o, case, w, "conv", d, ld, out="out2") == 0
    assert np.array_equal(_to_host(w["out2"].t, "h"), _to_host(w["out"].t, "h"))


@pytest.mark.parametrize("shape", bc.TRAIN_CASES, ids=_cid)
def test_film_train_exact_operands_u_and_decision_bytes(lib, shape):
    case = _train_case(shape)
    o, ref, w, d, ld, _, _ = run_conv(lib, case, "exact", "train")
    z = fr.ZERO_FILM_CHANNEL
    assert not ref["dec"][..., z].any() and ref["dec"].any()            # the forced zero channel decides 0
    _check_train(lib, case, o, w, d, ld, ref["out"], ref["u"], ref["dec_bits"])


@pytest.mark.parametrize("shape", bc.TRAIN_CASES, ids=_cid)
def test_film_train_real_operands_equal_the_sibling(lib, shape):
    """u_out == RNE(sibling out_pre); dec == (float32 FiLM of the sibling's out_pre > 0): one multiply, then one add,
    every element; out == RNE(sibling out)."""
    case = _train_case(shape)
    o, _, w, d, ld, _, _ = run_conv(lib, case, "real", "train")
    sib_out, sib_pre = sibling_conv(lib, o, case, d, ld)
    v = (sib_pre * o.fmul[:, None, None, :]).astype(np.float32)
    v = (v + o.fadd[:, None, None, :]).astype(np.float32)
    _check_train(lib, case, o, w, d, ld, fr.rne_bf16(sib_out), fr.rne_bf16(sib_pre), fr.pack_dec(v > 0))


# ---------------------------------------------------------------------------------------------------------------------
# depgan_op_deconv2x2_bf16s: the output is a channel window of a (2H, 2W) concat-style buffer with padded rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("case", bc.DECONV_CASES, ids=_cid)
def test_deconv2x2(lib, case, kind):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = case
    x, wt, o = bc.deconv_ops(case, kind)
    win = Win((B, H, W, ci), 16, 8, "h", NAN_H, x)
    wout = Win((B, 2 * H, 2 * W, co), 24, 8, "h", SENT_H)
    d = [dev(a) for a in (wt, o.bias, o.scale, o.shift)]
    _lib.check(lib.depgan_op_deconv2x2_bf16s(*win.args(), *map(P, d), *wout.args(), B, H, W, ci, co, 1, None))
    torch.cuda.synchronize()
    if kind == "exact":
        want = fr.rne_bf16(np.maximum(fr.affine(fr.deconv2x2(x, wt), o, np.float64), 0).astype(np.float32))
    else:
        sin = Win((B, H, W, ci), 12, 4, "f", NANF, x)
        sout = Win((B, 2 * H, 2 * W, co), 20, 8, "f", SENT)
        _lib.check(lib.depgan_op_deconv2x2_igemm(0, *sin.args(), *map(P, d), *sout.args(), *NONE, B, H, W, ci, co, 1, 3, None))
        torch.cuda.synchronize()
        want = fr.rne_bf16(sout.read())
    same(wout.read(), want, "deconv out")
    assert wout.outside_unchanged() and win.unchanged()


# ---------------------------------------------------------------------------------------------------------------------
# depgan_op_edge_conv_bf16s: Cin in {1, 2} x Cout in {8, 16, 24, 32}; dense fp32 input, the output is a window
# ---------------------------------------------------------------------------------------------------------------------
def _run_edge(lib, case, kind):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = case
    x, wgt, o = bc.edge_ops(case, kind)
    xin = Flat(x.size, "f", x, fill=NANF)
    wout = Win((B, H, W, co), 24, 8, "h", SENT_H)
    # bias, scale and shift are read as rows of 8 floats: exactly Cout of them, NaN behind
    d = [Flat(a.size, "f", a, fill=NANF) for a in (wgt, o.bias, o.scale, o.shift)]
    _lib.check(lib.depgan_op_edge_conv_bf16s(xin.ptr(), *[f.ptr() for f in d], *wout.args(), B, H, W, ci, co, 1, None))
    torch.cuda.synchronize()
    got = wout.read()
    assert wout.outside_unchanged() and xin.unchanged()
    return x, wgt, o, got


@pytest.mark.parametrize("case", bc.EDGE_CASES, ids=_cid)
def test_edge_conv_exact_operands(lib, case):
    x, wgt, o, got = _run_edge(lib, case, "exact")
    same(got, fr.rne_bf16(np.maximum(fr.affine(fr.conv_acc(x, wgt), o, np.float64), 0).astype(np.float32)), "edge out")


@pytest.mark.parametrize("case", bc.EDGE_CASES, ids=_cid)
def test_edge_conv_real_operands_within_the_storage_bound(lib, case):
    """No fp32-storage kernel shares this kernel's text: the bound of tests/test_gpu_bf16_store.py, TOL and S unchanged."""
    from test_gpu_bf16_store import _within_bound
    x, wgt, o, got = _run_edge(lib, case, "real")
    ref = np.maximum(fr.affine(fr.conv_acc(x, wgt), o, np.float64), 0)
    _within_bound(got, ref, float(np.abs(ref).max()), "edge conv %s" % (case,))


# ---------------------------------------------------------------------------------------------------------------------
# depgan_op_conv2d_bwd_data_bf16s: fp32 dy, res and dx next to a bf16 mask, four windows with four pitches
# ---------------------------------------------------------------------------------------------------------------------
def _join32(g, res, mask):
    """the kernel's epilogue on a given contraction, one float32 operation per step: + res, then the mask's selection"""
    v = g.astype(np.float32)
    if res is not None:
        v = (v + res).astype(np.float32)
    return np.where(mask > 0, v, np.float32(0)) if mask is not None else v


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("case", bc.BWD_CASES, ids=_cid)
def test_bwd_data_3x3(lib, case, kind):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co, res, mask = case
    o = bc.bwd_ops(case, kind)
    w = {"dy": Win((B, H, W, co), 12, 4, "f", NANF, o.x), "dx": Win((B, H, W, ci), 20, 8, "f", SENT)}
    if res:
        w["res"] = Win((B, H, W, ci), 36, 16, "f", NANF, o.res)
    if mask:
        w["mask"] = Win((B, H, W, ci), 16, 8, "h", NAN_H, o.mask)
    wd = dev(o.w)
    _lib.check(lib.depgan_op_conv2d_bwd_data_bf16s(
        *w["dy"].args(), P(wd), *(w["res"].args() if res else NONE), *(w["mask"].args() if mask else NONE),
        *w["dx"].args(), B, H, W, ci, co, 0, None))
    torch.cuda.synchronize()
    if kind == "exact":
        want = fr.reference(o)["out"]
    else:
        dyd, g = dev(o.x), torch.full((B, H, W, ci), float("nan"), device="cuda:0")
        _lib.check(lib.depgan_op_conv2d_bwd_data(P(dyd), P(wd), P(g), B, H, W, ci, co, 3, 3, None))
        torch.cuda.synchronize()
        want = _join32(g.cpu().numpy(), o.res, o.mask)
    same(w["dx"].read(), want, "dx")
    assert w["dx"].outside_unchanged()
    assert all(w[n].unchanged() for n in w if n != "dx")


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("case", bc.BWD_DECONV_CASES, ids=_cid)
def test_bwd_data_of_the_transposed_convolution(lib, case, kind):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co, res, mask = case
    dy, wt, r, m = bc.bwd_deconv_ops(case, kind)
    w = {"dy": Win((B, 2 * H, 2 * W, co), 12, 4, "f", NANF, dy), "dx": Win((B, H, W, ci), 20, 8, "f", SENT)}
    if res:
        w["res"] = Win((B, H, W, ci), 36, 16, "f", NANF, r)
    if mask:
        w["mask"] = Win((B, H, W, ci), 16, 8, "h", NAN_H, m)
    wd = dev(wt)
    _lib.check(lib.depgan_op_conv2d_bwd_data_bf16s(
        *w["dy"].args(), P(wd), *(w["res"].args() if res else NONE), *(w["mask"].args() if mask else NONE),
        *w["dx"].args(), B, H, W, ci, co, 1, None))
    torch.cuda.synchronize()
    if kind == "exact":
        g = fr.deconv2x2_bwd_data(dy, wt)
        want = np.where(m > 0, g + r, 0.0) if mask else g
    else:
        sdy = Win((B, 2 * H, 2 * W, co), 28, 12, "f", NANF, dy)
        sdx = Win((B, H, W, ci), 44, 20, "f", SENT)
        _lib.check(lib.depgan_op_deconv2x2_igemm(1, *sdy.args(), P(wd), None, None, None, *sdx.args(), *NONE,
                                                 B, H, W, ci, co, 0, 3, None))
        torch.cuda.synchronize()
        want = _join32(sdx.read(), r, m)
    same(w["dx"].read(), want, "dx")
    assert w["dx"].outside_unchanged()
    assert all(w[n].unchanged() for n in w if n != "dx")


# ---------------------------------------------------------------------------------------------------------------------
# depgan_op_conv2d_wgrad_bf16s: x a bf16 window, dy an fp32 window or the strided grid of a (2H, 2W) buffer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("case", bc.WGRAD_CASES, ids=_cid)
def test_wgrad(lib, case, kind):
    """exact: the integers of the float64 reference.  real: dw bit-equal to depgan_op_conv2d_wgrad_bf16 on the widened
    dense copies (same K order); colsum sums the UNROUNDED dy in an order of its own: float64 at TOL."""
    from dep_gan_im_amd import _lib
    B, H, W, ci, co, k, oi, grid, colsum = case
    x, dyf, dy = bc.wgrad_ops(case, kind)
    lay = (lambda a: np.ascontiguousarray(a.transpose(0, 1, 3, 2))) if oi else (lambda a: a)
    outs = []
    for rep in range(2):
        wx = Win((B, H, W, ci), 16, 8, "h", NAN_H, x)
        wdy = Win(dyf.shape, 20, 8, "f", NANF, dyf)
        dyargs = wdy.args(grid[0] * wdy.strides[1] + grid[1] * wdy.strides[2], (1, 2, 2)) if grid else wdy.args()
        fdw = Flat(k * k * ci * co, "f")
        fcol = Flat(co, "f") if colsum else None
        _lib.check(lib.depgan_op_conv2d_wgrad_bf16s(*wx.args(), *dyargs, fdw.ptr(), fcol.ptr() if colsum else None,
                                                    B, H, W, ci, co, k, oi, None))
        torch.cuda.synchronize()
        outs.append((fdw.read(), fcol.read() if colsum else None))
        assert fdw.outside_unchanged() and (not colsum or fcol.outside_unchanged())
        assert wx.unchanged() and wdy.unchanged()
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))            # two runs, the same bits
    assert not colsum or np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
    col64 = dy.astype(np.float64).sum(axis=(0, 1, 2))
    if kind == "exact":
        same(outs[0][0], lay(fr.wgrad(x, dy, k)).ravel(), "dw")
        if colsum:
            same(outs[0][1], col64, "colsum")
    else:
        xd, dyd = dev(x), dev(dy)
        g = torch.full((k, k, ci, co), float("nan"), device="cuda:0")
        _lib.check(lib.depgan_op_conv2d_wgrad_bf16(P(xd), P(dyd), P(g), B, H, W, ci, co, k, None))
        torch.cuda.synchronize()
        same(outs[0][0], lay(g.cpu().numpy()).ravel(), "dw vs depgan_op_conv2d_wgrad_bf16")
        if colsum:
            e = float(np.abs(outs[0][1] - col64).max() / np.abs(col64).max())
            print("colsum rel err %.3g" % e)
            assert e < TOL


# ---------------------------------------------------------------------------------------------------------------------
# depgan_op_unpool_mask_bf16s: four windows; small integers with equal maxima in most windows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.UNPOOL_CASES, ids=_cid)
def test_unpool_mask_first_maximum(lib, case):
    from dep_gan_im_amd import _lib
    B, Ho, Wo, Cc, skip = case
    dpool, a, sk = bc.unpool_ops(case)
    ref = fr.unpool_mask(dpool, a, sk)
    assert (ref != fr.unpool_mask(dpool, a, sk, last=True)).sum() > ref.size // 20       # the ties are there
    w = {"d": Win((B, Ho, Wo, Cc), 12, 4, "f", NANF, dpool), "a": Win((B, 2 * Ho, 2 * Wo, Cc), 16, 8, "h", NAN_H, a),
         "out": Win((B, 2 * Ho, 2 * Wo, Cc), 20, 8, "f", SENT)}
    if skip:
        w["skip"] = Win((B, 2 * Ho, 2 * Wo, Cc), 36, 16, "f", NANF, sk)
    _lib.check(lib.depgan_op_unpool_mask_bf16s(*w["d"].args(), *w["a"].args(), *(w["skip"].args() if skip else NONE),
                                               *w["out"].args(), B, Ho, Wo, Cc, None))
    torch.cuda.synchronize()
    same(w["out"].read(), ref, "unpool out")
    assert w["out"].outside_unchanged()
    assert all(w[n].unchanged() for n in w if n != "out")


# ---------------------------------------------------------------------------------------------------------------------
# refusals: a non-zero status, a message, every window bitwise unchanged.  Each of these checks is made by the entry or
# its launcher in front of any allocation, pack or launch (op_entries_bf16s.hip: dg_conv_bf16s_check before the packing;
# depgan_op_conv2d_bwd_data_bf16s refuses the gathered form before it allocates): no kernel runs on a view it was not
# written for.
# ---------------------------------------------------------------------------------------------------------------------
REFUSE_SHAPE = (2, 22, 18, 8, 32, 3)


def _refusal_call(lib, shape, feat="film", entry="conv", in_off=0, out_dY=0, drop_fadd=False, pool=False):
    B, H, W, ci, co, k = shape
    rng = np.random.default_rng(3)
    o = fr.make_ops_bf16s("exact", rng, B, H, W, ci, co, k, head=(entry == "head"), **bc.FEATS[feat])
    w = {"in": Win((B, H, W, ci), 24 - ci % 8, 8, "h", NAN_H, o.x), "out": Win((B, H, W, co), 24, 8, "h", SENT_H),
         "res": Win((B, H, W, co), 40, 16, "h", NAN_H, o.res)}
    if pool:
        w["pool"] = Flat(B * (H // 2) * (W // 2) * co, "h")
    if entry == "head":
        w["head"] = Flat(B * H * W, "f")
    d = {n: dev(getattr(o, n)) for n in ("w", "bias", "scale", "shift", "head_w", "head_b")}
    f, ld = _film_rows(o, co)
    common = (*w["in"].args(off=in_off), P(d["w"]), P(d["bias"]), P(d["scale"]), P(d["shift"]), P(f["fmul"]),
              None if drop_fadd else P(f["fadd"]), ld, *w["res"].args(), *w["out"].args(dY=out_dY),
              w["pool"].ptr() if pool else None, B, H, W, ci, co, k, 1)
    if entry == "head":
        rc = lib.depgan_op_conv2d_head_bf16s(*common, P(d["head_w"]), P(d["head_b"]), w["head"].ptr(), 0, 0, None)
    else:
        rc = lib.depgan_op_conv2d_bf16s(*common, None)
    torch.cuda.synchronize()
    return rc, w


def _refuse_pointer_8_bytes_off(lib):
    return _refusal_call(lib, REFUSE_SHAPE, in_off=4) + (None,)            # 4 bf16 elements


def _refuse_row_stride_not_multiple_of_8(lib):
    return _refusal_call(lib, REFUSE_SHAPE, out_dY=4) + (None,)


def _refuse_pool_odd_h(lib):
    return _refusal_call(lib, (2, 21, 18, 8, 32, 3), pool=True) + (None,)


def _refuse_head_cout_64(lib):
    return _refusal_call(lib, (2, 22, 18, 8, 64, 3), entry="head") + (3,)


def _refuse_ks_5(lib):
    return _refusal_call(lib, (2, 22, 18, 8, 32, 5)) + (1,)


def _refuse_cin_12(lib):
    return _refusal_call(lib, (2, 22, 18, 12, 32, 3)) + (3,)


def _refuse_film_mul_without_add(lib):
    return _refusal_call(lib, REFUSE_SHAPE, drop_fadd=True) + (None,)


def _refuse_gathered_cout_not_multiple_of_32(lib):
    B, H, W, ci, co = 2, 6, 10, 64, 48
    rng = np.random.default_rng(4)
    w = {"dy": Win((B, 2 * H, 2 * W, co), 12, 4, "f", NANF, rng.integers(-2, 3, (B, 2 * H, 2 * W, co)).astype(np.float32)),
         "dx": Win((B, H, W, ci), 20, 8, "f", SENT)}
    wd = dev(rng.integers(-1, 2, (2, 2, co, ci)).astype(np.float32))
    rc = lib.depgan_op_conv2d_bwd_data_bf16s(*w["dy"].args(), P(wd), *NONE, *NONE, *w["dx"].args(), B, H, W, ci, co, 1, None)
    torch.cuda.synchronize()
    return rc, w, 3


@pytest.mark.parametrize("name", bc.REFUSALS)
def test_refusals_return_a_status_and_write_nothing(lib, name):
    rc, w, status = globals()["_refuse_" + name](lib)
    assert rc != 0 and lib.depgan_last_error(), name
    assert status is None or rc == status, (name, rc)
    for n, win in w.items():
        assert win.unchanged(), (name, n)
