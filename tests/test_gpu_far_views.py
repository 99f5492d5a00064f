"""GPU, operator level: every strided-view operator on views whose samples lie 2 GiB and more from the view's origin.

The other files check windows of buffers of a few megabytes.  Here ONE operand of a call at a time is a view into a flat
allocation of about 8 GiB with a freely chosen sample stride sB, so that what a kernel computes per sample in 32 bits
(a byte offset next to a buffer descriptor, an `int` product of the batch index and the stride) goes wrong visibly.

Stride classes (E = element size of the view; sB * E is a multiple of 16 bytes in every class):
  straddle  B = 2,  sB * E = 2^31 - half the sample window's extent: sample 1 begins below byte 2^31 of the view and ends
            above it -- range checks of "vector offset + scalar offset" against a 2 GiB descriptor fail for half a sample.
  beyond    B = 3,  sB * E = 2^31 + 256: sample 1 lies wholly past 2 GiB, sample 2 wholly past 4 GiB.  Every sample has its
            own contents, so an offset that wraps modulo 2^32 lands on data that gives another answer.
  many      B = 32, sB * E = 2^28 + 256 (8 GiB in all): the persistent kernels -- more items than resident workgroups, a
            late item's sample past 2 GiB and 4 GiB while the same workgroup's first item was not.

FarWin: sample b of a (B, H, W, C) view is the window (rows from 1, columns from 2, channels from c0) of a padded sample of
(H + 2, W + 3, C + extra) elements, with one padded sample of margin before and after it; only these three padded samples
per batch index are ever filled (from small host arrays, by device slice copies) and read back.  The margins of a
read-only operand hold NaN, those of a written operand the sentinel 0x4B3C2D1E, compared bit for bit afterwards.  The
compact form of the same class (sB = the three padded samples, an allocation of its own) carries the same operands: every
case runs both, and the far result must equal the compact result bit for bit -- a far-addressing failure and an ordinary
kernel bug are told apart by which of the two comparisons fails.

Reference: tests/fused_ref.py on exact operands -- no fp32 operation rounds, the float64 evaluation is the one correct
bit pattern (tests/test_fused_ref_cpu.py, tests/test_bf16s_ref_cpu.py) -> np.array_equal; there is no tolerance in this
file.  Where an operator's result is not exact on any operands (the batch statistics: a division by 3 H W, an rsqrt) the
far result is compared with the compact result bit for bit, which tests/test_gpu_train_ops.py holds against float64.

Operators whose views share ONE stride triple (depgan_op_bn_backward, depgan_op_affine_act) have all their views in the
far allocation at once, interleaved at that stride.  Entries that take dense tensors only (depgan_op_deconv2x2,
depgan_op_conv2d_wgrad_bf16, depgan_op_maxpool) cannot be handed a far view; the bf16 weight gradient is reached through
depgan_op_conv2d_wgrad_ex(bf16 = 1) and depgan_op_conv2d_wgrad_bf16s.  dg_deconv_fwd_supported refuses B * sB > 2^31 - 1
floats by itself: depgan_op_deconv2x2_ex, the same kernel with a strided output, cannot span 2 GiB either -- its views and
that refusal are tests/test_gpu_deconv_tiles.py.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_ref as fr  # noqa: E402
import test_gpu_fused_ops as tfo  # noqa: E402
from test_gpu_fused_ops import NONE, SENT, Flat, P, bits, dev  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GIB = 1 << 30
STORE_BYTES = 8 * GIB + (1 << 26)      # 8.06 GiB: class `many` (32 x (2^28 + 256) bytes) and its margins
NEED_FREE = 10 * GIB
NANF = np.float32("nan")
SENT_H, NAN_H = 0x4B3C, 0x7FC0         # bf16 bit patterns: the sentinel's upper half, a NaN
BATCH = {"straddle": 2, "beyond": 3, "many": 32}
ESZ = {"f": 4, "h": 2}
DG_ERR_UNSUPPORTED = 3


def stride_bytes(cls, extent_bytes):
    if cls == "straddle":
        return ((1 << 31) - extent_bytes // 2) // 16 * 16
    return {"beyond": (1 << 31) + 256, "many": (1 << 28) + 256}[cls]


@pytest.fixture(scope="module")
def store():
    """The one far allocation of the module: {"f": float32 view, "h": the same memory as 2-byte elements}."""
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_FREE:
        pytest.skip("far views need 10 GiB of free device memory, %.1f GiB are free" % (free / GIB))
    assert STORE_BYTES < 9 * GIB
    flat = torch.empty(STORE_BYTES // 4, dtype=torch.float32, device=DEV)
    h = {"f": flat, "h": flat.view(torch.int16)}
    del flat
    yield h
    h.clear()
    torch.cuda.empty_cache()


def h_bits(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def h_wide(u16):
    return (np.ascontiguousarray(u16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _raw(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


class FarWin:
    """A (B, H, W, C) view with sample stride sB in `flat` (a far class in the module's store, or -- flat None -- compact
    in an allocation of its own); dt "f" fp32 or "h" bf16 (as bits).  See the module docstring."""

    def __init__(self, shape, extra, c0, dt="f", ro=True, data=None, flat=None, cls=None, org=0, sB=None):
        B, H, W, Cc = shape
        E, q = ESZ[dt], 16 // ESZ[dt]
        Ct = Cc + extra
        self.dt, self.B, self.ro = dt, B, ro
        self.sY, self.sX = (W + 3) * Ct, Ct
        PS = (H + 2) * self.sY                       # one padded sample
        self.reg = 3 * PS                            # margin, padded sample, margin
        extent = ((H - 1) * self.sY + (W - 1) * self.sX + Cc) * E
        if flat is None:
            self.sB = -(-self.reg // q) * q
            flat = torch.empty((B - 1) * self.sB + self.reg, dtype=torch.int16 if dt == "h" else torch.float32, device=DEV)
            org = 0
        else:
            self.sB = sB if sB is not None else stride_bytes(cls, extent) // E
        self.flat, self.org = flat, org
        assert self.sB % q == 0 and org % q == 0 and self.sB >= self.reg, (self.sB, self.reg)
        assert org + (B - 1) * self.sB + self.reg <= flat.numel(), "the view leaves its allocation"
        fill = ((NAN_H if ro else SENT_H) if dt == "h" else (NANF if ro else SENT))
        self.full0 = np.full((B, 3, H + 2, W + 3, Ct), fill, np.uint16 if dt == "h" else np.float32)
        self.sl = (slice(None), 1, slice(1, 1 + H), slice(2, 2 + W), slice(c0, c0 + Cc))
        if data is not None:
            self.full0[self.sl] = h_bits(data) if dt == "h" else data
        up = torch.from_numpy(self.full0.view(np.int16) if dt == "h" else self.full0).to(DEV).reshape(B, self.reg)
        for b in range(B):
            self._region(b).copy_(up[b])
        self.off = org + PS + self.sY + 2 * self.sX + c0
        assert Ct % q or (self.off % q == 0 and flat.data_ptr() % 16 == 0)

    def _region(self, b):
        s = self.org + b * self.sB
        return self.flat[s:s + self.reg]

    def args(self):
        return (C.c_void_p(self.flat.data_ptr() + ESZ[self.dt] * self.off), self.sB, self.sY, self.sX)

    def _fetch(self):
        a = torch.stack([self._region(b) for b in range(self.B)]).cpu().numpy()
        return (a.view(np.uint16) if self.dt == "h" else a).reshape(self.full0.shape)

    def read(self):
        self.now = self._fetch()
        w = self.now[self.sl].copy()
        return h_wide(w) if self.dt == "h" else w

    def outside_unchanged(self):
        """every margin and every padding row, column and channel, sample by sample, bit for bit; call after read()"""
        a, b = _raw(self.now).copy(), _raw(self.full0).copy()
        a[self.sl] = 0
        b[self.sl] = 0
        return all(np.array_equal(a[i], b[i]) for i in range(self.B))

    def unchanged(self):
        return np.array_equal(_raw(self._fetch()), _raw(self.full0))


def make_views(spec, store, far, cls):
    """spec: {name: (shape, extra, c0, dt, read-only, data)}; the names in `far` become views of class `cls` in the store,
    interleaved at one stride when there are several, the others compact views."""
    w, org = {}, 0
    for n, (shape, extra, c0, dt, ro, data) in spec.items():
        if n in far:
            w[n] = FarWin(shape, extra, c0, dt, ro, data, flat=store[dt], cls=cls, org=org // ESZ[dt])
            org += -(-w[n].reg * ESZ[dt] // 16) * 16
        else:
            w[n] = FarWin(shape, extra, c0, dt, ro, data)
    assert all(n in w for n in far), far
    if len(far) > 1:
        assert org <= min(w[n].sB * ESZ[w[n].dt] for n in far)
    return w


def collect(w, skip=()):
    """the written windows (their surroundings bitwise untouched); the read-only ones bitwise unchanged"""
    got = {}
    for n, v in w.items():
        if isinstance(v, Flat):
            got[n] = v.read()
            assert v.outside_unchanged(), n
        elif n in skip or v.ro:
            assert v.unchanged(), "%s was written" % n
        else:
            got[n] = v.read()
            assert v.outside_unchanged(), "%s: written outside its window" % n
    return got


def same3(far, compact, ref, what):
    """far == compact bit for bit, compact == the float64 reference; the message says which comparison failed"""
    for n in ref:
        f, c = far[n], compact[n]
        r = np.asarray(ref[n]).reshape(c.shape)
        f_c = np.array_equal(bits(f) if f.dtype == np.float32 else f, bits(c) if c.dtype == np.float32 else c)
        c_r, f_r = np.array_equal(c, r), np.array_equal(f, r)
        assert f_c and c_r, "%s %s: far view %s the compact-view run (%d values differ, first at %s), far %s and compact %s the float64 reference" % (
            what, n, "==" if f_c else "!=", int((f != c).sum()), np.argwhere(f != c)[:1].tolist(),
            "==" if f_r else "!=", "==" if c_r else "!=")


# ---------------------------------------------------------------------------------------------------------------------
# convolutions through depgan_op_conv2d_fused
# ---------------------------------------------------------------------------------------------------------------------
OPER = {"in": (12, 4, True), "out": (20, 8, False), "pre": (28, 12, False), "res": (36, 16, True), "mask": (44, 20, True),
        "pool": (52, 24, False)}       # extra, c0, read-only: the pitches of tests/test_gpu_fused_ops.py


@functools.lru_cache(maxsize=2)
def conv_case(feat, shape):
    """operands and the float64 reference of a case, computed once and shared (read only); as float32, which holds every
    exact value"""
    B, H, W, ci, co, k = shape
    f = dict(tfo.FEATS[feat])
    pre, pool, head = f.pop("pre", 0), f.pop("pool", 0), f.pop("head", 0)
    rng = np.random.default_rng(sum(shape) * 131 + len(feat))
    o = fr.make_ops("exact", rng, B, H, W, ci, co, k, head=bool(head), **f)
    r = fr.reference(o)
    assert fr.bounds_hold(r["stages"])
    ref = {"out": r["out"]}
    if pre:
        ref["pre"] = r["out_pre"]
    if pool:
        ref["pool"] = r["pool"]
    if head:
        ref["head"] = r["head"]
    for n in ref:
        assert np.array_equal(ref[n].astype(np.float32).astype(np.float64), ref[n])
        ref[n] = ref[n].astype(np.float32)
    if head == 2:
        del ref["out"]                 # head_skip_out: the 32-channel output is not stored
    return o, ref, pre, pool, head


def run_fused(lib, store, path, feat, shape, far, cls):
    from dep_gan_im_amd import _lib
    o, ref, pre, pool, head = conv_case(feat, shape)
    B, H, W, ci, co, k = shape
    cin, cout = (co, ci) if o.bwd else (ci, co)
    spec = {"in": ((B, H, W, cin), o.x), "out": ((B, H, W, cout), o.old)}
    if pre:
        spec["pre"] = ((B, H, W, cout), None)
    if o.res is not None:
        spec["res"] = ((B, H, W, cout), o.res)
    if o.mask is not None:
        spec["mask"] = ((B, H, W, cout), o.mask)
    if pool:
        spec["pool"] = ((B, H // 2, W // 2, cout), None)
    w = make_views({n: (s, OPER[n][0], OPER[n][1], "f", OPER[n][2], d) for n, (s, d) in spec.items()}, store, far, cls)
    if head:
        w["head"] = Flat(B * H * W)
    d = {n: dev(getattr(o, n)) for n in ("w", "bias", "scale", "shift", "head_w", "head_b")}
    ld = cout + 12                     # FiLM rows at their own pitch, NaN between them
    for n in ("fmul", "fadd"):
        a = getattr(o, n)
        if a is not None:
            full = np.full((B, ld), NANF, np.float32)
            full[:, :cout] = a
            a = full
        d[n] = dev(a)
    arg = lambda n: w[n].args() if n in w else NONE   # noqa: E731
    rc = lib.depgan_op_conv2d_fused(
        *w["in"].args(), P(d["w"]), P(d["bias"]), P(d["scale"]), P(d["shift"]), P(d["fmul"]), P(d["fadd"]), ld,
        *w["out"].args(), *arg("pre"), *arg("res"), *arg("mask"), *arg("pool"), P(d["head_w"]), P(d["head_b"]),
        w["head"].ptr() if head else None, 0, int(head == 2), B, H, W, ci, co, k, o.relu,
        int(o.old is not None), path, o.bwd, None)
    torch.cuda.synchronize()
    _lib.check(rc, "op_conv2d_fused path %d %s" % (path, feat))
    return collect(w, skip=("out",) if head == 2 else ()), ref


_compact = {}


def compact_fused(lib, path, feat, shape):
    """the compact-view run of a case, once for all its far operands"""
    key = (path, feat, shape)
    if key not in _compact:
        _compact.clear()
        _compact[key] = run_fused(lib, None, path, feat, shape, (), None)[0]
    return _compact[key]


def _fused_cases():
    """(path, feature set, (H, W, Cin, Cout, KS) of the layer, far operand, class)"""
    out = []
    epi = [("film_pool", ("in", "out", "pre", "res", "pool")), ("join", ("mask",))]
    for cls in ("straddle", "beyond"):
        # path 8, 8-row tiles: two channel chunks, border and interior tiles
        for feat, fars in [("bias", ("in", "out"))] + [epi[0], ("join", ("in", "out", "mask"))]:
            out += [(8, feat, (24, 48, 16, 32, 3), far, cls) for far in fars]
        # ... with the fused head: the 16-row form
        out += [(8, feat, (48, 48, 16, 32, 3), "in", cls) for feat in ("head", "head_skip")]
        # paths 1 (3x3, 5x5, 1x1), 6, 7, 3 at 20 x 20
        for path, hw in ((1, (8, 32, 3)), (1, (16, 32, 5)), (1, (16, 32, 1)), (6, (8, 32, 3)), (7, (8, 32, 3)), (3, (8, 32, 3))):
            for feat, fars in epi:
                out += [(path, feat, (20, 20) + hw, far, cls) for far in fars]
        # path 2 takes no pool: odd channels 3 -> 5, the FiLM layer's operands and the join's
        out += [(2, "film", (20, 20, 3, 5, 3), far, cls) for far in ("in", "out", "pre", "res")]
        out += [(2, "join", (20, 20, 3, 5, 3), "mask", cls)]
        # paths 9 and 10: the 5x5 weight-stationary and 16-channel bf16 kernels
        for path in (9, 10):
            out += [(path, "bias", (20, 20, 16, 16, 5), far, cls) for far in ("in", "out")]
    # the persistent forms: 1024 items on path 8 (tests/test_gpu_epi_classes.py), PERSIST of tests/test_gpu_fused_ops.py
    for path, hw in ((8, (64, 64, 8, 32, 3)), (1, tfo.PERSIST[1:])):
        out += [(path, "film_pool", hw, far, "many") for far in ("in", "out")]
    return out


def _layer(feat, hw, B):
    """the join runs the layer's backward-data form, Cout -> Cin: the table names the LAUNCH's channels"""
    H, W, ci, co, k = hw
    return (B, H, W, co, ci, k) if tfo.FEATS[feat].get("bwd") else (B, H, W, ci, co, k)


FUSED = _fused_cases()


@pytest.mark.parametrize("case", FUSED, ids=lambda c: "p%d-%s-%s-far_%s-%s" % (c[0], c[1], "x".join(map(str, c[2])), c[3], c[4]))
def test_fused_conv_far_operand(lib, store, case):
    path, feat, hw, far, cls = case
    shape = _layer(feat, hw, BATCH[cls])
    got, ref = run_fused(lib, store, path, feat, shape, (far,), cls)
    same3(got, compact_fused(lib, path, feat, shape), ref, "path %d %s far %s %s" % (path, feat, far, cls))


def test_the_case_table_holds_the_forms():
    have = {(p, f, far, cls) for p, f, _, far, cls in FUSED}
    for cls in ("straddle", "beyond"):
        for far in ("in", "out", "pre", "res", "pool"):
            assert (8, "film_pool", far, cls) in have
        assert (8, "join", "mask", cls) in have and (8, "head", "in", cls) in have and (8, "head_skip", "in", cls) in have
        for p in (1, 6, 7, 3, 2, 9, 10):
            assert any(h[0] == p and h[2] == "in" and h[3] == cls for h in have), p
            assert any(h[0] == p and h[2] == "out" and h[3] == cls for h in have), p
    for p in (8, 1):
        assert any(h[0] == p and h[3] == "many" and h[2] == "in" for h in have)
        assert any(h[0] == p and h[3] == "many" and h[2] == "out" for h in have)
    # the classes are what the docstring says
    ext = 1000 * 16
    assert stride_bytes("straddle", ext) < (1 << 31) < stride_bytes("straddle", ext) + ext
    assert stride_bytes("beyond", ext) > (1 << 31) and 2 * stride_bytes("beyond", ext) > (1 << 32)
    assert 31 * stride_bytes("many", ext) > (1 << 32) + (1 << 31) and 32 * stride_bytes("many", ext) + (1 << 25) < STORE_BYTES
    # 1024 items against 3 x 256 resident workgroups; the path-1 persistent shape is tfo.PERSIST
    assert 32 * (64 // 8) * (64 // 16) * (32 // 32) == 1024 and tfo.PERSIST[0] == BATCH["many"]


@pytest.mark.parametrize("cls", ["straddle", "beyond"])
def test_wino_gathered_far_in(lib, store, cls):
    """two runs of 16 channels at channels 0 and 24 of a 40-channel window: the run offsets point into the wider row"""
    from dep_gan_im_amd import _lib
    B, H, W, cin, co, gap = BATCH[cls], 24, 48, 32, 32, 8
    rng = np.random.default_rng(cin * 7 + 2)
    x = rng.integers(-2, 3, (B, H, W, cin)).astype(np.float32)
    wt = rng.integers(-1, 2, (3, 3, cin, co)).astype(np.float32)
    bias = (rng.integers(-16, 17, co) / 8.0).astype(np.float32)
    row = np.full((B, H, W, cin + gap), NANF, np.float32)
    row[..., :16], row[..., 16 + gap:] = x[..., :16], x[..., 16:]
    run_off = (C.c_long * 4)(0, 16 + gap, 0, 0)
    dw, db = dev(wt), dev(bias)
    ref = {"out": (fr.conv_acc(x, wt) + bias.astype(np.float64)).astype(np.float32)}
    got = {}
    for far in (("in",), ()):
        w = make_views({"in": ((B, H, W, cin + gap), 12, 4, "f", True, row), "out": ((B, H, W, co), 20, 8, "f", False, None)},
                       store, far, cls)
        _lib.check(lib.depgan_op_conv3x3_wino_gathered(*w["in"].args(), run_off, 2, P(dw), P(db), *w["out"].args(),
                                                       B, H, W, cin, co, None), "op_conv3x3_wino_gathered")
        torch.cuda.synchronize()
        got[far] = collect(w)
    same3(got[("in",)], got[()], ref, "gathered K, far in, %s" % cls)


def test_wino_refuses_a_tile_that_32_bit_offsets_cannot_span(lib):
    """What stays in 32 bits is one halo tile plus the channel row: ((TH + 2) sY + 18 sX + Cin + max run_off) * 4 bytes.  A
    row stride that takes it to 2^31 is refused with a status; nothing is written (and nothing read: the rows are not
    there)."""
    x = torch.zeros(4 * 16 * 16, device=DEV)
    wt = torch.zeros(3 * 3 * 16 * 32, device=DEV)
    out = tfo.Win((1, 4, 16, 32), 20, 8, SENT)
    args = lambda sY, sX: (P(x), 4 * sY, sY, sX, P(wt), None, None, None, None, None, 0, *out.args(), *NONE, *NONE,   # noqa: E731
                           *NONE, *NONE, None, None, None, 0, 0, 1, 4, 16, 16, 32, 3, 0, 0, 8, 0, None)
    for sY, sX in ((29826164, 16), (1 << 29, 16), (16 * 16, 29826164), (1 << 40, 16)):
        rc = lib.depgan_op_conv2d_fused(*args(sY, sX))
        torch.cuda.synchronize()
        assert rc == DG_ERR_UNSUPPORTED and lib.depgan_last_error(), (sY, sX, rc)
        assert out.unchanged()
    run_off = (C.c_long * 4)(0, 1 << 29, 0, 0)
    rc = lib.depgan_op_conv3x3_wino_gathered(P(x), 4 * 256, 256, 16, run_off, 2, P(wt), None, *out.args(), 1, 4, 16, 16, 32, None)
    torch.cuda.synchronize()
    assert rc == DG_ERR_UNSUPPORTED and out.unchanged()
    # the layout itself is accepted
    rc = lib.depgan_op_conv2d_fused(*args(16 * 16, 16))
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(out.read(), np.zeros((1, 4, 16, 32), np.float32)) and out.outside_unchanged()


# ---------------------------------------------------------------------------------------------------------------------
# the transposed convolution on the implicit-GEMM kernels
# ---------------------------------------------------------------------------------------------------------------------
DECONV = (8, 8, 96, 96)                # the smallest entry of tfo.DECONV_CASES


@functools.lru_cache(maxsize=None)
def _deconv_case():
    B = BATCH["beyond"]
    H, W, ci, co = DECONV
    x, dy, wt = tfo._deconv_ops("exact", (B, H, W, ci, co), ci + co + H)
    o = fr.make_ops("exact", np.random.default_rng(H), 1, 1, 1, ci, co, 1, bias=1, affine=1, relu=1)
    mask = np.random.default_rng(W).choice(fr.MASKS, (B, H, W, ci)).astype(np.float32)
    fwd = np.maximum(fr.affine(fr.deconv2x2(x, wt), o, np.float64), 0)
    bwd = np.where(mask > 0, fr.deconv2x2_bwd_data(dy, wt), 0.0)
    for a in (fwd, bwd):
        assert np.abs(a).max() < fr.VALUE_BOUND and np.array_equal(a / fr.QUANTUM, np.round(a / fr.QUANTUM))
    return x, dy, wt, o, mask, fwd.astype(np.float32), bwd.astype(np.float32)


@pytest.mark.parametrize("path", [1, 3])
@pytest.mark.parametrize("form,far", [(0, "in"), (0, "out")] + [(f, n) for f in (1, 2) for n in ("in", "out", "mask")])
def test_deconv_igemm_far_operand(lib, store, form, far, path):
    from dep_gan_im_amd import _lib
    B = BATCH["beyond"]
    H, W, ci, co = DECONV
    x, dy, wt, o, mask, fwd, bwd = _deconv_case()
    wd, aff = dev(wt), [dev(a) for a in (o.bias, o.scale, o.shift)]
    got = {}
    for f in ((far,), ()):
        if form == 0:
            w = make_views({"in": ((B, H, W, ci), 12, 4, "f", True, x), "out": ((B, 2 * H, 2 * W, co), 20, 8, "f", False, None)},
                           store, f, "beyond")
            rc = lib.depgan_op_deconv2x2_igemm(0, *w["in"].args(), P(wd), *map(P, aff), *w["out"].args(), *NONE,
                                               B, H, W, ci, co, 1, path, None)
        else:
            w = make_views({"in": ((B, 2 * H, 2 * W, co), 12, 4, "f", True, dy), "out": ((B, H, W, ci), 20, 8, "f", False, None),
                            "mask": ((B, H, W, ci), 44, 20, "f", True, mask)}, store, f, "beyond")
            rc = lib.depgan_op_deconv2x2_igemm(form, *w["in"].args(), P(wd), None, None, None, *w["out"].args(),
                                               *w["mask"].args(), B, H, W, ci, co, 0, path, None)
        torch.cuda.synchronize()
        _lib.check(rc, "op_deconv2x2_igemm form %d" % form)
        got[f] = collect(w)
    same3(got[(far,)], got[()], {"out": fwd if form == 0 else bwd}, "deconv form %d path %d far %s" % (form, path, far))


# ---------------------------------------------------------------------------------------------------------------------
# weight gradients: dg_wgrad's span limit from both sides; the bf16 kernels, which form 64-bit pointers, beyond it
# ---------------------------------------------------------------------------------------------------------------------
WG = (10, 12, 16, 32, 3)               # H, W, Cin, Cout, KS
WG_LIM = 0x7FFFFFFF - (1 << 20)        # dg_wgrad refuses B sB 4 + (sY + sX) 4 KS >= this (x), B sB 4 >= this (dy)


@functools.lru_cache(maxsize=None)
def _wgrad_case(B):
    H, W, ci, co, k = WG
    rng = np.random.default_rng(ci * 100 + co + k + B)
    x = rng.integers(-2, 3, (B, H, W, ci)).astype(np.float32)
    dy = rng.integers(-2, 3, (B, H, W, co)).astype(np.float32)
    scale = rng.choice(fr.SCALES, co).astype(np.float32)
    cscale = rng.choice(fr.SCALES, co).astype(np.float32)
    g = fr.wgrad(x, dy, k)
    col = dy.astype(np.float64).sum(axis=(0, 1, 2))
    ref = {"dw": g * scale.astype(np.float64), "raw": g, "colout": col * cscale.astype(np.float64), "colraw": col}
    for a in ref.values():
        assert np.abs(a).max() < fr.VALUE_BOUND and np.array_equal(a * 8, np.round(a * 8))
    return x, dy, scale, cscale, {n: a.astype(np.float32).ravel() for n, a in ref.items()}


def _wgrad_ex(lib, store, B, far, sB, bf16, cls=None):
    """one depgan_op_conv2d_wgrad_ex call with scale, raw and column sums; `far` ("x", "dy" or None) in the store with
    sample stride sB floats, or of class cls"""
    H, W, ci, co, k = WG
    x, dy, scale, cscale, ref = _wgrad_case(B)
    spec = {"x": ((B, H, W, ci), 12, 4, "f", True, x), "dy": ((B, H, W, co), 20, 8, "f", True, dy)}
    w = {n: (FarWin(*s, flat=store["f"], cls=cls, sB=sB) if n == far else FarWin(*s)) for n, s in spec.items()}
    fl = {"dw": Flat(k * k * ci * co), "raw": Flat(k * k * ci * co), "colout": Flat(co), "colraw": Flat(co)}
    sd, csd = dev(scale), dev(cscale)
    rc = lib.depgan_op_conv2d_wgrad_ex(*w["x"].args(), *w["dy"].args(), P(sd), fl["dw"].ptr(), fl["raw"].ptr(), 0, 0, B, P(csd),
                                       fl["colout"].ptr(), fl["colraw"].ptr(), B, H, W, ci, co, k, bf16, None)
    torch.cuda.synchronize()
    return rc, w, fl, ref


def _wgrad_limit_stride(far, probe):
    """the largest sample stride (a multiple of 4 floats) dg_wgrad accepts for this operand, B = 2"""
    halo = (probe.sY + probe.sX) * 4 * WG[4] if far == "x" else 0
    sB = (WG_LIM - 1 - halo) // 8 // 4 * 4
    assert 2 * sB * 4 + halo < WG_LIM <= 2 * (sB + 4) * 4 + halo and WG_LIM - (2 * sB * 4 + halo) <= 32
    return sB


@pytest.mark.parametrize("far", ["x", "dy"])
def test_wgrad_at_the_largest_accepted_span(lib, store, far):
    from dep_gan_im_amd import _lib
    H, W, ci, co, k = WG
    probe = FarWin((1, H, W, ci if far == "x" else co), 12 if far == "x" else 20, 4, "f")
    rc, w, fl, ref = _wgrad_ex(lib, store, 2, far, _wgrad_limit_stride(far, probe), 0)
    _lib.check(rc, "op_conv2d_wgrad_ex")
    got_far = {n: f.read() for n, f in fl.items()}
    assert all(f.outside_unchanged() for f in fl.values()) and w["x"].unchanged() and w["dy"].unchanged()
    rc, w, fl, _ = _wgrad_ex(lib, store, 2, None, None, 0)
    _lib.check(rc, "op_conv2d_wgrad_ex")
    same3(got_far, {n: f.read() for n, f in fl.items()}, ref, "wgrad, far %s at the limit" % far)


@pytest.mark.parametrize("far", ["x", "dy"])
def test_wgrad_refuses_the_first_span_past_the_limit(lib, store, far):
    H, W, ci, co, k = WG
    probe = FarWin((1, H, W, ci if far == "x" else co), 12 if far == "x" else 20, 4, "f")
    rc, w, fl, _ = _wgrad_ex(lib, store, 2, far, _wgrad_limit_stride(far, probe) + 4, 0)
    assert rc == DG_ERR_UNSUPPORTED
    msg = lib.depgan_last_error()
    assert b"2 GiB" in msg and b"span" in msg, msg
    assert all(f.unchanged() for f in fl.values()), "a refused call wrote dw, raw or the column sums"
    assert w["x"].unchanged() and w["dy"].unchanged()


@pytest.mark.parametrize("far", ["x", "dy"])
def test_wgrad_bf16_beyond(lib, store, far):
    """wgrad_bf16_kernel.inc forms 64-bit pointers and has no span limit: depgan_op_conv2d_wgrad_ex(bf16 = 1)"""
    from dep_gan_im_amd import _lib
    B = BATCH["beyond"]
    rc, w, fl, ref = _wgrad_ex(lib, store, B, far, None, 1, cls="beyond")
    _lib.check(rc, "op_conv2d_wgrad_ex bf16")
    got_far = {n: f.read() for n, f in fl.items()}
    assert all(f.outside_unchanged() for f in fl.values()) and w["x"].unchanged() and w["dy"].unchanged()
    rc, w, fl, _ = _wgrad_ex(lib, store, B, None, None, 1)
    _lib.check(rc, "op_conv2d_wgrad_ex bf16")
    same3(got_far, {n: f.read() for n, f in fl.items()}, ref, "bf16 wgrad, far %s" % far)


@pytest.mark.parametrize("far", ["x", "dy"])
def test_wgrad_bf16s_beyond(lib, store, far):
    """depgan_op_conv2d_wgrad_bf16s: x a bf16 view, dy an fp32 view"""
    from dep_gan_im_amd import _lib
    B = BATCH["beyond"]
    H, W, ci, co, k = WG
    x, dy, _, _, ref = _wgrad_case(B)
    got = {}
    for f in ((far,), ()):
        w = make_views({"x": ((B, H, W, ci), 16, 8, "h", True, x), "dy": ((B, H, W, co), 20, 8, "f", True, dy)}, store, f, "beyond")
        fl = {"raw": Flat(k * k * ci * co), "colraw": Flat(co)}
        _lib.check(lib.depgan_op_conv2d_wgrad_bf16s(*w["x"].args(), *w["dy"].args(), fl["raw"].ptr(), fl["colraw"].ptr(),
                                                    B, H, W, ci, co, k, 0, None), "op_conv2d_wgrad_bf16s")
        torch.cuda.synchronize()
        got[f] = {n: v.read() for n, v in fl.items()}
        assert all(v.outside_unchanged() for v in fl.values()) and w["x"].unchanged() and w["dy"].unchanged()
    same3(got[(far,)], got[()], {n: ref[n] for n in ("raw", "colraw")}, "bf16s wgrad, far %s" % far)


# ---------------------------------------------------------------------------------------------------------------------
# view operators
# ---------------------------------------------------------------------------------------------------------------------
VB = BATCH["beyond"]


def _ints(rng, shape, lo=-2, hi=2):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def test_exact_sums_are_exact_in_float32_on_the_cpu():
    """what the column sums and moments tests rely on: integer operands keep every fp32 partial sum exact, in any order"""
    rng = np.random.default_rng(5)
    x = _ints(rng, (VB, 8, 8, 32), 0, 3)
    s64 = x.reshape(-1, 32).astype(np.float64).sum(0)
    for order in (np.arange(VB * 64), rng.permutation(VB * 64)):
        acc = np.zeros(32, np.float32)
        for p in order:
            acc = (acc + x.reshape(-1, 32)[p]).astype(np.float32)
        assert np.array_equal(acc.astype(np.float64), s64)
    assert s64.max() < 2 ** 24
    # the mean is not: 3 H W is no power of two -- the moments are compared far against compact
    assert not np.array_equal((s64.astype(np.float32) / np.float32(VB * 64)).astype(np.float64), s64 / (VB * 64))


def test_colsum_far(lib, store):
    from dep_gan_im_amd import _lib
    B, H, W, Cc = VB, 8, 8, 32
    rng = np.random.default_rng(B * H * W + Cc)
    x = _ints(rng, (B, H, W, Cc), 0, 3)
    scale = rng.choice(fr.SCALES, Cc).astype(np.float32)
    tot = x.reshape(-1, Cc).astype(np.float64).sum(0)
    ref = {"raw": tot.astype(np.float32), "out": (tot * scale).astype(np.float32)}
    assert np.array_equal(ref["out"].astype(np.float64), tot * scale)
    sd = dev(scale)
    got = {}
    for f in (("v",), ()):
        w = make_views({"v": ((B, H, W, Cc), 12, 4, "f", True, x)}, store, f, "beyond")
        fl = {"out": Flat(Cc), "raw": Flat(Cc)}
        _lib.check(lib.depgan_op_colsum(*w["v"].args(), B, H, W, Cc, P(sd), fl["out"].ptr(), fl["raw"].ptr(), 0, None, 0, None), "colsum")
        torch.cuda.synchronize()
        got[f] = {n: v.read() for n, v in fl.items()}
        assert all(v.outside_unchanged() for v in fl.values()) and w["v"].unchanged()
    same3(got[("v",)], got[()], ref, "colsum")


def test_bn_moments_far(lib, store):
    from dep_gan_im_amd import _lib
    B, H, W, Cc = VB, 8, 8, 32
    x = _ints(np.random.default_rng(3), (B, H, W, Cc)) * np.arange(1, B + 1, dtype=np.float32)[:, None, None, None]
    got = {}
    for f in (("x",), ()):
        w = make_views({"x": ((B, H, W, Cc), 12, 4, "f", True, x)}, store, f, "beyond")
        fl = {"mean": Flat(Cc), "var": Flat(Cc)}
        _lib.check(lib.depgan_op_bn_moments(*w["x"].args(), B, H, W, Cc, fl["mean"].ptr(), fl["var"].ptr(), 0, None), "bn_moments")
        torch.cuda.synchronize()
        got[f] = {n: v.read() for n, v in fl.items()}
        assert all(v.outside_unchanged() for v in fl.values()) and w["x"].unchanged()
    for n in ("mean", "var"):
        assert np.isfinite(got[()][n]).all()
        assert np.array_equal(bits(got[("x",)][n]), bits(got[()][n])), "%s: far != compact" % n
    assert (got[()]["var"] > 0).all()   # the samples differ: a sample read twice or not at all changes the variance


def test_bn_backward_far(lib, store):
    """dy, raw and draw share one stride triple: all three are far, interleaved"""
    from dep_gan_im_amd import _lib
    B, H, W, Cc = VB, 8, 8, 32
    rng = np.random.default_rng(11)
    x, dy = _ints(rng, (B, H, W, Cc), -4, 4), _ints(rng, (B, H, W, Cc))
    xd = x.reshape(-1, Cc).astype(np.float64)
    g = [dev(a.astype(np.float32)) for a in (0.5 + rng.random(Cc), xd.mean(0), xd.var(0))]
    got = {}
    for f in (("dy", "raw", "draw"), ()):
        w = make_views({n: ((B, H, W, Cc), 12, 4, "f", n != "draw", d) for n, d in (("dy", dy), ("raw", x), ("draw", None))},
                       store, f, "beyond")
        assert len({v.args()[1:] for v in w.values()}) == 1
        fl = {"dgamma": Flat(Cc), "dbeta": Flat(Cc)}
        _lib.check(lib.depgan_op_bn_backward(w["dy"].args()[0], w["raw"].args()[0], *w["draw"].args(), B, H, W, Cc, *map(P, g),
                                             1e-3, 1.0 / (B * H * W), 1.0, fl["dgamma"].ptr(), fl["dbeta"].ptr(), 0, None), "bn_backward")
        torch.cuda.synchronize()
        got[f] = collect({**w, **fl})
    for n in ("draw", "dgamma", "dbeta"):
        assert np.isfinite(got[()][n]).all()
        assert np.array_equal(bits(got[("dy", "raw", "draw")][n]), bits(got[()][n])), "%s: far != compact" % n
    assert np.array_equal(got[()]["dbeta"], dy.reshape(-1, Cc).astype(np.float64).sum(0))      # an exact sum


def test_affine_act_far(lib, store):
    """in, out, out_pre and res share one stride triple: all four are far, interleaved"""
    from dep_gan_im_amd import _lib
    B, H, W, Cc = VB, 8, 8, 32
    o = fr.make_ops("exact", np.random.default_rng(17), B, H, W, Cc, Cc, 1, affine=1, film=1, relu=1, res=1)
    pre = fr.affine(o.x, o, np.float64)
    out, st = fr.post_chain(pre, o, np.float64)
    assert fr.bounds_hold([pre] + st)
    ref = {"out": out.astype(np.float32), "pre": pre.astype(np.float32)}
    ld = Cc + 12
    fm, fa = np.full((B, ld), NANF, np.float32), np.full((B, ld), NANF, np.float32)
    fm[:, :Cc], fa[:, :Cc] = o.fmul, o.fadd
    d = [dev(a) for a in (o.scale, o.shift, fm, fa)]
    got = {}
    for f in (("in", "out", "pre", "res"), ()):
        w = make_views({n: ((B, H, W, Cc), 12, 4, "f", ro, dat) for n, ro, dat in
                        (("in", True, o.x), ("out", False, None), ("pre", False, None), ("res", True, o.res))}, store, f, "beyond")
        _lib.check(lib.depgan_op_affine_act(w["in"].args()[0], w["out"].args()[0], w["pre"].args()[0], *w["res"].args(),
                                            *map(P, d), ld, 1, B, H, W, Cc, 0, 0.0, None), "affine_act")
        torch.cuda.synchronize()
        got[f] = collect(w)
    same3(got[("in", "out", "pre", "res")], got[()], ref, "affine_act")


UNPOOL = (VB, 9, 7, 32)                # B, Ho, Wo, C: tests/bf16s_cases.py


@functools.lru_cache(maxsize=None)
def _unpool_case():
    B, Ho, Wo, Cc = UNPOOL
    rng = np.random.default_rng(Ho * 10 + Cc + 1)
    a = _ints(rng, (B, 2 * Ho, 2 * Wo, Cc), -1, 2)               # equal maxima in most windows
    dpool = _ints(rng, (B, Ho, Wo, Cc), -4, 4)
    sk = (rng.integers(-16, 17, (B, 2 * Ho, 2 * Wo, Cc)) / 8.0).astype(np.float32)
    u = _ints(rng, (B, 2 * Ho, 2 * Wo, Cc), -8, 8)
    ref = fr.unpool_mask(dpool, a, sk)
    assert (ref != fr.unpool_mask(dpool, a, sk, last=True)).sum() > ref.size // 20
    win = lambda t: t.reshape(B, Ho, 2, Wo, 2, Cc).transpose(0, 1, 3, 5, 2, 4).reshape(B, Ho, Wo, Cc, 4)   # noqa: E731
    gath = np.take_along_axis(win(u), win(a).argmax(-1)[..., None], -1)[..., 0]      # numpy: the first of equal maxima
    return a, dpool, sk, u, ref.astype(np.float32), gath


@pytest.mark.parametrize("far", ["d", "a", "skip", "out"])
@pytest.mark.parametrize("dt", ["f", "h"], ids=["fp32", "bf16s"])
def test_unpool_mask_far_operand(lib, store, far, dt):
    from dep_gan_im_amd import _lib
    B, Ho, Wo, Cc = UNPOOL
    a, dpool, sk, _, ref, _ = _unpool_case()
    got = {}
    for f in ((far,), ()):
        w = make_views({"d": ((B, Ho, Wo, Cc), 12, 4, "f", True, dpool),
                        "a": ((B, 2 * Ho, 2 * Wo, Cc), 16, 8, dt, True, a),
                        "skip": ((B, 2 * Ho, 2 * Wo, Cc), 36, 16, "f", True, sk),
                        "out": ((B, 2 * Ho, 2 * Wo, Cc), 20, 8, "f", False, None)}, store, f, "beyond")
        fn = lib.depgan_op_unpool_mask_bf16s if dt == "h" else lib.depgan_op_unpool_mask
        _lib.check(fn(*w["d"].args(), *w["a"].args(), *w["skip"].args(), *w["out"].args(), B, Ho, Wo, Cc, None), "unpool_mask")
        torch.cuda.synchronize()
        got[f] = collect(w)
    same3(got[(far,)], got[()], {"out": ref}, "unpool_mask far %s" % far)


@pytest.mark.parametrize("far", ["u", "a", "out"])
def test_gather_pool_far_operand(lib, store, far):
    from dep_gan_im_amd import _lib
    B, Ho, Wo, Cc = UNPOOL
    a, _, _, u, _, gath = _unpool_case()
    got = {}
    for f in ((far,), ()):
        w = make_views({"u": ((B, 2 * Ho, 2 * Wo, Cc), 12, 4, "f", True, u), "a": ((B, 2 * Ho, 2 * Wo, Cc), 20, 8, "f", True, a),
                        "out": ((B, Ho, Wo, Cc), 28, 12, "f", False, None)}, store, f, "beyond")
        _lib.check(lib.depgan_op_gather_pool(*w["u"].args(), *w["a"].args(), *w["out"].args(), B, Ho, Wo, Cc, None), "gather_pool")
        torch.cuda.synchronize()
        got[f] = collect(w)
    same3(got[(far,)], got[()], {"out": gath}, "gather_pool far %s" % far)


# ---------------------------------------------------------------------------------------------------------------------
# bf16-storage operators: strides in ELEMENTS, sample 1 sits 2^30 + 128 elements out
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bf16s_conv_case():
    shape = (VB, 22, 18, 8, 32, 3)     # CIN8 of tests/bf16s_cases.py
    o = fr.make_ops_bf16s("exact", np.random.default_rng(sum(shape) * 131 + 7 * 4), *shape, bias=1, affine=1, film=1, relu=1, res=1)
    q = fr.reference_bf16s(o)
    assert fr.bounds_hold(q["stages"]) and fr.is_bf16(o.x) and fr.is_bf16(o.res)
    return shape, o, q["out"]


@pytest.mark.parametrize("far", ["in", "res", "out"])
def test_conv2d_bf16s_far_operand(lib, store, far):
    from dep_gan_im_amd import _lib
    (B, H, W, ci, co, k), o, ref = _bf16s_conv_case()
    d = {n: dev(getattr(o, n)) for n in ("w", "bias", "scale", "shift")}
    ld = co + 12
    fm, fa = np.full((B, ld), NANF, np.float32), np.full((B, ld), NANF, np.float32)
    fm[:, :co], fa[:, :co] = o.fmul, o.fadd
    fmd, fad = dev(fm), dev(fa)
    got = {}
    for f in ((far,), ()):
        w = make_views({"in": ((B, H, W, ci), 16, 8, "h", True, o.x), "res": ((B, H, W, co), 40, 16, "h", True, o.res),
                        "out": ((B, H, W, co), 24, 8, "h", False, None)}, store, f, "beyond")
        _lib.check(lib.depgan_op_conv2d_bf16s(*w["in"].args(), P(d["w"]), P(d["bias"]), P(d["scale"]), P(d["shift"]), P(fmd), P(fad),
                                              ld, *w["res"].args(), *w["out"].args(), None, B, H, W, ci, co, k, o.relu, None),
                   "op_conv2d_bf16s")
        torch.cuda.synchronize()
        got[f] = collect(w)
    same3(got[(far,)], got[()], {"out": ref}, "conv2d_bf16s far %s" % far)


@pytest.mark.parametrize("far", ["in", "out"])
def test_deconv2x2_bf16s_far_operand(lib, store, far):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = VB, 8, 8, 64, 64
    rng = np.random.default_rng(ci + 3 * co + H)
    x = _ints(rng, (B, H, W, ci))
    wt = _ints(rng, (2, 2, co, ci), -1, 1)
    o = fr.make_ops("exact", np.random.default_rng(H + co), 1, 1, 1, 8, co, 1, bias=1, affine=1, relu=1)
    v = np.maximum(fr.affine(fr.deconv2x2(x, wt), o, np.float64), 0)
    assert fr.bounds_hold([v])
    ref = fr.rne_bf16(v.astype(np.float32))
    d = [dev(a) for a in (wt, o.bias, o.scale, o.shift)]
    got = {}
    for f in ((far,), ()):
        w = make_views({"in": ((B, H, W, ci), 16, 8, "h", True, x), "out": ((B, 2 * H, 2 * W, co), 24, 8, "h", False, None)},
                       store, f, "beyond")
        _lib.check(lib.depgan_op_deconv2x2_bf16s(*w["in"].args(), *map(P, d), *w["out"].args(), B, H, W, ci, co, 1, None),
                   "op_deconv2x2_bf16s")
        torch.cuda.synchronize()
        got[f] = collect(w)
    same3(got[(far,)], got[()], {"out": ref}, "deconv2x2_bf16s far %s" % far)


@pytest.mark.parametrize("far", ["dy", "res", "mask", "dx"])
def test_bwd_data_bf16s_far_operand(lib, store, far):
    from dep_gan_im_amd import _lib
    B, H, W, ci, co = VB, 16, 16, 32, 32
    o = fr.make_ops_bf16s("exact", np.random.default_rng(ci * 100 + co + H + 3), B, H, W, ci, co, 3, res=True, mask=True, bwd=True)
    r = fr.reference(o)
    assert fr.bounds_hold(r["stages"])
    wd = dev(o.w)
    got = {}
    for f in ((far,), ()):
        w = make_views({"dy": ((B, H, W, co), 12, 4, "f", True, o.x), "res": ((B, H, W, ci), 36, 16, "f", True, o.res),
                        "mask": ((B, H, W, ci), 16, 8, "h", True, o.mask), "dx": ((B, H, W, ci), 20, 8, "f", False, None)},
                       store, f, "beyond")
        _lib.check(lib.depgan_op_conv2d_bwd_data_bf16s(*w["dy"].args(), P(wd), *w["res"].args(), *w["mask"].args(), *w["dx"].args(),
                                                       B, H, W, ci, co, 0, None), "op_conv2d_bwd_data_bf16s")
        torch.cuda.synchronize()
        got[f] = collect(w)
    same3(got[(far,)], got[()], {"dx": r["out"].astype(np.float32)}, "bwd_data_bf16s far %s" % far)
