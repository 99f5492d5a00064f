"""GPU: depgan_op_signed_distance and depgan_op_boundary_loss, the boundary loss at operator level.

phi is asserted BIT FOR BIT against tests/boundary_ref.py (per slice from surface_ref.edt_sq_brute): shapes (1, 1, 1),
(1, 9, 70) (W past one wave), (3, 37, 70) (nothing a multiple of a tile), (2, 3, 300) and (2, 300, 3) (several row-scan
elements per thread, a column past the staging chunk); contents empty, full, a class in slice 0 only (slice 1 must be all
zero: slices do not leak), one pixel in opposite corners, a checkerboard, random at densities 0.01 and 0.5; C = 2, 3, 4,
8, spacings (1, 1), (0.9375, 0.9375), (0.977, 1.013), inside_offset 0 and the spacing's minimum, a class switched off.
Class 1 follows the content, the other pixels are spread over the other classes, so every class has a map to check.
Exact too: codes against one-hot rows, an ignore code against all-zero rows, a second call into the same buffers, and
phi of one class against depgan_eval_edt_sq run on every slice (the two entries share one distance-transform text).

The loss and dz against float64 formed from the device's own stored probabilities and phi, P = 1 (one thread), 255 (a
ragged block), 3219 (a ragged grid of 13 blocks) and 262181 (37 pixels past the 1024-block cap, where the grid-stride loop
takes over): dz within 1e-5 max|dz| (the softmax-CE bound), L_B within 1e-5 of sum|terms| / M -- the terms are signed, so a
bound relative to L_B itself means nothing near 0.  dz null gives the loss only, M = 0 gives 0.0 and an untouched dz,
and every refusal leaves the buffers' bits as they were."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boundary_ref as BR  # noqa: E402
import weighted_ce_ref as R  # noqa: E402
from test_gpu_softmax_ce_weighted import P_, _u32  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (1, 9, 70), (3, 37, 70), (2, 3, 300), (2, 300, 3)]
CONTENTS = ["empty", "full", "slice0", "corners", "checker", "random0.01", "random0.5"]
# (classes, spacing, inside_offset, the classes switched on or None): walked over the contents, shifted per shape
PARAMS = [(2, (1.0, 1.0), 0.0, None), (3, (0.9375, 0.9375), 0.9375, None), (4, (0.977, 1.013), 0.0, (0, 1, 1, 1)),
          (8, (1.0, 1.0), 1.0, None), (3, (0.977, 1.013), 0.977, (1, 1, 0)), (4, (0.9375, 0.9375), 0.0, None),
          (2, (0.977, 1.013), 0.977, (0, 1)), (8, (0.9375, 0.9375), 0.0, (1, 1, 0, 1, 0, 1, 1, 1))]
PIXELS = [1, 255, 3219, 262181]


@functools.lru_cache(maxsize=None)
def _labels(shape, content, Cc):
    """(n, H, W) uint8 codes: class 1 where the content's pattern is set, the other classes spread over the rest."""
    n, H, W = shape
    rng = np.random.default_rng(n * 1000003 + H * 1009 + W + 17 * CONTENTS.index(content) + Cc)
    pat = np.zeros(shape, bool)
    if content == "full":
        pat[:] = True
    elif content == "slice0":
        pat[0] = rng.uniform(size=(H, W)) < 0.3
        pat[0, 0, 0] = True
    elif content == "corners":
        pat[:, 0, 0] = pat[:, H - 1, W - 1] = True
    elif content == "checker":
        pat[:] = (np.add.outer(np.arange(H), np.arange(W)) % 2 == 0)[None]
    elif content.startswith("random"):
        pat[:] = rng.uniform(size=shape) < float(content[6:])
    others = np.array([k for k in range(Cc) if k != 1], np.uint8)
    return np.where(pat, np.uint8(1), others[rng.integers(0, len(others), shape)]).astype(np.uint8)


def _phi(lib, labels, Cc, spacing=(1.0, 1.0), off=0.0, on=None, ign=-1, out=None):
    """One call: (rc, phi (n, H, W, Cc) float32).  labels: uint8 codes (n, H, W) or float32 one-hot rows; the output
    starts NaN-filled unless `out` (a device tensor) is given."""
    n, H, W = labels.shape[:3]
    ld = torch.from_numpy(labels).cuda()
    onehot = labels.dtype == np.float32
    phi = out if out is not None else torch.full((n, H, W, Cc), float("nan"), device="cuda:0")
    sw = (C.c_int * Cc)(*on) if on is not None else None
    rc = lib.depgan_op_signed_distance(P_(ld) if onehot else None, None if onehot else P_(ld), ign, n, H, W, Cc, sw,
                                       spacing[0], spacing[1], off, P_(phi), None)
    torch.cuda.synchronize()
    return rc, phi.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_phi_equals_the_restatement_bit_for_bit(lib, shape):
    si = SHAPES.index(shape)
    for ci, content in enumerate(CONTENTS):
        # two parameter sets per content; the largest shape takes one, its float64 reference is the slow part
        sets = (PARAMS[(ci + si) % len(PARAMS)], PARAMS[(ci + si + 4) % len(PARAMS)])
        for Cc, spacing, off, on in sets[:1 if shape == (3, 37, 70) else 2]:
            codes = _labels(shape, content, Cc)
            rc, phi = _phi(lib, codes, Cc, spacing, off, on)
            assert rc == 0, lib.depgan_last_error()
            want = BR.signed_distance(BR.true_class(codes, Cc), Cc, spacing, off, on)
            assert np.array_equal(_u32(phi), _u32(want)), (content, Cc, spacing, off, on,
                                                           float(np.nanmax(np.abs(phi - want))))
            if content in ("empty", "full") or (content == "slice0" and shape[0] > 1):
                quiet = phi[..., 1] if content != "slice0" else phi[1:, :, :, 1]
                assert np.all(quiet == 0)                       # absent, filling, or present in another slice only
            if content == "slice0" and shape[1] * shape[2] > 1:
                assert np.any(phi[0, :, :, 1] != 0)
            if on is not None:
                assert all(np.all(phi[..., k] == 0) for k in range(Cc) if not on[k])


def _edt_sq_slice(lib, member, wy, wx):
    """depgan_eval_edt_sq on one (H, W) slice as a (1, H, W) volume: float64 squared distances to the nearest member."""
    H, W = member.shape
    s = torch.from_numpy(np.ascontiguousarray(member, np.uint8)).cuda()
    d2 = torch.full((H, W), float("nan"), dtype=torch.float64, device="cuda:0")
    scratch = torch.empty((lib.depgan_eval_edt_scratch_bytes(1, H, W) // 8,), dtype=torch.float64, device="cuda:0")
    assert lib.depgan_eval_edt_sq(P_(s), 1, H, W, 1.0, wy, wx, P_(d2), P_(scratch), None) == 0, lib.depgan_last_error()
    torch.cuda.synchronize()
    return d2.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_phi_is_the_surface_distance_transform_of_the_slice(lib, shape):
    """The invariant the shared distance-transform text exists for: phi of class 1 is, in every pixel of every slice,
    the square root of what depgan_eval_edt_sq gives for S = {label == 1} (outside S) or for its complement (inside S,
    negated and shifted by inside_offset), rounded once to float32, and 0 where that distance is infinite.  IEEE sqrt
    is correctly rounded on both sides, so the comparison is on bits."""
    n, H, W = shape
    for content in ("empty", "full", "corners", "checker", "random0.01", "random0.5"):
        codes = _labels(shape, content, 2)
        for (sy, sx), off in (((1.0, 1.0), 0.0), ((0.977, 1.013), 0.977)):
            rc, phi = _phi(lib, codes, 2, (sy, sx), off, on=(0, 1))
            assert rc == 0, lib.depgan_last_error()
            assert np.all(phi[..., 0] == 0)
            for z in range(n):
                S = codes[z] == 1
                out = np.sqrt(_edt_sq_slice(lib, S, sy * sy, sx * sx)).astype(np.float32)
                ins = (-(np.sqrt(_edt_sq_slice(lib, ~S, sy * sy, sx * sx)) - off)).astype(np.float32)
                want = np.where(S, ins, out)
                want[~np.isfinite(want)] = 0.0
                np.testing.assert_array_equal(_u32(phi[z, :, :, 1]), _u32(want), err_msg=str((content, sy, sx, off, z)))


@pytest.mark.parametrize("Cc", [2, 3, 4, 8])
def test_codes_equal_one_hot_rows_and_a_second_call_reuses_the_buffers(lib, Cc):
    shape = (2, 21, 70)
    codes = _labels(shape, "random0.5", Cc)
    sp, off = (0.977, 1.013), 0.5
    a = _phi(lib, codes, Cc, sp, off)
    b = _phi(lib, R.onehot_rows(codes, Cc), Cc, sp, off)
    assert a[0] == 0 and b[0] == 0 and np.array_equal(_u32(a[1]), _u32(b[1]))
    # an ignore code against all-zero rows: the marked pixels are members of no class
    marked = codes.copy()
    marked[:, ::3, ::4] = 255
    c = _phi(lib, marked, Cc, sp, off, ign=255)
    d = _phi(lib, R.onehot_rows(marked, Cc, 255), Cc, sp, off, ign=0)
    assert c[0] == 0 and d[0] == 0 and np.array_equal(_u32(c[1]), _u32(d[1]))
    want = BR.signed_distance(BR.true_class(marked, Cc, 255), Cc, sp, off)
    assert np.array_equal(_u32(c[1]), _u32(want)) and not np.array_equal(_u32(c[1]), _u32(a[1]))
    # without an ignore code the all-zero rows are class 0 (the first arg-max), a code >= C has no class
    e = _phi(lib, R.onehot_rows(marked, Cc, 255), Cc, sp, off, ign=-1)
    assert np.array_equal(_u32(e[1]), _u32(BR.signed_distance(np.where(marked == 255, 0, marked), Cc, sp, off)))
    f = _phi(lib, marked, Cc, sp, off, ign=-1)
    assert np.array_equal(_u32(f[1]), _u32(want))
    # a second call into the same output: nothing of the first call survives, nothing needs zeroing
    buf = torch.full(shape + (Cc,), float("nan"), device="cuda:0")
    assert _phi(lib, _labels(shape, "checker", Cc), Cc, (1.0, 1.0), 1.0, out=buf)[0] == 0
    again = _phi(lib, codes, Cc, sp, off, out=buf)
    assert again[0] == 0 and np.array_equal(_u32(again[1]), _u32(a[1]))


@functools.lru_cache(maxsize=None)
def _operands(lib, Cc, P):
    """(probabilities as depgan_op_softmax_ce stores them, phi, codes): phi from the device's distance pass for P = 3219
    = 37 x 87, else signed float32 values of a map's size (a few pixels, some exact zeros)."""
    rng = np.random.default_rng(31 * Cc + P % 1013)
    z = (2.0 * rng.standard_normal((P, Cc))).astype(np.float32)
    codes = rng.integers(0, Cc, P).astype(np.uint8)
    zd = torch.from_numpy(z).cuda()
    probs = torch.full((P, Cc), float("nan"), device="cuda:0")
    assert lib.depgan_op_softmax_ce(P_(zd), None, None, P_(probs), None, None, P, Cc, None) == 0, lib.depgan_last_error()
    torch.cuda.synchronize()
    if P == 3219:
        rc, phi = _phi(lib, codes.reshape(1, 37, 87), Cc, (0.9375, 0.9375), 0.0)
        assert rc == 0
        phi = phi.reshape(P, Cc)
    else:
        phi = (8.0 * rng.standard_normal((P, Cc))).astype(np.float32)
        phi[rng.uniform(size=(P, Cc)) < 0.1] = 0.0
    return probs.cpu().numpy(), phi, codes


def _loss(lib, p, phi, onehot, codes, ign, coef, bc, Cc, dz_in="nan", n=None):
    """One call: (rc, dz or None, L_B, M).  dz_in: an array, "nan" for a NaN-filled dz, None for a null dz."""
    P = len(p)
    pd, fd = torch.from_numpy(p).cuda(), torch.from_numpy(phi).cuda()
    od = torch.from_numpy(onehot).cuda() if onehot is not None else None
    cd = torch.from_numpy(codes).cuda() if codes is not None else None
    dz = None if dz_in is None else (torch.full((P, Cc), float("nan"), device="cuda:0") if isinstance(dz_in, str)
                                     else torch.from_numpy(dz_in).cuda())
    ca = (C.c_float * len(coef))(*[float(v) for v in coef]) if coef is not None else None
    out = (C.c_double * 2)(-7.0, -7.0)
    rc = lib.depgan_op_boundary_loss(P_(pd), P_(fd), P_(od), P_(cd), ign, ca,
                                     (len(coef) if coef is not None else 0) if n is None else n, bc, P_(dz), out, P, Cc,
                                     None)
    torch.cuda.synchronize()
    return rc, (None if dz is None else dz.cpu().numpy()), out[0], out[1]


def _coef(Cc):
    c = np.array([0.0, 1.25, 0.7, 3.0, 0.5, 1.0, 2.0, 0.25], np.float32)[:Cc]
    c[Cc - 1] = 0.25
    return c


@pytest.mark.parametrize("P", PIXELS)
@pytest.mark.parametrize("Cc", [2, 3, 4, 8])
def test_loss_and_gradient_against_float64(lib, Cc, P):
    p, phi, codes = _operands(lib, Cc, P)
    rng = np.random.default_rng(7 * Cc + P)
    d0 = (rng.standard_normal((P, Cc)) / P).astype(np.float32)
    marked = codes.copy()
    marked[::5] = 255
    worst_dz = worst_l = 0.0
    for coef, bc in ((None, 1.0), (_coef(Cc), 0.37)):
        c64 = BR.class_coef(Cc, coef)
        for lab, ign in ((codes, -1), (marked, 255)):
            keep = (lab != 255).astype(np.float64)
            a = _loss(lib, p, phi, None, lab, ign, coef, bc, Cc, dz_in=d0)
            assert a[0] == 0, lib.depgan_last_error()
            inc, L, M, scale = BR.boundary_np(p, phi, keep, c64)
            want = d0.astype(np.float64) + float(np.float32(bc)) * inc
            assert a[3] == M == keep.sum()
            e_dz = float(np.abs(a[1] - want).max() / np.abs(want).max())
            e_l = abs(a[2] - L) / scale if scale else abs(a[2] - L)
            worst_dz, worst_l = max(worst_dz, e_dz), max(worst_l, e_l)
            assert e_dz <= 1e-5, (coef is None, ign, e_dz)
            assert e_l <= 1e-5, (coef is None, ign, a[2], L, scale)
            assert np.array_equal(_u32(a[1][keep == 0]), _u32(d0[keep == 0]))      # a pixel that takes no part keeps its dz
            # the increment alone, on a zero dz
            z0 = _loss(lib, p, phi, None, lab, ign, coef, bc, Cc, dz_in=np.zeros((P, Cc), np.float32))
            ref = float(np.float32(bc)) * inc
            if np.abs(ref).max() > 0:
                assert np.abs(z0[1] - ref).max() <= 1e-5 * np.abs(ref).max()
            # one-hot rows give the bits of the codes; all-zero rows those of the ignore code
            oh = R.onehot_rows(lab, Cc, 255 if ign == 255 else None)
            b = _loss(lib, p, phi, oh, None, 0 if ign == 255 else -1, coef, bc, Cc, dz_in=d0)
            assert b[0] == 0 and np.array_equal(_u32(a[1]), _u32(b[1])) and a[2:] == b[2:]
            # dz null: the loss only, the same bits
            n0 = _loss(lib, p, phi, None, lab, ign, coef, bc, Cc, dz_in=None)
            assert n0[0] == 0 and n0[2:] == a[2:]
    print("C = %d, P = %d: worst |dz - fp64| / max|dz| = %.2e, worst |L_B - fp64| / (sum|terms| / M) = %.2e"
          % (Cc, P, worst_dz, worst_l))


@pytest.mark.parametrize("Cc", [3, 4])
def test_no_pixel_takes_part_and_refusals_touch_nothing(lib, Cc):
    P = 3219
    p, phi, codes = _operands(lib, Cc, P)
    nothing = np.full(P, 255, np.uint8)
    a = _loss(lib, p, phi, None, nothing, 255, None, 1.0, Cc)                  # NaN-filled dz
    assert a[0] == 0 and a[2] == 0.0 and a[3] == 0.0
    assert np.all(_u32(a[1]) == _u32(np.full((P, Cc), float("nan"), np.float32)))
    b = _loss(lib, p, phi, np.zeros((P, Cc), np.float32), None, 0, None, 1.0, Cc)
    assert b[0] == 0 and b[2] == 0.0 and b[3] == 0.0 and np.isnan(b[1]).all()
    # boundary_coef = 0 adds a zero to every dz that takes part and still reports L_B
    d0 = np.full((P, Cc), 0.25, np.float32)
    z = _loss(lib, p, phi, None, codes, -1, None, 0.0, Cc, dz_in=d0)
    assert z[0] == 0 and np.array_equal(z[1], d0) and z[2] != 0.0 and z[3] == P
    # refusals: status 1, a message, and the bits of dz and phi as they were
    mark = np.full((P, Cc), -3.5, np.float32)
    nan = float("nan")
    for kw in ({"coef": [1.0] * (Cc - 1)}, {"coef": [0.0] * Cc}, {"coef": [1.0, nan] + [1.0] * (Cc - 2)},
               {"coef": [-1.0] + [1.0] * (Cc - 1)}, {"bc": -1.0}, {"bc": nan}, {"bc": float("inf")}, {"ign": 256}):
        args = dict({"coef": None, "bc": 1.0, "ign": -1}, **kw)
        r = _loss(lib, p, phi, None, codes, args["ign"], args["coef"], args["bc"], Cc, dz_in=mark)
        assert r[0] == 1 and lib.depgan_last_error() and np.array_equal(_u32(r[1]), _u32(mark)), kw
        assert (r[2], r[3]) == (-7.0, -7.0)
    lab = codes.reshape(1, 37, 87)
    for kw in ({"spacing": (0.0, 1.0)}, {"spacing": (1.0, nan)}, {"off": 1.5}, {"off": -0.1}, {"on": [0] * Cc},
               {"ign": 256}):
        args = dict({"spacing": (1.0, 1.0), "off": 0.0, "on": None, "ign": -1}, **kw)
        buf = torch.full((1, 37, 87, Cc), -3.5, device="cuda:0")
        r = _phi(lib, lab, Cc, args["spacing"], args["off"], args["on"], args["ign"], out=buf)
        assert r[0] == 1 and lib.depgan_last_error() and np.all(r[1] == -3.5), kw
