"""GPU: the surface-distance kernels (csrc/surface_dist.hip) at operator level and evaluate.distance_transform /
surface_distances / label_surface_metrics on top of them, against the NumPy restatement (tests/surface_ref.py).

Asserted bit for bit: the squared distance map against the brute-force minimum over all set voxels (the 3 x 256 x 256
case against the three-pass restatement, which tests/test_surface_cpu.py holds equal to the brute-force one), both
surface masks, the surface count, the maximum, the count of infinite distances and the Hausdorff distances.  The
percentiles are within 4 units in the last place of np.percentile on the reference distances (NumPy's interpolation
statement is restated, and 0 units were measured).  The sum of the square roots is within (n_surface + 2) 2^-52
relative to math.fsum of the reference terms: all terms are non-negative, each square root is correctly rounded on both
sides, and the adds are the rest (measured 4.3e-16 at worst); the directed means within (n_surface + 3) 2^-52, one
division more (measured 3.1e-16).

Shapes: the smallest at which a kernel takes another path -- a single voxel; one slice (no third pass) with W past one
wave; nothing a multiple of a tile; a row, a column and a depth longer than the 64-column / 16-row tiles and the
64-row staging chunk (300 > 256 also gives the row scan two voxels per thread).

Measured worst deviations are printed (pytest -s) and recorded in DESIGN.md section 7."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SPACINGS = [(1, 1, 1), (3, 0.9375, 0.9375), (2.7, 0.977, 1.013)]
SHAPES = [(1, 1, 1), (1, 9, 70), (5, 37, 70), (3, 3, 300), (3, 300, 3), (70, 5, 9)]
CONTENTS = ["empty", "full", "corners", "slab", "random_0.01", "random_0.5"]
BLOBS = (3, 256, 256)
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def volume(shape, name):
    """bool (D, H, W), read-only"""
    rng = np.random.default_rng(sum(shape) + len(name))
    D, H, W = shape
    a = np.zeros(shape, bool)
    if name == "full":
        a[:] = True
    elif name == "corners":
        a[0, 0, 0] = a[-1, -1, -1] = True
    elif name == "slab":
        a[D // 2] = True
    elif name.startswith("random_"):
        a = rng.uniform(size=shape) < float(name[7:])
    elif name.startswith("blobs"):
        zz, yy, xx = np.indices(shape)
        for _ in range(40):
            c = rng.uniform(size=3) * shape
            r = rng.uniform(2, 14)
            a |= ((zz - c[0]) * 3.0) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 < r * r
    elif name != "empty":
        raise KeyError(name)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ref_d2(shape, name, spacing):
    edt = R.edt_sq_separable if shape == BLOBS else R.edt_sq_brute
    out = edt(volume(shape, name), R.weights(spacing))
    out.setflags(write=False)
    return out


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Dev:
    def __init__(self, lib):
        import torch
        self.torch, self.lib = torch, lib
        self.dev = torch.device("cuda:0")
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def u8(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(self.dev)

    def f64(self, a):
        return self.torch.from_numpy(np.array(a, np.float64)).to(self.dev)        # a copy: `a` may be read-only

    def edt_sq(self, set_np, spacing):
        D, H, W = set_np.shape
        s = self.u8(set_np)
        d2 = self.torch.full((D, H, W), -1.0, dtype=self.torch.float64, device=self.dev)
        nbytes = self.lib.depgan_eval_edt_scratch_bytes(D, H, W)
        assert nbytes >= D * H * W * 10
        scratch = self.torch.empty((nbytes // 8,), dtype=self.torch.float64, device=self.dev)
        w = R.weights(spacing)
        assert self.lib.depgan_eval_edt_sq(_p(s), D, H, W, w[0], w[1], w[2], _p(d2), _p(scratch), self.stream) == 0, \
            self.lib.depgan_last_error()
        return d2.cpu().numpy()

    def surface_mask(self, set_np, in_plane):
        D, H, W = set_np.shape
        s = self.u8(set_np)
        out = self.torch.full((D, H, W), 7, dtype=self.torch.uint8, device=self.dev)
        assert self.lib.depgan_eval_surface_mask(_p(s), D, H, W, in_plane, _p(out), self.stream) == 0, \
            self.lib.depgan_last_error()
        return out.cpu().numpy()

    def sums(self, d2_np, surf_np):
        n = d2_np.size
        d2, surf = self.f64(d2_np), self.u8(surf_np)
        nbytes = self.lib.depgan_eval_surface_sums_scratch_bytes(n)
        assert nbytes >= 64
        partial = self.torch.empty((nbytes // 8,), dtype=self.torch.float64, device=self.dev)
        out = (C.c_double * 4)()
        assert self.lib.depgan_eval_surface_sums(_p(d2), _p(surf), n, _p(partial), out, self.stream) == 0, \
            self.lib.depgan_last_error()
        return [float(v) for v in out]


@pytest.fixture(scope="module")
def dev(lib):
    return Dev(lib)


WORST = {"sum_rel": 0.0, "msd_rel": 0.0, "percentile_ulp": 0.0}


def check_sums(got, d2, surf):
    cnt, mx, ref_sum, ninf = R.surface_sums(d2, surf)
    assert got[0] == cnt and got[1] == mx and got[3] == ninf
    if math.isinf(ref_sum):
        assert got[2] == ref_sum
    elif ref_sum == 0.0:
        assert got[2] == 0.0
    else:
        rel = abs(got[2] - ref_sum) / ref_sum
        WORST["sum_rel"] = max(WORST["sum_rel"], rel)
        print("sum of sqrt: relative deviation %.3g (bound %.3g)" % (rel, (cnt + 2) * EPS))
        assert rel <= (cnt + 2) * EPS


@pytest.mark.parametrize("name", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_against_the_brute_force_reference(dev, shape, name):
    a = volume(shape, name)
    for in_plane in (0, 1):
        np.testing.assert_array_equal(dev.surface_mask(a, in_plane), R.surface_mask(a, in_plane))
    # the voxels the sums run over: the surface of another volume, so the distances are not all zero
    surf = R.surface_mask(volume(shape, "random_0.5" if name != "random_0.5" else "slab"), 0)
    for sp in SPACINGS:
        want = ref_d2(shape, name, sp)
        got = dev.edt_sq(a, sp)
        np.testing.assert_array_equal(got, want)
        check_sums(dev.sums(got, surf), want, surf)
    check_sums(dev.sums(ref_d2(shape, name, SPACINGS[2]), np.zeros(shape, np.uint8)), want, np.zeros(shape, np.uint8))


def test_blobs_256_against_the_three_pass_reference(dev):
    a = volume(BLOBS, "blobs")
    assert 0.02 < a.mean() < 0.5
    for in_plane in (0, 1):
        np.testing.assert_array_equal(dev.surface_mask(a, in_plane), R.surface_mask(a, in_plane))
    surf = R.surface_mask(volume(BLOBS, "blobs2"), 1)
    for sp in SPACINGS:
        want = ref_d2(BLOBS, "blobs", sp)
        got = dev.edt_sq(a, sp)
        np.testing.assert_array_equal(got, want)
        check_sums(dev.sums(got, surf), want, surf)


def check_metrics(got, want):
    assert tuple(got) == R.KEYS
    assert (got["n_surface_a"], got["n_surface_b"]) == (want["n_surface_a"], want["n_surface_b"])
    na, nb = got["n_surface_a"], got["n_surface_b"]
    if na == 0 or nb == 0:
        assert all(math.isnan(got[k]) for k in R.KEYS[2:])
        return
    assert got["hd_ab"] == want["hd_ab"] and got["hd_ba"] == want["hd_ba"] and got["hd"] == want["hd"]
    for key, cnt in (("msd_ab", na), ("msd_ba", nb)):
        rel = abs(got[key] - want[key]) / want[key] if want[key] else abs(got[key])
        WORST["msd_rel"] = max(WORST["msd_rel"], rel)
        assert rel <= (cnt + 3) * EPS, key                 # the sum's bound and the division
    assert got["assd"] == (got["msd_ab"] + got["msd_ba"]) / 2
    assert abs(got["assd"] - want["assd"]) <= (max(na, nb) + 4) * EPS * want["assd"]
    for key in ("hd95_ab", "hd95_ba", "hd95_pooled", "hd95"):
        ulp = abs(got[key] - want[key]) / np.spacing(want[key]) if want[key] else abs(got[key])
        WORST["percentile_ulp"] = max(WORST["percentile_ulp"], ulp)
        assert ulp <= 4, key
    assert got["hd95"] == max(got["hd95_ab"], got["hd95_ba"])
    assert got["hd"] == max(got["hd_ab"], got["hd_ba"])


PAIRS = [((5, 37, 70), "random_0.01", "random_0.5"), ((5, 37, 70), "slab", "corners"),
         ((1, 9, 70), "random_0.5", "full"), ((70, 5, 9), "corners", "random_0.5"),
         ((3, 3, 300), "random_0.5", "random_0.01"), ((1, 1, 1), "full", "full")]


@pytest.mark.parametrize("in_plane", [False, True])
@pytest.mark.parametrize("shape,na,nb", PAIRS)
def test_surface_distances_against_the_reference_algebra(lib, shape, na, nb, in_plane):
    from dep_gan_im_amd import evaluate
    a, b = volume(shape, na), volume(shape, nb)
    for sp, q in zip(SPACINGS, (95.0, 50, 99.9)):
        got = evaluate.surface_distances(a.astype(np.float32), b.astype(np.int8), sp, in_plane, q)
        check_metrics(got, R.surface_distances(a, b, sp, in_plane, q))
    print("worst so far: %r" % (WORST,))


def test_surface_distances_of_blobs_and_device_inputs(lib):
    import torch
    from dep_gan_im_amd import evaluate
    a, b = volume(BLOBS, "blobs"), volume(BLOBS, "blobs2")
    sp = SPACINGS[1]
    a_dev, b_dev = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.astype(np.float32)).cuda()
    got = evaluate.surface_distances(a_dev, b_dev, sp, in_plane=True)
    check_metrics(got, R.surface_distances(a, b, sp, True, 95.0, edt=R.edt_sq_separable))
    assert got["hd"] > got["hd95"] > got["assd"] > 0
    print("worst so far: %r" % (WORST,))


def test_empty_surfaces_give_nan_and_nothing_raises(lib):
    from dep_gan_im_amd import evaluate
    shape = (5, 37, 70)
    some, none = volume(shape, "random_0.01"), volume(shape, "empty")
    for a, b in ((some, none), (none, some), (none, none)):
        got = evaluate.surface_distances(a, b, SPACINGS[1])
        check_metrics(got, R.surface_distances(a, b, SPACINGS[1]))
        assert all(math.isnan(got[k]) for k in R.KEYS[2:])
    assert evaluate.surface_distances(some, none)["n_surface_a"] > 0


def test_distance_transform(lib):
    import torch
    from dep_gan_im_amd import evaluate
    shape, sp = (5, 37, 70), SPACINGS[2]
    a = volume(shape, "random_0.01")
    want = ref_d2(shape, "random_0.01", sp)
    d2 = evaluate.distance_transform(a.astype(np.float32) * 3.5, sp, squared=True)
    assert d2.is_cuda and d2.dtype == torch.float64 and tuple(d2.shape) == shape
    np.testing.assert_array_equal(d2.cpu().numpy(), want)
    d = evaluate.distance_transform(torch.from_numpy(a.copy()).cuda(), sp)
    np.testing.assert_array_equal(d.cpu().numpy(), np.sqrt(want))
    assert torch.isinf(evaluate.distance_transform(volume(shape, "empty"))).all()


def test_label_surface_metrics_equals_per_class_calls(lib):
    import torch
    from dep_gan_im_amd import evaluate
    shape, sp = (5, 37, 70), SPACINGS[1]
    rng = np.random.default_rng(11)
    labels = rng.integers(0, 4, size=shape).astype(np.int8)
    code = np.where(rng.uniform(size=shape) < 0.7, labels, rng.integers(0, 4, size=shape)).astype(np.float32)
    mask = (rng.uniform(size=shape) < 0.8).astype(np.float32)
    got = evaluate.label_surface_metrics(torch.from_numpy(labels).cuda(), code[..., None], spacing=sp, mask=mask,
                                         in_plane=True)
    assert sorted(got) == [1, 2, 3]
    lm, cm = labels * (mask != 0), code * (mask != 0)
    for k in (1, 2, 3):
        assert got[k] == evaluate.surface_distances(lm == k, cm == k, sp, True)      # the same calls: the same bits
        check_metrics(got[k], R.surface_distances(lm == k, cm == k, sp, True))
    two = evaluate.label_surface_metrics(labels, code, classes=(0, 3), spacing=sp)
    assert sorted(two) == [0, 3] and two[3] == evaluate.surface_distances(labels == 3, code == 3, sp)


def test_refusals_launch_nothing(dev):
    """Status 1 and depgan_last_error; the outputs keep the bytes they had."""
    lib, torch = dev.lib, dev.torch
    D, H, W = 2, 4, 6
    n = D * H * W
    s = dev.u8(np.ones((D, H, W), np.uint8))
    surf = torch.full((n,), 7, dtype=torch.uint8, device=dev.dev)
    d2 = torch.full((n + 8,), -1.0, dtype=torch.float64, device=dev.dev)
    scratch = torch.full((lib.depgan_eval_edt_scratch_bytes(D, H, W) // 8,), -1.0, dtype=torch.float64, device=dev.dev)
    partial = torch.full((lib.depgan_eval_surface_sums_scratch_bytes(n) // 8,), -1.0, dtype=torch.float64,
                         device=dev.dev)
    out = (C.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
    st, one = dev.stream, (1.0, 1.0, 1.0)
    inside = C.c_void_p(d2.data_ptr() + 8)                 # a range that overlaps d2
    refused = [
        lib.depgan_eval_surface_mask(_p(s), 0, H, W, 0, _p(surf), st),
        lib.depgan_eval_surface_mask(_p(s), D, 4097, W, 0, _p(surf), st),
        lib.depgan_eval_surface_mask(_p(s), 2048, 1024, 1024, 0, _p(surf), st),
        lib.depgan_eval_surface_mask(None, D, H, W, 0, _p(surf), st),
        lib.depgan_eval_surface_mask(_p(s), D, H, W, 0, None, st),
        lib.depgan_eval_surface_mask(_p(s), D, H, W, 2, _p(surf), st),
        lib.depgan_eval_surface_mask(_p(s), D, H, W, 0, C.c_void_p(s.data_ptr() + 1), st),
        lib.depgan_eval_edt_sq(_p(s), D, H, 0, *one, _p(d2), _p(scratch), st),
        lib.depgan_eval_edt_sq(_p(s), 4097, H, W, *one, _p(d2), _p(scratch), st),
        lib.depgan_eval_edt_sq(None, D, H, W, *one, _p(d2), _p(scratch), st),
        lib.depgan_eval_edt_sq(_p(s), D, H, W, *one, None, _p(scratch), st),
        lib.depgan_eval_edt_sq(_p(s), D, H, W, *one, _p(d2), None, st),
        lib.depgan_eval_edt_sq(_p(s), D, H, W, 0.0, 1.0, 1.0, _p(d2), _p(scratch), st),
        lib.depgan_eval_edt_sq(_p(s), D, H, W, 1.0, -1.0, 1.0, _p(d2), _p(scratch), st),
        lib.depgan_eval_edt_sq(_p(s), D, H, W, 1.0, 1.0, float("inf"), _p(d2), _p(scratch), st),
        lib.depgan_eval_edt_sq(_p(s), D, H, W, float("nan"), 1.0, 1.0, _p(d2), _p(scratch), st),
        lib.depgan_eval_edt_sq(_p(s), D, H, W, *one, _p(d2), inside, st),
        lib.depgan_eval_surface_sums(_p(d2), _p(surf), 0, _p(partial), out, st),
        lib.depgan_eval_surface_sums(_p(d2), _p(surf), 1 << 31, _p(partial), out, st),
        lib.depgan_eval_surface_sums(None, _p(surf), n, _p(partial), out, st),
        lib.depgan_eval_surface_sums(_p(d2), None, n, _p(partial), out, st),
        lib.depgan_eval_surface_sums(_p(d2), _p(surf), n, None, out, st),
        lib.depgan_eval_surface_sums(_p(d2), _p(surf), n, _p(partial), None, st),
        lib.depgan_eval_surface_sums(_p(d2), _p(surf), n, inside, out, st),
    ]
    assert refused == [1] * len(refused)
    assert b"eval_surface_sums" in lib.depgan_last_error()
    torch.cuda.synchronize()
    assert (surf == 7).all() and (d2 == -1).all() and (scratch == -1).all() and (partial == -1).all()
    assert list(out) == [-1.0] * 4
