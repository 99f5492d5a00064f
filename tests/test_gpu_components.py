"""GPU: the connected-component kernels (csrc/components.hip) at operator level and evaluate.connected_components /
component_sizes / remove_small_components / lesion_detection / label_lesion_metrics on top of them, against the NumPy
restatement (tests/ccl_ref.py).  Every output is an integer (or one division of two of them), so everything is
asserted bit for bit: there is no tolerance in this file.

Shapes (tests/ccl_cases.py): the smallest at which a kernel takes another path.  Every per-voxel kernel runs blocks of
256 voxels = four waves with lane = v mod 64, and cc_init_kernel cuts a run at each multiple of 64.
  (1, 1, 1)     one voxel, one partly filled wave
  (1, 9, 70)    one slice (no row below in z); W = 70 is no multiple of 64, so rows begin and end inside waves and
                most rows cross a wave boundary; three blocks
  (5, 37, 70)   nothing a multiple of a wave or a block; 51 blocks
  (3, 3, 300)   a run of 300 crosses four or five wave boundaries: the merge launch joins the pieces
  (3, 300, 3)   21 rows per wave: run starts inside the wave from the ballot; a column crosses several blocks
  (70, 5, 9)    a depth of 70: neighbours in z lie 45 voxels apart, in the same or the previous wave
  (2, 64, 64)   every row is exactly one wave and every block four rows: no run is cut
  (3, 256, 256) random blobs; 768 blocks, so cc_scan_kernel's single round of 1024 is nearly full
The scan's second round (more than 1024 blocks) is reached by test_scan_carries_past_one_round with 300 x 1024 voxels.
Contents: see ccl_cases.volume -- the late merges (comb, u), the long chains (serpentine, spirals), the singletons
(checker), the diagonals that tell the neighbourhoods apart, and random volumes around the percolation threshold."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ccl_cases as K  # noqa: E402
import ccl_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def ref_label(shape, name, connectivity, in_plane):
    """computed once, shared, read-only"""
    lab, n = R.label(K.volume(shape, name), connectivity, in_plane)
    lab.setflags(write=False)
    return lab, n


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

    def i32(self, a):
        return self.torch.from_numpy(np.array(a, np.int32)).to(self.dev)          # a copy: `a` may be read-only

    def label(self, set_np, connectivity, in_plane):
        D, H, W = set_np.shape
        s = self.u8(set_np.astype(np.uint8) * 255)                                # non-zero means set, not 1
        labels = self.torch.full((D, H, W), -5, dtype=self.torch.int32, device=self.dev)
        nbytes = self.lib.depgan_eval_cc_scratch_bytes(D, H, W)
        assert nbytes >= D * H * W * 4 + 8 and nbytes % 8 == 0
        scratch = self.torch.full((nbytes // 8,), -1, dtype=self.torch.int64, device=self.dev)
        out = (C.c_longlong * 1)(-1)
        assert self.lib.depgan_eval_cc_label(_p(s), D, H, W, connectivity, in_plane, _p(labels), _p(scratch), out,
                                             self.stream) == 0, self.lib.depgan_last_error()
        return labels.cpu().numpy(), int(out[0])

    def overlap(self, labels_np, other_np, n_comp):
        lab = self.i32(labels_np)
        other = None if other_np is None else self.u8(np.asarray(other_np, np.uint8) * 7)
        size = self.torch.full((max(n_comp, 1),), -3, dtype=self.torch.int32, device=self.dev)
        hits = self.torch.full((max(n_comp, 1),), -3, dtype=self.torch.int32, device=self.dev)
        assert self.lib.depgan_eval_cc_overlap(_p(lab), _p(other), lab.numel(), n_comp, _p(size), _p(hits),
                                               self.stream) == 0, self.lib.depgan_last_error()
        return size.cpu().numpy(), hits.cpu().numpy()


@pytest.fixture(scope="module")
def dev(lib):
    return Dev(lib)


def check_volume(dev, shape, names):
    for name in names:
        a = K.volume(shape, name)
        for c, in_plane in K.NEIGHBOURHOODS:
            want, n = ref_label(shape, name, c, in_plane)
            got, n_got = dev.label(a, c, in_plane)
            assert n_got == n, (name, c, in_plane)
            np.testing.assert_array_equal(got, want, err_msg="%s %d %d" % (name, c, in_plane))
            again, n_again = dev.label(a, c, in_plane)
            assert n_again == n and got.tobytes() == again.tobytes(), (name, c, in_plane)
        # in-plane rank 3 is rank 2
        got3, n3 = dev.label(a, 3, 1)
        assert n3 == ref_label(shape, name, 2, 1)[1] and np.array_equal(got3, ref_label(shape, name, 2, 1)[0])


# smallest first: the order in which a fault would be cheapest to read
@pytest.mark.parametrize("shape", K.SMALL_SHAPES)
def test_labels_against_the_reference(dev, shape):
    check_volume(dev, shape, K.CONTENTS)


def test_blobs_256_against_the_reference(dev):
    check_volume(dev, K.BLOBS, ["blobs"])
    assert ref_label(K.BLOBS, "blobs", 1, 1)[1] > ref_label(K.BLOBS, "blobs", 3, 0)[1] > 3


def test_scan_carries_past_one_round(dev):
    """1200 blocks of 256 voxels: cc_scan_kernel takes a second round with the carry of the first.  Isolated voxels, one
    in five, so that every block holds roots and the expected labels are a running count."""
    shape = (3, 100, 1024)
    a = (np.arange(3 * 100 * 1024) % 5 == 0).reshape(shape)
    assert a.size // 256 > 1024
    got, n = dev.label(a, 1, 1)                           # in the slice: the voxel 102400 = 5 x 20480 below is set too
    want = np.where(a, np.cumsum(a.ravel()).reshape(shape), 0).astype(np.int32)
    assert n == a.sum()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("shape", K.SMALL_SHAPES + [K.BLOBS])
def test_overlap_tables_against_bincount(dev, shape):
    names = ["blobs"] if shape == K.BLOBS else ["full", "checker", "comb", "random_0.31", "random_0.6"]
    rng = np.random.default_rng(5)
    other = rng.uniform(size=shape) < 0.3
    for name in names:
        a = K.volume(shape, name)
        for c, in_plane in ((1, 0), (3, 0), (2, 1)):
            lab, n = ref_label(shape, name, c, in_plane)
            for o in (other, a, None):
                size, hits = dev.overlap(lab, o, n)
                want_size, want_hits = R.sizes_hits(lab, n, o)
                np.testing.assert_array_equal(size[:n], want_size)
                np.testing.assert_array_equal(hits[:n], want_hits)
                if o is a:
                    np.testing.assert_array_equal(hits[:n], size[:n])
    # n_comp = 0 launches nothing: the tables keep their bytes; a label beyond n_comp is not counted
    lab, n = ref_label(shape, names[-1], 1, 0)
    size, hits = dev.overlap(lab, other, 0)
    assert size.tolist() == [-3] and hits.tolist() == [-3]
    if n > 1:
        size, hits = dev.overlap(lab, other, n - 1)
        np.testing.assert_array_equal(size[:n - 1], R.sizes_hits(lab, n, other)[0][:n - 1])
        np.testing.assert_array_equal(hits[:n - 1], R.sizes_hits(lab, n, other)[1][:n - 1])


def test_refusals_launch_nothing(dev):
    """Status 1 and depgan_last_error; the outputs keep the bytes they had."""
    lib, torch = dev.lib, dev.torch
    D, H, W = 2, 4, 6
    n = D * H * W
    s = dev.u8(np.ones((D, H, W), np.uint8))
    labels = torch.full((n + 8,), -5, dtype=torch.int32, device=dev.dev)
    scratch = torch.full((lib.depgan_eval_cc_scratch_bytes(D, H, W) // 8 + 1,), -1, dtype=torch.int64, device=dev.dev)
    size = torch.full((8,), -3, dtype=torch.int32, device=dev.dev)
    hits = torch.full((8,), -3, dtype=torch.int32, device=dev.dev)
    out = (C.c_longlong * 1)(-7)
    st = dev.stream
    label, overlap = lib.depgan_eval_cc_label, lib.depgan_eval_cc_overlap

    def off(t, nbytes):
        return C.c_void_p(t.data_ptr() + nbytes)

    refused = [
        label(_p(s), 0, H, W, 1, 0, _p(labels), _p(scratch), out, st),
        label(_p(s), D, 4097, W, 1, 0, _p(labels), _p(scratch), out, st),
        label(_p(s), 2048, 1024, 1024, 1, 0, _p(labels), _p(scratch), out, st),
        label(None, D, H, W, 1, 0, _p(labels), _p(scratch), out, st),
        label(_p(s), D, H, W, 1, 0, None, _p(scratch), out, st),
        label(_p(s), D, H, W, 1, 0, _p(labels), None, out, st),
        label(_p(s), D, H, W, 1, 0, _p(labels), _p(scratch), None, st),
        label(_p(s), D, H, W, 0, 0, _p(labels), _p(scratch), out, st),
        label(_p(s), D, H, W, 4, 0, _p(labels), _p(scratch), out, st),
        label(_p(s), D, H, W, 1, 2, _p(labels), _p(scratch), out, st),
        label(_p(s), D, H, W, 1, 0, off(labels, 2), _p(scratch), out, st),           # labels misaligned
        label(_p(s), D, H, W, 1, 0, _p(labels), off(scratch, 4), out, st),           # scratch misaligned
        label(_p(s), D, H, W, 1, 0, _p(labels), off(labels, 16), out, st),           # scratch over labels
        label(_p(s), D, H, W, 1, 0, off(scratch, 8), _p(scratch), out, st),          # labels over scratch
        overlap(_p(labels), _p(s), 0, 4, _p(size), _p(hits), st),
        overlap(_p(labels), _p(s), 1 << 31, 4, _p(size), _p(hits), st),
        overlap(_p(labels), _p(s), n, -1, _p(size), _p(hits), st),
        overlap(_p(labels), _p(s), n, n + 1, _p(size), _p(hits), st),
        overlap(None, _p(s), n, 4, _p(size), _p(hits), st),
        overlap(_p(labels), _p(s), n, 4, None, _p(hits), st),
        overlap(_p(labels), _p(s), n, 4, _p(size), None, st),
        overlap(_p(labels), _p(s), n, 4, off(size, 2), _p(hits), st),                # size misaligned
        overlap(_p(labels), _p(s), n, 4, _p(size), off(size, 8), st),                # hits over size
        overlap(_p(labels), _p(s), n, 4, off(labels, 32), _p(hits), st),             # size over labels
    ]
    assert refused == [1] * len(refused)
    assert b"eval_cc_overlap" in lib.depgan_last_error()
    torch.cuda.synchronize()
    assert (labels == -5).all() and (scratch == -1).all() and (size == -3).all() and (hits == -3).all()
    assert out[0] == -7


def test_connected_components_takes_any_dtype_host_or_device(lib):
    import torch
    from dep_gan_im_amd import evaluate
    shape = (5, 37, 70)
    a = K.volume(shape, "random_0.31")
    want, n = ref_label(shape, "random_0.31", 1, 0)
    for mask in (a, a.astype(np.uint8) * 9, a.astype(np.float32) * -0.5, torch.from_numpy(a.copy()).cuda(),
                 torch.from_numpy(a.astype(np.float32)).cuda()):
        labels, n_got = evaluate.connected_components(mask)
        assert labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == shape
        assert type(n_got) is int and n_got == n
        np.testing.assert_array_equal(labels.cpu().numpy(), want)
    for c, in_plane in K.NEIGHBOURHOODS:
        labels, n_got = evaluate.connected_components(a, connectivity=c, in_plane=bool(in_plane))
        assert n_got == ref_label(shape, "random_0.31", c, in_plane)[1]
        np.testing.assert_array_equal(labels.cpu().numpy(), ref_label(shape, "random_0.31", c, in_plane)[0])
    other = K.volume(shape, "random_0.5")
    labels, n_got = evaluate.connected_components(a)
    for o in (other, torch.from_numpy(other.astype(np.float32)).cuda(), None):
        for lab in (labels, np.array(want)):              # the device tensor, and a host array of labels
            size, hits = evaluate.component_sizes(lab, n, o)
            assert size.is_cuda and size.dtype == hits.dtype == torch.int32 and size.numel() == hits.numel() == n
            np.testing.assert_array_equal(size.cpu().numpy(), R.sizes_hits(want, n, None if o is None else other)[0])
            np.testing.assert_array_equal(hits.cpu().numpy(), R.sizes_hits(want, n, None if o is None else other)[1])
    empty, n0 = evaluate.connected_components(K.volume(shape, "empty"))
    assert n0 == 0 and not empty.any()
    size, hits = evaluate.component_sizes(empty, 0, other)
    assert size.numel() == 0 == hits.numel()


@pytest.mark.parametrize("min_voxels", [1, 2, 5])
def test_remove_small_components(lib, min_voxels):
    import torch
    from dep_gan_im_amd import evaluate
    shape = (5, 37, 70)
    for name, c, in_plane in (("random_0.25", 1, False), ("random_0.25", 2, True), ("random_0.01", 3, False)):
        a = K.volume(shape, name)
        got = evaluate.remove_small_components(a.astype(np.float32) * 2.5, min_voxels, c, in_plane)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == shape
        np.testing.assert_array_equal(got.cpu().numpy(), R.remove_small(a, min_voxels, c, in_plane))


def check_lesions(got, want):
    assert tuple(got) == R.KEYS + ("sizes_truth", "sizes_pred")
    for key in R.KEYS:
        assert type(got[key]) is type(want[key]), key
        if isinstance(want[key], float) and math.isnan(want[key]):
            assert math.isnan(got[key]), key
        else:
            assert got[key] == want[key], key
    for key in ("sizes_truth", "sizes_pred"):
        assert got[key].is_cuda
        host = got[key].cpu().numpy()
        assert host.dtype == want[key].dtype, key
        np.testing.assert_array_equal(host, want[key], err_msg=key)


def lesion_pairs():
    """(pred, truth) on the blobs volume: shifted, eroded, against empty, empty against, both empty, identical"""
    blobs = K.volume(K.BLOBS, "blobs")
    shifted = np.roll(blobs, (1, 5, -7), axis=(0, 1, 2))
    p = np.pad(blobs, 1, constant_values=False)
    eroded = (blobs & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1])
    none = np.zeros_like(blobs)
    return {"shifted": (shifted, blobs), "eroded": (eroded, blobs), "vs_empty": (none, blobs),
            "empty_vs": (blobs, none), "both_empty": (none, none), "identical": (blobs, blobs)}


@pytest.mark.parametrize("pair", ["shifted", "eroded", "vs_empty", "empty_vs", "both_empty", "identical"])
def test_lesion_detection_against_the_reference_algebra(lib, pair):
    import torch
    from dep_gan_im_amd import evaluate
    pred, truth = lesion_pairs()[pair]
    for kw in (dict(), dict(min_voxels=3, voxel_volume=0.9375 * 0.9375 * 3.0),
               dict(connectivity=1, in_plane=True, min_voxels=3)):
        got = evaluate.lesion_detection(pred.astype(np.float32), torch.from_numpy(truth.astype(np.int8)).cuda(), **kw)
        check_lesions(got, R.lesion_detection(pred, truth, **kw))
    if pair == "identical":
        assert got["recall"] == got["precision"] == got["f1"] == 1.0 and got["avd_percent"] == 0.0
    if pair == "shifted":
        assert 0 < got["recall"] and 0 < got["precision"] and got["n_truth"] > 3


def test_label_lesion_metrics_equals_per_class_calls(lib):
    import torch
    from dep_gan_im_amd import evaluate
    shape = (5, 37, 70)
    rng = np.random.default_rng(11)
    blocks = np.kron(rng.integers(0, 4, size=(5, 10, 14)), np.ones((1, 4, 5), np.int64))[:, :37, :]
    labels = np.where(rng.uniform(size=shape) < 0.5, blocks, 0).astype(np.int8)            # 4 classes, ragged lesions
    code = np.where(rng.uniform(size=shape) < 0.7, labels, rng.integers(0, 4, size=shape)).astype(np.float32)
    mask = (rng.uniform(size=shape) < 0.8).astype(np.float32)
    kw = dict(connectivity=2, in_plane=True, min_voxels=2, voxel_volume=0.5)
    got = evaluate.label_lesion_metrics(torch.from_numpy(labels).cuda(), code[..., None], mask=mask, **kw)
    assert sorted(got) == [1, 2, 3]
    lm, cm = labels * (mask != 0), code * (mask != 0)
    for k in (1, 2, 3):
        check_lesions(got[k], R.lesion_detection(lm == k, cm == k, **kw))
        check_lesions(evaluate.lesion_detection(lm == k, cm == k, **kw), R.lesion_detection(lm == k, cm == k, **kw))
    two = evaluate.label_lesion_metrics(labels, code, classes=(0, 3))
    assert sorted(two) == [0, 3]
    check_lesions(two[3], R.lesion_detection(labels == 3, code == 3))
