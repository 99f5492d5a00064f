"""GPU: evaluate.predict_stats through the model (64 x 64, three slices, three noise draws): the mean is predict_mean's
bit for bit, the variance is the restatement's on the same predictions, test-time flips agree with a hand-written NumPy
loop, and the uncertainty maps survive the trip through NIfTI."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_stats_ref as R  # noqa: E402
from test_gpu_eval_stats import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

N, HW, REPEAT = 3, 64, 3


def _inputs():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((N, HW, HW, 1)).astype(np.float32)
    mask = (rng.uniform(size=(N, HW, HW)) > 0.2).astype(np.float32)
    return x, mask


def _host(stats):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in stats.items()}


@pytest.mark.parametrize("nc_out", [4, 1])
def test_mean_is_predict_mean_and_var_the_restatement(nc_out):
    import torch
    import dep_gan_im_amd as dg
    from dep_gan_im_amd import evaluate as EV
    x, mask = _inputs()
    netG = dg.Gen_UNet2D((HW, HW, 1), (32, 1), 32, nc_out, seed=2)
    stats = EV.predict_stats(netG, x, n_repeat=REPEAT, mask=mask, rng=np.random.RandomState(4), ddof=1)
    mean = EV.predict_mean(netG, x, n_repeat=REPEAT, mask=mask, rng=np.random.RandomState(4))
    got = _host(stats)
    shape = (N, HW, HW, nc_out) if nc_out > 1 else (N, HW, HW)
    assert stats["mean"].dtype == torch.float64 and stats["var"].dtype == torch.float64
    assert got["mean"].shape == shape and got["var"].shape == shape
    same_bits(got["mean"], mean.cpu().numpy(), "mean against predict_mean")
    assert sorted(got) == (sorted(["mean", "var", "count", "entropy", "expected_entropy", "mutual_info", "votes"])
                           if nc_out > 1 else ["count", "mean", "var"])
    # the restatement on the same three predictions
    rng, ref = np.random.RandomState(4), R.new_state(N, HW, HW, nc_out)
    for _ in range(REPEAT):
        noise = rng.normal(size=(N, 32, 1)).astype("float32")
        R.accumulate(ref, netG.predict([x, noise]), mask)
    want = R.finish(ref, REPEAT, 1)
    same_bits(got["var"].reshape(ref["sum"].shape), want["var"], "var")
    same_bits(got["mean"].reshape(ref["sum"].shape), want["mean"], "mean")
    assert (got["count"] == REPEAT).all() and got["count"].dtype == np.uint8
    assert float(got["var"].max()) > 0
    if nc_out > 1:
        same_bits(got["votes"], ref["votes"], "votes")
        for k in ("entropy", "expected_entropy", "mutual_info"):
            assert got[k].shape == (N, HW, HW) and np.abs(got[k] - want[k]).max() <= 1e-12, k
        assert (got["mutual_info"] >= 0).all()


def test_tta_flips_against_a_numpy_loop():
    import dep_gan_im_amd as dg
    from dep_gan_im_amd import evaluate as EV
    from dep_gan_im_amd.data import Augmenter
    x, mask = _inputs()
    netG = dg.Gen_UNet2D((HW, HW, 1), (32, 1), 32, 4, seed=2)
    stats = EV.predict_stats(netG, x, n_repeat=REPEAT, mask=mask, rng=np.random.RandomState(4),
                             tta=Augmenter(flip_lr=True, flip_ud=True, seed=0))
    got = _host(stats)
    # by hand: the same rows say which slice is mirrored how; flip, predict, flip back, accumulate
    aug, rng, ref = Augmenter(flip_lr=True, flip_ud=True, seed=0), np.random.RandomState(4), R.new_state(N, HW, HW, 4)
    flipped = 0
    for _ in range(REPEAT):
        noise = rng.normal(size=(N, 32, 1)).astype("float32")
        rows = aug.draw(N, HW, HW)
        ud, lr = rows[:, 0] == -1, rows[:, 4] == -1
        flipped += int(ud.sum() + lr.sum())

        def flip(a):
            a = np.stack([s[::-1] if u else s for s, u in zip(a, ud)])
            return np.ascontiguousarray(np.stack([s[:, ::-1] if m else s for s, m in zip(a, lr)]))

        R.accumulate(ref, flip(netG.predict([flip(x), noise])), mask)
    assert flipped > 0
    want = R.finish(ref, REPEAT, 0)
    same_bits(got["mean"], want["mean"], "mean")
    same_bits(got["var"], want["var"], "var")
    same_bits(got["votes"], ref["votes"], "votes")
    assert (got["count"] == REPEAT).all()
    # explicit rows do what the Augmenter's did
    aug2 = Augmenter(flip_lr=True, flip_ud=True, seed=0)
    again = EV.predict_stats(netG, x, n_repeat=REPEAT, mask=mask, rng=np.random.RandomState(4),
                             tta=np.stack([aug2.draw(N, HW, HW) for _ in range(REPEAT)]))
    same_bits(_host(again)["mean"], got["mean"], "mean from explicit rows")


def test_uncertainty_maps_round_trip(tmp_path):
    import dep_gan_im_amd as dg
    from dep_gan_im_amd import evaluate as EV
    from dep_gan_im_amd import nifti
    x, mask = _inputs()
    affine = np.diag([0.9375, 0.9375, 4.0, 1.0])
    affine[:3, 3] = [-30.0, 12.0, 5.0]

    def back(a):
        return np.transpose(a, (1, 2, 0)).astype(np.float32)       # (Z, X, Y) slices -> file order, as data_prep_save

    stats = EV.predict_stats(dg.Gen_UNet2D((HW, HW, 1), (32, 1), 32, 4, seed=2), x, n_repeat=2, mask=mask,
                             rng=np.random.RandomState(1))
    paths = EV.save_uncertainty_maps(str(tmp_path), "s0", stats, affine)
    got = _host(stats)
    assert [os.path.basename(p) for p in paths] == ["s0_unc_entropy.nii.gz", "s0_unc_mutual_info.nii.gz"] + [
        "s0_unc_var_c%d.nii.gz" % c for c in range(4)]
    want = [got["entropy"], got["mutual_info"]] + [got["var"][..., c] for c in range(4)]
    for p, w in zip(paths, want):
        vol = nifti.load(p)
        assert vol.image.dtype == np.float32 and vol.image.shape == (HW, HW, N)
        assert np.array_equal(vol.image, back(w)) and np.allclose(vol.affine, affine)
    one = EV.predict_stats(dg.Gen_UNet2D((HW, HW, 1), seed=3), x, n_repeat=2, rng=np.random.RandomState(1))
    paths = EV.save_uncertainty_maps(str(tmp_path), "s1", one, affine)
    assert [os.path.basename(p) for p in paths] == ["s1_unc_var.nii.gz"]
    assert np.array_equal(nifti.load(paths[0]).image, back(_host(one)["var"]))
