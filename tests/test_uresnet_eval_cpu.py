"""CPU: the DEP-UResNet evaluation's scalar algebra (DEP-UResNet_testing_4fold.py "UE":566-700) against the NumPy
statements themselves, the host-side checks of the UT data step, and the new C ABI entries.

The float64 NumPy restatement of the UE statements lives here; tests/test_gpu_uresnet_eval.py imports it."""
import os
import re

import numpy as np
import pytest

from dep_gan_im_amd import _lib, data, evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("depgan_data_zscore_scratch_floats", "depgan_data_prep_zscore", "depgan_data_mask_slices",
               "depgan_labels_to_onehot", "depgan_eval_accumulate_channels", "depgan_eval_label_counts")


# ---- restatement of the UE statements (UE:166-185, 570-700) ----

def convert_from_1hot(label):
    """UE:166-185 (to_float=False): argmax over the channels as uint8, squeezed."""
    N, H, W, C = label.shape
    label_flat = label.reshape((N * H * W, C))
    n_data = len(label_flat)
    label_n_class = np.zeros((n_data, 1), dtype='uint8')
    label_n_class[range(n_data), 0] = np.argmax(label_flat, axis=1)
    return np.squeeze(label_n_class.reshape((N, H, W, 1)))


def ue_vol_dsc(output_img_pred_lbl, brain_cod_2tp, icv_and_sl_mask_1tp, brain_wmh_1tp, icv_and_sl_mask_2tp,
               brain_wmh_2tp, voxel_volume):
    """UE:572-700 statement by statement, from the label map on."""
    wmh_from_iam_1tp = np.multiply(icv_and_sl_mask_1tp, brain_wmh_1tp)
    vol_1tp__ml = np.count_nonzero(wmh_from_iam_1tp) * voxel_volume / 1000
    wmh_from_iam_2tp = np.multiply(icv_and_sl_mask_2tp, brain_wmh_2tp)
    vol_2tp__ml = np.count_nonzero(wmh_from_iam_2tp) * voxel_volume / 1000
    wmh_mask = np.zeros(output_img_pred_lbl.shape)
    wmh_mask[output_img_pred_lbl > 0] = 1
    vol_out__ml = np.count_nonzero(wmh_mask) * voxel_volume / 1000
    err_vol = vol_out__ml - vol_2tp__ml
    mse_vol = np.mean((vol_2tp__ml - vol_out__ml) ** 2)
    true_pred = true_prog = true_regg = prog = regg = 0
    if (vol_2tp__ml - vol_1tp__ml) >= 0:
        prog = 1
        if vol_out__ml - vol_1tp__ml >= 0:
            true_pred = true_prog = 1
    else:
        regg = 1
        if vol_out__ml - vol_1tp__ml < 0:
            true_pred = true_regg = 1
    fake = output_img_pred_lbl
    real = np.squeeze(brain_cod_2tp)
    smooth = 1e-7

    def dice(f, r, k):
        return (np.count_nonzero(f[r == k] == k) * 2.0 + smooth) / \
            (smooth + np.count_nonzero(r[r == k] == k) + np.count_nonzero(f[f == k] == k))

    dice_1, dice_2, dice_3 = (dice(fake, real, k) for k in (1, 2, 3))
    dice_4 = dice(fake > 0, real > 0, 1)
    dice_5 = dice(((fake == 1) + (fake == 2)) > 0, ((real == 1) + (real == 2)) > 0, 1)
    dice_6 = dice(fake == 3, real == 3, 1)
    avg_all_dice = (dice_1 + dice_2 + dice_3) / 3.0
    avg_dice__56 = (dice_5 + dice_6) / 2.0
    return [true_pred, prog, true_prog, regg, true_regg, vol_1tp__ml, vol_2tp__ml, vol_out__ml,
            mse_vol, err_vol, dice_5, dice_6, avg_dice__56, dice_1, dice_2, dice_3, dice_4, avg_all_dice]


def label_counts(lbl, real=None, mask1=None, wmh1=None, mask2=None, wmh2=None):
    """The 18 counts of depgan_eval_label_counts from a label map, in NumPy."""
    real = np.zeros(lbl.shape, np.float32) if real is None else np.asarray(real, np.float32).reshape(lbl.shape)
    c = [0, 0, int(np.count_nonzero(lbl > 0))]
    if mask1 is not None and wmh1 is not None:
        c[0] = int(np.count_nonzero(np.multiply(mask1, wmh1)))
    if mask2 is not None and wmh2 is not None:
        c[1] = int(np.count_nonzero(np.multiply(mask2, wmh2)))
    for r, f in [(real == k, lbl == k) for k in (1, 2, 3)] + [(real > 0, lbl > 0),
                                                           ((real == 1) | (real == 2), (lbl == 1) | (lbl == 2))]:
        c += [int(np.count_nonzero(r & f)), int(np.count_nonzero(r)), int(np.count_nonzero(f))]
    return c


def random_maps(seed, shape=(3, 32, 32), p_lbl=(0.55, 0.15, 0.15, 0.15), p_real=(0.55, 0.15, 0.15, 0.15),
                wmh1_rate=0.2, wmh2_rate=0.2):
    rng = np.random.default_rng(seed)
    lbl = rng.choice(4, size=shape, p=p_lbl).astype(np.uint8)
    real = rng.choice(4, size=shape, p=p_real).astype(np.float32)
    m1 = (rng.uniform(size=shape) > 0.1).astype(np.float32)
    m2 = (rng.uniform(size=shape) > 0.1).astype(np.float32)
    w1 = (rng.uniform(size=shape) < wmh1_rate).astype(np.float32)
    w2 = (rng.uniform(size=shape) < wmh2_rate).astype(np.float32)
    return lbl, real, m1, w1, m2, w2


# ---- tests ----

@pytest.mark.parametrize("seed,kw", [
    (0, {}),
    (1, {"p_lbl": (0.7, 0.0, 0.15, 0.15), "p_real": (0.7, 0.0, 0.15, 0.15)}),      # class 1 empty on both sides
    (2, {"p_lbl": (1.0, 0.0, 0.0, 0.0), "p_real": (1.0, 0.0, 0.0, 0.0),            # every class empty
         "wmh1_rate": 0.0, "wmh2_rate": 0.0}),
    (3, {"wmh1_rate": 0.05, "wmh2_rate": 0.3}),                                      # growing volume
    (4, {"wmh1_rate": 0.3, "wmh2_rate": 0.05}),                                      # shrinking, predicted growing
    (5, {"wmh1_rate": 0.6, "wmh2_rate": 0.05}),                                      # shrinking, predicted shrinking
])
def test_label_metrics_match_the_ue_statements(seed, kw):
    vox = 0.9375 * 0.9375 * 4.0
    lbl, real, m1, w1, m2, w2 = random_maps(seed, **kw)
    c = label_counts(lbl, real, m1, w1, m2, w2)
    got = evaluate.label_metrics_from_census(c, vox)
    want = ue_vol_dsc(lbl, real, m1, w1, m2, w2, vox)
    np.testing.assert_array_equal(np.array(got["vol_dsc"], np.float64), np.array(want, np.float64))
    assert got["dice"][5] == got["dice"][2]                              # dice_6 restates dice_3 (UE:681-690)
    assert got["census"] == c and len(c) == evaluate.NCOUNT_LABEL


def test_label_metrics_cover_both_volume_branches():
    vox = 1.0
    rows = []
    for seed, kw in ((3, {"wmh1_rate": 0.05, "wmh2_rate": 0.3}), (4, {"wmh1_rate": 0.3, "wmh2_rate": 0.05}),
                     (5, {"wmh1_rate": 0.6, "wmh2_rate": 0.05})):
        lbl, real, m1, w1, m2, w2 = random_maps(seed, **kw)
        rows.append(evaluate.label_metrics_from_census(label_counts(lbl, real, m1, w1, m2, w2), vox))
    assert rows[0]["prog"] == 1 and rows[0]["regg"] == 0
    assert rows[1]["regg"] == 1 and rows[1]["true_regg"] == 0
    assert rows[2]["regg"] == 1 and rows[2]["true_regg"] == 1 and rows[2]["true_pred"] == 1
    empty = evaluate.label_metrics_from_census([0] * 18, vox)
    assert empty["dice"] == [1.0] * 6 and empty["prog"] == 1 and empty["true_prog"] == 1


@pytest.mark.parametrize("n_class", [0, 128, 2.5, True, "4", None])
def test_to_one_hot_rejects_bad_class_counts(n_class):
    with pytest.raises(ValueError):
        data.to_one_hot(np.zeros((2, 4, 4, 1), np.float32), n_class=n_class)


@pytest.mark.parametrize("shape", [(2, 4, 4, 2), (4, 4), (2, 4, 4, 1, 1), (8,)])
def test_to_one_hot_rejects_bad_shapes(shape):
    with pytest.raises(ValueError):
        data.to_one_hot(np.zeros(shape, np.float32), n_class=4)


def test_uresnet_file_lists(tmp_path):
    stems = ("flair_1tp", "wmh_subtracted_coded_2tp_1tp", "icv_1tp", "sl_cleaned_1tp")
    for stem in stems:
        (tmp_path / ("%s_fold2.txt" % stem)).write_text("".join("/d/%s_%d.nii.gz\n" % (stem, i) for i in range(3)))
    subjects = data.uresnet_file_lists(str(tmp_path), 2)
    assert len(subjects) == 3
    assert subjects[1] == data.UResNetFiles("/d/flair_1tp_1.nii.gz", "/d/wmh_subtracted_coded_2tp_1tp_1.nii.gz",
                                            "/d/icv_1tp_1.nii.gz", "/d/sl_cleaned_1tp_1.nii.gz")
    (tmp_path / "icv_1tp_fold2.txt").write_text("/d/a\n")
    with pytest.raises(ValueError):
        data.uresnet_file_lists(str(tmp_path), 2)


def test_new_entry_points_are_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    declared = set(re.findall(r"\b(depgan_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define DEPGAN_EVAL_LABEL_NCOUNT %d\b" % evaluate.NCOUNT_LABEL, hdr)
    assert re.search(r"#define DEPGAN_ABI_VERSION 3\b", hdr) and _lib.ABI_VERSION == 3
    assert lib.depgan_data_zscore_scratch_floats(0, 4, 4) == 0
    assert lib.depgan_data_zscore_scratch_floats(64, 64, 2) >= 2 * (1024 + 2) + 2
