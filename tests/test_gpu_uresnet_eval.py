"""GPU: the DEP-UResNet data step (UT:434-566) and evaluation (UE:496-717) through the C ABI, against NumPy
restatements of the reference statements.  Elementwise float32 work is bit-exact, counts are exact integers, the
z-score statistics are float64 sums rounded to float32."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_uresnet_eval_cpu import convert_from_1hot, label_counts, ue_vol_dsc  # noqa: E402

pytestmark = pytest.mark.gpu


def data_prep(vol):
    """GT:106-118 / UE:89-104: (X, Y, Z) -> (Z, X, Y, 1) float32 slices."""
    return np.array([vol[:, :, z] for z in range(vol.shape[2])], dtype='float32')[..., None]


def ut_brain_flair(f1, icv1, sl1):
    brain = np.multiply(data_prep(f1), data_prep(icv1))
    if sl1 is not None:
        brain = np.multiply(brain, 1 - data_prep(sl1))
    return brain


def nan_to_num_zscore(brain, mean32, std32):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.nan_to_num((brain - np.float32(mean32)) / np.float32(std32))


def convert_to_1hot(label, n_class):
    """UT:209-222 (int16 in the reference; 0 / 1 either way)."""
    label_flat = label.flatten().astype(int)
    n_data = len(label_flat)
    label_1hot = np.zeros((n_data, n_class), dtype='int16')
    label_1hot[range(n_data), label_flat] = 1
    return label_1hot.reshape(label.shape[:4] + (n_class,))


def _vols(seed, X, Y, Z):
    rng = np.random.default_rng(seed)
    f1 = rng.uniform(0, 3000, size=(X, Y, Z)).astype(np.int16)
    icv = (rng.uniform(size=(X, Y, Z)) > 0.3).astype(np.uint8)
    sl = (rng.uniform(size=(X, Y, Z)) > 0.9).astype(np.uint8)
    code = rng.choice(4, size=(X, Y, Z), p=(0.6, 0.1, 0.15, 0.15)).astype(np.uint8)
    return f1, icv, sl, code


@pytest.mark.parametrize("shape,with_sl", [((64, 64, 5), True), ((64, 64, 5), False), ((40, 50, 3), True)])
def test_zscore_stats_and_bits(shape, with_sl):
    import torch
    from dep_gan_im_amd import data as D
    f1, icv, sl, _ = _vols(sum(shape), *shape)
    sl = sl if with_sl else None
    out, stats = D.zscore_flair(f1, icv, sl, with_stats=True)
    out2, stats2 = D.zscore_flair(f1, icv, sl, with_stats=True)
    torch.cuda.synchronize()
    got, (m32, s32) = out.cpu().numpy(), stats.cpu().numpy()
    brain = ut_brain_flair(f1, icv, sl)
    b64 = brain.astype(np.float64)
    assert abs(m32 / b64.mean() - 1) < 1e-6 and abs(s32 / b64.std() - 1) < 1e-6
    assert got.shape == brain.shape and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), nan_to_num_zscore(brain, m32, s32).view(np.uint32))
    # second run: identical bits (fixed-order reductions, no float atomics)
    assert np.array_equal(out2.cpu().numpy().view(np.uint32), got.view(np.uint32))
    assert np.array_equal(stats2.cpu().numpy().view(np.uint32), stats.cpu().numpy().view(np.uint32))


def test_zscore_of_an_empty_brain_is_zero():
    import torch
    from dep_gan_im_amd import data as D
    f1, icv, sl, _ = _vols(7, 64, 64, 4)
    out, stats = D.zscore_flair(np.zeros_like(f1), icv, sl, with_stats=True)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert not np.isnan(o).any() and np.array_equal(o, np.zeros_like(o))
    assert stats.cpu().numpy().tolist() == [0.0, 0.0]


def test_mask_slices_and_onehot_bit_exact():
    import torch
    from dep_gan_im_amd import _lib
    from dep_gan_im_amd import data as D
    f1, icv, sl, code = _vols(11, 64, 48, 3)
    wmh = (np.random.default_rng(3).uniform(size=code.shape) > 0.8).astype(np.float32)
    cases = [(code, icv, sl), (code, icv, None), (icv, None, sl), (wmh, icv, sl), (f1, None, None)]
    for vol, m_a, s in cases:
        want = data_prep(vol)
        if m_a is not None:
            want = np.multiply(want, data_prep(m_a))
        if s is not None:
            want = np.multiply(want, 1 - data_prep(s))
        got = D.mask_slices(vol, m_a, s).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # UT:563-566: astype(int) truncates toward zero, then one-hot
    coded = D.mask_slices(code, icv, sl)
    coded_np = coded.cpu().numpy()
    coded_np[0, :4, 0, 0] = [2.7, -0.5, 0.999, 3.25]
    oh = D.to_one_hot(torch.from_numpy(coded_np).cuda(), 4)
    torch.cuda.synchronize()
    want = np.squeeze(convert_to_1hot(coded_np.astype(int), 4)).astype(np.float32)
    assert tuple(oh.shape) == coded_np.shape[:3] + (4,) and np.array_equal(oh.cpu().numpy(), want)
    for bad in (4.0, -1.0, np.nan, 1e9):
        c = coded_np.copy()
        c[1, 5, 7, 0] = bad
        with pytest.raises(_lib.DepganError):
            D.to_one_hot(c, 4)


def _probs(seed, n=3, img=64, C=4):
    rng = np.random.default_rng(seed)
    p = rng.uniform(size=(n, img, img, C))
    p = p / p.sum(-1, keepdims=True)
    # ties: two maxima (the first wins), all four equal (label 0), fully masked pixels (all zero: label 0)
    p[0, 0, :8] = [0.1, 0.4, 0.4, 0.1]
    p[0, 1, :8] = [0.1, 0.2, 0.35, 0.35]
    p[0, 2, :8] = 0.25
    mask2 = (rng.uniform(size=(n, img, img)) > 0.15).astype(np.float32)
    mask2[0, :3, :8] = 1.0
    p = p * mask2[..., None]
    code = rng.choice(4, size=(n, img, img), p=(0.4, 0.2, 0.2, 0.2)).astype(np.float32)
    m1 = (rng.uniform(size=(n, img, img)) > 0.1).astype(np.float32)
    w1 = (rng.uniform(size=(n, img, img)) > 0.7).astype(np.float32)
    w2 = (rng.uniform(size=(n, img, img)) > 0.6).astype(np.float32)
    return p, code, m1, w1, mask2, w2


def test_label_census_exact():
    import torch
    from dep_gan_im_amd import evaluate as EV
    p, code, m1, w1, m2, w2 = _probs(5)
    lbl = np.argmax(p, axis=-1)
    assert (lbl[0, 0, :8] == 1).all() and (lbl[0, 1, :8] == 2).all() and (lbl[0, 2, :8] == 0).all()
    c, labels = EV.label_census(p, code, m1, w1, m2, w2, return_labels=True)
    torch.cuda.synchronize()
    assert np.array_equal(labels.cpu().numpy(), lbl.astype(np.int8))
    assert (labels.cpu().numpy()[m2 == 0] == 0).all()
    assert c == label_counts(lbl, code, m1, w1, m2, w2)
    # absent optional arrays
    assert EV.label_census(p) == label_counts(lbl)
    assert EV.label_census(p, code, None, w1, m2, None) == label_counts(lbl, code)
    # the metrics row equals UE's statements on the same arrays
    vox = 0.9375 * 0.9375 * 4.0
    m = EV.uresnet_metrics(p, code, m1, w1, m2, w2, vox)
    np.testing.assert_array_equal(np.array(m["vol_dsc"]), np.array(ue_vol_dsc(convert_from_1hot(p), code, m1, w1,
                                                                                m2, w2, vox)))
    with pytest.raises(ValueError):
        EV.label_census(p, code[:, :32])


def _ue_mean(netG, x, mask, n_repeat, seed):
    """UE:553-564: float64 np.zeros of the mask's shape += predict * mask (broadcast over the channels)."""
    rng = np.random.RandomState(seed)
    icv_and_sl_mask_2tp = mask[..., None]
    output_img_pred_mean = np.zeros(icv_and_sl_mask_2tp.shape)
    for _ in range(n_repeat):
        noise = rng.normal(size=(len(x), 32, 1)).astype('float32')
        output_img_pred = netG.predict([x, noise])
        output_img_pred = np.multiply(output_img_pred, icv_and_sl_mask_2tp)
        output_img_pred_mean = output_img_pred_mean + output_img_pred
    return output_img_pred_mean / float(n_repeat)


def test_predict_mean_four_channels():
    import torch
    import dep_gan_im_amd as dg
    from dep_gan_im_amd import evaluate as EV
    rng = np.random.default_rng(9)
    x = rng.standard_normal((3, 64, 64, 1)).astype(np.float32)
    mask = (rng.uniform(size=(3, 64, 64)) > 0.2).astype(np.float32)
    netG = dg.Gen_UNet2D((64, 64, 1), (32, 1), 32, 4, seed=2)
    got = EV.predict_mean(netG, x, n_repeat=3, mask=mask, rng=np.random.RandomState(4))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (3, 64, 64, 4) and got.dtype == torch.float64
    g = got.cpu().numpy()
    want = _ue_mean(netG, x, mask, 3, 4)
    np.testing.assert_allclose(g, want, rtol=1e-14, atol=1e-300)
    _, labels = EV.label_census(got, return_labels=True)
    assert np.array_equal(labels.cpu().numpy(), np.argmax(g, -1).astype(np.int8))
    assert np.array_equal(np.argmax(g, -1), convert_from_1hot(want))
    # the single-channel path: (n, H, W), the GE statements
    net1 = dg.Gen_UNet2D((64, 64, 1), seed=3)
    got1 = EV.predict_mean(net1, x, n_repeat=2, mask=mask, rng=np.random.RandomState(6)).cpu().numpy()
    want1 = _ue_mean(net1, x, mask, 2, 6)
    assert got1.shape == (3, 64, 64)
    np.testing.assert_allclose(got1, want1[..., 0], rtol=1e-14, atol=1e-300)


def test_uresnet_end_to_end_from_files(tmp_path):
    """UT data lines -> split / shuffle -> one-hot -> fit, then UE's evaluation on a subject, against the NumPy
    statements applied to the same files; the written maps read back through nifti.load."""
    import torch
    import dep_gan_im_amd as dg
    from dep_gan_im_amd import data as D
    from dep_gan_im_amd import evaluate as EV
    from dep_gan_im_amd import nifti
    X = Y = 64
    Z = 4
    affine = np.diag([0.9375, 0.9375, 4.0, 1.0])
    affine[:3, 3] = [-30.0, 12.0, 5.0]
    names = ["s0", "s1", "s2", "s3"]
    lists = {k: [] for k in ("flair_1tp", "wmh_subtracted_coded_2tp_1tp", "icv_1tp", "sl_cleaned_1tp", "wmh_1tp",
                             "wmh_2tp", "icv_2tp", "sl_cleaned_2tp")}
    vols = {}
    for i, nm in enumerate(names):
        f1, icv1, sl1, code = _vols(100 + i, X, Y, Z)
        _, icv2, sl2, _ = _vols(200 + i, X, Y, Z)
        rng = np.random.default_rng(300 + i)
        w1 = (rng.uniform(size=(X, Y, Z)) > 0.8).astype(np.uint8)
        w2 = (rng.uniform(size=(X, Y, Z)) > 0.75).astype(np.uint8)
        v = {"flair_1tp": f1, "wmh_subtracted_coded_2tp_1tp": code, "icv_1tp": icv1, "sl_cleaned_1tp": sl1,
             "wmh_1tp": w1, "wmh_2tp": w2, "icv_2tp": icv2, "sl_cleaned_2tp": sl2}
        for k, a in v.items():
            p = str(tmp_path / ("%s_%s.nii.gz" % (nm, k)))
            missing = (k == "sl_cleaned_1tp" and i == 1) or (k == "flair_1tp" and i == 3)
            if not missing:
                nifti.save(p, a, affine)
            lists[k].append(p)
        vols[nm] = v
    for k, v in lists.items():
        (tmp_path / ("%s_fold1.txt" % k)).write_text("".join(p + "\n" for p in v))

    # ---- UT:434-566 ----
    subjects = D.uresnet_file_lists(str(tmp_path), 1)
    flair, coded = D.load_uresnet_training_set(subjects)
    torch.cuda.synchronize()
    want_f, want_c = [], []
    for i in range(3):                        # s3's FLAIR is missing: skipped; s1 has no stroke-lesion file
        v = vols[names[i]]
        sl1 = v["sl_cleaned_1tp"] if i != 1 else None
        brain = ut_brain_flair(v["flair_1tp"], v["icv_1tp"], sl1)
        _, st = D.zscore_flair(v["flair_1tp"], v["icv_1tp"], sl1, with_stats=True)
        want_f.append(nan_to_num_zscore(brain, *st.cpu().numpy()))
        c = np.multiply(data_prep(v["wmh_subtracted_coded_2tp_1tp"]), data_prep(v["icv_1tp"]))
        want_c.append(c if sl1 is None else np.multiply(c, 1 - data_prep(sl1)))
    assert np.array_equal(flair.cpu().numpy(), np.concatenate(want_f, 0))
    assert np.array_equal(coded.cpu().numpy(), np.concatenate(want_c, 0))
    ftr, fval, ctr, cval = D.split_and_shuffle(flair, coded, rng=np.random.RandomState(1))
    lab_tr = D.to_one_hot(ctr, 4)
    assert np.array_equal(lab_tr.cpu().numpy(),
                          np.squeeze(convert_to_1hot(ctr.cpu().numpy().astype(int), 4)).astype(np.float32))
    netG = dg.Gen_UNet2D((X, Y, 1), (32, 1), 32, 4, seed=1)
    np.random.seed(0)
    for _ in range(2):
        noise = np.random.normal(size=(len(ftr), 32, 1)).astype('float32')
        h = netG.fit([ftr, noise], lab_tr, epochs=1, batch_size=4, verbose=0)
        assert np.isfinite(h.history["loss"][0])

    # ---- UE:496-717 on subject s0 ----
    v = vols["s0"]
    brain_flair_1tp, st = D.zscore_flair(v["flair_1tp"], v["icv_1tp"], v["sl_cleaned_1tp"], with_stats=True)
    brain_wmh_1tp = D.mask_slices(v["wmh_1tp"], v["icv_1tp"], v["sl_cleaned_1tp"])
    brain_wmh_2tp = D.mask_slices(v["wmh_2tp"], v["icv_2tp"], v["sl_cleaned_2tp"])
    brain_cod_2tp = D.mask_slices(v["wmh_subtracted_coded_2tp_1tp"], v["icv_2tp"])
    mask_1tp = D.mask_slices(v["icv_1tp"], None, v["sl_cleaned_1tp"])
    mask_2tp = D.mask_slices(v["icv_2tp"], None, v["sl_cleaned_2tp"])
    vox = float(np.prod(np.abs(np.diag(affine)[:3])))
    prob = EV.predict_mean(netG, brain_flair_1tp, n_repeat=2, mask=mask_2tp, rng=np.random.RandomState(8))
    m = EV.uresnet_metrics(prob, brain_cod_2tp, mask_1tp, brain_wmh_1tp, mask_2tp, brain_wmh_2tp, vox)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    paths = EV.save_uresnet_maps(str(out_dir), "s0", m["labels"], prob, affine)
    torch.cuda.synchronize()
    # the NumPy statements on the files
    i1, s1 = data_prep(v["icv_1tp"]), 1 - data_prep(v["sl_cleaned_1tp"])
    i2, s2 = data_prep(v["icv_2tp"]), 1 - data_prep(v["sl_cleaned_2tp"])
    n_flair = nan_to_num_zscore(ut_brain_flair(v["flair_1tp"], v["icv_1tp"], v["sl_cleaned_1tp"]), *st.cpu().numpy())
    assert np.array_equal(brain_flair_1tp.cpu().numpy(), n_flair)
    n_wmh_1tp = np.multiply(np.multiply(data_prep(v["wmh_1tp"]), i1), s1)
    n_wmh_2tp = np.multiply(np.multiply(data_prep(v["wmh_2tp"]), i2), s2)
    n_cod_2tp = np.multiply(data_prep(v["wmh_subtracted_coded_2tp_1tp"]), i2)
    n_mask_1tp, n_mask_2tp = np.multiply(i1, s1), np.multiply(i2, s2)
    for got, want in ((brain_wmh_1tp, n_wmh_1tp), (brain_wmh_2tp, n_wmh_2tp), (brain_cod_2tp, n_cod_2tp),
                      (mask_1tp, n_mask_1tp), (mask_2tp, n_mask_2tp)):
        assert np.array_equal(got.cpu().numpy(), want)
    n_prob = _ue_mean(netG, n_flair, n_mask_2tp[..., 0], 2, 8)
    np.testing.assert_allclose(prob.cpu().numpy(), n_prob, rtol=1e-14, atol=1e-300)
    n_lbl = convert_from_1hot(n_prob)
    assert np.array_equal(m["labels"].cpu().numpy(), n_lbl.astype(np.int8))
    want_row = ue_vol_dsc(n_lbl, n_cod_2tp, n_mask_1tp, n_wmh_1tp, n_mask_2tp, n_wmh_2tp, vox)
    np.testing.assert_array_equal(np.array(m["vol_dsc"]), np.array(want_row))
    # UE:705-717: the maps are back in file orientation, int8 / float32, with the input's affine
    assert [os.path.basename(p) for p in paths] == ["s0_cls_map.nii.gz"] + ["s0_prb_map_c%d.nii.gz" % c
                                                                             for c in range(4)]
    cls = nifti.load(paths[0])
    assert cls.image.dtype == np.int8 and cls.image.shape == (X, Y, Z)
    assert np.array_equal(cls.image, np.transpose(n_lbl, (1, 2, 0)).astype(np.int8))
    np.testing.assert_allclose(cls.affine, affine, rtol=0, atol=1e-6)
    for c in range(4):
        im = nifti.load(paths[1 + c]).image
        assert im.dtype == np.float32 and im.shape == (X, Y, Z)
        assert np.array_equal(im, np.transpose(n_prob[..., c], (1, 2, 0)).astype(np.float32))
