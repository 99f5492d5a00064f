"""CPU: the table of tests/rect_cases.py against the library's own kernel choice, so that a later change of a threshold
cannot quietly turn its rows into repeats of the square power-of-two sizes.

Per row: which of the generator's three transposed convolutions take the fused weight-gradient kernel
(depgan_debug_wgrad_plan with kernel DG_WG_DECONV answers "not covered" where model.hip deconv_wgrad_all falls back to the
column-sum pass and four per-tap launches), which launch the fallback forward and backward-data take
(depgan_debug_conv_choice: the four taps grouped, gathered K), and which of the critics' 3x3 layers are Winograd in forward
and backward-data (depgan_debug_conv_choice as build_critics plans them, and depgan_op_conv3x3_wino_kernel_name).  The fused
forward kernel has no host-only export: its rule (dg_deconv_fwd_supported) is restated here, and test_gpu_rect_model.py reads
the kernel names of a real pass from the profile.
"""
import ctypes as C

import pytest

import rect_cases as RC
from dep_gan_im_amd import _lib

K = _lib._K
BIAS, AFFINE, RELU, MASK, POOL = (K["DEPGAN_EPF_" + n] for n in ("BIAS", "AFFINE", "RELU", "MASK", "POOL"))
BAR = BIAS | AFFINE | RELU
WG_DECONV, OK, UNSUPPORTED = 4, 0, 3


def pow2(v):
    return v >= 1 and not v & (v - 1)


def conv_choice(lib, KS, planN, B, H, W, Cin, Cout, flags, groups=0, runs=0):
    name, out = C.create_string_buffer(64), (C.c_long * 5)()
    status = lib.depgan_debug_conv_choice(0, 0, 1, KS, planN, B, H, W, Cin, Cout, flags, groups, runs, name, 64, out)
    return status, name.value.decode()


@pytest.mark.parametrize("case", RC.CASES, ids=RC.IDS)
def test_deconv_levels_take_the_kernels_the_table_says(lib, case):
    plan = (C.c_int * 4)()
    for name in RC.DECONVS:
        div, ch = RC.DECONV_LEVEL[name]
        h, w = case.H // div, case.W // div
        assert case.H % 16 == 0 and case.W % 16 == 0
        # weight gradient: the fused kernel where the table says so, "not covered" elsewhere
        status = lib.depgan_debug_wgrad_plan(WG_DECONV, 1, case.B, h, w, ch, ch, plan)
        assert status == (OK if name in case.fused_wgrad else UNSUPPORTED), (name, h, w, status, lib.depgan_last_error())
        # forward: dg_deconv_fwd_supported restated (the views of a context are dense and aligned)
        fwd = pow2(h) and pow2(w) and w >= 8 and (case.B * h * w) % 32 == 0
        assert fwd == (name in case.fused_fwd), (name, h, w)
        # the fallbacks exist for every level: the four taps as one grouped 1x1 launch, backward-data with gathered K
        status, kernel = conv_choice(lib, 1, 0, case.B, h, w, ch, ch, BAR, groups=4)
        assert status == OK and kernel.startswith("igemm_conv_kernel<32,1,"), (name, status, kernel)
        status, kernel = conv_choice(lib, 1, 0, case.B, h, w, 4 * ch, ch, MASK, runs=4)
        assert status == OK and kernel.startswith("igemm_conv_kernel<32,1,"), (name, status, kernel)
        # and the per-tap weight gradient of the fallback is the general fp32 slab kernel
        out = (C.c_long * 4)()
        assert lib.depgan_debug_wgrad_choice(1, case.B, h, w, ch, ch, 0, 0, out) == OK and out[0] == 0, (name, list(out))


@pytest.mark.parametrize("case", RC.CASES, ids=RC.IDS)
def test_critic_3x3_layers_take_the_kernels_the_table_says(lib, case):
    buf = C.create_string_buffer(64)
    for name in RC.CRITIC_3X3:
        ci, co, div = RC.CRITIC_LEVEL[name]
        h, w = case.H // div, case.W // div
        pool = POOL if name in ("dis_3", "dis_5") else 0
        want = name in case.wino
        for batch in (3 * case.B, case.B):                                   # [real | fake | mixed], and one of them
            for cin, cout, flags in ((ci, co, BIAS | RELU | pool), (co, ci, MASK), (co, ci, 0)):   # forward, backward-data
                status, kernel = conv_choice(lib, 3, 96, batch, h, w, cin, cout, flags)
                assert status == OK, (name, lib.depgan_last_error())
                assert kernel.startswith("wino_conv_kernel<") == want, (name, h, w, kernel)
                assert want or kernel.startswith("igemm_conv_kernel<32,3,"), (name, h, w, kernel)
                status = lib.depgan_op_conv3x3_wino_kernel_name(flags, batch, h, w, cin, cout, buf, 64)
                assert status == (OK if want else UNSUPPORTED), (name, h, w, status)
                assert not want or buf.value.decode() == kernel, (name, kernel, buf.value)


def test_generator_3x3_layers_stay_winograd_at_every_row(lib):
    """the generator's levels are H, H/2, H/4, H/8 of a multiple of 16: all even, so what differs between the rows is the
    deconvs and the critic bottom, not the generator's convolutions"""
    for case in RC.CASES:
        for div, ch in ((1, 32), (2, 64), (4, 96), (8, 128)):
            status, kernel = conv_choice(lib, 3, 32, case.B, case.H // div, case.W // div, ch, ch, BAR)
            assert status == OK and kernel.startswith("wino_conv_kernel<"), (case.name, div, kernel)


def test_the_table_reaches_every_branch():
    """one row with all three deconvs on the fallback, one with all three fused, one mixed-kernel critic pass, one
    all-Winograd critic pass off the square, H > W and H < W, and an odd batch"""
    assert any(c.fused_fwd == () and c.fused_wgrad == () for c in RC.CASES)
    assert any(c.fused_fwd == RC.DECONVS and c.fused_wgrad == RC.DECONVS and c.H != c.W for c in RC.CASES)
    assert any(0 < len(c.wino) < len(RC.CRITIC_3X3) for c in RC.CASES)
    assert any(c.wino == RC.CRITIC_3X3 and c.fused_fwd == () for c in RC.CASES)
    assert any(c.H > c.W for c in RC.CASES) and any(c.H < c.W for c in RC.CASES)
    assert any(c.B % 2 for c in RC.CASES)
    assert all(c.H != c.W for c in RC.CASES)
    assert len({c.name for c in RC.CASES}) == len(RC.CASES)


def test_square_power_of_two_sizes_reach_none_of_it(lib):
    """the sizes every other whole-network test uses: all fused, all Winograd"""
    plan = (C.c_int * 4)()
    for img in (64, 128, 256):
        for name in RC.DECONVS:
            div, ch = RC.DECONV_LEVEL[name]
            assert lib.depgan_debug_wgrad_plan(WG_DECONV, 1, 2, img // div, img // div, ch, ch, plan) == OK
        for name in RC.CRITIC_3X3:
            ci, co, div = RC.CRITIC_LEVEL[name]
            status, kernel = conv_choice(lib, 3, 96, 6, img // div, img // div, ci, co, BIAS | RELU)
            assert status == OK and kernel.startswith("wino_conv_kernel<"), (img, name, kernel)


def test_init_critic_takes_a_pair_and_keeps_the_square_draws():
    import numpy as np
    from oracle import depgan_oracle as O
    a, b, c = O.init_critic(7, bias_std=0.05, img=64), O.init_critic(7, bias_std=0.05, img=(64, 64)), \
        O.init_critic(7, bias_std=0.05, img=64, width=64)
    assert all(np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]) for k in a)
    r, s = O.init_critic(7, bias_std=0.05, img=(48, 80)), O.init_critic(7, bias_std=0.05, img=48, width=80)
    assert r["dense_1/kernel"].shape == (15, 1) and all(np.array_equal(r[k], s[k]) for k in r)
    assert all(np.array_equal(a[k], r[k]) for k in a if not k.startswith("dense_1"))     # the trunk's draws come first
