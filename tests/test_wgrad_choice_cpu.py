"""CPU: the weight-gradient kernel choice (dg_wgrad_choose, csrc/wgrad_select.hip) through depgan_debug_wgrad_choice.

The rule is restated here and held against the export on every tile row of tests/wgrad_plan_cases.py and on every layer
of the two networks at batch 2, 32 x 32 (generator trunk with first_fm 32 and 1 or 2 input channels, the 32 -> 4 head of
the DEP-UResNet, the critics on their 3 B samples), each in all four combinations of the two flags.  The numbers that go
with the kernel are held against depgan_debug_wgrad_plan, the launchers' own chunking, of the same library.
"""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_plan_cases as wc  # noqa: E402

UNSUPPORTED = 3


def rule(KS, Cin, Cout, bf16_pipe, x_bf16):
    """kernel, or None where the choice is refused (the *_supported predicates of wgrad_bf16.hip / wgrad_bf16s.hip)"""
    mfma = Cin % 4 == 0 and Cout % 4 == 0 and Cin >= 8
    if x_bf16:
        return wc.K_BF16S if (KS in (1, 3) and Cin >= 8 and Cin % 8 == 0 and Cout % 4 == 0) else None
    if bf16_pipe and mfma and KS in (1, 3, 5):
        return wc.K_BF16
    return wc.K_F32 if mfma else wc.K_EDGE


def network_shapes(B=2, H=32, W=32, fm=32):
    """(B, H, W, Cin, Cout, KS) of every weight-gradient call of the backward passes (kTrunk, kDis of model.hip)"""
    trunk = [("c", -1, 1), ("c", 1, 1), ("c", 1, 1), ("p",), ("c", 1, 2), ("c", 2, 2), ("c", 2, 2), ("p",), ("c", 2, 3),
             ("c", 3, 3), ("c", 3, 3), ("p",), ("c", 3, 4), ("c", 4, 4), ("c", 4, 4), ("d", 4, 4), ("c", 7, 3), ("c", 3, 3),
             ("c", 3, 3), ("d", 3, 3), ("c", 5, 2), ("c", 2, 2), ("c", 2, 2), ("d", 2, 2), ("c", 3, 1), ("c", 1, 1),
             ("c", 1, 1)]
    out = []
    for nicg in (1, 2):
        h, w = H, W
        for e in trunk:
            if e[0] == "p":
                h, w = h // 2, w // 2
                continue
            ci, co = (nicg if e[1] < 0 else e[1] * fm), e[2] * fm
            out.append((B, h, w, ci, co, 3 if e[0] == "c" else 1))       # a transposed convolution: one 1x1 call per tap
            if e[0] == "d":
                h, w = 2 * h, 2 * w
    out.append((B, H, W, fm, 4, 1))                                      # the 32 -> 4 head (u_backward)
    dis = [(5, 1, 16, 0), (5, 16, 16, 1), (5, 16, 32, 0), (5, 32, 32, 1), (3, 32, 64, 0), (3, 64, 64, 1), (3, 64, 128, 0),
           (3, 128, 128, 1), (3, 128, 256, 0), (3, 256, 256, 0), (3, 256, 256, 0)]
    h, w = H, W
    for k, ci, co, pool in dis:
        out.append((3 * B, h, w, ci, co, k))
        if pool:
            h, w = h // 2, w // 2
    return sorted(set(out))


SHAPES = [(c.name, c.shape) for c in wc.TILE_CASES] + [("net-%d-%dx%d-%d-%d-k%d" % s, s) for s in network_shapes()]


@pytest.mark.parametrize("shape", [s for _, s in SHAPES], ids=[n for n, _ in SHAPES])
def test_choice_is_the_rule_and_its_numbers_are_the_launchers_plan(lib, shape):
    B, H, W, ci, co, k = shape
    for pipe in (0, 1):
        for xh in (0, 1):
            out, plan = (C.c_long * 4)(-7, -7, -7, -7), (C.c_int * 4)()
            want = rule(k, ci, co, pipe, xh)
            status = lib.depgan_debug_wgrad_choice(k, B, H, W, ci, co, pipe, xh, out)
            if want is None:
                assert status == UNSUPPORTED and list(out) == [-7] * 4, (pipe, xh)
                continue
            assert status == 0, (pipe, xh, lib.depgan_last_error())
            assert out[0] == want, (pipe, xh, list(out))
            assert lib.depgan_debug_wgrad_plan(want, k, B, H, W, ci, co, plan) == 0
            assert out[1] == plan[2] and out[1] >= 1
            assert out[2] == out[1] * k * k * ci * co
            assert out[3] == (0 if want == wc.K_EDGE else out[1])


def test_every_row_of_the_case_table_is_chosen_by_the_flags_of_its_entry(lib):
    """a row's kernel is the one its operator entry reaches: bf16 = 0 / 1 of depgan_op_conv2d_wgrad_ex, x in bf16 memory"""
    flags = {wc.K_F32: (0, 0), wc.K_EDGE: (0, 0), wc.K_BF16: (1, 0), wc.K_BF16S: (1, 1)}
    out = (C.c_long * 4)()
    for c in wc.TILE_CASES:
        B, H, W, ci, co, k = c.shape
        assert lib.depgan_debug_wgrad_choice(k, B, H, W, ci, co, *flags[c.kernel], out) == 0 and out[0] == c.kernel, c.name
    assert {rule(s[5], s[3], s[4], 0, 0) for s in network_shapes()} == {wc.K_F32, wc.K_EDGE}   # both networks have edge layers


def test_refusals_write_nothing(lib):
    out = (C.c_long * 4)(-7, -7, -7, -7)
    refused = [
        # (KS, B, H, W, Cin, Cout, bf16_pipe, x_bf16, status)
        (3, 0, 8, 8, 32, 32, 0, 0, 1), (3, 2, 0, 8, 32, 32, 0, 0, 1), (3, 2, 8, -1, 32, 32, 0, 0, 1),     # sizes
        (3, 2, 8, 8, 0, 32, 0, 0, 1), (3, 2, 8, 8, 32, 0, 0, 0, 1),
        (3, 2, 8, 8, 32, 32, 2, 0, 1), (3, 2, 8, 8, 32, 32, 0, -1, 1),                                     # flags
        (3, 2, 8, 8, 36, 32, 0, 1, 3), (5, 2, 8, 8, 32, 32, 1, 1, 3), (3, 2, 8, 8, 2, 32, 0, 1, 3),        # x_bf16, uncovered
        (7, 2, 8, 8, 32, 32, 0, 0, 3), (7, 2, 8, 8, 32, 32, 1, 0, 3),                                      # the launcher's own
        (1, 2, 8, 8, 1, 16, 0, 0, 3), (3, 2, 8, 8, 4, 32, 0, 0, 3), (3, 2, 8, 8, 2, 68, 1, 0, 3),
    ]
    for *args, status in refused:
        assert lib.depgan_debug_wgrad_choice(*args, out) == status, args
        assert lib.depgan_last_error()
    assert lib.depgan_debug_wgrad_choice(3, 2, 8, 8, 32, 32, 0, 0, None) == 1
    assert list(out) == [-7] * 4
