"""CPU: the epilogue classes of the 5x5 kernels (igemm_ws5_kernel<32,8> / <16,16>, the persistent
igemm_conv_kernel<32,5,8,25,true> / <16,5,16,25,true>; csrc/common.h kConv5ClassMask, csrc/conv_select.hip
dg_conv5_epi_class) -- the host selector, the process-wide switch it shares with the Winograd kernel, and the launch a
class is taken IN: the classes are bodies inside the one kernel, so the choice entry answers the same kernel name, grid,
block and LDS size whether the switch is on or off.  No HIP call anywhere."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import pytest

from dep_gan_im_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = _lib._K
BIAS, AFFINE, FILM, RELU, PRE, RES, MASK, POOL, ACCUM, HEAD = (
    K["DEPGAN_EPF_" + n] for n in ("BIAS", "AFFINE", "FILM", "RELU", "PRE", "RES", "MASK", "POOL", "ACCUM", "HEAD"))
# what the model launches on the 5x5 kernels (model.hip: d_forward, d_backward_chain, the u-forward of critic_enqueue)
TABLE = {BIAS | RELU: 1, BIAS | RELU | POOL: 2, MASK: 3, 0: 4}


@pytest.fixture()
def switch(lib):
    """the switch on, and restored afterwards"""
    before = lib.depgan_get_epilogue_classes()
    assert lib.depgan_set_epilogue_classes(1) == 0
    yield lib
    assert lib.depgan_set_epilogue_classes(before) == 0


def test_entry_is_exported_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    declared = set(re.findall(r"\b(depgan_[a-z0-9_]+)\s*\(", hdr))
    name = "depgan_conv5_epilogue_class"
    assert name in _lib.EXPORTS and name in declared and hasattr(lib, name)
    assert lib.depgan_conv5_epilogue_class.argtypes == [C.c_uint] and lib.depgan_conv5_epilogue_class.restype is C.c_int
    assert "DEPGAN_ABI_VERSION 3" in hdr and lib.depgan_abi_version() == 3      # an additive entry: the ABI stays


def test_the_four_flag_sets_have_ids_one_to_four(switch):
    lib = switch
    for flags, want in TABLE.items():
        assert lib.depgan_conv5_epilogue_class(flags) == want, flags
        assert lib.depgan_conv5_epilogue_class(flags) == want              # a pure function: asked twice, the same answer


def test_every_other_flag_set_takes_the_run_time_body(switch):
    lib = switch
    # accumulate, the affine, FiLM and res first: what the generator's layers and the operator entries combine
    for flags in (ACCUM, MASK | ACCUM, BIAS | RELU | ACCUM, BIAS | AFFINE | RELU, BIAS | AFFINE | RELU | POOL,
                  BIAS | AFFINE | FILM | RELU | RES, BIAS | RELU | FILM, RES, RES | MASK, BIAS | RELU | RES,
                  BIAS, RELU, POOL, BIAS | POOL, RELU | POOL, MASK | POOL, BIAS | RELU | MASK, BIAS | RELU | PRE, PRE,
                  BIAS | RELU | HEAD, HEAD):
        assert lib.depgan_conv5_epilogue_class(flags) == 0, flags
    # and the whole space: exactly the four sets of the table are classes
    bits = (BIAS, AFFINE, FILM, RELU, PRE, RES, MASK, POOL, ACCUM, HEAD)
    for n in range(len(bits) + 1):
        for sub in itertools.combinations(bits, n):
            flags = sum(sub)
            assert lib.depgan_conv5_epilogue_class(flags) == TABLE.get(flags, 0), flags


def test_switch_off_answers_zero(switch):
    lib = switch
    assert lib.depgan_set_epilogue_classes(0) == 0 and lib.depgan_get_epilogue_classes() == 0
    for flags in TABLE:
        assert lib.depgan_conv5_epilogue_class(flags) == 0
    assert lib.depgan_set_epilogue_classes(1) == 0
    assert lib.depgan_conv5_epilogue_class(MASK) == 3


def test_flags_outside_the_mask_are_refused(switch):
    lib = switch
    for flags in (1024, MASK | 4096, 1 << 31):
        assert lib.depgan_conv5_epilogue_class(flags) == -1 and b"conv5_epilogue_class" in lib.depgan_last_error()


def test_switch_is_initialised_from_the_environment():
    code = ("from dep_gan_im_amd import _lib; lib = _lib.load(); "
            "print(lib.depgan_get_epilogue_classes(), lib.depgan_conv5_epilogue_class(%d))" % MASK)
    for val, want in (("0", "0 0"), (None, "1 3")):
        env = {k: v for k, v in os.environ.items() if k != "DEPGAN_EPI_CLASSES"}
        if val is not None:
            env["DEPGAN_EPI_CLASSES"] = val
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip().splitlines()[-1] == want


# (KS, planN, B, H, W, Cin, Cout) of 5x5 launches: the critics' layers at both batches of the canonical step, the
# backward-data forms, and sizes below the persistent and weight-stationary thresholds
LAUNCHES = [(5, 96, 96, 256, 256, 16, 16), (5, 96, 32, 256, 256, 16, 16), (5, 96, 96, 128, 128, 16, 32),
            (5, 96, 32, 128, 128, 16, 32), (5, 96, 96, 128, 128, 32, 32), (5, 96, 32, 128, 128, 32, 32),
            (5, 96, 96, 128, 128, 32, 16), (5, 96, 32, 128, 128, 32, 16), (5, 96, 2, 16, 16, 16, 16),
            (5, 96, 3, 20, 36, 32, 32), (5, 96, 6, 256, 256, 16, 16), (5, 96, 40, 64, 64, 24, 16)]


def choice(lib, case, flags):
    name, out = C.create_string_buffer(b"untouched", 64), (C.c_long * 5)(*[-7] * 5)
    KS, planN, *rest = case
    status = lib.depgan_debug_conv_choice(0, 0, 1, KS, planN, *rest, flags, 0, 0, name, 64, out)
    return status, name.value.decode(), list(out)


@pytest.mark.parametrize("case", LAUNCHES, ids=lambda c: "x".join(map(str, c[2:])))
def test_choice_is_the_same_launch_with_the_switch_on_and_off(switch, case):
    lib = switch
    seen = set()
    for flags in list(TABLE) + [BIAS | RELU | ACCUM, MASK | ACCUM]:
        if flags & POOL and (case[3] | case[4]) & 1:
            continue
        assert lib.depgan_set_epilogue_classes(1) == 0
        on = choice(lib, case, flags)
        assert lib.depgan_set_epilogue_classes(0) == 0
        off = choice(lib, case, flags)
        assert on[0] == 0 and on == off, (flags, on, off)
        assert re.fullmatch(r"igemm_ws5_kernel<(32,8|16,16)>|igemm_conv_kernel<(32,5,8|16,5,16),25,(true|false)>", on[1]), on[1]
        seen.add(on[1])
    assert len(seen) == 1                                   # nor does the flag set change the kernel


def test_the_cases_reach_all_four_kernels(switch):
    lib = switch
    names = {choice(lib, case, MASK)[1] for case in LAUNCHES}
    assert {"igemm_ws5_kernel<32,8>", "igemm_ws5_kernel<16,16>", "igemm_conv_kernel<32,5,8,25,true>",
            "igemm_conv_kernel<16,5,16,25,true>"} <= names, names
