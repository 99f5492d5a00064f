"""CPU: the epilogue classes of the Winograd 3x3 kernel (csrc/igemm_wino.hip) -- the host selector that maps a flag set
of the fused epilogue to the instantiation a launch takes, the process-wide switch, and the refusals of the new entries,
all without a GPU (none of these makes a HIP call)."""
import ctypes as C
import os
import re

import pytest

from dep_gan_im_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = _lib._K
BIAS, AFFINE, FILM, RELU, PRE, RES, MASK, POOL, ACCUM, HEAD = (
    K["DEPGAN_EPF_" + n] for n in ("BIAS", "AFFINE", "FILM", "RELU", "PRE", "RES", "MASK", "POOL", "ACCUM", "HEAD"))
BAR = BIAS | AFFINE | RELU
FILM_LAYER = BAR | FILM | RES
# what the model launches on the Winograd kernel (model.hip: g_forward + g_layer_epilogue, g_conv_bn_bwd, d_forward,
# d_backward_chain, the u-forward of critic_enqueue), by form: 0 the 8-row kernel, 1 the fused-head kernel
TABLE = {
    0: {"g_conv": BAR, "g_conv_pool": BAR | POOL,
        "film": FILM_LAYER, "film_pre": FILM_LAYER | PRE,      # a pool only ever follows a plain conv layer (gen_1 / 3 / 5)
        "bwd_join": RES | MASK, "bwd_mask": MASK, "bwd_plain": 0,
        "critic": BIAS | RELU, "critic_pool": BIAS | RELU | POOL},
    1: {"head": BAR | HEAD},
}
NAMES = ["depgan_set_epilogue_classes", "depgan_get_epilogue_classes", "depgan_wino_epilogue_class",
         "depgan_op_conv3x3_wino_kernel_name"]


@pytest.fixture()
def switch(lib):
    """the switch on, and restored afterwards"""
    before = lib.depgan_get_epilogue_classes()
    assert lib.depgan_set_epilogue_classes(1) == 0
    yield lib
    assert lib.depgan_set_epilogue_classes(before) == 0


def test_entries_are_exported_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    declared = set(re.findall(r"\b(depgan_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in _lib.EXPORTS and name in declared and hasattr(lib, name), name
    assert lib.depgan_get_epilogue_classes.argtypes == [] and lib.depgan_wino_epilogue_class.argtypes == [C.c_uint, C.c_int]
    assert "DEPGAN_ABI_VERSION 3" in hdr and lib.depgan_abi_version() == 3      # additive entries: the ABI stays
    assert K["DEPGAN_EPF_ALL"] == BIAS | AFFINE | FILM | RELU | PRE | RES | MASK | POOL | ACCUM | HEAD == 1023


def test_every_set_of_the_table_has_a_class_of_its_own(switch):
    lib = switch
    ids = {}
    for form, sets in TABLE.items():
        for name, flags in sets.items():
            ids[(form, name)] = lib.depgan_wino_epilogue_class(flags, form)
            assert ids[(form, name)] > 0, (form, name)
    assert len(set(ids.values())) == len(ids) == 10, ids              # distinct sets, distinct ids
    # the id does not depend on anything but (flags, form): asked twice, the same answer
    for (form, name), i in ids.items():
        assert lib.depgan_wino_epilogue_class(TABLE[form][name], form) == i


def test_sets_outside_the_table_take_the_generic_kernel(switch):
    lib = switch
    for flags in (BAR | ACCUM, ACCUM, MASK | ACCUM, BIAS, BIAS | AFFINE, RELU, RES, BAR | PRE, BAR | FILM, FILM_LAYER | MASK,
                  BIAS | RELU | MASK, FILM_LAYER | POOL, FILM_LAYER | PRE | POOL,
                  BAR | HEAD, BAR | HEAD | POOL):        # a head launch is not form 0
        assert lib.depgan_wino_epilogue_class(flags, 0) == 0, flags
    for flags in (BAR | HEAD | POOL, BAR | HEAD | ACCUM, HEAD, BIAS | RELU | HEAD, BAR, BAR | HEAD | RES):
        assert lib.depgan_wino_epilogue_class(flags, 1) == 0, flags          # head with pool, head without its set
    for form in (2, 3):                                                      # 16-row tiles without head, gathered K
        for sets in TABLE.values():
            for flags in sets.values():
                assert lib.depgan_wino_epilogue_class(flags, form) == 0, (form, flags)


def test_switch_off_makes_every_launch_generic(switch):
    lib = switch
    assert lib.depgan_get_epilogue_classes() == 1
    assert lib.depgan_set_epilogue_classes(0) == 0 and lib.depgan_get_epilogue_classes() == 0
    for form, sets in TABLE.items():
        for flags in sets.values():
            assert lib.depgan_wino_epilogue_class(flags, form) == 0
    assert lib.depgan_set_epilogue_classes(1) == 0
    assert lib.depgan_wino_epilogue_class(BAR, 0) > 0


def test_refusals_precede_any_hip_call(switch):
    lib = switch
    for bad in (2, -1, 7):
        assert lib.depgan_set_epilogue_classes(bad) == 1 and b"set_epilogue_classes" in lib.depgan_last_error()
    assert lib.depgan_get_epilogue_classes() == 1                            # a refused value changes nothing
    for flags, form in ((1024, 0), (BAR | 4096, 0), (BAR, 4), (BAR, -1)):
        assert lib.depgan_wino_epilogue_class(flags, form) == -1 and lib.depgan_last_error()
    buf = C.create_string_buffer(64)
    name = lib.depgan_op_conv3x3_wino_kernel_name
    for kw in ({"flags": 1024}, {"B": 0}, {"H": 0}, {"W": -2}, {"ci": 0}, {"co": 0}, {"buf": None}, {"cap": 0}):
        a = dict(flags=BAR, B=2, H=16, W=16, ci=8, co=32, buf=buf, cap=64)
        a.update(kw)
        assert name(a["flags"], a["B"], a["H"], a["W"], a["ci"], a["co"], a["buf"], a["cap"]) == 1, kw
        assert lib.depgan_last_error()
    # what the Winograd kernel does not cover: status 3, from the plan and the shape alone
    for kw in ({"ci": 12}, {"co": 16}, {"H": 15}, {"W": 17}):
        a = dict(B=2, H=16, W=16, ci=8, co=32)
        a.update(kw)
        assert name(BAR, a["B"], a["H"], a["W"], a["ci"], a["co"], buf, 64) == 3, kw


def test_switch_is_initialised_from_the_environment():
    """DEPGAN_EPI_CLASSES=0 in a fresh process: off, and the selector answers 0; unset: on."""
    import subprocess
    import sys
    code = ("from dep_gan_im_amd import _lib; lib = _lib.load(); "
            "print(lib.depgan_get_epilogue_classes(), lib.depgan_wino_epilogue_class(%d, 0))" % BAR)
    for val, want in (("0", "0 0"), (None, None)):
        env = {k: v for k, v in os.environ.items() if k != "DEPGAN_EPI_CLASSES"}
        if val is not None:
            env["DEPGAN_EPI_CLASSES"] = val
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
        got = out.stdout.strip().splitlines()[-1]
        if want is None:
            on, cls = got.split()
            assert on == "1" and int(cls) > 0, got
        else:
            assert got == want
