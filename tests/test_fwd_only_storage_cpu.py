"""CPU: the surface of bf16 activation storage for the forward-only generator passes of the training closures -- the new
entry points are declared, exported and bound; the argument errors that need no GPU; the fused-head kernel's resources."""
import ctypes as C
import os
import re
import subprocess

import pytest

import dep_gan_im_amd as dg
from dep_gan_im_amd import _lib, build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["depgan_set_fwd_only_storage", "depgan_get_fwd_only_storage", "depgan_op_conv2d_head_bf16s"]
FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments


def test_entries_are_exported_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    declared = set(re.findall(r"\b(depgan_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in _lib.EXPORTS and name in declared, name
        assert getattr(lib, name).argtypes, name
    assert "DEPGAN_ABI_VERSION 3" in hdr and lib.depgan_abi_version() == 3      # additive entries: the ABI stays
    assert lib.depgan_config_size() == C.sizeof(_lib.Config)                   # no field was added to depgan_config
    assert "58 MB per sample" in hdr                                           # the extra memory is stated


def test_setter_and_operator_refuse_bad_arguments_before_any_hip_call(lib):
    assert lib.depgan_set_fwd_only_storage(None, 1) == 1
    assert lib.depgan_get_fwd_only_storage(None) == 0
    s = (64 * 32, 8 * 32, 32)
    call = lambda hw=FAKE, hb=FAKE, ho=FAKE, co=32, k=3, i=FAKE: lib.depgan_op_conv2d_head_bf16s(   # noqa: E731
        i, *s, FAKE, None, None, None, None, None, 0, None, 0, 0, 0, FAKE, *s, None, 1, 8, 8, 32, co, k, 1, hw, hb, ho, 1, 0,
        None)
    for kw in ({"hw": None}, {"hb": None}, {"ho": None}, {"i": None}, {"k": 2}):
        assert call(**kw) == 1, kw
        assert lib.depgan_last_error()
    assert call(co=64) == 3 and b"32 channels" in lib.depgan_last_error()       # more than one channel tile
    assert call(k=1) == 3


def test_python_argument_errors_need_no_gpu():
    nets = [dg.Gen_UNet2D((64, 64, 2)), dg.Dis_C2D_FCN1((64, 64, 1)), dg.Dis_C2D_FCN1((64, 64, 1))]
    with pytest.raises(ValueError, match="forward_only_storage"):
        dg.build_trainers(*nets, batchSize=2, forward_only_storage="float16")
    with pytest.raises(ValueError, match="activations_dtype"):
        dg.build_trainers(*nets, batchSize=2, forward_only_storage="bfloat16")
    with pytest.raises(ValueError, match="activations_dtype"):
        dg.build_trainers(*nets, batchSize=2, weights_dtype="bfloat16", forward_only_storage="bfloat16")
    assert all(n._engine is None for n in nets if hasattr(n, "_engine"))        # no engine was created or bound
    for cfg, ok in ((_lib.Config(bf16_weights=1, bf16_mfma=1, nc_out=1), True), (_lib.Config(bf16_weights=1, nc_out=1), False),
                    (_lib.Config(nc_out=1), False), (_lib.Config(nc_out=4), False)):
        eng = engine.Engine.__new__(engine.Engine)              # no context: the check reads the configuration only
        eng.cfg = cfg
        eng.h = None
        assert eng.forward_only_storage == "float32"
        with pytest.raises(ValueError):
            eng.forward_only_storage = "float16"
        if ok:
            eng.forward_only_storage = "bfloat16"
            assert eng.forward_only_storage == "bfloat16" and eng.forward_storage == "float32"   # independent
            eng.forward_only_storage = "float32"
        else:
            with pytest.raises(ValueError, match="bf16_mfma"):
                eng.forward_only_storage = "bfloat16"
        assert eng.forward_only_storage == "float32"


def test_fused_head_kernel_is_a_sibling_without_scratch(tmp_path):
    """-Rpass-analysis=kernel-resource-usage of igemm_bf16s.hip: exactly one fused-head instantiation (3x3), no scratch,
    at least two waves per SIMD; the plain kernels are still the two they were."""
    src = os.path.join(ROOT, "dep_gan_im_amd", "csrc", "igemm_bf16s.hip")
    r = subprocess.run([build._hipcc(), "-O3", "--offload-arch=" + build.ARCH, "-std=c++17", "-fPIC", "-Wno-unused-result",
                        "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "igemm_bf16s.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    head, plain = [], []
    for blk in re.split(r"Function Name: ", r.stderr)[1:]:
        name = blk.split()[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1))
        vgpr = int(re.search(r"\bVGPRs: (\d+)", blk).group(1))
        if "igemm_bf16s_head_kernel" in name:
            head.append((name, vgpr, scratch, occ))
        elif "igemm_bf16s_kernel" in name:
            plain.append((name, vgpr, scratch, occ))
    print("fused head kernel:", head, "plain:", plain)
    assert len(head) == 1 and "Li3ELi9E" in head[0][0]
    assert head[0][2] == 0 and head[0][3] >= 2
    assert len(plain) == 2 and all(p[2] == 0 for p in plain)
