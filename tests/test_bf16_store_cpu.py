"""CPU: the surface of the bf16-activation-storage generator forward -- exports, header, argument checks that come
before any HIP call, the Python-side argument errors, and the cross-compiled kernel's resource usage."""
import ctypes as C
import os
import re
import subprocess

import pytest

import dep_gan_im_amd as dg
from dep_gan_im_amd import _lib, build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["depgan_g_forward_bf16s", "depgan_debug_tensor_bf16s", "depgan_op_conv2d_bf16s", "depgan_op_deconv2x2_bf16s",
         "depgan_op_edge_conv_bf16s", "depgan_op_head_bf16s"]
FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments


def test_entries_are_exported_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    declared = set(re.findall(r"\b(depgan_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in _lib.EXPORTS and name in declared, name
        assert getattr(lib, name).argtypes, name
    assert "DEPGAN_ABI_VERSION 3" in hdr                      # a new entry point is not a new ABI


def test_operators_refuse_null_and_non_positive_arguments_before_any_hip_call(lib):
    s = (64 * 32, 8 * 32, 32)
    conv = lambda i=FAKE, w=FAKE, o=FAKE, B=1, H=8, W=8, ci=32, co=32, k=3, os_=s: lib.depgan_op_conv2d_bf16s(   # noqa: E731
        i, *s, w, None, None, None, None, None, 0, None, 0, 0, 0, o, *os_, None, B, H, W, ci, co, k, 1, None)
    for kw in ({"i": None}, {"w": None}, {"o": None}, {"B": 0}, {"H": 0}, {"W": -1}, {"ci": 0}, {"co": 0}, {"k": 2},
               {"os_": (0, 0, 0)}):
        assert conv(**kw) == 1, kw
        assert lib.depgan_last_error()
    assert conv(ci=12) == 3 and conv(co=16) == 3               # shapes the kernel does not cover: refused, not rerouted
    dec = lambda i=FAKE, w=FAKE, o=FAKE, B=1, H=8: lib.depgan_op_deconv2x2_bf16s(   # noqa: E731
        i, *s, w, None, None, None, o, 4 * 64 * 64, 16 * 64, 64, B, H, 8, 32, 32, 1, None)
    for kw in ({"i": None}, {"w": None}, {"o": None}, {"B": 0}, {"H": 0}):
        assert dec(**kw) == 1, kw
    edge = lambda i=FAKE, w=FAKE, o=FAKE, B=1, ci=1, co=32: lib.depgan_op_edge_conv_bf16s(   # noqa: E731
        i, w, None, None, None, o, *s, B, 8, 8, ci, co, 1, None)
    for kw in ({"i": None}, {"w": None}, {"o": None}, {"B": 0}, {"ci": 0}, {"co": 0}):
        assert edge(**kw) == 1, kw
    assert edge(ci=3) == 3 and edge(co=64) == 3
    head = lambda a=FAKE, w=FAKE, b=FAKE, o=FAKE, P=64, C_=32: lib.depgan_op_head_bf16s(a, w, b, o, P, C_, 1, None)   # noqa: E731
    for kw in ({"a": None}, {"w": None}, {"b": None}, {"o": None}, {"P": 0}, {"C_": 0}, {"C_": 24}):
        assert head(**kw) == 1, kw
    shape = (C.c_int * 4)()
    assert lib.depgan_debug_tensor_bf16s(None, b"g/out/gen_0", None, 0, shape) == 1
    assert lib.depgan_g_forward_bf16s(None, FAKE, FAKE, FAKE, 1) == 1


def test_python_argument_errors_need_no_gpu():
    with pytest.raises(ValueError, match="nc_out"):
        dg.Gen_UNet2D((64, 64, 2), nc_out=4, inference_dtype="bfloat16")
    with pytest.raises(ValueError, match="inference_dtype"):
        dg.Gen_UNet2D((64, 64, 2), inference_dtype="float16")
    assert dg.Gen_UNet2D((64, 64, 2)).inference_dtype == "float32"
    assert dg.Gen_UNet2D((64, 64, 2), inference_dtype="bfloat16").inference_dtype == "bfloat16"
    for cfg, ok in ((_lib.Config(bf16_weights=1, bf16_mfma=1, nc_out=1), True), (_lib.Config(bf16_weights=1, nc_out=1), False),
                    (_lib.Config(nc_out=1), False), (_lib.Config(nc_out=4), False)):
        eng = engine.Engine.__new__(engine.Engine)              # no context: the check reads the configuration only
        eng.cfg = cfg
        assert eng.forward_storage == "float32"
        with pytest.raises(ValueError):
            eng.forward_storage = "float16"
        if ok:
            eng.forward_storage = "bfloat16"
            assert eng.forward_storage == "bfloat16"
        else:
            with pytest.raises(ValueError, match="bf16_mfma"):
                eng.forward_storage = "bfloat16"
            with pytest.raises(ValueError, match="bf16_mfma"):
                eng.g_forward(None, None, storage="bfloat16")
        eng.h = None


def test_conv_kernel_cross_compiles_without_scratch_at_two_workgroups_per_cu(tmp_path):
    """hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage: the bf16-storage convolution kernels use no
    scratch and leave room for two workgroups (eight waves) per CU, i.e. at least two waves per SIMD."""
    src = os.path.join(ROOT, "dep_gan_im_amd", "csrc", "igemm_bf16s.hip")
    r = subprocess.run([build._hipcc(), "-O3", "--offload-arch=" + build.ARCH, "-std=c++17", "-fPIC", "-Wno-unused-result",
                        "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "igemm_bf16s.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    seen = 0
    for blk in blocks:
        name = blk.split()[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1))
        assert scratch == 0, (name, scratch)
        if "igemm_bf16s_kernel" in name:
            seen += 1
            assert occ >= 2, (name, occ)
    assert seen == 2                                            # KS = 3 and KS = 1
