"""CPU: the surface of the critics' 16-channel 5x5 layers on the bf16 matrix pipe (depgan_set_critic16_pipe, operator
path 10) -- exports, header, the refusals that are decided before any HIP call, the Python-side argument errors, and the
cross-compiled kernel's resource usage."""
import ctypes as C
import os
import re
import subprocess

import pytest

import dep_gan_im_amd as dg
from dep_gan_im_amd import _lib, build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["depgan_set_critic16_pipe", "depgan_get_critic16_pipe"]
FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments
NONE = (None, 0, 0, 0)


def test_entries_are_exported_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    declared = set(re.findall(r"\b(depgan_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in _lib.EXPORTS and name in declared, name
        assert getattr(lib, name).argtypes, name
    assert "DEPGAN_ABI_VERSION 3" in hdr                      # a new entry point is not a new ABI
    assert lib.depgan_set_critic16_pipe(None, 1) == 1 and lib.depgan_last_error()
    assert lib.depgan_set_critic16_pipe(None, 0) == 1
    assert lib.depgan_get_critic16_pipe(None) == 0


def _fused(lib, i=FAKE, w=FAKE, o=FAKE, ci=16, co=16, k=5, head=False, bwd=0, path=10):
    v = lambda p, c: (p, 8 * 8 * c, 8 * c, c)   # noqa: E731
    cin, cout = (co, ci) if bwd else (ci, co)
    hw = (FAKE, FAKE, FAKE) if head else (None, None, None)
    return lib.depgan_op_conv2d_fused(*v(i, cin), w, None, None, None, None, None, 0, *v(o, cout), *NONE, *NONE, *NONE, *NONE,
                                      *hw, 0, 0, 1, 8, 8, ci, co, k, 0, 0, path, bwd, None)


def test_path_10_refusals_are_decided_before_any_hip_call(lib):
    conv = lambda i=FAKE, w=FAKE, o=FAKE, ci=16, co=16, k=5: lib.depgan_op_conv2d(   # noqa: E731
        i, w, None, o, 1, 8, 8, ci, co, k, 0, 10, None)
    bwd = lambda dy=FAKE, w=FAKE, dx=FAKE, ci=16, co=16, k=5: lib.depgan_op_conv2d_bwd_data(   # noqa: E731
        dy, w, dx, 1, 8, 8, ci, co, k, 10, None)
    for fn in (conv, bwd, lambda **kw: _fused(lib, **kw), lambda **kw: _fused(lib, bwd=1, **kw)):
        assert fn(k=3) == 1 and b"KS" in lib.depgan_last_error()         # a 5x5 kernel: another KS is a bad argument
        assert fn(k=1) == 1
    # shapes the plan does not cover: refused, not rerouted.  Forward: Cout % 16, Cin >= 8, Cin % 4
    for fn in (conv, lambda **kw: _fused(lib, **kw)):
        assert fn(co=24) == 3 and lib.depgan_last_error()
        assert fn(ci=6) == 3 and fn(ci=4) == 3
    # backward-data: the launch's output channels are the layer's Cin, its input channels the layer's Cout
    for fn in (bwd, lambda **kw: _fused(lib, bwd=1, **kw)):
        assert fn(ci=24) == 3 and fn(ci=8) == 3
        assert fn(co=6) == 3 and fn(co=4) == 3
    for kw in ({"i": None}, {"w": None}, {"o": None}):
        assert conv(**kw) == 1, kw
        assert _fused(lib, **kw) == 1, kw
    for kw in ({"dy": None}, {"w": None}, {"dx": None}):
        assert bwd(**kw) == 1, kw
    assert _fused(lib, head=True) == 1 and b"head" in lib.depgan_last_error()
    assert _fused(lib, path=11) == 1                                      # and there is no path 11


def test_python_argument_errors_need_no_gpu():
    nets = [dg.Gen_UNet2D((64, 64, 2)), dg.Dis_C2D_FCN1((64, 64, 1)), dg.Dis_C2D_FCN1((64, 64, 1))]
    with pytest.raises(ValueError, match="activations_dtype"):
        dg.build_trainers(*nets, batchSize=2, critic16_pipe="bfloat16")
    with pytest.raises(ValueError, match="activations_dtype"):
        dg.build_trainers(*nets, batchSize=2, weights_dtype="bfloat16", critic16_pipe="bfloat16")
    with pytest.raises(ValueError, match="critic16_pipe"):
        dg.build_trainers(*nets, batchSize=2, weights_dtype="bfloat16", activations_dtype="bfloat16", critic16_pipe="float16")
    for cfg, ok in ((_lib.Config(bf16_weights=1, bf16_mfma=1, nc_out=1), True), (_lib.Config(bf16_weights=1, nc_out=1), False),
                    (_lib.Config(nc_out=1), False), (_lib.Config(nc_out=4), False)):
        eng = engine.Engine.__new__(engine.Engine)              # no context: the check reads the configuration only
        eng.cfg = cfg
        assert eng.critic16_pipe == "float32"
        with pytest.raises(ValueError, match="critic16_pipe"):
            eng.critic16_pipe = "float16"
        if ok:
            eng.critic16_pipe = "bfloat16"
            assert eng.critic16_pipe == "bfloat16"
            eng.critic16_pipe = "float32"
            assert eng.critic16_pipe == "float32"
        else:
            with pytest.raises(ValueError, match="bf16_mfma"):
                eng.critic16_pipe = "bfloat16"
            assert eng.critic16_pipe == "float32"
        eng.h = None


def test_n16_kernel_cross_compiles_without_scratch_at_two_workgroups_per_cu(tmp_path):
    """hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on igemm_bf16.hip: every instantiation of the
    16-channel kernel uses no scratch and its registers leave room for two workgroups (eight waves) per CU, i.e. at
    least two waves per SIMD.  (Its LDS does too: 64,000 bytes of 163,840 with all 25 taps staged.)"""
    src = os.path.join(ROOT, "dep_gan_im_amd", "csrc", "igemm_bf16.hip")
    r = subprocess.run([build._hipcc(), "-O3", "--offload-arch=" + build.ARCH, "-std=c++17", "-fPIC", "-Wno-unused-result",
                        "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "igemm_bf16.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = []
    for blk in re.split(r"Function Name: ", r.stderr)[1:]:
        name = blk.split()[0]
        if "igemm_bf16_n16_kernel" not in name:
            continue
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1))
        assert scratch == 0, (name, scratch)
        assert occ >= 2, (name, occ)
        seen.append(name)
    assert any("ILi5ELi25ELi2EE" in n for n in seen), seen       # the shipped instantiation: KS 5, 25 taps per stage
