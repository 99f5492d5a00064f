"""CPU: the surface of the DEP-UResNet predict on bf16 activation storage -- the new operator entry (export, header,
binding, argument checks that come before any HIP call), the Python-side refusals and acceptances that read the
configuration only, and the cross-compiled head kernel's resource usage."""
import ctypes as C
import os
import re
import subprocess

import pytest

import dep_gan_im_amd as dg
from dep_gan_im_amd import _lib, build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "depgan_op_head_softmax_bf16s"
FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments


def test_entry_is_exported_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    declared = set(re.findall(r"\b(depgan_[a-z0-9_]+)\s*\(", hdr))
    assert NAME in _lib.EXPORTS and NAME in declared
    assert len(getattr(lib, NAME).argtypes) == 9
    assert "DEPGAN_ABI_VERSION 3" in hdr                      # a new entry point is not a new ABI
    assert _lib.ABI_VERSION == 3


def test_operator_refuses_its_arguments_before_any_hip_call(lib):
    head = lambda a=FAKE, ld=32, w=FAKE, b=FAKE, p=FAKE, lg=None, P=64, C_=32: getattr(lib, NAME)(   # noqa: E731
        a, ld, w, b, p, lg, P, C_, None)
    for kw in ({"a": None}, {"w": None}, {"b": None}, {"p": None}, {"P": 0}, {"P": -3}, {"C_": 0}, {"C_": 24}, {"C_": 1024},
               {"ld": 24}, {"ld": 36}, {"ld": 0}, {"a": C.c_void_p(0x1008)}, {"w": C.c_void_p(0x1004)},
               {"p": C.c_void_p(0x1008)}, {"lg": C.c_void_p(0x1004)}):
        assert head(**kw) == 1, kw
        assert lib.depgan_last_error()


def test_python_argument_errors_need_no_gpu():
    with pytest.raises(ValueError, match="nc_out"):
        dg.Gen_UNet2D((64, 64, 1), nc_out=4, inference_dtype="bfloat16")
    with pytest.raises(ValueError, match="inference_copy"):
        dg.Gen_UNet2D((64, 64, 1), nc_out=4, inference_dtype="bfloat16")
    for nc in (1, 4):
        m = dg.Gen_UNet2D((64, 64, 1), nc_out=nc)
        with pytest.raises(ValueError, match="bfloat16"):
            m.inference_copy("float16")
        assert not m.inference_only
    # a context-less engine: the checks read the configuration only
    eng = engine.Engine.__new__(engine.Engine)
    eng.cfg = _lib.Config(bf16_weights=1, bf16_mfma=1, nc_out=4)
    eng.h = None
    assert eng.inference_only and eng.forward_storage == "float32"
    eng.forward_storage = "bfloat16"
    assert eng.forward_storage == "bfloat16"
    with pytest.raises(ValueError):
        eng.forward_storage = "float16"
    for attr in ("forward_only_storage", "g_update_storage", "critic16_pipe"):
        with pytest.raises(ValueError, match="inference"):
            setattr(eng, attr, "bfloat16")
    for call in (lambda: eng.uresnet(None, None, None), lambda: eng.apply_adam("G"), lambda: eng.critic("D_y2", 0, 0, 0, 0),
                 lambda: eng.generator(0, 0, 0), lambda: eng.generator_eval_multi(0, 0, []),
                 lambda: eng.gen_iteration(None, None, None), lambda: eng.d_forward("D_y2", None)):
        with pytest.raises(ValueError, match="inference"):                  # raised before the library is touched
            call()
    plain = engine.Engine.__new__(engine.Engine)
    plain.cfg = _lib.Config(nc_out=4)
    plain.h = None
    assert not plain.inference_only
    with pytest.raises(ValueError, match="bf16_mfma"):
        plain.forward_storage = "bfloat16"
    with pytest.raises(ValueError, match="bf16_mfma"):
        plain.g_forward(None, None, storage="bfloat16")


def test_inference_copy_is_a_predict_only_twin_with_its_own_weights():
    m = dg.Gen_UNet2D((64, 64, 1), nc_out=4, seed=3)
    fast = m.inference_copy()
    assert fast.inference_only and fast.inference_dtype == "bfloat16" and fast.nc_out == 4 and fast.name == m.name
    w, wf = m.get_weights_dict(), fast.get_weights_dict()
    assert list(w) == list(wf) and all((w[k] == wf[k]).all() and w[k] is not wf[k] for k in w)
    k = "gen_segmentation/kernel"
    m.set_weights({k: w[k] + 1.0})
    assert (fast.get_weights_dict()[k] == w[k]).all()                       # later changes are not followed
    for call in (fast.compile, lambda: fast.fit(None, None), lambda: fast.train_on_batch(None, None),
                 lambda: fast.test_on_batch(None, None), lambda: fast.evaluate(None, None)):
        with pytest.raises(RuntimeError, match="predict-only"):
            call()
    m.compile()                                                             # the source stays trainable
    one = dg.Gen_UNet2D((64, 64, 2), seed=4).inference_copy("bfloat16")
    assert one.inference_only and one.nc_out == 1
    with pytest.raises(RuntimeError, match="predict-only"):
        one.compile()


def test_head_kernel_cross_compiles_without_scratch(tmp_path):
    """hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage: head_softmax_bf16s_kernel uses no scratch (its
    32 weights stay in registers across the grid-stride loop)."""
    src = os.path.join(ROOT, "dep_gan_im_amd", "csrc", "igemm_bf16s.hip")
    r = subprocess.run([build._hipcc(), "-O3", "--offload-arch=" + build.ARCH, "-std=c++17", "-fPIC", "-Wno-unused-result",
                        "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "igemm_bf16s.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in re.split(r"Function Name: ", r.stderr)[1:] if "head_softmax_bf16s_kernel" in b.split()[0]]
    assert len(blocks) == 1
    assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blocks[0]).group(1)) == 0
    assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blocks[0]).group(1)) >= 4
