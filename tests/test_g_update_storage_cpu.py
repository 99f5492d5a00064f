"""CPU: the surface of the generator update on bf16 activation storage (depgan_set_g_update_storage) -- the new entry
points are declared, exported and bound; the argument errors that need no GPU; the new kernels' resources; the three
instantiations of igemm_bf16s.hip are the three they were."""
import ctypes as C
import os
import re
import subprocess

import pytest

import dep_gan_im_amd as dg
from dep_gan_im_amd import _lib, build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dep_gan_im_amd", "csrc")
NAMES = ["depgan_set_g_update_storage", "depgan_get_g_update_storage", "depgan_debug_film_decision_bf16s",
         "depgan_op_conv2d_film_train_bf16s", "depgan_op_conv2d_wgrad_bf16s", "depgan_op_conv2d_bwd_data_bf16s",
         "depgan_op_unpool_mask_bf16s", "depgan_op_film_bwd_bf16s", "depgan_op_head_bwd_bf16s"]
FAKE = C.c_void_p(0x1000)        # never dereferenced: the calls below are refused on their arguments


def test_entries_are_exported_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    declared = set(re.findall(r"\b(depgan_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in _lib.EXPORTS and name in declared, name
        assert getattr(lib, name).argtypes, name
    assert "DEPGAN_ABI_VERSION 3" in hdr and lib.depgan_abi_version() == 3      # additive entries: the ABI stays
    assert lib.depgan_config_size() == C.sizeof(_lib.Config)                   # no field was added to depgan_config
    assert "58 MB per sample" in hdr and "14.4 MB per sample" in hdr           # both memory statements are there
    assert all(s in build.SOURCES for s in ("igemm_bf16s_train.hip", "igemm_bf16_mh.hip", "wgrad_bf16s.hip",
                                            "ops_bf16s.hip", "model_bf16s_train.hip"))


def test_setter_and_operators_refuse_bad_arguments_before_any_hip_call(lib):
    assert lib.depgan_set_g_update_storage(None, 1) == 1
    assert lib.depgan_get_g_update_storage(None) == 0
    shape = (C.c_int * 4)()
    assert lib.depgan_debug_film_decision_bf16s(None, b"gen_2", None, 0, shape) == 1
    assert lib.depgan_debug_tensor_bf16s(None, b"g/u/gen_2", None, 0, shape) == 1
    s = (64 * 32, 8 * 32, 32)
    train = lambda i=FAKE, w=FAKE, m=FAKE, a=FAKE, o=FAKE, u=FAKE, d=FAKE, B=1, ci=32, co=32: (   # noqa: E731
        lib.depgan_op_conv2d_film_train_bf16s(i, *s, w, None, None, None, m, a, 32, None, 0, 0, 0, o, *s, u, d, B, 8, 8, ci, co,
                                              1, None))
    for kw in ({"i": None}, {"w": None}, {"m": None}, {"a": None}, {"o": None}, {"u": None}, {"d": None}, {"B": 0}, {"ci": 0}):
        assert train(**kw) == 1, kw
        assert lib.depgan_last_error()
    assert train(ci=12) == 3 and train(co=16) == 3
    wg = lambda x=FAKE, d=FAKE, w=FAKE, B=1, H=8, ci=32, co=32, k=3: lib.depgan_op_conv2d_wgrad_bf16s(   # noqa: E731
        x, *s, d, *s, w, None, B, H, 8, ci, co, k, 0, None)
    for kw in ({"x": None}, {"d": None}, {"w": None}, {"B": 0}, {"H": -1}, {"ci": 0}, {"co": 0}, {"k": 2}, {"k": 5}):
        assert wg(**kw) == 1, kw
    assert wg(ci=12) == 3
    bd = lambda d=FAKE, w=FAKE, o=FAKE, B=1, ci=32, co=32, dc=0: lib.depgan_op_conv2d_bwd_data_bf16s(   # noqa: E731
        d, *s, w, None, 0, 0, 0, None, 0, 0, 0, o, *s, B, 8, 8, ci, co, dc, None)
    for kw in ({"d": None}, {"w": None}, {"o": None}, {"B": 0}, {"ci": 0}, {"co": -2}, {"dc": 2}):
        assert bd(**kw) == 1, kw
    assert bd(ci=16) == 3                                       # channels the kernel does not cover: refused, not rerouted
    up = lambda d=FAKE, a=FAKE, o=FAKE, B=1, Cc=32: lib.depgan_op_unpool_mask_bf16s(   # noqa: E731
        d, *s, a, *s, None, 0, 0, 0, o, *s, B, 4, 4, Cc, None)
    for kw in ({"d": None}, {"a": None}, {"o": None}, {"B": 0}, {"Cc": 0}, {"Cc": 12}):
        assert up(**kw) == 1, kw
    fb = lambda dr=FAKE, u=FAKE, d=FAKE, m=FAKE, du=FAKE, dm=FAKE, da=FAKE, B=1, HW=64, Cc=32: (   # noqa: E731
        lib.depgan_op_film_bwd_bf16s(dr, u, d, m, 32, du, dm, da, B, HW, Cc, None))
    for kw in ({"dr": None}, {"u": None}, {"d": None}, {"m": None}, {"du": None}, {"dm": None}, {"da": None}, {"B": 0},
               {"HW": 0}, {"Cc": 0}):
        assert fb(**kw) == 1, kw
    hb = lambda bw=1, a=FAKE, w=FAKE, d=FAKE, o=FAKE, Pn=64, Cc=32: lib.depgan_op_head_bwd_bf16s(   # noqa: E731
        bw, a, 32, w, d, o, Pn, Cc, None)
    for kw in ({"a": None}, {"w": None}, {"d": None}, {"o": None}, {"Pn": 0}, {"Cc": 0}, {"Cc": 12}):
        assert hb(**kw) == 1, kw


def test_python_argument_errors_need_no_gpu():
    nets = [dg.Gen_UNet2D((64, 64, 2)), dg.Dis_C2D_FCN1((64, 64, 1)), dg.Dis_C2D_FCN1((64, 64, 1))]
    with pytest.raises(ValueError, match="generator_update_storage"):
        dg.build_trainers(*nets, batchSize=2, generator_update_storage="float16")
    with pytest.raises(ValueError, match="generator_update_storage"):
        dg.build_trainers(*nets, batchSize=2, generator_update_storage="bfloat16")
    with pytest.raises(ValueError, match="generator_update_storage"):
        dg.build_trainers(*nets, batchSize=2, weights_dtype="bfloat16", generator_update_storage="bfloat16")
    assert all(n._engine is None for n in nets if hasattr(n, "_engine"))        # no engine was created or bound
    for cfg, ok in ((_lib.Config(bf16_weights=1, bf16_mfma=1, nc_out=1), True), (_lib.Config(bf16_weights=1, nc_out=1), False),
                    (_lib.Config(nc_out=1), False), (_lib.Config(nc_out=4), False)):
        eng = engine.Engine.__new__(engine.Engine)              # no context: the check reads the configuration only
        eng.cfg = cfg
        eng.h = None
        assert eng.g_update_storage == "float32"
        with pytest.raises(ValueError):
            eng.g_update_storage = "float16"
        if ok:
            eng.g_update_storage = "bfloat16"
            assert eng.g_update_storage == "bfloat16"
            assert eng.forward_only_storage == "float32" and eng.forward_storage == "float32"   # independent
            eng.g_update_storage = "float32"
        else:
            with pytest.raises(ValueError, match="bf16_mfma"):
                eng.g_update_storage = "bfloat16"
        assert eng.g_update_storage == "float32"


def _resources(src, tmp_path):
    r = subprocess.run([build._hipcc(), "-O3", "--offload-arch=" + build.ARCH, "-std=c++17", "-fPIC", "-Wno-unused-result",
                        "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o",
                        str(tmp_path / (src + ".o"))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for blk in re.split(r"Function Name: ", r.stderr)[1:]:
        out.append((blk.split()[0], int(re.search(r"\bVGPRs: (\d+)", blk).group(1)),
                    int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)),
                    int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1))))
    return out


@pytest.mark.parametrize("src,kernels", [("igemm_bf16s_train.hip", ["igemm_bf16s_train_kernelILi3ELi9E"]),
                                         ("igemm_bf16_mh.hip", ["igemm_bf16_mh_kernelILi3ELi9E", "igemm_bf16_mh_kernelILi1ELi1E"]),
                                         ("wgrad_bf16s.hip", ["wgrad_bf16s_kernelILi3E", "wgrad_bf16s_kernelILi1E"]),
                                         ("ops_bf16s.hip", ["unpool_mask_bf16s_kernel", "film_bwd_bf16s_partial",
                                                            "colsum_rowmul_bf16s_partial", "head_bwd_bf16s_kernel"])])
def test_new_kernels_cross_compile_without_scratch_at_two_waves_per_simd(tmp_path, src, kernels):
    res = _resources(src, tmp_path)
    print(src, res)
    for want in kernels:
        hit = [r for r in res if want in r[0]]
        assert len(hit) == 1, (want, res)
    for name, vgpr, scratch, occ in res:
        assert scratch == 0 and occ >= 2, (name, vgpr, scratch, occ)


def test_the_three_instantiations_of_igemm_bf16s_are_unchanged(tmp_path):
    """igemm_bf16s_kernel.inc gained a hook that is off in igemm_bf16s.hip: that unit still holds exactly the two plain
    kernels and the one fused-head kernel, none with scratch, and no training kernel."""
    res = _resources("igemm_bf16s.hip", tmp_path)
    plain = [r for r in res if "igemm_bf16s_kernel" in r[0]]
    head = [r for r in res if "igemm_bf16s_head_kernel" in r[0]]
    assert len(plain) == 2 and len(head) == 1 and not [r for r in res if "train" in r[0]]
    assert all(r[2] == 0 and r[3] >= 2 for r in plain + head)
    text = open(os.path.join(CSRC, "igemm_bf16s.hip")).read()
    assert text.count('#include "igemm_bf16s_kernel.inc"') == 2 and "IGEMM_BF16S_TRAIN" not in text
