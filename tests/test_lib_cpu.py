"""CPU: the C-ABI library builds for gfx950, loads, exports every symbol declared
in include/depgan.h, and the host-side facade mirrors the reference surface."""
import os
import re

import numpy as np
import pytest

import dep_gan_im_amd as dg
from dep_gan_im_amd import _lib, models
from oracle import depgan_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    declared = set(re.findall(r"\b(depgan_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"depgan_ctx", "depgan_config"}
    assert len(declared) >= 25
    for name in sorted(declared):
        assert hasattr(lib, name), "libdepgan.so does not export %s" % name
    assert set(_lib.EXPORTS) <= declared


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.DepganError):
        _lib.load()


def test_no_gpu_means_no_silent_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    g = dg.Gen_UNet2D((256, 256, 1))
    with pytest.raises(_lib.DepganError):
        g.predict([np.zeros((1, 256, 256, 1), np.float32), np.zeros((1, 32, 1), np.float32)])


def test_weight_tables_follow_reference_layer_names():
    g = dg.Gen_UNet2D((256, 256, 1), (32, 1), 32, 1, seed=0)
    ref = O.init_generator(0)
    assert [(n, tuple(s)) for n, s, _ in g._static_table()] == [(k, v.shape) for k, v in ref.items()]
    assert [w.name for w in g.trainable_weights] == O.trainable_names(ref)
    d = dg.Dis_C2D_FCN1((256, 256, 1), seed=0)
    refd = O.init_critic(0)
    assert [(n, tuple(s)) for n, s, _ in d._static_table()] == [(k, v.shape) for k, v in refd.items()]
    assert g.count_params() == 2486145 + 2 * 2912 and d.count_params() == 1798002
    g2 = dg.Gen_UNet2D((256, 256, 2))
    assert dict((n, s) for n, s, _ in g2._static_table())["conv2d_gen_0/kernel"] == (3, 3, 2, 32)


def test_keras_default_initialisers():
    g = dg.Gen_UNet2D((256, 256, 1), seed=3)
    w = g.get_weights_dict()
    assert np.all(w["bn_gen_0/gamma"] == 1) and np.all(w["bn_gen_0/moving_variance"] == 1)
    assert np.all(w["conv2d_gen_0/bias"] == 0) and np.all(w["bn_gen_0/moving_mean"] == 0)
    k = w["conv2d_gen_1/kernel"]
    lim = np.sqrt(6.0 / (9 * 32 + 9 * 32))
    assert k.shape == (3, 3, 32, 32) and np.abs(k).max() <= lim and np.abs(k).max() > 0.9 * lim
    hk = w["dense_noise_2_mul/kernel"]
    # truncated normal whose RESULT has std sqrt(2/fan_in) (Keras >= 2.2.3; models.HE_NORMAL_TRUNC_STD), never beyond
    # two sampled standard deviations -- and the same definition as the oracle's initialiser
    assert hk.shape == (1024, 128) and abs(hk.std() / np.sqrt(2.0 / 1024) - 1.0) < 0.03
    assert np.abs(hk).max() <= 2.0 * np.sqrt(2.0 / 1024) / models.HE_NORMAL_TRUNC_STD + 1e-7
    ok = O.init_generator(5)["dense_noise_2_mul/kernel"]
    assert abs(ok.std() / hk.std() - 1.0) < 0.03


def test_host_save_load_and_errors(tmp_path):
    d = dg.Dis_C2D_FCN1((256, 256, 1), seed=1)
    p = str(tmp_path / "d.npz")
    d.save(p)
    d2 = dg.Dis_C2D_FCN1((256, 256, 1), seed=2)
    d2.load_weights(p)
    for a, b in zip(d.get_weights(), d2.get_weights()):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError):
        d2.set_weights([np.zeros(3)])
    with pytest.raises(ValueError):
        d2.set_weights({"conv2d_dis_0a/kernel": np.zeros((3, 3, 1, 16), np.float32)})
    with pytest.raises(ValueError):
        dg.Dis_C2D_FCN1((256, 256, 2))
    with pytest.raises(ValueError):
        dg.Gen_UNet2D((256, 256, 1), (16, 1))
    lines = []
    d.summary(print_fn=lines.append)
    assert any("1798002" in ln for ln in lines)


def _header_config_fields():
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    body = re.search(r"typedef struct depgan_config \{(.*?)\} depgan_config;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_config_struct_matches_header_binding_and_integration_doc(lib):
    import ctypes as C
    fields = _header_config_fields()
    assert fields[0] == ("struct_size", "int")
    ctypes_of = {"int": C.c_int, "float": C.c_float}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(_lib.Config._fields_)
    assert lib.depgan_config_size() == C.sizeof(_lib.Config) == 4 * len(fields)
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    assert int(re.search(r"#define DEPGAN_ABI_VERSION (\d+)", hdr).group(1)) == lib.depgan_abi_version() \
        == _lib.ABI_VERSION
    # the stub a maintainer would copy out of INTEGRATION.md declares the same struct
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    stub = doc[doc.index("class Config(C.Structure)"):]
    stub = stub[:stub.index("ctx = C.c_void_p()")]
    doc_fields = re.findall(r'\("([a-z0-9_A-Z]+)", C\.c_(int|float)\)', stub)
    assert doc_fields == fields
    assert "depgan_abi_version() == %d" % _lib.ABI_VERSION in stub
    kw = re.search(r"cfg = Config\((.*?)\)\n", stub, re.S).group(1)
    assert [k.strip().split("=")[0] for k in kw.split(",")] == [n for n, _ in fields]


def test_create_rejects_a_config_of_another_size(lib):
    """No GPU needed: the size check comes before any HIP call."""
    import ctypes as C
    cfg = _lib.Config(batch=2, height=64, width=64, nicg=1, first_fm=32, im_thresh=0.5, delta=10.0, lrD=1e-4, lrG=1e-4,
                      beta1=0.0, beta2=0.9, adam_eps=1e-7, nc_out=1)
    assert cfg.struct_size == C.sizeof(_lib.Config)
    cfg.struct_size -= 4                     # what a caller bound to the previous header would pass
    h = C.c_void_p()
    assert lib.depgan_create(C.byref(cfg), C.byref(h)) != 0 and not h.value
    assert b"struct_size" in lib.depgan_last_error()
    cfg.struct_size = 0                      # a caller that never heard of the field
    assert lib.depgan_create(C.byref(cfg), C.byref(h)) != 0


def test_library_carries_the_hash_of_the_sources_it_was_built_from(lib, tmp_path, monkeypatch):
    """The GPU box loads the library that was cross-compiled here: the binding refuses one whose embedded source hash
    is not the hash of the sources lying next to it."""
    from dep_gan_im_amd import build
    assert lib.depgan_source_hash().decode() == build.source_hash()
    real = build.source_hash
    monkeypatch.setattr(build, "source_hash", lambda: "0" * 32)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.DepganError, match="other sources"):
        _lib.load()
    monkeypatch.setattr(build, "source_hash", real)
    monkeypatch.setattr(_lib, "_lib", None)
    assert _lib.load() is not None


def test_every_moments_and_colsum_call_passes_its_scratch_capacity():
    """dg_col_moments / dg_colsum_pair write nb x 3 x C / nb x 2 x C floats into their scratch and refuse a smaller one:
    every call in the model passes the capacity of the buffer it passes (the context's scratch and scratchFloats)."""
    src = open(os.path.join(ROOT, "dep_gan_im_amd", "csrc", "uresnet.hip")).read()
    calls = re.findall(r"\b(dg_col_moments|dg_colsum_pair)\s*\(([^;]*)\);", src)
    assert len(calls) >= 2 and {c[0] for c in calls} == {"dg_col_moments", "dg_colsum_pair"}
    for name, args in calls:
        args = [a.strip() for a in args.replace("\n", " ").split(",")]
        assert args[-3:-1] == ["c->scratch", "c->scratchFloats"], (name, args)
    model = open(os.path.join(ROOT, "dep_gan_im_amd", "csrc", "model.hip")).read()
    assert re.search(r"dmalloc\(c, &c->scratch, c->scratchFloats\)", model)


SCRATCH_REDUCTIONS = ["dg_colsum", "dg_colsum_rowmul", "dg_sum", "dg_gp_u0", "dg_gloss_sums", "dg_film_bwd",
                      "dg_critic_tail_wgrad", "dg_noise_bwd"]


def test_every_step_reduction_call_passes_its_scratch_capacity():
    """The step's reductions write their partials (colsum: up to 2048 x C floats) into the context's scratch and
    refuse a smaller capacity: every call in the model passes c->scratch together with c->scratchFloats (the
    depgan_op_* entries: the scratch they allocate and its capacity), and each declares its capacity argument and a
    *_scratch size helper."""
    model_calls = set()
    for f in ("model.hip", "op_entries.hip", "uresnet.hip"):
        src = open(os.path.join(ROOT, "dep_gan_im_amd", "csrc", f)).read()
        for name, args in re.findall(r"\b(%s)\s*\(([^;]*)\);" % "|".join(SCRATCH_REDUCTIONS), src):
            args = [a.strip() for a in args.replace("\n", " ").split(",")]
            pairs = [tuple(args[i:i + 2]) for i in range(len(args) - 1)]
            assert ("c->scratch", "c->scratchFloats") in pairs or ("scratch", "cap") in pairs, (name, args)
            if "c->scratch" in args:
                model_calls.add(name)
    assert model_calls == set(SCRATCH_REDUCTIONS)
    hdr = open(os.path.join(ROOT, "dep_gan_im_amd", "csrc", "ops.h")).read()
    hdr += open(os.path.join(ROOT, "dep_gan_im_amd", "csrc", "noise.h")).read()
    for name in SCRATCH_REDUCTIONS:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, hdr).group(1)
        assert re.search(r"float\* scratch,\s*size_t scratch_floats", decl), name
    for helper in ("dg_colsum", "dg_sum", "dg_gp_u0", "dg_gloss_sums", "dg_film_bwd", "dg_critic_tail_wgrad",
                   "dg_noise_bwd"):
        assert re.search(r"\bsize_t %s_scratch\(" % helper, hdr), helper


STEP_OPS = ["unpool_mask", "gather_pool", "head", "critic_tail_fwd", "critic_tail_bwd", "critic_tail_wgrad", "colsum",
            "sum", "critic_inputs", "gp_u0", "critic_stats", "gloss_sums", "g_dpre", "film_bwd", "bn_prepare_batch",
            "bn_gamma_grad_batch", "noise_fwd", "noise_bwd", "best_noise", "round_bf16_masked"]


def test_step_operator_entries_are_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    for op in STEP_OPS:
        name = "depgan_op_" + op
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name + " has no argtypes"


DEBUG_ENTRIES = ["capture", "tensor", "tensor_bf16s", "film_decision_bf16s", "wgrad_plan", "wgrad_choice", "conv_choice",
                 "deconv_fwd_plan"]


def test_debug_entries_are_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    assert sorted(set(re.findall(r"\bint depgan_debug_(\w+)\(", hdr))) == sorted(DEBUG_ENTRIES)
    for op in DEBUG_ENTRIES:
        name = "depgan_debug_" + op
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name + " has no argtypes"


# ---- the binding is derived from include/depgan.h (dep_gan_im_amd/_lib.py::parse_header) ----

def _pinned_signatures():
    """argtypes / restype as the hand-kept table listed them before the binding was derived from the header (typed
    pointers written as c_void_p), one entry of every declaration form."""
    import ctypes as C
    vp, i, L, f, u, s = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_uint, C.c_char_p
    return {
        "depgan_create": (i, [vp, vp]),
        "depgan_destroy": (None, [vp]),
        "depgan_param_info": (i, [vp, i, i, s, i, vp, vp, vp, vp]),
        "depgan_arena_ptr": (vp, [vp, i, i]),
        "depgan_arena_floats": (L, [vp, i, i]),
        "depgan_data_prep_scratch_floats": (C.c_size_t, [i] * 3),
        "depgan_last_error": (s, []),
        "depgan_set_allreduce": (i, [vp, _lib.ALLREDUCE_FN, vp, i]),
        "depgan_gen_iteration": (i, [vp, vp, vp, vp, vp, i, vp, vp, vp, vp, i, L, vp, vp, vp, i, vp, vp]),
        "depgan_eval_counts": (i, [vp, i] + [vp] * 7 + [L, C.c_double, vp, vp]),
        "depgan_op_affine_act": (i, [vp] * 4 + [L] * 3 + [vp] * 4 + [i] * 6 + [u, f, vp]),
        "depgan_profile_read": (i, [vp, i, vp, vp, vp]),
        # 47 parameters: four-word views of in / out / out_pre / res / mask / pool, 9 bare pointers, 13 ints, the stream
        "depgan_op_conv2d_fused": (i, [vp, L, L, L] + [vp] * 6 + [i] + [vp, L, L, L] * 5 + [vp] * 3 + [i] * 12 + [vp]),
        "depgan_op_unpool_mask_bf16s": (i, [vp, L, L, L] * 4 + [i] * 4 + [vp]),
        "depgan_debug_tensor": (i, [vp, s, vp, L, vp]),
        "depgan_debug_wgrad_plan": (i, [i] * 7 + [vp]),      # host only; an `int out[4]` array parameter
        "depgan_debug_deconv_fwd_plan": (i, [i] * 5 + [vp]),  # host only; a `long out[4]` array parameter
        # depgan_op_deconv2x2 with the output as a view: six pointers, three strides, six ints, the stream
        "depgan_op_deconv2x2_ex": (i, [vp] * 6 + [L] * 3 + [i] * 6 + [vp]),
        "depgan_op_deconv2x2": (i, [vp] * 6 + [i] * 6 + [vp]),
    }


def test_derived_binding_matches_the_pinned_signatures(lib):
    import ctypes as C
    for name, (restype, argtypes) in _pinned_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype)
        assert list(fn.argtypes) == argtypes, (name, fn.argtypes)
    hook = _lib.ALLREDUCE_FN
    assert hook._restype_ is C.c_int and list(hook._argtypes_) == [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    assert len(lib.depgan_gen_iteration.argtypes) == 18 and len(lib.depgan_op_conv2d_fused.argtypes) == 47


def test_every_prototype_is_bound_with_the_header_s_parameter_count(lib):
    """The count does not come from _lib's parser: names by the regex of test_library_exports_every_declared_symbol,
    parameters by the commas between the parentheses of the comment-stripped text."""
    hdr = open(os.path.join(ROOT, "include", "depgan.h")).read()
    declared = set(re.findall(r"\b(depgan_[a-z0-9_]+)\s*\(", hdr)) - {"depgan_ctx", "depgan_config"}
    assert set(_lib.EXPORTS) == declared and len(_lib.EXPORTS) == len(declared) >= 174
    stripped = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in sorted(declared):
        found = re.findall(r"\b%s\s*\(([^()]*)\)\s*;" % name, stripped)
        assert len(found) == 1, name
        count = 0 if found[0].strip() == "void" else found[0].count(",") + 1
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count, (name, count, fn.argtypes)


def test_header_parser_refuses_what_it_cannot_map(tmp_path):
    with pytest.raises(_lib.DepganError, match="depgan_x"):
        _lib.parse_header("int depgan_x(short a);")
    with pytest.raises(_lib.DepganError, match="depgan_x"):
        _lib.parse_header("int depgan_ok(int a);\nint depgan_x(int a")
    missing = str(tmp_path / "include" / "depgan.h")
    with pytest.raises(_lib.DepganError, match=re.escape(missing)):
        _lib.read_header(missing)
    ok = _lib.parse_header("int depgan_ok(int a);")
    assert list(ok.prototypes) == ["depgan_ok"]


def test_constants_taken_from_the_header_keep_their_values():
    from dep_gan_im_amd import evaluate
    assert (_lib.ABI_VERSION, _lib.MAX_MULTI, _lib.MAX_CRITIC_STEPS, _lib.RCCL_ID_BYTES) == (3, 32, 256, 128)
    assert (evaluate.NCOUNT, evaluate.NCOUNT_LABEL) == (20, 18)
    assert (_lib.NET_G, _lib.NET_D_Y2, _lib.NET_D_DEM) == (0, 1, 2)
    assert (_lib.ARENA_PARAMS, _lib.ARENA_NONTRAINABLE, _lib.ARENA_GRADS, _lib.ARENA_ADAM_M, _lib.ARENA_ADAM_V) \
        == (0, 1, 2, 3, 4)
