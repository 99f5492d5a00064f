"""ctypes binding of libdepgan.so (the C ABI declared in include/depgan.h).

There is no CPU fallback: if the HIP library is missing the import fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DEPGAN_LIB") or os.path.join(HERE, "libdepgan.so")   # DEPGAN_LIB: A/B another build

EXPORTS = [
    "depgan_last_error", "depgan_create", "depgan_destroy", "depgan_set_stream", "depgan_param_count",
    "depgan_param_info", "depgan_arena_floats", "depgan_arena_ptr", "depgan_weights_changed", "depgan_g_forward",
    "depgan_d_forward", "depgan_critic_grads", "depgan_critic_step", "depgan_g_eval", "depgan_g_grads",
    "depgan_g_step", "depgan_apply_adam", "depgan_last_sums", "depgan_profile_enable", "depgan_profile_read",
    "depgan_profile_reset", "depgan_profile_dump", "depgan_op_conv2d", "depgan_op_conv2d_bwd_data", "depgan_op_conv2d_wgrad",
    "depgan_op_maxpool", "depgan_op_deconv2x2", "depgan_op_deconv2x2_wgrad", "depgan_op_conv2d_stamps", "depgan_uresnet_grads", "depgan_uresnet_step",
    "depgan_uresnet_eval", "depgan_profile_read_bytes", "depgan_g_eval_multi", "depgan_eval_accumulate", "depgan_eval_counts",
    "depgan_data_prep_scratch_floats", "depgan_data_prep_subject", "depgan_abi_version", "depgan_config_size",
    "depgan_set_allreduce", "depgan_get_adam_step", "depgan_set_adam_step", "depgan_gen_iteration", "depgan_eval_divide",
    "depgan_source_hash", "depgan_debug_capture", "depgan_debug_tensor", "depgan_rccl_unique_id", "depgan_rccl_init",
    "depgan_rccl_broadcast", "depgan_rccl_info", "depgan_rccl_shutdown", "depgan_op_conv2d_wgrad_bf16",
    "depgan_op_bn_moments", "depgan_op_bn_backward", "depgan_op_affine_act", "depgan_op_softmax_ce4",
    "depgan_op_bn_rows_fwd", "depgan_op_bn_rows_bwd", "depgan_op_small_gemm",
    "depgan_op_unpool_mask", "depgan_op_gather_pool", "depgan_op_head", "depgan_op_critic_tail_fwd",
    "depgan_op_critic_tail_bwd", "depgan_op_critic_tail_wgrad", "depgan_op_colsum", "depgan_op_sum",
    "depgan_op_critic_inputs", "depgan_op_gp_u0", "depgan_op_critic_stats", "depgan_op_gloss_sums", "depgan_op_g_dpre",
    "depgan_op_film_bwd", "depgan_op_bn_prepare_batch", "depgan_op_bn_gamma_grad_batch", "depgan_op_noise_fwd",
    "depgan_op_noise_bwd", "depgan_op_best_noise", "depgan_op_round_bf16_masked",
    "depgan_data_zscore_scratch_floats", "depgan_data_prep_zscore", "depgan_data_mask_slices", "depgan_labels_to_onehot",
    "depgan_eval_accumulate_channels", "depgan_eval_label_counts",
    "depgan_g_forward_bf16s", "depgan_debug_tensor_bf16s", "depgan_op_conv2d_bf16s", "depgan_op_deconv2x2_bf16s",
    "depgan_op_edge_conv_bf16s", "depgan_op_head_bf16s",
    "depgan_set_fwd_only_storage", "depgan_get_fwd_only_storage", "depgan_op_conv2d_head_bf16s",
    "depgan_set_g_update_storage", "depgan_get_g_update_storage", "depgan_debug_film_decision_bf16s",
    "depgan_op_conv2d_film_train_bf16s", "depgan_op_conv2d_wgrad_bf16s", "depgan_op_conv2d_bwd_data_bf16s",
    "depgan_op_unpool_mask_bf16s", "depgan_op_film_bwd_bf16s", "depgan_op_head_bwd_bf16s",
    "depgan_op_conv2d_fused", "depgan_op_deconv2x2_igemm", "depgan_op_conv2d_wgrad_ex",
    "depgan_set_critic16_pipe", "depgan_get_critic16_pipe", "depgan_op_head_softmax_bf16s",
]

ABI_VERSION = 3          # DEPGAN_ABI_VERSION of the include/depgan.h this binding was written against
MAX_MULTI, MAX_CRITIC_STEPS = 32, 256
RCCL_ID_BYTES = 128


class Config(C.Structure):
    """depgan_config of include/depgan.h, field for field (tests/test_lib_cpu.py parses the header and compares)."""
    _fields_ = [("struct_size", C.c_int), ("batch", C.c_int), ("height", C.c_int), ("width", C.c_int),
                ("nicg", C.c_int), ("first_fm", C.c_int), ("im_thresh", C.c_float), ("delta", C.c_float),
                ("lrD", C.c_float), ("lrG", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("adam_eps", C.c_float), ("nc_out", C.c_int), ("bf16_weights", C.c_int), ("bf16_mfma", C.c_int),
                ("f32_split", C.c_int)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(Config)


# int fn(void* user, float* dev_ptr, long n, void* hip_stream): the all-reduce hook of depgan_set_allreduce
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p)


NET_G, NET_D_Y2, NET_D_DEM = 0, 1, 2
ARENA_PARAMS, ARENA_NONTRAINABLE, ARENA_GRADS, ARENA_ADAM_M, ARENA_ADAM_V = range(5)

_lib = None


class DepganError(RuntimeError):
    pass


def load():
    """Load libdepgan.so; raises if it has not been built (python -m dep_gan_im_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DepganError(
            "libdepgan.so not found at %s -- the HIP library is the product; build it with "
            "`python -m dep_gan_im_amd.build` (needs hipcc). There is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm ships its own HIP runtime.  It must be in the process BEFORE libdepgan.so is loaded, so that the
    # library binds to that runtime: loaded the other way round, two runtimes coexist and hipMalloc inside the
    # library reports "no ROCm-capable device is detected".
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    fp, vp, ip = C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_int)
    lib.depgan_last_error.restype = C.c_char_p
    lib.depgan_abi_version.argtypes = []
    lib.depgan_config_size.argtypes = []
    lib.depgan_config_size.restype = C.c_size_t
    if lib.depgan_abi_version() != ABI_VERSION or lib.depgan_config_size() != C.sizeof(Config):
        raise DepganError("libdepgan.so at %s has ABI %d / depgan_config of %d bytes, this binding expects ABI %d / %d "
                          "bytes: rebuild with `python -m dep_gan_im_amd.build`"
                          % (LIB_PATH, lib.depgan_abi_version(), lib.depgan_config_size(), ABI_VERSION, C.sizeof(Config)))
    lib.depgan_source_hash.restype = C.c_char_p
    if os.path.isdir(os.path.join(HERE, "csrc")) and not os.environ.get("DEPGAN_LIB"):
        from .build import source_hash
        built, here = lib.depgan_source_hash().decode(), source_hash()
        if built != here:
            raise DepganError("libdepgan.so at %s was built from other sources (hash %s, the sources here hash to %s): "
                              "rebuild with `python -m dep_gan_im_amd.build`" % (LIB_PATH, built, here))
    lib.depgan_set_allreduce.argtypes = [vp, ALLREDUCE_FN, vp, C.c_int]
    lib.depgan_get_adam_step.argtypes = [vp, C.c_int]
    lib.depgan_get_adam_step.restype = C.c_long
    lib.depgan_set_adam_step.argtypes = [vp, C.c_int, C.c_long]
    lib.depgan_gen_iteration.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_long, vp, vp, vp,
                                         C.c_int, fp, ip]
    lib.depgan_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.depgan_destroy.argtypes = [vp]
    lib.depgan_destroy.restype = None
    lib.depgan_set_stream.argtypes = [vp, vp]
    lib.depgan_param_count.argtypes = [vp, C.c_int]
    lib.depgan_param_info.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_int, ip, ip, C.POINTER(C.c_long), ip]
    lib.depgan_arena_floats.argtypes = [vp, C.c_int, C.c_int]
    lib.depgan_arena_floats.restype = C.c_long
    lib.depgan_arena_ptr.argtypes = [vp, C.c_int, C.c_int]
    lib.depgan_arena_ptr.restype = vp
    lib.depgan_weights_changed.argtypes = [vp, C.c_int]
    lib.depgan_g_forward.argtypes = [vp, vp, vp, vp, C.c_int]
    lib.depgan_d_forward.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    lib.depgan_critic_grads.argtypes = [vp, C.c_int, vp, vp, vp, vp, fp]
    lib.depgan_critic_step.argtypes = [vp, C.c_int, vp, vp, vp, vp, fp]
    lib.depgan_g_eval.argtypes = [vp, vp, vp, vp, fp]
    lib.depgan_g_grads.argtypes = [vp, vp, vp, vp, fp]
    lib.depgan_g_eval_multi.argtypes = [vp, vp, vp, vp, C.c_int, fp, fp]
    lib.depgan_g_step.argtypes = [vp, vp, vp, vp, fp]
    lib.depgan_apply_adam.argtypes = [vp, C.c_int]
    lib.depgan_last_sums.argtypes = [vp, fp]
    lib.depgan_profile_enable.argtypes = [vp, C.c_int]
    lib.depgan_profile_read.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_double)]
    lib.depgan_profile_read_bytes.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
    lib.depgan_profile_reset.argtypes = [vp]
    lib.depgan_profile_dump.argtypes = [vp, C.c_char_p]
    lib.depgan_op_conv2d.argtypes = [vp, vp, vp, vp] + [C.c_int] * 8 + [vp]
    lib.depgan_op_conv2d_bwd_data.argtypes = [vp, vp, vp] + [C.c_int] * 7 + [vp]
    lib.depgan_op_conv2d_wgrad.argtypes = [vp, vp, vp] + [C.c_int] * 6 + [vp]
    lib.depgan_op_conv2d_wgrad_bf16.argtypes = [vp, vp, vp] + [C.c_int] * 6 + [vp]
    lib.depgan_eval_accumulate.argtypes = [vp, vp, vp, C.c_long, vp]
    lib.depgan_eval_divide.argtypes = [vp, C.c_long, C.c_double, vp]
    lib.depgan_eval_counts.argtypes = [vp, C.c_int] + [vp] * 7 + [C.c_long, C.c_double, C.POINTER(C.c_longlong), vp]
    lib.depgan_data_prep_scratch_floats.argtypes = [C.c_int] * 3
    lib.depgan_data_prep_scratch_floats.restype = C.c_size_t
    lib.depgan_data_prep_subject.argtypes = [vp] * 7 + [C.c_int] * 4 + [vp] * 4
    lib.depgan_data_zscore_scratch_floats.argtypes = [C.c_int] * 3
    lib.depgan_data_zscore_scratch_floats.restype = C.c_size_t
    lib.depgan_data_prep_zscore.argtypes = [vp] * 3 + [C.c_int] * 3 + [vp] * 4
    lib.depgan_data_mask_slices.argtypes = [vp] * 3 + [C.c_int] * 3 + [vp] * 2
    lib.depgan_labels_to_onehot.argtypes = [vp, C.c_long, C.c_int, vp, vp]
    lib.depgan_eval_accumulate_channels.argtypes = [vp, vp, vp, C.c_long, C.c_int, vp]
    lib.depgan_eval_label_counts.argtypes = [vp, C.c_int] + [vp] * 5 + [C.c_long, vp, C.POINTER(C.c_longlong), vp]
    lib.depgan_op_maxpool.argtypes = [vp, vp] + [C.c_int] * 4 + [vp]
    lib.depgan_op_deconv2x2.argtypes = [vp] * 6 + [C.c_int] * 6 + [vp]
    lib.depgan_op_deconv2x2_wgrad.argtypes = [vp] * 4 + [C.c_int] * 5 + [vp]
    lib.depgan_op_conv2d_stamps.argtypes = [vp, vp, vp] + [C.c_int] * 6 + [vp, C.c_int, vp]
    L, f, u = C.c_long, C.c_float, C.c_uint
    lib.depgan_op_bn_moments.argtypes = [vp, L, L, L] + [C.c_int] * 4 + [vp, vp, L, vp]
    lib.depgan_op_bn_backward.argtypes = [vp] * 3 + [L] * 3 + [C.c_int] * 4 + [vp] * 3 + [f] * 3 + [vp, vp, L, vp]
    lib.depgan_op_affine_act.argtypes = [vp] * 4 + [L] * 3 + [vp] * 4 + [C.c_int] * 6 + [u, f, vp]
    lib.depgan_op_softmax_ce4.argtypes = [vp] * 5 + [L, vp]
    lib.depgan_op_bn_rows_fwd.argtypes = [vp, vp] + [C.c_int] * 3 + [vp, vp] + [f] * 3 + [vp] * 4 + [C.c_int, vp]
    lib.depgan_op_bn_rows_bwd.argtypes = [vp] * 4 + [C.c_int] * 3 + [vp] * 5 + [vp]
    lib.depgan_op_small_gemm.argtypes = [C.c_int] + [vp] * 4 + [C.c_int] * 3 + [vp]
    i = C.c_int
    lib.depgan_op_unpool_mask.argtypes = [vp, L, L, L] * 4 + [i] * 4 + [vp]
    lib.depgan_op_gather_pool.argtypes = [vp, L, L, L] * 3 + [i] * 4 + [vp]
    lib.depgan_op_head.argtypes = [i] + [vp] * 5 + [L, i, i, vp]
    lib.depgan_op_critic_tail_fwd.argtypes = [vp] * 7 + [i] * 3 + [vp]
    lib.depgan_op_critic_tail_bwd.argtypes = [vp] * 4 + [i, vp] + [i] * 3 + [vp]
    lib.depgan_op_critic_tail_wgrad.argtypes = [vp] * 5 + [i] * 3 + [vp] * 4 + [i] * 3 + [L, vp]
    lib.depgan_op_colsum.argtypes = [vp, L, L, L] + [i] * 4 + [vp] * 3 + [i, vp, L, vp]
    lib.depgan_op_sum.argtypes = [vp, L, vp, L, vp]
    lib.depgan_op_critic_inputs.argtypes = [vp, vp, i] + [vp] * 3 + [i, L, i, vp]
    lib.depgan_op_gp_u0.argtypes = [vp] * 4 + [f, i, L, L, vp]
    lib.depgan_op_critic_stats.argtypes = [vp] * 3 + [i, vp]
    lib.depgan_op_gloss_sums.argtypes = [vp, i, vp, vp, f, vp, L, L, vp]
    lib.depgan_op_g_dpre.argtypes = [vp, i] + [vp] * 5 + [i, L, vp]
    lib.depgan_op_film_bwd.argtypes = [vp] * 4 + [i] + [vp] * 3 + [i, L, i, L, vp]
    lib.depgan_op_bn_prepare_batch.argtypes = [vp, vp, i, f, vp]
    lib.depgan_op_bn_gamma_grad_batch.argtypes = [vp, vp, i, vp]
    lib.depgan_op_noise_fwd.argtypes = [vp] * 6 + [i, vp]
    lib.depgan_op_noise_bwd.argtypes = [vp] * 10 + [i, L, vp]
    lib.depgan_op_best_noise.argtypes = [vp, i, vp, L, vp, vp, vp]
    lib.depgan_op_round_bf16_masked.argtypes = [vp] * 3 + [L, vp]
    lib.depgan_uresnet_grads.argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint, fp]
    lib.depgan_uresnet_step.argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint, fp]
    lib.depgan_uresnet_eval.argtypes = [vp, vp, vp, vp, C.c_int, fp]
    lib.depgan_debug_capture.argtypes = [vp, C.c_int]
    lib.depgan_rccl_unique_id.argtypes = [vp]
    lib.depgan_rccl_init.argtypes = [vp, vp, C.c_int, C.c_int]
    lib.depgan_rccl_broadcast.argtypes = [vp, vp, C.c_long, C.c_int]
    lib.depgan_rccl_info.argtypes = [vp, ip, ip, C.POINTER(C.c_long)]
    lib.depgan_rccl_shutdown.argtypes = [vp]
    lib.depgan_debug_tensor.argtypes = [vp, C.c_char_p, vp, C.c_long, ip]
    # generator forward with bf16 activation storage: bf16 tensors are void pointers + (sB, sY, sX) in elements
    lib.depgan_g_forward_bf16s.argtypes = [vp, vp, vp, vp, i]
    lib.depgan_debug_tensor_bf16s.argtypes = [vp, C.c_char_p, vp, L, ip]
    lib.depgan_op_conv2d_bf16s.argtypes = [vp, L, L, L] + [vp] * 6 + [i] + [vp, L, L, L] * 2 + [vp] + [i] * 7 + [vp]
    lib.depgan_op_deconv2x2_bf16s.argtypes = [vp, L, L, L] + [vp] * 4 + [vp, L, L, L] + [i] * 6 + [vp]
    lib.depgan_op_edge_conv_bf16s.argtypes = [vp] * 5 + [vp, L, L, L] + [i] * 6 + [vp]
    lib.depgan_op_head_bf16s.argtypes = [vp] * 4 + [L, i, i, vp]
    lib.depgan_op_head_softmax_bf16s.argtypes = [vp, L] + [vp] * 4 + [L, i, vp]
    lib.depgan_op_conv2d_head_bf16s.argtypes = ([vp, L, L, L] + [vp] * 6 + [i] + [vp, L, L, L] * 2 + [vp] + [i] * 7 +
                                                [vp] * 3 + [i, i, vp])
    # bf16 storage for the forward-only generator passes of the training closures
    lib.depgan_set_fwd_only_storage.argtypes = [vp, i]
    lib.depgan_get_fwd_only_storage.argtypes = [vp]
    # bf16 storage for the generator update: setter, debug surface and the operators of its backward
    lib.depgan_set_g_update_storage.argtypes = [vp, i]
    lib.depgan_get_g_update_storage.argtypes = [vp]
    lib.depgan_set_critic16_pipe.argtypes = [vp, i]
    lib.depgan_get_critic16_pipe.argtypes = [vp]
    lib.depgan_debug_film_decision_bf16s.argtypes = [vp, C.c_char_p, vp, L, ip]
    lib.depgan_op_conv2d_film_train_bf16s.argtypes = ([vp, L, L, L] + [vp] * 6 + [i] + [vp, L, L, L] * 2 + [vp, vp] +
                                                      [i] * 6 + [vp])
    lib.depgan_op_conv2d_wgrad_bf16s.argtypes = [vp, L, L, L] * 2 + [vp, vp] + [i] * 7 + [vp]
    lib.depgan_op_conv2d_bwd_data_bf16s.argtypes = [vp, L, L, L] + [vp] + [vp, L, L, L] * 3 + [i] * 6 + [vp]
    lib.depgan_op_unpool_mask_bf16s.argtypes = [vp, L, L, L] * 4 + [i] * 4 + [vp]
    lib.depgan_op_film_bwd_bf16s.argtypes = [vp] * 4 + [i] + [vp] * 3 + [i, L, i, vp]
    lib.depgan_op_head_bwd_bf16s.argtypes = [i, vp, L] + [vp] * 3 + [L, i, vp]
    # the fp32 convolution kernels with views and the whole fused epilogue (tests/test_gpu_fused_ops.py)
    lib.depgan_op_conv2d_fused.argtypes = ([vp, L, L, L] + [vp] * 6 + [i] + [vp, L, L, L] * 5 + [vp] * 3 + [i] * 12 +
                                           [vp])
    lib.depgan_op_deconv2x2_igemm.argtypes = [i] + [vp, L, L, L] + [vp] * 4 + [vp, L, L, L] * 2 + [i] * 7 + [vp]
    lib.depgan_op_conv2d_wgrad_ex.argtypes = [vp, L, L, L] * 2 + [vp] * 3 + [i] * 3 + [vp] * 3 + [i] * 7 + [vp]
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().depgan_last_error()
        raise DepganError("%s failed (status %d): %s" % (what or "libdepgan call", rc,
                                                         msg.decode() if msg else "?"))


_hip = None


def hip():
    """libamdhip64 for raw device copies (weights in/out of the C-side arenas)."""
    global _hip
    if _hip is None:
        last = None
        for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
            try:
                _hip = C.CDLL(name)
                break
            except OSError as e:  # pragma: no cover
                last = e
        if _hip is None:
            raise DepganError("cannot load libamdhip64: %s" % last)
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipDeviceSynchronize.argtypes = []
    return _hip


H2D, D2H, D2D = 1, 2, 3


def memcpy(dst, src, nbytes, kind):
    rc = hip().hipMemcpy(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), C.c_int(kind))
    if rc != 0:
        raise DepganError("hipMemcpy failed with status %d" % rc)
