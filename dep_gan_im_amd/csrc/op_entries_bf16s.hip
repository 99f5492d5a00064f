// The single-operator entries of the bf16-activation-storage kernels (depgan_op_*_bf16s; igemm_bf16s.hip,
// igemm_bf16s_train.hip, igemm_bf16_mh.hip, wgrad_bf16s.hip, ops_bf16s.hip): the unit-test surface next to op_entries.hip.
// Each plans, packs and launches on its own stream and workspace; nothing here touches a context's state.
// Explicit view strides in ELEMENTS, stream last, checks before any HIP call; a view may have sB = 0 (one sample read by
// every batch index).
#include "model.h"

#include <stdio.h>
#include <string.h>

static int op_conv2d_bf16s_impl(const char* who, const void* in, long isB, long isY, long isX, const float* w_hwio,
                                const float* bias, const float* scale, const float* shift, const float* film_mul,
                                const float* film_add, int film_ld, const void* res, long rsB, long rsY, long rsX,
                                void* out, long osB, long osY, long osX, void* pool, int B, int H, int W, int Cin, int Cout,
                                int KS, int relu, const float* head_w, const float* head_b, float* head_out, int tanh_act,
                                int skip_out, void* stream) {
  if (op_view_bad_broadcast(in, isB, isY, isX) || op_view_bad_broadcast(out, osB, osY, osX) || !w_hwio || B < 1 || H < 1 || W < 1 || Cin < 1 ||
      Cout < 1 || (res && op_view_bad_broadcast(res, rsB, rsY, rsX))) {
    dg_set_error("%s: null or non-positive argument", who);
    return DG_ERR_ARG;
  }
  if (KS != 1 && KS != 3) { dg_set_error("%s: KS must be 1 or 3", who); return DG_ERR_ARG; }
  const ConvPlan pl = dg_plan_conv_bf16(KS, Cin, Cout);
  if (!dg_plan_bf16(pl) || (Cin % 8)) { dg_set_error("%s: the bf16 MFMA kernel does not cover %d -> %d", who, Cin, Cout); return DG_ERR_UNSUPPORTED; }
  if (head_out && (KS != 3 || Cout != 32)) {
    dg_set_error("%s: the fused head needs a 3x3 convolution to exactly 32 channels (KS %d, Cout %d)", who, KS, Cout);
    return DG_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  ConvArgsH a = conv_args_h(op_view_h(in, isB, isY, isX), op_view_h(out, osB, osY, osX), B, H, W, Cin, Cout);
  a.ep.bias = bias; a.ep.scale = scale; a.ep.shift = shift;
  a.ep.film_mul = film_mul; a.ep.film_add = film_add; a.ep.film_ld = film_ld;
  a.ep.res = op_view_h_or_null(res, rsB, rsY, rsX);
  a.ep.relu = relu;
  a.ep.pool = pool ? make_view_h(reinterpret_cast<__bf16*>(pool), H / 2, W / 2, Cout) : null_view_h();
  a.ep.head_w = head_w; a.ep.head_b = head_b; a.ep.head_out = head_out;
  a.ep.head_tanh = tanh_act; a.ep.head_skip_out = head_out ? skip_out : 0;
  DGCHECK(dg_conv_bf16s_check(KS, a));   // alignment, pool parity, FiLM pairs: before the temporary and the pack launch
  DevTmp wp(st);
  DGCHECK(wp.alloc(pl.packedFloats * sizeof(float)));
  DGCHECK(dg_pack_weights(pl, w_hwio, Cin, Cout, 0, 0, 0, nullptr, wp.as<float>(), st));
  a.w = wp.as<float>();
  return dg_conv_bf16s(KS, a, st);
}

int depgan_op_conv2d_bf16s(const void* in, long isB, long isY, long isX, const float* w_hwio, const float* bias,
                           const float* scale, const float* shift, const float* film_mul, const float* film_add,
                           int film_ld, const void* res, long rsB, long rsY, long rsX, void* out, long osB, long osY,
                           long osX, void* pool, int B, int H, int W, int Cin, int Cout, int KS, int relu, void* stream) {
  return op_conv2d_bf16s_impl("op_conv2d_bf16s", in, isB, isY, isX, w_hwio, bias, scale, shift, film_mul, film_add, film_ld,
                              res, rsB, rsY, rsX, out, osB, osY, osX, pool, B, H, W, Cin, Cout, KS, relu, nullptr, nullptr,
                              nullptr, 0, 0, stream);
}

int depgan_op_conv2d_head_bf16s(const void* in, long isB, long isY, long isX, const float* w_hwio, const float* bias,
                                const float* scale, const float* shift, const float* film_mul, const float* film_add,
                                int film_ld, const void* res, long rsB, long rsY, long rsX, void* out, long osB,
                                long osY, long osX, void* pool, int B, int H, int W, int Cin, int Cout, int KS, int relu,
                                const float* head_w, const float* head_b, float* head_out, int tanh_act, int skip_out,
                                void* stream) {
  if (!head_w || !head_b || !head_out) { dg_set_error("op_conv2d_head_bf16s: null head argument"); return DG_ERR_ARG; }
  return op_conv2d_bf16s_impl("op_conv2d_head_bf16s", in, isB, isY, isX, w_hwio, bias, scale, shift, film_mul, film_add,
                              film_ld, res, rsB, rsY, rsX, out, osB, osY, osX, pool, B, H, W, Cin, Cout, KS, relu, head_w,
                              head_b, head_out, tanh_act, skip_out, stream);
}

int depgan_op_deconv2x2_bf16s(const void* in, long isB, long isY, long isX, const float* w_hwoi, const float* bias,
                              const float* scale, const float* shift, void* out, long osB, long osY, long osX, int B,
                              int H, int W, int Cin, int Cout, int relu, void* stream) {
  if (op_view_bad_broadcast(in, isB, isY, isX) || op_view_bad_broadcast(out, osB, osY, osX) || !w_hwoi || B < 1 || H < 1 || W < 1 || Cin < 1 ||
      Cout < 1) {
    dg_set_error("op_deconv2x2_bf16s: null or non-positive argument");
    return DG_ERR_ARG;
  }
  const ConvPlan pl = dg_plan_conv_bf16(1, Cin, Cout);
  if (!dg_plan_bf16(pl) || (Cin % 8)) { dg_set_error("op_deconv2x2_bf16s: the bf16 MFMA kernel does not cover %d -> %d", Cin, Cout); return DG_ERR_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  const TViewH o = op_view_h(out, osB, osY, osX);   // the (2H, 2W) output
  ConvArgsH a = conv_args_h(op_view_h(in, isB, isY, isX), o, B, H, W, Cin, Cout);
  a.ep.bias = bias; a.ep.scale = scale; a.ep.shift = shift; a.ep.relu = relu;
  a.ep.res = null_view_h();
  a.ep.pool = null_view_h();
  const float* panels[4] = {nullptr, nullptr, nullptr, nullptr};
  deconv_groups(&a, o, panels);          // the groups' output offsets are part of what is checked
  DGCHECK(dg_conv_bf16s_check(1, a));
  DevTmp wp(st);
  DGCHECK(wp.alloc(4 * pl.packedFloats * sizeof(float)));
  for (int t = 0; t < 4; ++t) {
    float* dst = wp.as<float>() + (size_t)t * pl.packedFloats;
    DGCHECK(dg_pack_weights(pl, w_hwoi + (size_t)t * Cout * Cin, Cin, Cout, 1, 0, 0, nullptr, dst, st));
    panels[t] = dst;
  }
  deconv_groups(&a, o, panels);
  return dg_conv_bf16s(1, a, st);
}

int depgan_op_edge_conv_bf16s(const float* in, const float* w_hwio, const float* bias, const float* scale,
                              const float* shift, void* out, long osB, long osY, long osX, int B, int H, int W, int Cin,
                              int Cout, int relu, void* stream) {
  if (!in || !w_hwio || op_view_bad_broadcast(out, osB, osY, osX) || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) {
    dg_set_error("op_edge_conv_bf16s: null or non-positive argument");
    return DG_ERR_ARG;
  }
  EdgeArgsH e;
  memset(&e, 0, sizeof(e));
  e.in = in; e.w = w_hwio; e.bias = bias; e.scale = scale; e.shift = shift;
  e.out = op_view_h(out, osB, osY, osX);
  e.B = B; e.H = H; e.W = W; e.Cin = Cin; e.Cout = Cout; e.relu = relu;
  return dg_edge_conv_bf16s(e, (hipStream_t)stream);
}

int depgan_op_head_softmax_k_bf16s(const void* a, long ld, const float* w, const float* b, float* probs, float* logits,
                                   long P, int C, int K, void* stream) {
  if (!a || !w || !b || !probs || P < 1 || C < 1 || ld < 1) { dg_set_error("op_head_softmax_bf16s: null or non-positive argument"); return DG_ERR_ARG; }
  if (K < 2 || K > DEPGAN_MAX_HEAD_CLASSES) {
    dg_set_error("op_head_softmax_k_bf16s: %d classes (2 to %d)", K, DEPGAN_MAX_HEAD_CLASSES);
    return DG_ERR_ARG;
  }
  return dg_head_softmax_bf16s(reinterpret_cast<const __bf16*>(a), ld, w, b, probs, logits, P, C, K, (hipStream_t)stream);
}
int depgan_op_head_softmax_bf16s(const void* a, long ld, const float* w, const float* b, float* probs, float* logits,
                                 long P, int C, void* stream) {
  return depgan_op_head_softmax_k_bf16s(a, ld, w, b, probs, logits, P, C, 4, stream);
}

int depgan_op_head_bf16s(const void* a, const float* w, const float* b, float* out, long P, int C, int tanh_act,
                         void* stream) {
  if (!a || !w || !b || !out || P < 1 || C < 1) { dg_set_error("op_head_bf16s: null or non-positive argument"); return DG_ERR_ARG; }
  return dg_head_bf16s(reinterpret_cast<const __bf16*>(a), C, w, b, out, P, C, tanh_act, (hipStream_t)stream);
}

// ---- the operators of the generator update (bf16s_train.h) ----

int depgan_op_conv2d_film_train_bf16s(const void* in, long isB, long isY, long isX, const float* w_hwio, const float* bias,
                                      const float* scale, const float* shift, const float* film_mul, const float* film_add,
                                      int film_ld, const void* res, long rsB, long rsY, long rsX, void* out, long osB,
                                      long osY, long osX, void* u_out, unsigned char* dec_bits, int B, int H, int W, int Cin,
                                      int Cout, int relu, void* stream) {
  if (op_view_bad_broadcast(in, isB, isY, isX) || op_view_bad_broadcast(out, osB, osY, osX) || !w_hwio || !film_mul || !film_add || !u_out || !dec_bits ||
      B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (res && op_view_bad_broadcast(res, rsB, rsY, rsX))) {
    dg_set_error("op_conv2d_film_train_bf16s: null or non-positive argument");
    return DG_ERR_ARG;
  }
  const ConvPlan pl = dg_plan_conv_bf16(3, Cin, Cout);
  if (!dg_plan_bf16(pl) || (Cin % 8)) { dg_set_error("op_conv2d_film_train_bf16s: the bf16 MFMA kernel does not cover %d -> %d", Cin, Cout); return DG_ERR_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  ConvArgsHT a;
  static_cast<ConvArgsH&>(a) = conv_args_h(op_view_h(in, isB, isY, isX), op_view_h(out, osB, osY, osX), B, H, W, Cin, Cout);
  a.ep.bias = bias; a.ep.scale = scale; a.ep.shift = shift;
  a.ep.film_mul = film_mul; a.ep.film_add = film_add; a.ep.film_ld = film_ld;
  a.ep.res = op_view_h_or_null(res, rsB, rsY, rsX);
  a.ep.relu = relu;
  a.ep.pool = null_view_h();
  a.u = make_view_h(reinterpret_cast<__bf16*>(u_out), H, W, Cout);
  a.fdec = dec_bits;
  DGCHECK(dg_conv_bf16s_train_check(a));
  DevTmp wp(st);
  DGCHECK(wp.alloc(pl.packedFloats * sizeof(float)));
  DGCHECK(dg_pack_weights(pl, w_hwio, Cin, Cout, 0, 0, 0, nullptr, wp.as<float>(), st));
  a.w = wp.as<float>();
  return dg_conv_bf16s_train(a, st);
}

int depgan_op_conv2d_wgrad_bf16s(const void* x, long xsB, long xsY, long xsX, const float* dy, long dsB, long dsY, long dsX,
                                 float* dw, float* colsum, int B, int H, int W, int Cin, int Cout, int KS, int oi,
                                 void* stream) {
  if (op_view_bad_broadcast(x, xsB, xsY, xsX) || op_view_bad_broadcast(dy, dsB, dsY, dsX) || !dw || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) {
    dg_set_error("op_conv2d_wgrad_bf16s: null or non-positive argument");
    return DG_ERR_ARG;
  }
  if (KS != 1 && KS != 3) { dg_set_error("op_conv2d_wgrad_bf16s: KS must be 1 or 3"); return DG_ERR_ARG; }
  if (!dg_wgrad_bf16s_supported(KS, Cin, Cout)) { dg_set_error("op_conv2d_wgrad_bf16s: shape not covered (%d -> %d)", Cin, Cout); return DG_ERR_UNSUPPORTED; }
  const ColSum cs = {B, nullptr, colsum, nullptr};   // over all samples: the entry knows no other form
  return op_wgrad("op_conv2d_wgrad_bf16s", KS, op_view_h(x, xsB, xsY, xsX), op_view(dy, dsB, dsY, dsX), B, H, W, Cin, Cout,
                  true, nullptr, dw, nullptr, 0, oi, colsum ? &cs : nullptr, (hipStream_t)stream);
}

// KS = 3: dx = mask(conv_bwd_data(dy, w_hwio) + res); KS = 1 with deconv = 1: dy is the (2H, 2W) upstream gradient of a
// 2x2 / stride-2 transposed convolution with HWOI weights (Cin of the transposed convolution = channels of dx)
int depgan_op_conv2d_bwd_data_bf16s(const float* dy, long dsB, long dsY, long dsX, const float* w, const float* res,
                                    long rsB, long rsY, long rsX, const void* mask, long msB, long msY, long msX, float* dx,
                                    long osB, long osY, long osX, int B, int H, int W, int Cin, int Cout, int deconv,
                                    void* stream) {
  if (op_view_bad_broadcast(dy, dsB, dsY, dsX) || op_view_bad_broadcast(dx, osB, osY, osX) || !w || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 ||
      (res && op_view_bad_broadcast(res, rsB, rsY, rsX)) || (mask && op_view_bad_broadcast(mask, msB, msY, msX))) {
    dg_set_error("op_conv2d_bwd_data_bf16s: null or non-positive argument");
    return DG_ERR_ARG;
  }
  if (deconv != 0 && deconv != 1) { dg_set_error("op_conv2d_bwd_data_bf16s: deconv must be 0 or 1"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  ConvArgs a = conv_args(null_view(), op_view(dx, osB, osY, osX), B, H, W, Cout, Cin);
  a.ep.res = op_view_or_null(res, rsB, rsY, rsX);
  const TViewH mh = op_view_h_or_null(mask, msB, msY, msX);
  const TView d = op_view(dy, dsB, dsY, dsX);
  DevTmp wp(st);
  ConvPlan pl;
  if (!deconv) {
    pl = dg_plan_conv_bf16(3, Cout, Cin);
    if (!dg_plan_bf16(pl)) { dg_set_error("op_conv2d_bwd_data_bf16s: the bf16 MFMA kernel does not cover %d -> %d", Cout, Cin); return DG_ERR_UNSUPPORTED; }
    DGCHECK(wp.alloc(pl.packedFloats * sizeof(float)));
    DGCHECK(dg_pack_weights(pl, w, Cin, Cout, 0, 1, 1, nullptr, wp.as<float>(), st));
    a.in = d;
  } else {
    const ConvPlan pb = dg_plan_conv_bf16(1, Cout, Cin);
    pl = dg_plan_conv_bf16(1, 4 * Cout, Cin);
    if (!dg_plan_bf16(pb) || !dg_plan_bf16(pl) || (Cout % pb.CK) || pl.packedFloats != 4 * pb.packedFloats) {
      dg_set_error("op_conv2d_bwd_data_bf16s: the gathered 1x1 form does not cover %d -> %d", Cout, Cin);
      return DG_ERR_UNSUPPORTED;
    }
    DGCHECK(wp.alloc(pl.packedFloats * sizeof(float)));
    // the four per-tap panels interleaved per channel tile, as refresh_generator builds GLayer::wpb_all
    const size_t per_nt = (size_t)pb.nCC * pb.NT * pb.CK;   // bf16 elements of one channel tile of one tap
    PackJob jobs[4];
    for (int t = 0; t < 4; ++t)
      DGCHECK(dg_pack_job(pb, w + (size_t)t * Cout * Cin, Cin, Cout, 1, 1, 0, nullptr,
                          reinterpret_cast<float*>(wp.as<__bf16>() + (size_t)t * per_nt), 4 * per_nt, &jobs[t]));
    DGCHECK(op_pack_jobs(jobs, 4, st));
    deconv_gather_k(&a, d, Cout, pb.CK);
  }
  a.w = wp.as<float>();
  return dg_conv_bf16_mh(pl, a, mh, st);
}

int depgan_op_unpool_mask_bf16s(const float* dpool, long dsB, long dsY, long dsX, const void* a, long asB, long asY, long asX,
                                const float* skip, long ssB, long ssY, long ssX, float* out, long osB, long osY, long osX,
                                int B, int Ho, int Wo, int C, void* stream) {
  if (op_view_bad_broadcast(dpool, dsB, dsY, dsX) || op_view_bad_broadcast(a, asB, asY, asX) || op_view_bad_broadcast(out, osB, osY, osX) || (skip && op_view_bad_broadcast(skip, ssB, ssY, ssX)) ||
      B < 1 || Ho < 1 || Wo < 1 || C < 1) {
    dg_set_error("op_unpool_mask_bf16s: null or non-positive argument");
    return DG_ERR_ARG;
  }
  return dg_unpool_mask_bf16s(op_view(dpool, dsB, dsY, dsX), op_view_h(a, asB, asY, asX),
                              op_view_or_null(skip, ssB, ssY, ssX), op_view(out, osB, osY, osX), B, Ho, Wo, C,
                              (hipStream_t)stream);
}

int depgan_op_film_bwd_bf16s(const float* dr, const void* u, const unsigned char* dec_bits, const float* fmul, int film_ld,
                             float* du, float* dmul, float* dadd, int B, long HW, int C, void* stream) {
  if (!dr || !u || !dec_bits || !fmul || !du || !dmul || !dadd || B < 1 || HW < 1 || C < 1 || film_ld < C) {
    dg_set_error("op_film_bwd_bf16s: null or non-positive argument");
    return DG_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t need = dg_film_bwd_bf16s_scratch(B, C);
  DevTmp scratch(st);
  DGCHECK(scratch.alloc(need * sizeof(float)));
  return dg_film_bwd_bf16s(dr, reinterpret_cast<const __bf16*>(u), dec_bits, fmul, film_ld, du, dmul, dadd, B, HW, C,
                           scratch.as<float>(), need, st);
}

// backward = 0: out[c] = sum_p dpre[p] a[p ld + c] (C floats); backward = 1: out[p][c] = (a > 0) ? dpre[p] w[c] : 0
int depgan_op_head_bwd_bf16s(int backward, const void* a, long ld, const float* w, const float* dpre, float* out, long P,
                             int C, void* stream) {
  if (!a || !dpre || !out || P < 1 || C < 1 || ld < 1 || (backward && !w)) {
    dg_set_error("op_head_bwd_bf16s: null or non-positive argument");
    return DG_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (backward) return dg_head_bwd_bf16s(dpre, w, reinterpret_cast<const __bf16*>(a), ld, out, P, C, st);
  const size_t need = dg_colsum_rowmul_bf16s_scratch(P, C);
  DevTmp scratch(st);
  DGCHECK(scratch.alloc(need * sizeof(float)));
  return dg_colsum_rowmul_bf16s(reinterpret_cast<const __bf16*>(a), ld, P, C, dpre, out, scratch.as<float>(), need, st);
}
