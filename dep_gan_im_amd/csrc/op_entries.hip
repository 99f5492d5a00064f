// The single-operator entries (depgan_op_*): the unit-test surface of the kernels.  Each plans, packs and launches on
// its own stream and workspace; nothing here touches a context's state.
#include "model.h"

#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

int op_pack_jobs(PackJob* jobs, int n, hipStream_t st) {
  const unsigned nb = dg_pack_layout(jobs, n);
  DevTmp jd(st);
  DGCHECK(jd.alloc(n * sizeof(PackJob)));
  hipError_t e = hipMemcpyAsync(jd.p, jobs, n * sizeof(PackJob), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) { dg_set_error("op_pack_jobs: upload failed: %s", hipGetErrorString(e)); return DG_ERR_HIP; }
  return dg_pack_weights_batch(jd.as<PackJob>(), n, nb, st);
}

static int op_alloc(DevTmp* t, size_t floats, const char* who) {
  if (t->alloc((floats ? floats : 1) * sizeof(float)) != DG_OK) {
    dg_set_error("%s: out of device memory (%zu floats)", who, floats);
    return DG_ERR_HIP;
  }
  return DG_OK;
}

// The weight gradient of an operator entry as the model runs it (wgrad_run), on workspaces of this call sized from the
// choice: the slabs, and for column sums one partial row per col_rows or the scratch of the streaming pass.
template <typename XV>
int op_wgrad(const char* who, int KS, XV x, TView dy, int B, int H, int W, int Cin, int Cout, bool bf16,
             const float* scale, float* dw, float* raw, int accumulate, int oi, const ColSum* cs, hipStream_t st) {
  DgWgradChoice ch;
  DGCHECK(dg_wgrad_choose(KS, B, H, W, Cin, Cout, bf16, std::is_same<XV, TViewH>::value, &ch));
  WgradWs ws;
  memset(&ws, 0, sizeof(ws));
  ws.partFloats = ch.part_floats;
  ws.scratchFloats = !cs ? 0 : ch.col_rows ? (size_t)ch.col_rows * Cout : dg_colsum_scratch(cs->B, H, W, Cout);
  ws.bf16 = bf16;
  ws.st = st;
  DevTmp part(st), scratch(st);
  DGCHECK(op_alloc(&part, ws.partFloats, who));
  DGCHECK(op_alloc(&scratch, ws.scratchFloats, who));
  ws.part = part.as<float>();
  ws.scratch = scratch.as<float>();
  return wgrad_run(ws, KS, x, dy, B, H, W, Cin, Cout, scale, dw, raw, accumulate, oi, cs);
}
template int op_wgrad<TViewH>(const char*, int, TViewH, TView, int, int, int, int, int, bool, const float*, float*, float*,
                              int, int, const ColSum*, hipStream_t);   // op_entries_bf16s.hip

extern "C" {

// ---- single operators (unit tests) ----
// a: views, sizes and epilogue of the launch (bwd: Cin / Cout already in their launch roles); w_hwio (KS, KS, Cin, Cout)
// of the layer.  Plans, packs and launches on the kernel `path` names; what that kernel does not cover is an error.
// What an operator path means: the plan function it takes, the routes of the chain it leaves open (dg_conv_prepare),
// and below the refusals that belong to it.  0 (and any other number) is the model's choice for the fp32 tile plan.
static ConvPlan op_conv_plan(int path, int KS, int ci, int co) {
  switch (path) {
    case 2: return dg_plan_direct();
    case 3: return dg_plan_conv_bf16(KS, ci, co);
    case 4: case 5: return dg_plan_conv_split(KS, ci, co, path == 5 ? 3 : 2);
    case 6: case 7: return dg_plan_conv_items(KS, ci, co, 1L << 30);
    case 8: return KS == 3 ? dg_plan_conv_wino(ci, co) : dg_plan_conv(KS, ci, co);
    case 10: return dg_plan_conv_bf16_n16(KS, ci, co);
  }
  return dg_plan_conv(KS, ci, co);
}
static unsigned op_conv_routes(int path) {
  // 6 and 1: the workgroup-tile kernel itself (the reference the wave-private kernels must match bit for bit)
  return (path == 1 || path == 6) ? DG_ROUTE_TILE : path == 7 ? DG_ROUTE_WP : path == 9 ? DG_ROUTE_WS5 : DG_ROUTE_ALL;
}
#define OP_REFUSE(status, ...) do { dg_set_error(__VA_ARGS__); return status; } while (0)
static int op_conv_run(ConvArgs a, const float* w_hwio, int Cin, int Cout, int KS, int path, int bwd, hipStream_t st) {
  const int ci = a.Cin, co = a.Cout;
  const ConvPlan pl = op_conv_plan(path, KS, ci, co);
  switch (path) {   // decided before any HIP call
    case 10:
      if (KS != 5) OP_REFUSE(DG_ERR_ARG, "op_conv: path 10 is the 16-channel 5x5 bf16 kernel, KS must be 5");
      if (!a.in.p || !a.out.p || !w_hwio) OP_REFUSE(DG_ERR_ARG, "op_conv: null operand");
      if (a.ep.head_w || a.ep.head_b || a.ep.head_out) OP_REFUSE(DG_ERR_ARG, "op_conv: path 10 has no fused head");
      if (!dg_plan_bf16(pl) || pl.MF != 16) OP_REFUSE(DG_ERR_UNSUPPORTED, "op_conv: the 16-channel bf16 kernel does not cover a launch of %d -> %d channels", ci, co);
      break;
    case 8:
      if (!dg_plan_wino(pl) || !dg_conv_wino_supported(pl, a)) OP_REFUSE(DG_ERR_UNSUPPORTED, "op_conv: the Winograd kernel does not cover this shape");
      break;
    case 6: case 7:
      if (pl.CK != 8) OP_REFUSE(DG_ERR_UNSUPPORTED, "op_conv: the 8-channel-chunk variant does not cover this shape");
      break;
    case 3: case 4: case 5:
      if (!pl.planes) OP_REFUSE(DG_ERR_UNSUPPORTED, "op_conv: the bf16 MFMA kernel does not cover this shape");
      break;
    case 9:
      // path 9 names a 5x5 kernel: another KS is a bad argument (status 1, as for a path number that does not exist),
      // what the 5x5 kernel does not cover is status 3
      if (KS != 5) OP_REFUSE(DG_ERR_ARG, "op_conv: path 9 is the weight-stationary 5x5 kernel, KS must be 5");
      if (!dg_conv_igemm_ws5_supported(pl, a, true)) OP_REFUSE(DG_ERR_UNSUPPORTED, "op_conv: the weight-stationary 5x5 kernel does not cover this shape");
      break;
    case 1:
      if (!dg_plan_mfma(pl)) OP_REFUSE(DG_ERR_UNSUPPORTED, "op_conv: MFMA path not available for this shape");
      break;
  }
  DevTmp wp(st);
  if (dg_plan_mfma(pl)) {
    DGCHECK(wp.alloc(pl.packedFloats * sizeof(float)));
    DGCHECK(dg_pack_weights(pl, w_hwio, Cin, Cout, 0, bwd, bwd, nullptr, wp.as<float>(), st));
    a.w = wp.as<float>();
    if (path == 7 && !dg_conv_igemm_wp_supported(pl, a, true)) OP_REFUSE(DG_ERR_UNSUPPORTED, "op_conv: the wave-private kernel does not cover this shape");
  } else if (!bwd) {
    conv_set_weights(&a, pl, nullptr, w_hwio, Cin, Cout);
  } else {
    conv_set_weights_bwd(&a, pl, nullptr, w_hwio, Cin, Cout);
  }
  DgConvLaunch L;
  DGCHECK(dg_conv_prepare(pl, a, KS, op_conv_routes(path), &L));
  return dg_conv_run(L, st);
}
#undef OP_REFUSE

static int op_conv(const float* in, const float* w_hwio, const float* bias, float* out, int B, int H, int W, int Cin,
                   int Cout, int KS, int relu, int path, int bwd, hipStream_t st) {
  // bwd: compute dx = conv_bwd_data(dy=in (Cout ch), W) -> out (Cin ch)
  const int ci = bwd ? Cout : Cin, co = bwd ? Cin : Cout;
  ConvArgs a = conv_args(make_view(const_cast<float*>(in), H, W, ci), make_view(out, H, W, co), B, H, W, ci, co);
  a.ep.bias = bias;
  a.ep.relu = relu;
  return op_conv_run(a, w_hwio, Cin, Cout, KS, path, bwd, st);
}

// diagnostics: run the MFMA conv with per-workgroup phase stamps (16 x u64 per workgroup) into `stamps`
int depgan_op_conv2d_stamps(const float* in, const float* w_hwio, float* out, int B, int H, int W, int Cin, int Cout,
                            int KS, unsigned long long* stamps, int reps, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  ConvArgs a = conv_args(make_view(const_cast<float*>(in), H, W, Cin), make_view(out, H, W, Cout), B, H, W, Cin, Cout);
  a.ep.relu = 1;
  ConvPlan pl = dg_plan_conv(KS, Cin, Cout);
  if (!dg_plan_mfma(pl)) { dg_set_error("no MFMA variant"); return DG_ERR_UNSUPPORTED; }
  DevTmp wp(st);
  DGCHECK(wp.alloc(pl.packedFloats * sizeof(float)));
  DGCHECK(dg_pack_weights(pl, w_hwio, Cin, Cout, 0, 0, 0, nullptr, wp.as<float>(), st));
  a.w = wp.as<float>();
  for (int i = 0; i < reps; ++i) {
    a.dbg = (i == reps - 1) ? stamps : nullptr;
    DGCHECK(dg_conv_igemm(pl, a, st));
  }
  return DG_OK;
}

int depgan_op_conv2d(const float* in, const float* w_hwio, const float* bias, float* out, int B, int H, int W,
                     int Cin, int Cout, int KS, int relu, int path, void* stream) {
  return op_conv(in, w_hwio, bias, out, B, H, W, Cin, Cout, KS, relu, path, 0, (hipStream_t)stream);
}
int depgan_op_conv2d_bwd_data(const float* dy, const float* w_hwio, float* dx, int B, int H, int W, int Cin,
                              int Cout, int KS, int path, void* stream) {
  return op_conv(dy, w_hwio, nullptr, dx, B, H, W, Cin, Cout, KS, 0, path, 1, (hipStream_t)stream);
}
int depgan_op_conv2d_wgrad(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout, int KS,
                           void* stream) {
  return op_wgrad("op_conv2d_wgrad", KS, make_view(const_cast<float*>(x), H, W, Cin),
                  make_view(const_cast<float*>(dy), H, W, Cout), B, H, W, Cin, Cout, false, nullptr, dw, nullptr, 0, 0,
                  nullptr, (hipStream_t)stream);
}
int depgan_op_conv2d_wgrad_bf16(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout,
                                int KS, void* stream) {
  if (!dg_wgrad_bf16_supported(KS, Cin, Cout)) { dg_set_error("op_wgrad_bf16: shape not covered"); return DG_ERR_UNSUPPORTED; }
  return op_wgrad("op_conv2d_wgrad_bf16", KS, make_view(const_cast<float*>(x), H, W, Cin),
                  make_view(const_cast<float*>(dy), H, W, Cout), B, H, W, Cin, Cout, true, nullptr, dw, nullptr, 0, 0,
                  nullptr, (hipStream_t)stream);
}
static int op_deconv2x2(const float* in, const float* w_hwoi, const float* bias, const float* scale, const float* shift,
                        TView out, int B, int H, int W, int Cin, int Cout, int relu, void* stream) {
  if (!in || !w_hwoi || !out.p || B < 1 || H < 1 || W < 1) { dg_set_error("op_deconv2x2: bad argument"); return DG_ERR_ARG; }
  DeconvArgs d;
  memset(&d, 0, sizeof(d));
  d.in = in;
  d.w = w_hwoi;
  d.out = out;
  d.bias = bias; d.scale = scale; d.shift = shift; d.relu = relu;
  d.H = H; d.W = W; d.Cin = Cin; d.Cout = Cout;
  return dg_deconv_fwd(d, B, (hipStream_t)stream);
}
int depgan_op_deconv2x2(const float* in, const float* w_hwoi, const float* bias, const float* scale,
                        const float* shift, float* out, int B, int H, int W, int Cin, int Cout, int relu,
                        void* stream) {
  return op_deconv2x2(in, w_hwoi, bias, scale, shift, make_view(out, 2 * H, 2 * W, Cout), B, H, W, Cin, Cout, relu, stream);
}
int depgan_op_deconv2x2_ex(const float* in, const float* w_hwoi, const float* bias, const float* scale,
                           const float* shift, float* out, long osB, long osY, long osX, int B, int H, int W, int Cin,
                           int Cout, int relu, void* stream) {
  return op_deconv2x2(in, w_hwoi, bias, scale, shift, op_view(out, osB, osY, osX), B, H, W, Cin, Cout, relu, stream);
}
// host only: the geometry dg_deconv_fwd launches a dense layer of this shape with
int depgan_debug_deconv_fwd_plan(int B, int H, int W, int Cin, int Cout, long out[4]) {
  if (!out || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) {
    dg_set_error("debug_deconv_fwd_plan: null or non-positive argument");
    return DG_ERR_ARG;
  }
  return dg_deconv_fwd_plan(B, H, W, Cin, Cout, out);
}
int depgan_op_deconv2x2_wgrad(const float* in, const float* dout, float* dw_hwoi, float* colsum, int B, int H, int W,
                              int Cin, int Cout, void* stream) {
  if (!in || !dout || !dw_hwoi || B < 1 || H < 1 || W < 1) { dg_set_error("op_deconv2x2_wgrad: bad argument"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  DeconvWgradArgs d;
  memset(&d, 0, sizeof(d));
  d.in = in;
  d.dout = make_view(const_cast<float*>(dout), 2 * H, 2 * W, Cout);
  d.H = H; d.W = W; d.Cin = Cin; d.Cout = Cout;
  if (!dg_deconv_wgrad_supported(B, H, W, Cin, Cout, make_view(const_cast<float*>(in), H, W, Cin), d.dout)) {
    dg_set_error("op_deconv2x2_wgrad: shape %dx%dx%d %d->%d not covered by the fused kernel", B, H, W, Cin, Cout);
    return DG_ERR_UNSUPPORTED;
  }
  const size_t pf = dg_deconv_wgrad_part_floats(B, H, W, Cin, Cout);
  DevTmp part(st), col(st);
  DGCHECK(part.alloc(pf * sizeof(float)));
  if (col.alloc((pf / ((size_t)Cin * Cout)) * Cout * sizeof(float)) != DG_OK) {
    dg_set_error("op_deconv2x2_wgrad: out of memory");
    return DG_ERR_HIP;
  }
  d.part = part.as<float>();
  d.colpart = colsum ? col.as<float>() : nullptr;
  int nch = 0;
  DGCHECK(dg_deconv_wgrad(d, B, &nch, st));
  return dg_wgrad_finish_rows(d.part, nch, 4, Cin, Cout, nullptr, dw_hwoi, nullptr, 0, 1, d.colpart, 4 * nch, Cout, nullptr,
                              colsum, nullptr, st);
}
int depgan_op_maxpool(const float* in, float* out, int B, int Ho, int Wo, int C, void* stream) {
  return dg_maxpool(make_view(const_cast<float*>(in), 2 * Ho, 2 * Wo, C), make_view(out, Ho, Wo, C), B, Ho, Wo, C,
                    (hipStream_t)stream);
}

// ---- evaluation step after the path (GE:616-807): stateless, caller's stream ----
int depgan_eval_accumulate(const float* pred, const float* mask, double* acc, long n, void* stream) {
  if (!pred || !acc || n < 0) { dg_set_error("eval_accumulate: null argument"); return DG_ERR_ARG; }
  return dg_eval_accumulate(pred, mask, acc, (size_t)n, (hipStream_t)stream);
}
int depgan_eval_divide(double* acc, long n, double divisor, void* stream) {
  if (!acc || n < 0) { dg_set_error("eval_divide: null argument"); return DG_ERR_ARG; }
  return dg_eval_divide(acc, (size_t)n, divisor, (hipStream_t)stream);
}
int depgan_eval_counts(const float* x, int nicg, const double* pred, const float* code_real, const float* mask1,
                       const float* wmh1, const float* mask2, const float* wmh2, const float* prob2, long npix,
                       double thr, long long out_host[DEPGAN_EVAL_NCOUNT], void* stream) {
  if (!x || !pred || !out_host || nicg < 1 || npix < 0) { dg_set_error("eval_counts: bad argument"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  DevTmp dev(st);
  DGCHECK(dev.alloc(DEPGAN_EVAL_NCOUNT * sizeof(unsigned long long)));
  DGCHECK(dg_eval_counts(x, nicg, pred, code_real, mask1, wmh1, mask2, wmh2, prob2, (size_t)npix, thr,
                         dev.as<unsigned long long>(), st));
  unsigned long long h[DEPGAN_EVAL_NCOUNT];
  if (hipMemcpyAsync(h, dev.p, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    dg_set_error("eval_counts: copy back failed");
    return DG_ERR_HIP;
  }
  for (int k = 0; k < DEPGAN_EVAL_NCOUNT; ++k) out_host[k] = (long long)h[k];
  return DG_OK;
}


// ---- learning-phase-1 operators (train_ops.hip), as uresnet.hip calls them; each view is NHWC with the strides
// (sB, sY, sX) in floats and channel stride 1 ----
static size_t op_scratch(long scratch_floats, size_t need) { return scratch_floats > 0 ? (size_t)scratch_floats : need; }

// ---- the fp32 convolution kernels with the whole fused epilogue and strided views (unit tests) ----

int depgan_op_conv2d_fused(const float* in, long isB, long isY, long isX, const float* w_hwio, const float* bias,
                           const float* scale, const float* shift, const float* film_mul, const float* film_add,
                           int film_ld, float* out, long osB, long osY, long osX, float* out_pre, long psB, long psY,
                           long psX, const float* res, long rsB, long rsY, long rsX, const float* mask, long msB,
                           long msY, long msX, float* pool, long qsB, long qsY, long qsX, const float* head_w,
                           const float* head_b, float* head_out, int head_tanh, int head_skip_out, int B, int H, int W,
                           int Cin, int Cout, int KS, int relu, int accumulate, int path, int bwd, void* stream) {
  if (op_view_bad_batched(in, isB, isY, isX) || op_view_bad_batched(out, osB, osY, osX) || !w_hwio || B < 1 || H < 1 || W < 1 || Cin < 1 ||
      Cout < 1 || (KS != 1 && KS != 3 && KS != 5) || (out_pre && op_view_bad_batched(out_pre, psB, psY, psX)) ||
      (res && op_view_bad_batched(res, rsB, rsY, rsX)) || (mask && op_view_bad_batched(mask, msB, msY, msX)) ||
      (pool && op_view_bad_batched(pool, qsB, qsY, qsX))) {
    dg_set_error("op_conv2d_fused: null or non-positive argument");
    return DG_ERR_ARG;
  }
  const int co = bwd ? Cin : Cout;
  if (!scale != !shift || !film_mul != !film_add || (film_mul && film_ld < co)) {
    dg_set_error("op_conv2d_fused: scale / shift and film_mul / film_add come in pairs, film_ld >= output channels");
    return DG_ERR_ARG;
  }
  if ((head_w || head_b || head_out) && !(head_w && head_b && head_out)) { dg_set_error("op_conv2d_fused: null head argument"); return DG_ERR_ARG; }
  if (head_skip_out && !head_out) { dg_set_error("op_conv2d_fused: head_skip_out without a head"); return DG_ERR_ARG; }
  if (path < 1 || path > 10) { dg_set_error("op_conv2d_fused: path must be 1 ... 10"); return DG_ERR_ARG; }
  ConvArgs a = conv_args(op_view(in, isB, isY, isX), op_view(out, osB, osY, osX), B, H, W, bwd ? Cout : Cin, co);
  Epilogue& e = a.ep;
  e.bias = bias; e.scale = scale; e.shift = shift;
  e.film_mul = film_mul; e.film_add = film_add; e.film_ld = film_ld;
  e.out_pre = op_view_or_null(out_pre, psB, psY, psX);
  e.res = op_view_or_null(res, rsB, rsY, rsX);
  e.mask = op_view_or_null(mask, msB, msY, msX);
  e.pool = op_view_or_null(pool, qsB, qsY, qsX);
  e.relu = relu; e.accumulate = accumulate;
  e.head_w = head_w; e.head_b = head_b; e.head_out = head_out;
  e.head_tanh = head_tanh; e.head_skip_out = head_skip_out;
  return op_conv_run(a, w_hwio, Cin, Cout, KS, path, bwd ? 1 : 0, (hipStream_t)stream);
}


int depgan_op_conv3x3_wino_gathered(const float* in, long isB, long isY, long isX, const long* run_off, int runs,
                                    const float* w_hwio, const float* bias, float* out, long osB, long osY, long osX,
                                    int B, int H, int W, int Cin, int Cout, void* stream) {
  if (op_view_bad_batched(in, isB, isY, isX) || op_view_bad_batched(out, osB, osY, osX) || !w_hwio || !run_off || B < 1 || H < 1 ||
      W < 1 || Cin < 1 || Cout < 1 || runs < 1 || runs > 4) {
    dg_set_error("op_conv3x3_wino_gathered: null or non-positive argument, or not 1 ... 4 runs");
    return DG_ERR_ARG;
  }
  if (Cin % (runs * 8)) {
    dg_set_error("op_conv3x3_wino_gathered: %d channels are not %d runs of whole 8-channel chunks", Cin, runs);
    return DG_ERR_UNSUPPORTED;
  }
  ConvArgs a = conv_args(op_view(in, isB, isY, isX), op_view(out, osB, osY, osX), B, H, W, Cin, Cout);
  a.ep.bias = bias;
  a.cpt = Cin / (runs * 8);
  for (int t = 0; t < runs; ++t) a.in_run_off[t] = run_off[t];
  return op_conv_run(a, w_hwio, Cin, Cout, 3, 8, 0, (hipStream_t)stream);
}


// ---- epilogue classes of the Winograd kernel (igemm_wino.hip): the switch, the selector, the name of a launch ----
static_assert(DEPGAN_EPF_BIAS == DG_EPF_BIAS && DEPGAN_EPF_AFFINE == DG_EPF_AFFINE && DEPGAN_EPF_FILM == DG_EPF_FILM &&
              DEPGAN_EPF_RELU == DG_EPF_RELU && DEPGAN_EPF_PRE == DG_EPF_PRE && DEPGAN_EPF_RES == DG_EPF_RES &&
              DEPGAN_EPF_MASK == DG_EPF_MASK && DEPGAN_EPF_POOL == DG_EPF_POOL && DEPGAN_EPF_ACCUM == DG_EPF_ACCUM &&
              DEPGAN_EPF_HEAD == DG_EPF_HEAD && DEPGAN_EPF_ALL == DG_EPF_ALL, "include/depgan.h and common.h");
int depgan_set_epilogue_classes(int on) {
  if (on != 0 && on != 1) { dg_set_error("set_epilogue_classes: 0 or 1, not %d", on); return DG_ERR_ARG; }
  dg_set_epi_classes(on);
  return DG_OK;
}
int depgan_get_epilogue_classes(void) { return dg_get_epi_classes(); }
int depgan_wino_epilogue_class(unsigned flags, int form) {
  if ((flags & ~(unsigned)DG_EPF_ALL) || form < 0 || form > 3) {
    dg_set_error("wino_epilogue_class: flags 0x%x outside DEPGAN_EPF_ALL or form %d outside 0 ... 3", flags, form);
    return -1;
  }
  return dg_wino_epi_class(flags, form);
}
int depgan_conv5_epilogue_class(unsigned flags) {
  if (flags & ~(unsigned)DG_EPF_ALL) {
    dg_set_error("conv5_epilogue_class: flags 0x%x outside DEPGAN_EPF_ALL", flags);
    return -1;
  }
  return dg_conv5_epi_class(flags);
}
// A launch description for the host-only entries below.  Only which operands are present matters to the selection:
// every present one points at these floats
static ConvArgs op_flag_args(unsigned flags, int B, int H, int W, int Cin, int Cout) {
  alignas(16) static float present[4];
  const TView pv = make_view(present, H, W, Cout);
  ConvArgs a = conv_args(make_view(present, H, W, Cin), pv, B, H, W, Cin, Cout);
  Epilogue& e = a.ep;
  if (flags & DG_EPF_BIAS) e.bias = present;
  if (flags & DG_EPF_AFFINE) e.scale = e.shift = present;
  if (flags & DG_EPF_FILM) { e.film_mul = e.film_add = present; e.film_ld = Cout; }
  e.relu = (flags & DG_EPF_RELU) ? 1 : 0;
  if (flags & DG_EPF_PRE) e.out_pre = pv;
  if (flags & DG_EPF_RES) e.res = pv;
  if (flags & DG_EPF_MASK) e.mask = pv;
  if (flags & DG_EPF_POOL) e.pool = pv;
  e.accumulate = (flags & DG_EPF_ACCUM) ? 1 : 0;
  if (flags & DG_EPF_HEAD) { e.head_w = e.head_b = present; e.head_out = present; }
  a.w = present;
  return a;
}

int depgan_op_conv3x3_wino_kernel_name(unsigned flags, int B, int H, int W, int Cin, int Cout, char* buf, int cap) {
  if ((flags & ~(unsigned)DG_EPF_ALL) || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || !buf || cap < 1) {
    dg_set_error("op_conv3x3_wino_kernel_name: null or non-positive argument, or flags outside DEPGAN_EPF_ALL");
    return DG_ERR_ARG;
  }
  const ConvArgs a = op_flag_args(flags, B, H, W, Cin, Cout);
  const ConvPlan pl = dg_plan_conv_wino(Cin, Cout);
  if (!dg_plan_wino(pl) || !dg_conv_wino_supported(pl, a)) {
    dg_set_error("op_conv3x3_wino_kernel_name: the Winograd kernel does not cover this shape");
    return DG_ERR_UNSUPPORTED;
  }
  DgConvLaunch L;
  DGCHECK(dg_conv_prepare(pl, a, 3, DG_ROUTE_ALL, &L));
  snprintf(buf, (size_t)cap, "%s", L.k->name);
  return DG_OK;
}

// host only: the launch conv_launch prepares for a layer planned as a context in the given mode plans it
int depgan_debug_conv_choice(int f32_split, int bf16_mfma, int winograd, int KS, int planN, int B, int H, int W, int Cin,
                             int Cout, unsigned epilogue_flags, int groups, int runs, char* name, int cap, long out[5]) {
  if ((f32_split != 0 && f32_split != 3 && f32_split != 6) || (bf16_mfma != 0 && bf16_mfma != 1) ||
      (winograd != 0 && winograd != 1) || planN < 0 || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 ||
      (epilogue_flags & ~(unsigned)DG_EPF_ALL) || (groups != 0 && groups != 1 && groups != 4) || runs < 0 || runs > 4 ||
      !name || cap < 1 || !out) {
    dg_set_error("debug_conv_choice: null or non-positive argument, a mode flag that is not one of its values, flags outside "
                 "DEPGAN_EPF_ALL, groups not 0, 1 or 4, or runs outside 0 ... 4");
    return DG_ERR_ARG;
  }
  const ConvPlan pl = dg_conv_plan(f32_split, bf16_mfma, winograd, KS, Cin, Cout, planN, H, W);
  ConvArgs a = op_flag_args(epilogue_flags, B, H, W, Cin, Cout);
  a.groups = groups;
  for (int g = 0; g < groups; ++g) a.w_group[g] = a.w;
  if (runs > 0) {
    if (!dg_plan_mfma(pl) || Cin % (runs * pl.CK)) {
      dg_set_error("debug_conv_choice: %d channels are not %d runs of whole chunks of this plan", Cin, runs);
      return DG_ERR_UNSUPPORTED;
    }
    a.cpt = Cin / (runs * pl.CK);
    for (int t = 0; t < runs; ++t) a.in_run_off[t] = 4L * t;
  }
  DgConvLaunch L;
  DGCHECK(dg_conv_prepare(pl, a, KS, DG_ROUTE_ALL, &L));
  snprintf(name, (size_t)cap, "%s", L.k->name);
  out[0] = (long)L.grid * L.grid_y; out[1] = L.block; out[2] = (long)L.lds; out[3] = L.k->attr_lds;
  out[4] = L.a.lgx > 0 && out[0] < (long)L.a.lgx * L.a.lgy;
  return DG_OK;
}

int depgan_op_deconv2x2_igemm(int form, const float* in, long isB, long isY, long isX, const float* w_hwoi,
                              const float* bias, const float* scale, const float* shift, float* out, long osB, long osY,
                              long osX, const float* mask, long msB, long msY, long msX, int B, int H, int W, int Cin,
                              int Cout, int relu, int path, void* stream) {
  if (op_view_bad_batched(in, isB, isY, isX) || op_view_bad_batched(out, osB, osY, osX) || !w_hwoi || B < 1 || H < 1 || W < 1 || Cin < 1 ||
      Cout < 1 || (mask && op_view_bad_batched(mask, msB, msY, msX))) {
    dg_set_error("op_deconv2x2_igemm: null or non-positive argument");
    return DG_ERR_ARG;
  }
  if (form < 0 || form > 2 || !scale != !shift || (path != 1 && path != 3 && path != 8)) {
    dg_set_error("op_deconv2x2_igemm: form must be 0, 1 or 2, path 1, 3 or 8, scale and shift come as a pair");
    return DG_ERR_ARG;
  }
  if (form == 0 ? mask != nullptr : (bias || scale || relu)) {
    dg_set_error("op_deconv2x2_igemm: the forward takes bias / scale / shift / relu, the backward-data forms a mask");
    return DG_ERR_ARG;
  }
  if (path == 8) { dg_set_error("op_deconv2x2_igemm: the Winograd kernel has no 1x1 form"); return DG_ERR_UNSUPPORTED; }
  auto plan = [&](int ci, int co) { return path == 3 ? dg_plan_conv_bf16(1, ci, co) : dg_plan_conv(1, ci, co); };
  auto covered = [&](const ConvPlan& p) { return dg_plan_mfma(p) && (path == 3) == dg_plan_bf16(p); };
  hipStream_t st = (hipStream_t)stream;
  ConvArgs a = conv_args(null_view(), null_view(), B, H, W, 0, 0);   // views and channels by form, below
  DevTmp wt(st);
  if (form == 0) {
    // as g_forward: four 1x1 convolutions of one input, tap (di, dj) writing the pixel grid (2i+di, 2j+dj), one launch
    const ConvPlan pf = plan(Cin, Cout);
    if (!covered(pf)) { dg_set_error("op_deconv2x2_igemm: no MFMA plan for %d -> %d on path %d", Cin, Cout, path); return DG_ERR_UNSUPPORTED; }
    const TView o = op_view(out, osB, osY, osX);
    a.in = op_view(in, isB, isY, isX);
    a.Cin = Cin; a.Cout = Cout;
    a.ep.bias = bias; a.ep.scale = scale; a.ep.shift = shift; a.ep.relu = relu;
    DGCHECK(wt.alloc(4 * pf.packedFloats * sizeof(float)));
    const float* panels[4];
    for (int t = 0; t < 4; ++t) {
      float* dst = wt.as<float>() + (size_t)t * pf.packedFloats;
      DGCHECK(dg_pack_weights(pf, w_hwoi + (size_t)t * Cout * Cin, Cin, Cout, 1, 0, 0, nullptr, dst, st));
      panels[t] = dst;
    }
    deconv_groups(&a, o, panels);
    return dg_conv_igemm(pf, a, st);
  }
  // as deconv_bwd_data: in = the upstream gradient (B, 2H, 2W, Cout), out = dIn (B, H, W, Cin)
  const ConvPlan pb = plan(Cout, Cin);
  if (!covered(pb)) { dg_set_error("op_deconv2x2_igemm: no MFMA plan for %d -> %d on path %d", Cout, Cin, path); return DG_ERR_UNSUPPORTED; }
  const TView d = op_view(in, isB, isY, isX);
  a.out = op_view(out, osB, osY, osX);
  a.Cout = Cin;
  a.ep.mask = op_view_or_null(mask, msB, msY, msX);
  if (form == 1) {
    const ConvPlan pbf = plan(4 * Cout, Cin);
    if (!(pbf.family == pb.family && pbf.planes == pb.planes && (Cout % pb.CK) == 0 && pbf.packedFloats == 4 * pb.packedFloats)) {
      dg_set_error("op_deconv2x2_igemm: the gathered 1x1 form does not cover %d -> %d", Cout, Cin);
      return DG_ERR_UNSUPPORTED;
    }
    DGCHECK(wt.alloc(pbf.packedFloats * sizeof(float)));
    // the four per-tap panels interleaved per channel tile, as refresh_generator builds GLayer::wpb_all
    const size_t blk = (size_t)pb.nCC * pb.NT * pb.CK;   // elements
    PackJob jobs[4];
    for (int t = 0; t < 4; ++t) {
      float* dst = reinterpret_cast<float*>(wt.as<char>() + t * blk * dg_plan_elem_bytes(pb));
      DGCHECK(dg_pack_job(pb, w_hwoi + (size_t)t * Cout * Cin, Cin, Cout, 1, 1, 0, nullptr, dst, 4 * blk, &jobs[t]));
    }
    DGCHECK(op_pack_jobs(jobs, 4, st));
    deconv_gather_k(&a, d, Cout, pb.CK);
    a.w = wt.as<float>();
    return dg_conv_igemm(pbf, a, st);
  }
  DGCHECK(wt.alloc(4 * pb.packedFloats * sizeof(float)));
  a.Cin = Cout;
  for (int t = 0; t < 4; ++t) {
    float* dst = wt.as<float>() + (size_t)t * pb.packedFloats;
    DGCHECK(dg_pack_weights(pb, w_hwoi + (size_t)t * Cout * Cin, Cin, Cout, 1, 1, 0, nullptr, dst, st));
    a.in = strided2(d, t / 2, t % 2);
    a.w = dst;
    a.ep.accumulate = (t > 0);
    DGCHECK(dg_conv_igemm(pb, a, st));
  }
  return DG_OK;
}

int depgan_op_conv2d_wgrad_ex(const float* x, long xsB, long xsY, long xsX, const float* dy, long dsB, long dsY,
                              long dsX, const float* scale, float* dw, float* raw, int accumulate, int oi,
                              int colB, const float* colscale, float* colout, float* colraw, int B, int H, int W,
                              int Cin, int Cout, int KS, int bf16, void* stream) {
  if (op_view_bad_batched(x, xsB, xsY, xsX) || op_view_bad_batched(dy, dsB, dsY, dsX) || !dw || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 ||
      (KS != 1 && KS != 3 && KS != 5)) {
    dg_set_error("op_conv2d_wgrad_ex: null or non-positive argument");
    return DG_ERR_ARG;
  }
  const bool cols = colout || colraw;
  if ((bf16 != 0 && bf16 != 1) || (cols ? (colB < 1 || colB > B) : (colB != 0 || colscale != nullptr))) {
    dg_set_error("op_conv2d_wgrad_ex: bf16 must be 0 or 1; column sums need colout or colraw and 1 <= colB <= B");
    return DG_ERR_ARG;
  }
  if (bf16 && !dg_wgrad_bf16_supported(KS, Cin, Cout)) {
    dg_set_error("op_conv2d_wgrad_ex: the bf16 weight-gradient kernel does not cover %d -> %d", Cin, Cout);
    return DG_ERR_UNSUPPORTED;
  }
  const ColSum cs = {colB, colscale, colout, colraw};
  return op_wgrad("op_conv2d_wgrad_ex", KS, op_view(x, xsB, xsY, xsX), op_view(dy, dsB, dsY, dsX), B, H, W, Cin, Cout,
                  bf16 != 0, scale, dw, raw, accumulate, oi, cols ? &cs : nullptr, (hipStream_t)stream);
}

// host only: what the launcher of `kernel` would do with this shape, from the launcher's own chunking function
int depgan_debug_wgrad_plan(int kernel, int KS, int B, int H, int W, int Cin, int Cout, int out[4]) {
  if (!out || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) {
    dg_set_error("debug_wgrad_plan: null or non-positive argument");
    return DG_ERR_ARG;
  }
  if (kernel == DG_WG_DECONV) return dg_deconv_wgrad_plan(B, H, W, Cin, Cout, out);
  if (kernel >= DG_WG_F32 && kernel <= DG_WG_BF16S) return dg_wgrad_plan_of(kernel, KS, B, H, W, Cin, Cout, out);
  dg_set_error("debug_wgrad_plan: kernel %d is not one of 0..4", kernel);
  return DG_ERR_ARG;
}

// host only: the kernel wgrad_run launches for this shape, pipe and storage of x, and what the launch needs
int depgan_debug_wgrad_choice(int KS, int B, int H, int W, int Cin, int Cout, int bf16_pipe, int x_bf16, long out[4]) {
  if (!out || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (bf16_pipe != 0 && bf16_pipe != 1) ||
      (x_bf16 != 0 && x_bf16 != 1)) {
    dg_set_error("debug_wgrad_choice: null or non-positive argument, or a flag that is not 0 or 1");
    return DG_ERR_ARG;
  }
  DgWgradChoice ch;
  DGCHECK(dg_wgrad_choose(KS, B, H, W, Cin, Cout, bf16_pipe != 0, x_bf16 != 0, &ch));
  out[0] = ch.kernel; out[1] = ch.nchunks; out[2] = (long)ch.part_floats; out[3] = ch.col_rows;
  return DG_OK;
}


int depgan_op_bn_moments(const float* x, long sB, long sY, long sX, int B, int H, int W, int C, float* mean, float* var,
                         long scratch_floats, void* stream) {
  if (!x || !mean || !var || B < 1 || H < 1 || W < 1 || C < 4) { dg_set_error("op_bn_moments: bad argument"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const size_t cap = op_scratch(scratch_floats, dg_col_moments_scratch(B, H, W, C));
  DevTmp scratch(st);
  DGCHECK(op_alloc(&scratch, cap, "op_bn_moments"));
  return dg_col_moments(op_view(x, sB, sY, sX), B, H, W, C, mean, var, scratch.as<float>(), cap, st);
}

int depgan_op_bn_backward(const float* dy, const float* raw, float* draw, long sB, long sY, long sX, int B, int H, int W,
                          int C, const float* gamma, const float* mean, const float* var, float eps, float invN,
                          float dyscale, float* dgamma, float* dbeta, long scratch_floats, void* stream) {
  if (!dy || !raw || !draw || !gamma || !mean || !var || !dgamma || !dbeta || B < 1 || H < 1 || W < 1 || C < 4) {
    dg_set_error("op_bn_backward: bad argument");
    return DG_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t cap = op_scratch(scratch_floats, dg_colsum_pair_scratch(B, H, W, C));
  DevTmp scratch(st), coeft(st);
  DGCHECK(op_alloc(&scratch, cap, "op_bn_backward"));
  DGCHECK(op_alloc(&coeft, (size_t)8 * C, "op_bn_backward"));
  // uresnet.hip: dg_bn_train_prepare (s, t, rstd) in the forward; dg_colsum_pair -> dg_bn_bwd_coeffs -> dg_axpby_ch
  float* const coef = coeft.as<float>();
  float *s = coef, *t = coef + C, *rstd = coef + 2 * C, *sums = coef + 3 * C, *cA = coef + 5 * C, *cB = coef + 6 * C,
        *cC = coef + 7 * C;
  const TView dyv = op_view(dy, sB, sY, sX), rawv = op_view(raw, sB, sY, sX), dv = op_view(draw, sB, sY, sX);
  DGCHECK(dg_bn_train_prepare(gamma, gamma, mean, var, eps, 0.f, 0.f, nullptr, nullptr, s, t, rstd, C, st));  // t unused
  DGCHECK(dg_colsum_pair(dyv, rawv, mean, B, H, W, C, sums, scratch.as<float>(), cap, st));
  DGCHECK(dg_bn_bwd_coeffs(sums, mean, rstd, s, invN, dyscale, dgamma, dbeta, cA, cB, cC, C, st));
  return dg_axpby_ch(dyv, rawv, dv, B, H, W, C, cA, cB, cC, st);
}

int depgan_op_affine_act(const float* in, float* out, float* out_pre, const float* res, long sB, long sY, long sX,
                         const float* s, const float* t, const float* film_mul, const float* film_add, int film_ld,
                         int relu, int B, int H, int W, int C, unsigned drop_seed, float drop_rate, void* stream) {
  if (!in || !out || !s || !t || (!film_mul != !film_add) || B < 1 || H < 1 || W < 1 || C < 4) {
    dg_set_error("op_affine_act: bad argument");
    return DG_ERR_ARG;
  }
  AffineActArgs a;
  memset(&a, 0, sizeof(a));
  a.in = op_view(in, sB, sY, sX);
  a.out = op_view(out, sB, sY, sX);
  a.out_pre = out_pre ? op_view(out_pre, sB, sY, sX) : null_view();
  a.res = res ? op_view(res, sB, sY, sX) : null_view();
  a.s = s;
  a.t = t;
  a.film_mul = film_mul;
  a.film_add = film_add;
  a.film_ld = film_ld;
  a.relu = relu;
  a.B = B; a.H = H; a.W = W; a.C = C;
  a.drop_seed = drop_seed;
  a.drop_rate = drop_rate;
  return dg_affine_act(a, (hipStream_t)stream);
}

// The softmax + cross-entropy entries behind their own refusals: `a` holds the caller's operands and the setting.  This
// adds the reduction scratch and, behind it, the one device tail (DgCeDev; the caller's loss_sum stands for its loss
// slot), launches, copies back what the setting wrote, and reports the class codes outside [0, C).  census_host /
// counts_host: where the census and the label counts go (null where the setting has none)
static int op_softmax_ce_run(const char* who, SoftmaxCeArgs a, long long* census_host, long long* counts_host,
                             hipStream_t st) {
  const long P = a.P;
  const int C = a.C;
  const bool labels = a.lab.onehot || a.lab.codes;
  const size_t cap = (dg_softmax_ce_scratch(P, C, a.set) + 1) & ~(size_t)1;   // even: the tail is 8-byte aligned
  DgCeDev h;
  const auto bind = [&](float* scratch, DgCeDev* tail) {
    if (!labels) return;
    a.scratch = scratch;
    a.scratch_floats = cap;
    a.bad_count = &tail->bad;
    a.census = tail->census;
    a.counts = tail->counts;
  };
  // the refusals come before anything is allocated: the host's copy of the tail, never read through, stands in
  bind(reinterpret_cast<float*>(&h), &h);
  DGCHECK(dg_softmax_ce_check(who, a));
  DevTmp dev(st);
  DgCeDev* tail = nullptr;
  if (labels) {
    DGCHECK(op_alloc(&dev, cap + sizeof(DgCeDev) / sizeof(float), who));
    tail = reinterpret_cast<DgCeDev*>(dev.as<float>() + cap);
    bind(dev.as<float>(), tail);
  }
  DGCHECK(dg_softmax_ce(a, st));
  // one-hot labels on the plain path: no code can be out of range, nothing to fetch, no synchronisation
  if (!a.lab.codes && !census_host && !counts_host) return DG_OK;
  if (hipMemcpyAsync(&h, tail, DgCeDev::bytes(C, a.set), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    dg_set_error("%s: copy back failed", who);
    return DG_ERR_HIP;
  }
  if (census_host) memcpy(census_host, h.census, (size_t)C * C * sizeof(long long));
  if (counts_host) memcpy(counts_host, h.counts, (size_t)(C + 3) * sizeof(long long));
  if (h.bad) {
    dg_set_error("%s: %u of %ld class codes are outside [0, %d)", who, h.bad, P, C);
    return DG_ERR_ARG;
  }
  return DG_OK;
}
// the operands every entry passes on
static SoftmaxCeArgs op_softmax_ce_args(const float* logits, const float* onehot, const unsigned char* codes,
                                        float* probs, float* dz, float* loss_sum, long P, int C) {
  return SoftmaxCeArgs{logits, {onehot, codes}, probs, dz, loss_sum, nullptr, nullptr, nullptr, DgCeSetting{}, P, C,
                       nullptr, 0};
}
int depgan_op_softmax_ce(const float* logits, const float* onehot, const unsigned char* codes, float* probs, float* dz,
                         float* loss_sum, long P, int C, void* stream) {
  const SoftmaxCeArgs a = op_softmax_ce_args(logits, onehot, codes, probs, dz, loss_sum, P, C);
  return op_softmax_ce_run("op_softmax_ce", a, nullptr, nullptr, (hipStream_t)stream);
}
int depgan_op_softmax_ce_census(const float* logits, const float* onehot, const unsigned char* codes, float* probs,
                                float* dz, float* loss_sum, long long* census_host, long P, int C, void* stream) {
  if (!census_host) { dg_set_error("op_softmax_ce_census: null census_host"); return DG_ERR_ARG; }
  if (!onehot && !codes) { dg_set_error("op_softmax_ce_census: a census needs labels (onehot or codes)"); return DG_ERR_ARG; }
  SoftmaxCeArgs a = op_softmax_ce_args(logits, onehot, codes, probs, dz, loss_sum, P, C);
  a.set.census = true;
  return op_softmax_ce_run("op_softmax_ce_census", a, census_host, nullptr, (hipStream_t)stream);
}
int depgan_op_softmax_ce_weighted(const float* logits, const float* onehot, const unsigned char* codes,
                                  const float* w_host, int n, int ignore_code, float* probs, float* dz, float* loss_sum,
                                  long long* census_host, long long* counts_host, long P, int C, void* stream) {
  if (!w_host || !counts_host) { dg_set_error("op_softmax_ce_weighted: null w_host or counts_host"); return DG_ERR_ARG; }
  if (!onehot && !codes) { dg_set_error("op_softmax_ce_weighted: loss weights need labels (onehot or codes)"); return DG_ERR_ARG; }
  DGCHECK(dg_loss_weights_check("op_softmax_ce_weighted", w_host, n, C, ignore_code));
  SoftmaxCeArgs a = op_softmax_ce_args(logits, onehot, codes, probs, dz, loss_sum, P, C);
  a.set.census = census_host != nullptr;
  a.set.set_weights(w_host, C, ignore_code);
  return op_softmax_ce_run("op_softmax_ce_weighted", a, census_host, counts_host, (hipStream_t)stream);
}
int depgan_op_softmax_ce_focal(const float* logits, const float* onehot, const unsigned char* codes, const float* w_host,
                               int n, int ignore_code, float gamma, float label_smoothing, float* probs, float* dz,
                               float* loss_sum, long long* census_host, long long* counts_host, long P, int C,
                               void* stream) {
  if (!counts_host) { dg_set_error("op_softmax_ce_focal: null counts_host"); return DG_ERR_ARG; }
  if (!onehot && !codes) { dg_set_error("op_softmax_ce_focal: the focal loss needs labels (onehot or codes)"); return DG_ERR_ARG; }
  DGCHECK(dg_focal_check("op_softmax_ce_focal", gamma, label_smoothing));
  DGCHECK(dg_loss_weights_check("op_softmax_ce_focal", w_host, n, C, ignore_code));
  SoftmaxCeArgs a = op_softmax_ce_args(logits, onehot, codes, probs, dz, loss_sum, P, C);
  a.set.census = census_host != nullptr;
  a.set.set_weights(w_host, C, ignore_code);   // null: unit weights, the ignore code still holds
  a.set.focal = true;
  a.set.gamma = gamma;
  a.set.eps = label_smoothing;
  return op_softmax_ce_run("op_softmax_ce_focal", a, census_host, counts_host, (hipStream_t)stream);
}
int depgan_op_label_counts(const float* onehot, const unsigned char* codes, long P, int C, int ignore_code,
                           long long* out_host, void* stream) {
  if (!out_host) { dg_set_error("op_label_counts: null out_host"); return DG_ERR_ARG; }
  DGCHECK(dg_loss_weights_check("op_label_counts", nullptr, C, C, ignore_code));
  if (P < 1 || (!onehot == !codes)) { dg_set_error("op_label_counts: P < 1, or not exactly one of onehot and codes"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const size_t cap = (dg_label_counts_scratch(P, C) + 1) & ~(size_t)1;
  DevTmp scratch(st);
  DGCHECK(op_alloc(&scratch, cap + 2 * DEPGAN_LABEL_NCOUNT, "op_label_counts"));
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(scratch.as<float>() + cap);
  DGCHECK(dg_label_counts(onehot, codes, P, C, nullptr, ignore_code, cnt, scratch.as<float>(), cap, st));
  if (hipMemcpyAsync(out_host, cnt, (size_t)(C + 3) * sizeof(long long), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    dg_set_error("op_label_counts: copy back failed");
    return DG_ERR_HIP;
  }
  return DG_OK;
}
int depgan_op_dice_loss(const float* probs, const float* onehot, const unsigned char* codes, int ignore_code, int form,
                        const float* class_coef_host, int n, float smooth, float ce_coef, float dice_coef, float* dz,
                        double* sums_host, float* loss_host, long P, int C, void* stream) {
  if (!dz || !sums_host || !loss_host) { dg_set_error("op_dice_loss: null dz_inout, sums_host or loss_host"); return DG_ERR_ARG; }
  DGCHECK(dg_dice_check("op_dice_loss", form, ce_coef, dice_coef, smooth, class_coef_host, n, C));
  const DgLabels lab{onehot, codes};
  DGCHECK(dg_loss_operands_check("op_dice_loss", probs, nullptr, nullptr, lab, ignore_code, dz, P, false, C));
  hipStream_t st = (hipStream_t)stream;
  DgDiceSetting set;
  set.set(form, ce_coef, dice_coef, smooth, class_coef_host, C);
  // the reduction scratch, then what the coefficient stage leaves
  const size_t cap = (dg_dice_scratch(P, C) + 1) & ~(size_t)1;
  DevTmp scratch(st);
  DGCHECK(op_alloc(&scratch, cap + sizeof(DgDiceDev) / sizeof(float), "op_dice_loss"));
  DgDiceDev* out = reinterpret_cast<DgDiceDev*>(scratch.as<float>() + cap);
  DGCHECK(dg_dice_loss(probs, lab, ignore_code, set, dz, out, P, C, scratch.as<float>(), cap, st));
  DgDiceDev h;
  if (hipMemcpyAsync(&h, out, offsetof(DgDiceDev, A), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    dg_set_error("op_dice_loss: copy back failed");
    return DG_ERR_HIP;
  }
  memcpy(sums_host, h.sums, (size_t)3 * C * sizeof(double));
  *loss_host = h.loss;
  return DG_OK;
}
int depgan_op_signed_distance(const float* onehot, const unsigned char* codes, int ignore_code, int n, int H, int W, int C,
                              const int* class_on_host, double sy, double sx, double inside_offset, float* phi_out,
                              void* stream) {
  DGCHECK(dg_signed_distance_check("op_signed_distance", n, H, W, C, sy, sx, inside_offset));
  if (!phi_out || ((uintptr_t)phi_out & 3) || (!onehot == !codes) || ((uintptr_t)onehot & 3)) {
    dg_set_error("op_signed_distance: null or misaligned phi_out, or not exactly one of onehot and codes (4-byte aligned)");
    return DG_ERR_ARG;
  }
  if (ignore_code < -1 || ignore_code > 255) {
    dg_set_error("op_signed_distance: ignore code %d (-1 for none, else a byte value 0..255)", ignore_code);
    return DG_ERR_ARG;
  }
  unsigned mask = 0;
  for (int k = 0; k < C; ++k) mask |= ((!class_on_host || class_on_host[k]) ? 1u : 0u) << k;
  if (!mask) { dg_set_error("op_signed_distance: every class is switched off"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = dg_signed_distance_scratch_bytes(n, H, W, C);
  DevTmp scratch(st);
  DGCHECK(op_alloc(&scratch, (bytes + 3) / 4, "op_signed_distance"));
  return dg_signed_distance(DgLabels{onehot, codes}, ignore_code, n, H, W, C, mask, sy, sx, inside_offset, phi_out,
                            scratch.p, bytes, st);
}
int depgan_op_boundary_loss(const float* probs, const float* phi, const float* onehot, const unsigned char* codes,
                            int ignore_code, const float* class_coef_host, int ncoef, float boundary_coef,
                            float* dz_inout, double* loss_host, long P, int C, void* stream) {
  if (!loss_host) { dg_set_error("op_boundary_loss: null loss_host"); return DG_ERR_ARG; }
  DGCHECK(dg_boundary_check("op_boundary_loss", boundary_coef, class_coef_host, ncoef, C));
  const DgLabels lab{onehot, codes};
  DGCHECK(dg_loss_operands_check("op_boundary_loss", probs, "phi", phi, lab, ignore_code, dz_inout, P, true, C));
  hipStream_t st = (hipStream_t)stream;
  float coef[DEPGAN_MAX_HEAD_CLASSES];
  for (int k = 0; k < C; ++k) coef[k] = class_coef_host ? class_coef_host[k] : 1.0f / (float)C;
  // the block partials (doubles), what the finish stage leaves, then -- with an ignore code -- the label pre-pass's
  // counts and its scratch: M = P - the pixels without a true class - the codes out of range.  Without one M = P
  const size_t part = dg_boundary_scratch(P) * 2, outf = sizeof(DgBoundaryDev) / sizeof(float);
  const size_t cntf = 2 * DEPGAN_LABEL_NCOUNT, lcf = ignore_code >= 0 ? dg_label_counts_scratch(P, C) : 0;
  DevTmp scratch(st);
  DGCHECK(op_alloc(&scratch, part + outf + cntf + lcf, "op_boundary_loss"));
  double* partials = scratch.as<double>();
  DgBoundaryDev* out = reinterpret_cast<DgBoundaryDev*>(scratch.as<float>() + part);
  unsigned long long* counts = nullptr;
  if (ignore_code >= 0) {
    counts = reinterpret_cast<unsigned long long*>(scratch.as<float>() + part + outf);
    DGCHECK(dg_label_counts(onehot, codes, P, C, nullptr, ignore_code, counts, scratch.as<float>() + part + outf + cntf,
                            lcf, st));
  }
  DGCHECK(dg_boundary_loss(probs, phi, lab, ignore_code, coef, boundary_coef, counts, dz_inout, out, P, C, partials,
                           dg_boundary_scratch(P), st));
  DgBoundaryDev h;
  if (hipMemcpyAsync(&h, out, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    dg_set_error("op_boundary_loss: copy back failed");
    return DG_ERR_HIP;
  }
  loss_host[0] = h.loss;
  loss_host[1] = h.M;
  return DG_OK;
}
int depgan_op_softmax_ce4(const float* logits, const float* onehot, float* probs, float* dz, float* loss_sum, long P,
                          void* stream) {
  return depgan_op_softmax_ce(logits, onehot, nullptr, probs, dz, loss_sum, P, 4, stream);
}

// the fp32 head to K = 2..8 class logits (uresnet.hip's calls for a class count other than 4)
int depgan_op_head_k_fwd(const float* a, long ld, const float* w, const float* b, float* logits, long P, int C, int K,
                         void* stream) {
  return dg_head_k_fwd(a, ld, w, b, logits, P, C, K, (hipStream_t)stream);
}
int depgan_op_head_k_bwd(const float* dz, const float* w, const float* mask, long ldm, float* din, long ldd, long P, int C,
                         int K, void* stream) {
  return dg_head_k_bwd(dz, w, mask, ldm, din, ldd, P, C, K, (hipStream_t)stream);
}
int depgan_op_head_k_wgrad(const float* a, long lda, const float* dz, float* dW, float* db, long P, int C, int K,
                           long scratch_floats, void* stream) {
  // the scratch size is only defined for sizes the launcher takes; everything else is the launcher's to refuse
  if (!a || !dz || !dW || !db || P < 1 || C < 1 || K < 1 || C > 4096 || K > 4096) {
    dg_set_error("op_head_k_wgrad: bad argument");
    return DG_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t cap = op_scratch(scratch_floats, dg_head_k_wgrad_scratch(P, C, K));
  DevTmp scratch(st);
  DGCHECK(op_alloc(&scratch, cap, "op_head_k_wgrad"));
  // NaN in every partial: the two stages must write what they read
  if (hipMemsetAsync(scratch.p, 0xFF, cap * sizeof(float), st) != hipSuccess) {
    dg_set_error("op_head_k_wgrad: scratch fill failed");
    return DG_ERR_HIP;
  }
  return dg_head_k_wgrad(a, lda, dz, dW, db, P, C, K, scratch.as<float>(), cap, st);
}

int depgan_op_bn_rows_fwd(const float* x, float* y, int R, int C, int ld, const float* gamma, const float* beta,
                          float eps, float momentum, float corr, float* moving_mean, float* moving_var, float* mean,
                          float* rstd, int relu, void* stream) {
  if (!x || !y || !gamma || !beta || !mean || !rstd || (!moving_mean != !moving_var) || R < 1 || C < 1 || ld < C) {
    dg_set_error("op_bn_rows_fwd: bad argument");
    return DG_ERR_ARG;
  }
  return dg_bn_rows_fwd(x, y, R, C, ld, gamma, beta, eps, momentum, corr, moving_mean, moving_var, mean, rstd, relu,
                        (hipStream_t)stream);
}
int depgan_op_bn_rows_bwd(const float* dy, const float* x, const float* relu_out, float* dx, int R, int C, int ld,
                          const float* gamma, const float* mean, const float* rstd, float* dgamma, float* dbeta,
                          void* stream) {
  if (!dy || !x || !dx || !gamma || !mean || !rstd || !dgamma || !dbeta || R < 1 || C < 1 || ld < C) {
    dg_set_error("op_bn_rows_bwd: bad argument");
    return DG_ERR_ARG;
  }
  return dg_bn_rows_bwd(dy, x, relu_out, dx, R, C, ld, gamma, mean, rstd, dgamma, dbeta, (hipStream_t)stream);
}

int depgan_op_small_gemm(int form, const float* A, const float* Bm, const float* bias, float* Cm, int M, int K, int N,
                         void* stream) {
  if (!A || !Bm || !Cm || M < 1 || K < 1 || N < 1) { dg_set_error("op_small_gemm: bad argument"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  if (form == 0) return dg_small_gemm(A, Bm, bias, Cm, M, K, N, st);
  if (form == 1) return dg_small_gemm_at(A, Bm, Cm, M, K, N, st);
  if (form == 2) return dg_small_gemm_bt(A, Bm, Cm, M, K, N, st);
  dg_set_error("op_small_gemm: form %d is not 0, 1 or 2", form);
  return DG_ERR_ARG;
}


// ---- the two-critic step's HBM-bound operators (ops.hip) and the noise MLP (noise.hip), each the dg_* function the
// model calls; views as above, scratch_floats <= 0 for what the launch needs ----
extern "C++" {
// allocate a reduction scratch of op_scratch(scratch_floats, need) floats, run the call, synchronise, free
template <typename F>
static int op_with_scratch(long scratch_floats, size_t need, const char* who, hipStream_t st, F&& call) {
  const size_t cap = op_scratch(scratch_floats, need);
  DevTmp scratch(st);
  DGCHECK(op_alloc(&scratch, cap, who));
  return call(scratch.as<float>(), cap);
}
// a job table on the device, as the model's upload_table makes it
template <typename T>
static int op_upload_jobs(const std::vector<T>& jobs, DevTmp* dev, const char* who) {
  if (dev->alloc(jobs.size() * sizeof(T)) != DG_OK) { dg_set_error("%s: out of device memory", who); return DG_ERR_HIP; }
  if (hipMemcpy(dev->p, jobs.data(), jobs.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
    dg_set_error("%s: job table upload failed", who);
    return DG_ERR_HIP;
  }
  return DG_OK;
}
}  // extern "C++"

int depgan_op_unpool_mask(const float* dpool, long dsB, long dsY, long dsX, const float* a, long asB, long asY, long asX,
                          const float* skip, long ssB, long ssY, long ssX, float* out, long osB, long osY, long osX,
                          int B, int Ho, int Wo, int C, void* stream) {
  if (!dpool || !a || !out || B < 1 || Ho < 1 || Wo < 1 || C < 1) { dg_set_error("op_unpool_mask: bad argument"); return DG_ERR_ARG; }
  return dg_unpool_mask(op_view(dpool, dsB, dsY, dsX), op_view(a, asB, asY, asX), op_view_or_null(skip, ssB, ssY, ssX),
                        op_view(out, osB, osY, osX), B, Ho, Wo, C, (hipStream_t)stream);
}
int depgan_op_gather_pool(const float* u, long usB, long usY, long usX, const float* a, long asB, long asY, long asX,
                          float* out, long osB, long osY, long osX, int B, int Ho, int Wo, int C, void* stream) {
  if (!u || !a || !out || B < 1 || Ho < 1 || Wo < 1 || C < 1) { dg_set_error("op_gather_pool: bad argument"); return DG_ERR_ARG; }
  return dg_gather_pool(op_view(u, usB, usY, usX), op_view(a, asB, asY, asX), op_view(out, osB, osY, osX), B, Ho, Wo, C,
                        (hipStream_t)stream);
}

int depgan_op_head(int backward, const float* a, const float* w, const float* b, const float* dpre, float* out, long P,
                   int C, int tanh_act, void* stream) {
  if (!a || !w || !out || P < 1 || C < 1 || (backward ? !dpre : !b)) { dg_set_error("op_head: bad argument"); return DG_ERR_ARG; }
  if (backward) return dg_head_bwd(dpre, w, a, out, P, C, (hipStream_t)stream);
  return dg_head_fwd(a, w, b, out, P, C, tanh_act, (hipStream_t)stream);
}

int depgan_op_critic_tail_fwd(const float* a, const float* w9, const float* b9, const float* wd, const float* bd,
                              float* t9, float* out, int N, int HW, int C, void* stream) {
  if (!a || !w9 || !b9 || !wd || !bd || !t9 || !out || N < 1 || HW < 1 || C < 1) {
    dg_set_error("op_critic_tail_fwd: bad argument");
    return DG_ERR_ARG;
  }
  return dg_critic_tail_fwd(a, w9, b9, wd, bd, t9, out, N, HW, C, (hipStream_t)stream);
}
int depgan_op_critic_tail_bwd(const float* a, const float* w9, const float* wd, const float* coefs, int per, float* dz,
                              int N, int HW, int C, void* stream) {
  if (!a || !w9 || !wd || !coefs || !dz || per < 1 || N < 1 || HW < 1 || C < 4 || (C % 4)) {
    dg_set_error("op_critic_tail_bwd: bad argument");
    return DG_ERR_ARG;
  }
  return dg_critic_tail_bwd(a, w9, wd, coefs, per, dz, N, HW, C, (hipStream_t)stream);
}
int depgan_op_critic_tail_wgrad(const float* src, const float* w9, const float* b9, const float* wd, const float* coefs,
                                int per, int add_bias_terms, int accumulate, float* dw9, float* db9, float* dwd,
                                float* dbd, int N, int HW, int C, long scratch_floats, void* stream) {
  if (!src || !w9 || !wd || !coefs || !dw9 || !dwd || per < 1 || N < 1 || HW < 1 || C < 1 ||
      (add_bias_terms && (!b9 || !db9 || !dbd))) {
    dg_set_error("op_critic_tail_wgrad: bad argument");
    return DG_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  return op_with_scratch(scratch_floats, dg_critic_tail_wgrad_scratch(N, HW, C), "op_critic_tail_wgrad", st,
                         [&](float* scratch, size_t cap) {
                           return dg_critic_tail_wgrad(src, w9, b9, wd, coefs, per, add_bias_terms, accumulate, dw9,
                                                       db9, dwd, dbd, scratch, cap, N, HW, C, st);
                         });
}

int depgan_op_colsum(const float* v, long sB, long sY, long sX, int B, int H, int W, int C, const float* scale,
                     float* out, float* raw, int accumulate, const float* rowmul, long scratch_floats, void* stream) {
  if (!v || B < 1 || H < 1 || W < 1 || C < 1 || (!out && !raw) || (rowmul && (!out || scale || raw || accumulate))) {
    dg_set_error("op_colsum: bad argument");
    return DG_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const TView vv = op_view(v, sB, sY, sX);
  return op_with_scratch(scratch_floats, dg_colsum_scratch(B, H, W, C), "op_colsum", st, [&](float* scratch, size_t cap) {
    if (rowmul) return dg_colsum_rowmul(vv, B, H, W, C, rowmul, out, scratch, cap, st);
    return dg_colsum(vv, B, H, W, C, scale, out, raw, accumulate, scratch, cap, st);
  });
}
int depgan_op_sum(const float* in, long n, float* out, long scratch_floats, void* stream) {
  if (!in || !out || n < 1) { dg_set_error("op_sum: bad argument"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  return op_with_scratch(scratch_floats, dg_sum_scratch((size_t)n), "op_sum", st, [&](float* scratch, size_t cap) {
    return dg_sum(in, (size_t)n, out, scratch, cap, st);
  });
}

int depgan_op_critic_inputs(const float* y2, const float* x, int nicg, const float* attr, const float* ep, float* out,
                            int B, long HW, int which, void* stream) {
  if (!x || !attr || !out || nicg < 1 || B < 1 || HW < 1 || which < 0 || which > 2 || (which < 2 && (!y2 || !ep))) {
    dg_set_error("op_critic_inputs: bad argument");
    return DG_ERR_ARG;
  }
  if (which == 2) return dg_add_ch0(x, nicg, attr, out, (long)B * HW, (hipStream_t)stream);
  return dg_critic_inputs(y2, x, nicg, attr, ep, out, B, HW, which, (hipStream_t)stream);
}

int depgan_op_gp_u0(const float* g0, float* u0, float* norms, float* gp_out, float delta, int B, long HW,
                    long scratch_floats, void* stream) {
  if (!g0 || !u0 || !norms || B < 1 || HW < 1) { dg_set_error("op_gp_u0: bad argument"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  return op_with_scratch(scratch_floats, dg_gp_u0_scratch(B), "op_gp_u0", st, [&](float* scratch, size_t cap) {
    return dg_gp_u0(g0, u0, norms, gp_out, delta, B, HW, scratch, cap, st);
  });
}
int depgan_op_critic_stats(const float* d_out, const float* norms, float* out, int B, void* stream) {
  if (!d_out || !norms || !out || B < 1) { dg_set_error("op_critic_stats: bad argument"); return DG_ERR_ARG; }
  return dg_critic_stats(d_out, norms, out, B, (hipStream_t)stream);
}

int depgan_op_gloss_sums(const float* x, int nicg, const float* y2, const float* attr, float thr, float* sums, long P,
                         long scratch_floats, void* stream) {
  if (!x || !y2 || !attr || !sums || nicg < 1 || P < 1) { dg_set_error("op_gloss_sums: bad argument"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  return op_with_scratch(scratch_floats, dg_gloss_sums_scratch(P), "op_gloss_sums", st, [&](float* scratch, size_t cap) {
    return dg_gloss_sums(x, nicg, y2, attr, thr, sums, P, scratch, cap, st);
  });
}
int depgan_op_g_dpre(const float* x, int nicg, const float* y2, const float* attr, const float* g1, const float* g2,
                     float* dpre, int B, long P, void* stream) {
  if (!x || !y2 || !attr || !g1 || !g2 || !dpre || nicg < 1 || B < 1 || P < 1) {
    dg_set_error("op_g_dpre: bad argument");
    return DG_ERR_ARG;
  }
  return dg_g_dpre(x, nicg, y2, attr, g1, g2, dpre, B, P, (hipStream_t)stream);
}

int depgan_op_film_bwd(const float* dr, const float* u, const float* fmul, const float* fadd, int film_ld, float* du,
                       float* dmul, float* dadd, int B, long HW, int C, long scratch_floats, void* stream) {
  if (!dr || !u || !fmul || !fadd || !du || !dmul || !dadd || film_ld < C || B < 1 || HW < 1 || C < 1) {
    dg_set_error("op_film_bwd: bad argument");
    return DG_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  return op_with_scratch(scratch_floats, dg_film_bwd_scratch(B, C), "op_film_bwd", st, [&](float* scratch, size_t cap) {
    return dg_film_bwd(dr, u, fmul, fadd, film_ld, du, dmul, dadd, B, HW, C, scratch, cap, st);
  });
}

int depgan_op_bn_prepare_batch(void* const* ptrs, const int* C, int njobs, float eps, void* stream) {
  if (!ptrs || !C || njobs < 1) { dg_set_error("op_bn_prepare_batch: bad argument"); return DG_ERR_ARG; }
  std::vector<BnJob> jobs(njobs);
  for (int j = 0; j < njobs; ++j) {
    void* const* q = ptrs + 8 * j;
    for (int k = 0; k < 7; ++k)   // q[7], mean_copy, is optional
      if (!q[k] || C[j] < 1) { dg_set_error("op_bn_prepare_batch: job %d: bad argument", j); return DG_ERR_ARG; }
    jobs[j] = {(const float*)q[0], (const float*)q[1], (const float*)q[2], (const float*)q[3], (float*)q[4],
               (float*)q[5], (float*)q[6], (float*)q[7], C[j]};
  }
  hipStream_t st = (hipStream_t)stream;
  DevTmp dev(st);
  DGCHECK(op_upload_jobs(jobs, &dev, "op_bn_prepare_batch"));
  return dg_bn_prepare_batch(dev.as<BnJob>(), njobs, eps, st);
}

int depgan_op_bn_gamma_grad_batch(void* const* ptrs, const int* dims, int njobs, void* stream) {
  if (!ptrs || !dims || njobs < 1) { dg_set_error("op_bn_gamma_grad_batch: bad argument"); return DG_ERR_ARG; }
  std::vector<GammaJob> jobs(njobs);
  int nblocks = 0;
  for (int j = 0; j < njobs; ++j) {
    void* const* q = ptrs + 7 * j;
    const int* d = dims + 4 * j;   // K, Cout, oi, Cin
    for (int k = 0; k < 7; ++k)
      if (!q[k]) { dg_set_error("op_bn_gamma_grad_batch: job %d: null pointer", j); return DG_ERR_ARG; }
    if (d[0] < 1 || d[1] < 1 || (d[2] != 0 && d[2] != 1) || (d[2] && (d[3] < 1 || d[0] % d[3]))) {
      dg_set_error("op_bn_gamma_grad_batch: job %d: bad shape", j);
      return DG_ERR_ARG;
    }
    jobs[j] = {(const float*)q[0], (const float*)q[1], (const float*)q[2], (const float*)q[3], (const float*)q[4],
               (const float*)q[5], (float*)q[6], d[0], d[1], d[2], d[3], nblocks};
    nblocks += d[1];   // one block per output channel, jobs back to back (the model's g_gamma_jobs)
  }
  hipStream_t st = (hipStream_t)stream;
  DevTmp dev(st);
  DGCHECK(op_upload_jobs(jobs, &dev, "op_bn_gamma_grad_batch"));
  return dg_bn_gamma_grad_batch(dev.as<GammaJob>(), njobs, nblocks, st);
}

// NoiseParams / NoiseGrads over packed buffers (include/depgan.h)
static int op_noise_params(const float* trunk, const float* Wh, const float* hvec, const int* ncol, NoiseParams* P) {
  if (!trunk || !Wh || !hvec || !ncol) { dg_set_error("op_noise: bad argument"); return DG_ERR_ARG; }
  P->W0 = trunk; P->b0 = trunk + 32; P->s0 = trunk + 64; P->t0 = trunk + 96; P->mean0 = trunk + 128;
  P->rstd0 = trunk + 160;
  P->W1 = trunk + 192; P->b1 = trunk + 1216; P->s1 = trunk + 1248; P->t1 = trunk + 1280; P->mean1 = trunk + 1312;
  P->rstd1 = trunk + 1344;
  int col = 0;
  size_t woff = 0;
  for (int h = 0; h < NOISE_NHEADS; ++h) {
    if (ncol[h] < 1) { dg_set_error("op_noise: head %d has %d columns", h, ncol[h]); return DG_ERR_ARG; }
    P->Wh[h] = Wh + woff;
    P->bh[h] = hvec + col;
    P->col0[h] = col;
    P->ncol[h] = ncol[h];
    woff += (size_t)1024 * ncol[h];
    col += ncol[h];
  }
  if (col != 1024) { dg_set_error("op_noise: head widths sum to %d, not 1024", col); return DG_ERR_ARG; }
  P->sh = hvec + 1024; P->th = hvec + 2048; P->meanh = hvec + 3072; P->rstdh = hvec + 4096;
  return DG_OK;
}
static NoiseActs op_noise_acts(float* acts, int B) {
  const size_t n = (size_t)B * 1024;
  NoiseActs A;
  A.h0 = acts; A.a0 = acts + n; A.h1 = acts + 2 * n; A.a1 = acts + 3 * n; A.lin = acts + 4 * n; A.heads = acts + 5 * n;
  return A;
}

int depgan_op_noise_fwd(const float* trunk, const float* Wh, const float* hvec, const int* ncol, const float* z,
                        float* acts, int B, void* stream) {
  NoiseParams P;
  DGCHECK(op_noise_params(trunk, Wh, hvec, ncol, &P));
  if (!z || !acts || B < 1) { dg_set_error("op_noise_fwd: bad argument"); return DG_ERR_ARG; }
  return dg_noise_fwd(P, z, op_noise_acts(acts, B), B, (hipStream_t)stream);
}
int depgan_op_noise_bwd(const float* trunk, const float* Wh, const float* hvec, const int* ncol, const float* z,
                        float* acts, const float* dheads, float* gtrunk, float* dWh, float* ghvec, int B,
                        long scratch_floats, void* stream) {
  NoiseParams P;
  DGCHECK(op_noise_params(trunk, Wh, hvec, ncol, &P));
  if (!z || !acts || !dheads || !gtrunk || !dWh || !ghvec || B < 1) { dg_set_error("op_noise_bwd: bad argument"); return DG_ERR_ARG; }
  NoiseGrads G;
  G.dW0 = gtrunk; G.db0 = gtrunk + 32; G.dgamma0 = gtrunk + 64; G.dbeta0 = gtrunk + 96;
  G.dW1 = gtrunk + 128; G.db1 = gtrunk + 1152; G.dgamma1 = gtrunk + 1184; G.dbeta1 = gtrunk + 1216;
  for (int h = 0; h < NOISE_NHEADS; ++h) {
    G.dWh[h] = dWh + ((size_t)(P.Wh[h] - Wh));
    G.dbh[h] = ghvec + P.col0[h];
    G.dgamma_h[h] = ghvec + 1024 + P.col0[h];
    G.dbeta_h[h] = ghvec + 2048 + P.col0[h];
  }
  hipStream_t st = (hipStream_t)stream;
  const NoiseActs A = op_noise_acts(acts, B);
  return op_with_scratch(scratch_floats, dg_noise_bwd_scratch(B), "op_noise_bwd", st, [&](float* scratch, size_t cap) {
    return dg_noise_bwd(P, G, z, A, dheads, scratch, cap, B, st);
  });
}

int depgan_op_best_noise(const float* stats, int k, const float* z_all, long zfloats, int* best, float* z_out,
                         void* stream) {
  if (!stats || !z_all || !best || !z_out || k < 1 || zfloats < 1) { dg_set_error("op_best_noise: bad argument"); return DG_ERR_ARG; }
  return dg_best_noise(stats, k, z_all, zfloats, best, z_out, (hipStream_t)stream);
}

int depgan_op_round_bf16_masked(const float* src, const unsigned char* mask, float* dst, long n, void* stream) {
  if (!src || !mask || !dst || n < 1) { dg_set_error("op_round_bf16_masked: bad argument"); return DG_ERR_ARG; }
  return dg_round_bf16_masked(src, mask, dst, (size_t)n, (hipStream_t)stream);
}

int depgan_op_grad_sqnorm(const float* g, long n, float gscale, double* out_host, void* stream) {
  if (!g || n < 1 || !out_host) { dg_set_error("op_grad_sqnorm: bad argument"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  DevTmp out(st);
  if (out.alloc(sizeof(double)) != DG_OK) { dg_set_error("op_grad_sqnorm: out of device memory"); return DG_ERR_HIP; }
  DGCHECK(op_with_scratch(0, dg_grad_sqnorm_scratch((size_t)n), "op_grad_sqnorm", st, [&](float* scratch, size_t cap) {
    return dg_grad_sqnorm(g, (size_t)n, gscale, scratch, cap, out.as<double>(), st);
  }));
  HIPCHECK(hipMemcpyAsync(out_host, out.p, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  return DG_OK;
}

int depgan_op_adam_opts(float* p, const float* g, float* m, float* v, long n, float lr_t, float lr, float b1, float b2,
                        float eps, float gscale, float clipnorm, float clipvalue, float weight_decay,
                        const long* seg_end_host, const int* seg_decay_host, int nseg, double* norm_host, void* stream) {
  if (!p || !g || !m || !v || n < 1 || !(clipnorm >= 0.f) || !(clipvalue >= 0.f) || !(weight_decay >= 0.f) ||
      nseg < 0 || (nseg > 0 && (!seg_end_host || !seg_decay_host)) || (clipnorm > 0.f && !norm_host)) {
    dg_set_error("op_adam_opts: bad argument");
    return DG_ERR_ARG;
  }
  // the segments tile [0, n): ends ascending, the last one n
  long at = 0;
  for (int s = 0; s < nseg; ++s) {
    if (seg_end_host[s] <= at || seg_end_host[s] > n) { dg_set_error("op_adam_opts: segment ends must ascend within (0, n]"); return DG_ERR_ARG; }
    at = seg_end_host[s];
  }
  if (nseg > 0 && at != n) { dg_set_error("op_adam_opts: the last segment must end at n"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const size_t words = ((size_t)n + 31) / 32;
  std::vector<unsigned> bits(words, 0u);
  at = 0;
  for (int s = 0; s < nseg; ++s) {
    if (seg_decay_host[s])
      for (long i = at; i < seg_end_host[s]; ++i) bits[(size_t)i >> 5] |= 1u << (i & 31);
    at = seg_end_host[s];
  }
  DevTmp dbits(st), nrm(st);
  if (dbits.alloc(words * sizeof(unsigned)) != DG_OK || nrm.alloc(4 * sizeof(double)) != DG_OK) {
    dg_set_error("op_adam_opts: out of device memory");
    return DG_ERR_HIP;
  }
  HIPCHECK(hipMemcpyAsync(dbits.p, bits.data(), words * sizeof(unsigned), hipMemcpyHostToDevice, st));
  HIPCHECK(hipMemsetAsync(nrm.p, 0, 4 * sizeof(double), st));
  if (clipnorm > 0.f)
    DGCHECK(op_with_scratch(0, dg_grad_sqnorm_scratch((size_t)n), "op_adam_opts", st, [&](float* scratch, size_t cap) {
      return dg_grad_sqnorm(g, (size_t)n, gscale, scratch, cap, nrm.as<double>(), st);
    }));
  DGCHECK(dg_adam_opts(p, g, m, v, (size_t)n, lr_t, lr, b1, b2, eps, gscale, clipnorm, clipvalue, weight_decay,
                       dbits.as<unsigned>(), nrm.as<double>(), st));
  double h[3] = {0.0, 0.0, 1.0};
  if (clipnorm > 0.f) HIPCHECK(hipMemcpyAsync(h, nrm.p, sizeof(h), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  if (norm_host) {
    norm_host[0] = h[1];
    norm_host[1] = h[2];
  }
  return DG_OK;
}

}  // extern "C"
