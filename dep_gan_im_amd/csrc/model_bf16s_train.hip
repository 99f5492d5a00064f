// Generator UPDATE of a bf16_mfma context on bf16 activation storage (depgan_set_g_update_storage; bf16s_train.h,
// DESIGN.md section 3).  The training forward is g_forward_bf16s -- the walk of depgan_g_forward_bf16s and of
// g_forward_only, so attr has their bits -- with the FiLM layers on the sibling kernel that also keeps RNE_bf16(u) and
// the ReLU decision it took.  g_backward_bf16s is g_backward (model.hip) over the same layer table, gradient arena,
// raw_all slots, batched BN-gamma launch and noise-MLP backward; every ACTIVATION operand (weight-gradient x, ReLU masks,
// pool arg-max, u) is read from the bf16 buffers, every gradient (dout / din / du) stays an fp32 tensor of the fp32 set.
// No fp32 copy of a generator activation is written.  Straight-through: each storage rounding is the identity for the
// gradient; ReLU masks are `stored > 0`, the pool arg-max is taken on the stored values, the FiLM mask is the stored bit.
#include "model.h"

#include <stdio.h>
#include <string.h>

int bf16s_train_alloc(depgan_ctx* c) {
  if (c->hu_ready) return DG_OK;
  DGCHECK(bf16s_alloc(c));
  const int B = c->cfg.batch;
  const size_t nl = c->gl.size();
  std::vector<TViewH> hu(nl, null_view_h());
  std::vector<unsigned char*> hd(nl, nullptr);
  for (size_t i = 0; i < nl; ++i) {
    const GLayer& L = c->gl[i];
    if (L.kind != G_FILM) continue;
    void *pu = nullptr, *pd = nullptr;
    const size_t ub = (size_t)B * L.H * L.W * L.Cout * sizeof(__bf16), db = dg_film_dec_bytes(B, L.H, L.W, L.Cout);
    if (hipMalloc(&pu, ub) != hipSuccess || hipMalloc(&pd, db) != hipSuccess) {
      if (pu) hipFree(pu);
      dg_set_error("depgan_set_g_update_storage: out of device memory for u and the FiLM decisions of %s (%zu bytes)",
                   L.name.c_str(), ub + db);
      return DG_ERR_HIP;
    }
    c->allocs.push_back(pu);
    c->allocs.push_back(pd);
    HIPCHECK(hipMemset(pu, 0, ub));
    HIPCHECK(hipMemset(pd, 0, db));
    hu[i] = make_view_h((__bf16*)pu, L.H, L.W, L.Cout);
    hd[i] = (unsigned char*)pd;
  }
  c->h_u.swap(hu);
  c->h_dec.swap(hd);
  c->hu_ready = true;
  return DG_OK;
}

int g_forward_train_bf16s(depgan_ctx* c, const float* x, const float* z) {
  DGCHECK(bf16s_train_alloc(c));
  c->h_valid = false;
  c->hu_valid = false;
  // gen_17 is stored (its backward reads it); the head may still ride in its epilogue
  DGCHECK(g_forward_bf16s(c, x, z, c->attr.p, c->cfg.batch, c->bf16s_head_fused, true, true));
  c->h_valid = true;
  c->hu_valid = true;
  return DG_OK;
}

// weight gradient with the activation operand in bf16 memory: slabs + the finish launch of wgrad_full
static int wgrad_full_h(depgan_ctx* c, int KS, TViewH x, TView dy, int N, int H, int W, int Cin, int Cout,
                        const float* scale, float* out, float* raw, int oi, const ColSum* cs) {
  if (!dg_wgrad_bf16s_supported(KS, Cin, Cout)) {
    dg_set_error("g_backward_bf16s: no bf16-staged weight gradient for k%d %d -> %d", KS, Cin, Cout);
    return DG_ERR_UNSUPPORTED;
  }
  if (dg_wgrad_bf16s_part_floats(KS, N, H, W, Cin, Cout) > c->partFloats) {
    dg_set_error("wgrad slab workspace too small");
    return DG_ERR_ARG;
  }
  WgradArgsH a;
  a.x = x;
  a.dy = dy;
  a.part = c->part;
  a.B = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  a.nTiles = a.tilesPerChunk = 0;
  a.colpart = cs ? c->scratch : nullptr;
  a.colB = cs ? cs->B : 0;
  int nch = 0;
  char lb[56];
  snprintf(lb, sizeof(lb), "wgrad(bf16s) k%d b%d %dx%d %d->%d", KS, N, H, W, Cin, Cout);
  {
    const double px = (double)N * H * W;
    ProfScope ps(c, 1, 2.0 * px * Cin * Cout * KS * KS, lb, px * (2.0 * Cin + 4.0 * Cout));
    DGCHECK(dg_wgrad_bf16s(KS, a, &nch, c->st));
  }
  ProfScope ps(c, 2, 0.0, "slab reduce");
  return dg_wgrad_finish(c->part, nch, KS * KS, Cin, Cout, scale, out, raw, 0, oi, cs ? c->scratch : nullptr, Cout,
                         cs ? cs->scale : nullptr, cs ? cs->out : nullptr, cs ? cs->raw : nullptr, c->st);
}

static int bwd_data_h(depgan_ctx* c, const ConvPlan& pl, const ConvArgs& a, TViewH mask, int KS) {
  char lb[56];
  snprintf(lb, sizeof(lb), "conv(bf16,mask bf16) k%d b%d %dx%d %d->%d", KS, a.B, a.H, a.W, a.Cin, a.Cout);
  const double px = (double)a.B * a.H * a.W;
  ProfScope ps(c, 0, 2.0 * px * a.Cin * a.Cout * KS * KS, lb,
               px * (4.0 * a.Cin + a.Cout * (4.0 + (a.ep.res.p ? 4.0 : 0.0) + (mask.p ? 2.0 : 0.0))) +
                   2.0 * KS * KS * a.Cin * a.Cout,
               dg_conv_bf16_mh_name(KS));
  return dg_conv_bf16_mh(pl, a, mask, c->st);
}

// conv + phase-0 BN backward given dy (g_conv_bn_bwd of model.hip); layer 0 reads the fp32 network input
static int conv_bn_bwd_h(depgan_ctx* c, GLayer& L, size_t li, const float* x_user, TView dy, TView res, int n) {
  const ColSum cs = {n, L.s, L.db, L.dbeta};
  float* raw = c->raw_all + (L.dW - c->g.G);
  if (li == 0)
    return wgrad_full(c, 3, make_view(const_cast<float*>(x_user), L.H, L.W, L.Cin), dy, n, L.H, L.W, L.Cin, L.Cout, L.s,
                      L.dW, raw, 0, 0, &cs);
  DGCHECK(wgrad_full_h(c, 3, c->h_in[li], dy, n, L.H, L.W, L.Cin, L.Cout, L.s, L.dW, raw, 0, &cs));
  ConvArgs a = conv_args(dy, L.din, n, L.H, L.W, L.Cout, L.Cin);
  a.w = L.wpb[0];
  a.ep.res = res;
  // the mask of the fp32 path is the layer's own input tensor (the producer's output, or the whole concat buffer)
  return bwd_data_h(c, L.pb, a, L.in_mask.p ? c->h_in[li] : null_view_h(), 3);
}

int g_backward_bf16s(depgan_ctx* c, const float* x, const float* z, int n) {
  if (!c->hu_ready || !c->hu_valid) { dg_set_error("g_backward_bf16s: no training forward on bf16 storage has run"); return DG_ERR_ARG; }
  for (int i = (int)c->gl.size() - 1; i >= 0; --i) {
    GLayer& L = c->gl[i];
    if (L.kind == G_HEAD) {
      ProfScope ps(c, 2, 0.0, "head bwd(bf16s)");
      const long P = (long)n * L.H * L.W;
      const TViewH in = c->h_in[i];
      DGCHECK(dg_colsum_rowmul_bf16s(in.p, in.sX, P, L.Cin, c->dpre, L.dW, c->scratch, c->scratchFloats, c->st));
      DGCHECK(dg_sum(c->dpre, (size_t)P, L.db, c->scratch, c->scratchFloats, c->st));
      DGCHECK(dg_head_bwd_bf16s(c->dpre, L.Wt, in.p, in.sX, L.din.p, P, L.Cin, c->st));
    } else if (L.kind == G_CONV) {
      DGCHECK(conv_bn_bwd_h(c, L, (size_t)i, x, L.dout, null_view(), n));
    } else if (L.kind == G_FILM) {
      TView du = make_view(c->du_tmp.p, L.H, L.W, L.Cout);
      {
        ProfScope ps(c, 2, 0.0, "film bwd(bf16s)");
        DGCHECK(dg_film_bwd_bf16s(L.dout.p, c->h_u[i].p, c->h_dec[i], c->na.heads + L.col_mul, 1024, du.p,
                                  c->dheads + L.col_mul, c->dheads + L.col_add, n, (long)L.H * L.W, L.Cout, c->scratch,
                                  c->scratchFloats, c->st));
      }
      DGCHECK(conv_bn_bwd_h(c, L, (size_t)i, x, du, L.dout, n));
    } else if (L.kind == G_POOL) {
      ProfScope ps(c, 2, 0.0, "unpool+mask(bf16s)");
      DGCHECK(dg_unpool_mask_bf16s(L.pool_dsrc, c->h_out[L.skip_of], L.pool_skipgrad, L.pool_dst, n, L.H / 2, L.W / 2,
                                   L.Cout, c->st));
    } else if (L.kind == G_DECONV) {
      // weight gradient: the column sums of the fp32 upstream gradient, then one 1x1 launch per tap (HWOI)
      {
        ProfScope ps(c, 2, 0.0, "colsum");
        DGCHECK(dg_colsum(L.dout, n, 2 * L.H, 2 * L.W, L.Cout, L.s, L.db, L.dbeta, 0, c->scratch, c->scratchFloats, c->st));
      }
      float* raw = c->raw_all + (L.dW - c->g.G);
      for (int t = 0; t < 4; ++t) {
        const size_t o = (size_t)t * L.Cout * L.Cin;
        DGCHECK(wgrad_full_h(c, 1, c->h_in[i], strided2(L.dout, t / 2, t % 2), n, L.H, L.W, L.Cin, L.Cout, L.s, L.dW + o,
                             raw + o, 1, nullptr));
      }
      // backward-data: one 1x1 convolution over the four strided grids of the upstream gradient (deconv_bwd_data)
      if (!L.wpb_all) { dg_set_error("g_backward_bf16s: %s has no gathered backward-data panel", L.name.c_str()); return DG_ERR_UNSUPPORTED; }
      ConvArgs a = conv_args(null_view(), L.din, n, L.H, L.W, L.Cout, L.Cin);
      deconv_gather_k(&a, L.dout, L.Cout, L.pb.CK);
      a.w = L.wpb_all;
      DGCHECK(bwd_data_h(c, L.pbf, a, L.in_mask.p ? c->h_in[i] : null_view_h(), 1));
    }
  }
  return g_backward_finish(c, z, n);
}

int depgan_set_g_update_storage(depgan_ctx* c, int storage) {
  if (!c) { dg_set_error("depgan_set_g_update_storage: null context"); return DG_ERR_ARG; }
  if (storage != 0 && storage != 1) {
    dg_set_error("depgan_set_g_update_storage: storage must be 0 (fp32) or 1 (bf16), got %d", storage);
    return DG_ERR_ARG;
  }
  DGCHECK(infer_refuse(c, "depgan_set_g_update_storage"));
  if (storage == 1) DGCHECK(bf16s_check_ctx(c, "depgan_set_g_update_storage"));
  c->g_update_bf16 = storage == 1;
  return DG_OK;
}

int depgan_get_g_update_storage(depgan_ctx* c) { return (c && c->g_update_bf16) ? 1 : 0; }

static const GLayer* film_layer(depgan_ctx* c, const char* who, const char* lname, size_t* idx) {
  if (!c->hu_ready || !c->hu_valid) {
    dg_set_error("%s: no generator update on bf16 storage (depgan_set_g_update_storage) has run its forward on this context", who);
    return nullptr;
  }
  for (size_t i = 0; i < c->gl.size(); ++i)
    if (c->gl[i].name == lname) {
      if (c->gl[i].kind != G_FILM) { dg_set_error("%s: %s is not a FiLM layer", who, lname); return nullptr; }
      *idx = i;
      return &c->gl[i];
    }
  dg_set_error("%s: unknown layer '%s'", who, lname);
  return nullptr;
}

// "g/u/<film layer>" of depgan_debug_tensor_bf16s
int bf16s_debug_u(depgan_ctx* c, const char* name, float* host, long cap, int shape[4]) {
  size_t i = 0;
  const GLayer* L = film_layer(c, "debug_tensor_bf16s", name + 4, &i);
  if (!L) return DG_ERR_ARG;
  return bf16s_debug_copy(c, name, c->h_u[i], L->H, L->W, L->Cout, host, cap, shape);
}

int depgan_debug_film_decision_bf16s(depgan_ctx* c, const char* layer, unsigned char* host, long cap, int shape[4]) {
  if (!c || !layer || !shape) { dg_set_error("debug_film_decision_bf16s: null argument"); return DG_ERR_ARG; }
  if (host && cap < 1) { dg_set_error("debug_film_decision_bf16s: non-positive capacity"); return DG_ERR_ARG; }
  size_t i = 0;
  const GLayer* L = film_layer(c, "debug_film_decision_bf16s", layer, &i);
  if (!L) return DG_ERR_ARG;
  const int N = c->cfg.batch;
  shape[0] = N; shape[1] = L->H; shape[2] = L->W; shape[3] = L->Cout;
  if (!host) return DG_OK;
  const long need = (long)N * L->H * L->W * L->Cout;
  if (cap < need) { dg_set_error("debug_film_decision_bf16s: %s needs %ld bytes, the buffer holds %ld", layer, need, cap); return DG_ERR_ARG; }
  unsigned char* tmp = nullptr;
  HIPCHECK(hipMalloc((void**)&tmp, (size_t)need));
  int rc = dg_unpack_bits(c->h_dec[i], tmp, need, c->st);
  hipError_t e = hipStreamSynchronize(c->st);
  if (rc == DG_OK && e == hipSuccess) e = hipMemcpy(host, tmp, (size_t)need, hipMemcpyDeviceToHost);
  hipFree(tmp);
  if (rc != DG_OK) return rc;
  if (e != hipSuccess) { dg_set_error("debug_film_decision_bf16s: copy failed: %s", hipGetErrorString(e)); return DG_ERR_HIP; }
  return DG_OK;
}

// ---- single operators (unit tests): explicit view strides in ELEMENTS, stream last, checks before any HIP call ----

int depgan_op_conv2d_film_train_bf16s(const void* in, long isB, long isY, long isX, const float* w_hwio, const float* bias,
                                      const float* scale, const float* shift, const float* film_mul, const float* film_add,
                                      int film_ld, const void* res, long rsB, long rsY, long rsX, void* out, long osB,
                                      long osY, long osX, void* u_out, unsigned char* dec_bits, int B, int H, int W, int Cin,
                                      int Cout, int relu, void* stream) {
  if (bad_view(in, isB, isY, isX) || bad_view(out, osB, osY, osX) || !w_hwio || !film_mul || !film_add || !u_out || !dec_bits ||
      B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (res && bad_view(res, rsB, rsY, rsX))) {
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
  float* wp = nullptr;
  HIPCHECK(hipMalloc((void**)&wp, pl.packedFloats * sizeof(float)));
  int rc = dg_pack_weights(pl, w_hwio, Cin, Cout, 0, 0, 0, nullptr, wp, st);
  a.w = wp;
  if (rc == DG_OK) rc = dg_conv_bf16s_train(a, st);
  hipStreamSynchronize(st);
  hipFree(wp);
  return rc;
}

int depgan_op_conv2d_wgrad_bf16s(const void* x, long xsB, long xsY, long xsX, const float* dy, long dsB, long dsY, long dsX,
                                 float* dw, float* colsum, int B, int H, int W, int Cin, int Cout, int KS, int oi,
                                 void* stream) {
  if (bad_view(x, xsB, xsY, xsX) || bad_view(dy, dsB, dsY, dsX) || !dw || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) {
    dg_set_error("op_conv2d_wgrad_bf16s: null or non-positive argument");
    return DG_ERR_ARG;
  }
  if (KS != 1 && KS != 3) { dg_set_error("op_conv2d_wgrad_bf16s: KS must be 1 or 3"); return DG_ERR_ARG; }
  if (!dg_wgrad_bf16s_supported(KS, Cin, Cout)) { dg_set_error("op_conv2d_wgrad_bf16s: shape not covered (%d -> %d)", Cin, Cout); return DG_ERR_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  const size_t pf = dg_wgrad_bf16s_part_floats(KS, B, H, W, Cin, Cout);
  const size_t cf = pf / ((size_t)KS * KS * Cin * Cout) * Cout;
  float *part = nullptr, *col = nullptr;
  HIPCHECK(hipMalloc((void**)&part, pf * sizeof(float)));
  if (colsum && hipMalloc((void**)&col, cf * sizeof(float)) != hipSuccess) {
    hipFree(part);
    dg_set_error("op_conv2d_wgrad_bf16s: out of memory");
    return DG_ERR_HIP;
  }
  WgradArgsH a;
  a.x = op_view_h(x, xsB, xsY, xsX);
  a.dy = op_view(dy, dsB, dsY, dsX);
  a.part = part;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  a.nTiles = a.tilesPerChunk = 0;
  a.colpart = col;
  a.colB = col ? B : 0;
  int nch = 0;
  int rc = dg_wgrad_bf16s(KS, a, &nch, st);
  if (rc == DG_OK)
    rc = dg_wgrad_finish(part, nch, KS * KS, Cin, Cout, nullptr, dw, nullptr, 0, oi, col, Cout, nullptr, colsum, nullptr, st);
  hipStreamSynchronize(st);
  hipFree(part);
  if (col) hipFree(col);
  return rc;
}

// KS = 3: dx = mask(conv_bwd_data(dy, w_hwio) + res); KS = 1 with deconv = 1: dy is the (2H, 2W) upstream gradient of a
// 2x2 / stride-2 transposed convolution with HWOI weights (Cin of the transposed convolution = channels of dx)
int depgan_op_conv2d_bwd_data_bf16s(const float* dy, long dsB, long dsY, long dsX, const float* w, const float* res,
                                    long rsB, long rsY, long rsX, const void* mask, long msB, long msY, long msX, float* dx,
                                    long osB, long osY, long osX, int B, int H, int W, int Cin, int Cout, int deconv,
                                    void* stream) {
  if (bad_view(dy, dsB, dsY, dsX) || bad_view(dx, osB, osY, osX) || !w || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 ||
      (res && bad_view(res, rsB, rsY, rsX)) || (mask && bad_view(mask, msB, msY, msX))) {
    dg_set_error("op_conv2d_bwd_data_bf16s: null or non-positive argument");
    return DG_ERR_ARG;
  }
  if (deconv != 0 && deconv != 1) { dg_set_error("op_conv2d_bwd_data_bf16s: deconv must be 0 or 1"); return DG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  ConvArgs a = conv_args(null_view(), op_view(dx, osB, osY, osX), B, H, W, Cout, Cin);
  a.ep.res = op_view_or_null(res, rsB, rsY, rsX);
  const TViewH mh = op_view_h_or_null(mask, msB, msY, msX);
  const TView d = op_view(dy, dsB, dsY, dsX);
  float* wp = nullptr;
  int rc = DG_OK;
  ConvPlan pl;
  if (!deconv) {
    pl = dg_plan_conv_bf16(3, Cout, Cin);
    if (!dg_plan_bf16(pl)) { dg_set_error("op_conv2d_bwd_data_bf16s: the bf16 MFMA kernel does not cover %d -> %d", Cout, Cin); return DG_ERR_UNSUPPORTED; }
    HIPCHECK(hipMalloc((void**)&wp, pl.packedFloats * sizeof(float)));
    rc = dg_pack_weights(pl, w, Cin, Cout, 0, 1, 1, nullptr, wp, st);
    a.in = d;
  } else {
    const ConvPlan pb = dg_plan_conv_bf16(1, Cout, Cin);
    pl = dg_plan_conv_bf16(1, 4 * Cout, Cin);
    if (!dg_plan_bf16(pb) || !dg_plan_bf16(pl) || (Cout % pb.CK) || pl.packedFloats != 4 * pb.packedFloats) {
      dg_set_error("op_conv2d_bwd_data_bf16s: the gathered 1x1 form does not cover %d -> %d", Cout, Cin);
      return DG_ERR_UNSUPPORTED;
    }
    HIPCHECK(hipMalloc((void**)&wp, pl.packedFloats * sizeof(float)));
    // the four per-tap panels interleaved per channel tile, as refresh_generator builds GLayer::wpb_all
    const size_t per_nt = (size_t)pb.nCC * pb.NT * pb.CK;   // bf16 elements of one channel tile of one tap
    for (int t = 0; t < 4 && rc == DG_OK; ++t) {
      PackJob j;
      rc = dg_pack_job(pb, w + (size_t)t * Cout * Cin, Cin, Cout, 1, 1, 0, nullptr,
                       reinterpret_cast<float*>(reinterpret_cast<__bf16*>(wp) + (size_t)t * per_nt), 4 * per_nt, &j);
      if (rc != DG_OK) break;
      unsigned nb = dg_pack_layout(&j, 1);
      PackJob* jd = nullptr;
      if (hipMalloc((void**)&jd, sizeof(PackJob)) != hipSuccess) { rc = DG_ERR_HIP; dg_set_error("op_conv2d_bwd_data_bf16s: out of memory"); break; }
      hipMemcpy(jd, &j, sizeof(PackJob), hipMemcpyHostToDevice);
      rc = dg_pack_weights_batch(jd, 1, nb, st);
      hipStreamSynchronize(st);
      hipFree(jd);
    }
    deconv_gather_k(&a, d, Cout, pb.CK);
  }
  a.w = wp;
  if (rc == DG_OK) rc = dg_conv_bf16_mh(pl, a, mh, st);
  hipStreamSynchronize(st);
  hipFree(wp);
  return rc;
}

int depgan_op_unpool_mask_bf16s(const float* dpool, long dsB, long dsY, long dsX, const void* a, long asB, long asY, long asX,
                                const float* skip, long ssB, long ssY, long ssX, float* out, long osB, long osY, long osX,
                                int B, int Ho, int Wo, int C, void* stream) {
  if (bad_view(dpool, dsB, dsY, dsX) || bad_view(a, asB, asY, asX) || bad_view(out, osB, osY, osX) || (skip && bad_view(skip, ssB, ssY, ssX)) ||
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
  float* scratch = nullptr;
  HIPCHECK(hipMalloc((void**)&scratch, need * sizeof(float)));
  int rc = dg_film_bwd_bf16s(dr, reinterpret_cast<const __bf16*>(u), dec_bits, fmul, film_ld, du, dmul, dadd, B, HW, C,
                             scratch, need, st);
  hipStreamSynchronize(st);
  hipFree(scratch);
  return rc;
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
  float* scratch = nullptr;
  HIPCHECK(hipMalloc((void**)&scratch, need * sizeof(float)));
  int rc = dg_colsum_rowmul_bf16s(reinterpret_cast<const __bf16*>(a), ld, P, C, dpre, out, scratch, need, st);
  hipStreamSynchronize(st);
  hipFree(scratch);
  return rc;
}
