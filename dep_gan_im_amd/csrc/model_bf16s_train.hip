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
  for (GLayer& L : c->gl) {
    if (L.kind != G_FILM) continue;
    void *pu = nullptr, *pd = nullptr;
    const size_t ub = (size_t)B * L.H * L.W * L.Cout * sizeof(__bf16), db = dg_film_dec_bytes(B, L.H, L.W, L.Cout);
    hipError_t e = dalloc_bytes(c, &pu, ub);
    if (e == hipSuccess) e = dalloc_bytes(c, &pd, db);
    if (e == hipErrorOutOfMemory) {
      dg_set_error("depgan_set_g_update_storage: out of device memory for u and the FiLM decisions of %s (%zu bytes)",
                   L.name.c_str(), ub + db);
      return DG_ERR_HIP;
    }
    HIPCHECK(e);
    L.hu = make_view_h((__bf16*)pu, L.H, L.W, L.Cout);
    L.hdec = (unsigned char*)pd;
  }
  c->hu_ready = true;
  return dalloc_fills_done();
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

static int bwd_data_h(depgan_ctx* c, const ConvPlan& pl, const ConvArgs& a, TViewH mask, int KS) {
  char lb[56];
  snprintf(lb, sizeof(lb), "conv(bf16,mask bf16) k%d b%d %dx%d %d->%d", KS, a.B, a.H, a.W, a.Cin, a.Cout);
  const double px = (double)a.B * a.H * a.W;
  ProfScope ps(c, 0, 2.0 * px * a.Cin * a.Cout * KS * KS, lb,
               px * (4.0 * a.Cin + a.Cout * (4.0 + (a.ep.res.p ? 4.0 : 0.0) + (mask.p ? 2.0 : 0.0))) +
                   2.0 * KS * KS * a.Cin * a.Cout,
               dg_conv_bf16_mh_kernel(KS)->name);
  return dg_conv_bf16_mh(pl, a, mask, c->st);
}

// conv + phase-0 BN backward given dy (g_conv_bn_bwd of model.hip); layer 0 reads the fp32 network input, every other
// layer its bf16 input: the storage of x picks the weight-gradient kernel (dg_wgrad_choose)
static int conv_bn_bwd_h(depgan_ctx* c, GLayer& L, size_t li, const float* x_user, TView dy, TView res, int n) {
  const ColSum cs = {n, L.s, L.db, L.dbeta};
  float* raw = c->raw_all + (L.dW - c->g.G);
  if (li == 0)
    return wgrad_full(c, 3, make_view(const_cast<float*>(x_user), L.H, L.W, L.Cin), dy, n, L.H, L.W, L.Cin, L.Cout, L.s,
                      L.dW, raw, 0, 0, &cs);
  DGCHECK(wgrad_full(c, 3, L.hin, dy, n, L.H, L.W, L.Cin, L.Cout, L.s, L.dW, raw, 0, 0, &cs));
  ConvArgs a = conv_args(dy, L.din, n, L.H, L.W, L.Cout, L.Cin);
  a.w = L.wpb[0];
  a.ep.res = res;
  // the mask of the fp32 path is the layer's own input tensor (the producer's output, or the whole concat buffer)
  return bwd_data_h(c, L.pb, a, L.in_mask.p ? L.hin : null_view_h(), 3);
}

int g_backward_bf16s(depgan_ctx* c, const float* x, const float* z, int n) {
  if (!c->hu_ready || !c->hu_valid) { dg_set_error("g_backward_bf16s: no training forward on bf16 storage has run"); return DG_ERR_ARG; }
  for (int i = (int)c->gl.size() - 1; i >= 0; --i) {
    GLayer& L = c->gl[i];
    if (L.kind == G_HEAD) {
      ProfScope ps(c, 2, 0.0, "head bwd(bf16s)");
      const long P = (long)n * L.H * L.W;
      const TViewH in = L.hin;
      DGCHECK(dg_colsum_rowmul_bf16s(in.p, in.sX, P, L.Cin, c->dpre, L.dW, c->scratch, c->scratchFloats, c->st));
      DGCHECK(dg_sum(c->dpre, (size_t)P, L.db, c->scratch, c->scratchFloats, c->st));
      DGCHECK(dg_head_bwd_bf16s(c->dpre, L.Wt, in.p, in.sX, L.din.p, P, L.Cin, c->st));
    } else if (L.kind == G_CONV) {
      DGCHECK(conv_bn_bwd_h(c, L, (size_t)i, x, L.dout, null_view(), n));
    } else if (L.kind == G_FILM) {
      TView du = make_view(c->du_tmp.p, L.H, L.W, L.Cout);
      {
        ProfScope ps(c, 2, 0.0, "film bwd(bf16s)");
        DGCHECK(dg_film_bwd_bf16s(L.dout.p, L.hu.p, L.hdec, c->na.heads + L.col_mul, 1024, du.p,
                                  c->dheads + L.col_mul, c->dheads + L.col_add, n, (long)L.H * L.W, L.Cout, c->scratch,
                                  c->scratchFloats, c->st));
      }
      DGCHECK(conv_bn_bwd_h(c, L, (size_t)i, x, du, L.dout, n));
    } else if (L.kind == G_POOL) {
      ProfScope ps(c, 2, 0.0, "unpool+mask(bf16s)");
      DGCHECK(dg_unpool_mask_bf16s(L.pool_dsrc, c->gl[L.skip_of].hout, L.pool_skipgrad, L.pool_dst, n, L.H / 2, L.W / 2,
                                   L.Cout, c->st));
    } else if (L.kind == G_DECONV) {
      // weight gradient: the column sums of the fp32 upstream gradient, then one 1x1 launch per tap (HWOI)
      DGCHECK(deconv_wgrad_all(c, L, L.hin, L.dout, n, L.s, c->raw_all + (L.dW - c->g.G), L.s, L.db, L.dbeta));
      // backward-data: one 1x1 convolution over the four strided grids of the upstream gradient (deconv_bwd_data)
      if (!L.wpb_all) { dg_set_error("g_backward_bf16s: %s has no gathered backward-data panel", L.name.c_str()); return DG_ERR_UNSUPPORTED; }
      ConvArgs a = conv_args(null_view(), L.din, n, L.H, L.W, L.Cout, L.Cin);
      deconv_gather_k(&a, L.dout, L.Cout, L.pb.CK);
      a.w = L.wpb_all;
      DGCHECK(bwd_data_h(c, L.pbf, a, L.in_mask.p ? L.hin : null_view_h(), 1));
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

static const GLayer* film_layer(depgan_ctx* c, const char* who, const char* lname) {
  if (!c->hu_ready || !c->hu_valid) {
    dg_set_error("%s: no generator update on bf16 storage (depgan_set_g_update_storage) has run its forward on this context", who);
    return nullptr;
  }
  for (size_t i = 0; i < c->gl.size(); ++i)
    if (c->gl[i].name == lname) {
      if (c->gl[i].kind != G_FILM) { dg_set_error("%s: %s is not a FiLM layer", who, lname); return nullptr; }
      return &c->gl[i];
    }
  dg_set_error("%s: unknown layer '%s'", who, lname);
  return nullptr;
}

// "g/u/<film layer>" of depgan_debug_tensor_bf16s
int bf16s_debug_u(depgan_ctx* c, const char* name, float* host, long cap, int shape[4]) {
  const GLayer* L = film_layer(c, "debug_tensor_bf16s", name + 4);
  if (!L) return DG_ERR_ARG;
  return bf16s_debug_copy(c, name, L->hu, L->H, L->W, L->Cout, host, cap, shape);
}

int depgan_debug_film_decision_bf16s(depgan_ctx* c, const char* layer, unsigned char* host, long cap, int shape[4]) {
  if (!c || !layer || !shape) { dg_set_error("debug_film_decision_bf16s: null argument"); return DG_ERR_ARG; }
  if (host && cap < 1) { dg_set_error("debug_film_decision_bf16s: non-positive capacity"); return DG_ERR_ARG; }
  const GLayer* L = film_layer(c, "debug_film_decision_bf16s", layer);
  if (!L) return DG_ERR_ARG;
  const int N = c->cfg.batch;
  shape[0] = N; shape[1] = L->H; shape[2] = L->W; shape[3] = L->Cout;
  if (!host) return DG_OK;
  const long need = (long)N * L->H * L->W * L->Cout;
  if (cap < need) { dg_set_error("debug_film_decision_bf16s: %s needs %ld bytes, the buffer holds %ld", layer, need, cap); return DG_ERR_ARG; }
  DevTmp tmp(c->st);
  DGCHECK(tmp.alloc((size_t)need));
  DGCHECK(dg_unpack_bits(L->hdec, tmp.as<unsigned char>(), need, c->st));
  hipError_t e = hipStreamSynchronize(c->st);
  if (e == hipSuccess) e = hipMemcpy(host, tmp.p, (size_t)need, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { dg_set_error("debug_film_decision_bf16s: copy failed: %s", hipGetErrorString(e)); return DG_ERR_HIP; }
  return DG_OK;
}
