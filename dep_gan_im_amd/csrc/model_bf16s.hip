// Generator forward (Model.predict, GT:846-859; the evaluation's ten-noise mean, GE:616-628) of a bf16_mfma context
// with every inter-layer activation STORED as bf16 (bf16s.h): the drivers and the debug surface
// (the operator entries of the kernels are in op_entries_bf16s.hip).  The fp32 path (g_forward in model.hip) and its buffers are
// not touched: this is a second, opt-in walk over the same layer table, the same packed bf16 panels (GLayer::wpf), the
// same BN affines and the same fp32 noise MLP.
// Second consumer (depgan_set_fwd_only_storage): the forward-only generator passes of the training closures --
// g_forward_only, called by critic_enqueue and by g_eval_enqueue(train = false) in model.hip -- run the same walk into
// c->attr, with gen_segmentation fused into gen_17's epilogue and gen_17 itself stored only under debug capture.
// Third consumer (depgan_set_g_update_storage, model_bf16s_train.hip): the generator update; g_forward_bf16s(train = true)
// runs the FiLM layers on the sibling kernel that also keeps the pre-FiLM tensor and the ReLU decisions.
// Fourth consumer (an inference context: bf16_mfma = 1 with nc_out >= 2): depgan_g_forward_bf16s of the DEP-UResNet in
// learning phase 0 -- the same walk, bit for bit, up to gen_17, then dg_head_softmax_bf16s instead of the tanh head.
#include "model.h"

#include <stdio.h>
#include <string.h>

static int bf16s_malloc(depgan_ctx* c, __bf16** p, size_t elems) {
  const size_t bytes = (elems ? elems : 8) * sizeof(__bf16);
  const hipError_t e = dalloc_bytes(c, (void**)p, bytes);
  if (e == hipErrorOutOfMemory) {
    dg_set_error("depgan_g_forward_bf16s: out of device memory for the bf16 activation buffers (%zu bytes)", bytes);
    return DG_ERR_HIP;
  }
  HIPCHECK(e);
  return DG_OK;
}

int infer_refuse(const depgan_ctx* c, const char* who) {
  if (!c->infer_only) return DG_OK;
  dg_set_error("%s: this is an inference context (created with bf16_mfma = 1 and nc_out >= 2): predict-only, it holds no "
               "critics, gradients or optimiser scratch; depgan_g_forward and depgan_g_forward_bf16s are its entries",
               who);
  return DG_ERR_UNSUPPORTED;
}

// what the context must be for the bf16-storage forward; no HIP call.  softmax_head: the caller also serves the
// inference context (nc_out >= 2), which only depgan_g_forward_bf16s does
int bf16s_check_ctx(const depgan_ctx* c, const char* who, bool softmax_head) {
  if (!c->cfg.bf16_mfma || !c->cfg.bf16_weights || (c->cfg.nc_out != 1 && !(softmax_head && c->infer_only))) {
    dg_set_error("%s: needs a context created with bf16_mfma = 1 (hence bf16_weights = 1, nc_out = 1%s); this one has "
                 "bf16_mfma = %d, bf16_weights = %d, nc_out = %d", who,
                 softmax_head ? ", or nc_out >= 2 for the inference context" : "", c->cfg.bf16_mfma, c->cfg.bf16_weights,
                 c->cfg.nc_out);
    return DG_ERR_UNSUPPORTED;
  }
  for (size_t i = 0; i < c->gl.size(); ++i) {
    const GLayer& L = c->gl[i];
    const bool conv = (L.kind == G_CONV && i > 0) || L.kind == G_FILM || L.kind == G_DECONV;
    if (conv && (!dg_plan_bf16(L.pf) || !L.wpf[0] || (L.Cin % 8) || (L.Cout % 32))) {
      dg_set_error("%s: layer %s (%d -> %d) has no bf16 plan; the storage types are not mixed", who, L.name.c_str(),
                   L.Cin, L.Cout);
      return DG_ERR_UNSUPPORTED;
    }
  }
  if (c->gl.empty() || c->gl[0].kind != G_CONV || c->gl[0].Cin > 2 || c->gl[0].Cout != 32) {
    dg_set_error("%s: the edge layer must be nicg -> 32", who);
    return DG_ERR_UNSUPPORTED;
  }
  return DG_OK;
}

// The bf16 twin of build_generator's activation set (GLayer::hin / hout): one buffer per layer output; a convolution that
// feeds a pool writes into the upper channels of its concat buffer, the transposed convolution of the same level
// (GLayer::cat_deconv) into the lower ones (GT:450/465/479: [deconv | skip])
int bf16s_alloc(depgan_ctx* c) {
  if (c->h_ready) return DG_OK;
  const int B = c->cfg.batch;
  TViewH cur = null_view_h();
  for (GLayer& L : c->gl) {
    L.hin = cur;
    __bf16* p = nullptr;
    if (L.kind == G_CONV && L.cat_deconv >= 0) {
      GLayer& D = c->gl[L.cat_deconv];
      const int Ctot = D.Cout + L.Cout;
      DGCHECK(bf16s_malloc(c, &p, (size_t)B * L.H * L.W * Ctot));
      L.hout = make_view_slice_h(p, L.H, L.W, Ctot, D.Cout);
      D.hout = make_view_slice_h(p, L.H, L.W, Ctot, 0);
    } else if (L.kind == G_CONV || L.kind == G_FILM) {
      DGCHECK(bf16s_malloc(c, &p, (size_t)B * L.H * L.W * L.Cout));
      L.hout = make_view_h(p, L.H, L.W, L.Cout);
    } else if (L.kind == G_POOL) {
      DGCHECK(bf16s_malloc(c, &p, (size_t)B * (L.H / 2) * (L.W / 2) * L.Cout));
      L.hout = make_view_h(p, L.H / 2, L.W / 2, L.Cout);
    }
    // a transposed convolution got slice 0 of its concat buffer above: the whole buffer for a consumer that reads all its
    // channels; the head writes fp32
    if (L.kind != G_HEAD) cur = L.hout;
  }
  c->h_ready = true;
  return dalloc_fills_done();
}

// algorithmic bytes of one bf16-storage convolution launch: activations at 2 bytes per element, bf16 panels
static double bf16s_bytes(const ConvArgsH& a, int KS) {
  const int ng = a.groups > 1 ? a.groups : 1;
  const double px = 2.0 * a.B * a.H * a.W;
  const double head = a.ep.head_out ? 4.0 * a.B * a.H * a.W : 0.0;
  return px * a.Cin + head +
         ng * (px * a.Cout * (1 + (a.ep.res.p ? 1 : 0) + (a.ep.pool.p ? 0.25 : 0) - (a.ep.head_skip_out ? 1 : 0)) +
               2.0 * KS * KS * a.Cin * a.Cout);
}

static int conv_launch_bf16s(depgan_ctx* c, const ConvArgsH& a, int KS) {
  const int ng = a.groups > 1 ? a.groups : 1;
  const double fl = 2.0 * a.B * a.H * a.W * (double)a.Cin * a.Cout * KS * KS * ng;
  char lb[56];
  snprintf(lb, sizeof(lb), "conv(bf16s) k%d b%d %dx%d %d->%d%s", KS, a.B, a.H, a.W, a.Cin, a.Cout,
           ng > 1 ? " x4" : (a.ep.head_out ? (a.ep.head_skip_out ? " +head, no store" : " +head") : ""));
  ProfScope ps(c, 0, fl, lb, bf16s_bytes(a, KS), dg_conv_bf16s_kernel(KS, a.ep.head_out != nullptr)->name);
  return dg_conv_bf16s(KS, a, c->st);
}

int g_forward_bf16s(depgan_ctx* c, const float* x, const float* z, float* out, int n, bool fused_head, bool keep_17,
                    bool train) {
  {
    ProfScope ps(c, 2, 0.0, "noise mlp fwd");
    DGCHECK(dg_noise_fwd(c->np, z, c->na, n, c->st));
  }
  c->h_17_skipped = false;
  bool pooled_by_conv = false, head_by_conv = false;
  for (size_t i = 0; i < c->gl.size(); ++i) {
    const GLayer& L = c->gl[i];
    if (L.kind == G_CONV && i == 0) {
      EdgeArgsH e;
      memset(&e, 0, sizeof(e));
      e.in = x; e.w = L.Wt; e.bias = L.b; e.scale = L.s; e.shift = L.t;
      e.out = L.hout;
      e.B = n; e.H = L.H; e.W = L.W; e.Cin = L.Cin; e.Cout = L.Cout; e.relu = 1;
      char lb[56];
      snprintf(lb, sizeof(lb), "edge conv(bf16s) b%d %dx%d %d->%d", n, L.H, L.W, L.Cin, L.Cout);
      const double px = (double)n * L.H * L.W;
      ProfScope ps(c, 2, 2.0 * px * L.Cin * L.Cout * 9, lb, px * (4.0 * L.Cin + 2.0 * L.Cout) + 36.0 * L.Cin * L.Cout);
      DGCHECK(dg_edge_conv_bf16s(e, c->st));
      pooled_by_conv = false;
    } else if (L.kind == G_CONV || L.kind == G_FILM) {
      ConvArgsH a = conv_args_h(L.hin, L.hout, n, L.H, L.W, L.Cin, L.Cout);
      a.w = L.wpf[0];
      g_layer_epilogue(&a.ep, L, c->na.heads, L.hin);
      // the 2x2 max-pool that follows rides in this launch's epilogue
      if (g_pool_follows(c->gl, i)) a.ep.pool = c->gl[i + 1].hout;
      pooled_by_conv = a.ep.pool.p != nullptr;
      // gen_segmentation rides in gen_17's epilogue (one channel tile, no pool); a pass that keeps nothing then does not
      // store gen_17 at all -- the bf16 twin of g_forward's head_skip_out
      head_by_conv = false;
      if (fused_head && c->cfg.nc_out == 1 && L.kind == G_CONV && L.Cout == 32 && !a.ep.pool.p &&
          i + 1 < c->gl.size() && c->gl[i + 1].kind == G_HEAD) {
        const GLayer& Hd = c->gl[i + 1];
        a.ep.head_w = Hd.Wt; a.ep.head_b = Hd.b; a.ep.head_out = out;
        a.ep.head_tanh = 1;
        a.ep.head_skip_out = keep_17 ? 0 : 1;
        head_by_conv = true;
        c->h_17_skipped = !keep_17;
      }
      if (train && L.kind == G_FILM) {
        // the generator update: the same launch under the sibling kernel that also keeps RNE_bf16(u) and the FiLM decisions
        ConvArgsHT t;
        static_cast<ConvArgsH&>(t) = a;
        t.u = L.hu;
        t.fdec = L.hdec;
        char lb[56];
        snprintf(lb, sizeof(lb), "conv(bf16s) k3 b%d %dx%d %d->%d +u", n, L.H, L.W, L.Cin, L.Cout);
        const double px = (double)n * L.H * L.W;
        ProfScope ps(c, 0, 2.0 * px * L.Cin * L.Cout * 9, lb, bf16s_bytes(a, 3) + px * L.Cout * (2.0 + 0.125),
                     dg_conv_bf16s_train_kernel()->name);
        DGCHECK(dg_conv_bf16s_train(t, c->st));
        continue;
      }
      DGCHECK(conv_launch_bf16s(c, a, 3));
    } else if (L.kind == G_POOL) {
      if (pooled_by_conv && L.skip_of == (int)i - 1) continue;
      // height and width are multiples of 16 (depgan_create), so every pooled level is even: not reached
      dg_set_error("depgan_g_forward_bf16s: %s is not covered by the fused pool", L.name.c_str());
      return DG_ERR_UNSUPPORTED;
    } else if (L.kind == G_DECONV) {
      // four 1x1 convolutions of the same input, tap (di, dj) writing the pixel grid (2i + di, 2j + dj): one grouped launch
      ConvArgsH a = conv_args_h(L.hin, L.hout, n, L.H, L.W, L.Cin, L.Cout);
      g_layer_epilogue(&a.ep, L, c->na.heads, L.hin);
      deconv_groups(&a, L.hout, L.wpf);
      DGCHECK(conv_launch_bf16s(c, a, 1));
    } else if (L.kind == G_HEAD) {
      if (head_by_conv) continue;
      const TViewH in = L.hin;
      const long P = (long)n * L.H * L.W;
      if (c->cfg.nc_out >= 2) {
        // the DEP-UResNet's head: the class logits and their softmax from the stored gen_17, never fused into its epilogue
        ProfScope ps(c, 2, 2.0 * P * L.Cin * 4, "head softmax fwd(bf16s)", P * (2.0 * L.Cin + 16.0));
        DGCHECK(dg_head_softmax_bf16s(in.p, in.sX, L.Wt, L.b, out, nullptr, P, L.Cin, c->cfg.nc_out, c->st));
        continue;
      }
      ProfScope ps(c, 2, 2.0 * P * L.Cin, "head fwd(bf16s)", P * (2.0 * L.Cin + 4.0));
      DGCHECK(dg_head_bf16s(in.p, in.sX, L.Wt, L.b, out, P, L.Cin, 1, c->st));
    }
  }
  return DG_OK;
}

int depgan_g_forward_bf16s(depgan_ctx* c, const float* x, const float* z, float* out, int n) {
  if (!c || !x || !z || !out) { dg_set_error("depgan_g_forward_bf16s: null argument"); return DG_ERR_ARG; }
  DGCHECK(bf16s_check_ctx(c, "depgan_g_forward_bf16s", true));
  if (n < 1 || n > c->cfg.batch) { dg_set_error("depgan_g_forward_bf16s: n must be in [1, batch]"); return DG_ERR_ARG; }
  DGCHECK(bf16s_alloc(c));
  c->h_valid = false;
  DGCHECK(g_forward_bf16s(c, x, z, out, n, false, true));   // predict: two launches, gen_17 stored
  c->h_valid = true;
  return DG_OK;
}

int g_forward_only(depgan_ctx* c, const float* x, const float* z) {
  const int B = c->cfg.batch;
  if (!c->fwd_only_bf16) return g_forward(c, x, z, B, false);
  DGCHECK(bf16s_alloc(c));
  c->h_valid = false;
  DGCHECK(g_forward_bf16s(c, x, z, c->attr.p, B, c->bf16s_head_fused, c->dbg_capture));
  c->h_valid = true;
  return DG_OK;
}

int depgan_set_fwd_only_storage(depgan_ctx* c, int storage) {
  if (!c) { dg_set_error("depgan_set_fwd_only_storage: null context"); return DG_ERR_ARG; }
  if (storage != 0 && storage != 1) {
    dg_set_error("depgan_set_fwd_only_storage: storage must be 0 (fp32) or 1 (bf16), got %d", storage);
    return DG_ERR_ARG;
  }
  DGCHECK(infer_refuse(c, "depgan_set_fwd_only_storage"));
  if (storage == 1) DGCHECK(bf16s_check_ctx(c, "depgan_set_fwd_only_storage"));
  c->fwd_only_bf16 = storage == 1;
  return DG_OK;
}

int depgan_get_fwd_only_storage(depgan_ctx* c) { return (c && c->fwd_only_bf16) ? 1 : 0; }

int bf16s_debug_copy(depgan_ctx* c, const char* name, TViewH v, int H, int W, int C, float* host, long cap, int shape[4]) {
  const int N = c->cfg.batch;
  shape[0] = N; shape[1] = H; shape[2] = W; shape[3] = C;
  if (!host) return DG_OK;
  const long need = (long)N * H * W * C;
  if (cap < need) { dg_set_error("debug_tensor_bf16s: %s needs %ld floats, the buffer holds %ld", name, need, cap); return DG_ERR_ARG; }
  DevTmp tmp(c->st);
  DGCHECK(tmp.alloc((size_t)need * sizeof(float)));
  DGCHECK(dg_widen_bf16(v, N, H, W, C, tmp.as<float>(), c->st));
  hipError_t e = hipStreamSynchronize(c->st);
  if (e == hipSuccess) e = hipMemcpy(host, tmp.p, (size_t)need * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) { dg_set_error("debug_tensor_bf16s: copy of %s failed: %s", name, hipGetErrorString(e)); return DG_ERR_HIP; }
  return DG_OK;
}

int depgan_debug_tensor_bf16s(depgan_ctx* c, const char* name, float* host, long cap, int shape[4]) {
  if (!c || !name || !shape) { dg_set_error("debug_tensor_bf16s: null argument"); return DG_ERR_ARG; }
  if (host && cap < 1) { dg_set_error("debug_tensor_bf16s: non-positive capacity"); return DG_ERR_ARG; }
  if (strncmp(name, "g/u/", 4) == 0) return bf16s_debug_u(c, name, host, cap, shape);
  if (strncmp(name, "g/out/", 6) != 0) {
    dg_set_error("debug_tensor_bf16s: '%s' is not a g/out/<layer> or g/u/<film layer> name", name);
    return DG_ERR_ARG;
  }
  if (!c->h_ready || !c->h_valid) {
    dg_set_error("debug_tensor_bf16s: no depgan_g_forward_bf16s has run on this context");
    return DG_ERR_ARG;
  }
  const std::string ln(name + 6);
  for (size_t i = 0; i < c->gl.size(); ++i) {
    const GLayer& L = c->gl[i];
    if (L.name != ln) continue;
    if (L.kind == G_HEAD) {
      dg_set_error("debug_tensor_bf16s: %s is the fp32 output of depgan_g_forward_bf16s, not a bf16 buffer", name);
      return DG_ERR_ARG;
    }
    if (c->h_17_skipped && i + 1 < c->gl.size() && c->gl[i + 1].kind == G_HEAD) {
      dg_set_error("debug_tensor_bf16s: the last bf16-storage pass was a forward-only pass with the fused head and did "
                   "not store %s (depgan_debug_capture(ctx, 1) makes those passes store it)", name);
      return DG_ERR_ARG;
    }
    const int H = L.kind == G_POOL ? L.H / 2 : (L.kind == G_DECONV ? 2 * L.H : L.H);
    const int W = L.kind == G_POOL ? L.W / 2 : (L.kind == G_DECONV ? 2 * L.W : L.W);
    return bf16s_debug_copy(c, name, L.hout, H, W, L.Cout, host, cap, shape);
  }
  dg_set_error("debug_tensor_bf16s: unknown tensor '%s'", name);
  return DG_ERR_ARG;
}
