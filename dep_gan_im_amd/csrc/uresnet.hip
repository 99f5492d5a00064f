// DEP-UResNet supervised path: the same U-ResNet as the DEP-GAN generator with a
// softmax head over nc_out = 2..8 classes (the reference's n_label = 4, UT:573), trained by my_network.fit /
// train_on_batch in Keras learning phase 1
// (DEP-UResNet-wNoises-training-4fold.py "UT":355-427 model, 583-606 compile + fit).
//
// What phase 1 changes relative to the GAN closures (which never feed the learning phase):
//   * every BatchNormalization uses the statistics of the current batch and the gradient flows
//     through them; moving_mean / moving_variance are updated with momentum 0.99 (App. B.3);
//   * Dropout(0.25) after conv_10 is active (UT:388);
//   * loss = keras categorical_crossentropy on the softmax probabilities (App. B.9);
//   * Adam(1e-4, beta_1 0.9, beta_2 0.999).
//
// Per conv layer, forward:  igemm (bias only) -> RAW ; per-channel batch moments of RAW ;
//                           y = act(film(RAW*s + t)) (+res, dropout) in one elementwise pass.
//            backward: sums (dy, dy*RAW) -> dgamma, dbeta and the three coefficients of
//                           dRAW = A*dy + B*RAW + C ; then the same wgrad / bwd-data kernels as the GAN path
//                           on dRAW with unscaled weights.
#include <stddef.h>
#include <string.h>

#include <string>

#include "model.h"

static const float kBnEps = 1e-3f, kBnMomentum = 0.99f, kDropRate = 0.25f;
static const char* kDropLayer = "gen_10";

static const char* kUHeadSfx[NOISE_NHEADS] = {"add_m3", "mul_m3", "add_m2", "mul_m2", "add_m1", "mul_m1", "add",
                                              "mul",    "add_p3", "mul_p3", "add_p2", "mul_p2", "add_p1", "mul_p1"};

struct UNoiseBn {
  float *gamma, *beta, *mm, *mv, *dgamma, *dbeta;
};
static UNoiseBn noise_bn(Net& g, const std::string& nm) {
  UNoiseBn b;
  b.gamma = g.p(nm + "/gamma");
  b.beta = g.p(nm + "/beta");
  b.mm = g.p(nm + "/moving_mean");
  b.mv = g.p(nm + "/moving_variance");
  b.dgamma = g.g(nm + "/gamma");
  b.dbeta = g.g(nm + "/beta");
  return b;
}

// loss_dev, on the device and as the host reads it
struct ULossHost {
  DgCeDev ce;
  DgDiceDev dice;   // the Dice mode: the 3 C sums and the Dice term (the copy stops in front of A and B)
  DgBoundaryDev bl; // the boundary mode: L_B and M (the copy then runs to the end of the struct)
};
static_assert(offsetof(ULossHost, dice) % 8 == 0, "the Dice sums are doubles");
static_assert(offsetof(ULossHost, bl) % 8 == 0, "L_B and M are doubles");

int uresnet_build(depgan_ctx* c) {
  const int B = c->cfg.batch;
  size_t maxOut = 0, nsmall = 0;
  for (GLayer& L : c->gl)
    if (L.kind == G_CONV || L.kind == G_FILM || L.kind == G_DECONV) nsmall += 11 * (size_t)((L.Cout + 3) & ~3);
  float* sm = nullptr;
  DGCHECK(dmalloc(c, &sm, nsmall + 64));
  auto take = [&](int n) {
    float* r = sm;
    sm += (n + 3) & ~3;
    return r;
  };
  for (GLayer& L : c->gl) {
    if (L.kind != G_CONV && L.kind != G_FILM && L.kind != G_DECONV) continue;
    const int up = (L.kind == G_DECONV) ? 2 : 1;
    DGCHECK(talloc(c, &L.raw, B, L.H * up, L.W * up, L.Cout));
    const size_t per = (size_t)L.H * up * L.W * up * L.Cout;
    if (per > maxOut) maxOut = per;
    L.bmean = take(L.Cout); L.bvar = take(L.Cout); L.bs = take(L.Cout); L.bt = take(L.Cout); L.brstd = take(L.Cout);
    L.cA = take(L.Cout); L.cB = take(L.Cout); L.cC = take(L.Cout); L.sums = take(2 * L.Cout);
  }
  DGCHECK(dmalloc(c, &c->draw_tmp.p, (size_t)B * maxOut));
  const size_t P = (size_t)B * c->cfg.height * c->cfg.width;
  DGCHECK(dmalloc(c, &c->logits, P * c->cfg.nc_out));
  DGCHECK(dmalloc(c, &c->dz, P * c->cfg.nc_out));
  // what the loss launches leave for the host: DgCeDev, then what the Dice mode's coefficient stage leaves
  DGCHECK(dmalloc(c, &c->loss_dev, sizeof(ULossHost) / sizeof(float)));
  DGCHECK(dmalloc(c, &c->ones1k, 1024));
  DGCHECK(dmalloc(c, &c->zeros1k, 1024));
  {
    std::vector<float> one(1024, 1.0f);
    HIPCHECK(hipMemcpy(c->ones1k, one.data(), 1024 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(c->zeros1k, 0, 1024 * sizeof(float)));
  }
  DGCHECK(dmalloc(c, &c->n_mean0, 32)); DGCHECK(dmalloc(c, &c->n_rstd0, 32));
  DGCHECK(dmalloc(c, &c->n_mean1, 32)); DGCHECK(dmalloc(c, &c->n_rstd1, 32));
  DGCHECK(dmalloc(c, &c->n_meanh, 1024)); DGCHECK(dmalloc(c, &c->n_rstdh, 1024));
  DGCHECK(dmalloc(c, &c->n_dl, (size_t)B * 1024)); DGCHECK(dmalloc(c, &c->n_dflat, (size_t)B * 1024));
  DGCHECK(dmalloc(c, &c->n_dl1, (size_t)B * 1024)); DGCHECK(dmalloc(c, &c->n_da0, (size_t)B * 1024));
  DGCHECK(dmalloc(c, &c->n_dl0, (size_t)B * 1024));
  return DG_OK;
}

// ---------------------------------------------------------------------------
// noise MLP, learning phase 1
// ---------------------------------------------------------------------------
static NoiseParams lin_params(depgan_ctx* c) {
  NoiseParams P = c->np;
  P.sh = c->ones1k;
  P.th = c->zeros1k;
  return P;
}

static int u_noise_fwd(depgan_ctx* c, const float* z, int n) {
  Net& g = c->g;
  const int R = n * 32;
  const float corrR = (float)((double)R / ((double)R - (1.0 + (double)kBnEps)));
  const float corrN = (float)((double)n / ((double)n - (1.0 + (double)kBnEps)));
  UNoiseBn b0 = noise_bn(g, "dense_bn_noise_1_add_f0"), b1 = noise_bn(g, "dense_bn_noise_1_add_f1");
  DGCHECK(dg_small_gemm(z, c->np.W0, c->np.b0, c->na.h0, R, 1, 32, c->st));
  DGCHECK(dg_bn_rows_fwd(c->na.h0, c->na.a0, R, 32, 32, b0.gamma, b0.beta, kBnEps, kBnMomentum, corrR, b0.mm, b0.mv,
                         c->n_mean0, c->n_rstd0, 1, c->st));
  DGCHECK(dg_small_gemm(c->na.a0, c->np.W1, c->np.b1, c->na.h1, R, 32, 32, c->st));
  DGCHECK(dg_bn_rows_fwd(c->na.h1, c->na.a1, R, 32, 32, b1.gamma, b1.beta, kBnEps, kBnMomentum, corrR, b1.mm, b1.mv,
                         c->n_mean1, c->n_rstd1, 1, c->st));
  DGCHECK(dg_noise_heads_lin(lin_params(c), c->na.a1, c->na.lin, c->na.heads, n, c->st));
  for (int h = 0; h < NOISE_NHEADS; ++h) {
    UNoiseBn bh = noise_bn(g, std::string("dense_bn_noise_2_") + kUHeadSfx[h]);
    const int c0 = c->np.col0[h], nc = c->np.ncol[h];
    DGCHECK(dg_bn_rows_fwd(c->na.lin + c0, c->na.heads + c0, n, nc, 1024, bh.gamma, bh.beta, kBnEps, kBnMomentum,
                           corrN, bh.mm, bh.mv, c->n_meanh + c0, c->n_rstdh + c0, 0, c->st));
  }
  return DG_OK;
}

static int u_noise_bwd(depgan_ctx* c, const float* z, int n) {
  Net& g = c->g;
  const int R = n * 32;
  NoiseGrads& G = c->ng;
  for (int h = 0; h < NOISE_NHEADS; ++h) {
    UNoiseBn bh = noise_bn(g, std::string("dense_bn_noise_2_") + kUHeadSfx[h]);
    const int c0 = c->np.col0[h], nc = c->np.ncol[h];
    DGCHECK(dg_bn_rows_bwd(c->dheads + c0, c->na.lin + c0, nullptr, c->n_dl + c0, n, nc, 1024, bh.gamma,
                           c->n_meanh + c0, c->n_rstdh + c0, bh.dgamma, bh.dbeta, c->st));
    DGCHECK(dg_colsum_small(c->n_dl + c0, G.dbh[h], n, nc, 1024, c->st));
  }
  DGCHECK(dg_noise_heads_bwd_lin(lin_params(c), G, c->na.a1, c->n_dl, c->n_dflat, n, c->st));
  UNoiseBn b0 = noise_bn(g, "dense_bn_noise_1_add_f0"), b1 = noise_bn(g, "dense_bn_noise_1_add_f1");
  // layer f1: rows = (sample, position), 32 columns
  DGCHECK(dg_bn_rows_bwd(c->n_dflat, c->na.h1, c->na.a1, c->n_dl1, R, 32, 32, b1.gamma, c->n_mean1, c->n_rstd1,
                         b1.dgamma, b1.dbeta, c->st));
  DGCHECK(dg_colsum_small(c->n_dl1, G.db1, R, 32, 32, c->st));
  DGCHECK(dg_small_gemm_at(c->na.a0, c->n_dl1, G.dW1, R, 32, 32, c->st));
  DGCHECK(dg_small_gemm_bt(c->n_dl1, c->np.W1, c->n_da0, R, 32, 32, c->st));
  // layer f0
  DGCHECK(dg_bn_rows_bwd(c->n_da0, c->na.h0, c->na.a0, c->n_dl0, R, 32, 32, b0.gamma, c->n_mean0, c->n_rstd0,
                         b0.dgamma, b0.dbeta, c->st));
  DGCHECK(dg_colsum_small(c->n_dl0, G.db0, R, 32, 32, c->st));
  return dg_small_gemm_at(z, c->n_dl0, G.dW0, R, 1, 32, c->st);
}

// ---------------------------------------------------------------------------
// trunk, learning phase 1
// ---------------------------------------------------------------------------
static int u_bn_act(depgan_ctx* c, GLayer& L, int Ho, int Wo, int n, unsigned drop_seed) {
  ProfScope ps(c, 2, 0.0, "bn fwd: moments + affine / act");
  const double N = (double)n * Ho * Wo;
  DGCHECK(dg_col_moments(L.raw.view(), n, Ho, Wo, L.Cout, L.bmean, L.bvar, c->scratch, c->scratchFloats,
                         c->st));
  DGCHECK(dg_bn_train_prepare(L.gamma, L.beta, L.bmean, L.bvar, kBnEps, kBnMomentum, (float)(N / (N - 1.0)), L.mean,
                              L.var, L.bs, L.bt, L.brstd, L.Cout, c->st));
  AffineActArgs a;
  memset(&a, 0, sizeof(a));
  a.in = L.raw.view();
  a.out = L.out;
  a.out_pre = a.res = null_view();
  a.s = L.bs;
  a.t = L.bt;
  a.relu = 1;
  a.B = n; a.H = Ho; a.W = Wo; a.C = L.Cout;
  a.drop_rate = kDropRate;
  if (L.kind == G_FILM) {
    a.film_mul = c->na.heads + L.col_mul;
    a.film_add = c->na.heads + L.col_add;
    a.film_ld = 1024;
    a.res = L.in;
    a.out_pre = L.u.view();
  }
  if (L.kind == G_CONV && L.name == kDropLayer) a.drop_seed = drop_seed;
  return dg_affine_act(a, c->st);
}

static int u_forward_train(depgan_ctx* c, const float* x, const float* z, int n, unsigned drop_seed) {
  {
    ProfScope ps(c, 2, 0.0, "noise mlp fwd");
    DGCHECK(u_noise_fwd(c, z, n));
  }
  for (size_t i = 0; i < c->gl.size(); ++i) {
    GLayer& L = c->gl[i];
    if (L.kind == G_CONV || L.kind == G_FILM) {
      ConvArgs a = conv_args((i == 0) ? make_view(const_cast<float*>(x), L.H, L.W, L.Cin) : L.in, L.raw.view(),
                             n, L.H, L.W, L.Cin, L.Cout);
      a.ep.bias = L.b;
      conv_set_weights(&a, L.pf, L.wpf[0], L.Wt, L.Cin, L.Cout);
      DGCHECK(conv_launch(c, L.pf, a, 3));
      DGCHECK(u_bn_act(c, L, L.H, L.W, n, drop_seed));
    } else if (L.kind == G_POOL) {
      ProfScope ps(c, 2, 0.0, "maxpool");
      DGCHECK(dg_maxpool(c->gl[L.skip_of].out, L.out, n, L.H / 2, L.W / 2, L.Cout, c->st));
    } else if (L.kind == G_DECONV) {
      for (int t = 0; t < 4 && !deconv_fused(c, L, n); ++t) {
        ConvArgs a = conv_args(L.in, strided2(L.raw.view(), t / 2, t % 2), n, L.H, L.W, L.Cin, L.Cout);
        a.ep.bias = L.b;
        a.w = L.wpf[t];
        DGCHECK(conv_launch(c, L.pf, a, 1));
      }
      if (deconv_fused(c, L, n)) DGCHECK(deconv_fwd_launch(c, L, L.raw.view(), L.b, nullptr, nullptr, 0, n));
      DGCHECK(u_bn_act(c, L, 2 * L.H, 2 * L.W, n, 0));
    }
  }
  return DG_OK;
}

// the head's input, its gradient and its mask as pixel rows: dg_head_k_* take no (sB, sY, sX) views
static bool u_flat(const TView& t, int H, int W) { return t.sY == (long)W * t.sX && t.sB == (long)H * t.sY; }

// 1x1 head to the class logits, dense (P, nc_out).  4 classes: the direct kernel (N = 4 is far below an MFMA tile);
// any other count: dg_head_k_fwd
static int u_head_logits(depgan_ctx* c, int n) {
  GLayer& L = c->gl.back();
  if (L.Cout != 4) {
    ProfScope ps(c, 2, 0.0, "head fwd (classes)");
    if (!u_flat(L.in, L.H, L.W)) { dg_set_error("uresnet: the head's input is not pixel-contiguous"); return DG_ERR_UNSUPPORTED; }
    return dg_head_k_fwd(L.in.p, L.in.sX, L.Wt, L.b, c->logits, (long)n * L.H * L.W, L.Cin, L.Cout, c->st);
  }
  ConvArgs a = conv_args(L.in, make_view(c->logits, L.H, L.W, 4), n, L.H, L.W, L.Cin, 4);
  a.ep.bias = L.b;
  conv_set_weights(&a, dg_plan_direct(), nullptr, L.Wt, L.Cin, 4);
  return conv_launch(c, dg_plan_direct(), a, 1);
}

// BN backward of one layer: dy (grad at the BN output, ReLU / FiLM already applied) -> dRAW in draw_tmp,
// dgamma / dbeta written.  dyscale: constant factor still to be applied to dy (dropout's 1/(1-rate)).
static int u_bn_bwd(depgan_ctx* c, GLayer& L, TView dy, int Ho, int Wo, int n, float dyscale, TView* draw) {
  ProfScope ps(c, 2, 0.0, "bn bwd: sums + dRAW");
  const double N = (double)n * Ho * Wo;
  *draw = make_view(c->draw_tmp.p, Ho, Wo, L.Cout);
  DGCHECK(dg_colsum_pair(dy, L.raw.view(), L.bmean, n, Ho, Wo, L.Cout, L.sums, c->scratch, c->scratchFloats,
                         c->st));
  DGCHECK(dg_bn_bwd_coeffs(L.sums, L.bmean, L.brstd, L.bs, (float)(1.0 / N), dyscale, L.dgamma, L.dbeta, L.cA, L.cB,
                           L.cC, L.Cout, c->st));
  return dg_axpby_ch(dy, L.raw.view(), *draw, n, Ho, Wo, L.Cout, L.cA, L.cB, L.cC, c->st);
}

static int u_conv_bwd(depgan_ctx* c, GLayer& L, size_t li, const float* x_user, TView dy, TView res, int n,
                      float dyscale) {
  TView xin = (li == 0) ? make_view(const_cast<float*>(x_user), L.H, L.W, L.Cin) : L.in;
  TView draw;
  DGCHECK(u_bn_bwd(c, L, dy, L.H, L.W, n, dyscale, &draw));
  const ColSum cs = {n, nullptr, L.db, nullptr};
  DGCHECK(wgrad_full(c, 3, xin, draw, n, L.H, L.W, L.Cin, L.Cout, nullptr, L.dW, nullptr, 0, 0, &cs));
  if (li == 0) return DG_OK;
  ConvArgs a = conv_args(draw, L.din, n, L.H, L.W, L.Cout, L.Cin);
  a.w = L.wpb[0];
  a.ep.res = res;
  a.ep.mask = L.in_mask;
  return conv_launch(c, L.pb, a, 3);
}

static int u_backward(depgan_ctx* c, const float* x, const float* z, int n) {
  for (int i = (int)c->gl.size() - 1; i >= 0; --i) {
    GLayer& L = c->gl[i];
    if (L.kind == G_HEAD && L.Cout != 4) {
      ProfScope ps(c, 2, 0.0, "head bwd (classes)");
      const long P = (long)n * L.H * L.W;
      if (!u_flat(L.in, L.H, L.W) || !u_flat(L.din, L.H, L.W) || (L.in_mask.p && !u_flat(L.in_mask, L.H, L.W))) {
        dg_set_error("uresnet: the head's input, gradient or mask is not pixel-contiguous");
        return DG_ERR_UNSUPPORTED;
      }
      DGCHECK(dg_head_k_wgrad(L.in.p, L.in.sX, c->dz, L.dW, L.db, P, L.Cin, L.Cout, c->scratch, c->scratchFloats,
                              c->st));
      DGCHECK(dg_head_k_bwd(c->dz, L.Wt, L.in_mask.p, L.in_mask.sX, L.din.p, L.din.sX, P, L.Cin, L.Cout, c->st));
    } else if (L.kind == G_HEAD) {
      TView dzv = make_view(c->dz, L.H, L.W, 4);
      const ColSum cs = {n, nullptr, L.db, nullptr};
      DGCHECK(wgrad_full(c, 1, L.in, dzv, n, L.H, L.W, L.Cin, 4, nullptr, L.dW, nullptr, 0, 0, &cs));
      ConvArgs a = conv_args(dzv, L.din, n, L.H, L.W, 4, L.Cin);
      conv_set_weights_bwd(&a, dg_plan_direct(), nullptr, L.Wt, L.Cin, 4);   // W[ci][co] read as (k = co, n = ci)
      a.ep.mask = L.in_mask;
      DGCHECK(conv_launch(c, dg_plan_direct(), a, 1));
    } else if (L.kind == G_CONV) {
      const float k = (L.name == kDropLayer && c->last_drop_seed) ? 1.0f / (1.0f - kDropRate) : 1.0f;
      DGCHECK(u_conv_bwd(c, L, (size_t)i, x, L.dout, null_view(), n, k));
    } else if (L.kind == G_FILM) {
      TView du = make_view(c->du_tmp.p, L.H, L.W, L.Cout);
      {
        ProfScope ps(c, 2, 0.0, "film bwd");
        DGCHECK(dg_film_bwd(L.dout.p, L.u.p, c->na.heads + L.col_mul, c->na.heads + L.col_add, 1024, du.p,
                            c->dheads + L.col_mul, c->dheads + L.col_add, n, (long)L.H * L.W, L.Cout, c->scratch,
                            c->scratchFloats, c->st));
      }
      DGCHECK(u_conv_bwd(c, L, (size_t)i, x, du, L.dout, n, 1.0f));
    } else if (L.kind == G_POOL) {
      ProfScope ps(c, 2, 0.0, "unpool+mask");
      DGCHECK(dg_unpool_mask(L.pool_dsrc, c->gl[L.skip_of].out, L.pool_skipgrad, L.pool_dst, n, L.H / 2, L.W / 2,
                             L.Cout, c->st));
    } else if (L.kind == G_DECONV) {
      const int Ho = 2 * L.H, Wo = 2 * L.W;
      TView draw;
      DGCHECK(u_bn_bwd(c, L, L.dout, Ho, Wo, n, 1.0f, &draw));
      DGCHECK(deconv_wgrad_all(c, L, L.in, draw, n, nullptr, nullptr, nullptr, L.db, nullptr));
      DGCHECK(deconv_bwd_data(c, L, draw, n));
    }
  }
  ProfScope ps(c, 2, 0.0, "noise mlp bwd");
  return u_noise_bwd(c, z, n);
}

// ---------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------
static int u_check(depgan_ctx* c, const char* who) {
  DGCHECK(infer_refuse(c, who));
  if (!c->train_bn) {
    dg_set_error("%s: the context was not created with nc_out >= 2", who);
    return DG_ERR_ARG;
  }
  return DG_OK;
}

// phase 0 (predict / validation): moving statistics, no dropout
static int u_forward_infer(depgan_ctx* c, const float* x, const float* z, int n) {
  DGCHECK(g_forward(c, x, z, n, false));
  return u_head_logits(c, n);
}

int uresnet_predict(depgan_ctx* c, const float* x, const float* z, float* out, int n) {
  DGCHECK(u_forward_infer(c, x, z, n));
  const long P = (long)n * c->cfg.height * c->cfg.width;
  ProfScope ps(c, 2, 0.0, "softmax");
  SoftmaxCeArgs a{};
  a.logits = c->logits;
  a.probs = out;
  a.P = P;
  a.C = c->cfg.nc_out;
  return dg_softmax_ce(a, c->st);
}

// The cross-entropy of one call under the context's setting; what it leaves for the host goes to loss_dev (ULossHost)
static int u_softmax_ce_only(depgan_ctx* c, DgLabels lab, long P) {
  ProfScope ps(c, 2, 0.0, "softmax + cross-entropy");
  DgCeDev* dev = &reinterpret_cast<ULossHost*>(c->loss_dev)->ce;
  const SoftmaxCeArgs a = {c->logits, lab, c->attr.p, c->dz, &dev->loss, &dev->bad, dev->census, dev->counts, c->loss.ce,
                           P, c->cfg.nc_out, c->scratch, c->scratchFloats};
  return dg_softmax_ce(a, c->st);
}

// The Dice mode: its three launches follow the cross-entropy on the stream and reuse the scratch (the cross-entropy's
// second stage has read its partials by then).  A pixel takes part unless the loss-weight mode says it has no true class:
// the ignore code with codes, the all-zero row with one-hot labels.  grad = false (eval): no gradient pass
static int u_softmax_ce(depgan_ctx* c, DgLabels lab, long P, bool grad) {
  DGCHECK(u_softmax_ce_only(c, lab, P));
  const DgCeSetting& ce = c->loss.ce;
  const int ignore = !ce.weighted ? -1 : (lab.codes ? ce.ignore : 0);
  ULossHost* dev = reinterpret_cast<ULossHost*>(c->loss_dev);
  if (c->loss.dice.form != DEPGAN_DICE_OFF) {
    ProfScope ps(c, 2, 0.0, "dice loss");
    DGCHECK(dg_dice_loss(c->attr.p, lab, ignore, c->loss.dice, grad ? c->dz : nullptr, &dev->dice, P, c->cfg.nc_out,
                         c->scratch, c->scratchFloats, c->st));
  }
  // The boundary mode, last: the signed distance maps of this call's labels (two launches whatever n), then one pass
  // that adds its gradient to what the cross-entropy and the Dice mode left in dz, and the one-block sum.  The same
  // pixels take part as in the Dice term; M is read on the device from the label pre-pass's counts
  if (!c->loss.boundary.on) return DG_OK;
  ProfScope ps(c, 2, 0.0, "boundary loss");
  const DgBoundarySetting& b = c->loss.boundary;
  const int C = c->cfg.nc_out;
  DGCHECK(dg_signed_distance(lab, ignore, P / ((long)c->cfg.height * c->cfg.width), c->cfg.height, c->cfg.width, C,
                             b.class_mask(C), b.sy, b.sx, b.inside_offset, c->bl_phi, c->bl_rows, c->bl_rows_bytes,
                             c->st));
  return dg_boundary_loss(c->attr.p, c->bl_phi, lab, ignore, b.c, b.coef, ce.weighted ? dev->ce.counts : nullptr,
                          grad ? c->dz : nullptr, &dev->bl, P, C, c->bl_part, dg_boundary_scratch(P), c->st);
}

// the one synchronisation of a call: what the launches under the setting left in loss_dev comes back in one copy -- the
// summed loss and the count of out-of-range class codes, the census, the label counts behind the largest census, and
// the Dice sums and term behind those
static int u_loss_to_host(depgan_ctx* c, const char* who, long P, float* loss_host) {
  const DgCeSetting& ce = c->loss.ce;
  const DgDiceSetting& dice = c->loss.dice;
  const int C = c->cfg.nc_out;
  ULossHost h;
  h.ce.loss = 0.f;
  h.ce.bad = 0;
  const DgBoundarySetting& bl = c->loss.boundary;
  const size_t bytes = bl.on ? sizeof(ULossHost)
                             : dice.form != DEPGAN_DICE_OFF ? offsetof(ULossHost, dice) + offsetof(DgDiceDev, A)
                                                            : DgCeDev::bytes(C, ce);
  HIPCHECK(hipMemcpyAsync(&h, c->loss_dev, bytes, hipMemcpyDeviceToHost, c->st));
  HIPCHECK(hipStreamSynchronize(c->st));
  if (ce.census) {
    memcpy(c->last.census, h.ce.census, (size_t)C * C * sizeof(long long));
    c->last.census_valid = true;
  }
  // the mean's denominator: every pixel, or on the weighted path the pixels with a non-zero weight (0.0 for none)
  float den = (float)P;
  if (ce.weighted_path()) {
    memcpy(c->last.counts, h.ce.counts, (size_t)(C + 3) * sizeof(long long));
    c->last.counts_valid = true;
    den = (float)h.ce.counts[0];
  }
  c->last_sums[0] = h.ce.loss;
  c->last_sums[1] = den;
  float loss = (den != 0.f) ? h.ce.loss / den : 0.f;
  if (dice.form != DEPGAN_DICE_OFF) {
    memcpy(c->last.dice_sums, h.dice.sums, (size_t)3 * C * sizeof(double));
    c->last.dice_loss = h.dice.loss;
    c->last.dice_valid = true;
    loss = dice.ce_coef * loss + dice.dice_coef * h.dice.loss;
  }
  if (bl.on) {
    c->last.boundary_loss = h.bl.loss;
    c->last.boundary_M = h.bl.M;
    c->last.boundary_valid = true;
    loss = loss + bl.coef * (float)h.bl.loss;
  }
  if (loss_host) *loss_host = loss;
  if (h.ce.bad) {
    dg_set_error("%s: %u of %ld class codes are outside [0, %d)", who, h.ce.bad, P, C);
    return DG_ERR_ARG;
  }
  return DG_OK;
}

static int u_grads(depgan_ctx* c, const char* who, const float* x, const float* z, DgLabels lab, int n,
                   unsigned drop_seed, float* loss_host, bool refresh_bn) {
  DGCHECK(u_check(c, who));
  if (n < 1 || n > c->cfg.batch) {
    dg_set_error("uresnet: n must be in [1, batch]");
    return DG_ERR_ARG;
  }
  if (!lab.onehot && !lab.codes) { dg_set_error("%s: null labels", who); return DG_ERR_ARG; }
  const long P = (long)n * c->cfg.height * c->cfg.width;
  c->last_drop_seed = drop_seed;
  DGCHECK(u_forward_train(c, x, z, n, drop_seed));
  DGCHECK(u_head_logits(c, n));
  DGCHECK(u_softmax_ce(c, lab, P, true));
  DGCHECK(u_backward(c, x, z, n));
  // the forward pass moved the BN moving statistics: the phase-0 affines are stale (the step variant
  // refreshes everything after Adam anyway)
  if (refresh_bn) DGCHECK(refresh_generator_bn(c));
  const int rc = u_loss_to_host(c, who, P, loss_host);
  // a refused step applies no Adam, so nothing after it refreshes the phase-0 affines of the statistics that moved
  if (rc != DG_OK && !refresh_bn) refresh_generator_bn(c);
  return rc;
}

static int u_step(depgan_ctx* c, const char* who, const float* x, const float* z, DgLabels lab, int n,
                  unsigned drop_seed, float* loss_host) {
  DGCHECK(infer_refuse(c, who));
  // an out-of-range class code comes back here as status 1, after the loss fetch: no Adam update, the step counter
  // stays; the phase-1 forward has moved the BN moving statistics by then, as depgan_uresnet_grads always does
  DGCHECK(u_grads(c, who, x, z, lab, n, drop_seed, loss_host, false));
  // the loss-weight mode or the focal mode with no weighted pixel in the batch: loss 0.0 and an all-zero dz, status 0; no Adam update and
  // the step counter stays, the path of a refused sparse step (the moving statistics have moved)
  // With the Dice mode on the same holds once no pixel takes part in the Dice term either: every pixel is without a true
  // class (then den == 0 too); pixels of zero-weight classes still carry a Dice gradient, and that batch is updated
  const long P = (long)n * c->cfg.height * c->cfg.width;
  const bool ce_empty = c->loss.ce.weighted_path() && c->last.counts[0] == 0;
  const bool dice_empty = c->loss.ce.weighted && c->last.counts[1] + c->last.counts[2] == P;
  // The boundary mode follows the Dice mode's rule: its term has a gradient wherever a pixel takes part
  const bool regional_only = c->loss.dice.form == DEPGAN_DICE_OFF && !c->loss.boundary.on;
  if (regional_only ? ce_empty : dice_empty) return refresh_generator_bn(c);
  return depgan_apply_adam(c, DEPGAN_NET_G);
}

static int u_eval(depgan_ctx* c, const char* who, const float* x, const float* z, DgLabels lab, int n,
                  float* loss_host) {
  DGCHECK(u_check(c, who));
  if (n < 1 || n > c->cfg.batch) { dg_set_error("uresnet_eval: n must be in [1, batch]"); return DG_ERR_ARG; }
  if (!lab.onehot && !lab.codes) { dg_set_error("%s: null labels", who); return DG_ERR_ARG; }
  const long P = (long)n * c->cfg.height * c->cfg.width;
  DGCHECK(u_forward_infer(c, x, z, n));
  DGCHECK(u_softmax_ce(c, lab, P, false));
  return u_loss_to_host(c, who, P, loss_host);
}

extern "C" {

int depgan_uresnet_set_census(depgan_ctx* c, int on) {
  if (!c) { dg_set_error("depgan_uresnet_set_census: null context"); return DG_ERR_ARG; }
  if (on != 0 && on != 1) { dg_set_error("depgan_uresnet_set_census: on must be 0 or 1, got %d", on); return DG_ERR_ARG; }
  if (on) {
    DGCHECK(u_check(c, "depgan_uresnet_set_census"));
  }
  c->loss.ce.census = on != 0;
  if (!on) c->last.census_valid = false;
  return DG_OK;
}
int depgan_uresnet_get_census(depgan_ctx* c) { return (c && c->loss.ce.census) ? 1 : 0; }
int depgan_uresnet_last_census(depgan_ctx* c, long long out_host[DEPGAN_MAX_HEAD_CLASSES * DEPGAN_MAX_HEAD_CLASSES],
                               int* classes) {
  if (!c || !out_host) { dg_set_error("depgan_uresnet_last_census: null argument"); return DG_ERR_ARG; }
  if (!c->loss.ce.census || !c->last.census_valid) {
    dg_set_error("depgan_uresnet_last_census: no depgan_uresnet_* call has run with the census on "
                 "(depgan_uresnet_set_census)");
    return DG_ERR_ARG;
  }
  const int C = c->cfg.nc_out;
  memcpy(out_host, c->last.census, (size_t)C * C * sizeof(long long));
  if (classes) *classes = C;
  return DG_OK;
}

int depgan_uresnet_set_loss_weights(depgan_ctx* c, const float* w_host, int n, int ignore_code) {
  if (!c) { dg_set_error("depgan_uresnet_set_loss_weights: null context"); return DG_ERR_ARG; }
  if (!w_host) {
    c->loss.ce.weighted = c->last.counts_valid = false;
    return DG_OK;
  }
  DGCHECK(u_check(c, "depgan_uresnet_set_loss_weights"));
  DGCHECK(dg_loss_weights_check("depgan_uresnet_set_loss_weights", w_host, n, c->cfg.nc_out, ignore_code));
  c->loss.ce.set_weights(w_host, n, ignore_code);
  c->last.counts_valid = false;
  return DG_OK;
}
int depgan_uresnet_get_loss_weights(depgan_ctx* c, float w_host[DEPGAN_MAX_HEAD_CLASSES], int* ignore_code) {
  if (!c || !c->loss.ce.weighted) return 0;
  if (w_host) memcpy(w_host, c->loss.ce.cw, (size_t)c->cfg.nc_out * sizeof(float));
  if (ignore_code) *ignore_code = c->loss.ce.ignore;
  return 1;
}
int depgan_uresnet_last_label_counts(depgan_ctx* c, long long out_host[DEPGAN_LABEL_NCOUNT], int* classes) {
  if (!c || !out_host) { dg_set_error("depgan_uresnet_last_label_counts: null argument"); return DG_ERR_ARG; }
  if (!c->loss.ce.weighted_path() || !c->last.counts_valid) {
    dg_set_error("depgan_uresnet_last_label_counts: no depgan_uresnet_* call has run in the loss-weight mode "
                 "(depgan_uresnet_set_loss_weights) or the focal mode (depgan_uresnet_set_focal)");
    return DG_ERR_ARG;
  }
  memcpy(out_host, c->last.counts, (size_t)(c->cfg.nc_out + 3) * sizeof(long long));
  if (classes) *classes = c->cfg.nc_out;
  return DG_OK;
}

int depgan_uresnet_set_focal(depgan_ctx* c, float gamma, float label_smoothing) {
  if (!c) { dg_set_error("depgan_uresnet_set_focal: null context"); return DG_ERR_ARG; }
  DGCHECK(dg_focal_check("depgan_uresnet_set_focal", gamma, label_smoothing));
  const bool on = gamma != 0.f || label_smoothing != 0.f;
  if (on) {
    DGCHECK(u_check(c, "depgan_uresnet_set_focal"));
  }
  c->loss.ce.focal = on;
  c->loss.ce.gamma = on ? gamma : 0.f;
  c->loss.ce.eps = on ? label_smoothing : 0.f;
  // the counts on the host are those of a call made under the setting in force
  c->last.counts_valid = false;
  return DG_OK;
}
int depgan_uresnet_get_focal(depgan_ctx* c, float* gamma, float* label_smoothing) {
  if (!c || !c->loss.ce.focal) return 0;
  if (gamma) *gamma = c->loss.ce.gamma;
  if (label_smoothing) *label_smoothing = c->loss.ce.eps;
  return 1;
}

int depgan_uresnet_set_dice_loss(depgan_ctx* c, int form, float ce_coef, float dice_coef, float smooth,
                                 const float* class_coef_host, int n) {
  if (!c) { dg_set_error("depgan_uresnet_set_dice_loss: null context"); return DG_ERR_ARG; }
  if (form == DEPGAN_DICE_OFF) {
    c->loss.dice.form = DEPGAN_DICE_OFF;
    c->last.dice_valid = false;
    return DG_OK;
  }
  DGCHECK(u_check(c, "depgan_uresnet_set_dice_loss"));
  const int C = c->cfg.nc_out;
  DGCHECK(dg_dice_check("depgan_uresnet_set_dice_loss", form, ce_coef, dice_coef, smooth, class_coef_host, n, C));
  c->loss.dice.set(form, ce_coef, dice_coef, smooth, class_coef_host, C);
  c->last.dice_valid = false;
  return DG_OK;
}
int depgan_uresnet_get_dice_loss(depgan_ctx* c, float* ce_coef, float* dice_coef, float* smooth,
                                 float class_coef_host[DEPGAN_MAX_HEAD_CLASSES]) {
  if (!c || c->loss.dice.form == DEPGAN_DICE_OFF) return DEPGAN_DICE_OFF;
  const DgDiceSetting& d = c->loss.dice;
  if (ce_coef) *ce_coef = d.ce_coef;
  if (dice_coef) *dice_coef = d.dice_coef;
  if (smooth) *smooth = d.smooth;
  if (class_coef_host && d.form == DEPGAN_DICE_CLASS) memcpy(class_coef_host, d.c, (size_t)c->cfg.nc_out * sizeof(float));
  return d.form;
}
int depgan_uresnet_last_dice_sums(depgan_ctx* c, double out_host[3 * DEPGAN_MAX_HEAD_CLASSES], int* classes,
                                  float* dice_loss) {
  if (!c || !out_host) { dg_set_error("depgan_uresnet_last_dice_sums: null argument"); return DG_ERR_ARG; }
  if (c->loss.dice.form == DEPGAN_DICE_OFF || !c->last.dice_valid) {
    dg_set_error("depgan_uresnet_last_dice_sums: no depgan_uresnet_* call has run with the Dice loss on "
                 "(depgan_uresnet_set_dice_loss)");
    return DG_ERR_ARG;
  }
  memcpy(out_host, c->last.dice_sums, (size_t)3 * c->cfg.nc_out * sizeof(double));
  if (classes) *classes = c->cfg.nc_out;
  if (dice_loss) *dice_loss = c->last.dice_loss;
  return DG_OK;
}

int depgan_uresnet_set_boundary_loss(depgan_ctx* c, int on, float boundary_coef, const float* class_coef_host, int n,
                                     double sy, double sx, double inside_offset) {
  const char* who = "depgan_uresnet_set_boundary_loss";
  if (!c) { dg_set_error("%s: null context", who); return DG_ERR_ARG; }
  if (on != 0 && on != 1) { dg_set_error("%s: on must be 0 or 1, got %d", who, on); return DG_ERR_ARG; }
  if (!on) {
    c->loss.boundary.on = c->last.boundary_valid = false;
    return DG_OK;
  }
  DGCHECK(u_check(c, who));
  const int C = c->cfg.nc_out, B = c->cfg.batch, H = c->cfg.height, W = c->cfg.width;
  DGCHECK(dg_boundary_check(who, boundary_coef, class_coef_host, n, C));
  DGCHECK(dg_signed_distance_check(who, B, H, W, C, sy, sx, inside_offset));
  // the buffers, once: phi, the row pass's maps for every class (so that other coefficients need no other buffer) and
  // the block partials.  Setting the mode again finds them and allocates nothing.  Each pointer is kept as it is
  // obtained (dalloc_bytes registers it with the context only on success), so a call that runs out of memory half way
  // leaves what it got to the next call instead of allocating it twice
  if (!c->bl_phi || !c->bl_rows || !c->bl_part) {
    const size_t rbytes = dg_signed_distance_scratch_bytes(B, H, W, C);
    hipError_t e = hipSuccess;
    void* p = nullptr;
    if (!c->bl_phi && (e = dalloc_bytes(c, &p, (size_t)B * H * W * C * sizeof(float))) == hipSuccess) c->bl_phi = (float*)p;
    if (e == hipSuccess && !c->bl_rows && (e = dalloc_bytes(c, &p, rbytes)) == hipSuccess) {
      c->bl_rows = p;
      c->bl_rows_bytes = rbytes;
    }
    if (e == hipSuccess && !c->bl_part &&
        (e = dalloc_bytes(c, &p, dg_boundary_scratch((long)B * H * W) * sizeof(double))) == hipSuccess)
      c->bl_part = (double*)p;
    if (e == hipErrorOutOfMemory) {
      dg_set_error("%s: out of device memory for the signed distance maps (%zu bytes)", who,
                   (size_t)B * H * W * C * sizeof(float) + rbytes);
      return DG_ERR_HIP;
    }
    HIPCHECK(e);
    DGCHECK(dalloc_fills_done());
  }
  DgBoundarySetting& b = c->loss.boundary;
  b.on = true;
  b.coef = boundary_coef;
  for (int k = 0; k < C; ++k) b.c[k] = class_coef_host ? class_coef_host[k] : 1.0f / (float)C;
  b.sy = sy;
  b.sx = sx;
  b.inside_offset = inside_offset;
  c->last.boundary_valid = false;
  return DG_OK;
}
int depgan_uresnet_get_boundary_loss(depgan_ctx* c, float* boundary_coef, float class_coef_host[DEPGAN_MAX_HEAD_CLASSES],
                                     double* sy, double* sx, double* inside_offset) {
  if (!c || !c->loss.boundary.on) return 0;
  const DgBoundarySetting& b = c->loss.boundary;
  if (boundary_coef) *boundary_coef = b.coef;
  if (class_coef_host) memcpy(class_coef_host, b.c, (size_t)c->cfg.nc_out * sizeof(float));
  if (sy) *sy = b.sy;
  if (sx) *sx = b.sx;
  if (inside_offset) *inside_offset = b.inside_offset;
  return 1;
}
int depgan_uresnet_last_boundary_loss(depgan_ctx* c, double* boundary_loss, long long* taking_part) {
  if (!c || !boundary_loss) { dg_set_error("depgan_uresnet_last_boundary_loss: null argument"); return DG_ERR_ARG; }
  if (!c->loss.boundary.on || !c->last.boundary_valid) {
    dg_set_error("depgan_uresnet_last_boundary_loss: no depgan_uresnet_* call has run with the boundary loss on "
                 "(depgan_uresnet_set_boundary_loss)");
    return DG_ERR_ARG;
  }
  *boundary_loss = c->last.boundary_loss;
  if (taking_part) *taking_part = (long long)c->last.boundary_M;
  return DG_OK;
}

int depgan_uresnet_grads(depgan_ctx* c, const float* x, const float* z, const float* labels, int n,
                         unsigned drop_seed, float* loss_host) {
  return u_grads(c, "uresnet_grads", x, z, DgLabels{labels, nullptr}, n, drop_seed, loss_host, true);
}
int depgan_uresnet_step(depgan_ctx* c, const float* x, const float* z, const float* labels, int n,
                        unsigned drop_seed, float* loss_host) {
  return u_step(c, "depgan_uresnet_step", x, z, DgLabels{labels, nullptr}, n, drop_seed, loss_host);
}
int depgan_uresnet_eval(depgan_ctx* c, const float* x, const float* z, const float* labels, int n,
                        float* loss_host) {
  return u_eval(c, "uresnet_eval", x, z, DgLabels{labels, nullptr}, n, loss_host);
}

int depgan_uresnet_grads_sparse(depgan_ctx* c, const float* x, const float* z, const unsigned char* codes, int n,
                                unsigned drop_seed, float* loss_host) {
  return u_grads(c, "uresnet_grads_sparse", x, z, DgLabels{nullptr, codes}, n, drop_seed, loss_host, true);
}
int depgan_uresnet_step_sparse(depgan_ctx* c, const float* x, const float* z, const unsigned char* codes, int n,
                               unsigned drop_seed, float* loss_host) {
  return u_step(c, "depgan_uresnet_step_sparse", x, z, DgLabels{nullptr, codes}, n, drop_seed, loss_host);
}
int depgan_uresnet_eval_sparse(depgan_ctx* c, const float* x, const float* z, const unsigned char* codes, int n,
                               float* loss_host) {
  return u_eval(c, "uresnet_eval_sparse", x, z, DgLabels{nullptr, codes}, n, loss_host);
}

}  // extern "C"
