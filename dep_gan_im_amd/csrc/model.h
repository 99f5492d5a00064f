// Host-side model state for the DEP-GAN hot path: parameter arenas, layer
// tables (GT:316-345, GT:349-498), activation storage and the step drivers.
#pragma once
#include <string.h>

#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/depgan.h"
#include "common.h"
#include "bf16s.h"
#include "bf16s_train.h"
#include "deconv_fwd.h"
#include "noise.h"
#include "ops.h"
#include "train_ops.h"

struct PInfo {
  std::string name;
  int shape[4];
  int ndim;
  size_t off, size;
  bool trainable;
};

struct Net {
  std::vector<PInfo> params;
  std::map<std::string, int> index;
  size_t nTrain = 0, nNon = 0;
  float *P = nullptr, *NT = nullptr, *G = nullptr, *M = nullptr, *V = nullptr;
  // bf16-weights mode (BASELINE config 4): P stays the fp32 master that Adam updates; every kernel reads the
  // compute copy Pq, in which the "/kernel" tensors are rounded to bf16 (RNE) and everything else is P verbatim
  float* Pq = nullptr;
  unsigned char* qmask = nullptr;   // 1 where Pq is rounded
  long adam_t = 0;
  float lr = 1e-4f;
  // depgan_set_optimizer (all 0: net_adam launches the plain kernel).  decay_bits: bit i set where element i of the
  // arena belongs to a "/kernel" tensor; gnorm: 3 doubles on the device, the squared norm, the norm and the scale of the
  // last clipped update (both allocated by the first call that turns an option on)
  float clipnorm = 0.f, clipvalue = 0.f, weight_decay = 0.f;
  unsigned* decay_bits = nullptr;
  double* gnorm = nullptr;
  bool gnorm_valid = false;
  void add(const std::string& name, std::vector<int> shape, bool trainable);
  float* p(const std::string& name) const;   // parameter pointer the kernels read (either arena; Pq when quantised)
  float* g(const std::string& name) const;   // gradient pointer (trainable only)
};

struct Tn {  // dense NHWC tensor
  float* p = nullptr;
  int H = 0, W = 0, C = 0;
  TView view() const { return make_view(p, H, W, C); }
  TView slice(int c0) const { return make_view_slice(p, H, W, C, c0); }
  size_t per_sample() const { return (size_t)H * W * C; }
};

enum GKind { G_CONV, G_FILM, G_POOL, G_DECONV, G_HEAD };

struct GLayer {
  GKind kind;
  std::string name;
  int Cin = 0, Cout = 0;
  int H = 0, W = 0;      // spatial size of the layer INPUT
  // parameters
  float *Wt = nullptr, *b = nullptr, *gamma = nullptr, *beta = nullptr, *mean = nullptr, *var = nullptr;
  float *dW = nullptr, *db = nullptr, *dgamma = nullptr, *dbeta = nullptr;
  float *s = nullptr, *t = nullptr, *rstd = nullptr;
  // packed weights (deconv: one per tap)
  ConvPlan pf, pb;
  float* wpf[4] = {nullptr, nullptr, nullptr, nullptr};
  float* wpb[4] = {nullptr, nullptr, nullptr, nullptr};
  // deconv backward-data as ONE 1x1 convolution over the four strided grids of the upstream gradient (K = 4 Cout):
  // the four per-tap panels interleaved per channel tile; null when the channel counts do not allow it
  ConvPlan pbf;
  float* wpb_all = nullptr;
  // FiLM
  int col_mul = -1, col_add = -1;
  // tensors
  TView in, out;           // forward views (in has Cin channels, out has Cout)
  // bf16 activation storage (bf16s_alloc, bf16_mfma contexts): the bf16 twins of in / out, concat buffers shared as in
  // the fp32 set; FiLM layers of the generator update (bf16s_train_alloc): RNE_bf16(u) and the ReLU decision bits
  TViewH hin = null_view_h(), hout = null_view_h(), hu = null_view_h();
  unsigned char* hdec = nullptr;
  int cat_deconv = -1;     // conv that feeds a pool: index of the transposed convolution that shares its concat buffer
  TView din, dout;         // gradient views (dout = grad wrt out, after the producer's mask)
  TView in_mask;           // mask applied when writing din (null: none)
  Tn u;                    // FiLM pre-activation (kept when training G)
  // learning-phase-1 path (DEP-UResNet): raw conv output and batch-statistics BN state
  Tn raw;
  float *bmean = nullptr, *bvar = nullptr, *bs = nullptr, *bt = nullptr, *brstd = nullptr;
  float *cA = nullptr, *cB = nullptr, *cC = nullptr, *sums = nullptr;
  int skip_of = -1;        // pool: index of the conv layer whose output is pooled
  TView pool_dsrc;         // pool: gradient wrt the pooled tensor (raw)
  TView pool_skipgrad;     // pool: gradient arriving through the concat
  TView pool_dst;          // pool: masked gradient of the pooled conv's output
};

struct DLayer {
  std::string name;
  int KS, Cin, Cout, H, W;  // H, W: spatial size at this layer
  bool pool;
  ConvPlan pf, pb;
  // depgan_set_critic16_pipe: the 16-channel bf16 plans of the launches the bf16 plan above leaves on the fp32 pipe
  // (dis_0b forward, dis_0b / dis_1a backward-data); has16f / has16b say where one exists (bf16_mfma contexts only)
  ConvPlan pf16, pb16;
  bool has16f = false, has16b = false;
};

struct DNet {
  Net net;
  PackJob* pack_jobs = nullptr;   // device table of this critic's packing jobs (built at the first refresh)
  int n_pack = 0;
  unsigned pack_blocks = 0;
  float* wpf[11];
  float* wpb[11];
  float* wpf16[11];                // panels of DLayer::pf16 / pb16 (null where the layer has none); packed with the others
  float* wpb16[11];
  float *W[11], *b[11], *dW[11], *db[11];
  float *w9, *b9, *wd, *bd, *dw9, *db9, *dwd, *dbd;
};

struct ProfRec {
  hipEvent_t a, b;
  int klass;
  double flops;
  double bytes;   // algorithmic HBM bytes of the launch (operands read once, results written once)
  char label[56];
  char kernel[48];   // kernel instantiation (class 0 / 1) as rocprofv3 names it; empty for the HBM-bound helpers
};

struct depgan_ctx {
  depgan_config cfg;
  hipStream_t st = nullptr;
  std::vector<void*> allocs;

  // ---- generator ----
  Net g;
  std::vector<GLayer> gl;
  NoiseParams np;
  NoiseGrads ng;
  NoiseActs na;
  float* derived = nullptr;       // BN affines
  // device tables for the batched refresh launches (built at the first refresh; every pointer in them is stable)
  PackJob* g_pack_jobs = nullptr;
  int g_n_pack = 0;
  unsigned g_pack_blocks = 0;
  BnJob* g_bn_jobs = nullptr;
  int g_n_bn = 0;
  // BN-gamma gradients of the generator: the un-scaled weight gradients of a backward pass are kept per layer
  // (raw_all mirrors the gradient arena) and all gammas are formed in ONE launch at the end of the pass
  float* raw_all = nullptr;
  GammaJob* g_gamma_jobs = nullptr;
  int g_n_gamma = 0, g_gamma_blocks = 0;
  float* heads_mean = nullptr;    // concatenated moving means of the head BNs
  float* dheads = nullptr;        // [B][1024]
  Tn attr;                        // generator output (B,H,W,1)
  Tn du_tmp;                      // FiLM dU scratch (largest FiLM tensor)
  float* dpre = nullptr;          // [B*H*W]
  float* zbuf = nullptr;          // [B][32]

  // ---- critics ----
  DNet d[2];
  std::vector<DLayer> dl;
  int NB3 = 0;                     // 3*B
  float* d_in = nullptr;           // [3B][H][W][1]
  Tn d_act[11];                    // post-ReLU activations [3B]
  Tn d_pool[11];                   // pooled outputs (pool layers only)
  Tn d_dz[11];                     // gradient at the conv output (after ReLU mask)
  Tn d_dpool[11];                  // gradient wrt pooled tensor (raw)
  Tn d_ufull;                      // u-forward scratch for pooled layers [B]
  float *d_t9 = nullptr, *d_out = nullptr;  // [3B][hw], [3B]
  float* g0 = nullptr;             // [2B][H][W][1] image gradients
  float* coefs = nullptr;          // [4] per-group upstream coefficients
  float *norms = nullptr, *gp = nullptr;

  // ---- data parallelism + deferred scalars ----
  depgan_allreduce_fn ar_fn = nullptr;   // all-reduce (sum) hook, enqueued on the stream (include/depgan.h)
  void* ar_user = nullptr;
  int world = 1;
  void* rccl_comm = nullptr;       // ncclComm_t of the direct binding (depgan_rccl_init); takes precedence over ar_fn
  long rccl_issued = 0;
  int device = 0;                  // HIP device the context was created on
  bool winograd = true;           // 3x3 convolutions on the Winograd F(2x2,3x3) kernel where it covers them (DEPGAN_WINOGRAD=0: direct)
  bool head_fused = true;         // gen_segmentation in gen_17's epilogue where the kernel allows (DEPGAN_HEAD_FUSED=0: own launch)
  bool wgrad_bf16 = true;          // bf16_mfma contexts: weight gradients on the bf16 pipe (DEPGAN_WGRAD_BF16=0: fp32)
  float* host_stats = nullptr;     // pinned: un-normalised loss pieces of the updates of one call, fetched asynchronously
  int* best_dev = nullptr;         // arg-min of the best-of-k search (device) and its pinned host copy
  int* best_host = nullptr;
  float* z_best = nullptr;         // [B][32] the chosen noise, gathered on the device

  // ---- shared scratch ----
  float* part = nullptr;           // wgrad slabs
  size_t partFloats = 0;
  float* raw = nullptr;            // dWraw scratch (largest kernel)
  float* Sraw = nullptr;           // [256] raw column sums
  float* scratch = nullptr;        // reductions
  size_t scratchFloats = 0;
  float* scal = nullptr;           // device scalars
  float* scal_multi = nullptr;     // 8 floats per evaluation of depgan_g_eval_multi
  float* fake_y2 = nullptr;        // [B*H*W]
  float last_sums[8];

  // ---- inference context (bf16_mfma = 1 with nc_out >= 2): the DEP-UResNet in learning phase 0 on the bf16 pipe ----
  // predict-only: generator arena, BN affines, noise MLP, forward panels and the fp32 forward activations; no critics, no
  // gradient tensors, no backward panels, no phase-1 buffers, no weight-gradient slab.  Every training entry refuses it
  // (infer_refuse) before any launch
  bool infer_only = false;

  // ---- learning-phase-1 path (nc_out >= 2, not the inference context) ----
  bool train_bn = false;
  unsigned last_drop_seed = 0;
  Tn draw_tmp;                     // gradient at the raw conv output (largest layer)
  float *logits = nullptr, *dz = nullptr, *loss_dev = nullptr;
  // the supervised loss as the depgan_uresnet_set_* entries left it (everything off by default): the census, the
  // loss-weight mode and the focal mode in ce (train_ops.h states each), the soft Dice loss beside it
  struct {
    DgCeSetting ce;
    DgDiceSetting dice;
    DgBoundarySetting boundary;
  } loss;
  // the boundary mode's buffers, allocated when the mode is first set and never inside a step: phi (batch, H, W, nc_out),
  // the row pass's 16-bit maps and the loss pass's block partials
  float* bl_phi = nullptr;
  void* bl_rows = nullptr;
  size_t bl_rows_bytes = 0;
  double* bl_part = nullptr;
  // what came back with the loss of the last depgan_uresnet_* call made under that setting: the census table (row =
  // true class, row-major nc_out x nc_out), the label pre-pass counts of the weighted path ([0] den, [1] ignored, [2]
  // out of range, [3 + k] class k), and the Dice sums I_k, P_k, T_k (3 nc_out, packed) with the Dice term.  Cleared:
  // census_valid when the census is switched off; counts_valid and dice_valid when their mode is set anew or switched
  // off, counts_valid also by every depgan_uresnet_set_focal
  struct {
    bool census_valid = false, counts_valid = false, dice_valid = false;
    long long census[DEPGAN_MAX_HEAD_CLASSES * DEPGAN_MAX_HEAD_CLASSES];
    long long counts[DEPGAN_LABEL_NCOUNT];
    double dice_sums[3 * DEPGAN_MAX_HEAD_CLASSES];
    float dice_loss = 0.f;
    // the boundary mode: L_B and M of the last call made with it on; cleared when the mode is set anew or switched off
    bool boundary_valid = false;
    double boundary_loss = 0.0, boundary_M = 0.0;
  } last;
  float *ones1k = nullptr, *zeros1k = nullptr;
  float *n_mean0 = nullptr, *n_rstd0 = nullptr, *n_mean1 = nullptr, *n_rstd1 = nullptr, *n_meanh = nullptr,
        *n_rstdh = nullptr;
  float *n_dl = nullptr, *n_dflat = nullptr, *n_dl1 = nullptr, *n_da0 = nullptr, *n_dl0 = nullptr;

  // ---- parity-test surface (depgan_debug_capture / depgan_debug_tensor) ----
  bool dbg_capture = false;
  float* dbg_mixed[11] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool dbg_mixed_valid = false;

  // ---- bf16 activation storage of the generator forward (model_bf16s.hip; bf16_mfma contexts) ----
  // GLayer::hin / hout, one view per generator layer, allocated by the first depgan_g_forward_bf16s and freed with the
  // context; the fp32 set above is not touched by that path
  bool h_ready = false, h_valid = false;
  // depgan_set_fwd_only_storage(1): the forward-only generator passes of the training closures (critic updates,
  // netG_no_update) run on that forward and write c->attr; the generator update keeps fp32 storage
  bool fwd_only_bf16 = false;
  bool bf16s_head_fused = true;    // those passes: gen_segmentation in gen_17's epilogue (DEPGAN_BF16S_HEAD_FUSED=0: own launch)
  bool h_17_skipped = false;       // the last bf16-storage pass did not store gen_17 (fused head, no debug capture)
  // depgan_set_g_update_storage(1): the generator update runs on the bf16-storage forward too and its backward reads the
  // bf16 buffers (model_bf16s_train.hip).  Per FiLM layer the pre-FiLM tensor as bf16 and the decision bits the forward
  // stored (GLayer::hu / hdec); allocated by the first update in the mode, valid after a training forward in the mode
  bool g_update_bf16 = false;
  bool hu_ready = false, hu_valid = false;

  // depgan_set_critic16_pipe(1): the critics' 16-channel 5x5 launches on igemm_bf16_n16_kernel (DLayer::pf16 / pb16)
  bool critic16_bf16 = false;

  // ---- profiling ----
  bool prof_on = false;
  std::vector<ProfRec> recs;
};

struct ProfScope {
  depgan_ctx* c;
  bool live;
  ProfScope(depgan_ctx* c_, int klass, double flops, const char* label = "", double bytes = 0.0,
            const char* kernel = "")
      : c(c_), live(c_ && c_->prof_on) {
    if (!live) return;
    ProfRec r;
    r.klass = klass;
    r.flops = flops;
    r.bytes = bytes;
    strncpy(r.label, label, sizeof(r.label) - 1);
    r.label[sizeof(r.label) - 1] = 0;
    strncpy(r.kernel, kernel, sizeof(r.kernel) - 1);
    r.kernel[sizeof(r.kernel) - 1] = 0;
    hipEventCreate(&r.a);
    hipEventCreate(&r.b);
    hipEventRecord(r.a, c->st);
    c->recs.push_back(r);
  }
  ~ProfScope() {
    if (live) hipEventRecord(c->recs.back().b, c->st);
  }
};

// helpers shared between model.hip and uresnet.hip
// zero-filled device memory of the context's lifetime (depgan_destroy frees it), sized in bytes.  The status of the
// hipMalloc or of the fill comes back unworded: dmalloc (floats) and bf16s_alloc (bf16 elements) word their own messages
hipError_t dalloc_bytes(depgan_ctx* c, void** p, size_t bytes);
// The fill of dalloc_bytes is a hipMemset on the null stream, which does not wait for the host, and the context's stream
// may be a non-blocking one that the null stream does not order itself against.  Every entry that allocates context
// memory (depgan_create and the lazy allocators) ends with this wait, once, so that on its return every fill and table
// upload is complete on the device whatever stream the first kernel or the caller's upload runs on.
int dalloc_fills_done();
int dmalloc(depgan_ctx* c, float** p, size_t floats);
// A device temporary of ONE call (never a context's: those go through c->allocs).  alloc reports failure as a status and
// frees nothing; the destructor waits for the stream the work went to and frees, so every return after alloc is covered
struct DevTmp {
  hipStream_t st;
  void* p = nullptr;
  explicit DevTmp(hipStream_t st_) : st(st_) {}
  DevTmp(const DevTmp&) = delete;
  DevTmp& operator=(const DevTmp&) = delete;
  ~DevTmp() {
    if (!p) return;
    hipStreamSynchronize(st);
    hipFree(p);
  }
  int alloc(size_t bytes) {
    HIPCHECK(hipMalloc(&p, bytes));
    return DG_OK;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};
int talloc(depgan_ctx* c, Tn* t, int N, int H, int W, int C);
int conv_launch(depgan_ctx* c, const ConvPlan& pl, const ConvArgs& a, int KS);
void zero_ep(Epilogue* e);
// a launch description with nothing but its views and sizes: every other field zero, a null-view epilogue
static inline ConvArgs conv_args(TView in, TView out, int B, int H, int W, int Cin, int Cout) {
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  zero_ep(&a.ep);
  a.in = in;
  a.out = out;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  return a;
}
static inline ConvArgsH conv_args_h(TViewH in, TViewH out, int B, int H, int W, int Cin, int Cout) {
  ConvArgsH a;
  memset(&a, 0, sizeof(a));
  a.in = in;
  a.out = out;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  return a;
}
// the weights of a launch of the (KS, KS, Cin, Cout) layer `raw_hwio`: the packed panel where the plan is an MFMA plan,
// else the raw tensor behind the direct kernel's strides.  conv_set_weights in the forward roles (K = Cin, N = Cout);
// conv_set_weights_bwd transposed and flipped (backward-data: K = Cout, N = Cin)
static inline void conv_set_weights(ConvArgs* a, const ConvPlan& pl, const float* packed, const float* raw_hwio, int Cin,
                                    int Cout) {
  if (dg_plan_mfma(pl)) { a->w = packed; return; }
  a->w = raw_hwio;
  a->wsT = (long)Cin * Cout; a->wsI = Cout; a->wsO = 1; a->flip = 0;
}
static inline void conv_set_weights_bwd(ConvArgs* a, const ConvPlan& pl, const float* packed, const float* raw_hwio,
                                        int Cin, int Cout) {
  if (dg_plan_mfma(pl)) { a->w = packed; return; }
  a->w = raw_hwio;
  a->wsT = (long)Cin * Cout; a->wsI = 1; a->wsO = Cout; a->flip = 1;
}
// WgradArgs / WgradArgsH (activation operand in bf16 memory) with no column sums
template <typename A, typename X>
static inline A wgrad_args_of(X x, TView dy, float* part, int B, int H, int W, int Cin, int Cout) {
  A a;
  a.x = x;
  a.dy = dy;
  a.part = part;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  a.nTiles = a.tilesPerChunk = 0;
  a.colpart = nullptr;
  a.colB = 0;
  return a;
}
TView view_offset(TView v, long samples);
// pixel grid (2i + di, 2j + dj) of a (2H, 2W) view (TView or TViewH)
template <typename V>
static inline V strided2(V v, int di, int dj) {
  v.p += di * v.sY + dj * v.sX;
  v.sY *= 2;
  v.sX *= 2;
  return v;
}
// 2x2 / stride-2 transposed convolution = four 1x1 convolutions of the same input, tap (di, dj) = panels[2 di + dj]
// writing the pixel grid (2i + di, 2j + dj) of the (2H, 2W) view out2: one grouped launch (ConvArgs or ConvArgsH)
template <typename A, typename V>
static inline void deconv_groups(A* a, V out2, const float* const panels[4]) {
  a->out = strided2(out2, 0, 0);
  a->groups = 4;
  for (int t = 0; t < 4; ++t) {
    a->w_group[t] = panels[t];
    a->out_group_off[t] = strided2(out2, t / 2, t % 2).p - a->out.p;
  }
  a->w = panels[0];
}
// epilogue of generator layer L in learning phase 0 (Epilogue or EpilogueH): BN affine and ReLU; a FiLM layer also takes
// its mul / add columns of the noise heads (rows of 1024) and adds `res`, its own input
template <typename E, typename V>
static inline void g_layer_epilogue(E* e, const GLayer& L, const float* heads, V res) {
  e->bias = L.b; e->scale = L.s; e->shift = L.t; e->relu = 1;
  if (L.kind != G_FILM) return;
  e->film_mul = heads + L.col_mul;
  e->film_add = heads + L.col_add;
  e->film_ld = 1024;
  e->res = res;
}
// layer i + 1 is the 2x2 max-pool of layer i (gen_1 / gen_3 / gen_5, GT:409/422/435) and H, W are even: the pool can
// ride in the epilogue of layer i's launch
static inline bool g_pool_follows(const std::vector<GLayer>& gl, size_t i) {
  return i + 1 < gl.size() && gl[i + 1].kind == G_POOL && gl[i + 1].skip_of == (int)i && !((gl[i].H | gl[i].W) & 1);
}
// backward-data of a 2x2 / stride-2 transposed convolution as ONE 1x1 convolution (dIn[p] = sum_t W_t^T dOut[2p + t]):
// fills a->in, Cin, cpt and in_run_off so that the K axis gathers the four strided pixel grids of the upstream gradient
// d, Cout channels each, in chunks of CK
void deconv_gather_k(ConvArgs* a, TView d, int Cout, int CK);
// views of the single-operator entries (depgan_op_*): NHWC, strides in elements, channel stride 1
static inline TView op_view(const float* p, long sB, long sY, long sX) {
  TView v;
  v.p = const_cast<float*>(p);
  v.sB = sB; v.sY = sY; v.sX = sX;
  return v;
}
static inline TView op_view_or_null(const float* p, long sB, long sY, long sX) {
  return p ? op_view(p, sB, sY, sX) : null_view();
}
static inline TViewH op_view_h(const void* p, long sB, long sY, long sX) {
  TViewH v;
  v.p = reinterpret_cast<__bf16*>(const_cast<void*>(p));
  v.sB = sB; v.sY = sY; v.sX = sX;
  return v;
}
static inline TViewH op_view_h_or_null(const void* p, long sB, long sY, long sX) {
  return p ? op_view_h(p, sB, sY, sX) : null_view_h();
}
// what the operator entries refuse as a view.  The two meanings differ on purpose: the fp32 entries (op_entries.hip) want
// a batch stride; the bf16-storage entries (op_entries_bf16s.hip) also take sB = 0, one sample read by every batch index
static inline bool op_view_bad_batched(const void* p, long sB, long sY, long sX) { return !p || sB < 1 || sY < 1 || sX < 1; }
static inline bool op_view_bad_broadcast(const void* p, long sB, long sY, long sX) { return !p || sB < 0 || sY < 1 || sX < 1; }
// upload and run pack jobs whose destinations interleave (GLayer::wpb_all); synchronises: `jobs` is the caller's
int op_pack_jobs(PackJob* jobs, int n, hipStream_t st);
int deconv_bwd_data(depgan_ctx* c, GLayer& L, TView dsrc, int n);
// weight gradient (four taps) + column sums of the upstream gradient of a transposed convolution whose input is the
// view x (XV = TView: L.in; TViewH: L.hin, the bf16 activation storage)
template <typename XV>
int deconv_wgrad_all(depgan_ctx* c, const GLayer& L, XV x, TView dsrc, int n, const float* scale, float* raw,
                     const float* colscale, float* colout, float* colraw);
// forward of a transposed convolution on the fused four-tap kernel (deconv_fwd.hip) where it covers the layer
bool deconv_fused(const depgan_ctx* c, const GLayer& L, int n);
int deconv_fwd_launch(depgan_ctx* c, const GLayer& L, TView out, const float* bias, const float* scale,
                      const float* shift, int relu, int n);
// column sums of dy over its first B samples, delivered with the weight gradient: out = scale * sum, raw = sum
struct ColSum {
  int B;
  const float* scale;
  float *out, *raw;
};
// the workspaces of one weight gradient are the caller's: the context's own in the model, a call's own in the
// depgan_op_conv2d_wgrad* entries
struct WgradWs {
  float* part;           // slabs
  size_t partFloats;
  float* scratch;        // partial column-sum rows ([col_rows][Cout]) or the scratch of the streaming column-sum pass
  size_t scratchFloats;
  bool bf16;             // contraction on the bf16 matrix pipe where wgrad_bf16.hip covers the shape
  hipStream_t st;
  depgan_ctx* prof;      // profile records go to this context; null: none
};
// THE weight-gradient driver, the only code that launches a slab kernel and its finish: the kernel dg_wgrad_choose names
// for the shape, ws.bf16 and the storage of x (XV = TView: fp32; TViewH: bf16), the capacity checks (status 1 before any
// launch), the streaming column-sum pass where the kernel has no column rows, the launch, the finish
template <typename XV>
int wgrad_run(const WgradWs& ws, int KS, XV x, TView dy, int N, int H, int W, int Cin, int Cout, const float* scale,
              float* out, float* raw, int accumulate, int oi, const ColSum* cs);
// ... on the context's workspaces and stream, with its profile records
template <typename XV>
static inline int wgrad_full(depgan_ctx* c, int KS, XV x, TView dy, int N, int H, int W, int Cin, int Cout,
                             const float* scale, float* out, float* raw, int accumulate, int oi,
                             const ColSum* cs = nullptr) {
  const WgradWs ws = {c->part, c->partFloats, c->scratch, c->scratchFloats, c->cfg.bf16_mfma && c->wgrad_bf16, c->st, c};
  return wgrad_run(ws, KS, x, dy, N, H, W, Cin, Cout, scale, out, raw, accumulate, oi, cs);
}
// ... of an operator entry, after its own argument checks: DevTmp workspaces of the call, sized from the choice
template <typename XV>
int op_wgrad(const char* who, int KS, XV x, TView dy, int B, int H, int W, int Cin, int Cout, bool bf16,
             const float* scale, float* dw, float* raw, int accumulate, int oi, const ColSum* cs, hipStream_t st);
int net_adam(depgan_ctx* c, Net& n, float gscale = 1.0f);
int g_forward(depgan_ctx* c, const float* x, const float* z, int n, bool store_u);
// model_bf16s.hip.  bf16s_check_ctx: what the context must be for the bf16-storage forward (no HIP call);
// g_forward_bf16s: fused_head = gen_segmentation in gen_17's epilogue, and then gen_17 is stored only if keep_17;
// g_forward_only: the generator pass of a closure that keeps nothing for a backward pass, batch samples into c->attr,
// on the storage depgan_set_fwd_only_storage chose
int bf16s_check_ctx(const depgan_ctx* c, const char* who, bool softmax_head = false);
// DG_ERR_UNSUPPORTED with a text that names the inference context where c is one (no HIP call); DG_OK otherwise
int infer_refuse(const depgan_ctx* c, const char* who);
int bf16s_alloc(depgan_ctx* c);
int g_forward_bf16s(depgan_ctx* c, const float* x, const float* z, float* out, int n, bool fused_head, bool keep_17,
                    bool train = false);
int g_forward_only(depgan_ctx* c, const float* x, const float* z);
// model_bf16s_train.hip: the generator update on bf16 activation storage.  g_forward_train_bf16s: batch samples into
// c->attr, additionally keeping u and the FiLM decisions; g_backward_bf16s: g_backward over the same layer table, gradient
// arena and raw_all slots, reading the bf16 buffers; g_backward_finish (model.hip): the BN-gamma launch and the noise MLP
int bf16s_train_alloc(depgan_ctx* c);
int bf16s_debug_u(depgan_ctx* c, const char* name, float* host, long cap, int shape[4]);
// the tail of depgan_debug_tensor_bf16s (model_bf16s.hip): shape of the (batch, H, W, C) bf16 view v and, where host is
// given, its dense fp32 copy
int bf16s_debug_copy(depgan_ctx* c, const char* name, TViewH v, int H, int W, int C, float* host, long cap, int shape[4]);
int g_forward_train_bf16s(depgan_ctx* c, const float* x, const float* z);
int g_backward_bf16s(depgan_ctx* c, const float* x, const float* z, int n);
int g_backward_finish(depgan_ctx* c, const float* z, int n);
int refresh_generator(depgan_ctx* c);
int refresh_generator_bn(depgan_ctx* c);  // phase-0 BN affines only (after the moving statistics moved)
int uresnet_build(depgan_ctx* c);
int uresnet_predict(depgan_ctx* c, const float* x, const float* z, float* out, int n);
