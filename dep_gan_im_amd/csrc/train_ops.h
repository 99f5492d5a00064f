// Operators only the learning-phase-1 path needs (DEP-UResNet `fit`):
// batch-statistics BatchNorm forward / backward, Dropout, softmax + categorical cross-entropy.
#pragma once
#include "common.h"
#include "../../include/depgan.h"

// per-channel batch mean and biased variance of an NHWC view (one pass, shifted sums; C % 4 == 0, C <= 1024).
// scratch: dg_col_moments_scratch(B, H, W, C) floats (at most 3 * 1024 * C); DG_ERR_ARG when scratch_floats is less
int dg_col_moments(TView v, int B, int H, int W, int C, float* mean, float* var, float* scratch, size_t scratch_floats,
                   hipStream_t st);
size_t dg_col_moments_scratch(int B, int H, int W, int C);
// sums[0..C) = sum_p d[p][c] ; sums[C..2C) = sum_p d[p][c] * (x[p][c] - mean[c])
// scratch: dg_colsum_pair_scratch(B, H, W, C) floats (at most 2 * 1024 * C); DG_ERR_ARG when scratch_floats is less
int dg_colsum_pair(TView d, TView x, const float* mean, int B, int H, int W, int C, float* sums, float* scratch,
                   size_t scratch_floats, hipStream_t st);
size_t dg_colsum_pair_scratch(int B, int H, int W, int C);

// training-mode BN bookkeeping for one layer: s = gamma*rsqrt(var+eps), t = beta - mean*s, rstd;
// moving_mean/var <- momentum*moving + (1-momentum)*(mean, var*corr)       
int dg_bn_train_prepare(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                        float momentum, float corr, float* moving_mean, float* moving_var, float* s, float* t,
                        float* rstd, int C, hipStream_t st);

// y = act( film( x*s[c] + t[c] ) ) + res, optional pre-FiLM copy, optional dropout (hash RNG shared with the oracle)
struct AffineActArgs {
  TView in, out, out_pre, res;
  const float *s, *t, *film_mul, *film_add;
  int film_ld, relu;
  int B, H, W, C;
  unsigned drop_seed;   // 0 = no dropout
  float drop_rate;
};
int dg_affine_act(const AffineActArgs& a, hipStream_t st);

// BN backward coefficients from sums = [sum dy, sum dy*(raw-mean)]:
//   dbeta = sum dy ; dgamma = rstd * sum dy*(raw-mean)
//   draw = A*dy + Bc*raw + Cc with A = s, Bc = -s*rstd^2*dgamma'/N ... (see train_ops.hip)
// dyscale: constant still to be applied to dy (dropout's 1/(1-rate) on the kept elements)
int dg_bn_bwd_coeffs(const float* sums, const float* mean, const float* rstd, const float* s, float invN,
                     float dyscale, float* dgamma, float* dbeta, float* coefA, float* coefB, float* coefC, int C, hipStream_t st);
// out[p][c] = A[c]*d[p][c] + Bc[c]*x[p][c] + Cc[c]
int dg_axpby_ch(TView d, TView x, TView out, int B, int H, int W, int C, const float* A, const float* Bc,
                const float* Cc, hipStream_t st);

// ---- the supervised loss (softmax_ce.hip, dice_loss.hip) ----
// the labels of one call: a float32 one-hot row per pixel (onehot) or one class code per pixel (codes), never both
struct DgLabels {
  const float* onehot;
  const unsigned char* codes;
};
// The cross-entropy setting, on the host.  census: also count (true class, predicted class) pairs.  weighted: the
// loss-weight mode -- cw: C class weights, finite and >= 0 with at least one > 0; ignore: -1 for none, else a byte value
// whose pixels have t = 0 and are not counted as out of range (read with codes only: with one-hot labels the ignored
// pixel is the all-zero row).  focal: the focal mode (include/depgan.h, depgan_uresnet_set_focal, states the rule) with
// gamma finite and >= 0 and label smoothing eps in [0, 1); it runs the weighted path, with unit weights and no ignore
// code unless weighted is on too.  gamma = 0 with eps = 0 is allowed and runs the focal statements.
struct DgCeSetting {
  bool census = false, weighted = false, focal = false;
  float cw[DEPGAN_MAX_HEAD_CLASSES];
  int ignore = -1;
  float gamma = 0.f, eps = 0.f;
  bool weighted_path() const { return weighted || focal; }   // the label pre-pass runs and leaves counts
  // the loss-weight mode on: C weights (null: unit weights) and the ignore code
  void set_weights(const float* w, int C, int ignore_code) {
    for (int k = 0; k < C; ++k) cw[k] = w ? w[k] : 1.0f;
    ignore = ignore_code;
    weighted = true;
  }
};
// What a labelled launch leaves on the device beside probs and dz, as the host reads it: the summed loss (entries that
// take a loss_sum of their own leave the slot unused), bad = the codes >= C that are not the ignore code (0 with
// onehot), census[tc * C + pc] = the pixels of true class tc predicted as pc, and the label pre-pass counts: [0] den =
// the pixels with weight w = sum_k cw[k] t[k] != 0, [1] the pixels without a true class (the ignore code, an all-zero
// one-hot row), [2] the codes >= C that are not the ignore code, [3 + k] the pixels of true class k (the code, or the
// first arg-max of the row).  pc = the first index of the maximum of the stored probability row (np.argmax of probs);
// tc = the code, or the first arg-max of the one-hot row (an all-zero row is class 0; on the weighted path it joins no
// bin).  A pixel whose code is >= C is in no bin: sum(census) + bad + (weighted path: pixels without a true class) == P.
struct DgCeDev {
  float loss;
  unsigned bad;
  unsigned long long census[DEPGAN_MAX_HEAD_CLASSES * DEPGAN_MAX_HEAD_CLASSES];
  unsigned long long counts[DEPGAN_LABEL_NCOUNT];
  // the leading bytes a launch under s writes: what a copy back to the host takes
  static size_t bytes(int C, const DgCeSetting& s) {
    if (s.weighted_path()) return offsetof(DgCeDev, counts) + (size_t)(C + 3) * sizeof(long long);
    return offsetof(DgCeDev, census) + (s.census ? (size_t)C * C : 0) * sizeof(long long);
  }
};
// softmax + keras categorical cross-entropy on dense (P, C) logits, C = 2..8: probs out; with labels also dz =
// dLoss/dlogits (loss = mean over pixels) and loss_sum[0] = sum over pixels of the per-pixel loss.  Without labels:
// probabilities only -- nothing else is written, no scratch is needed and every setting is off.  bad_count: required
// with codes, with a census and on the weighted path, else optional.  census (C*C counts) with set.census, counts
// (C + 3) with set.weighted_path(), both 8-byte aligned.  On the weighted path the label pre-pass runs first and the
// loss runs on the label row cw[k] t[k] with 1 / den for 1 / P (0 for den = 0), den read on the device from counts[0];
// loss_sum[0] = the weighted sum, the mean is loss_sum / den; with unit weights and nothing ignored every output has
// the plain path's bits.  The scratch holds the partials of both passes in turn.  Two stages,
// no atomics, nothing to zero between calls; the pre-pass shares the scratch: dg_softmax_ce_scratch(P, C, set) floats =
// max(2048 + the census's block tables, the pre-pass's block tables), at most 2048 + 1024 C C.  Rows are accessed 16
// bytes at a time where C % 4 == 0 (16-byte aligned operands), else float by float.
struct SoftmaxCeArgs {
  const float* logits;
  DgLabels lab;
  float *probs, *dz, *loss_sum;
  unsigned* bad_count;
  unsigned long long *census, *counts;
  DgCeSetting set;
  long P;
  int C;
  float* scratch;
  size_t scratch_floats;
};
size_t dg_softmax_ce_scratch(long P, int C, const DgCeSetting& set);
// every refusal of dg_softmax_ce, without a HIP call and without reading through a pointer: DG_ERR_ARG and a message
int dg_softmax_ce_check(const char* who, const SoftmaxCeArgs& a);
int dg_softmax_ce(const SoftmaxCeArgs& a, hipStream_t st);
// dg_loss_weights_check and dg_focal_check validate a setting's values without a HIP call (n must equal C where w is
// given).  dg_label_counts: the label pre-pass alone (cw null: unit weights); dg_label_counts_scratch(P, C) floats.
int dg_loss_weights_check(const char* who, const float* w, int n, int C, int ignore_code);
int dg_focal_check(const char* who, float gamma, float label_smoothing);
size_t dg_label_counts_scratch(long P, int C);
int dg_label_counts(const float* onehot, const unsigned char* codes, long P, int C, const float* cw, int ignore_code,
                    unsigned long long* counts, float* scratch, size_t scratch_floats, hipStream_t st);

// The soft Dice loss (dice_loss.hip; include/depgan.h, depgan_uresnet_set_dice_loss, states the rule).  It runs behind the
// cross-entropy on the same stream, on the probabilities AS STORED: sums I_k = sum m t_k p_k, P_k = sum m p_k,
// T_k = sum m t_k over the pixels that take part (m), per-class scalars A_k, B_k with dL/dp_k = m (A_k t_k + B_k), and
// dz = ce_coef dz + dice_coef p_k (g_k - sum_j p_j g_j).  What the coefficient stage leaves on the device:
struct DgDiceDev {
  double sums[3 * DEPGAN_MAX_HEAD_CLASSES];   // I_0..I_{C-1}, P_0..P_{C-1}, T_0..T_{C-1} (3 C entries, packed)
  float loss, pad;                            // the Dice term, rounded once from the double result
  float A[DEPGAN_MAX_HEAD_CLASSES], B[DEPGAN_MAX_HEAD_CLASSES];
};
// The Dice setting, on the host: form DEPGAN_DICE_OFF / _FLAT / _CLASS, ce_coef finite >= 0, dice_coef and smooth finite
// > 0, c: the class form's C coefficients (finite, >= 0, at least one > 0).
struct DgDiceSetting {
  int form = DEPGAN_DICE_OFF;
  float ce_coef = 1.f, dice_coef = 1.f, smooth = 0.f;
  float c[DEPGAN_MAX_HEAD_CLASSES];
  // coef null: 1 / C each
  void set(int form_, float ce, float dice, float smooth_, const float* coef, int C) {
    form = form_, ce_coef = ce, dice_coef = dice, smooth = smooth_;
    for (int k = 0; k < C; ++k) c[k] = coef ? coef[k] : 1.0f / (float)C;
  }
};
// dg_dice_check validates the values of a setting without a HIP call: coef null or (class form only) n == C values.
// dg_dice_loss: ignore_code: -1 = every pixel takes part; with codes the pixels of that code stay out (a code >= C
// always does), with onehot any value >= 0 keeps the all-zero rows out.  dz null: the sums, the coefficients and the
// loss only (no gradient pass).  ce_coef == 0: dz is written without being read.  Two-stage sums, no atomics, the
// partials added in index order in double; dg_dice_scratch(P, C) floats of scratch (at most 1024 * 3 C).
int dg_dice_check(const char* who, int form, float ce_coef, float dice_coef, float smooth, const float* coef, int n,
                  int C);
// What the losses behind the cross-entropy share, each without a HIP call: C in DG_MIN_CLASSES..DG_MAX_CLASSES; n == C
// class coefficients, each finite and >= 0, at least one > 0; and the operands' checks alone, what an entry asks before
// it allocates -- probs, the labels, the ignore code, P >= 1 (p_below_2_31: and < 2^31), one more operand where
// extra_name names it (the boundary loss's phi), and the alignment of every row pointer for C classes.
int dg_class_count_check(const char* who, int C);
int dg_class_coef_check(const char* who, const float* coef, int n, int C);
int dg_loss_operands_check(const char* who, const float* probs, const char* extra_name, const float* extra, DgLabels lab,
                           int ignore_code, const float* dz, long P, bool p_below_2_31, int C);
size_t dg_dice_scratch(long P, int C);
int dg_dice_loss(const float* probs, DgLabels lab, int ignore_code, const DgDiceSetting& set, float* dz, DgDiceDev* out,
                 long P, int C, float* scratch, size_t scratch_floats, hipStream_t st);

// The boundary loss (boundary_loss.hip; include/depgan.h, depgan_uresnet_set_boundary_loss, states the rule).  It runs
// behind the cross-entropy and the Dice mode on the same stream: the signed distance maps of the call's labels, then one
// pass over the stored probabilities that adds its gradient to dz.  The setting, on the host: c: C class coefficients
// (finite, >= 0, at least one > 0; a class with c_k == 0 gets no map), coef = boundary_coef finite >= 0, the spacings
// finite > 0 and inside_offset in [0, min(sy, sx)].
struct DgBoundarySetting {
  bool on = false;
  float coef = 1.f;
  float c[DEPGAN_MAX_HEAD_CLASSES];
  double sy = 1.0, sx = 1.0, inside_offset = 0.0;
  unsigned class_mask(int C) const {
    unsigned m = 0;
    for (int k = 0; k < C; ++k) m |= (c[k] != 0.f ? 1u : 0u) << k;
    return m;
  }
};
// what the finish stage leaves on the device: L_B = sum / M (0.0 for M = 0) and M, the pixels that take part
struct DgBoundaryDev {
  double loss, M;
};
// the values of a setting, without a HIP call: coef null or n == C values
int dg_boundary_check(const char* who, float boundary_coef, const float* coef, int n, int C);
// the geometry of a signed distance call, without a HIP call: n >= 1, H and W within edt.h's limit, n H W < 2^31, n H
// and the 64 x 16 tiles of all n C maps each < 2^24 (the two grids), C in 2..8
int dg_signed_distance_check(const char* who, long n, int H, int W, int C, double sy, double sx, double inside_offset);
// phi (n, H, W, C) float32 of n label slices: the classes of class_mask get their map, the others 0.  ignore_code as
// dg_dice_loss takes it.  Two launches whatever n; dg_signed_distance_scratch_bytes(n, H, W, classes) of scratch, where
// `classes` is at least the number of bits set in class_mask (2-byte aligned).
size_t dg_signed_distance_scratch_bytes(long n, int H, int W, int C);
int dg_signed_distance(DgLabels lab, int ignore_code, long n, int H, int W, int C, unsigned class_mask, double sy,
                       double sx, double inside_offset, float* phi, void* scratch, size_t scratch_bytes, hipStream_t st);
// L_B and, with dz, dz += boundary_coef p (g - sum p g).  counts: null for M = P, else the label pre-pass counts
// (DgCeDev::counts) on the device, M = P - counts[1] - counts[2].  dg_boundary_scratch(P) doubles of scratch (at most
// 1024), 8-byte aligned.  One partial per block, added in index order by one block: no atomics, nothing to zero.
size_t dg_boundary_scratch(long P);
int dg_boundary_loss(const float* probs, const float* phi, DgLabels lab, int ignore_code, const float* class_coef,
                     float boundary_coef, const unsigned long long* counts, float* dz, DgBoundaryDev* out, long P, int C,
                     double* scratch, size_t scratch_doubles, hipStream_t st);

// the 1x1 head to K = 2..8 class logits on dense (P, K) rows; a, mask and din are pixel rows of C channels at strides
// ld* (multiples of 4 floats, 16-byte aligned), w is (C, K) dense, C / 4 a power of two <= 64
int dg_head_k_fwd(const float* a, long ld, const float* w, const float* b, float* logits, long P, int C, int K,
                  hipStream_t st);
// din[p][c] = (mask[p][c] > 0 or no mask) ? sum_k dz[p][k] w[c][k] : 0
int dg_head_k_bwd(const float* dz, const float* w, const float* mask, long ldm, float* din, long ldd, long P, int C,
                  int K, hipStream_t st);
// dW[c][k] = sum_p a[p][c] dz[p][k], db[k] = sum_p dz[p][k]; two fixed-order stages through
// dg_head_k_wgrad_scratch(P, C, K) floats of scratch (at most 1024 (C K + K)); DG_ERR_ARG when scratch_floats is less
int dg_head_k_wgrad(const float* a, long lda, const float* dz, float* dW, float* db, long P, int C, int K,
                    float* scratch, size_t scratch_floats, hipStream_t st);
size_t dg_head_k_wgrad_scratch(long P, int C, int K);

// ---- noise MLP in training mode: BN over the rows of small [R][C] matrices ----
// y = relu?( gamma*(x-mean)*rstd + beta ), stats over the R rows; also updates the moving stats
int dg_bn_rows_fwd(const float* x, float* y, int R, int C, int ld, const float* gamma, const float* beta, float eps,
                   float momentum, float corr, float* moving_mean, float* moving_var, float* mean, float* rstd,
                   int relu, hipStream_t st);
// dx, dgamma, dbeta from dy (after the ReLU mask of y when relu_out != null)
int dg_bn_rows_bwd(const float* dy, const float* x, const float* relu_out, float* dx, int R, int C, int ld,
                   const float* gamma, const float* mean, const float* rstd, float* dgamma, float* dbeta,
                   hipStream_t st);
// small dense helpers: C[M][N] = A[M][K] @ B[K][N] (+bias) ; At: C[K][N] = A[M][K]^T @ D[M][N] ; Bt: C[M][K] = D[M][N] @ B[K][N]^T
int dg_small_gemm(const float* A, const float* Bm, const float* bias, float* Cm, int M, int K, int N, hipStream_t st);
int dg_small_gemm_at(const float* A, const float* D, float* Cm, int M, int K, int N, hipStream_t st);
int dg_small_gemm_bt(const float* D, const float* Bm, float* Cm, int M, int K, int N, hipStream_t st);
int dg_colsum_small(const float* x, float* out, int R, int C, int ld, hipStream_t st);
