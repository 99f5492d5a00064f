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

// softmax + keras categorical cross-entropy on dense (P, C) logits, C = 2..8: probs out; with labels also
// dz = dLoss/dlogits (loss = mean over pixels) and loss_sum[0] = sum over pixels of the per-pixel loss.  Labels are a
// float32 one-hot row (onehot) or one class code per pixel (codes), never both; neither: probabilities only.  With
// codes, bad_count[0] receives the number of pixels whose code is >= C (they add no loss and no gradient); with onehot
// it receives 0 where it is given.  scratch: 2048 floats (unused without labels).  Rows are accessed 16 bytes at a time
// where C % 4 == 0 (16-byte aligned operands), else float by float.
int dg_softmax_ce(const float* logits, const float* onehot, const unsigned char* codes, float* probs, float* dz,
                  float* loss_sum, unsigned* bad_count, long P, int C, float* scratch, hipStream_t st);
// dg_softmax_ce with labels plus the class census of the same pass: census[tc * C + pc] (C*C 64-bit device counts,
// 8-byte aligned) = the pixels of true class tc predicted as pc.  pc = the first index of the maximum of the stored
// probability row (k = 0..C-1, strict >: np.argmax of probs); tc = the code, or the first index of the maximum of the
// one-hot row (an all-zero row is class 0).  A pixel whose code is >= C is in no bin: sum(census) + bad_count == P.
// probs, dz and loss_sum have the bits dg_softmax_ce gives.  Two stages, no atomics, nothing to zero between calls; the
// block tables follow the 2048 floats of the other partials: dg_softmax_ce_census_scratch(P, C) floats of scratch
// (at most 2048 + 1024 C C), DG_ERR_ARG when scratch_floats is less.  bad_count is required (0 with onehot).
size_t dg_softmax_ce_census_scratch(long P, int C);
int dg_softmax_ce_census(const float* logits, const float* onehot, const unsigned char* codes, float* probs, float* dz,
                         float* loss_sum, unsigned* bad_count, unsigned long long* census, long P, int C, float* scratch,
                         size_t scratch_floats, hipStream_t st);
// The loss-weight mode.  cw: C host class weights, finite and >= 0 with at least one > 0 (null: unit weights);
// ignore_code: -1 for none, else a byte value whose pixels have t = 0 and are not counted as out of range (read with
// codes only: with one-hot labels the ignored pixel is the all-zero row).
// dg_loss_weights_check validates both without a HIP call (n must equal C where w is given).
// dg_label_counts: the label pre-pass alone.  counts (C + 3 64-bit device counts, 8-byte aligned) receives
// [0] den = the pixels with weight w = sum_k cw[k] t[k] != 0, [1] the pixels without a true class (the ignore code, an
// all-zero one-hot row), [2] the codes >= C that are not the ignore code, [3 + k] the pixels of true class k (the code,
// or the first arg-max of the row).  Two stages, no atomics, nothing to zero; dg_label_counts_scratch(P, C) floats.
// dg_softmax_ce_weighted: that pass, then dg_softmax_ce (census == null) or dg_softmax_ce_census on the label row
// cw[k] t[k] with 1 / den for 1 / P (0 for den = 0), den read on the device from counts[0]; loss_sum[0] = the weighted
// sum, the mean is loss_sum / den.  Under it a pixel without a true class joins no census bin.  With unit weights and
// nothing ignored every output has dg_softmax_ce's bits.  dg_softmax_ce_weighted_scratch(P, C, census) floats.
int dg_loss_weights_check(const char* who, const float* w, int n, int C, int ignore_code);
size_t dg_label_counts_scratch(long P, int C);
int dg_label_counts(const float* onehot, const unsigned char* codes, long P, int C, const float* cw, int ignore_code,
                    unsigned long long* counts, float* scratch, size_t scratch_floats, hipStream_t st);
size_t dg_softmax_ce_weighted_scratch(long P, int C, bool census);
int dg_softmax_ce_weighted(const float* logits, const float* onehot, const unsigned char* codes, float* probs, float* dz,
                           float* loss_sum, unsigned* bad_count, unsigned long long* census,
                           unsigned long long* counts, const float* cw, int ignore_code, long P, int C, float* scratch,
                           size_t scratch_floats, hipStream_t st);
// The focal mode (include/depgan.h, depgan_uresnet_set_focal, states the rule): dg_softmax_ce_weighted with the focal
// cross-entropy and label smoothing in the same kernel text -- gamma finite and >= 0, label_smoothing in [0, 1)
// (dg_focal_check validates both without a HIP call).  cw null: unit weights.  The pre-pass, den, the ignore code, the
// census, the stored probabilities and the scratch (dg_softmax_ce_weighted_scratch) are the loss-weight mode's.  gamma =
// 0 with label_smoothing = 0 is allowed here and runs the focal statements; a caller that wants the plain bits calls
// dg_softmax_ce_weighted or dg_softmax_ce instead.
int dg_focal_check(const char* who, float gamma, float label_smoothing);
int dg_softmax_ce_focal(const float* logits, const float* onehot, const unsigned char* codes, float* probs, float* dz,
                        float* loss_sum, unsigned* bad_count, unsigned long long* census, unsigned long long* counts,
                        const float* cw, int ignore_code, float gamma, float label_smoothing, long P, int C,
                        float* scratch, size_t scratch_floats, hipStream_t st);
// its argument checks alone (no HIP call): what an entry asks before it allocates
int dg_softmax_ce_check(const float* logits, const float* onehot, const unsigned char* codes, const float* probs,
                        const float* dz, const float* loss_sum, long P, int C);

// The soft Dice loss (dice_loss.hip; include/depgan.h, depgan_uresnet_set_dice_loss, states the rule).  It runs behind the
// cross-entropy on the same stream, on the probabilities AS STORED: sums I_k = sum m t_k p_k, P_k = sum m p_k,
// T_k = sum m t_k over the pixels that take part (m), per-class scalars A_k, B_k with dL/dp_k = m (A_k t_k + B_k), and
// dz = ce_coef dz + dice_coef p_k (g_k - sum_j p_j g_j).  What the coefficient stage leaves on the device:
struct DgDiceDev {
  double sums[3 * DEPGAN_MAX_HEAD_CLASSES];   // I_0..I_{C-1}, P_0..P_{C-1}, T_0..T_{C-1} (3 C entries, packed)
  float loss, pad;                            // the Dice term, rounded once from the double result
  float A[DEPGAN_MAX_HEAD_CLASSES], B[DEPGAN_MAX_HEAD_CLASSES];
};
// dg_dice_check validates the setting without a HIP call: form DEPGAN_DICE_FLAT / _CLASS, ce_coef finite >= 0, dice_coef
// and smooth finite > 0, coef null or (class form only) n == C finite values >= 0 with at least one > 0.
// dg_dice_loss: coef null = 1 / C each.  ignore_code: -1 = every pixel takes part; with codes the pixels of that code
// stay out (a code >= C always does), with onehot any value >= 0 keeps the all-zero rows out.  dz null: the sums, the
// coefficients and the loss only (no gradient pass).  ce_coef == 0: dz is written without being read.  Two-stage sums,
// no atomics, the partials added in index order in double; dg_dice_scratch(P, C) floats of scratch (at most 1024 * 3 C).
int dg_dice_check(const char* who, int form, float ce_coef, float dice_coef, float smooth, const float* coef, int n,
                  int C);
// the operands' checks alone (no HIP call): what an entry asks before it allocates
int dg_dice_operands_check(const char* who, const float* probs, const float* onehot, const unsigned char* codes,
                           int ignore_code, const float* dz, long P, int C);
size_t dg_dice_scratch(long P, int C);
int dg_dice_loss(const float* probs, const float* onehot, const unsigned char* codes, int ignore_code, int form,
                 const float* coef, float smooth, float ce_coef, float dice_coef, float* dz, DgDiceDev* out, long P, int C,
                 float* scratch, size_t scratch_floats, hipStream_t st);

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
