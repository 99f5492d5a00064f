// Softmax + categorical cross-entropy of the supervised path (see train_ops.h, dg_softmax_ce): one kernel text for
// every class count, label source and loss mode, the label pre-pass of the weighted path, and the one host entry.
#include "train_ops.h"

#include <float.h>

#include "block_sum.h"
#include "labels.h"

// ---------------------------------------------------------------------------
// softmax + categorical cross-entropy (keras, probabilities path)
// ---------------------------------------------------------------------------
// One kernel for every class count C = 2..8 and every label source: LBL_ONEHOT reads a float32 one-hot row,
// LBL_CODES forms t[k] = (k == code) in registers from one byte and then runs the same statements (so the two agree
// value for value), LBL_NONE stops after the probabilities.  A code is only ever compared, never used as an index:
// any byte is safe; a code >= C gives an all-zero t (no loss, no gradient from that pixel) and is counted.
// Evaluation order (softmax_row.h): maximum and S over pairs folded left to right -- for C = 4 that is the pairwise
// max and S = (p0 + p1) + (p2 + p3); S0, the loss, dot and pg run over k = 0..C-1 left to right.
//
// CENSUS (labels present): every pixel also adds 1 to bin [tc][pc] of a C x C table, tc = the code (LBL_CODES; a code
// >= C joins no bin, it is in nbad) or the first arg-max of the label row (LBL_ONEHOT; an all-zero row is class 0),
// pc = the first arg-max of p as stored.  Integers only: no float statement reads anything the census writes, and the
// CENSUS = false instantiations compile to the instructions they were.  In a block the table is kept per wave, with no
// atomics and no LDS traffic in the loop: one ballot per true class and one per predicted class (2 C compares), then
// lane l, the owner of bin l = k * C + j, adds popcount(ballot_t[k] & ballot_p[j]) to its one counter.  The four
// waves' tables meet in LDS after the loop and C*C lanes store the block's partial.
//
// WEIGHTED (labels present; the loss-weight setting): the label row becomes cw[k] * t[k] before the statements above run
// on it, a code equal to wa.ignore gives t = 0 without being counted in nbad, and 1/N becomes 1/den, den = the count of
// pixels with a non-zero weight that label_count_kernel left in wa.den (invDen = 0 for den = 0: no division by zero, an
// all-zero dz).  With unit weights, no ignored pixel and den = P every float is the one the WEIGHTED = false
// instantiation computes (1 * t = t, and 1.0f / (float)den is the host's 1.0f / (float)P).  A pixel with t = 0 --
// ignored, or of a zero-weight class -- has a dz row of zeros and still gets its probabilities.  CENSUS under WEIGHTED:
// a pixel without a true class (the ignore code, an all-zero one-hot row) joins no bin.  The WEIGHTED = false
// instantiations ignore wa and compile to the instructions they were.
//
// FOCAL (with WEIGHTED only; the focal setting): the focal cross-entropy with label smoothing of include/depgan.h
// (depgan_uresnet_set_focal).  The label row stays unweighted until the pixel weight w = sum_k cw[k] t[k] (left to right,
// the pre-pass's statement) and has = any t[k] != 0 are formed from it; then ts[k] = w ((1 - eps) t[k] + (has ? eps / C
// : 0)) takes the row's place, the loss term is -ts[k] (1 - r)^gamma log r and dL/dq_k = -ts[k] (1/den) ((1 - r)^gamma / q
// - gamma (1 - r)^(gamma - 1) log r) on the closed clip interval.  1 - r is formed directly (>= 2^-23 inside the clip);
// the power is 1, 1 - r or (1 - r)^2 for gamma = 0, 1, 2 (a uniform branch: gamma is a kernel argument) and
// exp2f(gamma log2f(1 - r)) otherwise, (1 - r)^(gamma - 1) the power over 1 - r.  Everything behind dL/dq, the census and
// the stored probabilities are the text above.  The FOCAL = false instantiations read neither gamma nor eps, the last
// two arguments, and compile to the instructions they were.  The LBL_* values are labels.h's.

// the loss-weight mode's kernel arguments, by value: C class weights (the rest 0), the ignore code (-1: none) and the
// device count of weighted pixels
struct SmWeights {
  float cw[DG_MAX_CLASSES];
  int ignore;
  const unsigned long long* den;
};

__device__ __forceinline__ unsigned t_block_sum_u(unsigned v, unsigned* shu4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) shu4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (shu4[0] + shu4[1]) + (shu4[2] + shu4[3]);
}

// pw = x^gamma and pm1 = x^(gamma - 1) for x = 1 - r in [2^-23, 1) and gamma >= 0
__device__ __forceinline__ void t_focal_pow(float x, float gamma, float& pw, float& pm1) {
  if (gamma == 0.f) {
    pw = 1.0f;
    pm1 = 1.0f / x;     // multiplied by gamma = 0 where it is used
  } else if (gamma == 1.0f) {
    pw = x;
    pm1 = 1.0f;
  } else if (gamma == 2.0f) {
    pw = x * x;
    pm1 = x;
  } else {
    pw = exp2f(gamma * log2f(x));
    pm1 = pw / x;
  }
}

template <int C, int LBL, bool CENSUS, bool WEIGHTED, bool FOCAL>
__global__ void softmax_ce_kernel(const float* __restrict__ logits, const float* __restrict__ onehot,
                                  const unsigned char* __restrict__ codes, float* __restrict__ probs,
                                  float* __restrict__ dz, float* __restrict__ part, unsigned* __restrict__ bad_part,
                                  unsigned* __restrict__ cen_part, long P, float invN, SmWeights wa, float gamma,
                                  float eps) {
  static_assert(!CENSUS || LBL != LBL_NONE, "a census needs labels");
  static_assert(!WEIGHTED || LBL != LBL_NONE, "loss weights need labels");
  static_assert(!FOCAL || WEIGHTED, "the focal mode runs the weighted path");
  if (WEIGHTED) {
    const unsigned long long den = *wa.den;
    invN = den ? 1.0f / (float)den : 0.f;
  }
  __shared__ float sh4[4];
  __shared__ unsigned shu4[4];
  float lsum = 0.f;
  unsigned nbad = 0;
  // CENSUS: lane l of a wave owns bin l (true class l / C, predicted class l % C) of the wave's table
  const int bin_t = CENSUS ? (int)(threadIdx.x & 63) / C : 0, bin_p = CENSUS ? (int)(threadIdx.x & 63) % C : 0;
  unsigned cen = 0;
  // CENSUS keeps the whole wave in the loop until its last lane is done (a ballot must meet every bin's owner)
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; CENSUS ? (__any(i < (size_t)P) != 0) : (i < (size_t)P);
       i += (size_t)gridDim.x * blockDim.x) {
    int tc = -1, pc = -1;
    if (!CENSUS || i < (size_t)P) {
      float z[C], p[C];
      dg_row_load<C>(logits + i * C, z);
      dg_softmax_row<C>(z, p);
      dg_row_store<C>(probs + i * C, p);
      if (LBL != LBL_NONE) {
        float t[C];
        if (LBL == LBL_ONEHOT) {
          dg_row_load<C>(onehot + i * C, t);
          if (CENSUS) tc = dg_row_argmax<C>(t);
          if (CENSUS && WEIGHTED) tc = dg_row_any<C>(t) ? tc : -1;
        } else {
          // WEIGHTED: the ignore code becomes -1, which equals no k: t = 0, in no bin and not in nbad
          const int code = (WEIGHTED && codes[i] == wa.ignore) ? -1 : codes[i];
#pragma unroll
          for (int k = 0; k < C; ++k) t[k] = (k == code) ? 1.0f : 0.0f;
          nbad += (code >= C) ? 1u : 0u;
          if (CENSUS) tc = (code < C) ? code : -1;
        }
        if (WEIGHTED && !FOCAL) {
#pragma unroll
          for (int k = 0; k < C; ++k) t[k] = wa.cw[k] * t[k];
        }
        if (FOCAL) {
          // ts = w ((1 - eps) t + (has ? eps / C : 0)): a row without a true class stays 0, a zero-weight class too
          float w = 0.f;
#pragma unroll
          for (int k = 0; k < C; ++k) w += wa.cw[k] * t[k];
          const float u = dg_row_any<C>(t) ? eps / (float)C : 0.f;
#pragma unroll
          for (int k = 0; k < C; ++k) t[k] = w * ((1.0f - eps) * t[k] + u);
        }
        const float S = dg_row_pairsum<C>(p);
        float gq[C];
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < C; ++k) {
          const float q = p[k] / S;
          const float r = fminf(fmaxf(q, 1e-7f), 1.0f - 1e-7f);
          // clip's gradient passes on the closed interval, bounds included (TF clip_by_value, torch.clamp)
          const bool in = (q >= 1e-7f) && (q <= 1.0f - 1e-7f);
          if (FOCAL) {
            const float lg = logf(r);
            float pw, pm1;
            t_focal_pow(1.0f - r, gamma, pw, pm1);
            lsum -= t[k] * pw * lg;
            gq[k] = in ? (-t[k] * invN * (pw / q - gamma * pm1 * lg)) : 0.f;
          } else {
            lsum -= t[k] * logf(r);
            gq[k] = in ? (-t[k] * invN / q) : 0.f;    // dL/dq
          }
          dot += gq[k] * p[k];
        }
        // q = p/S: dL/dp_j = gq_j/S - dot/S^2 ; softmax: dL/dz_k = p_k (dL/dp_k - sum_j p_j dL/dp_j)
        float gp[C];
        float pg = 0.f;
#pragma unroll
        for (int k = 0; k < C; ++k) {
          gp[k] = gq[k] / S - dot / (S * S);
          pg += p[k] * gp[k];
        }
        float o[C];
#pragma unroll
        for (int k = 0; k < C; ++k) o[k] = p[k] * (gp[k] - pg);
        dg_row_store<C>(dz + i * C, o);
        if (CENSUS) pc = dg_row_argmax<C>(p);
      }
    }
    if (CENSUS) {
      // the ballots of the lane's own row and column, selected out of the C + C; a lane without a pixel, or with a code
      // >= C, has tc = -1 and is in no ballot; lanes C*C.. own no bin (bin_t >= C)
      unsigned long long mt = 0, mp = 0;
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const unsigned long long bt = __ballot(tc == k), bp = __ballot(pc == k);
        mt = (bin_t == k) ? bt : mt;
        mp = (bin_p == k) ? bp : mp;
      }
      cen += (unsigned)__popcll(mt & mp);
    }
  }
  if (LBL != LBL_NONE) {
    lsum = t_block_sum(lsum, sh4);
    if (threadIdx.x == 0) part[blockIdx.x] = lsum;
  }
  if (LBL == LBL_CODES) {
    nbad = t_block_sum_u(nbad, shu4);
    if (threadIdx.x == 0) bad_part[blockIdx.x] = nbad;
  }
  if (CENSUS) {
    __shared__ unsigned shc[4][64];
    shc[threadIdx.x >> 6][threadIdx.x & 63] = cen;
    __syncthreads();
    const int b = threadIdx.x;
    if (b < C * C) cen_part[(size_t)blockIdx.x * (C * C) + b] = (shc[0][b] + shc[1][b]) + (shc[2][b] + shc[3][b]);
  }
}
// second stage, one block: the block partials in index order; bad_out[0] = the out-of-range codes (0 without bad_part).
// CENSUS: cen_out[b] = the sum over the nb blocks of bin b of their CC-entry tables, as 64-bit counts (wave g takes the
// blocks g, g + 4, ..., lane b the bin; integer sums, any order gives the same table)
template <bool CENSUS>
__global__ void sum_small_kernel(const float* __restrict__ part, int nb, float* __restrict__ out,
                                 const unsigned* __restrict__ bad_part, unsigned* __restrict__ bad_out,
                                 const unsigned* __restrict__ cen_part, unsigned long long* __restrict__ cen_out,
                                 int CC) {
  __shared__ float sh4[4];
  __shared__ unsigned shu4[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) acc += part[i];
  acc = t_block_sum(acc, sh4);
  if (threadIdx.x == 0) out[0] = acc;
  if (bad_out) {
    unsigned nbad = 0;
    if (bad_part)
      for (int i = threadIdx.x; i < nb; i += blockDim.x) nbad += bad_part[i];
    nbad = t_block_sum_u(nbad, shu4);
    if (threadIdx.x == 0) bad_out[0] = nbad;
  }
  if (CENSUS) {
    __shared__ unsigned long long shc[4][DG_MAX_CLASSES * DG_MAX_CLASSES];
    const int g = threadIdx.x >> 6, b = threadIdx.x & 63;
    unsigned long long a = 0;
    if (b < CC)
      for (int i = g; i < nb; i += 4) a += cen_part[(size_t)i * CC + b];
    shc[g][b] = a;
    __syncthreads();
    if (g == 0 && b < CC) cen_out[b] = (shc[0][b] + shc[1][b]) + (shc[2][b] + shc[3][b]);
  }
}

// ---------------------------------------------------------------------------
// the label pre-pass of the weighted path
// ---------------------------------------------------------------------------
// The gradient needs 1 / den inside the pass that writes dz, so den exists before that pass starts: this kernel reads
// the labels alone (1 byte per pixel, or a one-hot row) and counts, per pixel, C + 3 predicates -- slot 0: the pixel's
// weight w = sum_k cw[k] t[k] (left to right) is not 0 (den); slot 1: no true class (the ignore code, an all-zero
// one-hot row); slot 2: a code >= C that is not the ignore code; slot 3 + k: true class k (the code, or the first
// arg-max of the row: the census rule).  The census's conventions: no atomics, one ballot per slot, lane j of a wave
// adds the popcount of slot j's ballot to its one counter, the four waves meet in LDS, C + 3 lanes store the block's
// partial, and a one-block second stage sums the at most 1024 partials into 64-bit counts.
template <int C, int LBL>
__global__ void label_count_kernel(const float* __restrict__ onehot, const unsigned char* __restrict__ codes,
                                   SmWeights wa, unsigned* __restrict__ cnt_part, long P) {
  static_assert(LBL == LBL_ONEHOT || LBL == LBL_CODES, "a label count needs labels");
  constexpr int NS = C + 3;
  const int lane = (int)(threadIdx.x & 63);
  unsigned cnt = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; __any(i < (size_t)P) != 0;
       i += (size_t)gridDim.x * blockDim.x) {
    int tc = -1;
    bool has_w = false, ign = false, bad = false;
    if (i < (size_t)P) {
      float w = 0.f;
      if (LBL == LBL_ONEHOT) {
        float t[C];
        dg_row_load<C>(onehot + i * C, t);
        ign = !dg_row_any<C>(t);
        tc = ign ? -1 : dg_row_argmax<C>(t);
#pragma unroll
        for (int k = 0; k < C; ++k) w += wa.cw[k] * t[k];
      } else {
        const int raw = codes[i];
        ign = raw == wa.ignore;
        bad = !ign && raw >= C;
        tc = (ign || bad) ? -1 : raw;
#pragma unroll
        for (int k = 0; k < C; ++k) w = (k == tc) ? wa.cw[k] : w;
      }
      has_w = w != 0.f;
    }
    unsigned long long m = 0;
    const unsigned long long b0 = __ballot(has_w), b1 = __ballot(ign), b2 = __ballot(bad);
    m = (lane == 0) ? b0 : m;
    m = (lane == 1) ? b1 : m;
    m = (lane == 2) ? b2 : m;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const unsigned long long bk = __ballot(tc == k);
      m = (lane == 3 + k) ? bk : m;
    }
    cnt += (unsigned)__popcll(m);
  }
  __shared__ unsigned shc[4][16];
  if (lane < NS) shc[threadIdx.x >> 6][lane] = cnt;
  __syncthreads();
  const int b = threadIdx.x;
  if (b < NS) cnt_part[(size_t)blockIdx.x * NS + b] = (shc[0][b] + shc[1][b]) + (shc[2][b] + shc[3][b]);
}
// second stage, one block of 256: out[j] = the sum over the nb blocks of slot j (wave g takes the blocks g, g + 4, ...,
// lane j the slot; integer sums, any order gives the same counts)
__global__ void label_count_sum_kernel(const unsigned* __restrict__ cnt_part, int nb, int NS,
                                       unsigned long long* __restrict__ out) {
  __shared__ unsigned long long shc[4][16];
  const int g = threadIdx.x >> 6, b = threadIdx.x & 63;
  unsigned long long a = 0;
  if (b < NS)
    for (int i = g; i < nb; i += 4) a += cnt_part[(size_t)i * NS + b];
  if (b < NS) shc[g][b] = a;
  __syncthreads();
  if (g == 0 && b < NS) out[b] = (shc[0][b] + shc[1][b]) + (shc[2][b] + shc[3][b]);
}

int dg_loss_weights_check(const char* who, const float* w, int n, int C, int ignore_code) {
  if (C < DG_MIN_CLASSES || C > DG_MAX_CLASSES) {
    dg_set_error("%s: %d classes (the kernel covers %d to %d)", who, C, DG_MIN_CLASSES, DG_MAX_CLASSES);
    return DG_ERR_ARG;
  }
  if (ignore_code < -1 || ignore_code > 255) {
    dg_set_error("%s: ignore code %d (-1 for none, else a byte value 0..255)", who, ignore_code);
    return DG_ERR_ARG;
  }
  if (!w) return DG_OK;
  if (n != C) { dg_set_error("%s: %d class weights for %d classes", who, n, C); return DG_ERR_ARG; }
  bool any = false;
  for (int k = 0; k < C; ++k) {
    if (!(w[k] >= 0.f) || w[k] > FLT_MAX) {
      dg_set_error("%s: class weight %d is %g (every weight is finite and >= 0)", who, k, (double)w[k]);
      return DG_ERR_ARG;
    }
    any = any || w[k] > 0.f;
  }
  if (!any) { dg_set_error("%s: every class weight is 0 (at least one must be > 0)", who); return DG_ERR_ARG; }
  return DG_OK;
}

static SmWeights sm_weights(const float* cw, int C, int ignore_code, const unsigned long long* den) {
  SmWeights wa;
  for (int k = 0; k < DG_MAX_CLASSES; ++k) wa.cw[k] = (k < C) ? (cw ? cw[k] : 1.0f) : 0.f;
  wa.ignore = ignore_code;
  wa.den = den;
  return wa;
}

size_t dg_label_counts_scratch(long P, int C) { return (size_t)t_nblk((size_t)P, 1024) * (C + 3); }

static int label_counts_run(const float* onehot, const unsigned char* codes, long P, int C, const SmWeights& wa,
                            unsigned long long* counts, float* scratch, hipStream_t st) {
  const int nb = t_nblk((size_t)P, 1024);
  unsigned* cnt_part = reinterpret_cast<unsigned*>(scratch);
#define DG_LC(N)                                                                                                       \
  if (onehot) hipLaunchKernelGGL((label_count_kernel<N, LBL_ONEHOT>), dim3(nb), dim3(256), 0, st, onehot, codes, wa, cnt_part, P); \
  else hipLaunchKernelGGL((label_count_kernel<N, LBL_CODES>), dim3(nb), dim3(256), 0, st, onehot, codes, wa, cnt_part, P)
  DG_FOR_CLASS_COUNT(C, DG_LC)
#undef DG_LC
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(label_count_sum_kernel, dim3(1), dim3(256), 0, st, cnt_part, nb, C + 3, counts);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

static int label_counts_check(const char* who, const float* onehot, const unsigned char* codes, long P, int C,
                              const unsigned long long* counts, const float* scratch, size_t scratch_floats) {
  if (P < 1 || (!onehot == !codes)) { dg_set_error("%s: P < 1, or not exactly one of onehot and codes", who); return DG_ERR_ARG; }
  if (onehot && ((uintptr_t)onehot & dg_row_align_mask(C))) { dg_set_error("%s: misaligned onehot", who); return DG_ERR_ARG; }
  if (!counts || ((uintptr_t)counts & 7)) { dg_set_error("%s: null or misaligned counts", who); return DG_ERR_ARG; }
  const size_t need = dg_label_counts_scratch(P, C);
  if (!scratch || scratch_floats < need) {
    dg_set_error("%s: scratch of %zu floats, the label pass needs %zu", who, scratch ? scratch_floats : (size_t)0, need);
    return DG_ERR_ARG;
  }
  return DG_OK;
}

int dg_label_counts(const float* onehot, const unsigned char* codes, long P, int C, const float* cw, int ignore_code,
                    unsigned long long* counts, float* scratch, size_t scratch_floats, hipStream_t st) {
  DGCHECK(dg_loss_weights_check("dg_label_counts", cw, C, C, ignore_code));
  DGCHECK(label_counts_check("dg_label_counts", onehot, codes, P, C, counts, scratch, scratch_floats));
  return label_counts_run(onehot, codes, P, C, sm_weights(cw, C, ignore_code, nullptr), counts, scratch, st);
}

int dg_focal_check(const char* who, float gamma, float label_smoothing) {
  if (!(gamma >= 0.f) || gamma > FLT_MAX) {
    dg_set_error("%s: focal gamma %g (finite and >= 0)", who, (double)gamma);
    return DG_ERR_ARG;
  }
  if (!(label_smoothing >= 0.f) || !(label_smoothing < 1.0f)) {
    dg_set_error("%s: label smoothing %g (in [0, 1))", who, (double)label_smoothing);
    return DG_ERR_ARG;
  }
  return DG_OK;
}

// ---------------------------------------------------------------------------
// the host entry
// ---------------------------------------------------------------------------
// The 13 legal instantiations per class count, picked by labels, then census, then the loss mode; the kernel's
// static_asserts keep the other combinations from being named here.
using SmKernel = void (*)(const float*, const float*, const unsigned char*, float*, float*, float*, unsigned*, unsigned*,
                          long, float, SmWeights, float, float);
enum { SM_PLAIN = 0, SM_WEIGHTED = 1, SM_FOCAL = 2 };

template <int C, int LBL, bool CENSUS>
static SmKernel sm_pick_mode(int mode) {
  if (mode == SM_FOCAL) return softmax_ce_kernel<C, LBL, CENSUS, true, true>;
  if (mode == SM_WEIGHTED) return softmax_ce_kernel<C, LBL, CENSUS, true, false>;
  return softmax_ce_kernel<C, LBL, CENSUS, false, false>;
}
template <int C, int LBL>
static SmKernel sm_pick_census(bool census, int mode) {
  return census ? sm_pick_mode<C, LBL, true>(mode) : sm_pick_mode<C, LBL, false>(mode);
}
template <int C>
static SmKernel sm_pick(int lbl, bool census, int mode) {
  if (lbl == LBL_ONEHOT) return sm_pick_census<C, LBL_ONEHOT>(census, mode);
  if (lbl == LBL_CODES) return sm_pick_census<C, LBL_CODES>(census, mode);
  return softmax_ce_kernel<C, LBL_NONE, false, false, false>;
}

// the cross-entropy pass's partials: 1024 floats of loss, 1024 counters of out-of-range codes, then the census's tables
size_t dg_softmax_ce_scratch(long P, int C, const DgCeSetting& set) {
  const size_t a = 2048 + (set.census ? (size_t)t_nblk((size_t)P, 1024) * C * C : 0);
  const size_t b = set.weighted_path() ? dg_label_counts_scratch(P, C) : 0;
  return a > b ? a : b;
}

int dg_softmax_ce_check(const char* who, const SoftmaxCeArgs& a) {
  const DgCeSetting& s = a.set;
  const int C = a.C;
  if (s.focal) DGCHECK(dg_focal_check(who, s.gamma, s.eps));
  if (s.weighted) DGCHECK(dg_loss_weights_check(who, s.cw, C, C, s.ignore));
  if (!a.logits || !a.probs || a.P < 1) { dg_set_error("%s: null logits or probs, or P < 1", who); return DG_ERR_ARG; }
  if (C < DG_MIN_CLASSES || C > DG_MAX_CLASSES) {
    dg_set_error("%s: %d classes (the kernel covers %d to %d)", who, C, DG_MIN_CLASSES, DG_MAX_CLASSES);
    return DG_ERR_ARG;
  }
  if (a.lab.onehot && a.lab.codes) { dg_set_error("%s: one-hot labels and class codes are both given", who); return DG_ERR_ARG; }
  const bool labels = a.lab.onehot || a.lab.codes;
  if (labels && (!a.dz || !a.loss_sum)) { dg_set_error("%s: labels without dz or loss_sum", who); return DG_ERR_ARG; }
  // rows are read and written 16 bytes at a time where C is a multiple of 4, else float by float
  const uintptr_t al = dg_row_align_mask(C);
  if ((((uintptr_t)a.logits | (uintptr_t)a.probs | (uintptr_t)a.lab.onehot | (uintptr_t)a.dz) & al) ||
      ((uintptr_t)a.loss_sum & 3)) {
    dg_set_error("%s: logits, probs, onehot and dz must be %d-byte aligned for %d classes", who, (int)al + 1, C);
    return DG_ERR_ARG;
  }
  if (!labels) {
    if (s.census || s.weighted_path()) { dg_set_error("%s: a census, loss weights and the focal loss need labels", who); return DG_ERR_ARG; }
    return DG_OK;
  }
  if (s.census && (!a.census || ((uintptr_t)a.census & 7))) { dg_set_error("%s: null or misaligned census", who); return DG_ERR_ARG; }
  if (s.weighted_path() && (!a.counts || ((uintptr_t)a.counts & 7))) { dg_set_error("%s: null or misaligned counts", who); return DG_ERR_ARG; }
  if (!a.bad_count && (a.lab.codes || s.census || s.weighted_path())) {
    dg_set_error("%s: no counter of out-of-range codes", who);
    return DG_ERR_ARG;
  }
  const size_t need = dg_softmax_ce_scratch(a.P, C, s);
  if (!a.scratch || a.scratch_floats < need) {
    dg_set_error("%s: scratch of %zu floats, the launches need %zu", who, a.scratch ? a.scratch_floats : (size_t)0, need);
    return DG_ERR_ARG;
  }
  return DG_OK;
}

int dg_softmax_ce(const SoftmaxCeArgs& a, hipStream_t st) {
  DGCHECK(dg_softmax_ce_check("dg_softmax_ce", a));
  const DgCeSetting& s = a.set;
  const int C = a.C;
  const int lbl = a.lab.onehot ? LBL_ONEHOT : (a.lab.codes ? LBL_CODES : LBL_NONE);
  const int mode = s.focal ? SM_FOCAL : (s.weighted ? SM_WEIGHTED : SM_PLAIN);
  SmWeights wa{};
  if (mode != SM_PLAIN) {
    // the focal mode alone: unit weights and no ignore code.  The label pass's partials and the cross-entropy pass's
    // share the scratch: the second stage of the first has read them before the second pass, behind it on the stream,
    // writes; and a.counts[0] holds den when that pass runs
    wa = sm_weights(s.weighted ? s.cw : nullptr, C, (s.weighted && a.lab.codes) ? s.ignore : -1, a.counts);
    DGCHECK(label_counts_run(a.lab.onehot, a.lab.codes, a.P, C, wa, a.counts, a.scratch, st));
  }
  const int nb = t_nblk((size_t)a.P, 1024);
  float* part = a.scratch;
  unsigned* bad_part = a.scratch ? reinterpret_cast<unsigned*>(a.scratch + 1024) : nullptr;
  unsigned* cen_part = s.census ? reinterpret_cast<unsigned*>(a.scratch + 2048) : nullptr;
  const float invN = (lbl == LBL_NONE) ? 0.f : 1.0f / (float)a.P;
  SmKernel kernel = nullptr;
#define DG_SM(N) kernel = sm_pick<N>(lbl, s.census, mode)
  DG_FOR_CLASS_COUNT(C, DG_SM)
#undef DG_SM
  hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, st, a.logits, a.lab.onehot, a.lab.codes, a.probs, a.dz, part,
                     bad_part, cen_part, a.P, invN, wa, s.focal ? s.gamma : 0.f, s.focal ? s.eps : 0.f);
  HIPCHECK(hipGetLastError());
  if (lbl == LBL_NONE) return DG_OK;
  const unsigned* bad_in = lbl == LBL_CODES ? bad_part : nullptr;
  if (s.census)
    hipLaunchKernelGGL(sum_small_kernel<true>, dim3(1), dim3(256), 0, st, part, nb, a.loss_sum, bad_in, a.bad_count,
                       cen_part, a.census, C * C);
  else
    hipLaunchKernelGGL(sum_small_kernel<false>, dim3(1), dim3(256), 0, st, part, nb, a.loss_sum, bad_in, a.bad_count,
                       nullptr, nullptr, 0);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
