// Soft Dice loss of the supervised path (see train_ops.h, dg_dice_loss): a reduction pass over the stored probabilities
// and the labels, a one-block coefficient stage, and a gradient pass that reads the coefficients on the device.  All
// HBM-bound; rows move through softmax_row.h's helpers (16-byte accesses for C = 4 and 8).  No atomics: block partials
// in the caller's scratch, summed in index order in double by the one block of the second stage, so a call's result does
// not depend on what any buffer held before or on how the blocks were scheduled.
#include "train_ops.h"

#include <float.h>

#include "block_sum.h"
#include "labels.h"

// Stage 1.  Per thread 3 C float accumulators over its grid-stride pixels -- I_k += t_k p_k, P_k += p_k, T_k += t_k for
// the pixels that take part -- then wave shuffles, the four waves through LDS, and one partial of 3 C floats per block:
// part[block * 3 C + j], j = k (I), C + k (P), 2 C + k (T).
template <int C, int LBL>
__global__ __launch_bounds__(256) void dice_sums_kernel(const float* __restrict__ probs, const float* __restrict__ onehot,
                                                        const unsigned char* __restrict__ codes, int ignore,
                                                        float* __restrict__ part, long P) {
  float acc[3 * C];
#pragma unroll
  for (int j = 0; j < 3 * C; ++j) acc[j] = 0.f;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * blockDim.x) {
    float p[C], t[C];
    const bool m = dg_label_row<C, LBL>(onehot, codes, i, ignore, t);
    dg_row_load<C>(probs + i * C, p);
    if (m) {
#pragma unroll
      for (int k = 0; k < C; ++k) {
        acc[k] = __fmaf_rn(t[k], p[k], acc[k]);
        acc[C + k] += p[k];
        acc[2 * C + k] += t[k];
      }
    }
  }
  __shared__ float sh[4][3 * C];
#pragma unroll
  for (int j = 0; j < 3 * C; ++j) {
    float v = acc[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][j] = v;
  }
  __syncthreads();
  const int b = threadIdx.x;
  if (b < 3 * C) part[(size_t)blockIdx.x * (3 * C) + b] = (sh[0][b] + sh[1][b]) + (sh[2][b] + sh[3][b]);
}

// the Dice setting as a kernel argument: the form, the smoothing term and the class coefficients c_k (class form)
struct DiceCoef {
  int form;
  float smooth;
  float c[DG_MAX_CLASSES];
};

// Stage 2, one block of 256.  The nb block partials go through LDS 256 blocks at a time (coalesced loads, all in
// flight), and lane j < 3 C adds its slot over the blocks in index order in double.  Thread 0 then forms, in double,
//   class form: Num_k = 2 I_k + s, Den_k = T_k + P_k + s, L = sum_k c_k (1 - Num_k / Den_k)   (k left to right)
//               A_k = -2 c_k / Den_k, B_k = c_k Num_k / Den_k^2
//   flat form:  the same with Num = 2 sum_k I_k + s, Den = sum_k T_k + sum_k P_k + s, L = 1 - Num / Den, c_k = 1
// and stores the sums as doubles, L rounded once to float, and A_k, B_k as floats.  Den > 0 because s > 0.
__global__ __launch_bounds__(256) void dice_coeffs_kernel(const float* __restrict__ part, int nb, int C, DiceCoef dc,
                                                          DgDiceDev* __restrict__ out) {
  __shared__ float sh[256 * 3 * DG_MAX_CLASSES];
  __shared__ double sums[3 * DG_MAX_CLASSES];
  const int NS = 3 * C;
  double a = 0.0;
  for (int b0 = 0; b0 < nb; b0 += 256) {
    const int nbk = min(256, nb - b0), cnt = nbk * NS;
    __syncthreads();
    for (int e = threadIdx.x; e < cnt; e += 256) sh[e] = part[(size_t)b0 * NS + e];
    __syncthreads();
    if ((int)threadIdx.x < NS)
      for (int b = 0; b < nbk; ++b) a += (double)sh[b * NS + threadIdx.x];
  }
  if ((int)threadIdx.x < NS) {
    sums[threadIdx.x] = a;
    out->sums[threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double s = (double)dc.smooth;
  double L;
  if (dc.form == DEPGAN_DICE_FLAT) {
    double I = 0.0, Pp = 0.0, T = 0.0;
    for (int k = 0; k < C; ++k) {
      I += sums[k];
      Pp += sums[C + k];
      T += sums[2 * C + k];
    }
    const double num = 2.0 * I + s, den = T + Pp + s;
    L = 1.0 - num / den;
    for (int k = 0; k < C; ++k) {
      out->A[k] = (float)(-2.0 / den);
      out->B[k] = (float)(num / (den * den));
    }
  } else {
    L = 0.0;
    for (int k = 0; k < C; ++k) {
      const double ck = (double)dc.c[k];
      const double num = 2.0 * sums[k] + s, den = sums[2 * C + k] + sums[C + k] + s;
      L += ck * (1.0 - num / den);
      out->A[k] = (float)(-2.0 * ck / den);
      out->B[k] = (float)(ck * num / (den * den));
    }
  }
  out->loss = (float)L;
}

// Stage 3.  g_k = m (A_k t_k + B_k) = dL/dp_k, pg = sum_j p_j g_j (left to right), and through the softmax
// x_k = p_k (g_k - pg); dz_k = ce_coef dz_k + dice_coef x_k.  READ_DZ = false (ce_coef == 0): dz is written without
// being read, dz_k = dice_coef x_k.  A pixel that takes no part has x = 0.  The products and fused multiply-adds are
// spelled out, so the two label sources and every instantiation round alike whatever the compiler would contract.
template <int C, int LBL, bool READ_DZ>
__global__ __launch_bounds__(256) void dice_grad_kernel(const float* __restrict__ probs, const float* __restrict__ onehot,
                                                        const unsigned char* __restrict__ codes, int ignore,
                                                        const DgDiceDev* __restrict__ co, float ce_coef, float dice_coef,
                                                        float* __restrict__ dz, long P) {
  float A[C], B[C];
#pragma unroll
  for (int k = 0; k < C; ++k) {
    A[k] = co->A[k];
    B[k] = co->B[k];
  }
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * blockDim.x) {
    float p[C], t[C], g[C], o[C];
    const bool m = dg_label_row<C, LBL>(onehot, codes, i, ignore, t);
    dg_row_load<C>(probs + i * C, p);
    float pg = 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      g[k] = m ? __fmaf_rn(A[k], t[k], B[k]) : 0.f;
      pg = __fmaf_rn(p[k], g[k], pg);
    }
#pragma unroll
    for (int k = 0; k < C; ++k) o[k] = m ? __fmul_rn(dice_coef, __fmul_rn(p[k], g[k] - pg)) : 0.f;
    if (READ_DZ) {
      float d[C];
      dg_row_load<C>(dz + i * C, d);
#pragma unroll
      for (int k = 0; k < C; ++k) o[k] = __fmaf_rn(ce_coef, d[k], o[k]);
    }
    dg_row_store<C>(dz + i * C, o);
  }
}

int dg_class_count_check(const char* who, int C) {
  if (C < DG_MIN_CLASSES || C > DG_MAX_CLASSES) {
    dg_set_error("%s: %d classes (the kernels cover %d to %d)", who, C, DG_MIN_CLASSES, DG_MAX_CLASSES);
    return DG_ERR_ARG;
  }
  return DG_OK;
}

int dg_class_coef_check(const char* who, const float* coef, int n, int C) {
  if (n != C) { dg_set_error("%s: %d class coefficients for %d classes", who, n, C); return DG_ERR_ARG; }
  bool any = false;
  for (int k = 0; k < C; ++k) {
    if (!(coef[k] >= 0.f) || coef[k] > FLT_MAX) {
      dg_set_error("%s: class coefficient %d is %g (every coefficient is finite and >= 0)", who, k, (double)coef[k]);
      return DG_ERR_ARG;
    }
    any = any || coef[k] > 0.f;
  }
  if (!any) { dg_set_error("%s: every class coefficient is 0 (at least one must be > 0)", who); return DG_ERR_ARG; }
  return DG_OK;
}

int dg_loss_operands_check(const char* who, const float* probs, const char* extra_name, const float* extra, DgLabels lab,
                           int ignore_code, const float* dz, long P, bool p_below_2_31, int C) {
  DGCHECK(dg_class_count_check(who, C));
  if (!probs || (extra_name && !extra) || P < 1 || (p_below_2_31 && P >= (1L << 31)) || (!lab.onehot == !lab.codes)) {
    dg_set_error("%s: null probs%s%s, P %s, or not exactly one of onehot and codes", who, extra_name ? " or " : "",
                 extra_name ? extra_name : "", p_below_2_31 ? "outside [1, 2^31)" : "< 1");
    return DG_ERR_ARG;
  }
  if (ignore_code < -1 || ignore_code > 255) {
    dg_set_error("%s: ignore code %d (-1 for none, else a byte value 0..255)", who, ignore_code);
    return DG_ERR_ARG;
  }
  const uintptr_t al = dg_row_align_mask(C);
  if (((uintptr_t)probs | (uintptr_t)extra | (uintptr_t)lab.onehot | (uintptr_t)dz) & al) {
    dg_set_error("%s: probs, %s%sonehot and dz must be %d-byte aligned for %d classes", who,
                 extra_name ? extra_name : "", extra_name ? ", " : "", (int)al + 1, C);
    return DG_ERR_ARG;
  }
  return DG_OK;
}

int dg_dice_check(const char* who, int form, float ce_coef, float dice_coef, float smooth, const float* coef, int n,
                  int C) {
  DGCHECK(dg_class_count_check(who, C));
  if (form != DEPGAN_DICE_FLAT && form != DEPGAN_DICE_CLASS) {
    dg_set_error("%s: form %d (DEPGAN_DICE_FLAT = 1 or DEPGAN_DICE_CLASS = 2)", who, form);
    return DG_ERR_ARG;
  }
  if (!(ce_coef >= 0.f) || ce_coef > FLT_MAX) {
    dg_set_error("%s: ce_coef is %g (finite and >= 0)", who, (double)ce_coef);
    return DG_ERR_ARG;
  }
  if (!(dice_coef > 0.f) || dice_coef > FLT_MAX) {
    dg_set_error("%s: dice_coef is %g (finite and > 0)", who, (double)dice_coef);
    return DG_ERR_ARG;
  }
  if (!(smooth > 0.f) || smooth > FLT_MAX) {
    dg_set_error("%s: smooth is %g (finite and > 0)", who, (double)smooth);
    return DG_ERR_ARG;
  }
  if (!coef) return DG_OK;
  if (form == DEPGAN_DICE_FLAT) {
    dg_set_error("%s: the flat form takes no class coefficients", who);
    return DG_ERR_ARG;
  }
  return dg_class_coef_check(who, coef, n, C);
}

size_t dg_dice_scratch(long P, int C) { return (size_t)t_nblk((size_t)P, 1024) * 3 * C; }

template <int C>
static void dice_launch(bool onehot_lbl, bool read_dz, int nb, hipStream_t st, const float* probs, const float* onehot,
                        const unsigned char* codes, int ignore, float* part, const DiceCoef& dc, DgDiceDev* out,
                        float ce_coef, float dice_coef, float* dz, long P) {
  if (onehot_lbl)
    hipLaunchKernelGGL((dice_sums_kernel<C, LBL_ONEHOT>), dim3(nb), dim3(256), 0, st, probs, onehot, codes, ignore, part, P);
  else
    hipLaunchKernelGGL((dice_sums_kernel<C, LBL_CODES>), dim3(nb), dim3(256), 0, st, probs, onehot, codes, ignore, part, P);
  hipLaunchKernelGGL(dice_coeffs_kernel, dim3(1), dim3(256), 0, st, part, nb, C, dc, out);
  if (!dz) return;
#define DG_DICE_GRAD(LBL, RD)                                                                                          \
  hipLaunchKernelGGL((dice_grad_kernel<C, LBL, RD>), dim3(nb), dim3(256), 0, st, probs, onehot, codes, ignore, out,    \
                     ce_coef, dice_coef, dz, P)
  DG_FOR_LABELS_AND_FLAG(onehot_lbl, read_dz, DG_DICE_GRAD);
#undef DG_DICE_GRAD
}

int dg_dice_loss(const float* probs, DgLabels lab, int ignore_code, const DgDiceSetting& set, float* dz, DgDiceDev* out,
                 long P, int C, float* scratch, size_t scratch_floats, hipStream_t st) {
  DGCHECK(dg_dice_check("dg_dice_loss", set.form, set.ce_coef, set.dice_coef, set.smooth,
                        set.form == DEPGAN_DICE_CLASS ? set.c : nullptr, C, C));
  DGCHECK(dg_loss_operands_check("dg_dice_loss", probs, nullptr, nullptr, lab, ignore_code, dz, P, false, C));
  if (!out || ((uintptr_t)out & 7)) { dg_set_error("dg_dice_loss: null or misaligned out"); return DG_ERR_ARG; }
  const size_t need = dg_dice_scratch(P, C);
  if (!scratch || scratch_floats < need) {
    dg_set_error("dg_dice_loss: scratch of %zu floats, the launches need %zu", scratch ? scratch_floats : (size_t)0, need);
    return DG_ERR_ARG;
  }
  DiceCoef dc;
  dc.form = set.form;
  dc.smooth = set.smooth;
  for (int k = 0; k < DG_MAX_CLASSES; ++k) dc.c[k] = (k < C) ? set.c[k] : 0.f;
  const int nb = t_nblk((size_t)P, 1024);
  const bool read_dz = set.ce_coef != 0.f;
#define DG_DICE(N)                                                                                                \
  dice_launch<N>(lab.onehot != nullptr, read_dz, nb, st, probs, lab.onehot, lab.codes, ignore_code, scratch, dc, out, \
                 set.ce_coef, set.dice_coef, dz, P)
  DG_FOR_CLASS_COUNT(C, DG_DICE)
#undef DG_DICE
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
