// One pixel's class row in registers: C = 2..8 logits, probabilities or gradient entries (DEPGAN_MAX_HEAD_CLASSES = 8
// keeps a row within two float4).  Shared by softmax_ce_kernel (softmax_ce.hip) and head_softmax_bf16s_kernel
// (igemm_bf16s.hip), so the two softmaxes are one text.
#pragma once
#include "common.h"
#include "../../include/depgan.h"

#define DG_MIN_CLASSES 2
#define DG_MAX_CLASSES DEPGAN_MAX_HEAD_CLASSES
static_assert(DG_MAX_CLASSES <= 8, "a class row lives in registers as two float4");

// dense rows of C floats: 16-byte accesses where C is a multiple of 4 (the row start is then 16-byte aligned whenever
// the base is), else one float at a time.  dg_row_align_mask: the address bits a host check wants clear for that
static inline uintptr_t dg_row_align_mask(int C) { return (C % 4 == 0) ? 15 : 3; }
template <int C>
__device__ __forceinline__ void dg_row_load(const float* __restrict__ p, float (&r)[C]) {
  if constexpr (C % 4 == 0) {
#pragma unroll
    for (int j = 0; j < C / 4; ++j) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) r[4 * j + k] = v[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < C; ++k) r[k] = p[k];
  }
}
template <int C>
__device__ __forceinline__ void dg_row_store(float* __restrict__ p, const float (&r)[C]) {
  if constexpr (C % 4 == 0) {
#pragma unroll
    for (int j = 0; j < C / 4; ++j) {
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = r[4 * j + k];
      *reinterpret_cast<f32x4*>(p + 4 * j) = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < C; ++k) p[k] = r[k];
  }
}

// Evaluation order of a row reduction, for every C: the pairs (r0 . r1), (r2 . r3), ... are formed first and folded
// left to right, an odd last element folded in at the end.  For C = 4 that is (r0 . r1) . (r2 . r3).
template <int C>
__device__ __forceinline__ float dg_row_max(const float (&z)[C]) {
  float m = fmaxf(z[0], z[1]);
#pragma unroll
  for (int k = 2; k + 1 < C; k += 2) m = fmaxf(m, fmaxf(z[k], z[k + 1]));
  if (C & 1) m = fmaxf(m, z[C - 1]);
  return m;
}
template <int C>
__device__ __forceinline__ float dg_row_pairsum(const float (&p)[C]) {
  float s = p[0] + p[1];
#pragma unroll
  for (int k = 2; k + 1 < C; k += 2) s = s + (p[k] + p[k + 1]);
  if (C & 1) s = s + p[C - 1];
  return s;
}

// first index of the row's maximum: k = 0..C-1 left to right, replaced on a strict >, so a tie keeps the lower index
// (np.argmax of the same floats; a NaN never wins a comparison here, where np.argmax would return it)
template <int C>
__device__ __forceinline__ int dg_row_argmax(const float (&r)[C]) {
  int a = 0;
  float m = r[0];
#pragma unroll
  for (int k = 1; k < C; ++k)
    if (r[k] > m) {
      m = r[k];
      a = k;
    }
  return a;
}

// whether any entry of the row is not zero (a NaN is not zero)
template <int C>
__device__ __forceinline__ bool dg_row_any(const float (&r)[C]) {
  bool any = false;
#pragma unroll
  for (int k = 0; k < C; ++k) any = any || (r[k] != 0.f);
  return any;
}

// p = softmax(z): maximum in dg_row_max's order, e_k = expf(z_k - m), S0 = ((0 + e_0) + e_1) + ... left to right,
// p_k = e_k / S0
template <int C>
__device__ __forceinline__ void dg_softmax_row(const float (&z)[C], float (&p)[C]) {
  const float m = dg_row_max<C>(z);
  float S0 = 0.f;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    p[k] = expf(z[k] - m);
    S0 += p[k];
  }
#pragma unroll
  for (int k = 0; k < C; ++k) p[k] /= S0;
}
