// The labels of the supervised losses, stated once for softmax_ce.hip, dice_loss.hip and boundary_loss.hip: where a
// pixel's label comes from, which pixels take part, and the host's way from a class count to a kernel instantiation.
#pragma once
#include "softmax_row.h"

// LBL_ONEHOT reads a float32 one-hot row, LBL_CODES one byte per pixel, LBL_NONE (the cross-entropy alone) no label
enum { LBL_NONE = 0, LBL_ONEHOT = 1, LBL_CODES = 2 };

// One pixel's label row and whether the pixel takes part (m).  LBL_CODES: t[k] = (k == code) formed in registers, a
// code is only compared, never used as an index; the ignore code and any code >= C stay out.  LBL_ONEHOT: the row as
// given; with ignore >= 0 an all-zero row stays out.  The statements that follow are the same for both sources, so
// codes and their one-hot encoding agree bit for bit.  M_ONLY: the caller wants m alone and does not read t, so a
// one-hot row is not loaded where ignore < 0 lets every pixel in (left to the compiler, C <= 4 loads it regardless).
template <int C, int LBL, bool M_ONLY = false>
__device__ __forceinline__ bool dg_label_row(const float* __restrict__ onehot, const unsigned char* __restrict__ codes,
                                             size_t i, int ignore, float (&t)[C]) {
  static_assert(LBL == LBL_ONEHOT || LBL == LBL_CODES, "a label row needs labels");
  if (LBL == LBL_ONEHOT) {
    if (M_ONLY && ignore < 0) return true;
    dg_row_load<C>(onehot + i * C, t);
    return ignore < 0 || dg_row_any<C>(t);
  }
  const int raw = codes[i];
  const int code = (raw == ignore || raw >= C) ? -1 : raw;
#pragma unroll
  for (int k = 0; k < C; ++k) t[k] = (k == code) ? 1.0f : 0.0f;
  return code >= 0;
}

// Host: the class count C = 2..8 (the checks have refused every other) becomes the constant N of CALL(N), and a label
// source with one more switch the two constants of CALL(LBL, FLAG).
#define DG_FOR_CLASS_COUNT(C, CALL)                                                                    \
  switch (C) {                                                                                         \
    case 2: CALL(2); break;                                                                            \
    case 3: CALL(3); break;                                                                            \
    case 4: CALL(4); break;                                                                            \
    case 5: CALL(5); break;                                                                            \
    case 6: CALL(6); break;                                                                            \
    case 7: CALL(7); break;                                                                            \
    case 8: CALL(8); break;                                                                            \
  }
#define DG_FOR_LABELS_AND_FLAG(ONEHOT, FLAG, CALL)                                                     \
  do {                                                                                                 \
    if ((ONEHOT) && (FLAG)) CALL(LBL_ONEHOT, true);                                                    \
    else if (ONEHOT) CALL(LBL_ONEHOT, false);                                                          \
    else if (FLAG) CALL(LBL_CODES, true);                                                              \
    else CALL(LBL_CODES, false);                                                                       \
  } while (0)
static_assert(DG_MIN_CLASSES == 2 && DG_MAX_CLASSES == 8, "DG_FOR_CLASS_COUNT names every class count");
