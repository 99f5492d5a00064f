// Boundary loss of the supervised path (Kervadec et al.; include/depgan.h, depgan_uresnet_set_boundary_loss, states the
// rule): per slice and class the signed distance map of the labels, then the softmax probabilities integrated against
// it.  Slices are (H, W) with W contiguous; a batch is n of them and no slice sees another.
//
//   bl_rows_kernel    one workgroup per (slice, row): the true class of every pixel of the row (the census rule), then
//                     per switched-on class k the distance in pixels to the nearest pixel of the row whose membership
//                     of S_k = {true class == k} differs from the pixel's own, 15 bits (BL_NONE: the row is all of one
//                     membership), bit 15 = the pixel is in S_k
//   bl_cols_kernel    along H, per (slice, class): d2[y] = min_y' fl(a(y') + fl((y - y')^2 wy)) over the rows y' whose
//                     nearest pixel of the OTHER membership than pixel y's lies at a(y') = fl(g^2 wx) -- 0 where the
//                     pixel of row y' in this column is of the other membership itself, g's value where it is of the
//                     same.  So one 16-bit map per class serves the inside and the outside distances.  Then phi.
//   bl_loss_kernel    L_B's block partials and (GRAD) dz += boundary_coef p (g - sum p g)
//   bl_finish_kernel  one block adds the partials in index order, divides by M
//
// The scan and the sweep are edt.h's, the text depgan_eval_edt_sq runs, so d2 is bit for bit what that entry gives on
// the slice as a (1, H, W) volume.  No atomics anywhere, nothing to zero between calls.
#include "train_ops.h"

#include <float.h>

#include "block_sum.h"
#include "edt.h"
#include "labels.h"

// every double operation of this file is rounded on its own too (edt.h has the reasons)
#pragma clang fp contract(off)

namespace {

constexpr unsigned short BL_NONE = 0x7FFF, BL_IN = 0x8000;
constexpr int BL_MAX_BLOCKS = 1024;
constexpr unsigned char BL_NO_CLASS = 0xFF;

// the switched-on classes of a call, by value: k[0..n) ascending
struct BlClasses {
  int n;
  unsigned char k[DG_MAX_CLASSES];
};

// grid n * H, block 256, workgroup = one row of one slice: per switched-on class the scan of edt.h over the row's
// changes of membership.  g is (n, classes.n, H, W); ignore as dg_dice_loss takes it (codes: that code has no class;
// onehot: >= 0 keeps the all-zero rows without one, < 0 gives them class 0, the first arg-max).  A code >= C has no
// class.  The decode stays here and not in labels.h: C is a runtime value in this kernel, and it wants the class.
template <int LBL>
__global__ __launch_bounds__(256) void bl_rows_kernel(const float* __restrict__ onehot,
                                                      const unsigned char* __restrict__ codes, int ignore,
                                                      unsigned short* __restrict__ g, int H, int W, int C,
                                                      BlClasses cls) {
  __shared__ unsigned char tc[DG_EDT_MAX_DIM];
  const size_t row = blockIdx.x;                        // slice * H + y
  const size_t base = row * (size_t)W;
  for (int x = threadIdx.x; x < W; x += 256) {
    int cl;
    if (LBL == LBL_ONEHOT) {
      const float* r = onehot + (base + x) * (size_t)C;
      float m = r[0];
      bool any = m != 0.f;
      cl = 0;
      for (int k = 1; k < C; ++k) {
        const float v = r[k];
        any = any || (v != 0.f);
        if (v > m) {
          m = v;
          cl = k;
        }
      }
      if (ignore >= 0 && !any) cl = BL_NO_CLASS;
    } else {
      const int raw = codes[base + x];
      cl = (raw == ignore || raw >= C) ? BL_NO_CLASS : raw;
    }
    tc[x] = (unsigned char)cl;
  }
  __syncthreads();
  const size_t slice = row / (size_t)H, y = row - slice * (size_t)H;
  for (int ka = 0; ka < cls.n; ++ka) {
    const int k = cls.k[ka];
    unsigned short* grow = g + ((slice * (size_t)cls.n + (size_t)ka) * (size_t)H + y) * (size_t)W;
    dg_edt_row_scan<true>(
        W, [&](int x) { return (tc[x] == k) != (tc[x - 1] == k); },
        [&](int x, int d) {
          const unsigned short in = tc[x] == k ? BL_IN : (unsigned short)0;
          grow[x] = (unsigned short)((d >= DG_EDT_MAX_DIM ? (int)BL_NONE : d) | in);
        });
    __syncthreads();                                    // the scan's summaries are written again by the next class
  }
}

// grid ceil(W / 64) * ceil(H / 16) * n * classes.n (column tile fastest), block 256: the sweep of edt.h over one
// (slice, class) with two staged values per candidate row, a = the squared row distance to the nearest pixel NOT in S
// (0 where the pixel is not in S itself) and b = to the nearest pixel in S.  An output pixel in S reads a, one outside
// reads b.  phi is (n, H, W, C).  The workgroups of the first switched-on class also write 0 to the switched-off
// classes.
__global__ __launch_bounds__(256) void bl_cols_kernel(const unsigned short* __restrict__ g, float* __restrict__ phi,
                                                      int H, int W, int C, BlClasses cls, int col_tiles, int row_tiles,
                                                      double wx, double wy, double inside_offset) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned bid = blockIdx.x;
  const int ct = (int)(bid % (unsigned)col_tiles);
  bid /= (unsigned)col_tiles;
  const int rt = (int)(bid % (unsigned)row_tiles);
  const unsigned map = bid / (unsigned)row_tiles;        // slice * cls.n + ka
  const unsigned slice = map / (unsigned)cls.n;
  const int ka = (int)(map - slice * (unsigned)cls.n);
  const int col = ct * DG_EDT_COLS + lane;
  const bool live = col < W;
  const size_t base = (size_t)map * (size_t)H * (size_t)W;
  const int r0 = rt * DG_EDT_TILE_ROWS + wave * DG_EDT_ROWS_PER_THREAD;
  const double inf = INFINITY;
  double best[DG_EDT_ROWS_PER_THREAD];
  bool in[DG_EDT_ROWS_PER_THREAD];
#pragma unroll
  for (int k = 0; k < DG_EDT_ROWS_PER_THREAD; ++k)
    in[k] = live && r0 + k < H && (g[base + (size_t)(r0 + k) * (size_t)W + (size_t)col] & BL_IN) != 0;
  dg_edt_axis_sweep<32, true>(H, r0, live, wy, in, [&](int r, double& ao, double& ai) {
    const unsigned short gv = g[base + (size_t)r * (size_t)W + (size_t)col];
    const int d = gv & BL_NONE;
    double a = inf;
    if (d != BL_NONE) {
      const double gd = (double)d;
      a = (gd * gd) * wx;                                   // gd * gd is exact
    }
    const bool is_in = (gv & BL_IN) != 0;
    ao = is_in ? a : 0.0;
    ai = is_in ? 0.0 : a;
  }, best);
  if (!live) return;
  const int kclass = cls.k[ka];
#pragma unroll
  for (int k = 0; k < DG_EDT_ROWS_PER_THREAD; ++k) {
    if (r0 + k >= H) continue;
    const double d2 = best[k];
    float v = 0.f;
    if (d2 != inf) {
      const double d = __dsqrt_rn(d2);
      v = in[k] ? (float)(-(d - inside_offset)) : (float)d;
    }
    float* prow = phi + (((size_t)slice * (size_t)H + (size_t)(r0 + k)) * (size_t)W + (size_t)col) * (size_t)C;
    prow[kclass] = v;
    if (ka == 0) {
      int next = 0;                                         // cls.k ascending: every class not listed gets 0
      for (int c = 0; c < C; ++c) {
        if (next < cls.n && cls.k[next] == c) ++next;
        else prow[c] = 0.f;
      }
    }
  }
}

// the coefficients of the loss as a kernel argument
struct BlCoef {
  float c[DG_MAX_CLASSES];
  float boundary_coef;
};

// M of a call: every pixel, or P less the pixels without a true class and the codes out of range, as the label pre-pass
// counted them (DgCeDev::counts)
__device__ __forceinline__ double bl_taking_part(const unsigned long long* __restrict__ counts, long P) {
  if (!counts) return (double)P;
  return (double)((long long)P - (long long)counts[1] - (long long)counts[2]);
}

// grid min(1024, ceil(P / 256)), block 256, grid-stride over the pixels.  Per pixel that takes part, in float32:
//   w_k = c_k phi_k, term = sum_k w_k p_k (fused multiply-adds, k left to right), added to the thread's double
//   GRAD: g_k = w_k (1 / M), pg = sum_k p_k g_k, dz_k = dz_k + boundary_coef (p_k (g_k - pg))
// A pixel that takes no part is neither read further nor written.  part[block] = the block's sum: wave shuffles, then
// the four waves in LDS.
template <int C, int LBL, bool GRAD>
__global__ __launch_bounds__(256) void bl_loss_kernel(const float* __restrict__ probs, const float* __restrict__ phi,
                                                      const float* __restrict__ onehot,
                                                      const unsigned char* __restrict__ codes, int ignore, BlCoef co,
                                                      const unsigned long long* __restrict__ counts,
                                                      float* __restrict__ dz, double* __restrict__ part, long P) {
  float invM = 0.f;
  if (GRAD) {
    const double M = bl_taking_part(counts, P);
    invM = M > 0.0 ? 1.0f / (float)M : 0.f;
  }
  double acc = 0.0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * blockDim.x) {
    float t[C];                                             // not read: membership alone
    if (!dg_label_row<C, LBL, true>(onehot, codes, i, ignore, t)) continue;
    float p[C], w[C];
    dg_row_load<C>(probs + i * C, p);
    dg_row_load<C>(phi + i * C, w);
    float term = 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      w[k] = __fmul_rn(co.c[k], w[k]);
      term = __fmaf_rn(w[k], p[k], term);
    }
    acc = acc + (double)term;
    if (GRAD) {
      float gk[C], d[C];
      float pg = 0.f;
#pragma unroll
      for (int k = 0; k < C; ++k) {
        gk[k] = __fmul_rn(w[k], invM);
        pg = __fmaf_rn(p[k], gk[k], pg);
      }
      dg_row_load<C>(dz + i * C, d);
#pragma unroll
      for (int k = 0; k < C; ++k) d[k] = d[k] + __fmul_rn(co.boundary_coef, __fmul_rn(p[k], gk[k] - pg));
      dg_row_store<C>(dz + i * C, d);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_down(acc, o, 64);
  __shared__ double sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// one block of 256: the nb <= 1024 partials go through LDS, thread 0 adds them in index order;
// out = {L_B = sum / M (0.0 for M = 0), M}
__global__ __launch_bounds__(256) void bl_finish_kernel(const double* __restrict__ part, int nb,
                                                        const unsigned long long* __restrict__ counts, long P,
                                                        DgBoundaryDev* __restrict__ out) {
  __shared__ double sh[BL_MAX_BLOCKS];
  for (int i = threadIdx.x; i < nb; i += 256) sh[i] = part[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s = s + sh[b];
  const double M = bl_taking_part(counts, P);
  out->loss = M > 0.0 ? s / M : 0.0;
  out->M = M;
}

template <int C>
void bl_loss_launch(bool onehot_lbl, int nb, hipStream_t st, const float* probs, const float* phi, const float* onehot,
                    const unsigned char* codes, int ignore, const BlCoef& co, const unsigned long long* counts,
                    float* dz, double* part, long P) {
#define DG_BL(LBL, GR)                                                                                              \
  hipLaunchKernelGGL((bl_loss_kernel<C, LBL, GR>), dim3(nb), dim3(256), 0, st, probs, phi, onehot, codes, ignore, co, \
                     counts, dz, part, P)
  DG_FOR_LABELS_AND_FLAG(onehot_lbl, dz != nullptr, DG_BL);
#undef DG_BL
}

}  // namespace

int dg_boundary_check(const char* who, float boundary_coef, const float* coef, int n, int C) {
  DGCHECK(dg_class_count_check(who, C));
  if (!(boundary_coef >= 0.f) || boundary_coef > FLT_MAX) {
    dg_set_error("%s: boundary_coef is %g (finite and >= 0)", who, (double)boundary_coef);
    return DG_ERR_ARG;
  }
  return coef ? dg_class_coef_check(who, coef, n, C) : DG_OK;
}

int dg_signed_distance_check(const char* who, long n, int H, int W, int C, double sy, double sx, double inside_offset) {
  DGCHECK(dg_class_count_check(who, C));
  if (n < 1 || H < 1 || W < 1 || H > DG_EDT_MAX_DIM || W > DG_EDT_MAX_DIM || n * (long)H * W >= (1L << 31)) {
    dg_set_error("%s: n=%ld H=%d W=%d (n >= 1, H and W in 1..%d as the distance transform takes them, n*H*W < 2^31)",
                 who, n, H, W, DG_EDT_MAX_DIM);
    return DG_ERR_ARG;
  }
  // one workgroup of 256 per row (row pass) and per 64 x 16 tile of a map (column pass): a grid stays below 2^32 threads
  const long tiles = (long)cdiv(W, DG_EDT_COLS) * cdiv(H, DG_EDT_TILE_ROWS) * n * C;
  if (n * (long)H >= (1L << 24) || tiles >= (1L << 24)) {
    dg_set_error("%s: n=%ld slices of %d x %d with %d classes: n*H (%ld) and the 64 x 16 tiles of all maps (%ld) must "
                 "each stay below 2^24, one workgroup each", who, n, H, W, C, n * (long)H, tiles);
    return DG_ERR_ARG;
  }
  if (!isfinite(sy) || !(sy > 0.0) || !isfinite(sx) || !(sx > 0.0)) {
    dg_set_error("%s: the spacings must be finite and > 0 (sy=%g sx=%g)", who, sy, sx);
    return DG_ERR_ARG;
  }
  const double lim = sy < sx ? sy : sx;
  if (!(inside_offset >= 0.0) || !(inside_offset <= lim)) {
    dg_set_error("%s: inside_offset is %g (in [0, min(sy, sx)] = [0, %g])", who, inside_offset, lim);
    return DG_ERR_ARG;
  }
  return DG_OK;
}

size_t dg_signed_distance_scratch_bytes(long n, int H, int W, int C) {
  return dg_edt_round8((size_t)n * (size_t)H * (size_t)W * (size_t)C * sizeof(unsigned short));
}

int dg_signed_distance(DgLabels lab, int ignore_code, long n, int H, int W, int C, unsigned class_mask, double sy,
                       double sx, double inside_offset, float* phi, void* scratch, size_t scratch_bytes,
                       hipStream_t st) {
  DGCHECK(dg_signed_distance_check("dg_signed_distance", n, H, W, C, sy, sx, inside_offset));
  if (!phi || ((uintptr_t)phi & 3) || (!lab.onehot == !lab.codes) || ((uintptr_t)lab.onehot & 3)) {
    dg_set_error("dg_signed_distance: null or misaligned phi, or not exactly one of onehot and codes (4-byte aligned)");
    return DG_ERR_ARG;
  }
  if (ignore_code < -1 || ignore_code > 255) {
    dg_set_error("dg_signed_distance: ignore code %d (-1 for none, else a byte value 0..255)", ignore_code);
    return DG_ERR_ARG;
  }
  BlClasses cls;
  cls.n = 0;
  for (int k = 0; k < DG_MAX_CLASSES; ++k) {
    cls.k[k] = 0;
    if (k < C && (class_mask >> k & 1u)) cls.k[cls.n++] = (unsigned char)k;
  }
  if (cls.n == 0) { dg_set_error("dg_signed_distance: every class is switched off"); return DG_ERR_ARG; }
  if (!scratch || ((uintptr_t)scratch & 1) || scratch_bytes < dg_signed_distance_scratch_bytes(n, H, W, cls.n)) {
    dg_set_error("dg_signed_distance: scratch of %zu bytes, the launches need %zu", scratch ? scratch_bytes : (size_t)0,
                 dg_signed_distance_scratch_bytes(n, H, W, cls.n));
    return DG_ERR_ARG;
  }
  unsigned short* g = (unsigned short*)scratch;
  const dim3 grows((unsigned)(n * H));
  if (lab.onehot)
    hipLaunchKernelGGL(bl_rows_kernel<LBL_ONEHOT>, grows, dim3(256), 0, st, lab.onehot, lab.codes, ignore_code, g, H, W,
                       C, cls);
  else
    hipLaunchKernelGGL(bl_rows_kernel<LBL_CODES>, grows, dim3(256), 0, st, lab.onehot, lab.codes, ignore_code, g, H, W,
                       C, cls);
  const int col_tiles = cdiv(W, DG_EDT_COLS), row_tiles = cdiv(H, DG_EDT_TILE_ROWS);
  const long tiles = (long)col_tiles * row_tiles * n * cls.n;
  // the squared spacings as evaluate.surface_distances forms its weights
  hipLaunchKernelGGL(bl_cols_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (const unsigned short*)g, phi, H, W, C,
                     cls, col_tiles, row_tiles, sx * sx, sy * sy, inside_offset);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

size_t dg_boundary_scratch(long P) { return (size_t)t_nblk((size_t)P, BL_MAX_BLOCKS); }

int dg_boundary_loss(const float* probs, const float* phi, DgLabels lab, int ignore_code, const float* class_coef,
                     float boundary_coef, const unsigned long long* counts, float* dz, DgBoundaryDev* out, long P, int C,
                     double* scratch, size_t scratch_doubles, hipStream_t st) {
  DGCHECK(dg_boundary_check("dg_boundary_loss", boundary_coef, class_coef, C, C));
  DGCHECK(dg_loss_operands_check("dg_boundary_loss", probs, "phi", phi, lab, ignore_code, dz, P, true, C));
  if (!class_coef || !out || ((uintptr_t)out & 7) || ((uintptr_t)counts & 7)) {
    dg_set_error("dg_boundary_loss: null class_coef, or null or misaligned out or counts");
    return DG_ERR_ARG;
  }
  const int nb = t_nblk((size_t)P, BL_MAX_BLOCKS);
  if (!scratch || ((uintptr_t)scratch & 7) || scratch_doubles < (size_t)nb) {
    dg_set_error("dg_boundary_loss: scratch of %zu doubles, the launches need %d", scratch ? scratch_doubles : (size_t)0, nb);
    return DG_ERR_ARG;
  }
  BlCoef co;
  for (int k = 0; k < DG_MAX_CLASSES; ++k) co.c[k] = k < C ? class_coef[k] : 0.f;
  co.boundary_coef = boundary_coef;
#define DG_BLC(N)                                                                                              \
  bl_loss_launch<N>(lab.onehot != nullptr, nb, st, probs, phi, lab.onehot, lab.codes, ignore_code, co, counts, dz, \
                    scratch, P)
  DG_FOR_CLASS_COUNT(C, DG_BLC)
#undef DG_BLC
  hipLaunchKernelGGL(bl_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)scratch, nb, counts, P, out);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
