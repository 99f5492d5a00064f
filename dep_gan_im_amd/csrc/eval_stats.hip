// Per-draw statistics of the stochastic predictions (evaluate.predict_stats): what the n_repeat noise draws say beyond
// their mean, and test-time augmentation.  Takes the place of depgan_eval_accumulate[_channels] (ops.hip,
// eval_uresnet.hip) when more than the mean is wanted; those kernels are untouched.
//
//   per draw (eval_accumulate_stats_kernel), pixel t of the original frame, channel c:
//     u_c = pred[t, c]                                   or, with a parameter row, the bilinear sample of the draw's
//                                                        prediction at the row's source coordinate (augment.hip's
//                                                        float32 statements without the gain / offset statement)
//     v_c = u_c * mask[t]                                float32 product (mask NULL: v_c = u_c)
//     sum[t, c]   += (double)v_c                         the bits of eval_accumulate_channels_kernel
//     sumsq[t, c] += (double)v_c * (double)v_c           the product is exact in double, the add rounds
//     ent_sum[t]  += ((0 - t_0) - t_1) - ...             t_c = v_c > 0 ? (double)v_c * log((double)v_c) : 0.0
//     votes[t, argmax_c v_c] += 1                        first maximum, a NaN counts as the maximum
//     count[t]    += 1
//   once (eval_finish_stats_kernel): mean, variance, expected entropy, entropy of the mean, mutual information.
//
// Memory-bound: 4C + 4 bytes read and 16C + 8 + 1 + 1 bytes read and written back per pixel and draw.  One thread per
// output pixel over its C channels, consecutive lanes walk ox; a thread owns its pixel's state, so there are no
// atomics and no LDS.  Tap addressing never leaves the sample (a coordinate is compared and clamped as a float before
// it becomes an integer).
#include "common.h"

#include "model.h"

// every float and double operation below is rounded on its own, as NumPy's statement sequence is
#pragma clang fp contract(off)

namespace {

// augment.hip's tap: f is an integral-valued float (or +-inf / NaN).  Returns the index clamped into [0, n); *in says
// whether f itself was inside (false for NaN, which clamps to 0).
__device__ __forceinline__ int tap(float f, int n, bool* in) {
  const float hi = (float)(n - 1);                   // exact: n <= 2^24 (checked by the entry)
  *in = f >= 0.0f && f <= hi;
  return (int)fminf(fmaxf(f, 0.0f), hi);
}

// t = v > 0 ? v * log(v) : 0 -- 0 for a zero, a negative value and a NaN
__device__ __forceinline__ double plogp(double v) { return v > 0.0 ? v * log(v) : 0.0; }

struct StatArgs {
  const float* pred;
  const float* mask;
  const float* params;
  double* sum;
  double* sumsq;
  double* ent_sum;
  unsigned char* votes;
  unsigned char* count;
  long total;          // n * H * W
  int H, W;
  int valid;           // border: 0 edge, 1 valid
};

// grid ceil(total / 256), block 256, thread = output pixel.  TTA: a.params is given.
template <int C, bool TTA>
__global__ __launch_bounds__(256) void eval_accumulate_stats_kernel(const StatArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.total) return;
  float v[C];
  if (!TTA) {
    const float* p = a.pred + (size_t)t * C;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = p[c];
  } else {
    const int H = a.H, W = a.W;
    const unsigned HW = (unsigned)H * (unsigned)W;     // <= 2^31 - 1 (checked by the entry)
    const long i = a.total <= 0xFFFFFFFFL ? (long)((unsigned)t / HW) : t / HW;
    const unsigned pix = (unsigned)(t - i * HW);
    const int oy = (int)(pix / (unsigned)W), ox = (int)(pix - (unsigned)oy * (unsigned)W);
    const float* p = a.params + (size_t)i * DEPGAN_AUG_NPARAM;
    const float a00 = p[0], a01 = p[1], a02 = p[2], a10 = p[3], a11 = p[4], a12 = p[5];
    const float fyo = (float)oy, fxo = (float)ox;
    const float sy = (a00 * fyo + a01 * fxo) + a02;
    const float sx = (a10 * fyo + a11 * fxo) + a12;
    const float y0 = floorf(sy), x0 = floorf(sx);
    const float fy = sy - y0, fx = sx - x0;
    const float gy = 1.0f - fy, gx = 1.0f - fx;
    bool iy0, iy1, ix0, ix1;
    const int ty0 = tap(y0, H, &iy0), ty1 = tap(y0 + 1.0f, H, &iy1);
    const int tx0 = tap(x0, W, &ix0), tx1 = tap(x0 + 1.0f, W, &ix1);
    // valid: the draw takes part only where every tap that carries weight lies inside the prediction
    if (a.valid && !(iy0 && ix0 && (fy == 0.0f || iy1) && (fx == 0.0f || ix1))) return;
    const float* src = a.pred + (size_t)i * HW * C;
    const float* r0 = src + (size_t)ty0 * W * C;
    const float* r1 = src + (size_t)ty1 * W * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {                    // clamped addresses: always inside the sample
      const float v00 = r0[(size_t)tx0 * C + c], v01 = r0[(size_t)tx1 * C + c];
      const float v10 = r1[(size_t)tx0 * C + c], v11 = r1[(size_t)tx1 * C + c];
      const float top = v00 * gx + v01 * fx;
      const float bot = v10 * gx + v11 * fx;
      v[c] = top * gy + bot * fy;
    }
  }
  if (a.mask) {
    const float m = a.mask[t];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = __fmul_rn(v[c], m);
  }
  {
    double* s = a.sum + (size_t)t * C;
    double r[C];
#pragma unroll
    for (int c = 0; c < C; ++c) r[c] = s[c];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = __dadd_rn(r[c], (double)v[c]);
  }
  if (a.sumsq) {
    double* s = a.sumsq + (size_t)t * C;
    double r[C];
#pragma unroll
    for (int c = 0; c < C; ++c) r[c] = s[c];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = r[c] + (double)v[c] * (double)v[c];
  }
  if (a.ent_sum) {
    double h = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) h = h - plogp((double)v[c]);
    a.ent_sum[t] = a.ent_sum[t] + h;
  }
  if (a.votes) {
    // np.argmax: the first maximum; a NaN counts as the maximum (its first occurrence wins)
    int lab = 0;
    float best = v[0];
    bool open = best == best;
#pragma unroll
    for (int c = 1; c < C; ++c) {
      if (open) {
        if (v[c] != v[c]) {
          lab = c;
          open = false;
        } else if (v[c] > best) {
          best = v[c];
          lab = c;
        }
      }
    }
    unsigned char* q = a.votes + (size_t)t * C + lab;
    *q = (unsigned char)(*q + 1);
  }
  if (a.count) a.count[t] = (unsigned char)(a.count[t] + 1);
}

// grid ceil(npix / 256), block 256, thread = pixel.  In place: sum -> mean, sumsq -> var, ent_sum -> expected entropy.
// The rows have a constant length, so their loads and stores are wide.
template <int C>
__global__ __launch_bounds__(256) void eval_finish_stats_kernel(double* __restrict__ sum, double* __restrict__ sumsq,
                                                                double* __restrict__ ent_sum,
                                                                const unsigned char* __restrict__ count,
                                                                double* __restrict__ entropy,
                                                                double* __restrict__ mutual_info, long npix,
                                                                int n_draws, int ddof) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= npix) return;
  const int R = count ? (int)count[t] : n_draws;
  double* s = sum + (size_t)t * C;
  double* q = sumsq ? sumsq + (size_t)t * C : nullptr;
  if (R == 0) {                                      // no draw reached this pixel
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = 0.0;
    if (q) {
#pragma unroll
      for (int c = 0; c < C; ++c) q[c] = 0.0;
    }
    if (ent_sum) ent_sum[t] = 0.0;
    if (entropy) entropy[t] = 0.0;
    if (mutual_info) mutual_info[t] = 0.0;
    return;
  }
  const double Rd = (double)R, dof = Rd - (double)ddof;
  const double bessel = dof == 0.0 ? 0.0 : Rd / dof;
  double m[C];
#pragma unroll
  for (int c = 0; c < C; ++c) m[c] = s[c];
#pragma unroll
  for (int c = 0; c < C; ++c) m[c] = __ddiv_rn(m[c], Rd);      // the bits of eval_divide_kernel
#pragma unroll
  for (int c = 0; c < C; ++c) s[c] = m[c];
  if (q) {
    double v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = q[c];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double d = v[c] / Rd - m[c] * m[c];
      v[c] = dof == 0.0 ? 0.0 : (d < 0.0 ? 0.0 : d) * bessel;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = v[c];
  }
  double e = 0.0;
  if (ent_sum) {
    e = ent_sum[t] / Rd;
    ent_sum[t] = e;
  }
  if (entropy || mutual_info) {
    double h = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) h = h - plogp(m[c]);
    if (entropy) entropy[t] = h;
    if (mutual_info) {
      const double d = h - e;
      mutual_info[t] = d < 0.0 ? 0.0 : d;
    }
  }
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || !na || !nb) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// true when one of the `ns` state ranges overlaps one of the `ni` input ranges or another state range
bool any_overlap(const void* const* st, const size_t* st_bytes, int ns, const void* const* in, const size_t* in_bytes,
                 int ni) {
  for (int j = 0; j < ns; ++j) {
    for (int k = 0; k < ni; ++k)
      if (overlaps(st[j], st_bytes[j], in[k], in_bytes[k])) return true;
    for (int k = j + 1; k < ns; ++k)
      if (overlaps(st[j], st_bytes[j], st[k], st_bytes[k])) return true;
  }
  return false;
}

template <int C>
void launch(int blocks, hipStream_t st, const StatArgs& a) {
  if (a.params) hipLaunchKernelGGL((eval_accumulate_stats_kernel<C, true>), dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((eval_accumulate_stats_kernel<C, false>), dim3(blocks), dim3(256), 0, st, a);
}

}  // namespace

extern "C" {

static_assert(DEPGAN_MAX_HEAD_CLASSES == 8, "depgan_eval_accumulate_stats' switch covers 1..8 channels");

int depgan_eval_accumulate_stats(const float* pred_dev, const float* mask_dev, const float* params_dev, int border,
                                 int n, int H, int W, int C, double* sum_dev, double* sumsq_dev, double* ent_sum_dev,
                                 unsigned char* votes_dev, unsigned char* count_dev, void* stream) {
  if (n < 1 || H < 1 || W < 1 || C < 1 || C > DEPGAN_MAX_HEAD_CLASSES || (border != 0 && border != 1) || !pred_dev ||
      !sum_dev || ((ent_sum_dev || votes_dev) && C < 2)) {
    dg_set_error("eval_accumulate_stats: bad argument (n=%d H=%d W=%d C=%d border=%d)", n, H, W, C, border);
    return DG_ERR_ARG;
  }
  if (H > (1 << 24) || W > (1 << 24) || (long)H * W > 0x7FFFFFFFL) {
    dg_set_error("eval_accumulate_stats: image too large (H=%d W=%d)", H, W);
    return DG_ERR_ARG;
  }
  const size_t npix = (size_t)n * H * W;
  if ((npix + 255) / 256 > 0x7FFFFFFFul) {
    dg_set_error("eval_accumulate_stats: batch too large for one launch (n=%d H=%d W=%d)", n, H, W);
    return DG_ERR_ARG;
  }
  const void* st[5] = {sum_dev, sumsq_dev, ent_sum_dev, votes_dev, count_dev};
  const size_t st_bytes[5] = {npix * C * 8, npix * C * 8, npix * 8, npix * C, npix};
  const void* in[3] = {pred_dev, mask_dev, params_dev};
  const size_t in_bytes[3] = {npix * C * 4, npix * 4, (size_t)n * DEPGAN_AUG_NPARAM * 4};
  if (any_overlap(st, st_bytes, 5, in, in_bytes, 3)) {
    dg_set_error("eval_accumulate_stats: a state range overlaps an input range or another state range");
    return DG_ERR_ARG;
  }
  StatArgs a;
  a.pred = pred_dev;
  a.mask = mask_dev;
  a.params = params_dev;
  a.sum = sum_dev;
  a.sumsq = sumsq_dev;
  a.ent_sum = ent_sum_dev;
  a.votes = votes_dev;
  a.count = count_dev;
  a.total = (long)npix;
  a.H = H;
  a.W = W;
  a.valid = border;
  const int blocks = (int)((npix + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  switch (C) {
    case 1: launch<1>(blocks, s, a); break;
    case 2: launch<2>(blocks, s, a); break;
    case 3: launch<3>(blocks, s, a); break;
    case 4: launch<4>(blocks, s, a); break;
    case 5: launch<5>(blocks, s, a); break;
    case 6: launch<6>(blocks, s, a); break;
    case 7: launch<7>(blocks, s, a); break;
    default: launch<8>(blocks, s, a); break;
  }
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

int depgan_eval_finish_stats(double* sum_dev, double* sumsq_dev, double* ent_sum_dev, const unsigned char* count_dev,
                             double* entropy_dev, double* mutual_info_dev, long npix, int C, int n_draws, int ddof,
                             void* stream) {
  if (!sum_dev || npix < 1 || C < 1 || C > DEPGAN_MAX_HEAD_CLASSES || n_draws < 1 || n_draws > 255 ||
      (ddof != 0 && ddof != 1) || ((ent_sum_dev || entropy_dev || mutual_info_dev) && C < 2) ||
      (mutual_info_dev && !ent_sum_dev)) {
    dg_set_error("eval_finish_stats: bad argument (npix=%ld C=%d n_draws=%d ddof=%d)", npix, C, n_draws, ddof);
    return DG_ERR_ARG;
  }
  const size_t np_ = (size_t)npix;
  if ((np_ + 255) / 256 > 0x7FFFFFFFul) {
    dg_set_error("eval_finish_stats: too many pixels for one launch (npix=%ld)", npix);
    return DG_ERR_ARG;
  }
  const void* st[5] = {sum_dev, sumsq_dev, ent_sum_dev, entropy_dev, mutual_info_dev};
  const size_t st_bytes[5] = {np_ * C * 8, np_ * C * 8, np_ * 8, np_ * 8, np_ * 8};
  const void* in[1] = {count_dev};
  const size_t in_bytes[1] = {np_};
  if (any_overlap(st, st_bytes, 5, in, in_bytes, 1)) {
    dg_set_error("eval_finish_stats: two of the ranges overlap");
    return DG_ERR_ARG;
  }
#define DG_FINISH(K)                                                                                               \
  case K:                                                                                                          \
    hipLaunchKernelGGL(eval_finish_stats_kernel<K>, dim3((unsigned)((np_ + 255) / 256)), dim3(256), 0,             \
                       (hipStream_t)stream, sum_dev, sumsq_dev, ent_sum_dev, count_dev, entropy_dev,               \
                       mutual_info_dev, npix, n_draws, ddof);                                                      \
    break;
  switch (C) {
    DG_FINISH(1) DG_FINISH(2) DG_FINISH(3) DG_FINISH(4) DG_FINISH(5) DG_FINISH(6) DG_FINISH(7) DG_FINISH(8)
  }
#undef DG_FINISH
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
