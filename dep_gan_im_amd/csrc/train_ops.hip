// Learning-phase-1 operators (see train_ops.h).  All HBM-bound: 16-byte accesses over the channel
// axis, block reductions through LDS, deterministic second passes.
#include "train_ops.h"

#include <float.h>

#include "epilogue.h"
#include "softmax_row.h"

__device__ __forceinline__ float t_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ float t_block_sum(float v, float* sh4) {
  v = t_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}
static inline int t_nblk(size_t n, int cap) {
  size_t b = (n + 255) / 256;
  return (int)(b > (size_t)cap ? cap : (b < 1 ? 1 : b));
}

// MODE 0: (sum x, -)   MODE 1: (sum (x-m)^2, -)   MODE 2: (sum d, sum d*(x-m))   [v = d, w = x]
// FLAT: both views are pixel-contiguous (sY == W*sX, sB == H*sY), so pixel q sits at q*sX: no divisions in the loop.
template <int MODE, bool FLAT>
__global__ void colsum2_partial(TView v, TView w, const float* __restrict__ m, long npix, int H, int W, int C4,
                                float* __restrict__ part, int pixPerBlock) {
  extern __shared__ __attribute__((aligned(16))) float sh[];  // [256][8]
  const int LP = C4, PP = 256 / LP;
  const int lp = threadIdx.x % LP, pp = threadIdx.x / LP;
  const long q0 = (long)blockIdx.x * pixPerBlock, q1 = min(q0 + pixPerBlock, npix);
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  if (pp < PP) {
    f32x4 mv = {0.f, 0.f, 0.f, 0.f};
    if (MODE >= 1) mv = *reinterpret_cast<const f32x4*>(m + lp * 4);
    for (long q = q0 + pp; q < q1; q += PP) {
      long ov, ow;
      if (FLAT) {
        ov = q * v.sX;
        ow = q * w.sX;
      } else {
        const int x = (int)(q % W);
        const long r = q / W;
        const int y = (int)(r % H);
        const int b = (int)(r / H);
        ov = view_off(v, b, y, x);
        ow = (MODE == 2) ? view_off(w, b, y, x) : 0;
      }
      const f32x4 xv = *reinterpret_cast<const f32x4*>(v.p + ov + lp * 4);
      if (MODE == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a0[k] += xv[k];
      } else if (MODE == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float d = xv[k] - mv[k];
          a0[k] = fmaf(d, d, a0[k]);
        }
      } else {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w.p + ow + lp * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          a0[k] += xv[k];
          a1[k] = fmaf(xv[k], wv[k] - mv[k], a1[k]);
        }
      }
    }
  }
  *reinterpret_cast<f32x4*>(sh + threadIdx.x * 8) = a0;
  *reinterpret_cast<f32x4*>(sh + threadIdx.x * 8 + 4) = a1;
  __syncthreads();
  for (int idx = threadIdx.x; idx < LP * 8; idx += 256) {
    const int l = idx / 8, k = idx % 8;
    float s = 0.f;
    for (int j = 0; j < PP; ++j) s += sh[(j * LP + l) * 8 + k];
    const int C = C4 * 4;
    part[((size_t)blockIdx.x * 2 + (k >> 2)) * C + l * 4 + (k & 3)] = s;
  }
}
// out[j][c] = scale * sum_blk part[blk][j][c], one block per (c, j)
__global__ void colsum2_final(const float* __restrict__ part, int nb, int C, float scale, float* __restrict__ out0,
                              float* __restrict__ out1) {
  __shared__ float sh4[4];
  const int c = blockIdx.x, j = blockIdx.y;
  float s = 0.f;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) s += part[((size_t)b * 2 + j) * C + c];
  s = t_block_sum(s, sh4);
  if (threadIdx.x == 0) (j == 0 ? out0 : out1)[c] = s * scale;
}

// grid of the per-channel reductions over pixels: at most 1024 blocks of ppb pixels each (the last one may be short)
static void t_pix_grid(long npix, int* nb_out, int* ppb_out) {
  int nb = (int)((npix + 255) / 256);
  if (nb > 1024) nb = 1024;
  const int ppb = (int)((npix + nb - 1) / nb);
  *nb_out = (int)((npix + ppb - 1) / ppb);
  *ppb_out = ppb;
}
size_t dg_col_moments_scratch(int B, int H, int W, int C) {
  int nb, ppb;
  t_pix_grid((long)B * H * W, &nb, &ppb);
  return (size_t)nb * 3 * C;
}
size_t dg_colsum_pair_scratch(int B, int H, int W, int C) {
  int nb, ppb;
  t_pix_grid((long)B * H * W, &nb, &ppb);
  return (size_t)nb * 2 * C;
}

static int colsum2_launch(int mode, TView v, TView w, const float* m, int B, int H, int W, int C, float scale,
                          float* out0, float* out1, float* scratch, size_t scratch_floats, hipStream_t st) {
  if ((C % 4) || C > 1024 || B < 1 || H < 1 || W < 1) {
    dg_set_error("train colsum: C must be a multiple of 4 and <= 1024, B H W >= 1 (got %d %d %d %d)", B, H, W, C);
    return DG_ERR_ARG;
  }
  const long npix = (long)B * H * W;
  int nb, ppb;
  t_pix_grid(npix, &nb, &ppb);
  if ((size_t)nb * 2 * C > scratch_floats) {
    dg_set_error("train colsum: scratch holds %zu floats, %d blocks x 2 x %d channels need %zu", scratch_floats, nb, C,
                 (size_t)nb * 2 * C);
    return DG_ERR_ARG;
  }
  const size_t lds = 256 * 8 * sizeof(float);
  auto is_flat = [&](const TView& t) { return !t.p || (t.sY == (long)W * t.sX && t.sB == (long)H * t.sY); };
  const bool flat = is_flat(v) && is_flat(w);
#define DG_CS2(MODE)                                                                                                  \
  do {                                                                                                                 \
    if (flat)                                                                                                          \
      hipLaunchKernelGGL((colsum2_partial<MODE, true>), dim3(nb), dim3(256), lds, st, v, w, m, npix, H, W, C / 4,      \
                         scratch, ppb);                                                                                \
    else                                                                                                               \
      hipLaunchKernelGGL((colsum2_partial<MODE, false>), dim3(nb), dim3(256), lds, st, v, w, m, npix, H, W, C / 4,     \
                         scratch, ppb);                                                                                \
  } while (0)
  if (mode == 0) DG_CS2(0);
  else if (mode == 1) DG_CS2(1);
  else DG_CS2(2);
#undef DG_CS2
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(colsum2_final, dim3(C, out1 ? 2 : 1), dim3(256), 0, st, scratch, nb, C, scale, out0, out1);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

// Batch mean and (biased) variance per channel in ONE pass over the tensor (round 3; was two: mean, then centred squares).
// Plain E[x^2] - E[x]^2 loses the variance of channels with |mean| >> sigma, so every block sums (x - s) and (x - s)^2
// around a shift s of its own -- the value of its first pixel, a sample of the very distribution, so |mean_b - s| is a
// few sigma and the block's subtraction M2_b = S2 - S1^2 / n_b is benign -- and the per-channel finish combines the
// blocks' (n_b, mean_b, M2_b) with the parallel-variance formula (Chan et al.) in double precision:
//   mean = sum n_b mean_b / N,   M2 = sum M2_b + sum n_b (mean_b - mean)^2,   var = M2 / N.
template <bool FLAT>
__global__ void moments_partial(TView v, long npix, int H, int W, int C4, float* __restrict__ part, int pixPerBlock) {
  extern __shared__ __attribute__((aligned(16))) float sh[];  // [256][8]
  const int LP = C4, PP = 256 / LP;
  const int lp = threadIdx.x % LP, pp = threadIdx.x / LP;
  const long q0 = (long)blockIdx.x * pixPerBlock, q1 = min(q0 + pixPerBlock, npix);
  auto off = [&](long q) -> long {
    if (FLAT) return q * v.sX;
    const int x = (int)(q % W);
    const long r = q / W;
    return view_off(v, (int)(r / H), (int)(r % H), x);
  };
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f}, sv = {0.f, 0.f, 0.f, 0.f};
  if (pp < PP) {
    sv = *reinterpret_cast<const f32x4*>(v.p + off(q0) + lp * 4);          // the block's shift: its first pixel
    for (long q = q0 + pp; q < q1; q += PP) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(v.p + off(q) + lp * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = xv[k] - sv[k];
        a0[k] += d;
        a1[k] = fmaf(d, d, a1[k]);
      }
    }
  }
  *reinterpret_cast<f32x4*>(sh + threadIdx.x * 8) = a0;
  *reinterpret_cast<f32x4*>(sh + threadIdx.x * 8 + 4) = a1;
  __syncthreads();
  const int C = C4 * 4;
  for (int idx = threadIdx.x; idx < LP * 8; idx += 256) {
    const int l = idx / 8, k = idx % 8;
    float s = 0.f;
    for (int j = 0; j < PP; ++j) s += sh[(j * LP + l) * 8 + k];
    part[((size_t)blockIdx.x * 3 + (k >> 2)) * C + l * 4 + (k & 3)] = s;
  }
  if (pp == 0) *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.x * 3 + 2) * C + lp * 4) = sv;
}
// one block per channel: Chan's combination of the blocks' (n_b, mean_b, M2_b), double precision, fixed order
__global__ void moments_final(const float* __restrict__ part, int nb, int C, long npix, int pixPerBlock,
                              float* __restrict__ mean, float* __restrict__ var) {
  __shared__ double shd[256];
  const int c = blockIdx.x;
  auto nof = [&](int b) -> double {
    const long q0 = (long)b * pixPerBlock;
    const long q1 = q0 + pixPerBlock < npix ? q0 + pixPerBlock : npix;
    return (double)(q1 - q0);
  };
  auto block_sum = [&](double x) -> double {
    shd[threadIdx.x] = x;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) shd[threadIdx.x] += shd[threadIdx.x + o];
      __syncthreads();
    }
    const double r = shd[0];
    __syncthreads();
    return r;
  };
  double sm = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) {
    const double s1 = part[((size_t)b * 3 + 0) * C + c], sh_ = part[((size_t)b * 3 + 2) * C + c];
    sm += nof(b) * sh_ + s1;                       // n_b mean_b = n_b s_b + S1_b
  }
  const double mu = block_sum(sm) / (double)npix;
  double m2 = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) {
    const double n = nof(b);
    const double s1 = part[((size_t)b * 3 + 0) * C + c], s2 = part[((size_t)b * 3 + 1) * C + c];
    const double mb = (double)part[((size_t)b * 3 + 2) * C + c] + s1 / n;
    m2 += (s2 - s1 * s1 / n) + n * (mb - mu) * (mb - mu);
  }
  const double M2 = block_sum(m2);
  if (threadIdx.x == 0) {
    mean[c] = (float)mu;
    var[c] = (float)(M2 / (double)npix);
  }
}

int dg_col_moments(TView v, int B, int H, int W, int C, float* mean, float* var, float* scratch, size_t scratch_floats,
                   hipStream_t st) {
  if ((C % 4) || C > 1024 || B < 1 || H < 1 || W < 1) {
    dg_set_error("train moments: C must be a multiple of 4 and <= 1024, B H W >= 1 (got %d %d %d %d)", B, H, W, C);
    return DG_ERR_ARG;
  }
  const long npix = (long)B * H * W;
  int nb, ppb;
  t_pix_grid(npix, &nb, &ppb);
  if ((size_t)nb * 3 * C > scratch_floats) {
    dg_set_error("train moments: scratch holds %zu floats, %d blocks x 3 x %d channels need %zu", scratch_floats, nb, C,
                 (size_t)nb * 3 * C);
    return DG_ERR_ARG;
  }
  const size_t lds = 256 * 8 * sizeof(float);
  const bool flat = (v.sY == (long)W * v.sX && v.sB == (long)H * v.sY);
  if (flat)
    hipLaunchKernelGGL((moments_partial<true>), dim3(nb), dim3(256), lds, st, v, npix, H, W, C / 4, scratch, ppb);
  else
    hipLaunchKernelGGL((moments_partial<false>), dim3(nb), dim3(256), lds, st, v, npix, H, W, C / 4, scratch, ppb);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(moments_final, dim3(C), dim3(256), 0, st, scratch, nb, C, npix, ppb, mean, var);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
int dg_colsum_pair(TView d, TView x, const float* mean, int B, int H, int W, int C, float* sums, float* scratch,
                   size_t scratch_floats, hipStream_t st) {
  return colsum2_launch(2, d, x, mean, B, H, W, C, 1.0f, sums, sums + C, scratch, scratch_floats, st);
}

__global__ void bn_train_prepare_kernel(const float* gamma, const float* beta, const float* mean, const float* var,
                                        float eps, float momentum, float corr, float* mm, float* mv, float* s,
                                        float* t, float* rstd, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float r = 1.0f / sqrtf(var[c] + eps);
  const float sc = gamma[c] * r;
  s[c] = sc;
  t[c] = beta[c] - mean[c] * sc;
  rstd[c] = r;
  if (mm) {
    mm[c] = mm[c] * momentum + mean[c] * (1.0f - momentum);
    mv[c] = mv[c] * momentum + var[c] * corr * (1.0f - momentum);
  }
}
int dg_bn_train_prepare(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                        float momentum, float corr, float* moving_mean, float* moving_var, float* s, float* t,
                        float* rstd, int C, hipStream_t st) {
  hipLaunchKernelGGL(bn_train_prepare_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, gamma, beta, mean, var, eps,
                     momentum, corr, moving_mean, moving_var, s, t, rstd, C);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

__device__ __forceinline__ unsigned hash_u32(unsigned i, unsigned seed) {
  unsigned x = (i * 0x9E3779B1u) ^ seed;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// FLAT: every view is pixel-contiguous, so pixel q of view t sits at q * t.sX -- 32-bit index arithmetic only.
// No contraction: every step below is one correctly rounded operation (tests/test_gpu_train_ops.py replays it bitwise).
// __fmul_rn / __fadd_rn do not ensure that: in HIP they are plain * and +, and under the default -ffp-contract=fast
// __fadd_rn(__fmul_rn(x, s), t) compiled to one FMA.  The pragma covers the operators written in this body.
template <bool FLAT>
__global__ void affine_act_kernel(const AffineActArgs a, unsigned drop_thr, float drop_scale) {
#pragma clang fp contract(off)
  const int C4 = a.C / 4;
  const size_t total = (size_t)a.B * a.H * a.W * C4;
  const unsigned HW = (unsigned)a.H * (unsigned)a.W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int c, b;
    long o_in, o_out, o_pre, o_res;
    if (FLAT) {
      const unsigned pix = (unsigned)(i / (unsigned)C4);
      c = (int)((unsigned)i - pix * (unsigned)C4) * 4;
      b = (int)(pix / HW);
      o_in = (long)pix * a.in.sX;
      o_out = (long)pix * a.out.sX;
      o_pre = (long)pix * a.out_pre.sX;
      o_res = (long)pix * a.res.sX;
    } else {
      size_t q = i;
      c = (int)(q % C4) * 4;
      q /= C4;
      const int x = (int)(q % a.W);
      q /= a.W;
      const int y = (int)(q % a.H);
      b = (int)(q / a.H);
      o_in = view_off(a.in, b, y, x);
      o_out = view_off(a.out, b, y, x);
      o_pre = a.out_pre.p ? view_off(a.out_pre, b, y, x) : 0;
      o_res = a.res.p ? view_off(a.res, b, y, x) : 0;
    }
    f32x4 v = *reinterpret_cast<const f32x4*>(a.in.p + o_in + c);
    const f32x4 sv = *reinterpret_cast<const f32x4*>(a.s + c);
    const f32x4 tv = *reinterpret_cast<const f32x4*>(a.t + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = v[k] * sv[k] + tv[k];
    if (a.out_pre.p) *reinterpret_cast<f32x4*>(a.out_pre.p + o_pre + c) = v;
    if (a.film_mul) {
      const f32x4 fm = *reinterpret_cast<const f32x4*>(a.film_mul + (size_t)b * a.film_ld + c);
      const f32x4 fa = *reinterpret_cast<const f32x4*>(a.film_add + (size_t)b * a.film_ld + c);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = film_preact(v[k], fm[k], fa[k]);
    }
    if (a.relu) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
    }
    if (a.drop_seed) {
      const unsigned base = (unsigned)(i * 4);  // NHWC linear index of element 0 (dense tensor)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (hash_u32(base + k, a.drop_seed) >= drop_thr) ? v[k] * drop_scale : 0.f;
    }
    if (a.res.p) {
      const f32x4 r = *reinterpret_cast<const f32x4*>(a.res.p + o_res + c);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] += r[k];
    }
    *reinterpret_cast<f32x4*>(a.out.p + o_out + c) = v;
  }
}
int dg_affine_act(const AffineActArgs& a, hipStream_t st) {
  if (a.C % 4) { dg_set_error("dg_affine_act: C %% 4 != 0"); return DG_ERR_ARG; }
  const size_t total = (size_t)a.B * a.H * a.W * (a.C / 4);
  const unsigned thr = (unsigned)(a.drop_rate * 4294967296.0);
  auto is_flat = [&](const TView& t) { return !t.p || (t.sY == (long)a.W * t.sX && t.sB == (long)a.H * t.sY); };
  const bool flat = is_flat(a.in) && is_flat(a.out) && is_flat(a.out_pre) && is_flat(a.res) &&
                    (size_t)a.B * a.H * a.W < (1ull << 31);
  if (flat)
    hipLaunchKernelGGL(affine_act_kernel<true>, dim3(t_nblk(total, 8192)), dim3(256), 0, st, a, thr,
                       1.0f / (1.0f - a.drop_rate));
  else
    hipLaunchKernelGGL(affine_act_kernel<false>, dim3(t_nblk(total, 8192)), dim3(256), 0, st, a, thr,
                       1.0f / (1.0f - a.drop_rate));
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

__global__ void bn_bwd_coeffs_kernel(const float* sums, const float* mean, const float* rstd, const float* s,
                                     float invN, float dyscale, float* dgamma, float* dbeta, float* A, float* Bc,
                                     float* Cc, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sd = sums[c] * dyscale, sdx = sums[C + c] * dyscale;
  const float dg = rstd[c] * sdx;   // sdx is already centred: sum dy*(raw - mean)
  dgamma[c] = dg;
  dbeta[c] = sd;
  // draw = s*(dy - dbeta/N - xhat*dgamma/N),  xhat = (raw - mean)*rstd
  A[c] = s[c] * dyscale;
  const float k = s[c] * rstd[c] * dg * invN;
  Bc[c] = -k;
  Cc[c] = -s[c] * sd * invN + k * mean[c];
}
int dg_bn_bwd_coeffs(const float* sums, const float* mean, const float* rstd, const float* s, float invN,
                     float dyscale, float* dgamma, float* dbeta, float* coefA, float* coefB, float* coefC, int C, hipStream_t st) {
  hipLaunchKernelGGL(bn_bwd_coeffs_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, sums, mean, rstd, s, invN, dyscale,
                     dgamma, dbeta, coefA, coefB, coefC, C);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

template <bool FLAT>
__global__ void axpby_ch_kernel(TView d, TView xv, TView out, int B, int H, int W, int C4, const float* A,
                                const float* Bc, const float* Cc) {
  const size_t total = (size_t)B * H * W * C4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int c;
    long o_d, o_x, o_o;
    if (FLAT) {
      const unsigned pix = (unsigned)(i / (unsigned)C4);
      c = (int)((unsigned)i - pix * (unsigned)C4) * 4;
      o_d = (long)pix * d.sX;
      o_x = (long)pix * xv.sX;
      o_o = (long)pix * out.sX;
    } else {
      size_t q = i;
      c = (int)(q % C4) * 4;
      q /= C4;
      const int x = (int)(q % W);
      q /= W;
      const int y = (int)(q % H);
      const int b = (int)(q / H);
      o_d = view_off(d, b, y, x);
      o_x = view_off(xv, b, y, x);
      o_o = view_off(out, b, y, x);
    }
    const f32x4 dv = *reinterpret_cast<const f32x4*>(d.p + o_d + c);
    const f32x4 rv = *reinterpret_cast<const f32x4*>(xv.p + o_x + c);
    const f32x4 a4 = *reinterpret_cast<const f32x4*>(A + c);
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(Bc + c);
    const f32x4 c4 = *reinterpret_cast<const f32x4*>(Cc + c);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = fmaf(a4[k], dv[k], fmaf(b4[k], rv[k], c4[k]));
    *reinterpret_cast<f32x4*>(out.p + o_o + c) = o;
  }
}
int dg_axpby_ch(TView d, TView x, TView out, int B, int H, int W, int C, const float* A, const float* Bc,
                const float* Cc, hipStream_t st) {
  const size_t total = (size_t)B * H * W * (C / 4);
  auto is_flat = [&](const TView& t) { return t.sY == (long)W * t.sX && t.sB == (long)H * t.sY; };
  if (is_flat(d) && is_flat(x) && is_flat(out) && (size_t)B * H * W < (1ull << 31))
    hipLaunchKernelGGL(axpby_ch_kernel<true>, dim3(t_nblk(total, 8192)), dim3(256), 0, st, d, x, out, B, H, W, C / 4, A,
                       Bc, Cc);
  else
    hipLaunchKernelGGL(axpby_ch_kernel<false>, dim3(t_nblk(total, 8192)), dim3(256), 0, st, d, x, out, B, H, W, C / 4,
                       A, Bc, Cc);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

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
// WEIGHTED (labels present; dg_softmax_ce_weighted): the label row becomes cw[k] * t[k] before the statements above run
// on it, a code equal to wa.ignore gives t = 0 without being counted in nbad, and 1/N becomes 1/den, den = the count of
// pixels with a non-zero weight that label_count_kernel left in wa.den (invDen = 0 for den = 0: no division by zero, an
// all-zero dz).  With unit weights, no ignored pixel and den = P every float is the one the WEIGHTED = false
// instantiation computes (1 * t = t, and 1.0f / (float)den is the host's 1.0f / (float)P).  A pixel with t = 0 --
// ignored, or of a zero-weight class -- has a dz row of zeros and still gets its probabilities.  CENSUS under WEIGHTED:
// a pixel without a true class (the ignore code, an all-zero one-hot row) joins no bin.  The WEIGHTED = false
// instantiations ignore wa and compile to the instructions they were.
//
// FOCAL (with WEIGHTED only; dg_softmax_ce_focal): the focal cross-entropy with label smoothing of include/depgan.h
// (depgan_uresnet_set_focal).  The label row stays unweighted until the pixel weight w = sum_k cw[k] t[k] (left to right,
// the pre-pass's statement) and has = any t[k] != 0 are formed from it; then ts[k] = w ((1 - eps) t[k] + (has ? eps / C
// : 0)) takes the row's place, the loss term is -ts[k] (1 - r)^gamma log r and dL/dq_k = -ts[k] (1/den) ((1 - r)^gamma / q
// - gamma (1 - r)^(gamma - 1) log r) on the closed clip interval.  1 - r is formed directly (>= 2^-23 inside the clip);
// the power is 1, 1 - r or (1 - r)^2 for gamma = 0, 1, 2 (a uniform branch: gamma is a kernel argument) and
// exp2f(gamma log2f(1 - r)) otherwise, (1 - r)^(gamma - 1) the power over 1 - r.  Everything behind dL/dq, the census and
// the stored probabilities are the text above.  The FOCAL = false instantiations read neither gamma nor eps, the last
// two arguments, and compile to the instructions they were.
enum { LBL_NONE = 0, LBL_ONEHOT = 1, LBL_CODES = 2 };

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

// what the focal mode adds to the weighted launch, by value
struct SmFocal {
  float gamma, eps;
};

template <int C>
static void softmax_ce_launch(int lbl, bool census, int nb, hipStream_t st, const float* logits, const float* onehot,
                              const unsigned char* codes, float* probs, float* dz, float* part, unsigned* bad_part,
                              unsigned* cen_part, long P, float invN, const SmWeights* weights, const SmFocal* focal) {
  const SmWeights wa = weights ? *weights : SmWeights{};
  const SmFocal fa = focal ? *focal : SmFocal{0.f, 0.f};
#define DG_SM_GO(LBL, CEN, WGT, FOC)                                                                                   \
  hipLaunchKernelGGL((softmax_ce_kernel<C, LBL, CEN, WGT, FOC>), dim3(nb), dim3(256), 0, st, logits, onehot, codes, probs, \
                     dz, part, bad_part, cen_part, P, invN, wa, fa.gamma, fa.eps)
  if (focal && lbl == LBL_ONEHOT && census) DG_SM_GO(LBL_ONEHOT, true, true, true);
  else if (focal && lbl == LBL_CODES && census) DG_SM_GO(LBL_CODES, true, true, true);
  else if (focal && lbl == LBL_ONEHOT) DG_SM_GO(LBL_ONEHOT, false, true, true);
  else if (focal && lbl == LBL_CODES) DG_SM_GO(LBL_CODES, false, true, true);
  else if (weights && lbl == LBL_ONEHOT && census) DG_SM_GO(LBL_ONEHOT, true, true, false);
  else if (weights && lbl == LBL_CODES && census) DG_SM_GO(LBL_CODES, true, true, false);
  else if (weights && lbl == LBL_ONEHOT) DG_SM_GO(LBL_ONEHOT, false, true, false);
  else if (weights && lbl == LBL_CODES) DG_SM_GO(LBL_CODES, false, true, false);
  else if (lbl == LBL_ONEHOT && census) DG_SM_GO(LBL_ONEHOT, true, false, false);
  else if (lbl == LBL_CODES && census) DG_SM_GO(LBL_CODES, true, false, false);
  else if (lbl == LBL_ONEHOT) DG_SM_GO(LBL_ONEHOT, false, false, false);
  else if (lbl == LBL_CODES) DG_SM_GO(LBL_CODES, false, false, false);
  else DG_SM_GO(LBL_NONE, false, false, false);
#undef DG_SM_GO
}

int dg_softmax_ce_check(const float* logits, const float* onehot, const unsigned char* codes, const float* probs,
                        const float* dz, const float* loss_sum, long P, int C) {
  if (!logits || !probs || P < 1) { dg_set_error("dg_softmax_ce: null logits or probs, or P < 1"); return DG_ERR_ARG; }
  if (C < DG_MIN_CLASSES || C > DG_MAX_CLASSES) {
    dg_set_error("dg_softmax_ce: %d classes (the kernel covers %d to %d)", C, DG_MIN_CLASSES, DG_MAX_CLASSES);
    return DG_ERR_ARG;
  }
  if (onehot && codes) { dg_set_error("dg_softmax_ce: one-hot labels and class codes are both given"); return DG_ERR_ARG; }
  if ((onehot || codes) && (!dz || !loss_sum)) { dg_set_error("dg_softmax_ce: labels without dz or loss_sum"); return DG_ERR_ARG; }
  // rows are read and written 16 bytes at a time where C is a multiple of 4, else float by float
  const uintptr_t al = (C % 4 == 0) ? 15 : 3;
  if ((((uintptr_t)logits | (uintptr_t)probs | (uintptr_t)onehot | (uintptr_t)dz) & al) || ((uintptr_t)loss_sum & 3)) {
    dg_set_error("dg_softmax_ce: logits, probs, onehot and dz must be %d-byte aligned for %d classes", (int)al + 1, C);
    return DG_ERR_ARG;
  }
  return DG_OK;
}

// census: null, or C*C device counts; the block tables then follow the 2048 floats of the other partials.  weights:
// null, or the loss-weight mode's arguments (weights->den already holds the count when this launch runs).  focal: null,
// or the focal mode's two floats (with weights only)
static int softmax_ce_run(const float* logits, const float* onehot, const unsigned char* codes, float* probs, float* dz,
                          float* loss_sum, unsigned* bad_count, unsigned long long* census, long P, int C, float* scratch,
                          hipStream_t st, const SmWeights* weights = nullptr, const SmFocal* focal = nullptr) {
  const int lbl = onehot ? LBL_ONEHOT : (codes ? LBL_CODES : LBL_NONE);
  if (lbl != LBL_NONE && !scratch) { dg_set_error("dg_softmax_ce: labels without scratch"); return DG_ERR_ARG; }
  if (lbl == LBL_CODES && !bad_count) { dg_set_error("dg_softmax_ce: class codes without a counter"); return DG_ERR_ARG; }
  const int nb = t_nblk((size_t)P, 1024);
  float* part = scratch;
  unsigned* bad_part = scratch ? reinterpret_cast<unsigned*>(scratch + 1024) : nullptr;
  unsigned* cen_part = census ? reinterpret_cast<unsigned*>(scratch + 2048) : nullptr;
  const float invN = (lbl == LBL_NONE) ? 0.f : 1.0f / (float)P;
  switch (C) {
#define DG_SM(N) case N: softmax_ce_launch<N>(lbl, census != nullptr, nb, st, logits, onehot, codes, probs, dz, part, bad_part, cen_part, P, invN, weights, focal); break;
    DG_SM(2) DG_SM(3) DG_SM(4) DG_SM(5) DG_SM(6) DG_SM(7) DG_SM(8)
#undef DG_SM
  }
  HIPCHECK(hipGetLastError());
  if (lbl == LBL_NONE) return DG_OK;
  if (census)
    hipLaunchKernelGGL(sum_small_kernel<true>, dim3(1), dim3(256), 0, st, part, nb, loss_sum,
                       lbl == LBL_CODES ? bad_part : nullptr, bad_count, cen_part, census, C * C);
  else
    hipLaunchKernelGGL(sum_small_kernel<false>, dim3(1), dim3(256), 0, st, part, nb, loss_sum,
                       lbl == LBL_CODES ? bad_part : nullptr, bad_count, nullptr, nullptr, 0);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

int dg_softmax_ce(const float* logits, const float* onehot, const unsigned char* codes, float* probs, float* dz,
                  float* loss_sum, unsigned* bad_count, long P, int C, float* scratch, hipStream_t st) {
  DGCHECK(dg_softmax_ce_check(logits, onehot, codes, probs, dz, loss_sum, P, C));
  return softmax_ce_run(logits, onehot, codes, probs, dz, loss_sum, bad_count, nullptr, P, C, scratch, st);
}

size_t dg_softmax_ce_census_scratch(long P, int C) { return 2048 + (size_t)t_nblk((size_t)P, 1024) * C * C; }

int dg_softmax_ce_census(const float* logits, const float* onehot, const unsigned char* codes, float* probs, float* dz,
                         float* loss_sum, unsigned* bad_count, unsigned long long* census, long P, int C, float* scratch,
                         size_t scratch_floats, hipStream_t st) {
  DGCHECK(dg_softmax_ce_check(logits, onehot, codes, probs, dz, loss_sum, P, C));
  if (!onehot && !codes) { dg_set_error("dg_softmax_ce_census: a census needs labels"); return DG_ERR_ARG; }
  if (!census || ((uintptr_t)census & 7)) { dg_set_error("dg_softmax_ce_census: null or misaligned census"); return DG_ERR_ARG; }
  if (!bad_count) { dg_set_error("dg_softmax_ce_census: no counter of out-of-range codes"); return DG_ERR_ARG; }
  const size_t need = dg_softmax_ce_census_scratch(P, C);
  if (!scratch || scratch_floats < need) {
    dg_set_error("dg_softmax_ce_census: scratch of %zu floats, the launch needs %zu", scratch ? scratch_floats : (size_t)0, need);
    return DG_ERR_ARG;
  }
  return softmax_ce_run(logits, onehot, codes, probs, dz, loss_sum, bad_count, census, P, C, scratch, st);
}

// ---------------------------------------------------------------------------
// the loss-weight mode: label pre-pass and weighted cross-entropy
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
  switch (C) {
#define DG_LC(N)                                                                                                       \
  case N:                                                                                                              \
    if (onehot) hipLaunchKernelGGL((label_count_kernel<N, LBL_ONEHOT>), dim3(nb), dim3(256), 0, st, onehot, codes, wa, cnt_part, P); \
    else hipLaunchKernelGGL((label_count_kernel<N, LBL_CODES>), dim3(nb), dim3(256), 0, st, onehot, codes, wa, cnt_part, P); \
    break;
    DG_LC(2) DG_LC(3) DG_LC(4) DG_LC(5) DG_LC(6) DG_LC(7) DG_LC(8)
#undef DG_LC
  }
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(label_count_sum_kernel, dim3(1), dim3(256), 0, st, cnt_part, nb, C + 3, counts);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

static int label_counts_check(const char* who, const float* onehot, const unsigned char* codes, long P, int C,
                              const unsigned long long* counts, const float* scratch, size_t scratch_floats) {
  if (P < 1 || (!onehot == !codes)) { dg_set_error("%s: P < 1, or not exactly one of onehot and codes", who); return DG_ERR_ARG; }
  if (onehot && ((uintptr_t)onehot & ((C % 4 == 0) ? 15 : 3))) { dg_set_error("%s: misaligned onehot", who); return DG_ERR_ARG; }
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

size_t dg_softmax_ce_weighted_scratch(long P, int C, bool census) {
  const size_t a = census ? dg_softmax_ce_census_scratch(P, C) : 2048, b = dg_label_counts_scratch(P, C);
  return a > b ? a : b;
}

// the weighted and the focal entry: one set of checks, one pre-pass, one launch (focal null: the loss-weight mode alone)
static int softmax_ce_weighted_run(const char* who, const float* logits, const float* onehot, const unsigned char* codes,
                                   float* probs, float* dz, float* loss_sum, unsigned* bad_count,
                                   unsigned long long* census, unsigned long long* counts, const float* cw,
                                   int ignore_code, const SmFocal* focal, long P, int C, float* scratch,
                                   size_t scratch_floats, hipStream_t st) {
  DGCHECK(dg_loss_weights_check(who, cw, C, C, ignore_code));
  DGCHECK(dg_softmax_ce_check(logits, onehot, codes, probs, dz, loss_sum, P, C));
  if (!onehot && !codes) { dg_set_error("%s: loss weights need labels", who); return DG_ERR_ARG; }
  if (census && ((uintptr_t)census & 7)) { dg_set_error("%s: misaligned census", who); return DG_ERR_ARG; }
  if (!bad_count) { dg_set_error("%s: no counter of out-of-range codes", who); return DG_ERR_ARG; }
  const size_t need = dg_softmax_ce_weighted_scratch(P, C, census != nullptr);
  if (!scratch || scratch_floats < need) {
    dg_set_error("%s: scratch of %zu floats, the launches need %zu", who, scratch ? scratch_floats : (size_t)0, need);
    return DG_ERR_ARG;
  }
  DGCHECK(label_counts_check(who, onehot, codes, P, C, counts, scratch, scratch_floats));
  const SmWeights wa = sm_weights(cw, C, ignore_code, counts);
  // the label pass's partials and the cross-entropy pass's share the scratch: the second stage of the first has read them
  // before the second pass, behind it on the stream, writes
  DGCHECK(label_counts_run(onehot, codes, P, C, wa, counts, scratch, st));
  return softmax_ce_run(logits, onehot, codes, probs, dz, loss_sum, bad_count, census, P, C, scratch, st, &wa, focal);
}

int dg_softmax_ce_weighted(const float* logits, const float* onehot, const unsigned char* codes, float* probs, float* dz,
                           float* loss_sum, unsigned* bad_count, unsigned long long* census,
                           unsigned long long* counts, const float* cw, int ignore_code, long P, int C, float* scratch,
                           size_t scratch_floats, hipStream_t st) {
  return softmax_ce_weighted_run("dg_softmax_ce_weighted", logits, onehot, codes, probs, dz, loss_sum, bad_count, census,
                                 counts, cw, ignore_code, nullptr, P, C, scratch, scratch_floats, st);
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

int dg_softmax_ce_focal(const float* logits, const float* onehot, const unsigned char* codes, float* probs, float* dz,
                        float* loss_sum, unsigned* bad_count, unsigned long long* census, unsigned long long* counts,
                        const float* cw, int ignore_code, float gamma, float label_smoothing, long P, int C,
                        float* scratch, size_t scratch_floats, hipStream_t st) {
  DGCHECK(dg_focal_check("dg_softmax_ce_focal", gamma, label_smoothing));
  const SmFocal fa{gamma, label_smoothing};
  return softmax_ce_weighted_run("dg_softmax_ce_focal", logits, onehot, codes, probs, dz, loss_sum, bad_count, census,
                                 counts, cw, ignore_code, &fa, P, C, scratch, scratch_floats, st);
}

// ---------------------------------------------------------------------------
// the 1x1 head to K class logits for K other than 4 (K = 4 keeps the direct-convolution and MFMA weight-gradient
// launches of uresnet.hip): dense rows of K floats, HBM-bound, K a template parameter so that a row stays in registers
// ---------------------------------------------------------------------------
// Forward.  head_fwd_kernel's lane mapping (C / 4 lanes per pixel, one 16-byte load each) with K columns of w (C, K):
// per 4-channel part v = a0 w0, fmaf over channels 1..3; xor butterfly over the parts; + b[k].  The grid stride is a
// multiple of 256, hence of the lanes per pixel: a lane keeps its part and loads its 4 K weights once.
template <int K>
__global__ __launch_bounds__(256) void head_k_fwd_kernel(const float* __restrict__ a, long ld,
                                                          const float* __restrict__ w, const float* __restrict__ b,
                                                          float* __restrict__ logits, long P, int lgLP) {
#pragma clang fp contract(off)
  const int LP = 1 << lgLP;
  const int part = threadIdx.x & (LP - 1);
  float wv[4][K];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < K; ++k) wv[j][k] = w[(part * 4 + j) * K + k];
  const long total = P << lgLP;
  // the trip count is the same for every lane of a block: the shuffles below run with all 64 lanes
  for (long t0 = blockIdx.x * 256L; t0 < total; t0 += gridDim.x * 256L) {
    const long p = (t0 + threadIdx.x) >> lgLP;
    float z[K];
#pragma unroll
    for (int k = 0; k < K; ++k) z[k] = 0.f;
    if (p < P) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(a + p * ld + part * 4);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float v = av[0] * wv[0][k];
#pragma unroll
        for (int j = 1; j < 4; ++j) v = fmaf(av[j], wv[j][k], v);
        z[k] = v;
      }
    }
    for (int o = LP >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < K; ++k) z[k] += __shfl_xor(z[k], o, 64);
    }
    if (p < P && part == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) z[k] += b[k];
      dg_row_store<K>(logits + p * K, z);
    }
  }
}

// Backward-data onto the head's input under its ReLU mask: din[p][c] = (a[p][c] > 0) ? sum_k dz[p][k] w[c][k] : 0,
// the sum as d0 w0 then fmaf over k = 1..K-1.  Thread = one pixel x 4 channels, lane mapping as above.
template <int K>
__global__ __launch_bounds__(256) void head_k_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ w,
                                                          const float* __restrict__ a, long lda,
                                                          float* __restrict__ din, long ldd, long P, int lgLP) {
#pragma clang fp contract(off)
  const int LP = 1 << lgLP;
  const int part = threadIdx.x & (LP - 1);
  float wv[4][K];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < K; ++k) wv[j][k] = w[(part * 4 + j) * K + k];
  const long total = P << lgLP;
  for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += gridDim.x * 256L) {
    const long p = t >> lgLP;
    float d[K];
    dg_row_load<K>(dz + p * K, d);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = d[0] * wv[j][0];
#pragma unroll
      for (int k = 1; k < K; ++k) v = fmaf(d[k], wv[j][k], v);
      o[j] = v;
    }
    if (a) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(a + p * lda + part * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (av[j] > 0.f) ? o[j] : 0.f;
    }
    *reinterpret_cast<f32x4*>(din + p * ldd + part * 4) = o;
  }
}

// Weight and bias gradient, two stages, fixed order, no atomics.  Stage 1: block b covers pixels [b ppb, (b+1) ppb);
// thread (pixel row pp, part lp) walks its pixels in order, 4 K accumulators dW[c][k] += a[p][c] dz[p][k] (fmaf) and,
// in part 0, K bias sums; the 256 / LP pixel rows are then added in index order through LDS -> part[b][C K + K].
template <int K>
__global__ __launch_bounds__(256) void head_k_wgrad_partial(const float* __restrict__ a, long lda,
                                                             const float* __restrict__ dz, long P, int lgLP, int ppb,
                                                             float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sh[];   // [256][4 K], then [256 / LP][K]
  const int LP = 1 << lgLP, PP = 256 >> lgLP;
  const int lp = threadIdx.x & (LP - 1), pp = threadIdx.x >> lgLP;
  float* shb = sh + 256 * 4 * K;
  const long q0 = (long)blockIdx.x * ppb, q1 = min(q0 + ppb, P);
  float acc[4][K], bs[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    bs[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j][k] = 0.f;
  }
  for (long q = q0 + pp; q < q1; q += PP) {
    float d[K];
    dg_row_load<K>(dz + q * K, d);
    const f32x4 av = *reinterpret_cast<const f32x4*>(a + q * lda + lp * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < K; ++k) acc[j][k] = fmaf(av[j], d[k], acc[j][k]);
    if (lp == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) bs[k] += d[k];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < K; ++k) sh[threadIdx.x * 4 * K + j * K + k] = acc[j][k];
  if (lp == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) shb[pp * K + k] = bs[k];
  }
  __syncthreads();
  const int nw = LP * 4 * K, nout = nw + K;
  for (int idx = threadIdx.x; idx < nout; idx += 256) {
    float s = 0.f;
    if (idx < nw) {
      const int c = idx / K, k = idx - c * K;
      const int l = c >> 2, j = c & 3;
      for (int r = 0; r < PP; ++r) s += sh[((r << lgLP) + l) * 4 * K + j * K + k];
    } else {
      for (int r = 0; r < PP; ++r) s += shb[r * K + (idx - nw)];
    }
    part[(size_t)blockIdx.x * nout + idx] = s;
  }
}
// Stage 2: one block per gradient entry, the nb block partials strided over the threads and a fixed-order block sum.
// Entries [0, nw) are dW (C, K) dense -- the (1, 1, C, K) arena tensor -- and [nw, nw + K) are db.
__global__ void head_k_wgrad_final(const float* __restrict__ part, int nb, int nout, int nw, float* __restrict__ dW,
                                   float* __restrict__ db) {
  __shared__ float sh4[4];
  const int e = blockIdx.x;
  float s = 0.f;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) s += part[(size_t)b * nout + e];
  s = t_block_sum(s, sh4);
  if (threadIdx.x == 0) {
    if (e < nw) dW[e] = s; else db[e - nw] = s;
  }
}

static int head_k_check(const char* who, long P, int C, int K, int* lg) {
  const int LP = C / 4;
  if (P < 1 || K < DG_MIN_CLASSES || K > DG_MAX_CLASSES) {
    dg_set_error("%s: P >= 1 and %d to %d classes (got %ld, %d)", who, DG_MIN_CLASSES, DG_MAX_CLASSES, P, K);
    return DG_ERR_ARG;
  }
  if (C < 4 || (C % 4) || LP > 64 || (LP & (LP - 1))) { dg_set_error("%s: C/4 must be a power of two <= 64", who); return DG_ERR_ARG; }
  if (P > (0x7FFFFFFFFFFFFFFFL >> 8) / 256) { dg_set_error("%s: %ld pixels", who, P); return DG_ERR_UNSUPPORTED; }
  *lg = 0;
  while ((1 << *lg) < LP) ++*lg;
  return DG_OK;
}
static unsigned head_k_blocks(long P, int lg) {
  const long b = ((P << lg) + 255) / 256;
  return (unsigned)(b > 2048 ? 2048 : b);   // 256 CUs x 8 resident blocks; the loop takes the rest
}
#define DG_HEAD_K(CALL)                                                                                    \
  switch (K) {                                                                                             \
    case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; case 5: CALL(5); break;        \
    case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break;                                \
  }

int dg_head_k_fwd(const float* a, long ld, const float* w, const float* b, float* logits, long P, int C, int K,
                  hipStream_t st) {
  int lg;
  DGCHECK(head_k_check("dg_head_k_fwd", P, C, K, &lg));
  if (!a || !w || !b || !logits || ld < C || (ld % 4) || (((uintptr_t)a) & 15) || (((uintptr_t)logits) & (K % 4 ? 3 : 15))) {
    dg_set_error("dg_head_k_fwd: null, misaligned or short-strided operand");
    return DG_ERR_ARG;
  }
#define DG_CALL(N) hipLaunchKernelGGL(head_k_fwd_kernel<N>, dim3(head_k_blocks(P, lg)), dim3(256), 0, st, a, ld, w, b, logits, P, lg)
  DG_HEAD_K(DG_CALL)
#undef DG_CALL
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

int dg_head_k_bwd(const float* dz, const float* w, const float* mask, long ldm, float* din, long ldd, long P, int C,
                  int K, hipStream_t st) {
  int lg;
  DGCHECK(head_k_check("dg_head_k_bwd", P, C, K, &lg));
  if (!dz || !w || !din || ldd < C || (ldd % 4) || (((uintptr_t)din) & 15) || (((uintptr_t)dz) & (K % 4 ? 3 : 15)) ||
      (mask && (ldm < C || (ldm % 4) || (((uintptr_t)mask) & 15)))) {
    dg_set_error("dg_head_k_bwd: null, misaligned or short-strided operand");
    return DG_ERR_ARG;
  }
#define DG_CALL(N) hipLaunchKernelGGL(head_k_bwd_kernel<N>, dim3(head_k_blocks(P, lg)), dim3(256), 0, st, dz, w, mask, ldm, din, ldd, P, lg)
  DG_HEAD_K(DG_CALL)
#undef DG_CALL
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

size_t dg_head_k_wgrad_scratch(long P, int C, int K) {
  int nb, ppb;
  t_pix_grid(P, &nb, &ppb);
  return (size_t)nb * ((size_t)C * K + K);
}
int dg_head_k_wgrad(const float* a, long lda, const float* dz, float* dW, float* db, long P, int C, int K,
                    float* scratch, size_t scratch_floats, hipStream_t st) {
  int lg;
  DGCHECK(head_k_check("dg_head_k_wgrad", P, C, K, &lg));
  if (!a || !dz || !dW || !db || !scratch || lda < C || (lda % 4) || (((uintptr_t)a) & 15) ||
      (((uintptr_t)dz) & (K % 4 ? 3 : 15))) {
    dg_set_error("dg_head_k_wgrad: null, misaligned or short-strided operand");
    return DG_ERR_ARG;
  }
  if (dg_head_k_wgrad_scratch(P, C, K) > scratch_floats) {
    dg_set_error("dg_head_k_wgrad: scratch holds %zu floats, %zu needed", scratch_floats, dg_head_k_wgrad_scratch(P, C, K));
    return DG_ERR_ARG;
  }
  int nb, ppb;
  t_pix_grid(P, &nb, &ppb);
  const int nw = C * K, nout = nw + K;
  const size_t lds = (size_t)(256 * 4 * K + (256 >> lg) * K) * sizeof(float);
#define DG_CALL(N) hipLaunchKernelGGL(head_k_wgrad_partial<N>, dim3(nb), dim3(256), lds, st, a, lda, dz, P, lg, ppb, scratch)
  DG_HEAD_K(DG_CALL)
#undef DG_CALL
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(head_k_wgrad_final, dim3(nout), dim3(256), 0, st, scratch, nb, nout, nw, dW, db);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
#undef DG_HEAD_K

// ---------------------------------------------------------------------------
// BN over the rows of small matrices (noise MLP), thread = column
// ---------------------------------------------------------------------------
// One 256-thread block per column: rows are strided over the threads, sums go through a fixed-order block reduction.
__global__ void bn_rows_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int R, int C, int ld,
                                   const float* gamma, const float* beta, float eps, float momentum, float corr,
                                   float* mm, float* mv, float* mean, float* rstd, int relu) {
  __shared__ float sh4[4];
  const int c = blockIdx.x;
  float s = 0.f;
  for (int r = threadIdx.x; r < R; r += blockDim.x) s += x[(size_t)r * ld + c];
  const float mu = t_block_sum(s, sh4) / (float)R;
  float q = 0.f;
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    const float d = x[(size_t)r * ld + c] - mu;
    q = fmaf(d, d, q);
  }
  const float var = t_block_sum(q, sh4) / (float)R;
  const float rs = 1.0f / sqrtf(var + eps);
  if (threadIdx.x == 0) {
    mean[c] = mu;
    rstd[c] = rs;
    if (mm) {
      mm[c] = mm[c] * momentum + mu * (1.0f - momentum);
      mv[c] = mv[c] * momentum + var * corr * (1.0f - momentum);
    }
  }
  const float g = gamma[c], bt = beta[c];
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    float v = (x[(size_t)r * ld + c] - mu) * rs * g + bt;
    if (relu) v = fmaxf(v, 0.f);
    y[(size_t)r * ld + c] = v;
  }
}
int dg_bn_rows_fwd(const float* x, float* y, int R, int C, int ld, const float* gamma, const float* beta, float eps,
                   float momentum, float corr, float* moving_mean, float* moving_var, float* mean, float* rstd,
                   int relu, hipStream_t st) {
  hipLaunchKernelGGL(bn_rows_fwd_kernel, dim3(C), dim3(256), 0, st, x, y, R, C, ld, gamma, beta, eps, momentum, corr,
                     moving_mean, moving_var, mean, rstd, relu);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
__global__ void bn_rows_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                   const float* __restrict__ relu_out, float* __restrict__ dx, int R, int C, int ld,
                                   const float* gamma, const float* mean, const float* rstd, float* dgamma,
                                   float* dbeta) {
  __shared__ float sh4[4];
  const int c = blockIdx.x;
  const float mu = mean[c], rs = rstd[c];
  float sd = 0.f, sdx = 0.f;
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    const size_t o = (size_t)r * ld + c;
    const float d = (relu_out && !(relu_out[o] > 0.f)) ? 0.f : dy[o];
    sd += d;
    sdx = fmaf(d, (x[o] - mu) * rs, sdx);
  }
  sd = t_block_sum(sd, sh4);
  sdx = t_block_sum(sdx, sh4);
  if (threadIdx.x == 0) {
    dgamma[c] = sdx;
    dbeta[c] = sd;
  }
  const float s = gamma[c] * rs, invR = 1.0f / (float)R;
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    const size_t o = (size_t)r * ld + c;
    const float d = (relu_out && !(relu_out[o] > 0.f)) ? 0.f : dy[o];
    dx[o] = s * (d - sd * invR - (x[o] - mu) * rs * sdx * invR);
  }
}
int dg_bn_rows_bwd(const float* dy, const float* x, const float* relu_out, float* dx, int R, int C, int ld,
                   const float* gamma, const float* mean, const float* rstd, float* dgamma, float* dbeta,
                   hipStream_t st) {
  hipLaunchKernelGGL(bn_rows_bwd_kernel, dim3(C), dim3(256), 0, st, dy, x, relu_out, dx, R, C, ld, gamma, mean, rstd,
                     dgamma, dbeta);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

__global__ void small_gemm_kernel(const float* A, const float* Bm, const float* bias, float* Cm, int M, int K, int N) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)M * N) return;
  const int m = (int)(i / N), n = (int)(i % N);
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(A[(size_t)m * K + k], Bm[(size_t)k * N + n], acc);
  Cm[i] = acc + (bias ? bias[n] : 0.f);
}
int dg_small_gemm(const float* A, const float* Bm, const float* bias, float* Cm, int M, int K, int N, hipStream_t st) {
  hipLaunchKernelGGL(small_gemm_kernel, dim3(cdiv((long)M * N, 256)), dim3(256), 0, st, A, Bm, bias, Cm, M, K, N);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
// C[k][n] = sum_m A[m][k] D[m][n]: one 256-thread block per output element, rows strided over the threads
__global__ void small_gemm_at_kernel(const float* A, const float* D, float* Cm, int M, int K, int N) {
  __shared__ float sh4[4];
  const int k = blockIdx.x / N, n = blockIdx.x % N;
  float acc = 0.f;
  for (int m = threadIdx.x; m < M; m += blockDim.x) acc = fmaf(A[(size_t)m * K + k], D[(size_t)m * N + n], acc);
  acc = t_block_sum(acc, sh4);
  if (threadIdx.x == 0) Cm[blockIdx.x] = acc;
}
int dg_small_gemm_at(const float* A, const float* D, float* Cm, int M, int K, int N, hipStream_t st) {
  hipLaunchKernelGGL(small_gemm_at_kernel, dim3(K * N), dim3(256), 0, st, A, D, Cm, M, K, N);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
__global__ void small_gemm_bt_kernel(const float* D, const float* Bm, float* Cm, int M, int K, int N) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)M * K) return;
  const int m = (int)(i / K), k = (int)(i % K);
  float acc = 0.f;
  for (int n = 0; n < N; ++n) acc = fmaf(D[(size_t)m * N + n], Bm[(size_t)k * N + n], acc);
  Cm[i] = acc;
}
int dg_small_gemm_bt(const float* D, const float* Bm, float* Cm, int M, int K, int N, hipStream_t st) {
  hipLaunchKernelGGL(small_gemm_bt_kernel, dim3(cdiv((long)M * K, 256)), dim3(256), 0, st, D, Bm, Cm, M, K, N);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
__global__ void colsum_small_kernel(const float* x, float* out, int R, int C, int ld) {
  __shared__ float sh4[4];
  const int c = blockIdx.x;
  float s = 0.f;
  for (int r = threadIdx.x; r < R; r += blockDim.x) s += x[(size_t)r * ld + c];
  s = t_block_sum(s, sh4);
  if (threadIdx.x == 0) out[c] = s;
}
int dg_colsum_small(const float* x, float* out, int R, int C, int ld, hipStream_t st) {
  hipLaunchKernelGGL(colsum_small_kernel, dim3(C), dim3(256), 0, st, x, out, R, C, ld);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
