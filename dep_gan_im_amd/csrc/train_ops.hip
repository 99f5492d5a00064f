// Learning-phase-1 operators (see train_ops.h).  All HBM-bound: 16-byte accesses over the channel
// axis, block reductions through LDS, deterministic second passes.
#include "train_ops.h"

#include "block_sum.h"
#include "epilogue.h"
#include "softmax_row.h"

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
