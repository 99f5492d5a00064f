// HBM-bound operators of the generator update on bf16 activation storage (bf16s_train.h): the bf16-operand siblings of
// pool_bwd_kernel<0>, film_bwd_partial / film_bwd_final, colsum_partial (with a row multiplier) and head_bwd_kernel in
// ops.hip.  The activation operand is read as 16-byte pieces of 8 bf16 and widened (exact); gradients are fp32 in and
// out.  Reductions as there: per-thread partial sums -> LDS -> a second deterministic pass, no float atomics.
#include "bf16s_train.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8), aligned(16)));

static inline int nblk(size_t n, int cap) {
  size_t b = (n + 255) / 256;
  return (int)(b > (size_t)cap ? cap : (b < 1 ? 1 : b));
}
static int scratch_ok(const char* who, size_t need, size_t have) {
  if (need <= have) return 1;
  dg_set_error("%s: scratch holds %zu floats, the launch needs %zu", who, have, need);
  return 0;
}
__device__ __forceinline__ f32x8 ld8h(const __bf16* p) {
  return __builtin_convertvector(*reinterpret_cast<const bf16x8*>(p), f32x8);
}
__device__ __forceinline__ f32x8 ld8f(const float* p) { return *reinterpret_cast<const f32x8*>(p); }

// ---------------------------------------------------------------------------
// un-pool + skip gradient + ReLU mask.  Arg-max = the FIRST maximum of the window in the order (0,0), (0,1), (1,0),
// (1,1) (strict > against the running maximum): first_argmax4 of ops.hip, here on the stored bf16 values.
// ---------------------------------------------------------------------------
__global__ void unpool_mask_bf16s_kernel(TView d, TViewH a, TView skip, TView out, int B, int Ho, int Wo, int C8) {
  const size_t total = (size_t)B * Ho * Wo * C8;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    size_t q = i;
    const int c = (int)(q % C8) * 8;
    q /= C8;
    const int x = (int)(q % Wo);
    q /= Wo;
    const int y = (int)(q % Ho);
    const long b = (long)(q / Ho);
    const __bf16* pa = a.p + b * a.sB + (long)(2 * y) * a.sY + (long)(2 * x) * a.sX + c;
    f32x8 av[4];
    av[0] = ld8h(pa);
    av[1] = ld8h(pa + a.sX);
    av[2] = ld8h(pa + a.sY);
    av[3] = ld8h(pa + a.sY + a.sX);
    const f32x8 dv = ld8f(d.p + b * d.sB + (long)y * d.sY + (long)x * d.sX + c);
    f32x8 o[4];
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int k = 0; k < 8; ++k) o[w][k] = 0.f;
    if (skip.p) {
      const float* ps = skip.p + b * skip.sB + (long)(2 * y) * skip.sY + (long)(2 * x) * skip.sX + c;
      o[0] = ld8f(ps);
      o[1] = ld8f(ps + skip.sX);
      o[2] = ld8f(ps + skip.sY);
      o[3] = ld8f(ps + skip.sY + skip.sX);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int am = 0;
      float m = av[0][k];
      if (av[1][k] > m) { m = av[1][k]; am = 1; }
      if (av[2][k] > m) { m = av[2][k]; am = 2; }
      if (av[3][k] > m) { m = av[3][k]; am = 3; }
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float v = o[w][k] + ((w == am) ? dv[k] : 0.f);
        o[w][k] = (av[w][k] > 0.f) ? v : 0.f;
      }
    }
    float* po = out.p + b * out.sB + (long)(2 * y) * out.sY + (long)(2 * x) * out.sX + c;
    *reinterpret_cast<f32x8*>(po) = o[0];
    *reinterpret_cast<f32x8*>(po + out.sX) = o[1];
    *reinterpret_cast<f32x8*>(po + out.sY) = o[2];
    *reinterpret_cast<f32x8*>(po + out.sY + out.sX) = o[3];
  }
}

static bool al_f(const TView& v) { return !v.p || (!(v.sX % 4) && !(v.sY % 4) && !(v.sB % 4) && !(((uintptr_t)v.p) & 15)); }
static bool al_h(const TViewH& v) { return !(v.sX % 8) && !(v.sY % 8) && !(v.sB % 8) && !(((uintptr_t)v.p) & 15); }

int dg_unpool_mask_bf16s(TView dpool, TViewH a, TView skip, TView out, int B, int Ho, int Wo, int C, hipStream_t st) {
  if (!dpool.p || !a.p || !out.p || B < 1 || Ho < 1 || Wo < 1 || C < 1) { dg_set_error("dg_unpool_mask_bf16s: bad argument"); return DG_ERR_ARG; }
  if (C % 8) { dg_set_error("dg_unpool_mask_bf16s: C %% 8 != 0"); return DG_ERR_ARG; }
  if (!al_f(dpool) || !al_h(a) || !al_f(skip) || !al_f(out)) { dg_set_error("dg_unpool_mask_bf16s: every view must be 16-byte aligned"); return DG_ERR_ARG; }
  const size_t total = (size_t)B * Ho * Wo * (C / 8);
  hipLaunchKernelGGL(unpool_mask_bf16s_kernel, dim3(nblk(total, 8192)), dim3(256), 0, st, dpool, a, skip, out, B, Ho, Wo,
                     C / 8);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

// ---------------------------------------------------------------------------
// FiLM backward: the mask is the decision the forward stored, never a recomputation from the rounded u
// ---------------------------------------------------------------------------
#define FILMH_SPLIT 64
__global__ void film_bwd_bf16s_partial(const float* __restrict__ dr, const __bf16* __restrict__ u,
                                       const unsigned char* __restrict__ dec, const float* __restrict__ fmul, int film_ld,
                                       float* __restrict__ du, float* __restrict__ part, long HW, int C8) {
  extern __shared__ __attribute__((aligned(16))) float sh[];  // [256][16]
  const int b = blockIdx.x, s = blockIdx.y;
  const int LP = C8, PP = 256 / LP;
  const int lp = threadIdx.x % LP, pp = threadIdx.x / LP;
  const long per = (HW + FILMH_SPLIT - 1) / FILMH_SPLIT;
  const long q0 = s * per, q1 = min(q0 + per, HW);
  const int C = C8 * 8;
  f32x8 am, aa;
#pragma unroll
  for (int k = 0; k < 8; ++k) { am[k] = 0.f; aa[k] = 0.f; }
  if (pp < PP) {
    const f32x8 fm = ld8f(fmul + (size_t)b * film_ld + lp * 8);
    for (long q = q0 + pp; q < q1; q += PP) {
      const size_t pix = (size_t)b * HW + q;
      const size_t off = pix * C + lp * 8;
      const f32x8 d = ld8f(dr + off);
      const f32x8 uu = ld8h(u + off);
      const unsigned m = dec[pix * C8 + lp];
      f32x8 o;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float dv = ((m >> k) & 1u) ? d[k] : 0.f;
        aa[k] += dv;
        am[k] = fmaf(dv, uu[k], am[k]);
        o[k] = dv * fm[k];
      }
      *reinterpret_cast<f32x8*>(du + off) = o;
    }
  }
  *reinterpret_cast<f32x8*>(sh + threadIdx.x * 16) = am;
  *reinterpret_cast<f32x8*>(sh + threadIdx.x * 16 + 8) = aa;
  __syncthreads();
  for (int t = threadIdx.x; t < LP * 16; t += 256) {
    const int l = t / 16, k = t % 16;
    float acc = 0.f;
    for (int j = 0; j < PP; ++j) acc += sh[(j * LP + l) * 16 + k];
    // part layout: [b][split][2][C]
    part[(((size_t)b * FILMH_SPLIT + s) * 2 + (k >> 3)) * C + l * 8 + (k & 7)] = acc;
  }
}
__global__ void film_bwd_bf16s_final(const float* __restrict__ part, float* __restrict__ dmul, float* __restrict__ dadd,
                                     int film_ld, int C) {
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float sm = 0.f, sa = 0.f;
    for (int s = 0; s < FILMH_SPLIT; ++s) {
      sm += part[(((size_t)b * FILMH_SPLIT + s) * 2 + 0) * C + c];
      sa += part[(((size_t)b * FILMH_SPLIT + s) * 2 + 1) * C + c];
    }
    dmul[(size_t)b * film_ld + c] = sm;
    dadd[(size_t)b * film_ld + c] = sa;
  }
}
size_t dg_film_bwd_bf16s_scratch(int B, int C) { return (size_t)B * FILMH_SPLIT * 2 * C; }
int dg_film_bwd_bf16s(const float* dr, const __bf16* u, const unsigned char* dec, const float* fmul, int film_ld, float* du,
                      float* dmul, float* dadd, int B, long HW, int C, float* scratch, size_t scratch_floats,
                      hipStream_t st) {
  if (!dr || !u || !dec || !fmul || !du || !dmul || !dadd || !scratch || B < 1 || HW < 1 || C < 1) {
    dg_set_error("dg_film_bwd_bf16s: bad argument");
    return DG_ERR_ARG;
  }
  if ((C % 8) || C > 256 || (film_ld % 4)) { dg_set_error("dg_film_bwd_bf16s: C must be a multiple of 8 and <= 256, ld a multiple of 4"); return DG_ERR_ARG; }
  if ((((uintptr_t)dr) | ((uintptr_t)u) | ((uintptr_t)du) | ((uintptr_t)fmul)) & 15) { dg_set_error("dg_film_bwd_bf16s: operands must be 16-byte aligned"); return DG_ERR_ARG; }
  if (!scratch_ok("dg_film_bwd_bf16s", dg_film_bwd_bf16s_scratch(B, C), scratch_floats)) return DG_ERR_ARG;
  hipLaunchKernelGGL(film_bwd_bf16s_partial, dim3(B, FILMH_SPLIT), dim3(256), 256 * 16 * sizeof(float), st, dr, u, dec,
                     fmul, film_ld, du, scratch, HW, C / 8);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(film_bwd_bf16s_final, dim3(B), dim3(256), 0, st, scratch, dmul, dadd, film_ld, C);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

// ---------------------------------------------------------------------------
// head backward: dW[c] = sum_p dpre[p] a[p][c] and dz[p][c] = (a > 0) ? dpre[p] w[c] : 0
// ---------------------------------------------------------------------------
__global__ void colsum_rowmul_bf16s_partial(const __bf16* __restrict__ a, long ld, long P, int C8, int ppb,
                                            const float* __restrict__ rowmul, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sh[];  // [256][8]
  const int LP = C8, PP = 256 / LP;
  const int lp = threadIdx.x % LP, pp = threadIdx.x / LP;
  const long q0 = (long)blockIdx.x * ppb, q1 = min(q0 + ppb, P);
  f32x8 acc;
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  if (pp < PP) {
    for (long q = q0 + pp; q < q1; q += PP) {
      const f32x8 v = ld8h(a + q * ld + lp * 8);
      const float m = rowmul[q];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = fmaf(v[k], m, acc[k]);
    }
  }
  *reinterpret_cast<f32x8*>(sh + threadIdx.x * 8) = acc;
  __syncthreads();
  for (int t = threadIdx.x; t < LP * 8; t += 256) {
    const int l = t / 8, k = t % 8;
    float s = 0.f;
    for (int j = 0; j < PP; ++j) s += sh[(j * LP + l) * 8 + k];
    part[(size_t)blockIdx.x * (C8 * 8) + t] = s;
  }
}
__global__ void colsum_bf16s_final(const float* __restrict__ part, int nb, int C, float* __restrict__ out) {
  // one 256-thread block per channel
  __shared__ float sh4[4];
  const int c = blockIdx.x;
  float s = 0.f;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) s += part[(size_t)b * C + c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[c] = (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}
static void rowmul_grid(long P, int* nb_out, int* ppb_out) {
  int nb = (int)((P + 255) / 256);
  if (nb > 2048) nb = 2048;
  if (nb < 1) nb = 1;
  const int ppb = (int)((P + nb - 1) / nb);
  *nb_out = (int)((P + ppb - 1) / ppb);
  *ppb_out = ppb;
}
size_t dg_colsum_rowmul_bf16s_scratch(long P, int C) {
  int nb, ppb;
  rowmul_grid(P, &nb, &ppb);
  return (size_t)nb * C;
}
int dg_colsum_rowmul_bf16s(const __bf16* a, long ld, long P, int C, const float* rowmul, float* out, float* scratch,
                           size_t scratch_floats, hipStream_t st) {
  if (!a || !rowmul || !out || !scratch || P < 1 || C < 1) { dg_set_error("dg_colsum_rowmul_bf16s: bad argument"); return DG_ERR_ARG; }
  if ((C % 8) || C > 256 || ld < C || (ld % 8) || (((uintptr_t)a) & 15)) {
    dg_set_error("dg_colsum_rowmul_bf16s: C a multiple of 8 and <= 256, ld >= C a multiple of 8, a 16-byte aligned");
    return DG_ERR_ARG;
  }
  if (!scratch_ok("dg_colsum_rowmul_bf16s", dg_colsum_rowmul_bf16s_scratch(P, C), scratch_floats)) return DG_ERR_ARG;
  int nb, ppb;
  rowmul_grid(P, &nb, &ppb);
  hipLaunchKernelGGL(colsum_rowmul_bf16s_partial, dim3(nb), dim3(256), 256 * 8 * sizeof(float), st, a, ld, P, C / 8, ppb,
                     rowmul, scratch);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(colsum_bf16s_final, dim3(C), dim3(256), 0, st, scratch, nb, C, out);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

__global__ void head_bwd_bf16s_kernel(const float* __restrict__ dpre, const float* __restrict__ w,
                                      const __bf16* __restrict__ a, long ld, float* __restrict__ dz, long P, int C8) {
  const size_t total = (size_t)P * C8;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const long p = (long)(i / C8);
    const int c = (int)(i % C8) * 8;
    const float d = dpre[p];
    const f32x8 av = ld8h(a + p * ld + c);
    const f32x8 wv = ld8f(w + c);
    f32x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = (av[k] > 0.f) ? d * wv[k] : 0.f;
    *reinterpret_cast<f32x8*>(dz + p * (C8 * 8) + c) = o;
  }
}
int dg_head_bwd_bf16s(const float* dpre, const float* w, const __bf16* a, long ld, float* dz, long P, int C,
                      hipStream_t st) {
  if (!dpre || !w || !a || !dz || P < 1 || C < 1) { dg_set_error("dg_head_bwd_bf16s: bad argument"); return DG_ERR_ARG; }
  if ((C % 8) || ld < C || (ld % 8) || ((((uintptr_t)a) | ((uintptr_t)w) | ((uintptr_t)dz)) & 15)) {
    dg_set_error("dg_head_bwd_bf16s: C a multiple of 8, ld >= C a multiple of 8, operands 16-byte aligned");
    return DG_ERR_ARG;
  }
  hipLaunchKernelGGL(head_bwd_bf16s_kernel, dim3(nblk((size_t)P * (C / 8), 8192)), dim3(256), 0, st, dpre, w, a, ld, dz, P,
                     C / 8);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

__global__ void unpack_bits_kernel(const unsigned char* __restrict__ bits, unsigned char* __restrict__ out, long nbytes) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nbytes; i += (long)gridDim.x * blockDim.x) {
    const unsigned m = bits[i];
#pragma unroll
    for (int k = 0; k < 8; ++k) out[i * 8 + k] = (unsigned char)((m >> k) & 1u);
  }
}
int dg_unpack_bits(const unsigned char* bits, unsigned char* out, long n, hipStream_t st) {
  if (!bits || !out || n < 8 || (n % 8)) { dg_set_error("dg_unpack_bits: bad argument"); return DG_ERR_ARG; }
  hipLaunchKernelGGL(unpack_bits_kernel, dim3(nblk((size_t)(n / 8), 4096)), dim3(256), 0, st, bits, out, n / 8);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
