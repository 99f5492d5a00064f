// Data step in front of the path: what the reference does to the NIfTI volumes of one subject
// between nib.load and the training arrays (GT:93-118 load_data / data_prep, GT:124-146
// map_image_to_intensity_range, GT:667-723 masking, clamping, channel concatenation).
//
//   slices[z][x][y] = vol(x, y, z)                                    (data_prep: image[:, :, z], channel axis added)
//   brain_prob_1 = p1 * icv1 [* (1 - sl1)]     brain_flair_1 = f1 * icv1 [* (1 - sl1)]
//   brain_prob_2 = p2 * icv2 [* (1 - sl2)]
//   brain_flair_1 = clip((brain_flair_1 - min) / (max - min) * (1 - 0) + 0, 0, 1)   (min / max over the subject)
//   brain_prob_* [ < 0 ] = 0;   x = concat(brain_prob_1, brain_flair_1) on the channel axis when nicg = 2
//
// All of it is HBM-bound fp32 elementwise work plus one min/max reduction; the only structure is the per-slice
// transpose (file order is x fastest, the network wants NHWC with y fastest), done through a 32 x 33 LDS tile so
// that both the volume reads and the slice writes are coalesced.  Every arithmetic step is a single correctly
// rounded fp32 operation in the reference's order, so the result is bit-identical to the NumPy statements.
#include "common.h"

#include "model.h"

namespace {

constexpr int TS = 32;

__device__ __forceinline__ float masked(const float* v, const float* icv, const float* sl, size_t i) {
  float r = __fmul_rn(v[i], icv[i]);
  if (sl) r = __fmul_rn(r, __fsub_rn(1.0f, sl[i]));
  return r;
}

// grid (ceil(X/32), ceil(Y/32), Z), block (32, 8)
__global__ __launch_bounds__(256) void subject_prep_kernel(const float* __restrict__ p1, const float* __restrict__ f1,
                                                           const float* __restrict__ icv1,
                                                           const float* __restrict__ sl1,
                                                           const float* __restrict__ p2,
                                                           const float* __restrict__ icv2,
                                                           const float* __restrict__ sl2, int X, int Y, int nicg,
                                                           float* __restrict__ xo, float* __restrict__ yo,
                                                           float* __restrict__ part) {
  __shared__ float tp[TS][TS + 1], tf[TS][TS + 1], ty[TS][TS + 1];
  __shared__ float rmin[8], rmax[8];
  const int z = blockIdx.z;
  const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
  const size_t vbase = (size_t)z * X * Y;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  // read: x fastest (file order); threadIdx.x walks x
  for (int j = threadIdx.y; j < TS; j += 8) {
    const int x = x0 + threadIdx.x, y = y0 + j;
    if (x < X && y < Y) {
      const size_t i = vbase + (size_t)y * X + x;
      tp[j][threadIdx.x] = masked(p1, icv1, sl1, i);
      ty[j][threadIdx.x] = masked(p2, icv2, sl2, i);
      if (nicg == 2) {
        const float f = masked(f1, icv1, sl1, i);
        tf[j][threadIdx.x] = f;
        mn = fminf(mn, f);
        mx = fmaxf(mx, f);
      }
    }
  }
  __syncthreads();
  // write: y fastest (NHWC slice [z][x][y][c]); threadIdx.x walks y
  for (int j = threadIdx.y; j < TS; j += 8) {
    const int x = x0 + j, y = y0 + threadIdx.x;
    if (x < X && y < Y) {
      const size_t o = ((size_t)z * X + x) * Y + y;
      float a = tp[threadIdx.x][j], b = ty[threadIdx.x][j];
      a = (a < 0.f) ? 0.f : a;     // brain_prob[brain_prob < 0] = 0 (GT:706-707); NaN stays NaN as in NumPy
      b = (b < 0.f) ? 0.f : b;
      yo[o] = b;
      if (nicg == 2) {
        xo[2 * o] = a;
        xo[2 * o + 1] = tf[threadIdx.x][j];   // normalised in place by the second kernel
      } else {
        xo[o] = a;
      }
    }
  }
  if (nicg == 2) {
    // block min / max of the masked FLAIR -> partials (NaNs are ignored by fminf / fmaxf; np.percentile would return
    // NaN -- volumes with NaNs are outside what the reference can process either)
    for (int o = 32; o > 0; o >>= 1) {
      mn = fminf(mn, __shfl_down(mn, o));
      mx = fmaxf(mx, __shfl_down(mx, o));
    }
    const int tid = threadIdx.y * 32 + threadIdx.x;
    if ((tid & 63) == 0) {
      rmin[tid >> 6] = mn;
      rmax[tid >> 6] = mx;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w) {
        mn = fminf(mn, rmin[w]);
        mx = fmaxf(mx, rmax[w]);
      }
      const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
      part[2 * b] = mn;
      part[2 * b + 1] = mx;
    }
  }
}

__global__ __launch_bounds__(256) void minmax_final_kernel(const float* __restrict__ part, size_t n,
                                                           float* __restrict__ out) {
  __shared__ float rmin[4], rmax[4];
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (size_t i = threadIdx.x; i < n; i += 256) {
    mn = fminf(mn, part[2 * i]);
    mx = fmaxf(mx, part[2 * i + 1]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_down(mn, o));
    mx = fmaxf(mx, __shfl_down(mx, o));
  }
  if ((threadIdx.x & 63) == 0) {
    rmin[threadIdx.x >> 6] = mn;
    rmax[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      mn = fminf(mn, rmin[w]);
      mx = fmaxf(mx, rmax[w]);
    }
    out[0] = mn;
    out[1] = mx;
  }
}

// channel 1 of x (npix, 2): v -> clip((v - min) / (max - min) * (max_o - min_o) + min_o, min_o, max_o), GT:140-144
__global__ __launch_bounds__(256) void flair_normalise_kernel(float* __restrict__ xo, size_t npix,
                                                              const float* __restrict__ mm, float min_o, float max_o) {
  // hipcc's __fmul_rn / __fadd_rn are plain `*` / `+` inside a header and may be contracted into an FMA; operators
  // written HERE under the pragma are what keeps every operation individually rounded, as NumPy's statement sequence
  // is (GT:140-144)
#pragma clang fp contract(off)
  const float mn = mm[0], rng = __fsub_rn(mm[1], mm[0]), span = __fsub_rn(max_o, min_o);
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
    float v = xo[2 * i + 1];
    const float q = __fdiv_rn(v - mn, rng);
    const float t = q * span;
    v = t + min_o;
    v = (v > max_o) ? max_o : v;
    v = (v < min_o) ? min_o : v;
    xo[2 * i + 1] = v;
  }
}

// ---- DEP-UResNet data step (DEP-UResNet-wNoises-training-4fold.py "UT":485-566, DEP-UResNet_testing_4fold.py
// "UE":496-540) ----
//   brain_flair_1 = f1 * icv1 [* (1 - sl1)];   out = nan_to_num((brain_flair_1 - mean) / std)   (UT:510-512)
//   mean / std (ddof 0) over the whole masked volume, zeros outside the brain included
// mean and std are float64 sums of the float32 volume, each a fixed-order two-stage reduction (block partials in a
// fixed grid, then one block summing them in index order): no float atomics, so the bits repeat from run to run.
// Two passes (mean, then the squared deviations from it) rather than sum / sum of squares: no cancellation.

constexpr int ZS_PASS2_BLOCKS = 1024;

// fixed-order sum of one double per thread of a 256-thread block; the total lands in thread 0
__device__ __forceinline__ double block_sum_256(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) v = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  return v;
}

// pass 1: masked FLAIR -> slice layout (the tile transpose of subject_prep_kernel) + per-block float64 sums
// grid (ceil(X/32), ceil(Y/32), Z), block (32, 8)
__global__ __launch_bounds__(256) void zscore_mask_sum_kernel(const float* __restrict__ f1,
                                                              const float* __restrict__ icv1,
                                                              const float* __restrict__ sl1, int X, int Y,
                                                              float* __restrict__ out, double* __restrict__ part) {
  __shared__ float tf[TS][TS + 1];
  __shared__ double sh[4];
  const int z = blockIdx.z;
  const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
  const size_t vbase = (size_t)z * X * Y;
  double s = 0.0;
  for (int j = threadIdx.y; j < TS; j += 8) {
    const int x = x0 + threadIdx.x, y = y0 + j;
    if (x < X && y < Y) {
      const float f = masked(f1, icv1, sl1, vbase + (size_t)y * X + x);
      tf[j][threadIdx.x] = f;
      s += (double)f;
    }
  }
  __syncthreads();
  for (int j = threadIdx.y; j < TS; j += 8) {
    const int x = x0 + j, y = y0 + threadIdx.x;
    if (x < X && y < Y) out[((size_t)z * X + x) * Y + y] = tf[threadIdx.x][j];
  }
  s = block_sum_256(s, sh);
  if (threadIdx.x == 0 && threadIdx.y == 0) part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
}

// pass 2: per-block float64 sums of (v - mean64)^2 over the slices pass 1 wrote; fixed grid ZS_PASS2_BLOCKS (or fewer)
__global__ __launch_bounds__(256) void zscore_sq_sum_kernel(const float* __restrict__ v, size_t n,
                                                            const double* __restrict__ dstat,
                                                            double* __restrict__ part) {
  __shared__ double sh[4];
  const double mean = dstat[0];
  double s = 0.0;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double d = (double)v[i] - mean;
    s += d * d;
  }
  s = block_sum_256(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one block: total of the partials in index order, divided by n.  final_std = 0: dstat[0] = mean64;
// final_std = 1: std64 = sqrt(total / n), then (mean32, std32) = the two rounded to float32 -> fstat (and stats_out)
__global__ __launch_bounds__(256) void zscore_final_kernel(const double* __restrict__ part, size_t nparts, double n,
                                                           int final_std, double* __restrict__ dstat,
                                                           float* __restrict__ fstat, float* __restrict__ stats_out) {
  __shared__ double sh[4];
  double s = 0.0;
  for (size_t i = threadIdx.x; i < nparts; i += 256) s += part[i];
  s = block_sum_256(s, sh);
  if (threadIdx.x == 0) {
    if (!final_std) {
      dstat[0] = __ddiv_rn(s, n);
    } else {
      const double sd = sqrt(__ddiv_rn(s, n));
      const float m32 = (float)dstat[0], s32 = (float)sd;
      dstat[1] = sd;
      fstat[0] = m32;
      fstat[1] = s32;
      if (stats_out) {
        stats_out[0] = m32;
        stats_out[1] = s32;
      }
    }
  }
}

// out = nan_to_num((out - mean32) / std32) in float32 (UT:510-512): NaN -> 0, +-inf -> +-FLT_MAX
__global__ __launch_bounds__(256) void zscore_apply_kernel(float* __restrict__ v, size_t n,
                                                           const float* __restrict__ fstat) {
#pragma clang fp contract(off)
  const float mean = fstat[0], sd = fstat[1];
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float q = __fdiv_rn(v[i] - mean, sd);
    if (q != q) q = 0.0f;
    else if (__builtin_isinf(q)) q = q > 0.0f ? 3.402823466e+38f : -3.402823466e+38f;
    v[i] = q;
  }
}

// out = (vol [* m_a]) [* (1 - sl)] in slice layout: every other array UT / UE build from a volume and its masks
// (UT:494-502 brain_wsc_1tp; UE:512-532 brain_wmh_1tp / _2tp, brain_cod_2tp, icv_and_sl_mask_1tp / _2tp)
// grid (ceil(X/32), ceil(Y/32), Z), block (32, 8)
__global__ __launch_bounds__(256) void mask_slices_kernel(const float* __restrict__ vol, const float* __restrict__ m_a,
                                                          const float* __restrict__ sl, int X, int Y,
                                                          float* __restrict__ out) {
  __shared__ float t[TS][TS + 1];
  const int z = blockIdx.z;
  const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
  const size_t vbase = (size_t)z * X * Y;
  for (int j = threadIdx.y; j < TS; j += 8) {
    const int x = x0 + threadIdx.x, y = y0 + j;
    if (x < X && y < Y) {
      const size_t i = vbase + (size_t)y * X + x;
      float r = vol[i];
      if (m_a) r = __fmul_rn(r, m_a[i]);
      if (sl) r = __fmul_rn(r, __fsub_rn(1.0f, sl[i]));
      t[j][threadIdx.x] = r;
    }
  }
  __syncthreads();
  for (int j = threadIdx.y; j < TS; j += 8) {
    const int x = x0 + j, y = y0 + threadIdx.x;
    if (x < X && y < Y) out[((size_t)z * X + x) * Y + y] = t[threadIdx.x][j];
  }
}

// UT:563-566 (convert_to_1hot after astype(int)): onehot[i][c] = (c == trunc(coded[i])), (npix, C) float32.  A value
// whose truncation is outside [0, C) (NaN included) gets an all-zero row and is counted in *bad.
__global__ __launch_bounds__(256) void onehot_kernel(const float* __restrict__ coded, size_t npix, int C,
                                                     float* __restrict__ out, unsigned int* __restrict__ bad) {
  const size_t n = npix * (size_t)C;
  for (size_t j = blockIdx.x * (size_t)256 + threadIdx.x; j < n; j += (size_t)gridDim.x * 256) {
    const size_t i = j / (size_t)C;
    const int c = (int)(j - i * (size_t)C);
    const float v = coded[i];
    const bool ok = v > -1.0f && v < (float)C;      // trunc(v) in [0, C); false for NaN
    const int k = ok ? (int)v : -1;                 // (int) truncates toward zero, as astype(int)
    out[j] = (c == k) ? 1.0f : 0.0f;
    if (!ok && c == 0) atomicAdd(bad, 1u);
  }
}

}  // namespace

extern "C" {

size_t depgan_data_prep_scratch_floats(int X, int Y, int Z) {
  if (X <= 0 || Y <= 0 || Z <= 0) return 0;
  return 2 * (size_t)cdiv(X, TS) * cdiv(Y, TS) * Z + 2;
}

int depgan_data_prep_subject(const float* p1, const float* f1, const float* icv1, const float* sl1, const float* p2,
                             const float* icv2, const float* sl2, int X, int Y, int Z, int nicg, float* x_out,
                             float* y2_out, float* scratch, void* stream) {
  if (!p1 || !icv1 || !p2 || !icv2 || !x_out || !y2_out || X <= 0 || Y <= 0 || Z <= 0 || (nicg != 1 && nicg != 2) ||
      (nicg == 2 && (!f1 || !scratch))) {
    dg_set_error("data_prep_subject: bad argument (X=%d Y=%d Z=%d nicg=%d)", X, Y, Z, nicg);
    return DG_ERR_ARG;
  }
  if (Z > 65535 || cdiv(Y, TS) > 65535) {
    dg_set_error("data_prep_subject: volume too large for one launch (Y=%d Z=%d)", Y, Z);
    return DG_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(cdiv(X, TS), cdiv(Y, TS), Z);
  const size_t nblk = (size_t)grid.x * grid.y * grid.z;
  hipLaunchKernelGGL(subject_prep_kernel, grid, dim3(32, 8), 0, st, p1, f1, icv1, sl1, p2, icv2, sl2, X, Y, nicg, x_out,
                     y2_out, scratch);
  HIPCHECK(hipGetLastError());
  if (nicg == 2) {
    float* mm = scratch + 2 * nblk;
    hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(256), 0, st, scratch, nblk, mm);
    HIPCHECK(hipGetLastError());
    const size_t npix = (size_t)X * Y * Z;
    const int blocks = (int)((npix + 255) / 256 < 2048 ? (npix + 255) / 256 : 2048);
    hipLaunchKernelGGL(flair_normalise_kernel, dim3(blocks), dim3(256), 0, st, x_out, npix, mm, 0.0f, 1.0f);
    HIPCHECK(hipGetLastError());
  }
  return DG_OK;
}

// scratch of depgan_data_prep_zscore: max(pass-1 blocks, ZS_PASS2_BLOCKS) float64 partials, 2 float64 statistics,
// 2 float32 statistics -- counted in floats
size_t depgan_data_zscore_scratch_floats(int X, int Y, int Z) {
  if (X <= 0 || Y <= 0 || Z <= 0) return 0;
  const size_t nblk = (size_t)cdiv(X, TS) * cdiv(Y, TS) * Z;
  const size_t nparts = nblk > (size_t)ZS_PASS2_BLOCKS ? nblk : (size_t)ZS_PASS2_BLOCKS;
  return 2 * (nparts + 2) + 2;
}

int depgan_data_prep_zscore(const float* f1, const float* icv1, const float* sl1, int X, int Y, int Z,
                            float* flair_out, float* stats_out, float* scratch, void* stream) {
  if (!f1 || !icv1 || !flair_out || !scratch || X <= 0 || Y <= 0 || Z <= 0 || ((uintptr_t)scratch & 7)) {
    dg_set_error("data_prep_zscore: bad argument (X=%d Y=%d Z=%d; scratch must be 8-byte aligned)", X, Y, Z);
    return DG_ERR_ARG;
  }
  if (Z > 65535 || cdiv(Y, TS) > 65535) {
    dg_set_error("data_prep_zscore: volume too large for one launch (Y=%d Z=%d)", Y, Z);
    return DG_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(cdiv(X, TS), cdiv(Y, TS), Z);
  const size_t nblk = (size_t)grid.x * grid.y * grid.z;
  const size_t nparts = nblk > (size_t)ZS_PASS2_BLOCKS ? nblk : (size_t)ZS_PASS2_BLOCKS;
  double* part = (double*)scratch;
  double* dstat = part + nparts;
  float* fstat = (float*)(dstat + 2);
  const size_t npix = (size_t)X * Y * Z;
  const int blocks2 = (int)((npix + 255) / 256 < (size_t)ZS_PASS2_BLOCKS ? (npix + 255) / 256 : ZS_PASS2_BLOCKS);
  hipLaunchKernelGGL(zscore_mask_sum_kernel, grid, dim3(32, 8), 0, st, f1, icv1, sl1, X, Y, flair_out, part);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(zscore_final_kernel, dim3(1), dim3(256), 0, st, part, nblk, (double)npix, 0, dstat, fstat,
                     stats_out);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(zscore_sq_sum_kernel, dim3(blocks2), dim3(256), 0, st, flair_out, npix, dstat, part);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(zscore_final_kernel, dim3(1), dim3(256), 0, st, part, (size_t)blocks2, (double)npix, 1, dstat,
                     fstat, stats_out);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(zscore_apply_kernel, dim3(blocks2), dim3(256), 0, st, flair_out, npix, fstat);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

int depgan_data_mask_slices(const float* vol, const float* m_a, const float* sl, int X, int Y, int Z, float* out,
                            void* stream) {
  if (!vol || !out || X <= 0 || Y <= 0 || Z <= 0) {
    dg_set_error("data_mask_slices: bad argument (X=%d Y=%d Z=%d)", X, Y, Z);
    return DG_ERR_ARG;
  }
  if (Z > 65535 || cdiv(Y, TS) > 65535) {
    dg_set_error("data_mask_slices: volume too large for one launch (Y=%d Z=%d)", Y, Z);
    return DG_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(mask_slices_kernel, dim3(cdiv(X, TS), cdiv(Y, TS), Z), dim3(32, 8), 0, (hipStream_t)stream, vol,
                     m_a, sl, X, Y, out);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

int depgan_labels_to_onehot(const float* coded, long npix, int C, float* onehot_out, void* stream) {
  if (!coded || !onehot_out || npix < 0 || C < 1 || C > DEPGAN_MAX_CLASSES) {
    dg_set_error("labels_to_onehot: bad argument (npix=%ld C=%d)", npix, C);
    return DG_ERR_ARG;
  }
  if (npix == 0) return DG_OK;
  hipStream_t st = (hipStream_t)stream;
  unsigned int* bad = nullptr;
  HIPCHECK(hipMalloc((void**)&bad, sizeof(unsigned int)));
  unsigned int h = 0;
  int rc = DG_OK;
  const size_t n = (size_t)npix * C;
  const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  if (hipMemsetAsync(bad, 0, sizeof(unsigned int), st) != hipSuccess) {
    dg_set_error("labels_to_onehot: memset failed");
    rc = DG_ERR_HIP;
  } else {
    hipLaunchKernelGGL(onehot_kernel, dim3(blocks), dim3(256), 0, st, coded, (size_t)npix, C, onehot_out, bad);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&h, bad, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      dg_set_error("labels_to_onehot: launch or copy back failed");
      rc = DG_ERR_HIP;
    } else if (h) {
      dg_set_error("labels_to_onehot: %u of %ld values truncate to a class outside [0, %d)", h, npix, C);
      rc = DG_ERR_ARG;
    }
  }
  hipFree(bad);
  return rc;
}

}  // extern "C"
