// Evaluation step of the DEP-UResNet (DEP-UResNet_testing_4fold.py "UE":553-700): the C-channel counterpart of the
// GE kernels in ops.hip.
//
//   output_img_pred_mean += pred * icv_and_sl_mask_2tp       (UE:553-560; float32 product broadcast over the channels,
//                                                             float64 running sum: np.zeros accumulator)
//   label = np.argmax(mean, channel axis)                     (convert_from_1hot, UE:166-185; first index wins on ties)
//   volumes and six Dice figures from the label map           (UE:570-697)
//
// Both are HBM-bound elementwise passes; the census is one grid-stride pass with per-thread integer counters,
// folded per block in LDS and per grid with one 64-bit integer atomic per counter and block (exact in any order).
#include "common.h"

#include "model.h"

namespace {

inline int grid_for(size_t n, int cap) {
  const size_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b < (size_t)cap ? b : (size_t)cap));
}

// acc[i*C + c] += (double)(pred[i*C + c] * mask[i])      (UE:557-558; mask NULL = 1)
__global__ __launch_bounds__(256) void eval_accumulate_channels_kernel(const float* __restrict__ pred,
                                                                       const float* __restrict__ mask,
                                                                       double* __restrict__ acc, size_t npix, int C) {
  const size_t n = npix * (size_t)C;
  for (size_t j = blockIdx.x * (size_t)256 + threadIdx.x; j < n; j += (size_t)gridDim.x * 256) {
    const float m = mask ? mask[j / (size_t)C] : 1.0f;
    acc[j] = __dadd_rn(acc[j], (double)__fmul_rn(pred[j], m));
  }
}

//  [0] nnz(mask1*wmh1)  [1] nnz(mask2*wmh2)  [2] #(label > 0)
//  [3+3(k-1) ..] for k = 1,2,3: #(label == k & real == k), #(real == k), #(label == k)
//  [12..14] the same for > 0 (whole WMH), [15..17] for in {1,2} (changing WMH)
// real = code_real, a float32 array compared with integers as NumPy does (UE:626-697); NULL = all zero
__global__ __launch_bounds__(256) void eval_label_counts_kernel(const double* __restrict__ pred, int C,
                                                                const float* __restrict__ code_real,
                                                                const float* __restrict__ mask1,
                                                                const float* __restrict__ wmh1,
                                                                const float* __restrict__ mask2,
                                                                const float* __restrict__ wmh2, size_t npix,
                                                                signed char* __restrict__ labels,
                                                                unsigned long long* __restrict__ out) {
  __shared__ unsigned int sh[DEPGAN_EVAL_LABEL_NCOUNT];
  if (threadIdx.x < DEPGAN_EVAL_LABEL_NCOUNT) sh[threadIdx.x] = 0;
  __syncthreads();
  unsigned int c[DEPGAN_EVAL_LABEL_NCOUNT];
#pragma unroll
  for (int k = 0; k < DEPGAN_EVAL_LABEL_NCOUNT; ++k) c[k] = 0;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
    // np.argmax: the first maximum; a NaN counts as the maximum (its first occurrence wins)
    const double* p = pred + i * (size_t)C;
    int lab = 0;
    double best = p[0];
    if (best == best) {
      for (int ch = 1; ch < C; ++ch) {
        const double v = p[ch];
        if (v != v) {
          lab = ch;
          break;
        }
        if (v > best) {
          best = v;
          lab = ch;
        }
      }
    }
    if (labels) labels[i] = (signed char)lab;
    if (mask1 && wmh1) c[0] += (__fmul_rn(mask1[i], wmh1[i]) != 0.0f);
    if (mask2 && wmh2) c[1] += (__fmul_rn(mask2[i], wmh2[i]) != 0.0f);
    c[2] += (lab > 0);
    const float r = code_real ? code_real[i] : 0.0f;
#pragma unroll
    for (int k = 1; k <= 3; ++k) {
      const bool rk = (r == (float)k), fk = (lab == k);
      c[3 + 3 * (k - 1)] += (rk && fk);
      c[4 + 3 * (k - 1)] += rk;
      c[5 + 3 * (k - 1)] += fk;
    }
    {
      const bool rk = r > 0.0f, fk = lab > 0;
      c[12] += (rk && fk); c[13] += rk; c[14] += fk;
    }
    {
      const bool rk = (r == 1.0f) || (r == 2.0f), fk = (lab == 1) || (lab == 2);
      c[15] += (rk && fk); c[16] += rk; c[17] += fk;
    }
  }
#pragma unroll
  for (int k = 0; k < DEPGAN_EVAL_LABEL_NCOUNT; ++k)
    if (c[k]) atomicAdd(&sh[k], c[k]);       // integer adds: any order gives the same total
  __syncthreads();
  if (threadIdx.x < DEPGAN_EVAL_LABEL_NCOUNT && sh[threadIdx.x])
    atomicAdd(&out[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

}  // namespace

extern "C" {

int depgan_eval_accumulate_channels(const float* pred, const float* mask, double* acc, long npix, int C,
                                    void* stream) {
  if (!pred || !acc || npix < 0 || C < 1) {
    dg_set_error("eval_accumulate_channels: bad argument (npix=%ld C=%d)", npix, C);
    return DG_ERR_ARG;
  }
  if (npix == 0) return DG_OK;
  hipLaunchKernelGGL(eval_accumulate_channels_kernel, dim3(grid_for((size_t)npix * C, 2048)), dim3(256), 0,
                     (hipStream_t)stream, pred, mask, acc, (size_t)npix, C);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

int depgan_eval_label_counts(const double* pred, int C, const float* code_real, const float* mask1, const float* wmh1,
                             const float* mask2, const float* wmh2, long npix, signed char* labels_out,
                             long long out_host[DEPGAN_EVAL_LABEL_NCOUNT], void* stream) {
  if (!pred || !out_host || C < 1 || C > DEPGAN_MAX_CLASSES || npix < 0) {
    dg_set_error("eval_label_counts: bad argument (npix=%ld C=%d)", npix, C);
    return DG_ERR_ARG;
  }
  for (int k = 0; k < DEPGAN_EVAL_LABEL_NCOUNT; ++k) out_host[k] = 0;
  if (npix == 0) return DG_OK;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* dev = nullptr;
  HIPCHECK(hipMalloc((void**)&dev, DEPGAN_EVAL_LABEL_NCOUNT * sizeof(unsigned long long)));
  int rc = DG_OK;
  unsigned long long h[DEPGAN_EVAL_LABEL_NCOUNT];
  if (hipMemsetAsync(dev, 0, sizeof(h), st) != hipSuccess) {
    dg_set_error("eval_label_counts: memset failed");
    rc = DG_ERR_HIP;
  } else {
    hipLaunchKernelGGL(eval_label_counts_kernel, dim3(grid_for((size_t)npix, 1024)), dim3(256), 0, st, pred, C,
                       code_real, mask1, wmh1, mask2, wmh2, (size_t)npix, labels_out, dev);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, dev, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      dg_set_error("eval_label_counts: launch or copy back failed");
      rc = DG_ERR_HIP;
    } else {
      for (int k = 0; k < DEPGAN_EVAL_LABEL_NCOUNT; ++k) out_host[k] = (long long)h[k];
    }
  }
  hipFree(dev);
  return rc;
}

}  // extern "C"
