// Training-time augmentation of the resident slice set (DEP-UResNet fit): the batch gather, an affine warp of the
// image (bilinear) and of its labels (nearest), and a gain / offset on the intensities, in one pass.
//
//   out[i] = warp(x_src[index[i]], params[i]),  lab_out[i] = warp_nearest(lab_src[index[i]], params[i])
//
// params row i: a00 a01 a02 a10 a11 a12 gain offset, the output-to-source map
//   sy = (a00*oy + a01*ox) + a02          sx = (a10*oy + a11*ox) + a12
//   y0 = floorf(sy); fy = sy - y0         x0 = floorf(sx); fx = sx - x0
//   top = v(y0,x0)*(1-fx) + v(y0,x0+1)*fx
//   bot = v(y0+1,x0)*(1-fx) + v(y0+1,x0+1)*fx
//   out = gain*(top*(1-fy) + bot*fy) + offset                              per channel
//   label: row (floorf(sy+0.5f), floorf(sx+0.5f)) of the source labels, copied bit for bit
// Every operation is one correctly rounded float32 operation in that order (no contraction into FMAs), so a NumPy
// restatement with float32 operands gives the same bits (tests/augment_ref.py).
//
// Memory-bound: 4*nicg bytes read (the four taps of neighbouring lanes share cache lines) and written per pixel, plus
// the label row.  One thread per output pixel over all channels and the label row; consecutive lanes walk ox, so
// stores are coalesced and the reads of a near-axis-aligned map are close to it.  No atomics; no LDS but the 384 bytes
// in which a block of augment_fields_kernel shares its collapsed control rows.
//
// depgan_data_augment_fields adds, in the same launch, an elastic displacement of the source coordinate and a smooth
// multiplicative bias on the intensities: three low-resolution control grids per output sample, evaluated at every
// output pixel as a cubic B-spline (include/depgan.h states it operation by operation)
//   sy' = sy + f_dy   sx' = sx + f_dx   out = gain*((top*(1-fy) + bot*fy) * (1 + f_b)) + offset
// and the taps, the bilinear weights and the nearest label are the statements above on sy', sx'.
//
// Tap addressing never leaves the source: a tap coordinate is compared and clamped as a float BEFORE it becomes an
// integer (a coordinate may be anything, +-inf and NaN included), and a sample whose index is outside [0, n_src) reads
// nothing at all.
#include "common.h"

#include "model.h"

// every float operation below is rounded on its own, as NumPy's statement sequence is
#pragma clang fp contract(off)

namespace {

// f: an integral-valued float (or +-inf / NaN).  Returns the tap index clamped into [0, n); *in says whether f itself
// was inside (false for NaN, which clamps to 0).
__device__ __forceinline__ int tap(float f, int n, bool* in) {
  const float hi = (float)(n - 1);                   // exact: n <= 2^24 (checked by the entry)
  *in = f >= 0.0f && f <= hi;
  return (int)fminf(fmaxf(f, 0.0f), hi);
}

template <int K>
__device__ __forceinline__ void copy_row(unsigned* __restrict__ dst, const unsigned* __restrict__ src) {
#pragma unroll
  for (int k = 0; k < K; ++k) dst[k] = src[k];
}

template <int K>
__device__ __forceinline__ void fill_row(float* __restrict__ dst, int hot) {
#pragma unroll
  for (int k = 0; k < K; ++k) dst[k] = (k == hot) ? 1.0f : 0.0f;
}

template <int K>
__device__ __forceinline__ void put_row(float* dst, const float* src, bool in, int hot) {
  if (in) copy_row<K>((unsigned*)dst, (const unsigned*)src);
  else fill_row<K>(dst, hot);
}

struct AugArgs {
  const float* x_src;
  const void* lab_src;
  const long* index;
  const float* params;
  float* x_out;
  void* lab_out;
  long n_src;
  long total;          // n * H * W
  int H, W, C;
  int constant;        // border: 0 edge, 1 constant
  float x_fill;
  int label_fill;
};

// Output pixel t of a sample whose index is outside the set: the fill values, nothing of the source is read.
template <int NICG, int LAB>
__device__ __forceinline__ void fill_pixel(const AugArgs& a, long t) {
  float* xo = a.x_out + (size_t)t * NICG;
#pragma unroll
  for (int c = 0; c < NICG; ++c) xo[c] = a.x_fill;
  if (LAB == 1) ((unsigned char*)a.lab_out)[t] = (unsigned char)a.label_fill;
  if (LAB == 2) {
    float* lo = (float*)a.lab_out + (size_t)t * a.C;
    for (int k = 0; k < a.C; ++k) lo[k] = (k == a.label_fill) ? 1.0f : 0.0f;
  }
}

// Output pixel t from source coordinate (sy, sx) of slice s, 0 <= s < n_src: the image bilinearly, the label row of
// the nearest pixel.  BIAS: the interpolated value is multiplied by `bias` before the gain (depgan_data_augment_fields).
template <int NICG, int LAB, bool BIAS>
__device__ __forceinline__ void sample_pixel(const AugArgs& a, long s, float sy, float sx, float gain, float offset,
                                             float bias, long t) {
  const int H = a.H, W = a.W;
  const unsigned HW = (unsigned)H * (unsigned)W;     // <= 2^31 - 1 (checked by the entry)
  float* xo = a.x_out + (size_t)t * NICG;

  // ---- image: bilinear ----
  {
    const float y0 = floorf(sy), x0 = floorf(sx);
    const float fy = sy - y0, fx = sx - x0;
    const float gy = 1.0f - fy, gx = 1.0f - fx;
    bool iy0, iy1, ix0, ix1;
    const int ty0 = tap(y0, H, &iy0), ty1 = tap(y0 + 1.0f, H, &iy1);
    const int tx0 = tap(x0, W, &ix0), tx1 = tap(x0 + 1.0f, W, &ix1);
    const float* src = a.x_src + (size_t)s * HW * NICG;
    const float* r0 = src + (size_t)ty0 * W * NICG;
    const float* r1 = src + (size_t)ty1 * W * NICG;
    float v00[NICG], v01[NICG], v10[NICG], v11[NICG];
#pragma unroll
    for (int c = 0; c < NICG; ++c) {                 // clamped addresses: always inside the slice
      v00[c] = r0[tx0 * NICG + c];
      v01[c] = r0[tx1 * NICG + c];
      v10[c] = r1[tx0 * NICG + c];
      v11[c] = r1[tx1 * NICG + c];
    }
    if (a.constant) {
#pragma unroll
      for (int c = 0; c < NICG; ++c) {
        if (!(iy0 && ix0)) v00[c] = a.x_fill;
        if (!(iy0 && ix1)) v01[c] = a.x_fill;
        if (!(iy1 && ix0)) v10[c] = a.x_fill;
        if (!(iy1 && ix1)) v11[c] = a.x_fill;
      }
    }
#pragma unroll
    for (int c = 0; c < NICG; ++c) {
      const float top = v00[c] * gx + v01[c] * fx;
      const float bot = v10[c] * gx + v11[c] * fx;
      float v = top * gy + bot * fy;
      if (BIAS) v = v * bias;
      xo[c] = gain * v + offset;
    }
  }

  // ---- labels: nearest ----
  if (LAB != 0) {
    bool iy, ix;
    const int ly = tap(floorf(sy + 0.5f), H, &iy), lx = tap(floorf(sx + 0.5f), W, &ix);
    const bool in = !a.constant || (iy && ix);
    const size_t at = (size_t)s * HW + (size_t)ly * W + lx;
    if (LAB == 1) {
      const unsigned char v = ((const unsigned char*)a.lab_src)[at];
      ((unsigned char*)a.lab_out)[t] = in ? v : (unsigned char)a.label_fill;
    } else {
      const int C = a.C;
      const float* ls = (const float*)a.lab_src + at * C;
      float* lo = (float*)a.lab_out + (size_t)t * C;
      switch (C) {                                   // uniform; a constant row length lets the copies be wide
        case 2: put_row<2>(lo, ls, in, a.label_fill); break;
        case 3: put_row<3>(lo, ls, in, a.label_fill); break;
        case 4: put_row<4>(lo, ls, in, a.label_fill); break;
        case 5: put_row<5>(lo, ls, in, a.label_fill); break;
        case 6: put_row<6>(lo, ls, in, a.label_fill); break;
        case 7: put_row<7>(lo, ls, in, a.label_fill); break;
        default: put_row<8>(lo, ls, in, a.label_fill); break;
      }
    }
  }
}

// One output pixel: sample i, pixel pix = oy * W + ox of it, flat output pixel t.
template <int NICG, int LAB>
__device__ __forceinline__ void augment_pixel(const AugArgs& a, long i, unsigned pix, long t) {
  const unsigned W = (unsigned)a.W;
  const int oy = (int)(pix / W), ox = (int)(pix - (unsigned)oy * W);
  const long s = a.index ? a.index[i] : i;
  if (s < 0 || s >= a.n_src) return fill_pixel<NICG, LAB>(a, t);
  const float* p = a.params + (size_t)i * DEPGAN_AUG_NPARAM;
  const float a00 = p[0], a01 = p[1], a02 = p[2], a10 = p[3], a11 = p[4], a12 = p[5], gain = p[6], offset = p[7];
  const float fyo = (float)oy, fxo = (float)ox;
  const float sy = (a00 * fyo + a01 * fxo) + a02;
  const float sx = (a10 * fyo + a11 * fxo) + a12;
  sample_pixel<NICG, LAB, false>(a, s, sy, sx, gain, offset, 1.0f, t);
}

// LAB: 0 none, 1 uint8 codes, 2 one-hot float32 rows of a.C.  grid ceil(total / 256), block 256, thread = output pixel.
// A block whose 256 pixels lie in one sample (every block when H*W is a multiple of 256) takes the sample number from
// the block number alone, so the index and the parameter row are uniform loads and no lane divides by H*W.
template <int NICG, int LAB>
__global__ __launch_bounds__(256) void augment_kernel(const AugArgs a) {
  const unsigned HW = (unsigned)a.H * (unsigned)a.W;
  const long t0 = (long)blockIdx.x * 256;
  const bool small = a.total <= 0xFFFFFFFFL;         // then 32-bit divisions, a fraction of the 64-bit ones
  const long i0 = small ? (long)((unsigned)t0 / HW) : t0 / HW;
  const long first = t0 - i0 * HW;                   // pixel of the block's first thread within sample i0
  const long t = t0 + threadIdx.x;
  if (t >= a.total) return;
  if (first + 255 < (long)HW) {
    augment_pixel<NICG, LAB>(a, i0, (unsigned)first + threadIdx.x, t);
  } else {
    const long i = small ? (long)((unsigned)t / HW) : t / HW;
    augment_pixel<NICG, LAB>(a, i, (unsigned)(t - i * HW), t);
  }
}

// ---- depgan_data_augment_fields ----

struct FieldArgs {
  const float* fields;   // (n, 3, gh, gw)
  float* dense;          // NULL or (n, H, W, 3)
  float ky, kx;          // control cells per pixel, rounded once on the host
  int gh, gw;
};

// Output coordinate o along an axis of g control points: its cell c (returned; 0 <= c <= g - 4, since u is finite and
// >= 0) and six times the four cubic B-spline weights at t = u - c.
__device__ __forceinline__ int spline_cell(int o, float k, int g, float* B) {
  const float u = (float)o * k;
  const float c = fminf(floorf(u), (float)(g - 4));
  const float t = u - c;
  const float t2 = t * t;
  const float t3 = t2 * t;
  const float gt = 1.0f - t;
  B[0] = (gt * gt) * gt;
  B[1] = (3.0f * t3 - 6.0f * t2) + 4.0f;
  B[2] = ((3.0f * t2 - 3.0f * t3) + 3.0f * t) + 1.0f;
  B[3] = t3;
  return (int)c;
}

// r[j] of the header: column j of four consecutive control rows (Cj points at the first) under the y-weights
__device__ __forceinline__ float spline_rows(const float* Cj, int gw, const float* By) {
  return ((By[0] * Cj[0] + By[1] * Cj[gw]) + By[2] * Cj[2 * gw]) + By[3] * Cj[3 * gw];
}

__device__ __forceinline__ float spline_across(const float* r, const float* Bx) {
  return (((Bx[0] * r[0] + Bx[1] * r[1]) + Bx[2] * r[2]) + Bx[3] * r[3]) * (1.0f / 36.0f);
}

// One output pixel (oy, ox) of sample i.  rows: the block's r[plane][0..gw) in LDS when all its pixels share (i, oy),
// else NULL and the lane collapses its own four columns from the grid; the statements are the same either way.
template <int NICG, int LAB>
__device__ __forceinline__ void fields_pixel(const AugArgs& a, const FieldArgs& fa, long i, int oy, int ox, long t,
                                             const float* rows) {
  const long s = a.index ? a.index[i] : i;
  if (s < 0 || s >= a.n_src) {
    fill_pixel<NICG, LAB>(a, t);
    if (fa.dense) {
      float* d = fa.dense + (size_t)t * 3;
      d[0] = 0.0f, d[1] = 0.0f, d[2] = 0.0f;
    }
    return;
  }
  const int gh = fa.gh, gw = fa.gw;
  float Bx[4], f[3];
  const int cx = spline_cell(ox, fa.kx, gw, Bx);
  if (rows) {
#pragma unroll
    for (int p = 0; p < 3; ++p) f[p] = spline_across(rows + p * gw + cx, Bx);
  } else {
    float By[4];
    const int cy = spline_cell(oy, fa.ky, gh, By);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const float* Cp = fa.fields + (((size_t)i * 3 + p) * gh + cy) * gw + cx;
      float r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = spline_rows(Cp + j, gw, By);
      f[p] = spline_across(r, Bx);
    }
  }
  if (fa.dense) {
    float* d = fa.dense + (size_t)t * 3;
    d[0] = f[0], d[1] = f[1], d[2] = f[2];
  }
  const float* p = a.params + (size_t)i * DEPGAN_AUG_NPARAM;
  const float a00 = p[0], a01 = p[1], a02 = p[2], a10 = p[3], a11 = p[4], a12 = p[5], gain = p[6], offset = p[7];
  const float fyo = (float)oy, fxo = (float)ox;
  const float sy = (a00 * fyo + a01 * fxo) + a02;
  const float sx = (a10 * fyo + a11 * fxo) + a12;
  sample_pixel<NICG, LAB, true>(a, s, sy + f[0], sx + f[1], gain, offset, 1.0f + f[2], t);
}

// Grid, block and the sample-uniform case as augment_kernel.  A block whose 256 pixels lie in one image row as well
// (every block when W is a multiple of 256) has one c_y and one set of y-weights: its first 3 * gw threads collapse
// the four control rows of the three planes into LDS once (<= 384 B), and after one barrier a lane takes four LDS
// values per plane in place of sixteen grid values.  Any other block evaluates per lane, from the grid.
template <int NICG, int LAB>
__global__ __launch_bounds__(256) void augment_fields_kernel(const AugArgs a, const FieldArgs fa) {
  __shared__ float rows[3 * DEPGAN_AUG_MAX_GRID];
  const unsigned W = (unsigned)a.W, HW = (unsigned)a.H * W;
  const long t0 = (long)blockIdx.x * 256;
  const bool small = a.total <= 0xFFFFFFFFL;
  const long i0 = small ? (long)((unsigned)t0 / HW) : t0 / HW;
  const long first = t0 - i0 * HW;                   // pixel of the block's first thread within sample i0
  const long t = t0 + threadIdx.x;
  const unsigned oy0 = (unsigned)first / W, ox0 = (unsigned)first - oy0 * W;
  if (first + 255 < (long)HW && ox0 + 255 < W) {     // block-uniform: every thread is a pixel of row oy0 of sample i0
    const int gw = fa.gw;
    if ((int)threadIdx.x < 3 * gw) {
      const int p = (int)threadIdx.x / gw, j = (int)threadIdx.x - p * gw;
      float By[4];
      const int cy = spline_cell((int)oy0, fa.ky, fa.gh, By);
      rows[threadIdx.x] = spline_rows(fa.fields + (((size_t)i0 * 3 + p) * fa.gh + cy) * gw + j, gw, By);
    }
    __syncthreads();
    fields_pixel<NICG, LAB>(a, fa, i0, (int)oy0, (int)(ox0 + threadIdx.x), t, rows);
  } else {
    if (t >= a.total) return;
    const long i = first + 255 < (long)HW ? i0 : (small ? (long)((unsigned)t / HW) : t / HW);
    const unsigned pix = (unsigned)(t - i * HW);
    const int oy = (int)(pix / W);
    fields_pixel<NICG, LAB>(a, fa, i, oy, (int)(pix - (unsigned)oy * W), t, nullptr);
  }
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || !na || !nb) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// fa NULL: augment_kernel, else augment_fields_kernel
template <int NICG, int LAB>
void launch_one(int blocks, hipStream_t st, const AugArgs& a, const FieldArgs* fa) {
  if (fa) hipLaunchKernelGGL((augment_fields_kernel<NICG, LAB>), dim3(blocks), dim3(256), 0, st, a, *fa);
  else hipLaunchKernelGGL((augment_kernel<NICG, LAB>), dim3(blocks), dim3(256), 0, st, a);
}

template <int NICG>
void launch(int lab_kind, int blocks, hipStream_t st, const AugArgs& a, const FieldArgs* fa) {
  if (lab_kind == 0) launch_one<NICG, 0>(blocks, st, a, fa);
  else if (lab_kind == 1) launch_one<NICG, 1>(blocks, st, a, fa);
  else launch_one<NICG, 2>(blocks, st, a, fa);
}

// Both entries: the checks, the arguments and the launch.  with_fields says which; `what` names it in error texts.
int augment(const char* what, bool with_fields, const float* x_src, int nicg, const void* lab_src, int lab_kind, int C,
            const long* index_dev, long n_src, const float* params_dev, const float* fields_dev, int gh, int gw, int n,
            int H, int W, int border, float x_fill, int label_fill, float* x_out, void* lab_out, float* dense_out,
            void* stream) {
  if (n < 1 || H < 1 || W < 1 || n_src < 1 || nicg < 1 || nicg > 2 || lab_kind < 0 || lab_kind > 2 ||
      (border != 0 && border != 1) || !x_src || !params_dev || !x_out ||
      (lab_kind != 0 && (!lab_src || !lab_out)) ||
      (lab_kind == 2 && (C < 2 || C > DEPGAN_MAX_HEAD_CLASSES || label_fill >= C)) ||
      (lab_kind == 1 && (label_fill < 0 || label_fill > 255)) || (!index_dev && n_src < n)) {
    dg_set_error("%s: bad argument (n=%d H=%d W=%d nicg=%d lab_kind=%d C=%d n_src=%ld border=%d label_fill=%d)", what,
                 n, H, W, nicg, lab_kind, C, n_src, border, label_fill);
    return DG_ERR_ARG;
  }
  if (with_fields && (!fields_dev || gh < 4 || gh > DEPGAN_AUG_MAX_GRID || gw < 4 || gw > DEPGAN_AUG_MAX_GRID)) {
    dg_set_error("%s: fields_dev is NULL or the control grid is outside [4, %d] (gh=%d gw=%d)", what,
                 DEPGAN_AUG_MAX_GRID, gh, gw);
    return DG_ERR_ARG;
  }
  if (H > (1 << 24) || W > (1 << 24) || (long)H * W > 0x7FFFFFFFL) {
    dg_set_error("%s: image too large (H=%d W=%d)", what, H, W);
    return DG_ERR_UNSUPPORTED;
  }
  const size_t hw = (size_t)H * W;
  const size_t total = (size_t)n * hw;
  if ((total + 255) / 256 > 0x7FFFFFFFul) {
    dg_set_error("%s: batch too large for one launch (n=%d H=%d W=%d)", what, n, H, W);
    return DG_ERR_UNSUPPORTED;
  }
  const size_t lab_px = lab_kind == 1 ? 1 : lab_kind == 2 ? 4 * (size_t)C : 0;
  const void* srcs[5] = {x_src, lab_src, index_dev, params_dev, with_fields ? fields_dev : nullptr};
  const size_t src_bytes[5] = {(size_t)n_src * hw * nicg * 4, (size_t)n_src * hw * lab_px, (size_t)n * sizeof(long),
                               (size_t)n * DEPGAN_AUG_NPARAM * 4, with_fields ? (size_t)n * 3 * gh * gw * 4 : 0};
  const void* outs[3] = {x_out, lab_out, with_fields ? dense_out : nullptr};
  const size_t out_bytes[3] = {total * nicg * 4, total * lab_px, total * 3 * 4};
  for (int o = 0; o < 3; ++o) {
    for (int k = 0; k < 5; ++k) {
      if (overlaps(outs[o], out_bytes[o], srcs[k], src_bytes[k])) {
        dg_set_error("%s: an output range overlaps a source range", what);
        return DG_ERR_ARG;
      }
    }
    for (int q = 0; q < o; ++q) {
      if (overlaps(outs[o], out_bytes[o], outs[q], out_bytes[q])) {
        dg_set_error("%s: two output ranges overlap", what);
        return DG_ERR_ARG;
      }
    }
  }
  AugArgs a;
  a.x_src = x_src;
  a.lab_src = lab_kind ? lab_src : nullptr;
  a.index = index_dev;
  a.params = params_dev;
  a.x_out = x_out;
  a.lab_out = lab_kind ? lab_out : nullptr;
  a.n_src = n_src;
  a.total = (long)total;
  a.H = H;
  a.W = W;
  a.C = C;
  a.constant = border;
  a.x_fill = x_fill;
  a.label_fill = label_fill;
  FieldArgs fa;
  if (with_fields) {
    fa.fields = fields_dev;
    fa.dense = dense_out;
    fa.ky = H > 1 ? (float)((double)(gh - 3) / (double)(H - 1)) : 0.0f;
    fa.kx = W > 1 ? (float)((double)(gw - 3) / (double)(W - 1)) : 0.0f;
    fa.gh = gh;
    fa.gw = gw;
  }
  const int blocks = (int)((total + 255) / 256);
  if (nicg == 1) launch<1>(lab_kind, blocks, (hipStream_t)stream, a, with_fields ? &fa : nullptr);
  else launch<2>(lab_kind, blocks, (hipStream_t)stream, a, with_fields ? &fa : nullptr);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

}  // namespace

extern "C" {

static_assert(DEPGAN_MAX_HEAD_CLASSES == 8, "sample_pixel's row switch covers 2..8 classes");

int depgan_data_augment(const float* x_src, int nicg, const void* lab_src, int lab_kind, int C, const long* index_dev,
                        long n_src, const float* params_dev, int n, int H, int W, int border, float x_fill,
                        int label_fill, float* x_out, void* lab_out, void* stream) {
  return augment("data_augment", false, x_src, nicg, lab_src, lab_kind, C, index_dev, n_src, params_dev, nullptr, 0, 0,
                 n, H, W, border, x_fill, label_fill, x_out, lab_out, nullptr, stream);
}

int depgan_data_augment_fields(const float* x_src, int nicg, const void* lab_src, int lab_kind, int C,
                               const long* index_dev, long n_src, const float* params_dev, const float* fields_dev,
                               int gh, int gw, int n, int H, int W, int border, float x_fill, int label_fill,
                               float* x_out, void* lab_out, float* dense_out, void* stream) {
  return augment("data_augment_fields", true, x_src, nicg, lab_src, lab_kind, C, index_dev, n_src, params_dev,
                 fields_dev, gh, gw, n, H, W, border, x_fill, label_fill, x_out, lab_out, dense_out, stream);
}

}  // extern "C"
