// Surface distances (evaluate.surface_distances): the surface voxels of a binary volume, the exact squared Euclidean
// distance from every voxel to the nearest set voxel, and the four sums the directed Hausdorff and mean surface
// distances are formed from.  Volumes are (D, H, W) bytes with W contiguous; non-zero means set.
//
//   surface_mask_kernel      surf[v] = set[v] != 0 && a face neighbour (6 in the volume, or 4 in the slice) is unset or
//                            lies outside the volume
//   edt_rows_kernel          pass 1, one workgroup per row: g[x] = distance in voxels to the nearest set voxel of the
//                            row, 16-bit, EDT_NONE for a row without one
//   edt_axis_kernel<true>    pass 2, along H:  F[y]  = min_y' fl(fl(g[y']^2 wx) + fl((y - y')^2 wy))
//   edt_axis_kernel<false>   pass 3, along D:  d2[z] = min_z' fl(F[z'] + fl((z - z')^2 wz))
//   surface_sums_kernel, surface_sums_finish_kernel
//                            count, max d2, sum sqrt(d2) and the number of infinite d2 over the voxels with surf != 0:
//                            one partial per block, then one block adds the partials in index order
//
// The scan of pass 1, the sweep of passes 2 and 3 and the reasons why the nested minima are exact are edt.h's.  This
// file owns what a pass reads and writes: passes 2 and 3 are one kernel over a (batch, rows, columns) view with the
// columns contiguous, (D, H, W) for pass 2 and (1, D, H*W) for pass 3.
#include "edt.h"

#include "../../include/depgan.h"

// every double operation of this file is rounded on its own too (edt.h has the reasons)
#pragma clang fp contract(off)

namespace {

constexpr unsigned short EDT_NONE = 0xFFFF;      // pass 1: the row has no set voxel (a distance is at most 4095)
constexpr int SUMS_MAX_BLOCKS = 1024, SUMS_PER_THREAD = 8;

// grid ceil(n / 256), block 256, thread = voxel.  HW = H * W; n = D * H * W < 2^31.
__global__ __launch_bounds__(256) void surface_mask_kernel(const unsigned char* __restrict__ set,
                                                           unsigned char* __restrict__ surf, int D, int H, int W,
                                                           int in_plane, unsigned n) {
  const unsigned v = blockIdx.x * 256u + threadIdx.x;
  if (v >= n) return;
  const unsigned HW = (unsigned)H * (unsigned)W;
  const int z = (int)(v / HW);
  const unsigned pix = v - (unsigned)z * HW;
  const int y = (int)(pix / (unsigned)W), x = (int)(pix - (unsigned)y * (unsigned)W);
  bool s = false;
  if (set[v]) {
    // a neighbour outside the volume counts as unset; an index is formed only for one inside
    s = x == 0 || x == W - 1 || y == 0 || y == H - 1 || !set[v - 1] || !set[v + 1] || !set[v - W] || !set[v + W];
    if (!in_plane && !s) s = z == 0 || z == D - 1 || !set[v - HW] || !set[v + HW];
  }
  surf[v] = s ? 1 : 0;
}

// grid D * H, block 256, workgroup = row: the scan of edt.h over the row's bytes, a set voxel being a hit
__global__ __launch_bounds__(256) void edt_rows_kernel(const unsigned char* __restrict__ set,
                                                       unsigned short* __restrict__ g, int W) {
  __shared__ unsigned char row[DG_EDT_MAX_DIM];
  const size_t base = (size_t)blockIdx.x * W;
  for (int x = threadIdx.x; x < W; x += 256) row[x] = set[base + x];
  __syncthreads();
  unsigned short* grow = g + base;
  dg_edt_row_scan<false>(
      W, [&](int x) { return row[x] != 0; },
      [&](int x, int d) { grow[x] = d >= DG_EDT_MAX_DIM ? EDT_NONE : (unsigned short)d; });
}

// grid (ceil(ncols / 64), ceil(nrows / 16), batch), block 256.  src is (batch, nrows, ncols): the 16-bit row distances
// (FROM_G: the staged value is fl(g^2 w_src), +inf for EDT_NONE) or doubles taken as they are.
// dst[b, r, c] = min_r' fl(staged[b, r', c] + fl((r - r')^2 w_axis)).
template <bool FROM_G>
__global__ __launch_bounds__(256) void edt_axis_kernel(const void* __restrict__ src, double* __restrict__ dst,
                                                       int nrows, int ncols, double w_src, double w_axis) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned col = blockIdx.x * (unsigned)DG_EDT_COLS + (unsigned)lane;    // < 2^31 + 64: ncols < 2^31
  const bool live = col < (unsigned)ncols;
  const size_t base = (size_t)blockIdx.z * (size_t)nrows * (size_t)ncols;
  const int r0 = (int)blockIdx.y * DG_EDT_TILE_ROWS + wave * DG_EDT_ROWS_PER_THREAD;
  double best[DG_EDT_ROWS_PER_THREAD];
  const bool in[DG_EDT_ROWS_PER_THREAD] = {};
  dg_edt_axis_sweep<64, false>(nrows, r0, live, w_axis, in, [&](int r, double& a, double&) {
    const size_t at = base + (size_t)r * (size_t)ncols + (size_t)col;
    if (FROM_G) {
      const unsigned short gv = ((const unsigned short*)src)[at];
      if (gv != EDT_NONE) {
        const double gd = (double)gv;
        a = (gd * gd) * w_src;                              // gd * gd is exact
      }
    } else {
      a = ((const double*)src)[at];
    }
  }, best);
  if (live) {
#pragma unroll
    for (int k = 0; k < DG_EDT_ROWS_PER_THREAD; ++k)
      if (r0 + k < nrows) dst[base + (size_t)(r0 + k) * (size_t)ncols + (size_t)col] = best[k];
  }
}

// The number of blocks is a function of n alone, so the order of every add is too.
int sums_blocks(long n) {
  const long per_block = 256L * SUMS_PER_THREAD;
  const long nb = (n + per_block - 1) / per_block;
  return (int)(nb < SUMS_MAX_BLOCKS ? nb : SUMS_MAX_BLOCKS);
}

// grid sums_blocks(n), block 256.  partial[4 b ..] = {count, max d2, sum sqrt(d2), count of infinite d2} of block b:
// a thread walks its voxels in index order, then a tree over the 256 threads in LDS.  The maximum starts at 0 (d2 >= 0).
__global__ __launch_bounds__(256) void surface_sums_kernel(const double* __restrict__ d2,
                                                           const unsigned char* __restrict__ surf, long n,
                                                           double* __restrict__ partial) {
  __shared__ double red[4][256];
  const int t = threadIdx.x;
  double cnt = 0.0, mx = 0.0, sum = 0.0, ninf = 0.0;
  for (long i = (long)blockIdx.x * 256 + t; i < n; i += (long)gridDim.x * 256) {
    if (surf[i]) {
      const double v = d2[i];
      cnt = cnt + 1.0;
      mx = v > mx ? v : mx;
      sum = sum + __dsqrt_rn(v);
      if (v == INFINITY) ninf = ninf + 1.0;
    }
  }
  red[0][t] = cnt;
  red[1][t] = mx;
  red[2][t] = sum;
  red[3][t] = ninf;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      red[0][t] = red[0][t] + red[0][t + o];
      red[1][t] = red[1][t + o] > red[1][t] ? red[1][t + o] : red[1][t];
      red[2][t] = red[2][t] + red[2][t + o];
      red[3][t] = red[3][t] + red[3][t + o];
    }
    __syncthreads();
  }
  if (t < 4) partial[(size_t)blockIdx.x * 4 + t] = red[t][0];
}

// one block of 256: the nb <= 1024 partials are brought into LDS by all threads, then thread q < 4 folds quantity q in
// index order into partial[4 nb + q]
__global__ __launch_bounds__(256) void surface_sums_finish_kernel(double* __restrict__ partial, int nb) {
  __shared__ double part[SUMS_MAX_BLOCKS * 4];
  for (int i = threadIdx.x; i < nb * 4; i += 256) part[i] = partial[i];
  __syncthreads();
  const int q = threadIdx.x;
  if (q >= 4) return;
  double acc = 0.0;
  for (int b = 0; b < nb; ++b) {
    const double v = part[b * 4 + q];
    if (q == 1) acc = v > acc ? v : acc;
    else acc = acc + v;
  }
  partial[(size_t)nb * 4 + q] = acc;
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || !na || !nb) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// D, H, W in 1..DG_EDT_MAX_DIM and D*H*W < 2^31
bool volume_ok(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1 || D > DG_EDT_MAX_DIM || H > DG_EDT_MAX_DIM || W > DG_EDT_MAX_DIM) return false;
  return (long)D * H * W < (1L << 31);
}

bool weight_ok(double w) { return isfinite(w) && w > 0.0; }

}  // namespace

extern "C" {

int depgan_eval_surface_mask(const unsigned char* set, int D, int H, int W, int in_plane, unsigned char* surf,
                             void* stream) {
  if (!volume_ok(D, H, W) || !set || !surf || (in_plane != 0 && in_plane != 1)) {
    dg_set_error("eval_surface_mask: bad argument (D=%d H=%d W=%d in_plane=%d; dimensions 1..%d, D*H*W < 2^31)", D, H,
                 W, in_plane, DG_EDT_MAX_DIM);
    return DG_ERR_ARG;
  }
  const size_t n = (size_t)D * H * W;
  if (overlaps(surf, n, set, n)) {
    dg_set_error("eval_surface_mask: surf overlaps set");
    return DG_ERR_ARG;
  }
  hipLaunchKernelGGL(surface_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, set,
                     surf, D, H, W, in_plane, (unsigned)n);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

size_t depgan_eval_edt_scratch_bytes(int D, int H, int W) {
  if (!volume_ok(D, H, W)) return 0;
  const size_t n = (size_t)D * H * W;
  return n * sizeof(double) + dg_edt_round8(n * sizeof(unsigned short));     // F, then g
}

int depgan_eval_edt_sq(const unsigned char* set, int D, int H, int W, double wz, double wy, double wx, double* d2,
                       void* scratch, void* stream) {
  if (!volume_ok(D, H, W) || !set || !d2 || !scratch || ((uintptr_t)scratch & 7) || ((uintptr_t)d2 & 7)) {
    dg_set_error("eval_edt_sq: bad argument (D=%d H=%d W=%d; dimensions 1..%d, D*H*W < 2^31; set, d2 and scratch "
                 "given, d2 and scratch 8-byte aligned)", D, H, W, DG_EDT_MAX_DIM);
    return DG_ERR_ARG;
  }
  if (!weight_ok(wz) || !weight_ok(wy) || !weight_ok(wx)) {
    dg_set_error("eval_edt_sq: the weights must be finite and > 0 (wz=%g wy=%g wx=%g)", wz, wy, wx);
    return DG_ERR_ARG;
  }
  const size_t n = (size_t)D * H * W;
  const size_t sbytes = depgan_eval_edt_scratch_bytes(D, H, W);
  if (overlaps(d2, n * 8, set, n) || overlaps(scratch, sbytes, set, n) || overlaps(scratch, sbytes, d2, n * 8)) {
    dg_set_error("eval_edt_sq: two of set, d2 and scratch overlap");
    return DG_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  double* F = (double*)scratch;
  unsigned short* g = (unsigned short*)((char*)scratch + n * sizeof(double));
  hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)(D * H)), dim3(256), 0, st, set, g, W);
  // a single slice has no third pass: fl(F + fl(0 wz)) = F
  const dim3 g2((unsigned)cdiv(W, DG_EDT_COLS), (unsigned)cdiv(H, DG_EDT_TILE_ROWS), (unsigned)D);
  hipLaunchKernelGGL(edt_axis_kernel<true>, g2, dim3(256), 0, st, (const void*)g, D == 1 ? d2 : F, H, W, wx, wy);
  if (D > 1) {
    const long HW = (long)H * W;
    const dim3 g3((unsigned)cdiv(HW, DG_EDT_COLS), (unsigned)cdiv(D, DG_EDT_TILE_ROWS), 1);
    hipLaunchKernelGGL(edt_axis_kernel<false>, g3, dim3(256), 0, st, (const void*)F, d2, D, (int)HW, 0.0, wz);
  }
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

size_t depgan_eval_surface_sums_scratch_bytes(long n) {
  if (n < 1 || n >= (1L << 31)) return 0;
  return ((size_t)sums_blocks(n) + 1) * 4 * sizeof(double);
}

int depgan_eval_surface_sums(const double* d2, const unsigned char* surf, long n, double* partial, double out_host[4],
                             void* stream) {
  if (!d2 || !surf || !partial || !out_host || n < 1 || n >= (1L << 31) || ((uintptr_t)partial & 7)) {
    dg_set_error("eval_surface_sums: bad argument (n=%ld; 1 <= n < 2^31, every pointer given, partial 8-byte aligned)",
                 n);
    return DG_ERR_ARG;
  }
  const size_t pbytes = depgan_eval_surface_sums_scratch_bytes(n);
  if (overlaps(partial, pbytes, d2, (size_t)n * 8) || overlaps(partial, pbytes, surf, (size_t)n)) {
    dg_set_error("eval_surface_sums: partial overlaps d2 or surf");
    return DG_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nb = sums_blocks(n);
  hipLaunchKernelGGL(surface_sums_kernel, dim3(nb), dim3(256), 0, st, d2, surf, n, partial);
  hipLaunchKernelGGL(surface_sums_finish_kernel, dim3(1), dim3(256), 0, st, partial, nb);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(out_host, partial + (size_t)nb * 4, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  return DG_OK;
}

}  // extern "C"
