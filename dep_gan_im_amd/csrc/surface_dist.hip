// Surface distances (evaluate.surface_distances): the surface voxels of a binary volume, the exact squared Euclidean
// distance from every voxel to the nearest set voxel, and the four sums the directed Hausdorff and mean surface
// distances are formed from.  Volumes are (D, H, W) bytes with W contiguous; non-zero means set.
//
//   surface_mask_kernel      surf[v] = set[v] != 0 && a face neighbour (6 in the volume, or 4 in the slice) is unset or
//                            lies outside the volume
//   edt_rows_kernel          pass 1, one workgroup per row: g[x] = distance in voxels to the nearest set voxel of the
//                            row (two-sided scan), 16-bit, EDT_NONE for a row without one
//   edt_axis_kernel<true>    pass 2, along H:  F[y]  = min_y' fl(fl(g[y']^2 wx) + fl((y - y')^2 wy))
//   edt_axis_kernel<false>   pass 3, along D:  d2[z] = min_z' fl(F[z'] + fl((z - z')^2 wz))
//   surface_sums_kernel, surface_sums_finish_kernel
//                            count, max d2, sum sqrt(d2) and the number of infinite d2 over the voxels with surf != 0:
//                            one partial per block, then one block adds the partials in index order
//
// Rounding is monotone, so the minimum over the set voxels of fl(fl(fl(dx^2 wx) + fl(dy^2 wy)) + fl(dz^2 wz)) equals
// the three nested minima bit for bit; a minimum of doubles does not depend on its order, so nothing here does.  The
// integer squares are exact in double (< 2^24).  No atomics.
//
// Passes 2 and 3 are one kernel over a (batch, rows, columns) view with the columns contiguous: (D, H, W) for pass 2
// and (1, D, H*W) for pass 3.  Lanes run along the columns, so every global access is coalesced.  A workgroup of four
// waves owns 64 columns x 16 output rows (four rows per thread, in registers) and walks all candidate rows in chunks
// of 64 staged in LDS as doubles (32 KiB, so four workgroups fit the 160 KiB of a CU); a staged value serves the
// thread's four outputs, and the four axis terms of a thread shift along as the candidate row advances (the term depends
// on the row difference alone), so a candidate costs one add and one minimum.  Work is O(rows) per voxel.
#include "common.h"

#include <math.h>

#include "../../include/depgan.h"

// Every double operation below is rounded on its own, as the NumPy restatement's statements are.  The arithmetic is
// written with plain operators on purpose: the pragma governs the operations of THIS text, while __dmul_rn / __dadd_rn
// are inline functions of the HIP headers and carry the headers' contraction mode, so a __dmul_rn fed into a __dadd_rn
// compiles to one v_fma_f64 (seen in this file's first version: one rounding instead of two, an ulp off).
#pragma clang fp contract(off)

namespace {

constexpr int EDT_MAX_DIM = 4096;
constexpr unsigned short EDT_NONE = 0xFFFF;      // pass 1: the row has no set voxel (a distance is at most 4095)
constexpr int EDT_COLS = 64, EDT_CHUNK = 64, EDT_ROWS_PER_THREAD = 4, EDT_TILE_ROWS = 16;
static_assert(EDT_ROWS_PER_THREAD == 4 && EDT_CHUNK % 4 == 0 && EDT_TILE_ROWS == 4 * EDT_ROWS_PER_THREAD,
              "edt_axis_kernel: four waves of four rows, candidate rows in steps of four");
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

// grid D * H, block 256, workgroup = row.  Thread t owns the run [t * run, (t + 1) * run) of the row, run =
// ceil(W / 256) <= 16: the last set voxel at or before the run's end and the first at or after its start come from a
// scan over the 256 run summaries, the rest is the two-sided scan inside the run.
__global__ __launch_bounds__(256) void edt_rows_kernel(const unsigned char* __restrict__ set,
                                                       unsigned short* __restrict__ g, int W) {
  __shared__ unsigned char row[EDT_MAX_DIM];
  __shared__ int last_s[256], first_s[256];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * W;
  for (int x = t; x < W; x += 256) row[x] = set[base + x];
  __syncthreads();
  const int NONE = 1 << 20;                           // beyond any distance: |x - (+-NONE)| > 4095
  const int run = (W + 255) / 256;
  const int x0 = t * run, x1 = min(W, x0 + run);      // x0 may lie beyond W: an empty run
  int last = -NONE, first = NONE;
  for (int x = x0; x < x1; ++x)
    if (row[x]) {
      last = x;
      if (first == NONE) first = x;
    }
  last_s[t] = last;
  first_s[t] = first;
  __syncthreads();
  // inclusive prefix maximum of last_s, inclusive suffix minimum of first_s
  for (int o = 1; o < 256; o <<= 1) {
    const int a = t >= o ? last_s[t - o] : -NONE;
    const int b = t + o < 256 ? first_s[t + o] : NONE;
    __syncthreads();
    last_s[t] = max(last_s[t], a);
    first_s[t] = min(first_s[t], b);
    __syncthreads();
  }
  int left[16];                                       // run <= 16 (W <= 4096)
  int cur = t > 0 ? last_s[t - 1] : -NONE;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int x = x0 + i;
    if (x < x1) {
      if (row[x]) cur = x;
      left[i] = x - cur;
    }
  }
  cur = t < 255 ? first_s[t + 1] : NONE;
#pragma unroll
  for (int i = 15; i >= 0; --i) {
    const int x = x0 + i;
    if (x < x1) {
      if (row[x]) cur = x;
      const int d = min(left[i], cur - x);
      g[base + x] = d >= EDT_MAX_DIM ? EDT_NONE : (unsigned short)d;
    }
  }
}

// One v_min_f64.  fmin() compiles to three: IEEE minNum first canonicalises every operand it cannot prove free of
// signalling NaNs (dg_vmax of common.h).  No operand here is a NaN: a staged value is >= 0 or +inf and a term is >= 0
// (the weights are finite and > 0, checked by the entry), so no inf - inf and no 0 * inf arises.
__device__ __forceinline__ double edt_min(double a, double b) {
  double o;
  asm("v_min_f64 %0, %1, %2" : "=v"(o) : "v"(a), "v"(b));
  return o;
}

// grid (ceil(ncols / 64), ceil(nrows / 16), batch), block 256.  src is (batch, nrows, ncols): the 16-bit row distances
// (FROM_G: the staged value is fl(g^2 w_src), +inf for EDT_NONE) or doubles taken as they are.
// dst[b, r, c] = min_r' fl(staged[b, r', c] + fl((r - r')^2 w_axis)).
template <bool FROM_G>
__global__ __launch_bounds__(256) void edt_axis_kernel(const void* __restrict__ src, double* __restrict__ dst,
                                                       int nrows, int ncols, double w_src, double w_axis) {
  __shared__ double stage[EDT_CHUNK][EDT_COLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned col = blockIdx.x * (unsigned)EDT_COLS + (unsigned)lane;       // < 2^31 + 64: ncols < 2^31
  const bool live = col < (unsigned)ncols;
  const size_t base = (size_t)blockIdx.z * (size_t)nrows * (size_t)ncols;
  const int r0 = (int)blockIdx.y * EDT_TILE_ROWS + wave * EDT_ROWS_PER_THREAD;
  const double inf = INFINITY;
  double best[EDT_ROWS_PER_THREAD];
#pragma unroll
  for (int k = 0; k < EDT_ROWS_PER_THREAD; ++k) best[k] = inf;
  for (int c0 = 0; c0 < nrows; c0 += EDT_CHUNK) {
    const int cn = min(EDT_CHUNK, nrows - c0);
    const int cn4 = (cn + 3) & ~3;                         // <= EDT_CHUNK, a multiple of 4
    __syncthreads();                                       // the previous chunk has been read
    for (int r = wave; r < cn4; r += 4) {
      double a = inf;
      if (live && r < cn) {
        const size_t at = base + (size_t)(c0 + r) * (size_t)ncols + (size_t)col;
        if (FROM_G) {
          const unsigned short gv = ((const unsigned short*)src)[at];
          if (gv != EDT_NONE) {
            const double gd = (double)gv;
            a = (gd * gd) * w_src;                          // gd * gd is exact
          }
        } else {
          a = ((const double*)src)[at];
        }
      }
      stage[r][lane] = a;
    }
    __syncthreads();
    // The axis term of output row r_k against candidate row r' depends on r_k - r' alone, so stepping r' by one
    // shifts the thread's four terms along and needs one new one, fl((r_0 - r')^2 w_axis), the square exact.  Four
    // steps bring the names back to where they were, so the shift costs no moves.
    double e = (double)(r0 - c0);                           // r_0 - r'
    double t0 = (e * e) * w_axis;
    double t1 = ((e + 1.0) * (e + 1.0)) * w_axis;
    double t2 = ((e + 2.0) * (e + 2.0)) * w_axis;
    double t3 = ((e + 3.0) * (e + 3.0)) * w_axis;
#define EDT_STEP(R, T0, T1, T2, T3)        \
  {                                        \
    const double a = stage[r + R][lane];   \
    best[0] = edt_min(best[0], a + T0);    \
    best[1] = edt_min(best[1], a + T1);    \
    best[2] = edt_min(best[2], a + T2);    \
    best[3] = edt_min(best[3], a + T3);    \
    e = e - 1.0;                           \
    T3 = (e * e) * w_axis;                 \
  }
    for (int r = 0; r < cn4; r += 4) {                      // rows cn .. cn4 - 1 hold +inf
      EDT_STEP(0, t0, t1, t2, t3)
      EDT_STEP(1, t3, t0, t1, t2)
      EDT_STEP(2, t2, t3, t0, t1)
      EDT_STEP(3, t1, t2, t3, t0)
    }
#undef EDT_STEP
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < EDT_ROWS_PER_THREAD; ++k)
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

// D, H, W in 1..4096 and D*H*W < 2^31
bool volume_ok(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1 || D > EDT_MAX_DIM || H > EDT_MAX_DIM || W > EDT_MAX_DIM) return false;
  return (long)D * H * W < (1L << 31);
}

bool weight_ok(double w) { return isfinite(w) && w > 0.0; }

size_t round8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace

extern "C" {

int depgan_eval_surface_mask(const unsigned char* set, int D, int H, int W, int in_plane, unsigned char* surf,
                             void* stream) {
  if (!volume_ok(D, H, W) || !set || !surf || (in_plane != 0 && in_plane != 1)) {
    dg_set_error("eval_surface_mask: bad argument (D=%d H=%d W=%d in_plane=%d; dimensions 1..%d, D*H*W < 2^31)", D, H,
                 W, in_plane, EDT_MAX_DIM);
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
  return n * sizeof(double) + round8(n * sizeof(unsigned short));     // F, then g
}

int depgan_eval_edt_sq(const unsigned char* set, int D, int H, int W, double wz, double wy, double wx, double* d2,
                       void* scratch, void* stream) {
  if (!volume_ok(D, H, W) || !set || !d2 || !scratch || ((uintptr_t)scratch & 7) || ((uintptr_t)d2 & 7)) {
    dg_set_error("eval_edt_sq: bad argument (D=%d H=%d W=%d; dimensions 1..%d, D*H*W < 2^31; set, d2 and scratch "
                 "given, d2 and scratch 8-byte aligned)", D, H, W, EDT_MAX_DIM);
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
  const dim3 g2((unsigned)cdiv(W, EDT_COLS), (unsigned)cdiv(H, EDT_TILE_ROWS), (unsigned)D);
  hipLaunchKernelGGL(edt_axis_kernel<true>, g2, dim3(256), 0, st, (const void*)g, D == 1 ? d2 : F, H, W, wx, wy);
  if (D > 1) {
    const long HW = (long)H * W;
    const dim3 g3((unsigned)cdiv(HW, EDT_COLS), (unsigned)cdiv(D, EDT_TILE_ROWS), 1);
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
