// The exact Euclidean distance transform's device text, stated once: the row scan and the axis sweep that the surface
// distances (surface_dist.hip: edt_rows_kernel, edt_axis_kernel) and the boundary loss's signed distance maps
// (boundary_loss.hip: bl_rows_kernel, bl_cols_kernel) both run.  One text, so one rounding tree: what either caller
// computes per candidate is fl(staged + fl(e e w)) below and nothing else, and the boundary maps are bit for bit what
// depgan_eval_edt_sq gives on the slice.
//
// Rounding is monotone, so the minimum over the set voxels of fl(fl(fl(dx^2 wx) + fl(dy^2 wy)) + fl(dz^2 wz)) equals
// the nested minima along the axes bit for bit; a minimum of doubles does not depend on its order, so nothing here
// does.  The integer squares are exact in double (< 2^24).  No atomics.
#pragma once
#include "common.h"

#include <math.h>

// Every double operation below is rounded on its own, as the NumPy restatement's statements are.  The arithmetic is
// written with plain operators on purpose: the pragma governs the operations of THIS text, while __dmul_rn / __dadd_rn
// are inline functions of the HIP headers and carry the headers' contraction mode, so a __dmul_rn fed into a __dadd_rn
// compiles to one v_fma_f64 (seen in surface_dist.hip's first version: one rounding instead of two, an ulp off).
#pragma clang fp contract(off)

constexpr int DG_EDT_MAX_DIM = 4096;             // the longest row or column: a distance in voxels fits 12 bits
constexpr int DG_EDT_COLS = 64, DG_EDT_ROWS_PER_THREAD = 4, DG_EDT_TILE_ROWS = 16;
static_assert(DG_EDT_ROWS_PER_THREAD == 4 && DG_EDT_TILE_ROWS == 4 * DG_EDT_ROWS_PER_THREAD,
              "dg_edt_axis_sweep: four waves of four rows, candidate rows in steps of four");
constexpr int DG_EDT_FAR = 1 << 20;              // a flag position beyond any distance: |x - (+-FAR)| > 4095

constexpr size_t dg_edt_round8(size_t b) { return (b + 7) & ~(size_t)7; }

// One v_min_f64.  fmin() compiles to three: IEEE minNum first canonicalises every operand it cannot prove free of
// signalling NaNs (dg_vmax of common.h).  No operand here is a NaN: a staged value is >= 0 or +inf and a term is >= 0
// (the weights are finite and > 0, checked by the entry), so no inf - inf and no 0 * inf arises.
__device__ __forceinline__ double dg_edt_min(double a, double b) {
  double o;
  asm("v_min_f64 %0, %1, %2" : "=v"(o) : "v"(a), "v"(b));
  return o;
}

// The row scan of a workgroup of 256 over one row of W <= DG_EDT_MAX_DIM positions: emit(x, d) for every x, d = the
// distance in positions to the nearest one the flags point at (>= DG_EDT_MAX_DIM: there is none).  Thread t owns the
// run [t * run, (t + 1) * run) of the row, run = ceil(W / 256) <= 16: the last flag at or before the run's end and the
// first at or after its start come from a scan over the 256 run summaries, the rest is the two-sided scan inside the
// run.  With L(x) the last flag at or before x:
//   CHANGE = false  a flag at x is itself a hit: d = min(x - L(x), R(x) - x), R(x) the first flag at or after x
//   CHANGE = true   a flag at x > 0 says that x and x - 1 differ in membership, and d is the distance to the nearest
//                   position of the other membership than x's own: min(x - L(x) + 1, R(x) - x), R(x) the first flag
//                   strictly after x.  flag(0) is never asked.
// flag(x) reads what the caller has made visible to the workgroup before the call; the summaries are free for the next
// call after a __syncthreads().
template <bool CHANGE, class Flag, class Emit>
__device__ __forceinline__ void dg_edt_row_scan(int W, Flag flag, Emit emit) {
  __shared__ int last_s[256], first_s[256];
  const int t = threadIdx.x;
  const int run = (W + 255) / 256;
  const int x0 = t * run, x1 = min(W, x0 + run);      // x0 may lie beyond W: an empty run
  int last = -DG_EDT_FAR, first = DG_EDT_FAR;
  for (int x = CHANGE ? max(x0, 1) : x0; x < x1; ++x)
    if (flag(x)) {
      last = x;
      if (first == DG_EDT_FAR) first = x;
    }
  last_s[t] = last;
  first_s[t] = first;
  __syncthreads();
  // inclusive prefix maximum of last_s, inclusive suffix minimum of first_s
  for (int o = 1; o < 256; o <<= 1) {
    const int a = t >= o ? last_s[t - o] : -DG_EDT_FAR;
    const int b = t + o < 256 ? first_s[t + o] : DG_EDT_FAR;
    __syncthreads();
    last_s[t] = max(last_s[t], a);
    first_s[t] = min(first_s[t], b);
    __syncthreads();
  }
  int left[16];                                       // run <= 16 (W <= DG_EDT_MAX_DIM)
  int cur = t > 0 ? last_s[t - 1] : -DG_EDT_FAR;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int x = x0 + i;
    if (x < x1) {
      if ((!CHANGE || x > 0) && flag(x)) cur = x;
      left[i] = x - cur + (CHANGE ? 1 : 0);
    }
  }
  cur = t < 255 ? first_s[t + 1] : DG_EDT_FAR;
#pragma unroll
  for (int i = 15; i >= 0; --i) {
    const int x = x0 + i;
    if (x < x1) {
      if (!CHANGE && flag(x)) cur = x;
      emit(x, min(left[i], cur - x));
      if (CHANGE && x > 0 && flag(x)) cur = x;
    }
  }
}

// The axis sweep of a workgroup of 256 (four waves) over 64 columns x 16 output rows, four rows per thread in
// registers: best[k] = min_r' fl(staged[r'] + fl((r0 + k - r')^2 w_axis)) over all nrows candidate rows r' of the
// thread's column, r0 = the thread's first output row.  Lanes run along the columns, so a caller's global accesses are
// coalesced.  The candidate rows go through LDS in chunks of CHUNK doubles per column (32 KiB: 64 rows in one stage, or
// 32 in two); a staged value serves the thread's four outputs.
//   stage(r', a, b) gives candidate row r' of the thread's column its staged value(s); it is asked only for a live
//                   column and r' < nrows, everything else holds +inf.
//   DUAL = false    one staged value, a; b and in[] are not read.
//   DUAL = true     two: output row k reads a where in[k] and b where not.
// Work is O(nrows) per output.
template <int CHUNK, bool DUAL, class Stage>
__device__ __forceinline__ void dg_edt_axis_sweep(int nrows, int r0, bool live, double w_axis,
                                                  const bool (&in)[DG_EDT_ROWS_PER_THREAD], Stage stage,
                                                  double (&best)[DG_EDT_ROWS_PER_THREAD]) {
  static_assert(CHUNK % 4 == 0, "candidate rows in steps of four");
  __shared__ double staged[DUAL ? 2 : 1][CHUNK][DG_EDT_COLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double inf = INFINITY;
#pragma unroll
  for (int k = 0; k < DG_EDT_ROWS_PER_THREAD; ++k) best[k] = inf;
  for (int c0 = 0; c0 < nrows; c0 += CHUNK) {
    const int cn = min(CHUNK, nrows - c0);
    const int cn4 = (cn + 3) & ~3;                         // <= CHUNK, a multiple of 4
    __syncthreads();                                       // the previous chunk has been read
    for (int r = wave; r < cn4; r += 4) {
      double a = inf, b = inf;
      if (live && r < cn) stage(c0 + r, a, b);
      staged[0][r][lane] = a;
      if (DUAL) staged[DUAL ? 1 : 0][r][lane] = b;
    }
    __syncthreads();
    // The axis term of output row r_k against candidate row r' depends on r_k - r' alone, so stepping r' by one
    // shifts the thread's four terms along and needs one new one, fl((r_0 - r')^2 w_axis), the square exact: a
    // candidate costs one add and one minimum per output.  Output k reads t[(k - s) & 3] at step s and the new term
    // takes the place of the one that fell off, so four steps bring the terms back to where they were and the shift
    // costs no moves.
    double e = (double)(r0 - c0);                           // r_0 - r'
    double t[4];
    t[0] = (e * e) * w_axis;
#pragma unroll
    for (int k = 1; k < 4; ++k) t[k] = ((e + (double)k) * (e + (double)k)) * w_axis;
    for (int r = 0; r < cn4; r += 4) {                      // rows cn .. cn4 - 1 hold +inf
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double a = staged[0][r + s][lane];
        const double b = DUAL ? staged[DUAL ? 1 : 0][r + s][lane] : a;
#pragma unroll
        for (int k = 0; k < 4; ++k) best[k] = dg_edt_min(best[k], (DUAL ? (in[k] ? a : b) : a) + t[(k - s) & 3]);
        e = e - 1.0;
        t[(3 - s) & 3] = (e * e) * w_axis;
      }
    }
  }
}
