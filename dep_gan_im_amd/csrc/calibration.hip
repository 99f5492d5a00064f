// Calibration of the class probabilities (evaluate.calibration_census, fit_temperature, apply_temperature): can the
// probabilities of predict / predict_mean be believed?  include/depgan.h states every operation.
//
//   cal_census_kernel<C, T>        per pixel that takes part: the top-label bin and one bin per class (one against the
//                                  rest), each with a count, a hit count and the fixed-point sum of the confidence; four
//                                  scalar counts; the Brier and the NLL sums in double
//   cal_census_finish_kernel       adds the blocks' integer tables; block 0 also folds the double partials in index order
//   cal_temperature_kernel<C, T>   {N, sum L, sum L', sum L''} of the softmax of beta * log(max(p, eps)) against the labels
//   cal_sums_finish_kernel         one block folds those partials in index order
//   cal_apply_kernel<C, T>         out = softmax(beta * log(max(p, eps))), rounded once to the kind of prob
//
// The census is memory-bound in intent: C * sizeof(T) + 1 (+ 4 with a mask) bytes per pixel, 33 for a float64 mean of
// four classes.  Everything binned is an integer, so LDS integer adds may land in any order; what has to be avoided is
// the conflict: with brain labels ~97 % of a wave's lanes hit the same bin of every table, and 64 lane-wise LDS adds on
// one address serialise.  So a wave PEELS its distinct bins with ballots: the first remaining lane's bin is broadcast,
// the lanes in that bin are balloted, one lane adds the population count, the count of hits among them and the
// wave-reduced sum of q to the block's table, and the loop goes on with the lanes that remain.  A wave whose lanes share
// a bin makes one pass per table; the loop ends after at most min(64, bins) passes because every pass removes a lane.
// No global atomics: a block stores its table with plain stores and a second launch adds the tables.
#include "common.h"

#include "../../include/depgan.h"

// every double operation below is rounded on its own, as the NumPy restatement's are (tests/calibration_ref.py)
#pragma clang fp contract(off)

namespace {

constexpr int CAL_MAX_BLOCKS = 1024, CAL_PER_THREAD = 4;        // a block takes 256 * CAL_PER_THREAD pixels, up to the cap
constexpr int CAL_NSCALAR = 4;                                  // N, n_nan, n_bad, n_floored
constexpr int CAL_MAX_TABLE = (1 + DEPGAN_MAX_HEAD_CLASSES) * DEPGAN_CAL_MAX_BINS * 3 + CAL_NSCALAR;
constexpr double CAL_FIX_ONE = (double)(1ULL << DEPGAN_CAL_FIX_SHIFT);

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the integers of one census: (1 + C) tables of bins x {count, hits, sum q}, then the scalars
__host__ __device__ inline int cal_table_len(int C, int bins) { return (1 + C) * bins * 3 + CAL_NSCALAR; }

// The number of blocks is a function of n alone, so the order of every double add is too.
int cal_blocks(long n) {
  const long per_block = 256L * CAL_PER_THREAD;
  const long nb = (n + per_block - 1) / per_block;
  return (int)(nb < CAL_MAX_BLOCKS ? nb : CAL_MAX_BLOCKS);
}

// One row of C elements as doubles (the conversion of a float is exact).  A row whose size is a multiple of 16 bytes is
// read with 16-byte accesses (float32 C = 4, 8; float64 C even), of 8 bytes with 8-byte ones; prob is 16-byte aligned.
template <int C, typename T>
__device__ __forceinline__ void cal_row_load(const T* p, double v[C]) {
  constexpr int BYTES = C * (int)sizeof(T);
  T raw[C];
  if constexpr (BYTES % 16 == 0) {
    u32x4 chunk[BYTES / 16];
#pragma unroll
    for (int k = 0; k < BYTES / 16; ++k) chunk[k] = ((const u32x4*)p)[k];
    __builtin_memcpy(raw, chunk, BYTES);
  } else if constexpr (BYTES % 8 == 0) {
    u32x2 chunk[BYTES / 8];
#pragma unroll
    for (int k = 0; k < BYTES / 8; ++k) chunk[k] = ((const u32x2*)p)[k];
    __builtin_memcpy(raw, chunk, BYTES);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) raw[c] = p[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = (double)raw[c];
}

// the reverse: (T)v[c] is the one rounding of a float32 row
template <int C, typename T>
__device__ __forceinline__ void cal_row_store(T* p, const double v[C]) {
  constexpr int BYTES = C * (int)sizeof(T);
  T raw[C];
#pragma unroll
  for (int c = 0; c < C; ++c) raw[c] = (T)v[c];
  if constexpr (BYTES % 16 == 0) {
    u32x4 chunk[BYTES / 16];
    __builtin_memcpy(chunk, raw, BYTES);
#pragma unroll
    for (int k = 0; k < BYTES / 16; ++k) ((u32x4*)p)[k] = chunk[k];
  } else if constexpr (BYTES % 8 == 0) {
    u32x2 chunk[BYTES / 8];
    __builtin_memcpy(chunk, raw, BYTES);
#pragma unroll
    for (int k = 0; k < BYTES / 8; ++k) ((u32x2*)p)[k] = chunk[k];
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = raw[c];
  }
}

// b(v) = (int)min(max(v * bins, 0.0), bins - 1); v is not a NaN here
__device__ __forceinline__ int cal_bin(double v, double dbins, double top) {
  double x = v * dbins;
  x = x < 0.0 ? 0.0 : x;
  x = x > top ? top : x;
  return (int)x;
}

// q(v) = (long long)rint(v * 2^32): the product is exact (a power of two), rint rounds once, ties to even
__device__ __forceinline__ long long cal_fix(double v) { return (long long)rint(v * CAL_FIX_ONE); }

// max(p, eps) = p < eps ? eps : p, so a NaN stays one
__device__ __forceinline__ double cal_floor(double p, double eps) { return p < eps ? eps : p; }

__device__ __forceinline__ long long cal_wave_sum(long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// One table of a wave's 64 pixels: tb[3 b ..] += {lanes in bin b, those of them with `hit`, their sum of q}, one pass
// per distinct bin among the lanes with `act`.  Called by the whole wave.
__device__ __forceinline__ void cal_peel(unsigned long long* tb, bool act, int b, bool hit, long long q, int lane) {
  unsigned long long rem = __ballot(act);
  const unsigned long long hits = __ballot(act && hit);
  while (rem) {
    const int lead = __ffsll((long long)rem) - 1;
    const int b0 = __builtin_amdgcn_readlane(b, lead);
    const bool in = act && b == b0;
    const unsigned long long m = __ballot(in);
    const long long s = cal_wave_sum(in ? q : 0LL);
    if (lane == 0) {
      atomicAdd(&tb[b0 * 3 + 0], (unsigned long long)__popcll(m));
      atomicAdd(&tb[b0 * 3 + 1], (unsigned long long)__popcll(m & hits));
      atomicAdd(&tb[b0 * 3 + 2], (unsigned long long)s);
    }
    rem &= ~m;
  }
}

// the fixed-order tree of surface_sums_kernel over NQ quantities; red is [NQ][256]; the result is red[q][0]
template <int NQ>
__device__ __forceinline__ void cal_block_tree(double (*red)[256], int t) {
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) red[q][t] = red[q][t] + red[q][t + o];
    }
    __syncthreads();
  }
}

struct CalArgs {
  const void* prob;
  const unsigned char* lab;
  const float* mask;
  long n;
  int ignore, bins;
  double eps, beta;
  unsigned long long* tab_part;   // census: [nb][cal_table_len]
  double* dpart;                  // [nb][2] (census) or [nb][4] (temperature sums)
};

// What a pixel is: 0 takes no part (masked or ignored), 1 takes part, 2 a code >= C, 3 a row with a NaN.  v is the row
// (zeros unless 1), tc the true class (-1 unless 1).
template <int C, typename T>
__device__ __forceinline__ int cal_pixel(const CalArgs& a, long i, double v[C], int* tc) {
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = 0.0;
  *tc = -1;
  if (i >= a.n) return 0;
  const int code = a.lab[i];
  if ((a.mask && a.mask[i] == 0.0f) || code == a.ignore) return 0;
  if (code >= C) return 2;
  double w[C];
  cal_row_load<C, T>((const T*)a.prob + (size_t)i * C, w);
  bool nan = false;
#pragma unroll
  for (int c = 0; c < C; ++c) nan = nan || w[c] != w[c];
  if (nan) return 3;
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = w[c];
  *tc = code;
  return 1;
}

// grid cal_blocks(n), block 256.  The whole wave stays in the loop until its last lane is done: a ballot must see every
// lane.  tab: the block's integer table in LDS (integer adds, any order); the two double sums go through the tree.
template <int C, typename T>
__global__ __launch_bounds__(256) void cal_census_kernel(const CalArgs a) {
  __shared__ unsigned long long tab[CAL_MAX_TABLE];
  __shared__ double red[2][256];
  const int t = threadIdx.x, lane = t & 63;
  const int bins = a.bins, len = cal_table_len(C, bins);
  for (int i = t; i < len; i += 256) tab[i] = 0;
  __syncthreads();
  const double dbins = (double)bins, top = (double)(bins - 1);
  double brier = 0.0, nll = 0.0;
  unsigned nN = 0, nNan = 0, nBad = 0, nFloor = 0;      // the same in every lane of a wave
  for (long i = (long)blockIdx.x * 256 + t; __any(i < a.n) != 0; i += (long)gridDim.x * 256) {
    double v[C];
    int tc;
    const int what = cal_pixel<C, T>(a, i, v, &tc);
    const bool act = what == 1;
    // top label: the first maximum
    double conf = v[0];
    int pred = 0;
#pragma unroll
    for (int c = 1; c < C; ++c) {
      if (v[c] > conf) {
        conf = v[c];
        pred = c;
      }
    }
    cal_peel(tab, act, cal_bin(conf, dbins, top), pred == tc, cal_fix(conf), lane);
    double r = 0.0, bs = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      cal_peel(tab + (1 + c) * bins * 3, act, cal_bin(v[c], dbins, top), tc == c, cal_fix(v[c]), lane);
      r = (tc == c) ? v[c] : r;
      const double d = v[c] - ((tc == c) ? 1.0 : 0.0);
      bs = bs + d * d;
    }
    bool floored = false;
    if (act) {
      floored = r < a.eps;
      brier = brier + bs;
      nll = nll + (0.0 - log(cal_floor(r, a.eps)));
    }
    nN += (unsigned)__popcll(__ballot(act));
    nNan += (unsigned)__popcll(__ballot(what == 3));
    nBad += (unsigned)__popcll(__ballot(what == 2));
    nFloor += (unsigned)__popcll(__ballot(floored));
  }
  if (lane == 0) {
    unsigned long long* sc = tab + len - CAL_NSCALAR;
    atomicAdd(&sc[0], (unsigned long long)nN);
    atomicAdd(&sc[1], (unsigned long long)nNan);
    atomicAdd(&sc[2], (unsigned long long)nBad);
    atomicAdd(&sc[3], (unsigned long long)nFloor);
  }
  red[0][t] = brier;
  red[1][t] = nll;
  cal_block_tree<2>(red, t);          // its first barrier also closes the table
  for (int i = t; i < len; i += 256) a.tab_part[(size_t)blockIdx.x * len + i] = tab[i];
  if (t < 2) a.dpart[(size_t)blockIdx.x * 2 + t] = red[t][0];
}

// grid ceil(len / 16), block 256 = 16 entries x 16 slices of the blocks: out[e] = the sum over the nb blocks of entry e
// (integers: any order).  Block 0 then folds the nb x 2 double partials: thread q < 2 adds quantity q in index order.
__global__ __launch_bounds__(256) void cal_census_finish_kernel(const unsigned long long* __restrict__ tab_part,
                                                                const double* __restrict__ dpart, int nb, int len,
                                                                unsigned long long* __restrict__ tab_out,
                                                                double* __restrict__ d_out) {
  __shared__ unsigned long long sl[16][16];
  __shared__ double part[CAL_MAX_BLOCKS * 2];
  const int t = threadIdx.x, e = (int)blockIdx.x * 16 + (t & 15), slice = t >> 4;
  unsigned long long acc = 0;
  if (e < len)
    for (int b = slice; b < nb; b += 16) acc += tab_part[(size_t)b * len + e];
  sl[slice][t & 15] = acc;
  if (blockIdx.x == 0)
    for (int i = t; i < nb * 2; i += 256) part[i] = dpart[i];
  __syncthreads();
  if (t < 16 && e < len) {
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += sl[k][t];
    tab_out[e] = s;
  }
  if (blockIdx.x == 0 && t < 2) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s = s + part[b * 2 + t];
    d_out[t] = s;
  }
}

// grid cal_blocks(n), block 256.  dpart[4 b ..] = {N, sum L, sum L', sum L''} of block b.
template <int C, typename T>
__global__ __launch_bounds__(256) void cal_temperature_kernel(const CalArgs a) {
  __shared__ double red[4][256];
  const int t = threadIdx.x;
  double cnt = 0.0, sL = 0.0, sL1 = 0.0, sL2 = 0.0;
  for (long i = (long)blockIdx.x * 256 + t; i < a.n; i += (long)gridDim.x * 256) {
    double v[C];
    int tc;
    if (cal_pixel<C, T>(a, i, v, &tc) != 1) continue;
    double z[C], s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      z[c] = log(cal_floor(v[c], a.eps));
      s[c] = a.beta * z[c];
    }
    double m = s[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = s[c] > m ? s[c] : m;
    double e[C], S = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      e[c] = exp(s[c] - m);
      S = S + e[c];
    }
    const double lse = m + log(S);
    double A = 0.0, B = 0.0, st = 0.0, zt = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double pi = e[c] / S;
      A = A + pi * z[c];
      B = B + pi * (z[c] * z[c]);
      st = (tc == c) ? s[c] : st;
      zt = (tc == c) ? z[c] : zt;
    }
    cnt = cnt + 1.0;
    sL = sL + (lse - st);
    sL1 = sL1 + (A - zt);
    sL2 = sL2 + (B - A * A);
  }
  red[0][t] = cnt;
  red[1][t] = sL;
  red[2][t] = sL1;
  red[3][t] = sL2;
  cal_block_tree<4>(red, t);
  if (t < 4) a.dpart[(size_t)blockIdx.x * 4 + t] = red[t][0];
}

// one block of 256: thread q < 4 folds quantity q of the nb <= CAL_MAX_BLOCKS partials in index order
__global__ __launch_bounds__(256) void cal_sums_finish_kernel(const double* __restrict__ dpart, int nb,
                                                              double* __restrict__ d_out) {
  __shared__ double part[CAL_MAX_BLOCKS * 4];
  for (int i = threadIdx.x; i < nb * 4; i += 256) part[i] = dpart[i];
  __syncthreads();
  const int q = threadIdx.x;
  if (q >= 4) return;
  double acc = 0.0;
  for (int b = 0; b < nb; ++b) acc = acc + part[b * 4 + q];
  d_out[q] = acc;
}

// grid ceil(n / 256), block 256, thread = pixel: the whole row is read before any of it is written, so out may be prob
template <int C, typename T>
__global__ __launch_bounds__(256) void cal_apply_kernel(const T* prob, T* out, long n, double beta, double eps) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double v[C], s[C];
  cal_row_load<C, T>(prob + (size_t)i * C, v);
#pragma unroll
  for (int c = 0; c < C; ++c) s[c] = beta * log(cal_floor(v[c], eps));
  double m = s[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = s[c] > m ? s[c] : m;
  double S = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) S = S + exp(s[c] - m);
  const double lse = m + log(S);
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = exp(s[c] - lse);
  cal_row_store<C, T>(out + (size_t)i * C, v);
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || !na || !nb) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

size_t elem_bytes(int prob_kind) { return prob_kind ? sizeof(double) : sizeof(float); }

// the checks the three entries share; `who` names the entry in the message
bool common_ok(const char* who, const void* prob, int prob_kind, int C, long npix, double eps, bool eps_positive) {
  if (npix < 1 || npix >= (1L << 31) || C < 2 || C > DEPGAN_MAX_HEAD_CLASSES || (prob_kind != 0 && prob_kind != 1) ||
      !prob || ((uintptr_t)prob & 15) || !(eps >= 0.0 && eps < 1.0) || (eps_positive && !(eps > 0.0))) {
    dg_set_error("%s: bad argument (npix=%ld C=%d prob_kind=%d eps=%g; 1 <= npix < 2^31, C in 2..%d, prob_kind 0 / 1, "
                 "eps in %s0, 1), prob given and 16-byte aligned)", who, npix, C, prob_kind, eps,
                 DEPGAN_MAX_HEAD_CLASSES, eps_positive ? "(" : "[");
    return false;
  }
  return true;
}

bool labels_ok(const char* who, const unsigned char* lab, int ignore_label, const float* mask, const void* scratch) {
  if (!lab || ignore_label < -1 || ignore_label > 255 || ((uintptr_t)mask & 3) || !scratch || ((uintptr_t)scratch & 7)) {
    dg_set_error("%s: bad argument (ignore_label=%d; -1..255, lab and scratch given, mask 4-byte and scratch 8-byte "
                 "aligned)", who, ignore_label);
    return false;
  }
  return true;
}

bool scratch_clear(const char* who, const void* scratch, size_t sbytes, const void* prob, size_t pbytes,
                   const unsigned char* lab, const float* mask, long npix) {
  if (overlaps(scratch, sbytes, prob, pbytes) || overlaps(scratch, sbytes, lab, (size_t)npix) ||
      overlaps(scratch, sbytes, mask, (size_t)npix * 4)) {
    dg_set_error("%s: scratch overlaps prob, lab or mask", who);
    return false;
  }
  return true;
}

template <typename T>
const void* census_fn(int C) {
  switch (C) {
    case 2: return (const void*)cal_census_kernel<2, T>;
    case 3: return (const void*)cal_census_kernel<3, T>;
    case 4: return (const void*)cal_census_kernel<4, T>;
    case 5: return (const void*)cal_census_kernel<5, T>;
    case 6: return (const void*)cal_census_kernel<6, T>;
    case 7: return (const void*)cal_census_kernel<7, T>;
    default: return (const void*)cal_census_kernel<8, T>;
  }
}

template <typename T>
const void* temperature_fn(int C) {
  switch (C) {
    case 2: return (const void*)cal_temperature_kernel<2, T>;
    case 3: return (const void*)cal_temperature_kernel<3, T>;
    case 4: return (const void*)cal_temperature_kernel<4, T>;
    case 5: return (const void*)cal_temperature_kernel<5, T>;
    case 6: return (const void*)cal_temperature_kernel<6, T>;
    case 7: return (const void*)cal_temperature_kernel<7, T>;
    default: return (const void*)cal_temperature_kernel<8, T>;
  }
}

template <typename T>
const void* apply_fn(int C) {
  switch (C) {
    case 2: return (const void*)cal_apply_kernel<2, T>;
    case 3: return (const void*)cal_apply_kernel<3, T>;
    case 4: return (const void*)cal_apply_kernel<4, T>;
    case 5: return (const void*)cal_apply_kernel<5, T>;
    case 6: return (const void*)cal_apply_kernel<6, T>;
    case 7: return (const void*)cal_apply_kernel<7, T>;
    default: return (const void*)cal_apply_kernel<8, T>;
  }
}

}  // namespace

extern "C" {

// [final table: len][final doubles: 4][block tables: nb * len][double partials: nb * 4], all 8-byte words
size_t depgan_eval_calibration_scratch_bytes(long npix, int C, int bins) {
  if (npix < 1 || npix >= (1L << 31) || C < 2 || C > DEPGAN_MAX_HEAD_CLASSES || bins < 1 || bins > DEPGAN_CAL_MAX_BINS)
    return 0;
  return ((size_t)cal_blocks(npix) + 1) * ((size_t)cal_table_len(C, bins) + 4) * 8;
}

int depgan_eval_calibration_census(const void* prob, int prob_kind, int C, const unsigned char* lab, int ignore_label,
                                   const float* mask, long npix, int bins, double eps, void* scratch,
                                   long long* counts_out_host, double* sums_out_host, void* stream) {
  const char* who = "eval_calibration_census";
  if (!common_ok(who, prob, prob_kind, C, npix, eps, false) || !labels_ok(who, lab, ignore_label, mask, scratch))
    return DG_ERR_ARG;
  if (bins < 1 || bins > DEPGAN_CAL_MAX_BINS || !counts_out_host || !sums_out_host) {
    dg_set_error("%s: bad argument (bins=%d; 1..%d, counts_out_host and sums_out_host given)", who, bins,
                 DEPGAN_CAL_MAX_BINS);
    return DG_ERR_ARG;
  }
  const size_t sbytes = depgan_eval_calibration_scratch_bytes(npix, C, bins);
  if (!scratch_clear(who, scratch, sbytes, prob, (size_t)npix * C * elem_bytes(prob_kind), lab, mask, npix))
    return DG_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int nb = cal_blocks(npix), len = cal_table_len(C, bins);
  unsigned long long* tab_out = (unsigned long long*)scratch;
  double* d_out = (double*)(tab_out + len);
  unsigned long long* tab_part = tab_out + len + 4;
  double* dpart = (double*)(tab_part + (size_t)nb * len);
  CalArgs a = {prob, lab, mask, npix, ignore_label, bins, eps, 1.0, tab_part, dpart};
  void* kargs[] = {&a};
  HIPCHECK(hipLaunchKernel(prob_kind ? census_fn<double>(C) : census_fn<float>(C), dim3(nb), dim3(256), kargs, 0, st));
  hipLaunchKernelGGL(cal_census_finish_kernel, dim3((unsigned)cdiv(len, 16)), dim3(256), 0, st,
                     (const unsigned long long*)tab_part, (const double*)dpart, nb, len, tab_out, d_out);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(counts_out_host, tab_out, (size_t)len * 8, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(sums_out_host, d_out, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  return DG_OK;
}

int depgan_eval_temperature_sums(const void* prob, int prob_kind, int C, const unsigned char* lab, int ignore_label,
                                 const float* mask, long npix, double beta, double eps, void* scratch,
                                 double out_host[4], void* stream) {
  const char* who = "eval_temperature_sums";
  if (!common_ok(who, prob, prob_kind, C, npix, eps, true) || !labels_ok(who, lab, ignore_label, mask, scratch))
    return DG_ERR_ARG;
  if (!(beta > 0.0 && beta < (double)INFINITY) || !out_host) {
    dg_set_error("%s: bad argument (beta=%g; finite and > 0, out_host given)", who, beta);
    return DG_ERR_ARG;
  }
  const size_t sbytes = depgan_eval_calibration_scratch_bytes(npix, C, 1);
  if (!scratch_clear(who, scratch, sbytes, prob, (size_t)npix * C * elem_bytes(prob_kind), lab, mask, npix))
    return DG_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int nb = cal_blocks(npix);
  double* d_out = (double*)scratch;
  double* dpart = d_out + 4;
  CalArgs a = {prob, lab, mask, npix, ignore_label, 1, eps, beta, nullptr, dpart};
  void* kargs[] = {&a};
  HIPCHECK(hipLaunchKernel(prob_kind ? temperature_fn<double>(C) : temperature_fn<float>(C), dim3(nb), dim3(256), kargs,
                           0, st));
  hipLaunchKernelGGL(cal_sums_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)dpart, nb, d_out);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(out_host, d_out, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  return DG_OK;
}

int depgan_eval_apply_temperature(const void* prob, int prob_kind, int C, double beta, double eps, void* out, long npix,
                                  void* stream) {
  const char* who = "eval_apply_temperature";
  if (!common_ok(who, prob, prob_kind, C, npix, eps, false)) return DG_ERR_ARG;
  if (!(beta > 0.0 && beta < (double)INFINITY) || !out || ((uintptr_t)out & 15)) {
    dg_set_error("%s: bad argument (beta=%g; finite and > 0, out given and 16-byte aligned)", who, beta);
    return DG_ERR_ARG;
  }
  const size_t bytes = (size_t)npix * C * elem_bytes(prob_kind);
  if (out != prob && overlaps(out, bytes, prob, bytes)) {
    dg_set_error("%s: out overlaps prob without being prob", who);
    return DG_ERR_ARG;
  }
  void* kargs[] = {&prob, &out, &npix, &beta, &eps};
  HIPCHECK(hipLaunchKernel(prob_kind ? apply_fn<double>(C) : apply_fn<float>(C), dim3((unsigned)((npix + 255) / 256)),
                           dim3(256), kargs, 0, (hipStream_t)stream));
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
