// Generator forward with bf16 activation STORAGE (bf16s.h): bf16-in / bf16-out implicit GEMM on
// v_mfma_f32_32x32x16_bf16, the fp32-in edge layer, the bf16-in head and the widening copy.
//
// The convolution starts from igemm_bf16_kernel<KS, TAPG> (igemm_bf16.hip): same tile (16 x 16 pixels x 32 output
// channels per workgroup), same LDS image (80-byte rows), same XCD-aware item order, same packed panels, same K order
// (chunk, tap, 16-channel sub-chunk) -- so its result is RNE_bf16 of what that kernel computes on the widened operands,
// bit for bit (tests/test_gpu_bf16_store.py pins it).  What differs:
//   * the halo tile is fetched as 16-byte pieces of 8 bf16 (half the load instructions of the fp32-input kernel for the
//     same pixels) and copied to LDS as it is: the rounding happened when the producer stored it;
//   * the epilogue is its own, smaller text: affine, FiLM, ReLU, bf16 residual, bf16 store, optional fused bf16 pool.
//     A pixel's 32 channels are 64 bytes = 4 lanes x 16 bytes, so a wave covers a 16-pixel row per pass and its 4 x 16
//     block in four passes of 16-byte stores (8-byte stores would double the issue-bound store tail).
//   * igemm_bf16s_head_kernel is the same text with gen_segmentation (1x1 to one channel, + tanh) fused into the
//     epilogue: the 4 lanes of a pixel are exactly head_bf16s_kernel's 4 lanes, so the head of the STORED values comes
//     out bit for bit as that kernel computes it, and a forward-only pass need not store the 32-channel tensor at all.
//     It is a sibling kernel, not a run-time branch: igemm_bf16s_kernel<3, 9> keeps its registers and occupancy.
#include <stdlib.h>

#include "bf16s.h"
#include "epilogue.h"
#include "softmax_row.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8), aligned(16)));   // loaded from 16-byte aligned tables
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

#define IGEMM_BF16S_KERNEL igemm_bf16s_kernel
#define IGEMM_BF16S_HEAD 0
#include "igemm_bf16s_kernel.inc"
#undef IGEMM_BF16S_KERNEL
#undef IGEMM_BF16S_HEAD
#define IGEMM_BF16S_KERNEL igemm_bf16s_head_kernel
#define IGEMM_BF16S_HEAD 1
#include "igemm_bf16s_kernel.inc"
#undef IGEMM_BF16S_KERNEL
#undef IGEMM_BF16S_HEAD

// one kernel per KS, and the 3x3 one with the fused head: the launch and the profile's name read the same entry
#define BF16S_K(KERN, KS, TAPG) {reinterpret_cast<const void*>(&KERN<KS, TAPG>), #KERN "<" #KS ", " #TAPG ">", dg_bf16s_lds(KS, TAPG)}
static const DgKernel kBf16s[3] = {BF16S_K(igemm_bf16s_kernel, 1, 1), BF16S_K(igemm_bf16s_kernel, 3, 9),
                                   BF16S_K(igemm_bf16s_head_kernel, 3, 9)};
#undef BF16S_K
const DgKernel* dg_conv_bf16s_kernel(int KS, bool head) { return &kBf16s[head ? 2 : (KS == 3 ? 1 : 0)]; }

static bool aligned16_h(const TViewH& v) {
  return !v.p || (!(v.sX % 8) && !(v.sY % 8) && !(v.sB % 8) && !(((uintptr_t)v.p) & 15));
}
// the epilogue's per-lane and per-pass byte offsets (up to four rows and sixteen pixels from the wave's origin) are ints
static bool offsets_fit(const TViewH& v) {
  return !v.p || (v.sX > 0 && v.sY > 0 && v.sB >= 0 && 2 * (4 * v.sY + 16 * v.sX + 32) < 0x7FFFFFFFL);
}

int dg_conv_bf16s_check(int KS, const ConvArgsH& a) {
  if (KS != 1 && KS != 3) { dg_set_error("dg_conv_bf16s: kernel size %d (1 or 3)", KS); return DG_ERR_UNSUPPORTED; }
  if (!a.in.p || !a.out.p || a.B < 1 || a.H < 1 || a.W < 1) { dg_set_error("dg_conv_bf16s: bad argument"); return DG_ERR_ARG; }
  if (a.Cin < 8 || (a.Cin % 8) || a.Cout < 32 || (a.Cout % 32)) {
    dg_set_error("dg_conv_bf16s: %d -> %d channels (Cin a multiple of 8, Cout a multiple of 32)", a.Cin, a.Cout);
    return DG_ERR_UNSUPPORTED;
  }
  const int ng = a.groups > 1 ? a.groups : 1;
  if (ng != 1 && ng != 4) { dg_set_error("dg_conv_bf16s: groups must be 0, 1 or 4"); return DG_ERR_ARG; }
  bool al = aligned16_h(a.in) && aligned16_h(a.out) && aligned16_h(a.ep.res) && aligned16_h(a.ep.pool);
  for (int g = 0; g < ng && ng > 1; ++g) al = al && !(a.out_group_off[g] % 8);
  if (!al) { dg_set_error("dg_conv_bf16s: every view must be 16-byte aligned (pointer, strides in multiples of 8 elements)"); return DG_ERR_ARG; }
  if (!offsets_fit(a.in) || !offsets_fit(a.out) || !offsets_fit(a.ep.res) || !offsets_fit(a.ep.pool)) {
    dg_set_error("dg_conv_bf16s: view strides out of range");
    return DG_ERR_ARG;
  }
  if (a.ep.film_mul && (!a.ep.film_add || (a.ep.film_ld % 4))) { dg_set_error("dg_conv_bf16s: FiLM needs both vectors, ld a multiple of 4"); return DG_ERR_ARG; }
  if ((a.ep.scale != nullptr) != (a.ep.shift != nullptr)) { dg_set_error("dg_conv_bf16s: scale and shift come together"); return DG_ERR_ARG; }
  if (a.ep.pool.p && ((a.H | a.W) & 1)) { dg_set_error("dg_conv_bf16s: the fused pool needs even H and W"); return DG_ERR_ARG; }
  const long total = (long)cdiv(a.W, 16) * cdiv(a.H, 16) * a.B * cdiv(a.Cout, 32) * ng;
  if (total > 0x7FFFFFFFL) { dg_set_error("dg_conv_bf16s: %ld work items", total); return DG_ERR_UNSUPPORTED; }
  if (a.ep.head_out) {
    // the fused head needs the 4 lanes of a pixel to hold ALL its channels: one channel tile, one group, 3x3
    if (KS != 3 || a.Cout != 32 || ng != 1) {
      dg_set_error("dg_conv_bf16s: the fused head needs a 3x3 convolution to exactly 32 channels, ungrouped (KS %d, Cout %d, groups %d)",
                   KS, a.Cout, ng);
      return DG_ERR_UNSUPPORTED;
    }
    if (!a.ep.head_w || !a.ep.head_b || (((uintptr_t)a.ep.head_w) & 15)) {
      dg_set_error("dg_conv_bf16s: the fused head needs its weights (16-byte aligned) and bias");
      return DG_ERR_ARG;
    }
    return DG_OK;
  }
  if (a.ep.head_skip_out) { dg_set_error("dg_conv_bf16s: head_skip_out without a fused head"); return DG_ERR_ARG; }
  return DG_OK;
}

int dg_conv_bf16s(int KS, const ConvArgsH& a, hipStream_t st) {
  DGCHECK(dg_conv_bf16s_check(KS, a));
  const int ng = a.groups > 1 ? a.groups : 1;
  for (int g = 0; g < ng && ng > 1; ++g)
    if (!a.w_group[g]) { dg_set_error("dg_conv_bf16s: null weight panel of group %d", g); return DG_ERR_ARG; }
  if (ng == 1 && !a.w) { dg_set_error("dg_conv_bf16s: null weight panel"); return DG_ERR_ARG; }
  ConvArgsH b = a;
  b.lgx = cdiv(a.W, 16) * cdiv(a.H, 16) * a.B;
  b.lgy = cdiv(a.Cout, 32) * ng;
  const DgKernel* k = dg_conv_bf16s_kernel(KS, a.ep.head_out != nullptr);
  return dg_launch(*k, (unsigned)((long)b.lgx * b.lgy), 256, (size_t)k->attr_lds, &b, st);
}

// ---------------------------------------------------------------------------
// gen_0: Cin = 1 or 2 -> up to 32 channels, 3x3, fp32 in, bf16 out.  HBM-bound (the output write is the traffic that
// matters) VALU kernel after conv_cin12_kernel (direct.hip): thread = 4 consecutive pixels x 8 consecutive output
// channels, so that each store is 16 bytes of bf16 and the 4 lanes of a pixel fill its 64 bytes.  Block = 16 x 16 pixels.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void edge_conv_bf16s_kernel(const EdgeArgsH a) {
  constexpr int KS = 3, PAD = 1, ROWS = 16;
  constexpr int TWX = 16 + KS - 1, TWY = ROWS + KS - 1;
  constexpr int RS = 24;   // LDS row stride (floats): 18 used + read slack
  constexpr int CT = 32;
  __shared__ __attribute__((aligned(16))) float xs[2 * TWY * RS];
  __shared__ __attribute__((aligned(16))) float ws[2 * KS * KS * CT];

  const int tid = threadIdx.x;
  const int tilesX = (a.W + 15) >> 4, tilesY = (a.H + ROWS - 1) / ROWS;
  int t = blockIdx.x;
  const int tx0 = (t % tilesX) * 16;
  t /= tilesX;
  const int ty0 = (t % tilesY) * ROWS;
  const int b = t / tilesY;
  const int g = tid & 3, pg = tid >> 2;      // channel group of 8, pixel group
  const int qx = (pg & 3) * 4, py = pg >> 2;
  const float* inb = a.in + (long)b * a.H * a.W * a.Cin;

  for (int q = tid; q < a.Cin * TWY * RS; q += 256) {
    const int lx = q % RS, ly = (q / RS) % TWY, c = q / (RS * TWY);
    const int iy = ty0 + ly - PAD, ix = tx0 + lx - PAD;
    float v = 0.f;
    if (lx < TWX && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = inb[((long)iy * a.W + ix) * a.Cin + c];
    xs[q] = v;
  }
  for (int q = tid; q < a.Cin * KS * KS * CT; q += 256) {
    const int n = q % CT, tap = (q / CT) % (KS * KS), c = q / (CT * KS * KS);
    ws[q] = (n < a.Cout) ? a.w[((long)tap * a.Cin + c) * a.Cout + n] : 0.f;
  }
  __syncthreads();

  f32x8 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
  // channel, tap row, tap column: a fixed order
  for (int c = 0; c < a.Cin; ++c) {
#pragma unroll
    for (int ty = 0; ty < KS; ++ty) {
      const float* row = xs + (c * TWY + py + ty) * RS + qx;
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(row);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(row + 4);
      const float xv[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
#pragma unroll
      for (int tx = 0; tx < KS; ++tx) {
        const f32x8 w8 = *reinterpret_cast<const f32x8*>(ws + ((c * KS + ty) * KS + tx) * CT + 8 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[j][k] = fmaf(xv[j + tx], w8[k], acc[j][k]);
      }
    }
  }
  const int co = 8 * g;
  const int oy = ty0 + py;
  if (co < a.Cout && oy < a.H) {
    f32x8 sc8, sh8;
#pragma unroll
    for (int k = 0; k < 8; ++k) { sc8[k] = 1.f; sh8[k] = 0.f; }
    if (a.scale) {
      sc8 = *reinterpret_cast<const f32x8*>(a.scale + co);
      sh8 = *reinterpret_cast<const f32x8*>(a.shift + co);
    }
    if (a.bias) {
      const f32x8 bias8 = *reinterpret_cast<const f32x8*>(a.bias + co);
#pragma unroll
      for (int k = 0; k < 8; ++k) sh8[k] = fmaf(bias8[k], sc8[k], sh8[k]);
    }
    __bf16* orow = a.out.p + (long)b * a.out.sB + (long)oy * a.out.sY + co;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ox = tx0 + qx + j;
      if (ox >= a.W) continue;
      f32x8 v;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v[k] = fmaf(acc[j][k], sc8[k], sh8[k]);
        if (a.relu) v[k] = dg_vmax(v[k], 0.f);
      }
      *reinterpret_cast<bf16x8*>(orow + (long)ox * a.out.sX) = __builtin_convertvector(v, bf16x8);   // RNE
    }
  }
}

int dg_edge_conv_bf16s(const EdgeArgsH& a, hipStream_t st) {
  if (!a.in || !a.w || !a.out.p || a.B < 1 || a.H < 1 || a.W < 1) { dg_set_error("dg_edge_conv_bf16s: bad argument"); return DG_ERR_ARG; }
  if (a.Cin < 1 || a.Cin > 2 || a.Cout < 8 || a.Cout > 32 || (a.Cout % 8)) {
    dg_set_error("dg_edge_conv_bf16s: %d -> %d channels (Cin 1 or 2, Cout 8, 16, 24 or 32)", a.Cin, a.Cout);
    return DG_ERR_UNSUPPORTED;
  }
  if ((a.scale != nullptr) != (a.shift != nullptr)) { dg_set_error("dg_edge_conv_bf16s: scale and shift come together"); return DG_ERR_ARG; }
  if (!aligned16_h(a.out)) { dg_set_error("dg_edge_conv_bf16s: the output view must be 16-byte aligned"); return DG_ERR_ARG; }
  const long blocks = (long)cdiv(a.W, 16) * cdiv(a.H, 16) * a.B;
  if (blocks > 0x7FFFFFFFL) { dg_set_error("dg_edge_conv_bf16s: %ld blocks", blocks); return DG_ERR_UNSUPPORTED; }
  hipLaunchKernelGGL(edge_conv_bf16s_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

// ---------------------------------------------------------------------------
// head: 1x1 convolution to one channel (+ tanh), bf16 in, fp32 out; C / 8 lanes per pixel, 16 bytes each
// ---------------------------------------------------------------------------
__global__ void head_bf16s_kernel(const __bf16* __restrict__ a, long ld, const float* __restrict__ w,
                                  const float* __restrict__ b, float* __restrict__ out, long P, int LP, int tanh_act) {
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long p = t / LP;
  const int part = (int)(t % LP);
  float v = 0.f;
  if (p < P) {
    const f32x8 av = __builtin_convertvector(*reinterpret_cast<const bf16x8*>(a + p * ld + part * 8), f32x8);
    const f32x8 wv = *reinterpret_cast<const f32x8*>(w + part * 8);
    v = av[0] * wv[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) v = fmaf(av[k], wv[k], v);
  }
  for (int o = LP >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (p < P && part == 0) {
    v += b[0];
    out[p] = tanh_act ? tanhf(v) : v;
  }
}

int dg_head_bf16s(const __bf16* a, long ld, const float* w, const float* b, float* out, long P, int C, int tanh_act,
                  hipStream_t st) {
  if (!a || !w || !b || !out || P < 1) { dg_set_error("dg_head_bf16s: bad argument"); return DG_ERR_ARG; }
  const int LP = C / 8;
  if (C < 8 || (C % 8) || LP > 64 || (LP & (LP - 1))) { dg_set_error("dg_head_bf16s: C/8 must be a power of two <= 64"); return DG_ERR_ARG; }
  if (ld < C || (ld % 8) || (((uintptr_t)a) & 15) || (((uintptr_t)w) & 15)) { dg_set_error("dg_head_bf16s: the input must be 16-byte aligned, ld a multiple of 8"); return DG_ERR_ARG; }
  const long blocks = (P * LP + 255) / 256;
  if (blocks > 0x7FFFFFFFL) { dg_set_error("dg_head_bf16s: %ld blocks", blocks); return DG_ERR_UNSUPPORTED; }
  hipLaunchKernelGGL(head_bf16s_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, ld, w, b, out, P, LP, tanh_act);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

// ---------------------------------------------------------------------------
// DEP-UResNet head: 1x1 convolution to K = 2..8 class logits + softmax over them, bf16 in, fp32 out.
// head_bf16s_kernel's lane mapping (C / 8 lanes per pixel, one 16-byte load each, consecutive lanes on consecutive
// addresses) with K columns of w (C, K) instead of one: logit k is formed exactly as that kernel forms its output with
// column k (per 8-channel part v = a0 w0, fmaf over channels 1..7; the same xor butterfly; + b[k]), and the softmax is
// dg_softmax_row (softmax_row.h), the text softmax_ce_kernel runs -- so both halves have an existing kernel to be
// bit-equal to.  HBM-bound (2 C + 4 K bytes per pixel): a grid-stride loop, so that a lane's 8 K weights are loaded once;
// the stride is a multiple of 256, hence of LP, and a lane keeps its part.  Lane 0 of a pixel stores its row.
// One body; the reference's four classes keep the kernel name the resource checks know, the other counts are
// instantiations of head_softmax_k_bf16s_kernel.
// ---------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void head_softmax_bf16s_body(const __bf16* __restrict__ a, long ld,
                                                        const float* __restrict__ w, const float* __restrict__ b,
                                                        float* __restrict__ probs, float* __restrict__ logits, long P,
                                                        int lgLP) {
#pragma clang fp contract(off)
  const int LP = 1 << lgLP;
  const int part = threadIdx.x & (LP - 1);
  float wv[8][K];
#pragma unroll
  for (int j = 0; j < 8; ++j) dg_row_load<K>(w + (part * 8 + j) * K, wv[j]);
  const long total = P << lgLP;
  // the trip count is the same for every lane of a block: the shuffles below run with all 64 lanes
  for (long t0 = blockIdx.x * 256L; t0 < total; t0 += gridDim.x * 256L) {
    const long p = (t0 + threadIdx.x) >> lgLP;
    float z[K];
#pragma unroll
    for (int k = 0; k < K; ++k) z[k] = 0.f;
    if (p < P) {
      const f32x8 av = __builtin_convertvector(*reinterpret_cast<const bf16x8*>(a + p * ld + part * 8), f32x8);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float v = av[0] * wv[0][k];
#pragma unroll
        for (int j = 1; j < 8; ++j) v = fmaf(av[j], wv[j][k], v);
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
      if (logits) dg_row_store<K>(logits + p * K, z);
      float pr[K];
      dg_softmax_row<K>(z, pr);
      dg_row_store<K>(probs + p * K, pr);
    }
  }
}
__global__ __launch_bounds__(256) void head_softmax_bf16s_kernel(const __bf16* __restrict__ a, long ld,
                                                                  const float* __restrict__ w,
                                                                  const float* __restrict__ b, float* __restrict__ probs,
                                                                  float* __restrict__ logits, long P, int lgLP) {
  head_softmax_bf16s_body<4>(a, ld, w, b, probs, logits, P, lgLP);
}
template <int K>
__global__ __launch_bounds__(256) void head_softmax_k_bf16s_kernel(const __bf16* __restrict__ a, long ld,
                                                                    const float* __restrict__ w,
                                                                    const float* __restrict__ b,
                                                                    float* __restrict__ probs,
                                                                    float* __restrict__ logits, long P, int lgLP) {
  head_softmax_bf16s_body<K>(a, ld, w, b, probs, logits, P, lgLP);
}

int dg_head_softmax_bf16s(const __bf16* a, long ld, const float* w, const float* b, float* probs, float* logits, long P,
                          int C, int K, hipStream_t st) {
  if (!a || !w || !b || !probs || P < 1) { dg_set_error("dg_head_softmax_bf16s: bad argument"); return DG_ERR_ARG; }
  if (K < DG_MIN_CLASSES || K > DG_MAX_CLASSES) {
    dg_set_error("dg_head_softmax_bf16s: %d classes (the head covers %d to %d)", K, DG_MIN_CLASSES, DG_MAX_CLASSES);
    return DG_ERR_UNSUPPORTED;
  }
  const int LP = C / 8;
  if (C < 8 || (C % 8) || LP > 64 || (LP & (LP - 1))) { dg_set_error("dg_head_softmax_bf16s: C/8 must be a power of two <= 64"); return DG_ERR_ARG; }
  if (ld < C || (ld % 8) || (((uintptr_t)a) & 15)) { dg_set_error("dg_head_softmax_bf16s: the input must be 16-byte aligned, ld a multiple of 8"); return DG_ERR_ARG; }
  // rows of K floats: 16-byte accesses where K % 4 == 0, else float by float
  const uintptr_t al = (K % 4 == 0) ? 15 : 3;
  if ((((uintptr_t)w) | ((uintptr_t)probs) | ((uintptr_t)logits)) & al) {
    dg_set_error("dg_head_softmax_bf16s: the weights, probs and logits must be %d-byte aligned for %d classes", (int)al + 1, K);
    return DG_ERR_ARG;
  }
  if (P > (0x7FFFFFFFFFFFFFFFL >> 8) / (ld > 64 ? ld : 64)) { dg_set_error("dg_head_softmax_bf16s: %ld pixels", P); return DG_ERR_UNSUPPORTED; }
  int lg = 0;
  while ((1 << lg) < LP) ++lg;
  long blocks = (P * LP + 255) / 256;
  if (blocks > 2048) blocks = 2048;   // 256 CUs x 8 resident blocks; the loop takes the rest
  switch (K) {
    case 4: hipLaunchKernelGGL(head_softmax_bf16s_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, ld, w, b, probs, logits, P, lg); break;
#define DG_HS(N) case N: hipLaunchKernelGGL(head_softmax_k_bf16s_kernel<N>, dim3((unsigned)blocks), dim3(256), 0, st, a, ld, w, b, probs, logits, P, lg); break;
    DG_HS(2) DG_HS(3) DG_HS(5) DG_HS(6) DG_HS(7) DG_HS(8)
#undef DG_HS
  }
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

// ---------------------------------------------------------------------------
// bf16 view -> dense fp32 (exact), 8 channels per thread where the view allows, else one
// ---------------------------------------------------------------------------
__global__ void widen_bf16_kernel(TViewH s, long npix, int H, int W, int C, int vec, float* __restrict__ dst) {
  const int per = vec ? C / 8 : C;
  const long total = npix * per;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long pix = i / per;
    const int part = (int)(i - pix * per);
    const int x = (int)(pix % W);
    const long t = pix / W;
    const int y = (int)(t % H);
    const long b = t / H;
    const __bf16* src = s.p + b * s.sB + (long)y * s.sY + (long)x * s.sX;
    if (vec) {
      const f32x8 v = __builtin_convertvector(*reinterpret_cast<const bf16x8*>(src + part * 8), f32x8);
      *reinterpret_cast<f32x8*>(dst + pix * C + part * 8) = v;
    } else {
      dst[pix * C + part] = (float)src[part];
    }
  }
}

int dg_widen_bf16(TViewH src, int N, int H, int W, int C, float* dst, hipStream_t st) {
  if (!src.p || !dst || N < 1 || H < 1 || W < 1 || C < 1) { dg_set_error("dg_widen_bf16: bad argument"); return DG_ERR_ARG; }
  const int vec = (C % 8 == 0) && aligned16_h(src) && !(((uintptr_t)dst) & 31);
  const long npix = (long)N * H * W;
  const long total = npix * (vec ? C / 8 : C);
  long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(widen_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, npix, H, W, C, vec, dst);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
