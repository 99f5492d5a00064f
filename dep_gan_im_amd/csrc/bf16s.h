// bf16 activation STORAGE for the generator forward of a bf16_mfma context (BASELINE config 4 as SURVEY 8d words it:
// bf16 weights AND bf16 activations, fp32 accumulate).  Kernels in igemm_bf16s.hip, drivers in model_bf16s.hip.
//
// Storage contract: element type bf16, NHWC, channel stride 1, view strides in elements (TViewH).
// A stored value is RNE_bf16(v) of the fp32 epilogue result v (v_cvt_pk_bf16_f32 through __builtin_convertvector) and
// nothing else.  Everything between the contraction and the store is fp32 in the order of igemm_epilogue.inc:
//   v = fma(acc, scale, bias * scale + shift);  v = film_preact(v, mul, add);  v = max(v, 0);  v += widen(res)
// The 2x2 max-pool is the max of the stored values (RNE is monotone: the same as rounding the fp32 max).
#pragma once
#include "common.h"

struct EpilogueH {
  const float* bias;
  const float* scale;
  const float* shift;
  const float* film_mul;
  const float* film_add;
  int film_ld;   // row stride (floats) of film_mul / film_add
  TViewH res;    // residual operand, read as bf16 and widened (exact)
  int relu;
  TViewH pool;   // non-null: the 2x2 / stride-2 max-pool of the stored output, (H/2, W/2) pixels; H and W even
  // gen_segmentation fused (igemm_bf16s_head_kernel; KS = 3, Cout == 32, ungrouped): head_out[pixel] =
  // act(sum_c stored[pixel][c] head_w[c] + head_b[0]), dense (B, H, W) fp32, in head_bf16s_kernel's arithmetic and order
  // -- bit-equal to dg_head_bf16s of the stored tensor.  head_skip_out: the 16-byte stores of `out` are not issued
  // (forward-only passes); pool and residual are unaffected.
  const float* head_w;
  const float* head_b;
  float* head_out;   // non-null selects the fused-head kernel
  int head_tanh;
  int head_skip_out;
};

struct ConvArgsH {
  TViewH in, out;
  const float* w;   // packed bf16 panel of dg_plan_conv_bf16 (dg_pack_weights*, PackJob::bf16 = 1)
  int B, H, W, Cin, Cout;
  EpilogueH ep;
  // grouped launch as ConvArgs::groups: 4 convolutions sharing input and epilogue constants (the taps of a 2x2 / stride-2
  // transposed convolution); group g reads w_group[g] and writes to out.p + out_group_off[g] (elements)
  int groups;
  int lgx, lgy;     // logical grid, filled by the launcher
  const float* w_group[4];
  long out_group_off[4];
};

// bf16-in / bf16-out implicit GEMM on v_mfma_f32_32x32x16_bf16, KS in {1, 3}; Cin % 8 == 0, Cout % 32 == 0, every view
// 16-byte aligned (pointer and strides).  Argument checks come before the launch.
int dg_conv_bf16s(int KS, const ConvArgsH& a, hipStream_t st);
// every check of dg_conv_bf16s but the weight panels' pointers, no HIP call: what an entry that packs its weights into a
// temporary runs first, so that a call it refuses allocates and launches nothing
int dg_conv_bf16s_check(int KS, const ConvArgsH& a);
// the entry dg_conv_bf16s launches (its name is what the profiles print)
const DgKernel* dg_conv_bf16s_kernel(int KS, bool head = false);
// dynamic LDS of the kernels built from igemm_bf16s_kernel.inc / igemm_bf16_main.inc: the halo tile and the staged taps of
// 32 weight rows, in 80-byte rows, or the epilogue transpose where that is larger
constexpr int dg_bf16s_lds(int KS, int TAPG) {
  const size_t k = (size_t)((16 + KS - 1) * (16 + KS - 1) + TAPG * 32) * 80, e = (size_t)4 * 64 * (32 + 4) * sizeof(float);
  return (int)(k > e ? k : e);
}

// gen_0: 3x3, Cin in {1, 2}, dense fp32 input, HWIO fp32 weights, affine + ReLU, bf16 output; Cout % 8 == 0, <= 32
struct EdgeArgsH {
  const float* in;   // dense (B, H, W, Cin)
  const float* w;    // HWIO
  const float* bias;
  const float* scale;
  const float* shift;
  TViewH out;
  int B, H, W, Cin, Cout, relu;
};
int dg_edge_conv_bf16s(const EdgeArgsH& a, hipStream_t st);

// gen_segmentation: out[p] = act(sum_c a[p * ld + c] w[c] + b[0]); bf16 in, fp32 out; C % 8 == 0, C / 8 a power of two
int dg_head_bf16s(const __bf16* a, long ld, const float* w, const float* b, float* out, long P, int C, int tanh_act,
                  hipStream_t st);

// gen_segmentation of the DEP-UResNet: z[p][k] = sum_c a[p * ld + c] w[c * K + k] + b[k] in dg_head_bf16s's arithmetic
// and order per column k, probs[p] = softmax(z[p]) in softmax_ce_kernel's statements for K classes (softmax_row.h;
// contraction off around both); bf16 in, dense fp32 (P, K) out, the logits too where `logits` is given.  K = 2..8; C as
// dg_head_bf16s; a 16-byte aligned; w, probs and logits 16-byte aligned where K % 4 == 0 (16-byte rows), else 4-byte.
// Anything else is a status before any launch.
int dg_head_softmax_bf16s(const __bf16* a, long ld, const float* w, const float* b, float* probs, float* logits, long P,
                          int C, int K = 4, hipStream_t st = nullptr);

// dense fp32 (N, H, W, C) copy of a bf16 view (exact)
int dg_widen_bf16(TViewH src, int N, int H, int W, int C, float* dst, hipStream_t st);
