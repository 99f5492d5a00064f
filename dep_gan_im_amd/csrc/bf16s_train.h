// Generator UPDATE on bf16 activation storage (depgan_set_g_update_storage): what the backward pass
// of a bf16_mfma context needs when every generator activation lives in HBM as bf16 (bf16s.h) and every gradient as fp32.
// Kernels in igemm_bf16s_train.hip (forward of the FiLM layers), igemm_bf16_mh.hip (backward-data), wgrad_bf16s.hip
// (weight gradient) and ops_bf16s.hip (the HBM-bound operators); driver in model_bf16s_train.hip.
#pragma once
#include "bf16s.h"

// FiLM layer of the training forward: dg_conv_bf16s's 3x3 launch that ALSO stores u = RNE_bf16 of the pre-FiLM value (the
// fp32 one goes on into FiLM unchanged, so `out` has the bits of dg_conv_bf16s) and the ReLU decision the epilogue took
// on the FiLM result: bit (c & 7) of byte fdec[((b H + y) W + x) (Cout / 8) + c / 8] = (film_preact(u) > 0).
struct ConvArgsHT : ConvArgsH {
  TViewH u;
  unsigned char* fdec;   // dense, 4-byte aligned, B H W Cout / 8 bytes
};
int dg_conv_bf16s_train(const ConvArgsHT& a, hipStream_t st);
int dg_conv_bf16s_train_check(const ConvArgsHT& a);   // its checks but the weight panel's pointer, no HIP call
const DgKernel* dg_conv_bf16s_train_kernel();            // the entry it launches
static inline size_t dg_film_dec_bytes(int B, int H, int W, int C) { return (size_t)B * H * W * (C / 8); }

// Backward-data (3x3, or 1x1 with ConvArgs::cpt gathering the four grids of a transposed convolution) on the same
// included main-loop text as igemm_bf16_kernel (igemm_bf16_main.inc) -- dy fp32 in HBM, rounded while staged, as in every bf16_mfma context -- whose ReLU mask
// operand is a bf16 view: out = accumulate ? out + v : v, v = (mask_h > 0) ? acc + res : 0.  Of a.ep only res and
// accumulate are read (everything else must be unset); a.Cout % 32 == 0, a.Cin % 4 == 0.
int dg_conv_bf16_mh(const ConvPlan& pl, const ConvArgs& a, TViewH mask_h, hipStream_t st);
const DgKernel* dg_conv_bf16_mh_kernel(int KS);   // the entry it launches

// Weight gradient on the bf16 pipe, activation operand staged from bf16 memory (16-byte pieces of 8 bf16, no rounding
// step), dy staged as fp32 and rounded while committed: the same included text as wgrad_bf16_kernel
// (wgrad_bf16_kernel.inc), hence its tiles, LDS images, chunking, K order and slab format -- bit-equal to dg_wgrad_bf16 on the widened operand.  KS in {1, 3}; Cin % 8 == 0, Cout % 4 == 0.
struct WgradArgsH {
  TViewH x;
  TView dy;
  float* part;
  int B, H, W, Cin, Cout;
  int nTiles, tilesPerChunk;
  float* colpart;
  int colB;
};
bool dg_wgrad_bf16s_supported(int KS, int Cin, int Cout);
int dg_wgrad_bf16s(int KS, const WgradArgsH& a, int* nchunks, hipStream_t st);
int dg_wgrad_bf16s_plan(int KS, int B, int H, int W, int Cin, int Cout, int out[4]);   // as dg_wgrad_plan (common.h)

// out(2Ho, 2Wo) = ((a > 0) ? skip + (argmax ? dpool : 0) : 0), `a` bf16; the arg-max of a 2x2 window is the FIRST
// maximum in the order (0,0), (0,1), (1,0), (1,1) -- pool_bwd_kernel's rule.  C % 8 == 0.
int dg_unpool_mask_bf16s(TView dpool, TViewH a, TView skip /*optional*/, TView out, int B, int Ho, int Wo, int C,
                         hipStream_t st);
// FiLM backward from the stored u (bf16, dense) and the stored decision bits: dv = dec ? dr : 0; du = dv * mul;
// dmul[b][c] = sum_p dv * u; dadd[b][c] = sum_p dv.  dr / du dense fp32 (B, HW, C); C % 8 == 0, C <= 256.
size_t dg_film_bwd_bf16s_scratch(int B, int C);
int dg_film_bwd_bf16s(const float* dr, const __bf16* u, const unsigned char* dec, const float* fmul, int film_ld, float* du,
                      float* dmul, float* dadd, int B, long HW, int C, float* scratch, size_t scratch_floats,
                      hipStream_t st);
// head backward: out[c] = sum_p rowmul[p] a[p ld + c] (C % 8 == 0, C <= 256) and dz[p][c] = (a > 0) ? dpre[p] w[c] : 0
size_t dg_colsum_rowmul_bf16s_scratch(long P, int C);
int dg_colsum_rowmul_bf16s(const __bf16* a, long ld, long P, int C, const float* rowmul, float* out, float* scratch,
                           size_t scratch_floats, hipStream_t st);
int dg_head_bwd_bf16s(const float* dpre, const float* w, const __bf16* a, long ld, float* dz, long P, int C,
                      hipStream_t st);
// 0 / 1 bytes, one per element, from the packed decision bits (n = number of elements, a multiple of 8)
int dg_unpack_bits(const unsigned char* bits, unsigned char* out, long n, hipStream_t st);
