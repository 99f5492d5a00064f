// Weight-gradient contraction on the CDNA4 bf16 matrix cores (BASELINE configs[3]).
//
//   dW[tap][ci][co] = sum_{b,y,x} X[b, y+ty-p, x+tx-p, ci] * D[b, y, x, co]          (GT:549, 568, 594; A6)
//
// fp32 operands in HBM, rounded to bf16 (RNE, v_cvt_pk_bf16_f32) while a tile is committed to LDS, fp32 accumulation
// in v_mfma_f32_32x32x16_bf16 -- the weight-gradient counterpart of igemm_bf16.hip.  GEMM view as in wgrad.hip: M = ci,
// N = co, K = pixels; one workgroup owns one (ci tile, co tile) and a contiguous range of 16 x 16 pixel tiles and
// writes ONE partial slab in wgrad.hip's format (the same deterministic finish launch reduces them: no float atomics).
// Its 4 waves split the TAPS (wave w owns taps w, w + 4, ...: 3 / 2 / 2 / 2 of a 3x3 kernel, 7 / 6 / 6 / 6 of a 5x5 one)
// and walk all 16 pixel rows of a tile: every tap of a kernel size is served from ONE staging of the halo tile (a split
// by tap groups across workgroups multiplied the L2 traffic of the 5x5 layers by five), a wave's accumulators need no
// cross-wave reduction, and 48 / 112 accumulator registers leave room for two workgroups per CU.  (1x1: the waves split
// the rows and are summed through LDS.)
//
// K runs along PIXELS, which NHWC memory strides by the channel count, while the MFMA wants eight consecutive k of one
// row per lane: both operands are K-major.  The LDS images stay [pixel][32 channels] (64-byte rows, written with 8-byte
// stores straight from the channel-contiguous loads) and are read with ds_read_b64_tr_b16, which hands a group of 16
// lanes a 4-pixel x 16-channel block transposed: lane i gets channel i of 4 consecutive pixels.  Two reads per operand
// and MFMA; the D fragment of a pixel row serves all taps.
//
// At 16x the fp32 matrix rate the contraction is a few per cent of the launch: the kernel is bound by the HBM reads of
// its operands (4 bytes per element), which register staging keeps in flight under the MFMAs of the previous tile.
// Kernel text and host half: wgrad_bf16_kernel.inc, which wgrad_bf16s.hip includes with the x operand staged from bf16.
#include <stdlib.h>

#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

#define WGRAD_KERNEL wgrad_bf16_kernel
#define WGRAD_ARGS WgradArgs
#define WGRAD_X_BF16 0
#include "wgrad_bf16_kernel.inc"
#undef WGRAD_KERNEL
#undef WGRAD_ARGS
#undef WGRAD_X_BF16

}  // namespace

bool dg_wgrad_bf16_supported(int KS, int Cin, int Cout) {
  return (KS == 1 || KS == 3 || KS == 5) && Cin >= 8 && (Cin % 4) == 0 && (Cout % 4) == 0;
}

// the launch plan of dg_wgrad_bf16 for a shape, without launching (depgan_debug_wgrad_plan)
int dg_wgrad_bf16_plan(int KS, int B, int H, int W, int Cin, int Cout, int out[4]) {
  if (!dg_wgrad_bf16_supported(KS, Cin, Cout)) {
    dg_set_error("dg_wgrad_bf16: unsupported shape (KS=%d Cin=%d Cout=%d)", KS, Cin, Cout);
    return DG_ERR_UNSUPPORTED;
  }
  chunking(KS, B, H, W, Cin, Cout, &out[0], &out[1], &out[2], &out[3]);
  return DG_OK;
}

int dg_wgrad_bf16(int KS, const WgradArgs& a, int* nchunks_out, hipStream_t st) {
  if (!dg_wgrad_bf16_supported(KS, a.Cin, a.Cout)) {
    dg_set_error("dg_wgrad_bf16: unsupported shape (KS=%d Cin=%d Cout=%d)", KS, a.Cin, a.Cout);
    return DG_ERR_UNSUPPORTED;
  }
  if ((a.x.sX % 4) || (a.x.sY % 4) || (a.x.sB % 4) || (a.dy.sX % 4) || (a.dy.sY % 4) || (a.dy.sB % 4) ||
      (((uintptr_t)a.x.p) & 15) || (((uintptr_t)a.dy.p) & 15)) {
    dg_set_error("dg_wgrad_bf16: strides must be multiples of 4 floats and the operands 16-byte aligned");
    return DG_ERR_ARG;
  }
  return run(KS, a, nchunks_out, st);
}
