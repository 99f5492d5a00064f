// Weight-gradient contraction on the bf16 matrix cores with the ACTIVATION operand staged from bf16 memory: the
// generator update on bf16 activation storage (bf16s_train.h).  The same included text as wgrad_bf16_kernel
// (wgrad_bf16_kernel.inc) in its bf16 operand form: the halo tile of x is fetched as 16-byte pieces of 8 bf16 (half the
// bytes, half the load instructions, no conversion) and copied into the same [pixel][32 channels] LDS image; dy is
// staged as fp32 and rounded (RNE) while committed, as there.  The result equals dg_wgrad_bf16 on the widened operand
// bit for bit (tests/test_gpu_g_update_storage.py).
// KS in {1, 3}: the generator's 3x3 layers and the four taps of its transposed convolutions.
#include <stdlib.h>

#include "bf16s_train.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define WGRAD_KERNEL wgrad_bf16s_kernel
#define WGRAD_ARGS WgradArgsH
#define WGRAD_X_BF16 1
#include "wgrad_bf16_kernel.inc"
#undef WGRAD_KERNEL
#undef WGRAD_ARGS
#undef WGRAD_X_BF16

}  // namespace

bool dg_wgrad_bf16s_supported(int KS, int Cin, int Cout) {
  return (KS == 1 || KS == 3) && Cin >= 8 && (Cin % 8) == 0 && (Cout % 4) == 0;
}

// the launch plan of dg_wgrad_bf16s for a shape, without launching (depgan_debug_wgrad_plan)
int dg_wgrad_bf16s_plan(int KS, int B, int H, int W, int Cin, int Cout, int out[4]) {
  if (!dg_wgrad_bf16s_supported(KS, Cin, Cout)) {
    dg_set_error("dg_wgrad_bf16s: unsupported shape (KS=%d Cin=%d Cout=%d)", KS, Cin, Cout);
    return DG_ERR_UNSUPPORTED;
  }
  chunking(KS, B, H, W, Cin, Cout, &out[0], &out[1], &out[2], &out[3]);
  return DG_OK;
}

int dg_wgrad_bf16s(int KS, const WgradArgsH& a, int* nchunks_out, hipStream_t st) {
  if (!a.x.p || !a.dy.p || !a.part || !nchunks_out || a.B < 1 || a.H < 1 || a.W < 1) {
    dg_set_error("dg_wgrad_bf16s: bad argument");
    return DG_ERR_ARG;
  }
  if (!dg_wgrad_bf16s_supported(KS, a.Cin, a.Cout)) {
    dg_set_error("dg_wgrad_bf16s: unsupported shape (KS=%d Cin=%d Cout=%d)", KS, a.Cin, a.Cout);
    return DG_ERR_UNSUPPORTED;
  }
  if ((a.x.sX % 8) || (a.x.sY % 8) || (a.x.sB % 8) || (a.dy.sX % 4) || (a.dy.sY % 4) || (a.dy.sB % 4) ||
      (((uintptr_t)a.x.p) & 15) || (((uintptr_t)a.dy.p) & 15)) {
    dg_set_error("dg_wgrad_bf16s: strides must be multiples of 16 bytes and the operands 16-byte aligned");
    return DG_ERR_ARG;
  }
  return run(KS, a, nchunks_out, st);
}
