// Training forward of the generator's FiLM layers on bf16 activation storage (bf16s_train.h): igemm_bf16s_kernel's text
// a third time, under its own name, with the stores of RNE_bf16(u) and of the FiLM ReLU decision bits added to the
// epilogue.  A sibling kernel in its own translation unit: the two plain kernels and the fused-head one in
// igemm_bf16s.hip are built from the same text with the hook off and keep their code.
#include <stdlib.h>

#include "bf16s_train.h"
#include "epilogue.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8), aligned(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

#define IGEMM_BF16S_KERNEL igemm_bf16s_train_kernel
#define IGEMM_BF16S_HEAD 0
#define IGEMM_BF16S_TRAIN 1
#define IGEMM_BF16S_ARGS ConvArgsHT
#include "igemm_bf16s_kernel.inc"
#undef IGEMM_BF16S_KERNEL
#undef IGEMM_BF16S_HEAD
#undef IGEMM_BF16S_TRAIN
#undef IGEMM_BF16S_ARGS

static bool al16(const TViewH& v) {
  return v.p && !(v.sX % 8) && !(v.sY % 8) && !(v.sB % 8) && !(((uintptr_t)v.p) & 15);
}
static bool fits(const TViewH& v) { return v.sX > 0 && v.sY > 0 && v.sB >= 0 && 2 * (4 * v.sY + 16 * v.sX + 32) < 0x7FFFFFFFL; }

int dg_conv_bf16s_train_check(const ConvArgsHT& a) {
  if (!a.in.p || !a.out.p || !a.u.p || !a.fdec || a.B < 1 || a.H < 1 || a.W < 1) {
    dg_set_error("dg_conv_bf16s_train: bad argument");
    return DG_ERR_ARG;
  }
  if (a.Cin < 8 || (a.Cin % 8) || a.Cout < 32 || (a.Cout % 32)) {
    dg_set_error("dg_conv_bf16s_train: %d -> %d channels (Cin a multiple of 8, Cout a multiple of 32)", a.Cin, a.Cout);
    return DG_ERR_UNSUPPORTED;
  }
  if (a.groups > 1 || a.ep.head_out || a.ep.head_skip_out || a.ep.pool.p) {
    dg_set_error("dg_conv_bf16s_train: one ungrouped 3x3 convolution without fused head or pool");
    return DG_ERR_UNSUPPORTED;
  }
  if (!a.ep.film_mul || !a.ep.film_add || (a.ep.film_ld % 4)) { dg_set_error("dg_conv_bf16s_train: FiLM needs both vectors, ld a multiple of 4"); return DG_ERR_ARG; }
  if ((a.ep.scale != nullptr) != (a.ep.shift != nullptr)) { dg_set_error("dg_conv_bf16s_train: scale and shift come together"); return DG_ERR_ARG; }
  if (!al16(a.in) || !al16(a.out) || !al16(a.u) || (a.ep.res.p && !al16(a.ep.res)) || (((uintptr_t)a.fdec) & 3)) {
    dg_set_error("dg_conv_bf16s_train: every view must be 16-byte aligned (pointer, strides in multiples of 8 elements)");
    return DG_ERR_ARG;
  }
  if (!fits(a.in) || !fits(a.out) || !fits(a.u) || (a.ep.res.p && !fits(a.ep.res))) {
    dg_set_error("dg_conv_bf16s_train: view strides out of range");
    return DG_ERR_ARG;
  }
  const long total = (long)cdiv(a.W, 16) * cdiv(a.H, 16) * a.B * cdiv(a.Cout, 32);
  if (total > 0x7FFFFFFFL) { dg_set_error("dg_conv_bf16s_train: %ld work items", total); return DG_ERR_UNSUPPORTED; }
  return DG_OK;
}

// the one kernel of this file: the launch and the profile's name read the same entry
const DgKernel* dg_conv_bf16s_train_kernel() {
  static const DgKernel k = {reinterpret_cast<const void*>(&igemm_bf16s_train_kernel<3, 9>), "igemm_bf16s_train_kernel<3, 9>",
                             dg_bf16s_lds(3, 9)};
  return &k;
}

int dg_conv_bf16s_train(const ConvArgsHT& a, hipStream_t st) {
  DGCHECK(dg_conv_bf16s_train_check(a));
  if (!a.w) { dg_set_error("dg_conv_bf16s_train: null weight panel"); return DG_ERR_ARG; }
  ConvArgsHT b = a;
  b.groups = 0;
  b.lgx = cdiv(a.W, 16) * cdiv(a.H, 16) * a.B;
  b.lgy = cdiv(a.Cout, 32);
  const DgKernel* k = dg_conv_bf16s_train_kernel();
  return dg_launch(*k, (unsigned)((long)b.lgx * b.lgy), 256, (size_t)k->attr_lds, &b, st);
}
