// Backward-data of the generator update on bf16 activation storage (bf16s_train.h): igemm_bf16_kernel's contraction --
// dy fp32 in HBM, rounded to bf16 (RNE) while the halo tile is committed, bf16 panels, fp32 accumulation, the same tile,
// LDS image, item order, gathered K and K order -- with an epilogue of its own whose ReLU mask operand is a bf16 view:
//   v = acc;  v += res;  v = (widen(mask) > 0) ? v : 0;  out = accumulate ? out + v : v
// in igemm_epilogue.inc's order (without bias and affine its fma(acc, 1, 0) is acc).  The shared epilogue text and the
// fp32 headline kernels that include it are not touched: this is a sibling kernel compiled only here.  The main loop
// is the same included text as igemm_bf16_kernel's (igemm_bf16_main.inc).  Lane mapping of the epilogue as
// igemm_bf16s_kernel, from the same included text (igemm_bf16_acc8.inc): 8 consecutive channels of one pixel per lane
// (two 16-byte fp32 accesses, one 16-byte bf16 mask read), 4 lanes per pixel, one 16-pixel row of the wave's 4 x 16 block
// per pass.
#include <stdlib.h>

#include "bf16s_train.h"
#include "epilogue.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x8 __attribute__((ext_vector_type(8), aligned(16)));

struct ConvArgsM : ConvArgs {
  TViewH mask_h;   // null: no mask
};

template <int KS, int TAPG>
__global__ __launch_bounds__(256, 2) void igemm_bf16_mh_kernel(const ConvArgsM a) {
  constexpr int NT = 32, MT = 2, CK = 32;
#define IGEMM_X_BF16 0
#include "igemm_bf16_main.inc"
#undef IGEMM_X_BF16
#include "igemm_bf16_acc8.inc"
  const bool has_res = a.ep.res.p != nullptr, has_msk = a.mask_h.p != nullptr, accum = a.ep.accumulate != 0;
  const int ox = tx0 + pl0;
  if (ox >= a.W) return;
  float* orow = a.out.p + out_goff + (long)b * a.out.sB + (long)ox * a.out.sX + co;
  const float* rrow = has_res ? a.ep.res.p + (long)b * a.ep.res.sB + (long)ox * a.ep.res.sX + co : nullptr;
  const __bf16* mrow = has_msk ? a.mask_h.p + (long)b * a.mask_h.sB + (long)ox * a.mask_h.sX + co : nullptr;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int oy = ty0 + 4 * wv + p;
    if (oy >= a.H) break;
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(es + (p * 16 + pl0) * CP + c8);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(es + (p * 16 + pl0) * CP + c8 + 4);
    f32x8 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = v0[k]; v[4 + k] = v1[k]; }
    if (has_res) {
      const f32x8 rr = *reinterpret_cast<const f32x8*>(rrow + (long)oy * a.ep.res.sY);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += rr[k];
    }
    if (has_msk) {
      const f32x8 mm = __builtin_convertvector(*reinterpret_cast<const bf16x8*>(mrow + (long)oy * a.mask_h.sY), f32x8);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = (mm[k] > 0.f) ? v[k] : 0.f;
    }
    float* o = orow + (long)oy * a.out.sY;
    if (accum) {
      const f32x8 old = *reinterpret_cast<const f32x8*>(o);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += old[k];
    }
    *reinterpret_cast<f32x8*>(o) = v;
  }
}

// one kernel per KS: the launch and the profile's name read the same entry
#define MH_K(KS, TAPG) {reinterpret_cast<const void*>(&igemm_bf16_mh_kernel<KS, TAPG>), "igemm_bf16_mh_kernel<" #KS ", " #TAPG ">", dg_bf16s_lds(KS, TAPG)}
static const DgKernel kMh[2] = {MH_K(1, 1), MH_K(3, 9)};
#undef MH_K
const DgKernel* dg_conv_bf16_mh_kernel(int KS) { return &kMh[KS == 3]; }

static bool al16f(const TView& v) { return !(v.sX % 4) && !(v.sY % 4) && !(v.sB % 4) && !(((uintptr_t)v.p) & 15); }

int dg_conv_bf16_mh(const ConvPlan& pl, const ConvArgs& a, TViewH mask_h, hipStream_t st) {
  if (!a.in.p || !a.out.p || !a.w || a.B < 1 || a.H < 1 || a.W < 1 || a.Cin < 1 || a.Cout < 1) {
    dg_set_error("dg_conv_bf16_mh: bad argument");
    return DG_ERR_ARG;
  }
  if (!dg_plan_bf16(pl) || (pl.KS != 3 && pl.KS != 1) || (a.Cout % 32) || (a.Cin % 4)) {
    dg_set_error("dg_conv_bf16_mh: needs a bf16 plan of a 3x3 or 1x1 convolution, Cin %% 4 == 0, Cout %% 32 == 0 (%d -> %d)",
                 a.Cin, a.Cout);
    return DG_ERR_UNSUPPORTED;
  }
  const Epilogue& e = a.ep;
  if (e.bias || e.scale || e.shift || e.film_mul || e.film_add || e.out_pre.p || e.mask.p || e.pool.p || e.relu ||
      e.head_out || a.groups > 1) {
    dg_set_error("dg_conv_bf16_mh: only res and accumulate of the epilogue are served");
    return DG_ERR_UNSUPPORTED;
  }
  if (a.cpt > 0 && (a.Cin % (a.cpt * 32))) { dg_set_error("dg_conv_bf16_mh: gathered K needs whole runs of chunks"); return DG_ERR_ARG; }
  bool al = al16f(a.in) && al16f(a.out) && (!e.res.p || al16f(e.res)) &&
            (!mask_h.p || (!(mask_h.sX % 8) && !(mask_h.sY % 8) && !(mask_h.sB % 8) && !(((uintptr_t)mask_h.p) & 15)));
  for (int t = 0; t < 4 && a.cpt > 0; ++t) al = al && !(a.in_run_off[t] % 4);
  if (!al) { dg_set_error("dg_conv_bf16_mh: every view must be 16-byte aligned"); return DG_ERR_ARG; }
  ConvArgsM m;
  static_cast<ConvArgs&>(m) = a;
  m.mask_h = mask_h;
  m.lgx = cdiv(a.W, 16) * cdiv(a.H, 16) * a.B;
  m.lgy = cdiv(a.Cout, 32);
  const long total = (long)m.lgx * m.lgy;
  if (total > 0x7FFFFFFFL) { dg_set_error("dg_conv_bf16_mh: %ld work items", total); return DG_ERR_UNSUPPORTED; }
  const DgKernel* k = dg_conv_bf16_mh_kernel(pl.KS);
  return dg_launch(*k, (unsigned)total, 256, (size_t)k->attr_lds, &m, st);
}
