// Which kernel a convolution takes and with what geometry: the one statement of the rule (common.h).  conv_launch
// (model.hip) and the operator entries launch by it, the profile's kernel name is the chosen entry's, and
// depgan_debug_conv_choice shows it to the tests.  dg_conv_prepare is host only: no launch, no allocation.
#include "common.h"

ConvPlan dg_conv_plan(int f32_split, int bf16_mfma, int winograd, int KS, int Cin, int Cout, int N, int H, int W) {
  if (f32_split) return dg_plan_conv_split(KS, Cin, Cout, f32_split == 6 ? 3 : 2);
  if (bf16_mfma) return dg_plan_conv_bf16(KS, Cin, Cout);
  // 3x3 layers the Winograd kernel covers (igemm_wino.hip: 4/9 of the MFMAs of the direct form)
  if (winograd && KS == 3 && H > 0 && W > 0 && !((H | W) & 1)) {
    const ConvPlan w = dg_plan_conv_wino(Cin, Cout);
    if (dg_plan_wino(w)) return w;
  }
  return dg_plan_conv_items(KS, Cin, Cout, (long)N * cdiv(H, 16) * cdiv(W, 16) * cdiv(Cout, 32));
}

// The epilogue class of a 5x5 launch (common.h, kConv5ClassMask): a pure function of the flag set and the switch.  The
// empty set is class 4, not the run-time-flag body, whose mask is only a placeholder
int dg_conv5_epi_class(unsigned flags) {
  if (!dg_get_epi_classes()) return 0;
  for (int i = 1; i < DG_CONV5_NCLASS; ++i)
    if (kConv5ClassMask[i] == flags) return i;
  return 0;
}

int dg_conv_prepare(const ConvPlan& pl, const ConvArgs& a, int KS, unsigned routes, DgConvLaunch* out) {
  out->grid_y = 1;
  out->klass = 0;
  if (!dg_plan_mfma(pl)) return dg_conv_direct_prepare(KS, a, out);
  DGCHECK(dg_conv_igemm_check(pl, a));
  if (dg_plan_bf16(pl) || dg_plan_split(pl)) return dg_conv_bf16_prepare(pl, a, out);
  if (dg_plan_wino(pl)) return dg_conv_wino_prepare(pl, a, out);   // its panel fits no other kernel
  const bool forced = !(routes & DG_ROUTE_TILE);
  if ((routes & DG_ROUTE_WP) && dg_conv_igemm_wp_supported(pl, a, forced)) return dg_conv_wp_prepare(pl, a, out);
  if ((routes & DG_ROUTE_WS5) && dg_conv_igemm_ws5_supported(pl, a, forced)) return dg_conv_ws5_prepare(pl, a, out);
  if (forced) {
    dg_set_error("dg_conv_prepare: the forced %s kernel does not cover this launch",
                 (routes & DG_ROUTE_WP) ? "wave-private 3x3" : "weight-stationary 5x5");
    return DG_ERR_UNSUPPORTED;
  }
  return dg_conv_tile_prepare(pl, a, out);
}

int dg_conv_run(const DgConvLaunch& L, hipStream_t st) {
  return dg_launch(*L.k, L.grid, L.block, L.lds, &L.a, st, L.grid_y);
}

int dg_conv_igemm(const ConvPlan& pl, const ConvArgs& a, hipStream_t st) {
  DgConvLaunch L;
  DGCHECK(dg_conv_prepare(pl, a, pl.KS, DG_ROUTE_ALL, &L));
  return dg_conv_run(L, st);
}
