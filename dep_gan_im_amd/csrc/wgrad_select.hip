// Which slab kernel a weight gradient takes, how many slabs and partial column-sum rows its launch writes: the one
// statement of the rule (common.h).  wgrad_run (model.hip) launches by it, the operator entries and depgan_create size
// their workspaces from it, depgan_debug_wgrad_choice shows it to the tests.  Host only: no HIP call, no allocation.
#include "bf16s_train.h"

int dg_wgrad_plan_of(int kernel, int KS, int B, int H, int W, int Cin, int Cout, int out[4]) {
  switch (kernel) {
    case DG_WG_F32: return dg_wgrad_plan(KS, B, H, W, Cin, Cout, out);
    case DG_WG_EDGE: return dg_wgrad_small_plan(KS, B, H, W, Cin, Cout, out);
    case DG_WG_BF16: return dg_wgrad_bf16_plan(KS, B, H, W, Cin, Cout, out);
    case DG_WG_BF16S: return dg_wgrad_bf16s_plan(KS, B, H, W, Cin, Cout, out);
  }
  dg_set_error("dg_wgrad_plan_of: %d is not a slab kernel", kernel);
  return DG_ERR_ARG;
}

int dg_wgrad_choose(int KS, int B, int H, int W, int Cin, int Cout, bool bf16_pipe, bool x_bf16, DgWgradChoice* out) {
  const bool mfma = Cin % 4 == 0 && Cout % 4 == 0 && Cin >= 8;
  int kernel = mfma ? DG_WG_F32 : DG_WG_EDGE;
  if (x_bf16) {
    // the storage types are not mixed: no fp32 kernel reads a bf16 operand
    if (!dg_wgrad_bf16s_supported(KS, Cin, Cout)) {
      dg_set_error("no bf16-staged weight gradient for k%d %d -> %d", KS, Cin, Cout);
      return DG_ERR_UNSUPPORTED;
    }
    kernel = DG_WG_BF16S;
  } else if (bf16_pipe && mfma && dg_wgrad_bf16_supported(KS, Cin, Cout)) {
    kernel = DG_WG_BF16;
  }
  int plan[4];
  DGCHECK(dg_wgrad_plan_of(kernel, KS, B, H, W, Cin, Cout, plan));
  out->kernel = kernel;
  out->nchunks = plan[2];
  out->part_floats = (size_t)plan[2] * KS * KS * Cin * Cout;
  out->col_rows = kernel == DG_WG_EDGE ? 0 : plan[2];
  return DG_OK;
}
