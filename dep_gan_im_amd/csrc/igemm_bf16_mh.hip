// Backward-data of the generator update on bf16 activation storage (bf16s_train.h): igemm_bf16_kernel's contraction --
// dy fp32 in HBM, rounded to bf16 (RNE) while the halo tile is committed, bf16 panels, fp32 accumulation, the same tile,
// LDS image, item order, gathered K and K order -- with an epilogue of its own whose ReLU mask operand is a bf16 view:
//   v = acc;  v += res;  v = (widen(mask) > 0) ? v : 0;  out = accumulate ? out + v : v
// in igemm_epilogue.inc's order (without bias and affine its fma(acc, 1, 0) is acc).  The shared epilogue text and the
// fp32 headline kernels that include it are not touched: this is a sibling kernel compiled only here.  The main loop
// below is igemm_bf16_kernel's, statement for statement.  Lane mapping of the epilogue as igemm_bf16s_kernel: 8
// consecutive channels of one pixel per lane (two 16-byte fp32 accesses, one 16-byte bf16 mask read), 4 lanes per pixel,
// one 16-pixel row of the wave's 4 x 16 block per pass.
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
  constexpr int PAD = KS / 2;
  constexpr int TW = 16 + KS - 1;
  constexpr int PIXT = TW * TW;
  constexpr int NTAPS = KS * KS;
  constexpr int NG = NTAPS / TAPG;
  constexpr int ROWB = 80;   // bytes per LDS row: 32 bf16 + 16 bytes of padding (conflict-free 16-byte reads of 16 rows)
  constexpr int XV = CK / 4;  // float4 pieces of one pixel's chunk in global memory
  constexpr int XTOT = PIXT * XV;
  constexpr int XPIECES = (XTOT + 255) / 256;
  constexpr int WV = CK / 8;  // 16-byte pieces (8 bf16) of one packed weight row
  constexpr int WTOT = TAPG * NT * WV;
  constexpr int WPIECES = (WTOT + 255) / 256;
  static_assert(NTAPS % TAPG == 0, "tap grouping");
  typedef f32x16 acc_t;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* xs = reinterpret_cast<char*>(smem);      // [PIXT][ROWB]
  char* ws = xs + PIXT * ROWB;                   // [TAPG][NT][ROWB]

  const int tid = threadIdx.x;
  const int tilesX = (a.W + 15) >> 4, tilesY = (a.H + 15) >> 4;
  // work item -> (pixel tile, channel tile): the XCD-aware order of igemm_conv.hip (each XCD walks a contiguous eighth
  // of the pixel tiles with the channel tile fastest)
  const unsigned nNTall = (unsigned)a.lgy, nPix = (unsigned)a.lgx;
  const unsigned id = blockIdx.x;
  int t, ntile;
  if ((nPix & 7u) == 0) {
    const unsigned x = id & 7u, sl = id >> 3;
    ntile = (int)(sl % nNTall);
    t = (int)(x * (nPix >> 3) + sl / nNTall);
  } else {
    t = (int)(id % nPix);
    ntile = (int)(id / nPix);
  }
  const int tx0 = (t % tilesX) * 16;
  t /= tilesX;
  const int ty0 = (t % tilesY) * 16;
  const int b = t / tilesY;
  const int ngrp = a.groups > 1 ? a.groups : 1;
  const int nNTg = (int)nNTall / ngrp;
  const int grp = ntile / nNTg;
  ntile -= grp * nNTg;
  const __bf16* wbase = reinterpret_cast<const __bf16*>(a.groups > 1 ? a.w_group[grp] : a.w);
  const long out_goff = a.groups > 1 ? a.out_group_off[grp] : 0;
  const int n0 = ntile * NT;
  const int nCC = (a.Cin + CK - 1) / CK;
  const int NS = nCC * NG;
  const float* inb = a.in.p + (long)b * a.in.sB;

  f32x4 xr[XPIECES];
  u32x4 wr[WPIECES];
  auto coff = [&](int cc) -> long {     // gathered K, see ConvArgs::cpt
    if (a.cpt > 0) {
      const int run = cc / a.cpt;
      return a.in_run_off[run] + (long)(cc - run * a.cpt) * CK;
    }
    return (long)cc * CK;
  };
  auto prefetch = [&](int s) {
    const int cc = s / NG, tg = s - cc * NG;
    if (tg == 0) {
#pragma unroll
      for (int i = 0; i < XPIECES; ++i) {
        const int q = tid + i * 256;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < XTOT) {
          const int pix = q / XV, part = q - pix * XV;
          const int ly = pix / TW, lx = pix - ly * TW;
          const int iy = ty0 + ly - PAD, ix = tx0 + lx - PAD;
          const int c = cc * CK + part * 4;
          if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && c < a.Cin)
            v = *reinterpret_cast<const f32x4*>(inb + (long)iy * a.in.sY + (long)ix * a.in.sX + coff(cc) + part * 4);
        }
        xr[i] = v;
      }
    }
    const __bf16* wsrc = wbase + ((size_t)((size_t)ntile * nCC + cc) * NTAPS + (size_t)tg * TAPG) * (NT * CK);
#pragma unroll
    for (int i = 0; i < WPIECES; ++i) {
      const int q = tid + i * 256;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (q < WTOT) v = *reinterpret_cast<const u32x4*>(wsrc + (size_t)q * 8);
      wr[i] = v;
    }
  };
  auto commit = [&](int s) {
    const int cc = s / NG, tg = s - cc * NG;
    (void)cc;
    if (tg == 0) {
#pragma unroll
      for (int i = 0; i < XPIECES; ++i) {
        const int q = tid + i * 256;
        if (q < XTOT) {
          const int pix = q / XV, part = q - pix * XV;
          // the activation operand becomes bf16 here: plain casts = v_cvt_pk_bf16_f32, round to nearest even
          const bf16x4 h4 = __builtin_convertvector(xr[i], bf16x4);
          *reinterpret_cast<u32x2*>(xs + pix * ROWB + part * 8) = __builtin_bit_cast(u32x2, h4);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < WPIECES; ++i) {
      const int q = tid + i * 256;
      if (q < WTOT) {
        const int row = q / WV, part = q - row * WV;
        *reinterpret_cast<u32x4*>(ws + row * ROWB + part * 16) = wr[i];
      }
    }
  };

  const int lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, h = lane >> 5;   // h: which 8 of the 16 k-values of an MFMA this lane carries
  int apix[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int py = 4 * wv + 2 * mt + (r >> 4), px = r & 15;
    apix[mt] = (py * TW + px) * ROWB + 16 * h;
  }
  const int boff = r * ROWB + 16 * h;

  acc_t acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[mt][j] = 0.f;

  prefetch(0);
  for (int s = 0; s < NS; ++s) {
    __syncthreads();
    commit(s);
    __syncthreads();
    if (s + 1 < NS) prefetch(s + 1);
    const int tg = s % NG;
#pragma unroll
    for (int tl = 0; tl < TAPG; ++tl) {
      const int tap = (TAPG == NTAPS) ? tl : (tg * TAPG + tl);
      const int ty = tap / KS, tx = tap - ty * KS;
      const int tapoff = (ty * TW + tx) * ROWB;
#pragma unroll
      for (int sub = 0; sub < CK / 16; ++sub) {
        const bf16x8 bw = *reinterpret_cast<const bf16x8*>(ws + tl * (NT * ROWB) + boff + 32 * sub);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const bf16x8 ax = *reinterpret_cast<const bf16x8*>(xs + apix[mt] + tapoff + 32 * sub);
          // weight fragment first: D[channel][pixel], the layout the shared epilogue expects
          acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw, ax, acc[mt], 0, 0, 0);
        }
      }
    }
  }
  __syncthreads();   // every wave is done with its fragment reads; the tile region is free
  constexpr int CP = NT + 4;
  float* es = smem + wv * (64 * CP);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 q4;
#pragma unroll
      for (int k = 0; k < 4; ++k) q4[k] = acc[mt][4 * g + k];
      *reinterpret_cast<f32x4*>(es + (32 * mt + r) * CP + 8 * g + 4 * h) = q4;
    }
  const int c8 = (lane & 3) * 8, pl0 = lane >> 2;
  const int co = n0 + c8;   // < Cout: Cout is a multiple of 32 (launcher)
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

template <int KS, int TAPG>
static int launch_mh(const ConvArgsM& a, hipStream_t st) {
  constexpr int TW = 16 + KS - 1;
  constexpr size_t lds_k = (size_t)(TW * TW + TAPG * 32) * 80;
  constexpr size_t lds_e = (size_t)4 * 64 * (32 + 4) * sizeof(float);
  constexpr size_t lds = lds_k > lds_e ? lds_k : lds_e;
  static DgOncePerDevice once;
  if (once.need()) {
    HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&igemm_bf16_mh_kernel<KS, TAPG>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  ConvArgsM b = a;
  b.lgx = cdiv(a.W, 16) * cdiv(a.H, 16) * a.B;
  b.lgy = cdiv(a.Cout, 32);
  const long total = (long)b.lgx * b.lgy;
  if (total > 0x7FFFFFFFL) { dg_set_error("dg_conv_bf16_mh: %ld work items", total); return DG_ERR_UNSUPPORTED; }
  hipLaunchKernelGGL((igemm_bf16_mh_kernel<KS, TAPG>), dim3((unsigned)total), dim3(256), lds, st, b);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

const char* dg_conv_bf16_mh_name(int KS) { return KS == 3 ? "igemm_bf16_mh_kernel<3, 9>" : "igemm_bf16_mh_kernel<1, 1>"; }

static bool al16f(const TView& v) { return !(v.sX % 4) && !(v.sY % 4) && !(v.sB % 4) && !(((uintptr_t)v.p) & 15); }

int dg_conv_bf16_mh(const ConvPlan& pl, const ConvArgs& a, TViewH mask_h, hipStream_t st) {
  if (!a.in.p || !a.out.p || !a.w || a.B < 1 || a.H < 1 || a.W < 1 || a.Cin < 1 || a.Cout < 1) {
    dg_set_error("dg_conv_bf16_mh: bad argument");
    return DG_ERR_ARG;
  }
  if (pl.bf16 != 1 || (pl.variant != 100 && pl.variant != 102) || (a.Cout % 32) || (a.Cin % 4)) {
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
  return pl.variant == 100 ? launch_mh<3, 9>(m, st) : launch_mh<1, 1>(m, st);
}
