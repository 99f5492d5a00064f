// Main loop of the bf16 MFMA implicit-GEMM kernels, from the tile constants to the end of the contraction: the ONE text
// of igemm_bf16_kernel (igemm_bf16.hip), igemm_bf16_mh_kernel (igemm_bf16_mh.hip) and the three kernels of
// igemm_bf16s_kernel.inc.  Included inside the kernel body after `constexpr int NT = 32, MT = 2, CK = 32;` with the
// argument struct `a`; leaves acc[MT] (D[channel][pixel]) and tid, lane, wv, r, h, tx0, ty0, b, n0, out_goff and smem
// to the epilogue that follows.  Shared by inclusion, not by a function: DESIGN.md section 4.
// One hook, the form of the activation operand in HBM:
//   IGEMM_X_BF16 = 0: fp32 (TView), rounded to bf16 (RNE) while the halo tile is committed, K gathered by ConvArgs::cpt
//   IGEMM_X_BF16 = 1: bf16 (TViewH), copied; Cin is a multiple of 8 (launcher); no gathered K
// and one for the MFMA shape (not defined = 32):
//   IGEMM_MF = 32: v_mfma_f32_32x32x16_bf16, 32 channels x 32 pixels (two image rows of the tile), two per 32-channel chunk
//   IGEMM_MF = 16: v_mfma_f32_16x16x32_bf16, 16 channels x 16 pixels (one image row), one per chunk; included after
//                  `constexpr int NT = 16, MT = 4, CK = 32;` (igemm_bf16_n16_kernel, the critics' 16-channel 5x5 layers)
#ifndef IGEMM_MF
#define IGEMM_MF 32
#define IGEMM_MF_DEFAULTED
#endif
  constexpr int PAD = KS / 2;
  constexpr int TW = 16 + KS - 1;
  constexpr int PIXT = TW * TW;
  constexpr int NTAPS = KS * KS;
  constexpr int NG = NTAPS / TAPG;
  constexpr int ROWB = 80;   // bytes per LDS row: 32 bf16 + 16 bytes of padding (conflict-free 16-byte reads of 16 rows)
#if IGEMM_X_BF16
  constexpr int XV = CK / 8;  // 16-byte pieces (8 bf16) of one pixel's chunk in global memory
#else
  constexpr int XV = CK / 4;  // float4 pieces of one pixel's chunk in global memory
#endif
  constexpr int XTOT = PIXT * XV;
  constexpr int XPIECES = (XTOT + 255) / 256;
  constexpr int WV = CK / 8;  // 16-byte pieces (8 bf16) of one packed weight row
  constexpr int WTOT = TAPG * NT * WV;
  constexpr int WPIECES = (WTOT + 255) / 256;
  static_assert(NTAPS % TAPG == 0, "tap grouping");
#if IGEMM_MF == 16
  typedef f32x4 acc_t;
  constexpr int NACC = 4, KM = 32;   // accumulator registers, K of one MFMA
#else
  typedef f32x16 acc_t;
  constexpr int NACC = 16, KM = 16;
#endif

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
#if IGEMM_X_BF16
  const __bf16* inb = a.in.p + (long)b * a.in.sB;

  u32x4 xr[XPIECES];
#else
  const float* inb = a.in.p + (long)b * a.in.sB;

  f32x4 xr[XPIECES];
#endif
  u32x4 wr[WPIECES];
#if !IGEMM_X_BF16
  auto coff = [&](int cc) -> long {     // gathered K, see ConvArgs::cpt
    if (a.cpt > 0) {
      const int run = cc / a.cpt;
      return a.in_run_off[run] + (long)(cc - run * a.cpt) * CK;
    }
    return (long)cc * CK;
  };
#endif
  auto prefetch = [&](int s) {
    const int cc = s / NG, tg = s - cc * NG;
    if (tg == 0) {
#pragma unroll
      for (int i = 0; i < XPIECES; ++i) {
        const int q = tid + i * 256;
#if IGEMM_X_BF16
        u32x4 v = {0u, 0u, 0u, 0u};
#else
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#endif
        if (q < XTOT) {
          const int pix = q / XV, part = q - pix * XV;
          const int ly = pix / TW, lx = pix - ly * TW;
          const int iy = ty0 + ly - PAD, ix = tx0 + lx - PAD;
#if IGEMM_X_BF16
          const int c = cc * CK + part * 8;
          // Cin is a multiple of 8 (launcher): a piece is inside the channels or outside, never across the end
          if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && c < a.Cin)
            v = *reinterpret_cast<const u32x4*>(inb + (long)iy * a.in.sY + (long)ix * a.in.sX + c);
#else
          const int c = cc * CK + part * 4;
          if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && c < a.Cin)
            v = *reinterpret_cast<const f32x4*>(inb + (long)iy * a.in.sY + (long)ix * a.in.sX + coff(cc) + part * 4);
#endif
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
#if IGEMM_X_BF16
    const int tg = s % NG;
#else
    const int cc = s / NG, tg = s - cc * NG;
    (void)cc;
#endif
    if (tg == 0) {
#pragma unroll
      for (int i = 0; i < XPIECES; ++i) {
        const int q = tid + i * 256;
        if (q < XTOT) {
          const int pix = q / XV, part = q - pix * XV;
#if IGEMM_X_BF16
          *reinterpret_cast<u32x4*>(xs + pix * ROWB + part * 16) = xr[i];   // a copy: the operand is bf16 already
#else
          // the activation operand becomes bf16 here: plain casts = v_cvt_pk_bf16_f32, round to nearest even
          const bf16x4 h4 = __builtin_convertvector(xr[i], bf16x4);
          *reinterpret_cast<u32x2*>(xs + pix * ROWB + part * 8) = __builtin_bit_cast(u32x2, h4);
#endif
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
#if IGEMM_MF == 16
  const int r = lane & 15, h = lane >> 4;   // h: which 8 of the 32 k-values of an MFMA this lane carries
#else
  const int r = lane & 31, h = lane >> 5;   // h: which 8 of the 16 k-values of an MFMA this lane carries
#endif
  int apix[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#if IGEMM_MF == 16
    const int py = 4 * wv + mt, px = r;
#else
    const int py = 4 * wv + 2 * mt + (r >> 4), px = r & 15;
#endif
    apix[mt] = (py * TW + px) * ROWB + 16 * h;
  }
  const int boff = r * ROWB + 16 * h;

  acc_t acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NACC; ++j) acc[mt][j] = 0.f;

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
      for (int sub = 0; sub < CK / KM; ++sub) {
        const bf16x8 bw = *reinterpret_cast<const bf16x8*>(ws + tl * (NT * ROWB) + boff + 2 * KM * sub);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const bf16x8 ax = *reinterpret_cast<const bf16x8*>(xs + apix[mt] + tapoff + 2 * KM * sub);
          // weight fragment first: D[channel][pixel], the layout the shared epilogue expects
#if IGEMM_MF == 16
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw, ax, acc[mt], 0, 0, 0);
#else
          acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw, ax, acc[mt], 0, 0, 0);
#endif
        }
      }
    }
  }
#ifdef IGEMM_MF_DEFAULTED
#undef IGEMM_MF
#undef IGEMM_MF_DEFAULTED
#endif
