// Text of the bf16-storage implicit-GEMM kernel, included by igemm_bf16s.hip once per kernel: the including file defines
// IGEMM_BF16S_KERNEL (the kernel's name) and IGEMM_BF16S_HEAD (0 / 1: gen_segmentation fused into the epilogue).  Two
// kernels from one text, so that the plain one compiles exactly as it did before the fused head existed.
// igemm_bf16s_train.hip includes it a third time with IGEMM_BF16S_TRAIN = 1 and IGEMM_BF16S_ARGS = ConvArgsHT (ConvArgsH
// plus `u` and `fdec`): the FiLM layers of the generator update, which also store RNE_bf16 of the pre-FiLM tensor and
// the ReLU decision the epilogue took, one bit per element.  Both default to what the two kernels above are built with.
#ifndef IGEMM_BF16S_TRAIN
#define IGEMM_BF16S_TRAIN 0
#define IGEMM_BF16S_ARGS ConvArgsH
#define IGEMM_BF16S_TRAIN_DEFAULTED
#endif
template <int KS, int TAPG>
__global__ __launch_bounds__(256, 2) void IGEMM_BF16S_KERNEL(const IGEMM_BF16S_ARGS a) {
  constexpr bool HEAD = IGEMM_BF16S_HEAD != 0;
  constexpr int NT = 32, MT = 2, CK = 32;
  constexpr int PAD = KS / 2;
  constexpr int TW = 16 + KS - 1;
  constexpr int PIXT = TW * TW;
  constexpr int NTAPS = KS * KS;
  constexpr int NG = NTAPS / TAPG;
  constexpr int ROWB = 80;   // bytes per LDS row: 32 bf16 + 16 bytes of padding, as igemm_bf16_kernel
  constexpr int XV = CK / 8;  // 16-byte pieces (8 bf16) of one pixel's chunk in global memory
  constexpr int XTOT = PIXT * XV;
  constexpr int XPIECES = (XTOT + 255) / 256;
  constexpr int WV = CK / 8;  // 16-byte pieces of one packed weight row
  constexpr int WTOT = TAPG * NT * WV;
  constexpr int WPIECES = (WTOT + 255) / 256;
  static_assert(NTAPS % TAPG == 0, "tap grouping");
  typedef f32x16 acc_t;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* xs = reinterpret_cast<char*>(smem);      // [PIXT][ROWB]
  char* ws = xs + PIXT * ROWB;                   // [TAPG][NT][ROWB]

  const int tid = threadIdx.x;
  const int tilesX = (a.W + 15) >> 4, tilesY = (a.H + 15) >> 4;
  // work item -> (pixel tile, channel tile): the XCD-aware order of igemm_conv.hip
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
  const __bf16* inb = a.in.p + (long)b * a.in.sB;

  u32x4 xr[XPIECES];
  u32x4 wr[WPIECES];
  auto prefetch = [&](int s) {
    const int cc = s / NG, tg = s - cc * NG;
    if (tg == 0) {
#pragma unroll
      for (int i = 0; i < XPIECES; ++i) {
        const int q = tid + i * 256;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (q < XTOT) {
          const int pix = q / XV, part = q - pix * XV;
          const int ly = pix / TW, lx = pix - ly * TW;
          const int iy = ty0 + ly - PAD, ix = tx0 + lx - PAD;
          const int c = cc * CK + part * 8;
          // Cin is a multiple of 8 (launcher): a piece is inside the channels or outside, never across the end
          if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && c < a.Cin)
            v = *reinterpret_cast<const u32x4*>(inb + (long)iy * a.in.sY + (long)ix * a.in.sX + c);
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
    const int tg = s % NG;
    if (tg == 0) {
#pragma unroll
      for (int i = 0; i < XPIECES; ++i) {
        const int q = tid + i * 256;
        if (q < XTOT) {
          const int pix = q / XV, part = q - pix * XV;
          *reinterpret_cast<u32x4*>(xs + pix * ROWB + part * 16) = xr[i];   // a copy: the operand is bf16 already
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
          // weight fragment first: D[channel][pixel]
          acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw, ax, acc[mt], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue ----
  // As igemm_epilogue.inc: each wave's 64 x 32 tile goes through LDS (rows of NT + 4 floats) so that a lane owns
  // consecutive channels of one pixel; here 8 of them = 16 bytes of bf16, 4 lanes per pixel, 16 pixels (one row of the
  // wave's 4 x 16 block) per pass.  Per view one buffer descriptor on a 64-bit base at pixel (oyw, tx0) of sample b, a
  // per-lane 32-bit byte offset computed once and a scalar byte offset per pass: offsets stay inside four image rows.
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
  const int wvu = __builtin_amdgcn_readfirstlane(wv);
  const EpilogueH& e = a.ep;
  const bool affine = e.scale != nullptr, film = e.film_mul != nullptr, relu = e.relu != 0;
  const bool has_bias = e.bias != nullptr, has_res = e.res.p != nullptr, has_pool = e.pool.p != nullptr;
  const int oyw = ty0 + 4 * wvu;
  const bool full = (ty0 + 16 <= a.H) && (tx0 + 16 <= a.W);

  f32x8 sc8, sh8, fm8, fa8;
#pragma unroll
  for (int k = 0; k < 8; ++k) { sc8[k] = 1.f; sh8[k] = 0.f; fm8[k] = 1.f; fa8[k] = 0.f; }
  if (affine) {
    sc8 = *reinterpret_cast<const f32x8*>(e.scale + co);
    sh8 = *reinterpret_cast<const f32x8*>(e.shift + co);
  }
  if (has_bias) {
    const f32x8 bias8 = *reinterpret_cast<const f32x8*>(e.bias + co);
    // (acc + bias) s + t as ONE fused multiply-add per value; the constant bias s + t is formed once per item
#pragma unroll
    for (int k = 0; k < 8; ++k) sh8[k] = fmaf(bias8[k], sc8[k], sh8[k]);
  }
  if (film) {
    fm8 = *reinterpret_cast<const f32x8*>(e.film_mul + (long)b * e.film_ld + co);
    fa8 = *reinterpret_cast<const f32x8*>(e.film_add + (long)b * e.film_ld + co);
  }
  auto voff = [&](const TViewH& v, int y, int x) { return (long)b * v.sB + (long)y * v.sY + (long)x * v.sX; };
  auto mk = [&](const __bf16* p) {
    // the descriptor must be wave-uniform: the pointer depends on the wave index
    const unsigned long long u = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, 0x7FFFFFFF, 0x00020000);
  };
  const int lo_out = 2 * (pl0 * (int)a.out.sX + co);
  const int lo_res = has_res ? 2 * (pl0 * (int)e.res.sX + co) : 0;
  const int lo_pool = has_pool ? 2 * ((pl0 >> 1) * (int)e.pool.sX + co) : 0;
  const __amdgpu_buffer_rsrc_t r_out = mk(a.out.p + out_goff + voff(a.out, oyw, tx0));
  const __amdgpu_buffer_rsrc_t r_res = mk(has_res ? e.res.p + voff(e.res, oyw, tx0) : a.out.p);
  const __amdgpu_buffer_rsrc_t r_pool = mk(has_pool ? e.pool.p + voff(e.pool, oyw >> 1, tx0 >> 1) : a.out.p);
  const int sY_out = 2 * (int)a.out.sY, sY_res = 2 * (int)e.res.sY, sY_pool = 2 * (int)e.pool.sY;
  f32x8 vrow;
#pragma unroll
  for (int k = 0; k < 8; ++k) vrow[k] = 0.f;
  // HEAD (launcher: Cout == 32, ungrouped, so co = c8 and the 4 lanes of a pixel hold all its channels)
  f32x8 hw8;
#pragma unroll
  for (int k = 0; k < 8; ++k) hw8[k] = 0.f;
  float* hrow = nullptr;
  bool skip_out = false;
  if (HEAD) {
    hw8 = *reinterpret_cast<const f32x8*>(e.head_w + co);
    hrow = e.head_out + ((long)b * a.H + oyw) * a.W + tx0 + pl0;
    skip_out = e.head_skip_out != 0;
  }
#if IGEMM_BF16S_TRAIN
  // TRAIN (launcher: FiLM present): the pre-FiLM tensor as bf16 and the decision bits, dense [B][H][W][Cout / 8] bytes
  const int lo_u = 2 * (pl0 * (int)a.u.sX + co);
  const __amdgpu_buffer_rsrc_t r_u = mk(a.u.p + voff(a.u, oyw, tx0));
  const int sY_u = 2 * (int)a.u.sY;
  unsigned* drow = reinterpret_cast<unsigned*>(a.fdec + (((long)b * a.H + oyw) * a.W + tx0 + pl0) * (a.Cout >> 3) + (n0 >> 3));
#endif
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    // pass p = row p of the wave's 4 x 16 block: the two rows of a 2x2 pool window are consecutive passes, its two
    // columns 4 lanes apart
    const bool ok = full || (oyw + p < a.H && tx0 + pl0 < a.W);
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(es + (p * 16 + pl0) * CP + c8);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(es + (p * 16 + pl0) * CP + c8 + 4);
    f32x8 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = v0[k]; v[4 + k] = v1[k]; }
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = fmaf(v[k], sc8[k], sh8[k]);
#if IGEMM_BF16S_TRAIN
    if (ok) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, __builtin_convertvector(v, bf16x8)), r_u, lo_u, p * sY_u, 0);
#endif
    if (film) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = film_preact(v[k], fm8[k], fa8[k]);
    }
#if IGEMM_BF16S_TRAIN
    {
      // the decision of the ReLU below, taken on the very value it clamps: bit k of this lane's byte = (v[k] > 0); the 4
      // lanes of a pixel hold its 32 channels = one 32-bit word, gathered by two shuffles and stored by lane 0 of the four
      unsigned m = 0u;
#pragma unroll
      for (int k = 0; k < 8; ++k) m |= (v[k] > 0.f ? 1u : 0u) << k;
      m <<= 8 * (lane & 3);
      m |= __shfl_xor(m, 1, 64);
      m |= __shfl_xor(m, 2, 64);
      if (ok && (lane & 3) == 0) drow[(long)p * a.W * (a.Cout >> 5)] = m;
    }
#endif
    if (relu) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = dg_vmax(v[k], 0.f);
    }
    if (has_res) {
      i32x4 rr = {0, 0, 0, 0};
      if (ok) rr = __builtin_amdgcn_raw_buffer_load_b128(r_res, lo_res, p * sY_res, 0);
      const f32x8 rf = __builtin_convertvector(__builtin_bit_cast(bf16x8, rr), f32x8);   // widening: exact
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += rf[k];
    }
    // the one rounding of the storage contract: fp32 -> bf16, round to nearest even (v_cvt_pk_bf16_f32)
    const bf16x8 o = __builtin_convertvector(v, bf16x8);
    if (ok && !(HEAD && skip_out))
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, o), r_out, lo_out, p * sY_out, 0);
    if (HEAD) {
      // head_bf16s_kernel's arithmetic on the STORED values: per lane a0 w0, then fma over channels 1..7; the lanes of
      // a pixel are summed xor 2, xor 1; + b[0]; tanh.  Every lane takes part in the shuffles.
      const f32x8 sv = __builtin_convertvector(o, f32x8);
      float hv = sv[0] * hw8[0];
#pragma unroll
      for (int k = 1; k < 8; ++k) hv = fmaf(sv[k], hw8[k], hv);
      hv += __shfl_xor(hv, 2, 64);
      hv += __shfl_xor(hv, 1, 64);
      if (ok && (lane & 3) == 0) {
        hv += e.head_b[0];
        hrow[(long)p * a.W] = e.head_tanh ? tanhf(hv) : hv;
      }
    }
    if (has_pool) {
      const f32x8 sv = __builtin_convertvector(o, f32x8);   // the STORED values
      if ((p & 1) == 0) {
        vrow = sv;
      } else {
        f32x8 m;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float t2 = dg_vmax(vrow[k], sv[k]);
          m[k] = dg_vmax(t2, __shfl_xor(t2, 4, 64));
        }
        const bf16x8 mo = __builtin_convertvector(m, bf16x8);   // exact: m is one of the stored values
        if (ok && (pl0 & 1) == 0)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, mo), r_pool, lo_pool, (p >> 1) * sY_pool, 0);
      }
    }
  }
}
#ifdef IGEMM_BF16S_TRAIN_DEFAULTED
#undef IGEMM_BF16S_TRAIN
#undef IGEMM_BF16S_ARGS
#undef IGEMM_BF16S_TRAIN_DEFAULTED
#endif
