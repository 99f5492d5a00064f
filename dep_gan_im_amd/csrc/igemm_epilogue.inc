// Fused epilogue of the MFMA convolution kernels, included textually inside the kernel body (igemm_conv.hip,
// igemm_bf16.hip) so that both share ONE text and neither pays for a call boundary.  Expects in scope: MF, MT, NT, a,
// acc[MT], smem, tid, lane, wv, r, h, b, ty0, tx0, n0, out_goff; the transposed accumulator layout D[channel][pixel] of
// v_mfma_f32_32x32x2_f32 / _16x16x4_f32 / _32x32x16_bf16 with the WEIGHT fragment as first operand.
// Hooks (defaults = the workgroup-tile kernels; igemm_wp.hip overrides them for its wave-private items):
//   EPI_PRE_SYNC   statement before the tile region is reused for the transpose (default: __syncthreads())
//   EPI_ES_BASE    LDS float pointer of this wave's transpose scratch            (default: smem + wv * 64 * (NT + 4))
//   EPI_PHASED     defined: the scratch holds ONE 32-pixel MFMA tile; the tiles go through it one after the other
//   EPI_OYW        image row of the wave's 4 x 16 block                          (default: ty0 + 4 * wave)
//   EPI_FULL       the wave's whole block lies inside the image                  (default: the 16 x 16 tile does)
//   EPI_HEAD       constexpr bool: the instantiation carries the fused one-channel head (default: absent)
//   EPI_STAGE      statement replacing the accumulator -> scratch staging (igemm_wino.hip: done by the kernel itself)
//   EPI_STAGE_LATE statement run between the per-item setup (constant loads, descriptors) and the first pass
//   EPI_NPASS      passes of 8 pixels x 32 channels the wave's block takes (default 8 = 4 x 16 pixels)
//   EPI_FETCH(v, py, px)  statement producing the four channels c4 .. c4+3 of pixel (py, px) of the wave's 4 x 16 block
//                  in v (default: one 16-byte read of the transposed tile)
//   EPI_CLASS      a type with constexpr bool members fixed, bias, affine, film, relu, pre, res, msk, pool, head:
//                  fixed = true makes the epilogue's flags those compile-time constants (accumulate: false) instead of
//                  run-time tests on a.ep -- the launcher must then pass exactly that flag set (igemm_wino.hip);
//                  fixed = false, or the hook undefined (default): every flag is read from a.ep
#ifndef EPI_PRE_SYNC
#define EPI_PRE_SYNC __syncthreads()
#define EPI_PRE_SYNC_DEFAULTED
#endif
  // ---- epilogue ----
  // The CU retires only about one vector-memory wave-instruction per ~100 cycles here, so the
  // store tail is as long as the MFMA phase unless every instruction covers whole lines.  Each wave's 64 x NT tile
  // goes through LDS and is emitted as 16-byte accesses: 8 lanes x 16 B cover one pixel's 32 channels (one full
  // 128-B line).  (Storing the quads straight from the accumulators -- 32 lines of 32 bytes per instruction -- was
  // measured 3 % slower than this.)
  EPI_PRE_SYNC;  // every wave is done with its fragment reads; the tile region is free
  constexpr int CP = NT + 4;
#ifdef EPI_ES_BASE
  float* es = EPI_ES_BASE;
#else
  float* es = smem + wv * (64 * CP);
#endif
  // The MFMAs take the WEIGHT fragment as their first operand, so the accumulators hold the transposed tile
  // D[channel][pixel]: lane (r, h) owns pixel r of each pixel tile and its registers 4g .. 4g+3 are four consecutive
  // channels (8g + 4h + 0..3 of the 32x32 tile, 4h + 0..3 of the 16x16 one) -> one 16-byte LDS write per quad
  // (rows of CP = NT + 4 floats: 8 consecutive lanes hit 8 different 16-byte bank groups).
  constexpr int NQ = (MF == 32) ? 4 : 1, CSTEP = (MF == 32) ? 8 : 4;
#if defined(EPI_STAGE)
  EPI_STAGE;
  (void)es;
#elif !defined(EPI_PHASED)
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int g = 0; g < NQ; ++g) {
      f32x4 q4;
#pragma unroll
      for (int k = 0; k < 4; ++k) q4[k] = acc[mt][4 * g + k];
      *reinterpret_cast<f32x4*>(es + (MF * mt + r) * CP + CSTEP * g + 4 * h) = q4;
    }
#endif
  // On a SIMD nothing that is issued overlaps with fp32 MFMAs (DESIGN.md section 4), so the epilogue is written for
  // instruction count: every operand test is a scalar branch on a kernel argument, and every access is
  // (uniform 64-bit base in SGPRs) + (per-lane 32-bit byte offset computed once) so that the loads and stores take the
  // saddr form and the per-pass address arithmetic is a handful of scalar adds.
  constexpr int LPP = NT / 4;     // lanes per pixel
  constexpr int PPP = 64 / LPP;   // pixels per pass (8 for NT = 32: half a tile row; 16 for NT = 16: one row)
#ifdef EPI_NPASS
  constexpr int NPASS = EPI_NPASS;   // the wave's block has fewer rows than four (igemm_wino.hip, 8-row tiles: 2 x 16)
#else
  constexpr int NPASS = 64 / PPP;
#endif
  const int c4 = (lane % LPP) * 4, pl0 = lane / LPP;
  const int co = n0 + c4;
#ifndef EPI_OYW
  const int wvu = __builtin_amdgcn_readfirstlane(wv);
#endif
  const Epilogue& e = a.ep;
#ifdef EPI_CLASS
  // the launcher chose this instantiation for exactly this flag set (EPI_CLASS::fixed; otherwise the class is the
  // generic one and reads the flags as below): the tests on absent operands, their descriptors, lane offsets and strides
  // fold away at compile time.  The statements are the same text, so every class computes the generic kernel's bits
  typedef EPI_CLASS EpiC;
  constexpr bool EPI_CT = EpiC::fixed;
  const bool affine = EPI_CT ? EpiC::affine : (e.scale != nullptr), film = EPI_CT ? EpiC::film : (e.film_mul != nullptr),
             relu = EPI_CT ? EpiC::relu : (e.relu != 0), accum = EPI_CT ? false : (e.accumulate != 0);
  const bool has_bias = EPI_CT ? EpiC::bias : (e.bias != nullptr), has_pre = EPI_CT ? EpiC::pre : (e.out_pre.p != nullptr),
             has_res = EPI_CT ? EpiC::res : (e.res.p != nullptr), has_msk = EPI_CT ? EpiC::msk : (e.mask.p != nullptr),
             has_pool = EPI_CT ? EpiC::pool : (e.pool.p != nullptr);
#else
  const bool affine = e.scale != nullptr, film = e.film_mul != nullptr, relu = e.relu != 0, accum = e.accumulate != 0;
  const bool has_bias = e.bias != nullptr, has_pre = e.out_pre.p != nullptr, has_res = e.res.p != nullptr,
             has_msk = e.mask.p != nullptr, has_pool = e.pool.p != nullptr;
#endif
#ifdef EPI_OYW
  const int oyw = EPI_OYW;
#else
  const int oyw = ty0 + 4 * wvu;
#endif
#ifdef EPI_HEAD
  float hkeep_out = 0.f;
#endif
#ifdef EPI_FULL
  const bool full = EPI_FULL;
#else
  const bool full = (ty0 + 16 <= a.H) && (tx0 + 16 <= a.W);
#endif
  if (co < a.Cout) {
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f}, sc4 = {1.f, 1.f, 1.f, 1.f}, sh4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 fm4 = {1.f, 1.f, 1.f, 1.f}, fa4 = {0.f, 0.f, 0.f, 0.f};
    if (has_bias) bias4 = *reinterpret_cast<const f32x4*>(e.bias + co);
    if (affine) {
      sc4 = *reinterpret_cast<const f32x4*>(e.scale + co);
      sh4 = *reinterpret_cast<const f32x4*>(e.shift + co);
    }
    // (acc + bias) s + t as ONE fused multiply-add per value: the constant term bias s + t is formed once per item
    // (without the affine s = 1, t = 0 and the FMA is the plain bias add, exactly)
#pragma unroll
    for (int k = 0; k < 4; ++k) sh4[k] = fmaf(bias4[k], sc4[k], sh4[k]);
    if (film) {
      fm4 = *reinterpret_cast<const f32x4*>(e.film_mul + (long)b * e.film_ld + co);
      fa4 = *reinterpret_cast<const f32x4*>(e.film_add + (long)b * e.film_ld + co);
    }
    // Buffer addressing: per view one resource descriptor (SGPRs) at pixel (oyw, tx0) of sample b, a per-lane byte
    // offset computed once (pixel pl0 of the pass, channel co) and a scalar byte offset per pass -- the eight passes
    // issue no address arithmetic on the vector ALU at all.
    auto mk = [&](const float* p) {
      // the descriptor must be wave-uniform: the pointer depends on the wave index
      const unsigned long long u = (unsigned long long)p;
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
      return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, 0x7FFFFFFF, 0x00020000);
    };
    const int lo_out = 4 * (pl0 * (int)a.out.sX + co);
    const int lo_pre = has_pre ? 4 * (pl0 * (int)e.out_pre.sX + co) : 0;
    const int lo_res = has_res ? 4 * (pl0 * (int)e.res.sX + co) : 0;
    const int lo_msk = has_msk ? 4 * (pl0 * (int)e.mask.sX + co) : 0;
    const __amdgpu_buffer_rsrc_t r_out = mk(a.out.p + out_goff + view_off(a.out, b, oyw, tx0));
    const __amdgpu_buffer_rsrc_t r_pre = mk(has_pre ? e.out_pre.p + view_off(e.out_pre, b, oyw, tx0) : a.out.p);
    const __amdgpu_buffer_rsrc_t r_res = mk(has_res ? e.res.p + view_off(e.res, b, oyw, tx0) : a.out.p);
    const __amdgpu_buffer_rsrc_t r_msk = mk(has_msk ? e.mask.p + view_off(e.mask, b, oyw, tx0) : a.out.p);
    // fused 2x2 max-pool: the wave's 4 x 16 block holds whole pool windows (tile origins are multiples of 16); the
    // two rows of a window are two passes apart, its two columns 8 lanes (NT = 32) or 4 lanes (NT = 16) apart
    const __amdgpu_buffer_rsrc_t r_pool =
        mk(has_pool ? e.pool.p + view_off(e.pool, b, oyw >> 1, tx0 >> 1) : a.out.p);
    const int lo_pool = has_pool ? 4 * ((pl0 >> 1) * (int)e.pool.sX + co) : 0;
    const int sY_pool = 4 * (int)e.pool.sY, sX_pool = 4 * (int)e.pool.sX;
    f32x4 vrow = {0.f, 0.f, 0.f, 0.f};
#ifdef EPI_HEAD
    // fused 1x1 head to one channel: the 8 lanes of a pixel hold its 32 channels (4 each) -- a 4-FMA partial dot product,
    // an all-reduce over the 8 lanes in three DPP steps, and lane (pass index) of each pixel group keeps the sum of its
    // pass, so that after the eight passes every lane owns one pixel: ONE activation and ONE store per lane and item
#ifdef EPI_CLASS
    const bool has_head = EPI_HEAD && (EPI_CT ? EpiC::head : (e.head_out != nullptr));
#else
    const bool has_head = EPI_HEAD && e.head_out != nullptr;
#endif
    f32x4 hw4 = {0.f, 0.f, 0.f, 0.f};
    if (has_head) hw4 = *reinterpret_cast<const f32x4*>(e.head_w + co);
    const bool skip_out = has_head && e.head_skip_out != 0;
#else
    constexpr bool has_head = false, skip_out = false;
#endif
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    auto ld = [&](const __amdgpu_buffer_rsrc_t& r, int voff, int soff) {
      const i32x4 t = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
      return __builtin_bit_cast(f32x4, t);
    };
    auto st = [&](const __amdgpu_buffer_rsrc_t& r, int voff, int soff, f32x4 v) {
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, v), r, voff, soff, 0);
    };
    const int sY_out = 4 * (int)a.out.sY, sX_out = 4 * (int)a.out.sX;
    const int sY_pre = 4 * (int)e.out_pre.sY, sX_pre = 4 * (int)e.out_pre.sX;
    const int sY_res = 4 * (int)e.res.sY, sX_res = 4 * (int)e.res.sX;
    const int sY_msk = 4 * (int)e.mask.sY, sX_msk = 4 * (int)e.mask.sX;
#ifdef EPI_STAGE_LATE
    // the kernel's own staging, AFTER the loads of the per-item constants above have been issued: their global-memory
    // latency then runs under the staging's barriers instead of in front of the first pass
    EPI_STAGE_LATE;
#endif
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      // pass p covers pixels (py, px0 .. px0 + PPP) of the wave's 4 x 16 block; the passes walk the block so that
      // the two rows of a 2x2 pool window are consecutive passes (row pair, then the next column part)
      constexpr int RP = 16 / PPP;      // passes per pixel row
      const int py = (p & 1) + 2 * (p / (2 * RP)), px0 = ((p >> 1) % RP) * PPP;
      const bool ok = full || (oyw + py < a.H && tx0 + px0 + pl0 < a.W);
#if defined(EPI_FETCH)
      f32x4 v;
      EPI_FETCH(v, py, (px0 + pl0));
#elif defined(EPI_PHASED)
      // the scratch holds one 32-pixel MFMA tile (two rows of 16 pixels): tile p / (NPASS / MT) goes in when its first
      // pass comes up.  In-order LDS execution of the wave's own instructions is all the ordering this needs.
      static_assert(MF == 32, "phased epilogue: 32-pixel tiles");
      if (p % (NPASS / MT) == 0) {
        const int mtp = p / (NPASS / MT);   // a constant after unrolling
#pragma unroll
        for (int g = 0; g < NQ; ++g) {
          f32x4 q4;
#pragma unroll
          for (int k = 0; k < 4; ++k) q4[k] = acc[mtp][4 * g + k];
          *reinterpret_cast<f32x4*>(es + r * CP + CSTEP * g + 4 * h) = q4;
        }
      }
      f32x4 v = *reinterpret_cast<const f32x4*>(es + ((py & 1) * 16 + px0 + pl0) * CP + c4);
#else
      f32x4 v = *reinterpret_cast<const f32x4*>(es + (py * 16 + px0 + pl0) * CP + c4);
#endif
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = fmaf(v[k], sc4[k], sh4[k]);
      if (has_pre) {
        if (ok) st(r_pre, lo_pre, py * sY_pre + px0 * sX_pre, v);
      }
      if (film) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = film_preact(v[k], fm4[k], fa4[k]);
      }
      if (relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = dg_vmax(v[k], 0.f);
      }
      if (has_res) {
        f32x4 rr = {0.f, 0.f, 0.f, 0.f};
        if (ok) rr = ld(r_res, lo_res, py * sY_res + px0 * sX_res);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += rr[k];
      }
      if (has_msk) {
        f32x4 mm = {1.f, 1.f, 1.f, 1.f};
        if (ok) mm = ld(r_msk, lo_msk, py * sY_msk + px0 * sX_msk);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (mm[k] > 0.f) ? v[k] : 0.f;
      }
      const int so = py * sY_out + px0 * sX_out;
      if (accum) {
        f32x4 old = {0.f, 0.f, 0.f, 0.f};
        if (ok) old = ld(r_out, lo_out, so);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += old[k];
      }
      if (ok && !skip_out) st(r_out, lo_out, so, v);
#ifdef EPI_HEAD
      if (has_head) {
        static_assert(!EPI_HEAD || (NT == 32 && NPASS == 8), "fused head: 32-channel tiles, eight passes");
        float d = v[0] * hw4[0];
        d = fmaf(v[1], hw4[1], d);
        d = fmaf(v[2], hw4[2], d);
        d = fmaf(v[3], hw4[3], d);
#define EPI_DPP(x, ctrl) \
  __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (x)), (ctrl), 0xF, 0xF, false))
        d += EPI_DPP(d, 0xB1);    // quad_perm [1,0,3,2]: lane ^ 1
        d += EPI_DPP(d, 0x4E);    // quad_perm [2,3,0,1]: lane ^ 2
        d += EPI_DPP(d, 0x141);   // row_half_mirror: the other quad of the 8-lane group
#undef EPI_DPP
        hkeep_out = ((lane & 7) == p) ? d : hkeep_out;
      }
#endif
      if (has_pool) {
        if ((py & 1) == 0) {
          vrow = v;
        } else {
          f32x4 m;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float t = dg_vmax(vrow[k], v[k]);
            m[k] = dg_vmax(t, __shfl_xor(t, LPP, 64));
          }
          if (ok && (pl0 & 1) == 0) st(r_pool, lo_pool, (py >> 1) * sY_pool + (px0 >> 1) * sX_pool, m);
        }
      }
    }
  }
#ifdef EPI_HEAD
  if (EPI_HEAD && a.ep.head_out != nullptr && n0 < a.Cout) {
    const int ph = lane & 7, plh = lane >> 3;                       // this lane's pass and its pixel inside the pass
    const int pyh = (ph & 1) + 2 * (ph >> 2), pxh = ((ph >> 1) & 1) * 8 + plh;
    const int yh = oyw + pyh, xh = tx0 + pxh;
    if (yh < a.H && xh < a.W) {
      const float t = hkeep_out + a.ep.head_b[0];
      a.ep.head_out[((long)b * a.H + yh) * a.W + xh] = a.ep.head_tanh ? tanhf(t) : t;
    }
  }
#endif
#ifdef EPI_PRE_SYNC_DEFAULTED
#undef EPI_PRE_SYNC
#undef EPI_PRE_SYNC_DEFAULTED
#endif
