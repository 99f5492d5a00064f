// Text of the bf16-storage implicit-GEMM kernel, included by igemm_bf16s.hip once per kernel: the including file defines
// IGEMM_BF16S_KERNEL (the kernel's name) and IGEMM_BF16S_HEAD (0 / 1: gen_segmentation fused into the epilogue).  Two
// kernels from one text, so that the plain one compiles exactly as it did before the fused head existed.
// igemm_bf16s_train.hip includes it a third time with IGEMM_BF16S_TRAIN = 1 and IGEMM_BF16S_ARGS = ConvArgsHT (ConvArgsH
// plus `u` and `fdec`): the FiLM layers of the generator update, which also store RNE_bf16 of the pre-FiLM tensor and
// the ReLU decision the epilogue took, one bit per element.  Both default to what the two kernels above are built with.
// The main loop is the same included text as igemm_bf16_kernel's (igemm_bf16_main.inc with the bf16 operand form).
#ifndef IGEMM_BF16S_TRAIN
#define IGEMM_BF16S_TRAIN 0
#define IGEMM_BF16S_ARGS ConvArgsH
#define IGEMM_BF16S_TRAIN_DEFAULTED
#endif
template <int KS, int TAPG>
__global__ __launch_bounds__(256, 2) void IGEMM_BF16S_KERNEL(const IGEMM_BF16S_ARGS a) {
  constexpr bool HEAD = IGEMM_BF16S_HEAD != 0;
  constexpr int NT = 32, MT = 2, CK = 32;
#define IGEMM_X_BF16 1
#include "igemm_bf16_main.inc"
#undef IGEMM_X_BF16

  // ---- epilogue ----
  // A lane owns 8 consecutive channels of one pixel = 16 bytes of bf16 (igemm_bf16_acc8.inc).  Per view one buffer
  // descriptor on a 64-bit base at pixel (oyw, tx0) of sample b, a per-lane 32-bit byte offset computed once and a scalar
  // byte offset per pass: offsets stay inside four image rows.
#include "igemm_bf16_acc8.inc"
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
