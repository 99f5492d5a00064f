// 3x3 NHWC fp32 implicit-GEMM convolution with WAVE-PRIVATE work items: no workgroup barrier in steady state.
//
// Why: in igemm_conv_kernel the four waves of a workgroup meet at two barriers
// per K chunk, and counters put the matrix pipe idle 23 % of the 32->32@256x256 launch although 3-4 waves are resident
// per SIMD -- an fp32 MFMA stream is served oldest-first and never pre-empted, so a younger workgroup's staging only
// advances in the older one's stalls and every barrier re-exposes its latencies.  Here a wave never waits for another:
//   * the WHOLE-K weight panel of the workgroup's channel tile (9 x Cin x 32 floats: 36 KB at Cin = 32, 72 KB at 64)
//     is loaded into LDS once per persistent workgroup -- the only __syncthreads of the kernel follows it;
//   * every wave owns its work items (a 4 x 16 pixel block x 32 output channels), stages its own 6 x 18 halo rows
//     into a wave-private LDS region chunk by chunk (8 input channels) and reads its fragments from there;
//     ordering between its own LDS writes and reads is the LDS unit's in-order execution -- s_waitcnt only;
//   * 16 waves per workgroup (one workgroup per CU, four waves per SIMD) share the panel.
// Same K order as igemm_conv_kernel<32,3,8,9> (chunk -> tap -> 4 MFMAs), same packed panel, same fused epilogue text:
// results are bit-identical to that kernel.  Covers Cin in {8..64, multiple of 8}, Cout multiple of 32, no groups /
// gathered K; the launcher falls back to igemm_conv_kernel for everything else.
//
// MEASURED (round 3, profiles/r03_conv_experiments.md): bit-identical on every test shape, and NEUTRAL -- -2.1 % ...
// +2.3 % against the workgroup-tile kernel on the five shapes of the step it covers (32->32@256^2 batch 32: 356 vs
// 360 us, 0.69 of the fp32 matrix peak either way).  Removing every barrier did not move the time; its ablations say
// why: without the epilogue 313 us, without the staging of chunks 1..3 335 us, without both 298 us (0.82) -- the
// non-MFMA instructions of a wave (fragment reads, staging, epilogue) ADD to the MFMA time of its SIMD whether or not
// another wave could run meanwhile, exactly as the micro-benchmarks of round 1 said (an fp32 MFMA stream is the vector
// ALU: nothing issued overlaps with it).  The kernel therefore stays OPT-IN (DEPGAN_IGEMM_WP=1); the default path is the
// workgroup-tile kernel.
//
// The same body, templated on (MF, KS, CK), is the WEIGHT-STATIONARY 5x5 kernel igemm_ws5_kernel<MF, CK> for the critics'
// 5x5 layers (Cin, Cout in {16, 32}: one channel tile, so the packed panel is the same for every item of a launch and
// igemm_conv_kernel<., 5, ., 25> re-stages it per item).  Per persistent workgroup the whole panel (25 x Cin x Cout
// floats: 25.6 / 51.2 / 102.4 KB) goes into LDS once, unpadded, 16-byte slots XOR-swizzled so that the B-fragment reads
// are conflict-free; a wave's item is a 4 x 16 pixel block x all channels (MF = 16: four v_mfma_f32_16x16x4_f32 tiles;
// MF = 32: two 32x32x2 tiles), its 8 x 20 halo chunk staged through registers into an unpadded wave-private region (5 KB
// at CK = 8, 10 KB at CK = 16, the latter swizzled conflict-free).  As many waves as 160 KB admit beside the panel, 12 at
// the most: 12 / 12 / 11 / 12 for 16->16 / 16->32 / 32->16 / 32->32 (32->16 cannot reach three waves on every SIMD at the
// plan's 16-channel chunks: 51.2 KB + 12 x 10 KB > 160 KB).  Same panel (the 5x5 tile plans of dg_plan_conv), same K order,
// the plan's chunk width for all four pairs, same epilogue text: bit-identical to the tile kernel
// (tests/test_gpu_conv5_ws.py).  -Rpass-analysis=kernel-resource-usage: <32, 8> 124 VGPRs, <16, 16> 162 VGPRs, no scratch
// (the 3x3 instantiation: 114, none).
// MEASURED (profiles/ws5_experiments.md; tools/ab_ws5.py, against the tile kernel in one process): 16->16 @256^2 -8.5 % at
// batch 96 (0.707 -> 0.773 of the fp32 matrix peak), -4.4 % at batch 32; 32->32 @128^2 -7.6 % at batch 96 (0.787 -> 0.852),
// +5.4 % at batch 32 (2.7 items per wave slot); 16->32 @128^2 -9.3 % / -5.0 % with 16 waves (12 waves: -9.1 % / +5.1 %);
// 32->16 +3 ... +5 % at both batches.  Default where it is faster (dg_conv_igemm_ws5_supported), the tile kernel
// elsewhere.  Canonical step: 49.83 -> 49.16 ms forced on for all eight launches, 49.66 -> 48.74 ms with that default
// (medians of five alternating runs; every run with it faster than every run without).
// EPILOGUE CLASSES (profiles/conv5_classes_experiments.md): igemm_ws5_kernel holds five item loops, selected once per wave by
// ConvArgs::epi_class (dg_conv5_epi_class: {bias, relu}, {bias, relu, pool}, {mask}, {} -- the flag sets of the critics'
// layers; 0 = the loop that reads the flags at run time, which is the parent's and keeps its registers and its speed).
// A class loop carries its flag set as constants (EPI_CLASS of igemm_epilogue.inc): no test, descriptor, lane offset or
// stride of an absent operand, and none of the 65 / 105 SGPRs the run-time loop spills.  Same statements, same loads:
// bit-identical (tests/test_gpu_conv5_classes.py).  The kernel's name, grid, block and LDS size do not depend on the class.
// Counters, 16->16 @256^2 batch 96, per wave (32 items): SALU 4474 -> 2833, VALU without MFMAs 11492 -> 7897, wave
// cycles -3.9 %; the eight launches -1.7 ... -5.1 %.
#include <stdlib.h>

#include "common.h"
#include "epilogue.h"

namespace {

constexpr int WP_NW = 16;                   // waves per workgroup of the 3x3 form

// One text for the 3x3 form (MF = 32, CK = 8) and the weight-stationary 5x5 forms (MF = 32 / CK = 8, MF = 16 / CK = 16).
// The 3x3 halo keeps its padded 48-byte pixel rows; the 5x5 halos are unpadded (8 x 20 pixels x CK floats: 5 KB / 10 KB
// per wave -- padded rows would cost the third wave per SIMD).
template <int MF, int KS, int CK>
struct WpGeo {
  static constexpr int NT = MF, MT = 64 / MF, PAD = KS / 2, NTAPS = KS * KS;
  static constexpr int TWX = 16 + KS - 1, TWY = 4 + KS - 1;   // halo of a 4 x 16 block
  static constexpr int PIX = TWX * TWY;
  static constexpr int XV = CK / 4;                           // 16-byte pieces per halo pixel
  static constexpr int CKP = (KS == 3) ? CK + 4 : CK;         // floats per halo pixel row
  static constexpr int EPI_FLOATS = (MF == 32 ? 32 : 64) * (NT + 4);   // transpose scratch of the epilogue
  static constexpr int WAVE_FLOATS = PIX * CKP > EPI_FLOATS ? PIX * CKP : EPI_FLOATS;
  static constexpr int SLOTS = PIX * XV;
  static constexpr int PIECES = (SLOTS + 63) / 64;            // per lane; the last one may be partial
  // 16-byte slot swizzles (slot ^= f): within each 16-lane group of a ds_read_b128 every lane must hit another slot
  // of the 256-byte bank row.
  //   panel, 32-byte rows (MF = 32): f = bit 4 of the row for 5x5 (conflict-free); the 3x3 form keeps the bit-2 swizzle
  //     it was measured with.
  //   panel, 64-byte rows (MF = 16): f = {0, 2, 3, 1}[row >> 2] (conflict-free).
  //   halo, 64-byte rows (MF = 16): f = 2 * bit 2 of the pixel index (conflict-free at every tap offset).
  //   halo, 32-byte rows (MF = 32, 5x5): none -- rows 20 pixels apart admit no conflict-free one-bit swizzle; 2-way, as
  //     the padded rows of the tile kernel are, and the LDS is not what limits this form (3 reads per 8 MFMAs).
  static __device__ __forceinline__ int panel_sw(int n) {
    if (MF == 32) return (n >> (KS == 3 ? 2 : 4)) & 1;
    return (0x78 >> (2 * (n >> 2))) & 3;
  }
  static __device__ __forceinline__ int halo_off(int pix, int part) {   // float offset of piece `part` of halo pixel `pix`
    if (CK == 16) return pix * CKP + 4 * (part ^ (((pix >> 2) & 1) << 1));
    return pix * CKP + 4 * part;
  }
};

template <int MF> struct WpMfma;
template <> struct WpMfma<32> {
  typedef f32x16 acc_t;
  static constexpr int NREG = 16;
  static __device__ __forceinline__ acc_t run(float w, float x, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(w, x, c, 0, 0, 0); }
};
template <> struct WpMfma<16> {
  typedef f32x4 acc_t;
  static constexpr int NREG = 4;
  static __device__ __forceinline__ acc_t run(float w, float x, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(w, x, c, 0, 0, 0); }
};

// ABL: ablation bits for tools/ab_wp.py (0 = the product kernel): 1 no epilogue, 2 no staging after an item's first
// chunk, 4 no MFMAs
// The number of waves is the launch's (blockDim.x / 64 <= NWMAX): the launcher takes what the LDS budget admits.
// EC: epilogue class of the 5x5 forms (common.h, Conv5Epi; the 3x3 form is class 0 as it always was)
template <int MF, int KS, int CK, int ABL, int EC = 0>
static __device__ __forceinline__ void igemm_wp_body(const ConvArgs& a) {
  typedef WpGeo<MF, KS, CK> G;
  constexpr int NT = G::NT, MT = G::MT, TW = G::TWX, PAD = G::PAD, NTAPS = G::NTAPS, CKP = G::CKP;
  constexpr int PIECES = G::PIECES, SLOTS = G::SLOTS, XV = G::XV;
  typedef typename WpMfma<MF>::acc_t acc_t;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int NW = (int)(blockDim.x >> 6);
  const int r = lane % MF, h = lane / MF;
  const int nCC = a.Cin / CK;
  const int panelFloats = nCC * NTAPS * NT * CK;
  float* panel = smem;
  float* wbuf = smem + panelFloats + wv * G::WAVE_FLOATS;

  // ---- work items: one wave's 4 x 16 pixel block x channel tile.  Blocks are numbered row-in-band fastest (four
  // blocks = 16 rows), then along the row, then band, then sample; a group of NW consecutive blocks is what the
  // workgroup's waves take together (16 waves: 16 rows x 64 columns).  Group ids are dealt over the 8 XCDs as in
  // igemm_conv_kernel (an XCD walks a contiguous eighth of the groups, channel tile fastest).  The grid is a multiple of
  // 8 nNT or there is one channel tile, so a workgroup's channel tile never changes: one panel.
  const unsigned nNT = (unsigned)a.lgy, nSup = (unsigned)a.lgx;
  const int bxN = (a.W + 15) >> 4, bandsY = (a.H + 15) >> 4;
  const int nItems = a.B * bandsY * bxN * 4;
  unsigned id = blockIdx.x;
  auto decode = [&](unsigned i, int& st, int& nt) {
    if ((nSup & 7u) == 0) {
      const unsigned x = i & 7u, sl = i >> 3;
      nt = (int)(sl % nNT);
      st = (int)(x * (nSup >> 3) + sl / nNT);
    } else {
      st = (int)(i % nSup);
      nt = (int)(i / nSup);
    }
  };
  int st0, ntile;
  decode(id, st0, ntile);

  // ---- the panel: [chunk][tap][n][CK floats], unpadded rows, the 16-byte pieces of row n swizzled (WpGeo::panel_sw):
  // the lanes of a b128 fragment read fall into different bank groups
  {
    const float* src = a.w + (size_t)ntile * panelFloats;
    const int nq = panelFloats / 4;
    for (int q = tid; q < nq; q += (int)blockDim.x) {
      const int row = q / XV, part = q % XV;
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)q * 4);
      *reinterpret_cast<f32x4*>(panel + row * CK + 4 * (part ^ G::panel_sw(row % NT))) = v;
    }
  }
  __syncthreads();   // the only one: from here on a wave waits for nobody

  // ---- per-lane staging geometry, once per wave: piece i covers halo slot q = lane + 64 i -> pixel q / XV, part q % XV
  // (the LDS offset of piece i is that of piece 0 plus a constant: 64 / XV pixels further on, where the swizzle repeats)
  unsigned xgb[PIECES];
  constexpr int PSTEP = 64 / XV;                      // pixels between a lane's consecutive pieces
  static_assert(PSTEP % 8 == 0, "the halo swizzle must repeat from piece to piece");
  const int xpart = lane % XV, xpix0 = lane / XV;
#pragma unroll
  for (int i = 0; i < PIECES; ++i) {
    const int pix = min(xpix0 + PSTEP * i, G::PIX - 1);
    const int ly = pix / TW, lx = pix - ly * TW;
    xgb[i] = 4u * (unsigned)(ly * (int)a.in.sY + lx * (int)a.in.sX + xpart * 4);
  }
  const unsigned xlb0 = 4u * (unsigned)G::halo_off(xpix0, xpart);
  const bool in_last = lane < (SLOTS - 64 * (PIECES - 1));
  const unsigned wb0 = (unsigned)(size_t)(__attribute__((address_space(3))) float*)wbuf;
  // fragment bases: A = the lane's pixel of MFMA tile mt (MF = 32: (2 mt + (r >> 4), r & 15); MF = 16: (mt, r)) of the
  // halo tile, channels 4h..; B = panel row r, swizzled piece
  int apix[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    apix[mt] = (MF == 32) ? ((2 * mt + (r >> 4)) * TW + (r & 15)) * CKP + 4 * h : (mt * TW + r) * CKP + 4 * h;
  // swizzled halo (CK = 16): the swizzle bit of pixel (mt + ty) TW + r + tx is bit 2 of r + tx, flipped when mt + ty is
  // odd (TW = 20 = 4 x 5) -- one lane offset per (tx, parity), every other term a constant of the unrolled loop
  int asw[KS][2];
#pragma unroll
  for (int tx = 0; tx < KS; ++tx)
#pragma unroll
    for (int par = 0; par < 2; ++par)
      asw[tx][par] = (CK == 16) ? (r + tx) * CKP + 4 * (h ^ (((((r + tx) >> 2) & 1) ^ par) << 1)) : 0;
  const int boff = r * CK + 4 * (h ^ G::panel_sw(r));

  for (;;) {
    int st, nt_unused;
    decode(id, st, nt_unused);
    const int item = st * NW + wv;
    const int wrow = item & 3;
    int t = item >> 2;
    const int bxi = t % bxN;
    t /= bxN;
    const int sy = t % bandsY;
    const int b = t / bandsY;
    const int ty0 = sy * 16 + 4 * wrow, tx0 = bxi * 16;   // this wave's 4 x 16 block
    if (item < nItems && ty0 < a.H) {
      // (opaque per item: the epilogue's per-channel pointers are then formed per item instead of living in 64-bit
      // register pairs across the item loop)
      int n0 = ntile * NT;
      asm volatile("" : "+s"(n0));
      const float* inb = a.in.p + (long)b * a.in.sB;
      const bool interior = ty0 >= PAD && ty0 + 4 + PAD <= a.H && tx0 >= PAD && tx0 + 16 + PAD <= a.W;
      const char* halo0 = reinterpret_cast<const char*>(inb + ((long)(ty0 - PAD) * a.in.sY + (long)(tx0 - PAD) * a.in.sX));
      // only used for interior blocks, whose whole halo lies inside the image
      // (readfirstlane returns int: through unsigned, or the low word's bit 31 would be sign-extended into the high one)
      const unsigned long long hu = (unsigned long long)halo0;
      const unsigned hlo = __builtin_amdgcn_readfirstlane((unsigned)hu), hhi = __builtin_amdgcn_readfirstlane((unsigned)(hu >> 32));
      const __amdgpu_buffer_rsrc_t halo_rsrc =
          __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hhi << 32) | hlo), 0, 0x7FFFFFFF, 0x00020000);
      f32x4 xr[PIECES];
      auto prefetch = [&](int cc) {
        const char* src = halo0 + 4 * (long)cc * CK;
        if (interior) {
          // (uniform base in a buffer descriptor) + (the lane's 32-bit byte offset): as plain pointers the compiler keeps
          // every offset as a 64-bit pair across the item loop
          typedef int i32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
          for (int i = 0; i < PIECES - 1; ++i)
            xr[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(halo_rsrc, (int)xgb[i], 4 * cc * CK, 0));
          if (in_last)
            xr[PIECES - 1] =
                __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(halo_rsrc, (int)xgb[PIECES - 1], 4 * cc * CK, 0));
        } else {
          // border blocks only: the geometry is recomputed here from a value the compiler cannot trace back to the
          // lane index, so that it is not hoisted out of the item loop into registers the interior path never uses
          int xp = xpix0;
          asm volatile("" : "+v"(xp));
#pragma unroll
          for (int i = 0; i < PIECES; ++i) {
            const int pix = min(xp + PSTEP * i, G::PIX - 1);
            const int ly = pix / TW, lx = pix - ly * TW;
            const int iy = ty0 + ly - PAD, ix = tx0 + lx - PAD;
            const bool ok = (i < PIECES - 1 || in_last) && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = *reinterpret_cast<const f32x4*>(src + 4 * (ly * (int)a.in.sY + lx * (int)a.in.sX + xpart * 4));
            xr[i] = v;
          }
        }
      };
      auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < PIECES - 1; ++i)
          *reinterpret_cast<__attribute__((address_space(3))) f32x4*>((size_t)(wb0 + xlb0 + 4u * PSTEP * CKP * i)) = xr[i];
        if (in_last)
          *reinterpret_cast<__attribute__((address_space(3))) f32x4*>((size_t)(wb0 + xlb0 + 4u * PSTEP * CKP * (PIECES - 1))) =
              xr[PIECES - 1];
      };

      acc_t acc[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < WpMfma<MF>::NREG; ++j) acc[mt][j] = 0.f;

      prefetch(0);
      commit();
      for (int cc = 0; cc < nCC; ++cc) {
        if (!(ABL & 2) && cc + 1 < nCC) prefetch(cc + 1);
        const float* wp = panel + (size_t)cc * (NTAPS * NT * CK) + boff;
        f32x4 av[2][MT], bv[2];
        auto load_frag = [&](int tap, f32x4* a_, f32x4& b_) {
          const int ty = tap / KS, tx = tap - ty * KS;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            if (CK == 16) a_[mt] = *reinterpret_cast<const f32x4*>(wbuf + asw[tx][(mt + ty) & 1] + (mt + ty) * TW * CKP);
            else a_[mt] = *reinterpret_cast<const f32x4*>(wbuf + apix[mt] + (ty * TW + tx) * CKP);
          }
          b_ = *reinterpret_cast<const f32x4*>(wp + tap * (NT * CK));
        };
        load_frag(0, av[0], bv[0]);
#pragma unroll
        for (int q = 0; q < NTAPS; ++q) {
          if (q + 1 < NTAPS) load_frag(q + 1, av[(q + 1) & 1], bv[(q + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              if (ABL & 4) acc[mt][j] += bv[q & 1][j] * av[q & 1][mt][j];
              else acc[mt] = WpMfma<MF>::run(bv[q & 1][j], av[q & 1][mt][j], acc[mt]);
            }
          __builtin_amdgcn_sched_barrier(0);
        }
        // the next chunk replaces this one in the wave's region: its fragment reads were all issued above and the LDS
        // unit executes a wave's instructions in order
        if (!(ABL & 2) && cc + 1 < nCC) commit();
      }

      const long out_goff = 0;
      if (ABL & 1) {
        if (acc[0][0] + acc[1][0] == 123.456f) a.out.p[0] = 1.f;   // keeps the accumulators alive
      } else {
#define EPI_PRE_SYNC ((void)0)
#define EPI_ES_BASE wbuf
#define EPI_OYW ty0
#define EPI_FULL ((ty0 + 4 <= a.H) && (tx0 + 16 <= a.W))
#define EPI_CLASS Conv5Epi<EC>
        // 32-pixel tiles go through the scratch one after the other (it holds one); the four 16-pixel tiles fit at once
        if constexpr (MF == 32) {
#define EPI_PHASED
#include "igemm_epilogue.inc"
#undef EPI_PHASED
        } else {
#include "igemm_epilogue.inc"
        }
#undef EPI_CLASS
#undef EPI_PRE_SYNC
#undef EPI_ES_BASE
#undef EPI_OYW
#undef EPI_FULL
      }
    }
    id += gridDim.x;
    if (id >= nSup * nNT) break;
  }
}

template <int ABL>
__global__ __launch_bounds__(WP_NW * 64, 1) void igemm_wp_kernel(const ConvArgs a) {
  igemm_wp_body<32, 3, 8, ABL>(a);
}

// the weight-stationary 5x5 forms: compiled for up to 16 waves (MF = 32: 124 VGPRs) and 12 waves (MF = 16: 162 VGPRs),
// no scratch in either
constexpr int ws5_nwmax(int MF) { return MF == 32 ? 16 : 12; }
// One item loop per epilogue class inside the one kernel (its name, grid and LDS size are pinned): the class id is
// wave-uniform, read once, and the loop it selects carries its flag set as compile-time constants
template <int MF, int CK>
__global__ __launch_bounds__(ws5_nwmax(MF) * 64, 1) void igemm_ws5_kernel(const ConvArgs a) {
  switch (a.epi_class) {
    case 1: igemm_wp_body<MF, 5, CK, 0, 1>(a); break;
    case 2: igemm_wp_body<MF, 5, CK, 0, 2>(a); break;
    case 3: igemm_wp_body<MF, 5, CK, 0, 3>(a); break;
    case 4: igemm_wp_body<MF, 5, CK, 0, 4>(a); break;
    default: igemm_wp_body<MF, 5, CK, 0, 0>(a); break;
  }
}

}  // namespace

typedef WpGeo<32, 3, 8> Wp3;
// groups of `nw` wave items (4 x 16 pixel blocks, whole 16-row bands) of a launch: the kernel's logical grid
static long wp_groups(const ConvArgs& a, int nw) { return cdiv((long)a.B * cdiv(a.H, 16) * cdiv(a.W, 16) * 4, nw); }

// whether the wave-private kernel covers this launch of plan `pl` (the 8-channel-chunk 3x3 plan, whose packed panel it
// reads as it is)
// force: the shape test only (unit tests run small launches through it); otherwise also "is it worth it": enough
// groups for a whole chip of 16-wave workgroups, and DEPGAN_IGEMM_WP=1 (opt-in: measured neutral)
bool dg_conv_igemm_wp_supported(const ConvPlan& pl, const ConvArgs& a, bool force) {
  if (!dg_plan_tile3_ck8(pl)) return false;
  if (a.Cin != pl.Cin || (a.Cin % 8) || a.Cin > 64 || (a.Cout % 32) || a.groups > 1 || a.cpt > 0 || a.dbg) return false;
  if (a.ep.head_out) return false;   // the fused head lives in the tile kernel's epilogue only
  const size_t lds = ((size_t)a.Cin * 9 * 32 + (size_t)WP_NW * Wp3::WAVE_FLOATS) * sizeof(float);
  if (lds > 160 * 1024) return false;
  if (force) return true;
  static int on = -1;
  if (on < 0) {
    const char* e = getenv("DEPGAN_IGEMM_WP");
    on = (e && atoi(e) != 0) ? 1 : 0;     // opt-in: measured neutral (see the header of this file)
  }
  if (!on) return false;
  const long sup = wp_groups(a, WP_NW);
  return (sup & 7) == 0 && sup * (a.Cout / 32) >= 256;
}

// 160 KB for every entry of this file: their launches' LDS sizes depend on Cin and on the wave count
#define WP_K(N) {reinterpret_cast<const void*>(&igemm_wp_kernel<N>), "igemm_wp_kernel<" #N ">", 160 * 1024},
static const DgKernel kWp[] = {
    WP_K(0)
#ifdef DEPGAN_WP_ABLATIONS
    WP_K(1) WP_K(2) WP_K(3) WP_K(4)   // tools/ab_wp_ablation.sh: DEPGAN_WP_ABL selects an ablated instantiation
#endif
};
#undef WP_K

int dg_conv_wp_prepare(const ConvPlan&, const ConvArgs& a, DgConvLaunch* L) {
  const int nNT = a.Cout / 32;
  L->a = a;
  L->a.lgx = (int)wp_groups(a, WP_NW);
  L->a.lgy = nNT;
  const long total = (long)L->a.lgx * nNT;
  // one workgroup per CU, rounded down to a multiple of 8 nNT (XCD round-robin x channel tiles: a workgroup keeps its
  // channel tile and thereby its panel for all its items)
  long G = dg_cu_count();
  G -= G % (8L * nNT);
  if (G < 8L * nNT) G = 8L * nNT;
  // (a group count that is not a multiple of 8 takes the plain id -> (group, channel tile) form, in which a
  // persistent workgroup would change its channel tile: one item per workgroup then -- unit tests only)
  if (G > total || (L->a.lgx & 7) != 0) G = total;
  int abl = 0;
#ifdef DEPGAN_WP_ABLATIONS
  static int abl_env = -1;
  if (abl_env < 0) {
    const char* e = getenv("DEPGAN_WP_ABL");
    abl_env = e ? atoi(e) : 0;
  }
  abl = abl_env ? (abl_env >= 1 && abl_env <= 3 ? abl_env : 4) : 0;
#endif
  L->k = &kWp[abl];
  L->grid = (unsigned)G;
  L->block = WP_NW * 64;
  L->lds = ((size_t)a.Cin * 9 * 32 + (size_t)WP_NW * Wp3::WAVE_FLOATS) * sizeof(float);
  return DG_OK;
}

// ---------------------------------------------------------------------------
// the weight-stationary 5x5 forms (the 5x5 tile plans of dg_plan_conv, whose packed panels they read as they are)
// ---------------------------------------------------------------------------
// waves per workgroup: what 160 KB of LDS admit beside the panel, at most the instantiation's register budget
template <int MF, int CK>
static int ws5_waves(int Cin) {
  const long panel = (long)Cin * 25 * MF, wave = WpGeo<MF, 5, CK>::WAVE_FLOATS;
  long nw = (160L * 1024 / 4 - panel) / wave;
  // DEPGAN_IGEMM_WS5_WAVES=<n> caps it for A/B runs.  Default 16: only 16->32 has room for more than 12, and there
  // 16 waves measured equal at batch 96 and 10 % faster at batch 32 (125 against 139 us)
  static int cap = -1;
  if (cap < 0) {
    const char* e = getenv("DEPGAN_IGEMM_WS5_WAVES");
    cap = (e && atoi(e) >= 4) ? atoi(e) : 16;
  }
  if (nw > cap) nw = cap;
  return (int)(nw < ws5_nwmax(MF) ? nw : ws5_nwmax(MF));
}
static int ws5_waves_of(const ConvPlan& pl, int Cin) { return pl.MF == 32 ? ws5_waves<32, 8>(Cin) : ws5_waves<16, 16>(Cin); }

// force: the shape test only (the operator surface, path 9); otherwise also the measured per-shape default and the size
// threshold, or DEPGAN_IGEMM_WS5=0|1 for all covered shapes (read once)
bool dg_conv_igemm_ws5_supported(const ConvPlan& pl, const ConvArgs& a, bool force) {
  if (!dg_plan_tile5(pl)) return false;
  if (pl.CK != (pl.MF == 32 ? 8 : 16)) return false;
  if (a.Cin != pl.Cin || a.Cout != pl.Cout || a.Cout != pl.MF || (a.Cin != 16 && a.Cin != 32)) return false;
  if (a.groups > 1 || a.cpt > 0 || a.dbg || a.ep.head_out) return false;
  if (force) return true;
  static int mode = -2;
  if (mode == -2) {
    const char* e = getenv("DEPGAN_IGEMM_WS5");
    mode = e ? (atoi(e) != 0 ? 1 : 0) : -1;
  }
  if (mode == 0) return false;
  // fewer wave items than two per wave slot of the chip: the tile kernel's smaller items balance better
  const long items = (long)a.B * cdiv(a.H, 4) * cdiv(a.W, 16);
  const long slots = (long)dg_cu_count() * ws5_waves_of(pl, a.Cin);
  if (items < 2 * slots) return false;
  if (mode == 1) return true;
  // the measured per-shape default (profiles/ws5_experiments.md): 16->16 and 16->32 at both batches of the step
  // (-4 ... -9 %); 32->32 at batch 96 (8 items per slot: -7.6 %) but not at batch 32 (2.7 per slot: +5 %, the 102 KB
  // panel load in front of three short rounds); 32->16 at neither (+3 ... +5 %: 11 waves, two SIMDs with two)
  if (a.Cin == 32 && a.Cout == 16) return false;
  if (a.Cin == 32 && a.Cout == 32) return items >= 4 * slots;
  return true;
}

static const DgKernel kWs5[2] = {   // [MF == 16]
    {reinterpret_cast<const void*>(&igemm_ws5_kernel<32, 8>), "igemm_ws5_kernel<32,8>", 160 * 1024},
    {reinterpret_cast<const void*>(&igemm_ws5_kernel<16, 16>), "igemm_ws5_kernel<16,16>", 160 * 1024}};

int dg_conv_ws5_prepare(const ConvPlan& pl, const ConvArgs& a, DgConvLaunch* L) {
  const bool wide = pl.MF == 32;
  const int nw = ws5_waves_of(pl, a.Cin);
  const size_t wave = wide ? WpGeo<32, 5, 8>::WAVE_FLOATS : WpGeo<16, 5, 16>::WAVE_FLOATS;
  L->a = a;
  L->a.epi_class = dg_conv5_epi_class(dg_epilogue_flags(a.ep));
  L->a.lgx = (int)wp_groups(a, nw);
  L->a.lgy = 1;
  // one workgroup per CU; a multiple of 8 when the groups are dealt over the XCDs
  long G = dg_cu_count();
  if ((L->a.lgx & 7) == 0) G -= G % 8;
  if (G > L->a.lgx || G < 1) G = L->a.lgx;
  L->k = &kWs5[wide ? 0 : 1];
  L->grid = (unsigned)G;
  L->block = (unsigned)nw * 64;
  L->lds = ((size_t)a.Cin * 25 * pl.MF + (size_t)nw * wave) * sizeof(float);
  return DG_OK;
}
