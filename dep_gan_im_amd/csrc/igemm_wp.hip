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
#include <stdlib.h>

#include "common.h"
#include "epilogue.h"

namespace {

constexpr int WP_NW = 16;                   // waves per workgroup
constexpr int WP_TWX = 18, WP_TWY = 6;      // halo of a 4 x 16 block
constexpr int WP_PIX = WP_TWX * WP_TWY;     // 108 pixels
constexpr int WP_CK = 8, WP_CKP = 12;       // channels per chunk; floats per halo pixel row (48 B: conflict-free b128 reads)
constexpr int WP_WAVE_FLOATS = WP_PIX * WP_CKP;   // 1296 floats = 5184 B >= the 32 x 36-float transpose tile (4608 B)
constexpr int WP_SLOTS = WP_PIX * 2;        // 16-byte pieces of one halo chunk (two per pixel)
constexpr int WP_PIECES = (WP_SLOTS + 63) / 64;   // 4 per lane, the last one partial (24 lanes)

// ABL: ablation bits for tools/ab_wp.py (0 = the product kernel): 1 no epilogue, 2 no staging after an item's first
// chunk, 4 no MFMAs
template <int ABL>
__global__ __launch_bounds__(WP_NW * 64, 1) void igemm_wp_kernel(const ConvArgs a) {
  constexpr int MF = 32, NT = 32, MT = 2, KS = 3, TW = WP_TWX;
  typedef f32x16 acc_t;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nCC = a.Cin / WP_CK;
  const int panelFloats = nCC * 9 * NT * WP_CK;
  float* panel = smem;
  float* wbuf = smem + panelFloats + wv * WP_WAVE_FLOATS;

  // ---- work items: super-tiles of 16 rows x 64 columns (wave w: rows 4 (w & 3), columns 16 (w >> 2)) x channel tile;
  // ids dealt over the 8 XCDs as in igemm_conv_kernel (an XCD walks a contiguous eighth of the super-tiles, channel
  // tile fastest).  The grid is a multiple of 8 nNT, so a workgroup's channel tile never changes: one panel.
  const unsigned nNT = (unsigned)a.lgy, nSup = (unsigned)a.lgx;
  const int supX = (a.W + 63) >> 6, supY = (a.H + 15) >> 4;
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
  const int n0 = ntile * NT;

  // ---- the panel: [chunk][tap][n][8 floats], 32-byte rows, the two 16-byte halves of row n swapped when bit 2 of n
  // is set: lanes r and r + 4 of a b128 fragment read then fall into different bank groups (conflict-free, unpadded)
  {
    const float* src = a.w + (size_t)ntile * panelFloats;
    const int nq = panelFloats / 4;
    for (int q = tid; q < nq; q += WP_NW * 64) {
      const int row = q >> 1, half = q & 1;
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)q * 4);
      *reinterpret_cast<f32x4*>(panel + row * 8 + 4 * (half ^ ((row >> 2) & 1))) = v;
    }
  }
  __syncthreads();   // the only one: from here on a wave waits for nobody

  // ---- per-lane staging geometry, once per wave: piece i covers halo slot q = lane + 64 i -> pixel q / 2, half q & 1
  unsigned xgb[WP_PIECES], xlb[WP_PIECES];
  int xyx[WP_PIECES];
#pragma unroll
  for (int i = 0; i < WP_PIECES; ++i) {
    const int q = min(lane + 64 * i, WP_SLOTS - 1);
    const int pix = q >> 1, part = q & 1;
    const int ly = pix / TW, lx = pix - ly * TW;
    xgb[i] = 4u * (unsigned)(ly * (int)a.in.sY + lx * (int)a.in.sX + part * 4);
    xlb[i] = 4u * (unsigned)(pix * WP_CKP + part * 4);
    xyx[i] = (ly << 16) | (lx << 8) | (part * 4);
  }
  const bool in_last = lane < (WP_SLOTS - 64 * (WP_PIECES - 1));
  const unsigned wb0 = (unsigned)(size_t)(__attribute__((address_space(3))) float*)wbuf;
  // fragment bases: A = pixel (2 mt + (r >> 4), r & 15) of the halo tile, channels 4h..; B = panel row r, swizzled half
  int apix[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) apix[mt] = ((2 * mt + (r >> 4)) * TW + (r & 15)) * WP_CKP + 4 * h;
  const int boff = r * 8 + 4 * (h ^ ((r >> 2) & 1));
  const int wrow = wv & 3, wcol = wv >> 2;

  for (;;) {
    int st, nt_unused;
    decode(id, st, nt_unused);
    const int sx = st % supX;
    int t = st / supX;
    const int sy = t % supY;
    const int b = t / supY;
    const int ty0 = sy * 16 + 4 * wrow, tx0 = sx * 64 + 16 * wcol;   // this wave's 4 x 16 block
    if (ty0 < a.H && tx0 < a.W) {
      const float* inb = a.in.p + (long)b * a.in.sB;
      const bool interior = ty0 >= 1 && ty0 + 5 <= a.H && tx0 >= 1 && tx0 + 17 <= a.W;
      const char* halo0 = reinterpret_cast<const char*>(inb + ((long)(ty0 - 1) * a.in.sY + (long)(tx0 - 1) * a.in.sX));
      f32x4 xr[WP_PIECES];
      auto prefetch = [&](int cc) {
        const char* src = halo0 + 4 * (long)cc * WP_CK;
        if (interior) {
#pragma unroll
          for (int i = 0; i < WP_PIECES - 1; ++i) xr[i] = *reinterpret_cast<const f32x4*>(src + xgb[i]);
          if (in_last) xr[WP_PIECES - 1] = *reinterpret_cast<const f32x4*>(src + xgb[WP_PIECES - 1]);
        } else {
#pragma unroll
          for (int i = 0; i < WP_PIECES; ++i) {
            const int iy = ty0 + (xyx[i] >> 16) - 1, ix = tx0 + ((xyx[i] >> 8) & 255) - 1;
            const bool ok = (i < WP_PIECES - 1 || in_last) && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = *reinterpret_cast<const f32x4*>(src + xgb[i]);
            xr[i] = v;
          }
        }
      };
      auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < WP_PIECES - 1; ++i)
          *reinterpret_cast<__attribute__((address_space(3))) f32x4*>((size_t)(wb0 + xlb[i])) = xr[i];
        if (in_last)
          *reinterpret_cast<__attribute__((address_space(3))) f32x4*>((size_t)(wb0 + xlb[WP_PIECES - 1])) = xr[WP_PIECES - 1];
      };

      acc_t acc[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[mt][j] = 0.f;

      prefetch(0);
      commit();
      for (int cc = 0; cc < nCC; ++cc) {
        if (!(ABL & 2) && cc + 1 < nCC) prefetch(cc + 1);
        const float* wp = panel + (size_t)cc * (9 * NT * WP_CK) + boff;
        f32x4 av[2][MT], bv[2];
        auto load_frag = [&](int tap, f32x4* a_, f32x4& b_) {
          const int ty = tap / KS, tx = tap - ty * KS;
          const int tapoff = (ty * TW + tx) * WP_CKP;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) a_[mt] = *reinterpret_cast<const f32x4*>(wbuf + apix[mt] + tapoff);
          b_ = *reinterpret_cast<const f32x4*>(wp + tap * (NT * WP_CK));
        };
        load_frag(0, av[0], bv[0]);
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          if (q + 1 < 9) load_frag(q + 1, av[(q + 1) & 1], bv[(q + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              if (ABL & 4) acc[mt][j] += bv[q & 1][j] * av[q & 1][mt][j];
              else acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[q & 1][j], av[q & 1][mt][j], acc[mt], 0, 0, 0);
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
#define EPI_PHASED
#define EPI_OYW ty0
#define EPI_FULL ((ty0 + 4 <= a.H) && (tx0 + 16 <= a.W))
#include "igemm_epilogue.inc"
#undef EPI_PRE_SYNC
#undef EPI_ES_BASE
#undef EPI_PHASED
#undef EPI_OYW
#undef EPI_FULL
      }
    }
    id += gridDim.x;
    if (id >= nSup * nNT) break;
  }
}

}  // namespace

// whether the wave-private kernel covers this launch of plan `pl` (the 8-channel-chunk 3x3 plan, whose packed panel it
// reads as it is)
// force: the shape test only (unit tests run small launches through it); otherwise also "is it worth it": enough
// super-tiles for a whole chip of 16-wave workgroups, and DEPGAN_IGEMM_WP=1 (opt-in: measured neutral)
bool dg_conv_igemm_wp_supported(const ConvPlan& pl, const ConvArgs& a, bool force) {
  if (pl.variant != 8 || pl.bf16 || pl.KS != 3 || pl.CK != WP_CK) return false;
  if (a.Cin != pl.Cin || (a.Cin % WP_CK) || a.Cin > 64 || (a.Cout % 32) || a.groups > 1 || a.cpt > 0 || a.dbg) return false;
  if (a.ep.head_out) return false;   // the fused head lives in the tile kernel's epilogue only
  const size_t lds = ((size_t)a.Cin * 9 * 32 + (size_t)WP_NW * WP_WAVE_FLOATS) * sizeof(float);
  if (lds > 160 * 1024) return false;
  if (force) return true;
  static int on = -1;
  if (on < 0) {
    const char* e = getenv("DEPGAN_IGEMM_WP");
    on = (e && atoi(e) != 0) ? 1 : 0;     // opt-in: measured neutral (see the header of this file)
  }
  if (!on) return false;
  const long sup = (long)a.B * cdiv(a.H, 16) * cdiv(a.W, 64);
  return (sup & 7) == 0 && sup * (a.Cout / 32) >= 256;
}

int dg_conv_igemm_wp(const ConvPlan& pl, const ConvArgs& a_in, hipStream_t st) {
  ConvArgs a = a_in;
  DGCHECK(dg_conv_igemm_check(pl, a));   // unit tests launch this kernel directly, not through dg_conv_igemm
  const size_t lds = ((size_t)a.Cin * 9 * 32 + (size_t)WP_NW * WP_WAVE_FLOATS) * sizeof(float);
  static DgOncePerDevice once;
  if (once.need())
    HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&igemm_wp_kernel<0>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  const int nNT = a.Cout / 32;
  a.lgx = a.B * cdiv(a.H, 16) * cdiv(a.W, 64);
  a.lgy = nNT;
  const long total = (long)a.lgx * nNT;
  // one workgroup per CU, rounded down to a multiple of 8 nNT (XCD round-robin x channel tiles: a workgroup keeps its
  // channel tile and thereby its panel for all its items)
  long G = dg_cu_count();
  G -= G % (8L * nNT);
  if (G < 8L * nNT) G = 8L * nNT;
  // (a super-tile count that is not a multiple of 8 takes the plain id -> (super-tile, channel tile) form, in which a
  // persistent workgroup would change its channel tile: one item per workgroup then -- unit tests only)
  if (G > total || (a.lgx & 7) != 0) G = total;
#ifdef DEPGAN_WP_ABLATIONS
  // tools/ab_wp_ablation.sh (build with -DDEPGAN_WP_ABLATIONS): DEPGAN_WP_ABL selects an ablated instantiation
  static int abl = -1;
  if (abl < 0) {
    const char* e = getenv("DEPGAN_WP_ABL");
    abl = e ? atoi(e) : 0;
  }
  if (abl) {
    static DgOncePerDevice once2;
    if (once2.need()) {
      HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&igemm_wp_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&igemm_wp_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&igemm_wp_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&igemm_wp_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    }
    switch (abl) {
      case 1: hipLaunchKernelGGL((igemm_wp_kernel<1>), dim3((unsigned)G), dim3(WP_NW * 64), lds, st, a); break;
      case 2: hipLaunchKernelGGL((igemm_wp_kernel<2>), dim3((unsigned)G), dim3(WP_NW * 64), lds, st, a); break;
      case 3: hipLaunchKernelGGL((igemm_wp_kernel<3>), dim3((unsigned)G), dim3(WP_NW * 64), lds, st, a); break;
      default: hipLaunchKernelGGL((igemm_wp_kernel<4>), dim3((unsigned)G), dim3(WP_NW * 64), lds, st, a); break;
    }
    HIPCHECK(hipGetLastError());
    return DG_OK;
  }
#endif
  hipLaunchKernelGGL((igemm_wp_kernel<0>), dim3((unsigned)G), dim3(WP_NW * 64), lds, st, a);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
