// 3x3 NHWC fp32 convolution as Winograd F(2x2, 3x3) on the CDNA4 fp32 matrix cores: 16 multiplications per 2x2 output
// block and input channel instead of 36 -- the contraction of igemm_conv_kernel<32,3,8,9> with 4/9 of its MFMAs.
//
// Why: on this machine an fp32 MFMA stream is the vector ALU (nothing a SIMD issues overlaps with
// it), igemm_conv_kernel sits at 0.68 ... 0.84 of the fp32 matrix peak on the 3x3 layers and its ablations
// (profiles/r03_conv_experiments.md) put 0.82 as the ceiling of ANY direct form.  The remaining lever is the number of
// MFMAs.  Y = A^T [ (G g G^T) . (B^T d B) ] A with the usual F(2x2,3x3) matrices: B^T and A^T hold only 0 and +-1 (the
// input and output transforms are additions), G holds 1 and 1/2 (the weight transform is done once per weight update by
// the packing kernel, in double, rounded once).  Same operands, same fp32 accumulation over Cin in the same chunk order;
// what changes is the summation tree (measured against an fp64 convolution: 1.7 x the rounding error of the direct
// kernel, both ~1e-7 of the output's range -- tests/test_gpu_ops.py).
//
// Mapping (one workgroup = 256 threads = 4 waves; item = 8 MT x 16 output pixels of one sample x 32 output channels;
// MT = 1: 8-row tiles, 64 accumulator registers per wave, three workgroups per CU -- the default; MT = 2: 16-row tiles,
// 128 registers, two per CU -- the form that carries the fused one-channel head):
//   * the tile is 4 MT x 8 Winograd tiles (2 x 2 outputs each); the 16 "frequencies" (a, b) of the transform domain are
//     16 independent GEMMs  M_f[tile][n] = sum_c V_f[tile][c] U_f[c][n]  (32 MT x Cin x 32);
//   * wave w owns the frequencies a = w (b = 0..3): 4 frequencies x MT row tiles of v_mfma_f32_32x32x2_f32.  Its
//     weight fragments U_f are nobody else's: from the packed panel [nt][chunk][f][n][8] straight into registers, never
//     through LDS.  And it transforms exactly the V values it multiplies, each LANE its own: v_mfma_f32_32x32x2_f32
//     takes from lane (r = lane & 31, h = lane >> 5) the operand V_f[tile 32 mt + r][channels 4h .. 4h + 3], so transform
//     task mt of a lane is (tile 32 mt + r, channel half h, row a = w): two halo rows x four columns in, the four
//     frequencies b = 0..3 x four channels out -- exactly the 16 operand registers of the lane's MFMAs for row tile mt.
//     V never exists in memory: no LDS write, no read back, no wait between the transform and the MFMAs;
//   * per chunk of 8 input channels: the raw (8 MT + 2) x 18 x 8 halo is copied global -> LDS by the DMA path
//     (buffer_load_dwordx4 ... lds: no registers, no ds_write pass, asynchronous) into a ring of NBUF raw buffers (two:
//     three measured the same, profiles/wino_ring_experiments.md): the first NBUF - 1 chunks of an item are issued back
//     to back, chunk c + NBUF - 1 behind the barrier of chunk c -- the ONE barrier of the chunk, a bare s_barrier in
//     front of which a wave waits for its own pieces of chunk c only (s_waitcnt vmcnt(N), N = the younger DMA
//     instructions + the four weight-fragment loads: vector-memory instructions complete in order).  The fragment loads are asm statements, waited for by count in front of the
//     first MFMA: the compiler, which next to a DMA in flight waits vmcnt(0) for every load it knows of and in front
//     of every __syncthreads(), sees no load in the chunk loop and drains nothing.  Then the transform (8 b128 reads
//     of the raw image and 16 packed additions per task) and 16 MT MFMAs per wave out of registers.  The chunk loop is
//     straight-line: with two buffers a chunk differs from its neighbour only in being the first (zero C operand), in
//     its ring slot and in being the last (no DMA behind the barrier, vmcnt(0) in front of the MFMAs), so the steady
//     state is unrolled by two with the slot an immediate (the offset: field of the ds_read_b128, a constant m0 of the
//     DMA), both waits immediates, one scalar addition each for the DMA's offset and the fragment base (a scalar
//     pointer; the lane's part is a fixed 32-bit offset), one compare and one branch per two chunks; whether a DMA
//     piece lies in the image is decided once per item (interior and border items issue the same instructions), and
//     gathered K is a kernel of its own (profiles/wino_straightline_experiments.md).  The raw image is
//     XOR-swizzled (rslot): the lanes the LDS serves together on a b128 read are neighbouring tiles of one channel
//     half, 64 bytes apart unswizzled;
//   * epilogue: each wave reduces its four b's to the two output columns in registers (Z[a][q] = row transform), the
//     waves exchange Z through LDS, and the fused epilogue of igemm_conv (igemm_epilogue.inc, same text) fetches
//     v = Z[0] + Z[1] + Z[2] (even rows) or Z[1] - Z[2] - Z[3] (odd rows) where it used to fetch one transposed value.
// Covers KS = 3, stride 1, 'same' padding, Cin % 8 == 0, Cout % 32 == 0, even H and W; gathered K (ConvArgs::cpt) as in
// igemm_conv; no groups; an input view whose halo tile (18 rows, 18 pixels, the channel row and the largest run offset)
// spans less than 2 GiB -- the sample stride is free (64-bit descriptor base per item).  Everything else stays on
// igemm_conv_kernel.
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "epilogue.h"

namespace {

constexpr int WN_CK = 8;                         // channels per chunk (one b128 fragment read = 4 MFMAs of 2 channels)
constexpr int WN_TW = 18;                       // halo columns of a 16-pixel-wide tile
constexpr int WN_CP = 36;                       // floats per tile row of the Z exchange (32 channels + 4)
constexpr int WN_XV = WN_CK / 4;

// MT = MFMA row tiles (32 Winograd tiles = 8 x 16 output pixels each) per wave: the workgroup's pixel tile is 8 MT rows
// x 16 columns.  MT = 2: 128 accumulator registers per wave, two workgroups per CU.  MT = 1: 64, three per CU -- more
// waves per SIMD to keep the matrix pipe busy (one wave reaches 0.60 of it, two 0.72, four 0.84:
// profiles/r03_conv_experiments.md) at twice the weight-fragment traffic per MFMA and a larger halo share.
template <int MT>
struct WnCfg {
  static constexpr int TH = 8 * MT;                     // output rows per workgroup
  static constexpr int NTILE = 32 * MT;                 // Winograd tiles per workgroup
  static constexpr int PIXT = (TH + 2) * WN_TW;         // raw halo pixels
  // The raw halo chunk is copied global -> LDS by the DMA path (buffer_load_dwordx4 ... lds: no VGPR destination, no
  // ds_write pass, asynchronous): a wave-instruction writes 64 lanes x 16 B lane-linearly, so the LDS image is the
  // unpadded [pixel][8 channels] one, in whole rounds of 256 pieces.  Which piece a lane FETCHES is free, and that is
  // where the bank swizzle goes (rslot): logical piece (pixel, half) lives in slot (2 pixel + half) ^ ((column >> 2) & 3)
  // -- the transform's reads come from lanes that hold neighbouring tiles of ONE channel half, pixels two apart = slots
  // four apart, and the XOR spreads each run of four such slots over the four positions of its 64 bytes.
  static constexpr int XTOT = PIXT * WN_XV;             // 16-byte pieces of a raw chunk
  static constexpr int NXP = (XTOT + 255) / 256;        // DMA instructions per wave and chunk
  static constexpr int RAW = NXP * 256 * 4;             // floats
  static_assert(XTOT % 4 == 0 && WN_TW % 2 == 0, "rslot permutes inside aligned groups of four slots: halo and padding stay apart");
  static constexpr int ZPLANE = NTILE * WN_CP + 32;     // one (a, q): +128 B so that q = 0 / 1 of a pixel pair differ in bank group
  static constexpr int Z = 8 * ZPLANE;
  // a ring of NBUF raw buffers (one barrier per chunk: after the barrier of chunk c a wave stages chunk c + NBUF - 1 into
  // the buffer the transform of chunk c - 1 read last).  Two: the weight-fragment wait in front of the MFMAs completes,
  // in order, every DMA issued before this chunk's barrier, so only ONE chunk is ever in flight behind it, and three
  // buffers measured no faster than two (profiles/wino_ring_experiments.md).  The chunk walk of wino_body is written for
  // two: the ring slot of a chunk is a compile-time tag of its body (profiles/wino_straightline_experiments.md).
  // The Z exchange of the epilogue aliases the ring and is the larger of the two in both forms (37.9 KB / 73 KB against
  // 24 / 36 KB for three buffers), so the ring costs no LDS and the workgroups per CU stay what the registers allow
  static constexpr int NBUF = 2;
  static_assert(NBUF >= 2 && NBUF * RAW <= Z, "the raw ring must fit under the Z exchange: LDS and workgroups per CU unchanged");
  static_assert((NBUF - 1) * NXP + 4 < 64, "counted waits: vmcnt is a 6-bit field");
  static constexpr size_t LDS = sizeof(float) * (size_t)Z;
  static constexpr int WGS_PER_CU = (MT == 2) ? 2 : 3;
};

// s_waitcnt vmcnt(N) with N a compile-time count of vector-memory instructions that may stay in flight.  Explicit, with a
// memory clobber: the compiler knows neither that the DMA writes LDS nor (the weight fragments are loaded in an asm
// statement) that these loads exist
template <int N>
static __device__ __forceinline__ void wn_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// compile-time ring slot of a chunk body
template <int S>
using WnSlot = std::integral_constant<int, S>;

// 16-byte slot of the raw LDS image that holds logical piece (pixel, channel half) of the (rows x 18) halo: the two low
// bits of the linear slot 2 pixel + half XORed with bits 2..3 of the pixel's column.  A b128 read of the transform
// (row y, column 2 tx + j, half h over the lanes' tiles tx = 0..7, ty = 0..3) then hits different 16-byte slots of the
// bank window in every group of lanes the LDS serves together -- eight consecutive lanes modulo 8 slots as well as the
// 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} modulo 16 (enumerated in tests/test_wino_regmap_cpu.py)
static __device__ __forceinline__ int rslot(int pix, int half) { return (2 * pix + half) ^ (((pix % WN_TW) >> 2) & 3); }
// its inverse on slot indices: the key depends on slot >> 2 only (18 columns are even), so the same XOR undoes it
static __device__ __forceinline__ int rslot_inv(int q) { return q ^ ((((q >> 1) % WN_TW) >> 2) & 3); }

// Epilogue classes (profiles/epi_classes_experiments.md).  The fused epilogue tests nine flags of ConvArgs::ep per item
// and again in every pass, and forms descriptors, lane offsets and strides of operands that are absent: next to the 64
// MFMAs of a short-K item that is most of what a wave executes outside its chunks, and it costs the persistent kernel 66
// spilled SGPRs.  An instantiation whose flags are constants carries only the statements of its flag set (the same text:
// igemm_epilogue.inc, EPI_CLASS).  The table is closed: exactly the flag sets the model launches on this kernel
// (model.hip: g_forward with g_layer_epilogue -- a pool only ever follows a plain conv layer, never a FiLM layer --,
// g_conv_bn_bwd, d_forward, d_backward_chain, the u-forward of critic_enqueue).  Class 0 is the generic kernel, which
// everything else takes: accumulate, the phase-1 bias-only launches, what the operator entries combine.
constexpr unsigned WN_BAR = DG_EPF_BIAS | DG_EPF_AFFINE | DG_EPF_RELU;    // convolution + BatchNorm affine + ReLU
constexpr unsigned WN_FILM = WN_BAR | DG_EPF_FILM | DG_EPF_RES;           // the generator's FiLM layer
constexpr int WN_NCLASS = 11, WN_HEAD_CLASS = 10;                          // 1 .. 9: the 8-row kernel; 10: the fused head
constexpr unsigned kWnClassMask[WN_NCLASS] = {
    0,                                                   //  0 generic (run-time flags)
    WN_BAR,                                              //  1 generator conv
    WN_BAR | DG_EPF_POOL,                                //  2   ... with the fused pool (gen_1 / gen_3 / gen_5)
    WN_FILM,                                             //  3 FiLM layer, forward-only passes
    WN_FILM | DG_EPF_PRE,                                //  4   ... storing u for the backward
    DG_EPF_RES | DG_EPF_MASK,                            //  5 generator backward-data: gradient join + ReLU mask
    DG_EPF_MASK,                                         //  6 backward-data with a mask; the critics' u-forward
    0,                                                   //  7 backward-data into a pooled layer: nothing
    DG_EPF_BIAS | DG_EPF_RELU,                           //  8 critic 3x3 forward
    DG_EPF_BIAS | DG_EPF_RELU | DG_EPF_POOL,             //  9   ... with the fused pool
    WN_BAR | DG_EPF_HEAD,                                // 10 gen_17 with the fused one-channel head (stored or skipped)
};
#define WN_CLASSES8(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9)
template <int EC>
struct WnEpi {
  static_assert(EC >= 0 && EC < WN_NCLASS, "epilogue class");
  static constexpr unsigned M = kWnClassMask[EC];
  static constexpr bool fixed = EC != 0;
  static constexpr bool bias = M & DG_EPF_BIAS, affine = M & DG_EPF_AFFINE, film = M & DG_EPF_FILM, relu = M & DG_EPF_RELU,
                        pre = M & DG_EPF_PRE, res = M & DG_EPF_RES, msk = M & DG_EPF_MASK, pool = M & DG_EPF_POOL,
                        head = M & DG_EPF_HEAD;
};

// ABL: ablation bits for tools/time_wino.py (0 = the product kernel; the others are compiled with
// -DDEPGAN_WINO_ABLATIONS only): 1 no epilogue, 2 no input transform (zero operands), 4 no MFMAs, 8 no raw staging
// GATH: gathered K (ConvArgs::cpt > 0), an instantiation of its own: the plain kernels carry no test for it
// EC: epilogue class (0: the flags of a.ep are read at run time)
template <int MT, bool PERS, bool HEAD, bool GATH = false, int ABL = 0, int EC = 0>
static __device__ __forceinline__ void wino_body(const ConvArgs& a) {
  typedef WnCfg<MT> C;
  constexpr int MF = 32, NT = 32;
  constexpr int WN_RAW = C::RAW, WN_ZPLANE = C::ZPLANE, WN_XTOT = C::XTOT, NXP = C::NXP, NBUF = C::NBUF;
  constexpr int NXI = (ABL & 8) ? 0 : NXP;   // DMA instructions a wave really issues per chunk
  typedef f32x16 acc_t;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // raw halo buffers [(8 MT + 2) x 18][8] x NBUF at smem + slot * RAW, in whole rounds of 256 pieces; the Z planes of the
  // epilogue alias all of them

  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int tilesX = (a.W + 15) >> 4, tilesY = (a.H + C::TH - 1) / C::TH;
  const unsigned nNTall = (unsigned)a.lgy, nPix = (unsigned)a.lgx;
  const int nCC = a.Cin / WN_CK;

  // ---- per-thread geometry, once per workgroup ----
  // raw staging: DMA piece i of this thread fills LDS slot q = tid + 256 i with logical piece rslot_inv(q): byte offset
  // from the halo origin, or an out-of-range offset for the padding slots behind the halo tile (the hardware returns
  // zeros for those, as for out-of-image pixels)
  constexpr int SENT = (int)0x80000000;
  int xvo[NXP], xyx[NXP];
#pragma unroll
  for (int i = 0; i < NXP; ++i) {
    const int q = tid + i * 256;
    const int lq = rslot_inv(q);
    const int pix = lq >> 1, part = lq & 1;
    const int ly = pix / WN_TW, lx = pix - ly * WN_TW;
    xvo[i] = (q < WN_XTOT) ? 4 * (ly * (int)a.in.sY + lx * (int)a.in.sX + part * 4) : SENT;
    xyx[i] = (ly << 8) | lx;
  }
  // transform task i of a lane: tile 32 i + (lane & 31), channel half lane >> 5, transform row a = wave -- the operand
  // layout of the MFMA, so the task's results are the lane's own A operands of row tile mt = i.
  // Row a of B^T d needs two of the tile's four halo rows:  a = 0: d0 - d2,  1: d1 + d2,  2: d2 - d1,  3: d1 - d3
  // = x + s y with (x, y) = rows (0,2) (1,2) (2,1) (1,3) and s = +1 for a = 1, else -1.
  int tA[MT][4], tB[MT][4];
  float tS[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int cg = h, aa = wv, T = 32 * i + r;
    const int tyi = T >> 3, txi = T & 7;
    const int rA = (aa == 0) ? 0 : (aa == 2 ? 2 : 1), rB = (aa == 3) ? 3 : (aa == 2 ? 1 : 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tA[i][j] = 16 * rslot((2 * tyi + rA) * WN_TW + 2 * txi + j, cg);   // bytes; the ring slot is an immediate offset
      tB[i][j] = 16 * rslot((2 * tyi + rB) * WN_TW + 2 * txi + j, cg);
    }
    tS[i] = (aa == 1) ? 1.f : -1.f;
  }
  const int wbase = __builtin_amdgcn_readfirstlane(wv * 256);   // this wave's float offset inside a 256-piece round
  // fragments: A = V[f][32 mt + r][4h ..] = vr[mt][f] of the transform, B = panel[f][r][4h ..]
  const int wvo = 4 * ((4 * wv * 32 + r) * WN_CK + 4 * h);   // bytes

  unsigned id = blockIdx.x;
  do {
    int t, ntile;
    if ((nPix & 7u) == 0) {   // ids dealt over the 8 XCDs as in igemm_conv_kernel
      const unsigned x = id & 7u, sl = id >> 3;
      ntile = (int)(sl % nNTall);
      t = (int)(x * (nPix >> 3) + sl / nNTall);
    } else {
      t = (int)(id % nPix);
      ntile = (int)(id / nPix);
    }
    const int tx0 = (t % tilesX) * 16;
    t /= tilesX;
    const int ty0 = (t % tilesY) * C::TH;
    const int b = t / tilesY;
    const long out_goff = 0;
    const int n0 = ntile * NT;
    // descriptor at the pixel one row and one column before the item's tile origin, formed in 64 bits per item (b, ty0
    // and tx0 are wave-uniform: scalar work): every in-image piece has a non-negative offset from it, and what stays in
    // the 32-bit vector and scalar offsets is one halo tile plus the channel row (dg_conv_wino_supported bounds it) --
    // a sample may lie any distance from the view's origin.  (sY and sX fit an int, the same bound: their products
    // are 32 x 32 -> 64-bit scalar multiplications)
    const float* const xorg = a.in.p + ((long)b * a.in.sB + (long)(ty0 - 1) * (int)a.in.sY + (long)(tx0 - 1) * (int)a.in.sX);
    const unsigned long long xu = (unsigned long long)xorg;
    // (unsigned locals: readfirstlane returns int, and a low half with bit 31 set would sign-extend into the high one)
    const unsigned xlo = __builtin_amdgcn_readfirstlane((unsigned)xu), xhi = __builtin_amdgcn_readfirstlane((unsigned)(xu >> 32));
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)xhi << 32) | xlo), 0, 0x7FFFFFFF, 0x00020000);
    // in the image or not is decided once per item and piece: the chunk loop issues the same NXP DMA instructions for
    // interior and border items, with no test (the hardware returns zeros for the sentinel, as for the padding slots)
    int xvi[NXP];
#pragma unroll
    for (int i = 0; i < NXP; ++i) {
      const int iy = ty0 + (xyx[i] >> 8) - 1, ix = tx0 + (xyx[i] & 255) - 1;
      xvi[i] = ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) ? xvo[i] : SENT;
    }
    // scalar byte offset of the chunk staged next, from the item's descriptor base: the channel, one addition per chunk.
    // Gathered K (ConvArgs::cpt): run t of cpt chunks starts at in_run_off[t], formed when the run starts
    int xso = GATH ? 4 * (int)a.in_run_off[0] : 0;
    int grun = 0, gleft = GATH ? a.cpt : 0;
    auto next_chunk = [&]() {
      if constexpr (GATH) {
        if (--gleft == 0) {
          ++grun;
          gleft = a.cpt;
          xso = 4 * (int)a.in_run_off[grun];
        } else {
          xso += 4 * WN_CK;
        }
      } else {
        xso += 4 * WN_CK;
      }
    };
    auto stage_dma = [&](auto buf_tag) {   // the chunk at xso -> ring slot BUF (a constant m0 per slot and piece)
      constexpr int BUF = decltype(buf_tag)::value;
      float* xs = smem + BUF * WN_RAW + wbase;
#pragma unroll
      for (int i = 0; i < NXP; ++i) {
        // (a plain int local: with a type-dependent argument such as xvi[i] hipcc drops the host-side instantiation
        // of the kernel without a diagnostic)
        const int vo = xvi[i];
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(xs + i * 1024), 16, vo,
                                                 xso, 0, 0);
      }
    };

    // no zeroing pass: the first MFMA of every accumulator (chunk 0, j = 0) takes a constant-zero C operand -- 64 MT
    // vector moves per item less on a pipe where every vector instruction costs its issue time next to the MFMAs
    acc_t acc[4][MT];

    // this wave's weight fragments: a scalar base that advances by one chunk's panel, and the lane's byte offset in it
    const float* wsp = a.w + (size_t)ntile * nCC * (16 * NT * WN_CK);
    // the first chunk of the item (no DMA of the previous item is in flight: its last chunk waited for everything, and
    // the end-of-item barrier is behind us)
    if (!(ABL & 8)) stage_dma(WnSlot<0>{});
    // One text, instantiated per (first chunk, ring slot, last chunk): with two buffers nothing else varies from chunk
    // to chunk, so in the steady state the slot is an immediate offset of the transform's reads and a constant m0 of the
    // DMA, both waits are immediates and nothing in the body branches.  slot_tag -1: the slot is rt_slot; last_tag 1 /
    // 0: the item's last chunk or not, -1: rt_last says (both once per item)
    int rt_slot = 0;
    bool rt_last = false;
    auto chunk = [&](auto first_tag, auto slot_tag, auto last_tag) {
      constexpr bool FIRST = decltype(first_tag)::value;
      constexpr int SLOT = decltype(slot_tag)::value, LASTT = decltype(last_tag)::value;
      constexpr bool LAST = LASTT == 1;
      static_assert(NBUF == 2 && (SLOT == 0 || SLOT == 1 || SLOT == -1), "the walk below is written for two buffers");
      // this wave's weight fragments of the chunk: four frequencies x (32 channels x 8), in flight across the barrier and
      // the transform.  Loaded in an asm statement: next to a DMA in flight the compiler waits vmcnt(0) for the result of
      // any load it knows of, which would drain the ring in front of the MFMAs; these four are counted by hand
      f32x4 bq[4];
      {
        static_assert(3 * NT * WN_CK * sizeof(float) < 4096, "immediate offsets of the fragment loads");
        asm volatile(
            "global_load_dwordx4 %0, %4, %5\n\t"
            "global_load_dwordx4 %1, %4, %5 offset:1024\n\t"
            "global_load_dwordx4 %2, %4, %5 offset:2048\n\t"
            "global_load_dwordx4 %3, %4, %5 offset:3072"
            : "=&v"(bq[0]), "=&v"(bq[1]), "=&v"(bq[2]), "=&v"(bq[3])
            : "v"(wvo), "s"(wsp)
            : "memory");
        static_assert(NT * WN_CK * sizeof(float) == 1024, "the offsets above");
        wsp += 16 * NT * WN_CK;
      }
      // this wave's DMA pieces of this chunk have landed: vector-memory instructions complete in order, and younger than
      // them are only the four loads above (the next chunk is issued behind the barrier).  (The compiler does not know
      // that the DMA writes LDS: the wait is explicit)
      wn_wait_vm<4>();
      // ... and so have everybody else's -- the only barrier of the chunk.  The bare instruction: __syncthreads() fences,
      // and the fence drains vmcnt while a DMA is in flight.  Nothing else needs the fence: a wave's LDS reads of the
      // previous chunk have returned before its MFMAs of that chunk took them
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // the other slot was last read by the transform of the previous chunk: every wave is past this chunk's barrier
      if constexpr (LASTT == 0) {
        next_chunk();
        if (!(ABL & 8)) stage_dma(WnSlot<1 - SLOT>{});
      } else if constexpr (LASTT == -1) {
        if (!rt_last) {
          next_chunk();
          if (!(ABL & 8)) stage_dma(WnSlot<1 - SLOT>{});
        }
      }
      const char* raw = reinterpret_cast<const char*>(smem + (SLOT < 0 ? rt_slot : SLOT) * WN_RAW);
      // ---- input transform: raw -> vr[mt][b] = V[(wave, b)][32 mt + r][4h .. 4h + 3], the lane's own MFMA operands ----
      // (in channel pairs, the packed fp32 forms of the vector ALU: the pair is (k, k + 1) of one 16-byte read, so nothing
      // moves between registers -- left to itself the compiler pairs across the columns j and pays 24 moves per task)
      f32x2 vr[MT][4][2];
      if (ABL & 2) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int bb = 0; bb < 4; ++bb) vr[i][bb][0] = vr[i][bb][1] = f32x2{0.f, 0.f};
      }
#pragma unroll
      for (int i = 0; i < ((ABL & 2) ? 0 : MT); ++i) {
        const f32x2 s2 = {tS[i], tS[i]};
        f32x2 tc[4][2];
        // all eight reads of the task in flight before the first addition waits for one (the scheduler's own order is
        // four round trips of two reads each)
        f32x4 xs[4], ys[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xs[j] = *reinterpret_cast<const f32x4*>(raw + tA[i][j]);
          ys[j] = *reinterpret_cast<const f32x4*>(raw + tB[i][j]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 x = xs[j], y = ys[j];
          tc[j][0] = __builtin_elementwise_fma(f32x2{y[0], y[1]}, s2, f32x2{x[0], x[1]});   // exact: s = +-1
          tc[j][1] = __builtin_elementwise_fma(f32x2{y[2], y[3]}, s2, f32x2{x[2], x[3]});
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          vr[i][0][p] = tc[0][p] - tc[2][p];
          vr[i][1][p] = tc[1][p] + tc[2][p];
          vr[i][2][p] = tc[2][p] - tc[1][p];
          vr[i][3][p] = tc[1][p] - tc[3][p];
        }
      }
      // the weight fragments have landed, their latency spent under the barrier and the transform.  In-order completion:
      // this also completes every DMA issued before them; only the one issued behind this chunk's barrier stays in flight.
      // The transform's results are operands of an empty statement in front of the wait (its additions stay above it,
      // where they would otherwise be free to sink to their first use), the fragments of one behind it (nothing that
      // reads them moves above it)
#pragma unroll
      for (int i = 0; i < MT; ++i)
        asm volatile("" : "+v"(vr[i][0][0]), "+v"(vr[i][0][1]), "+v"(vr[i][1][0]), "+v"(vr[i][1][1]), "+v"(vr[i][2][0]),
                          "+v"(vr[i][2][1]), "+v"(vr[i][3][0]), "+v"(vr[i][3][1]));
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (LASTT == -1) {
        if (rt_last) wn_wait_vm<0>();
        else wn_wait_vm<NXI>();
      } else {
        wn_wait_vm<LAST ? 0 : NXI>();
      }
      asm volatile("" : "+v"(bq[0]), "+v"(bq[1]), "+v"(bq[2]), "+v"(bq[3])::"memory");
      // ---- 16 GEMMs, this wave's four: 16 MT MFMAs on the operands formed just above ----
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            if (!(ABL & 4)) {
              if (FIRST && j == 0) {
                const acc_t zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                acc[f][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[f][j], vr[mt][f][j >> 1][j & 1], zero, 0, 0, 0);
              } else {
                acc[f][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[f][j], vr[mt][f][j >> 1][j & 1], acc[f][mt], 0, 0, 0);
              }
            } else {
              if (FIRST && j == 0) acc[f][mt] = acc_t{};
              acc[f][mt][j] += bq[f][j] * vr[mt][f][j >> 1][j & 1];
            }
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // the item's walk: the first chunk (slot 0; whether it is also the last is a run-time test, once per item); the
    // steady state two chunks a round (slot 1, slot 0: one counter, one branch); one more slot-1 chunk if the count is
    // odd; the last chunk, which issues no DMA and waits for everything, with its slot a run-time scalar.  Every step
    // updates the accumulators in place on ONE path: with a body per parity on either side of an if / else the
    // compiler keeps two sets of accumulators and spills (35 ... 250 registers, profiles/wino_straightline_experiments.md)
    {
      const std::true_type yes;
      const std::false_type no;
      const WnSlot<1> last;
      const WnSlot<0> more;
      const WnSlot<-1> rt;
      rt_last = nCC == 1;
      chunk(yes, WnSlot<0>{}, rt);
      if (nCC > 1) {
#pragma unroll 1
        for (int k = (nCC - 2) >> 1; k > 0; --k) {
          chunk(no, WnSlot<1>{}, more);
          chunk(no, WnSlot<0>{}, more);
        }
        if (nCC & 1) chunk(no, WnSlot<1>{}, more);
        rt_slot = (nCC - 1) & 1;
        chunk(no, rt, last);
      }
    }

    if (ABL & 1) {   // keep the accumulators alive with one store that never happens
      float sacc = 0.f;
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int j = 0; j < 16; ++j) sacc += acc[f][mt][j];
      if (sacc == 12345.678f) a.out.p[tid] = sacc;
      __syncthreads();
      continue;
    }
    // ---- output transform, first half (this wave's row a = wv: the four b's -> the two output columns q) ----
    // run from inside the fused epilogue (EPI_STAGE_LATE): after its per-item constant loads have been issued
    auto zstage = [&]() {
      // every wave is done with the last chunk's raw image, and no DMA is in flight (the last chunk issued none and
      // waited for all): the Z exchange may overwrite the ring
      __syncthreads();
      float* zw = smem + (2 * wv) * WN_ZPLANE + r * WN_CP + 4 * h;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 z0, z1;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float m0 = acc[0][mt][4 * g + k], m1 = acc[1][mt][4 * g + k], m2 = acc[2][mt][4 * g + k],
                        m3 = acc[3][mt][4 * g + k];
            z0[k] = (m0 + m1) + m2;
            z1[k] = (m1 - m2) - m3;
          }
          *reinterpret_cast<f32x4*>(zw + mt * (32 * WN_CP) + 8 * g) = z0;
          *reinterpret_cast<f32x4*>(zw + WN_ZPLANE + mt * (32 * WN_CP) + 8 * g) = z1;
        }
      __syncthreads();
    };
    // second half inside the fused epilogue: pixel (py, px) of the wave's 4 x 16 block is output (py & 1, px & 1) of
    // tile (2 wv + py / 2, px / 2); even rows Z[0] + Z[1] + Z[2], odd rows Z[1] - Z[2] - Z[3]
#define EPI_PRE_SYNC
#define EPI_STAGE
#define EPI_STAGE_LATE zstage()
#define EPI_NPASS (4 * MT)
#define EPI_OYW (ty0 + 2 * MT * __builtin_amdgcn_readfirstlane(wv))
#define EPI_FULL ((ty0 + C::TH <= a.H) && (tx0 + 16 <= a.W))
#define EPI_FETCH(v, py, px)                                                                                         \
  {                                                                                                                  \
    const float* zb = smem + ((px)&1) * WN_ZPLANE +                                                                  \
                      ((MT * __builtin_amdgcn_readfirstlane(wv) + ((py) >> 1)) * 8 + ((px) >> 1)) * WN_CP + c4;       \
    const f32x4 za = *reinterpret_cast<const f32x4*>(zb + (((py)&1) ? 2 : 0) * WN_ZPLANE);                           \
    const f32x4 zb1 = *reinterpret_cast<const f32x4*>(zb + (((py)&1) ? 4 : 2) * WN_ZPLANE);                          \
    const f32x4 zc = *reinterpret_cast<const f32x4*>(zb + (((py)&1) ? 6 : 4) * WN_ZPLANE);                           \
    _Pragma("unroll") for (int k_ = 0; k_ < 4; ++k_) v[k_] = ((py)&1) ? (za[k_] - zb1[k_]) - zc[k_] : (za[k_] + zb1[k_]) + zc[k_]; \
  }
#define EPI_HEAD HEAD
#define EPI_CLASS WnEpi<EC>
#include "igemm_epilogue.inc"
#undef EPI_CLASS
#undef EPI_HEAD
#undef EPI_FETCH
#undef EPI_FULL
#undef EPI_OYW
#undef EPI_NPASS
#undef EPI_STAGE_LATE
#undef EPI_STAGE
#undef EPI_PRE_SYNC
    // the next item's first raw tile overwrites the Z planes (keeping raw buffer 0 apart from them -- 46.5 KB for 8-row
    // tiles, still three workgroups per CU -- and dropping this barrier measured neutral: 3230 -> 3218 us over the
    // twelve shapes, inside the run-to-run spread)
    if (PERS) __syncthreads();
  } while (PERS && (id += gridDim.x) < nPix * nNTall);
}

template <int MT, bool PERS, int EC>
__global__ __launch_bounds__(256, WnCfg<MT>::WGS_PER_CU) void wino_conv_kernel(const ConvArgs a) {
  wino_body<MT, PERS, false, false, 0, EC>(a);
}
template <bool PERS, int EC>
__global__ __launch_bounds__(256, 2) void wino_conv_head_kernel(const ConvArgs a) {
  wino_body<2, PERS, true, false, 0, EC>(a);
}
template <int MT, bool PERS>
__global__ __launch_bounds__(256, WnCfg<MT>::WGS_PER_CU) void wino_conv_gathered_kernel(const ConvArgs a) {
  wino_body<MT, PERS, false, true>(a);
}
#ifdef DEPGAN_WINO_ABLATIONS
template <int MT, int ABL>
__global__ __launch_bounds__(256, WnCfg<MT>::WGS_PER_CU) void wino_conv_abl_kernel(const ConvArgs a) {
  wino_body<MT, true, false, false, ABL>(a);
}
#endif

// Every instantiation a launch can take, with the name rocprofv3 prints for it and its LDS size: wino_pick() is the one
// place that maps a launch to an entry
#define WN_FN(...) reinterpret_cast<const void*>(&__VA_ARGS__)
#define WN_K8(EC)                                                                                \
  {{WN_FN(wino_conv_kernel<1, false, EC>), "wino_conv_kernel<1,false," #EC ">", WnCfg<1>::LDS}, \
   {WN_FN(wino_conv_kernel<1, true, EC>), "wino_conv_kernel<1,true," #EC ">", WnCfg<1>::LDS}},
const DgKernel kWn8[WN_HEAD_CLASS][2] = {WN_K8(0) WN_CLASSES8(WN_K8)};   // [class][persistent]
#undef WN_K8
const DgKernel kWn16[2] = {{WN_FN(wino_conv_kernel<2, false, 0>), "wino_conv_kernel<2,false,0>", WnCfg<2>::LDS},
                           {WN_FN(wino_conv_kernel<2, true, 0>), "wino_conv_kernel<2,true,0>", WnCfg<2>::LDS}};
const DgKernel kWnHead[2][2] = {   // [generic / head class][persistent]
    {{WN_FN(wino_conv_head_kernel<false, 0>), "wino_conv_head_kernel<false,0>", WnCfg<2>::LDS},
     {WN_FN(wino_conv_head_kernel<true, 0>), "wino_conv_head_kernel<true,0>", WnCfg<2>::LDS}},
    {{WN_FN(wino_conv_head_kernel<false, WN_HEAD_CLASS>), "wino_conv_head_kernel<false,10>", WnCfg<2>::LDS},
     {WN_FN(wino_conv_head_kernel<true, WN_HEAD_CLASS>), "wino_conv_head_kernel<true,10>", WnCfg<2>::LDS}}};
static_assert(WN_HEAD_CLASS == 10, "the names above");
const DgKernel kWnGath[2][2] = {   // [MT - 1][persistent]
    {{WN_FN(wino_conv_gathered_kernel<1, false>), "wino_conv_gathered_kernel<1,false>", WnCfg<1>::LDS},
     {WN_FN(wino_conv_gathered_kernel<1, true>), "wino_conv_gathered_kernel<1,true>", WnCfg<1>::LDS}},
    {{WN_FN(wino_conv_gathered_kernel<2, false>), "wino_conv_gathered_kernel<2,false>", WnCfg<2>::LDS},
     {WN_FN(wino_conv_gathered_kernel<2, true>), "wino_conv_gathered_kernel<2,true>", WnCfg<2>::LDS}}};
#ifdef DEPGAN_WINO_ABLATIONS
// tools/build_wino_abl.sh: DEPGAN_WINO_ABL=<N> takes the ablated persistent instantiation N of either form
constexpr int kWnAblN[] = {1, 2, 3, 4, 8, 10, 11};
#define WN_ABL(MT, N) {WN_FN(wino_conv_abl_kernel<MT, N>), "wino_conv_abl_kernel<" #MT "," #N ">", WnCfg<MT>::LDS},
#define WN_ABLS(MT) {WN_ABL(MT, 1) WN_ABL(MT, 2) WN_ABL(MT, 3) WN_ABL(MT, 4) WN_ABL(MT, 8) WN_ABL(MT, 10) WN_ABL(MT, 11)}
const DgKernel kWnAbl[2][7] = {WN_ABLS(1), WN_ABLS(2)};   // [MT - 1][index in kWnAblN]
#undef WN_ABLS
#undef WN_ABL
#endif
#undef WN_FN

// DEPGAN_EPI_CLASSES=0: every launch takes the generic kernel (A/B); depgan_set_epilogue_classes overrides it
int g_epi_classes = -1;

}  // namespace

void dg_set_epi_classes(int on) { g_epi_classes = on ? 1 : 0; }
int dg_get_epi_classes() {
  if (g_epi_classes < 0) {
    const char* e = getenv("DEPGAN_EPI_CLASSES");
    g_epi_classes = (e && atoi(e) == 0) ? 0 : 1;
  }
  return g_epi_classes;
}

unsigned dg_epilogue_flags(const Epilogue& e) {
  return (e.bias ? DG_EPF_BIAS : 0u) | (e.scale ? DG_EPF_AFFINE : 0u) | (e.film_mul ? DG_EPF_FILM : 0u) |
         (e.relu ? DG_EPF_RELU : 0u) | (e.out_pre.p ? DG_EPF_PRE : 0u) | (e.res.p ? DG_EPF_RES : 0u) |
         (e.mask.p ? DG_EPF_MASK : 0u) | (e.pool.p ? DG_EPF_POOL : 0u) | (e.accumulate ? DG_EPF_ACCUM : 0u) |
         (e.head_out ? DG_EPF_HEAD : 0u);
}

int dg_wino_epi_class(unsigned flags, int form) {
  if (!dg_get_epi_classes()) return 0;
  if (form == 1) return flags == kWnClassMask[WN_HEAD_CLASS] ? WN_HEAD_CLASS : 0;
  if (form != 0) return 0;
  for (int i = 1; i < WN_HEAD_CLASS; ++i)
    if (kWnClassMask[i] == flags) return i;
  return 0;
}

bool dg_conv_wino_supported(const ConvPlan& pl, const ConvArgs& a) {
  if (!dg_plan_wino(pl)) return false;
  if (a.Cin != pl.Cin || (a.Cin % WN_CK) || (a.Cout % 32) || a.groups > 1 || a.dbg || ((a.H | a.W) & 1)) return false;
  if (a.cpt > 0 && ((a.Cin % (a.cpt * WN_CK)) != 0 || a.Cin / (a.cpt * WN_CK) > 4)) return false;
  // Input addressing: a 64-bit descriptor base per item (sample and tile origin), 32-bit byte offsets inside it.  What
  // the offsets span is one halo tile plus the channel row and the largest run offset; the 16-row form bounds both
  // forms.  No layout of the model comes near 2 GiB here; the sample stride is not part of it
  long run = 0;
  for (int t = 0; a.cpt > 0 && t < a.Cin / (a.cpt * WN_CK); ++t) {
    if (a.in_run_off[t] < 0) return false;
    run = a.in_run_off[t] > run ? a.in_run_off[t] : run;
  }
  constexpr long lim = 1L << 29;   // 2^31 bytes in floats; each term below it first, so that the sum cannot overflow
  if (a.in.sY < 0 || a.in.sX < 0 || a.in.sY >= lim || a.in.sX >= lim || run >= lim) return false;
  if ((WnCfg<2>::TH + 2) * a.in.sY + WN_TW * a.in.sX + a.Cin + run >= lim) return false;
  return true;
}

// MT of a launch: DEPGAN_WINO_MT=1|2 forces one form for A/B runs; the fused head exists for MT = 2 only
static int wino_mt(const ConvArgs& a) {
  static int forced = -1;
  if (forced < 0) {
    const char* e = getenv("DEPGAN_WINO_MT");
    forced = e ? atoi(e) : 0;
  }
  if (a.ep.head_out) return 2;
  if (forced == 1 || forced == 2) return forced;
  // 8-row tiles, three workgroups per CU: with ONE barrier per chunk (wave-private transform) the third wave per SIMD
  // pays -- sum over the step's twelve shapes 3246 us against 3335 us for 16-row tiles, never slower, up to 9 % faster
  // where 16-row tiles leave CUs without a workgroup (profiles/r03_conv_experiments.md)
  return 1;
}

// the instantiation of a launch: its form, then the epilogue class of its flag set
static const DgKernel* wino_pick(const ConvArgs& a, int mt, bool pers) {
  const int form = a.ep.head_out ? 1 : (a.cpt > 0 ? 3 : (mt == 2 ? 2 : 0));
  const int ec = dg_wino_epi_class(dg_epilogue_flags(a.ep), form);
  if (form == 1) return &kWnHead[ec ? 1 : 0][pers];
  if (form == 3) return &kWnGath[mt - 1][pers];
  if (form == 2) return &kWn16[pers];
  return &kWn8[ec][pers];
}

int dg_conv_wino_prepare(const ConvPlan& pl, const ConvArgs& a, DgConvLaunch* L) {
  if (!dg_conv_wino_supported(pl, a)) {
    dg_set_error("dg_conv_wino: shape not covered (3x3, Cin %% 8, Cout %% 32, even H and W, no groups, a halo tile of the input view within 2 GiB)");
    return DG_ERR_UNSUPPORTED;
  }
  const int mt = wino_mt(a);
  if (a.ep.head_out && (a.Cout != 32 || a.ep.pool.p || a.cpt > 0)) {
    dg_set_error("dg_conv_wino: the fused head needs 32 output channels, no fused pool and no gathered K");
    return DG_ERR_ARG;
  }
  L->a = a;
  L->a.lgx = cdiv(a.W, 16) * cdiv(a.H, mt == 2 ? WnCfg<2>::TH : WnCfg<1>::TH) * a.B;
  L->a.lgy = a.Cout / 32;
  const long total = (long)L->a.lgx * L->a.lgy;
  // resident workgroups per CU by LDS and registers; persistent when there are more items than that
  const long cap = (long)(mt == 2 ? WnCfg<2>::WGS_PER_CU : WnCfg<1>::WGS_PER_CU) * dg_cu_count();
  const bool pers = total > cap;
  L->k = wino_pick(a, mt, pers);
#ifdef DEPGAN_WINO_ABLATIONS
  if (const char* e = getenv("DEPGAN_WINO_ABL")) {
    const int abl = atoi(e);
    if (abl && pers && !a.ep.head_out && a.cpt <= 0) {
      L->k = nullptr;
      for (int i = 0; i < 7; ++i)
        if (kWnAblN[i] == abl) L->k = &kWnAbl[mt - 1][i];
      if (!L->k) { dg_set_error("DEPGAN_WINO_ABL=%d not instantiated", abl); return DG_ERR_ARG; }
    }
  }
#endif
  L->grid = (unsigned)(pers ? cap : total);
  L->block = 256;
  L->lds = (size_t)L->k->attr_lds;
  return DG_OK;
}
