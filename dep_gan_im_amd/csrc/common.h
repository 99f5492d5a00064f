// Shared declarations for the DEP-GAN hot-path HIP library (gfx950 / MI355X).
//
// Data layout: every activation is NHWC fp32 with the channel dimension
// contiguous; a TView carries (batch, row, pixel) strides in floats so one
// kernel serves plain tensors, channel slices of a concat buffer (reference
// concatenate() at GT:450/465/479 is never materialised twice) and the 2x
// strided pixel grids of the 2x2/stride-2 transposed convolution (GT:308).
// The one exception: the opt-in generator forward with bf16 activation storage
// (bf16s.h) keeps its inter-layer activations as NHWC bf16 behind a TViewH.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct TView {
  float* p;
  long sB, sY, sX;  // strides in floats; channel stride is 1
};

static inline TView make_view(float* p, int H, int W, int C) {
  TView v;
  v.p = p;
  v.sX = C;
  v.sY = (long)W * C;
  v.sB = (long)H * W * C;
  return v;
}
// channel slice [c0, ...) of a tensor with Ctot channels
static inline TView make_view_slice(float* p, int H, int W, int Ctot, int c0) {
  TView v = make_view(p, H, W, Ctot);
  v.p = p + c0;
  return v;
}
static inline TView null_view() {
  TView v;
  v.p = nullptr;
  v.sB = v.sY = v.sX = 0;
  return v;
}

// bf16 activation storage (generator forward of a bf16_mfma context, bf16s.h): the same three strides, counted in
// ELEMENTS of 2 bytes; channel stride 1.  A second type next to TView, so that no fp32 call site changes.
struct TViewH {
  __bf16* p;
  long sB, sY, sX;  // strides in bf16 elements; channel stride is 1
};

static inline TViewH make_view_h(__bf16* p, int H, int W, int C) {
  TViewH v;
  v.p = p;
  v.sX = C;
  v.sY = (long)W * C;
  v.sB = (long)H * W * C;
  return v;
}
// channel slice [c0, ...) of a tensor with Ctot channels
static inline TViewH make_view_slice_h(__bf16* p, int H, int W, int Ctot, int c0) {
  TViewH v = make_view_h(p, H, W, Ctot);
  v.p = p + c0;
  return v;
}
static inline TViewH null_view_h() {
  TViewH v;
  v.p = nullptr;
  v.sB = v.sY = v.sX = 0;
  return v;
}

// Fused epilogue description, applied in this order to acc (the raw contraction):
//   v = (acc + bias[co]) * scale[co] + shift[co]   (phase-0 BatchNorm affine; the MFMA kernels
//                                          evaluate it as fma(acc, scale, bias * scale + shift): one rounding)
//   out_pre = v                            (pre-FiLM tensor kept for the G backward)
//   v = v * film_mul[b,co] + film_add[b,co]  (GT:403-404)
//   v = max(v, 0)                          (relu)
//   v += res                               (residual add GT:407, or a gradient join)
//   v *= (mask > 0)                        (ReLU mask of the consumer side in backward passes)
//   out = accumulate ? out + v : v
struct Epilogue {
  const float* bias;
  const float* scale;
  const float* shift;
  const float* film_mul;
  const float* film_add;
  int film_ld;  // row stride (floats) of film_mul / film_add
  TView out_pre;
  TView res;
  TView mask;
  int relu;
  int accumulate;
  // igemm only: when pool.p is non-null the 2x2 / stride-2 max-pool of the final output is written here as well
  // (view of (H/2, W/2) pixels; H and W must be even).  Saves the pooling pass its read of the whole output.
  TView pool;
  // igemm, 32-channel layers only (the 8-channel-chunk 3x3 kernel): when head_out is non-null the 1x1 convolution to ONE
  // channel that follows (gen_segmentation after gen_17, GT:494-495) rides in this launch: head_out[pixel] =
  // act(sum_c out[pixel][c] head_w[c] + head_b[0]), act = tanh when head_tanh.  head_skip_out: the 32-channel output
  // itself is not stored (forward-only passes, where the head is its only consumer).
  const float* head_w;
  const float* head_b;
  float* head_out;
  int head_tanh, head_skip_out;
};

struct ConvArgs {
  TView in;
  TView out;
  const float* w;  // packed (igemm) or strided (direct) weights
  int B, H, W, Cin, Cout;
  Epilogue ep;
  // direct kernel only: weight element (tap, ci, co) = w[tapidx*wsT + ci*wsI + co*wsO],
  // tapidx = flip ? ntaps-1-tap : tap
  long wsT, wsI, wsO;
  int flip;
  int vec4;  // direct kernel: all output-side views 16-byte aligned (set by the launcher)
  // diagnostics: when non-null, thread 0 of every workgroup writes 8 x u64 phase stamps here
  unsigned long long* dbg;
  // igemm only: grouped launch.  groups > 1 runs `groups` convolutions that share the input and the epilogue
  // constants in ONE launch (the 4 taps of a 2x2 / stride-2 transposed convolution): group g uses the packed weights
  // w_group[g] and writes to out.p + out_group_off[g]; `w` is ignored.  0 or 1: a single convolution.
  int groups;
  int lgx, lgy;   // igemm: logical grid (pixel tiles, channel tiles x groups), filled by the launcher
  const float* w_group[4];
  long out_group_off[4];
  // igemm only: gathered K.  cpt > 0 splits the Cin axis into consecutive runs of cpt channel chunks; run r reads its
  // channels at in.p + in_run_off[r] (floats) instead of contiguously after run r-1 -- the backward-data of the
  // 2x2 / stride-2 transposed convolution as ONE 1x1 convolution over the four strided pixel grids of its upstream
  // gradient (K = 4 Cout).  The run length cpt * CK must divide into whole chunks (no channel tail inside a run).
  int cpt;
  // the 5x5 kernels only (igemm_ws5_kernel, the persistent igemm_conv_kernel<., 5, ., 25, true>): the epilogue class of
  // this launch's flag set (dg_conv5_epi_class), filled by the launcher; 0 = the body that reads the flags at run time.
  // (In the four bytes that padded cpt: no other field moves and the struct keeps its size.)
  int epi_class;
  long in_run_off[4];
};

struct WgradArgs {
  TView x;      // operand shifted by the tap ('same' padding)
  TView dy;     // operand at the output pixel
  float* part;  // [nchunks][ntaps][Cin][Cout] partial sums
  int B, H, W, Cin, Cout;
  int nTiles, tilesPerChunk;
  // MFMA kernel only: when non-null, the column sums of dy over the samples b < colB (bias / BN-beta gradients) ride
  // along: the workgroups of input-channel tile 0 / tap group 0 write one partial row per chunk, [nchunks][Cout]
  float* colpart;
  int colB;
};

// One v_max_f32.  fmaxf() compiles to two: IEEE maxNum has to quiet a signalling NaN, so the compiler first
// canonicalises every operand it cannot prove canonical (v_max_f32 x, x, x).  On a SIMD every vector instruction costs
// its issue time next to the fp32 MFMAs: the 32 extra ones per ReLU'd 64x32 wave tile are not free.
// For non-NaN operands the result is bit-identical.
#ifdef __HIPCC__
static __device__ __forceinline__ float dg_vmax(float a, float b) {
  float o;
  asm("v_max_f32 %0, %1, %2" : "=v"(o) : "v"(a), "v"(b));
  return o;
}
#endif

#define DG_OK 0
#define DG_ERR_ARG 1
#define DG_ERR_HIP 2
#define DG_ERR_UNSUPPORTED 3

void dg_set_error(const char* fmt, ...);

#define HIPCHECK(expr)                                                              \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess) {                                                         \
      dg_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return DG_ERR_HIP;                                                            \
    }                                                                               \
  } while (0)

#define DGCHECK(expr)          \
  do {                         \
    int _r = (expr);           \
    if (_r != DG_OK) return _r; \
  } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Launcher-side state that belongs to a DEVICE, not to the process: a kernel's dynamic-LDS attribute, its occupancy, the
// CU count.  A process may hold contexts on several GPUs (Engine(device=...)): function-local statics would give the
// second device the first one's numbers and never set its attributes.
#define DG_MAX_DEVICES 64
static inline int dg_device_slot() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= DG_MAX_DEVICES) return -1;
  return d;
}
struct DgOncePerDevice {   // `if (once.need()) { set attribute ... }`; a device beyond the table is set every time
  bool done[DG_MAX_DEVICES] = {};
  bool need() {
    const int d = dg_device_slot();
    if (d < 0) return true;
    if (done[d]) return false;
    done[d] = true;
    return true;
  }
};
// One kernel instantiation a launcher can take: its address, the name rocprofv3 prints for it, and the
// MaxDynamicSharedMemorySize it needs (0 = none).  The attribute belongs to the ENTRY, not to a launch: the wave-private
// kernels launch with LDS sizes that depend on Cin and the wave count, and all of them must fit what was set once.
// Every conv launcher keeps a static table of these; the launch and the reported name read the same entry.
struct DgKernel {
  const void* fn;
  const char* name;
  int attr_lds;
  mutable DgOncePerDevice once = {};
};
// the attribute, once per (device, entry)
static inline int dg_kernel_ready(const DgKernel& k) {
  if (k.attr_lds && k.once.need()) HIPCHECK(hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.attr_lds));
  return DG_OK;
}
// args: the kernel's one by-value argument struct
static inline int dg_launch(const DgKernel& k, unsigned grid, unsigned block, size_t lds, const void* args, hipStream_t st,
                            unsigned grid_y = 1) {
  DGCHECK(dg_kernel_ready(k));
  void* kargs[] = {const_cast<void*>(args)};
  HIPCHECK(hipLaunchKernel(k.fn, dim3(grid, grid_y), dim3(block), kargs, lds, st));
  HIPCHECK(hipGetLastError());
  return DG_OK;
}
static inline int dg_cu_count() {   // CUs of the current device, asked once per device (the query is slower than a launch)
  static int cus[DG_MAX_DEVICES] = {};
  const int d = dg_device_slot();
  if (d >= 0 && cus[d]) return cus[d];
  int n = 256;
  hipDeviceProp_t p;
  if (d >= 0 && hipGetDeviceProperties(&p, d) == hipSuccess && p.multiProcessorCount > 0) n = p.multiProcessorCount;
  if (d >= 0) cus[d] = n;
  return n;
}

// ---- conv plans -----------------------------------------------------------
// How one convolution maps on the MFMA implicit-GEMM kernels: the kernel family, and within it the instantiation that
// the fields MF / KS / CK select.
enum ConvFamily {
  CONV_DIRECT = 0,  // not MFMA-eligible: the direct kernel on the raw HWIO tensor (no packed panel)
  CONV_TILE,        // fp32 workgroup-tile kernels (igemm_conv.hip; the wave-private kernels read the same panels)
  CONV_WINO,        // Winograd F(2x2,3x3) (igemm_wino.hip): panel [nt][chunk][16 frequencies][32][8] of G g G^T
  CONV_BF16,        // bf16 matrix pipe (igemm_bf16.hip): panels are packed as bf16, the activation operand is rounded
                    // to bf16 while it is staged, accumulation stays fp32
  CONV_SPLIT,       // fp32 operands split into `planes` bf16 terms each (igemm_split_kernel)
};
struct ConvPlan {
  int KS, Cin, Cout;
  int MF;    // MFMA tile edge: 32 (v_mfma_f32_32x32x2_f32) or 16 (v_mfma_f32_16x16x4_f32); bf16 plans: 32x32x16 or 16x16x32
  int NT;    // output channels per workgroup
  int CK;    // input channels staged per LDS chunk
  int nNT, nCC;
  size_t packedFloats;  // size of the packed panel in 4-byte units (bf16 plans: two elements per unit)
  ConvFamily family;
  int planes;           // bf16 terms per packed element: 0 for fp32, 1 for bf16, 2 or 3 for split
  // taps of the packed panel [nt][cc][tap][n][k]: the kernel's, or the 16 Winograd "frequencies"
  int ntaps() const { return family == CONV_WINO ? 16 : KS * KS; }
  // split panels: taps per staged group of [nt][cc][tap group][plane][tap][n][k = 16]
  int tapg() const { return KS == 5 ? 5 : KS * KS; }
};
static inline bool dg_plan_mfma(const ConvPlan& pl) { return pl.family != CONV_DIRECT; }
static inline bool dg_plan_bf16(const ConvPlan& pl) { return pl.family == CONV_BF16; }
static inline bool dg_plan_split(const ConvPlan& pl) { return pl.family == CONV_SPLIT; }
static inline bool dg_plan_wino(const ConvPlan& pl) { return pl.family == CONV_WINO; }
// the 8-channel-chunk 3x3 tile plan (dg_plan_conv_items) and the 5x5 tile plans (32x5x8 and 16x5x16)
static inline bool dg_plan_tile3_ck8(const ConvPlan& pl) { return pl.family == CONV_TILE && pl.KS == 3 && pl.CK == 8; }
static inline bool dg_plan_tile5(const ConvPlan& pl) { return pl.family == CONV_TILE && pl.KS == 5; }
// the plan of a convolution that runs on the direct kernel
static inline ConvPlan dg_plan_direct() {
  ConvPlan p = {};
  p.family = CONV_DIRECT;
  return p;
}
ConvPlan dg_plan_conv(int KS, int Cin, int Cout);
// ... knowing the number of work items of its launches (chunk size by launch size, see igemm_conv.hip)
ConvPlan dg_plan_conv_items(int KS, int Cin, int Cout, long items);
// the bf16 plan where the bf16 kernel covers the shape (Cout % 32 == 0, Cin >= 8), else the fp32 plan
ConvPlan dg_plan_conv_bf16(int KS, int Cin, int Cout);
// the 16-output-channel 5x5 form of the bf16 plan (MF = NT = 16, CK = 32): KS == 5, Cout % 16 == 0, Cin >= 8,
// Cin % 4 == 0; else the fp32 plan.  Opt-in per context (depgan_set_critic16_pipe) and operator path 10
ConvPlan dg_plan_conv_bf16_n16(int KS, int Cin, int Cout);
// fp32 operands split into `planes` (2 or 3) bf16 terms each, 3 or 6 products on the bf16 pipe (igemm_split_kernel)
ConvPlan dg_plan_conv_split(int KS, int Cin, int Cout, int planes);
// bytes of packed storage per element of the plain [nt][cc][tap][n][k] panel (split plans store `planes` planes of it)
static inline size_t dg_plan_elem_bytes(const ConvPlan& pl) { return pl.planes ? 2 * (size_t)pl.planes : 4; }

// One weight-packing job of a batched launch (dg_pack_weights_batch): what dg_pack_weights takes, plus an optional
// re-spacing of the channel-tile blocks in the destination (nt_stride elements between consecutive channel tiles;
// 0 = dense) so that several sources can be interleaved per channel tile.
struct PackJob {
  const float* src;
  float* dst;
  const float* kscale;
  int ntaps, srcI, srcO, io, transpose, flip;
  int NT, CK, nCC, Kdim, Ndim;
  int bf16;             // 1: dst is a bf16 panel (elements of 2 bytes, RNE from the fp32 source x kscale); 2 / 3: split
                        // panel of that many planes (plane p = bf16 of what planes < p left over), TAPG taps per group
  int tapg;             // split panels only: taps per staged group
  int wino;             // 1: Winograd panel -- ntaps = 16 "frequencies" f = 4a + b, element = (G g G^T)[a][b] of the 3x3 source
  unsigned total;       // packed elements of this job
  unsigned per_nt;      // packed floats per channel tile (nCC * ntaps * NT * CK)
  unsigned nt_stride;   // destination elements between channel tiles
  unsigned blk0, nblk;  // first block and number of blocks of this job inside the batched grid
};
int dg_pack_job(const ConvPlan& pl, const float* src, int srcI, int srcO, int io, int transpose, int flip,
                const float* kscale, float* dst, size_t nt_stride, PackJob* job);
// jobs_dev: device copy of the array (blk0 / nblk filled by dg_pack_layout on the host copy before the upload)
unsigned dg_pack_layout(PackJob* jobs_host, int njobs);
int dg_pack_weights_batch(const PackJob* jobs_dev, int njobs, unsigned nblocks, hipStream_t st);

// weight packing: src is HWIO (io=0) or HWOI (io=1, Conv2DTranspose layout)
// roles: if transpose==0 the GEMM K index is the source I axis and N the O axis
// (forward conv); if transpose==1 K is the source O axis and N the I axis
// (backward-data).  flip reverses the tap order.  kscale (optional) multiplies
// by a per-K-channel factor (BN scale folded into backward-data weights).
int dg_pack_weights(const ConvPlan& pl, const float* src, int srcI, int srcO, int io, int transpose, int flip,
                    const float* kscale, float* dst, hipStream_t st);

// ---- one prepared convolution launch (conv_select.hip) ----
// THE rule that says which kernel a convolution takes (dg_conv_prepare; host only, no launch, no allocation):
//   a plan that is not MFMA                 the direct kernels (direct.hip), profile class 2
//   else dg_conv_igemm_check, then by plan  CONV_BF16 / CONV_SPLIT (igemm_bf16.hip), CONV_WINO (igemm_wino.hip)
//   CONV_TILE                               wave-private 3x3 (opt-in), weight-stationary 5x5, else the tile instantiation
// `routes` says which of the CONV_TILE kernels may be taken: all of them (the model), the tile kernels only (the reference
// the others must match bit for bit), or ONE of the wave-private families without the tile bit -- forced: the shape test
// alone decides, and a launch it does not cover is refused.
enum { DG_ROUTE_TILE = 1, DG_ROUTE_WP = 2, DG_ROUTE_WS5 = 4, DG_ROUTE_ALL = 7 };
struct DgConvLaunch {
  const DgKernel* k;
  unsigned grid, grid_y, block;
  size_t lds;
  int klass;    // profile class: 0 MFMA, 2 direct
  ConvArgs a;   // lgx, lgy and vec4 filled
};
// the plan of one convolution of a context in the given mode: split or bf16 matrix pipe where configured and covered, else
// fp32 -- Winograd for the 3x3 layers it covers, else the tile plan with its chunk size by launch size.  N, H, W: the
// batch and spatial size the layer is planned for (0: unknown, as for the 1x1 layers)
ConvPlan dg_conv_plan(int f32_split, int bf16_mfma, int winograd, int KS, int Cin, int Cout, int N, int H, int W);
int dg_conv_prepare(const ConvPlan& pl, const ConvArgs& a, int KS, unsigned routes, DgConvLaunch* out);
int dg_conv_run(const DgConvLaunch& L, hipStream_t st);
// prepare and run with every route open: what the model launches for (pl, a)
int dg_conv_igemm(const ConvPlan& pl, const ConvArgs& a, hipStream_t st);
// Each family's own part of dg_conv_prepare: the entry of its table and the geometry of the launch
int dg_conv_direct_prepare(int KS, const ConvArgs& a, DgConvLaunch* out);
int dg_conv_tile_prepare(const ConvPlan& pl, const ConvArgs& a, DgConvLaunch* out);
int dg_conv_bf16_prepare(const ConvPlan& pl, const ConvArgs& a, DgConvLaunch* out);
int dg_conv_wino_prepare(const ConvPlan& pl, const ConvArgs& a, DgConvLaunch* out);
int dg_conv_wp_prepare(const ConvPlan& pl, const ConvArgs& a, DgConvLaunch* out);
int dg_conv_ws5_prepare(const ConvPlan& pl, const ConvArgs& a, DgConvLaunch* out);
// the argument checks of the MFMA launchers (alignment, fused pool, gathered K, fused head); sets the error text
int dg_conv_igemm_check(const ConvPlan& pl, const ConvArgs& a);
// wave-private 3x3 kernel (igemm_wp.hip): no workgroup barrier in steady state; reads the 8-channel-chunk plan's panel
bool dg_conv_igemm_wp_supported(const ConvPlan& pl, const ConvArgs& a, bool force);
// weight-stationary, wave-private 5x5 kernel (igemm_wp.hip): Cin, Cout in {16, 32}, one channel tile; reads the packed
// panel of the 5x5 tile plans as it is and is bit-identical to igemm_conv_kernel<., 5, ., 25>
bool dg_conv_igemm_ws5_supported(const ConvPlan& pl, const ConvArgs& a, bool force);
// the launch for (pl, a) can carry the fused one-channel head (Epilogue::head_*): 32 -> 32, 8-channel-chunk 3x3 kernel
bool dg_conv_igemm_head_supported(const ConvPlan& pl, const ConvArgs& a);
// Winograd F(2x2,3x3) kernel (igemm_wino.hip): plan family CONV_WINO, panel [nt][chunk][16 frequencies][32][8] of G g G^T
ConvPlan dg_plan_conv_wino(int Cin, int Cout);
bool dg_conv_wino_supported(const ConvPlan& pl, const ConvArgs& a);
// Epilogue classes of the Winograd kernel: instantiations whose epilogue flags are compile-time constants, one per flag
// set the model launches (the table in igemm_wino.hip).  The flag set of an Epilogue as a bit mask (DEPGAN_EPF_* of
// include/depgan.h), and the pure host function dg_conv_wino_prepare selects with: form 0 the 8-row
// kernel, 1 the fused-head kernel, 2 the 16-row kernel without head, 3 gathered K.  Class 0 is the generic kernel (run-time
// flags): any set outside the table, forms 2 and 3, and everything while the process-wide switch is off.
enum { DG_EPF_BIAS = 1, DG_EPF_AFFINE = 2, DG_EPF_FILM = 4, DG_EPF_RELU = 8, DG_EPF_PRE = 16, DG_EPF_RES = 32,
       DG_EPF_MASK = 64, DG_EPF_POOL = 128, DG_EPF_ACCUM = 256, DG_EPF_HEAD = 512, DG_EPF_ALL = 1023 };
unsigned dg_epilogue_flags(const Epilogue& e);
int dg_wino_epi_class(unsigned flags, int form);
void dg_set_epi_classes(int on);
int dg_get_epi_classes();
// Epilogue classes of the 5x5 kernels (igemm_ws5_kernel<32,8> / <16,16>, igemm_conv_kernel<32,5,8,25,true> /
// <16,5,16,25,true>; profiles/conv5_classes_experiments.md).  Their names, grids and LDS sizes are pinned, so a class is
// not an instantiation of the kernel but a body INSIDE it: once per wave, before the item loop, ConvArgs::epi_class
// selects the item loop compiled for that flag set (the EPI_CLASS hook of igemm_epilogue.inc); class 0 is the loop that
// reads the flags at run time, which every other flag set takes, and everything while the process-wide switch is off.
// The table is closed: the flag sets the model launches on these kernels (model.hip: d_forward, d_backward_chain, the
// u-forward of critic_enqueue).
constexpr int DG_CONV5_NCLASS = 5;
constexpr unsigned kConv5ClassMask[DG_CONV5_NCLASS] = {
    0,                                          // 0 generic (run-time flags)
    DG_EPF_BIAS | DG_EPF_RELU,                  // 1 critic 5x5 forward
    DG_EPF_BIAS | DG_EPF_RELU | DG_EPF_POOL,    // 2   ... with the fused pool
    DG_EPF_MASK,                                // 3 backward-data with a ReLU mask; the critics' u-forward
    0,                                          // 4 backward-data into a pooled layer: nothing
};
template <int EC>
struct Conv5Epi {
  static_assert(EC >= 0 && EC < DG_CONV5_NCLASS, "epilogue class");
  static constexpr unsigned M = kConv5ClassMask[EC];
  static constexpr bool fixed = EC != 0;
  static constexpr bool bias = M & DG_EPF_BIAS, affine = M & DG_EPF_AFFINE, film = M & DG_EPF_FILM, relu = M & DG_EPF_RELU,
                        pre = M & DG_EPF_PRE, res = M & DG_EPF_RES, msk = M & DG_EPF_MASK, pool = M & DG_EPF_POOL,
                        head = M & DG_EPF_HEAD;
};
// pure host function: the class id of a flag set (a mask of DG_EPF_*), 0 while the switch is off
int dg_conv5_epi_class(unsigned flags);
#ifdef __HIPCC__
// The kernel's one by-value ConvArgs, read again from the kernel-argument segment through a pointer the compiler cannot
// trace: the scalar loads of whatever fields the caller goes on to use stay where this is called (once per item, in
// front of the epilogue) instead of being hoisted to the kernel's entry, where the whole struct then has to live in
// SGPRs -- or, spilled, in VGPR lanes -- across the item loop.  Only for kernels whose sole argument is the ConvArgs.
static __device__ __forceinline__ void dg_reload_conv_args(ConvArgs* dst) {
  auto kp = __builtin_amdgcn_kernarg_segment_ptr();   // constant address space: the loads below are scalar
  asm volatile("" : "+s"(kp));
  __builtin_memcpy(dst, (const void*)kp, sizeof(ConvArgs));
}
#endif

// wgrad: returns number of chunks used through *nchunks; part must hold nchunks slabs of KS * KS * Cin * Cout floats
// (DgWgradChoice::part_floats).
int dg_wgrad(int KS, const WgradArgs& a, int* nchunks, hipStream_t st);
// out[(tap,ci,co)] (+)= scale[co] * sum_chunks part ; raw (optional) gets the unscaled sum.
// oi=1 writes [tap][co][ci] (Conv2DTranspose kernel layout) instead of [tap][ci][co].
// slab reduction and (colpart non-null) the column-sum finish of the same weight-gradient launch, as ONE launch
int dg_wgrad_finish(const float* part, int nchunks, int ntaps, int Cin, int Cout, const float* scale, float* out,
                    float* raw, int accumulate, int oi, const float* colpart, int colC, const float* colscale,
                    float* colout, float* colraw, hipStream_t st);
// ... with a number of partial column rows that differs from the number of slabs (deconv_wgrad.hip: one row per tap)
int dg_wgrad_finish_rows(const float* part, int nchunks, int ntaps, int Cin, int Cout, const float* scale, float* out,
                         float* raw, int accumulate, int oi, const float* colpart, int colrows, int colC,
                         const float* colscale, float* colout, float* colraw, hipStream_t st);

// bf16 matrix pipe (wgrad_bf16.hip, BASELINE configs[3]): operands rounded to bf16 while staged, fp32 accumulation;
// same slab format, column-sum rows ([nchunks][Cout], samples b < colB) and finish launch as dg_wgrad
bool dg_wgrad_bf16_supported(int KS, int Cin, int Cout);
int dg_wgrad_bf16(int KS, const WgradArgs& a, int* nchunks, hipStream_t st);

// small-Cin wgrad (VALU), same slab format as dg_wgrad
int dg_wgrad_small(int KS, const WgradArgs& a, int* nchunks, hipStream_t st);

// The launch plan each of these launchers computes for a shape, from the launcher's own chunking function and without a
// launch or an allocation: out = {pixel tiles, tiles per workgroup, chunks (= gridDim.x = partial slabs), gridDim.y}.
// A shape the launcher refuses returns the launcher's status.
int dg_wgrad_plan(int KS, int B, int H, int W, int Cin, int Cout, int out[4]);
int dg_wgrad_small_plan(int KS, int B, int H, int W, int Cin, int Cout, int out[4]);
int dg_wgrad_bf16_plan(int KS, int B, int H, int W, int Cin, int Cout, int out[4]);

// THE rule that says which slab kernel a weight gradient takes and what the launch needs (wgrad_select.hip; host only,
// no HIP call).  With mfma = Cin % 4 == 0 && Cout % 4 == 0 && Cin >= 8:
//   x_bf16 (activation operand in bf16 memory)        DG_WG_BF16S where dg_wgrad_bf16s_supported, else DG_ERR_UNSUPPORTED
//   bf16_pipe && mfma && dg_wgrad_bf16_supported      DG_WG_BF16
//   mfma                                              DG_WG_F32
//   otherwise                                         DG_WG_EDGE
// nchunks is the chosen launcher's own plan (its refusal is returned), part_floats = nchunks slabs of KS KS Cin Cout
// floats, col_rows the partial column-sum rows of Cout floats the kernel writes when asked for column sums: nchunks for
// the three MFMA kernels, 0 for the edge kernel, whose column sums are the streaming dg_colsum pass.
// The numbering is that of depgan_debug_wgrad_plan; DG_WG_DECONV (deconv_wgrad.hip) is never chosen here.
enum DgWgradKernel { DG_WG_F32 = 0, DG_WG_EDGE = 1, DG_WG_BF16 = 2, DG_WG_BF16S = 3, DG_WG_DECONV = 4 };
struct DgWgradChoice {
  int kernel, nchunks;
  size_t part_floats;
  int col_rows;
};
int dg_wgrad_choose(int KS, int B, int H, int W, int Cin, int Cout, bool bf16_pipe, bool x_bf16, DgWgradChoice* out);
// the *_plan of slab kernel `kernel` (DG_WG_F32 .. DG_WG_BF16S)
int dg_wgrad_plan_of(int kernel, int KS, int B, int H, int W, int Cin, int Cout, int out[4]);
