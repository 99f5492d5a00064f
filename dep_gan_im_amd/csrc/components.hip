// Connected components of a binary volume (evaluate.connected_components / lesion_detection): label-equivalence
// union-find in a fixed number of launches, canonical numbering, and the per-component size / overlap tables.
// Volumes are (D, H, W) bytes with W contiguous; non-zero means set (the conventions of surface_dist.hip).
//
//   cc_init_kernel           parent[v] = the first voxel of v's run of set voxels in its row, as far as the run lies in
//                            v's wave (a ballot of "set and joined to the left"), -1 for an unset voxel.  A run that
//                            crosses a wave boundary starts anew at lane 0; the merge launch joins the two pieces.
//   cc_merge_kernel<R, P>    every set voxel unions itself with the set voxels of the BACKWARD half-neighbourhood (the
//                            offsets that precede it in index order; the one along W is the run and is already made)
//   cc_compress_kernel       label[v] = find(v), a launch of its own: the kernel boundary makes every atomic of the
//                            merge visible.  Also counts the roots (parent[v] == v) of every block of 256 voxels.
//   cc_scan_kernel           one block: exclusive prefix sum of the block counts in index order, and the total N
//   cc_rank_kernel           rank[root] = 1 + the number of roots before it (block offset + position inside the block),
//                            written over parent[root], which nothing reads any more
//   cc_relabel_kernel        label[v] = rank[label[v]], 0 for an unset voxel
//   cc_overlap_kernel        size[k - 1] += 1, hits[k - 1] += (other != 0) per voxel of component k, added per wave
//                            over runs of lanes with the same label
//
// The forest.  parent[x] <= x holds from the first launch on: a run start is not behind its voxel, and the only later
// write is atomicMin(&parent[a], b) with b < a.  The root of a tree is therefore the smallest index of its set, whatever
// order the atomics land in, so the labels do not depend on scheduling and a call repeats bit for bit; numbering the roots
// in index order is scipy.ndimage.label's numbering (components in the order of their first voxel).
//
// Termination, by construction and not by convergence.  cc_find follows parent while it is strictly smaller than the
// index it was read at, so it takes at most x steps from x.  cc_union chases both voxels to roots a > b and issues
// atomicMin(&parent[a], b).  Either the old value was a (a was a root: the trees are joined, done) or it was some
// r < a: parent[a] now holds min(r, b), and a ~ r ~ b is restored by going on with the pair (r, b).  Every retry
// replaces the larger index of the pair by a strictly smaller one, so a + b falls strictly and the loop ends after at
// most a + b rounds.  No thread waits for another.
//
// Coherence.  Inside the merge launch parent is read with relaxed device-scope atomic loads, so a CU's vector cache
// cannot serve one stale line for the whole kernel.  Correctness does not rest on it: parent[x] only ever falls, every
// value it held is an index of x's own set, so a stale read is an older ancestor and the chase merely starts higher; a
// stale "root" is corrected by the value atomicMin returns.
#include "common.h"

#include "../../include/depgan.h"

namespace {

constexpr int CC_MAX_DIM = 4096;
constexpr int CC_BLOCK = 256;      // voxels per block of the per-voxel kernels: four waves, lane = v & 63
constexpr int CC_SCAN_BLOCK = 1024;

// grid ceil(n / 256), block 256, thread = voxel.  The run start inside the wave: with m the ballot of "set, not the
// first of its row, and the voxel to the left is set", lane l's run reaches down to the highest lane <= l whose bit is
// clear -- or to lane 0 if there is none, where a run that came in from the previous wave is cut.
__global__ __launch_bounds__(CC_BLOCK) void cc_init_kernel(const unsigned char* __restrict__ set,
                                                           int* __restrict__ parent, int W, unsigned n) {
  const unsigned v = blockIdx.x * (unsigned)CC_BLOCK + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const bool live = v < n;
  const bool s = live && set[v] != 0;
  const bool link = s && (v % (unsigned)W) != 0u && set[v - 1] != 0;
  const unsigned long long m = __ballot(link);
  if (!live) return;
  int p = -1;
  if (s) {
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const unsigned long long clear = ~m & upto;
    const int start = clear ? 63 - __builtin_clzll(clear) : 0;
    p = (int)v - (lane - start);
  }
  parent[v] = p;
}

// At most x steps from x: the chase goes on only to a strictly smaller index (a negative value, which no set voxel
// holds, ends it as well).
__device__ __forceinline__ int cc_find(const int* parent, int x) {
  for (;;) {
    const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((unsigned)p >= (unsigned)x) return x;
    x = p;
  }
}

// See "Termination" above: a + b falls strictly with every round.
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(parent + a, b);      // device scope
    if (old == a) return;                          // a was a root and now hangs below b
    a = old;                                       // old < a: parent[a] = min(old, b); go on with (old, b)
  }
}

// One row (z + dz, y + dy) of the backward half-neighbourhood, `up` the index of its voxel at x.  WIDE: the row
// contributes x - 1, x, x + 1, else x alone.  `left`: the voxel at x - 1 of v's own row is set, so it belongs to v's
// run and has made, or has in turn left to its own left neighbour, every union with the voxels at x - 1 and x of this
// row.  Set voxels that are neighbours within the row above are one run, so one union per run is enough.
template <bool WIDE>
__device__ __forceinline__ void cc_row(const unsigned char* __restrict__ set, int* parent, int v, unsigned up, int x,
                                       int W, bool left) {
  const bool b = set[up] != 0;
  if (WIDE) {
    if (b) {
      if (!left) cc_union(parent, v, (int)up);
    } else {
      if (!left && x > 0 && set[up - 1] != 0) cc_union(parent, v, (int)up - 1);
      if (x < W - 1 && set[up + 1] != 0) cc_union(parent, v, (int)up + 1);
    }
  } else {
    if (b && !(left && set[up - 1] != 0)) cc_union(parent, v, (int)up);      // left: x > 0
  }
}

// grid ceil(n / 256), block 256, thread = voxel.  RANK: scipy's generate_binary_structure(3, RANK); PLANE: neighbours in
// the slice only.  The backward rows, (dz, dy) and their width:
//   in the slice    (0, -1): x alone at rank 1, x - 1 .. x + 1 at ranks 2 and 3
//   in the volume   rank 1: (0, -1) and (-1, 0), x alone                                         (3 offsets with the run)
//                   rank 2: (0, -1) and (-1, 0) wide, (-1, -1) and (-1, +1) x alone              (9)
//                   rank 3: (0, -1), (-1, -1), (-1, 0), (-1, +1), all wide                       (13)
template <int RANK, bool PLANE>
__global__ __launch_bounds__(CC_BLOCK) void cc_merge_kernel(const unsigned char* __restrict__ set, int* parent, int H,
                                                            int W, unsigned n) {
  const unsigned v = blockIdx.x * (unsigned)CC_BLOCK + threadIdx.x;
  if (v >= n || set[v] == 0) return;
  const unsigned HW = (unsigned)H * (unsigned)W;
  const int z = (int)(v / HW);
  const unsigned pix = v - (unsigned)z * HW;
  const int y = (int)(pix / (unsigned)W), x = (int)(pix - (unsigned)y * (unsigned)W);
  const bool left = x > 0 && set[v - 1] != 0;
  // the piece of a run that cc_init_kernel cut at the wave boundary
  if (left && (v & 63u) == 0u) cc_union(parent, (int)v, (int)v - 1);
  // an index is formed only for a row inside the volume
  if (y > 0) cc_row<(RANK >= 2)>(set, parent, (int)v, v - (unsigned)W, x, W, left);
  if (!PLANE && z > 0) {
    cc_row<(RANK >= 2)>(set, parent, (int)v, v - HW, x, W, left);
    if (RANK >= 2) {
      if (y > 0) cc_row<(RANK == 3)>(set, parent, (int)v, v - HW - (unsigned)W, x, W, left);
      if (y < H - 1) cc_row<(RANK == 3)>(set, parent, (int)v, v - HW + (unsigned)W, x, W, left);
    }
  }
}

// grid ceil(n / 256), block 256.  Plain loads: the merge launch has ended.  count[block] = roots among its voxels.
__global__ __launch_bounds__(CC_BLOCK) void cc_compress_kernel(const int* __restrict__ parent, int* __restrict__ label,
                                                               int* __restrict__ count, unsigned n) {
  __shared__ int wave_roots[CC_BLOCK / 64];
  const unsigned v = blockIdx.x * (unsigned)CC_BLOCK + threadIdx.x;
  bool root = false;
  if (v < n) {
    int x = (int)v, p = parent[v];
    root = p == x;
    while ((unsigned)p < (unsigned)x) {      // strictly down, at most v steps; -1 (unset) ends it at once
      x = p;
      p = parent[x];
    }
    label[v] = p < 0 ? -1 : x;
  }
  const unsigned long long m = __ballot(root);
  if ((threadIdx.x & 63u) == 0u) wave_roots[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) count[blockIdx.x] = wave_roots[0] + wave_roots[1] + wave_roots[2] + wave_roots[3];
}

// one block of 1024: count[0 .. nblk) becomes its exclusive prefix sum, in index order, 1024 entries per round with the
// carry of the rounds before; *total = N (< 2^31: there are fewer roots than voxels).
__global__ __launch_bounds__(CC_SCAN_BLOCK) void cc_scan_kernel(int* __restrict__ count, int nblk,
                                                                long long* __restrict__ total) {
  __shared__ int wave_sum[CC_SCAN_BLOCK / 64];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  int carry = 0;
  for (int base = 0; base < nblk; base += CC_SCAN_BLOCK) {
    const int i = base + t;
    const int c = i < nblk ? count[i] : 0;
    int s = c;                                           // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(s, o);
      if (lane >= o) s += up;
    }
    if (lane == 63) wave_sum[wave] = s;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < CC_SCAN_BLOCK / 64; ++w) {
      const int ws = wave_sum[w];
      if (w < wave) before += ws;
      all += ws;
    }
    if (i < nblk) count[i] = carry + before + s - c;
    carry += all;
    __syncthreads();                                     // wave_sum is rewritten in the next round
  }
  if (t == 0) *total = (long long)carry;
}

// grid ceil(n / 256), block 256.  label holds the root index of every set voxel; a root is a voxel that is its own.
// rank[root] = offset[block] + roots before it in the block + 1.
__global__ __launch_bounds__(CC_BLOCK) void cc_rank_kernel(const int* __restrict__ label, const int* __restrict__ offset,
                                                           int* __restrict__ rank, unsigned n) {
  __shared__ int wave_roots[CC_BLOCK / 64];
  const unsigned v = blockIdx.x * (unsigned)CC_BLOCK + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const bool root = v < n && label[v] == (int)v;
  const unsigned long long m = __ballot(root);
  if (lane == 0) wave_roots[wave] = __popcll(m);
  __syncthreads();
  if (!root) return;
  int before = __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) before += wave_roots[w];
  rank[v] = offset[blockIdx.x] + before + 1;
}

__global__ __launch_bounds__(CC_BLOCK) void cc_relabel_kernel(int* __restrict__ label, const int* __restrict__ rank,
                                                              unsigned n) {
  const unsigned v = blockIdx.x * (unsigned)CC_BLOCK + threadIdx.x;
  if (v >= n) return;
  const int r = label[v];
  label[v] = r < 0 ? 0 : rank[r];
}

// grid ceil(n / 256), block 256, thread = voxel.  A run of lanes with the same label adds once, from its first lane:
// the run's length to size, and the number of its lanes with other != 0 to hits.  Integer adds: any order, one result.
// A label outside 1 .. n_comp is not counted (and so never indexes a table).
__global__ __launch_bounds__(CC_BLOCK) void cc_overlap_kernel(const int* __restrict__ label,
                                                              const unsigned char* __restrict__ other, unsigned n,
                                                              int n_comp, int* size, int* hits) {
  const unsigned v = blockIdx.x * (unsigned)CC_BLOCK + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  int l = v < n ? label[v] : 0;
  if (l < 1 || l > n_comp) l = 0;
  const bool hit = l != 0 && other != nullptr && other[v] != 0;
  const int prev = __shfl_up(l, 1);
  const unsigned long long heads = __ballot(lane == 0 || prev != l);
  const unsigned long long hitmask = __ballot(hit);
  if (l == 0 || !((heads >> lane) & 1ull)) return;
  const unsigned long long later = lane == 63 ? 0ull : (heads >> (lane + 1));
  const int len = later ? __builtin_ctzll(later) + 1 : 64 - lane;         // lanes lane .. lane + len - 1
  const unsigned long long run = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
  atomicAdd(size + (l - 1), len);
  const int h = __popcll(hitmask & run);
  if (h) atomicAdd(hits + (l - 1), h);
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || !na || !nb) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// D, H, W in 1..4096 and D*H*W < 2^31
bool volume_ok(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1 || D > CC_MAX_DIM || H > CC_MAX_DIM || W > CC_MAX_DIM) return false;
  return (long)D * H * W < (1L << 31);
}

size_t round8(size_t b) { return (b + 7) & ~(size_t)7; }

size_t blocks_of(size_t n) { return (n + CC_BLOCK - 1) / CC_BLOCK; }

template <int RANK, bool PLANE>
void launch_merge(const unsigned char* set, int* parent, int H, int W, unsigned n, hipStream_t st) {
  hipLaunchKernelGGL((cc_merge_kernel<RANK, PLANE>), dim3((unsigned)blocks_of(n)), dim3(CC_BLOCK), 0, st, set, parent,
                     H, W, n);
}

}  // namespace

extern "C" {

// parent / rank (n ints), the block counts / offsets (ceil(n / 256) ints), N (8 bytes)
size_t depgan_eval_cc_scratch_bytes(int D, int H, int W) {
  if (!volume_ok(D, H, W)) return 0;
  const size_t n = (size_t)D * H * W;
  return round8(n * sizeof(int)) + round8(blocks_of(n) * sizeof(int)) + sizeof(long long);
}

int depgan_eval_cc_label(const unsigned char* set, int D, int H, int W, int connectivity, int in_plane, int* labels,
                         void* scratch, long long n_out_host[1], void* stream) {
  if (!volume_ok(D, H, W) || !set || !labels || !scratch || !n_out_host || ((uintptr_t)labels & 3) ||
      ((uintptr_t)scratch & 7) || connectivity < 1 || connectivity > 3 || (in_plane != 0 && in_plane != 1)) {
    dg_set_error("eval_cc_label: bad argument (D=%d H=%d W=%d connectivity=%d in_plane=%d; dimensions 1..%d, D*H*W < "
                 "2^31; connectivity 1..3, in_plane 0 / 1; every pointer given, labels 4-byte and scratch 8-byte "
                 "aligned)", D, H, W, connectivity, in_plane, CC_MAX_DIM);
    return DG_ERR_ARG;
  }
  const size_t n = (size_t)D * H * W;
  const size_t sbytes = depgan_eval_cc_scratch_bytes(D, H, W);
  if (overlaps(labels, n * 4, set, n) || overlaps(scratch, sbytes, set, n) || overlaps(scratch, sbytes, labels, n * 4)) {
    dg_set_error("eval_cc_label: two of set, labels and scratch overlap");
    return DG_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  int* parent = (int*)scratch;
  int* count = (int*)((char*)scratch + round8(n * sizeof(int)));
  long long* total = (long long*)((char*)count + round8(blocks_of(n) * sizeof(int)));
  const dim3 grid((unsigned)blocks_of(n)), block(CC_BLOCK);
  const unsigned un = (unsigned)n;
  hipLaunchKernelGGL(cc_init_kernel, grid, block, 0, st, set, parent, W, un);
  if (in_plane) {
    if (connectivity == 1) launch_merge<1, true>(set, parent, H, W, un, st);
    else launch_merge<2, true>(set, parent, H, W, un, st);          // ranks 2 and 3 are the same 8 neighbours
  } else {
    if (connectivity == 1) launch_merge<1, false>(set, parent, H, W, un, st);
    else if (connectivity == 2) launch_merge<2, false>(set, parent, H, W, un, st);
    else launch_merge<3, false>(set, parent, H, W, un, st);
  }
  hipLaunchKernelGGL(cc_compress_kernel, grid, block, 0, st, (const int*)parent, labels, count, un);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(CC_SCAN_BLOCK), 0, st, count, (int)blocks_of(n), total);
  hipLaunchKernelGGL(cc_rank_kernel, grid, block, 0, st, (const int*)labels, (const int*)count, parent, un);
  hipLaunchKernelGGL(cc_relabel_kernel, grid, block, 0, st, labels, (const int*)parent, un);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(n_out_host, total, sizeof(long long), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  return DG_OK;
}

int depgan_eval_cc_overlap(const int* labels, const unsigned char* other_or_null, long n, int n_comp, int* size,
                           int* hits, void* stream) {
  if (!labels || ((uintptr_t)labels & 3) || n < 1 || n >= (1L << 31) || n_comp < 0 || (long)n_comp > n ||
      (n_comp > 0 && (!size || !hits || ((uintptr_t)size & 3) || ((uintptr_t)hits & 3)))) {
    dg_set_error("eval_cc_overlap: bad argument (n=%ld n_comp=%d; 1 <= n < 2^31, 0 <= n_comp <= n; labels given, size "
                 "and hits given unless n_comp is 0, all 4-byte aligned)", n, n_comp);
    return DG_ERR_ARG;
  }
  if (n_comp == 0) return DG_OK;
  const size_t tbytes = (size_t)n_comp * sizeof(int);
  if (overlaps(size, tbytes, hits, tbytes) || overlaps(size, tbytes, labels, (size_t)n * 4) ||
      overlaps(hits, tbytes, labels, (size_t)n * 4) || overlaps(size, tbytes, other_or_null, (size_t)n) ||
      overlaps(hits, tbytes, other_or_null, (size_t)n)) {
    dg_set_error("eval_cc_overlap: size or hits overlaps the other one, labels or other");
    return DG_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  HIPCHECK(hipMemsetAsync(size, 0, tbytes, st));
  HIPCHECK(hipMemsetAsync(hits, 0, tbytes, st));
  hipLaunchKernelGGL(cc_overlap_kernel, dim3((unsigned)blocks_of((size_t)n)), dim3(CC_BLOCK), 0, st, labels,
                     other_or_null, (unsigned)n, n_comp, size, hits);
  HIPCHECK(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
