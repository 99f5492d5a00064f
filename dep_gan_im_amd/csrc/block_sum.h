// Block reductions and the grid size of the grid-stride operators, shared by train_ops.hip and softmax_ce.hip.
#pragma once
#include "common.h"

__device__ __forceinline__ float t_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ float t_block_sum(float v, float* sh4) {
  v = t_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}
static inline int t_nblk(size_t n, int cap) {
  size_t b = (n + 255) / 256;
  return (int)(b > (size_t)cap ? cap : (b < 1 ? 1 : b));
}
