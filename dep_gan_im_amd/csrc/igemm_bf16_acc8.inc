// Accumulator transposition of the kernels whose epilogue owns 8 consecutive channels of a pixel per lane
// (igemm_bf16_mh_kernel, igemm_bf16s_kernel.inc), included right after igemm_bf16_main.inc.  As igemm_epilogue.inc: each
// wave's 64 x 32 tile goes through LDS (rows of NT + 4 floats); here a lane then reads channels [c8, c8 + 8) of pixel
// p * 16 + pl0 of the wave's 4 x 16 block in pass p: 4 lanes per pixel, one 16-pixel row per pass.
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
