// Small pieces shared by every kernel file of the gfx950 GMM extension:
// block geometry, MFMA vector typedefs, the typed x load and the block sum.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#define WAVE 64
#define NT 256  // threads per workgroup (4 waves)

namespace gmm {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

__device__ inline float load_x(const float* x, int64_t idx) { return x[idx]; }
__device__ inline float load_x(const __hip_bfloat16* x, int64_t idx) {
  return __bfloat162float(x[idx]);
}

// Sum `acc` over an NT-thread block and have thread 0 write the total to
// partial[blockIdx.x]: __shfl_down tree per wave, then a serial add of the
// NT / WAVE wave sums in wave order (a fixed order: deterministic).
// wsum is the calling kernel's own `__shared__ float wsum[NT / WAVE]`: one
// array shared by every caller becomes module-level LDS, which changed the
// callers' register allocation.
__device__ __forceinline__ void block_sum(float acc, float* wsum,
                                          float* __restrict__ partial) {
  for (int off = WAVE / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = 0.0f;
    for (int wv = 0; wv < NT / WAVE; ++wv) total += wsum[wv];
    partial[blockIdx.x] = total;
  }
}

}  // namespace gmm
