// The block-wide sums of the guidance rescale's statistics, shared by the step tails (step_tail.hip cfg_rescale_factor) and the
// three-way guidance (ip2p.hip): one block of CRA_THREADS threads per sample, a lane keeps up to CRA_RES values per plane resident.
#pragma once
#include "common.h"

namespace sd {

constexpr int CRA_THREADS = 1024, CRA_RES = 32;

// a, b <- their sums over the block, in every lane; part: LDS [2][16]
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*part)[CRA_THREADS / 64]) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & 63;
  __syncthreads();   // (the readers of the previous call are done with part)
  if (lane == 0) {
    part[0][threadIdx.x >> 6] = a;
    part[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  a = part[0][lane & 15];
  b = part[1][lane & 15];
  for (int o = 8; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
}

}  // namespace sd
