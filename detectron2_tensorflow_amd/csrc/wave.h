// Wave (64 lanes) and workgroup primitives with more than one user: butterfly
// reductions, a 64-bit readlane, the four-wave workgroup sum and the pyramid
// level lookup.  Reductions over floats fix their addition order here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace d2mi {

// Butterfly (xor) reductions over the wave: every lane gets the result.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T w = __shfl_xor(v, o, 64);
    if constexpr (std::is_same_v<T, float>) v = fmaxf(v, w);
    else v = max(v, w);
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T w = __shfl_xor(v, o, 64);
    if constexpr (std::is_same_v<T, float>) v = fminf(v, w);
    else v = min(v, w);
  }
  return v;
}

// Lane l's 64-bit value in scalar registers (l wave-uniform).
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

// Down-shuffle sum: lane 0 gets lanes 0..63 added in the tree's fixed order.
template <typename T>
__device__ __forceinline__ T wave_sum_down(T v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ float2 wave_sum_down(float2 v) {
  for (int o = 32; o > 0; o >>= 1) {
    v.x += __shfl_down(v.x, o, 64);
    v.y += __shfl_down(v.y, o, 64);
  }
  return v;
}

// Fixed-order sum over a workgroup of 256 threads (four waves): each wave's
// down-shuffle sum, then the four in wave order.  The result is valid in
// thread 0.  red: four elements of LDS, free again after the caller's next
// barrier.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  v = wave_sum_down(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T s = T();
  if (threadIdx.x == 0) {
    s = red[0];
    for (int k = 1; k < 4; ++k) s += red[k];
  }
  return s;
}

// The level that holds flat index i of a pyramid whose level l starts at
// first[l] (first[0] = 0, ascending): the last l < L with first[l] <= i.
// (Kernels that spell this loop out on a member of their argument struct do
// so because the call compiled to different code there.)
template <typename T>
__device__ __forceinline__ int level_of(const T* first, int L, T i) {
  int l = 0;
  while (l + 1 < L && first[l + 1] <= i) ++l;
  return l;
}

}  // namespace d2mi
