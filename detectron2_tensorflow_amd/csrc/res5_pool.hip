// The C4 head's two readers of the res5 output X [R, P, C] (Res5ROIHeads,
// lib/modeling/roi_heads/roi_heads.py:345-373) in one pass each way:
//
//   forward   pooled[r, c] = (sum_p X[r, p, c]) / P        (tf.reduce_mean over H, W)
//             Y[dst[r]]    = X[r]  where dst[r] >= 0        (tf.gather(box_features, fg_inds))
//   backward  dX[r, p, c]  = dpooled[r, c] / P + (dst[r] >= 0 ? dY[dst[r], p, c] : 0)
//
// Both are pure streams: one lane owns one 16-byte channel group of one row
// and walks p = 0 .. P-1, so a wave reads / writes 1 KiB contiguous per p, the
// sum has one fixed order (bitwise reproducible) and the backward writes every
// element of dX exactly once (no zero fill, no atomics).  kUnroll loads per
// lane are issued before the first is consumed; no LDS, 62 / 54 VGPRs (8 waves
// per SIMD), so the HBM latency is covered by waves x kUnroll requests in
// flight.
#include "common.h"

#include <climits>

namespace d2mi {
namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 7;         // P = 49 = 7 x 7 in every shipped config
constexpr int kMaxBlocks = 16384;  // columns beyond: grid stride

struct Res5Args {
  const float4* x;       // fwd: X; bwd: dY (nullable)
  const float4* pooled;  // bwd: dpooled
  const int32_t* dst;    // [R] or null
  float4* out;           // fwd: pooled; bwd: dX
  float4* y;             // fwd: Y (nullable)
  int32_t* err;
  long long cols;        // R * C4
  int P, C4, M;
};

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// dst[r] of a row, -1 when the row is not taken.  A value outside [-1, M)
// breaks the entry's precondition: the row is skipped and the device error
// word says so (never an out-of-bounds access).
__device__ __forceinline__ int taken_row(const Res5Args& a, int r, int c4) {
  if (a.dst == nullptr) return -1;
  const int d = a.dst[r];
  if (d < 0) return -1;
  if (d >= a.M) {
    if (c4 == 0) atomicOr(a.err, kErrBoxInd);
    return -1;
  }
  return d;
}

__global__ __launch_bounds__(kThreads) void res5_pool_fwd_kernel(Res5Args a) {
  const size_t row = (size_t)a.P * a.C4;
  for (long long col = (long long)blockIdx.x * kThreads + threadIdx.x; col < a.cols;
       col += (long long)gridDim.x * kThreads) {
    const int r = (int)(col / a.C4), c4 = (int)(col - (long long)r * a.C4);
    const int d = taken_row(a, r, c4);
    const float4* src = a.x + (size_t)r * row + c4;
    float4* dy = d >= 0 ? a.y + (size_t)d * row + c4 : nullptr;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int p = 0;
    for (; p + kUnroll <= a.P; p += kUnroll) {
      float4 v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) v[u] = src[(size_t)(p + u) * a.C4];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        acc = add4(acc, v[u]);  // increasing p: the one order of the sum
        if (dy) dy[(size_t)(p + u) * a.C4] = v[u];
      }
    }
    for (; p < a.P; ++p) {
      const float4 v = src[(size_t)p * a.C4];
      acc = add4(acc, v);
      if (dy) dy[(size_t)p * a.C4] = v;
    }
    const float n = (float)a.P;
    a.out[col] = make_float4(acc.x / n, acc.y / n, acc.z / n, acc.w / n);
  }
}

__global__ __launch_bounds__(kThreads) void res5_pool_bwd_kernel(Res5Args a) {
  const size_t row = (size_t)a.P * a.C4;
  for (long long col = (long long)blockIdx.x * kThreads + threadIdx.x; col < a.cols;
       col += (long long)gridDim.x * kThreads) {
    const int r = (int)(col / a.C4), c4 = (int)(col - (long long)r * a.C4);
    const int d = a.x != nullptr ? taken_row(a, r, c4) : -1;
    const float n = (float)a.P;
    float4 g = a.pooled[col];
    g = make_float4(g.x / n, g.y / n, g.z / n, g.w / n);
    float4* dx = a.out + (size_t)r * row + c4;
    if (d < 0) {
      for (int p = 0; p < a.P; ++p) dx[(size_t)p * a.C4] = g;
      continue;
    }
    const float4* src = a.x + (size_t)d * row + c4;
    int p = 0;
    for (; p + kUnroll <= a.P; p += kUnroll) {
      float4 v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) v[u] = src[(size_t)(p + u) * a.C4];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) dx[(size_t)(p + u) * a.C4] = add4(g, v[u]);
    }
    for (; p < a.P; ++p) dx[(size_t)p * a.C4] = add4(g, src[(size_t)p * a.C4]);
  }
}

int res5_shape(const char* what, int R, int P, int C, int M, bool has_dst, Res5Args* a) {
  D2MI_REQUIRE(C >= 4 && C % 4 == 0, "%s: C = %d must be a positive multiple of 4", what, C);
  D2MI_REQUIRE(P >= 1, "%s: P = %d must be at least 1", what, P);
  D2MI_REQUIRE(R >= 0 && M >= 0, "%s: bad sizes R = %d, M = %d", what, R, M);
  D2MI_REQUIRE(has_dst || M == 0, "%s: M = %d destination rows without dst", what, M);
  a->P = P;
  a->C4 = C / 4;
  a->M = M;
  a->cols = (long long)R * (C / 4);
  return 0;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

dim3 res5_grid(long long cols) {
  const long long blocks = (cols + kThreads - 1) / kThreads;
  return dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks));
}

}  // namespace
}  // namespace d2mi

using namespace d2mi;

extern "C" int d2mi_res5_pool_fwd(const float* X, int R, int P, int C, const int32_t* dst, int M,
                                  float* pooled, float* Y, void* stream) {
  Res5Args a{};
  if (res5_shape("res5_pool_fwd", R, P, C, M, dst != nullptr, &a)) return -1;
  if (R == 0) return 0;
  D2MI_REQUIRE(X && pooled, "res5_pool_fwd: null pointer");
  D2MI_REQUIRE(dst == nullptr || M == 0 || Y, "res5_pool_fwd: dst with M = %d rows needs Y", M);
  D2MI_REQUIRE(aligned16(X) && aligned16(pooled) && aligned16(Y),
               "res5_pool_fwd: X, pooled and Y must be 16-byte aligned");
  a.x = reinterpret_cast<const float4*>(X);
  a.dst = M > 0 ? dst : nullptr;  // (M == 0: no row can be taken)
  a.out = reinterpret_cast<float4*>(pooled);
  a.y = reinterpret_cast<float4*>(Y);
  a.err = error_word();
  hipLaunchKernelGGL(res5_pool_fwd_kernel, res5_grid(a.cols), dim3(kThreads), 0,
                     as_stream(stream), a);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" int d2mi_res5_pool_bwd(const float* dpooled, const float* dY, const int32_t* dst, int R,
                                  int P, int C, int M, float* dX, void* stream) {
  Res5Args a{};
  if (res5_shape("res5_pool_bwd", R, P, C, M, dst != nullptr, &a)) return -1;
  if (R == 0) return 0;
  D2MI_REQUIRE(dpooled && dX, "res5_pool_bwd: null pointer");
  D2MI_REQUIRE(aligned16(dpooled) && aligned16(dX) && aligned16(dY),
               "res5_pool_bwd: dpooled, dY and dX must be 16-byte aligned");
  const bool gather = dst != nullptr && dY != nullptr && M > 0;
  a.x = gather ? reinterpret_cast<const float4*>(dY) : nullptr;
  a.pooled = reinterpret_cast<const float4*>(dpooled);
  a.dst = gather ? dst : nullptr;
  a.out = reinterpret_cast<float4*>(dX);
  a.err = error_word();
  hipLaunchKernelGGL(res5_pool_bwd_kernel, res5_grid(a.cols), dim3(kThreads), 0,
                     as_stream(stream), a);
  D2MI_LAUNCH_CHECK();
  return 0;
}
