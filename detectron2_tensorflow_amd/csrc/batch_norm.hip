// BatchNorm on batch statistics, NHWC f32 (lib/layers/normalization.py:97-119:
// tf.layers.BatchNormalization(...).apply(inputs, training=True); :120-165,
// the SyncBN branch, is the same layer on the moments of all replicas).  The
// input is x [M, C]: the M = N*H*W pixel rows of an NHWC map, or [R, C].
//
//   bn_stats_kernel      one read of x: per (row chunk, channel) a
//                        (count, mean, M2) triple.  Each thread runs Welford's
//                        update over its rows; the pixel slots of a workgroup
//                        and then the chunks are merged in index order by the
//                        parallel-variance formula (bn_merge), never by
//                        E[x^2] - E[x]^2 (a conv output with mean 30 and std
//                        0.3 loses three digits of y to that).
//   bn_merge_kernel      P triples per channel, in a fixed order: the chunks of one
//                        call -> this replica's triple; the replicas' triples
//                        (one locally) -> mean, var, invstd and the moving
//                        averages.  One kernel, two epilogues.
//   bn_apply_kernel      y = xh * gamma + beta (+ residual, ReLU before or
//                        after the add).
//   bn_bwd_reduce_kernel per (row chunk, channel) sum dz and sum dz * xh;
//   bn_sum_kernel        the chunks in order -> sums [2C] (dbeta, dgamma).
//   bn_bwd_apply_kernel  dx (and the residual's gradient, dz).
//
// Every streaming pass maps a workgroup to (row chunk, tile of <= 256 channel
// quads): consecutive threads read consecutive float4 of a row and then the
// next row (whole rows, coalesced), a thread keeps its quad's per-channel
// values in registers and walks its rows four loads at a time.  Chunks are
// cut over rows, not images, so the box head's [R,7,7,C] at a few hundred
// rows per image still fills the device; C up to 2048 takes two tiles.
// Reductions are per channel ACROSS the threads of a workgroup (a column of
// the [slot, channel] table in LDS, added in slot order), so wave.h's
// block_sum -- one value per workgroup -- does not apply; like it, they fix
// the addition order: no atomics, bitwise reproducible.
#include <algorithm>

#include "common.h"

namespace d2mi {
namespace {

constexpr int kBnThreads = 256;
constexpr int kBnMaxChunks = 512;  // workgroups per launch (two per CU), also the merge's loop
constexpr int kBnRowsPerThread = 8;

struct BnPlan {
  int QT, tiles, ppi, P;
  long long chunk_rows;
};

static BnPlan bn_plan(long long M, int C) {
  BnPlan p;
  const int C4 = C / 4;
  p.QT = std::min(C4, kBnThreads);
  p.tiles = (C4 + p.QT - 1) / p.QT;
  p.ppi = kBnThreads / p.QT;
  const long long per = (long long)p.ppi * kBnRowsPerThread;
  const long long maxP = std::max(1, kBnMaxChunks / p.tiles);
  long long P = std::min(maxP, std::max(1LL, (M + per - 1) / per));
  long long rows = (M + P - 1) / P;
  rows = (rows + p.ppi - 1) / p.ppi * p.ppi;
  p.chunk_rows = rows;
  p.P = (int)((M + rows - 1) / rows);
  return p;
}

// this thread's place in its workgroup's (row slot, channel quad) table
struct BnThread {
  int q, tp, ppi;
  bool active;
  long long r0, r1;
  __device__ BnThread(long long M, int C, long long chunk_rows) {
    const int C4 = C / 4;
    const int QT = min(C4, kBnThreads);
    ppi = kBnThreads / QT;
    q = blockIdx.y * QT + (int)threadIdx.x % QT;
    tp = (int)threadIdx.x / QT;
    active = tp < ppi && q < C4;
    r0 = (long long)blockIdx.x * chunk_rows;
    r1 = min(M, r0 + chunk_rows);
  }
};

__device__ __forceinline__ float4 ld4(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ float4 ld4_or(const float* p, float fill) {
  return p ? ld4(p) : make_float4(fill, fill, fill, fill);
}

// xh and z of one element: the forward's arithmetic, restated by the
// backward (relu_mode 1 takes its mask from this z: the same bits, whatever
// the contraction setting: the multiply-add is written as ONE fused op).
__device__ __forceinline__ float bn_xh(float v, float mu, float is) { return (v - mu) * is; }
__device__ __forceinline__ float bn_z(float xh, float g, float b) { return __fmaf_rn(xh, g, b); }

// P (count, mean, M2) triples of one channel, merged in index order with the
// parallel-variance formula in its many-way form: the total count, the
// count-weighted mean (about the first triple's mean: no large partial sums),
// then M2 = sum M2_i + count_i * (mean_i - mean)^2.  get(i, n, m, s).
template <typename F>
__device__ __forceinline__ void bn_merge(int P, F get, float& N, float& mean, float& M2) {
  float n, m, s, m0;
  get(0, n, m0, s);
  N = 0.f;
  float acc = 0.f;
  for (int i = 0; i < P; ++i) {
    get(i, n, m, s);
    N += n;
    acc += n * (m - m0);
  }
  mean = m0 + acc / N;
  M2 = 0.f;
  for (int i = 0; i < P; ++i) {
    get(i, n, m, s);
    const float d = m - mean;
    M2 += s + n * (d * d);
  }
}

__device__ __forceinline__ void welford(float v, float rn, float& mu, float& m2) {
  const float d = v - mu;
  mu += d * rn;
  m2 += d * (v - mu);
}

// pcnt [P], pmean / pm2 [P, C]
__global__ __launch_bounds__(kBnThreads) void bn_stats_kernel(const float* __restrict__ x,
                                                             long long M, int C,
                                                             long long chunk_rows,
                                                             float* __restrict__ pcnt,
                                                             float* __restrict__ pmean,
                                                             float* __restrict__ pm2) {
  __shared__ float s_cnt[kBnThreads];
  __shared__ float s_mean[kBnThreads * 4];
  __shared__ float s_m2[kBnThreads * 4];
  const BnThread t(M, C, chunk_rows);
  float n = 0.f;
  float4 mu = make_float4(0.f, 0.f, 0.f, 0.f), m2 = mu;
  if (t.active) {
    const float* xq = x + (size_t)t.q * 4;
    for (long long r = t.r0 + t.tp; r < t.r1; r += 4LL * t.ppi) {
      float4 v[4];
      bool ok[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long rr = r + (long long)k * t.ppi;
        ok[k] = rr < t.r1;
        v[k] = ok[k] ? ld4(xq + (size_t)rr * C) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (ok[k]) {
          n += 1.f;
          const float rn = 1.f / n;
          welford(v[k].x, rn, mu.x, m2.x);
          welford(v[k].y, rn, mu.y, m2.y);
          welford(v[k].z, rn, mu.z, m2.z);
          welford(v[k].w, rn, mu.w, m2.w);
        }
      }
    }
  }
  s_cnt[threadIdx.x] = n;
  reinterpret_cast<float4*>(s_mean)[threadIdx.x] = mu;
  reinterpret_cast<float4*>(s_m2)[threadIdx.x] = m2;
  __syncthreads();
  // per channel of the tile: its row slots in slot order (slot 0 always has a row)
  const int QT = min(C / 4, kBnThreads);
  for (int cl = threadIdx.x; cl < QT * 4; cl += kBnThreads) {
    const int ql = cl >> 2, e = cl & 3;
    const int c = (blockIdx.y * QT + ql) * 4 + e;
    if (c >= C) continue;
    float N, mean, M2;
    bn_merge(t.ppi, [&](int i, float& cn, float& cm, float& cs) {
      const int idx = i * QT + ql;
      cn = s_cnt[idx];
      cm = s_mean[idx * 4 + e];
      cs = s_m2[idx * 4 + e];
    }, N, mean, M2);
    if (c == 0) pcnt[blockIdx.x] = N;
    pmean[(size_t)blockIdx.x * C + c] = mean;
    pm2[(size_t)blockIdx.x * C + c] = M2;
  }
}

// A workgroup merges kBnCols channels: the P triples (cnt[i * cnt_stride],
// mean / m2 [i * row_stride + c]) are cut into kBnSlices runs of consecutive
// rows, one thread merges each run in order, then one thread per channel the
// runs in order (a fixed two-level order: P sequential steps would cost more
// than the pass that made the triples).  FINAL: the layer's statistics and
// its moving averages; else this replica's triple [2C + 1].
constexpr int kBnCols = 4, kBnSlices = 64;

template <bool FINAL>
__global__ __launch_bounds__(kBnCols* kBnSlices) void bn_merge_kernel(
    const float* __restrict__ cnt, long long cnt_stride, const float* __restrict__ mean_in,
    const float* __restrict__ m2_in, long long row_stride, int P, int C, float eps, float decay,
    float* __restrict__ moving_mean, float* __restrict__ moving_var, float* __restrict__ o_mean,
    float* __restrict__ o_var, float* __restrict__ o_invstd, float* __restrict__ triple) {
  __shared__ float s_n[kBnSlices][kBnCols], s_m[kBnSlices][kBnCols], s_s[kBnSlices][kBnCols];
  const int col = threadIdx.x % kBnCols, slice = threadIdx.x / kBnCols;
  const int c = blockIdx.x * kBnCols + col;
  const int per = (P + kBnSlices - 1) / kBnSlices;
  const int i0 = slice * per, i1 = min(P, i0 + per);
  float N = 0.f, mean = 0.f, M2 = 0.f;
  if (c < C && i0 < i1) {
    bn_merge(i1 - i0, [&](int i, float& cn, float& cm, float& cs) {
      cn = cnt[(size_t)(i0 + i) * cnt_stride];
      cm = mean_in[(size_t)(i0 + i) * row_stride + c];
      cs = m2_in[(size_t)(i0 + i) * row_stride + c];
    }, N, mean, M2);
  }
  s_n[slice][col] = N;
  s_m[slice][col] = mean;
  s_s[slice][col] = M2;
  __syncthreads();
  if (slice != 0 || c >= C) return;
  // (run 0 is never empty; an empty run counts 0 rows and adds nothing)
  bn_merge(kBnSlices, [&](int i, float& cn, float& cm, float& cs) {
    cn = s_n[i][col];
    cm = s_m[i][col];
    cs = s_s[i][col];
  }, N, mean, M2);
  if (FINAL) {
    const float var = M2 / N;
    o_mean[c] = mean;
    o_var[c] = var;
    o_invstd[c] = 1.f / sqrtf(var + eps);
    const float keep = 1.f - decay;
    moving_mean[c] = moving_mean[c] * decay + mean * keep;
    moving_var[c] = moving_var[c] * decay + var * keep;
  } else {
    if (c == 0) triple[0] = N;
    triple[1 + c] = mean;
    triple[1 + C + c] = M2;
  }
}

__device__ __forceinline__ float4 relu4(float4 v) {
  return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// the per-channel values a streaming thread keeps for its quad
struct BnQuad {
  float4 mu, is, g, b;
  __device__ BnQuad(const float* mean, const float* invstd, const float* gamma,
                    const float* beta, int q)
      : mu(ld4(mean + q * 4)), is(ld4(invstd + q * 4)),
        g(ld4_or(gamma ? gamma + q * 4 : nullptr, 1.f)),
        b(ld4_or(beta ? beta + q * 4 : nullptr, 0.f)) {}
  __device__ __forceinline__ float4 xh(float4 v) const {
    return make_float4(bn_xh(v.x, mu.x, is.x), bn_xh(v.y, mu.y, is.y), bn_xh(v.z, mu.z, is.z),
                       bn_xh(v.w, mu.w, is.w));
  }
  __device__ __forceinline__ float4 z(float4 h) const {
    return make_float4(bn_z(h.x, g.x, b.x), bn_z(h.y, g.y, b.y), bn_z(h.z, g.z, b.z),
                       bn_z(h.w, g.w, b.w));
  }
};

__global__ __launch_bounds__(kBnThreads) void bn_apply_kernel(
    const float* __restrict__ x, long long M, int C, long long chunk_rows,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ residual, int relu_mode, float* __restrict__ y) {
  const BnThread t(M, C, chunk_rows);
  if (!t.active) return;
  const BnQuad p(mean, invstd, gamma, beta, t.q);
  const size_t qo = (size_t)t.q * 4;
  for (long long r = t.r0 + t.tp; r < t.r1; r += 4LL * t.ppi) {
    float4 v[4], s[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long rr = r + (long long)k * t.ppi;
      ok[k] = rr < t.r1;
      const size_t o = (size_t)(ok[k] ? rr : t.r0) * C + qo;
      v[k] = ld4(x + o);
      s[k] = residual ? ld4(residual + o) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!ok[k]) continue;
      float4 o = p.z(p.xh(v[k]));
      if (relu_mode == 1) o = relu4(o);
      if (residual) o = add4(o, s[k]);
      if (relu_mode == 2) o = relu4(o);
      *reinterpret_cast<float4*>(y + (size_t)(r + (long long)k * t.ppi) * C + qo) = o;
    }
  }
}

// dz of one quad: dy through the fused ReLU's mask
__device__ __forceinline__ float4 bn_dz(float4 dy, float4 z, float4 yv, int relu_mode) {
  if (relu_mode == 0) return dy;
  const float4 m = relu_mode == 1 ? z : yv;
  return make_float4(m.x > 0.f ? dy.x : 0.f, m.y > 0.f ? dy.y : 0.f, m.z > 0.f ? dy.z : 0.f,
                     m.w > 0.f ? dy.w : 0.f);
}

// part [P, 2, C]: per chunk sum dz, sum dz * xh
__global__ __launch_bounds__(kBnThreads) void bn_bwd_reduce_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ y,
    long long M, int C, long long chunk_rows, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, int relu_mode, float* __restrict__ part) {
  __shared__ float s_1[kBnThreads * 4];
  __shared__ float s_2[kBnThreads * 4];
  const BnThread t(M, C, chunk_rows);
  float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f), a2 = a1;
  if (t.active) {
    const BnQuad p(mean, invstd, gamma, beta, t.q);
    const size_t qo = (size_t)t.q * 4;
    for (long long r = t.r0 + t.tp; r < t.r1; r += 4LL * t.ppi) {
      float4 v[4], g[4], yv[4];
      bool ok[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long rr = r + (long long)k * t.ppi;
        ok[k] = rr < t.r1;
        const size_t o = (size_t)(ok[k] ? rr : t.r0) * C + qo;
        v[k] = ld4(x + o);
        g[k] = ld4(dy + o);
        yv[k] = relu_mode == 2 ? ld4(y + o) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!ok[k]) continue;
        const float4 h = p.xh(v[k]);
        const float4 dz = bn_dz(g[k], p.z(h), yv[k], relu_mode);
        a1 = add4(a1, dz);
        a2.x += dz.x * h.x;
        a2.y += dz.y * h.y;
        a2.z += dz.z * h.z;
        a2.w += dz.w * h.w;
      }
    }
  }
  reinterpret_cast<float4*>(s_1)[threadIdx.x] = a1;
  reinterpret_cast<float4*>(s_2)[threadIdx.x] = a2;
  __syncthreads();
  const int QT = min(C / 4, kBnThreads);
  for (int cl = threadIdx.x; cl < QT * 4; cl += kBnThreads) {
    const int ql = cl >> 2, e = cl & 3;
    const int c = (blockIdx.y * QT + ql) * 4 + e;
    if (c >= C) continue;
    float b1 = 0.f, b2 = 0.f;
    for (int i = 0; i < t.ppi; ++i) {
      b1 += s_1[(i * QT + ql) * 4 + e];
      b2 += s_2[(i * QT + ql) * 4 + e];
    }
    part[((size_t)blockIdx.x * 2) * C + c] = b1;
    part[((size_t)blockIdx.x * 2 + 1) * C + c] = b2;
  }
}

// sums [2C] = the P rows of part [P, 2C] added in bn_merge_kernel's two-level
// order: each of kBnSlices runs of consecutive rows in order, then the runs.
__global__ __launch_bounds__(kBnCols* kBnSlices) void bn_sum_kernel(
    const float* __restrict__ part, int P, int C2, float* __restrict__ sums) {
  __shared__ float s_p[kBnSlices][kBnCols];
  const int col = threadIdx.x % kBnCols, slice = threadIdx.x / kBnCols;
  const int j = blockIdx.x * kBnCols + col;
  const int per = (P + kBnSlices - 1) / kBnSlices;
  const int i0 = slice * per, i1 = min(P, i0 + per);
  float s = 0.f;
  if (j < C2)
    for (int i = i0; i < i1; ++i) s += part[(size_t)i * C2 + j];
  s_p[slice][col] = s;
  __syncthreads();
  if (slice != 0 || j >= C2) return;
  s = s_p[0][col];
  for (int i = 1; i < kBnSlices; ++i) s += s_p[i][col];
  sums[j] = s;
}

__global__ __launch_bounds__(kBnThreads) void bn_bwd_apply_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ y,
    long long M, int C, long long chunk_rows, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, int relu_mode, const float* __restrict__ sums,
    float inv_total, float* __restrict__ dx, float* __restrict__ dres) {
  const BnThread t(M, C, chunk_rows);
  if (!t.active) return;
  const BnQuad p(mean, invstd, gamma, beta, t.q);
  const size_t qo = (size_t)t.q * 4;
  const float4 s1 = ld4(sums + qo), s2 = ld4(sums + C + qo);
  const float4 k1 = make_float4(s1.x * inv_total, s1.y * inv_total, s1.z * inv_total,
                                s1.w * inv_total);
  const float4 k2 = make_float4(s2.x * inv_total, s2.y * inv_total, s2.z * inv_total,
                                s2.w * inv_total);
  const float4 gi = make_float4(p.g.x * p.is.x, p.g.y * p.is.y, p.g.z * p.is.z, p.g.w * p.is.w);
  for (long long r = t.r0 + t.tp; r < t.r1; r += 4LL * t.ppi) {
    float4 v[4], g[4], yv[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long rr = r + (long long)k * t.ppi;
      ok[k] = rr < t.r1;
      const size_t o = (size_t)(ok[k] ? rr : t.r0) * C + qo;
      v[k] = ld4(x + o);
      g[k] = ld4(dy + o);
      yv[k] = relu_mode == 2 ? ld4(y + o) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!ok[k]) continue;
      const float4 h = p.xh(v[k]);
      const float4 dz = bn_dz(g[k], p.z(h), yv[k], relu_mode);
      float4 o;
      o.x = gi.x * ((dz.x - k1.x) - h.x * k2.x);
      o.y = gi.y * ((dz.y - k1.y) - h.y * k2.y);
      o.z = gi.z * ((dz.z - k1.z) - h.z * k2.z);
      o.w = gi.w * ((dz.w - k1.w) - h.w * k2.w);
      const size_t off = (size_t)(r + (long long)k * t.ppi) * C + qo;
      *reinterpret_cast<float4*>(dx + off) = o;
      if (dres) *reinterpret_cast<float4*>(dres + off) = dz;
    }
  }
}

// per-chunk counts and [P, C] means and M2s
struct BnStatsSpace {
  float *cnt, *mean, *m2;
  template <typename A>
  void lay(A& a, int P, int C) {
    cnt = a.template take<float>((size_t)P);
    mean = a.template take<float>((size_t)P * C);
    m2 = a.template take<float>((size_t)P * C);
  }
};

// per-chunk [2, C] partial sums
struct BnBwdSpace {
  float* part;
  template <typename A>
  void lay(A& a, int P, int C) {
    part = a.template take<float>((size_t)P * 2 * C);
  }
};

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace d2mi

using namespace d2mi;

#define BN_REQUIRE_SHAPE(M, C)                                                          \
  D2MI_REQUIRE((M) >= 1 && (C) > 0, "BatchNorm: M >= 1 rows and C > 0 channels");       \
  D2MI_REQUIRE((C) % 4 == 0, "BatchNorm: C must be a multiple of 4 (got %d)", (int)(C))

extern "C" size_t d2mi_bn_train_stats_workspace_size(long long M, int C) {
  if (M < 1 || C <= 0 || C % 4) return 0;
  return layout_bytes<BnStatsSpace>(bn_plan(M, C).P, C);
}

extern "C" int d2mi_bn_train_stats(const float* x, long long M, int C, float* triple,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  BN_REQUIRE_SHAPE(M, C);
  const BnPlan pl = bn_plan(M, C);
  Workspace w(workspace, workspace_bytes);
  BnStatsSpace o;
  o.lay(w, pl.P, C);
  D2MI_REQUIRE(w.ok(), "BatchNorm statistics workspace too small (%zu < %zu)", workspace_bytes,
               w.off);
  D2MI_REQUIRE(x && triple, "BatchNorm statistics: null x or triple");
  D2MI_REQUIRE(aligned16(x), "BatchNorm operands must be 16-B aligned");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(bn_stats_kernel, dim3(pl.P, pl.tiles), dim3(kBnThreads), 0, st, x, M, C,
                     pl.chunk_rows, o.cnt, o.mean, o.m2);
  D2MI_LAUNCH_CHECK();
  hipLaunchKernelGGL((bn_merge_kernel<false>), dim3((C + kBnCols - 1) / kBnCols),
                     dim3(kBnCols * kBnSlices), 0, st, o.cnt, 1LL,
                     o.mean, o.m2, (long long)C, pl.P, C, 0.f, 0.f, nullptr, nullptr, nullptr,
                     nullptr, nullptr, triple);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" int d2mi_bn_train_finalize(const float* triples, int P, int C, float eps, float decay,
                                      float* moving_mean, float* moving_var, float* mean,
                                      float* var, float* invstd, void* stream) {
  D2MI_REQUIRE(P >= 1 && C > 0, "BatchNorm finalize: P >= 1 triples and C > 0 channels");
  D2MI_REQUIRE(C % 4 == 0, "BatchNorm: C must be a multiple of 4 (got %d)", C);
  D2MI_REQUIRE(moving_mean && moving_var,
               "BatchNorm finalize: null moving_mean / moving_variance buffer");
  D2MI_REQUIRE(triples && mean && var && invstd, "BatchNorm finalize: null operand");
  D2MI_REQUIRE(eps > 0.f && decay >= 0.f && decay <= 1.f,
               "BatchNorm finalize: eps > 0 and decay in [0, 1]");
  const long long stride = 2LL * C + 1;
  hipLaunchKernelGGL((bn_merge_kernel<true>), dim3((C + kBnCols - 1) / kBnCols),
                     dim3(kBnCols * kBnSlices), 0, as_stream(stream), triples, stride, triples + 1, triples + 1 + C, stride, P, C, eps, decay,
                     moving_mean, moving_var, mean, var, invstd, nullptr);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" int d2mi_bn_train_apply(const float* x, long long M, int C, const float* mean,
                                   const float* invstd, const float* gamma, const float* beta,
                                   const float* residual, int relu_mode, float* y, void* stream) {
  BN_REQUIRE_SHAPE(M, C);
  D2MI_REQUIRE(relu_mode >= 0 && relu_mode <= 2, "BatchNorm: relu_mode is 0, 1 or 2");
  D2MI_REQUIRE(x && y && mean && invstd, "BatchNorm apply: null operand");
  D2MI_REQUIRE(aligned16(x) && aligned16(y) && aligned16(mean) && aligned16(invstd) &&
                   aligned16(gamma) && aligned16(beta) && aligned16(residual),
               "BatchNorm operands must be 16-B aligned");
  const BnPlan pl = bn_plan(M, C);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(pl.P, pl.tiles), dim3(kBnThreads), 0,
                     as_stream(stream), x, M, C, pl.chunk_rows, mean, invstd, gamma, beta,
                     residual, relu_mode, y);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t d2mi_bn_train_bwd_reduce_workspace_size(long long M, int C) {
  if (M < 1 || C <= 0 || C % 4) return 0;
  return layout_bytes<BnBwdSpace>(bn_plan(M, C).P, C);
}

extern "C" int d2mi_bn_train_bwd_reduce(const float* x, const float* dy, const float* y,
                                        long long M, int C, const float* mean,
                                        const float* invstd, const float* gamma,
                                        const float* beta, int relu_mode, float* sums,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  BN_REQUIRE_SHAPE(M, C);
  D2MI_REQUIRE(relu_mode >= 0 && relu_mode <= 2, "BatchNorm: relu_mode is 0, 1 or 2");
  const BnPlan pl = bn_plan(M, C);
  Workspace w(workspace, workspace_bytes);
  BnBwdSpace o;
  o.lay(w, pl.P, C);
  D2MI_REQUIRE(w.ok(), "BatchNorm backward workspace too small (%zu < %zu)", workspace_bytes,
               w.off);
  D2MI_REQUIRE(x && dy && mean && invstd && sums, "BatchNorm backward: null operand");
  D2MI_REQUIRE(relu_mode != 2 || y, "BatchNorm backward: relu_mode 2 reads y");
  D2MI_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(y) && aligned16(mean) &&
                   aligned16(invstd) && aligned16(gamma) && aligned16(beta),
               "BatchNorm operands must be 16-B aligned");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(pl.P, pl.tiles), dim3(kBnThreads), 0, st, x, dy, y,
                     M, C, pl.chunk_rows, mean, invstd, gamma, beta, relu_mode, o.part);
  D2MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_sum_kernel, dim3((2 * C + kBnCols - 1) / kBnCols),
                     dim3(kBnCols * kBnSlices), 0, st, o.part, pl.P, 2 * C, sums);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" int d2mi_bn_train_bwd_apply(const float* x, const float* dy, const float* y,
                                       long long M, int C, const float* mean,
                                       const float* invstd, const float* gamma,
                                       const float* beta, int relu_mode, const float* sums,
                                       float total_count, float* dx, float* dresidual,
                                       void* stream) {
  BN_REQUIRE_SHAPE(M, C);
  D2MI_REQUIRE(relu_mode >= 0 && relu_mode <= 2, "BatchNorm: relu_mode is 0, 1 or 2");
  D2MI_REQUIRE(total_count >= 1.f, "BatchNorm backward: total_count >= 1");
  D2MI_REQUIRE(x && dy && mean && invstd && sums && dx, "BatchNorm backward: null operand");
  D2MI_REQUIRE(relu_mode != 2 || y, "BatchNorm backward: relu_mode 2 reads y");
  D2MI_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(y) && aligned16(mean) &&
                   aligned16(invstd) && aligned16(gamma) && aligned16(beta) && aligned16(sums) &&
                   aligned16(dx) && aligned16(dresidual),
               "BatchNorm operands must be 16-B aligned");
  const BnPlan pl = bn_plan(M, C);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(pl.P, pl.tiles), dim3(kBnThreads), 0,
                     as_stream(stream), x, dy, y, M, C, pl.chunk_rows, mean, invstd, gamma, beta,
                     relu_mode, sums, 1.f / total_count, dx, dresidual);
  D2MI_LAUNCH_CHECK();
  return 0;
}
