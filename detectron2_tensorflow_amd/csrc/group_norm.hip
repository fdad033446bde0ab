// GroupNorm on NHWC (lib/layers/normalization.py:174-260: tf.nn.moments over
// (H, W, channels of the group), then tf.nn.batch_normalization:
// inv = rsqrt(var + eps) * gamma, y = x * inv + (beta - mean * inv)), with
// the ops that follow it in the SOLOv2 heads fused into the apply pass:
// ReLU (the conv's activation, solo_v2.py:173-183 / :659-669), the nearest
// x2 upsample of MaskFeatureBranch (wrappers.py:104-116 — the reference's
// Upsample ignores its method) and the running sum of the scale heads
// (solo_v2.py:705-721: res = res + head(feature)).
//
// Five launches, deterministic (fixed-order reductions, no atomics):
//   gn_sum_kernel        per (image, pixel chunk) per-group partial sums
//   gn_reduce_kernel     -> mean
//   gn_sum_kernel        per-group partial sums of (x - mean)^2 (the
//                        two-pass variance of tf.nn.moments)
//   gn_reduce_kernel     -> var
//   gn_apply_kernel      per-channel inv / shift, apply (+ ReLU, up2, sum)
// Each pass reads x once (float4 over channels, coalesced whole pixels).
#include <algorithm>

#include "common.h"
#include "wave.h"

namespace d2mi {
namespace {

constexpr int kGnThreads = 256;
constexpr int kGnMaxGroups = 64;

// partial[(n * chunks + chunk) * G + g]
__global__ __launch_bounds__(kGnThreads) void gn_sum_kernel(const float* __restrict__ x, int HW,
                                                           int C, int G, int chunk_px,
                                                           const float* __restrict__ mean,
                                                           float* __restrict__ partial) {
  __shared__ float red[kGnThreads];
  const int chunk = blockIdx.x, n = blockIdx.y, chunks = gridDim.x;
  const int C4 = C / 4;
  const int tc = threadIdx.x % C4;             // this thread's channel quad
  const int tp = threadIdx.x / C4;             // pixel slot
  const int ppi = kGnThreads / C4;             // pixels per iteration
  const int cpg = C / G;                       // channels per group
  const int g = tc * 4 / cpg;                  // the group of the quad (cpg % 4 == 0)
  const float mu = mean ? mean[n * G + g] : 0.f;
  const int p0 = chunk * chunk_px, p1 = min(HW, p0 + chunk_px);
  const float* xb = x + (size_t)n * HW * C;
  float acc = 0.f;
  if (threadIdx.x < ppi * C4) {
    for (int p = p0 + tp; p < p1; p += ppi) {
      const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)p * C + tc * 4);
      if (mean) {
        const float a = v.x - mu, b = v.y - mu, c = v.z - mu, d = v.w - mu;
        acc += (a * a + b * b) + (c * c + d * d);
      } else {
        acc += (v.x + v.y) + (v.z + v.w);
      }
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  // per group: the quads of the group over every pixel slot, fixed order
  for (int gg = threadIdx.x; gg < G; gg += kGnThreads) {
    float s = 0.f;
    const int q0 = gg * cpg / 4, q1 = (gg + 1) * cpg / 4;
    for (int t = 0; t < ppi; ++t)
      for (int q = q0; q < q1; ++q) s += red[t * C4 + q];
    partial[((size_t)n * chunks + chunk) * G + gg] = s;
  }
}

// mean[n * G + g] (or var) = sum over chunks / count
__global__ void gn_reduce_kernel(const float* __restrict__ partial, int chunks, int G, float inv_count,
                                 float* __restrict__ out) {
  const int n = blockIdx.x;
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += partial[((size_t)n * chunks + c) * G + g];
    out[n * G + g] = s * inv_count;
  }
}

// y = x * inv + shift (+ ReLU); up2: each pixel to its 2x2 block of the
// output [N, 2H, 2W, C]; accumulate: y += instead of y =.
template <bool UP2, bool ACC>
__global__ __launch_bounds__(kGnThreads) void gn_apply_kernel(
    const float* __restrict__ x, int H, int W, int C, int G, const float* __restrict__ mean,
    const float* __restrict__ var, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, int relu, float* __restrict__ y, int N) {
  const int C4 = C / 4, cpg = C / G;
  const size_t total = (size_t)N * H * W * C4;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total;
       e += (size_t)gridDim.x * blockDim.x) {
    const int q = (int)(e % C4);
    const size_t px = e / C4;
    const int n = (int)(px / ((size_t)H * W));
    const int c = q * 4;
    const int g = c / cpg;
    const float mu = mean[n * G + g];
    const float r = rsqrtf(var[n * G + g] + eps);
    const float4 v = *reinterpret_cast<const float4*>(x + px * C + c);
    const float4 gm = *reinterpret_cast<const float4*>(gamma + c);
    const float4 bt = *reinterpret_cast<const float4*>(beta + c);
    float4 o;
    {
      const float i0 = r * gm.x, i1 = r * gm.y, i2 = r * gm.z, i3 = r * gm.w;
      o.x = v.x * i0 + (bt.x - mu * i0);
      o.y = v.y * i1 + (bt.y - mu * i1);
      o.z = v.z * i2 + (bt.z - mu * i2);
      o.w = v.w * i3 + (bt.w - mu * i3);
    }
    if (relu) {
      o.x = fmaxf(o.x, 0.f);
      o.y = fmaxf(o.y, 0.f);
      o.z = fmaxf(o.z, 0.f);
      o.w = fmaxf(o.w, 0.f);
    }
    if (!UP2) {
      float4* d = reinterpret_cast<float4*>(y + px * C + c);
      if (ACC) {
        const float4 t = *d;
        o.x = t.x + o.x;
        o.y = t.y + o.y;
        o.z = t.z + o.z;
        o.w = t.w + o.w;
      }
      *d = o;
    } else {
      const int rem = (int)(px - (size_t)n * H * W);
      const int h = rem / W, w = rem - h * W;
      const int OW = 2 * W;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          float4* d = reinterpret_cast<float4*>(
              y + (((size_t)n * 2 * H + 2 * h + dy) * OW + 2 * w + dx) * C + c);
          float4 oo = o;
          if (ACC) {
            const float4 t = *d;
            oo.x = t.x + o.x;
            oo.y = t.y + o.y;
            oo.z = t.z + o.z;
            oo.w = t.w + o.w;
          }
          *d = oo;
        }
    }
  }
}

static int gn_chunks(int HW, int& chunk_px) {
  // ~32 pixel-chunks per image (enough workgroups for N >= 2 at every SOLO
  // level), at least 16 pixels each
  int chunks = std::max(1, std::min(64, HW / 16));
  chunk_px = (HW + chunks - 1) / chunks;
  chunks = (HW + chunk_px - 1) / chunk_px;
  return chunks;
}

// ---------------------------------------------------------------- levels
// Multi-level GroupNorm (d2mi_group_norm_nhwc_levels): the same layer over
// up to six feature levels (the SOLOv2 tower GroupNorms after a multi-level
// conv launch) in five launches total instead of five per level.  Level l's
// sum workgroups are [wg0[l], wg0[l + 1]) (one per (image, chunk): the
// partial row of that index), its statistics rows [st0[l], st0[l + 1]) (one
// per image), its apply elements [e0[l], e0[l + 1]) (float4 quads).  Per
// level the arithmetic is gn_sum / gn_reduce / gn_apply's, in the same order.
constexpr int kGnMaxLevels = 6;
struct GnLevels {
  const float* x[kGnMaxLevels];
  float* y[kGnMaxLevels];
  int HW[kGnMaxLevels], chunks[kGnMaxLevels], chunk_px[kGnMaxLevels];
  float inv_count[kGnMaxLevels];
  int wg0[kGnMaxLevels + 1], st0[kGnMaxLevels + 1];
  long long e0[kGnMaxLevels + 1];
  int L;
};

__global__ __launch_bounds__(kGnThreads) void gn_sum_levels_kernel(GnLevels lv, int C, int G,
                                                                  const float* __restrict__ mean,
                                                                  float* __restrict__ partial) {
  __shared__ float red[kGnThreads];
  const int l = level_of(lv.wg0, lv.L, (int)blockIdx.x);
  const int local = blockIdx.x - lv.wg0[l];
  const int chunks = lv.chunks[l];
  const int n = local / chunks, chunk = local - n * chunks;
  const int HW = lv.HW[l];
  const int C4 = C / 4;
  const int tc = threadIdx.x % C4;
  const int tp = threadIdx.x / C4;
  const int ppi = kGnThreads / C4;
  const int cpg = C / G;
  const int g = tc * 4 / cpg;
  const int srow = lv.st0[l] + n;
  const float mu = mean ? mean[srow * G + g] : 0.f;
  const int p0 = chunk * lv.chunk_px[l], p1 = min(HW, p0 + lv.chunk_px[l]);
  const float* xb = lv.x[l] + (size_t)n * HW * C;
  float acc = 0.f;
  if (threadIdx.x < ppi * C4) {
    for (int p = p0 + tp; p < p1; p += ppi) {
      const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)p * C + tc * 4);
      if (mean) {
        const float a = v.x - mu, b = v.y - mu, c = v.z - mu, d = v.w - mu;
        acc += (a * a + b * b) + (c * c + d * d);
      } else {
        acc += (v.x + v.y) + (v.z + v.w);
      }
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int gg = threadIdx.x; gg < G; gg += kGnThreads) {
    float sum = 0.f;
    const int q0 = gg * cpg / 4, q1 = (gg + 1) * cpg / 4;
    for (int t = 0; t < ppi; ++t)
      for (int q = q0; q < q1; ++q) sum += red[t * C4 + q];
    partial[(size_t)blockIdx.x * G + gg] = sum;
  }
}

// one workgroup per (level, image): out[row * G + g] = sum over its chunks / count
__global__ void gn_reduce_levels_kernel(GnLevels lv, const float* __restrict__ partial, int G,
                                        float* __restrict__ out) {
  const int row = blockIdx.x;
  const int l = level_of(lv.st0, lv.L, row);
  const int n = row - lv.st0[l];
  const int chunks = lv.chunks[l];
  const size_t base = (size_t)lv.wg0[l] + (size_t)n * chunks;
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    float sum = 0.f;
    for (int c = 0; c < chunks; ++c) sum += partial[(base + c) * G + g];
    out[row * G + g] = sum * lv.inv_count[l];
  }
}

__global__ __launch_bounds__(kGnThreads) void gn_apply_levels_kernel(
    GnLevels lv, int C, int G, const float* __restrict__ mean, const float* __restrict__ var,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu) {
  const int C4 = C / 4, cpg = C / G;
  const long long total = lv.e0[lv.L];
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    int l = 0;
    while (l + 1 < lv.L && e >= lv.e0[l + 1]) ++l;
    const long long le = e - lv.e0[l];
    const int q = (int)(le % C4);
    const long long px = le / C4;
    const int n = (int)(px / lv.HW[l]);
    const int c = q * 4;
    const int g = c / cpg;
    const int srow = lv.st0[l] + n;
    const float mu = mean[srow * G + g];
    const float r = rsqrtf(var[srow * G + g] + eps);
    const float4 v = *reinterpret_cast<const float4*>(lv.x[l] + px * C + c);
    const float4 gm = *reinterpret_cast<const float4*>(gamma + c);
    const float4 bt = *reinterpret_cast<const float4*>(beta + c);
    float4 o;
    const float i0 = r * gm.x, i1 = r * gm.y, i2 = r * gm.z, i3 = r * gm.w;
    o.x = v.x * i0 + (bt.x - mu * i0);
    o.y = v.y * i1 + (bt.y - mu * i1);
    o.z = v.z * i2 + (bt.z - mu * i2);
    o.w = v.w * i3 + (bt.w - mu * i3);
    if (relu) {
      o.x = fmaxf(o.x, 0.f);
      o.y = fmaxf(o.y, 0.f);
      o.z = fmaxf(o.z, 0.f);
      o.w = fmaxf(o.w, 0.f);
    }
    *reinterpret_cast<float4*>(lv.y[l] + px * C + c) = o;
  }
}

// level table + workspace layout of a multi-level call
static int gn_levels_plan(const int32_t* dims, int nlev, int C, int G, GnLevels& lv,
                          size_t& n_partial, size_t& n_stats) {
  lv = GnLevels{};
  lv.L = nlev;
  int wg = 0, st = 0;
  long long e = 0;
  for (int l = 0; l < nlev; ++l) {
    const int N = dims[3 * l], H = dims[3 * l + 1], W = dims[3 * l + 2];
    if (N < 0 || H <= 0 || W <= 0) return -1;
    lv.HW[l] = H * W;
    lv.chunks[l] = gn_chunks(H * W, lv.chunk_px[l]);
    lv.inv_count[l] = 1.f / (float)((size_t)H * W * (C / G));
    lv.wg0[l] = wg;
    lv.st0[l] = st;
    lv.e0[l] = e;
    wg += N * lv.chunks[l];
    st += N;
    e += (long long)N * H * W * (C / 4);
  }
  lv.wg0[nlev] = wg;
  lv.st0[nlev] = st;
  lv.e0[nlev] = e;
  n_partial = (size_t)wg * G;
  n_stats = (size_t)st * G;
  return 0;
}

// n_partial per-chunk group sums, n_stats means and variances (both ops)
struct GnSpace {
  float *partial, *mean, *var;
  template <typename A>
  void lay(A& a, size_t n_partial, size_t n_stats) {
    partial = a.template take<float>(n_partial);
    mean = a.template take<float>(n_stats);
    var = a.template take<float>(n_stats);
  }
};

// -------------------------------------------------------------- training
// GroupNorm with a gradient (d2mi_group_norm_train_fwd / _bwd).  The forward
// is the five launches above on caller-owned mean / var [N, G] (the same
// kernels, grids and chunking: the same bits as d2mi_group_norm_nhwc), with
// gn_sum_wide_kernel in place of gn_sum_kernel where C / 4 > 256.  The
// backward, with dz = dy through the ReLU's mask (z recomputed by the
// forward's own expression), xh = (x - mean) * r, r = rsqrt(var + eps):
//   gn_bwd_reduce_kernel  one read of x and dy: per (image, chunk, channel)
//                         sum dz and sum dz * xh
//   gn_bwd_chunks_kernel  per image: its chunks in a fixed two-level order ->
//                         per (image, channel) sums (skipped at one chunk)
//   gn_bwd_finalize_kernel S1 / S2 per (image, group) = sum over the group's
//                         channels of gamma_c * those; and the images in a
//                         fixed two-level order -> dbeta, dgamma
//   gn_bwd_apply_kernel   dx = r * (dz * gamma - S1 / m - xh * S2 / m)
// The streaming kernels map a workgroup to (image, pixel chunk); a thread
// keeps one channel quad's constants in registers and walks whole pixels
// (tiles of 256 quads in turn where C / 4 > 256).  The chunk count comes from
// the shape (gn_bwd_plan): about 1024 workgroups over all images.
constexpr int kGnTrainMaxC = 2048;
constexpr int kGnBwdMaxChunks = 256;
constexpr int kGnAffCols = 8, kGnAffSlices = 32;
constexpr int kGnSumCols = 32, kGnSumSlices = 8;

__global__ __launch_bounds__(kGnThreads) void gn_sum_wide_kernel(const float* __restrict__ x,
                                                                int HW, int C, int G,
                                                                int chunk_px,
                                                                const float* __restrict__ mean,
                                                                float* __restrict__ partial) {
  __shared__ float red[kGnTrainMaxC / 4];
  const int chunk = blockIdx.x, n = blockIdx.y, chunks = gridDim.x;
  const int C4 = C / 4, cpg = C / G;
  const int p0 = chunk * chunk_px, p1 = min(HW, p0 + chunk_px);
  const float* xb = x + (size_t)n * HW * C;
  for (int q = threadIdx.x; q < C4; q += kGnThreads) {
    const float mu = mean ? mean[n * G + q * 4 / cpg] : 0.f;
    float acc = 0.f;
    for (int p = p0; p < p1; ++p) {
      const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)p * C + q * 4);
      if (mean) {
        const float a = v.x - mu, b = v.y - mu, c = v.z - mu, d = v.w - mu;
        acc += (a * a + b * b) + (c * c + d * d);
      } else {
        acc += (v.x + v.y) + (v.z + v.w);
      }
    }
    red[q] = acc;
  }
  __syncthreads();
  for (int gg = threadIdx.x; gg < G; gg += kGnThreads) {
    float s = 0.f;
    const int q0 = gg * cpg / 4, q1 = (gg + 1) * cpg / 4;
    for (int q = q0; q < q1; ++q) s += red[q];
    partial[((size_t)n * chunks + chunk) * G + gg] = s;
  }
}

struct GnBwdPlan {
  int chunks, chunk_px;
};

static GnBwdPlan gn_bwd_plan(int N, int HW, int C) {
  // about 1024 workgroups (four per CU) over all images, every pixel slot of
  // a workgroup at least four pixels: [2,200,336,256] takes 256 chunks per
  // image, [1024,7,7,256] one
  const int ppi = kGnThreads / std::min(C / 4, kGnThreads);
  const int want = (1024 + N - 1) / std::max(N, 1);
  const int most = std::max(1, HW / (4 * ppi));
  GnBwdPlan p;
  p.chunks = std::max(1, std::min(std::min(want, most), kGnBwdMaxChunks));
  p.chunk_px = (HW + p.chunks - 1) / p.chunks;
  p.chunks = (HW + p.chunk_px - 1) / p.chunk_px;
  return p;
}

// the constants of one (image, channel quad): the forward's inv and shift
// (z = x * inv + shift is gn_apply_kernel's expression, bit for bit)
struct GnQuad {
  float mu, r;
  float4 gm, inv, shift;
  __device__ GnQuad(const float* mean, const float* var, const float* gamma, const float* beta,
                    float eps, int n, int G, int cpg, int c) {
    const int g = c / cpg;
    mu = mean[n * G + g];
    r = rsqrtf(var[n * G + g] + eps);
    gm = *reinterpret_cast<const float4*>(gamma + c);
    const float4 bt = *reinterpret_cast<const float4*>(beta + c);
    inv = make_float4(r * gm.x, r * gm.y, r * gm.z, r * gm.w);
    shift = make_float4(bt.x - mu * inv.x, bt.y - mu * inv.y, bt.z - mu * inv.z,
                        bt.w - mu * inv.w);
  }
  __device__ __forceinline__ float4 xh(float4 v) const {
    return make_float4((v.x - mu) * r, (v.y - mu) * r, (v.z - mu) * r, (v.w - mu) * r);
  }
  // dy where the forward's ReLU passed
  __device__ __forceinline__ float4 dz(float4 v, float4 dy, int relu) const {
    if (!relu) return dy;
    const float z0 = v.x * inv.x + shift.x, z1 = v.y * inv.y + shift.y;
    const float z2 = v.z * inv.z + shift.z, z3 = v.w * inv.w + shift.w;
    return make_float4(z0 > 0.f ? dy.x : 0.f, z1 > 0.f ? dy.y : 0.f, z2 > 0.f ? dy.z : 0.f,
                       z3 > 0.f ? dy.w : 0.f);
  }
};

// workgroup b = n * chunks + chunk; part[(b * 2 + k) * C + c], k = 0: sum dz,
// k = 1: sum dz * xh over the chunk's pixels (pixel slots added in slot order)
__global__ __launch_bounds__(kGnThreads) void gn_bwd_reduce_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, int HW, int C, int G, int chunks,
    int chunk_px, const float* __restrict__ mean, const float* __restrict__ var,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu,
    float* __restrict__ part) {
  __shared__ float s_1[kGnThreads * 4];
  __shared__ float s_2[kGnThreads * 4];
  const int n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
  const int C4 = C / 4, cpg = C / G;
  const int QT = min(C4, kGnThreads), ppi = kGnThreads / QT;
  const int tq = threadIdx.x % QT, tp = threadIdx.x / QT;
  const int p0 = chunk * chunk_px, p1 = min(HW, p0 + chunk_px);
  const size_t base = (size_t)n * HW * C;
  float* out = part + (size_t)blockIdx.x * 2 * C;
  for (int q0 = 0; q0 < C4; q0 += QT) {
    const int q = q0 + tq;
    float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f), a2 = a1;
    if (tp < ppi && q < C4) {
      const GnQuad k(mean, var, gamma, beta, eps, n, G, cpg, q * 4);
      for (int p = p0 + tp; p < p1; p += 2 * ppi) {
        // two pixels in flight (the second re-reads the first where it is past the end)
        const bool ok = p + ppi < p1;
        const size_t o0 = base + (size_t)p * C + q * 4;
        const size_t o1 = base + (size_t)(ok ? p + ppi : p) * C + q * 4;
        const float4 v0 = *reinterpret_cast<const float4*>(x + o0);
        const float4 g0 = *reinterpret_cast<const float4*>(dy + o0);
        const float4 v1 = *reinterpret_cast<const float4*>(x + o1);
        const float4 g1 = *reinterpret_cast<const float4*>(dy + o1);
        {
          const float4 h = k.xh(v0), d = k.dz(v0, g0, relu);
          a1.x += d.x; a1.y += d.y; a1.z += d.z; a1.w += d.w;
          a2.x += d.x * h.x; a2.y += d.y * h.y; a2.z += d.z * h.z; a2.w += d.w * h.w;
        }
        if (ok) {
          const float4 h = k.xh(v1), d = k.dz(v1, g1, relu);
          a1.x += d.x; a1.y += d.y; a1.z += d.z; a1.w += d.w;
          a2.x += d.x * h.x; a2.y += d.y * h.y; a2.z += d.z * h.z; a2.w += d.w * h.w;
        }
      }
    }
    reinterpret_cast<float4*>(s_1)[threadIdx.x] = a1;
    reinterpret_cast<float4*>(s_2)[threadIdx.x] = a2;
    __syncthreads();
    for (int cl = threadIdx.x; cl < QT * 4; cl += kGnThreads) {
      const int ql = cl >> 2, e = cl & 3;
      const int c = (q0 + ql) * 4 + e;
      if (c >= C) continue;
      float b1 = 0.f, b2 = 0.f;
      for (int i = 0; i < ppi; ++i) {
        b1 += s_1[(i * QT + ql) * 4 + e];
        b2 += s_2[(i * QT + ql) * 4 + e];
      }
      out[c] = b1;
      out[C + c] = b2;
    }
    __syncthreads();
  }
}

// pn[n * 2C + j] = the image's chunks of column j (k * C + c) added in a
// two-level order: each of kGnSumSlices runs of consecutive chunks in order,
// then the runs (256 serial steps in two workgroups would cost more than the
// reduce pass at two images of a SOLOv2 level)
__global__ __launch_bounds__(kGnSumCols* kGnSumSlices) void gn_bwd_chunks_kernel(
    const float* __restrict__ part, int chunks, int C2, float* __restrict__ pn) {
  __shared__ float s_p[kGnSumSlices][kGnSumCols];
  const int col = threadIdx.x % kGnSumCols, slice = threadIdx.x / kGnSumCols;
  const int j = blockIdx.x * kGnSumCols + col, n = blockIdx.y;
  const int per = (chunks + kGnSumSlices - 1) / kGnSumSlices;
  const int i0 = slice * per, i1 = min(chunks, i0 + per);
  const float* rows = part + (size_t)n * chunks * C2;
  float s = 0.f;
  if (j < C2)
    for (int i = i0; i < i1; ++i) s += rows[(size_t)i * C2 + j];
  s_p[slice][col] = s;
  __syncthreads();
  if (slice != 0 || j >= C2) return;
  s = s_p[0][col];
  for (int i = 1; i < kGnSumSlices; ++i) s += s_p[i][col];
  pn[(size_t)n * C2 + j] = s;
}

// Workgroups [0, images): S[(n * G + g) * 2 + k] of image n = sum over the
// group's channels, in channel order, of gamma_c * pn[n][k][c].  The others,
// kGnAffCols columns each: dbeta [C] / dgamma [C] = the N rows of pn [N, 2C]
// added in a two-level order, each of kGnAffSlices runs of consecutive images
// in order, then the runs (N serial steps per thread would cost more than the
// reduce pass at the box head's 1024 images).
__global__ __launch_bounds__(kGnThreads) void gn_bwd_finalize_kernel(
    const float* __restrict__ pn, int N, int C, int G, int images,
    const float* __restrict__ gamma, float* __restrict__ S, float* __restrict__ dgamma,
    float* __restrict__ dbeta) {
  __shared__ float s_1[kGnTrainMaxC];
  __shared__ float s_2[kGnTrainMaxC];
  if ((int)blockIdx.x < images) {
    const int n = blockIdx.x, cpg = C / G;
    for (int c = threadIdx.x; c < C; c += kGnThreads) {
      const float gm = gamma[c];
      s_1[c] = pn[((size_t)n * 2) * C + c] * gm;
      s_2[c] = pn[((size_t)n * 2 + 1) * C + c] * gm;
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += kGnThreads) {
      float t1 = 0.f, t2 = 0.f;
      for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
        t1 += s_1[c];
        t2 += s_2[c];
      }
      S[((size_t)n * G + g) * 2] = t1;
      S[((size_t)n * G + g) * 2 + 1] = t2;
    }
    return;
  }
  static_assert(kGnAffCols * kGnAffSlices == kGnThreads, "one thread per (column, run)");
  const int col = threadIdx.x % kGnAffCols, slice = threadIdx.x / kGnAffCols;
  const int j = ((int)blockIdx.x - images) * kGnAffCols + col;
  const int per = (N + kGnAffSlices - 1) / kGnAffSlices;
  const int i0 = slice * per, i1 = min(N, i0 + per);
  float s = 0.f;
  if (j < 2 * C)
    for (int i = i0; i < i1; ++i) s += pn[(size_t)i * 2 * C + j];
  s_1[slice * kGnAffCols + col] = s;
  __syncthreads();
  if (slice != 0 || j >= 2 * C) return;
  s = s_1[col];
  for (int i = 1; i < kGnAffSlices; ++i) s += s_1[i * kGnAffCols + col];
  if (j < C) {
    if (dbeta) dbeta[j] = s;
  } else if (dgamma) {
    dgamma[j - C] = s;
  }
}

__global__ __launch_bounds__(kGnThreads) void gn_bwd_apply_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, int HW, int C, int G, int chunks,
    int chunk_px, const float* __restrict__ mean, const float* __restrict__ var,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu,
    const float* __restrict__ S, float inv_m, float* __restrict__ dx) {
  const int n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
  const int C4 = C / 4, cpg = C / G;
  const int QT = min(C4, kGnThreads), ppi = kGnThreads / QT;
  const int tq = threadIdx.x % QT, tp = threadIdx.x / QT;
  if (tp >= ppi) return;
  const int p0 = chunk * chunk_px, p1 = min(HW, p0 + chunk_px);
  const size_t base = (size_t)n * HW * C;
  for (int q = tq; q < C4; q += QT) {
    const GnQuad k(mean, var, gamma, beta, eps, n, G, cpg, q * 4);
    const int g = q * 4 / cpg;
    const float k1 = S[((size_t)n * G + g) * 2] * inv_m;
    const float k2 = S[((size_t)n * G + g) * 2 + 1] * inv_m;
    for (int p = p0 + tp; p < p1; p += 2 * ppi) {
      const bool ok = p + ppi < p1;
      const size_t o0 = base + (size_t)p * C + q * 4;
      const size_t o1 = base + (size_t)(ok ? p + ppi : p) * C + q * 4;
      const float4 v0 = *reinterpret_cast<const float4*>(x + o0);
      const float4 g0 = *reinterpret_cast<const float4*>(dy + o0);
      const float4 v1 = *reinterpret_cast<const float4*>(x + o1);
      const float4 g1 = *reinterpret_cast<const float4*>(dy + o1);
      {
        const float4 h = k.xh(v0), d = k.dz(v0, g0, relu);
        float4 o;
        o.x = k.r * ((d.x * k.gm.x - k1) - h.x * k2);
        o.y = k.r * ((d.y * k.gm.y - k1) - h.y * k2);
        o.z = k.r * ((d.z * k.gm.z - k1) - h.z * k2);
        o.w = k.r * ((d.w * k.gm.w - k1) - h.w * k2);
        *reinterpret_cast<float4*>(dx + o0) = o;
      }
      if (ok) {
        const float4 h = k.xh(v1), d = k.dz(v1, g1, relu);
        float4 o;
        o.x = k.r * ((d.x * k.gm.x - k1) - h.x * k2);
        o.y = k.r * ((d.y * k.gm.y - k1) - h.y * k2);
        o.z = k.r * ((d.z * k.gm.z - k1) - h.z * k2);
        o.w = k.r * ((d.w * k.gm.w - k1) - h.w * k2);
        *reinterpret_cast<float4*>(dx + o1) = o;
      }
    }
  }
}

// per-(image, chunk) [2, C] partials, per-image [2, C] sums, S1 / S2 [N, G, 2]
struct GnBwdSpace {
  float *part, *pn, *S;
  template <typename A>
  void lay(A& a, size_t n_part, size_t n_image, size_t n_group) {
    part = a.template take<float>(n_part);
    pn = a.template take<float>(n_image);
    S = a.template take<float>(n_group);
  }
};

static bool gn_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the sizes both training entries take
static bool gn_train_sizes_ok(int N, int H, int W, int C, int G) {
  return N >= 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W <= (1 << 30) && C > 0 &&
         G > 0 && G <= kGnMaxGroups && C <= kGnTrainMaxC && C % G == 0 && (C / G) % 4 == 0;
}

}  // namespace
}  // namespace d2mi

using namespace d2mi;

extern "C" size_t d2mi_group_norm_workspace_size(int N, int H, int W, int C, int G) {
  int cp;
  const int chunks = gn_chunks(H * W, cp);
  return layout_bytes<GnSpace>((size_t)N * chunks * G, (size_t)N * G);
}

extern "C" int d2mi_group_norm_nhwc(const float* x, int N, int H, int W, int C, int G,
                                    const float* gamma, const float* beta, float eps, int relu,
                                    int up2, int accumulate, float* y, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  D2MI_REQUIRE(N >= 0 && H > 0 && W > 0 && C > 0 && G > 0 && G <= kGnMaxGroups,
               "bad GroupNorm sizes (groups <= %d)", kGnMaxGroups);
  D2MI_REQUIRE(C % G == 0 && (C / G) % 4 == 0, "GroupNorm: C / G must be a multiple of 4");
  D2MI_REQUIRE(C / 4 <= kGnThreads, "GroupNorm: C <= %d", 4 * kGnThreads);
  D2MI_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 &&
                   ((uintptr_t)gamma & 15) == 0 && ((uintptr_t)beta & 15) == 0,
               "GroupNorm operands must be 16-B aligned");
  if (N == 0) return 0;
  hipStream_t st = as_stream(stream);
  int chunk_px;
  const int HW = H * W;
  const int chunks = gn_chunks(HW, chunk_px);
  Workspace w(workspace, workspace_bytes);
  GnSpace o;
  o.lay(w, (size_t)N * chunks * G, (size_t)N * G);
  float *partial = o.partial, *mean = o.mean, *var = o.var;
  D2MI_REQUIRE(w.ok(), "GroupNorm workspace too small (%zu < %zu)", workspace_bytes, w.off);
  const float inv_count = 1.f / (float)((size_t)HW * (C / G));
  hipLaunchKernelGGL(gn_sum_kernel, dim3(chunks, N), dim3(kGnThreads), 0, st, x, HW, C, G,
                     chunk_px, nullptr, partial);
  D2MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_reduce_kernel, dim3(N), dim3(64), 0, st, partial, chunks, G, inv_count,
                     mean);
  D2MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_sum_kernel, dim3(chunks, N), dim3(kGnThreads), 0, st, x, HW, C, G,
                     chunk_px, mean, partial);
  D2MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_reduce_kernel, dim3(N), dim3(64), 0, st, partial, chunks, G, inv_count,
                     var);
  D2MI_LAUNCH_CHECK();
  const size_t total = (size_t)N * HW * (C / 4);
  const int grid = (int)std::min<size_t>((total + kGnThreads - 1) / kGnThreads, 16384);
#define GN_APPLY(U, A)                                                                          \
  hipLaunchKernelGGL((gn_apply_kernel<U, A>), dim3(grid), dim3(kGnThreads), 0, st, x, H, W, C, \
                     G, mean, var, gamma, beta, eps, relu, y, N)
  if (up2 && accumulate) GN_APPLY(true, true);
  else if (up2) GN_APPLY(true, false);
  else if (accumulate) GN_APPLY(false, true);
  else GN_APPLY(false, false);
#undef GN_APPLY
  D2MI_LAUNCH_CHECK();
  return 0;
}

// Reference: the per-level GroupNorm calls of the SOLOv2 towers
// (solo_v2.py:173-183) — d2mi_group_norm_nhwc per level, as ONE set of launches.
extern "C" size_t d2mi_group_norm_levels_workspace_size(const int32_t* dims, int nlev, int C,
                                                        int G) {
  if (nlev < 1 || nlev > kGnMaxLevels || G <= 0) return 0;
  GnLevels lv;
  size_t np = 0, ns = 0;
  if (gn_levels_plan(dims, nlev, C, G, lv, np, ns)) return 0;
  return layout_bytes<GnSpace>(np, ns);
}

extern "C" int d2mi_group_norm_nhwc_levels(const float* const* xs, const int32_t* dims, int nlev,
                                           int C, int G, const float* gamma, const float* beta,
                                           float eps, int relu, float* const* ys, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  D2MI_REQUIRE(nlev >= 1 && nlev <= kGnMaxLevels, "GroupNorm levels: 1..%d levels", kGnMaxLevels);
  D2MI_REQUIRE(C > 0 && G > 0 && G <= kGnMaxGroups, "bad GroupNorm sizes (groups <= %d)",
               kGnMaxGroups);
  D2MI_REQUIRE(C % G == 0 && (C / G) % 4 == 0, "GroupNorm: C / G must be a multiple of 4");
  D2MI_REQUIRE(C / 4 <= kGnThreads, "GroupNorm: C <= %d", 4 * kGnThreads);
  D2MI_REQUIRE(((uintptr_t)gamma & 15) == 0 && ((uintptr_t)beta & 15) == 0,
               "GroupNorm operands must be 16-B aligned");
  GnLevels lv;
  size_t np = 0, ns = 0;
  D2MI_REQUIRE(gn_levels_plan(dims, nlev, C, G, lv, np, ns) == 0, "bad GroupNorm level dims");
  for (int l = 0; l < nlev; ++l) {
    D2MI_REQUIRE(((uintptr_t)xs[l] & 15) == 0 && ((uintptr_t)ys[l] & 15) == 0,
                 "GroupNorm level %d operands must be 16-B aligned", l);
    lv.x[l] = xs[l];
    lv.y[l] = ys[l];
  }
  if (lv.wg0[nlev] == 0) return 0;
  hipStream_t st = as_stream(stream);
  Workspace w(workspace, workspace_bytes);
  GnSpace o;
  o.lay(w, np, ns);
  float *partial = o.partial, *mean = o.mean, *var = o.var;
  D2MI_REQUIRE(w.ok(), "GroupNorm workspace too small (%zu < %zu)", workspace_bytes, w.off);
  hipLaunchKernelGGL(gn_sum_levels_kernel, dim3(lv.wg0[nlev]), dim3(kGnThreads), 0, st, lv, C, G,
                     nullptr, partial);
  D2MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_reduce_levels_kernel, dim3(lv.st0[nlev]), dim3(64), 0, st, lv, partial, G,
                     mean);
  D2MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_sum_levels_kernel, dim3(lv.wg0[nlev]), dim3(kGnThreads), 0, st, lv, C, G,
                     mean, partial);
  D2MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_reduce_levels_kernel, dim3(lv.st0[nlev]), dim3(64), 0, st, lv, partial, G,
                     var);
  D2MI_LAUNCH_CHECK();
  const long long total = lv.e0[nlev];
  const int grid = (int)std::min<long long>((total + kGnThreads - 1) / kGnThreads, 16384);
  hipLaunchKernelGGL(gn_apply_levels_kernel, dim3(grid), dim3(kGnThreads), 0, st, lv, C, G, mean,
                     var, gamma, beta, eps, relu);
  D2MI_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------ training entries
#define GN_TRAIN_REQUIRE_SIZES(N, H, W, C, G)                                                  \
  D2MI_REQUIRE(gn_train_sizes_ok(N, H, W, C, G),                                               \
               "GroupNorm training: bad sizes N=%d H=%d W=%d C=%d G=%d (0 <= N <= 65535, "     \
               "C <= %d, groups <= %d, C / G a multiple of 4)",                                \
               N, H, W, C, G, kGnTrainMaxC, kGnMaxGroups)

extern "C" size_t d2mi_group_norm_train_fwd_workspace_size(int N, int H, int W, int C, int G) {
  if (!gn_train_sizes_ok(N, H, W, C, G)) return 0;
  return d2mi_group_norm_workspace_size(N, H, W, C, G);
}

extern "C" int d2mi_group_norm_train_fwd(const float* x, int N, int H, int W, int C, int G,
                                         const float* gamma, const float* beta, float eps,
                                         int relu, float* y, float* mean, float* var,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  GN_TRAIN_REQUIRE_SIZES(N, H, W, C, G);
  D2MI_REQUIRE(gn_aligned16(x) && gn_aligned16(y) && gn_aligned16(gamma) && gn_aligned16(beta),
               "GroupNorm operands must be 16-B aligned");
  if (N == 0) return 0;
  int chunk_px;
  const int HW = H * W;
  const int chunks = gn_chunks(HW, chunk_px);
  Workspace w(workspace, workspace_bytes);
  GnSpace o;
  o.lay(w, (size_t)N * chunks * G, (size_t)N * G);
  D2MI_REQUIRE(w.ok(), "GroupNorm workspace too small (%zu < %zu)", workspace_bytes, w.off);
  D2MI_REQUIRE(x && y && gamma && beta && mean && var, "GroupNorm training forward: null operand");
  hipStream_t st = as_stream(stream);
  float* partial = o.partial;  // (the workspace's own mean / var rows stay unused)
  const float inv_count = 1.f / (float)((size_t)HW * (C / G));
  const bool wide = C / 4 > kGnThreads;
  for (int pass = 0; pass < 2; ++pass) {
    const float* mu = pass ? mean : nullptr;
    if (wide)
      hipLaunchKernelGGL(gn_sum_wide_kernel, dim3(chunks, N), dim3(kGnThreads), 0, st, x, HW, C, G,
                         chunk_px, mu, partial);
    else
      hipLaunchKernelGGL(gn_sum_kernel, dim3(chunks, N), dim3(kGnThreads), 0, st, x, HW, C, G,
                         chunk_px, mu, partial);
    D2MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(gn_reduce_kernel, dim3(N), dim3(64), 0, st, partial, chunks, G, inv_count,
                       pass ? var : mean);
    D2MI_LAUNCH_CHECK();
  }
  const size_t total = (size_t)N * HW * (C / 4);
  const int grid = (int)std::min<size_t>((total + kGnThreads - 1) / kGnThreads, 16384);
  hipLaunchKernelGGL((gn_apply_kernel<false, false>), dim3(grid), dim3(kGnThreads), 0, st, x, H, W,
                     C, G, mean, var, gamma, beta, eps, relu, y, N);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t d2mi_group_norm_train_bwd_workspace_size(int N, int H, int W, int C, int G) {
  if (!gn_train_sizes_ok(N, H, W, C, G)) return 0;
  const GnBwdPlan pl = gn_bwd_plan(N, H * W, C);
  return layout_bytes<GnBwdSpace>((size_t)N * pl.chunks * 2 * C, (size_t)N * 2 * C,
                                  (size_t)N * G * 2);
}

extern "C" int d2mi_group_norm_train_bwd(const float* x, const float* dy, int N, int H, int W,
                                         int C, int G, const float* mean, const float* var,
                                         const float* gamma, const float* beta, float eps,
                                         int relu, float* dx, float* dgamma, float* dbeta,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  GN_TRAIN_REQUIRE_SIZES(N, H, W, C, G);
  D2MI_REQUIRE(gn_aligned16(x) && gn_aligned16(dy) && gn_aligned16(dx) && gn_aligned16(gamma) &&
                   gn_aligned16(beta),
               "GroupNorm operands must be 16-B aligned");
  if (N == 0) return 0;
  const int HW = H * W;
  const GnBwdPlan pl = gn_bwd_plan(N, HW, C);
  Workspace w(workspace, workspace_bytes);
  GnBwdSpace o;
  o.lay(w, (size_t)N * pl.chunks * 2 * C, (size_t)N * 2 * C, (size_t)N * G * 2);
  D2MI_REQUIRE(w.ok(), "GroupNorm workspace too small (%zu < %zu)", workspace_bytes, w.off);
  D2MI_REQUIRE(x && dy && mean && var && gamma && beta,
               "GroupNorm training backward: null operand");
  const bool affine = dgamma || dbeta;
  if (!dx && !affine) return 0;
  hipStream_t st = as_stream(stream);
  const int wgs = N * pl.chunks;
  hipLaunchKernelGGL(gn_bwd_reduce_kernel, dim3(wgs), dim3(kGnThreads), 0, st, x, dy, HW, C, G,
                     pl.chunks, pl.chunk_px, mean, var, gamma, beta, eps, relu, o.part);
  D2MI_LAUNCH_CHECK();
  const float* pn = o.part;  // (one chunk per image: the partials are the images' sums)
  if (pl.chunks > 1) {
    hipLaunchKernelGGL(gn_bwd_chunks_kernel, dim3((2 * C + kGnSumCols - 1) / kGnSumCols, N),
                       dim3(kGnSumCols * kGnSumSlices), 0, st, o.part, pl.chunks, 2 * C, o.pn);
    D2MI_LAUNCH_CHECK();
    pn = o.pn;
  }
  const int images = dx ? N : 0;
  const int columns = affine ? (2 * C + kGnAffCols - 1) / kGnAffCols : 0;
  hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(images + columns), dim3(kGnThreads), 0, st, pn, N,
                     C, G, images, gamma, o.S, dgamma, dbeta);
  D2MI_LAUNCH_CHECK();
  if (dx) {
    const float inv_m = 1.f / (float)((size_t)HW * (C / G));
    hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(wgs), dim3(kGnThreads), 0, st, x, dy, HW, C, G,
                       pl.chunks, pl.chunk_px, mean, var, gamma, beta, eps, relu, o.S, inv_m, dx);
    D2MI_LAUNCH_CHECK();
  }
  return 0;
}
