// Panoptic FPN's semantic branch and panoptic merge without a full-resolution
// tensor in HBM:
//
//  * d2mi_sem_seg_loss_fwd / _bwd: SemSegFPNHead.call's resize_images(x,
//    x scale) + sparse softmax cross-entropy over the not-ignored pixels
//    (lib/modeling/meta_arch/semantic_seg.py:197-218).  The quarter-resolution
//    logits are interpolated on the fly (resize.h: d2mi_resize_bilinear's
//    half-pixel arithmetic); the backward is a gather per low-resolution
//    pixel that recomputes the softmax.
//  * d2mi_sem_seg_argmax: sem_seg_postprocess("conventional") + tf.argmax
//    (lib/modeling/postprocessing.py:62-95, panoptic_fpn.py:118-131).
//  * d2mi_panoptic_combine: combine_semantic_and_instance_outputs
//    (panoptic_fpn.py:160-296).
//
// Tiling of the three segmentation kernels: one workgroup (256 threads) per
// kTile x kTile tile of low-resolution pixels.  The tile plus a one-pixel
// halo ((kTile + 2)^2 pixels x C floats, rows padded to an odd stride so
// that lanes on different pixels hit different LDS banks) is staged once;
// every corner read of the interpolation then comes from LDS.  For C = 54
// that is 10 * 10 * 55 * 4 B = 21.5 KiB of the CU's 160 KiB.
//
// Determinism: every float sum has a fixed order (per-thread sequential,
// fixed shuffle / LDS tree, per-workgroup partials, one ordered final pass;
// accumulators are f64); the only atomics are integer counters.
#include <limits.h>

#include <algorithm>

#include "common.h"
#include "resize.h"
#include "wave.h"

namespace d2mi {
namespace {

constexpr int kTile = 8;
constexpr int kHalo = kTile + 2;
constexpr int kThreads = 256;  // (block_sum's four waves)
constexpr int kMaxScale = 8;
constexpr size_t kMaxLds = 64 * 1024;

struct SegShape {
  int N, h, w, C, ldc, scale, H, W;
  float sh, sw;
};

__host__ __device__ inline int odd_stride(int C) { return C | 1; }

// Low-resolution rows [ly0, ly0 + kHalo) x columns [lx0, lx0 + kHalo) of image
// n, clamped into the map, as tile[(a * kHalo + b) * Cs + c].
__device__ __forceinline__ void stage_tile(const float* __restrict__ logits, const SegShape& s,
                                           int n, int ly0, int lx0, float* tile) {
  const int Cs = odd_stride(s.C);
  const float* img = logits + (size_t)n * s.h * s.w * s.ldc;
  for (int e = threadIdx.x; e < kHalo * kHalo * s.C; e += kThreads) {
    const int c = e % s.C, p = e / s.C;
    const int b = p % kHalo, a = p / kHalo;
    const int y = min(max(ly0 + a, 0), s.h - 1), x = min(max(lx0 + b, 0), s.w - 1);
    tile[p * Cs + c] = img[((size_t)y * s.w + x) * s.ldc + c];
  }
}

// The four corner rows of an output pixel inside the staged tile.
struct Corners {
  const float *tl, *tr, *bl, *br;
  float xl, yl;
};

__device__ __forceinline__ int local_index(int v, int v0) {
  return min(max(v - v0, 0), kHalo - 1);
}

__device__ __forceinline__ Corners corners_of(const float* tile, int Cs, const Interp& iy,
                                              const Interp& ix, int ly0, int lx0) {
  const int a0 = local_index(iy.lo, ly0), a1 = local_index(iy.hi, ly0);
  const int b0 = local_index(ix.lo, lx0), b1 = local_index(ix.hi, lx0);
  Corners k;
  k.tl = tile + (a0 * kHalo + b0) * Cs;
  k.tr = tile + (a0 * kHalo + b1) * Cs;
  k.bl = tile + (a1 * kHalo + b0) * Cs;
  k.br = tile + (a1 * kHalo + b1) * Cs;
  k.xl = ix.lerp;
  k.yl = iy.lerp;
  return k;
}

__device__ __forceinline__ float logit_at(const Corners& k, int c) {
  return tf_lerp(k.tl[c], k.tr[c], k.bl[c], k.br[c], k.xl, k.yl);
}

// log(sum_c exp(v_c)) of the interpolated logits (max-shifted, f32).
__device__ __forceinline__ float logsumexp_at(const Corners& k, int C) {
  float m = logit_at(k, 0);
  for (int c = 1; c < C; ++c) m = fmaxf(m, logit_at(k, c));
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf(logit_at(k, c) - m);
  return m + logf(sum);
}

// The label of output pixel (oy, ox) of image n, or -1 when the pixel does not
// count: outside the image's true shape or the label extent (the
// pad_value = ignore_value padding of ImageList.from_tensors), the ignore
// value itself, or a label that is no class.
__device__ __forceinline__ int label_at(const int32_t* __restrict__ labels, int Hl, int Wl,
                                        const int32_t* __restrict__ shapes, int ignore_value,
                                        int C, int n, int oy, int ox) {
  if (oy >= Hl || ox >= Wl || oy >= shapes[2 * n] || ox >= shapes[2 * n + 1]) return -1;
  const int l = labels[((size_t)n * Hl + oy) * Wl + ox];
  return (l == ignore_value || l < 0 || l >= C) ? -1 : l;
}

__global__ __launch_bounds__(kThreads) void seg_loss_fwd_kernel(
    const float* __restrict__ logits, SegShape s, const int32_t* __restrict__ labels, int Hl,
    int Wl, const int32_t* __restrict__ shapes, int ignore_value, double* __restrict__ psum,
    int32_t* __restrict__ pcnt) {
  extern __shared__ float tile[];
  __shared__ double red_d[kThreads / 64];
  __shared__ int red_i[kThreads / 64];
  const int n = blockIdx.z;
  const int ly0 = blockIdx.y * kTile - 1, lx0 = blockIdx.x * kTile - 1;
  stage_tile(logits, s, n, ly0, lx0, tile);
  __syncthreads();
  const int Cs = odd_stride(s.C);
  const int edge = kTile * s.scale;
  const int oy0 = blockIdx.y * edge, ox0 = blockIdx.x * edge;
  double sum = 0.0;
  int cnt = 0;
  for (int q = threadIdx.x; q < edge * edge; q += kThreads) {
    const int oy = oy0 + q / edge, ox = ox0 + q % edge;
    if (oy >= s.H || ox >= s.W) continue;
    const int l = label_at(labels, Hl, Wl, shapes, ignore_value, s.C, n, oy, ox);
    if (l < 0) continue;
    const Corners k = corners_of(tile, Cs, interp_at(oy, s.sh, s.h, 1), interp_at(ox, s.sw, s.w, 1),
                                 ly0, lx0);
    sum += (double)(logsumexp_at(k, s.C) - logit_at(k, l));
    ++cnt;
  }
  const double bs = block_sum(sum, red_d);
  const int bc = block_sum(cnt, red_i);
  if (threadIdx.x == 0) {
    const int b = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    psum[b] = bs;
    pcnt[b] = bc;
  }
}

__global__ __launch_bounds__(kThreads) void seg_loss_final_kernel(
    const double* __restrict__ psum, const int32_t* __restrict__ pcnt, int blocks,
    float loss_weight, float* __restrict__ loss, int32_t* __restrict__ count) {
  __shared__ double red_d[kThreads / 64];
  __shared__ int red_i[kThreads / 64];
  double sum = 0.0;
  int cnt = 0;
  for (int i = threadIdx.x; i < blocks; i += kThreads) {
    sum += psum[i];
    cnt += pcnt[i];
  }
  const double ts = block_sum(sum, red_d);
  const int tc = block_sum(cnt, red_i);
  if (threadIdx.x == 0) {
    *loss = tc > 0 ? loss_weight * (float)(ts / (double)tc) : 0.f;
    *count = tc;
  }
}

// Backward.  Region: the output rows / columns [s*i0 - s, s*(i0 + kTile) + s)
// around the tile -- every output pixel whose footprint touches a tile pixel
// lies inside (its source coordinate is within one of that pixel).
__global__ __launch_bounds__(kThreads) void seg_loss_bwd_kernel(
    const float* __restrict__ logits, SegShape s, const int32_t* __restrict__ labels, int Hl,
    int Wl, const int32_t* __restrict__ shapes, int ignore_value, float loss_weight,
    const int32_t* __restrict__ count, const float* __restrict__ grad_loss,
    float* __restrict__ grad_logits) {
  extern __shared__ float smem[];
  const int Cs = odd_stride(s.C);
  const int R = (kTile + 2) * s.scale;
  float* tile = smem;
  float* lse = tile + kHalo * kHalo * Cs;       // [R * R]
  int* lab = (int*)(lse + R * R);               // [R * R], -1: contributes nothing
  int* ylo = lab + R * R;                       // [R] each: source rows / columns and lerps
  int* yhi = ylo + R;
  int* xlo = yhi + R;
  int* xhi = xlo + R;
  float* yl = (float*)(xhi + R);
  float* xl = yl + R;
  const int n = blockIdx.z;
  const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
  const int ly0 = i0 - 1, lx0 = j0 - 1;
  const int ry0 = s.scale * i0 - s.scale, rx0 = s.scale * j0 - s.scale;
  stage_tile(logits, s, n, ly0, lx0, tile);
  for (int r = threadIdx.x; r < R; r += kThreads) {
    const int oy = ry0 + r, ox = rx0 + r;
    ylo[r] = yhi[r] = xlo[r] = xhi[r] = INT_MIN;  // matches no pixel
    yl[r] = xl[r] = 0.f;
    if (oy >= 0 && oy < s.H) {
      const Interp t = interp_at(oy, s.sh, s.h, 1);
      ylo[r] = t.lo; yhi[r] = t.hi; yl[r] = t.lerp;
    }
    if (ox >= 0 && ox < s.W) {
      const Interp t = interp_at(ox, s.sw, s.w, 1);
      xlo[r] = t.lo; xhi[r] = t.hi; xl[r] = t.lerp;
    }
  }
  __syncthreads();
  // pass A: each region pixel's label and logsumexp, once per workgroup
  for (int q = threadIdx.x; q < R * R; q += kThreads) {
    const int ry = q / R, rx = q % R;
    int l = -1;
    float v = 0.f;
    const bool touch_y = (ylo[ry] >= i0 && ylo[ry] < i0 + kTile) ||
                         (yhi[ry] >= i0 && yhi[ry] < i0 + kTile);
    const bool touch_x = (xlo[rx] >= j0 && xlo[rx] < j0 + kTile) ||
                         (xhi[rx] >= j0 && xhi[rx] < j0 + kTile);
    if (touch_y && touch_x) {
      l = label_at(labels, Hl, Wl, shapes, ignore_value, s.C, n, ry0 + ry, rx0 + rx);
      if (l >= 0) {
        Interp iy, ix;
        iy.lo = ylo[ry]; iy.hi = yhi[ry]; iy.lerp = yl[ry];
        ix.lo = xlo[rx]; ix.hi = xhi[rx]; ix.lerp = xl[rx];
        v = logsumexp_at(corners_of(tile, Cs, iy, ix, ly0, lx0), s.C);
      }
    }
    lab[q] = l;
    lse[q] = v;
  }
  __syncthreads();
  const int cnt = *count;
  const float factor = cnt > 0 ? *grad_loss * loss_weight / (float)cnt : 0.f;
  // pass B: an item is one tile pixel and the channels l16 + 16 j (j < 4) of
  // a block of 64: the 16 lanes of a pixel read consecutive LDS words, and the
  // bookkeeping of an output pixel is shared by the item's channels.  Each
  // channel sums its output pixels in row-major order.
  constexpr int kLanes = 16, kPer = 4;
  for (int it = threadIdx.x; it < kTile * kTile * kLanes; it += kThreads) {
    const int l16 = it % kLanes, p = it / kLanes;
    const int li = i0 + p / kTile, lj = j0 + p % kTile;
    if (li >= s.h || lj >= s.w) continue;
    const int ra = s.scale * (li - i0), rb = s.scale * (lj - j0);  // + 3 * scale <= R
    float* out = grad_logits + (((size_t)n * s.h + li) * s.w + lj) * s.ldc;
    for (int cb = l16; cb < s.ldc; cb += kLanes * kPer) {
      double acc[kPer] = {0.0, 0.0, 0.0, 0.0};
      if (cb < s.C) {
        for (int ry = ra; ry < ra + 3 * s.scale; ++ry) {
          if (ylo[ry] != li && yhi[ry] != li) continue;
          const float wy = (ylo[ry] == li ? 1.f - yl[ry] : 0.f) + (yhi[ry] == li ? yl[ry] : 0.f);
          for (int rx = rb; rx < rb + 3 * s.scale; ++rx) {
            if (xlo[rx] != lj && xhi[rx] != lj) continue;
            const int q = ry * R + rx;
            const int l = lab[q];
            if (l < 0) continue;
            const float wx =
                (xlo[rx] == lj ? 1.f - xl[rx] : 0.f) + (xhi[rx] == lj ? xl[rx] : 0.f);
            Interp iy, ix;
            iy.lo = ylo[ry]; iy.hi = yhi[ry]; iy.lerp = yl[ry];
            ix.lo = xlo[rx]; ix.hi = xhi[rx]; ix.lerp = xl[rx];
            const Corners k = corners_of(tile, Cs, iy, ix, ly0, lx0);
            const double wgt = (double)(wy * wx);
            const float z = lse[q];
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
              const int c = cb + kLanes * j;
              if (c < s.C) {
                const float g = expf(logit_at(k, c) - z) - (c == l ? 1.f : 0.f);
                acc[j] += wgt * (double)g;
              }
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int c = cb + kLanes * j;
        if (c < s.ldc) out[c] = (float)(acc[j] * (double)factor);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void seg_argmax_kernel(
    const float* __restrict__ logits, SegShape s, const int32_t* __restrict__ shapes,
    int64_t* __restrict__ out) {
  extern __shared__ float tile[];
  const int n = blockIdx.z;
  const int ly0 = blockIdx.y * kTile - 1, lx0 = blockIdx.x * kTile - 1;
  stage_tile(logits, s, n, ly0, lx0, tile);
  __syncthreads();
  const int Cs = odd_stride(s.C);
  const int edge = kTile * s.scale;
  const int oy0 = blockIdx.y * edge, ox0 = blockIdx.x * edge;
  const int th = shapes[2 * n], tw = shapes[2 * n + 1];
  for (int q = threadIdx.x; q < edge * edge; q += kThreads) {
    const int oy = oy0 + q / edge, ox = ox0 + q % edge;
    if (oy >= s.H || ox >= s.W) continue;
    int best = 0;
    if (oy < th && ox < tw) {
      const Corners k = corners_of(tile, Cs, interp_at(oy, s.sh, s.h, 1),
                                   interp_at(ox, s.sw, s.w, 1), ly0, lx0);
      float bv = logit_at(k, 0);
      for (int c = 1; c < s.C; ++c) {
        const float v = logit_at(k, c);
        if (v > bv) {  // strict: the lowest index wins a tie
          bv = v;
          best = c;
        }
      }
    }
    out[((size_t)n * s.H + oy) * s.W + ox] = best;
  }
}

// Checks the shape and fills s; the launch grid is (ceil(w / kTile),
// ceil(h / kTile), N).
int seg_shape(int N, int h, int w, int C, int ldc, int scale, SegShape* s) {
  D2MI_REQUIRE(N > 0 && h > 0 && w > 0 && C > 0 && ldc >= C, "bad sem_seg logits shape");
  D2MI_REQUIRE(scale >= 1 && scale <= kMaxScale, "sem_seg scale must be in [1, %d]", kMaxScale);
  D2MI_REQUIRE(N <= 65535 && (h + kTile - 1) / kTile <= 65535 &&
                   (int64_t)h * scale < (1 << 24) && (int64_t)w * scale < (1 << 24),
               "sem_seg map too large");
  s->N = N; s->h = h; s->w = w; s->C = C; s->ldc = ldc; s->scale = scale;
  s->H = h * scale; s->W = w * scale;
  s->sh = resize_scale(h, s->H, 0);
  s->sw = resize_scale(w, s->W, 0);
  return 0;
}

size_t tile_bytes(int C) { return (size_t)kHalo * kHalo * odd_stride(C) * sizeof(float); }
size_t bwd_lds_bytes(int C, int scale) {
  const size_t R = (size_t)(kTile + 2) * scale;
  return tile_bytes(C) + R * R * 8 + R * 6 * 4;
}
int seg_blocks(int N, int h, int w) {
  return N * ((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile);
}
dim3 seg_grid(const SegShape& s) {
  return dim3((s.w + kTile - 1) / kTile, (s.h + kTile - 1) / kTile, s.N);
}

struct SegLossSpace {
  double* psum;   // [blocks] per-workgroup loss sums
  int32_t* pcnt;  // [blocks] per-workgroup counted pixels
  template <typename A>
  void lay(A& a, int blocks) {
    psum = a.template take<double>(blocks);
    pcnt = a.template take<int32_t>(blocks);
  }
};

// ------------------------------------------------------------ panoptic combine
struct PanSpace {
  int32_t* order;  // [N, D] instance index of each score rank
  int32_t* area;   // [N, D] mask pixels of each rank
  int32_t* inter;  // [N, D] of those, already claimed when the rank is visited
  int32_t* sarea;  // [N, S] still-empty pixels of each stuff label
  int32_t* sbox;   // [N, S, 4] their ymin, xmin, ymax, xmax (inclusive)
  template <typename A>
  void lay(A& a, int N, int D, int S) {
    order = a.template take<int32_t>((size_t)N * D);
    area = a.template take<int32_t>((size_t)N * D);
    inter = a.template take<int32_t>((size_t)N * D);
    sarea = a.template take<int32_t>((size_t)N * S);
    sbox = a.template take<int32_t>((size_t)N * S * 4);
  }
};

constexpr int kMaxStuff = 1024;

struct PanArgs {
  const uint8_t* masks;     // [N, D, H, W]
  const float* scores;      // [N, D]
  const int64_t* classes;   // [N, D]
  const float* boxes;       // [N, D, 4]
  const uint8_t* is_valid;  // [N, D]
  const int64_t* sem_seg;   // [N, H, W]
  int N, D, H, W, S;
  float overlap_thresh, stuff_area_limit, conf_thresh;
  int32_t* pan;  // [N, H, W]
  PanSpace ws;
};

// tf.argsort(-scores): descending score, ties to the lower index; zero the counters.
__global__ __launch_bounds__(kThreads) void pan_init_kernel(PanArgs a) {
  const int n = blockIdx.x;
  for (int i = threadIdx.x; i < a.D; i += kThreads) {
    const uint64_t ki = ((uint64_t)(~orderable(a.scores[n * a.D + i])) << 32) | (uint32_t)i;
    int rank = 0;
    for (int j = 0; j < a.D; ++j) {
      const uint64_t kj = ((uint64_t)(~orderable(a.scores[n * a.D + j])) << 32) | (uint32_t)j;
      rank += kj < ki;
    }
    a.ws.order[n * a.D + rank] = i;  // (the keys are distinct: rank is a permutation)
    a.ws.area[n * a.D + i] = 0;
    a.ws.inter[n * a.D + i] = 0;
  }
  for (int l = threadIdx.x; l < a.S; l += kThreads) {
    a.ws.sarea[n * a.S + l] = 0;
    int32_t* b = a.ws.sbox + ((size_t)n * a.S + l) * 4;
    b[0] = b[1] = INT_MAX;
    b[2] = b[3] = -1;
  }
}

// panoptic_fpn.py:207-208 for score rank r of image n, from the finished counters.
__device__ __forceinline__ bool instance_applies(const PanArgs& a, int n, int r) {
  const int i = a.ws.order[n * a.D + r];
  const int area = a.ws.area[n * a.D + r], inter = a.ws.inter[n * a.D + r];
  return a.is_valid[n * a.D + i] != 0 && a.scores[n * a.D + i] > a.conf_thresh && area > 0 &&
         (float)inter / (float)area < a.overlap_thresh;
}

// Launch k of D + 1: apply rank k - 1 (its counters are final) and count rank k
// on the updated map; launch D counts the stuff labels instead.
__global__ __launch_bounds__(kThreads) void pan_step_kernel(PanArgs a, int k) {
  __shared__ int red_i[kThreads / 64];
  __shared__ int s_area[kMaxStuff];
  __shared__ int s_box[kMaxStuff][4];
  const int n = blockIdx.y;
  const size_t HW = (size_t)a.H * a.W;
  const bool apply = k >= 1 && instance_applies(a, n, k - 1);
  const uint8_t* m_apply =
      apply ? a.masks + ((size_t)n * a.D + a.ws.order[n * a.D + k - 1]) * HW : nullptr;
  const uint8_t* m_count =
      k < a.D ? a.masks + ((size_t)n * a.D + a.ws.order[n * a.D + k]) * HW : nullptr;
  const bool stuff = k == a.D;
  if (stuff) {
    for (int l = threadIdx.x; l < a.S; l += kThreads) {
      s_area[l] = 0;
      s_box[l][0] = s_box[l][1] = INT_MAX;
      s_box[l][2] = s_box[l][3] = -1;
    }
    __syncthreads();
  }
  int32_t* pan = a.pan + n * HW;
  const int64_t* sem = a.sem_seg + n * HW;
  int area = 0, inter = 0;
  for (size_t p = blockIdx.x * (size_t)kThreads + threadIdx.x; p < HW;
       p += (size_t)gridDim.x * kThreads) {
    int v = k == 0 ? 0 : pan[p];
    bool changed = k == 0;
    if (m_apply && v == 0 && m_apply[p] > 0) {
      v = k;
      changed = true;
    }
    if (changed) pan[p] = v;
    if (m_count && m_count[p] > 0) {
      ++area;
      inter += v > 0;
    }
    if (stuff && v == 0) {
      const int64_t l = sem[p];
      if (l >= 1 && l < a.S) {
        const int y = (int)(p / a.W), x = (int)(p % a.W);
        atomicAdd(&s_area[l], 1);
        atomicMin(&s_box[l][0], y);
        atomicMin(&s_box[l][1], x);
        atomicMax(&s_box[l][2], y);
        atomicMax(&s_box[l][3], x);
      }
    }
  }
  if (m_count) {
    const int ba = block_sum(area, red_i);
    __syncthreads();  // (red_i reused)
    const int bi = block_sum(inter, red_i);
    if (threadIdx.x == 0 && ba > 0) {
      atomicAdd(&a.ws.area[n * a.D + k], ba);
      if (bi > 0) atomicAdd(&a.ws.inter[n * a.D + k], bi);
    }
  }
  if (stuff) {
    __syncthreads();
    for (int l = threadIdx.x; l < a.S; l += kThreads) {
      if (s_area[l] == 0) continue;
      atomicAdd(&a.ws.sarea[n * a.S + l], s_area[l]);
      int32_t* b = a.ws.sbox + ((size_t)n * a.S + l) * 4;
      atomicMin(&b[0], s_box[l][0]);
      atomicMin(&b[1], s_box[l][1]);
      atomicMax(&b[2], s_box[l][2]);
      atomicMax(&b[3], s_box[l][3]);
    }
  }
}

struct PanTable {
  int32_t* id;
  uint8_t* isthing;
  float* score;
  int64_t* category_id;
  int32_t* instance_id;
  float* bbox;
  uint8_t* is_valid;
  float* area;
};

// The stuff labels claim their still-empty pixels (panoptic_fpn.py:237-260);
// workgroup 0 of each image writes the segment table.
__global__ __launch_bounds__(kThreads) void pan_finish_kernel(PanArgs a, PanTable t) {
  const int n = blockIdx.y;
  const size_t HW = (size_t)a.H * a.W;
  int32_t* pan = a.pan + n * HW;
  const int64_t* sem = a.sem_seg + n * HW;
  const int32_t* sarea = a.ws.sarea + n * a.S;
  for (size_t p = blockIdx.x * (size_t)kThreads + threadIdx.x; p < HW;
       p += (size_t)gridDim.x * kThreads) {
    if (pan[p] != 0) continue;
    const int64_t l = sem[p];
    if (l >= 1 && l < a.S && (float)sarea[l] > a.stuff_area_limit) pan[p] = a.D + (int)l;
  }
  if (blockIdx.x != 0) return;
  const int rows = a.D + a.S - 1;
  for (int r = threadIdx.x; r < rows; r += kThreads) {
    const size_t o = (size_t)n * rows + r;
    if (r < a.D) {
      const int i = a.ws.order[n * a.D + r];
      t.id[o] = r + 1;
      t.isthing[o] = 1;
      t.score[o] = a.scores[n * a.D + i];
      t.category_id[o] = a.classes[n * a.D + i];
      t.instance_id[o] = i;
      for (int e = 0; e < 4; ++e) t.bbox[o * 4 + e] = a.boxes[((size_t)n * a.D + i) * 4 + e];
      t.is_valid[o] = instance_applies(a, n, r);
      t.area[o] = (float)a.ws.area[n * a.D + r];
    } else {
      const int l = r - a.D + 1;
      const bool ok = (float)sarea[l] > a.stuff_area_limit;
      const int32_t* b = a.ws.sbox + ((size_t)n * a.S + l) * 4;
      t.id[o] = a.D + l;
      t.isthing[o] = 0;
      t.score[o] = 0.5f;
      t.category_id[o] = l;
      t.instance_id[o] = 0;
      for (int e = 0; e < 4; ++e) t.bbox[o * 4 + e] = ok ? (float)b[e] : 0.f;
      t.is_valid[o] = ok;
      t.area[o] = (float)sarea[l];
    }
  }
}

}  // namespace
}  // namespace d2mi

using namespace d2mi;

extern "C" size_t d2mi_sem_seg_loss_workspace_size(int N, int h, int w) {
  if (N <= 0 || h <= 0 || w <= 0) return 0;
  return layout_bytes<SegLossSpace>(seg_blocks(N, h, w));
}

extern "C" int d2mi_sem_seg_loss_fwd(const float* logits, int N, int h, int w, int C, int ldc,
                                     const int32_t* labels, int Hl, int Wl,
                                     const int32_t* image_shapes, int ignore_value, int scale,
                                     float loss_weight, float* loss, int32_t* count,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  SegShape s;
  if (seg_shape(N, h, w, C, ldc, scale, &s)) return -1;
  D2MI_REQUIRE(Hl > 0 && Wl > 0, "bad sem_seg label shape");
  D2MI_REQUIRE(tile_bytes(C) <= kMaxLds, "sem_seg: %d classes exceed the LDS tile", C);
  const int blocks = seg_blocks(N, h, w);
  Workspace wsp(workspace, workspace_bytes);
  SegLossSpace sp;
  sp.lay(wsp, blocks);
  D2MI_REQUIRE(wsp.ok(), "sem_seg_loss workspace too small (%zu < %zu)", workspace_bytes, wsp.off);
  D2MI_REQUIRE(logits && labels && image_shapes && loss && count && workspace,
               "sem_seg_loss_fwd: null pointer");
  hipLaunchKernelGGL(seg_loss_fwd_kernel, seg_grid(s), dim3(kThreads), tile_bytes(C),
                     as_stream(stream), logits, s, labels, Hl, Wl, image_shapes, ignore_value,
                     sp.psum, sp.pcnt);
  D2MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_loss_final_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream),
                     sp.psum, sp.pcnt, blocks, loss_weight, loss, count);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" int d2mi_sem_seg_loss_bwd(const float* logits, int N, int h, int w, int C, int ldc,
                                     const int32_t* labels, int Hl, int Wl,
                                     const int32_t* image_shapes, int ignore_value, int scale,
                                     float loss_weight, const int32_t* count,
                                     const float* grad_loss, float* grad_logits, void* stream) {
  SegShape s;
  if (seg_shape(N, h, w, C, ldc, scale, &s)) return -1;
  D2MI_REQUIRE(Hl > 0 && Wl > 0, "bad sem_seg label shape");
  D2MI_REQUIRE(bwd_lds_bytes(C, scale) <= kMaxLds,
               "sem_seg_loss_bwd: %d classes at scale %d exceed the LDS budget", C, scale);
  D2MI_REQUIRE(logits && labels && image_shapes && count && grad_loss && grad_logits,
               "sem_seg_loss_bwd: null pointer");
  hipLaunchKernelGGL(seg_loss_bwd_kernel, seg_grid(s), dim3(kThreads), bwd_lds_bytes(C, scale),
                     as_stream(stream), logits, s, labels, Hl, Wl, image_shapes, ignore_value,
                     loss_weight, count, grad_loss, grad_logits);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" int d2mi_sem_seg_argmax(const float* logits, int N, int h, int w, int C, int ldc,
                                   const int32_t* image_shapes, int scale, int64_t* out,
                                   void* stream) {
  SegShape s;
  if (seg_shape(N, h, w, C, ldc, scale, &s)) return -1;
  D2MI_REQUIRE(tile_bytes(C) <= kMaxLds, "sem_seg: %d classes exceed the LDS tile", C);
  D2MI_REQUIRE(logits && image_shapes && out, "sem_seg_argmax: null pointer");
  hipLaunchKernelGGL(seg_argmax_kernel, seg_grid(s), dim3(kThreads), tile_bytes(C),
                     as_stream(stream), logits, s, image_shapes, out);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t d2mi_panoptic_combine_workspace_size(int N, int D, int num_stuff_classes) {
  if (N <= 0 || D < 0 || num_stuff_classes < 1) return 0;
  return layout_bytes<PanSpace>(N, D, num_stuff_classes);
}

extern "C" int d2mi_panoptic_combine(const uint8_t* masks, const float* scores,
                                     const int64_t* classes, const float* boxes,
                                     const uint8_t* is_valid, const int64_t* sem_seg, int N, int D,
                                     int H, int W, float overlap_thresh, float stuff_area_limit,
                                     float conf_thresh, int num_stuff_classes,
                                     int32_t* panoptic_seg, int32_t* seg_id, uint8_t* seg_isthing,
                                     float* seg_score, int64_t* seg_category_id,
                                     int32_t* seg_instance_id, float* seg_bbox,
                                     uint8_t* seg_is_valid, float* seg_area, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  D2MI_REQUIRE(N > 0 && N <= 65535 && D >= 0 && H > 0 && W > 0, "bad panoptic_combine shape");
  D2MI_REQUIRE(num_stuff_classes >= 1 && num_stuff_classes <= kMaxStuff,
               "panoptic_combine: num_stuff_classes must be in [1, %d]", kMaxStuff);
  PanArgs a;
  Workspace wsp(workspace, workspace_bytes);
  a.ws.lay(wsp, N, D, num_stuff_classes);
  D2MI_REQUIRE(wsp.ok(), "panoptic_combine workspace too small (%zu < %zu)", workspace_bytes,
               wsp.off);
  D2MI_REQUIRE(sem_seg && panoptic_seg && workspace &&
                   (D == 0 || (masks && scores && classes && boxes && is_valid)),
               "panoptic_combine: null pointer");
  const int rows = D + num_stuff_classes - 1;
  D2MI_REQUIRE(rows == 0 || (seg_id && seg_isthing && seg_score && seg_category_id &&
                             seg_instance_id && seg_bbox && seg_is_valid && seg_area),
               "panoptic_combine: null segment table");
  a.masks = masks; a.scores = scores; a.classes = classes; a.boxes = boxes;
  a.is_valid = is_valid; a.sem_seg = sem_seg;
  a.N = N; a.D = D; a.H = H; a.W = W; a.S = num_stuff_classes;
  a.overlap_thresh = overlap_thresh; a.stuff_area_limit = stuff_area_limit;
  a.conf_thresh = conf_thresh;
  a.pan = panoptic_seg;
  const PanTable t = {seg_id, seg_isthing, seg_score, seg_category_id, seg_instance_id,
                      seg_bbox, seg_is_valid, seg_area};
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(pan_init_kernel, dim3(N), dim3(kThreads), 0, st, a);
  D2MI_LAUNCH_CHECK();
  const size_t HW = (size_t)H * W;
  const dim3 grid((unsigned)std::min<size_t>((HW + kThreads - 1) / kThreads, 1024), N);
  for (int k = 0; k <= D; ++k) {
    hipLaunchKernelGGL(pan_step_kernel, grid, dim3(kThreads), 0, st, a, k);
    D2MI_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pan_finish_kernel, grid, dim3(kThreads), 0, st, a, t);
  D2MI_LAUNCH_CHECK();
  return 0;
}
