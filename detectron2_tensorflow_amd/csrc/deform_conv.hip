// Deformable-convolution sampling (lib/layers/convolutional.py:51-115, :375-452):
// the data-dependent bilinear gather in front of DeformConv2D's GEMM.
//
//   cols[n, oh, ow, t, c] = ((w0 p0 + w1 p1) + w2 p2) + w3 p3      t = kh * k + kw
//
// where the sample position of tap t of output (oh, ow), channel group g is
//   y = clip(f32(oh * stride + kh * rate) + dy, 0, Hp - 1)   (x alike)
// in PADDED coordinates (Hp = H + pb + pe: fix_padding's zero ring, which the
// kernels never materialise: a corner in the ring reads 0 and its gradient is
// dropped), dy / dx = offsets[n, oh, ow, (g * k*k + t) * 2 + {0, 1}], the
// corners are y0 = floor(y), y1 = y0 + 1 BOTH clipped to [0, Hp - 1], and the
// weights use the clipped corners ((y1 - y)(x1 - x), ...: all four are 0 at
// y == Hp - 1, as in the reference).  The reference spells this as four
// gather_nd + a transpose + a k x k / stride-k conv over a 9x copy; here the
// column matrix [N*OH*OW, k*k*C] is written once, in the layout the 1x1 MFMA
// conv (weights reshaped [k*k*C, Cout]) reads.
//
// Forward: one wave per (output pixel, group); the tap loop's positions and
// row addresses are wave-uniform (readfirstlane'd wave index: scalar
// arithmetic), each corner is one contiguous Cg-float run read as float4 per
// lane, the column row is written contiguously.
//
// Backward (what TF autodiff gives for that graph: floor passes nothing, the
// clipped corner floats are constants, clip_by_value passes where the
// unclipped value lies in [0, Hp - 1]):
//   goffsets: a gather -- per (sample, group) 16 lanes walk the Cg channels
//     in a fixed order and reduce by a fixed butterfly.
//   gx: deterministic scatter-add without float atomics, every element
//     written (the form of d2mi_roi_align_bwd): (1) emit one 64-bit key
//     (destination pixel * G + g) << 32 | source (n, oh, ow, t, corner packed
//     in bit fields, ascending in that order) per corner, ~0 for a
//     corner in the pad ring; (2) order the keys by destination with a STABLE
//     least-significant-digit radix sort (the emit order is the source
//     order, so each destination's list comes out in ascending source order;
//     per-tile digit histograms, their scan, a scatter whose in-tile ranks come
//     from wave ballots: integer arithmetic only), and find every
//     destination's first key by binary search; (3) one wave per
//     (destination, 256-channel block) sums gcols[source, t, g*Cg ..] * w in ascending source order
//     (n, oh, ow, t, corner), the weight recomputed from the offsets.  Lists
//     are cut into chunks of kChunk entries whose partial sums are added in
//     chunk order; inside a chunk the wave's S = 64 / (Cg/4) lane slots take
//     entries s, s + S, ... of each 64-key block and are added in slot
//     order.  A destination without entries is written 0.
#include "common.h"

namespace d2mi {
namespace {

struct DeformArgs {
  int N, H, W, C, G, Cg, k, KK, stride, rate, pb, Hp, Wp, OH, OW, off_stride;
  int bh, bw;  // bits of oh / ow in a key's source word
};

// Source word of a key: n | oh | ow | t (4 bits) | corner (2 bits), most
// significant first -- ascending in (n, oh, ow, t, corner), and decoded by
// shifts in the sum pass (a flat ordinal cost five integer divisions per
// entry and lane there)
__device__ __forceinline__ uint32_t pack_source(const DeformArgs& a, int n, int oh, int ow, int t,
                                                int corner) {
  return ((((((uint32_t)n << a.bh) | (uint32_t)oh) << a.bw) | (uint32_t)ow) << 6) |
         ((uint32_t)t << 2) | (uint32_t)corner;
}

int bit_width(uint32_t v) {
  int b = 0;
  while (v) { ++b; v >>= 1; }
  return b;
}

struct Pos {
  float y, x;              // clipped sample position (padded coordinates)
  int y0, y1, x0, x1;      // clipped corners
  float fy0, fy1, fx0, fx1;
  bool pass_y, pass_x;     // clip_by_value passes the gradient
};

__device__ __forceinline__ Pos sample_pos(const DeformArgs& a, int oh, int ow, int t, float dy,
                                          float dx) {
  const int kh = (t * 11) >> 5, kw = t - kh * a.k;  // t / k for k in {1, 3}, t < k*k
  const float hmax = (float)(a.Hp - 1), wmax = (float)(a.Wp - 1);
  const float yy = (float)(oh * a.stride + kh * a.rate) + dy;
  const float xx = (float)(ow * a.stride + kw * a.rate) + dx;
  Pos p;
  p.pass_y = yy >= 0.f && yy <= hmax;
  p.pass_x = xx >= 0.f && xx <= wmax;
  p.y = fmaxf(fminf(yy, hmax), 0.f);
  p.x = fmaxf(fminf(xx, wmax), 0.f);
  const int fy = (int)floorf(p.y), fx = (int)floorf(p.x);
  p.y0 = min(max(fy, 0), a.Hp - 1);
  p.y1 = min(max(fy + 1, 0), a.Hp - 1);
  p.x0 = min(max(fx, 0), a.Wp - 1);
  p.x1 = min(max(fx + 1, 0), a.Wp - 1);
  p.fy0 = (float)p.y0; p.fy1 = (float)p.y1;
  p.fx0 = (float)p.x0; p.fx1 = (float)p.x1;
  return p;
}

// unpadded pixel index (h * W + w) of a padded corner, -1 in the pad ring
__device__ __forceinline__ int pixel_of(const DeformArgs& a, int yc, int xc) {
  const int h = yc - a.pb, w = xc - a.pb;
  return (h >= 0 && h < a.H && w >= 0 && w < a.W) ? h * a.W + w : -1;
}

__device__ __forceinline__ float4 ld4_or_zero(const float* base, int pix, int C, int ch) {
  if (pix < 0) return make_float4(0.f, 0.f, 0.f, 0.f);
  return *reinterpret_cast<const float4*>(base + (size_t)pix * C + ch);
}

__global__ __launch_bounds__(256) void deform_fwd_kernel(const float* __restrict__ x,
                                                         const float* __restrict__ offsets,
                                                         DeformArgs a, int total,
                                                         float* __restrict__ cols) {
  const int wv = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (wv >= total) return;
  const int lane = threadIdx.x & 63;
  const int g = wv % a.G, loc = wv / a.G;  // loc = (n * OH + oh) * OW + ow
  const int ow = loc % a.OW, oh = (loc / a.OW) % a.OH, n = loc / (a.OW * a.OH);
  const float* xn = x + (size_t)n * a.H * a.W * a.C;
  const float* off = offsets + (size_t)loc * a.off_stride + g * a.KK * 2;
  const int R = a.Cg >> 2;
#pragma unroll 3  // (three taps' corner loads in flight)
  for (int t = 0; t < a.KK; ++t) {
    const Pos p = sample_pos(a, oh, ow, t, off[2 * t], off[2 * t + 1]);
    const float w0 = (p.fy1 - p.y) * (p.fx1 - p.x), w1 = (p.fy1 - p.y) * (p.x - p.fx0);
    const float w2 = (p.y - p.fy0) * (p.fx1 - p.x), w3 = (p.y - p.fy0) * (p.x - p.fx0);
    const int i0 = pixel_of(a, p.y0, p.x0), i1 = pixel_of(a, p.y0, p.x1);
    const int i2 = pixel_of(a, p.y1, p.x0), i3 = pixel_of(a, p.y1, p.x1);
    float* dst = cols + ((size_t)loc * a.KK + t) * a.C + g * a.Cg;
    for (int r = lane; r < R; r += 64) {
      const int ch = g * a.Cg + 4 * r;
      const float4 p0 = ld4_or_zero(xn, i0, a.C, ch), p1 = ld4_or_zero(xn, i1, a.C, ch);
      const float4 p2 = ld4_or_zero(xn, i2, a.C, ch), p3 = ld4_or_zero(xn, i3, a.C, ch);
      float4 v;
      v.x = ((w0 * p0.x + w1 * p1.x) + w2 * p2.x) + w3 * p3.x;
      v.y = ((w0 * p0.y + w1 * p1.y) + w2 * p2.y) + w3 * p3.y;
      v.z = ((w0 * p0.z + w1 * p1.z) + w2 * p2.z) + w3 * p3.z;
      v.w = ((w0 * p0.w + w1 * p1.w) + w2 * p2.w) + w3 * p3.w;
      *reinterpret_cast<float4*>(dst + 4 * r) = v;
    }
  }
}

// goffsets: 16 lanes per item (loc, g, t); goff rows have goff_stride floats,
// the ones past 2*G*KK are written 0 (a row padded for the offset conv's
// dgrad / wgrad)
__global__ __launch_bounds__(256) void deform_goff_kernel(const float* __restrict__ x,
                                                          const float* __restrict__ offsets,
                                                          const float* __restrict__ gcols,
                                                          DeformArgs a, int items, int goff_stride,
                                                          float* __restrict__ goff) {
  const int item = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  const bool live = item < items;
  const int it = live ? item : 0;
  const int t = it % a.KK, g = (it / a.KK) % a.G, loc = it / (a.KK * a.G);
  const int ow = loc % a.OW, oh = (loc / a.OW) % a.OH, n = loc / (a.OW * a.OH);
  const float* xn = x + (size_t)n * a.H * a.W * a.C;
  const int oc = (g * a.KK + t) * 2;
  const float* off = offsets + (size_t)loc * a.off_stride + oc;
  const Pos p = sample_pos(a, oh, ow, t, off[0], off[1]);
  const float ax1 = p.fx1 - p.x, ax0 = p.x - p.fx0, ay1 = p.fy1 - p.y, ay0 = p.y - p.fy0;
  const int i0 = pixel_of(a, p.y0, p.x0), i1 = pixel_of(a, p.y0, p.x1);
  const int i2 = pixel_of(a, p.y1, p.x0), i3 = pixel_of(a, p.y1, p.x1);
  const float* gc = gcols + ((size_t)loc * a.KK + t) * a.C + g * a.Cg;
  const int R = a.Cg >> 2;
  float sy = 0.f, sx = 0.f;
  for (int r = sub; r < R; r += 16) {
    const int ch = g * a.Cg + 4 * r;
    const float4 p0 = ld4_or_zero(xn, i0, a.C, ch), p1 = ld4_or_zero(xn, i1, a.C, ch);
    const float4 p2 = ld4_or_zero(xn, i2, a.C, ch), p3 = ld4_or_zero(xn, i3, a.C, ch);
    const float4 gv = *reinterpret_cast<const float4*>(gc + 4 * r);
#define D2MI_DEFORM_TERM(F)                                                              \
    sy += gv.F * (((-(ax1 * p0.F) - ax0 * p1.F) + ax1 * p2.F) + ax0 * p3.F);             \
    sx += gv.F * (((-(ay1 * p0.F) + ay1 * p1.F) - ay0 * p2.F) + ay0 * p3.F);
    D2MI_DEFORM_TERM(x) D2MI_DEFORM_TERM(y) D2MI_DEFORM_TERM(z) D2MI_DEFORM_TERM(w)
#undef D2MI_DEFORM_TERM
  }
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) {
    sy += __shfl_xor(sy, m, 16);
    sx += __shfl_xor(sx, m, 16);
  }
  if (!live) return;
  float* row = goff + (size_t)loc * goff_stride;
  if (sub == 0) {
    row[oc] = p.pass_y ? sy : 0.f;
    row[oc + 1] = p.pass_x ? sx : 0.f;
  }
  const int OC = 2 * a.G * a.KK;
  if (t == 0 && g == 0 && OC + sub < goff_stride) row[OC + sub] = 0.f;
}

// one thread per item (loc, g, t): its four corner keys
__global__ __launch_bounds__(256) void deform_emit_kernel(const float* __restrict__ offsets,
                                                          DeformArgs a, int items,
                                                          uint64_t* __restrict__ keys) {
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= items) return;
  // item order (loc, g, t): the key's low word is group-free
  const int t = item % a.KK, g = (item / a.KK) % a.G, loc = item / (a.KK * a.G);
  const int ow = loc % a.OW, oh = (loc / a.OW) % a.OH, n = loc / (a.OW * a.OH);
  const float* off = offsets + (size_t)loc * a.off_stride + (g * a.KK + t) * 2;
  const Pos p = sample_pos(a, oh, ow, t, off[0], off[1]);
  const int pix[4] = {pixel_of(a, p.y0, p.x0), pixel_of(a, p.y0, p.x1), pixel_of(a, p.y1, p.x0),
                      pixel_of(a, p.y1, p.x1)};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    uint64_t key = ~0ull;
    if (pix[c] >= 0) {
      const uint32_t dest = ((uint32_t)n * (a.H * a.W) + pix[c]) * a.G + g;
      key = ((uint64_t)dest << 32) | (uint64_t)pack_source(a, n, oh, ow, t, c);
    }
    keys[(size_t)item * 4 + c] = key;
  }
}

// ---- stable LSD radix sort of the keys by destination (the high word; ~0
// keys take the digit of `ndest`, one past the last destination, and end up
// last).  A workgroup owns a tile of kRadixTile consecutive keys.
constexpr int kRadixTile = 4096;  // 4 waves x 16 rows x 64 lanes
constexpr int kRadixRows = kRadixTile / 256;
constexpr int kRadixMaxBits = 8, kRadixMaxBins = 1 << kRadixMaxBits;

__device__ __forceinline__ int digit_of(uint64_t key, uint32_t ndest, int shift, int mask) {
  const uint32_t d = min((uint32_t)(key >> 32), ndest);
  return (int)((d >> shift) & (uint32_t)mask);
}

// hist[bin * nblk + block] = keys of the block's tile with that digit
__global__ __launch_bounds__(256) void radix_hist_kernel(const uint64_t* __restrict__ keys, int n,
                                                         uint32_t ndest, int shift, int nbins,
                                                         int nblk, int32_t* __restrict__ hist) {
  __shared__ int32_t cnt[kRadixMaxBins];
  for (int i = threadIdx.x; i < nbins; i += 256) cnt[i] = 0;
  __syncthreads();
  const int t0 = blockIdx.x * kRadixTile;
  for (int j = threadIdx.x; j < kRadixTile; j += 256) {
    const int i = t0 + j;
    if (i < n) atomicAdd(&cnt[digit_of(keys[i], ndest, shift, nbins - 1)], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += 256) hist[i * nblk + blockIdx.x] = cnt[i];
}

// per digit (one wave each): the in-place exclusive scan of its row
// hist[bin][0..nblk) over the tiles, and the row total -> bintot[bin]; the
// scan over the (<= 256) digits is done by every scatter workgroup itself
__global__ __launch_bounds__(64) void radix_rowscan_kernel(int32_t* __restrict__ hist, int nblk,
                                                           int32_t* __restrict__ bintot) {
  const int lane = threadIdx.x;
  int32_t* row = hist + (size_t)blockIdx.x * nblk;
  int32_t carry = 0;
  for (int c0 = 0; c0 < nblk; c0 += 64) {
    const int i = c0 + lane;
    const int32_t v = i < nblk ? row[i] : 0;
    int32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t t = __shfl_up(x, d);
      if (lane >= d) x += t;
    }
    if (i < nblk) row[i] = carry + x - v;
    carry += __shfl(x, 63);
  }
  if (lane == 0) bintot[blockIdx.x] = carry;
}

// out[start of (digit, block) + rank inside the tile] = key, ranks in tile
// order: wave w owns rows [w * 16, w * 16 + 16) of the tile and walks them in
// order; inside a row a key's rank among equal digits is the count of lower
// lanes with that digit (ballots)
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint64_t* __restrict__ in,
                                                            uint64_t* __restrict__ out, int n,
                                                            uint32_t ndest, int shift, int nbits,
                                                            int nblk,
                                                            const int32_t* __restrict__ hist,
                                                            const int32_t* __restrict__ bintot) {
  __shared__ int32_t base[4][kRadixMaxBins];
  __shared__ int32_t binbase[kRadixMaxBins];
  const int nbins = 1 << nbits;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < 4 * kRadixMaxBins; i += 256) (&base[0][0])[i] = 0;
  // exclusive scan of the digit totals (thread = digit; kRadixMaxBins == 256)
  const int32_t tot = (int)threadIdx.x < nbins ? bintot[threadIdx.x] : 0;
  binbase[threadIdx.x] = tot;
  __syncthreads();
  for (int d = 1; d < kRadixMaxBins; d <<= 1) {
    const int32_t v = (int)threadIdx.x >= d ? binbase[threadIdx.x - d] : 0;
    __syncthreads();
    binbase[threadIdx.x] += v;
    __syncthreads();
  }
  const int32_t mybase = binbase[threadIdx.x] - tot;
  __syncthreads();
  binbase[threadIdx.x] = mybase;
  __syncthreads();
  const int w0 = blockIdx.x * kRadixTile + w * (kRadixRows * 64);
  for (int row = 0; row < kRadixRows; ++row) {
    const int i = w0 + row * 64 + lane;
    if (i < n) atomicAdd(&base[w][digit_of(in[i], ndest, shift, nbins - 1)], 1);
  }
  __syncthreads();
  for (int bin = threadIdx.x; bin < nbins; bin += 256) {
    int32_t run = binbase[bin] + hist[bin * nblk + blockIdx.x];
    for (int v = 0; v < 4; ++v) {
      const int32_t c = base[v][bin];
      base[v][bin] = run;
      run += c;
    }
  }
  __syncthreads();
  const uint64_t lower = (1ull << lane) - 1ull;
  for (int row = 0; row < kRadixRows; ++row) {
    const int i = w0 + row * 64 + lane;
    const bool valid = i < n;
    const uint64_t key = valid ? in[i] : 0ull;
    const int d = valid ? digit_of(key, ndest, shift, nbins - 1) : 0;
    uint64_t peers = __ballot(valid);
    for (int bit = 0; bit < nbits; ++bit) {
      const bool one = (d >> bit) & 1;
      const uint64_t bm = __ballot(valid && one);
      peers &= one ? bm : ~bm;
    }
    const int rank = __popcll(peers & lower);
    int32_t start = 0;
    if (valid) start = base[w][d];
    __syncthreads();  // every lane has read its start before a leader moves it
    if (valid) {
      out[start + rank] = key;
      if (rank == 0) base[w][d] = start + __popcll(peers);
    }
    __syncthreads();
  }
}

constexpr int kChunk = 512, kInFlight = 8;

__device__ __forceinline__ int lower_bound_key(const uint64_t* __restrict__ keys, int n,
                                               uint64_t v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (keys[m] < v) lo = m + 1;
    else hi = m;
  }
  return lo;
}

// start[d] = first sorted key of destination d, d in [0, ndest] (one thread
// each: a wave searching for its own list alone paid 2 x 21 dependent loads)
__global__ __launch_bounds__(256) void deform_bounds_kernel(const uint64_t* __restrict__ keys,
                                                            int nkeys, int ndest,
                                                            int32_t* __restrict__ start) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d <= ndest) start[d] = lower_bound_key(keys, nkeys, (uint64_t)(uint32_t)d << 32);
}

__global__ __launch_bounds__(256) void deform_gx_kernel(const uint64_t* __restrict__ keys,
                                                        const int32_t* __restrict__ start,
                                                        const float* __restrict__ offsets,
                                                        const float* __restrict__ gcols,
                                                        DeformArgs a, int nblk, int total,
                                                        float* __restrict__ gx) {
  const int wv = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (wv >= total) return;
  const int lane = threadIdx.x & 63;
  const int blk = wv % nblk, dest = wv / nblk;  // dest = pixel * G + g
  const int g = dest % a.G;
  const int R = a.Cg >> 2;
  const int Rb = min(R - blk * 64, 64);  // float4 lanes of this channel block
  const int S = 64 / Rb;                 // entry slots
  const int slot = lane / Rb, r = lane - slot * Rb;
  const bool active = slot < S;
  const int ch = g * a.Cg + (blk * 64 + r) * 4;
  const int lo = start[dest], hi = start[dest + 1];
  float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c0 = lo; c0 < hi; c0 += kChunk) {
    const int c1 = min(c0 + kChunk, hi);
    float4 part = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b0 = c0; b0 < c1; b0 += 64) {
      // 64 keys with one coalesced load, handed to their slots by shuffles;
      // then kInFlight entries of a slot at a time: their offsets and gcols
      // rows are loaded together and added in order
      const int nb = min(64, c1 - b0);
      const uint32_t mine = lane < nb ? (uint32_t)keys[b0 + lane] : 0u;
      for (int j0 = 0; j0 < nb; j0 += kInFlight * S) {
        uint32_t ord[kInFlight];
        bool ok[kInFlight];
        float dy[kInFlight], dx[kInFlight];
        float4 gv[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
          const int j = j0 + u * S + slot;
          ord[u] = __shfl(mine, j & 63);
          ok[u] = active && j < nb;
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
          if (!ok[u]) continue;
          const int t = (ord[u] >> 2) & 15;
          const int ow = (ord[u] >> 6) & ((1 << a.bw) - 1);
          const int oh = (ord[u] >> (6 + a.bw)) & ((1 << a.bh) - 1);
          const int loc = ((int)(ord[u] >> (6 + a.bw + a.bh)) * a.OH + oh) * a.OW + ow;
          const size_t st = (size_t)loc * a.KK + t;
          const float* off = offsets + (size_t)loc * a.off_stride + (g * a.KK + t) * 2;
          dy[u] = off[0];
          dx[u] = off[1];
          gv[u] = *reinterpret_cast<const float4*>(gcols + st * a.C + ch);
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
          if (!ok[u]) continue;
          const int corner = ord[u] & 3u;
          const int t = (ord[u] >> 2) & 15;
          const int ow = (ord[u] >> 6) & ((1 << a.bw) - 1);
          const int oh = (ord[u] >> (6 + a.bw)) & ((1 << a.bh) - 1);
          const Pos p = sample_pos(a, oh, ow, t, dy[u], dx[u]);
          const float wy = (corner & 2) ? (p.y - p.fy0) : (p.fy1 - p.y);
          const float wx = (corner & 1) ? (p.x - p.fx0) : (p.fx1 - p.x);
          const float w = wy * wx;
          part.x += gv[u].x * w; part.y += gv[u].y * w;
          part.z += gv[u].z * w; part.w += gv[u].w * w;
        }
      }
    }
    // slots added in slot order into slot 0's lanes
    float4 sum = part;
    for (int s = 1; s < S; ++s) {
      const int src = (r + s * Rb) & 63;
      sum.x += __shfl(part.x, src); sum.y += __shfl(part.y, src);
      sum.z += __shfl(part.z, src); sum.w += __shfl(part.w, src);
    }
    tot.x += sum.x; tot.y += sum.y; tot.z += sum.z; tot.w += sum.w;
  }
  if (slot == 0) *reinterpret_cast<float4*>(gx + (size_t)(dest / a.G) * a.C + ch) = tot;
}

int make_args(DeformArgs* a, int N, int H, int W, int C, int G, int k, int stride, int rate,
              int pb, int pe, int off_stride) {
  D2MI_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && G > 0, "deform_sample: bad shape");
  D2MI_REQUIRE(k == 1 || k == 3, "deform_sample: kernel size %d (1 and 3 are supported)", k);
  D2MI_REQUIRE(C % G == 0, "deform_sample: C %d is not divisible by the %d deformable groups", C,
               G);
  D2MI_REQUIRE((C / G) % 4 == 0,
               "deform_sample: channels per deformable group (%d) must be a multiple of 4", C / G);
  D2MI_REQUIRE(stride >= 1 && rate >= 1, "deform_sample: stride and rate must be >= 1");
  D2MI_REQUIRE(pb >= 0 && pe >= 0, "deform_sample: negative padding");
  const int keff = k + (k - 1) * (rate - 1);
  const int64_t Hp = (int64_t)H + pb + pe, Wp = (int64_t)W + pb + pe;
  D2MI_REQUIRE(Hp >= keff && Wp >= keff, "deform_sample: padded input smaller than the kernel");
  const int64_t OH = (Hp - keff) / stride + 1, OW = (Wp - keff) / stride + 1;
  const int OC = 2 * G * k * k;
  D2MI_REQUIRE(off_stride >= OC, "deform_sample: offset row stride %d < %d channels", off_stride,
               OC);
  // 32-bit key halves and int indices: destinations (N*H*W*G) and the key
  // count (N*OH*OW*G*k*k*4) below 2^31, the source word's fields in 32 bits
  D2MI_REQUIRE((int64_t)N * H * W * G < (1ll << 31) - 1 && Hp * Wp < (1ll << 31) &&
                   (int64_t)N * OH * OW * G * k * k * 4 < (1ll << 31) - 1024,
               "deform_sample: index range exceeds the 32-bit key halves");
  const int bh = bit_width((uint32_t)(OH - 1)), bw = bit_width((uint32_t)(OW - 1));
  D2MI_REQUIRE(bit_width((uint32_t)(N - 1)) + bh + bw + 6 <= 31,
               "deform_sample: index range exceeds the 32-bit key halves");
  *a = DeformArgs{N, H, W, C, G, C / G, k, k * k, stride, rate, pb, (int)Hp, (int)Wp, (int)OH,
                  (int)OW, off_stride, bh, bw};
  return 0;
}

size_t key_count(const DeformArgs& a) { return (size_t)a.N * a.OH * a.OW * a.G * a.KK * 4; }

size_t hist_count(size_t cap) {
  return (size_t)kRadixMaxBins * ((cap + kRadixTile - 1) / kRadixTile + 1);  // + the digit totals
}

struct BwdSpace {
  uint64_t* keys[2];  // ping-pong
  int32_t* hist;      // [bins][tiles] + the digit totals
  int32_t* start;     // [destinations + 1]
  template <typename A>
  void lay(A& w, const DeformArgs& a) {
    const size_t cap = key_count(a);
    keys[0] = w.template take<uint64_t>(cap);
    keys[1] = w.template take<uint64_t>(cap);
    hist = w.template take<int32_t>(hist_count(cap));
    start = w.template take<int32_t>((size_t)a.N * a.H * a.W * a.G + 1);
  }
};

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace d2mi

using namespace d2mi;

extern "C" int d2mi_deform_sample_fwd(const float* x, const float* offsets, int N, int H, int W,
                                      int C, int G, int k, int stride, int rate, int pb, int pe,
                                      int off_stride, float* cols, void* stream) {
  DeformArgs a;
  if (int rc = make_args(&a, N, H, W, C, G, k, stride, rate, pb, pe, off_stride)) return rc;
  D2MI_REQUIRE(x && offsets && cols && aligned16(x) && aligned16(cols),
               "deform_sample: x / cols must be non-null and 16-byte aligned");
  const int total = N * a.OH * a.OW * G;
  hipLaunchKernelGGL(deform_fwd_kernel, dim3((total + 3) / 4), dim3(256), 0, as_stream(stream), x,
                     offsets, a, total, cols);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t d2mi_deform_sample_bwd_workspace_size(int N, int H, int W, int C, int G, int k,
                                                        int stride, int rate, int pb, int pe) {
  DeformArgs a;
  if (make_args(&a, N, H, W, C, G, k, stride, rate, pb, pe, 2 * G * k * k)) return 0;
  return layout_bytes<BwdSpace>(a);
}

extern "C" int d2mi_deform_sample_bwd(const float* x, const float* offsets, const float* gcols,
                                      int N, int H, int W, int C, int G, int k, int stride,
                                      int rate, int pb, int pe, int off_stride, int goff_stride,
                                      float* gx, float* goffsets, void* ws, size_t ws_bytes,
                                      void* stream) {
  DeformArgs a;
  if (int rc = make_args(&a, N, H, W, C, G, k, stride, rate, pb, pe, off_stride)) return rc;
  const int OC = 2 * G * a.KK;
  D2MI_REQUIRE(goff_stride >= OC && goff_stride <= OC + 16,
               "deform_sample_bwd: offset-gradient row stride %d outside [%d, %d]", goff_stride, OC,
               OC + 16);
  D2MI_REQUIRE(x && offsets && gcols && aligned16(x) && aligned16(gcols) && aligned16(gx),
               "deform_sample_bwd: x / gcols / gx must be 16-byte aligned");
  D2MI_REQUIRE(gx || goffsets, "deform_sample_bwd: nothing to compute");
  hipStream_t st = as_stream(stream);
  const int items = N * a.OH * a.OW * G * a.KK;
  if (goffsets) {
    hipLaunchKernelGGL(deform_goff_kernel, dim3((items + 15) / 16), dim3(256), 0, st, x, offsets,
                       gcols, a, items, goff_stride, goffsets);
    D2MI_LAUNCH_CHECK();
  }
  if (!gx) return 0;
  Workspace w(ws, ws_bytes);
  BwdSpace s;
  s.lay(w, a);
  D2MI_REQUIRE(ws && w.ok(), "deform_sample_bwd: workspace too small (%zu < %zu)", ws_bytes, w.off);
  hipLaunchKernelGGL(deform_emit_kernel, dim3((items + 255) / 256), dim3(256), 0, st, offsets, a,
                     items, s.keys[0]);
  D2MI_LAUNCH_CHECK();
  const int cap = items * 4;
  const uint32_t ndest = (uint32_t)((int64_t)N * H * W * G);
  const int bits = bit_width(ndest);  // (ndest itself is the ~0 keys' digit source)
  const int npass = (bits + kRadixMaxBits - 1) / kRadixMaxBits;
  const int rb = (bits + npass - 1) / npass;
  const int tiles = (cap + kRadixTile - 1) / kRadixTile;
  int cur = 0;
  for (int p = 0; p < npass; ++p, cur ^= 1) {
    hipLaunchKernelGGL(radix_hist_kernel, dim3(tiles), dim3(256), 0, st, s.keys[cur], cap, ndest,
                       p * rb, 1 << rb, tiles, s.hist);
    D2MI_LAUNCH_CHECK();
    int32_t* bintot = s.hist + (size_t)kRadixMaxBins * tiles;
    hipLaunchKernelGGL(radix_rowscan_kernel, dim3(1 << rb), dim3(64), 0, st, s.hist, tiles, bintot);
    D2MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(tiles), dim3(256), 0, st, s.keys[cur],
                       s.keys[cur ^ 1], cap, ndest, p * rb, rb, tiles, s.hist, bintot);
    D2MI_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(deform_bounds_kernel, dim3(ndest / 256 + 1), dim3(256), 0, st, s.keys[cur],
                     cap, (int)ndest, s.start);
  D2MI_LAUNCH_CHECK();
  const int R = a.Cg / 4, nblk = (R + 63) / 64;
  const int64_t total = (int64_t)N * H * W * G * nblk;
  D2MI_REQUIRE(total < (1ll << 31) - 4, "deform_sample_bwd: too many destination blocks");
  hipLaunchKernelGGL(deform_gx_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, st,
                     s.keys[cur], s.start, offsets, gcols, a, nblk, (int)total, gx);
  D2MI_LAUNCH_CHECK();
  return 0;
}
