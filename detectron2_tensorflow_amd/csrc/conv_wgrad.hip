// Weight gradient of the NHWC convolution on gfx950 fp32 MFMA
// (v_mfma_f32_32x32x2_f32) — the backward of the FPN output / RPN share /
// mask-head 3x3 convs (lib/layers/convolutional.py:198-263 under tf.gradients).
//
//   dW[kh][kw][ci][co] = sum over pixels p=(n,oy,ox) of
//                        X[n, oy*s - pad + kh, ox*s - pad + kw, ci] * dY[p][co]
//
// GEMM view per tap (kh, kw): C[ci][co] = A^T B with A = X shifted [P][Cin] and
// B = dY [P][Cout] — both stored pixel-major with the OUTPUT dims contiguous
// ("TN" GEMM).  That is the natural operand order of the f32 32x32x2 MFMA,
// where lane l supplies A[l%32][k = l/32]: the LDS image keeps global rows as
// they are (k = pixel rows, channels contiguous) and every operand fetch is one
// conflict-free ds_read_b32 (the row pitch puts the two lane halves on
// disjoint bank halves).  A 256-thread workgroup (2x2 waves, TMxTN 32x32 MFMA
// tiles per wave) owns a (BM channels) x (BN out-channels) tile of one tap and
// walks a contiguous range of 32-pixel chunks; the pixel range is split over
// gridDim.y workgroups whose partial tiles are summed by a second kernel in a
// FIXED split order (deterministic).  Global loads of the next chunk are issued
// before the current chunk's MFMAs (register double buffering).
#include "common.h"
#include "conv_plan.h"
#include "internal.h"

namespace d2mi {
namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int KP = kWgradKP;  // pixels per k-step

struct WgradArgs {
  const float* x;   // [N,H,W,Cin]
  const float* dy;  // [N,OH,OW,Cout]
  float* dw;        // [KH,KW,Cin,Cout]
  float* partial;   // [splits][KH*KW*Cin*Cout] when splits > 1
  float* dbias;     // [Cout] bias gradient sum_p dy[p][co] (nullable)
  float* pbias;     // [splits][Cout] partial bias sums when splits > 1
  int N, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW;
  int P;                      // N*OH*OW
  int nCi, nCo, ntiles;       // channel tiles per tap, co tiles, total tiles
  int splits, chunks_per_split, nchunks;
  // the partial slabs are written (splits > 1, or an accumulating call:
  // the reduce then adds the sum into dw / dbias)
  int part;
  int x_bytes, dy_bytes;  // buffer ranges (split kernel; < 2 GiB)
  // tuning "wgrad_prio" (default 1, 0 off): wave priority 1 while issuing the
  // chunk's MFMAs, as conv_mfma.hip.  Measured (tools/ab_prio.sh): the wgrad
  // set 1.9 % faster in total (FPN p2 3x3 1025 -> 1008 us, res5 3x3 97 -> 92),
  // the training bench +1.4 % (89.6 -> 90.9 img/s, two alternating pairs).
  int prio;
  // tuning "wgrad_xcd" (default 1): the (tile, split) grid walked in an
  // XCD-contiguous order -- the tiles of one pixel range (its taps and channel
  // blocks, which read the same x rows and dY chunk) land on one XCD, so the
  // re-reads meet in that XCD's L2 instead of eight.  Bit-identical (each
  // workgroup's (tile, split) work is unchanged, only its placement).
  int xcd;
  // conv_wgrad_ws_kernel<.., LIST>: one bit per 32-pixel chunk, set where dy may
  // hold a non-zero row (RowCensusSpace::bitmap; d2mi_conv2d_wgrad_rows)
  const uint32_t* bitmap;
};

// (tile, split) of this workgroup: blockIdx as launched, or its XCD-contiguous
// remap (hardware dispatch puts linear workgroup L on XCD L % 8; logical index
// l = the L-th of XCD L % 8's contiguous block, tile fastest).
__device__ __forceinline__ void wgrad_tile_split(const WgradArgs& a, int& tile, int& split) {
  if (!a.xcd) {
    tile = blockIdx.x;
    split = blockIdx.y;
    return;
  }
  const int nwg = gridDim.x * gridDim.y;
  const int L = blockIdx.x + blockIdx.y * gridDim.x;
  const int q = nwg / 8, r8 = nwg % 8, x8 = L % 8;
  const int l = (x8 < r8 ? x8 * (q + 1) : r8 * (q + 1) + (x8 - r8) * q) + L / 8;
  split = l / gridDim.x;
  tile = l - split * gridDim.x;
}

template <int TM, int TN>
__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(WgradArgs a) {
  constexpr int BM = 2 * TM * 32, BN = 2 * TN * 32;
  constexpr int PA = BM + 32, PB = BN + 32;  // row pitch: lane halves on disjoint banks
  constexpr int CA = BM / 4, CB = BN / 4;    // float4 columns per row
  constexpr int RA = KP * CA / 256, RB = KP * CB / 256;  // float4 loads per thread
  __shared__ __attribute__((aligned(16))) float As[KP * PA];
  __shared__ __attribute__((aligned(16))) float Bs[KP * PB];

  const int tile = blockIdx.x;
  const int per_tap = a.nCi * a.nCo;
  const int tap = tile / per_tap;
  const int rem = tile - tap * per_tap;
  const int cit = rem / a.nCo, cot = rem - cit * a.nCo;
  const int kh = tap / a.KW, kw = tap - kh * a.KW;
  const int ci0 = cit * BM, co0 = cot * BN;
  const int split = blockIdx.y;
  const int c_begin = split * a.chunks_per_split;
  const int c_end = min(a.nchunks, c_begin + a.chunks_per_split);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int li = lane & 31, lh = lane >> 5;

  float4 ra[RA], rb[RB];
  auto load_chunk = [&](int ch) {
    const int pbase = ch * KP;
#pragma unroll
    for (int q = 0; q < RA; ++q) {
      const int idx = tid + 256 * q;
      const int row = idx / CA, c4 = idx - row * CA;
      const int p = pbase + row;
      const int ci = ci0 + c4 * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p < a.P && ci < a.Cin) {
        const int n = p / (a.OH * a.OW);
        const int r2 = p - n * a.OH * a.OW;
        const int oy = r2 / a.OW, ox = r2 - oy * a.OW;
        const int iy = oy * a.stride - a.pad + kh, ix = ox * a.stride - a.pad + kw;
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
          v = *reinterpret_cast<const float4*>(a.x + (((size_t)n * a.H + iy) * a.W + ix) * a.Cin +
                                               ci);
      }
      ra[q] = v;
    }
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      const int idx = tid + 256 * q;
      const int row = idx / CB, c4 = idx - row * CB;
      const int p = pbase + row;
      const int co = co0 + c4 * 4;
      rb[q] = (p < a.P && co < a.Cout)
                  ? *reinterpret_cast<const float4*>(a.dy + (size_t)p * a.Cout + co)
                  : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int q = 0; q < RA; ++q) {
      const int idx = tid + 256 * q;
      const int row = idx / CA, c4 = idx - row * CA;
      *reinterpret_cast<float4*>(&As[row * PA + c4 * 4]) = ra[q];
    }
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      const int idx = tid + 256 * q;
      const int row = idx / CB, c4 = idx - row * CB;
      *reinterpret_cast<float4*>(&Bs[row * PB + c4 * 4]) = rb[q];
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // the tap-0 / first-channel-tile blocks also sum dy's columns (bias gradient)
  const bool do_bias = a.dbias != nullptr && tap == 0 && cit == 0;
  float bsum = 0.f;

  if (c_begin < c_end) {
    load_chunk(c_begin);
    for (int ch = c_begin; ch < c_end; ++ch) {
      store_chunk();
      __syncthreads();
      if (ch + 1 < c_end) load_chunk(ch + 1);
      if (do_bias && tid < BN) {
#pragma unroll 8
        for (int k = 0; k < KP; ++k) bsum += Bs[k * PB + tid];
      }
#pragma unroll 4
      for (int k = 0; k < KP; k += 2) {
        const float* Ar = &As[(k + lh) * PA + wr * TM * 32 + li];
        const float* Br = &Bs[(k + lh) * PB + wc * TN * 32 + li];
        float fa[TM], fb[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i] = Ar[i * 32];
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[j] = Br[j * 32];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
  }

  if (do_bias && tid < BN && co0 + tid < a.Cout) {
    if (a.part) a.pbias[(size_t)split * a.Cout + co0 + tid] = bsum;
    else a.dbias[co0 + tid] = bsum;
  }

  // C/D map for 32x32: col (co) = lane & 31, row (ci) = (r&3) + 8*(r>>2) + 4*(lane>>5)
  const size_t wsz = (size_t)a.KH * a.KW * a.Cin * a.Cout;
  float* out = a.part ? a.partial + (size_t)split * wsz : a.dw;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int co = co0 + (wc * TN + j) * 32 + li;
    if (co >= a.Cout) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int cb = ci0 + (wr * TM + i) * 32 + 4 * lh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ci = cb + (r & 3) + 8 * (r >> 2);
        if (ci < a.Cin) out[((size_t)tap * a.Cin + ci) * a.Cout + co] = acc[i][j][r];
      }
    }
  }
}

// Fixed split order (deterministic); the last Cout entries are the bias
// gradient when pbias follows the weight partials.
// float4 form (total % 4 == 0, 16-B aligned): the same per-element split
// order, four elements and their split loads in flight per thread.
// accum: dw / dbias += the sum (a level accumulator: the old value plus this
// call's gradient, autograd's order for a weight shared by several calls).
__global__ void wgrad_reduce4_kernel(const float4* __restrict__ partial, int splits, size_t total4,
                                     float4* __restrict__ dw, const float* __restrict__ pbias,
                                     int Cout, float* __restrict__ dbias, int accum) {
  const size_t n = total4 + (dbias ? (size_t)Cout : 0);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    if (i < total4) {
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
      for (int k = 0; k < splits; ++k) {
        const float4 v = partial[(size_t)k * total4 + i];
        s.x += v.x;
        s.y += v.y;
        s.z += v.z;
        s.w += v.w;
      }
      if (accum) {
        const float4 o = dw[i];
        s.x = o.x + s.x;
        s.y = o.y + s.y;
        s.z = o.z + s.z;
        s.w = o.w + s.w;
      }
      dw[i] = s;
    } else {
      const size_t c = i - total4;
      float s = 0.f;
#pragma unroll 8  // (loads in flight; the sum stays in split order)
      for (int k = 0; k < splits; ++k) s += pbias[(size_t)k * Cout + c];
      dbias[c] = accum ? dbias[c] + s : s;
    }
  }
}

__global__ void wgrad_reduce_kernel(const float* __restrict__ partial, int splits, size_t total,
                                    float* __restrict__ dw, const float* __restrict__ pbias,
                                    int Cout, float* __restrict__ dbias, int accum) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total + Cout;
       i += (size_t)gridDim.x * blockDim.x) {
    if (i < total) {
      float s = 0.f;
#pragma unroll 4
      for (int k = 0; k < splits; ++k) s += partial[(size_t)k * total + i];
      dw[i] = accum ? dw[i] + s : s;
    } else if (dbias) {
      const size_t c = i - total;
      float s = 0.f;
#pragma unroll 8  // (loads in flight; the sum stays in split order)
      for (int k = 0; k < splits; ++k) s += pbias[(size_t)k * Cout + c];
      dbias[c] = accum ? dbias[c] + s : s;
    }
  }
}

// ---------------------------------------------------------------------------
// Split-product variant (d2mi_conv2d_wgrad_ex flags bit 2): the same GEMM on
// the bf16 MFMA with each f32 operand split exactly into three bf16 terms
// (h + m + l == x, truncation) and six products per k-step, as
// conv_mfma.hip's SPLIT path.  The MFMA operand wants 8 consecutive PIXELS of
// one channel, so each thread loads 4 pixels x 4 channels (four float4),
// transposes them in registers, splits, and writes 4 pixels (8 B) per plane
// per channel into [plane][channel][32 pixels] LDS images with XOR-swizzled
// 16-B chunks.  The bias gradient is summed from the f32 dY values before
// the split and reduced over the pixel groups in a fixed order.

typedef short bf16x8 __attribute__((ext_vector_type(8)));
constexpr int LDW = 32;  // bf16 per LDS row (one 32-pixel chunk)

__device__ __forceinline__ int wswz(int row, int elem) {
  return row * LDW + ((((elem >> 3) ^ (row >> 2)) & 3) << 3) + (elem & 7);
}

// n / d for 0 <= n < 2^31 by multiply-high (Granlund-Montgomery).
struct FastDiv {
  uint32_t d, m, l;
};
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
  return (__umulhi(n, f.m) + n) >> f.l;
}

// The work of one workgroup: output tile `tile` of problem `a` over pixel
// split `split` (the body of conv_wgrad_split_kernel and of its grouped form).
template <int TM, int TN>
__device__ __forceinline__ void wgrad_split_body(const WgradArgs& a, const FastDiv& fd_hw,
                                                 const FastDiv& fd_w, const int tile,
                                                 const int split) {
  constexpr int BM = 2 * TM * 32, BN = 2 * TN * 32;
  constexpr int GA = BM / 4, GB = BN / 4;  // 4-channel groups
  __shared__ __attribute__((aligned(16))) uint16_t As[3 * BM * LDW];
  __shared__ __attribute__((aligned(16))) uint16_t Bs[3 * BN * LDW];
  __shared__ float bred[8][BN];

  const int per_tap = a.nCi * a.nCo;
  const int tap = tile / per_tap;
  const int rem = tile - tap * per_tap;
  const int cit = rem / a.nCo, cot = rem - cit * a.nCo;
  const int kh = tap / a.KW, kw = tap - kh * a.KW;
  const int ci0 = cit * BM, co0 = cot * BN;
  const int c_begin = split * a.chunks_per_split;
  const int c_end = min(a.nchunks, c_begin + a.chunks_per_split);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int li = lane & 31, lh = lane >> 5;

  // A items: (cg, pg) = (tid % GA, tid / GA) for tid < 8 * GA; B likewise
  const bool a_on = tid < 8 * GA, b_on = tid < 8 * GB;
  const int cga = tid % GA, pga = tid / GA;
  const int cgb = tid % GB, pgb = tid / GB;
  const int ci = ci0 + 4 * cga, co = co0 + 4 * cgb;
  const bool ci_ok = a_on && ci < a.Cin, co_ok = b_on && co < a.Cout;

  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.dy), 0, a.dy_bytes, 0x00020000);
  constexpr uint32_t kOOB = 0x80000000u;

  float4 ra[4], rb[4];
  auto load_chunk = [&](int ch) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = ch * KP + 4 * pga + q;
      const uint32_t n = fdiv((uint32_t)p, fd_hw);
      const int r2 = p - (int)n * (a.OH * a.OW);
      const int oy = (int)fdiv((uint32_t)r2, fd_w), ox = r2 - oy * a.OW;
      const int iy = oy * a.stride - a.pad + kh, ix = ox * a.stride - a.pad + kw;
      const bool ok = ci_ok & (p < a.P) & ((unsigned)iy < (unsigned)a.H) &
                      ((unsigned)ix < (unsigned)a.W);
      const uint32_t off = ok ? (uint32_t)(((((int)n * a.H + iy) * a.W + ix) * a.Cin + ci) * 4) : kOOB;
      ra[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
      const int pb = ch * KP + 4 * pgb + q;
      const uint32_t offb = (co_ok & (pb < a.P)) ? (uint32_t)((pb * a.Cout + co) * 4) : kOOB;
      rb[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(yr, offb, 0, 0));
    }
  };
  const bool do_bias = a.dbias != nullptr && tap == 0 && cit == 0;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  auto store_chunk = [&]() {
    if (a_on) {
      const float* f = reinterpret_cast<const float*>(ra);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint2 h, m, l;
        split3(make_float4(f[j], f[4 + j], f[8 + j], f[12 + j]), h, m, l);
        const int o = wswz(4 * cga + j, 4 * pga);
        *reinterpret_cast<uint2*>(&As[o]) = h;
        *reinterpret_cast<uint2*>(&As[BM * LDW + o]) = m;
        *reinterpret_cast<uint2*>(&As[2 * BM * LDW + o]) = l;
      }
    }
    if (b_on) {
      const float* f = reinterpret_cast<const float*>(rb);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 v = make_float4(f[j], f[4 + j], f[8 + j], f[12 + j]);
        if (do_bias) bsum[j] += ((v.x + v.y) + v.z) + v.w;
        uint2 h, m, l;
        split3(v, h, m, l);
        const int o = wswz(4 * cgb + j, 4 * pgb);
        *reinterpret_cast<uint2*>(&Bs[o]) = h;
        *reinterpret_cast<uint2*>(&Bs[BN * LDW + o]) = m;
        *reinterpret_cast<uint2*>(&Bs[2 * BN * LDW + o]) = l;
      }
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (c_begin < c_end) {
    load_chunk(c_begin);
    for (int ch = c_begin; ch < c_end; ++ch) {
      store_chunk();
      __syncthreads();
      if (ch + 1 < c_end) load_chunk(ch + 1);
      if (a.prio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 fa[3][TM], fb[3][TN];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
          for (int i = 0; i < TM; ++i)
            fa[pl][i] = *reinterpret_cast<const bf16x8*>(
                &As[pl * BM * LDW + wswz((wr * TM + i) * 32 + li, ks * 16 + lh * 8)]);
#pragma unroll
          for (int j = 0; j < TN; ++j)
            fb[pl][j] = *reinterpret_cast<const bf16x8*>(
                &Bs[pl * BN * LDW + wswz((wc * TN + j) * 32 + li, ks * 16 + lh * 8)]);
        }
        constexpr int PAi[6] = {1, 2, 0, 0, 1, 0};
        constexpr int PBi[6] = {1, 0, 2, 1, 0, 0};
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[PAi[t]][i], fb[PBi[t]][j],
                                                                   acc[i][j], 0, 0, 0);
      }
      if (a.prio) __builtin_amdgcn_s_setprio(0);
      __syncthreads();
    }
  }

  if (do_bias) {  // fixed-order reduction over the 8 pixel groups
    if (b_on) {
#pragma unroll
      for (int j = 0; j < 4; ++j) bred[pgb][4 * cgb + j] = bsum[j];
    }
    __syncthreads();
    if (tid < BN && co0 + tid < a.Cout) {
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) s += bred[g][tid];
      if (a.part) a.pbias[(size_t)split * a.Cout + co0 + tid] = s;
      else a.dbias[co0 + tid] = s;
    }
  }

  const size_t wsz = (size_t)a.KH * a.KW * a.Cin * a.Cout;
  float* out = a.part ? a.partial + (size_t)split * wsz : a.dw;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int oc = co0 + (wc * TN + j) * 32 + li;
    if (oc >= a.Cout) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int cb = ci0 + (wr * TM + i) * 32 + 4 * lh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = cb + (r & 3) + 8 * (r >> 2);
        if (c < a.Cin) out[((size_t)tap * a.Cin + c) * a.Cout + oc] = acc[i][j][r];
      }
    }
  }
}

template <int TM, int TN, int OCC = 2>
__global__ __launch_bounds__(256, OCC) void conv_wgrad_split_kernel(WgradArgs a, FastDiv fd_hw,
                                                                    FastDiv fd_w) {
  int tile, split;
  wgrad_tile_split(a, tile, split);
  wgrad_split_body<TM, TN>(a, fd_hw, fd_w, tile, split);
}


// Warp-specialised split wgrad (the conv_ws_kernel structure of
// conv_mfma.hip for the weight gradient): a 256 (ci) x 128 (co) tile of one
// tap, 16 waves, one workgroup per CU.  Waves 0-7 compute (4 x 2 blocks of
// 64 x 64, ds_read + MFMA only); waves 8-15 stage: the 32-pixel chunks of X
// (shifted by the tap) and dY into registers two chunks ahead, transposed to
// [channel][pixel], split exactly into bf16 planes and written to one of two
// LDS stages; one barrier per chunk.  Stager threads 0-511 each own one
// (4-channel, 4-pixel) item of X; threads 256-511 also one item of dY (and
// its bias-gradient partial sums, reduced in the fixed order of the 128 x 128
// kernel).  Same pixel order, product order and accumulation sequence as
// conv_wgrad_split_kernel: bit-identical for equal pixel splits.
//
// LIST (d2mi_conv2d_wgrad_rows): the workgroup first compacts the chunks of
// its [c_begin, c_end) whose bit is set in a.bitmap into an ordered LDS list
// (ballots and a fixed-order prefix over the waves: no atomics), and stagers
// and compute waves walk that list instead of every chunk; the stagers seek
// each listed chunk by division (no incremental cursor).  A chunk that is not
// listed holds only zero dy rows: its products are +-0, added to accumulators
// that start at +0 and can never become -0, so for finite x the sums (and the
// bias sums) are bit-identical to the dense walk.  A split without a set
// chunk still writes its zero slab.
template <int LD, bool INC, bool LIST>
__device__ __forceinline__ void wgrad_ws_body(const WgradArgs& a, const FastDiv& fd_hw,
                                              const FastDiv& fd_w, const int tile,
                                              const int split) {
  static_assert(!(LIST && INC), "the listed chunks are not consecutive");
  constexpr int TM = 2, TN = 2, BM = 256, BN = 128, S = 2;
  constexpr int GA = BM / 4, GB = BN / 4;  // 4-channel groups
  constexpr int A_H = 3 * BM * LDW, B_H = 3 * BN * LDW;  // halfwords per stage
  constexpr int STAGE = A_H + B_H;                      // 36864 halfwords = 72 KiB
  __shared__ __attribute__((aligned(16))) uint16_t smem[S * STAGE];
  __shared__ float bred[8][BN];
  // LIST: the set chunks of this split, as offsets from c_begin, ascending
  __shared__ uint16_t clist[LIST ? kWgradListCap : 1];
  __shared__ int wcnt[LIST ? 17 : 1];

  const int per_tap = a.nCi * a.nCo;
  const int tap = tile / per_tap;
  const int rem = tile - tap * per_tap;
  const int cit = rem / a.nCo, cot = rem - cit * a.nCo;
  const int kh = tap / a.KW, kw = tap - kh * a.KW;
  const int ci0 = cit * BM, co0 = cot * BN;
  const int c_begin = split * a.chunks_per_split;
  const int c_end = min(a.nchunks, c_begin + a.chunks_per_split);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int nks = max(c_end - c_begin, 0);
  if constexpr (LIST) {
    // ordered compaction, 1024 chunks per pass (host: nks <= kWgradListCap)
    const int nall = nks;
    int base = 0;
    for (int i0 = 0; i0 < nall; i0 += 1024) {
      const int i = i0 + tid;
      bool set = false;
      if (i < nall) {
        const int ch = c_begin + i;
        set = (a.bitmap[ch >> 5] >> (ch & 31)) & 1u;
      }
      const unsigned long long b = __ballot(set);
      if (lane == 0) wcnt[wave] = __popcll(b);
      __syncthreads();
      int before = base;
      for (int w = 0; w < 16; ++w) {
        const int c = wcnt[w];
        before += w < wave ? c : 0;
        base += c;
      }
      if (set) clist[before + __popcll(b & ((1ull << lane) - 1ull))] = (uint16_t)i;
      __syncthreads();
    }
    nks = __builtin_amdgcn_readfirstlane(base);
  }
  const int wr = wave >> 1, wc = wave & 1;  // compute waves 0-7: 4 x 2
  const int li = lane & 31, lh = lane >> 5;
  const bool do_bias = a.dbias != nullptr && tap == 0 && cit == 0;

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (wave >= 8) {
    // ------------------------------------------------------------ stagers
    const int st = tid - 512;
    const int cga = st % GA, pga = st / GA;             // X item (all 512)
    const bool b_on = st >= 256;                        // dY item (threads 256-511)
    const int sb = st - 256;
    const int cgb = (b_on ? sb : 0) % GB, pgb = (b_on ? sb : 0) / GB;
    const int ci = ci0 + 4 * cga, co = co0 + 4 * cgb;
    const bool ci_ok = ci < a.Cin, co_ok = b_on && co < a.Cout;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.dy), 0, a.dy_bytes, 0x00020000);
    constexpr uint32_t kOOB = 0x80000000u;
    float4 ra[LD][4], rb[LD][4];
    // The loads walk the split's chunks in order (then the last one again).
    // INC (same-size stride-1 convs: the 3x3 / 1x1 this kernel takes, see
    // the launch): input pixel = output pixel + a uniform tap shift, so a
    // per-thread (oy, ox) cursor of its first pixel, advanced by 32 pixels
    // per chunk, gives the range test, and 24-bit multiplies the offsets --
    // two fast divisions and four 32-bit multiplies per pixel fewer.  Else
    // per-pixel division.  dY offsets advance by one uniform stride.  Same
    // addresses either way.
    const int clast = c_begin + max(nks, 1) - 1;
    int c_ch = c_begin;
    // LIST: position in the list of the chunk to load next (then the last again)
    const int jlast = max(nks, 1) - 1;
    int j_ld = 0;
    const int c_first = (LIST && nks > 0) ? c_begin + clist[0] : c_begin;
    int p0 = c_first * KP + 4 * pga;   // first of this thread's 4 X pixels
    int pb0 = c_first * KP + 4 * pgb;  // (dY)
    int oy0 = 0, ox0 = 0;
    if (INC) {
      const int r2 = p0 - (int)fdiv((uint32_t)p0, fd_hw) * (a.OH * a.OW);
      oy0 = (int)fdiv((uint32_t)r2, fd_w);
      ox0 = r2 - oy0 * a.OW;
    }
    const int dy32 = KP / a.OW, dx32 = KP - (KP / a.OW) * a.OW;  // (uniform)
    const int ybase = kh - a.pad, xbase = kw - a.pad;
    const int tsh = ybase * a.W + xbase;  // INC: input pixel - output pixel
    const uint32_t bstride = (uint32_t)KP * (uint32_t)a.Cout * 4u;
    uint32_t boff = (uint32_t)(pb0 * a.Cout + co) * 4u;
    auto load = [&](float4 (&la)[4], float4 (&lb)[4]) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int p = p0 + q;
        uint32_t off;
        if (INC) {
          int ox = ox0 + q, oy = oy0;
          const bool wrap = ox >= a.OW;
          ox = wrap ? ox - a.OW : ox;
          oy = wrap ? oy + 1 : oy;
          oy = oy >= a.OH ? oy - a.OH : oy;
          const bool ok = ci_ok & (p < a.P) & ((unsigned)(oy + ybase) < (unsigned)a.H) &
                          ((unsigned)(ox + xbase) < (unsigned)a.W);
          off = ok ? (__umul24((uint32_t)(p + tsh), (uint32_t)a.Cin) + (uint32_t)ci) * 4u : kOOB;
        } else {
          const int n = (int)fdiv((uint32_t)p, fd_hw);
          const int r2 = p - n * (a.OH * a.OW);
          const int oy = (int)fdiv((uint32_t)r2, fd_w), ox = r2 - oy * a.OW;
          const int iy = oy * a.stride - a.pad + kh, ix = ox * a.stride - a.pad + kw;
          const bool ok = ci_ok & (p < a.P) & ((unsigned)iy < (unsigned)a.H) &
                          ((unsigned)ix < (unsigned)a.W);
          off = ok ? (uint32_t)(((((int)n * a.H + iy) * a.W + ix) * a.Cin + ci) * 4) : kOOB;
        }
        la[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
        const uint32_t offb = (co_ok & (pb0 + q < a.P)) ? boff + (uint32_t)(q * a.Cout * 4) : kOOB;
        lb[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(yr, offb, 0, 0));
      }
      if constexpr (LIST) {
        if (j_ld < jlast) {  // seek the next listed chunk (uniform condition)
          ++j_ld;
          const int ch = c_begin + clist[j_ld];
          p0 = ch * KP + 4 * pga;
          pb0 = ch * KP + 4 * pgb;
          boff = (uint32_t)(pb0 * a.Cout + co) * 4u;
        }
      } else if (c_ch < clast) {  // advance to the next chunk (uniform condition)
        ++c_ch;
        p0 += KP;
        pb0 += KP;
        boff += bstride;
        if (INC) {
          ox0 += dx32;
          oy0 += dy32;
          const bool wrap = ox0 >= a.OW;
          ox0 = wrap ? ox0 - a.OW : ox0;
          oy0 = wrap ? oy0 + 1 : oy0;
          oy0 = oy0 >= a.OH ? oy0 - a.OH : oy0;
        }
      }
    };
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    auto write = [&](int buf, const float4 (&la)[4], const float4 (&lb)[4]) {
      uint16_t* As = smem + buf * STAGE;
      uint16_t* Bs = As + A_H;
      const float* f = reinterpret_cast<const float*>(la);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint2 h, m, l;
        split3(make_float4(f[j], f[4 + j], f[8 + j], f[12 + j]), h, m, l);
        const int o = wswz(4 * cga + j, 4 * pga);
        *reinterpret_cast<uint2*>(&As[o]) = h;
        *reinterpret_cast<uint2*>(&As[BM * LDW + o]) = m;
        *reinterpret_cast<uint2*>(&As[2 * BM * LDW + o]) = l;
      }
      if (b_on) {
        const float* g = reinterpret_cast<const float*>(lb);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 v = make_float4(g[j], g[4 + j], g[8 + j], g[12 + j]);
          if (do_bias) bsum[j] += ((v.x + v.y) + v.z) + v.w;
          uint2 h, m, l;
          split3(v, h, m, l);
          const int o = wswz(4 * cgb + j, 4 * pgb);
          *reinterpret_cast<uint2*>(&Bs[o]) = h;
          *reinterpret_cast<uint2*>(&Bs[BN * LDW + o]) = m;
          *reinterpret_cast<uint2*>(&Bs[2 * BN * LDW + o]) = l;
        }
      }
    };
    // unconditional loads (chunks past the end re-load the last one): hipcc
    // then counts the loads in flight instead of draining them
#pragma unroll
    for (int j = 0; j < LD; ++j) load(ra[j], rb[j]);
    if (nks > 0) write(0, ra[0], rb[0]);
    load(ra[0], rb[0]);
    __syncthreads();  // B_{-1}
    int u0 = 0;
    for (; u0 + LD <= nks; u0 += LD) {
#pragma unroll
      for (int j = 0; j < LD; ++j) {
        const int v = u0 + j + 1;
        const int set = (j + 1) % LD;
        if (v < nks) write(v & 1, ra[set], rb[set]);
        load(ra[set], rb[set]);  // chunk v + LD (clamped)
        __syncthreads();  // B_u
      }
    }
#pragma unroll
    for (int j = 0; j < LD - 1; ++j) {
      if (u0 + j < nks) {
        const int v = u0 + j + 1;
        const int set = (j + 1) % LD;
        if (v < nks) write(v & 1, ra[set], rb[set]);
        __syncthreads();
      }
    }
    if (do_bias && b_on) {
#pragma unroll
      for (int j = 0; j < 4; ++j) bred[pgb][4 * cgb + j] = bsum[j];
    }
  } else {
    // ------------------------------------------------------------ compute
    bf16x8 fa[3][TM], fb[3][TN];
    auto ld1 = [&](const uint16_t* As, const uint16_t* Bs, int pa, int pb, int ks) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
        fa[pa][i] = *reinterpret_cast<const bf16x8*>(
            &As[pa * BM * LDW + wswz((wr * TM + i) * 32 + li, ks * 16 + lh * 8)]);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        fb[pb][j] = *reinterpret_cast<const bf16x8*>(
            &Bs[pb * BN * LDW + wswz((wc * TN + j) * 32 + li, ks * 16 + lh * 8)]);
    };
    auto mm1 = [&](int pa, int pb) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] =
              __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[pa][i], fb[pb][j], acc[i][j], 0, 0, 0);
    };
    // products in the split kernel's order {mm, lh, hl, hm, mh, hh}, reads in
    // three plane batches one MFMA group ahead of their first use
    auto step16 = [&](const uint16_t* As, const uint16_t* Bs, int ks) {
      ld1(As, Bs, 1, 1, ks);
      __builtin_amdgcn_sched_barrier(0);
      ld1(As, Bs, 2, 0, ks);
      mm1(1, 1);
      __builtin_amdgcn_sched_barrier(0);
      ld1(As, Bs, 0, 2, ks);
      mm1(2, 0);
      __builtin_amdgcn_sched_barrier(0);
      mm1(0, 2);
      mm1(0, 1);
      mm1(1, 0);
      mm1(0, 0);
    };
    __syncthreads();  // B_{-1}
    for (int u = 0; u < nks; ++u) {
      const uint16_t* As = smem + (u & 1) * STAGE;
      const uint16_t* Bs = As + A_H;
      if (a.prio) __builtin_amdgcn_s_setprio(1);
      step16(As, Bs, 0);
      step16(As, Bs, 1);
      if (a.prio) __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();  // B_u
    }
  }
  if (do_bias) {  // fixed-order reduction over the 8 pixel groups
    __syncthreads();
    if (tid < BN && co0 + tid < a.Cout) {
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) s += bred[g][tid];
      if (a.part) a.pbias[(size_t)split * a.Cout + co0 + tid] = s;
      else a.dbias[co0 + tid] = s;
    }
  }
  if (wave >= 8) return;
  const size_t wsz = (size_t)a.KH * a.KW * a.Cin * a.Cout;
  float* out = a.part ? a.partial + (size_t)split * wsz : a.dw;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int oc = co0 + (wc * TN + j) * 32 + li;
    if (oc >= a.Cout) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int cb = ci0 + (wr * TM + i) * 32 + 4 * lh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = cb + (r & 3) + 8 * (r >> 2);
        if (c < a.Cin) out[((size_t)tap * a.Cin + c) * a.Cout + oc] = acc[i][j][r];
      }
    }
  }
}

template <int LD, bool INC = false, bool LIST = false>
__global__ __launch_bounds__(1024, 1) void conv_wgrad_ws_kernel(WgradArgs a, FastDiv fd_hw,
                                                                FastDiv fd_w) {
  int tile, split;
  wgrad_tile_split(a, tile, split);
  wgrad_ws_body<LD, INC, LIST>(a, fd_hw, fd_w, tile, split);
}

// ---------------------------------------------------------------------------
// Grouped forms (d2mi_conv2d_wgrad_group): the problems of one kernel family
// in one grid.  The launch reads a device table: the first workgroup of each
// problem (ascending), then one WgradGroupEntry per problem.  Logical order:
// the problems concatenated, split-major, tile fastest, and the linear
// workgroup id remapped XCD-contiguously over the whole grid as
// wgrad_tile_split does for one problem -- the tiles of one problem's pixel
// range stay on one XCD.  The problem is found by a wave-uniform binary search
// of the prefix and its arguments are read through uniform loads; the work is
// the single launch's body, so equal splits give equal bits.
struct WgradGroupEntry {
  WgradArgs a;
  FastDiv fd_hw, fd_w;
};
struct WgradGroupTable {
  int wg0[kMaxWgradGroup];  // [n] first workgroup of each problem
  WgradGroupEntry e[1];     // [n]
};

__device__ __forceinline__ int wgrad_group_locate(const WgradGroupTable* __restrict__ t, int n,
                                                  int nwg, int xcd, int& local) {
  const int L = blockIdx.x;
  int l = L;
  if (xcd) {
    const int q = nwg / 8, r8 = nwg % 8, x8 = L % 8;
    l = (x8 < r8 ? x8 * (q + 1) : r8 * (q + 1) + (x8 - r8) * q) + L / 8;
  }
  int lo = 0, hi = n;  // the last problem whose first workgroup is <= l
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t->wg0[mid] <= l) lo = mid;
    else hi = mid;
  }
  lo = __builtin_amdgcn_readfirstlane(lo);
  local = l - t->wg0[lo];
  return lo;
}

template <int TM, int TN, int OCC = 2>
__global__ __launch_bounds__(256, OCC) void conv_wgrad_split_group_kernel(
    const WgradGroupTable* __restrict__ t, int n, int nwg, int xcd) {
  int local;
  const int i = wgrad_group_locate(t, n, nwg, xcd, local);
  const WgradGroupEntry& e = t->e[i];
  const int split = local / e.a.ntiles;
  wgrad_split_body<TM, TN>(e.a, e.fd_hw, e.fd_w, local - split * e.a.ntiles, split);
}

template <int LD, bool INC>
__global__ __launch_bounds__(1024, 1) void conv_wgrad_ws_group_kernel(
    const WgradGroupTable* __restrict__ t, int n, int nwg, int xcd) {
  int local;
  const int i = wgrad_group_locate(t, n, nwg, xcd, local);
  const WgradGroupEntry& e = t->e[i];
  const int split = local / e.a.ntiles;
  wgrad_ws_body<LD, INC, false>(e.a, e.fd_hw, e.fd_w, local - split * e.a.ntiles, split);
}

// The reduce of one family's slabs: a flat index over the float4s of every
// problem's dw, each followed by its Cout bias elements (items [item0[i],
// item0[i + 1]) are problem i's).  Splits are summed in ascending order from
// 0.f, as wgrad_reduce4_kernel and wgrad_reduce_kernel do; a dw that is not
// 16-B aligned (a view into a gradient bucket) gets the same sums by four
// scalar stores.
struct WgradReduceEntry {
  const float* partial;  // [splits][4 * total4]
  const float* pbias;    // [splits][Cout]
  float* dw;
  float* dbias;  // nullable
  int splits, total4, Cout, pad_;
};
struct WgradReduceTable {
  int item0[kMaxWgradGroup + 1];  // [n + 1]
  int pad_;
  WgradReduceEntry e[1];  // [n]
};
__global__ void wgrad_group_reduce4_kernel(const WgradReduceTable* __restrict__ t, int n) {
  const int total = t->item0[n];
  for (int it = blockIdx.x * blockDim.x + threadIdx.x; it < total; it += gridDim.x * blockDim.x) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (t->item0[mid] <= it) lo = mid;
      else hi = mid;
    }
    const WgradReduceEntry& e = t->e[lo];
    const int j = it - t->item0[lo];
    const int splits = e.splits, total4 = e.total4;
    if (j < total4) {
      const float4* __restrict__ partial = reinterpret_cast<const float4*>(e.partial);
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
      for (int k = 0; k < splits; ++k) {
        const float4 v = partial[(size_t)k * total4 + j];
        s.x += v.x;
        s.y += v.y;
        s.z += v.z;
        s.w += v.w;
      }
      float* dw = e.dw + 4 * (size_t)j;
      if (((uintptr_t)e.dw & 15) == 0) {
        *reinterpret_cast<float4*>(dw) = s;
      } else {
        dw[0] = s.x;
        dw[1] = s.y;
        dw[2] = s.z;
        dw[3] = s.w;
      }
    } else if (e.dbias != nullptr) {
      const int c = j - total4;
      float s = 0.f;
#pragma unroll 8  // (loads in flight; the sum stays in split order)
      for (int k = 0; k < splits; ++k) s += e.pbias[(size_t)k * e.Cout + c];
      e.dbias[c] = s;
    }
  }
}

FastDiv make_fastdiv(uint32_t d) {
  FastDiv f;
  f.d = d;
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  f.l = l;
  f.m = (uint32_t)((((1ull << 32) * ((1ull << l) - d)) / d) + 1);
  return f;
}

}  // namespace
}  // namespace d2mi

using namespace d2mi;

extern "C" size_t d2mi_conv2d_wgrad_workspace_size(int N, int H, int W, int Cin, int Cout, int KH,
                                                   int KW, int stride, int pad_beg, int pad_end) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0)
    return 0;
  // the larger of the split-product and the f32 plans (either math mode fits)
  const ConvShape s = {N, H, W, Cin, Cout, KH, KW, stride, pad_beg, pad_end};
  WgradPlan split, f32;
  if (plan_wgrad(s, kPlanSplit3, kOpAllAligned | kOpWorkspace, SIZE_MAX, &split) ||
      plan_wgrad(s, 0, kOpAllAligned | kOpWorkspace, SIZE_MAX, &f32))
    return 0;
  return std::max(split.ws_bytes, f32.ws_bytes);
}

// The checks of d2mi_conv2d_wgrad_ex that need no pointer, then its plan.
static int wgrad_plan_checked(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                              int pad_beg, int pad_end, int flags, int operands,
                              size_t workspace_bytes, WgradPlan* p) {
  D2MI_REQUIRE((flags & ~12) == 0,
               "wgrad flags: bit2 = split-bf16 products, bit3 = accumulate into dw / dbias");
  D2MI_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && stride > 0,
               "bad conv shape");
  D2MI_REQUIRE(Cin % 4 == 0 && Cout % 4 == 0, "Cin and Cout must be multiples of 4 (%d, %d)",
               Cin, Cout);
  int OH, OW;
  D2MI_REQUIRE(conv_dims(H, W, KH, KW, stride, pad_beg, pad_end, OH, OW) == 0,
               "conv output is empty");
  D2MI_REQUIRE((long long)N * OH * OW < (1LL << 31), "too many pixels");
  if (flags & kPlanSplit3)
    D2MI_REQUIRE((int64_t)N * H * W * Cin * 4 < (1ll << 31) &&
                     (int64_t)N * OH * OW * Cout * 4 < (1ll << 31),
                 "split wgrad: x and dy must each be < 2 GiB");
  plan_wgrad({N, H, W, Cin, Cout, KH, KW, stride, pad_beg, pad_end}, flags, operands,
             workspace_bytes, p);
  if (flags & kPlanAccum)  // the sum goes through the reduce, which adds it: one slab at least
    D2MI_REQUIRE((operands & kOpWorkspace) && workspace_bytes >= p->ws_bytes,
                 "accumulating wgrad: workspace must hold %d slab(s)", p->splits);
  return 0;
}

// The plan as integers (include/d2mi.h lists the fields).
extern "C" int d2mi_conv2d_wgrad_plan(int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                      int stride, int pad_beg, int pad_end, int flags,
                                      int operands, size_t workspace_bytes, int32_t* out,
                                      int out_len) {
  D2MI_REQUIRE((operands & ~127) == 0, "wgrad plan: unknown operand bits");
  WgradPlan p;
  if (wgrad_plan_checked(N, H, W, Cin, Cout, KH, KW, stride, pad_beg, pad_end, flags, operands,
                         workspace_bytes, &p))
    return -1;
  const int32_t v[] = {p.kernel, p.TM, p.TN, p.BM, p.BN, p.nCi, p.nCo, p.ntiles, p.nchunks,
                       p.splits, p.chunks_per_split, p.part, p.reduce, p.reduce_grid,
                       (int32_t)(p.ws_bytes & 0x7fffffff), (int32_t)(p.ws_bytes >> 31)};
  return emit_plan(v, (int)(sizeof(v) / sizeof(v[0])), out, out_len);
}

// The kernel arguments of one problem under plan p (partial / pbias: its slabs
// when p.part).
static WgradArgs wgrad_args(const float* x, const float* dy, float* dw, float* dbias,
                            const ConvShape& s, const WgradPlan& p, float* partial,
                            float* pbias) {
  WgradArgs a = {};
  a.prio = tuning(kTuneWgradPrio);
  a.xcd = tuning(kTuneWgradXCD) > 0 ? 1 : 0;
  a.x = x;
  a.dy = dy;
  a.dw = dw;
  a.dbias = dbias;
  a.N = s.N;
  a.H = s.H;
  a.W = s.W;
  a.Cin = s.Cin;
  a.Cout = s.Cout;
  a.KH = s.KH;
  a.KW = s.KW;
  a.stride = s.stride;
  a.pad = s.pad_beg;
  a.OH = p.OH;
  a.OW = p.OW;
  a.P = s.N * a.OH * a.OW;
  a.nCi = p.nCi;
  a.nCo = p.nCo;
  a.ntiles = p.ntiles;
  a.splits = p.splits;
  a.chunks_per_split = p.chunks_per_split;
  a.nchunks = p.nchunks;
  a.part = p.part;
  a.partial = partial;
  a.pbias = pbias;
  if (p.kernel != kWgradF32) {
    a.x_bytes = (int)((int64_t)s.N * s.H * s.W * s.Cin * 4);
    a.dy_bytes = (int)((int64_t)a.P * s.Cout * 4);
  }
  return a;
}

// d2mi_conv2d_wgrad_ex, and with a chunk bitmap d2mi_conv2d_wgrad_rows: the
// same plan either way.  Returns 1 when the bitmap kernel ran, 0 after the
// dense launch (kernels other than the warp-specialised one ignore the
// bitmap, and so does a split of more than kWgradListCap chunks).
static int wgrad_launch(const float* x, const float* dy, float* dw_hwio, float* dbias, int N,
                        int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad_beg,
                        int pad_end, int flags, const uint32_t* bitmap, void* workspace,
                        size_t workspace_bytes, void* stream) {
  auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  WgradPlan p;
  if (wgrad_plan_checked(N, H, W, Cin, Cout, KH, KW, stride, pad_beg, pad_end, flags,
                         (al16(dw_hwio) ? kOpAligned : 0) | (workspace ? kOpWorkspace : 0) |
                             (al16(workspace) ? kOpWsAligned : 0),
                         workspace_bytes, &p))
    return -1;
  D2MI_REQUIRE(al16(x) && al16(dy), "x and dy must be 16-byte aligned");
  WgradSpace sp = {};
  if (p.part) {
    Workspace carve(workspace, workspace_bytes);
    sp.lay(carve, p.splits, (size_t)KH * KW * Cin * Cout, Cout);
  }
  WgradArgs a = wgrad_args(x, dy, dw_hwio, dbias,
                           {N, H, W, Cin, Cout, KH, KW, stride, pad_beg, pad_end}, p, sp.dw,
                           sp.dbias);
  hipStream_t st = as_stream(stream);
  const dim3 grid(p.ntiles, p.splits);
  const FastDiv fhw = make_fastdiv((uint32_t)(a.OH * a.OW)), fw = make_fastdiv((uint32_t)a.OW);
  const int tm = p.TM, tn = p.TN;
  const bool listed = bitmap != nullptr && p.chunks_per_split <= kWgradListCap &&
                      (p.kernel == kWgradWSInc || p.kernel == kWgradWS);
  a.bitmap = listed ? bitmap : nullptr;
  if (listed)
    hipLaunchKernelGGL((conv_wgrad_ws_kernel<1, false, true>), grid, dim3(1024), 0, st, a, fhw, fw);
  else if (p.kernel == kWgradWSInc)
    hipLaunchKernelGGL((conv_wgrad_ws_kernel<1, true>), grid, dim3(1024), 0, st, a, fhw, fw);
  else if (p.kernel == kWgradWS)
    hipLaunchKernelGGL((conv_wgrad_ws_kernel<1>), grid, dim3(1024), 0, st, a, fhw, fw);
  else if (p.kernel == kWgradSplitOcc3)
    hipLaunchKernelGGL((conv_wgrad_split_kernel<2, 2, 3>), grid, dim3(256), 0, st, a, fhw, fw);
  else if (p.kernel == kWgradSplit && tm == 2 && tn == 2)
    hipLaunchKernelGGL((conv_wgrad_split_kernel<2, 2>), grid, dim3(256), 0, st, a, fhw, fw);
  else if (p.kernel == kWgradSplit && tm == 2)
    hipLaunchKernelGGL((conv_wgrad_split_kernel<2, 1>), grid, dim3(256), 0, st, a, fhw, fw);
  else if (p.kernel == kWgradSplit && tn == 2)
    hipLaunchKernelGGL((conv_wgrad_split_kernel<1, 2>), grid, dim3(256), 0, st, a, fhw, fw);
  else if (p.kernel == kWgradSplit)
    hipLaunchKernelGGL((conv_wgrad_split_kernel<1, 1>), grid, dim3(256), 0, st, a, fhw, fw);
  else if (tm == 2 && tn == 2)
    hipLaunchKernelGGL((conv_wgrad_kernel<2, 2>), grid, dim3(256), 0, st, a);
  else if (tm == 2)
    hipLaunchKernelGGL((conv_wgrad_kernel<2, 1>), grid, dim3(256), 0, st, a);
  else if (tn == 2)
    hipLaunchKernelGGL((conv_wgrad_kernel<1, 2>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((conv_wgrad_kernel<1, 1>), grid, dim3(256), 0, st, a);
  D2MI_LAUNCH_CHECK();
  if (p.reduce == kReduceNone) return listed ? 1 : 0;
  const size_t total = (size_t)KH * KW * Cin * Cout;
  const int accum = (flags & kPlanAccum) != 0;
  if (p.reduce == kReduceFloat4)
    hipLaunchKernelGGL(wgrad_reduce4_kernel, dim3(p.reduce_grid), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(a.partial), a.splits, total / 4,
                       reinterpret_cast<float4*>(dw_hwio), a.pbias, Cout, dbias, accum);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(p.reduce_grid), dim3(256), 0, st, a.partial,
                       a.splits, total, dw_hwio, a.pbias, Cout, dbias, accum);
  D2MI_LAUNCH_CHECK();
  return listed ? 1 : 0;
}

extern "C" int d2mi_conv2d_wgrad_ex(const float* x, const float* dy, float* dw_hwio,
                                    float* dbias, int N, int H, int W, int Cin, int Cout, int KH,
                                    int KW, int stride, int pad_beg, int pad_end, int flags,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  return wgrad_launch(x, dy, dw_hwio, dbias, N, H, W, Cin, Cout, KH, KW, stride, pad_beg, pad_end,
                      flags, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int d2mi_conv2d_wgrad_rows(const float* x, const float* dy, float* dw_hwio,
                                      float* dbias, int N, int H, int W, int Cin, int Cout, int KH,
                                      int KW, int stride, int pad_beg, int pad_end, int flags,
                                      const void* census, size_t census_bytes, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  int OH, OW;
  D2MI_REQUIRE(N > 0 && H > 0 && W > 0 && KH > 0 && KW > 0 && stride > 0 &&
                   conv_dims(H, W, KH, KW, stride, pad_beg, pad_end, OH, OW) == 0 &&
                   (long long)N * OH * OW < (1LL << 31),
               "bad conv shape");
  // the census of dy's N x OH x OW pixel rows, as d2mi_row_census laid it out
  RowCensusSpace cs;
  Workspace carve(const_cast<void*>(census), census_bytes);
  cs.lay(carve, N * OH * OW, 0);  // (the head of the layout: no list needed here)
  D2MI_REQUIRE(census != nullptr && carve.ok(), "row census workspace too small (%zu < %zu)",
               census_bytes, carve.off);
  D2MI_REQUIRE(((uintptr_t)census & 3) == 0, "the row census must be 4-byte aligned");
  return wgrad_launch(x, dy, dw_hwio, dbias, N, H, W, Cin, Cout, KH, KW, stride, pad_beg, pad_end,
                      flags, cs.bitmap, workspace, workspace_bytes, stream);
}


extern "C" int d2mi_conv2d_wgrad(const float* x, const float* dy, float* dw_hwio, float* dbias,
                                 int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                 int stride, int pad_beg, int pad_end, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return d2mi_conv2d_wgrad_ex(x, dy, dw_hwio, dbias, N, H, W, Cin, Cout, KH, KW, stride,
                              pad_beg, pad_end, 0, workspace, workspace_bytes, stream);
}

// ---- grouped weight gradients
namespace {

struct WgradProblem {  // the host array of d2mi_conv2d_wgrad_group (include/d2mi.h)
  const float* x;
  const float* dy;
  float* dw;
  float* dbias;
  int32_t N, H, W, Cin, Cout, KH, KW, stride, pad_beg, pad_end;
};
static_assert(sizeof(WgradProblem) == 72, "d2mi_conv2d_wgrad_group: problem layout");

// The most workspace d2mi_conv2d_wgrad_group_workspace_size asks for.
constexpr size_t kWgradGroupMaxWorkspace = (size_t)1 << 30;

// The device table: per family the launch's table, then its reduce's.
struct WgradGroupLayout {
  size_t launch[kWgradFamilies], reduce[kWgradFamilies], bytes;
  explicit WgradGroupLayout(const int* count) {
    size_t off = 0;
    for (int f = 0; f < kWgradFamilies; ++f) {
      launch[f] = off;
      if (count[f]) off = align_up(off + offsetof(WgradGroupTable, e) + count[f] * sizeof(WgradGroupEntry), 16);
      reduce[f] = off;
      if (count[f]) off = align_up(off + offsetof(WgradReduceTable, e) + count[f] * sizeof(WgradReduceEntry), 16);
    }
    bytes = off;
  }
};
size_t wgrad_group_table_bytes(int n) {
  // every family non-empty, n entries in all, and the 16-B rounding of each block
  return kWgradFamilies * (offsetof(WgradGroupTable, e) + offsetof(WgradReduceTable, e) + 32) +
         (size_t)n * (sizeof(WgradGroupEntry) + sizeof(WgradReduceEntry));
}

ConvShape shape_of(const WgradProblem& q) {
  return {q.N, q.H, q.W, q.Cin, q.Cout, q.KH, q.KW, q.stride, q.pad_beg, q.pad_end};
}

int wgrad_group_cus() {
  int dev = 0, c = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) {
    (void)hipGetLastError();
    return 256;  // (plan queries without a GPU)
  }
  return c;
}

// The checks of every problem that need no pointer, then the group's plan.
int wgrad_group_plan_checked(const WgradProblem* q, int n, int flags, int operands,
                             size_t workspace_bytes, WgradGroupPlan* g) {
  D2MI_REQUIRE(q != nullptr && n > 0 && n <= kMaxWgradGroup,
               "wgrad group: 1..%d problems (got %d)", kMaxWgradGroup, n);
  D2MI_REQUIRE((flags & ~4) == 0, "wgrad group flags: bit2 = split-bf16 products");
  ConvShape shapes[kMaxWgradGroup];
  WgradPlan p;
  for (int i = 0; i < n; ++i) {
    if (wgrad_plan_checked(q[i].N, q[i].H, q[i].W, q[i].Cin, q[i].Cout, q[i].KH, q[i].KW,
                           q[i].stride, q[i].pad_beg, q[i].pad_end, flags, 0, 0, &p))
      return -1;
    shapes[i] = shape_of(q[i]);
  }
  static const int cus = wgrad_group_cus();
  D2MI_REQUIRE(plan_wgrad_group(shapes, n, flags, operands, workspace_bytes, cus, g) == 0,
               "wgrad group: no plan");
  return 0;
}

int wgrad_group_operands(const void* workspace) {
  return (workspace ? kOpWorkspace : 0) | (((uintptr_t)workspace & 15) == 0 ? kOpWsAligned : 0);
}

template <typename K>
void launch_group(K kernel, int threads, const WgradGroupFamily& F, const void* table, int xcd,
                  hipStream_t st) {
  hipLaunchKernelGGL(kernel, dim3(F.nwg), dim3(threads), 0, st,
                     reinterpret_cast<const WgradGroupTable*>(table), F.count, F.nwg, xcd);
}

}  // namespace

extern "C" size_t d2mi_conv2d_wgrad_group_table_size(int n) {
  return n > 0 && n <= kMaxWgradGroup ? wgrad_group_table_bytes(n) : 0;
}

extern "C" size_t d2mi_conv2d_wgrad_group_workspace_size(const void* problems, int n, int flags) {
  const WgradProblem* q = reinterpret_cast<const WgradProblem*>(problems);
  WgradGroupPlan g;
  // (asked for at most kWgradGroupMaxWorkspace: a group whose slabs need more
  // -- every problem's at once, under the default -- runs as single launches)
  if (wgrad_group_plan_checked(q, n, flags, kOpWorkspace | kOpWsAligned, kWgradGroupMaxWorkspace,
                               &g))
    return 0;
  // the group's slabs, or the largest of the problems that run alone
  size_t bytes = g.grouped ? g.ws_bytes : 0;
  for (int i = 0; i < n; ++i)
    if (!g.grouped || g.family[i] == kWgradFamNone)
      bytes = std::max(bytes, d2mi_conv2d_wgrad_workspace_size(q[i].N, q[i].H, q[i].W, q[i].Cin,
                                                               q[i].Cout, q[i].KH, q[i].KW,
                                                               q[i].stride, q[i].pad_beg,
                                                               q[i].pad_end));
  return bytes;
}

extern "C" int d2mi_conv2d_wgrad_group_plan(const void* problems, int n, int flags, int operands,
                                            size_t workspace_bytes, int32_t* out, int out_len) {
  D2MI_REQUIRE((operands & ~127) == 0, "wgrad group plan: unknown operand bits");
  WgradGroupPlan g;
  if (wgrad_group_plan_checked(reinterpret_cast<const WgradProblem*>(problems), n, flags,
                               operands, workspace_bytes, &g))
    return -1;
  int32_t v[2 + 6 * kWgradFamilies + 9 * kMaxWgradGroup + 2];
  int k = 0;
  v[k++] = g.grouped;
  v[k++] = n;
  for (int f = 0; f < kWgradFamilies; ++f) {
    const WgradGroupFamily& F = g.fam[f];
    const int32_t fv[] = {F.count, F.nwg, F.chunks_per_split, F.reduce_problems, F.reduce_grid, 0};
    for (int32_t x : fv) v[k++] = g.grouped ? x : 0;
  }
  size_t ws = g.grouped ? g.ws_bytes : 0;
  for (int i = 0; i < n; ++i) {
    const WgradPlan& p = g.p[i];
    const size_t off = g.grouped && p.part ? g.slab_off[i] * 4 : 0;
    const int32_t pv[] = {g.grouped ? g.family[i] : kWgradFamNone, p.kernel, p.ntiles, p.nchunks,
                          p.splits, p.chunks_per_split, g.grouped ? g.wg0[i] : 0,
                          (int32_t)(off & 0x7fffffff), (int32_t)(off >> 31)};
    for (int32_t x : pv) v[k++] = x;
    if (!g.grouped) ws = std::max(ws, p.ws_bytes);
  }
  v[k++] = (int32_t)(ws & 0x7fffffff);
  v[k++] = (int32_t)(ws >> 31);
  return emit_plan(v, k, out, out_len);
}

extern "C" int d2mi_conv2d_wgrad_group_table(const void* problems, int n, int flags,
                                             void* workspace, size_t workspace_bytes,
                                             void* table_host, size_t table_bytes) {
  const WgradProblem* q = reinterpret_cast<const WgradProblem*>(problems);
  WgradGroupPlan g;
  if (wgrad_group_plan_checked(q, n, flags, wgrad_group_operands(workspace), workspace_bytes, &g))
    return -1;
  D2MI_REQUIRE(table_host != nullptr && table_bytes >= wgrad_group_table_bytes(n),
               "wgrad group table too small (%zu < %zu)", table_bytes, wgrad_group_table_bytes(n));
  std::fill_n(reinterpret_cast<char*>(table_host), table_bytes, (char)0);
  if (!g.grouped) return 0;  // every problem runs alone: no table is read
  int count[kWgradFamilies];
  for (int f = 0; f < kWgradFamilies; ++f) count[f] = g.fam[f].count;
  const WgradGroupLayout lay(count);
  char* base = reinterpret_cast<char*>(table_host);
  float* ws = reinterpret_cast<float*>(workspace);
  for (int f = 0; f < kWgradFamilies; ++f) {
    if (!count[f]) continue;
    WgradGroupTable* lt = reinterpret_cast<WgradGroupTable*>(base + lay.launch[f]);
    WgradReduceTable* rt = reinterpret_cast<WgradReduceTable*>(base + lay.reduce[f]);
    // the family's problems by first workgroup (the plan's shape order)
    int idx[kMaxWgradGroup], m = 0;
    for (int i = 0; i < n; ++i)
      if (g.family[i] == f) idx[m++] = i;
    std::sort(idx, idx + m, [&](int a, int b) { return g.wg0[a] < g.wg0[b]; });
    int r = 0;
    for (int k = 0; k < m; ++k) {
      const int i = idx[k];
      const WgradPlan& p = g.p[i];
      const size_t wsize = (size_t)q[i].KH * q[i].KW * q[i].Cin * q[i].Cout;
      float* partial = p.part ? ws + g.slab_off[i] : nullptr;
      float* pbias = p.part ? partial + (size_t)p.splits * wsize : nullptr;
      lt->wg0[k] = g.wg0[i];
      lt->e[k].a = wgrad_args(q[i].x, q[i].dy, q[i].dw, q[i].dbias, shape_of(q[i]), p, partial,
                              pbias);
      lt->e[k].fd_hw = make_fastdiv((uint32_t)(p.OH * p.OW));
      lt->e[k].fd_w = make_fastdiv((uint32_t)p.OW);
      if (!p.part) continue;
      rt->item0[r] = (int)g.item0[i];
      rt->e[r] = {partial, pbias, q[i].dw, q[i].dbias, p.splits, (int)(wsize / 4), q[i].Cout, 0};
      ++r;
    }
    rt->item0[r] = (int)g.fam[f].reduce_items;
  }
  return 0;
}

extern "C" int d2mi_conv2d_wgrad_group(const void* problems, int n, int flags,
                                       const void* table_dev, size_t table_bytes, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  const WgradProblem* q = reinterpret_cast<const WgradProblem*>(problems);
  WgradGroupPlan g;
  if (wgrad_group_plan_checked(q, n, flags, wgrad_group_operands(workspace), workspace_bytes, &g))
    return -1;
  for (int i = 0; i < n; ++i)
    D2MI_REQUIRE(q[i].x && q[i].dy && q[i].dw && ((uintptr_t)q[i].x & 15) == 0 &&
                     ((uintptr_t)q[i].dy & 15) == 0 && ((uintptr_t)q[i].dw & 3) == 0,
                 "wgrad group: problem %d: x and dy must be 16-byte aligned, dw given", i);
  auto alone = [&](int i) {
    return wgrad_launch(q[i].x, q[i].dy, q[i].dw, q[i].dbias, q[i].N, q[i].H, q[i].W, q[i].Cin,
                        q[i].Cout, q[i].KH, q[i].KW, q[i].stride, q[i].pad_beg, q[i].pad_end,
                        flags, nullptr, workspace, workspace_bytes, stream);
  };
  if (!g.grouped) {
    for (int i = 0; i < n; ++i)
      if (alone(i) < 0) return -1;
    return 0;
  }
  D2MI_REQUIRE(table_dev != nullptr && table_bytes >= wgrad_group_table_bytes(n) &&
                   ((uintptr_t)table_dev & 15) == 0,
               "wgrad group: the device table must hold %zu bytes, 16-byte aligned",
               wgrad_group_table_bytes(n));
  D2MI_REQUIRE(g.ws_bytes <= workspace_bytes, "wgrad group workspace too small (%zu < %zu)",
               workspace_bytes, g.ws_bytes);
  int count[kWgradFamilies];
  for (int f = 0; f < kWgradFamilies; ++f) count[f] = g.fam[f].count;
  const WgradGroupLayout lay(count);
  const char* base = reinterpret_cast<const char*>(table_dev);
  hipStream_t st = as_stream(stream);
  const int xcd = tuning(kTuneWgradXCD) > 0 ? 1 : 0;
  for (int f = 0; f < kWgradFamilies; ++f) {
    const WgradGroupFamily& F = g.fam[f];
    if (!F.count) continue;
    const void* lt = base + lay.launch[f];
    switch (f) {
      case kWgradFamWS: launch_group(conv_wgrad_ws_group_kernel<1, false>, 1024, F, lt, xcd, st); break;
      case kWgradFamWSInc: launch_group(conv_wgrad_ws_group_kernel<1, true>, 1024, F, lt, xcd, st); break;
      case kWgradFamSplit22: launch_group(conv_wgrad_split_group_kernel<2, 2>, 256, F, lt, xcd, st); break;
      case kWgradFamSplit21: launch_group(conv_wgrad_split_group_kernel<2, 1>, 256, F, lt, xcd, st); break;
      case kWgradFamSplit12: launch_group(conv_wgrad_split_group_kernel<1, 2>, 256, F, lt, xcd, st); break;
      case kWgradFamSplit11: launch_group(conv_wgrad_split_group_kernel<1, 1>, 256, F, lt, xcd, st); break;
      default: launch_group(conv_wgrad_split_group_kernel<2, 2, 3>, 256, F, lt, xcd, st); break;
    }
    D2MI_LAUNCH_CHECK();
    if (F.reduce_problems == 0) continue;
    hipLaunchKernelGGL(wgrad_group_reduce4_kernel, dim3(F.reduce_grid), dim3(256), 0, st,
                       reinterpret_cast<const WgradReduceTable*>(base + lay.reduce[f]),
                       F.reduce_problems);
    D2MI_LAUNCH_CHECK();
  }
  for (int i = 0; i < n; ++i)  // the f32 kernels: alone, after the slabs were reduced
    if (g.family[i] == kWgradFamNone && alone(i) < 0) return -1;
  return 0;
}
