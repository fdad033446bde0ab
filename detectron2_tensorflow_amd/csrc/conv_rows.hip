// Row census of a sparse gradient map G [M = N*H*W][C]: which 32-pixel chunks
// (kWgradKP, the weight gradient's k-step) hold a non-zero row, how many rows
// are non-zero, and -- on request -- the sorted list of the output rows of a
// KxK stride-1 conv over G whose window holds a non-zero row.  The RPN loss
// has a gradient on the sampled anchors only (at most RPN.BATCH_SIZE_PER_IMAGE
// per image), so the gradient that reaches the head's shared 3x3 conv is
// all-zero on more than 99 % of its rows: the weight gradient walks the set
// chunks only (d2mi_conv2d_wgrad_rows), the data gradient computes the listed
// rows only (d2mi_conv2d_nhwc_rows).
//
// "Non-zero" compares bits: any element with a non-zero magnitude field (NaN
// and Inf included) makes the row non-zero, -0.0 does not.  Everything is
// deterministic -- flags, a prefix sum, a compaction, no ordering by atomics:
//   1. row_census_kernel: one workgroup per bitmap word (32 chunks = 1024
//      rows) ballots its rows' flags: the word, its row count, the row bits;
//   2. row_dilate_kernel: an output row is listed iff a row of its window is
//      flagged (the conv's own pads: nothing crosses an image border or runs
//      from one image into the next); ballots and per-block counts again;
//   3. row_scan_kernel (one workgroup): the totals, the blocks' exclusive
//      prefix, and the declared bound's check (kErrRowBound);
//   4. row_compact_kernel: block prefix + ballot prefix = list position;
//      positions past the list's capacity are dropped (the count is clamped).
#include "common.h"
#include "conv_plan.h"
#include "internal.h"

namespace d2mi {
namespace {

constexpr int kRowsPerWord = 32 * kWgradKP;  // 1024 rows per bitmap word

__global__ __launch_bounds__(256) void row_census_kernel(const float4* __restrict__ g, int M,
                                                         int C4, uint32_t* __restrict__ bitmap,
                                                         int32_t* __restrict__ word_rows,
                                                         unsigned long long* __restrict__ rowbits) {
  __shared__ unsigned long long ballots[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int base = blockIdx.x * kRowsPerWord;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // wave w of pass k tests rows base + 256 k + 64 w .. + 63: chunks 8 k + 2 w, + 1
    const int row = base + 256 * k + tid;
    bool nz = false;
    if (row < M) {
      const float4* r = g + (size_t)row * C4;
      uint32_t any = 0;
      for (int c = 0; c < C4; ++c) {
        const float4 v = r[c];
        any |= __float_as_uint(v.x) | __float_as_uint(v.y) | __float_as_uint(v.z) |
               __float_as_uint(v.w);
      }
      nz = (any & 0x7fffffffu) != 0u;
    }
    const unsigned long long b = __ballot(nz);
    if (lane == 0) ballots[4 * k + wave] = b;
  }
  __syncthreads();
  if (rowbits != nullptr && tid < 16) rowbits[(size_t)blockIdx.x * 16 + tid] = ballots[tid];
  if (tid == 0) {
    uint32_t bits = 0;
    int rows = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const unsigned long long b = ballots[i];
      if ((uint32_t)b) bits |= 1u << (2 * i);
      if ((uint32_t)(b >> 32)) bits |= 1u << (2 * i + 1);
      rows += __popcll(b);
    }
    bitmap[blockIdx.x] = bits;
    word_rows[blockIdx.x] = rows;
  }
}

// Output row (n, y, x) of a k x k stride-1 conv with pad_lo leading pad reads
// input rows (n, y - pad_lo + dy, x - pad_lo + dx), inside the image only.
__global__ __launch_bounds__(256) void row_dilate_kernel(
    const unsigned long long* __restrict__ rowbits, int M, int H, int W, int k, int pad_lo,
    unsigned long long* __restrict__ dilbits, int32_t* __restrict__ dil_rows) {
  __shared__ unsigned long long ballots[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int base = blockIdx.x * kRowsPerWord;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int p = base + 256 * kk + tid;
    bool f = false;
    if (p < M) {
      const int n = p / (H * W);
      const int r = p - n * H * W;
      const int y = r / W, x = r - y * W;
      for (int dy = 0; dy < k; ++dy) {
        const int iy = y - pad_lo + dy;
        if ((unsigned)iy >= (unsigned)H) continue;
        for (int dx = 0; dx < k; ++dx) {
          const int ix = x - pad_lo + dx;
          if ((unsigned)ix >= (unsigned)W) continue;
          const int q = (n * H + iy) * W + ix;
          f |= (rowbits[q >> 6] >> (q & 63)) & 1ull;
        }
      }
    }
    const unsigned long long b = __ballot(f);
    if (lane == 0) ballots[4 * kk + wave] = b;
  }
  __syncthreads();
  if (tid < 16) dilbits[(size_t)blockIdx.x * 16 + tid] = ballots[tid];
  if (tid == 0) {
    int rows = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) rows += __popcll(ballots[i]);
    dil_rows[blockIdx.x] = rows;
  }
}

// One workgroup: thread t owns the blocks [t * per, (t + 1) * per).
__global__ __launch_bounds__(256) void row_scan_kernel(const int32_t* __restrict__ word_rows,
                                                       const int32_t* __restrict__ dil_rows,
                                                       int words, int capacity, int list_cap,
                                                       int32_t* __restrict__ count,
                                                       int32_t* __restrict__ dil_prefix,
                                                       int32_t* __restrict__ nrows,
                                                       int32_t* __restrict__ err) {
  __shared__ int nz[256], dl[256];
  const int t = threadIdx.x;
  const int per = (words + 255) / 256;
  const int i0 = min(words, t * per), i1 = min(words, i0 + per);
  int s = 0, d = 0;
  for (int i = i0; i < i1; ++i) {
    s += word_rows[i];
    if (dil_rows != nullptr) d += dil_rows[i];
  }
  nz[t] = s;
  dl[t] = d;
  __syncthreads();
  if (t == 0) {
    int total = 0, run = 0;
    for (int i = 0; i < 256; ++i) {
      total += nz[i];
      const int c = dl[i];
      dl[i] = run;  // exclusive prefix of the threads' segments
      run += c;
    }
    *count = total;
    if (nrows != nullptr) *nrows = min(run, list_cap);
    if (total > capacity || run > list_cap) atomicOr(err, kErrRowBound);
  }
  __syncthreads();
  if (dil_rows != nullptr) {
    int run = dl[t];
    for (int i = i0; i < i1; ++i) {
      dil_prefix[i] = run;
      run += dil_rows[i];
    }
  }
}

__global__ __launch_bounds__(256) void row_compact_kernel(
    const unsigned long long* __restrict__ dilbits, const int32_t* __restrict__ dil_prefix,
    int list_cap, int32_t* __restrict__ rows) {
  __shared__ unsigned long long ballots[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 16) ballots[tid] = dilbits[(size_t)blockIdx.x * 16 + tid];
  __syncthreads();
  const int base = blockIdx.x * kRowsPerWord;
  const int first = dil_prefix[blockIdx.x];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int i = 4 * kk + wave;
    int pos = first;
    for (int j = 0; j < i; ++j) pos += __popcll(ballots[j]);
    const unsigned long long b = ballots[i];
    pos += __popcll(b & ((1ull << lane) - 1ull));
    if (((b >> lane) & 1ull) && pos < list_cap) rows[pos] = base + 64 * i + lane;
  }
}

int census_check_shape(int N, int H, int W) {
  D2MI_REQUIRE(N > 0 && H > 0 && W > 0 && (long long)N * H * W < (1LL << 31), "bad census shape");
  return 0;
}

}  // namespace
}  // namespace d2mi

using namespace d2mi;

extern "C" size_t d2mi_row_census_workspace_size(int N, int H, int W, int capacity, int dilate_k) {
  if (N <= 0 || H <= 0 || W <= 0 || (long long)N * H * W >= (1LL << 31) || capacity < 0) return 0;
  const int M = N * H * W;
  return layout_bytes<RowCensusSpace>(M, census_list_cap(M, capacity, dilate_k));
}

extern "C" int d2mi_row_census_layout(int N, int H, int W, int capacity, int dilate_k,
                                      int64_t* out, int out_len) {
  D2MI_REQUIRE(out != nullptr && out_len >= 7, "row census layout: 7 integers");
  if (census_check_shape(N, H, W)) return -1;
  D2MI_REQUIRE(capacity >= 0, "row census: negative capacity");
  const int M = N * H * W;
  RowCensusSpace sp;
  Workspace carve(nullptr, 0);
  const int cap = census_list_cap(M, capacity, dilate_k);
  sp.lay(carve, M, cap);
  auto off = [](const void* p) { return (int64_t)((const char*)p - (const char*)nullptr); };
  out[0] = off(sp.bitmap);
  out[1] = sp.words;
  out[2] = off(sp.word_rows);
  out[3] = off(sp.count);
  out[4] = cap ? off(sp.nrows) : -1;
  out[5] = cap ? off(sp.rows) : -1;
  out[6] = cap;
  return 0;
}

extern "C" int d2mi_row_census(const float* g, int N, int H, int W, int C, int capacity,
                               int dilate_k, int dilate_pad, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (census_check_shape(N, H, W)) return -1;
  D2MI_REQUIRE(C > 0 && C % 4 == 0, "row census: C must be a multiple of 4 (%d)", C);
  D2MI_REQUIRE(capacity >= 0, "row census: negative capacity");
  D2MI_REQUIRE(dilate_k >= 0 && dilate_k <= 7 && dilate_pad >= 0 &&
                   (dilate_k == 0 || dilate_pad < dilate_k),
               "row census: dilation window %d with pad %d", dilate_k, dilate_pad);
  const int M = N * H * W;
  const int cap = census_list_cap(M, capacity, dilate_k);
  RowCensusSpace sp;
  Workspace carve(workspace, workspace_bytes);
  sp.lay(carve, M, cap);
  D2MI_REQUIRE(workspace != nullptr && carve.ok(), "row census workspace too small (%zu < %zu)",
               workspace_bytes, carve.off);
  D2MI_REQUIRE(((uintptr_t)g & 15) == 0 && ((uintptr_t)workspace & 7) == 0,
               "row census: g must be 16-byte aligned, the workspace 8-byte");
  int32_t* err = error_word();
  D2MI_REQUIRE(err != nullptr, "cannot resolve the device error word");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(row_census_kernel, dim3(sp.words), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(g), M, C / 4, sp.bitmap, sp.word_rows,
                     sp.rowbits);
  D2MI_LAUNCH_CHECK();
  if (cap > 0) {
    hipLaunchKernelGGL(row_dilate_kernel, dim3(sp.words), dim3(256), 0, st, sp.rowbits, M, H, W,
                       dilate_k, dilate_pad, sp.dilbits, sp.dil_rows);
    D2MI_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(row_scan_kernel, dim3(1), dim3(256), 0, st, sp.word_rows, sp.dil_rows,
                     sp.words, capacity, cap, sp.count, sp.dil_prefix, sp.nrows, err);
  D2MI_LAUNCH_CHECK();
  if (cap > 0) {
    hipLaunchKernelGGL(row_compact_kernel, dim3(sp.words), dim3(256), 0, st, sp.dilbits,
                       sp.dil_prefix, cap, sp.rows);
    D2MI_LAUNCH_CHECK();
  }
  return 0;
}
