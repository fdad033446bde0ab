// YOLOv4 inference pieces on gfx950 (d2mi.h, "YOLOv4"):
//
//   d2mi_yolov4_predictions   YOLOV4Outputs._get_predictions written densely:
//       boxes, conf, max-class score and its class for every prediction.
//   d2mi_yolov4_inference     YOLOV4Outputs.inference fused, per call
//       score    256 predictions per workgroup: every thread tests its own
//                prediction's sigmoid(conf) against the threshold (conf * p <=
//                conf for p <= 1, so a prediction that fails here cannot pass
//                with any class); each wave then works through the rows of
//                its survivors together (lanes over the K classes, coalesced).
//                Writes one sort key per prediction (~0: dropped), the class
//                of each survivor and the workgroup's survivor count.
//       compact  many workgroups per image, no hand-off between them: each
//                sums the counts of the blocks before its own (written by the
//                previous launch) and scatters its survivors' keys behind
//                them, in prediction order.  The last block writes the
//                image's count.
//       sort     sort_keys_segmented (score descending, index ascending).
//       nms      one workgroup per image: windows of 1,024 sorted candidates,
//                their boxes decoded from the logits on the way in, greedy
//                class-agnostic NMS in 64-wide tiles against the kept list,
//                stopping at max_det; then the gather and the zero padding.
//                The candidate x candidate mask of nms.hip is never built.
//     Counts stay on the device; nothing synchronises.
//   d2mi_spp_pool             the SPP block's three stride-1 max pools over
//       the zero-padded map and their concat with the input, one launch.
//   d2mi_activation           in-place leaky ReLU / Mish.
//
// The decode, sigmoid, score and class expressions of the two YOLO entry
// points are the same __device__ functions, so their bits agree.
#include "wave.h"
#include "yolo.h"

namespace d2mi {
namespace {

constexpr int kNmsWG = 1024;
constexpr int kTile = 64;

__device__ __forceinline__ float yolo_conf(const float* row) { return sigmoidf_tf(row[4]); }

// max_c(conf * sigmoid(prob_c)) and the lowest c that attains it (tf.argmax),
// by one whole wave: lane i takes classes i, i + 64, ... (consecutive lanes
// read consecutive words, whatever the row's alignment).  Every lane returns
// the same pair.
__device__ __forceinline__ void wave_score_cls(const float* row, int K, float conf, float& score,
                                               int& cls) {
  const int lane = threadIdx.x & 63;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < K; c += 64) {
    const float v = conf * sigmoidf_tf(row[5 + c]);
    if (v > best || bi == 0x7fffffff) {
      best = v;
      bi = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) {
      best = ov;
      bi = oi;
    }
  }
  score = best;
  cls = bi;
}

// The rows flagged in `todo` (a wave ballot: bit i = the row of lane i), one
// after the other by the whole wave; lane i ends up with its own row's pair.
__device__ __forceinline__ void wave_rows(uint64_t todo, const float* my_row, float my_conf, int K,
                                          float& score, int& cls) {
  const int lane = threadIdx.x & 63;
  while (todo) {
    const int b = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    const float* row = reinterpret_cast<const float*>(
        ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)((uint64_t)(uintptr_t)my_row >> 32), b) << 32) |
        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uintptr_t)my_row, b));
    const float conf = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(my_conf), b));
    float s;
    int c;
    wave_score_cls(row, K, conf, s, c);
    if (lane == b) {
      score = s;
      cls = c;
    }
  }
}

// ------------------------------------------------------- dense predictions
__global__ __launch_bounds__(kYB) void yolo_predictions_kernel(YoloGeo g, float4* __restrict__ boxes,
                                                               float* __restrict__ conf,
                                                               float* __restrict__ score,
                                                               int32_t* __restrict__ cls) {
  const int n = blockIdx.y;
  const int p = blockIdx.x * kYB + threadIdx.x;
  const bool on = p < g.P;
  const PredAt q = locate(g, n, on ? p : g.P - 1);
  const float c = yolo_conf(q.row);
  float s = 0.f;
  int k = 0;
  wave_rows(__ballot(on), q.row, c, g.K, s, k);
  if (!on) return;
  const size_t o = (size_t)n * g.P + p;
  boxes[o] = yolo_box(g, q);
  conf[o] = c;
  score[o] = s;
  cls[o] = k;
}

// ------------------------------------------------------------------- score
__global__ __launch_bounds__(kYB) void yolo_score_kernel(YoloGeo g, float thresh,
                                                         uint64_t* __restrict__ keys,
                                                         int32_t* __restrict__ cls,
                                                         int32_t* __restrict__ bcnt) {
  __shared__ int s_cnt[kYB / 64];
  const int n = blockIdx.y;
  const int p = blockIdx.x * kYB + threadIdx.x;
  const bool on = p < g.P;
  const PredAt q = locate(g, n, on ? p : g.P - 1);
  const float c = yolo_conf(q.row);
  float s = 0.f;
  int k = 0;
  wave_rows(__ballot(on && c > thresh), q.row, c, g.K, s, k);
  const bool keep = on && c > thresh && s > thresh;
  const uint64_t kept = __ballot(keep);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(kept);
  if (on) {
    const size_t o = (size_t)n * g.P + p;
    keys[o] = keep ? desc_key(s, (uint32_t)p) : ~0ull;
    if (keep) cls[o] = k;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
#pragma unroll
    for (int v = 0; v < kYB / 64; ++v) tot += s_cnt[v];
    bcnt[n * g.nb + blockIdx.x] = tot;
  }
}

// ----------------------------------------------------------------- compact
__global__ __launch_bounds__(kYB) void yolo_compact_kernel(int P, int nb,
                                                           const uint64_t* __restrict__ keys,
                                                           const int32_t* __restrict__ bcnt,
                                                           uint64_t* __restrict__ ckeys,
                                                           int32_t* __restrict__ count) {
  __shared__ int s_w[kYB / 64], s_c[kYB / 64];
  const int n = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
  const int lane = t & 63, w = t >> 6;
  // survivors of the image's earlier blocks
  int before = 0;
  for (int i = t; i < b; i += kYB) before += bcnt[n * nb + i];
  before = wave_sum(before);
  const int p = b * kYB + t;
  const uint64_t key = p < P ? keys[(size_t)n * P + p] : ~0ull;
  const bool keep = key != ~0ull;
  const uint64_t m = __ballot(keep);
  if (lane == 0) {
    s_w[w] = before;
    s_c[w] = __popcll(m);
  }
  __syncthreads();
  int base = 0, mine = 0;
#pragma unroll
  for (int v = 0; v < kYB / 64; ++v) {
    base += s_w[v];
    if (v < w) mine += s_c[v];
  }
  if (keep) ckeys[(size_t)n * P + base + mine + __popcll(m & ((1ull << lane) - 1ull))] = key;
  if (b == nb - 1 && t == 0) {
    int tot = base;
#pragma unroll
    for (int v = 0; v < kYB / 64; ++v) tot += s_c[v];
    count[n] = tot;
  }
}

// --------------------------------------------------------------------- nms
// Greedy NonMaxSuppressionV3 of image n's sorted candidates (the NMS phase of
// retina_post.hip without class offsets): a tile's 64 candidates are tested
// against the kept list by all 16 waves (kept rows dealt round the waves),
// its own upper triangle by 4 rows a wave, and wave 0 walks the tile.
__global__ __launch_bounds__(kNmsWG) void yolo_nms_kernel(
    YoloGeo g, const uint64_t* __restrict__ sorted, const int32_t* __restrict__ count,
    const int32_t* __restrict__ cls, float thr, int max_det, float4* __restrict__ ob,
    float* __restrict__ os, int32_t* __restrict__ oc, uint8_t* __restrict__ ov) {
  extern __shared__ float4 dyn[];
  float4* kept_box = dyn;                     // [max_det]
  float4* wbox = kept_box + max_det;          // [kNmsWG]
  uint64_t* wkey = reinterpret_cast<uint64_t*>(wbox + kNmsWG);  // [kNmsWG]
  uint64_t* kept_key = wkey + kNmsWG;         // [max_det]
  __shared__ uint64_t diag[kTile], wsup[kNmsWG / 64];
  __shared__ int s_nk;
  const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int total = min(max(count[n], 0), g.P);
  const uint64_t* src = sorted + (size_t)n * g.P;
  if (t == 0) s_nk = 0;
  __syncthreads();
  int nk = 0;
  for (int w0 = 0; w0 < total && nk < max_det; w0 += kNmsWG) {
    const int wn = min(kNmsWG, total - w0);
    if (t < wn) {
      const uint64_t key = src[w0 + t];
      wkey[t] = key;
      wbox[t] = yolo_box(g, locate(g, n, (int)(uint32_t)key));
    }
    __syncthreads();
    for (int t0 = 0; t0 < wn && nk < max_det; t0 += kTile) {
      const int rem = wn - t0;
      const float4 cb = lane < rem ? wbox[t0 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
      bool sup = false;
      for (int i = w; i < nk; i += kNmsWG / 64) sup = sup || (tf_iou(kept_box[i], cb) > thr);
      const uint64_t ws = __ballot(sup);
      if (lane == 0) wsup[w] = ws;
      constexpr int RPW = kTile / (kNmsWG / 64);  // tile rows per wave
#pragma unroll
      for (int rr = 0; rr < RPW; ++rr) {
        const int r = w * RPW + rr;
        const bool live = r < rem && lane > r && lane < rem;
        const float4 rb = wbox[t0 + min(r, rem - 1)];
        const uint64_t d = __ballot(live && tf_iou(rb, cb) > thr);
        if (lane == 0) diag[r] = d;
      }
      __syncthreads();
      if (w == 0) {
        uint64_t removed = 0;
#pragma unroll
        for (int v = 0; v < kNmsWG / 64; ++v) removed |= wsup[v];
        if (rem < 64) removed |= ~((1ull << rem) - 1ull);
        uint64_t keptm = 0;
        int k2 = nk;
        const uint64_t my_diag = diag[lane];
        for (int r = 0; r < kTile; ++r) {
          if (k2 >= max_det) break;
          if (!((removed >> r) & 1ull)) {
            keptm |= 1ull << r;
            ++k2;
            removed |= readlane64(my_diag, r);
          }
        }
        if ((keptm >> lane) & 1ull) {
          const int pos = nk + __popcll(keptm & ((1ull << lane) - 1ull));
          kept_box[pos] = wbox[t0 + lane];
          kept_key[pos] = wkey[t0 + lane];
        }
        if (lane == 0) s_nk = k2;
      }
      __syncthreads();
      nk = s_nk;
    }
    __syncthreads();
  }
  for (int i = t; i < max_det; i += kNmsWG) {
    const size_t o = (size_t)n * max_det + i;
    const bool k = i < nk;
    const uint64_t key = k ? kept_key[i] : 0ull;
    ob[o] = k ? kept_box[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    os[o] = k ? key_score(key) : 0.f;
    oc[o] = k ? cls[(size_t)n * g.P + (uint32_t)key] : 0;
    ov[o] = k ? 1 : 0;
  }
}

struct YoloWs {
  uint64_t* keys;    // [N P] one key per prediction (~0: dropped)
  uint64_t* ckeys;   // [N P] the survivors' keys, compacted per image
  uint64_t* sorted;  // [N P]
  int32_t* cls;      // [N P] class of each survivor
  int32_t* bcnt;     // [N nb]
  int32_t* count;    // [N]
  void* sort_ws;
  size_t sort_bytes;
  template <typename A>
  void lay(A& a, int N, int P) {
    const int nb = (P + kYB - 1) / kYB;
    keys = a.template take<uint64_t>((size_t)N * P);
    ckeys = a.template take<uint64_t>((size_t)N * P);
    sorted = a.template take<uint64_t>((size_t)N * P);
    cls = a.template take<int32_t>((size_t)N * P);
    bcnt = a.template take<int32_t>((size_t)N * nb);
    count = a.template take<int32_t>(N);
    sort_bytes = sort_workspace_size(N, P);
    sort_ws = a.template take<char>(sort_bytes);
  }
};

}  // namespace

// (declared in yolo.h: yolo_loss.hip builds its tables with them too)
int64_t yolo_total(int N, int L, const int32_t* level_hw, int A) {
  D2MI_REQUIRE(N >= 1, "N=%d out of range", N);
  D2MI_REQUIRE(L >= 1 && L <= D2MI_MAX_LEVELS, "L=%d out of range [1,%d]", L, D2MI_MAX_LEVELS);
  D2MI_REQUIRE(A >= 1 && A <= kYoloMaxA, "A=%d out of range [1,%d]", A, kYoloMaxA);
  D2MI_REQUIRE(level_hw != nullptr, "level_hw is null");
  int64_t P = 0;
  for (int l = 0; l < L; ++l) {
    D2MI_REQUIRE(level_hw[2 * l] > 0 && level_hw[2 * l + 1] > 0, "level %d is empty", l);
    P += (int64_t)level_hw[2 * l] * level_hw[2 * l + 1] * A;
  }
  D2MI_REQUIRE(P < (1ll << 31) - kYB && (int64_t)N * ((P + kYB - 1) / kYB) < (1ll << 31),
               "too many predictions");
  D2MI_REQUIRE(N < 65536, "N=%d exceeds the grid", N);
  return P;
}

int make_geo_tables(YoloGeo& g, const int32_t* level_hw, const float* strides, const float* cell_hw,
                    const float* scale_yx, int L, int A, int K, int N) {
  D2MI_REQUIRE(K >= 1, "K=%d out of range", K);
  const int64_t P = yolo_total(N, L, level_hw, A);
  if (P < 0) return -1;
  D2MI_REQUIRE(strides && cell_hw, "null host array");
  g = YoloGeo{};
  g.L = L;
  g.A = A;
  g.K = K;
  g.N = N;
  g.P = (int32_t)P;
  g.nb = (int32_t)((P + kYB - 1) / kYB);
  g.p0[0] = 0;
  for (int l = 0; l < L; ++l) {
    g.H[l] = level_hw[2 * l];
    g.W[l] = level_hw[2 * l + 1];
    g.p0[l + 1] = g.p0[l] + g.H[l] * g.W[l] * A;
    g.stride[l] = strides[l];
    if (scale_yx) {
      g.s[l] = scale_yx[2 * l];
      g.half[l] = scale_yx[2 * l + 1];
    }
    for (int a = 0; a < A; ++a) {
      g.cell_h[l][a] = cell_hw[(l * A + a) * 2];
      g.cell_w[l][a] = cell_hw[(l * A + a) * 2 + 1];
    }
  }
  return 0;
}

int make_geo(YoloGeo& g, const float* const* logits, const int32_t* level_hw, const float* strides,
             const float* cell_hw, const float* scale_yx, int L, int A, int K, int N) {
  D2MI_REQUIRE(K >= 1, "K=%d out of range", K);
  if (yolo_total(N, L, level_hw, A) < 0) return -1;
  D2MI_REQUIRE(logits && strides && cell_hw && scale_yx, "null host array");
  int rc = make_geo_tables(g, level_hw, strides, cell_hw, scale_yx, L, A, K, N);
  if (rc) return rc;
  for (int l = 0; l < L; ++l) {
    g.ptr[l] = logits[l];
    D2MI_REQUIRE(g.ptr[l] != nullptr, "level %d logits are null", l);
  }
  return 0;
}

namespace {

// --------------------------------------------------------------------- SPP
// One workgroup per (channel chunk, output row h, image): the column maxima
// of the 5-, 9- and 13-row windows round h for every (w, channel quad) into
// LDS -- a row outside the map counts as 0 (tf.pad), and so does a column
// outside it, whose entries stay 0 -- then the three row maxima from LDS.
// Max is exact in any order, so this is the 25 / 81 / 169-tap pool's value.
__device__ __forceinline__ float4 max4(float4 a, float4 b) {
  return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

// max over columns [-R, R] round c (entries CC apart)
template <int R>
__device__ __forceinline__ float4 row_max(const float4* c, int CC) {
  float4 m = c[0];
#pragma unroll
  for (int d = 1; d <= R; ++d) m = max4(m, max4(c[-d * CC], c[d * CC]));
  return m;
}

constexpr int kSppT = 256;
constexpr int kSppPad = 6;

__global__ __launch_bounds__(kSppT) void spp_pool_kernel(const float4* __restrict__ x, int H, int W,
                                                         int C4, int CC, float4* __restrict__ out) {
  extern __shared__ float4 col[];  // [3][W + 12][CC]
  const int q0 = blockIdx.x * CC, h = blockIdx.y, n = blockIdx.z;
  const int cc = min(CC, C4 - q0);
  const int Wp = W + 2 * kSppPad;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = threadIdx.x; i < 3 * Wp * CC; i += kSppT) col[i] = zero;
  __syncthreads();
  const float4* xn = x + (size_t)n * H * W * C4;
  auto row = [&](int hh, int w, int q) -> float4 {
    if (hh < 0 || hh >= H) return make_float4(0.f, 0.f, 0.f, 0.f);  // (tf.pad)
    return xn[((size_t)hh * W + w) * C4 + q0 + q];
  };
  for (int i = threadIdx.x; i < W * cc; i += kSppT) {
    const int w = i / cc, q = i - w * cc;
    const float4 x0 = row(h, w, q);
    const float4 m5 = max4(max4(x0, max4(row(h - 1, w, q), row(h + 1, w, q))),
                           max4(row(h - 2, w, q), row(h + 2, w, q)));
    const float4 m9 = max4(max4(m5, max4(row(h - 3, w, q), row(h + 3, w, q))),
                           max4(row(h - 4, w, q), row(h + 4, w, q)));
    const float4 m13 = max4(max4(m9, max4(row(h - 5, w, q), row(h + 5, w, q))),
                            max4(row(h - 6, w, q), row(h + 6, w, q)));
    col[(0 * Wp + w + kSppPad) * CC + q] = m13;
    col[(1 * Wp + w + kSppPad) * CC + q] = m9;
    col[(2 * Wp + w + kSppPad) * CC + q] = m5;
    // the input's own quarter of the concat
    out[(((size_t)n * H + h) * W + w) * (4 * C4) + 3 * C4 + q0 + q] = x0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < W * cc; i += kSppT) {
    const int w = i / cc, q = i - w * cc;
    float4* o = out + (((size_t)n * H + h) * W + w) * (4 * C4) + q0 + q;
    const float4* c = col + (size_t)(w + kSppPad) * CC + q;
    o[0] = row_max<6>(c, CC);
    o[C4] = row_max<4>(c + (size_t)Wp * CC, CC);
    o[2 * (size_t)C4] = row_max<2>(c + 2 * (size_t)Wp * CC, CC);
  }
}

// -------------------------------------------------------------- activation
// Mish x * tanh(softplus(x)) (lib/layers/activation.py:5-7).  With e = exp(x),
// tanh(log(1 + e)) = ((1 + e)^2 - 1) / ((1 + e)^2 + 1) = n / (n + 2), n =
// e (e + 2): one exponential, no cancellation.  Evaluated in float64 and
// rounded once (the pass is bound by its 8 B per element, not by the
// arithmetic); past x = 20 the factor is 1 to float64's last bit.
__device__ __forceinline__ float mish_f(float x) {
  const double xd = (double)x;
  if (x > 20.f) return x;
  const double e = exp(xd);
  const double nn = e * (e + 2.0);
  return (float)(xd * (nn / (nn + 2.0)));
}
// tf.nn.leaky_relu / F.leaky_relu: x where x > 0, alpha * x elsewhere.
__device__ __forceinline__ float leaky_f(float x, float alpha) { return x > 0.f ? x : x * alpha; }

template <int CODE>
__device__ __forceinline__ float act_f(float x, float alpha) {
  return CODE == 1 ? leaky_f(x, alpha) : mish_f(x);
}

constexpr int kActT = 256;

// In place over n floats at x: a scalar head up to the first 16-byte
// boundary, float4s, a scalar tail.
template <int CODE>
__global__ __launch_bounds__(kActT) void activation_kernel(float* __restrict__ x, int64_t n, int head,
                                                           float alpha) {
  const int64_t tid = (int64_t)blockIdx.x * kActT + threadIdx.x;
  const int64_t nth = (int64_t)gridDim.x * kActT;
  const int64_t n4 = (n - head) >> 2;
  float4* x4 = reinterpret_cast<float4*>(x + head);
  for (int64_t i = tid; i < n4; i += nth) {
    float4 v = x4[i];
    v.x = act_f<CODE>(v.x, alpha);
    v.y = act_f<CODE>(v.y, alpha);
    v.z = act_f<CODE>(v.z, alpha);
    v.w = act_f<CODE>(v.w, alpha);
    x4[i] = v;
  }
  // head and tail: fewer than 8 elements in all
  if (tid < head) x[tid] = act_f<CODE>(x[tid], alpha);
  const int64_t t0 = head + 4 * n4;
  if (tid < n - t0) x[t0 + tid] = act_f<CODE>(x[t0 + tid], alpha);
}

}  // namespace
}  // namespace d2mi

using namespace d2mi;

extern "C" int d2mi_yolov4_predictions(const float* const* logits, const int32_t* level_hw,
                                       const float* strides, const float* cell_hw,
                                       const float* scale_yx, int L, int A, int K, int N,
                                       float* out_boxes, float* out_conf, float* out_score,
                                       int32_t* out_cls, void* stream) {
  YoloGeo g;
  int rc = make_geo(g, logits, level_hw, strides, cell_hw, scale_yx, L, A, K, N);
  if (rc) return rc;
  D2MI_REQUIRE(((uintptr_t)out_boxes & 15) == 0, "out_boxes must be 16B aligned");
  hipLaunchKernelGGL(yolo_predictions_kernel, dim3(g.nb, N), dim3(kYB), 0, as_stream(stream), g,
                     reinterpret_cast<float4*>(out_boxes), out_conf, out_score, out_cls);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t d2mi_yolov4_workspace_size(int N, int L, const int32_t* level_hw, int A) {
  const int64_t P = yolo_total(N, L, level_hw, A);
  if (P < 0) return 0;
  return layout_bytes<YoloWs>(N, (int)P);
}

extern "C" int d2mi_yolov4_inference(const float* const* logits, const int32_t* level_hw,
                                     const float* strides, const float* cell_hw,
                                     const float* scale_yx, int L, int A, int K, int N,
                                     float score_thresh, float nms_thresh, int max_det,
                                     float* out_boxes, float* out_scores, int32_t* out_classes,
                                     uint8_t* out_valid, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  hipStream_t st = as_stream(stream);
  D2MI_REQUIRE(K >= 1, "K=%d out of range", K);
  D2MI_REQUIRE(max_det >= 1 && max_det <= 1000, "max_det=%d out of range [1,1000]", max_det);
  const int64_t P64 = yolo_total(N, L, level_hw, A);
  if (P64 < 0) return -1;
  const int P = (int)P64;
  Workspace w(workspace, workspace_bytes);
  YoloWs o;
  o.lay(w, N, P);
  D2MI_REQUIRE(w.ok(), "yolov4 workspace too small (%zu < %zu)", workspace_bytes, w.off);
  YoloGeo g;
  int rc = make_geo(g, logits, level_hw, strides, cell_hw, scale_yx, L, A, K, N);
  if (rc) return rc;
  D2MI_REQUIRE(((uintptr_t)out_boxes & 15) == 0, "out_boxes must be 16B aligned");
  hipLaunchKernelGGL(yolo_score_kernel, dim3(g.nb, N), dim3(kYB), 0, st, g, score_thresh, o.keys,
                     o.cls, o.bcnt);
  D2MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(yolo_compact_kernel, dim3(g.nb, N), dim3(kYB), 0, st, P, g.nb, o.keys, o.bcnt,
                     o.ckeys, o.count);
  D2MI_LAUNCH_CHECK();
  rc = sort_keys_segmented(o.ckeys, o.sorted, o.count, N, P, o.sort_ws, o.sort_bytes, st);
  if (rc) return rc;
  const size_t lds = (size_t)(max_det + kNmsWG) * (sizeof(float4) + sizeof(uint64_t));
  hipLaunchKernelGGL(yolo_nms_kernel, dim3(N), dim3(kNmsWG), lds, st, g, o.sorted, o.count, o.cls,
                     nms_thresh, max_det, reinterpret_cast<float4*>(out_boxes), out_scores,
                     out_classes, out_valid);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" int d2mi_spp_pool(const float* x, int N, int H, int W, int C, float* out, void* stream) {
  D2MI_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 4, "bad SPP sizes");
  D2MI_REQUIRE(C % 4 == 0, "SPP: C=%d must be a multiple of 4", C);
  D2MI_REQUIRE(H < 65536 && N < 65536, "SPP: H=%d / N=%d exceed the grid", H, N);
  D2MI_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "SPP tensors must be 16B aligned");
  const int C4 = C / 4;
  // channel quads per workgroup: up to 8, fewer when the three LDS rows of a
  // wide map would pass 48 KB
  const size_t per = 3 * (size_t)(W + 2 * kSppPad) * sizeof(float4);
  const int CC = (int)std::min<size_t>(std::min(C4, 8), (48 * 1024) / per);
  D2MI_REQUIRE(CC >= 1, "SPP: W=%d is too wide", W);
  hipLaunchKernelGGL(spp_pool_kernel, dim3((C4 + CC - 1) / CC, H, N), dim3(kSppT), per * CC,
                     as_stream(stream), reinterpret_cast<const float4*>(x), H, W, C4, CC,
                     reinterpret_cast<float4*>(out));
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" int d2mi_activation(float* x, int64_t n, int code, float alpha, void* stream) {
  D2MI_REQUIRE(code == 1 || code == 2, "activation code %d is not 1 (leaky_relu) or 2 (mish)", code);
  D2MI_REQUIRE(n >= 0, "n is negative");
  if (n == 0) return 0;
  D2MI_REQUIRE(((uintptr_t)x & 3) == 0, "activation: x must be 4B aligned");
  const int head = (int)std::min<int64_t>(n, (4 - (((uintptr_t)x >> 2) & 3)) & 3);
  // one float4 per thread up to 4,096 workgroups, a grid stride beyond
  const int64_t want = ((n >> 2) + kActT - 1) / kActT;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, 4096));
  if (code == 1)
    hipLaunchKernelGGL(activation_kernel<1>, dim3(grid), dim3(kActT), 0, as_stream(stream), x, n, head,
                       alpha);
  else
    hipLaunchKernelGGL(activation_kernel<2>, dim3(grid), dim3(kActT), 0, as_stream(stream), x, n, head,
                       alpha);
  D2MI_LAUNCH_CHECK();
  return 0;
}
