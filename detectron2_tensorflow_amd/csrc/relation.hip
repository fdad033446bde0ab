// Relation Networks' object relation attention (relation_module.py:29-89,
// :141-194) without an R x R tensor in memory.  The reference embeds every
// ordered pair of an image's R proposal slots into E sin / cos channels
// ([N, R, R, E]), turns them into G geometry weights with a 1x1 conv + ReLU
// ([N, R, R, G]) and runs a G-group softmax attention over the R columns
// ([N, R, G, R]).  Here a wave owns one row i and walks the columns j in tiles
// of 64 staged in LDS (boxes, k, v): each lane recomputes its pair's embedding
// on the fly (4 logs, E / 2 sincosf), keeps the row's running max and sum per
// group, and the P.V product runs from an LDS tile of probabilities with the
// value channel on the lane.  The forward saves the per-(row, group)
// log-sum-exp (as maximum and sum); the backward recomputes embedding and probabilities from it in
// two passes: a row-owner pass (dq, the row's sum_d dO.O, and the pairs' sums
// for the geometry weights through an LDS image of the tile's embedding) and a
// column-owner pass (dk, dv: a lane owns a column, a wave a chunk of rows).
// Every sum over rows or pairs goes through fixed-order partials: no atomics,
// bit-identical runs.  sincosf / logf / expf are the precise forms: the
// arguments reach 100 log(1e-5) = -1151.
#include "common.h"
#include "wave.h"

namespace d2mi {
namespace {

constexpr int kGMax = 16;      // groups (register arrays are this long)
constexpr int kDkMax = 8;      // key channels per group
constexpr int kDvMax = 64;     // value channels (one per lane in the P.V product)
constexpr int kEMax = 128;     // embedding channels
constexpr int kTile = 64;      // columns per tile: one per lane
constexpr int kFwdWaves = 4;   // rows per forward workgroup
constexpr int kRowWaves = 2;   // rows per row-owner backward workgroup
constexpr int kMaxChunks = 32; // row chunks of the column-owner pass
constexpr int kEsStride = kTile + 1;  // embedding image row: odd, conflict-free both ways

struct RelArgs {
  const float4* boxes;         // [N, R] yxyx
  const unsigned char* valid;  // [N, R]
  const float *q, *k, *v;      // [N, R, G*dk] x 2, [N, R, dv]
  const float *wg, *bg;        // [E, G], [G]
  int N, R, G, dk, dv, E;
  float sqrt_dk;
  float dim[kEMax / 8];        // 1000^(8 f / E)
};

// (h, w, cy, cx) of a slot (relation_module.py:49-52)
__device__ __forceinline__ float4 slot_geo(const float4 b) {
  return make_float4(b.z - b.x + 1.f, b.w - b.y + 1.f, 0.5f * (b.x + b.z), 0.5f * (b.y + b.w));
}

// The pre-activation of the G geometry weights of the ordered pair (i, j):
// bg + sum_c emb_c Wg[c, :], the embedding channel c = t (E/4) + s (E/8) + f
// (relation_module.py:54-86).  STORE: the pair's embedding into es[c * 65].
template <int GT, bool STORE>
__device__ __forceinline__ void pair_preact(const RelArgs& a, const float4 gi, const float4 gj,
                                            float (&x)[kGMax], float* es) {
  const int G = GT ? GT : a.G;
  const int F = a.E >> 3;
  float p[4];
  p[0] = logf(fmaxf((gi.z - gj.z) / gi.x, 1e-5f));
  p[1] = logf(fmaxf((gi.w - gj.w) / gi.y, 1e-5f));
  p[2] = logf(gi.x / gj.x);
  p[3] = logf(gi.y / gj.y);
#pragma unroll
  for (int g = 0; g < kGMax; ++g) x[g] = g < G ? a.bg[g] : 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float pos = 100.f * p[t];
    for (int f = 0; f < F; ++f) {
      float s, c;
      sincosf(pos / a.dim[f], &s, &c);
      const int cs = 2 * t * F + f, cc = cs + F;
      if (STORE) {
        es[cs * kEsStride] = s;
        es[cc * kEsStride] = c;
      }
      const float* ws = a.wg + cs * G;
      const float* wc = a.wg + cc * G;
#pragma unroll
      for (int g = 0; g < kGMax; ++g)
        if (g < G) x[g] = fmaf(c, wc[g], fmaf(s, ws[g], x[g]));
    }
  }
}

// logit[g] = log(max(relu(x_g), 1e-6)) + q_{i,g} . k_{j,g} / sqrt(dk)
// (relation_module.py:177-183); qi wave-uniform, kj the lane's LDS row.
template <int GT>
__device__ __forceinline__ void pair_logits(const RelArgs& a, const float (&x)[kGMax],
                                            const float* qi, const float* kj,
                                            float (&lg)[kGMax]) {
  const int G = GT ? GT : a.G;
#pragma unroll
  for (int g = 0; g < kGMax; ++g) {
    lg[g] = 0.f;
    if (g < G) {
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < kDkMax; ++c)
        if (c < a.dk) dot = fmaf(qi[g * a.dk + c], kj[g * a.dk + c], dot);
      lg[g] = logf(fmaxf(fmaxf(x[g], 0.f), 1e-6f)) + dot / a.sqrt_dk;
    }
  }
}

// dP[g] = sum_d dO[i, g, d] v[j, d]; doi wave-uniform, vj the lane's LDS row.
template <int GT>
__device__ __forceinline__ void pair_dp(const RelArgs& a, const float* doi, const float* vj,
                                        float (&dp)[kGMax]) {
  const int G = GT ? GT : a.G;
#pragma unroll
  for (int g = 0; g < kGMax; ++g) dp[g] = 0.f;
#pragma unroll 4
  for (int d = 0; d < a.dv; ++d) {
    const float vv = vj[d];
#pragma unroll
    for (int g = 0; g < kGMax; ++g)
      if (g < G) dp[g] = fmaf(doi[g * a.dv + d], vv, dp[g]);
  }
}

// One tile of columns into LDS: geometry, k rows (stride ks) and v rows
// (stride vs).  Invalid and out-of-range columns are the zeros of
// SparseBoxList.to_dense (box_list.py:204-246): box 0, k = v = 0.
__device__ __forceinline__ void stage_columns(const RelArgs& a, int n, int j0, float4* s_geo,
                                              float* s_k, int ks, float* s_v, int vs) {
  const int KD = a.G * a.dk;
  const size_t row0 = (size_t)n * a.R;
  for (int e = threadIdx.x; e < kTile; e += blockDim.x) {
    const int j = j0 + e;
    const bool ok = j < a.R && a.valid[row0 + j];
    s_geo[e] = slot_geo(ok ? a.boxes[row0 + j] : make_float4(0.f, 0.f, 0.f, 0.f));
  }
  if (s_k)
    for (int e = threadIdx.x; e < kTile * KD; e += blockDim.x) {
      const int jj = e / KD, c = e - jj * KD, j = j0 + jj;
      const bool ok = j < a.R && a.valid[row0 + j];
      s_k[jj * ks + c] = ok ? a.k[(row0 + j) * KD + c] : 0.f;
    }
  if (s_v)
    for (int e = threadIdx.x; e < kTile * a.dv; e += blockDim.x) {
      const int jj = e / a.dv, c = e - jj * a.dv, j = j0 + jj;
      const bool ok = j < a.R && a.valid[row0 + j];
      s_v[jj * vs + c] = ok ? a.v[(row0 + j) * a.dv + c] : 0.f;
    }
}

extern __shared__ __align__(16) float rel_lds[];

// ---------------------------------------------------------------- forward
// grid (ceil(R / 4), N), 256 threads: wave w owns row 4 bx + w.
// LDS: geo [64] float4 | p [4][64][16] | k [64][KD|1] | v [64][dv|1]
template <int GT>
__global__ __launch_bounds__(kFwdWaves * 64) void relation_fwd_kernel(RelArgs a,
                                                                      float* __restrict__ out,
                                                                      float* __restrict__ lse) {
  const int G = GT ? GT : a.G;
  const int KD = G * a.dk, ks = KD | 1, vs = a.dv | 1;
  float4* s_geo = reinterpret_cast<float4*>(rel_lds);
  float* s_p = rel_lds + 4 * kTile;
  float* s_k = s_p + kFwdWaves * kTile * kGMax;
  float* s_v = s_k + kTile * ks;
  const int n = blockIdx.y;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int i = blockIdx.x * kFwdWaves + wave;
  const size_t row = (size_t)n * a.R + (i < a.R ? i : 0);
  const bool active = i < a.R && a.valid[row];
  const float4 gi = slot_geo(a.boxes[row]);
  const float* qi = a.q + row * KD;
  float* pw = s_p + wave * kTile * kGMax;
  const int dl = lane < a.dv ? lane : a.dv - 1;

  float m[kGMax], l[kGMax], acc[kGMax];
#pragma unroll
  for (int g = 0; g < kGMax; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
    acc[g] = 0.f;
  }
  for (int j0 = 0; j0 < a.R; j0 += kTile) {
    __syncthreads();
    stage_columns(a, n, j0, s_geo, s_k, ks, s_v, vs);
    __syncthreads();
    if (active) {
      float x[kGMax], lg[kGMax];
      pair_preact<GT, false>(a, gi, s_geo[lane], x, nullptr);
      pair_logits<GT>(a, x, qi, s_k + lane * ks, lg);
      const bool in = j0 + lane < a.R;
      float p[kGMax];
#pragma unroll
      for (int g = 0; g < kGMax; ++g) {
        p[g] = 0.f;
        if (g < G) {
          const float v = in ? lg[g] : -INFINITY;
          const float mn = fmaxf(m[g], wave_max(v));  // finite: column j0 is in range
          const float alpha = expf(m[g] - mn);
          p[g] = expf(v - mn);
          l[g] = l[g] * alpha + p[g];
          acc[g] *= alpha;
          m[g] = mn;
        }
      }
      float4* pl = reinterpret_cast<float4*>(pw + lane * kGMax);
#pragma unroll
      for (int g = 0; g < kGMax; g += 4) pl[g >> 2] = make_float4(p[g], p[g + 1], p[g + 2], p[g + 3]);
    }
    __syncthreads();
    if (active) {
      // out[i, g, d] += sum_j p[j, g] v[j, d], d on the lane
      for (int jj = 0; jj < kTile; ++jj) {
        const float vv = s_v[jj * vs + dl];
        const float4* pj = reinterpret_cast<const float4*>(pw + jj * kGMax);
#pragma unroll
        for (int g4 = 0; g4 < kGMax / 4; ++g4) {
          if (g4 * 4 < G) {
            const float4 pp = pj[g4];
            acc[g4 * 4] = fmaf(pp.x, vv, acc[g4 * 4]);
            acc[g4 * 4 + 1] = fmaf(pp.y, vv, acc[g4 * 4 + 1]);
            acc[g4 * 4 + 2] = fmaf(pp.z, vv, acc[g4 * 4 + 2]);
            acc[g4 * 4 + 3] = fmaf(pp.w, vv, acc[g4 * 4 + 3]);
          }
        }
      }
    }
  }
  if (i >= a.R) return;
  float* oi = out + row * (size_t)(G * a.dv);
#pragma unroll
  for (int g = 0; g < kGMax; ++g) {
    if (g < G) {
      const float lt = active ? wave_sum(l[g]) : 1.f;
      if (lane < a.dv) oi[g * a.dv + lane] = active ? acc[g] / lt : 0.f;
      // the log-sum-exp m + log l in its two parts: the backward's
      // exp(logit - m) / l divides by the very l that out was divided by
      if (lane == g) {
        lse[row * 2 * G + g] = active ? m[g] : 0.f;
        lse[row * 2 * G + G + g] = lt;
      }
    }
  }
}

// ------------------------------------------------- backward, row-owner pass
// grid (ceil(R / 2), N), 128 threads: wave w owns row 2 bx + w.  Writes
// dq [N, R, KD], dsum [N, R, G] = sum_d dO.O, and the wave's sums over its
// pairs of emb_c dx_g and dx_g into wpart[(n gridDim.x + bx) 2 + w][E G + G].
// LDS: geo [64] float4 | ds [2][64][16] | dx [2][64][16] | k | v | es [2][E][65]
template <int GT>
__global__ __launch_bounds__(kRowWaves * 64) void relation_bwd_rows_kernel(
    RelArgs a, const float* __restrict__ o, const float* __restrict__ lse,
    const float* __restrict__ d_out, float* __restrict__ d_q, float* __restrict__ dsum,
    float* __restrict__ wpart) {
  const int G = GT ? GT : a.G;
  const int KD = G * a.dk, ks = KD | 1, vs = a.dv | 1;
  float4* s_geo = reinterpret_cast<float4*>(rel_lds);
  float* s_ds = rel_lds + 4 * kTile;
  float* s_dx = s_ds + kRowWaves * kTile * kGMax;
  float* s_k = s_dx + kRowWaves * kTile * kGMax;
  float* s_v = s_k + kTile * ks;
  float* s_es = s_v + kTile * vs;
  const int n = blockIdx.y;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int i = blockIdx.x * kRowWaves + wave;
  const size_t row = (size_t)n * a.R + (i < a.R ? i : 0);
  const bool active = i < a.R && a.valid[row];
  const float4 gi = slot_geo(a.boxes[row]);
  const float* qi = a.q + row * KD;
  const float* doi = d_out + row * (size_t)(G * a.dv);
  const float* oi = o + row * (size_t)(G * a.dv);
  const float* mi = lse + row * 2 * G;
  const float* li = mi + G;
  float* dsw = s_ds + wave * kTile * kGMax;
  float* dxw = s_dx + wave * kTile * kGMax;
  float* esw = s_es + wave * a.E * kEsStride;

  // D[g] = sum_d dO[i, g, d] O[i, g, d] (= sum_j P dP), summed in pair_dp's
  // order: where a row has one column, O = v and dP - D cancels exactly
  float D[kGMax];
#pragma unroll
  for (int g = 0; g < kGMax; ++g) D[g] = 0.f;
  if (active) {
#pragma unroll 4
    for (int d = 0; d < a.dv; ++d) {
#pragma unroll
      for (int g = 0; g < kGMax; ++g)
        if (g < G) D[g] = fmaf(doi[g * a.dv + d], oi[g * a.dv + d], D[g]);
    }
  }
  float dqacc[2] = {0.f, 0.f}, dbacc = 0.f;
  float dwacc[2][kGMax], w0[kGMax];
#pragma unroll
  for (int g = 0; g < kGMax; ++g) dwacc[0][g] = dwacc[1][g] = w0[g] = 0.f;

  for (int j0 = 0; j0 < a.R; j0 += kTile) {
    __syncthreads();
    stage_columns(a, n, j0, s_geo, s_k, ks, s_v, vs);
    __syncthreads();
    if (active) {
      float x[kGMax], lg[kGMax], dp[kGMax];
      pair_preact<GT, true>(a, gi, s_geo[lane], x, esw + lane);
      pair_logits<GT>(a, x, qi, s_k + lane * ks, lg);
      pair_dp<GT>(a, doi, s_v + lane * vs, dp);
      const bool in = j0 + lane < a.R;
      float ds[kGMax], dx[kGMax];
#pragma unroll
      for (int g = 0; g < kGMax; ++g) {
        ds[g] = dx[g] = 0.f;
        if (g < G) {
          // d log(max(relu(x), 1e-6)) / dx = w: 1 / gw where gw > 1e-6, else 0
          const float w = x[g] > 1e-6f ? 1.f / x[g] : 0.f;
          if (j0 == 0) w0[g] = __shfl(w, 0, 64);
          if (in) {
            ds[g] = expf(lg[g] - mi[g]) / li[g] * (dp[g] - D[g]);
            dx[g] = x[g] > 1e-6f ? ds[g] / x[g] : 0.f;
          }
          // dbg[g] += sum_j dS[j, g] w[j, g].  A row's dS sum to zero, so this
          // is sum_j dS (w - w0) for any constant w0, here column 0's w: the
          // row's rounding residue sum_j dS (D times the rounding of l, about
          // 1e-7 D) then enters times (w - w0) and not times w, and columns
          // with column 0's geometry weight drop out exactly.  The tile's 64
          // terms are added as a tree: a running sum of many near-equal terms
          // would round one way.
          const float t = __shfl(wave_sum_down(ds[g] * (w - w0[g])), 0, 64);
          if (lane == g) dbacc += t;
        }
      }
      float4* sl = reinterpret_cast<float4*>(dsw + lane * kGMax);
      float4* xl = reinterpret_cast<float4*>(dxw + lane * kGMax);
#pragma unroll
      for (int g = 0; g < kGMax; g += 4) {
        sl[g >> 2] = make_float4(ds[g], ds[g + 1], ds[g + 2], ds[g + 3]);
        xl[g >> 2] = make_float4(dx[g], dx[g + 1], dx[g + 2], dx[g + 3]);
      }
    }
    __syncthreads();
    if (active) {
      // dq[i, c] += sum_j dS[j, g(c)] k[j, c], c on the lane
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int c = lane + 64 * r;
        if (c < KD) {
          const int g = c / a.dk;
          float s = 0.f;
          for (int jj = 0; jj < kTile; ++jj) s = fmaf(dsw[jj * kGMax + g], s_k[jj * ks + c], s);
          dqacc[r] += s;
        }
      }
      // dWg[c, g] += sum_j emb[j, c] dx[j, g], c on the lane
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int c = lane + 64 * r;
        if (c < a.E) {
          const float* ec = esw + c * kEsStride;
          for (int jj = 0; jj < kTile; ++jj) {
            const float e = ec[jj];
            const float4* xj = reinterpret_cast<const float4*>(dxw + jj * kGMax);
#pragma unroll
            for (int g4 = 0; g4 < kGMax / 4; ++g4) {
              if (g4 * 4 < G) {
                const float4 d4 = xj[g4];
                dwacc[r][g4 * 4] = fmaf(e, d4.x, dwacc[r][g4 * 4]);
                dwacc[r][g4 * 4 + 1] = fmaf(e, d4.y, dwacc[r][g4 * 4 + 1]);
                dwacc[r][g4 * 4 + 2] = fmaf(e, d4.z, dwacc[r][g4 * 4 + 2]);
                dwacc[r][g4 * 4 + 3] = fmaf(e, d4.w, dwacc[r][g4 * 4 + 3]);
              }
            }
          }
        }
      }
    }
  }
  // (an inactive wave writes its zeros: the reduction reads every partial row)
  const int WP = a.E * G + G;
  float* wp = wpart + ((size_t)(n * gridDim.x + blockIdx.x) * kRowWaves + wave) * WP;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int c = lane + 64 * r;
    if (c < a.E) {
#pragma unroll
      for (int g = 0; g < kGMax; ++g)
        if (g < G) wp[c * G + g] = dwacc[r][g];
    }
    if (c < KD && i < a.R) d_q[row * KD + c] = dqacc[r] / a.sqrt_dk;
  }
  if (lane < G) {
    wp[a.E * G + lane] = dbacc;
    if (i < a.R) {
      float dv = 0.f;
#pragma unroll
      for (int g = 0; g < kGMax; ++g)
        if (g == lane) dv = D[g];
      dsum[row * G + lane] = dv;
    }
  }
}

// ---------------------------------------------- backward, column-owner pass
// grid (ceil(R / 64), chunks, N), one wave: lane = column j, the wave walks
// the rows of its chunk and keeps dk[j, :] and dv[j, :] in registers.  Writes
// kvpart[n][chunk][KD + dv][R].  LDS: k [64][KD|1] | v [64][dv|1]
template <int GT>
__global__ __launch_bounds__(64) void relation_bwd_cols_kernel(
    RelArgs a, const float* __restrict__ lse, const float* __restrict__ d_out,
    const float* __restrict__ dsum, int rows_per_chunk, float* __restrict__ kvpart) {
  const int G = GT ? GT : a.G;
  const int KD = G * a.dk, ks = KD | 1, vs = a.dv | 1;
  float4* s_geo = reinterpret_cast<float4*>(rel_lds);
  float* s_k = rel_lds + 4 * kTile;
  float* s_v = s_k + kTile * ks;
  const int n = blockIdx.z, lane = threadIdx.x;
  const int j = blockIdx.x * kTile + lane;
  stage_columns(a, n, blockIdx.x * kTile, s_geo, s_k, ks, s_v, vs);
  __syncthreads();
  const float4 gj = s_geo[lane];
  const float* kj = s_k + lane * ks;
  const float* vj = s_v + lane * vs;

  float dkacc[kGMax][kDkMax], dvacc[kDvMax];
#pragma unroll
  for (int g = 0; g < kGMax; ++g)
#pragma unroll
    for (int c = 0; c < kDkMax; ++c) dkacc[g][c] = 0.f;
#pragma unroll
  for (int d = 0; d < kDvMax; ++d) dvacc[d] = 0.f;

  const int i0 = blockIdx.y * rows_per_chunk;
  const int i1 = i0 + rows_per_chunk < a.R ? i0 + rows_per_chunk : a.R;
  for (int i = i0; i < i1; ++i) {
    const size_t row = (size_t)n * a.R + i;
    if (!a.valid[row]) continue;
    const float4 gi = slot_geo(a.boxes[row]);
    const float* qi = a.q + row * KD;
    const float* doi = d_out + row * (size_t)(G * a.dv);
    const float* mi = lse + row * 2 * G;
    const float* li = mi + G;
    const float* Di = dsum + row * G;
    float x[kGMax], lg[kGMax], dp[kGMax], P[kGMax];
    pair_preact<GT, false>(a, gi, gj, x, nullptr);
    pair_logits<GT>(a, x, qi, kj, lg);
    pair_dp<GT>(a, doi, vj, dp);
#pragma unroll
    for (int g = 0; g < kGMax; ++g) {
      P[g] = 0.f;
      if (g < G) {
        P[g] = expf(lg[g] - mi[g]) / li[g];
        const float ds = P[g] * (dp[g] - Di[g]);
#pragma unroll
        for (int c = 0; c < kDkMax; ++c)
          if (c < a.dk) dkacc[g][c] = fmaf(ds, qi[g * a.dk + c], dkacc[g][c]);
      }
    }
#pragma unroll
    for (int d = 0; d < kDvMax; ++d) {
      if (d < a.dv) {
#pragma unroll
        for (int g = 0; g < kGMax; ++g)
          if (g < G) dvacc[d] = fmaf(P[g], doi[g * a.dv + d], dvacc[d]);
      }
    }
  }
  if (j >= a.R) return;
  float* kp = kvpart + ((size_t)(n * gridDim.y + blockIdx.y) * (KD + a.dv)) * a.R + j;
#pragma unroll
  for (int g = 0; g < kGMax; ++g)
#pragma unroll
    for (int c = 0; c < kDkMax; ++c)
      if (g < G && c < a.dk) kp[(size_t)(g * a.dk + c) * a.R] = dkacc[g][c];
#pragma unroll
  for (int d = 0; d < kDvMax; ++d)
    if (d < a.dv) kp[(size_t)(KD + d) * a.R] = dvacc[d];
}

// dWg [E, G] and dbg [G] from the row pass's partial rows: 64 elements per
// workgroup, four interleaved slices of the rows each summed in order, then
// the four in order.
__global__ __launch_bounds__(256) void relation_reduce_w_kernel(const float* __restrict__ wpart,
                                                                int rows, int EG, int G,
                                                                float* __restrict__ d_wg,
                                                                float* __restrict__ d_bg) {
  __shared__ float red[4][64];
  const int WP = EG + G;
  const int e = blockIdx.x * 64 + (threadIdx.x & 63), slice = threadIdx.x >> 6;
  float s = 0.f;
  if (e < WP)
    for (int r = slice; r < rows; r += 4) s += wpart[(size_t)r * WP + e];
  red[slice][threadIdx.x & 63] = s;
  __syncthreads();
  if (slice == 0 && e < WP) {
    const int t = threadIdx.x;
    const float v = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    if (e < EG) d_wg[e] = v;
    else d_bg[e - EG] = v;
  }
}

// dk [N, R, KD] (/ sqrt(dk)) and dv [N, R, dv] from the column pass's chunk
// partials, summed in chunk order; rows of invalid slots are zero.
__global__ __launch_bounds__(256) void relation_reduce_kv_kernel(
    const float* __restrict__ kvpart, const unsigned char* __restrict__ valid, int N, int R,
    int KD, int dv, int chunks, float sqrt_dk, float* __restrict__ d_k, float* __restrict__ d_v) {
  const int C = KD + dv;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)N * C * R) return;
  const int j = (int)(t % R);
  const int c = (int)((t / R) % C);
  const int n = (int)(t / ((long long)R * C));
  float s = 0.f;
  for (int ch = 0; ch < chunks; ++ch) s += kvpart[((size_t)(n * chunks + ch) * C + c) * R + j];
  const size_t row = (size_t)n * R + j;
  if (!valid[row]) s = 0.f;
  if (c < KD) d_k[row * KD + c] = s / sqrt_dk;
  else d_v[row * dv + (c - KD)] = s;
}

int rows_per_chunk(int R) {
  const int r = (R + kMaxChunks - 1) / kMaxChunks;
  return r < 8 ? 8 : r;
}

// The backward's workspace, laid out by the op and measured by
// d2mi_relation_workspace_size.
struct RelationSpace {
  float* dsum;    // [N, R, G]
  float* wpart;   // [N * ceil(R / 2) * 2][E G + G]
  float* kvpart;  // [N][chunks][G dk + dv][R]
  int wrows, chunks, rpc;
  template <typename A>
  void lay(A& al, int N, int R, int G, int dk, int dv, int E) {
    rpc = rows_per_chunk(R);
    chunks = (R + rpc - 1) / rpc;
    wrows = N * ((R + kRowWaves - 1) / kRowWaves) * kRowWaves;
    dsum = al.template take<float>((size_t)N * R * G);
    wpart = al.template take<float>((size_t)wrows * (E * G + G));
    kvpart = al.template take<float>((size_t)N * chunks * (G * dk + dv) * R);
  }
};

int check_shape(int N, int R, int G, int dk, int dv, int E) {
  D2MI_REQUIRE(N >= 1 && N <= 65535, "relation: N = %d outside 1..65535", N);
  D2MI_REQUIRE(R >= 1 && R <= (1 << 20), "relation: R = %d outside 1..2^20", R);
  D2MI_REQUIRE(G >= 1 && G <= kGMax, "relation: G = %d outside 1..%d", G, kGMax);
  D2MI_REQUIRE(dk >= 1 && dk <= kDkMax, "relation: dk = %d outside 1..%d", dk, kDkMax);
  D2MI_REQUIRE(dv >= 4 && dv % 4 == 0 && dv <= kDvMax,
               "relation: dv = %d is not a multiple of 4 in 4..%d", dv, kDvMax);
  D2MI_REQUIRE(E >= 8 && E % 8 == 0 && E <= kEMax,
               "relation: E = %d is not a multiple of 8 in 8..%d", E, kEMax);
  return 0;
}

RelArgs make_args(const float* boxes, const uint8_t* valid, const float* q, const float* k,
                  const float* v, const float* wg, const float* bg, int N, int R, int G, int dk,
                  int dv, int E) {
  RelArgs a;
  a.boxes = reinterpret_cast<const float4*>(boxes);
  a.valid = valid;
  a.q = q;
  a.k = k;
  a.v = v;
  a.wg = wg;
  a.bg = bg;
  a.N = N;
  a.R = R;
  a.G = G;
  a.dk = dk;
  a.dv = dv;
  a.E = E;
  a.sqrt_dk = sqrtf((float)dk);
  for (int f = 0; f < kEMax / 8; ++f) a.dim[f] = powf(1000.f, (8.f / (float)E) * (float)f);
  return a;
}

// More than 64 KiB of dynamic LDS (of the CU's 160) is opted into per kernel.
template <typename K>
int allow_lds(K kernel, size_t bytes) {
  D2MI_REQUIRE(bytes <= 160 * 1024, "relation: %zu bytes of LDS", bytes);
  if (bytes > 64 * 1024)
    D2MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return 0;
}

size_t column_lds_floats(int G, int dk, int dv) {
  return 4 * kTile + (size_t)kTile * ((G * dk) | 1) + (size_t)kTile * (dv | 1);
}

}  // namespace
}  // namespace d2mi

using namespace d2mi;

extern "C" int d2mi_relation_fwd(const float* boxes, const uint8_t* valid, const float* q,
                                 const float* k, const float* v, const float* wg,
                                 const float* bg, int N, int R, int G, int dk, int dv, int E,
                                 float* out, float* lse, void* stream) {
  const int rc = check_shape(N, R, G, dk, dv, E);
  if (rc) return rc;
  D2MI_REQUIRE(boxes && valid && q && k && v && wg && bg && out && lse, "relation: null tensor");
  D2MI_REQUIRE(((uintptr_t)boxes & 15) == 0, "relation: 16-byte aligned boxes");
  const RelArgs a = make_args(boxes, valid, q, k, v, wg, bg, N, R, G, dk, dv, E);
  const size_t lds =
      (column_lds_floats(G, dk, dv) + (size_t)kFwdWaves * kTile * kGMax) * sizeof(float);
  const dim3 grid((R + kFwdWaves - 1) / kFwdWaves, N);
  if (allow_lds(G == 16 ? relation_fwd_kernel<16> : relation_fwd_kernel<0>, lds)) return -2;
  if (G == 16)
    hipLaunchKernelGGL(relation_fwd_kernel<16>, grid, dim3(kFwdWaves * 64), lds,
                       as_stream(stream), a, out, lse);
  else
    hipLaunchKernelGGL(relation_fwd_kernel<0>, grid, dim3(kFwdWaves * 64), lds,
                       as_stream(stream), a, out, lse);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t d2mi_relation_workspace_size(int N, int R, int G, int dk, int dv, int E) {
  if (N < 1 || R < 1 || G < 1 || dk < 1 || dv < 1 || E < 1) return 0;
  return layout_bytes<RelationSpace>(N, R, G, dk, dv, E);
}

extern "C" int d2mi_relation_bwd(const float* boxes, const uint8_t* valid, const float* q,
                                 const float* k, const float* v, const float* wg,
                                 const float* bg, const float* out, const float* lse,
                                 const float* d_out, int N, int R, int G, int dk, int dv, int E,
                                 float* d_q, float* d_k, float* d_v, float* d_wg, float* d_bg,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = check_shape(N, R, G, dk, dv, E);
  if (rc) return rc;
  Workspace w(workspace, workspace_bytes);
  RelationSpace sp;
  sp.lay(w, N, R, G, dk, dv, E);
  D2MI_REQUIRE(workspace != nullptr && w.ok(), "relation workspace too small (%zu < %zu)",
               workspace_bytes, w.off);
  D2MI_REQUIRE(boxes && valid && q && k && v && wg && bg && out && lse && d_out && d_q && d_k &&
                   d_v && d_wg && d_bg,
               "relation: null tensor");
  D2MI_REQUIRE(((uintptr_t)boxes & 15) == 0, "relation: 16-byte aligned boxes");
  const RelArgs a = make_args(boxes, valid, q, k, v, wg, bg, N, R, G, dk, dv, E);
  hipStream_t st = as_stream(stream);
  const size_t col = column_lds_floats(G, dk, dv);
  const size_t lds_rows =
      (col + (size_t)kRowWaves * (2 * kTile * kGMax + (size_t)E * kEsStride)) * sizeof(float);
  const dim3 grid_rows((R + kRowWaves - 1) / kRowWaves, N);
  const dim3 grid_cols((R + kTile - 1) / kTile, sp.chunks, N);
  if (allow_lds(G == 16 ? relation_bwd_rows_kernel<16> : relation_bwd_rows_kernel<0>, lds_rows) ||
      allow_lds(G == 16 ? relation_bwd_cols_kernel<16> : relation_bwd_cols_kernel<0>,
                col * sizeof(float)))
    return -2;
  if (G == 16) {
    hipLaunchKernelGGL(relation_bwd_rows_kernel<16>, grid_rows, dim3(kRowWaves * 64), lds_rows, st,
                       a, out, lse, d_out, d_q, sp.dsum, sp.wpart);
    D2MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(relation_bwd_cols_kernel<16>, grid_cols, dim3(64), col * sizeof(float), st,
                       a, lse, d_out, sp.dsum, sp.rpc, sp.kvpart);
  } else {
    hipLaunchKernelGGL(relation_bwd_rows_kernel<0>, grid_rows, dim3(kRowWaves * 64), lds_rows, st,
                       a, out, lse, d_out, d_q, sp.dsum, sp.wpart);
    D2MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(relation_bwd_cols_kernel<0>, grid_cols, dim3(64), col * sizeof(float), st,
                       a, lse, d_out, sp.dsum, sp.rpc, sp.kvpart);
  }
  D2MI_LAUNCH_CHECK();
  const int WP = E * G + G;
  hipLaunchKernelGGL(relation_reduce_w_kernel, dim3((WP + 63) / 64), dim3(256), 0, st, sp.wpart,
                     sp.wrows, E * G, G, d_wg, d_bg);
  D2MI_LAUNCH_CHECK();
  const long long nkv = (long long)N * (G * dk + dv) * R;
  hipLaunchKernelGGL(relation_reduce_kv_kernel, dim3((unsigned)((nkv + 255) / 256)), dim3(256), 0,
                     st, sp.kvpart, valid, N, R, G * dk, dv, sp.chunks, a.sqrt_dk, d_k, d_v);
  D2MI_LAUNCH_CHECK();
  return 0;
}
