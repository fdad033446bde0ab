// Launch plans of the MFMA convolutions: forward (conv_mfma.hip), multi-level
// forward and weight gradient (conv_wgrad.hip).  Host integer arithmetic only
// (plain C++17, no HIP types): each family's plan is one value, computed
// here, consumed by its launcher and its *_workspace_size export alike, and
// readable through d2mi_conv2d_plan / _levels_plan / _wgrad_plan without a GPU.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "tuning.h"
#include "workspace.h"

namespace d2mi {

constexpr int kConvBK = 32;        // input channels per forward k-step
constexpr int kWgradKP = 32;       // pixels per wgrad k-step
constexpr int kMaxConvLevels = 6;
constexpr int kPlanSplit3 = 4;     // conv / wgrad flags bit 2: split-bf16 products
constexpr int kPlanAccum = 8;      // wgrad flags bit 3: accumulate into dw / dbias

// Facts about a launch's operands that the plan rules use (the `operands`
// mask of the plan queries).  A null pointer counts as aligned.
enum PlanOperands {
  kOpTopdown = 1,
  kOpResidual = 2,
  kOpGate = 4,
  kOpAligned = 8,       // the output (conv: and top-down / residual / gate) is 16-B aligned
  kOpBiasAligned = 16,  // conv: the bias is
  kOpWorkspace = 32,    // a workspace is passed
  kOpWsAligned = 64,    // and it is 16-B aligned
  kOpAllAligned = kOpAligned | kOpBiasAligned | kOpWsAligned,
};

inline int conv_dims(int H, int W, int KH, int KW, int stride, int pb, int pe, int& OH, int& OW) {
  OH = (H + pb + pe - KH) / stride + 1;
  OW = (W + pb + pe - KW) / stride + 1;
  return (OH > 0 && OW > 0) ? 0 : -1;
}

// n steps cut into about `want` equal ranges: the range length, then the
// count of non-empty ranges.
struct StepSplit {
  int splits, per;
};
inline StepSplit split_steps(int n, int want) {
  const int per = (n + want - 1) / want;
  return {(n + per - 1) / per, per};
}

// Split-K of the forward convs.  Fewer tiles than resident workgroups and a
// long K: split K (to about `slots` workgroups: every split writes and the
// reduce reads one more partial slab of the output).
inline StepSplit conv_split_k(int ntiles, int nk, int slots) {
  int want = 1;
  if (4 * ntiles < 3 * slots && nk >= 16)
    want = std::min(std::max(1, slots / std::max(ntiles, 1)), std::min(nk / 8, 16));
  return split_steps(nk, want);
}

enum ConvFamily {
  kConv128x128 = 0,
  kConv128x64 = 1,
  kConv128x32 = 2,
  kConvWS256x128 = 3,  // warp-specialised, split products only
  kConvStream1x1 = 4,
};
enum PlanReduce { kReduceNone = 0, kReduceScalar = 1, kReduceFloat4 = 2 };

// Resident workgroups per CU of a family's kernel: the 128x128 kernel runs
// three (168 VGPRs, 48 KiB LDS: conv_mfma_kernel<..., OCC = 3>), the narrower
// tiles two, the warp-specialised and the streaming kernel one.
inline int conv_occ(int family) {
  if (family >= kConvWS256x128) return 1;
  return family == kConv128x128 ? 3 : 2;
}

// The tile family of a shape.  wide_ok: the 128x128 tile may be used -- its
// kernels only carry the LDS epilogue (Cout % 4 == 0 and 16-B aligned
// operands); otherwise 128x64.  split: the split-product math; the
// warp-specialised 256x128 kernel exists only in that
// form, and takes the long-K convs (>= 16 k-steps: every 3x3 with Cin >= 64,
// the 1x1s with Cin >= 512), where its deeper staging pipeline pays; the
// short-K 1x1s (2-8 k-steps) stay on the 3-per-CU kernel, whose prologue /
// epilogue overlap across workgroups (tools/ws_ab.py, 16 Mask R-CNN shapes).
inline int conv_family(int Cout, int KH, int KW, int Cin, bool wide_ok, bool split) {
  const int f = Cout <= 32 ? kConv128x32 : (Cout <= 64 || !wide_ok ? kConv128x64 : kConv128x128);
  // tuning "conv_ws_mink": the fewest k-steps that go to the WS kernel (A/B)
  if (f == kConv128x128 && split &&
      KH * KW * ((Cin + kConvBK - 1) / kConvBK) >= tuning(kTuneConvWSMinK) &&
      KH * KW <= 32)  // (the WS stagers keep a 32-bit tap mask per row)
    return kConvWS256x128;
  return f;
}
inline int conv_bm(int family) { return family == kConvWS256x128 ? 256 : 128; }
inline int conv_bn(int family) {
  return family == kConv128x64 ? 64 : family == kConv128x32 ? 32 : 128;
}

// One launch of a tiled kernel: tiles [tile0, tile0 + tiles) x splits
// workgroups; with splits > 1 the partials of output rows [m_base, m_end) go
// to the launch's slab and `reduce` (grid reduce_grid x 256 threads) sums them
// in a fixed order and applies the epilogue.
struct ConvLaunch {
  int tile0, tiles, splits, kt_per_split, m_base, m_end, reduce, reduce_grid;
};

struct ConvPlan {
  int family, occ, split3, lds_epi;
  int M, OH, OW, BM, BN, nM, nN, nk;
  // the tiled launches (tail.tiles == 0: no tail launch); under the streaming
  // family: what the tiled kernels would run, not launched
  ConvLaunch main, tail;
  // streaming family: conv1x1_stream_kernel<tn, kmax, 8, form & 1 (residual),
  // form & 2 (gate)> on `grid` workgroups of 512 threads over nslices slices
  int kmax, tn, form, nslices, grid;
  size_t ws_bytes;  // what the tiled launches carve (ConvSpace)
};

// The workspace of a forward conv: the split-K slab of the main launch, then
// the tail launch's ([splits][rows][Cout] each; no plan has both today).
struct ConvSpace {
  float *main, *tail;
  template <typename A>
  void lay(A& a, const ConvPlan& p, int Cout) {
    main = tail = nullptr;
    if (p.main.splits > 1)
      main = a.template take<float>((size_t)p.main.splits * (p.main.m_end - p.main.m_base) * Cout);
    if (p.tail.tiles > 0)
      tail = a.template take<float>((size_t)p.tail.splits * (p.tail.m_end - p.tail.m_base) * Cout);
  }
};

struct ConvShape {
  int N, H, W, Cin, Cout, KH, KW, stride, pad_beg, pad_end;
};

// The plan of one forward conv launch (-1: the output is empty).  flags:
// d2mi_conv2d_nhwc_ex's; operands: PlanOperands; cus: the device's CU count.
// A missing or short workspace gives the one-pass plan (no split-K, no tail
// split), silently: d2mi_conv2d_nhwc passes none.
inline int plan_conv(const ConvShape& s, int flags, int operands, size_t workspace_bytes, int cus,
                     ConvPlan* out) {
  ConvPlan p = {};
  int OH, OW;
  if (conv_dims(s.H, s.W, s.KH, s.KW, s.stride, s.pad_beg, s.pad_end, OH, OW)) return -1;
  const int M = s.N * OH * OW, Cout = s.Cout, Cin = s.Cin;
  const bool split = (flags & kPlanSplit3) != 0, one_by_one = s.KH == 1 && s.KW == 1;
  const bool aligned = (operands & kOpAligned) != 0;
  p.M = M;
  p.OH = OH;
  p.OW = OW;
  p.split3 = split;
  p.lds_epi = Cout % 4 == 0 && aligned && (operands & kOpWsAligned) != 0;
  p.family = conv_family(Cout, s.KH, s.KW, Cin, p.lds_epi != 0, split);
  p.occ = conv_occ(p.family);
  p.BM = conv_bm(p.family);
  p.BN = conv_bn(p.family);
  p.nM = (M + p.BM - 1) / p.BM;
  p.nN = (Cout + p.BN - 1) / p.BN;
  p.nk = s.KH * s.KW * ((Cin + kConvBK - 1) / kConvBK);
  const int ntiles = p.nM * p.nN;
  const int G = p.occ * cus;  // resident workgroups
  // The stride-1 1x1 shapes with K = 256 that the streaming kernel takes
  // (1.17x into 64 channels, 1.12x into 512 at >= 32 k pixels,
  // profiles/r5_stream_ab_force_tn_rule.log).  The tiled plan of these
  // shapes never splits its tail tiles' K, so that a launch the streaming
  // kernel cannot take (operands not 16-B aligned: a gradient bucket view)
  // sums K in the streaming kernel's order: both round alike
  // (tests/test_gpu_dp.py's one-rank RCCL equality).  For K <= 128 the tiled
  // plan has no split at all (< 8 k-steps).
  const bool stream256 = one_by_one && Cin == 256 && M >= 32768 && (Cout <= 64 || Cout == 512) &&
                         Cout % 4 == 0;
  // split-K target: two workgroups per CU even for the 3-per-CU kernel (A/B
  // over 384..1024 slots on the training step: 512 fastest, +2.5 % over 768
  // -- fewer splits, less partial-slab traffic for the reduce); tuning
  // "conv_split_slots" overrides it
  const int gs = tuning(kTuneConvSplitSlots) > 0 ? tuning(kTuneConvSplitSlots)
                                                 : (p.family == kConvWS256x128 ? 1 : 2) * cus;
  const StepSplit ks = conv_split_k(ntiles, p.nk, gs);
  p.main = {0, ntiles, ks.splits, ks.per, 0, M, kReduceNone, 0};
  p.tail = {ntiles, 0, 1, p.nk, M, M, kReduceNone, 0};
  // Tail split: with more tiles than resident workgroups, a last round that
  // is mostly empty (1050 tiles = 2 rounds of 512 + 26 on the FPN p2 3x3,
  // 525 = 512 + 13 on p3) costs about a whole round for a few tiles.  Those
  // tiles (whole pixel-row blocks) are split along K over the idle slots
  // instead and reduced in a fixed order.
  // (tuning "conv_tail": 0 off; "conv_tail_mink": the fewest k-steps whose tail tiles are split)
  if (ks.splits == 1 && ntiles > G && p.nk >= std::max(2, tuning(kTuneConvTailMinK)) &&
      tuning(kTuneConvTail) != 0 && !stream256) {
    const int full = (ntiles / G) * G / p.nN * p.nN;
    const int tail = ntiles - full;
    const int want = tail > 0 && 2 * tail <= G ? std::min(std::min(G / tail, p.nk / 4), 32) : 1;
    if (want >= 2) {
      const StepSplit ts = split_steps(p.nk, want);
      p.main.tiles = full;
      p.tail = {full, tail, ts.splits, ts.per, full / p.nN * p.BM, M, kReduceNone, 0};
    }
  }
  p.ws_bytes = layout_bytes<ConvSpace>(p, Cout);
  if (p.ws_bytes > workspace_bytes || !(operands & kOpWorkspace)) {  // one pass
    p.main = {0, ntiles, 1, p.nk, 0, M, kReduceNone, 0};
    p.tail = {ntiles, 0, 1, p.nk, M, M, kReduceNone, 0};
    p.ws_bytes = 0;
  }
  // The split-K reduce of a launch: float4s when bias / top-down / residual /
  // gate, the slab and the output can be read and written as such.
  const bool bias_al = (operands & kOpBiasAligned) != 0, ws_al = (operands & kOpWsAligned) != 0;
  const bool wide = Cout % 4 == 0 && ws_al && aligned && bias_al;
  for (ConvLaunch* l : {&p.main, &p.tail}) {
    if (l->tiles == 0 || l->splits == 1) continue;
    const int64_t total = (int64_t)(l->m_end - l->m_base) * Cout;
    l->reduce = wide ? kReduceFloat4 : kReduceScalar;
    l->reduce_grid = wide ? (int)std::min<int64_t>((total / 4 + 255) / 256, 8192)
                          : (int)std::min<int64_t>((total + 255) / 256, 4096);
  }
  // r5: conv1x1_stream_kernel for the memory-bound stride-1 unpadded 1x1s:
  // split products, no top-down, Cin 64 / 128 / 256, Cout % 4 == 0, 16-B
  // aligned operands, and enough pixel strips to fill the chip (tuning
  // "conv_stream": 0 off; else the fewest output pixels; < 0, A/B: every
  // eligible shape of >= -value pixels).  Where it measured faster than the
  // tiled kernel (tools/stream_ab.py): every K = 64 and K = 128 launch, and
  // K = 256 into <= 64 or 512 channels (stream256; any K = 256 under force);
  // K = 256 with residual AND gate spills.  In all of them both kernels sum K
  // in the same order: bit-identical.
  const int tv = tuning(kTuneConvStream);
  const bool res = (operands & kOpResidual) != 0, gate = (operands & kOpGate) != 0;
  if (tv != 0 && split && one_by_one && s.stride == 1 && s.pad_beg == 0 &&
      !(operands & kOpTopdown) && (Cin == 64 || Cin == 128 || Cin == 256) &&
      M >= (tv < 0 ? -tv : tv) && Cout % 4 == 0 && aligned && bias_al &&
      !(Cin == 256 && ((res && gate) || !(tv < 0 || stream256)))) {
    p.family = kConvStream1x1;
    p.occ = conv_occ(p.family);
    p.kmax = Cin;
    p.form = (res ? 1 : 0) | (gate ? 2 : 0);
    // BN 128 (TN 4) for K <= 128 with at most one epilogue operand, else BN
    // 64 (TN 2): the registers of a residual AND a gate, and K = 256's A
    // fragments, leave no room for TN 4.  TN 2 also when 128-wide slices
    // leave fewer strip tasks than the chip has waves (one 8-wave workgroup per CU).
    const int nstrips = (M + 31) / 32;
    const bool few = (long long)nstrips * ((Cout + 127) / 128) < 8LL * cus;
    p.tn = (Cin == 256 || (res && gate) || few) ? 2 : 4;
    p.nslices = (Cout + 32 * p.tn - 1) / (32 * p.tn);
    // one resident workgroup per CU (LDS: the weight slice + the slabs) over
    // all slices, whole XCD rounds, and no group without a strip for each of
    // its waves
    int groups = std::max(1, cus / p.nslices / 8);
    groups = std::min(groups, std::max(1, nstrips / 8 / 8));
    p.grid = 8 * groups * p.nslices;
  }
  *out = p;
  return 0;
}

// ---- multi-level forward conv (d2mi_conv2d_nhwc_levels): the 128-row tiled
// kernels over the levels' concatenated tiles; no warp-specialised form (r3
// measured it neutral for Mask R-CNN and 2-8 % slower for the RetinaNet /
// SOLOv2 towers; removed in r4).  When all levels together are under a round
// of workgroups, K is split by the single-level rule on the summed tile
// count, over the levels' concatenated rows; the level-aware reduce needs
// Cout % 4 == 0 and 16-B aligned outputs and slab.
struct ConvLevelsPlan {
  int family, occ, lds_epi, BM, BN, nN, nk, ntiles, splits, kt_per_split, reduce_grid;
  int tile0[kMaxConvLevels + 1];  // level l owns tiles [tile0[l], tile0[l + 1])
  int moff[kMaxConvLevels + 1];   // first row of each level in the slab; [6] = all rows
  int OH[kMaxConvLevels], OW[kMaxConvLevels];
  size_t ws_bytes;
};
struct ConvLevelsSpace {
  float* partial;  // [splits][rows][Cout]
  template <typename A>
  void lay(A& a, int splits, int64_t rows, int Cout) {
    partial = splits > 1 ? a.template take<float>((size_t)splits * rows * Cout) : nullptr;
  }
};
// dims: {N, H, W} per level; operands: kOpAligned (every level's output),
// kOpWorkspace, kOpWsAligned.  Geometry is the caller's to validate.
inline void plan_conv_levels(const int32_t* dims, int nlev, int Cin, int Cout, int KH, int KW,
                             int stride, int pad_beg, int pad_end, int operands,
                             size_t workspace_bytes, int cus, ConvLevelsPlan* out) {
  ConvLevelsPlan p = {};
  p.lds_epi = Cout % 4 == 0 && (operands & kOpAligned) != 0;
  p.family = conv_family(Cout, KH, KW, Cin, p.lds_epi != 0, false);
  p.occ = conv_occ(p.family);
  p.BM = conv_bm(p.family);
  p.BN = conv_bn(p.family);
  p.nN = (Cout + p.BN - 1) / p.BN;
  p.nk = KH * KW * ((Cin + kConvBK - 1) / kConvBK);
  int64_t rows = 0;
  int t = 0;
  for (int l = 0; l <= kMaxConvLevels; ++l) {
    p.tile0[l] = l <= nlev ? t : 0;
    p.moff[l] = (int)rows;
    if (l >= nlev) continue;
    conv_dims(dims[3 * l + 1], dims[3 * l + 2], KH, KW, stride, pad_beg, pad_end, p.OH[l], p.OW[l]);
    const int64_t M = (int64_t)dims[3 * l] * p.OH[l] * p.OW[l];
    rows += M;
    t += (int)((M + p.BM - 1) / p.BM) * p.nN;
  }
  p.ntiles = t;
  StepSplit ks = {1, p.nk};
  if (p.lds_epi) ks = conv_split_k(t, p.nk, p.occ * cus);
  p.ws_bytes = layout_bytes<ConvLevelsSpace>(ks.splits, rows, Cout);
  if (ks.splits > 1 && (!(operands & kOpWorkspace) || workspace_bytes < p.ws_bytes ||
                        !(operands & kOpWsAligned))) {
    ks = {1, p.nk};  // no (usable) workspace: one pass per tile
    p.ws_bytes = 0;
  }
  p.splits = ks.splits;
  p.kt_per_split = ks.per;
  if (p.splits > 1)
    p.reduce_grid = (int)std::min<int64_t>((rows * (Cout / 4) + 255) / 256, 8192);
  *out = p;
}

// ---- weight gradient (conv_wgrad.hip)
enum WgradKernel {
  kWgradF32 = 0,        // conv_wgrad_kernel<TM, TN>
  kWgradSplit = 1,      // conv_wgrad_split_kernel<TM, TN>
  kWgradSplitOcc3 = 2,  // conv_wgrad_split_kernel<2, 2, 3>
  kWgradWS = 3,         // conv_wgrad_ws_kernel<1>
  kWgradWSInc = 4,      // conv_wgrad_ws_kernel<1, true>
};
struct WgradPlan {
  int kernel, TM, TN, BM, BN, OH, OW, nCi, nCo, ntiles, nchunks, splits, chunks_per_split;
  int part;  // the partial slabs are written (splits > 1, or an accumulating call)
  int reduce, reduce_grid;
  size_t ws_bytes;  // WgradSpace of the slabs written
};
// The wgrad workspace: `slabs` dw partials, then as many dbias partials (one
// block, nothing between them).
struct WgradSpace {
  float *dw, *dbias;
  template <typename A>
  void lay(A& a, int slabs, size_t wsize, int Cout) {
    dw = a.template take<float>((size_t)slabs * (wsize + Cout));
    dbias = dw ? dw + (size_t)slabs * wsize : nullptr;
  }
};

// The row census of a sparse gradient map of M pixel rows (conv_rows.hip):
// one bit per 32-pixel chunk (kWgradKP) that holds a non-zero row, the
// non-zero rows of each bitmap word, their total (read by
// d2mi_conv2d_wgrad_rows, which lays out this head alone: list_cap 0); then,
// with list_cap > 0, the sorted list of the output rows of a KxK stride-1
// conv whose window holds a non-zero row (d2mi_conv2d_nhwc_rows) and the
// flags and prefix sums it is compacted from.
struct RowCensusSpace {
  uint32_t* bitmap;    // [words]
  int32_t* word_rows;  // [words]
  int32_t* count;      // [1]
  int words;
  unsigned long long* rowbits;  // [16 * words] bit r % 64 of word r / 64: row r is non-zero
  unsigned long long* dilbits;  // [16 * words] the same of the dilated (listed) rows
  int32_t* dil_rows;            // [words] listed rows of each 1024-row block
  int32_t* dil_prefix;          // [words] their exclusive prefix sum
  int32_t* nrows;               // [1] listed rows (clamped to list_cap)
  int32_t* rows;                // [list_cap] ascending
  template <typename A>
  void lay(A& a, int M, int list_cap) {
    const int nchunks = (M + kWgradKP - 1) / kWgradKP;
    words = (nchunks + 31) / 32;
    bitmap = a.template take<uint32_t>(words);
    word_rows = a.template take<int32_t>(words);
    count = a.template take<int32_t>(1);
    rowbits = dilbits = nullptr;
    dil_rows = dil_prefix = nrows = rows = nullptr;
    if (list_cap <= 0) return;
    rowbits = a.template take<unsigned long long>((size_t)16 * words);
    dilbits = a.template take<unsigned long long>((size_t)16 * words);
    dil_rows = a.template take<int32_t>(words);
    dil_prefix = a.template take<int32_t>(words);
    nrows = a.template take<int32_t>(1);
    rows = a.template take<int32_t>(list_cap);
  }
};
// Capacity of the dilated row list: every one of `capacity` non-zero rows
// lies in the windows of k * k output rows (0 = no list).
inline int census_list_cap(int M, int capacity, int k) {
  if (k <= 0) return 0;
  return (int)std::max<long long>(1, std::min<long long>((long long)capacity * k * k, M));
}
// Most chunks of one pixel split that the bitmap weight gradient lists in LDS
// (a split with more runs the dense kernel).
constexpr int kWgradListCap = 2048;

// flags: d2mi_conv2d_wgrad_ex's; operands: kOpAligned (dw), kOpWorkspace,
// kOpWsAligned.  A missing or short workspace gives one split.
inline int plan_wgrad(const ConvShape& s, int flags, int operands, size_t workspace_bytes,
                      WgradPlan* out) {
  WgradPlan p = {};
  if (conv_dims(s.H, s.W, s.KH, s.KW, s.stride, s.pad_beg, s.pad_end, p.OH, p.OW)) return -1;
  const int Cin = s.Cin, Cout = s.Cout, taps = s.KH * s.KW;
  const bool split3 = (flags & kPlanSplit3) != 0;
  const long long P = (long long)s.N * p.OH * p.OW;
  // 128 x 128 tiles for 256-wide channels; 64-wide when a dimension is small
  p.TM = Cin > 64 ? 2 : 1;
  p.TN = Cout > 64 ? 2 : 1;
  // The warp-specialised kernel (256 x 128 tiles, one workgroup per CU; split
  // products only) takes the KxK convs with Cin % 256 == 0, Cout % 128 == 0
  // (3x3 shapes 10-20 %
  // faster, the 1x1s 9 % slower -- their 8 chunks of 32 pixels per split are
  // too short for its prologue).  1x1s (tuning "wgrad_ws1" = the GFLOP
  // threshold; 0 = off): only from ~6 GFLOP up -- the smaller ones have too
  // few 256x128 tiles x 16-chunk splits to fill the chip (tools/wgrad_ws1_ab.sh:
  // the FPN p2 lateral 165 -> 140 us, the strided shortcuts 8-13 % faster,
  // the 4.4 GFLOP res4 1x1s 7 % slower)
  const bool ws1 = taps == 1 && tuning(kTuneWgradWS1) > 0 &&
                   2.0 * (double)P * (double)Cin * Cout >= tuning(kTuneWgradWS1) * 1e9;
  const bool ws = split3 && (taps > 1 || ws1) && Cin % 256 == 0 && Cout % 128 == 0;
  p.BM = ws ? 256 : 64 * p.TM;
  p.BN = 64 * p.TN;
  p.nCi = (Cin + p.BM - 1) / p.BM;
  p.nCo = (Cout + p.BN - 1) / p.BN;
  p.ntiles = taps * p.nCi * p.nCo;
  p.nchunks = (int)((P + kWgradKP - 1) / kWgradKP);
  // The 128x128 split wgrad can run three workgroups per CU (168 VGPRs, 52 KiB
  // LDS).  Measured (tools/conv_ab.py --set wgrad): 3% faster on the FPN p2 3x3
  // (134,400 pixels), slower on everything smaller (the extra pixel splits cost
  // more partial traffic than the occupancy gains), so only pixel counts of
  // 64k and up take it (tuning "wgrad_occ3_min_p").
  const bool occ3 = !ws && p.TM == 2 && p.TN == 2 && P >= tuning(kTuneWgradOcc3MinP);
  // the incremental pixel cursor (conv_wgrad_ws_kernel INC): same-size
  // stride-1 convs whose per-thread runs of 4 pixels and 32-pixel chunk
  // steps wrap at most one row and one image, pixel indices < 2^24
  const bool inc = s.stride == 1 && p.OH == s.H && p.OW == s.W && p.OW >= 4 &&
                   kWgradKP / p.OW + 1 <= p.OH && P + kWgradKP < (1 << 24);
  p.kernel = !split3 ? kWgradF32
             : ws    ? (inc ? kWgradWSInc : kWgradWS)
                     : (occ3 ? kWgradSplitOcc3 : kWgradSplit);
  // about one round of resident workgroups (1, 2 or 3 per CU; tuning
  // "wgrad_slots"), each walking >= 16 chunks ("wgrad_minch"), at most 128
  // splits ("wgrad_maxsplit")
  const int minch = tuning(kTuneWgradMinCh) > 0 ? tuning(kTuneWgradMinCh) : 16;
  const int maxsplit = tuning(kTuneWgradMaxSplit) > 0 ? tuning(kTuneWgradMaxSplit) : 128;
  const int G = tuning(kTuneWgradSlots) > 0 ? tuning(kTuneWgradSlots) : (ws ? 256 : (occ3 ? 768 : 512));
  int want = std::max(1, G / p.ntiles);
  want = std::min(std::min(want, std::max(1, p.nchunks / minch)), maxsplit);
  StepSplit ps = split_steps(p.nchunks, want);
  const size_t wsize = (size_t)taps * Cin * Cout;
  if (ps.splits > 1 && (layout_bytes<WgradSpace>(ps.splits, wsize, Cout) > workspace_bytes ||
                        !(operands & kOpWorkspace)))
    ps = {1, p.nchunks};  // no workspace: one split
  p.splits = ps.splits;
  p.chunks_per_split = ps.per;
  p.part = p.splits > 1 || (flags & kPlanAccum) != 0;
  p.ws_bytes = p.part ? layout_bytes<WgradSpace>(p.splits, wsize, Cout) : 0;
  if (p.part) {
    const bool wide = wsize % 4 == 0 && (operands & kOpWsAligned) != 0 && (operands & kOpAligned) != 0;
    p.reduce = wide ? kReduceFloat4 : kReduceScalar;
    p.reduce_grid = wide ? (int)std::min<size_t>((wsize / 4 + Cout + 255) / 256, 8192)
                         : (int)std::min<size_t>((wsize + Cout + 255) / 256, 4096);
  }
  *out = p;
  return 0;
}

// ---- grouped weight gradients (d2mi_conv2d_wgrad_group): many small wgrads
// in one launch and one reduce per kernel family instead of a pair of small
// grids each (tuning "wgrad_group" = 1, the default: every problem with the
// pixel splits of its own plan, so with the bits of its single launch; the
// workspace then holds all the problems' slabs at once).  Alone, a wgrad of
// 2-72 output tiles also has to cut its pixels into 14-62 splits to fill the
// chip by itself; under "wgrad_group" = 2 a family's tile-chunks fill it
// together with long pixel walks and few partial slabs, at the price of
// other rounding.
constexpr int kMaxWgradGroup = 64;
// A workgroup's fixed cost (prologue, epilogue, slab write) in 32-pixel chunk
// steps: the warp-specialised kernel's share of its peak at 19, 75 and 300
// chunks per workgroup (0.321, 0.447, 0.506) fits 0.53 n / (n + 14).
constexpr int kWgradGroupFixed = 14;
enum WgradFamily {
  kWgradFamWS = 0,       // conv_wgrad_ws_kernel<1>
  kWgradFamWSInc = 1,    // conv_wgrad_ws_kernel<1, true>
  kWgradFamSplit22 = 2,  // conv_wgrad_split_kernel<2, 2>
  kWgradFamSplit21 = 3,
  kWgradFamSplit12 = 4,
  kWgradFamSplit11 = 5,
  kWgradFamSplitOcc3 = 6,  // conv_wgrad_split_kernel<2, 2, 3>
  kWgradFamilies = 7,
  kWgradFamNone = -1,  // the f32 kernels: launched alone
};
inline int wgrad_family(const WgradPlan& p) {
  switch (p.kernel) {
    case kWgradWS: return kWgradFamWS;
    case kWgradWSInc: return kWgradFamWSInc;
    case kWgradSplitOcc3: return kWgradFamSplitOcc3;
    case kWgradSplit:
      return p.TM == 2 ? (p.TN == 2 ? kWgradFamSplit22 : kWgradFamSplit21)
                       : (p.TN == 2 ? kWgradFamSplit12 : kWgradFamSplit11);
    default: return kWgradFamNone;
  }
}
// Resident workgroups of a family's kernel on 256 CUs (plan_wgrad's G).
inline int wgrad_family_slots(int family) {
  return family <= kWgradFamWSInc ? 256 : (family == kWgradFamSplitOcc3 ? 768 : 512);
}
struct WgradGroupFamily {
  int count;              // problems of the family (0: no launch)
  int nwg;                // workgroups of the grouped launch
  int chunks_per_split;   // common to the family's problems
  int reduce_problems;    // problems that go through slabs
  long long reduce_items; // float4s of dw + bias elements over those problems
  int reduce_grid;
  size_t slab_off, slab_floats;  // the family's block of the workspace, in floats
};
struct WgradGroupPlan {
  int n, grouped;  // grouped 0: every problem runs its own plan_wgrad plan, alone
  WgradPlan p[kMaxWgradGroup];        // own geometry; splits / chunks_per_split / part of the group
  int family[kMaxWgradGroup];         // WgradFamily
  int wg0[kMaxWgradGroup];            // first workgroup in the family's launch
  size_t slab_off[kMaxWgradGroup];    // floats from the workspace start: [splits][wsize] dw
                                      // partials, then [splits][Cout] bias partials
  long long item0[kMaxWgradGroup];    // first item of the family's reduce (-1: no slabs)
  WgradGroupFamily fam[kWgradFamilies];
  size_t ws_bytes;
};

// The total order the plan walks the problems in, so that it does not depend
// on the order they are given in: by shape (equal shapes get equal plans, and
// their relative order only permutes equal entries).
inline bool wgrad_shape_less(const ConvShape& a, const ConvShape& b) {
  const int ka[] = {a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad_beg, a.pad_end};
  const int kb[] = {b.N, b.H, b.W, b.Cin, b.Cout, b.KH, b.KW, b.stride, b.pad_beg, b.pad_end};
  return std::lexicographical_compare(ka, ka + 10, kb, kb + 10);
}

// Workgroups of a family at `per` chunks per split.
inline long long wgrad_group_wgs(const WgradGroupPlan& g, int family, int per) {
  long long w = 0;
  for (int i = 0; i < g.n; ++i)
    if (g.family[i] == family) w += (long long)g.p[i].ntiles * ((g.p[i].nchunks + per - 1) / per);
  return w;
}

// flags: d2mi_conv2d_wgrad_ex's without the accumulate bit; operands:
// kOpWorkspace, kOpWsAligned (a workspace that is not 16-B aligned counts as
// none).  A group of one, and a missing or short workspace, give each problem
// its own plan_wgrad plan (grouped = 0).  -1: a bad shape or too many problems.
inline int plan_wgrad_group(const ConvShape* shapes, int n, int flags, int operands,
                            size_t workspace_bytes, int cus, WgradGroupPlan* out) {
  WgradGroupPlan& g = *out;
  g = {};
  if (n <= 0 || n > kMaxWgradGroup) return -1;
  g.n = n;
  const size_t own_ws = (operands & kOpWorkspace) ? workspace_bytes : 0;
  for (int i = 0; i < n; ++i) {
    if (plan_wgrad(shapes[i], flags, operands | kOpAligned, own_ws, &g.p[i])) return -1;
    g.family[i] = wgrad_family(g.p[i]);
    g.item0[i] = -1;
  }
  const bool usable = (operands & kOpWorkspace) && (operands & kOpWsAligned);
  if (n == 1 || !usable || (flags & kPlanAccum)) return 0;
  // tuning "wgrad_group" 1: the problems keep the splits of their own plans and
  // only share the launches (and one reduce per family) -- every gradient has
  // the bits of its single launch; 2: one chunks-per-split per family, chosen
  // below -- long walks and few slabs, but other pixel ranges per partial sum,
  // so the gradients differ from the single launches' in the last bits
  const bool common = tuning(kTuneWgradGroup) >= 2;
  WgradGroupPlan t = g;
  const int minch = tuning(kTuneWgradMinCh) > 0 ? tuning(kTuneWgradMinCh) : 16;
  const int maxsplit = tuning(kTuneWgradMaxSplit) > 0 ? tuning(kTuneWgradMaxSplit) : 128;
  for (int f = 0; f < kWgradFamilies; ++f) {
    int count = 0, lo = minch, longest = 1, only = -1;
    for (int i = 0; i < n; ++i) {
      if (t.family[i] != f) continue;
      ++count;
      only = i;
      longest = std::max(longest, t.p[i].nchunks);
      lo = std::max(lo, (t.p[i].nchunks + maxsplit - 1) / maxsplit);
    }
    t.fam[f].count = count;
    if (count == 0) continue;
    int per;
    if (!common) {
      per = 0;  // every problem its own plan's splits: the single launches' sums, bit for bit
    } else if (count == 1) {
      per = t.p[only].chunks_per_split;  // alone in its family: its own plan
    } else {
      // resident workgroups: the kernel's per-CU count on this device (tuning
      // "wgrad_slots" overrides it, as in plan_wgrad)
      const int G = tuning(kTuneWgradSlots) > 0 ? tuning(kTuneWgradSlots)
                                                : wgrad_family_slots(f) / 256 * std::max(cus, 1);
      // The launch's time in chunk steps: rounds of resident workgroups x
      // (chunks per split + kWgradGroupFixed, a workgroup's prologue and
      // epilogue in chunk steps).  The candidates are the lengths that cut
      // some problem into whole splits, from two rounds' length down to the
      // shortest allowed and up to one split per problem; the cheapest wins,
      // the longer of equals (fewer slabs): totals that just fill whole
      // rounds, walks long enough to amortise the fixed part.
      lo = std::min(lo, longest);
      long long best = -1;
      per = longest;
      for (int i = 0; i < n; ++i) {
        bool seen = t.family[i] != f;  // (a pixel count already tried)
        for (int j = 0; j < i && !seen; ++j)
          seen = t.family[j] == f && t.p[j].nchunks == t.p[i].nchunks;
        if (seen) continue;
        // (as plan_wgrad: at most nchunks / minch splits of the problem itself)
        const int kmax = std::min(maxsplit, std::max(1, t.p[i].nchunks / minch));
        for (int k = 1; k <= kmax; ++k) {
          const int c = (t.p[i].nchunks + k - 1) / k;
          if (c < lo) break;
          const long long w = wgrad_group_wgs(t, f, c);
          const long long cost = (w + G - 1) / G * (c + kWgradGroupFixed);
          if (best < 0 || cost < best || (cost == best && c > per)) best = cost, per = c;
        }
      }
    }
    t.fam[f].chunks_per_split = per;
  }
  // per problem: splits, first workgroup, slab and reduce offsets, in shape order
  int order[kMaxWgradGroup];
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order, order + n,
                   [&](int a, int b) { return wgrad_shape_less(shapes[a], shapes[b]); });
  size_t off = 0;  // floats
  for (int f = 0; f < kWgradFamilies; ++f) {
    WgradGroupFamily& F = t.fam[f];
    if (F.count == 0) continue;
    F.slab_off = off;
    for (int k = 0; k < n; ++k) {
      const int i = order[k];
      if (t.family[i] != f) continue;
      WgradPlan& p = t.p[i];
      if (F.chunks_per_split > 0) {
        p.splits = (p.nchunks + F.chunks_per_split - 1) / F.chunks_per_split;
        p.chunks_per_split = F.chunks_per_split;
      }
      p.part = p.splits > 1;
      p.reduce = p.part ? kReduceFloat4 : kReduceNone;
      p.reduce_grid = 0;
      const ConvShape& s = shapes[i];
      const size_t wsize = (size_t)s.KH * s.KW * s.Cin * s.Cout;
      p.ws_bytes = p.part ? (size_t)p.splits * (wsize + s.Cout) * 4 : 0;
      t.wg0[i] = F.nwg;
      F.nwg += p.ntiles * p.splits;
      if (p.part) {
        t.slab_off[i] = off;
        off += (size_t)p.splits * (wsize + s.Cout);
        t.item0[i] = F.reduce_items;
        F.reduce_items += (long long)(wsize / 4) + s.Cout;
        ++F.reduce_problems;
      }
    }
    F.slab_floats = off - F.slab_off;
    F.reduce_grid = (int)std::min<long long>((F.reduce_items + 255) / 256, 8192);
  }
  t.ws_bytes = off * 4;
  if (t.ws_bytes > workspace_bytes) return 0;  // short workspace: the ungrouped plans
  t.grouped = 1;
  g = t;
  return 0;
}

}  // namespace d2mi
