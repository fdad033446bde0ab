// Library-internal host APIs shared between translation units.
#pragma once
#include "common.h"

namespace d2mi {

// Segmented ascending sort of 64-bit keys stored in "capacity layout":
// segment s owns keys[s*cap, s*cap + lens[s]).  Keys beyond lens[s] are
// ignored.  cap <= kLdsSortCap: the in-LDS counting-rank kernel; larger
// capacities: that kernel on kLdsSortCap-key tiles, then merge passes.
constexpr int kLdsSortCap = 8192;
size_t sort_workspace_size(int S, int cap);
int sort_keys_segmented(const uint64_t* keys_in, uint64_t* keys_out, const int32_t* lens, int S,
                        int cap, void* ws, size_t ws_bytes, hipStream_t stream);

// Greedy NMS core over candidates already in capacity layout.
//   keys   [S*cap] sort keys (desc_key(score, local idx)); lens [S]
//   boxes  candidate boxes; candidate i of segment s is at
//          boxes[(box_off ? box_off[s] : s*cap) + i]
//   keep   [S*max_out] local candidate indices, -1 padded; num_keep [S]
size_t nms_core_workspace_size(int S, int cap);
size_t nms_sorted_workspace_size(int S, int cap);
// nms_core's workspace.  d2mi_rpn_proposals_ex lays it out too: its decode
// writes sboxes / idx / count itself and nms_sorted runs on mask_ws.
struct NmsCoreSpace {
  uint64_t* sorted;  // [S*cap] sorted keys
  float4* sboxes;    // [S*cap] boxes in sorted order
  int32_t* idx;      // [S*cap] their local indices
  int32_t* count;    // [S]
  void *mask_ws, *sort_ws;
  size_t mask_bytes, sort_bytes;
  template <typename A>
  void lay(A& a, int S, int cap) {
    sorted = a.template take<uint64_t>((size_t)S * cap);
    sboxes = a.template take<float4>((size_t)S * cap);
    idx = a.template take<int32_t>((size_t)S * cap);
    count = a.template take<int32_t>(S);
    mask_bytes = nms_sorted_workspace_size(S, cap);
    mask_ws = a.template take<char>(mask_bytes);
    sort_bytes = sort_workspace_size(S, cap);
    sort_ws = a.template take<char>(sort_bytes);
  }
};
int nms_core(const uint64_t* keys, const int32_t* lens, const float4* boxes,
             const int32_t* box_off, int S, int cap, int max_out, float iou_thr, int32_t* keep,
             int32_t* num_keep, void* ws, size_t ws_bytes, hipStream_t stream);

// Mask + scan only, over candidates already sorted and gathered in capacity
// layout: sboxes[s*cap + i] (boxes used for IoU, e.g. class-offset boxes),
// sidx[s*cap + i] (the value written to keep for that candidate), count[s]
// selectable candidates.
int nms_sorted(const float4* sboxes, const int32_t* sidx, const int32_t* count, int S, int cap,
               int max_out, float iou_thr, int32_t* keep, int32_t* num_keep, void* ws,
               size_t ws_bytes, hipStream_t stream);

// Exact segmented top-k (value desc, index asc).  See d2mi_topk.
size_t topk_workspace_size(int S, int k);
int topk_core(const float* values, const int64_t* seg_start, const int32_t* seg_len, int S,
              int max_len, int k, int key_mode, float* vals_out, int32_t* idx_out,
              int32_t* count_out, void* ws, size_t ws_bytes, hipStream_t stream);
// seg_k (device, nullable): per-segment k limit (effective k = min(k, seg_k[s], len)).
// sampled_floor (key_mode 1 only): try the one-pass sampled-floor select first
// (topk.hip module comment); the output is the same top-k either way.
int topk_core_ex(const float* values, const int64_t* seg_start, const int32_t* seg_len,
                 const int32_t* seg_k, int S, int max_len, int k, int key_mode, float* vals_out,
                 int32_t* idx_out, int32_t* count_out, void* ws, size_t ws_bytes,
                 hipStream_t stream, bool sampled_floor = false);

// Process-wide kernel-selection knobs (d2mi_set_tuning; initial values from
// the environment): in-process A/B timing of kernel variants (tools/).
// One line per knob: X(enum id, d2mi_set_tuning key, default).  The enum and
// errors.hip's name and default arrays are generated from this list; the
// environment variable is D2MI_<key in capitals>.
// defaults: measured per shape and in the training step
// conv_stream: the streaming 1x1 for launches of >= 8192 output pixels (r5 in-step A/B:
// -0.85 %, profiles/r5_ab_inproc_conv_stream.log); roi_bwd_rec: run records (-0.41 %);
// retina_fused: RetinaNet inference in four launches (retina_post.hip; 0 the
// unfused pipeline, 2 the fused one with its in-workgroup exact select forced)
// rpn_merge: the RPN's per-image concat + top-k as a merge rank (proposals.hip)
// solo_mfma: the SOLOv2 Matrix-NMS intersections on int8 MFMA (solo.hip, r6):
// 2 = bits expanded by an LDS table (default), 1 = by arithmetic, 0 = the AND +
// popcount tiles; retina_var: the r6 RetinaNet post (compaction, early
// select bound, DPP / permlane bitonic and select, NMS IoU only where boxes
// meet, NMS tiles resolved as a ballot fixed point, the floor's radix select,
// the rank launch's rounds looped, small levels' floor samples spread over the
// level: 12018; 0 = the r5 form; + 4096, the rank
// inside the NMS per 128-candidate window, is faster on iid logits and slower
// on a model's head outputs, where the NMS needs several windows)
#define D2MI_TUNE_KNOBS(X)                       \
  X(kTuneConvWS, "conv_ws", 2)                   \
  X(kTuneRoiFwd, "roi_fwd", -1)                  \
  X(kTuneWgradWS, "wgrad_ws", 1)                 \
  X(kTuneConvEpi, "conv_epi", 1)                 \
  X(kTuneWgradWS1, "wgrad_ws1", 6)               \
  X(kTuneWgradXCD, "wgrad_xcd", 1)               \
  X(kTuneConvXCD, "conv_xcd", 1)                 \
  X(kTuneWgradInc, "wgrad_inc", 1)               \
  X(kTuneConvWSMinK, "conv_ws_mink", 16)         \
  X(kTuneRoiPixGrid, "roi_pix_grid", 8192)       \
  X(kTuneConvStream, "conv_stream", 8192)        \
  X(kTuneRoiBwdRec, "roi_bwd_rec", 1)            \
  X(kTuneRetinaFused, "retina_fused", 1)         \
  X(kTuneRpnMerge, "rpn_merge", 1)               \
  X(kTuneNmsScan, "nms_scan", 1)                 \
  X(kTuneRoiHeavy, "roi_heavy", 16)              \
  X(kTuneRpnCompact, "rpn_compact", 1)           \
  X(kTuneConvStreamNt, "conv_stream_nt", 2)      \
  X(kTuneConvNt, "conv_nt", 0)                   \
  X(kTuneConvTailMinK, "conv_tail_mink", 8)      \
  X(kTuneConvWSMinTiles, "conv_ws_mintiles", 0)  \
  X(kTuneSgdRev, "sgd_rev", 0)                   \
  X(kTuneRetinaRank, "retina_rank", 0)           \
  X(kTuneSoloMfma, "solo_mfma", 2)               \
  X(kTuneRetinaVar, "retina_var", 12018)
enum TuneKey {
#define X(id, key, def) id,
  D2MI_TUNE_KNOBS(X)
#undef X
  kTuneCount
};
int tuning(TuneKey k);

// Byte fill by a kernel launch on st (never hipMemsetAsync: errors.hip).
// 0 on success.
int fill_bytes(void* p, size_t nbytes, uint8_t value, hipStream_t st);

}  // namespace d2mi
