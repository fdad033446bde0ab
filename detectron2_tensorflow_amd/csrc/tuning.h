// Process-wide kernel-selection knobs (host-only header: no HIP types).
#pragma once

namespace d2mi {

// Process-wide kernel-selection knobs (d2mi_set_tuning; initial values from
// the environment): in-process A/B timing of kernel variants (tools/).
// One line per knob: X(enum id, d2mi_set_tuning key, default).  The enum and
// errors.hip's name and default arrays are generated from this list; the
// environment variable is D2MI_<key in capitals>.
// defaults: measured per shape and in the training step
// conv_stream: the streaming 1x1 for launches of >= 8192 output pixels (r5 in-step A/B:
// -0.85 %, profiles/r5_ab_inproc_conv_stream.log);
// retina_fused: RetinaNet inference in four launches (retina_post.hip; 0 the
// unfused pipeline, 2 the fused one with its in-workgroup exact select forced)
// rpn_merge: the RPN's per-image concat + top-k as a merge rank (proposals.hip)
// solo_mfma: the SOLOv2 Matrix-NMS intersections on int8 MFMA, bits expanded
// by an LDS table (solo.hip); 0 = the AND + popcount tiles;
// retina_var: the r6 RetinaNet post (compaction, early
// select bound, DPP / permlane bitonic and select, NMS IoU only where boxes
// meet, NMS tiles resolved as a ballot fixed point, the floor's radix select,
// the rank launch's rounds looped, small levels' floor samples spread over the
// level: 12018; 0 = the r5 form; + 4096, the rank
// inside the NMS per 128-candidate window, is faster on iid logits and slower
// on a model's head outputs, where the NMS needs several windows)
// conv_split_slots / wgrad_slots: the split-K / pixel-split
// workgroup target (0: the plan's own); conv_tail: 0 no tail split;
// wgrad_occ3_min_p: the pixel count from which the 3-per-CU wgrad runs;
// wgrad_minch / wgrad_maxsplit: fewest chunks per split / most splits (<= 0:
// the default); wgrad_prio: MFMA wave priority; topk_floor: 0 = radix passes only;
// wgrad_group: the folded backbone convs' weight gradients deferred to the
// fold's backward and launched per kernel family (d2mi_conv2d_wgrad_group):
// 1 = each with the pixel splits of its own plan (the bits of the single
// launches), 2 = one chunks-per-split per family (fewer slabs, longer walks,
// other rounding); 0 = each in its own conv's backward
#define D2MI_TUNE_KNOBS(X)                       \
  X(kTuneConvEpi, "conv_epi", 1)                 \
  X(kTuneWgradWS1, "wgrad_ws1", 6)               \
  X(kTuneWgradXCD, "wgrad_xcd", 1)               \
  X(kTuneConvXCD, "conv_xcd", 1)                 \
  X(kTuneConvWSMinK, "conv_ws_mink", 16)         \
  X(kTuneRoiPixGrid, "roi_pix_grid", 8192)       \
  X(kTuneConvStream, "conv_stream", 8192)        \
  X(kTuneRetinaFused, "retina_fused", 1)         \
  X(kTuneRpnMerge, "rpn_merge", 1)               \
  X(kTuneNmsScan, "nms_scan", 1)                 \
  X(kTuneRoiHeavy, "roi_heavy", 16)              \
  X(kTuneRpnCompact, "rpn_compact", 1)           \
  X(kTuneConvStreamNt, "conv_stream_nt", 2)      \
  X(kTuneConvNt, "conv_nt", 0)                   \
  X(kTuneConvTailMinK, "conv_tail_mink", 8)      \
  X(kTuneSgdRev, "sgd_rev", 0)                   \
  X(kTuneRetinaRank, "retina_rank", 0)           \
  X(kTuneSoloMfma, "solo_mfma", 2)               \
  X(kTuneRetinaVar, "retina_var", 12018)         \
  X(kTuneConvSplitSlots, "conv_split_slots", 0)  \
  X(kTuneConvTail, "conv_tail", 1)               \
  X(kTuneWgradOcc3MinP, "wgrad_occ3_min_p", 65536) \
  X(kTuneWgradSlots, "wgrad_slots", 0)           \
  X(kTuneWgradMinCh, "wgrad_minch", 16)          \
  X(kTuneWgradMaxSplit, "wgrad_maxsplit", 128)   \
  X(kTuneWgradPrio, "wgrad_prio", 1)             \
  X(kTuneTopkFloor, "topk_floor", 1)             \
  X(kTuneWgradGroup, "wgrad_group", 1)
enum TuneKey {
#define X(id, key, def) id,
  D2MI_TUNE_KNOBS(X)
#undef X
  kTuneCount
};
int tuning(TuneKey k);

}  // namespace d2mi
