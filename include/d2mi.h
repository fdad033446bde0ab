/*
 * d2mi.h — C ABI of libd2mi_hip.so, the MI355X (gfx950) hot path of the
 * detection stack (ROIAlign, batched greedy NMS, anchor/top-k/decode, FPN convs).
 *
 * Every entry point replaces a TensorFlow kernel (or a Python glue function
 * around one) that SimeonZhang/detectron2_tensorflow calls; the replaced
 * reference interface is cited above each declaration as path:line into the
 * reference tree.
 *
 * Conventions (all functions):
 *   - return 0 on success, a negative value on a host-detected argument error
 *     (message in d2mi_last_error(), thread-local);
 *   - every pointer argument named *_dev / listed as "device" is a device
 *     pointer owned by the CALLER (PyTorch allocates inputs, outputs and
 *     workspace; the library never hipMallocs); host arrays are plain host
 *     memory read during the call only;
 *   - `stream` is a hipStream_t passed as void* (torch's current stream);
 *     nothing synchronises, so every call is graph-capturable;
 *   - layouts follow the reference: NHWC activations, HWIO conv weights,
 *     boxes [ymin, xmin, ymax, xmax] (yxyx) in absolute pixels, deltas
 *     (dy, dx, dh, dw) — lib/data/fields.py, lib/layers/convolutional.py:175,
 *     lib/modeling/box_regression.py:53-73.
 *   - run-time data errors the reference raises inside a TF kernel (e.g.
 *     box_ind out of range in CropAndResize) are recorded in a device error
 *     word; d2mi_error_word_dev() returns it so the host can check lazily
 *     without a synchronisation on every call.
 */
#ifndef D2MI_H
#define D2MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2MI_MAX_LEVELS 8

/* ------------------------------------------------------------------ misc */
int d2mi_version(void);
/* sha256 prefix of the sources the library was built from (the csrc .hip
 * and .h files and this header): the loader checks it against its tree. */
const char* d2mi_source_hash(void);
const char* d2mi_last_error(void);
/* Process-wide kernel-selection knobs for in-process A/B timing (tools/);
 * each starts from its environment variable (D2MI_<KEY in capitals>).  No
 * reference counterpart (a tuning hook of this implementation).  Keys:
 *   "conv_epi"     split-K partials stored from the accumulators (1, default)
 *                  or through the LDS epilogue (0);
 *   "wgrad_ws1"    the WS weight gradient on 1x1 convs of >= N GFLOP (6);
 *   "wgrad_xcd" / "conv_xcd"  XCD-contiguous grid remaps (1 on);
 *   "conv_ws_mink" fewest k-steps that go to the WS conv (16);
 *   "roi_pix_grid" ROIAlign backward pixel-pass grid (8192);
 *   "conv_stream"  streaming short-K 1x1 conv (r5) for stride-1 1x1 launches
 *                  of at least this many output pixels; 0 = off;
 *   "retina_fused" RetinaNet post-processing in five launches (1), the same
 *                  with the exact select forced (2), the unfused pipeline (0);
 *   "rpn_merge"    RPN proposals' level merge by merge rank (1) or the one-
 *                  workgroup bitonic sort (0);
 *   "nms_scan"     fixed-point NMS tile resolve when T <= 64 tiles (1);
 *   "roi_heavy"    ROIAlign backward: pixels with >= N runs go first (16);
 *   "rpn_compact"  RPN decode compacts the valid boxes before NMS (1);
 *   "conv_stream_nt" streaming 1x1's output stores non-temporal (2);
 *   "conv_nt"      tiled conv final stores non-temporal (0);
 *   "conv_tail_mink" fewest k-steps whose tail tiles are split along K (8);
 *   "sgd_rev"      SGD update over its chunks in reverse order (0);
 *   "retina_rank"  RetinaNet merge rank inside the NMS workgroup (0);
 *   "solo_mfma"    SOLOv2 Matrix-NMS intersections on int8 MFMA, bits expanded
 *                  by an LDS table (2, default; any non-zero value); 0 = the
 *                  AND + popcount tiles;
 *   "retina_var"   RetinaNet fused-path variants (bits; default 12018, 0 = the
 *                  r5 form): 16 = the wave slots compacted by many workgroups
 *                  before the finish, 64 = the finish's k-th select stopped at
 *                  the first bound leaving <= 1,024 keys, 128 = its bitonic
 *                  exchanges in DPP / permlane lane permutations, 512 = its
 *                  k-th select's reductions and scans the same way, 1024 = the
 *                  NMS's IoU only where the boxes intersect, 2048 = the NMS
 *                  tiles resolved as a ballot fixed point over column words,
 *                  4096 = no rank launch (the NMS ranks each 128-candidate
 *                  window; off by default), 8192 = the floor's ts-th maximum
 *                  by a workgroup radix select, 32 = the rank launch's search
 *                  rounds capped and looped, 2 = a small level's floor
 *                  samples spread over the level, 4 = floor and finish
 *                  launched twice (measurement only);
 *   "conv_split_slots" split-K workgroup target of the convs (0 = the plan's
 *                  own: two per CU, one for the WS conv);
 *   "conv_tail"    tail tiles of a mostly empty last round split along K (1);
 *                  0 = off;
 *   "wgrad_occ3_min_p" the 128x128 split weight gradient runs three workgroups
 *                  per CU from this many pixels up (65536);
 *   "wgrad_slots"  pixel-split workgroup target of the weight gradient (0 =
 *                  the plan's own: 256 / 512 / 768 by kernel);
 *   "wgrad_minch"  fewest 32-pixel chunks per split (16; <= 0 = the default);
 *   "wgrad_maxsplit" most pixel splits (128; <= 0 = the default);
 *   "wgrad_prio"   wave priority 1 while issuing MFMAs in the weight gradient
 *                  (1 on);
 *   "topk_floor"   sampled-floor first pass of the segmented top-k (1); 0 =
 *                  radix passes only;
 *   "wgrad_group"  the folded convs' weight gradients deferred to the fold's
 *                  backward and launched per kernel family
 *                  (d2mi_conv2d_wgrad_group): 1 (default) = every problem keeps
 *                  the pixel splits of its own plan, bit-identical to its
 *                  single launch; 2 = one chunks-per-split per family (few
 *                  slabs, long walks; sums in another order); 0 = each in its
 *                  own backward. */
int d2mi_set_tuning(const char* key, int value);
/* Current value of a d2mi_set_tuning key (INT32_MIN for an unknown key). */
int d2mi_get_tuning(const char* key);
/* Device int32 error word. Bits: 1 = box_ind out of range (CropAndResize),
 * 2 = NMS segment longer than its declared capacity, 4 = top-k capacity,
 * 8 = more non-zero gradient rows than the declared bound (d2mi_row_census). */
int32_t* d2mi_error_word_dev(void);
int d2mi_clear_errors(void* stream);
/* Node census of a captured, not yet instantiated hipGraph (hipGraph_t as
 * void*): counts[t] = nodes of hipGraphNodeType t for t < ntypes (0 kernel,
 * 1 memcpy, 2 memset, ...).  No reference counterpart: the graphed training
 * step (engine/graphed.py, replacing the loop of lib/engine/trainer.py:173-199)
 * checks its captures with it. */
int d2mi_graph_census(void* graph, long long* counts, int ntypes);
/* The same census of the graph `stream` is capturing into now; returns 1
 * (counts 0) when the stream is not capturing.  A diagnosis (tools/). */
int d2mi_capture_census(void* stream, long long* counts, int ntypes);

/* -------------------------------------------------------------- ROIAlign
 * Multi-level ROIAlign / crop_and_resize, one launch for all levels.
 * Replaces:
 *   lib/layers/roi_align.py:45-66       ROIAlign.call (scale, SR crop, avg_pool)
 *   lib/layers/functional.py:100-166    crop_and_resize (SYMMETRIC pad + box transform
 *                                        + tf.image.crop_and_resize bilinear)
 *   lib/modeling/poolers.py:11-49       assign_boxes_to_levels (when num_levels > 1)
 *   lib/modeling/poolers.py:134-180     ROIPooler.call (gather/concat/invert_permutation:
 *                                        output is written directly in input order)
 * feats[l]      device NHWC float [N, H_l, W_l, C] (C equal over levels)
 * dims          host int32 [num_levels][3] = (N, H_l, W_l)
 * scales        host float [num_levels] spatial_scale per level (1/stride)
 * boxes         device float [R,4] yxyx, image pixels (before spatial_scale)
 * box_ind       device int32 [R] image index of each box
 * box_mode      0 = raw normalised boxes (tf.image.crop_and_resize),
 *               1 = aligned fpcoor (ROIAlignV2), 2 = unaligned fpcoor (ROIAlign)
 * assign        1: level per box by the FPN heuristic (min_level..max_level,
 *               canonical_box_size, canonical_level); 0: every box on level 0
 * level_out     device int32 [R] (nullable): assigned level index
 * out           device float [R, out_h, out_w, C]
 */
int d2mi_roi_align_fwd(const float* const* feats, const int32_t* dims, const float* scales,
                       int num_levels, int C, const float* boxes, const int32_t* box_ind,
                       int R, int out_h, int out_w, int sampling_ratio, int box_mode,
                       int pad_border, int assign, int min_level, int max_level,
                       int canonical_box_size, int canonical_level, int32_t* level_out,
                       float* out, void* stream);

/* Gradient of d2mi_roi_align_fwd w.r.t. the feature maps (TF
 * CropAndResizeGradImage + the pad/avg_pool chain rule; boxes get no gradient,
 * lib/layers/functional.py:120). Every element of every grad_feats[l] is
 * WRITTEN (not accumulated; no zero-fill needed): the scatter is computed as a
 * gather — contributions radix-sorted by destination pixel, one wave per pixel
 * summing them in the TF kernel's (box, y, x, corner) order (pixels with more
 * than 64 contributions are split into 64-long partial sums first).
 * Deterministic, no atomics. Workspace from d2mi_roi_align_bwd_workspace_size
 * (same dims / C / R / crop arguments). */
size_t d2mi_roi_align_bwd_workspace_size(const int32_t* dims, int num_levels, int C, int R,
                                         int out_h, int out_w, int sampling_ratio);
int d2mi_roi_align_bwd(float* const* grad_feats, const int32_t* dims, const float* scales,
                       int num_levels, int C, const float* boxes, const int32_t* box_ind,
                       int R, int out_h, int out_w, int sampling_ratio, int box_mode,
                       int pad_border, int assign, int min_level, int max_level,
                       int canonical_box_size, int canonical_level, const float* grad_out,
                       void* workspace, size_t workspace_bytes, void* stream);
/* d2mi_roi_align_bwd_ex with accumulate = 1: the maps already hold another
 * ROI set's gradient of the same features (the box pooler's, when the mask
 * pooler's backward runs second: lib/modeling/roi_heads/roi_heads.py:545-605
 * pool the same p2..p5 twice, and TF's AddN sums the two
 * CropAndResizeGradImage maps); touched pixels become old + new, untouched
 * ones are left unwritten (no clear, no separate add pass). */
int d2mi_roi_align_bwd_ex(float* const* grad_feats, const int32_t* dims, const float* scales,
                          int num_levels, int C, const float* boxes, const int32_t* box_ind,
                          int R, int out_h, int out_w, int sampling_ratio, int box_mode,
                          int pad_border, int assign, int min_level, int max_level,
                          int canonical_box_size, int canonical_level, const float* grad_out,
                          int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* One backward over TWO ROI sets pooled from the same maps -- the box (7x7)
 * and mask (14x14) poolers of a training step (roi_heads.py:497-605), whose
 * CropAndResizeGradImage maps TF sums (AddN): one emit per set, ONE sort on
 * (pixel, set) keys, one gather pass that sums each set's contributions in
 * its TF order and writes set0 + set1 (untouched pixels 0).  Every element
 * of grad_feats is written, except for the levels whose bit is set in
 * accumulate_mask: their maps already hold another gradient of the same
 * features (the RPN head's input gradient, rpn.py:83-96 reading the same
 * p2..p5) and get old + (set0 + set1) at touched pixels only (no clear, no
 * separate add).  Geometry / level parameters are shared; each set has its
 * ROIs, crop size, sampling ratio and grad_out. */
size_t d2mi_roi_align_bwd2_workspace_size(const int32_t* dims, int num_levels, int C, int R0,
                                          int out_h0, int out_w0, int sr0, int R1, int out_h1,
                                          int out_w1, int sr1);
int d2mi_roi_align_bwd2(float* const* grad_feats, const int32_t* dims, const float* scales,
                        int num_levels, int C, int box_mode, int pad_border, int assign,
                        int min_level, int max_level, int canonical_box_size, int canonical_level,
                        const float* boxes0, const int32_t* box_ind0, int R0, int out_h0,
                        int out_w0, int sr0, const float* grad_out0, const float* boxes1,
                        const int32_t* box_ind1, int R1, int out_h1, int out_w1, int sr1,
                        const float* grad_out1, int accumulate_mask, void* workspace,
                        size_t workspace_bytes, void* stream);
/* The same backward in phases (r4).  phase 1 (prepare): every step but the
 * pixel pass -- the counting sort of the contributions by (pixel, set) and
 * the long-run partials -- with the maps of levels [level_lo, level_hi] not
 * in accumulate_mask zeroed; its results stay in the workspace.  phase 2
 * (pixels): the pixel pass over the touched pixels of levels [level_lo,
 * level_hi] only, adding into the maps whose accumulate_mask bit is set
 * (others zeroed first).  phase 3 = d2mi_roi_align_bwd2.  Between a phase 1
 * and its phase-2 calls the workspace must not be reused; a level's map may
 * be null in a phase that does not touch it.  Lets a level's pixel pass run
 * after another backward wrote that map in full (the RPN head conv's dgrad
 * of the same FPN level): no clear of the map, no second pass over it. */
int d2mi_roi_align_bwd2_ex(float* const* grad_feats, const int32_t* dims, const float* scales,
                           int num_levels, int C, int box_mode, int pad_border, int assign,
                           int min_level, int max_level, int canonical_box_size,
                           int canonical_level, const float* boxes0, const int32_t* box_ind0,
                           int R0, int out_h0, int out_w0, int sr0, const float* grad_out0,
                           const float* boxes1, const int32_t* box_ind1, int R1, int out_h1,
                           int out_w1, int sr1, const float* grad_out1, int accumulate_mask,
                           int phase, int level_lo, int level_hi, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------- NMS
 * Segmented greedy NMS with TF NonMaxSuppressionV3 semantics
 * (score_threshold = -inf; IoU with min/max-normalised corners, 0 when an
 * area <= 0; suppress when IoU > iou_threshold; score desc, ties lowest index
 * first; stop at max_output_size).
 * Replaces tf.image.non_max_suppression at lib/layers/nms.py:23 (batch_nms),
 * lib/modeling/proposal_generator/rpn_outputs.py:90,
 * lib/modeling/roi_heads/fast_rcnn.py:145, single_stage_heads/retinanet.py:353.
 * boxes [total,4], scores [total] device; seg_offsets device int32 [num_segs+1];
 * seg_capacity = host upper bound of any segment length.
 * keep device int32 [num_segs, max_out] (segment-relative indices in selection
 * order, -1 padded); num_keep device int32 [num_segs].
 */
size_t d2mi_nms_workspace_size(int num_segs, int seg_capacity);
int d2mi_nms(const float* boxes, const float* scores, const int32_t* seg_offsets, int num_segs,
             int seg_capacity, int max_out, float iou_threshold, int32_t* keep,
             int32_t* num_keep, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------ top-k (segmented)
 * Exact segmented top-k with TF TopKV2 sorted=True order (value desc, ties
 * lowest index first).  key_mode 0: keys are the values; 1: keys are
 * sigmoid(values) (RetinaNet, retinanet.py:321-326); values_out receives the keys.
 * Segment s = values[seg_start[s] : seg_start[s] + seg_len[s]] (device int64
 * start, int32 len).  Replaces tf.nn.top_k at rpn_outputs.py:70/:106,
 * retinanet.py:326.  Output idx is segment-relative. */
size_t d2mi_topk_workspace_size(int num_segs, int k_max);
int d2mi_topk(const float* values, const int64_t* seg_start, const int32_t* seg_len,
              int num_segs, int max_seg_len, int k, int key_mode, float* values_out,
              int32_t* idx_out, int32_t* count_out, void* workspace, size_t workspace_bytes,
              void* stream);

/* ---------------------------------------------------------- subsampling
 * subsample_labels (lib/modeling/sampling.py, called at rpn_outputs.py:278-283
 * and roi_heads.py:160-216) over labels [N, P] int64: pos_out / neg_out [N, P]
 * (uint8) mark a uniformly random min(num_pos, #positive) of the positives
 * (label not -1 and not bg_label) and min(num_samples - that, #negative) of
 * the negatives (label == bg_label).  The draw: each element's rank among its
 * kind through a keyed pseudo-random bijection of [0, n), kept iff < k (the
 * reference shuffles and takes the first k: the same distribution, another
 * stream); seed [1] int64 on the device.  order_out [N, S] (nullable, with
 * order_valid [N, S] uint8): the selected indices positives first, each kind
 * in index order, then 0 / invalid -- the ROI heads' fg-first batch. */
size_t d2mi_subsample_workspace_size(int N, int P);
int d2mi_subsample(const int64_t* labels, int N, int P, long long bg_label, int num_samples,
                   int num_pos, const int64_t* seed, uint8_t* pos_out, uint8_t* neg_out,
                   int64_t* order_out, uint8_t* order_valid, int S, void* workspace,
                   size_t workspace_bytes, void* stream);

/* -------------------------------------------------------- anchors/deltas
 * DefaultAnchorGenerator.grid_anchors for one level (anchor_generator.py:92-109):
 * out[(h*W + w)*A + a] = cell[a] + (h*stride, w*stride, h*stride, w*stride).
 * 1 <= A <= 15 (5 sizes x 3 aspect ratios: the single-level C4 / DC5 RPNs);
 * the same bound holds for d2mi_rpn_proposals[_ex] and the RetinaNet entries. */
int d2mi_grid_anchors(int H, int W, float stride, const float* cell_anchors_host, int A,
                      float* out, void* stream);

/* Box2BoxTransform.apply_deltas (box_regression.py:76-123):
 * deltas [N, K*4] (dy,dx,dh,dw), boxes [N,4] -> out [N, K*4]. */
int d2mi_apply_deltas(const float* deltas, const float* boxes, int N, int K,
                      const float* weights4_host, float scale_clamp, float* out, void* stream);

/* ------------------------------------------------------ RPN proposals
 * Fused find_top_rpn_proposals (rpn_outputs.py:29-132) +
 * predict_proposals (:403-426) + anchors (anchor_generator.py:92-109):
 * per (image, level) exact top-k of the objectness logits, decode ONLY the
 * selected anchors (anchors regenerated from the index), clip to the image,
 * prune small boxes, per-level NMS, then per-image top-k(post) and zero pad.
 * logits[l]  device float [N, H_l, W_l, A]; deltas[l] device [N, H_l, W_l, A*4]
 * level_hw   host int32 [L][2]; strides host float [L]; cell_anchors host [L][A][4]
 * image_hw   device int32 [N,2] (true image height, width)
 * out_boxes  device [N, post, 4]; out_scores [N, post]; out_valid uint8 [N, post]
 * 1 <= A <= 15.  k = min(pre_nms_topk, max_l H_l W_l A) <= 16384.  k <= 8192
 * runs the radix select (d2mi_topk's); above it (the single-level C4 / DC5
 * RPNs in training: 12000 of up to 63,000 anchors) every (image, level)
 * segment is sorted whole -- keys, the tiled and merged segmented sort, the
 * first k kept -- with the same order: score descending, ties to the lowest
 * index, NaN and -inf never selected.  The workspace query covers both.
 */
size_t d2mi_rpn_proposals_workspace_size(int N, int L, const int32_t* level_hw, int A,
                                         int pre_nms_topk, int post_nms_topk);
int d2mi_rpn_proposals(const float* const* logits, const float* const* deltas,
                       const int32_t* level_hw, const float* strides,
                       const float* cell_anchors, int L, int A, int N, const int32_t* image_hw,
                       int pre_nms_topk, int post_nms_topk, float nms_thresh,
                       float min_box_side_len, const float* weights4_host, float scale_clamp,
                       float* out_boxes, float* out_scores, uint8_t* out_valid,
                       void* workspace, size_t workspace_bytes, void* stream);
/* d2mi_rpn_proposals over strided levels: level l of image n starts
 * logits_image_stride[l] elements (deltas: deltas_image_stride[l], a multiple
 * of 4) after image n - 1's, i.e. per-level views of ONE concatenated
 * [N, sum_l H_l W_l A] (x4) buffer -- the training path's RPN head output
 * (d2mi_rpn_head_gather), with no per-level copies.  Null strides: dense. */
int d2mi_rpn_proposals_ex(const float* const* logits, const float* const* deltas,
                          const int64_t* logits_image_stride, const int64_t* deltas_image_stride,
                          const int32_t* level_hw, const float* strides,
                          const float* cell_anchors, int L, int A, int N, const int32_t* image_hw,
                          int pre_nms_topk, int post_nms_topk, float nms_thresh,
                          float min_box_side_len, const float* weights4_host, float scale_clamp,
                          float* out_boxes, float* out_scores, uint8_t* out_valid,
                          void* workspace, size_t workspace_bytes, void* stream);
/* RPN head outputs of a training step in the RPNOutputs layout
 * (rpn_outputs.py:346-357: per-image level-major concatenation): ys[l]
 * device [N, HW_l, C] (the fused objectness / anchor-delta 1x1 output,
 * C >= 5A channels: A logits then 4A deltas, the rest padding) ->
 * logits [N, T*A], deltas [N, T*A, 4], T = sum_l HW_l.  One launch instead
 * of a slice copy per level and head and two concatenations. */
int d2mi_rpn_head_gather(const float* const* ys, const int32_t* level_hw_flat, int L, int N,
                         int A, int C, float* logits, float* deltas, void* stream);
/* Its adjoint: g_logits [N, T*A], g_deltas [N, T*A, 4] (either nullable =
 * zero) -> gys[l] [N, HW_l, C], every element written (padding channels 0). */
int d2mi_rpn_head_scatter(const float* g_logits, const float* g_deltas,
                          const int32_t* level_hw_flat, int L, int N, int A, int C,
                          float* const* gys, void* stream);

/* --------------------------------------------------- Fast R-CNN inference
 * FastRCNNOutputs.predict_boxes/predict_probs + fast_rcnn_inference
 * (fast_rcnn.py:28-187, :359-379): softmax, class-specific decode, clip to the
 * true image shape, score > thresh in class-major order, class-offset NMS
 * (offset = cls * (max clipped coord of the image + 1)), top-k, pad.
 * logits [R, K+1] (background last), deltas [R, K*4] (or [R,4] when
 * bit 0 of cls_agnostic is set), proposals [R,4]; bit 1 of cls_agnostic =
 * NMS_CLS_AGNOSTIC (fast_rcnn.py:138-139: plain NMS, no class offsets); roi_img/roi_slot int32 [R] = (image, dense
 * slot) of each ROI (SparseBoxList.indices); P = dense slots per image.
 * Outputs [N, max_det] boxes/scores/classes(int64)/valid(uint8) and
 * out_roi int32 [N, max_det] (kept ROI row, -1 pad).
 */
size_t d2mi_fast_rcnn_workspace_size(int N, int P, int K, float score_thresh, int max_det);
int d2mi_fast_rcnn_inference(const float* logits, const float* deltas, const float* proposals,
                             const int32_t* roi_img, const int32_t* roi_slot, int R, int N, int P,
                             int K, int cls_agnostic, const int32_t* image_hw,
                             const float* weights4_host, float scale_clamp, float score_thresh,
                             float nms_thresh, int max_det, float* out_boxes, float* out_scores,
                             int64_t* out_classes, uint8_t* out_valid, int32_t* out_roi,
                             void* workspace, size_t workspace_bytes, void* stream);
/* d2mi_fast_rcnn_inference on the scores of a cascade averaged over its
 * stages (cascade_rcnn.py:123-139): logits0..logits3 [R, K+1], the first
 * num_stages (1..4) of them used, the others null.  Each stage's softmax in
 * the single-stage order, summed left to right and multiplied by the f32
 * value of 1.0 / num_stages; deltas / weights4_host are the last stage's.
 * Same workspace (d2mi_fast_rcnn_workspace_size); num_stages = 1 gives
 * d2mi_fast_rcnn_inference's outputs bit for bit. */
int d2mi_fast_rcnn_inference_stages(const float* logits0, const float* logits1,
                                    const float* logits2, const float* logits3, int num_stages,
                                    const float* deltas, const float* proposals,
                                    const int32_t* roi_img, const int32_t* roi_slot, int R, int N,
                                    int P, int K, int cls_agnostic, const int32_t* image_hw,
                                    const float* weights4_host, float scale_clamp,
                                    float score_thresh, float nms_thresh, int max_det,
                                    float* out_boxes, float* out_scores, int64_t* out_classes,
                                    uint8_t* out_valid, int32_t* out_roi, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* --------------------------------------------------- RetinaNet inference
 * RetinaNetHead.inference (retinanet.py:285-387): per level sigmoid,
 * top_k(min(topk_candidates, H*W*A*K)), score > thresh, decode the chosen
 * anchors (no clipping), concat levels, class-offset NMS, pad to max_det.
 * cls[l] device [N, H_l, W_l, A*K]; box[l] device [N, H_l, W_l, A*4].
 */
size_t d2mi_retinanet_workspace_size(int N, int L, const int32_t* level_hw, int A, int K,
                                     int topk_candidates);
int d2mi_retinanet_inference(const float* const* cls, const float* const* box,
                             const int32_t* level_hw, const float* strides,
                             const float* cell_anchors, int L, int A, int K, int N,
                             int topk_candidates, float score_thresh, float nms_thresh,
                             int max_det, const float* weights4_host, float scale_clamp,
                             float* out_boxes, float* out_scores, int32_t* out_classes,
                             uint8_t* out_valid, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ----------------------------------------------------------------- YOLOv4
 * Host arrays shared by the two entry points below: level_hw [L][2];
 * strides [L]; cell_hw [L][A][2], the (h, w) of anchor_generator.py:240-243's
 * [0, 0, height, width] cell anchors; scale_yx [L][2], MODEL.YOLOV4.SCALE_YX
 * and 0.5 * (SCALE_YX - 1), each formed in double and rounded to f32 as the
 * reference's Python scalars are.  logits[l] device [N, H_l, W_l, A*(5+K)],
 * a row being (dy, dx, dh, dw, conf, K class logits).  The P = sum(H_l W_l A)
 * predictions of an image are level-major, then (h, w, a).
 *
 * YOLOV4Outputs._get_predictions (yolov4_outputs.py:208-264) without the
 * [N, P, K] probability tensor: out_boxes [N, P, 4] (no clamp, no clip),
 * out_conf [N, P] = sigmoid(conf), out_score [N, P] = max_c(sigmoid(conf) *
 * sigmoid(prob_c)), out_cls [N, P] the lowest class attaining it. */
int d2mi_yolov4_predictions(const float* const* logits, const int32_t* level_hw,
                            const float* strides, const float* cell_hw, const float* scale_yx,
                            int L, int A, int K, int N, float* out_boxes, float* out_conf,
                            float* out_score, int32_t* out_cls, void* stream);
/* YOLOV4Outputs.inference (yolov4_outputs.py:331-390) per image: predictions
 * with score > score_thresh in prediction order, class-agnostic
 * NonMaxSuppressionV3 on the max-class scores (score descending, ties lowest
 * index first, at most max_det <= 1000), gather, zero padding to max_det
 * with out_valid 0.  The same decode / score functions as
 * d2mi_yolov4_predictions.  Launches: score, compact, sort (1 - 3), NMS; no
 * host synchronisation.  The workspace is linear in N * P. */
size_t d2mi_yolov4_workspace_size(int N, int L, const int32_t* level_hw, int A);
int d2mi_yolov4_inference(const float* const* logits, const int32_t* level_hw,
                          const float* strides, const float* cell_hw, const float* scale_yx,
                          int L, int A, int K, int N, float score_thresh, float nms_thresh,
                          int max_det, float* out_boxes, float* out_scores, int32_t* out_classes,
                          uint8_t* out_valid, void* workspace, size_t workspace_bytes,
                          void* stream);
/* SPP.call's three stride-1 max pools and concat (necks/yolov4.py:171-182;
 * MaxPool2D pads with zeros, layers/wrappers.py:119-131, then pools VALID, so
 * a tap outside the map counts as 0): x [N, H, W, C] -> out [N, H, W, 4C] =
 * [pool13, pool9, pool5, x], C % 4 == 0, one launch. */
int d2mi_spp_pool(const float* x, int N, int H, int W, int C, float* out, void* stream);
/* In-place elementwise activation over n floats (lib/layers/activation.py):
 * code 1 = leaky_relu(alpha) (:16-17), code 2 = mish, x * tanh(softplus(x))
 * (:5-7). */
int d2mi_activation(float* x, int64_t n, int code, float alpha, void* stream);

/* -------------------------------------------------------- YOLOv4 training
 * The host arrays, the logits layout and the prediction order of the YOLOv4
 * section above; L = 3, any K >= 1, any G >= 0.  Device arrays: gt_boxes
 * [N, G, 4] yxyx (16-byte aligned), gt_classes [N, G] int64, valid [N, G]
 * bytes = is_valid & ~crowd & ~difficult (yolov4_outputs.py:77-80).
 *
 * YOLOV4Outputs._get_ground_truth's assignment (yolov4_outputs.py:86-146,
 * YOLOMatcher's argmax, matcher.py:233) and the slot collisions of its
 * sparse.to_dense scatters (:155-196): for every valid GT the first maximum
 * of the L * A plain IoUs of [0, 0, h / stride_l, w / stride_l] against level
 * l's cell anchors in pixels, level = best / A, anchor = best % A, cell =
 * floor(centre / stride_level).  slot [N, G]: the flat prediction index, -1
 * for a GT that is not valid or whose cell is outside the grid.  owner
 * [N, P]: the highest GT index whose slot the prediction is (the target box
 * the scatter leaves), -1 where none.  Two launches (owner's clear, the
 * assignment); no memset node. */
int d2mi_yolov4_assign(const int32_t* level_hw, const float* strides, const float* cell_hw, int L,
                       int A, int N, const float* gt_boxes, const uint8_t* valid, int G,
                       int32_t* slot, int32_t* owner, void* stream);
/* YOLOV4Outputs.losses (yolov4_outputs.py:266-329) before its 1 / N and
 * CLS_NORMALIZER / N factors, with the negatives of YOLOMatcher
 * (matcher.py:223-242: max over the valid GT of pairwise CIoU(GT, predicted
 * box), box_list_ops.py:295-372, below iou_threshold; none in an image without
 * a valid GT) and iou_loss "ciou" on matched_iou(prediction, GT)
 * (loss.py:140-196, box_list_ops.py:375-450, width2 = x_max1 - x_min2 kept).
 * partial [N * d2mi_yolov4_loss_blocks()][5] float64: per-workgroup sums (the
 * float32 terms added in float64) of
 *   0  (respond_bbox - sigmoid(conf))^2 * BCE(conf) over positives and negatives
 *   1  BCE(class logits, multi-hot of the slot's GT classes) over positives
 *   2  (2 - gt_area / image_area) * iou_normalizer / N * (1 - ciou) over positives
 *   3, 4  the positives and the negatives counted
 * to be added in a fixed order by the caller.  state [N, P] bytes: 0 neither,
 * 1 negative, 2 positive.  One launch. */
int d2mi_yolov4_loss_blocks(void);
int d2mi_yolov4_loss_fwd(const float* const* logits, const int32_t* level_hw, const float* strides,
                         const float* cell_hw, const float* scale_yx, int L, int A, int K, int N,
                         const float* gt_boxes, const int64_t* gt_classes, const uint8_t* valid,
                         int G, const int32_t* slot, const int32_t* owner, float image_area,
                         float iou_threshold, float iou_normalizer, double* partial,
                         uint8_t* state, void* stream);
/* The gradient of conf_scale * sum 0, cls_scale * sum 1 and sum 2 above with
 * respect to every logit, times the upstream gradients *g_conf, *g_cls, *g_box
 * (device scalars; null = 0): what TF differentiates, the focal factor, alpha
 * and v of the CIoU, width2 and the decode included; nothing through the
 * targets.  EVERY element of every d_logits[l] is written (zeros where the
 * loss does not reach).  One launch, no float atomics. */
int d2mi_yolov4_loss_bwd(const float* const* logits, float* const* d_logits,
                         const int32_t* level_hw, const float* strides, const float* cell_hw,
                         const float* scale_yx, int L, int A, int K, int N, const float* gt_boxes,
                         const int64_t* gt_classes, int G, const int32_t* slot,
                         const int32_t* owner, const uint8_t* state, float image_area,
                         float iou_normalizer, float conf_scale, float cls_scale,
                         const float* g_conf, const float* g_cls, const float* g_box,
                         void* stream);

/* ------------------------------------------------------------ Matrix NMS
 * lib/layers/nms.py:29-83 (SOLOv2 Matrix-NMS).  masks [M, HW] float,
 * classes int64 [M], scores [M], sum_masks [M] (nullable: computed);
 * kernel 0 = gaussian, 1 = linear.  out_scores [M]. */
size_t d2mi_matrix_nms_workspace_size(int M);
int d2mi_matrix_nms(const float* masks, const int64_t* classes, const float* scores,
                    const float* sum_masks, int M, int HW, int kernel, float sigma,
                    float* out_scores, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------- ResizeBilinear
 * tf.compat.v2.image.resize(method="bilinear") as the reference's
 * resize_images calls it (lib/layers/functional.py:9-36; TF >= 1.14 takes the
 * v2 branch, which drops align_corners: half-pixel centres, no antialias),
 * TF 1.15 resize_bilinear_op.cc arithmetic.  x [N,H,W,C] -> y [N,OH,OW,C]. */
int d2mi_resize_bilinear(const float* x, int N, int H, int W, int C, int OH, int OW,
                         int align_corners, int half_pixel_centers, float* y, void* stream);

/* ------------------------------------------------- SOLOv2 inference tail
 * MaskKernelBranch.inference (lib/modeling/single_stage_heads/solo_v2.py:476-627)
 * in four stages around the caller's dynamic-conv GEMM and d2mi_matrix_nms.
 *
 * d2mi_solo_cells: cate[l] device float [N, S_l, S_l, K] category logits
 * (grids host int32 [L] = S_l, T = sum S_l^2 cells) -> probs [N, T, K] =
 * point_nms(sigmoid(cate)) (solo_v2.py:29-40, :267-269) in the reference's
 * flattened order (:567-586); live_cells [N, T]: the cells with any prob >
 * score_thr in cell order, first live_count[n] valid; live_row [N, T]: a live
 * cell's position in live_cells, -1 otherwise.  cate is a host array of L
 * device pointers. */
int d2mi_solo_cells(const float* const* cate, const int32_t* grids, int L, int N, int K,
                    float score_thr, float* probs, int32_t* live_cells, int32_t* live_row,
                    int32_t* live_count, void* stream);

/* d2mi_solo_mask_stats: logits [R, P] (one dynamic-conv row per live cell,
 * :509-511) -> sum_masks[r] = #(sigmoid > mask_thr) (:513-517) and
 * sum_scores[r] = sum of those sigmoids (:529-531).  16-B aligned. */
int d2mi_solo_mask_stats(const float* logits, int R, int P, float mask_thr, float* sum_masks,
                         float* sum_scores, void* stream);

/* d2mi_solo_select: candidates (cell, class) with prob > score_thr and
 * sum_masks > stride of the cell's level (:482-526), scored prob *
 * sum_scores / sum_masks (:528-532); exact top-k (k = TOPK_CANDIDATES_TEST,
 * tf.nn.top_k sorted, ties by candidate order, :535-539); the top-k's binary
 * masks bit-packed, mask_bits [N, k, ceil(P/64)] uint64 (bit p % 64 of word
 * p / 64), classes [N, k] int64 (rows past top_count: zero masks, classes
 * -1 - t), sum_masks [N, k], scores [N, k] (:537-539).  row_off [N] device:
 * first logits row of each image; grids / strides host [L]. */
size_t d2mi_solo_select_workspace_size(int N, int T, int K, int k);
int d2mi_solo_select(const float* probs, const int32_t* live_row, const int32_t* row_off,
                     const float* logits, const float* sum_masks, const float* sum_scores,
                     const int32_t* grids, const float* strides, int L, int N, int K, int P,
                     float score_thr, float mask_thr, int k, float* top_scores,
                     int64_t* top_classes, float* top_sum_masks, int32_t* top_count,
                     uint64_t* mask_bits, void* workspace, size_t workspace_bytes, void* stream);

/* d2mi_solo_matrix_nms: matrix_nms (lib/layers/nms.py:29-83, called at
 * solo_v2.py:541-545) for N images of k binary masks at once: the
 * intersection matrix M M^T as popcounts of AND-ed mask words (exact), then
 * the IoU / class / compensation / decay arithmetic of d2mi_matrix_nms.
 * kernel 0 = gaussian, 1 = linear.  out_scores [N, k]. */
size_t d2mi_solo_matrix_nms_workspace_size(int N, int k);
int d2mi_solo_matrix_nms(const uint64_t* mask_bits, const int64_t* classes, const float* scores,
                         const float* sum_masks, int N, int k, int P, int kernel, float sigma,
                         float* out_scores, void* workspace, size_t workspace_bytes,
                         void* stream);

/* d2mi_solo_finalize: decayed Matrix-NMS scores [N, k] > update_thr in
 * candidate order, pad / clip to max_det (:547-557); the bit-packed masks
 * resized from [Hm, Wm] to the padded image [OH, OW] with TF bilinear
 * (half-pixel) and > mask_thr (:598-602) -> out_masks uint8
 * [N, max_det, OH, OW] (the reference's float 0/1 values); out_boxes
 * [N, max_det, 4] from the masks (:604-623); out_scores, out_classes int64,
 * out_valid uint8 [N, max_det]. */
size_t d2mi_solo_finalize_workspace_size(int N, int max_det, int OH);
int d2mi_solo_finalize(const float* nms_scores, const int64_t* top_classes,
                       const int32_t* top_count, const uint64_t* mask_bits, int N, int k, int Hm,
                       int Wm, float update_thr, int max_det, float mask_thr, int OH, int OW,
                       uint8_t* out_masks, float* out_boxes, float* out_scores,
                       int64_t* out_classes, uint8_t* out_valid, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------- GroupNorm
 * GroupNorm.call (lib/layers/normalization.py:235-260) on NHWC x [N,H,W,C]:
 * tf.nn.moments over (H, W, C/G) (two-pass mean / variance), then
 * y = x * inv + (beta - mean * inv), inv = rsqrt(var + eps) * gamma;
 * relu: max(y, 0) (the conv's activation after its normalizer,
 * convolutional.py:251-262); up2: y written to the 2x2 block of the nearest
 * x2 upsample (out [N,2H,2W,C], wrappers.py:104-116); accumulate: y added to
 * the output (the SOLOv2 scale-head sum, solo_v2.py:705-721).  C / G % 4 == 0,
 * C <= 1024, G <= 64, 16-B aligned; workspace from
 * d2mi_group_norm_workspace_size. */
size_t d2mi_group_norm_workspace_size(int N, int H, int W, int C, int G);
int d2mi_group_norm_nhwc(const float* x, int N, int H, int W, int C, int G, const float* gamma,
                         const float* beta, float eps, int relu, int up2, int accumulate,
                         float* y, void* workspace, size_t workspace_bytes, void* stream);
/* The same GroupNorm (+ relu) applied to up to 6 feature levels sharing the
 * layer — the SOLOv2 towers' per-level GroupNorm calls (solo_v2.py:173-183,
 * one layer per level) — in five launches for all levels.  xs[l] / ys[l]
 * [dims[3l], dims[3l+1], dims[3l+2], C]; per level identical arithmetic to
 * d2mi_group_norm_nhwc; workspace from d2mi_group_norm_levels_workspace_size. */
size_t d2mi_group_norm_levels_workspace_size(const int32_t* dims, int nlev, int C, int G);
int d2mi_group_norm_nhwc_levels(const float* const* xs, const int32_t* dims, int nlev, int C,
                                int G, const float* gamma, const float* beta, float eps, int relu,
                                float* const* ys, void* workspace, size_t workspace_bytes,
                                void* stream);
/* GroupNorm.call with a gradient, forward (lib/layers/normalization.py:174-260:
 * the layer's variables, tf.nn.moments and tf.nn.batch_normalization as TF
 * differentiates them): y [N,H,W,C] as d2mi_group_norm_nhwc writes it (the same
 * passes and chunking: the same bits; no up2 / accumulate), and the batch
 * moments mean / var [N, G] (biased, two-pass) to caller tensors for the
 * backward.  C / G % 4 == 0, C <= 2048 (C / 4 > 256: the channel quads in
 * tiles of 256), G <= 64, N <= 65535, 16-B aligned; N == 0 launches nothing.
 * One call launches all five passes; workspace from
 * d2mi_group_norm_train_fwd_workspace_size. */
size_t d2mi_group_norm_train_fwd_workspace_size(int N, int H, int W, int C, int G);
int d2mi_group_norm_train_fwd(const float* x, int N, int H, int W, int C, int G,
                              const float* gamma, const float* beta, float eps, int relu,
                              float* y, float* mean, float* var, void* workspace,
                              size_t workspace_bytes, void* stream);
/* The gradient of the above (lib/layers/normalization.py:174-260 under
 * tf.gradients), from x, dy [N,H,W,C], the forward's mean / var and gamma /
 * beta; no saved y.  With r = rsqrt(var + eps), xh = (x - mean) * r,
 * m = H*W*C/G and dz = dy where the fused ReLU passed (relu: the mask is
 * z > 0 of z recomputed by the forward's expression; else dz = dy):
 *   dbeta_c = sum_{n,hw} dz,  dgamma_c = sum_{n,hw} dz * xh,
 *   S1 = sum_{hw, c in g} dz * gamma_c,  S2 = sum_{hw, c in g} dz * gamma_c * xh,
 *   dx = r * (dz * gamma_c - S1 / m - xh * S2 / m).
 * A reduce pass (per image, pixel chunk and channel), two small finalize
 * launches (per image: its chunks; then S1 / S2 per image and dgamma / dbeta
 * over the images) and an apply pass, all from this one call; fixed-order sums, no
 * atomics, every output element written.  dx [N,H,W,C], dgamma / dbeta [C]
 * are each nullable: a null output and the pass that only serves it are
 * skipped.  Sizes as the forward; workspace from
 * d2mi_group_norm_train_bwd_workspace_size. */
size_t d2mi_group_norm_train_bwd_workspace_size(int N, int H, int W, int C, int G);
int d2mi_group_norm_train_bwd(const float* x, const float* dy, int N, int H, int W, int C, int G,
                              const float* mean, const float* var, const float* gamma,
                              const float* beta, float eps, int relu, float* dx, float* dgamma,
                              float* dbeta, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ------------------------------------------- BatchNorm, batch statistics
 * The training form of BatchNorm.call (lib/layers/normalization.py:97-119:
 * tf.layers.BatchNormalization(...).apply(inputs, training=True); the SyncBN
 * branch :121-165 is the same with the moments of all replicas) on x [M, C]
 * f32, M = N*H*W rows of an NHWC tensor (or the rows of [R, C]).  C % 4 == 0,
 * every tensor 16-byte aligned, M >= 1.  Deterministic: fixed-order
 * reductions, no atomics.
 *
 * d2mi_bn_train_stats: one read of x.  Per row chunk and channel a
 * (count, mean, M2) triple by Welford's update, merged in chunk order by the
 * parallel-variance formula into triple [2C + 1] = (count, mean[C], M2[C]),
 * M2 = sum (x - mean)^2.  Workspace from d2mi_bn_train_stats_workspace_size. */
size_t d2mi_bn_train_stats_workspace_size(long long M, int C);
int d2mi_bn_train_stats(const float* x, long long M, int C, float* triple, void* workspace,
                        size_t workspace_bytes, void* stream);
/* Merges P triples (rows of [P, 2C + 1]: one locally, one per rank under
 * SyncBN, normalization.py:121-165) in row order, weighted by their counts:
 * mean [C], var [C] = M2 / count (biased, as tf.layers.BatchNormalization
 * feeds its moving average) and invstd [C] = 1 / sqrt(var + eps), and
 *   moving = moving * decay + batch * (1 - decay)    (assign_moving_average)
 * in place on moving_mean / moving_var [C] (both required). */
int d2mi_bn_train_finalize(const float* triples, int P, int C, float eps, float decay,
                           float* moving_mean, float* moving_var, float* mean, float* var,
                           float* invstd, void* stream);
/* y = (x - mean) * invstd * gamma + beta  (normalization.py:97-119;
 * gamma / beta nullable: scale=False / center=False) with the ops that follow
 * it in a conv fused (convolutional.py:251-262, blocks.py:143-186):
 *   relu_mode 0: y = z (+ residual);  1: y = relu(z) (+ residual);
 *   relu_mode 2: y = relu(z + residual).   residual [M, C], nullable. */
int d2mi_bn_train_apply(const float* x, long long M, int C, const float* mean,
                        const float* invstd, const float* gamma, const float* beta,
                        const float* residual, int relu_mode, float* y, void* stream);
/* Backward, first pass (the gradient of normalization.py:97-119): with dz the
 * gradient at the BatchNorm output (dy through the fused ReLU: relu_mode 1
 * recomputes z from x as the forward did, relu_mode 2 reads y [M, C]) and
 * xh = (x - mean) * invstd:  sums [2C] = (sum dz [C], sum dz * xh [C]) over
 * this call's rows (dbeta and dgamma).  Workspace from
 * d2mi_bn_train_bwd_reduce_workspace_size. */
size_t d2mi_bn_train_bwd_reduce_workspace_size(long long M, int C);
int d2mi_bn_train_bwd_reduce(const float* x, const float* dy, const float* y, long long M, int C,
                             const float* mean, const float* invstd, const float* gamma,
                             const float* beta, int relu_mode, float* sums, void* workspace,
                             size_t workspace_bytes, void* stream);
/* Backward, second pass: sums [2C] as above over ALL rows the statistics were
 * taken over (every replica's under SyncBN), total_count their number:
 *   dx = gamma * invstd * (dz - sums[c] / total - xh * sums[C + c] / total)
 * and dresidual [M, C] = dz (nullable: no residual). */
int d2mi_bn_train_bwd_apply(const float* x, const float* dy, const float* y, long long M, int C,
                            const float* mean, const float* invstd, const float* gamma,
                            const float* beta, int relu_mode, const float* sums,
                            float total_count, float* dx, float* dresidual, void* stream);

/* --------------------------------------------------------------- conv2d
 * NHWC implicit-GEMM convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32),
 * lib/layers/convolutional.py:12-23 (fix_padding: symmetric pad) and
 * :198-263 (Conv2D.call: conv + bias + activation), with the FPN top-down
 * merge fused into the epilogue (lib/modeling/necks/fpn.py:138-149):
 *   y = act(conv(x, w) + bias) + (topdown ? up2_nearest(topdown) : 0)
 *        [+ residual]
 * x [N,H,W,Cin]; w_packed [KH,KW,Cout,Cin] (d2mi_conv_pack_weights of the
 * reference's HWIO [KH,KW,Cin,Cout] variable); bias [Cout] (nullable);
 * topdown [N, ceil(OH/2), ceil(OW/2), Cout] (nullable);
 * residual [N,OH,OW,Cout] (nullable); y [N,OH,OW,Cout].
 * act: 0 none, 1 relu.  pad_beg/pad_end: explicit spatial padding
 * (fix_padding gives pad_beg = (k-1)//2, pad_end = k-1-pad_beg).
 */
int d2mi_conv_pack_weights(const float* w_hwio, int KH, int KW, int Cin, int Cout,
                           float* w_packed, void* stream);

/* d2mi_conv_pack_weights_many: n weight tensors (w_hwio[i], dims[4i..4i+3] =
 * KH, KW, Cin, Cout) packed as d2mi_conv_pack_weights does, the Cin % 64 == 0
 * ones by one launch per 32 tensors (the per-step repack of every
 * un-normalised conv after the optimizer update: FPN, RPN, ROI heads,
 * convolutional.py:198-263's weights).  Host arrays of device pointers. */
int d2mi_conv_pack_weights_many(int n, const float* const* w_hwio, const int32_t* dims,
                                float* const* w_packed, void* stream);
int d2mi_conv2d_nhwc(const float* x, const float* w_packed, const float* bias,
                     const float* topdown, const float* residual, float* y, int N, int H, int W,
                     int Cin, int Cout, int KH, int KW, int stride, int pad_beg, int pad_end,
                     int act, void* stream);
/* Extended form: flags bit0 = ReLU, bit1 = apply the ReLU after the
 * residual / top-down add (ResNet bottleneck: relu(conv3 + bias + shortcut),
 * lib/modeling/backbone/blocks.py:143-186).  With a workspace of
 * d2mi_conv2d_workspace_size() bytes, small-M shapes split K over several
 * workgroups and reduce in a fixed order (deterministic). */
size_t d2mi_conv2d_workspace_size(int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                  int stride, int pad_beg, int pad_end);
/* The launch plan of d2mi_conv2d_nhwc_ex / _gated for a shape, as integers;
 * launches nothing (the same planner the launcher runs, and the device's CU
 * count -- 256 without a device).  flags: d2mi_conv2d_nhwc_ex's.  operands,
 * the facts about the pointers a launch would get (a null one counts as
 * aligned): 1 top-down, 2 residual, 4 gate present; 8 = y and the present
 * top-down / residual / gate are 16-byte aligned; 16 = the bias is; 32 = a
 * workspace is passed, of workspace_bytes; 64 = it is 16-byte aligned.
 * Writes 33 integers to out and returns 33; negative (d2mi_last_error) when
 * the launcher would refuse the shape or out_len is short:
 *   [0] family: 0 tiled 128x128, 1 128x64, 2 128x32, 3 warp-specialised
 *       256x128, 4 streaming 1x1;  [1] resident workgroups per CU;
 *   [2] split products;  [3] LDS epilogue usable;  [4] M = N*OH*OW;
 *   [5] BM  [6] BN  [7] nM  [8] nN  [9] nk (k-steps);
 *   [10..17] main launch: first tile, tiles, splits (grid = tiles x splits),
 *       k-steps per split, first row, end row, reduce (0 none, 1 scalar,
 *       2 float4), reduce grid;   [18..25] tail launch, the same (tiles 0:
 *       none);  under family 4 these describe the tiled kernels' plan, which
 *       is not launched;
 *   [26..30] streaming kernel: KMAX, TN, form (1 residual | 2 gate), slices,
 *       grid (workgroups of 512 threads); 0 otherwise;
 *   [31] + [32] * 2^31 = workspace bytes the plan carves: the main launch's
 *       slab, then the tail launch's, [splits][rows][Cout] floats each.
 * A missing or short workspace gives the one-pass plan. */
int d2mi_conv2d_plan(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                     int pad_beg, int pad_end, int flags, int operands, size_t workspace_bytes,
                     int32_t* out, int out_len);
int d2mi_conv2d_nhwc_ex(const float* x, const float* w_packed, const float* bias,
                        const float* topdown, const float* residual, float* y, int N, int H,
                        int W, int Cin, int Cout, int KH, int KW, int stride, int pad_beg,
                        int pad_end, int flags, void* workspace, size_t workspace_bytes,
                        void* stream);
/* Gated form, for an input gradient (dgrad) of a ReLU output x that feeds
 * two consumers -- the next bottleneck's conv1 and its identity shortcut
 * (lib/modeling/backbone/blocks.py:143-186): writes
 *   y = gate > 0 ? conv(x, w) + bias + residual : 0
 * i.e. the conv's input gradient plus the shortcut's gradient (residual),
 * passed through the producer's ReLU backward (gate = its output), in one
 * pass.  residual / bias nullable; flags: bit2 split products, bit3 flipped
 * taps only. */
int d2mi_conv2d_nhwc_gated(const float* x, const float* w_packed, const float* bias,
                           const float* residual, const float* gate, float* y, int N, int H,
                           int W, int Cin, int Cout, int KH, int KW, int stride, int pad_beg,
                           int pad_end, int flags, void* workspace, size_t workspace_bytes,
                           void* stream);
/* Multi-level form: the same conv (shared weights) over nlev <= 6 feature
 * levels in ONE launch -- the heads the reference applies per FPN level with
 * shared variables: RetinaNet towers / predictors (retinanet.py:110-145),
 * SOLOv2 kernel / category towers (solo_v2.py:173-272).  xs[l]
 * [N_l,H_l,W_l,Cin]; dims = {N_l, H_l, W_l} per level; ys[l]
 * [N_l,OH_l,OW_l,Cout]; flags bit0 ReLU, bit2 split products.  Every level's
 * tiles share one grid: the small levels run beside the big one instead of
 * after it; when all levels together are under a round of workgroups, K is
 * split over the levels' concatenated rows (workspace of
 * d2mi_conv2d_levels_workspace_size bytes; fixed-order reduce). */
size_t d2mi_conv2d_levels_workspace_size(const int32_t* dims, int nlev, int Cin, int Cout,
                                         int KH, int KW, int stride, int pad_beg, int pad_end);
/* The plan of d2mi_conv2d_nhwc_levels, as d2mi_conv2d_plan (operands: 8 =
 * every level's output is 16-byte aligned, 32 / 64 the workspace).  29 integers:
 *   [0] family (0..2)  [1] resident workgroups per CU  [2] split products
 *   [3] LDS epilogue  [4] BM  [5] BN  [6] nN  [7] nk  [8] tiles  [9] splits
 *   (grid = tiles x splits)  [10] k-steps per split  [11] reduce grid (0: no
 *   reduce)  [12] nlev  [13..19] first tile of each level, [nlev] = tiles
 *   [20..26] first slab row of each level, [26] = all rows
 *   [27] + [28] * 2^31 = workspace bytes ([splits][rows][Cout] floats). */
int d2mi_conv2d_levels_plan(const int32_t* dims, int nlev, int Cin, int Cout, int KH, int KW,
                            int stride, int pad_beg, int pad_end, int flags, int operands,
                            size_t workspace_bytes, int32_t* out, int out_len);
int d2mi_conv2d_nhwc_levels(const float* const* xs, const int32_t* dims, int nlev,
                            const float* w_packed, const float* bias, float* const* ys, int Cin,
                            int Cout, int KH, int KW, int stride, int pad_beg, int pad_end,
                            int flags, void* workspace, size_t workspace_bytes, void* stream);
/* flags bit2 = "split" products: the same f32 operands, each split EXACTLY
 * into three bf16 terms (x = h + m + l, truncation), multiplied with six
 * bf16 MFMA products (v_mfma_f32_32x32x16_bf16; the dropped m*l, l*m, l*l
 * terms are below f32's own rounding of the product) and accumulated in f32.
 *
 * d2mi_split_bf16x3: x [n] f32 -> out [3][n] (bf16 bit patterns of h, m, l);
 * n % 4 == 0 (the stem conv's weight planes, d2mi_stem_conv). */
int d2mi_split_bf16x3(const float* x, int64_t n, uint16_t* out, void* stream);

/* Weight gradient of the same convolution (the tf.gradients of Conv2D.call,
 * lib/layers/convolutional.py:198-263, w.r.t. its HWIO kernel):
 *   dw[kh][kw][ci][co] = sum_{n,oy,ox} x[n, oy*s-pb+kh, ox*s-pb+kw, ci] * dy[n,oy,ox,co].
 * x [N,H,W,Cin], dy [N,OH,OW,Cout] (OH/OW as the forward), dw HWIO, written;
 * dbias [Cout] (nullable) receives sum_p dy[p][co], the bias gradient.
 * Cin, Cout multiples of 4.  With d2mi_conv2d_wgrad_workspace_size() bytes the
 * pixel reduction is split over workgroups and summed in a fixed order. */
size_t d2mi_conv2d_wgrad_workspace_size(int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                        int stride, int pad_beg, int pad_end);
/* The plan of d2mi_conv2d_wgrad_ex (flags: its flags), as d2mi_conv2d_plan
 * (operands: 8 = dw is 16-byte aligned, 32 / 64 the workspace).  16 integers:
 *   [0] kernel: 0 f32 <TM,TN>, 1 split <TM,TN>, 2 split 128x128 at three
 *       workgroups per CU, 3 warp-specialised, 4 the same with the incremental
 *       pixel cursor;
 *   [1] TM  [2] TN  [3] BM  [4] BN  [5] Cin tiles  [6] Cout tiles  [7] tiles
 *   [8] 32-pixel chunks  [9] splits (grid = tiles x splits)  [10] chunks per
 *   split  [11] slabs are written (splits > 1 or accumulating)  [12] reduce
 *   (0 none, 1 scalar, 2 float4)  [13] reduce grid
 *   [14] + [15] * 2^31 = workspace bytes: [splits] dw slabs, then [splits]
 *   dbias slabs. */
int d2mi_conv2d_wgrad_plan(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                           int pad_beg, int pad_end, int flags, int operands,
                           size_t workspace_bytes, int32_t* out, int out_len);
int d2mi_conv2d_wgrad(const float* x, const float* dy, float* dw_hwio, float* dbias, int N,
                      int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad_beg,
                      int pad_end, void* workspace, size_t workspace_bytes, void* stream);
/* flags bit2: the split-bf16 products of d2mi_conv2d_nhwc_ex (exact 3-term
 * split of x and dy, six bf16 MFMA products, f32 accumulation).  bit3:
 * accumulate -- dw_hwio (and dbias) += this call's gradient, in the reduce
 * pass (a weight shared by several calls, e.g. one head over the FPN levels);
 * the workspace must then hold the plan's slabs even for one split
 * (d2mi_conv2d_wgrad_workspace_size, or one slab when that returns 0). */
int d2mi_conv2d_wgrad_ex(const float* x, const float* dy, float* dw_hwio, float* dbias, int N,
                         int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                         int pad_beg, int pad_end, int flags, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Many weight gradients in one launch per kernel family (flags bit2 as
 * d2mi_conv2d_wgrad_ex; no accumulate).  problems: a HOST array of n (<= 64)
 *   struct { const float* x; const float* dy; float* dw; float* dbias;
 *            int32_t N, H, W, Cin, Cout, KH, KW, stride, pad_beg, pad_end; }
 * (72 bytes each; dbias nullable).  Alone, a small weight gradient cuts its
 * pixels into many splits to fill the chip; in a group the problems of one
 * kernel family share one grid and one reduce launch.  Under tuning
 * "wgrad_group" = 1 each keeps the splits of its own d2mi_conv2d_wgrad_plan
 * (the same sums in the same order: the bits of d2mi_conv2d_wgrad_ex); under 2
 * a family has one common chunks-per-split, chosen from its summed tile-chunks
 * against rounds of resident workgroups: long pixel walks, few partial slabs.
 * A problem of one split writes dw directly.  A group of one runs exactly
 * d2mi_conv2d_wgrad_ex; so does every problem when the workspace is missing,
 * short or not 16-byte aligned, and every problem on the f32 kernels.
 *
 * The launches read their arguments from a device table.  The caller gets its
 * bytes from d2mi_conv2d_wgrad_group_table (host only: it writes table_bytes =
 * d2mi_conv2d_wgrad_group_table_size(n) bytes for THIS workspace address into
 * table_host), copies them to the device in stream order (or, for a captured
 * launch, any time before the replay) and passes that copy as table_dev.
 *
 * d2mi_conv2d_wgrad_group_plan: 2 + 7 * 6 + n * 9 + 2 integers --
 *   [0] grouped (0: the per-problem plans)  [1] n;
 *   per family f = 0..6 (ws, ws_inc, split 2x2, 2x1, 1x2, 1x1, 2x2 at three
 *   per CU): problems, workgroups, chunks per split, problems with slabs,
 *   reduce grid, 0;
 *   per problem (9): family (-1: alone), kernel, tiles, chunks, splits, chunks
 *   per split, first workgroup, slab byte offset as lo + hi * 2^31;
 *   then lo + hi * 2^31 = workspace bytes. */
size_t d2mi_conv2d_wgrad_group_workspace_size(const void* problems, int n, int flags);
size_t d2mi_conv2d_wgrad_group_table_size(int n);
int d2mi_conv2d_wgrad_group_plan(const void* problems, int n, int flags, int operands,
                                 size_t workspace_bytes, int32_t* out, int out_len);
int d2mi_conv2d_wgrad_group_table(const void* problems, int n, int flags, void* workspace,
                                  size_t workspace_bytes, void* table_host, size_t table_bytes);
int d2mi_conv2d_wgrad_group(const void* problems, int n, int flags, const void* table_dev,
                            size_t table_bytes, void* workspace, size_t workspace_bytes,
                            void* stream);

/* Row census of a sparse gradient map g [N*H*W][C] (C % 4 == 0), for a
 * gradient whose producer can bound its non-zero rows (the RPN loss: at most
 * RPN.BATCH_SIZE_PER_IMAGE sampled anchors per image).  Written into the
 * workspace (d2mi_row_census_workspace_size bytes, the caller keeps it until
 * its readers have run):
 *   bitmap    one bit per 32-pixel chunk (bit c % 32 of word c / 32), set iff
 *             a row of the chunk has a non-zero element.  Bits are compared:
 *             NaN and Inf count as non-zero, -0.0 as zero;
 *   word_rows the non-zero rows of each bitmap word's 1024 pixels;
 *   count     their sum;
 * and with dilate_k > 0
 *   rows      the ascending, duplicate-free list of the output rows of a
 *             dilate_k x dilate_k stride-1 conv over g with dilate_pad leading
 *             pad whose window holds a non-zero row (inside the image only);
 *             capacity min(capacity * dilate_k^2, N*H*W) entries (at least 1);
 *   nrows     their number, clamped to that capacity.
 * count > capacity (or a list past its capacity) sets bit value 8 of the
 * device error word: the declared bound was false; nothing is written past a
 * list's capacity.  d2mi_row_census_layout writes {bitmap byte offset, bitmap
 * words, word_rows byte offset, count byte offset, nrows byte offset, rows
 * byte offset (-1 without a list), list capacity} into out[7]. */
size_t d2mi_row_census_workspace_size(int N, int H, int W, int capacity, int dilate_k);
int d2mi_row_census_layout(int N, int H, int W, int capacity, int dilate_k, int64_t* out,
                           int out_len);
int d2mi_row_census(const float* g, int N, int H, int W, int C, int capacity, int dilate_k,
                    int dilate_pad, void* workspace, size_t workspace_bytes, void* stream);
/* d2mi_conv2d_nhwc_gated (gate nullable: then d2mi_conv2d_nhwc_ex without bias,
 * top-down or relu) over the dilated row list of x's census (d2mi_row_census
 * with this capacity, dilate_k = KH = KW, dilate_pad = pad_beg): for a
 * same-size stride-1 conv, every output row that is not listed has an
 * all-zero window.  The dense plan is kept; where the list's capacity is
 * below the plan's main-launch rows, that launch becomes a fill of its rows
 * with epilogue(0) (0.f + residual, zero where the gate is not positive) and
 * a launch over the listed rows with the same K splits and reduce order; the
 * plan's tail launch runs dense.  Every element sees the dense kernel's own
 * product sequence: bit-identical.  Returns 1 when the row-list launch ran,
 * 0 after the dense call, < 0 on error. */
int d2mi_conv2d_nhwc_rows(const float* x, const float* w_packed, const float* residual,
                          const float* gate, float* y, int N, int H, int W, int Cin, int Cout,
                          int KH, int KW, int stride, int pad_beg, int pad_end, int flags,
                          const void* census, size_t census_bytes, int capacity, int dilate_k,
                          int dilate_pad, void* workspace, size_t workspace_bytes, void* stream);
/* d2mi_conv2d_wgrad_ex with the row census of dy (census: the workspace
 * d2mi_row_census filled for dy's N x OH x OW rows; a superset bitmap is as
 * good).  Same plan, same slabs, same reduce; the warp-specialised kernel
 * walks only the chunks whose bit is set, which for finite x is bit-identical
 * to the dense call (a skipped chunk adds +-0 to sums that start at +0).
 * The other kernels ignore the bitmap.  Returns 1 when the bitmap kernel
 * ran, 0 after a dense launch, < 0 on error. */
int d2mi_conv2d_wgrad_rows(const float* x, const float* dy, float* dw_hwio, float* dbias, int N,
                           int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                           int pad_beg, int pad_end, int flags, const void* census,
                           size_t census_bytes, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ------------------------------------------------------- FrozenBN fold
 * A frozen BatchNorm (moving statistics; lib/layers/normalization.py:15-119
 * with training=False, gamma/beta trainable above FREEZE_AT per
 * lib/modeling/backbone/resnet.py:22-46) folded into the preceding Conv2D:
 *   scale = gamma / sqrt(var + eps);  w_eff = w * scale;
 *   b_eff = bias * scale + beta - mean * scale.
 * w HWIO [KH,KW,Cin,Cout]; bias / gamma / beta nullable.  Writes w_eff (HWIO,
 * nullable), w_packed ([KH,KW,Cout,Cin] for d2mi_conv2d_nhwc, nullable) and
 * b_eff [Cout]. */
int d2mi_fold_frozen_bn(const float* w_hwio, const float* bias, const float* gamma,
                        const float* beta, const float* mean, const float* var, float eps,
                        int KH, int KW, int Cin, int Cout, float* w_eff, float* w_packed,
                        float* b_eff, void* stream);
/* Backward: from gw_eff (HWIO) and gb_eff ([Cout], nullable) writes gw, gbias,
 * ggamma, gbeta (each nullable); per-channel reductions in a fixed order. */
size_t d2mi_fold_frozen_bn_bwd_workspace_size(int Cout);
int d2mi_fold_frozen_bn_bwd(const float* gw_eff, const float* gb_eff, const float* w_hwio,
                            const float* bias, const float* gamma, const float* mean,
                            const float* var, float eps, int KH, int KW, int Cin, int Cout,
                            float* gw, float* gbias, float* ggamma, float* gbeta,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Batched fold: every BN-conv of a network in one forward launch and one
 * backward pair (same arithmetic and summation order as the per-conv calls
 * above, so bit-identical results).  Replaces the per-layer
 * Conv2D -> BatchNorm(training=False) pairs of lib/modeling/backbone/resnet.py
 * (resnet_arg_scope, :22-46) for one training step.  table: DEVICE array of
 * entries sorted by fwd_begin / bwd_begin / co_begin (each ascending):
 *   fwd_begin  first forward workgroup: ceil(Cout/64)*ceil(Cin/64)*taps each;
 *   bwd_begin  first backward workgroup: ceil(Cout/64)*row_chunks each;
 *   co_begin   prefix sum of Cout;  partial_offset  floats into the backward
 *   workspace (row_chunks*Cout each).
 * Forward reads w/bias/gamma/beta/mean/var and writes w_eff/w_packed/b_eff
 * (w_eff, w_packed nullable); backward reads gw_eff/gb_eff (nullable = zero)
 * and writes gw/gbias/ggamma/gbeta (each nullable).  d2mi_fold_many_sizes
 * reports sizeof(entry) and the row-chunk count so a host can check its
 * layout. */
typedef struct d2mi_fold_entry {
  const float* w;
  const float* bias;
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* var;
  float* w_eff;
  float* w_packed;
  float* b_eff;
  const float* gw_eff;
  const float* gb_eff;
  float* gw;
  float* gbias;
  float* ggamma;
  float* gbeta;
  float eps;
  int taps, Cin, Cout;
  int fwd_begin, bwd_begin, co_begin, pad;
  long long partial_offset;
} d2mi_fold_entry;
int d2mi_fold_many_sizes(int* entry_bytes, int* row_chunks);
int d2mi_fold_frozen_bn_many(const d2mi_fold_entry* table, int num_entries, int fwd_blocks,
                             void* stream);
int d2mi_fold_frozen_bn_bwd_many(const d2mi_fold_entry* table, int num_entries, int bwd_blocks,
                                 int total_cout, float* workspace, void* stream);

/* ------------------------------------------------------- mask pasting
 * Replaces detector_postprocess (lib/modeling/postprocessing.py:9-59) for the
 * "conventional" / "fixed" SEGMENTATION_OUTPUT formats, i.e.
 * reframe_box_masks_to_image_masks (lib/structures/mask_ops.py:7-56):
 * normalise each box by the canvas (out_h, out_w), take the reverse box of the
 * unit square, tf.image.crop_and_resize the box mask onto the canvas
 * (bilinear, extrapolation 0) and threshold with tf.greater -> uint8.  Same
 * float32 sequence as the TF CPU kernels; the f32 canvas is never stored.
 * box_masks [D, mask_h, mask_w] f32 (probabilities); boxes [D, 4] f32 yxyx
 * absolute; yx_scale [D, 2] f32 (nullable): per-box (sy, sx) applied first
 * ("fixed": output_shape / image_shape, box_list_ops.scale); valid [D] u8
 * (nullable): rows with 0 are written as zeros (SparseBoxList.to_dense);
 * out [D, out_h, out_w] u8, 4-byte aligned. */
int d2mi_paste_masks(const float* box_masks, const float* boxes, const float* yx_scale,
                     const uint8_t* valid, int D, int mask_h, int mask_w, int out_h, int out_w,
                     float threshold, uint8_t* out, void* stream);

/* ------------------------------------------------ skinny 1x1 weight gradient
 * gw[Cin][Cout] = X^T G and gb[Cout] = column sums of G over P pixels, for
 * Cout <= 80 (the RPN head's objectness + anchor-delta 1x1 convs, fused:
 * lib/modeling/proposal_generator/rpn.py:83-96, whose TF gradient is
 * Conv2DBackpropFilter + BiasAddGrad; 16 outputs for 3 anchors, 76 for the
 * C4 / DC5 RPNs' 15).  x [P, Cin], g [P, Cout] f32 contiguous; gb nullable.
 * One streaming pass over x per block of 16 output columns (Cout <= 16: one
 * pass).  Fixed-order reduction (deterministic); workspace from
 * d2mi_wgrad_skinny_workspace_size: ceil(P / 128) * (Cin + 1) * Cout floats. */
size_t d2mi_wgrad_skinny_workspace_size(int P, int Cin, int Cout);
int d2mi_wgrad_skinny(const float* x, const float* g, int P, int Cin, int Cout, float* gw,
                      float* gb, void* workspace, size_t workspace_bytes, void* stream);
/* d2mi_wgrad_skinny_ex: accumulate != 0 adds the result into gw / gb (old +
 * new: autograd's accumulation of a weight shared by several calls -- the RPN
 * head's fused 1x1 over the FPN levels, rpn.py:83-96). */
int d2mi_wgrad_skinny_ex(const float* x, const float* g, int P, int Cin, int Cout, float* gw,
                         float* gb, int accumulate, void* workspace, size_t workspace_bytes,
                         void* stream);
/* d2mi_wgrad_skinny_levels: the skinny wgrad of L <= 8 calls sharing one
 * weight (the RPN head's fused 1x1 over the FPN levels, rpn.py:31-96: one
 * weight applied per level, its gradient the sum over levels) in one partial
 * launch and one reduce: x[l] [P[l], Cin] (16-B aligned, Cin % 4 == 0),
 * g[l] [P[l], Cout]; each level summed exactly as one d2mi_wgrad_skinny call
 * and the levels added in array order (accumulate != 0: after the old gw /
 * gb) -- bit-identical to the per-level calls with accumulate after the
 * first.  Cout <= 80 as above.  workspace >=
 * d2mi_wgrad_skinny_levels_workspace_size: (sum_l ceil(P[l] / 128)) *
 * (Cin + 1) * Cout floats. */
size_t d2mi_wgrad_skinny_levels_workspace_size(const int* P, int L, int Cin, int Cout);
int d2mi_wgrad_skinny_levels(const float* const* x, const float* const* g, const int* P, int L,
                             int Cin, int Cout, float* gw, float* gb, int accumulate,
                             void* workspace, size_t workspace_bytes, void* stream);
/* Column sums of a row-major [rows, cols] f32 matrix (a conv's bias gradient,
 * TF BiasAddGrad, when its weight gradient runs as a library GEMM): out[cols],
 * fixed-order two-level reduction; workspace from
 * d2mi_column_sum_workspace_size. */
size_t d2mi_column_sum_workspace_size(long long rows, int cols);
int d2mi_column_sum(const float* x, long long rows, int cols, float* out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------ IoU + Matcher
 * box_list_ops.pairwise_iou (:295-372) of gt_boxes [N,G,4] against boxes
 * ([P,4] shared by every image, or [N,P,4] with boxes_per_image = 1; yxyx
 * f32, 16-B aligned) fused with Matcher.__call__ (lib/modeling/matcher.py:
 * 8-173): matches [N,P] int64 = the first GT of maximal IoU among the
 * matchable GT (gt_flags bit0), labels [N,P] int64 from the n_intervals
 * intervals [thresholds[i], thresholds[i+1]) -> labels_of[i], low-quality
 * matches (IoU equal to that GT's best over all boxes -> 1) when
 * allow_low_quality, no matchable GT -> 0 / match 0, then -1 for background
 * boxes whose max IoU with a crowd GT (bit1) exceeds crowd_thr or with a
 * difficult GT (bit2) exceeds difficult_thr.  G <= 256; the workspace
 * (d2mi_match_workspace_size) holds the per-GT best IoU. */
size_t d2mi_match_workspace_size(int N, int G);
int d2mi_match_boxes(const float* gt_boxes, const int* gt_flags, const float* boxes,
                     int boxes_per_image, int N, int G, int P, const float* thresholds,
                     const int* labels_of, int n_intervals, int allow_low_quality,
                     float crowd_thr, float difficult_thr, long long* matches, long long* labels,
                     void* workspace, size_t workspace_bytes, void* stream);
/* d2mi_match_boxes with the GT flags as byte masks [N, G] (bool tensors as
 * they are: valid required, crowd / difficult nullable) instead of the
 * packed int32 word -- no packing passes on the host side.  The matchable GT
 * are valid && !crowd && !difficult (the reference's valid_gt_boxlist). */
int d2mi_match_boxes_ex(const float* gt_boxes, const uint8_t* valid, const uint8_t* crowd,
                        const uint8_t* difficult, const float* boxes, int boxes_per_image, int N,
                        int G, int P, const float* thresholds, const int* labels_of,
                        int n_intervals, int allow_low_quality, float crowd_thr,
                        float difficult_thr, long long* matches, long long* labels,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------ Cascade R-CNN stage hand-over
 * CascadeROIHeads._create_proposals_from_boxes + _match_and_label_boxes
 * (lib/modeling/roi_heads/cascade_rcnn.py:141-215, :244-273) in one launch,
 * one thread per proposal.  deltas [N*S, 4] (class-agnostic) of the previous
 * stage decoded on its boxes [N, S, 4] (yxyx f32, 16-B aligned) with
 * weights4_host / scale_clamp and clipped to [0, 0, h, w] of image_hw int32
 * [N, 2] -> out_boxes [N, S, 4]; valid / out_valid uint8 [N, S].
 * training = 0: out_valid = valid and the other outputs are not touched
 * (null allowed).  training = 1: out_valid = valid && area(out box) > 0, and
 * the boxes are matched against gt_boxes [N, G, 4] (1 <= G <= 256; gt_valid /
 * gt_crowd / gt_difficult uint8 [N, G], crowd / difficult nullable, as in
 * d2mi_match_boxes_ex; gt_cls [N, G] int64 when gt_cls_64 else int32, as in
 * d2mi_roi_gt_classes) like d2mi_match_boxes_ex with thresholds [-inf,
 * iou_thr, +inf], labels [0, 1], no low-quality matches, crowd_thr 1e-3 and
 * difficult_thr iou_thr: out_gt_index int64 = the match, out_gt_boxes
 * [N, S, 4] = its box, out_gt_classes int64 = its class (foreground) /
 * num_classes (background) / -1 (ignored, or !out_valid), out_loss_valid
 * uint8 = out_valid && class >= 0.  Every element of every output is
 * written; no workspace.  G = 0 is refused in training mode, unlike in
 * d2mi_match_boxes_ex: the matched class and box are gathered from row
 * out_gt_index, which needs a GT row to exist (pad the GT list to G >= 1
 * with gt_valid 0: every row is then background with match 0). */
int d2mi_cascade_refine(const float* deltas, const float* boxes, const uint8_t* valid,
                        const int32_t* image_hw, int N, int S, const float* weights4_host,
                        float scale_clamp, int training, const float* gt_boxes,
                        const uint8_t* gt_valid, const uint8_t* gt_crowd,
                        const uint8_t* gt_difficult, const void* gt_cls, int gt_cls_64, int G,
                        float iou_thr, int num_classes, float* out_boxes, uint8_t* out_valid,
                        int64_t* out_gt_classes, int64_t* out_gt_index, float* out_gt_boxes,
                        uint8_t* out_loss_valid, void* stream);

/* ------------------------------------------------ Relation Networks attention
 * ObjectRelationModule.call with compute_geometry_embeddings
 * (lib/modeling/roi_heads/relation_module.py:29-89, :141-194) on the dense
 * [N, R] proposal layout, without any tensor of R x R extent: boxes [N, R, 4]
 * (yxyx f32, 16-B aligned), valid uint8 [N, R], q / k [N, R, G*dk], v
 * [N, R, dv], wg [E, G] and bg [G] (the geometry 1x1 conv).  An invalid slot
 * takes part as SparseBoxList.to_dense leaves it: box 0, q = k = v = 0 (its
 * rows of q / k / v are not read); the softmax runs over all R columns.
 *   out [N, R, G*dv]: out[n, i, g*dv + d] = sum_j P[n, i, g, j] v[n, j, d],
 *                     zero rows for invalid i (the residual is the caller's);
 *   lse [N, R, 2, G]: the log-sum-exp of row (n, i, g)'s logits for the backward,
 *                     in its two parts (the maximum m, then the sum l of
 *                     exp(logit - m): lse = m + log l), so that the backward's
 *                     exp(logit - m) / l uses the l that out was divided by.
 * Envelope: 1 <= G <= 16, 1 <= dk <= 8, dv % 4 == 0 and dv <= 64, E % 8 == 0
 * and E <= 128, 1 <= N <= 65535, R >= 1; anything else is refused on the host.
 * One launch, no workspace, no host synchronisation. */
int d2mi_relation_fwd(const float* boxes, const uint8_t* valid, const float* q, const float* k,
                      const float* v, const float* wg, const float* bg, int N, int R, int G,
                      int dk, int dv, int E, float* out, float* lse, void* stream);
/* The backward of d2mi_relation_fwd (relation_module.py:29-89, :141-194
 * differentiated; no gradient to the boxes): out / lse as the forward wrote
 * them, d_out [N, R, G*dv] -> d_q, d_k [N, R, G*dk], d_v [N, R, dv] (zero rows
 * for invalid slots), d_wg [E, G], d_bg [G]; d log(max(relu(x), 1e-6)) / dx
 * is 1 / x where x > 1e-6 and 0 elsewhere.  Embedding and probabilities are
 * recomputed from lse; sums over rows and over pairs go through fixed-order
 * partials in the workspace (no atomics: two runs are bit-identical).  Four
 * launches, no host synchronisation. */
size_t d2mi_relation_workspace_size(int N, int R, int G, int dk, int dv, int E);
int d2mi_relation_bwd(const float* boxes, const uint8_t* valid, const float* q, const float* k,
                      const float* v, const float* wg, const float* bg, const float* out,
                      const float* lse, const float* d_out, int N, int R, int G, int dk, int dv,
                      int E, float* d_q, float* d_k, float* d_v, float* d_wg, float* d_bg,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------ RPN losses
 * RPNOutputs.losses (rpn_outputs.py:306-401) after matching and sampling:
 * logits [N,P], deltas [N,P,4], anchors [P,4], gt_boxes [N,G,4] (yxyx),
 * matches [N,P] int64, pos / sampled [N,P] bool (uint8).  Forward writes
 * partial [N][d2mi_rpn_loss_blocks()] float2 = (sigmoid CE over sampled,
 * smooth-L1(beta) over positives of the get_deltas targets with weights[4]),
 * summed by the caller in a fixed order.  Backward: grads = device float[2]
 * (d loss_cls_sum, d loss_loc_sum) -> d_logits [N,P], d_deltas [N,P,4]. */
int d2mi_rpn_loss_blocks(void);
int d2mi_rpn_loss_fwd(const float* logits, const float* deltas, const float* anchors,
                      const float* gt_boxes, const long long* matches, const unsigned char* pos,
                      const unsigned char* sampled, int N, int P, int G, const float* weights,
                      float beta, float* partial, void* stream);
int d2mi_rpn_loss_bwd(const float* logits, const float* deltas, const float* anchors,
                      const float* gt_boxes, const long long* matches, const unsigned char* pos,
                      const unsigned char* sampled, int N, int P, int G, const float* weights,
                      float beta, const float* grads, float* d_logits, float* d_deltas,
                      void* stream);
/* d2mi_rpn_loss_bwd with the two upstream gradients as separate device
 * scalars (null: zero) and the loss normaliser folded in: the gradients used
 * are g * scale (the losses' `* normalizer * loss_weight`, rpn_outputs.py:
 * 331-342, without its multiply launches or a gradient pack). */
int d2mi_rpn_loss_bwd_ex(const float* logits, const float* deltas, const float* anchors,
                         const float* gt_boxes, const long long* matches,
                         const unsigned char* pos, const unsigned char* sampled, int N, int P,
                         int G, const float* weights, float beta, const float* g_cls,
                         const float* g_loc, float scale, float* d_logits, float* d_deltas,
                         void* stream);

/* ----------------------------------------------------- ROI-head losses
 * FastRCNNOutputs.losses (lib/modeling/roi_heads/fast_rcnn.py:269-357) on
 * dense sampled rows: logits [B, K1 = K+1], deltas [B, nreg*4] (nreg 1 =
 * class-agnostic), proposals / gt_boxes [B] yxyx float4, gt_classes int64 [B]
 * (K = background), valid uint8 [B].  stats [4] device = (loss_cls, loss_box,
 * #valid, R = max(1, #valid)): loss_cls = sum of softmax CE over valid rows /
 * R, loss_box = sum of smooth-L1(beta) of the gt-class deltas against
 * get_deltas(proposal, gt box; weights) over foreground rows / R
 * (box_regression.py:38-74, layers/loss.py).  Row terms go to the workspace
 * and are summed by one workgroup in a fixed order (deterministic).
 * _bwd: d_logits / d_deltas (every element written) for the upstream
 * gradients grads [2] device (loss_cls, loss_box). */
size_t d2mi_fast_rcnn_loss_workspace_size(int B);
int d2mi_fast_rcnn_loss_fwd(const float* logits, const float* deltas, const float* proposals,
                            const long long* gt_classes, const float* gt_boxes,
                            const unsigned char* valid, int B, int K1, int nreg,
                            const float* weights, float beta, float* stats, void* workspace,
                            size_t workspace_bytes, void* stream);
int d2mi_fast_rcnn_loss_bwd(const float* logits, const float* deltas, const float* proposals,
                            const long long* gt_classes, const float* gt_boxes,
                            const unsigned char* valid, int B, int K1, int nreg,
                            const float* weights, float beta, const float* stats,
                            const float* grads, float* d_logits, float* d_deltas, void* stream);
/* mask_rcnn_loss (lib/modeling/roi_heads/mask_head.py:17-68): logits
 * [B, P = Hm*Wm, C], target [B, P] (the rounded crop_and_resize of the GT
 * mask), classes int64 [B], fg uint8 [B]; stats [3] = (loss, #fg,
 * n = max(1, #fg * P)), loss = sum over fg rows of the sigmoid BCE of the
 * class channel (clamped to [0, C-1]; channel 0 when C == 1) / n.  _bwd
 * writes the whole d_logits for grads [1] device. */
size_t d2mi_mask_loss_workspace_size(int B);
int d2mi_mask_loss_fwd(const float* logits, const float* target, const long long* classes,
                       const unsigned char* fg, int B, int P, int C, float* stats,
                       void* workspace, size_t workspace_bytes, void* stream);
int d2mi_mask_loss_bwd(const float* logits, const float* target, const long long* classes,
                       const unsigned char* fg, int B, int P, int C, const float* stats,
                       const float* grads, float* d_logits, void* stream);

/* ------------------------------------------------ ResNet stem tail
 * relu(y + shift) -> zero pad 1 -> 3x3 stride-2 VALID max pool
 * (lib/modeling/backbone/resnet.py:73-82) on the NHWC output y [N,H,W,C] of
 * the stem conv (without its bias); out [N,(H-1)/2+1,(W-1)/2+1,C].  shift
 * [C] nullable; C % 4 == 0; 16-B aligned. */
int d2mi_stem_pool(const float* y, const float* shift, int N, int H, int W, int C, float* out,
                   void* stream);
/* The stem conv feeding it: 7x7 / stride 2, Cin 3 -> Cout 64, the symmetric
 * pad of 3 then VALID of lib/layers/convolutional.py:12-24 (fix_padding) and
 * resnet.py Stem.conv1, on the split-bf16 MFMA (f32-class).  x [N,H,W,3]
 * NHWC f32; w3 [3][64][160] bf16 planes (d2mi_split_bf16x3) of the weights
 * transposed to [Cout][K] (K = (kh * 7 + kw) * 3 + c, HWIO order) and
 * zero-padded to K = 160; y [N,(H-1)/2+1,(W-1)/2+1,64] the raw sums (no bias:
 * d2mi_stem_pool adds the folded shift).  Replaces the MIOpen conv of the
 * frozen stem. */
int d2mi_stem_conv(const float* x, const uint16_t* w3, int N, int H, int W, float* y,
                   void* stream);
/* The preprocessing ahead of it (lib/modeling/meta_arch/rcnn.py:146-157
 * preprocess_image + structures/image_list.py:89-100 with pad value 0):
 * x [N,H,W,3] NHWC f32 0-255 RGB -> out [N,OHp,OWp,3], out = (x - mean[c]) /
 * std[c] (mean / std: 3 device floats), channels reversed when flip (BGR
 * input format), zeros at rows >= H and columns >= W.  One launch; the same
 * IEEE subtract and divide per value as the unfused form. */
int d2mi_preprocess_images(const float* x, const float* mean, const float* stdv, int N, int H,
                           int W, int OHp, int OWp, int flip, float* out, void* stream);

/* ------------------------------------------------ ROI-head sampling glue
 * (lib/modeling/roi_heads/roi_heads.py:100-232 label_and_sample_proposals,
 * :35-62 select_foreground_proposals)
 * d2mi_roi_gt_classes: out [N,M] int64 = -1 where !pvalid, else the matched
 * GT class gt_cls[n][matches] (gt_cls [N,G], int64 when gt_cls_64 else
 * int32) for label 1, K (background) for label 0, the label (-1) otherwise;
 * labels / matches [N,M] int64 (d2mi_match_boxes), pvalid [N,M] bool.
 * d2mi_roi_sample_take: the sampled slots in the sampler's order (order [N,S]
 * int64, d2mi_subsample): s_boxes [N,S,4] = boxes[n][order], s_cls =
 * gt_classes[n][order], s_gidx = matches[n][order], s_gtb [N,S,4] =
 * gt_boxes[n][s_gidx]; and (F > 0) the mask branch's rows over the first F
 * slots of each image (R = N*F rows, row i = slot (i / F, i % F)): fg_all[i]
 * = valid && s_cls < K, count[0] = the number of foreground rows, and
 * m_boxes / m_cls / m_fg / m_img (the image, int32) / m_mind (s_gidx + n*G) /
 * m_gtb [R(,4)] in stable foreground-first order.  One workgroup; box arrays
 * 16-byte aligned. */
int d2mi_roi_gt_classes(const int64_t* labels, const int64_t* matches, const void* gt_cls,
                        int gt_cls_64, const uint8_t* pvalid, int N, int M, int G, int K,
                        int64_t* out, void* stream);
int d2mi_roi_sample_take(const int64_t* order, const uint8_t* valid, const float* boxes,
                         const int64_t* gt_classes, const int64_t* matches, const float* gt_boxes,
                         int N, int M, int S, int G, int F, int K, float* s_boxes, int64_t* s_cls,
                         int64_t* s_gidx, float* s_gtb, float* m_boxes, int64_t* m_cls,
                         uint8_t* m_fg, int32_t* m_img, int64_t* m_mind, float* m_gtb,
                         uint8_t* fg_all, int64_t* count, void* stream);

/* ------------------------------------------------ resampling gradients
 * d2mi_upsample2x_grad: adjoint of the FPN top-down nearest 2x upsample
 * (lib/modeling/backbone/fpn.py:138-149): gy [N,OH,OW,C] -> gtd
 * [N,ceil(OH/2),ceil(OW/2),C], each the sum of the (up to) 2x2 pixels that
 * copy it, in the order (0,0), (0,1), (1,0), (1,1).
 * d2mi_stride_scatter: input gradient of a 1x1 stride-s conv from its GEMM on
 * the strided grid: g [N,ceil(H/s),ceil(W/s),C] -> out [N,H,W,C] with zeros
 * off the grid, plus add [N,H,W,C] (nullable).  C % 4 == 0, 16-B aligned. */
int d2mi_upsample2x_grad(const float* gy, int N, int OH, int OW, int C, float* gtd, void* stream);
int d2mi_stride_scatter(const float* g, const float* add, int N, int H, int W, int C, int stride,
                        float* out, void* stream);
/* d2mi_stride_scatter_ex: the same, then + add2 (nullable), then the ReLU
 * backward of the producer (gate nullable: out = gate > 0 ? v : 0, the
 * threshold_backward(v, gate, 0) of the ReLU output `gate`).  Used when a
 * ResNet stage output feeds the next stage's strided conv1 / shortcut pair
 * AND the FPN lateral (fpn.py:121-149, resnet.py:52-253): the last of the
 * three backwards forms the whole gated gradient. */
int d2mi_stride_scatter_ex(const float* g, const float* add, const float* add2, const float* gate,
                           int N, int H, int W, int C, int stride, float* out, void* stream);

/* ------------------------------------------------------ RetinaNet losses
 * Replaces RetinaNet.losses (lib/modeling/single_stage_heads/retinanet.py:
 * 147-210) up to the loss normaliser: sigmoid_focal_loss (lib/layers/
 * loss.py:59-104, alpha / gamma, reduction "sum") over every anchor whose
 * label is not "ignore" and every class (target 1 at the matched GT's class
 * for foreground anchors), and smooth_l1_loss (loss.py:9-58, beta, "sum")
 * of the foreground anchors' deltas against get_deltas(anchor, matched GT)
 * (lib/modeling/box_regression.py:38-74, weights[4] = wy, wx, wh, ww).
 * cls[l] / box[l]: level l's head outputs [N, H_l, W_l, A*K] / [N, H_l, W_l,
 * A*4] f32 (16-byte aligned), level_anchors[l] = H_l * W_l * A; anchors [R, 4]
 * (levels concatenated, (h, w, a) order, R = sum of level_anchors); gt_boxes
 * [N, G, 4]; gt_classes [N, G] int64; matches / labels [N, R] int64 (the
 * Matcher's: labels 1 fg, 0 bg, -1 ignore).  K % 4 == 0.  fwd: partial
 * [N * d2mi_retina_loss_blocks()][2] (cls, box) per-workgroup sums, to be
 * added in a fixed order.  bwd: d_cls / d_box levels (every element written),
 * scaled by the device scalars *g_cls / *g_box (null: zero). */
int d2mi_retina_loss_blocks(void);
int d2mi_retina_loss_fwd(const float* const* cls, const float* const* box,
                         const long long* level_anchors, int L, int N, int K, int A,
                         const float* anchors, const float* gt_boxes, const long long* gt_classes,
                         int G, const long long* matches, const long long* labels, float alpha,
                         float gamma, float beta, const float* weights, float* partial,
                         void* stream);
int d2mi_retina_loss_bwd(const float* const* cls, const float* const* box, float* const* d_cls,
                         float* const* d_box, const long long* level_anchors, int L, int N, int K,
                         int A, const float* anchors, const float* gt_boxes,
                         const long long* gt_classes, int G, const long long* matches,
                         const long long* labels, float alpha, float gamma, float beta,
                         const float* weights, const float* g_cls, const float* g_box,
                         void* stream);

/* ------------------------------------------------------ Momentum-SGD step
 * Replaces the update of lib/engine/trainer.py:116-139 for every trainable
 * tensor in two launches: g' = g + wd * w (slim.l2_regularizer gradient,
 * lib/solver/regularizer.py:6-24), per-tensor tf.clip_by_norm(g', clip_norm)
 * (slim.learning.clip_gradient_norms; clip_norm <= 0 disables it), then
 * ApplyMomentum: accum = accum * momentum + g''; w -= lr * accum.
 * tensor_table / chunk_table: device arrays of the records whose sizes
 * d2mi_sgd_table_sizes reports (tensor: {float* w; const float* g (nullable:
 * zero gradient); float* accum; int64 numel; float wd; int32 first_chunk,
 * num_chunks, pad}; chunk: {int32 tensor, pad; int64 begin, end}, chunks of at
 * most chunk_elems elements, a tensor's chunks consecutive).  partial: device
 * float [num_chunks] scratch.  Per-tensor norms are fixed-order sums. */
int d2mi_sgd_table_sizes(int* tensor_bytes, int* chunk_bytes, int* chunk_elems);
int d2mi_momentum_sgd(const void* tensor_table, const void* chunk_table, int num_chunks,
                      float* partial, float clip_norm, float momentum, float lr, void* stream);
/* The same step with the learning rate read from the device float *lr_dev at
 * run time when lr_dev is non-null (lr ignored): a training step captured in
 * a hipGraph (engine/graphed.py) replays with each iteration's LR of
 * lib/solver/learning_rate.py, which the host writes to lr_dev. */
int d2mi_momentum_sgd_ex(const void* tensor_table, const void* chunk_table, int num_chunks,
                         float* partial, float clip_norm, float momentum, float lr,
                         const float* lr_dev, void* stream);

/* ------------------------------------------------ Deformable-conv sampling
 * Replaces the sampling half of DeformConv2D.call (lib/layers/
 * convolutional.py:410-452: _get_sampling_indices :51-67, the offset add and
 * clip :422-431, _get_bilinear_interpolatied_pixels :70-115 -- four
 * tf.gather_nd -- and the reshape / transpose :443-452 into the image that
 * the k x k / stride-k VALID conv :455-483 reads).
 * x [N, H, W, C] f32 NHWC, UNPADDED: fix_padding's zero ring (:376) of pb
 * leading / pe trailing pixels is implied, never materialised (a corner in
 * the ring reads 0).  offsets: rows of off_stride >= 2*G*k*k floats per
 * output pixel (n, oh, ow), channel (g*k*k + t)*2 + {0: dy, 1: dx}, t = kh*k +
 * kw.  cols [N, OH, OW, k*k, C]: the column matrix whose product with
 * weights.reshape(k*k*C, Cout) is that conv.  OH = (H + pb + pe - k_eff) /
 * stride + 1 with k_eff = k + (k-1)(rate-1).  Positions, corner clipping and
 * the weights from the clipped corners follow the reference term by term
 * (f32, un-contracted).  k in {1, 3}; C % G == 0; (C/G) % 4 == 0; stride,
 * rate >= 1; x / cols 16-byte aligned. */
int d2mi_deform_sample_fwd(const float* x, const float* offsets, int N, int H, int W, int C,
                           int G, int k, int stride, int rate, int pb, int pe, int off_stride,
                           float* cols, void* stream);
/* Gradient of the above as TF autodiff forms it for convolutional.py:410-452
 * (floor passes nothing, clip_by_value passes inside [0, Hp-1], the clipped
 * corner floats are constants; gather_nd's gradient is a scatter-add).
 * gcols [N, OH, OW, k*k, C].  gx [N, H, W, C] (nullable): every element
 * written, no float atomics, bitwise reproducible (sorted destination keys,
 * fixed-order sums).  goffsets (nullable): rows of goff_stride floats, the
 * first 2*G*k*k as `offsets`, the rest (up to 16) written 0.  ws: at least
 * d2mi_deform_sample_bwd_workspace_size bytes (0 for a bad shape). */
size_t d2mi_deform_sample_bwd_workspace_size(int N, int H, int W, int C, int G, int k, int stride,
                                             int rate, int pb, int pe);
int d2mi_deform_sample_bwd(const float* x, const float* offsets, const float* gcols, int N, int H,
                           int W, int C, int G, int k, int stride, int rate, int pb, int pe,
                           int off_stride, int goff_stride, float* gx, float* goffsets, void* ws,
                           size_t ws_bytes, void* stream);

/* ------------------------------------- semantic segmentation / panoptic merge
 * SemSegFPNHead's tail without a full-resolution tensor
 * (lib/modeling/meta_arch/semantic_seg.py:197-218): resize_images(x, x scale)
 * -- the half-pixel ResizeBilinear, d2mi_resize_bilinear's arithmetic -- then
 * the mean over the not-ignored pixels of the sparse softmax cross-entropy,
 * times loss_weight.  logits [N, h, w, ldc] f32 (channels 0..C-1 of every
 * ldc-float row are the classes, C <= ldc); labels [N, Hl, Wl] int32 on the
 * [h*scale, w*scale] output grid's coordinates; image_shapes [N, 2] int32
 * true (h, w).  An output pixel counts unless its label equals ignore_value
 * (or is no class: outside [0, C)), or it lies outside the image's true shape
 * or the label extent (ImageList.from_tensors(..., pad_value=ignore_value),
 * semantic_seg.py:68-73, without the padded copy).  loss[0] = loss_weight *
 * sum / count, 0 when count[0] is 0.  Fixed-order sums (f64 accumulators,
 * per-workgroup partials, one ordered final pass): bitwise reproducible.
 * 1 <= scale <= 8; workspace from d2mi_sem_seg_loss_workspace_size. */
size_t d2mi_sem_seg_loss_workspace_size(int N, int h, int w);
int d2mi_sem_seg_loss_fwd(const float* logits, int N, int h, int w, int C, int ldc,
                          const int32_t* labels, int Hl, int Wl, const int32_t* image_shapes,
                          int ignore_value, int scale, float loss_weight, float* loss,
                          int32_t* count, void* workspace, size_t workspace_bytes, void* stream);
/* Gradient of the above w.r.t. logits (semantic_seg.py:197-218 through TF
 * autodiff), as a gather: grad_logits [N, h, w, ldc], every element written
 * (channels C..ldc-1 with 0), = grad_loss[0] * loss_weight / count[0] * the
 * sum over the output pixels whose bilinear footprint touches the pixel of
 * weight * (softmax - onehot), the softmax recomputed, summed in row-major
 * order of the output pixels.  count: d2mi_sem_seg_loss_fwd's (device);
 * grad_loss [1] f32 (device).  No atomics, bitwise reproducible. */
int d2mi_sem_seg_loss_bwd(const float* logits, int N, int h, int w, int C, int ldc,
                          const int32_t* labels, int Hl, int Wl, const int32_t* image_shapes,
                          int ignore_value, int scale, float loss_weight, const int32_t* count,
                          const float* grad_loss, float* grad_logits, void* stream);
/* sem_seg_postprocess(..., "conventional") + tf.argmax
 * (lib/modeling/postprocessing.py:62-95, lib/modeling/meta_arch/
 * panoptic_fpn.py:118-131; the resize of semantic_seg.py:197-201 before
 * them): out [N, h*scale, w*scale] int64 = the argmax over the C classes of
 * the interpolated logits (lowest index on ties) inside image_shapes[n], 0
 * outside (the argmax of the zero padding). */
int d2mi_sem_seg_argmax(const float* logits, int N, int h, int w, int C, int ldc,
                        const int32_t* image_shapes, int scale, int64_t* out, void* stream);
/* combine_semantic_and_instance_outputs (panoptic_fpn.py:160-296), N images.
 * masks [N, D, H, W] u8 (pasted, > 0 is set); scores [N, D] f32; classes
 * [N, D] int64; boxes [N, D, 4] f32; is_valid [N, D] u8; sem_seg [N, H, W]
 * int64.  Instances in descending score (ties: lower index); rank i has id
 * i + 1 and is applied when valid, score > conf_thresh, area > 0 and
 * (float)intersect / (float)area < overlap_thresh (integer pixel counts).
 * Stuff label l in [1, num_stuff_classes) has id D + l and claims the
 * still-empty pixels of its class when their count exceeds stuff_area_limit;
 * its bbox is their [ymin, xmin, ymax, xmax] (inclusive), else zeros.
 * panoptic_seg [N, H, W] int32; the seg_* arrays have D + num_stuff_classes
 * - 1 rows per image (seg_bbox x 4).  D + 3 launches: one per instance
 * (apply rank i from the device counters while counting rank i + 1, integer
 * atomics), two for the stuff labels.  No host read. */
size_t d2mi_panoptic_combine_workspace_size(int N, int D, int num_stuff_classes);
int d2mi_panoptic_combine(const uint8_t* masks, const float* scores, const int64_t* classes,
                          const float* boxes, const uint8_t* is_valid, const int64_t* sem_seg,
                          int N, int D, int H, int W, float overlap_thresh,
                          float stuff_area_limit, float conf_thresh, int num_stuff_classes,
                          int32_t* panoptic_seg, int32_t* seg_id, uint8_t* seg_isthing,
                          float* seg_score, int64_t* seg_category_id, int32_t* seg_instance_id,
                          float* seg_bbox, uint8_t* seg_is_valid, float* seg_area,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------ C4 head (Res5ROIHeads)
 * The two readers of the res5 output X [R, P, C] f32 (P = H*W) of
 * lib/modeling/roi_heads/roi_heads.py:345-373 in one pass over X:
 *   pooled[r, c] = (sum_p X[r, p, c]) / P    tf.reduce_mean(box_features, [1, 2])
 *   Y[dst[r]]    = X[r] where dst[r] >= 0    tf.gather(box_features, fg_inds)
 * The sum runs in increasing p from 0.f (one fixed order: bitwise
 * reproducible) and is divided by (float)P.  dst [R] int32 (nullable: no
 * gather): the row of Y [M, P, C] that takes X[r], or -1.  Precondition: the
 * values are in [-1, M) and no two rows name the same destination; rows of Y
 * no dst names are left unwritten.  (A value >= M is not dereferenced: the row
 * is skipped and bit 1 of the device error word is set.)  C % 4 == 0, P >= 1;
 * X, pooled, Y 16-byte aligned.  R == 0 is a no-op. */
int d2mi_res5_pool_fwd(const float* X, int R, int P, int C, const int32_t* dst, int M,
                       float* pooled, float* Y, void* stream);
/* Gradient of the above as the one gradient of X: every element of dX
 * [R, P, C] is written once,
 *   dX[r, p, c] = dpooled[r, c] / P + (dst[r] >= 0 ? dY[dst[r], p, c] : 0)
 * (no zero fill, no atomics, bitwise reproducible).  dY [M, P, C] and dst are
 * nullable (no gather: the broadcast alone); M bounds dst as in the forward. */
int d2mi_res5_pool_bwd(const float* dpooled, const float* dY, const int32_t* dst, int R, int P,
                       int C, int M, float* dX, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* D2MI_H */
