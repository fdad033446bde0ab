"""torch-facing wrappers of the libd2mi_hip.so hot-path kernels.

Every function here launches hand-written HIP on torch's current stream and
raises if the library is missing or a tensor is not on the GPU: there is no
CPU/eager fallback for the hot path.  Shapes and argument meaning follow the
reference op they replace (cited per function).

One module per kernel family, cut as csrc/ is; this
package re-exports their public functions, classes and constants.  The
process-wide toggles are not re-exported: each is an attribute of the one
module that owns it (roi.MERGED_BWD, roi.DEFER_PIXELS, conv.CONV_MATH,
relation.FUSED_RELATION, res5.FUSED_POOL, norm.FUSED_BN_TRAIN,
norm.FUSED_GN_TRAIN), read and written there.
"""
from ._common import (BOX_MODE_ALIGNED, BOX_MODE_RAW, BOX_MODE_UNALIGNED, get_tuning,  # noqa: F401
                      set_tuning)
from .boxes import (TOPK_MAX_K, apply_deltas, cascade_refine, grid_anchors,  # noqa: F401
                    match_boxes, match_boxes_masks, nms_segments, non_max_suppression,
                    roi_gt_classes, roi_sample_take, subsample, topk_segments)
from .conv import (CONV_FAMILIES, CONV_PLAN_FIELDS, LEVELS_PLAN_FIELDS, OP_ALIGNED,  # noqa: F401
                   OP_ALL_ALIGNED, OP_BIAS_ALIGNED, OP_GATE, OP_RESIDUAL, OP_TOPDOWN,
                   OP_WORKSPACE, OP_WS_ALIGNED, WGRAD_KERNELS, WGRAD_PLAN_FIELDS, RowCensus,
                   column_sum, conv2d_nhwc, conv2d_nhwc_levels, conv2d_wgrad, conv2d_wgrad_group,
                   conv_levels_plan, wgrad_group_plan, WGRAD_FAMILIES,
                   conv_plan, pack_conv_weights, pack_conv_weights_many, preprocess_images,
                   row_census, row_census_workspace_size, skinny_levels_ok, split_bf16x3,
                   stem_conv, stem_conv_weights, stem_pool, stride_scatter, upsample2x_grad,
                   wgrad_plan, wgrad_skinny, wgrad_skinny_levels)
from .deform import deform_sample, deform_sample_bwd  # noqa: F401
from .detect import (ACT_LEAKY_RELU, ACT_MISH, activation_, fast_rcnn_inference,  # noqa: F401
                     fast_rcnn_inference_stages, matrix_nms_scores, paste_masks,
                     retinanet_inference, rpn_head_gather, rpn_head_scatter, rpn_proposals,
                     solo_inference, spp_pool, yolo_host_arrays, yolov4_inference,
                     yolov4_predictions)
from .fold import fold_frozen_bn, fold_frozen_bn_many  # noqa: F401
from .losses import (fast_rcnn_loss, mask_loss, retina_loss, rpn_loss,  # noqa: F401
                     scale_gradient, yolov4_loss)
from .norm import (batch_norm_train, gn_train_fused, group_norm, group_norm_levels,  # noqa: F401
                   group_norm_train, resize_bilinear, resize_bilinear_grad)
from .relation import relation_attention, relation_supported  # noqa: F401
from .res5 import res5_pool, res5_pool_dense  # noqa: F401
from .roi import DeferredPixels, roi_align, roi_touched_rows  # noqa: F401
from .sem_seg import panoptic_combine, sem_seg_argmax, sem_seg_loss  # noqa: F401
from .timing import F32_RIDGE, SPLIT_RIDGE, KernelTimer, bound_of, conv_bytes  # noqa: F401
