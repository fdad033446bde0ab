"""The layers/ops package: one owner per process-wide toggle, and the public
surface the single ops.py module had (CPU only: imports, no launch)."""
import importlib
import pkgutil

TOGGLES = {"MERGED_BWD": "layers.ops.roi", "DEFER_PIXELS": "layers.ops.roi",
           "CONV_MATH": "layers.ops.conv",
           "FUSED_SAMPLE_TAKE": "modeling.roi_heads.roi_heads",
           "FUSED_PREPROCESS": "modeling.meta_arch.rcnn"}

# dir(ops) of the single-module ops.py, modules and underscore names left out
# (97 names, the five toggles among them).  A subset check: later additions
# do not touch it.
PUBLIC = (
    "ACT_LEAKY_RELU", "ACT_MISH", "BOX_MODE_ALIGNED", "BOX_MODE_RAW", "BOX_MODE_UNALIGNED",
    "CONV_FAMILIES", "CONV_MATH", "CONV_PLAN_FIELDS", "DEFER_PIXELS", "DeferredPixels",
    "F32_RIDGE", "FUSED_PREPROCESS", "FUSED_SAMPLE_TAKE", "KernelTimer", "LEVELS_PLAN_FIELDS",
    "MERGED_BWD", "OP_ALIGNED", "OP_ALL_ALIGNED", "OP_BIAS_ALIGNED", "OP_GATE", "OP_RESIDUAL",
    "OP_TOPDOWN", "OP_WORKSPACE", "OP_WS_ALIGNED", "RowCensus", "SPLIT_RIDGE", "TOPK_MAX_K",
    "WGRAD_KERNELS", "WGRAD_PLAN_FIELDS", "activation_", "apply_deltas", "bound_of",
    "cascade_refine", "column_sum", "conv2d_nhwc", "conv2d_nhwc_levels", "conv2d_wgrad",
    "conv_bytes", "conv_levels_plan", "conv_plan", "deform_sample", "deform_sample_bwd",
    "fast_rcnn_inference", "fast_rcnn_inference_stages", "fast_rcnn_loss", "fold_frozen_bn",
    "fold_frozen_bn_many", "get_tuning", "grid_anchors", "group_norm", "group_norm_levels",
    "mask_loss", "match_boxes", "match_boxes_masks", "matrix_nms_scores", "nms_segments",
    "non_max_suppression", "pack_conv_weights", "pack_conv_weights_many", "panoptic_combine",
    "paste_masks", "preprocess_images", "resize_bilinear", "resize_bilinear_grad", "retina_loss",
    "retinanet_inference", "roi_align", "roi_gt_classes", "roi_sample_take", "roi_touched_rows",
    "row_census", "row_census_workspace_size", "rpn_head_gather", "rpn_head_scatter", "rpn_loss",
    "rpn_proposals", "scale_gradient", "sem_seg_argmax", "sem_seg_loss", "set_tuning",
    "skinny_levels_ok", "solo_inference", "split_bf16x3", "spp_pool", "stem_conv",
    "stem_conv_weights", "stem_pool", "stride_scatter", "subsample", "topk_segments",
    "upsample2x_grad", "wgrad_plan", "wgrad_skinny", "wgrad_skinny_levels", "yolo_host_arrays",
    "yolov4_inference", "yolov4_predictions")


def test_each_toggle_has_one_owner():
    """No toggle is an attribute of the package (a write there would reach no
    reader); among the package's modules, roi_heads.py and rcnn.py exactly one
    module holds each name, so no import has copied its value."""
    from detectron2_tensorflow_amd.layers import ops
    pkg = "detectron2_tensorflow_amd."
    names = [m.name for m in pkgutil.iter_modules(ops.__path__, pkg + "layers.ops.")]
    names += [pkg + "modeling.roi_heads.roi_heads", pkg + "modeling.meta_arch.rcnn"]
    modules = [importlib.import_module(n) for n in names]
    for toggle, owner in TOGGLES.items():
        assert not hasattr(ops, toggle), toggle
        assert [m.__name__ for m in modules if hasattr(m, toggle)] == [pkg + owner], toggle


def test_public_surface_kept():
    from detectron2_tensorflow_amd.layers import ops
    assert len(PUBLIC) == 97 and set(TOGGLES) < set(PUBLIC)
    missing = [n for n in PUBLIC if n not in TOGGLES and not hasattr(ops, n)]
    assert not missing, missing
