"""Res5ROIHeads, the C4 head (lib/modeling/roi_heads/roi_heads.py:261-408).

The tensor formulations it runs for CPU tensors are in res5_dense.py.
"""
import torch

from ...layers import ShapeSpec, ops
from ...utils import host_sync
from ..poolers import ROIPooler
from .fast_rcnn import FastRCNNOutputLayers
from .mask_head import build_mask_head
from .roi_heads import ROI_HEADS_REGISTRY, StandardROIHeads, _cached_index


@ROI_HEADS_REGISTRY.register()
class Res5ROIHeads(StandardROIHeads):
    """One pooler on res4, the res5 stage over the pooled rows, the box
    predictor on their spatial mean and the mask head on rows of the same res5
    output.

    The step (sampling, the mask plan with its fg-first rows, the
    foreground-count read, the MASK_ROW_BUCKET padding, inference) is
    StandardROIHeads'; this class supplies the heads, the losses over one
    pooling and one res5 per training step, and the shared transform at
    inference.  The mean and the mask rows' gather are one launch
    (ops.res5_pool), and so is their backward.  Training is eager: the count
    read sits inside the forward (mask_loss_deferrable False; engine.graphed
    refuses the head), and the mask rows are always the compacted fg-first ones.

    ELIDE_STRIDE: with STRIDE_IN_1X1, an even POOLER_RESOLUTION 2n and
    POOLER_SAMPLING_RATIO 0, block_1's two stride-2 1x1 convs read only the
    even grid of the 2n x 2n crop, which is itself an n x n crop of a modified
    box (_even_grid_boxes): pool that and run block_1 at stride 1, the same
    weights.  Any other setting pools the full crop.
    Deviation: the reference's training branch reads an
    undefined name and hands the mask head's tuple to the loss; the evident
    intent, the loss on the head's mask logits, is what runs here."""
    # On by default: ahead of the literal path in tools/res5_ab.py (1.02x at
    # inference on 1000 proposals, 6.4x in training on 2 x 512 rows:
    # profiles/res5_ab.json, DESIGN.md section 5 "C4 head").
    ELIDE_STRIDE = True
    # (the pooled map has one reader, the head: no RPN / pooler gradient pair)
    merged_pool_backward = False
    # (the mask rows are gathered from the shared res5 output inside the
    # forward, after the foreground-count read)
    mask_loss_deferrable = False

    def _init_box_head(self, cfg):
        from ..backbone.resnet import BottleneckBlock, Stage, resnet_arg_scope
        from ...layers.conv_weights import FoldGroup
        assert len(self.in_features) == 1
        b, r = cfg.MODEL.ROI_BOX_HEAD, cfg.MODEL.RESNETS
        res = b.POOLER_RESOLUTION
        scales = (1.0 / self.feature_strides[self.in_features[0]],)
        self.pooler = ROIPooler(res, scales, b.POOLER_SAMPLING_RATIO, b.POOLER_TYPE)
        assert not r.DEFORM_ON_PER_STAGE[-1], "Deformable conv is not yet supported in res5 head."
        out_channels = r.RES2_OUT_CHANNELS * 8  # res5 is 8x res2
        kw = {"in_channels": out_channels // 2, "out_channels": out_channels,
              "bottleneck_channels": r.NUM_GROUPS * r.WIDTH_PER_GROUP * 8,
              "num_groups": r.NUM_GROUPS, "stride_in_1x1": r.STRIDE_IN_1X1}
        with resnet_arg_scope(False, r.NORM):
            self.res5 = Stage(BottleneckBlock, block_kwargs=kw, num_blocks=3, first_stride=2,
                              scope="res5")
        FoldGroup.attach(self.res5)
        self.out_channels = out_channels
        # the elision's n x n pooler, where its conditions hold
        self.half_pooler = None
        if r.STRIDE_IN_1X1 and b.POOLER_SAMPLING_RATIO == 0 and res % 2 == 0:
            self.half_pooler = ROIPooler(res // 2, scales, 0, b.POOLER_TYPE)
        self.box_predictor = FastRCNNOutputLayers(out_channels, self.num_classes,
                                                  self.cls_agnostic_bbox_reg, scope="fastrcnn")

    def _init_mask_head(self, cfg):
        res = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
        self.mask_head = build_mask_head(
            cfg, ShapeSpec(channels=self.out_channels, width=res, height=res), scope="mask_head")

    def elides(self):
        return self.ELIDE_STRIDE and self.half_pooler is not None

    def _even_grid_boxes(self, boxes):
        """The boxes whose n x n crop is the even grid (2i, 2j) of ``boxes``'
        2n x 2n crop.  ROIAlignV2 (aligned, sample i at y0 + (i + 1/2) h / 2n):
        the same size, moved up and left by a quarter bin of the n x n crop,
        (h / 4n, w / 4n).  ROIAlign (tf.image.crop_and_resize spacing h / (2n -
        1) from y0): the same corner, the size scaled by (2n - 2) / (2n - 1)."""
        n = self.half_pooler.output_size[0]
        hw = boxes[:, 2:] - boxes[:, :2]
        if self.pooler.aligned:
            q = hw / (4.0 * n)
            return torch.cat([boxes[:, :2] - q, boxes[:, 2:] - q], 1)
        return torch.cat([boxes[:, :2], boxes[:, :2] + hw * ((2.0 * n - 2.0) / (2.0 * n - 1.0))], 1)

    def _pool(self, feats, boxes, img):
        """The res5 input of boxes [R, 4]: (rows [R, h, w, C], the stride block_1 runs at)."""
        pooler, stride = self.pooler, None
        if self.elides():
            pooler, stride, boxes = self.half_pooler, 1, self._even_grid_boxes(boxes)
        if feats[0].is_cuda:
            return pooler.pool(feats, boxes.contiguous(), img), stride
        from ...layers.ops import BOX_MODE_ALIGNED, BOX_MODE_UNALIGNED
        from .res5_dense import crop_and_resize_dense
        if pooler.sampling_ratio > 0:
            raise NotImplementedError("the crop's tensor formulation takes one sample per bin")
        mode = BOX_MODE_ALIGNED if pooler.aligned else BOX_MODE_UNALIGNED
        return crop_and_resize_dense(feats[0], boxes, img, pooler.output_size, pooler.scales[0],
                                     mode), stride

    def _res5(self, x, stride=None):
        if not x.is_cuda:
            from .res5_dense import stage_dense
            return stage_dense(self.res5, x, stride)
        if stride is None:
            return self.res5(x)
        # block_1 at ``stride``: its strided convs read their stride at call time
        strided = [c for c in (self.res5.blocks[0].shortcut, self.res5.blocks[0].conv1)
                   if c is not None and c.stride > 1]
        saved = [c.stride for c in strided]
        try:
            for c in strided:
                c.stride = stride
            return self.res5(x)
        finally:
            for c, s in zip(strided, saved):
                c.stride = s

    def _shared_roi_transform(self, feats, boxes, img):
        x, stride = self._pool(feats, boxes, img)
        return self._res5(x, stride)

    def _pool_gather(self, x, dst=None, rows=0):
        """(the spatial mean [R, C], the rows dst names [rows, h, w, C] or None)
        of the res5 output x [R, h, w, C]."""
        R, h, w, C = x.shape
        fn = ops.res5_pool if x.is_cuda and ops.res5.FUSED_POOL and C % 4 == 0 \
            else ops.res5_pool_dense
        pooled, y = fn(x.reshape(R, h * w, C), dst, rows)
        return pooled, (y.reshape(rows, h, w, C) if y is not None else None)

    def _mask_head(self, x):
        if x.is_cuda:
            return self.mask_head(x)
        from .res5_dense import mask_head_dense
        return mask_head_dense(self.mask_head, x)

    def _mask_dst(self, fg, rows, N, S):
        """dst [N*S] int32 of the gather: mask row m < rows is the m-th slot
        of _mask_prep's order (fg first, each group in slot order) over the
        first F slots per image; slot k of that [N, F] layout is sampled row
        (k // F) * S + k % F."""
        F_ = fg.numel() // N
        order = torch.argsort((~fg).to(torch.uint8), stable=True)[:rows]
        src = torch.div(order, F_, rounding_mode="floor") * S + order % F_
        dst = torch.full((N * S,), -1, dtype=torch.int32, device=fg.device)
        dst[src] = torch.arange(rows, dtype=torch.int32, device=fg.device)
        return dst

    def _losses(self, feats, sampled, plan, images, targets):
        """One pooling and one res5 for both branches; the foreground count is
        read while they are enqueued."""
        if self.mask_on and not self.mask_compact_rows:
            raise NotImplementedError(
                "Res5ROIHeads runs its mask branch on compacted fg-first rows only "
                "(mask_compact_rows False would pair the gathered rows with other targets)")
        if self.mask_on:
            plan = self._prepared(plan, sampled, targets)
        boxes = sampled["boxes"]
        N, S = boxes.shape[:2]
        img = _cached_index("img", N, S, boxes.device)
        x = self._shared_roi_transform(feats, boxes.reshape(-1, 4), img)
        dst, rows = None, 0
        if self.mask_on:
            rows = self.mask_rows(host_sync.finish_read(plan.pending)[0], plan.fg_slots.numel())
            self.last_mask_rows = rows
            dst = self._mask_dst(plan.fg_slots, rows, N, S)
        pooled, mask_x = self._pool_gather(x, dst, rows)
        losses = self._predictor_losses(pooled, sampled)
        if self.mask_on:
            _, mask_logits = self._mask_head(mask_x)
            losses["loss_mask"] = self._mask_rcnn_loss(mask_logits, plan.head(rows))
        return losses

    def _forward_box(self, feats, proposals, image_shapes):
        boxes, _, img, slot, N, P = self._proposal_rows(proposals)
        x = self._shared_roi_transform(feats, boxes.reshape(-1, 4), img)
        return self._predict(self._pool_gather(x)[0], boxes, img, slot, N, P, image_shapes)

    def _mask_outputs(self, feats, boxes, img):
        # the detections through the same pooler and res5 as the proposals
        return self._mask_head(self._shared_roi_transform(feats, boxes, img))
