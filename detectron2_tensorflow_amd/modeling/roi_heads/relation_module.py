"""ObjectRelationModule (lib/modeling/roi_heads/relation_module.py:29-194).

Relation Networks for Object Detection: every proposal of an image attends
to every other through G groups whose logits add a learned geometry weight
(the pair's relative position, embedded into E sin / cos channels and put
through a 1x1 conv + ReLU) to a scaled query . key product; the attention's
output is added to the features.

On the GPU the attention runs as ops.relation_attention (csrc/relation.hip),
which recomputes the embedding per pair and writes no R x R tensor.
``relation_dense`` is the tensor formulation of the same math, in any dtype:
the CPU path, the path outside the kernels' envelope, the path with
ops.relation.FUSED_RELATION off, and the tests' differentiable reference.

Dense layout: features [N*R, C] with boxes [N, R, 4] and the is_valid mask
[N, R].  An invalid slot takes part as the reference's
SparseBoxList.to_dense leaves it -- box 0 and q = k = v = 0, zeros and not
the Linear's bias -- and its output row is the unchanged feature row (the
reference returns the valid rows only).  Reproduced quirks (DESIGN.md
section 9): the centre offsets carry no absolute value, so a negative offset
clamps to log 1e-5, and the softmax runs over all R columns, the invalid ones
included.  compute_rank_embeddings is not ported: it is dead code in the
reference and names an undefined variable.
"""
import math

import torch

from ...layers import Layer, Linear
from ...layers import initializers as init
from ...layers.ops import relation as _relation

WAVE_LENGTH = 1000.0


def geometry_embeddings(boxes, embedding_dim=64):
    """compute_geometry_embeddings (relation_module.py:29-89): boxes [N, R, 4]
    yxyx -> [N, R, R, E], channel t (E/4) + s (E/8) + f = sin (s = 0) or cos
    (s = 1) of 100 p_t / 1000^(8 f / E) for the pair's four log-ratios p_t."""
    assert embedding_dim % 8 == 0, embedding_dim
    y1, x1, y2, x2 = boxes.unbind(-1)
    h, w = y2 - y1 + 1.0, x2 - x1 + 1.0
    cy, cx = 0.5 * (y1 + y2), 0.5 * (x1 + x2)
    # (no absolute value: the reference's, :54-61)
    dy = torch.log(torch.clamp_min((cy[:, :, None] - cy[:, None, :]) / h[:, :, None], 1e-5))
    dx = torch.log(torch.clamp_min((cx[:, :, None] - cx[:, None, :]) / w[:, :, None], 1e-5))
    dh = torch.log(h[:, :, None] / h[:, None, :])
    dw = torch.log(w[:, :, None] / w[:, None, :])
    pos = torch.stack([dy, dx, dh, dw], dim=3)  # [N, R, R, 4]
    feat = torch.arange(embedding_dim // 8, dtype=boxes.dtype, device=boxes.device)
    dim = torch.pow(torch.tensor(WAVE_LENGTH, dtype=boxes.dtype, device=boxes.device),
                    (8.0 / embedding_dim) * feat)
    div = (100.0 * pos)[..., None] / dim  # [N, R, R, 4, E/8]
    emb = torch.cat([torch.sin(div), torch.cos(div)], dim=4)
    return emb.reshape(*emb.shape[:3], embedding_dim)


def relation_dense(boxes, valid, q, k, v, wg, bg, num_groups):
    """The attention of ObjectRelationModule.call (:160-192) as tensors:
    boxes [N, R, 4], valid [N, R], q / k [N, R, G*dk], v [N, R, dv], wg [E, G],
    bg [G] -> [N, R, G*dv], zero rows for invalid slots.  Builds the
    [N, R, R, E] embedding: the formulation ops.relation_attention avoids."""
    G = int(num_groups)
    N, R = valid.shape
    dt = q.dtype
    m = valid.to(dt)[..., None]
    boxes, q, k, v = boxes.to(dt) * m, q * m, k * m, v * m
    wg = wg.reshape(-1, G)
    emb = geometry_embeddings(boxes, wg.shape[0])
    gw = torch.relu(emb @ wg + bg)  # [N, R, R, G]
    dk = q.shape[-1] // G
    qg = q.reshape(N, R, G, dk).permute(0, 2, 1, 3)
    kg = k.reshape(N, R, G, dk).permute(0, 2, 1, 3)
    app = (qg @ kg.transpose(2, 3)) / math.sqrt(dk)  # [N, G, R, R]
    logit = torch.log(torch.clamp_min(gw, 1e-6)).permute(0, 1, 3, 2) + app.permute(0, 2, 1, 3)
    p = torch.softmax(logit, dim=3)  # [N, R, G, R]
    out = p.reshape(N, R * G, R) @ v  # the value is shared by the groups
    return out.reshape(N, R, G * v.shape[-1]) * m


class _Geometry(Layer):
    """The variables of the reference's 1x1 Conv2D E -> G ("geometry/weights"
    [1, 1, E, G], "geometry/bias" [G]); the conv itself is part of the
    attention op."""

    def __init__(self, embedding_dim, num_groups, **kwargs):
        super().__init__(**kwargs)
        w = torch.empty((1, 1, int(embedding_dim), int(num_groups)))
        init.variance_scaling(2.0, distribution="untruncated_normal")(w)
        self.weights = torch.nn.Parameter(w)
        self.bias = torch.nn.Parameter(torch.zeros(int(num_groups)))


class ObjectRelationModule(Layer):
    def __init__(self, input_size, embedding_dim=64, key_dim=64, num_groups=16, **kwargs):
        super().__init__(input_size=int(input_size), embedding_dim=int(embedding_dim),
                         key_dim=int(key_dim), num_groups=int(num_groups), **kwargs)
        assert self.key_dim % self.num_groups == 0, (
            f"`key_dim`({self.key_dim}) is not divisible by `num_groups`({self.num_groups}).")
        assert self.input_size % self.num_groups == 0, (self.input_size, self.num_groups)
        assert self.embedding_dim % 8 == 0, self.embedding_dim
        self.geometry = _Geometry(self.embedding_dim, self.num_groups, scope="geometry")
        self.query = Linear(self.input_size, self.key_dim, scope="query")
        self.key = Linear(self.input_size, self.key_dim, scope="key")
        self.value = Linear(self.input_size, self.input_size // self.num_groups, scope="value")

    def fused(self, features):
        """Whether this call runs ops.relation_attention."""
        return (features.is_cuda and _relation.FUSED_RELATION and features.dtype is torch.float32
                and _relation.relation_supported(self.num_groups, self.key_dim // self.num_groups,
                                                 self.input_size // self.num_groups,
                                                 self.embedding_dim))

    def call(self, features, boxes, valid):
        """features [N*R, input_size], boxes [N, R, 4], valid [N, R] ->
        features + attention, [N*R, input_size]."""
        N, R = valid.shape
        q = self.query(features).reshape(N, R, -1)
        k = self.key(features).reshape(N, R, -1)
        v = self.value(features).reshape(N, R, -1)
        wg = self.geometry.weights.reshape(self.embedding_dim, self.num_groups)
        attend = _relation.relation_attention if self.fused(features) else relation_dense
        out = attend(boxes, valid, q, k, v, wg, self.geometry.bias, self.num_groups)
        return features + out.reshape(N * R, self.input_size).to(features.dtype)
