"""The Relation Networks attention (csrc/relation.hip): geometry embedding,
geometry weights, grouped softmax attention and the value product of
ObjectRelationModule in one forward launch, differentiable w.r.t. q, k, v and
the geometry conv."""
import torch

from ... import _C
from ._common import _f32c, _mask_u8

# True: the relation module runs the fused kernels on the GPU; False: its
# tensor formulation (modeling.roi_heads.relation_module.relation_dense).
# Tests and tools/relation_ab.py compare the two.  Off by default: the fused
# forward is ahead of the tensor formulation (inference, R = 1000) but the
# fused forward + backward is behind it at the training shape
# (profiles/relation_ab.json, DESIGN.md section 5 "Relation head").
FUSED_RELATION = False

G_MAX, DK_MAX, DV_MAX, E_MAX = 16, 8, 64, 128


def relation_supported(num_groups, dk, dv, embedding_dim):
    """The kernels' envelope (d2mi_relation_fwd); outside it the module takes
    its tensor formulation."""
    return (1 <= num_groups <= G_MAX and 1 <= dk <= DK_MAX
            and dv % 4 == 0 and 4 <= dv <= DV_MAX
            and embedding_dim % 8 == 0 and 8 <= embedding_dim <= E_MAX)


class _RelationFn(torch.autograd.Function):
    """out [N, R, G*dv] of d2mi_relation_fwd / d2mi_relation_bwd; the forward
    saves its output and the per-(row, group) log-sum-exp."""

    @staticmethod
    def forward(ctx, boxes, valid, q, k, v, wg, bg, G):
        N, R = valid.shape
        dk, dv, E = q.shape[-1] // G, v.shape[-1], wg.shape[0]
        dev = q.device
        out = torch.empty((N, R, G * dv), dtype=torch.float32, device=dev)
        lse = torch.empty((N, R, 2, G), dtype=torch.float32, device=dev)  # (max, sum)
        rc = _C.lib().d2mi_relation_fwd(_C.ptr(boxes), _C.ptr(valid), _C.ptr(q), _C.ptr(k),
                                        _C.ptr(v), _C.ptr(wg), _C.ptr(bg), N, R, G, dk, dv, E,
                                        _C.ptr(out), _C.ptr(lse), _C.stream_of(dev))
        _C.check(rc, "d2mi_relation_fwd")
        ctx.save_for_backward(boxes, valid, q, k, v, wg, bg, out, lse)
        ctx.G = G
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        boxes, valid, q, k, v, wg, bg, out, lse = ctx.saved_tensors
        if g is None:
            return (None,) * 8
        G = ctx.G
        N, R = valid.shape
        dk, dv, E = q.shape[-1] // G, v.shape[-1], wg.shape[0]
        dev = q.device
        g = _f32c(g)
        d_q, d_k, d_v = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        d_wg, d_bg = torch.empty_like(wg), torch.empty_like(bg)
        lib = _C.lib()
        wsb = lib.d2mi_relation_workspace_size(N, R, G, dk, dv, E)
        ws = _C.scratch(wsb, dev)
        rc = lib.d2mi_relation_bwd(_C.ptr(boxes), _C.ptr(valid), _C.ptr(q), _C.ptr(k), _C.ptr(v),
                                   _C.ptr(wg), _C.ptr(bg), _C.ptr(out), _C.ptr(lse), _C.ptr(g), N,
                                   R, G, dk, dv, E, _C.ptr(d_q), _C.ptr(d_k), _C.ptr(d_v),
                                   _C.ptr(d_wg), _C.ptr(d_bg), _C.ptr(ws), wsb, _C.stream_of(dev))
        _C.check(rc, "d2mi_relation_bwd")
        return None, None, d_q, d_k, d_v, d_wg, d_bg, None


def relation_attention(boxes, valid, q, k, v, wg, bg, num_groups):
    """Fused relation attention (relation_module.py:29-89, :141-194): boxes
    [N, R, 4] yxyx, valid [N, R], q / k [N, R, G*dk], v [N, R, dv], wg [E, G]
    (the geometry 1x1 conv's weights), bg [G] -> [N, R, G*dv], the attention
    output before the residual, zero rows for invalid slots.  Invalid slots
    take part as zeros (box 0, q = k = v = 0) in every row's softmax."""
    G = int(num_groups)
    boxes, q, k, v = _f32c(boxes), _f32c(q), _f32c(k), _f32c(v)
    wg, bg = _f32c(wg.reshape(-1, G)), _f32c(bg)
    valid = _mask_u8(valid)
    _C.require_device(boxes, valid, q, k, v, wg, bg)
    N, R = valid.shape
    if (boxes.shape != (N, R, 4) or q.shape != k.shape or q.shape[:2] != (N, R)
            or v.shape[:2] != (N, R) or q.shape[-1] % G or bg.shape != (G,)):
        raise ValueError(f"relation attention: boxes {tuple(boxes.shape)}, q {tuple(q.shape)}, "
                         f"k {tuple(k.shape)}, v {tuple(v.shape)}, bg {tuple(bg.shape)} do not "
                         f"match valid {tuple(valid.shape)} and G={G}")
    return _RelationFn.apply(boxes, valid, q, k, v, wg, bg, G)
