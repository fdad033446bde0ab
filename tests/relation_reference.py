"""A literal float64 restatement of the reference's relation module
(lib/modeling/roi_heads/relation_module.py:29-89 compute_geometry_embeddings,
:141-194 ObjectRelationModule.call), statement by statement in torch so that
autograd differentiates it.  Written from the reference text, not from
modeling.roi_heads.relation_module.relation_dense: the tests compare the two.

Inputs are the dense [N, R] layout; the reference's SparseBoxList.to_dense
(structures/box_list.py:204-246) scatters the valid rows into zeros, which is
the masking step here.
"""
import math

import torch

F64 = torch.float64


def to_dense(t, valid):
    """Valid rows kept, every other row zero."""
    return torch.where(valid[..., None], t, torch.zeros_like(t))


def geometry_embeddings(boxes, embedding_dim=64, wave_length=1000):
    """:45-87 on dense boxes [N, R, 4] -> [N, R, R, embedding_dim]."""
    assert embedding_dim % 8 == 0, embedding_dim
    ymin, xmin, ymax, xmax = torch.split(boxes, 1, dim=2)  # [N, R, 1]
    height = ymax - ymin + 1.
    width = xmax - xmin + 1.
    center_y = 0.5 * (ymin + ymax)
    center_x = 0.5 * (xmin + xmax)

    delta_y = (center_y - center_y.permute(0, 2, 1)) / height  # [N, R, R]
    delta_y = torch.log(torch.maximum(delta_y, torch.tensor(1e-5, dtype=boxes.dtype)))
    delta_x = (center_x - center_x.permute(0, 2, 1)) / width
    delta_x = torch.log(torch.maximum(delta_x, torch.tensor(1e-5, dtype=boxes.dtype)))
    delta_height = torch.log(height / height.permute(0, 2, 1))
    delta_width = torch.log(width / width.permute(0, 2, 1))

    concat_list = [delta_y, delta_x, delta_height, delta_width]
    for idx, value in enumerate(concat_list):
        concat_list[idx] = value.unsqueeze(3)  # [N, R, R, 1]
    position_matrix = torch.cat(concat_list, dim=3)  # [N, R, R, 4]

    feat_range = torch.arange(int(embedding_dim / 8.), dtype=boxes.dtype, device=boxes.device)
    dim_matrix = torch.pow(torch.tensor(float(wave_length), dtype=boxes.dtype,
                                        device=boxes.device),
                           (8. / embedding_dim) * feat_range)
    dim_matrix = dim_matrix.reshape(1, 1, 1, 1, -1)
    position_matrix = (100.0 * position_matrix).unsqueeze(4)  # [N, R, R, 4, 1]
    div_matrix = position_matrix / dim_matrix  # [N, R, R, 4, E / 8]
    embeddings = torch.cat([torch.sin(div_matrix), torch.cos(div_matrix)], dim=4)
    shape = embeddings.shape
    return embeddings.reshape(shape[0], shape[1], shape[2], embedding_dim)


def relation(boxes, valid, q, k, v, wg, bg, num_groups):
    """:160-192 on the dense layout: returns the attention output [N, R, G*dv]
    with the rows of invalid slots zero (the reference gathers the valid rows;
    the residual is added by the caller).  wg [E, G] is the 1x1 conv's
    [1, 1, E, G] kernel."""
    valid = valid.bool()
    boxes, query, key, value = (to_dense(t.to(F64), valid) for t in (boxes, q, k, v))
    wg, bg = wg.to(F64), bg.to(F64)
    N, R = valid.shape
    G = num_groups
    key_dim = query.shape[-1]
    input_size = value.shape[-1] * G
    geometry_embeddings_ = geometry_embeddings(boxes, wg.shape[0])
    # self.geometry: Conv2D 1x1, E -> G, ReLU
    geometry_weight = torch.relu(torch.einsum("nijc,cg->nijg", geometry_embeddings_, wg) + bg)
    geometry_weight = geometry_weight.permute(0, 1, 3, 2)  # [N, R, G, R]

    query = query.reshape(N, R, G, int(key_dim / G)).permute(0, 2, 1, 3)
    key = key.reshape(N, R, G, int(key_dim / G)).permute(0, 2, 1, 3)
    dot = torch.matmul(query, key.transpose(2, 3))
    scaled_dot = dot / math.sqrt(key_dim / G)
    appearance_weight = scaled_dot.permute(0, 2, 1, 3)  # [N, R, G, R]

    relation_weight = torch.log(torch.maximum(geometry_weight, torch.tensor(1e-6, dtype=F64))) \
        + appearance_weight
    relation_weight = torch.softmax(relation_weight, dim=3)
    relation_weight = relation_weight.reshape(N, R * G, R)
    output = torch.matmul(relation_weight, value)  # [N, R * G, input_size / G]
    output = output.reshape(N, R, input_size)
    return to_dense(output, valid)
