// The pairwise IoU of the matcher (box_list_ops.pairwise_iou, :295-372) for
// one pair of yxyx boxes, shared by match.hip and cascade.hip.
//
// Float sequence: ih = min(y2a,y2b) - max(y1a,y1b) clamped at 0, iw the
// same, inter = ih * iw, union = (area_a + area_b) - inter, inter / union
// (0 when union == 0): the tensor code's order, so labels are identical.
#pragma once
#include "common.h"

namespace d2mi {

__device__ __forceinline__ float iou_of(const float4 a, const float4 b) {
  const float ih = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
  const float iw = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
  const float inter = ih * iw;
  const float area_a = (a.z - a.x) * (a.w - a.y);
  const float area_b = (b.z - b.x) * (b.w - b.y);
  const float uni = area_a + area_b - inter;
  return uni == 0.f ? 0.f : inter / uni;
}

}  // namespace d2mi
