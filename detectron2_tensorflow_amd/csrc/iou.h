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

// The complete IoU of one pair of yxyx boxes (box_list_ops.py:335-371
// pairwise_iou and :415-449 matched_iou, iou_type "ciou"), shared by the
// forward and backward kernels of yolo_loss.hip:
//   iou   as iou_of (0 when the union is 0)
//   diou  = iou - d^2 / c^2: d the distance of the centres, c the diagonal of
//           the enclosing box (the fraction counts as 0 when c^2 == 0)
//   v     = 4 / pi^2 (atan(w_a / h_a) - atan(w_b / h_b))^2
//   alpha = v / (1 - iou + v)
//   ciou  = diou - alpha v
// a is the reference's boxlist1, b its boxlist2.  wb is b's width AS THE
// CALLER STATES IT: pairwise_iou has x_max2 - x_min2 (:325), matched_iou has
// x_max1 - x_min2 (:405, the first list's x_max), and that value feeds both
// b's area and the atan term.  at_a / at_b are atan(w_a / h_a) and
// atan(wb / h_b): the caller computes each box's once.  Where 1 - iou + v == 0
// (coincident boxes) the reference divides 0 by 0; alpha v is 0 here.
constexpr float kCiouV = 0.40528473456935109f;  // 4 / pi^2, rounded where it meets a tensor

__device__ __forceinline__ float box_atan(float w, float h) { return atanf(w / h); }

__device__ __forceinline__ float ciou_of(const float4 a, float at_a, const float4 b, float wb,
                                         float at_b) {
  const float ih = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
  const float iw = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
  const float inter = ih * iw;
  const float area_a = (a.z - a.x) * (a.w - a.y);
  const float area_b = (b.z - b.x) * wb;
  const float uni = area_a + area_b - inter;
  const float iou = uni == 0.f ? 0.f : inter / uni;
  const float ch = fmaxf(a.z, b.z) - fminf(a.x, b.x);
  const float cw = fmaxf(a.w, b.w) - fminf(a.y, b.y);
  const float c2 = ch * ch + cw * cw;
  const float dx = (a.y + a.w) / 2.f - (b.y + b.w) / 2.f;
  const float dy = (a.x + a.z) / 2.f - (b.x + b.z) / 2.f;
  const float d2 = dx * dx + dy * dy;
  const float diou = iou - (c2 == 0.f ? 0.f : d2 / c2);
  const float t = at_a - at_b;
  const float v = kCiouV * (t * t);
  const float den = 1.f - iou + v;
  return diou - (den == 0.f ? 0.f : v / den * v);
}

// The partial derivatives of ciou_of with respect to a's four coordinates
// (da, yxyx) and to wb (dwb), b fixed: what TF's autodiff of the expressions
// above gives, alpha and v included.  min / max pass their gradient to the
// first argument on a tie (a's coordinate: tf.minimum / tf.maximum), the clamp
// at 0 passes none at 0 (tf.maximum(0.0, x)).
struct CiouGrad {
  float4 da;
  float dwb;
};

__device__ __forceinline__ CiouGrad ciou_grad(const float4 a, const float4 b, float wb) {
  const float ihr = fminf(a.z, b.z) - fmaxf(a.x, b.x);
  const float iwr = fminf(a.w, b.w) - fmaxf(a.y, b.y);
  const float ih = fmaxf(ihr, 0.f), iw = fmaxf(iwr, 0.f);
  const float inter = ih * iw;
  const float ha = a.z - a.x, wa = a.w - a.y, hb = b.z - b.x;
  const float uni = ha * wa + hb * wb - inter;
  const float iou = uni == 0.f ? 0.f : inter / uni;
  const float ch = fmaxf(a.z, b.z) - fminf(a.x, b.x);
  const float cw = fmaxf(a.w, b.w) - fminf(a.y, b.y);
  const float c2 = ch * ch + cw * cw;
  const float dx = (a.y + a.w) / 2.f - (b.y + b.w) / 2.f;
  const float dy = (a.x + a.z) / 2.f - (b.x + b.z) / 2.f;
  const float d2 = dx * dx + dy * dy;
  const float ra = wa / ha, rb = wb / hb;
  const float t = atanf(ra) - atanf(rb);
  const float v = kCiouV * (t * t);
  const float den = 1.f - iou + v;
  // d ciou = k_iou d iou - d(d2 / c2) - k_v d v
  float k_iou = 1.f, k_v = 0.f;
  if (den != 0.f) {
    const float al = v / den;
    k_iou = 1.f - al * al;
    k_v = 2.f * al - al * al;
  }
  // d iou = ((uni + inter) d inter - inter (d area_a + d area_b)) / uni^2
  float gi = 0.f, ga = 0.f;  // d iou / d inter, d iou / d area
  if (uni != 0.f) {
    gi = k_iou * (uni + inter) / (uni * uni);
    ga = -k_iou * inter / (uni * uni);
  }
  const float gih = ihr > 0.f ? gi * iw : 0.f;  // to the clamped intersection height
  const float giw = iwr > 0.f ? gi * ih : 0.f;
  // d (d2 / c2) = (d d2 c2 - d2 d c2) / c2^2
  float gd = 0.f, gc = 0.f;
  if (c2 != 0.f) {
    gd = -1.f / c2;
    gc = d2 / (c2 * c2);
  }
  // d v = 2 kCiouV t d t, d atan(r) = d r / (1 + r^2)
  const float gt = -k_v * 2.f * kCiouV * t;
  const float gwa = gt / (1.f + ra * ra) / ha;          // through w_a
  const float gha = gt / (1.f + ra * ra) * (-ra / ha);  // through h_a
  CiouGrad g;
  g.dwb = ga * hb - gt / (1.f + rb * rb) / hb;
  const float gch = gc * 2.f * ch, gcw = gc * 2.f * cw;  // to the enclosing box's sides
  g.da.x = (a.x >= b.x ? -gih : 0.f) - ga * wa + gd * dy - (a.x <= b.x ? gch : 0.f) - gha;
  g.da.z = (a.z <= b.z ? gih : 0.f) + ga * wa + gd * dy + (a.z >= b.z ? gch : 0.f) + gha;
  g.da.y = (a.y >= b.y ? -giw : 0.f) - ga * ha + gd * dx - (a.y <= b.y ? gcw : 0.f) - gwa;
  g.da.w = (a.w <= b.w ? giw : 0.f) + ga * ha + gd * dx + (a.w >= b.w ? gcw : 0.f) + gwa;
  return g;
}

}  // namespace d2mi
