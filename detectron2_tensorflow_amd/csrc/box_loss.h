// The element formulas of the training losses, each stated once: the
// box-regression target, smooth-L1 and the sigmoid cross-entropy with their
// gradients.  The RPN, Fast R-CNN / mask and RetinaNet loss kernels
// (rpn_loss.hip, roi_losses.hip, retina_loss.hip) fetch their operands in
// their own layouts and evaluate these, so the three agree to the bit.
#pragma once
#include "common.h"

namespace d2mi {

// Box2BoxTransform.get_deltas for one (source box, GT box) pair
// (lib/modeling/box_regression.py:38-74), float32, no contraction: boxes are
// (y0, x0, y1, x1), the result (dy, dx, dh, dw) times the weights.
__device__ __forceinline__ float4 box_deltas(float4 src, float4 gt, float wy, float wx, float wh,
                                             float ww) {
  const float sh = src.z - src.x, sw = src.w - src.y;
  const float scy = src.x + 0.5f * sh, scx = src.y + 0.5f * sw;
  const float th = gt.z - gt.x, tw = gt.w - gt.y;
  const float tcy = gt.x + 0.5f * th, tcx = gt.y + 0.5f * tw;
  return make_float4(wy * (tcy - scy) / sh, wx * (tcx - scx) / sw, wh * logf(th / sh),
                     ww * logf(tw / sw));
}

// smooth_l1_loss of one element (lib/layers/loss.py:9-58): t the label, p the
// prediction; plain L1 for beta < 1e-5.
__device__ __forceinline__ float sl1(float t, float p, float beta) {
  const float d = fabsf(t - p);
  return beta < 1e-5f ? d : (d < beta ? 0.5f * (d * d) / beta : d - 0.5f * beta);
}

// d sl1 / dp
__device__ __forceinline__ float sl1_grad(float t, float p, float beta) {
  const float d = p - t;  // d|t - p| / dp = sign(p - t)
  const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if (beta < 1e-5f) return sg;
  return fabsf(d) < beta ? d / beta : sg;
}

// Sigmoid cross-entropy of logit x against target z, as ATen's
// binary_cross_entropy_with_logits states it.
__device__ __forceinline__ float bce_logits(float x, float z) {
  const float m = fmaxf(-x, 0.f);
  return (1.f - z) * x + m + logf(expf(-m) + expf(-x - m));
}

// d bce_logits / dx = sigmoid(x) - z
__device__ __forceinline__ float bce_logits_grad(float x, float z) { return sigmoidf_tf(x) - z; }

}  // namespace d2mi
