// TF 1.15 ResizeBilinear arithmetic, stated once: d2mi_resize_bilinear
// (solo.hip) and the fused semantic-segmentation kernels (sem_seg.hip)
// interpolate with exactly these expressions.
//
// resize_bilinear_op.cc: compute_interpolation_weights with
// HalfPixelScaler ((x + 0.5) * scale - 0.5) or LegacyScaler (x * scale);
// lower = max(floor(in), 0), upper = min(ceil(in), in_size - 1),
// lerp = in - floor(in); compute_lerp: top = tl + (tr - tl) * xl,
// bottom = bl + (br - bl) * xl, out = top + (bottom - top) * yl.
#pragma once
#include "common.h"

namespace d2mi {

struct Interp {
  int lo, hi;
  float lerp;
};

__device__ __forceinline__ Interp interp_at(int i, float scale, int in_size, int half_pixel) {
  const float in = half_pixel ? ((float)i + 0.5f) * scale - 0.5f : (float)i * scale;
  const float in_f = floorf(in);
  Interp r;
  r.lo = max((int)in_f, 0);
  r.hi = min((int)ceilf(in), in_size - 1);
  r.lerp = in - in_f;
  return r;
}

__device__ __forceinline__ float tf_lerp(float tl, float tr, float bl, float br, float xl,
                                         float yl) {
  const float top = tl + (tr - tl) * xl;
  const float bottom = bl + (br - bl) * xl;
  return top + (bottom - top) * yl;
}

// CalculateResizeScale (TF image_resizer_state.h), float division.
static inline float resize_scale(int in, int out, int align_corners) {
  return (align_corners && out > 1) ? (float)(in - 1) / (float)(out - 1)
                                    : (float)in / (float)out;
}

}  // namespace d2mi
