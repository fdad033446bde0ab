// YOLOv4 geometry shared by the inference and the training kernels (yolo.hip,
// yolo_loss.hip): the per-level tables of the head's outputs, the prediction
// index -> (level, cell, anchor, row) map and the box decode of
// YOLOV4Outputs._get_predictions (yolov4_outputs.py:208-264), stated once so
// that the loss sees the bits the inference path sees.
#pragma once
#include "detect.h"

namespace d2mi {

constexpr int kYB = 256;       // predictions per workgroup of the YOLO kernels
constexpr int kYoloMaxA = 12;  // anchors per cell of a YOLO level (YoloGeo's cell tables)

struct YoloGeo {
  const float* ptr[D2MI_MAX_LEVELS];  // level l: [N, H, W, A * (5 + K)]
  int32_t H[D2MI_MAX_LEVELS], W[D2MI_MAX_LEVELS];
  int32_t p0[D2MI_MAX_LEVELS + 1];    // per-image prefix of predictions (H W A)
  float stride[D2MI_MAX_LEVELS];
  float cell_h[D2MI_MAX_LEVELS][kYoloMaxA], cell_w[D2MI_MAX_LEVELS][kYoloMaxA];
  float s[D2MI_MAX_LEVELS], half[D2MI_MAX_LEVELS];  // scale_yx, 0.5 * (scale_yx - 1)
  int32_t L, A, K, N, P;
  int32_t nb;                         // score blocks per image
};

struct PredAt {
  const float* row;  // the prediction's 5 + K logits
  int l, a, h, w;
};

// Prediction p of image n: level-major, then (h, w, a) (the reshape to
// [N, -1, ...] and concat of yolov4_outputs.py:247-260).
__device__ __forceinline__ PredAt locate(const YoloGeo& g, int n, int p) {
  int l = 0;
  while (l + 1 < g.L && g.p0[l + 1] <= p) ++l;
  const int j = p - g.p0[l];
  const int cell = j / g.A;
  PredAt q;
  q.l = l;
  q.a = j - cell * g.A;
  q.h = cell / g.W[l];
  q.w = cell - q.h * g.W[l];
  q.row = g.ptr[l] + ((int64_t)n * (g.p0[l + 1] - g.p0[l]) + j) * (int64_t)(5 + g.K);
  return q;
}

// yolov4_outputs.py:236-241, term by term in float32 (no contraction):
// anchors[:, :2] is the grid index (the cell anchors start at 0).
__device__ __forceinline__ float4 yolo_box(const YoloGeo& g, const PredAt& q) {
  const float r0 = q.row[0], r1 = q.row[1], r2 = q.row[2], r3 = q.row[3];
  const float s = g.s[q.l], half = g.half[q.l], stride = g.stride[q.l];
  const float dy = s * sigmoidf_tf(r0) - half;
  const float dx = s * sigmoidf_tf(r1) - half;
  const float y = ((float)q.h + dy) * stride;
  const float x = ((float)q.w + dx) * stride;
  const float hh = expf(r2) * g.cell_h[q.l][q.a];
  const float ww = expf(r3) * g.cell_w[q.l][q.a];
  return make_float4(y - 0.5f * hh, x - 0.5f * ww, y + 0.5f * hh, x + 0.5f * ww);
}

// Host (yolo.hip): predictions per image, or -1 when the sizes are out of
// range (message set); the tables of g from the host arrays of d2mi.h
// (make_geo_tables: everything but the level pointers; scale_yx may be null
// where no box is decoded).
int64_t yolo_total(int N, int L, const int32_t* level_hw, int A);
int make_geo_tables(YoloGeo& g, const int32_t* level_hw, const float* strides, const float* cell_hw,
                    const float* scale_yx, int L, int A, int K, int N);
int make_geo(YoloGeo& g, const float* const* logits, const int32_t* level_hw, const float* strides,
             const float* cell_hw, const float* scale_yx, int L, int A, int K, int N);

}  // namespace d2mi
