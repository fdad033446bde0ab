// YOLOv4 training targets and losses on gfx950 (d2mi.h, "YOLOv4 training";
// lib/modeling/single_stage_heads/yolov4_outputs.py:59-206 _get_ground_truth,
// :266-329 losses; lib/modeling/matcher.py:176-267 YOLOMatcher;
// lib/structures/box_list_ops.py:295-450 pairwise / matched CIoU;
// lib/layers/loss.py:140-196 iou_loss), straight from the head's per-level
// NHWC logits [N, H, W, A * (5 + K)]: no decoded [N, P, 4] boxes, no
// [M, P] CIoU matrix, no dense [N, P, K] multi-hot target.
//
//   d2mi_yolov4_assign    one thread per (image, GT): the best of the L * A
//       cell anchors, the cell, the flat prediction index (slot) and, by an
//       integer max, the highest GT index of every prediction that is some
//       GT's slot (owner).  owner is cleared by a launch of its own.
//   d2mi_yolov4_loss_fwd  256 predictions per workgroup: the decode (yolo.h),
//       the maximum CIoU over the image's valid GT staged in LDS 64 at a time
//       (each GT's atan once), the state (positive / negative / neither), the
//       confidence and box terms by the prediction's own thread, the class
//       rows of the positives by whole waves; per-workgroup partial sums in a
//       fixed order.
//   d2mi_yolov4_loss_bwd  64 predictions per workgroup pass: one wave puts
//       each row's five leading gradients into LDS, then the workgroup writes
//       the rows' 64 * (5 + K) contiguous floats in order (rows are 4 * (5 + K) bytes,
//       not 16-byte aligned: consecutive lanes, consecutive words), zeros
//       where the loss does not reach.  No float atomics.
//
// Memory-bound: the forward reads the five leading logits of every row and
// the class logits of the positives, the backward writes every gradient.
#include "box_loss.h"
#include "iou.h"
#include "wave.h"
#include "yolo.h"

namespace d2mi {
namespace {

constexpr int kYoloLossBlocks = 96;  // per image (22,743 predictions at 608 x 608: 89 chunks)
constexpr int kGtChunk = 64;         // GTs staged in LDS at a time
constexpr int kGtRows = 256;         // (slot, class) rows of an image kept in LDS
constexpr int kBwdRows = 64;         // predictions per backward workgroup pass
constexpr int kYoloBwdBlocks = 384;  // per image

enum : uint8_t { kNeither = 0, kNegative = 1, kPositive = 2 };

struct YoloGt {
  const float4* boxes;        // [N, G]
  const int64_t* classes;     // [N, G]
  const uint8_t* valid;       // [N, G]: is_valid & ~crowd & ~difficult
  const int32_t* slot;        // [N, G]
  const int32_t* owner;       // [N, P]
  int G;
  float image_area, thresh;
  float iou_norm, num_images;  // the box weight (2 - area / image_area) * iou_norm / N
};

struct YoloGrads {
  float* d[D2MI_MAX_LEVELS];
};

// ------------------------------------------------------------------ assign
__global__ __launch_bounds__(kYB) void yolo_owner_clear_kernel(int32_t* __restrict__ owner,
                                                               int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * kYB + threadIdx.x;
  if (i < total) owner[i] = -1;
}

// yolov4_outputs.py:86-146 for GT g of image n.  The GT's (h, w) in units of
// each level's stride against that level's cell anchors in pixels (the
// reference's mix of units), first maximum of the L * A plain IoUs
// (tf.argmax), the cell of the centre at the assigned level's stride.
__global__ __launch_bounds__(kYB) void yolo_assign_kernel(YoloGeo g, const float4* __restrict__ gt,
                                                          const uint8_t* __restrict__ valid, int G,
                                                          int32_t* __restrict__ slot,
                                                          int32_t* __restrict__ owner) {
  const int64_t i = (int64_t)blockIdx.x * kYB + threadIdx.x;
  if (i >= (int64_t)g.N * G) return;
  const int n = (int)(i / G), gi = (int)(i - (int64_t)n * G);
  int s = -1;
  if (valid[i]) {
    const float4 b = gt[i];
    float best = -INFINITY;
    int bi = 0;
    for (int l = 0; l < g.L; ++l) {
      const float st = g.stride[l];
      const float h = b.z * 1.f / st - b.x * 1.f / st;
      const float w = b.w * 1.f / st - b.y * 1.f / st;
      const float4 zb = make_float4(0.f, 0.f, h, w);
      for (int a = 0; a < g.A; ++a) {
        const float v = iou_of(zb, make_float4(0.f, 0.f, g.cell_h[l][a], g.cell_w[l][a]));
        if (v > best || (l == 0 && a == 0)) {
          best = v;
          bi = l * g.A + a;
        }
      }
    }
    const int l = bi / g.A, a = bi - l * g.A;
    const float st = g.stride[l];
    const float cy = floorf((b.x * 1.f / st + b.z * 1.f / st) / 2.f);
    const float cx = floorf((b.y * 1.f / st + b.w * 1.f / st) / 2.f);
    // a cell outside the grid gets no slot (the reference's scatter is
    // undefined there)
    if (cy >= 0.f && cy < (float)g.H[l] && cx >= 0.f && cx < (float)g.W[l]) {
      s = g.p0[l] + ((int)cy * g.W[l] + (int)cx) * g.A + a;
      atomicMax(&owner[(size_t)n * g.P + s], gi);  // the highest GT index: any order
    }
  }
  slot[i] = s;
}

// The (slot, class) pairs of image n's first kGtRows GT rows in LDS, read by
// class_target for every class logit of every positive; rows beyond them are
// read from memory.  Call by the whole workgroup, then a barrier.
struct GtRows {
  int slot[kGtRows], cls[kGtRows];
};

__device__ __forceinline__ void stage_rows(const YoloGt& t, int n, GtRows& r) {
  for (int j = threadIdx.x; j < min(t.G, kGtRows); j += kYB) {
    const int64_t c = t.classes[(size_t)n * t.G + j];
    r.slot[j] = t.slot[(size_t)n * t.G + j];
    r.cls[j] = c >= 0 && c < (1ll << 31) ? (int)c : -1;
  }
}

// 1 where some GT of image n with slot p has class c (the multi-hot row of
// sparse.to_dense over the colliding GTs, yolov4_outputs.py:168-177)
__device__ __forceinline__ float class_target(const YoloGt& t, const GtRows& r, int n, int p,
                                              int c) {
  float z = 0.f;
  const int staged = min(t.G, kGtRows);
  for (int j = 0; j < staged; ++j)
    if (r.slot[j] == p && r.cls[j] == c) z = 1.f;
  for (int j = staged; j < t.G; ++j)
    if (t.slot[(size_t)n * t.G + j] == p && t.classes[(size_t)n * t.G + j] == (int64_t)c) z = 1.f;
  return z;
}

// (2 - gt_area / image_area) * iou_normalizer / num_images (:300-309)
__device__ __forceinline__ float box_weight(const YoloGt& t, const float4 gt) {
  const float area = (gt.z - gt.x) * (gt.w - gt.y);
  return (2.f - area / t.image_area) * t.iou_norm / t.num_images;
}

// ----------------------------------------------------------------- forward
// grid (kYoloLossBlocks, N); partial[n][block] = (conf, cls, box, #pos, #neg)
__global__ __launch_bounds__(kYB) void yolo_loss_fwd_kernel(YoloGeo g, YoloGt t,
                                                            double* __restrict__ part,
                                                            uint8_t* __restrict__ state) {
  __shared__ float4 s_box[kGtChunk];
  __shared__ float s_at[kGtChunk];
  __shared__ int s_ok[kGtChunk];
  __shared__ double red[5][4];
  __shared__ GtRows s_rows;
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  stage_rows(t, n, s_rows);
  __syncthreads();
  // float32 terms, added in float64: the sums carry the terms' rounding only
  double conf = 0., cls = 0., box = 0., npos = 0., nneg = 0.;
  for (int c0 = blockIdx.x * kYB; c0 < g.P; c0 += gridDim.x * kYB) {
    const int p = c0 + tid;
    const bool on = p < g.P;
    const PredAt q = locate(g, n, on ? p : g.P - 1);
    const float4 pb = yolo_box(g, q);
    const float pw = pb.w - pb.y;
    const float at_p = box_atan(pw, pb.z - pb.x);
    // max over the valid GT of pairwise CIoU(GT, prediction) (matcher.py:227)
    float best = -INFINITY;
    int nvalid = 0;
    for (int g0 = 0; g0 < t.G; g0 += kGtChunk) {
      __syncthreads();
      if (tid < kGtChunk && g0 + tid < t.G) {
        const size_t o = (size_t)n * t.G + g0 + tid;
        const float4 b = t.boxes[o];
        s_box[tid] = b;
        s_at[tid] = box_atan(b.w - b.y, b.z - b.x);
        s_ok[tid] = t.valid[o];
      }
      __syncthreads();
      const int cnt = min(kGtChunk, t.G - g0);
      for (int j = 0; j < cnt; ++j) {
        if (!s_ok[j]) continue;
        const float c = ciou_of(s_box[j], s_at[j], pb, pw, at_p);
        best = c > best ? c : best;
        ++nvalid;
      }
    }
    int own = on ? t.owner[(size_t)n * g.P + p] : -1;
    if (own >= t.G) own = -1;
    // an image without a valid GT has no negatives (matcher.py:236-242)
    const uint8_t st = !on ? kNeither
                           : (own >= 0 ? kPositive
                                       : (nvalid > 0 && best < t.thresh ? kNegative : kNeither));
    if (on) state[(size_t)n * g.P + p] = st;
    if (st != kNeither) {
      // (respond_bbox - sigmoid(conf))^2 * BCE(conf logit, respond_bbox) (:315-322)
      const float x = q.row[4];
      const float rb = st == kPositive ? 1.f : 0.f;
      const float f = rb - sigmoidf_tf(x);
      conf += (double)(f * f * bce_logits(x, rb));
      if (st == kPositive) npos += 1.;
      else nneg += 1.;
    }
    if (st == kPositive) {
      // iou_loss "ciou" of matched_iou(prediction, GT): width2 = x_max1 - x_min2
      const float4 gb = t.boxes[(size_t)n * t.G + own];
      const float wb = pb.w - gb.y;
      const float c = ciou_of(pb, at_p, gb, wb, box_atan(wb, gb.z - gb.x));
      box += (double)((1.f - c) * box_weight(t, gb));
    }
    // the class rows of the positives, one after the other by the whole wave
    uint64_t todo = __ballot(st == kPositive);
    while (todo) {
      const int b = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const float* row = reinterpret_cast<const float*>(readlane64((uint64_t)(uintptr_t)q.row, b));
      const int pp = __builtin_amdgcn_readlane(p, b);
      for (int c = lane; c < g.K; c += 64)
        cls += (double)bce_logits(row[5 + c], class_target(t, s_rows, n, pp, c));
    }
  }
  const double s0 = block_sum(conf, red[0]);
  const double s1 = block_sum(cls, red[1]);
  const double s2 = block_sum(box, red[2]);
  const double s3 = block_sum(npos, red[3]);
  const double s4 = block_sum(nneg, red[4]);
  if (tid == 0) {
    double* o = part + ((size_t)n * gridDim.x + blockIdx.x) * 5;
    o[0] = s0;
    o[1] = s1;
    o[2] = s2;
    o[3] = s3;
    o[4] = s4;
  }
}

// ---------------------------------------------------------------- backward
// Every element of every level's gradient written.  sc_conf / sc_cls: 1 / N
// and CLS_NORMALIZER / N, the factors the caller applied to the forward sums.
__global__ __launch_bounds__(kYB) void yolo_loss_bwd_kernel(YoloGeo g, YoloGt t, YoloGrads dg,
                                                            const uint8_t* __restrict__ state,
                                                            float sc_conf, float sc_cls,
                                                            const float* __restrict__ g_conf_p,
                                                            const float* __restrict__ g_cls_p,
                                                            const float* __restrict__ g_box_p) {
  __shared__ float s_lead[kBwdRows][5];
  __shared__ uint8_t s_pos[kBwdRows];
  __shared__ GtRows s_rows;
  const int n = blockIdx.y, tid = threadIdx.x;
  stage_rows(t, n, s_rows);  // (visible after the first barrier below)
  const float g_conf = (g_conf_p ? g_conf_p[0] : 0.f) * sc_conf;
  const float g_cls = (g_cls_p ? g_cls_p[0] : 0.f) * sc_cls;
  const float g_box = g_box_p ? g_box_p[0] : 0.f;
  const int R = 5 + g.K;
  // the step of (row, column) from one element of a thread to its next
  const int dpl = kYB / R, dc = kYB - dpl * R;
  for (int c0 = blockIdx.x * kBwdRows; c0 < g.P; c0 += gridDim.x * kBwdRows) {
    // wave 0: the rows' own five gradients (the others wait: the rows are few
    // and the writes below are the work)
    const int p = c0 + tid;
    const bool on = tid < kBwdRows && p < g.P;
    const uint8_t st = on ? state[(size_t)n * g.P + p] : (uint8_t)kNeither;
    float lead[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (st != kNeither) {
      const PredAt q = locate(g, n, p);
      const float x = q.row[4];
      const float rb = st == kPositive ? 1.f : 0.f;
      const float sg = sigmoidf_tf(x);
      const float f = rb - sg;
      // d [f^2 bce] = 2 f (-sg (1 - sg)) bce + f^2 (sg - rb)
      lead[4] = g_conf * (2.f * f * (-(sg * (1.f - sg))) * bce_logits(x, rb) +
                          f * f * bce_logits_grad(x, rb));
      int own = st == kPositive ? t.owner[(size_t)n * g.P + p] : -1;
      if (own >= t.G) own = -1;
      if (own >= 0) {
        const float4 pb = yolo_box(g, q);
        const float4 gb = t.boxes[(size_t)n * t.G + own];
        const CiouGrad cg = ciou_grad(pb, gb, pb.w - gb.y);
        const float k = -(g_box * box_weight(t, gb));  // d (1 - ciou) w
        const float dy1 = k * cg.da.x, dx1 = k * cg.da.y;
        const float dy2 = k * cg.da.z, dx2 = k * (cg.da.w + cg.dwb);  // wb = x_max1 - x_min2
        // box = (y - hh / 2, x - ww / 2, y + hh / 2, x + ww / 2), y = (h + s sigmoid(r0) -
        // half) stride, hh = exp(r2) cell_h (yolo_box)
        const float s = g.s[q.l], stride = g.stride[q.l];
        const float s0 = sigmoidf_tf(q.row[0]), s1 = sigmoidf_tf(q.row[1]);
        const float hh = expf(q.row[2]) * g.cell_h[q.l][q.a];
        const float ww = expf(q.row[3]) * g.cell_w[q.l][q.a];
        lead[0] = (dy1 + dy2) * stride * s * (s0 * (1.f - s0));
        lead[1] = (dx1 + dx2) * stride * s * (s1 * (1.f - s1));
        lead[2] = (dy2 - dy1) * 0.5f * hh;
        lead[3] = (dx2 - dx1) * 0.5f * ww;
      }
    }
    __syncthreads();  // the previous chunk's rows are written
    if (tid < kBwdRows) {
#pragma unroll
      for (int k = 0; k < 5; ++k) s_lead[tid][k] = lead[k];
      s_pos[tid] = st == kPositive;
    }
    __syncthreads();
    const int cnt = min(kBwdRows, g.P - c0);
    int pl = tid / R, c = tid - pl * R;
    for (int i = tid; i < cnt * R; i += kYB, pl += dpl, c += dc) {
      if (c >= R) {
        c -= R;
        ++pl;
      }
      const int pp = c0 + pl;
      int l = 0;
      while (l + 1 < g.L && g.p0[l + 1] <= pp) ++l;
      const size_t off = ((size_t)n * (g.p0[l + 1] - g.p0[l]) + (pp - g.p0[l])) * R + c;
      float v = 0.f;
      if (c < 5) v = s_lead[pl][c];
      else if (s_pos[pl])
        v = g_cls * bce_logits_grad(g.ptr[l][off], class_target(t, s_rows, n, pp, c - 5));
      dg.d[l][off] = v;
    }
  }
}

int make_gt(YoloGt& t, const float* gt_boxes, const int64_t* gt_classes, const uint8_t* valid,
            int G, const int32_t* slot, const int32_t* owner, float image_area, float thresh,
            float iou_norm, int N, int K, bool forward) {
  D2MI_REQUIRE(G >= 0, "yolov4 loss: G=%d is negative", G);
  D2MI_REQUIRE(K < (1 << 20), "yolov4 loss: K=%d out of range", K);
  D2MI_REQUIRE(owner != nullptr, "yolov4 loss: owner is null");
  // (the backward reads the forward's state, not valid)
  D2MI_REQUIRE(G == 0 || (gt_boxes && gt_classes && (valid || !forward) && slot),
               "yolov4 loss: null GT arrays");
  D2MI_REQUIRE(((uintptr_t)gt_boxes & 15) == 0, "yolov4 loss: gt_boxes must be 16B aligned");
  D2MI_REQUIRE(image_area > 0.f, "yolov4 loss: image_area must be positive");
  t.boxes = reinterpret_cast<const float4*>(gt_boxes);
  t.classes = gt_classes;
  t.valid = valid;
  t.slot = slot;
  t.owner = owner;
  t.G = G;
  t.image_area = image_area;
  t.thresh = thresh;
  t.iou_norm = iou_norm;
  t.num_images = (float)N;
  return 0;
}

}  // namespace
}  // namespace d2mi

using namespace d2mi;

extern "C" int d2mi_yolov4_loss_blocks(void) { return kYoloLossBlocks; }

extern "C" int d2mi_yolov4_assign(const int32_t* level_hw, const float* strides,
                                  const float* cell_hw, int L, int A, int N,
                                  const float* gt_boxes, const uint8_t* valid, int G,
                                  int32_t* slot, int32_t* owner, void* stream) {
  YoloGeo g;
  int rc = make_geo_tables(g, level_hw, strides, cell_hw, nullptr, L, A, 1, N);
  if (rc) return rc;
  D2MI_REQUIRE(L == 3, "yolov4 assign: L=%d, the reference has 3 levels", L);
  D2MI_REQUIRE(G >= 0, "yolov4 assign: G=%d is negative", G);
  D2MI_REQUIRE(owner != nullptr, "yolov4 assign: owner is null");
  D2MI_REQUIRE(G == 0 || (gt_boxes && valid && slot), "yolov4 assign: null GT arrays");
  D2MI_REQUIRE(((uintptr_t)gt_boxes & 15) == 0, "yolov4 assign: gt_boxes must be 16B aligned");
  const int64_t total = (int64_t)N * g.P;
  hipLaunchKernelGGL(yolo_owner_clear_kernel, dim3((unsigned)((total + kYB - 1) / kYB)), dim3(kYB),
                     0, as_stream(stream), owner, total);
  D2MI_LAUNCH_CHECK();
  if (G == 0) return 0;
  const int64_t ng = (int64_t)N * G;
  D2MI_REQUIRE(ng < (1ll << 31), "yolov4 assign: too many GT rows");
  hipLaunchKernelGGL(yolo_assign_kernel, dim3((unsigned)((ng + kYB - 1) / kYB)), dim3(kYB), 0,
                     as_stream(stream), g, reinterpret_cast<const float4*>(gt_boxes), valid, G, slot,
                     owner);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" int d2mi_yolov4_loss_fwd(const float* const* logits, const int32_t* level_hw,
                                    const float* strides, const float* cell_hw,
                                    const float* scale_yx, int L, int A, int K, int N,
                                    const float* gt_boxes, const int64_t* gt_classes,
                                    const uint8_t* valid, int G, const int32_t* slot,
                                    const int32_t* owner, float image_area, float iou_threshold,
                                    float iou_normalizer, double* partial, uint8_t* state,
                                    void* stream) {
  YoloGeo g;
  int rc = make_geo(g, logits, level_hw, strides, cell_hw, scale_yx, L, A, K, N);
  if (rc) return rc;
  D2MI_REQUIRE(L == 3, "yolov4 loss: L=%d, the reference has 3 levels", L);
  D2MI_REQUIRE(partial && state, "yolov4 loss: null outputs");
  YoloGt t;
  rc = make_gt(t, gt_boxes, gt_classes, valid, G, slot, owner, image_area, iou_threshold,
               iou_normalizer, N, K, true);
  if (rc) return rc;
  hipLaunchKernelGGL(yolo_loss_fwd_kernel, dim3(kYoloLossBlocks, N), dim3(kYB), 0,
                     as_stream(stream), g, t, partial, state);
  D2MI_LAUNCH_CHECK();
  return 0;
}

extern "C" int d2mi_yolov4_loss_bwd(const float* const* logits, float* const* d_logits,
                                    const int32_t* level_hw, const float* strides,
                                    const float* cell_hw, const float* scale_yx, int L, int A,
                                    int K, int N, const float* gt_boxes,
                                    const int64_t* gt_classes, int G, const int32_t* slot,
                                    const int32_t* owner, const uint8_t* state, float image_area,
                                    float iou_normalizer, float conf_scale, float cls_scale,
                                    const float* g_conf, const float* g_cls, const float* g_box,
                                    void* stream) {
  YoloGeo g;
  int rc = make_geo(g, logits, level_hw, strides, cell_hw, scale_yx, L, A, K, N);
  if (rc) return rc;
  D2MI_REQUIRE(L == 3, "yolov4 loss: L=%d, the reference has 3 levels", L);
  D2MI_REQUIRE(d_logits && state, "yolov4 loss: null gradient levels or state");
  YoloGrads dg{};
  for (int l = 0; l < L; ++l) {
    dg.d[l] = d_logits[l];
    D2MI_REQUIRE(dg.d[l] != nullptr, "yolov4 loss: level %d gradient is null", l);
  }
  YoloGt t;
  rc = make_gt(t, gt_boxes, gt_classes, nullptr, G, slot, owner, image_area, 0.f, iou_normalizer,
               N, K, false);
  if (rc) return rc;
  hipLaunchKernelGGL(yolo_loss_bwd_kernel, dim3(kYoloBwdBlocks, N), dim3(kYB), 0,
                     as_stream(stream), g, t, dg, state, conf_scale, cls_scale, g_conf, g_cls, g_box);
  D2MI_LAUNCH_CHECK();
  return 0;
}
