// Cascade R-CNN stage hand-over in one launch (lib/modeling/roi_heads/
// cascade_rcnn.py:141-215 _match_and_label_boxes, :244-273
// _create_proposals_from_boxes): the previous stage's class-agnostic deltas
// decoded on its boxes, clipped to the image, and (training) re-matched
// against the ground truth at the next stage's IoU threshold, with the
// matched class / index / box gathered -- one thread per proposal instead of
// the some twenty launches of the composition of the existing device ops
// (decode 1, window + clip 4, area and validity 5, the fused matcher 1, class
// select 8, box gather 1, loss validity 2; counted from the call sites,
// unmeasured).
//
// Float sequences are the shared ones: apply_delta + clip_box (common.h),
// iou_of (iou.h) and match_kernel's selection (match.hip): the first GT of
// maximal IoU among the valid, non-crowd, non-difficult GT; IoU >= thr is
// foreground; no matchable GT -> background, match 0; background rows whose
// max crowd IoU > 1e-3 or max difficult IoU > thr are ignored (-1).  So every
// output equals the composition d2mi_apply_deltas -> clamp ->
// d2mi_match_boxes_ex -> gathers bit for bit.  Training mode needs G >= 1
// (d2mi_match_boxes_ex accepts G = 0, but the gathers of the matched class and
// box, here and in the composition, have no row to read then).
//
// Every output element is written on every call (no fill, no workspace, no
// atomics).
#include "common.h"
#include "internal.h"
#include "iou.h"

namespace d2mi {
namespace {

constexpr int kMaxGt = 256;

struct RefineCfg {
  float wy, wx, wh, ww, clamp;
  float thr, crowd_thr;
  int K, cls64;
};

__global__ __launch_bounds__(256) void cascade_refine_kernel(
    const float4* __restrict__ deltas, const float4* __restrict__ boxes,
    const uint8_t* __restrict__ valid, const int32_t* __restrict__ image_hw, int S, int G,
    int training, const float4* __restrict__ gt, const uint8_t* __restrict__ gt_valid,
    const uint8_t* __restrict__ gt_crowd, const uint8_t* __restrict__ gt_difficult,
    const void* __restrict__ gt_cls, RefineCfg c, float4* __restrict__ out_boxes,
    uint8_t* __restrict__ out_valid, int64_t* __restrict__ out_cls,
    int64_t* __restrict__ out_idx, float4* __restrict__ out_gtb,
    uint8_t* __restrict__ out_loss_valid) {
  __shared__ float4 g_s[kMaxGt];
  __shared__ int f_s[kMaxGt];  // bit0 matchable, bit1 crowd, bit2 difficult
  const int n = blockIdx.y;
  if (training) {
    for (int g = threadIdx.x; g < G; g += 256) {
      const size_t i = (size_t)n * G + g;
      const bool cr = gt_crowd && gt_crowd[i], df = gt_difficult && gt_difficult[i];
      g_s[g] = gt[i];
      f_s[g] = (gt_valid[i] && !cr && !df ? 1 : 0) | (cr ? 2 : 0) | (df ? 4 : 0);
    }
    __syncthreads();
  }
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const size_t i = (size_t)n * S + s;
  const float hmax = (float)image_hw[2 * n], wmax = (float)image_hw[2 * n + 1];
  const float4 b =
      clip_box(apply_delta(boxes[i], deltas[i], c.wy, c.wx, c.wh, c.ww, c.clamp), hmax, wmax);
  out_boxes[i] = b;
  if (!training) {
    out_valid[i] = valid[i] ? 1 : 0;  // inference: validity passes through
    return;
  }
  const float area = (b.z - b.x) * (b.w - b.y);
  const bool ok = valid[i] && area > 0.f;
  float v = -INFINITY, crowd = 0.f, diff = 0.f;
  int arg = 0;
  bool any = false;
  for (int g = 0; g < G; ++g) {
    const int f = f_s[g];
    if (!(f & 7)) continue;
    const float q = iou_of(g_s[g], b);
    if (f & 1) {
      any = true;
      if (q > v) {
        v = q;
        arg = g;
      }
    }
    if (f & 2) crowd = fmaxf(crowd, q);
    if (f & 4) diff = fmaxf(diff, q);
  }
  // intervals [-inf, thr) -> 0, [thr, +inf) -> 1
  int lab = (v >= c.thr && v < INFINITY) ? 1 : 0;
  if (!any) {
    lab = 0;
    arg = 0;
  }
  if (lab == 0 && crowd > c.crowd_thr) lab = -1;
  if (lab == 0 && diff > c.thr) lab = -1;
  long long cls = -1;
  if (ok) {
    if (lab == 1) {
      const size_t ci = (size_t)n * G + arg;
      cls = c.cls64 ? static_cast<const int64_t*>(gt_cls)[ci]
                    : (long long)static_cast<const int32_t*>(gt_cls)[ci];
    } else if (lab == 0) {
      cls = c.K;
    }
  }
  out_valid[i] = ok ? 1 : 0;
  out_cls[i] = cls;
  out_idx[i] = arg;
  out_gtb[i] = g_s[arg];
  out_loss_valid[i] = (ok && cls >= 0) ? 1 : 0;
}

}  // namespace
}  // namespace d2mi

using namespace d2mi;

extern "C" int d2mi_cascade_refine(const float* deltas, const float* boxes, const uint8_t* valid,
                                   const int32_t* image_hw, int N, int S,
                                   const float* weights4_host, float scale_clamp, int training,
                                   const float* gt_boxes, const uint8_t* gt_valid,
                                   const uint8_t* gt_crowd, const uint8_t* gt_difficult,
                                   const void* gt_cls, int gt_cls_64, int G, float iou_thr,
                                   int num_classes, float* out_boxes, uint8_t* out_valid,
                                   int64_t* out_gt_classes, int64_t* out_gt_index,
                                   float* out_gt_boxes, uint8_t* out_loss_valid, void* stream) {
  D2MI_REQUIRE(N >= 1 && N <= 65535 && S >= 0 && (!training || (G >= 1 && num_classes >= 1)),
               "cascade_refine: bad sizes (N %d, S %d, G %d, num_classes %d)", N, S, G,
               num_classes);
  D2MI_REQUIRE(!training || G <= kMaxGt,
               "cascade_refine: at most %d ground-truth boxes per image (got %d)", kMaxGt, G);
  D2MI_REQUIRE(((uintptr_t)deltas & 15) == 0 && ((uintptr_t)boxes & 15) == 0 &&
                   ((uintptr_t)out_boxes & 15) == 0 &&
                   (!training ||
                    (((uintptr_t)gt_boxes & 15) == 0 && ((uintptr_t)out_gt_boxes & 15) == 0)),
               "cascade_refine: deltas / boxes / gt boxes must be 16-byte aligned");
  D2MI_REQUIRE(!training || (gt_boxes && gt_valid && gt_cls && out_gt_classes && out_gt_index &&
                             out_gt_boxes && out_loss_valid),
               "cascade_refine: training mode needs the ground truth and every training output");
  if (S == 0) return 0;
  D2MI_REQUIRE(deltas && boxes && valid && image_hw && weights4_host && out_boxes && out_valid,
               "cascade_refine: null input or output");
  RefineCfg c;
  c.wy = weights4_host[0];
  c.wx = weights4_host[1];
  c.wh = weights4_host[2];
  c.ww = weights4_host[3];
  c.clamp = scale_clamp;
  c.thr = iou_thr;
  c.crowd_thr = 1e-3f;
  c.K = num_classes;
  c.cls64 = gt_cls_64;
  hipLaunchKernelGGL(cascade_refine_kernel, dim3((S + 255) / 256, N), dim3(256), 0,
                     as_stream(stream), reinterpret_cast<const float4*>(deltas),
                     reinterpret_cast<const float4*>(boxes), valid, image_hw, S, G,
                     training ? 1 : 0, reinterpret_cast<const float4*>(gt_boxes), gt_valid,
                     gt_crowd, gt_difficult, gt_cls, c, reinterpret_cast<float4*>(out_boxes),
                     out_valid, out_gt_classes, out_gt_index,
                     reinterpret_cast<float4*>(out_gt_boxes), out_loss_valid);
  D2MI_LAUNCH_CHECK();
  return 0;
}
