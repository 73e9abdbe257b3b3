// box_iou_loss.hpp -- IoU / GIoU / DIoU box-regression losses at the foreground anchors of every pyramid level of the batch: the
// opt-in alternative to the smooth-L1 walk of loss.hpp (`Model.box_loss`, `odtk train --box-loss`), axis-aligned boxes only.
// No reference equivalent; the formulas are torchvision's {,generalized_,distance_}box_iou_loss on boxes decoded from the deltas.
//
// The definition (the contract; restated in torch in odtk/loss.py:box_iou_loss, the ground truth of tests/test_gpu_box_iou_loss.py).
// One foreground anchor (depth > 0) of anchor slot a; (aw, ah) = (x2 - x1 + 1, y2 - y1 + 1) of the level's anchor table;
// p = the four predicted deltas (head dtype -> float32), t = the four target deltas.  Both boxes are decoded relative to the
// anchor centre -- the cell position cancels, so neither stride nor grid enters:
//     CLIP = log(1000 / 16);  pw' = min(pw, CLIP), ph' = min(ph, CLIP)            (predictions only; gradient 0 beyond the clip)
//     P: centre (px aw, py ah), size (exp(pw') aw, exp(ph') ah)                  T: the same from t, unclipped
//     inter = max(0, min(Px2, Tx2) - max(Px1, Tx1)) max(0, min(Py2, Ty2) - max(Py1, Ty1))      (corners: centre -+ size / 2)
//     union = area(P) + area(T) - inter + eps,  iou = inter / union,  eps = 1e-7;   (ew, eh) = size of the box enclosing both
//     iou : L = 1 - iou
//     giou: c = ew eh + eps,         L = 1 - iou + (c - union) / c
//     diou: c2 = ew^2 + eh^2 + eps,  L = 1 - iou + ((Pcx - Tcx)^2 + (Pcy - Tcy)^2) / c2
// Per level: box_sum = sum of L over the foreground anchors (float64, one fixed order: the same bits on every run), fg = their
// number.  Backward: d(deltas) = g[level] dL/dp at the foreground cells and +0 everywhere else, every element written, in the
// head's dtype and layout, rounded once at the store.  At the ties (min / max / clamp, inter = 0, pw = CLIP) the gradient is
// that of one side.  min / max here hand a NaN on (nan_min / nan_max), so a NaN delta at a foreground anchor reaches the sum as it
// does through smooth-L1; cells that are not foreground are never read from the head.
// Arithmetic: IEEE float32 per anchor, ocml expf, the gradient in closed form (reverse mode by hand, below).
//
// Shape: two launches for all levels (the level table and the anchor SIZES travel in the kernel arguments), both over one lane
// per anchor cell -- ~1 % of the lanes have work; the launches are bound by the depth read (forward) and the gradient write.
//   forward : lanes in depth's order (image, anchor, pixel): the depth read is coalesced; a foreground lane gathers its 4 + 4
//             deltas (NHWC: one vector of the head; NCHW: four planes).  Wave sum in double, one pair (sum, fg) per workgroup into
//             the workspace, then box_iou_reduce_kernel adds the pairs of a level up in a fixed order.  No atomics.
//   backward: lanes in the order d(deltas) lies in memory -- NCHW: (image, anchor, pixel), four plane stores of consecutive
//             elements per wave; NHWC: (image, pixel, anchor), ONE 16- / 8-byte vector per lane, a wave's stores one run.
// Measured: DESIGN.md (tools/box_iou_loss_probe.py, profiles/r11_box_iou_loss_probe.txt).
#pragma once

#include "loss.hpp"   // store_elem, store_vec4, box_grad_value, block_sum; element types; fastdiv

namespace odtk {

constexpr int kBoxIouThreads = 256;
constexpr float kBoxIouClip = 4.135166556742356f;     // log(1000 / 16): Detectron's BBOX_XFORM_CLIP
constexpr float kBoxIouEps = 1e-7f;

struct BoxIouLevel {
  const void *box;          // [B, A*4, H, W] predicted deltas, element type T
  const float *depth;       // [B, A, 1, H, W]
  const float *box_target;  // [B, A, 4, H, W]
  void *dbox;               // backward: gradient, dtype / layout of box
  const float *g;           // backward: device scalar d(out)/d(box_sum) of this level (null: 0)
  uint32_t hw, cells;       // H*W, B*A*H*W (4 * cells < 2^31: host)
  uint32_t channels_last, pad_;
  FastDiv by_hw, by_anchors;
  float aw[ODTK_MAX_ANCHORS], ah[ODTK_MAX_ANCHORS];
};

struct BoxIouArgs {
  BoxIouLevel lv[ODTK_MAX_LEVELS];
  uint32_t block_begin[ODTK_MAX_LEVELS + 1];
  double *partial;          // forward: [gridDim.x][2] = (sum, fg) per workgroup
  uint32_t n_levels, num_anchors, kind, pad_;
};

// min / max that hand a NaN of either side on (fminf / fmaxf drop it)
__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

// L of one anchor; kGrad: also dL/dp.
template <bool kGrad>
__device__ __forceinline__ float box_iou_term(const float *p, const float *t, float aw, float ah, uint32_t kind, float *grad) {
  const float w = expf(nan_min(p[2], kBoxIouClip)) * aw, h = expf(nan_min(p[3], kBoxIouClip)) * ah;
  const float tw = expf(t[2]) * aw, th = expf(t[3]) * ah;
  const float cx = p[0] * aw, cy = p[1] * ah, tcx = t[0] * aw, tcy = t[1] * ah;
  const float x1 = cx - 0.5f * w, x2 = cx + 0.5f * w, y1 = cy - 0.5f * h, y2 = cy + 0.5f * h;
  const float tx1 = tcx - 0.5f * tw, tx2 = tcx + 0.5f * tw, ty1 = tcy - 0.5f * th, ty2 = tcy + 0.5f * th;
  const float iw = nan_min(x2, tx2) - nan_max(x1, tx1), ih = nan_min(y2, ty2) - nan_max(y1, ty1);
  const float iwc = nan_max(iw, 0.0f), ihc = nan_max(ih, 0.0f);
  const float inter = iwc * ihc;
  const float uni = w * h + tw * th - inter + kBoxIouEps;
  const float iou = inter / uni;
  const float ew = nan_max(x2, tx2) - nan_min(x1, tx1), eh = nan_max(y2, ty2) - nan_min(y1, ty1);
  float loss = 1.0f - iou;
  // reverse mode: g_x = dL/dx
  float g_uni = iou / uni, g_ew = 0.0f, g_eh = 0.0f, g_cx = 0.0f, g_cy = 0.0f;
  if (kind == ODTK_BOX_LOSS_GIOU) {
    const float c = ew * eh + kBoxIouEps;
    loss += (c - uni) / c;
    if constexpr (kGrad) {
      const float g_c = uni / (c * c);
      g_uni -= 1.0f / c;
      g_ew = eh * g_c;
      g_eh = ew * g_c;
    }
  } else if (kind == ODTK_BOX_LOSS_DIOU) {
    const float c2 = ew * ew + eh * eh + kBoxIouEps;
    const float dx = cx - tcx, dy = cy - tcy;
    const float rho = dx * dx + dy * dy;
    loss += rho / c2;
    if constexpr (kGrad) {
      const float g_c2 = -rho / (c2 * c2);
      g_cx = 2.0f * dx / c2;
      g_cy = 2.0f * dy / c2;
      g_ew = 2.0f * ew * g_c2;
      g_eh = 2.0f * eh * g_c2;
    }
  }
  if constexpr (kGrad) {
    const float g_inter = -1.0f / uni - g_uni;                       // through iou and through the union
    const float g_iw = iw > 0.0f ? ihc * g_inter : 0.0f, g_ih = ih > 0.0f ? iwc * g_inter : 0.0f;
    const float g_x2 = (x2 < tx2 ? g_iw : 0.0f) + (x2 > tx2 ? g_ew : 0.0f);
    const float g_x1 = (x1 > tx1 ? -g_iw : 0.0f) + (x1 < tx1 ? -g_ew : 0.0f);
    const float g_y2 = (y2 < ty2 ? g_ih : 0.0f) + (y2 > ty2 ? g_eh : 0.0f);
    const float g_y1 = (y1 > ty1 ? -g_ih : 0.0f) + (y1 < ty1 ? -g_eh : 0.0f);
    const float g_w = h * g_uni + 0.5f * (g_x2 - g_x1), g_h = w * g_uni + 0.5f * (g_y2 - g_y1);
    grad[0] = (g_cx + g_x1 + g_x2) * aw;
    grad[1] = (g_cy + g_y1 + g_y2) * ah;
    grad[2] = p[2] < kBoxIouClip ? g_w * w : 0.0f;
    grad[3] = p[3] < kBoxIouClip ? g_h * h : 0.0f;
  }
  return loss;
}

// the four deltas of cell (image, anchor `an`, pixel) with ia = image * A + an: NHWC one vector, NCHW four planes
template <typename T>
__device__ __forceinline__ void box_iou_load(const BoxIouLevel &L, uint32_t A, uint32_t ia, uint32_t an, uint32_t pix, float *p, float *t) {
  const uint32_t plane = ia * 4u * L.hw + pix;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) t[k] = L.box_target[plane + k * L.hw];
  if (L.channels_last) {
    const uint32_t v = (ia - an) * L.hw + pix * A + an;              // (image * hw + pix) * A + an, with image * A = ia - an
    if constexpr (std::is_same_v<T, F32>) {
      const vuint4 raw = static_cast<const vuint4 *>(L.box)[v];
#pragma unroll
      for (int k = 0; k < 4; ++k) p[k] = __uint_as_float(raw[k]);
    } else {
      const uint2 raw = static_cast<const uint2 *>(L.box)[v];
      const uint32_t h4[4] = {raw.x & 0xffffu, raw.x >> 16, raw.y & 0xffffu, raw.y >> 16};
#pragma unroll
      for (int k = 0; k < 4; ++k) p[k] = std::is_same_v<T, BF16> ? bf16_bits_to_float(h4[k]) : f16_bits_to_float(h4[k]);
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) p[k] = load_raw<T>(L.box, plane + k * L.hw);
  }
}

__device__ __forceinline__ int box_iou_level_of(const BoxIouArgs &a) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < ODTK_MAX_LEVELS; ++i)
    if (i < static_cast<int>(a.n_levels) && blockIdx.x >= a.block_begin[i]) l = i;
  return l;
}

template <typename T>
__global__ __launch_bounds__(kBoxIouThreads) void box_iou_loss_forward_kernel(const BoxIouArgs a) {
  __shared__ double s_red[kBoxIouThreads / kWave];
  const int l = box_iou_level_of(a);
  const BoxIouLevel &L = a.lv[l];
  const uint32_t cell = (blockIdx.x - a.block_begin[l]) * kBoxIouThreads + threadIdx.x;   // (image * A + an) * hw + pix
  double loss = 0.0, fg = 0.0;
  if (cell < L.cells && L.depth[cell] > 0.0f) {
    uint32_t pix, an;
    const uint32_t ia = fastdivmod(cell, L.by_hw, &pix);
    fastdivmod(ia, L.by_anchors, &an);
    float p[4], t[4];
    box_iou_load<T>(L, a.num_anchors, ia, an, pix, p, t);
    loss = box_iou_term<false>(p, t, L.aw[an], L.ah[an], a.kind, nullptr);
    fg = 1.0;
  }
  const double s = block_sum(loss, s_red);
  const double f = block_sum(fg, s_red);
  if (threadIdx.x == 0) {
    a.partial[2 * static_cast<size_t>(blockIdx.x)] = s;
    a.partial[2 * static_cast<size_t>(blockIdx.x) + 1] = f;
  }
}

// Workgroup l adds up the pairs of level l: thread t takes workgroups t, t + 256, ... in order, then the wave / block tree.
struct BoxIouReduceArgs {
  const double *partial;
  double *sums;                                // [n_levels][2] = (box_sum, fg)
  uint32_t block_begin[ODTK_MAX_LEVELS + 1];
};

__global__ __launch_bounds__(kBoxIouThreads) void box_iou_reduce_kernel(const BoxIouReduceArgs a) {
  __shared__ double s_red[kBoxIouThreads / kWave];
  const uint32_t l = blockIdx.x, b1 = a.block_begin[l + 1];
  double s = 0.0, f = 0.0;
  for (uint32_t b = a.block_begin[l] + threadIdx.x; b < b1; b += kBoxIouThreads) {
    s += a.partial[2 * static_cast<size_t>(b)];
    f += a.partial[2 * static_cast<size_t>(b) + 1];
  }
  s = block_sum(s, s_red);
  f = block_sum(f, s_red);
  if (threadIdx.x == 0) {
    a.sums[2 * l] = s;
    a.sums[2 * l + 1] = f;
  }
}

template <typename T>
__global__ __launch_bounds__(kBoxIouThreads) void box_iou_loss_backward_kernel(const BoxIouArgs a) {
  const int l = box_iou_level_of(a);
  const BoxIouLevel &L = a.lv[l];
  const uint32_t cell = (blockIdx.x - a.block_begin[l]) * kBoxIouThreads + threadIdx.x;
  if (cell >= L.cells) return;
  const uint32_t A = a.num_anchors;
  uint32_t ia, an, pix;
  if (L.channels_last) {                                   // (launch-uniform per workgroup) cell = (image * hw + pix) * A + an
    const uint32_t ip = fastdivmod(cell, L.by_anchors, &an);
    const uint32_t img = fastdivmod(ip, L.by_hw, &pix);
    ia = img * A + an;
  } else {                                                 // cell = (image * A + an) * hw + pix
    ia = fastdivmod(cell, L.by_hw, &pix);
    fastdivmod(ia, L.by_anchors, &an);
  }
  float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (L.depth[ia * L.hw + pix] > 0.0f) {
    const float g = L.g ? *L.g : 0.0f;
    float p[4], t[4], grad[4];
    box_iou_load<T>(L, A, ia, an, pix, p, t);
    box_iou_term<true>(p, t, L.aw[an], L.ah[an], a.kind, grad);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = box_grad_value(g, grad[k]);
  }
  if (L.channels_last) {
    store_vec4<T>(L.dbox, cell, out);
  } else {
    const uint32_t plane = ia * 4u * L.hw + pix;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) store_elem<T>(L.dbox, plane + k * L.hw, out[k]);
  }
}

}  // namespace odtk
