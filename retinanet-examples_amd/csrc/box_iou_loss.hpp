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
// Shape: cell_loss.hpp's kernels with the policy BoxIouLoss (below) -- two launches for all levels (the level table and the anchor
// SIZES travel in the kernel arguments), both over one lane per anchor cell -- ~1 % of the lanes have work; the launches are
// bound by the depth read (forward) and the gradient write.
//   forward : lanes in depth's order (image, anchor, pixel): the depth read is coalesced; a foreground lane gathers its 4 + 4
//             deltas (NHWC: one vector of the head; NCHW: four planes).  Wave sum in double, one pair (sum, fg) per workgroup into
//             the workspace, then level_pair_reduce_kernel adds the pairs of a level up in a fixed order.  No atomics.
//   backward: lanes in the order d(deltas) lies in memory -- NCHW: (image, anchor, pixel), four plane stores of consecutive
//             elements per wave; NHWC: (image, pixel, anchor), ONE 16- / 8-byte vector per lane, a wave's stores one run.
// Measured: DESIGN.md (tools/box_iou_loss_probe.py, profiles/r11_box_iou_loss_probe.txt).
#pragma once

#include "cell_loss.hpp"   // CellLossLevel, the kernels that take BoxIouLoss; loss.hpp: store_vec4, box_grad_value, element types

namespace odtk {

constexpr float kBoxIouClip = 4.135166556742356f;     // log(1000 / 16): Detectron's BBOX_XFORM_CLIP
constexpr float kBoxIouEps = 1e-7f;

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
__device__ __forceinline__ void box_iou_load(const CellLossLevel &L, uint32_t A, uint32_t ia, uint32_t an, uint32_t pix, float *p, float *t) {
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

// The IoU family as cell_loss.hpp's kernels see it.
struct BoxIouLoss {
  static constexpr uint32_t kParams = 4;
  using Grad = float;
  template <typename T>
  static __device__ __forceinline__ void load(const CellLossLevel &L, uint32_t A, uint32_t ia, uint32_t an, uint32_t pix, float *p, float *t) {
    box_iou_load<T>(L, A, ia, an, pix, p, t);
  }
  template <bool kGrad>
  static __device__ __forceinline__ float term(const float *p, const float *t, float aw, float ah, uint32_t kind, float *grad) {
    return box_iou_term<kGrad>(p, t, aw, ah, kind, grad);
  }
  static __device__ __forceinline__ float grad_value(float g, float grad) { return box_grad_value(g, grad); }
  template <typename T>
  static __device__ __forceinline__ void store_cell(void *base, uint32_t cell, const float *v) { store_vec4<T>(base, cell, v); }   // ONE 16- / 8-byte vector
};

}  // namespace odtk
