// rotated_box_loss.hpp -- ProbIoU / KLD box-regression losses on the Gaussians of rotated boxes, at the foreground anchors of every
// pyramid level of the batch: the opt-in alternative to the smooth-L1 walk of loss.hpp for rotated models (`Model.box_loss`,
// `odtk train --rotated-bbox --box-loss probiou|kld`).  No reference equivalent; ProbIoU as in arXiv 2106.06072, KLD as in
// arXiv 2106.01883 (mmrotate's form), both on the covariance of the uniform distribution on the rectangle.
//
// The definition (the contract; restated in torch in odtk/loss.py:rotated_box_loss, the ground truth of
// tests/test_gpu_rotated_box_loss.py).  One foreground anchor (depth > 0) of anchor slot a; (aw, ah) = (x2 - x1 + 1, y2 - y1 + 1)
// of the level's AXIS anchor table; p = the six predicted deltas (head dtype -> float32), t = the six target deltas, (t4, t5) the
// box's (sin, cos).  Both boxes are decoded relative to the anchor centre -- the cell position cancels:
//     CLIP = log(1000 / 16);  pw' = min(p2, CLIP), ph' = min(p3, CLIP)            (predictions only; gradient 0 beyond the clip)
//     centre (p0 aw, p1 ah);  w = exp(pw') aw,  h = exp(ph') ah                   target: the same from t, unclipped
//     q = p4^2 + p5^2 + 1e-12;  cc = p5^2 / q,  ss = p4^2 / q,  sc = p4 p5 / q    (no atan2, no sqrt; target: the same from t4, t5)
//     a = (w^2 cc + h^2 ss) / 12     b = (w^2 ss + h^2 cc) / 12     c = -(w^2 - h^2) sc / 12
// [[a, c], [c, b]] is the covariance of the uniform distribution on the rotated rectangle in the convention of
// odtk/box.py:rotate_boxes (width axis (cos, -sin), height axis (sin, cos)).  Index 1 the prediction, 2 the target;
// (dx, dy) = centre(P) - centre(T):
//     probiou: A = a1 + a2, B = b1 + b2, C = c1 + c2, D = A B - C^2
//              BD = (B dx^2 + A dy^2 - 2 C dx dy) / (4 D) + 0.5 ln(36 D / (w h tw th))              (Bhattacharyya distance)
//              BD' = min(max(BD, 0), 100)       L = sqrt(1 - exp(-BD') + 1e-7)                       (gradient 0 where clamped)
//     kld:     d2 = (tw th / 12)^2
//              K = 0.5 [(b2 a1 + a2 b1 - 2 c2 c1) / d2 + (b2 dx^2 + a2 dy^2 - 2 c2 dx dy) / d2 - 2] + (t2 + t3 - pw' - ph')
//              K' = max(K, 0)                   L = 1 - 1 / (1 + ln(1 + K'))                         (KL(N_pred || N_target))
// min / max hand a NaN on (nan_min / nan_max as in box_iou_loss.hpp).  The loss does not depend on the length of (p4, p5), as the
// decode's atan2 does not: its gradient on the pair is tangential and scales with 1 / sqrt(q).  For w = h the angle gradient is 0.
// Per level: box_sum = sum of L over the foreground anchors (float64, one fixed order: the same bits on every run), fg = their
// number.  Backward: d(deltas) = g[level] dL/dp for all six deltas at the foreground cells and +0 everywhere else, every element
// written, in the head's dtype and layout, rounded once at the store; cells that are not foreground are never read from the head.
// Arithmetic: the float32 deltas are widened and each anchor's term runs in IEEE DOUBLE (ocml exp / log / log1p / sqrt): BD and K
// are small differences of O(1) terms (A B - C^2, the ln term near identical boxes, trace - 2), and probiou's gradient goes with
// BD^-1/2 -- evaluated in float32 (the torch definition on float32 inputs) single anchors miss the gradient bar of the other loss
// kernels, 1e-5 of the level's largest, by up to 4 x at sigma = 0.15 (tests/test_gpu_rotated_box_loss.py).  ~1 % of the lanes have
// work, so the double arithmetic costs nothing that shows.  The gradient is in closed form: both boxes to
// (cx, cy, w, h, a, b, c), the kind's scalar loss with its partials by (dx, dy, a1, b1, c1, w, h), one common chain to the deltas.
// Nothing here forms D^2: d(BD)/dD is written as (1/2 - t1) / D.
//
// Shape: cell_loss.hpp's kernels with the policy RotatedBoxLoss (below; six parameters per anchor) -- two launches for all levels
// and the fixed-order sum, one lane per anchor cell, ~1 % of the lanes with work.
//   forward : lanes in depth's order (image, anchor, pixel); a foreground lane gathers its 6 + 6 deltas.
//   backward: lanes in the order d(deltas) lies in memory -- NCHW: (image, anchor, pixel), six plane stores; NHWC: (image, pixel,
//             anchor), the cell's 24 (fp32) or 12 (16-bit) bytes as THREE 8- / 4-byte pieces per lane (a cell is 8- / 4-byte
//             aligned, not 16): a wave's stores are one run of 1536 / 768 bytes.
// Measured: DESIGN.md (tools/rotated_box_loss_probe.py).
#pragma once

#include "box_iou_loss.hpp"   // nan_min / nan_max in float; cell_loss.hpp: CellLossLevel, the kernels that take RotatedBoxLoss

namespace odtk {

constexpr double kRotatedDirEps = 1e-12;
constexpr double kProbIouEps = 1e-7;
constexpr double kProbIouMaxDistance = 100.0;
constexpr double kRotatedClip = 4.135166556742356;       // log(1000 / 16) in double: the clip of the float64 definition

// One box as the losses see it.
struct RotatedGauss {
  double cx, cy, w, h;       // centre relative to the anchor centre, size
  double cc, ss, sc, q;      // cos^2, sin^2, sin cos of the direction pair, and its squared length + eps
  double a, b, c;            // covariance [[a, c], [c, b]]
};

__device__ __forceinline__ RotatedGauss rotated_gauss(const double *d, double lw, double lh, double aw, double ah) {
  RotatedGauss g;
  g.cx = d[0] * aw;
  g.cy = d[1] * ah;
  g.w = exp(lw) * aw;
  g.h = exp(lh) * ah;
  g.q = d[4] * d[4] + d[5] * d[5] + kRotatedDirEps;
  g.cc = d[5] * d[5] / g.q;
  g.ss = d[4] * d[4] / g.q;
  g.sc = d[4] * d[5] / g.q;
  const double w2 = g.w * g.w, h2 = g.h * g.h;
  g.a = (w2 * g.cc + h2 * g.ss) * (1.0 / 12.0);
  g.b = (w2 * g.ss + h2 * g.cc) * (1.0 / 12.0);
  g.c = -(w2 - h2) * g.sc * (1.0 / 12.0);
  return g;
}

// min / max that hand a NaN of either side on, in double (the float forms: box_iou_loss.hpp)
__device__ __forceinline__ double nan_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

// L of one anchor, evaluated in double from the float32 deltas; kGrad: also dL/dp (six numbers).
template <bool kGrad>
__device__ __forceinline__ double rotated_box_term(const float *pf, const float *tf, float awf, float ahf, uint32_t kind, double *grad) {
  double p[6], t[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    p[k] = pf[k];
    t[k] = tf[k];
  }
  const double aw = awf, ah = ahf;
  const RotatedGauss P = rotated_gauss(p, nan_min(p[2], kRotatedClip), nan_min(p[3], kRotatedClip), aw, ah);
  const RotatedGauss T = rotated_gauss(t, t[2], t[3], aw, ah);
  const double dx = P.cx - T.cx, dy = P.cy - T.cy;
  double loss;
  // reverse mode: g_x = dL/dx of the kind's scalar, by (dx, dy, a1, b1, c1) and by (w, h) where they enter directly
  double g_dx = 0.0, g_dy = 0.0, g_a = 0.0, g_b = 0.0, g_c = 0.0, g_w = 0.0, g_h = 0.0;
  if (kind == ODTK_ROTATED_BOX_LOSS_PROBIOU) {
    const double A = P.a + T.a, B = P.b + T.b, C = P.c + T.c;
    const double D = A * B - C * C;
    const double t1 = (B * dx * dx + A * dy * dy - 2.0 * C * dx * dy) / (4.0 * D);
    const double bd = t1 + 0.5 * log(36.0 * D / (P.w * P.h * T.w * T.h));
    const double bdc = nan_min(nan_max(bd, 0.0), kProbIouMaxDistance);
    const double e = exp(-bdc);
    loss = sqrt(1.0 - e + kProbIouEps);
    if constexpr (kGrad) {
      const double g_bd = (bd > 0.0 && bd < kProbIouMaxDistance) ? e / (2.0 * loss) : 0.0;
      const double inv = 1.0 / D;
      const double k = (0.5 - t1) * inv;                             // d(BD)/dD
      g_dx = g_bd * 0.5 * (B * dx - C * dy) * inv;
      g_dy = g_bd * 0.5 * (A * dy - C * dx) * inv;
      g_a = g_bd * (0.25 * dy * dy * inv + k * B);
      g_b = g_bd * (0.25 * dx * dx * inv + k * A);
      g_c = g_bd * (-0.5 * dx * dy * inv - 2.0 * k * C);
      g_w = g_bd * -0.5 / P.w;
      g_h = g_bd * -0.5 / P.h;
    }
  } else {
    const double sd = T.w * T.h * (1.0 / 12.0);
    const double inv = 1.0 / (sd * sd);
    const double tr = T.b * P.a + T.a * P.b - 2.0 * T.c * P.c;
    const double mh = T.b * dx * dx + T.a * dy * dy - 2.0 * T.c * dx * dy;
    const double kl = 0.5 * (tr * inv + mh * inv - 2.0) + (t[2] + t[3] - nan_min(p[2], kRotatedClip) - nan_min(p[3], kRotatedClip));
    const double klc = nan_max(kl, 0.0);
    const double den = 1.0 + log1p(klc);
    loss = 1.0 - 1.0 / den;
    if constexpr (kGrad) {
      const double g_kl = kl > 0.0 ? 1.0 / ((1.0 + klc) * den * den) : 0.0;
      g_dx = g_kl * (T.b * dx - T.c * dy) * inv;
      g_dy = g_kl * (T.a * dy - T.c * dx) * inv;
      g_a = g_kl * 0.5 * T.b * inv;
      g_b = g_kl * 0.5 * T.a * inv;
      g_c = -g_kl * T.c * inv;
      g_w = -g_kl / P.w;
      g_h = -g_kl / P.h;
    }
  }
  if constexpr (kGrad) {
    // the common chain: (a, b, c) -> (w^2, h^2, cc, ss, sc) -> the deltas
    const double w2 = P.w * P.w, h2 = P.h * P.h;
    const double g_w2 = (g_a * P.cc + g_b * P.ss - g_c * P.sc) * (1.0 / 12.0);
    const double g_h2 = (g_a * P.ss + g_b * P.cc + g_c * P.sc) * (1.0 / 12.0);
    const double g_cc = (g_a * w2 + g_b * h2) * (1.0 / 12.0);
    const double g_ss = (g_a * h2 + g_b * w2) * (1.0 / 12.0);
    const double g_sc = -g_c * (w2 - h2) * (1.0 / 12.0);
    const double iq = 1.0 / P.q;
    grad[0] = g_dx * aw;
    grad[1] = g_dy * ah;
    grad[2] = p[2] < kRotatedClip ? (g_w + 2.0 * P.w * g_w2) * P.w : 0.0;
    grad[3] = p[3] < kRotatedClip ? (g_h + 2.0 * P.h * g_h2) * P.h : 0.0;
    grad[4] = (2.0 * p[4] * (g_ss * (1.0 - P.ss) - g_cc * P.cc) + g_sc * (p[5] - 2.0 * p[4] * P.sc)) * iq;
    grad[5] = (2.0 * p[5] * (g_cc * (1.0 - P.cc) - g_ss * P.ss) + g_sc * (p[4] - 2.0 * p[5] * P.sc)) * iq;
  }
  return loss;
}

// the six deltas of cell (image, anchor `an`, pixel) with ia = image * A + an: NHWC three 8- / 4-byte pieces, NCHW six planes
template <typename T>
__device__ __forceinline__ void rotated_box_load(const CellLossLevel &L, uint32_t A, uint32_t ia, uint32_t an, uint32_t pix, float *p, float *t) {
  const uint32_t plane = ia * 6u * L.hw + pix;
#pragma unroll
  for (uint32_t k = 0; k < 6; ++k) t[k] = L.box_target[plane + k * L.hw];
  if (L.channels_last) {
    const uint32_t v = ((ia - an) * L.hw + pix * A + an) * 3u;       // 3 * ((image * hw + pix) * A + an): the cell's first piece
    if constexpr (std::is_same_v<T, F32>) {
#pragma unroll
      for (uint32_t k = 0; k < 3; ++k) {
        const uint2 raw = static_cast<const uint2 *>(L.box)[v + k];
        p[2 * k] = __uint_as_float(raw.x);
        p[2 * k + 1] = __uint_as_float(raw.y);
      }
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 3; ++k) {
        const uint32_t raw = static_cast<const uint32_t *>(L.box)[v + k];
        p[2 * k] = std::is_same_v<T, BF16> ? bf16_bits_to_float(raw & 0xffffu) : f16_bits_to_float(raw & 0xffffu);
        p[2 * k + 1] = std::is_same_v<T, BF16> ? bf16_bits_to_float(raw >> 16) : f16_bits_to_float(raw >> 16);
      }
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) p[k] = load_raw<T>(L.box, plane + k * L.hw);
  }
}

// six consecutive elements, element index 6 * cell, as three pieces (the base is 8- / 4-byte aligned: checked by the host)
template <typename T>
__device__ __forceinline__ void store_vec6(void *base, uint32_t cell, const float *v) {
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) {
    if constexpr (std::is_same_v<T, F32>) {
      static_cast<uint2 *>(base)[3u * cell + k] = uint2{__float_as_uint(v[2 * k]), __float_as_uint(v[2 * k + 1])};
    } else {
      uint32_t h[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if constexpr (std::is_same_v<T, BF16>) h[e] = __float_as_uint(round_to_bf16(v[2 * k + e])) >> 16;
        else h[e] = __builtin_bit_cast(uint16_t, static_cast<_Float16>(v[2 * k + e]));
      }
      static_cast<uint32_t *>(base)[3u * cell + k] = h[0] | (h[1] << 16);
    }
  }
}

// The Gaussian family as cell_loss.hpp's kernels see it.
struct RotatedBoxLoss {
  static constexpr uint32_t kParams = 6;
  using Grad = double;
  template <typename T>
  static __device__ __forceinline__ void load(const CellLossLevel &L, uint32_t A, uint32_t ia, uint32_t an, uint32_t pix, float *p, float *t) {
    rotated_box_load<T>(L, A, ia, an, pix, p, t);
  }
  template <bool kGrad>
  static __device__ __forceinline__ double term(const float *p, const float *t, float aw, float ah, uint32_t kind, double *grad) {
    return rotated_box_term<kGrad>(p, t, aw, ah, kind, grad);
  }
  // the product in double, one rounding; a zero always +0
  static __device__ __forceinline__ float grad_value(float g, double grad) { return static_cast<float>(static_cast<double>(g) * grad + 0.0); }
  template <typename T>
  static __device__ __forceinline__ void store_cell(void *base, uint32_t cell, const float *v) { store_vec6<T>(base, cell, v); }   // THREE 8- / 4-byte pieces
};

}  // namespace odtk
