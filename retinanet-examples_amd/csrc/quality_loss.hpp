// quality_loss.hpp -- Quality Focal Loss (GFL, arXiv 2006.04388 eq. 4) and Varifocal Loss (VarifocalNet, arXiv 2008.13367 eq. 2,
// as mmdetection implements it) over the class logits of every pyramid level of the batch: the opt-in alternatives to the focal
// walk of loss.hpp (`Model.cls_loss`, `odtk train --cls-loss`), axis-aligned boxes only.  The class score is trained as a
// localisation-quality estimate: at a foreground anchor the target of the assigned class is the IoU between the box the network
// predicts there and the box it was assigned.  No reference equivalent.
//
// The definition (the contract; restated in torch in odtk/loss.py, in float64 numpy in tests/quality_loss_ref.py).  Per level:
//     depth = -1 ignore / 0 background / class + 1;   x = a class logit (head dtype -> float32);   s = sigmoid(x), sp = softplus(x)
//     q (foreground anchors only) = 1 - box_iou_loss(predicted deltas, target deltas, anchor sizes, 'iou'): box_iou_loss.hpp's own
//         term -- clip at BBOX_XFORM_CLIP, eps = 1e-7, decoded relative to the anchor centre -- so the bits `--box-loss iou` sees.
//         A constant of this loss: nothing flows into the box head.  A NaN delta at a foreground anchor makes q NaN.
//     y = q where depth - 1 == class, else 0.  Elements of ignored anchors (depth < 0) contribute 0 and get gradient +0 whatever
//         their logit (NaN included); the box head is never read at a cell that is not foreground.
//     qfl (gamma >= 1):   L = |s - y|^gamma (sp - y x)                       (y x = 0 where y = 0, an infinite logit included)
//                         dL/dx = gamma |s - y|^(gamma-1) sign(s - y) s (1 - s) (sp - y x) + |s - y|^gamma (s - y)
//     vfl (alpha, gamma): y > 0 (or NaN, so that it reaches the sum):  L = y (sp - y x),  dL/dx = y (s - y)
//                         otherwise:  L = alpha s^gamma sp  (also a foreground anchor whose predicted box misses its target, q == 0)
//     For y = 0 both are w s^gamma sp with w = 1 (qfl) or alpha (vfl): focal_term's negative form, focal_plain's for gamma = 2.
//     cls_sum = sum of L over the elements of non-ignored anchors (float64, one fixed order: the same bits on every run),
//     fg = number of foreground anchors.  Backward: d(logits) = g[level] dL/dx, every element written, in the head's dtype and
//     layout, rounded once at the store; d(deltas) is never written.
//
// Shape: loss.hpp's focal_stream with a soft target.  One launch per direction for all levels (level table and anchor SIZES in the
// kernel arguments); a lane streams 16-byte non-temporal vectors of logits as the convolution wrote them (fp32 / bf16 / fp16, NCHW
// or channels_last), a wave's vectors of a trip contiguous, index arithmetic by fastdiv.hpp.  About one vector in a thousand
// holds an element that is its anchor's class: only that vector gathers the anchor's 4 + 4 deltas (box_iou_load) and evaluates
// box_iou_term<false> in place -- no quality map, no target tensor, no extra launch; backward recomputes q the same way.  With
// gamma = 2 every other vector without a logit beyond kPlainMax takes focal_plain with one weight for the launch.  Class counts
// that are no multiple of the vector, levels whose H*W is not, and the n % kPer tail go element by element with carries.
// Forward: per-workgroup (cls_sum, fg) into the workspace, then level_pair_reduce_kernel adds a level's pairs up in a fixed order.
// The foreground count is taken where the walk meets class 0 of an anchor (every anchor has exactly one such element).
// No atomics, no scratch.  Measured: DESIGN.md (tools/quality_loss_probe.py, profiles/r12_quality_loss_probe.txt).
#pragma once

#include "box_iou_loss.hpp"   // box_iou_load, box_iou_term; cell_loss.hpp: CellLossLevel, store_block_pair, level_pair_reduce_kernel; loss.hpp: focal_term, ...

namespace odtk {

constexpr int kQualityThreads = 256;

struct QualityLevel {
  CellLossLevel b;           // box, depth, box_target, g (backward: device scalar d(out)/d(cls_sum)), hw, channels_last, by_hw,
                            // by_anchors, the anchor sizes; dbox is never written and stays null
  const void *cls;          // [B, A*C, H, W] logits, element type T, layout of box
  void *dcls;               // backward: gradient, dtype / layout of cls
  uint32_t n, pad_;         // B*A*C*H*W (< 2^32: host)
  FastDiv by_channels, by_classes;   // A*C, C
};

struct QualityArgs {
  QualityLevel lv[ODTK_MAX_LEVELS];
  uint32_t block_begin[ODTK_MAX_LEVELS + 1];
  double *partial;          // forward: [gridDim.x][2] = (cls_sum, fg) per workgroup
  uint32_t n_levels, num_anchors, num_classes, kind;
  float alpha, gamma;
};

// q of the foreground cell (image, anchor `an`, pixel), ia = image * A + an
template <typename T>
__device__ __forceinline__ float quality_at(const QualityLevel &L, uint32_t A, uint32_t ia, uint32_t an, uint32_t pix) {
  float p[4], t[4];
  box_iou_load<T>(L.b, A, ia, an, pix, p, t);                     // what BoxIouLoss::load / ::term forward to
  return 1.0f - box_iou_term<false>(p, t, L.b.aw[an], L.b.ah[an], ODTK_BOX_LOSS_IOU, nullptr);
}

// The element that is its anchor's class, target y = q.  kBackward = false: L; true: dL/dx (the caller applies the upstream gradient).
// The same three hardware transcendentals as focal_term; `sp - y x` is formed as (max(x, 0) - y x) + ln(1 + exp(-|x|)), the large
// parts first, so that it keeps its relative accuracy where y x cancels most of sp.
template <bool kBackward, bool kGamma2>
__device__ __forceinline__ float quality_term(float x, float y, bool vfl, float gamma) {
  const float e = __builtin_amdgcn_exp2f(fabsf(x) * -1.4426950408889634f);      // exp(-|x|) in (0, 1]
  const float d = 1.0f + e;
  const float r = __builtin_amdgcn_rcpf(d);
  const float er = e * r;
  const bool nonneg = x >= 0.0f;
  const float s = nonneg ? r : er;                                               // sigmoid(x)
  const float ce = fmaf(__builtin_amdgcn_logf(d), 0.6931471805599453f, fmaf(-y, x, fmaxf(x, 0.0f)));   // sp - y x
  const float u = s - y;
  if (vfl) return kBackward ? y * u : y * ce;
  const float oms = nonneg ? er : r;                                             // 1 - sigmoid(x), no cancellation
  if constexpr (kGamma2) {
    if constexpr (!kBackward) return u * u * ce;
    else return u * fmaf(2.0f * (s * oms), ce, u * u);
  } else {
    // |u|^gamma = exp2(gamma log2 |u|) on the hardware units; log2 0 = -inf is held at -150 as in focal_term (gamma - 1 = 0 gives
    // |u|^0 = 1 as torch's pow does; sign(0) = 0 then removes the term as autograd does)
    const float au = fabsf(u);
    const float l2 = fmaxf(__builtin_amdgcn_logf(au), -150.0f);
    if constexpr (!kBackward) return __builtin_amdgcn_exp2f(gamma * (au != au ? au : l2)) * ce;     // (fmaxf drops a NaN)
    else {
      const float m1 = __builtin_amdgcn_exp2f((gamma - 1.0f) * (au != au ? au : l2));               // |u|^(gamma - 1)
      const float sg = u > 0.0f ? 1.0f : (u < 0.0f ? -1.0f : u);                                    // (a NaN stays one)
      return gamma * m1 * sg * (s * oms) * ce + m1 * au * u;
    }
  }
}

// One element by the definition: `d` its anchor's depth, `c` its class, `q` the anchor's quality (read only where d == c + 1).
// w_neg = the weight of the negative form (x the upstream gradient backward), g = the upstream gradient (forward: 1).
// q <= 0 (the predicted box misses its target) takes the negative form in both kinds: varifocal by definition, quality focal because
// its y = 0 form IS the negative form; a NaN q fails the comparison and reaches the sum through quality_term.
template <bool kBackward, bool kGamma2>
__device__ __forceinline__ float quality_element(float x, bool is_target, float q, bool vfl, float w_neg, float g, float gamma) {
  if (is_target && !(q <= 0.0f)) {
    const float t = quality_term<kBackward, kGamma2>(x, q, vfl, gamma);
    return kBackward ? g * t + 0.0f : t;                     // (a zero is +0: no upstream gradient stores all-zero bits)
  }
  return focal_term<kBackward, kGamma2>(x, false, w_neg, w_neg, gamma);
}

// offset r in memory order -> (image * A + anchor, anchor, class, pixel)
template <bool kCL>
__device__ __forceinline__ void quality_decompose(const QualityLevel &L, uint32_t A, uint32_t r, uint32_t *ia, uint32_t *an, uint32_t *c,
                                                  uint32_t *pix) {
  if constexpr (kCL) {
    uint32_t ch;
    const uint32_t p = fastdivmod(r, L.by_channels, &ch);
    const uint32_t img = fastdivmod(p, L.b.by_hw, pix);
    *an = fastdivmod(ch, L.by_classes, c);
    *ia = img * A + *an;
  } else {
    const uint32_t q = fastdivmod(r, L.b.by_hw, pix);           // (img * A + an) * C + c
    *ia = fastdivmod(q, L.by_classes, c);
    fastdivmod(*ia, L.b.by_anchors, an);
  }
}

// One workgroup's share of one level's logits.  Forward: returns the lane's cls_sum, adds its foreground anchors to *fg_out.
template <typename T, bool kBackward, bool kGamma2, bool kCL, int kUnroll>
__device__ __forceinline__ double quality_stream(const QualityLevel &L, const QualityArgs &a, uint32_t block, uint32_t n_blocks, double *fg_out) {
  constexpr int kPer = T::kPerLoad;
  constexpr int kDep = kCL ? 1 : kPer;                     // depth words per fast vector
  const uint32_t A = a.num_anchors, C = a.num_classes, hw = L.b.hw;
  const bool vfl = a.kind == ODTK_CLS_LOSS_VFL;
  const float g = kBackward ? (L.b.g ? *L.b.g : 0.0f) : 1.0f;
  const float w_neg = (vfl ? a.alpha : 1.0f) * g;
  const float gamma = a.gamma;
  const uint32_t n = L.n, n_vec = n / kPer;
  const vuint4 *src = static_cast<const vuint4 *>(L.cls);
  // a wave's kUnroll vectors of a trip are contiguous (loss.hpp: window 1)
  const uint32_t stride = n_blocks * kQualityThreads * kUnroll;
  const uint32_t first = (block * kQualityThreads + (threadIdx.x & ~static_cast<uint32_t>(kWave - 1))) * kUnroll + (threadIdx.x & (kWave - 1));
  double acc = 0.0;
  float n_fg = 0.0f;                                       // (< 2^24 per lane: a lane meets n / (kPer * lanes) vectors)

  // n_vec <= 2^30 and the host keeps stride below 2^21 vectors (train.hip: quality_fill), so v0 cannot wrap
  for (uint32_t v0 = first; v0 < n_vec; v0 += stride) {
    vuint4 raw[kUnroll];
    float dep[kUnroll][kDep];
    uint32_t c0[kUnroll];                                  // class of the vector's first element
    bool fast[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint32_t v = v0 + u * kWave;
      fast[u] = false;
      c0[u] = 0;
#pragma unroll
      for (int e = 0; e < kDep; ++e) dep[u][e] = -1.0f;
      if (v < n_vec) {
        raw[u] = __builtin_nontemporal_load(src + v);
        uint32_t ia, an, c, pix;
        quality_decompose<kCL>(L, A, v * kPer, &ia, &an, &c, &pix);
        c0[u] = c;
        fast[u] = kCL ? c + kPer <= C : pix + kPer <= hw;
        if (fast[u]) {
#pragma unroll
          for (int e = 0; e < kDep; ++e) dep[u][e] = L.b.depth[ia * hw + pix + e];
        }
      } else {
        raw[u] = vuint4{0u, 0u, 0u, 0u};
      }
    }
    float sum = 0.0f;                                      // fp32 partial of <= kUnroll * kPer <= 16 elements -> fp64
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint32_t v = v0 + u * kWave;
      if (v >= n_vec) break;
      float out[kPer];
      if (fast[u]) {
        const float tgt0 = static_cast<float>(c0[u] + 1);
        // does the vector hold an element that is its anchor's class?  depth is integral by contract
        bool plain;
        if constexpr (kCL) {
          const float rel = dep[u][0] - tgt0;
          plain = !(rel >= 0.0f && rel < static_cast<float>(kPer));
        } else {
          plain = true;
#pragma unroll
          for (int e = 0; e < kPer; ++e) plain = plain && dep[u][e] != tgt0;
        }
        if constexpr (!kBackward) {
          if (c0[u] == 0) {                                // class 0 of kDep anchors: count the foreground ones
#pragma unroll
            for (int e = 0; e < kDep; ++e) n_fg += dep[u][e] > 0.0f ? 1.0f : 0.0f;
          }
        }
        float vs = 0.0f;
        bool done = false;
        if constexpr (kGamma2) {
          float mx = vec_elem<T>(raw[u], 0);
#pragma unroll
          for (int e = 1; e < kPer; ++e) mx = fmaxf(mx, vec_elem<T>(raw[u], e));
          if (plain && mx <= kPlainMax) {
            // a vector of negatives (or ignored cells): one weight for the whole vector
            const float wv = kBackward ? w_neg : w_neg * 0.6931471805599453f;
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
              const float t = focal_plain<kBackward>(vec_elem<T>(raw[u], e));
              if constexpr (kBackward) out[e] = dep[u][kCL ? 0 : e] >= 0.0f ? wv * t : 0.0f;
              else if constexpr (kCL) vs += t;
              else vs += dep[u][e] >= 0.0f ? t : 0.0f;
            }
            vs *= wv;
            done = true;
          }
        }
        if (!done) {
          // the rare vector: the anchors whose class lies in it gather their deltas (foreground by construction: depth = class + 1 >= 1)
          uint32_t ia = 0, an = 0, c = 0, pix = 0;
          if (!plain) quality_decompose<kCL>(L, A, v * kPer, &ia, &an, &c, &pix);
          float qv = 0.0f;
          if constexpr (kCL) {
            if (!plain) qv = quality_at<T>(L, A, ia, an, pix);
          }
#pragma unroll
          for (int e = 0; e < kPer; ++e) {
            const float d = dep[u][kCL ? 0 : e];
            const bool is_target = d == (kCL ? tgt0 + static_cast<float>(e) : tgt0);
            if constexpr (!kCL) {
              if (is_target) qv = quality_at<T>(L, A, ia, an, pix + e);
            }
            const float t = quality_element<kBackward, kGamma2>(vec_elem<T>(raw[u], e), is_target, qv, vfl, w_neg, g, gamma);
            if constexpr (kBackward) out[e] = d >= 0.0f ? t : 0.0f;
            else if constexpr (kCL) vs += t;
            else vs += d >= 0.0f ? t : 0.0f;
          }
        }
        if constexpr (!kBackward) sum += kCL ? (dep[u][0] >= 0.0f ? vs : 0.0f) : vs;
      } else {
        // decompose the first element; the others follow by increment with carry (i2 * A + a2 is kept as ia2)
        uint32_t ia2, a2, c2, p2;
        quality_decompose<kCL>(L, A, v * kPer, &ia2, &a2, &c2, &p2);
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
          const float d = L.b.depth[ia2 * hw + p2];
          const bool is_target = d == static_cast<float>(c2 + 1);
          float qv = 0.0f;
          if (is_target) qv = quality_at<T>(L, A, ia2, a2, p2);
          const float t = quality_element<kBackward, kGamma2>(vec_elem<T>(raw[u], e), is_target, qv, vfl, w_neg, g, gamma);
          if constexpr (kBackward) out[e] = d >= 0.0f ? t : 0.0f;
          else {
            sum += d >= 0.0f ? t : 0.0f;
            if (c2 == 0 && d > 0.0f) n_fg += 1.0f;
          }
          if constexpr (kCL) {
            // (image, pixel, anchor, class): the next anchor of the same pixel is ia2 + 1; the next pixel starts at anchor 0 again
            if (++c2 == C) { c2 = 0; ++ia2; if (++a2 == A) { a2 = 0; ia2 -= A; if (++p2 == hw) { p2 = 0; ia2 += A; } } }
          } else {
            if (++p2 == hw) { p2 = 0; if (++c2 == C) { c2 = 0; ++ia2; if (++a2 == A) a2 = 0; } }
          }
        }
      }
      if constexpr (kBackward) __builtin_nontemporal_store(pack_vec<T>(out), static_cast<vuint4 *>(L.dcls) + v);
    }
    if constexpr (!kBackward) acc += sum;
  }

  // scalar tail (n % kPer elements), first block only
  if (block == 0 && threadIdx.x < n - n_vec * kPer) {
    const uint32_t r = n_vec * kPer + threadIdx.x;
    uint32_t ia, an, c, pix;
    quality_decompose<kCL>(L, A, r, &ia, &an, &c, &pix);
    const float d = L.b.depth[ia * hw + pix];
    const bool is_target = d == static_cast<float>(c + 1);
    float qv = 0.0f;
    if (is_target) qv = quality_at<T>(L, A, ia, an, pix);
    const float t = quality_element<kBackward, kGamma2>(load_raw<T>(L.cls, r), is_target, qv, vfl, w_neg, g, gamma);
    if constexpr (kBackward) store_elem<T>(L.dcls, r, d >= 0.0f ? t : 0.0f);
    else {
      acc += d >= 0.0f ? t : 0.0f;
      if (c == 0 && d > 0.0f) n_fg += 1.0f;
    }
  }
  if constexpr (!kBackward) *fg_out = n_fg;
  return acc;
}

// The workgroups of level l are [block_begin[l], block_begin[l + 1]).  kBackward = false: (cls_sum, fg) of the workgroup into the
// workspace; true: d(logits).
template <typename T, bool kBackward, int kUnroll>
__global__ __launch_bounds__(kQualityThreads) void quality_loss_kernel(const QualityArgs a) {
  __shared__ double s_red[kQualityThreads / kWave];
  const int l = level_of<ODTK_MAX_LEVELS>(a.block_begin, a.n_levels);
  const QualityLevel &L = a.lv[l];
  const uint32_t block = blockIdx.x - a.block_begin[l], n_blocks = a.block_begin[l + 1] - a.block_begin[l];
  const bool g2 = a.gamma == 2.0f;                         // launch-uniform
  double fg = 0.0;
  double acc;
  if (L.b.channels_last) acc = g2 ? quality_stream<T, kBackward, true, true, kUnroll>(L, a, block, n_blocks, &fg)
                                  : quality_stream<T, kBackward, false, true, kUnroll>(L, a, block, n_blocks, &fg);
  else acc = g2 ? quality_stream<T, kBackward, true, false, kUnroll>(L, a, block, n_blocks, &fg)
                : quality_stream<T, kBackward, false, false, kUnroll>(L, a, block, n_blocks, &fg);
  if constexpr (!kBackward) store_block_pair(acc, fg, s_red, a.partial);
}

}  // namespace odtk
