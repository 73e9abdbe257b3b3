// soft_nms.hpp -- batched class-aware Soft-NMS (Bodla et al. 2017, linear and Gaussian): one 1024-thread workgroup per
// image, everything on chip, one barrier per emitted detection.
//
// No reference equivalent (the reference only has the hard rule of csrc/nms.hpp).  Definition, all in float32:
//   w = scores; alive iff w > 0.  Up to `ndet` times: pick the alive candidate with the largest w (ties: lowest input
//   position), emit (w, box, class, position), retire it, then visit every alive candidate j of the pick's class:
//     iou as box.py:321-332 (+1 pixel, `inter / (area_j + area_i - inter)`, torch.max / min / clamp NaN rules)
//     linear   : if !(iou <= thresh)  w_j = w_j * (1 - iou)
//     gaussian : w_j = w_j * exp_cr((-(iou * iou)) / sigma)           (three separate float32 operations, then one exp)
//     j stays alive iff w_j >= min_score  (a NaN does not).
//   The remaining output slots are zero (index -1), as odtk_nms pads.  Decays only lower scores, so the emitted scores are
//   non-increasing and nothing is sorted.
//
// Shape.  count <= ODTK_MAX_NMS_COUNT (7680): thread t owns the candidates at positions t, t + 1024, ... (up to 8) in
// REGISTERS -- box, class, working score: the decay of a round touches no memory.  A copy of every box and class also lies
// in LDS (count x 20 bytes, <= 150 KiB), so that the winner of a round is readable by everybody as soon as its position is
// known, without a second barrier:
//   round :  per-thread maximum of the packed key (w bits << 32 | ~position) over the owned candidates -> wave maximum on
//            the DPP network -> 16 partials in LDS (two buffers, by the round's parity) -> barrier -> every thread reads the
//            16 partials and the winner's box and class (broadcast reads) -> the owner emits and retires, everybody decays.
// A positive float's bit pattern orders like the float, and a dead candidate keeps w = 0, so key 0 means "nobody alive".
#pragma once

#include "common.hpp"
#include "../../include/odtk_hip.h"

namespace odtk {

constexpr int kSoftThreads = 1024;
constexpr int kSoftSlots = (ODTK_MAX_NMS_COUNT + kSoftThreads - 1) / kSoftThreads;   // 8 candidates per thread
constexpr int kSoftWaves = kSoftThreads / kWave;

struct SoftNmsArgs {
  const float *scores;     // [batch, count]
  const float *boxes;      // [batch, count, 4]
  const float *classes;    // [batch, count]
  float *out_scores;       // [batch, ndet]
  float *out_boxes;        // [batch, ndet, 4]
  float *out_classes;      // [batch, ndet]
  int32_t *out_indices;    // optional [batch, ndet]
  uint32_t count;          // <= ODTK_MAX_NMS_COUNT
  int ndet;
  float thresh;
  float sigma;
  float min_score;
};

// dynamic LDS of a launch: [count] float4 boxes | [count] float classes
__host__ __device__ inline size_t soft_nms_lds_bytes(uint32_t count) { return static_cast<size_t>(count) * (sizeof(float4) + sizeof(float)); }

// The decayed score of candidate (jb, w) after box m (area marea) of its class was picked, 0 when it does not stay alive.
template <bool kGaussian>
__device__ __forceinline__ float soft_decay(const float4 m, float marea, const float4 j, float w, float thr, float sigma, float min_score) {
  // torch.max / torch.min / clamp propagate NaN
  const float x1 = tmax_nan(j.x, m.x), y1 = tmax_nan(j.y, m.y);
  const float x2 = tmin_nan(j.z, m.z), y2 = tmin_nan(j.w, m.w);
  float iw = x2 - x1 + 1.0f, ih = y2 - y1 + 1.0f;
  iw = iw < 0.0f ? 0.0f : iw;  // clamp(0)
  ih = ih < 0.0f ? 0.0f : ih;
  const float inter = iw * ih;
  const float jarea = (j.z - j.x + 1.0f) * (j.w - j.y + 1.0f);
  const float both = jarea + marea;
  // disjoint boxes (almost every same-class pair): the quotient is +-0 whatever the non-zero, non-NaN union is; linear leaves
  // w alone (or multiplies by 1 - +-0 = 1 when thresh < 0) and gaussian multiplies by exp(-0) = 1: w is unchanged, bit for bit,
  // without the division and the double-precision exp.  A zero or NaN union (0 / 0) takes the general path.
  if (!(inter == 0.0f && both == both && both != 0.0f)) {
    const float iou = inter / (both - inter);
    if constexpr (kGaussian) {
      const float sq = iou * iou;
      const float e = (-sq) / sigma;
      w = w * exp_cr(e);
    } else {
      if (!(iou <= thr)) w = w * (1.0f - iou);
    }
  }
  return w >= min_score ? w : 0.0f;
}

template <bool kGaussian>
__global__ __launch_bounds__(kSoftThreads) void soft_nms_kernel(const SoftNmsArgs a) {
  extern __shared__ float4 s_soft[];
  __shared__ uint64_t s_part[2][kSoftWaves];
  const uint32_t count = a.count;
  float4 *s_box = s_soft;
  float *s_cls = reinterpret_cast<float *>(s_soft + count);
  const int tid = static_cast<int>(threadIdx.x);
  const size_t img = blockIdx.x;
  const float *scores = a.scores + img * count;
  const float *boxes = a.boxes + img * count * 4;
  const float *classes = a.classes + img * count;
  const int ndet = a.ndet;
  const float thr = a.thresh, sigma = a.sigma, min_score = a.min_score;

  float4 box[kSoftSlots];
  float cls[kSoftSlots], w[kSoftSlots];
#pragma unroll
  for (int k = 0; k < kSoftSlots; ++k) {
    const uint32_t p = static_cast<uint32_t>(tid) + static_cast<uint32_t>(k) * kSoftThreads;
    box[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    cls[k] = 0.0f;
    w[k] = 0.0f;
    if (p < count) {
      const float s = scores[p];
      box[k] = make_float4(boxes[p * 4], boxes[p * 4 + 1], boxes[p * 4 + 2], boxes[p * 4 + 3]);   // (no alignment is promised)
      cls[k] = classes[p];
      w[k] = s > 0.0f ? s : 0.0f;                              // scores <= 0 and NaN are padding
      s_box[p] = box[k];
      s_cls[p] = cls[k];
    }
  }

  int emitted = 0;
  for (; emitted < ndet; ++emitted) {
    // ---- pick: the largest (w, lowest position) among the alive ----
    uint64_t best = 0;
#pragma unroll
    for (int k = 0; k < kSoftSlots; ++k) {
      const uint32_t p = static_cast<uint32_t>(tid) + static_cast<uint32_t>(k) * kSoftThreads;
      const uint64_t key = (static_cast<uint64_t>(__float_as_uint(w[k])) << 32) | static_cast<uint32_t>(~p);
      if (w[k] > 0.0f && key > best) best = key;
    }
    best = wave_max_u64(best);
    uint64_t *part = s_part[emitted & 1];
    if (lane_id() == 0) part[tid >> 6] = best;
    __syncthreads();                                            // (round 0: also publishes s_box / s_cls)
    uint64_t win = 0;
#pragma unroll
    for (int i = 0; i < kSoftWaves; ++i) {
      const uint64_t v = part[i];
      win = v > win ? v : win;
    }
    win = uniform_u64(win);
    if (win == 0) break;                                        // nobody alive (the same in every thread)
    const uint32_t pos = ~static_cast<uint32_t>(win);
    const float4 mb = s_box[pos];
    const float mc = s_cls[pos];
    // ---- emit and retire: the owner holds the working score ----
    if (static_cast<uint32_t>(tid) == (pos & (kSoftThreads - 1))) {
      const size_t o = img * ndet + emitted;
      a.out_scores[o] = __uint_as_float(static_cast<uint32_t>(win >> 32));
      a.out_boxes[o * 4] = mb.x; a.out_boxes[o * 4 + 1] = mb.y; a.out_boxes[o * 4 + 2] = mb.z; a.out_boxes[o * 4 + 3] = mb.w;
      a.out_classes[o] = mc;
      if (a.out_indices) a.out_indices[o] = static_cast<int32_t>(pos);
#pragma unroll
      for (int k = 0; k < kSoftSlots; ++k)
        if (static_cast<uint32_t>(k) == pos / kSoftThreads) w[k] = 0.0f;
    }
    // ---- decay the alive candidates of the pick's class ----
    const float marea = (mb.z - mb.x + 1.0f) * (mb.w - mb.y + 1.0f);
#pragma unroll
    for (int k = 0; k < kSoftSlots; ++k)
      if (w[k] > 0.0f && cls[k] == mc) w[k] = soft_decay<kGaussian>(mb, marea, box[k], w[k], thr, sigma, min_score);
  }

  // ---- the zero-padded tail (box.py:322-324) ----
  for (int t = emitted + tid; t < ndet; t += kSoftThreads) {
    const size_t o = img * ndet + t;
    a.out_scores[o] = 0.0f;
    a.out_classes[o] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.out_boxes[o * 4 + k] = 0.0f;
    if (a.out_indices) a.out_indices[o] = -1;
  }
}

}  // namespace odtk
