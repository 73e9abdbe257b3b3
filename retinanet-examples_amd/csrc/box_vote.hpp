// box_vote.hpp -- box voting behind a suppression (Gidaris & Komodakis 2015), and the concatenation of candidate lists that
// the horizontal-flip test-time augmentation needs.  No reference equivalent; the definitions are in include/odtk_hip.h
// (odtk_box_vote, odtk_concat_candidates).
//
// box_vote_kernel.  One wave per output slot r, four waves per workgroup, grid ceil(ndet / 4) x batch.  p = kept[r] is the
// position of the kept candidate in the suppression's INPUT list; the lanes stride over the list -- score > 0 and class == class_p
// first (two coalesced 4-byte reads), only then the four box scalars and the float32 IoU of csrc/soft_nms.hpp, operation for
// operation -- and every lane keeps five double accumulators: the sum of the voters' scores and of score x box[0..3].  A product
// of two float32 values is exact in double, so the sums are the only place where the order matters: lanes in list order, then a
// butterfly over the wave with fixed partners (xor 32, 16, .. 1; two 32-bit moves per double), which is the same order on every
// run and leaves the same sum in every lane.  Lane 0 divides once in double, rounds once to float32 and stores.  No atomics, no LDS,
// no barrier, no scratch; the work is ndet x count pairs per image.
//
// concat_candidates_kernel.  Elementwise: output position q of an image belongs to the part whose [offset, offset + count) holds
// it; scores and classes are copied, and so is the box unless the part is a mirrored pass (mirror_width > 0) and the score is > 0:
// then x1' = (float)(W - 1) - x2 and x2' = (float)(W - 1) - x1, one float32 subtraction each.
#pragma once

#include "common.hpp"
#include "../../include/odtk_hip.h"

namespace odtk {

constexpr int kVoteWaves = 4;                          // output slots per workgroup
constexpr int kVoteThreads = kVoteWaves * kWave;
constexpr int kVoteUnroll = 4;                         // strides of the wave whose reads are issued together
constexpr int kConcatThreads = 256;
constexpr int kConcatMaxParts = 8;

struct BoxVoteArgs {
  const float *scores;     // [batch, count]     the suppression's input list
  const float *boxes;      // [batch, count, 4]
  const float *classes;    // [batch, count]
  const int32_t *kept;     // [batch, ndet]      input position of each emitted detection, or -1
  float *out_boxes;        // [batch, ndet, 4]
  uint32_t count;
  int ndet;
  float thresh;
};

struct ConcatArgs {
  const float *scores[kConcatMaxParts];    // [batch, count[i]]
  const float *boxes[kConcatMaxParts];     // [batch, count[i], 4]
  const float *classes[kConcatMaxParts];   // [batch, count[i]]
  uint32_t offset[kConcatMaxParts + 1];    // prefix sums of the counts (the entries past n_parts repeat the total)
  uint32_t total;                          // candidates per image of the output
  float mirror[kConcatMaxParts];           // (float)(W - 1) of a mirrored part
  uint32_t mirrored;                       // bit i: part i is a mirrored pass
  int n_parts;
  float *out_scores, *out_boxes, *out_classes;
  uint64_t elements;                       // batch x total
};

// the sum of `v` over the wave, in every lane: a butterfly with fixed partners, so the order of the additions never changes
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    const uint64_t b = static_cast<uint64_t>(__double_as_longlong(v));
    const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(b)), d, kWave));
    const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(b >> 32)), d, kWave));
    v = v + __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(hi) << 32) | lo));
  }
  return v;
}

__global__ __launch_bounds__(kVoteThreads) void box_vote_kernel(const BoxVoteArgs a) {
  const int r = static_cast<int>(blockIdx.x) * kVoteWaves + (static_cast<int>(threadIdx.x) >> 6);
  if (r >= a.ndet) return;                                       // (whole waves leave; the kernel has no barrier)
  const int lane = lane_id();
  const uint32_t count = a.count;
  const size_t img = blockIdx.y;
  float *out = a.out_boxes + (img * a.ndet + r) * 4;
  const int32_t kp = __builtin_amdgcn_readfirstlane(a.kept[img * a.ndet + r]);
  if (kp < 0 || static_cast<uint32_t>(kp) >= count) {            // an unused slot (or a position that is none): zeros
    if (lane < 4) out[lane] = 0.0f;
    return;
  }
  const uint32_t p = static_cast<uint32_t>(kp);
  const float *scores = a.scores + img * count;
  const float *boxes = a.boxes + img * count * 4;
  const float *classes = a.classes + img * count;
  const float4 m = make_float4(boxes[p * 4], boxes[p * 4 + 1], boxes[p * 4 + 2], boxes[p * 4 + 3]);   // (no alignment is promised)
  const float mc = classes[p];
  const float marea = (m.z - m.x + 1.0f) * (m.w - m.y + 1.0f);
  const float thr = a.thresh;

  double sw = 0.0, sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;
  // four strides of the wave per trip: their score and class reads are in flight together (a wave is alone on its SIMD at the
  // default sizes, so the loop is bound by the latency of its own dependent reads, not by bandwidth)
  for (uint32_t j0 = static_cast<uint32_t>(lane); j0 < count; j0 += kVoteUnroll * kWave) {
    float s[kVoteUnroll], c[kVoteUnroll];
#pragma unroll
    for (int u = 0; u < kVoteUnroll; ++u) {
      const uint32_t j = j0 + static_cast<uint32_t>(u) * kWave;
      s[u] = j < count ? scores[j] : 0.0f;
      c[u] = j < count ? classes[j] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < kVoteUnroll; ++u) {
      const uint32_t j = j0 + static_cast<uint32_t>(u) * kWave;
      if (!(s[u] > 0.0f) || !(c[u] == mc)) continue;             // (a position past the list has score 0)
      const float4 b = make_float4(boxes[j * 4], boxes[j * 4 + 1], boxes[j * 4 + 2], boxes[j * 4 + 3]);
      bool votes = j == p;                                       // the kept candidate always votes for itself
      if (!votes) {
        // torch.max / torch.min / clamp propagate NaN; a NaN IoU is not >= anything
        const float x1 = tmax_nan(b.x, m.x), y1 = tmax_nan(b.y, m.y);
        const float x2 = tmin_nan(b.z, m.z), y2 = tmin_nan(b.w, m.w);
        float iw = x2 - x1 + 1.0f, ih = y2 - y1 + 1.0f;
        iw = iw < 0.0f ? 0.0f : iw;  // clamp(0)
        ih = ih < 0.0f ? 0.0f : ih;
        const float inter = iw * ih;
        const float jarea = (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f);
        const float iou = inter / ((jarea + marea) - inter);
        votes = iou >= thr;
      }
      if (votes) {
        const double w = static_cast<double>(s[u]);
        sw = sw + w;
        sx1 = sx1 + w * static_cast<double>(b.x);
        sy1 = sy1 + w * static_cast<double>(b.y);
        sx2 = sx2 + w * static_cast<double>(b.z);
        sy2 = sy2 + w * static_cast<double>(b.w);
      }
    }
  }
  sw = wave_sum_f64(sw);
  sx1 = wave_sum_f64(sx1);
  sy1 = wave_sum_f64(sy1);
  sx2 = wave_sum_f64(sx2);
  sy2 = wave_sum_f64(sy2);
  if (lane == 0) {
    out[0] = static_cast<float>(sx1 / sw);
    out[1] = static_cast<float>(sy1 / sw);
    out[2] = static_cast<float>(sx2 / sw);
    out[3] = static_cast<float>(sy2 / sw);
  }
}

__global__ __launch_bounds__(kConcatThreads) void concat_candidates_kernel(const ConcatArgs a) {
  const uint32_t total = a.total;
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kConcatThreads;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kConcatThreads + threadIdx.x; t < a.elements; t += step) {
    const uint64_t img = t / total;
    const uint32_t q = static_cast<uint32_t>(t - img * total);
    int part = 0;
#pragma unroll
    for (int i = 1; i < kConcatMaxParts; ++i)
      if (i < a.n_parts && q >= a.offset[i]) part = i;
    // (selected with compares, not indexed: the tables stay in the kernel's scalar arguments)
    const float *ps = a.scores[0], *pb = a.boxes[0], *pc = a.classes[0];
    uint32_t off = 0, cnt = a.offset[1];
    float mirror = a.mirror[0];
#pragma unroll
    for (int i = 1; i < kConcatMaxParts; ++i)
      if (part == i) {
        ps = a.scores[i]; pb = a.boxes[i]; pc = a.classes[i];
        off = a.offset[i]; cnt = a.offset[i + 1] - a.offset[i];
        mirror = a.mirror[i];
      }
    const uint64_t src = img * cnt + (q - off);
    const float s = ps[src];
    float x1 = pb[src * 4], x2 = pb[src * 4 + 2];
    const float y1 = pb[src * 4 + 1], y2 = pb[src * 4 + 3];
    if (((a.mirrored >> part) & 1u) && s > 0.0f) {
      const float nx1 = mirror - x2, nx2 = mirror - x1;
      x1 = nx1;
      x2 = nx2;
    }
    a.out_scores[t] = s;
    a.out_classes[t] = pc[src];
    a.out_boxes[t * 4] = x1; a.out_boxes[t * 4 + 1] = y1; a.out_boxes[t * 4 + 2] = x2; a.out_boxes[t * 4 + 3] = y2;
  }
}

}  // namespace odtk
