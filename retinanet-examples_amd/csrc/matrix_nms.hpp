// matrix_nms.hpp -- batched class-aware Matrix NMS (Wang et al., SOLOv2, 2020; linear and Gaussian) on axis-aligned boxes:
// every candidate's score is multiplied by ONE factor that comes from pairwise IoUs alone, so there is no serial chain of
// picks as in soft_nms.hpp, the whole chip works on one image and the candidate list has no 7680 cap.
//
// No reference equivalent.  Definition, all in float32 (the library is built with -ffp-contract=off):
//   participants : the candidates with score > 0 (NaN is not), ranked by score descending, ties by lowest input position
//                  (the key `score bits << 32 | ~position`); only the first n = min(pre_top, #positive) take part.
//   iou(a, b)    : soft_nms.hpp's soft_decay, operation for operation: +1 pixel, tmax_nan / tmin_nan / clamp(0),
//                  inter / ((area_a + area_b) - inter).  Bitwise symmetric.
//   cmax_i       : max(+0, iou(k, i)) over the participants k of i's class ranked before i, as `acc = iou > acc ? iou : acc`
//                  from acc = 0: a NaN IoU is skipped whatever the order.
//   decay_j      : min(1, d(i, j)) over the participants i of j's class ranked before j, as `acc = d < acc ? d : acc` from
//                  acc = 1: a NaN or +inf d (a division by 1 - cmax_i = 0) decides nothing.
//                    linear   : d = (1 - iou(i, j)) / (1 - cmax_i)
//                    gaussian : d = exp_cr(((cmax_i * cmax_i) - (iou * iou)) / sigma)
//                  The first participant of a class has decay 1.  mmdetection's mask_matrix_nms takes the column minimum of
//                  the whole decay matrix instead; its row 0 (the best candidate, cmax = 0) holds 1 - iou <= 1 or
//                  exp(-iou^2 / sigma) <= 1, so that minimum never exceeds 1 and the two agree.
//   output       : s'_j = score_j * decay_j; j is alive iff s'_j >= min_score; the alive participants in order of s'
//                  descending, ties by lowest input position, at most ndet of them: (s', box, class, position).  The
//                  remaining slots are zero (position -1), as odtk_nms pads.
//
// Shape.  Four launches, nothing but the workspace between them:
//   matrix_nms_rank_kernel     one 1024-thread workgroup per image: positive scores -> keys in the workspace, the radix
//                              descent of select_decode.hpp where more than 4096 are positive, sort_keys_desc, then the n best
//                              in rank order: box, class, score, position; cmax = 0 and decay = 1 for the reductions below.
//   matrix_nms_pairs_kernel<0> one 256-thread workgroup per (image, 64 columns x 256 rows of row < column pairs): lane =
//                              column, a wave walks 64 rows out of LDS (broadcast reads), class test before the IoU; the four
//                              waves' partial maxima meet in LDS, one vector atomic max per column on the IoU's bit pattern
//                              (cmax >= +0: the bits of a non-negative float order like the float).
//   matrix_nms_pairs_kernel<1|2>  the same grid with the IoU recomputed: d from the rows' final cmax, partial minima, one
//                              vector atomic min per column on an order-preserving key of d.
//   matrix_nms_emit_kernel     one workgroup per image: s', the alive keys (s' bits << 32 | ~position), sort_keys_desc, outputs.
// max and min over integers do not depend on the order of the atomics: the same bits on every run.  The one value the float
// comparison and the integer key order differently is -0 against +0; a decay of either zero gives s' = +-0 < min_score, which is
// never emitted.
#pragma once

#include "common.hpp"
#include "select_decode.hpp"   // radix_threshold, sort_keys_desc
#include "../../include/odtk_hip.h"

namespace odtk {

constexpr int kMatThreads = 1024;              // rank and emit kernels (= kSelThreads: the selection and the sort are written for it)
constexpr int kMatPairThreads = 256;
constexpr uint32_t kMatCols = 64;              // columns of a pair tile: one wave-width
constexpr uint32_t kMatRows = 256;             // rows of a pair tile: 64 per wave
static_assert(kMatThreads == kSelThreads, "select_decode.hpp's selection runs with 1024 threads");
static_assert(ODTK_MAX_MATRIX_NMS_PRE <= kSortCap, "the participants are sorted by the 4096-key network");

struct MatrixNmsArgs {
  const float *scores;     // [batch, count]
  const float *boxes;      // [batch, count, 4]
  const float *classes;    // [batch, count]
  float *out_scores;       // [batch, ndet]
  float *out_boxes;        // [batch, ndet, 4]
  float *out_classes;      // [batch, ndet]
  int32_t *out_indices;    // optional [batch, ndet]
  // workspace; `stride` = pre_top rounded up to the tile's columns
  unsigned long long *keys;   // [batch, count]   positive candidates' keys (rank kernel only)
  float *r_box;            // [batch, stride, 4]  the participants in rank order
  float *r_cls;            // [batch, stride]
  float *r_score;          // [batch, stride]
  uint32_t *r_pos;         // [batch, stride]
  uint32_t *r_cmax;        // [batch, stride]     bit pattern of cmax
  uint32_t *r_decay;       // [batch, stride]     order-preserving key of decay
  uint32_t *r_n;           // [batch]
  uint32_t count;
  uint32_t stride;
  uint32_t pre_top;
  int ndet;
  float sigma;
  float min_score;
};

// float <-> unsigned, order-preserving over every non-NaN value (-0 below +0)
__device__ __forceinline__ uint32_t mat_order_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float mat_order_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// soft_decay's IoU (soft_nms.hpp), operation for operation
__device__ __forceinline__ float mat_iou(const float4 m, const float4 j) {
  const float x1 = tmax_nan(j.x, m.x), y1 = tmax_nan(j.y, m.y);
  const float x2 = tmin_nan(j.z, m.z), y2 = tmin_nan(j.w, m.w);
  float iw = x2 - x1 + 1.0f, ih = y2 - y1 + 1.0f;
  iw = iw < 0.0f ? 0.0f : iw;  // clamp(0)
  ih = ih < 0.0f ? 0.0f : ih;
  const float inter = iw * ih;
  const float jarea = (j.z - j.x + 1.0f) * (j.w - j.y + 1.0f);
  const float marea = (m.z - m.x + 1.0f) * (m.w - m.y + 1.0f);
  const float both = jarea + marea;
  return inter / (both - inter);
}

struct MatKeySource {    // the positive candidates' keys of this image, written by this workgroup
  const unsigned long long *keys;
  uint32_t count;
  template <typename F>
  __device__ __forceinline__ void for_each(F &&f) const {
    for (uint32_t i = threadIdx.x; i < count; i += kMatThreads) f(keys[i]);
  }
};

__global__ __launch_bounds__(kMatThreads) void matrix_nms_rank_kernel(const MatrixNmsArgs a) {
  __shared__ uint64_t s_sort[kSortCap];
  __shared__ uint32_t s_hist[kRadixBins];
  __shared__ uint32_t s_misc[32];
  const uint32_t tid = threadIdx.x;
  const size_t img = blockIdx.x;
  const uint32_t count = a.count;
  const float *in_s = a.scores + img * count;
  unsigned long long *keys = a.keys + img * count;
  if (tid == 0) { s_misc[24] = 0; s_misc[25] = 0; }
  __syncthreads();
  // ---- the positive candidates' keys (score bits << 32 | ~position), one append per wave ----
  for (uint32_t i0 = 0; i0 < count; i0 += kMatThreads) {     // (block-uniform trip count)
    const uint32_t i = i0 + tid;
    const float sc = i < count ? in_s[i] : 0.0f;
    const bool pos = sc > 0.0f;                               // NaN fails
    const uint32_t slot = wave_append_slot(&s_misc[24], pos);
    if (pos) keys[slot] = (static_cast<uint64_t>(__float_as_uint(sc)) << 32) | static_cast<uint32_t>(~i);
  }
  __threadfence_block();
  __syncthreads();
  const uint32_t list_n = __builtin_amdgcn_readfirstlane(s_misc[24]);
  const uint32_t n = list_n < a.pre_top ? list_n : a.pre_top;
  // ---- the keys to sort: all of them, or the ones at or above the radix descent's threshold (n <= taken <= 4096) ----
  uint32_t taken = list_n;
  if (list_n <= static_cast<uint32_t>(kSortCap)) {
    for (uint32_t i = tid; i < list_n; i += kMatThreads) s_sort[i] = keys[i];
  } else {
    const MatKeySource src{keys, list_n};
    const uint64_t thr = radix_threshold(src, n, kSortCap, s_hist, s_misc, &taken);
    for (uint32_t i0 = 0; i0 < list_n; i0 += kMatThreads) {
      const uint32_t i = i0 + tid;
      const uint64_t k = i < list_n ? keys[i] : 0ull;
      const bool in = k >= thr && i < list_n;
      const uint32_t slot = wave_append_slot(&s_misc[25], in);
      if (in && slot < static_cast<uint32_t>(kSortCap)) s_sort[slot] = k;
    }
    taken = taken < static_cast<uint32_t>(kSortCap) ? taken : static_cast<uint32_t>(kSortCap);
  }
  __syncthreads();
  sort_keys_desc<kSortCap>(s_sort, taken);
  // ---- the n best in rank order ----
  const size_t base = img * a.stride;
  const float *in_b = a.boxes + img * count * 4;
  const float *in_c = a.classes + img * count;
  for (uint32_t r = tid; r < n; r += kMatThreads) {
    const uint64_t k = s_sort[r];
    const uint32_t p = ~static_cast<uint32_t>(k);
    reinterpret_cast<float4 *>(a.r_box)[base + r] = make_float4(in_b[p * 4], in_b[p * 4 + 1], in_b[p * 4 + 2], in_b[p * 4 + 3]);
    a.r_cls[base + r] = in_c[p];
    a.r_score[base + r] = __uint_as_float(static_cast<uint32_t>(k >> 32));
    a.r_pos[base + r] = p;
    a.r_cmax[base + r] = 0u;                                  // +0
    a.r_decay[base + r] = mat_order_key(1.0f);
  }
  if (tid == 0) a.r_n[img] = n;
}

// kPhase 0: cmax; 1: linear decay; 2: Gaussian decay.  grid = (batch, stride / 64 column blocks * row chunks)
template <int kPhase>
__global__ __launch_bounds__(kMatPairThreads) void matrix_nms_pairs_kernel(const MatrixNmsArgs a) {
  __shared__ float4 s_rbox[kMatRows];
  __shared__ float s_rcls[kMatRows];
  __shared__ float s_rcmax[kMatRows];
  __shared__ float s_part[kMatPairThreads / kWave][kMatCols];
  const uint32_t ncol = a.stride / kMatCols;
  const uint32_t bj = blockIdx.y % ncol, rc = blockIdx.y / ncol;
  const size_t img = blockIdx.x;
  const uint32_t n = a.r_n[img];
  const uint32_t row0 = rc * kMatRows, col0 = bj * kMatCols;
  if (col0 >= n || row0 + 1 >= col0 + kMatCols) return;      // no column | no pair with row < column (block-uniform)
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const size_t base = img * a.stride;
  {
    const uint32_t k = row0 + tid;                             // rows >= n: a NaN class equals nothing
    const bool in = k < n;
    s_rbox[tid] = in ? reinterpret_cast<const float4 *>(a.r_box)[base + k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s_rcls[tid] = in ? a.r_cls[base + k] : __builtin_nanf("");
    if constexpr (kPhase != 0) s_rcmax[tid] = in ? __uint_as_float(a.r_cmax[base + k]) : 0.0f;
  }
  const uint32_t j = col0 + lane;
  const bool jin = j < n;
  const float4 jb = jin ? reinterpret_cast<const float4 *>(a.r_box)[base + j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float jc = jin ? a.r_cls[base + j] : __builtin_nanf("");
  __syncthreads();
  float acc = kPhase == 0 ? 0.0f : 1.0f;
  const float sigma = a.sigma;
  const uint32_t w0 = wave * kWave;                            // this wave's rows inside the chunk
  if (row0 + w0 < col0 + kMatCols - 1) {                       // (wave-uniform) some row of it lies before some column
    for (uint32_t r = 0; r < kWave; ++r) {
      const uint32_t il = w0 + r, i = row0 + il;
      if (i < j && s_rcls[il] == jc) {
        const float iou = mat_iou(s_rbox[il], jb);
        if constexpr (kPhase == 0) {
          acc = iou > acc ? iou : acc;
        } else if constexpr (kPhase == 1) {
          const float d = (1.0f - iou) / (1.0f - s_rcmax[il]);
          acc = d < acc ? d : acc;
        } else {
          const float c = s_rcmax[il];
          const float cc = c * c;
          const float ii = iou * iou;
          const float e = (cc - ii) / sigma;
          const float d = exp_cr(e);
          acc = d < acc ? d : acc;
        }
      }
    }
  }
  s_part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && jin) {
#pragma unroll
    for (int w = 1; w < kMatPairThreads / kWave; ++w) {
      const float v = s_part[w][lane];
      if constexpr (kPhase == 0) acc = v > acc ? v : acc;
      else acc = v < acc ? v : acc;
    }
    if constexpr (kPhase == 0) {
      if (acc > 0.0f) atomicMax(&a.r_cmax[base + j], __float_as_uint(acc));
    } else {
      if (acc < 1.0f) atomicMin(&a.r_decay[base + j], mat_order_key(acc));
    }
  }
}

__global__ __launch_bounds__(kMatThreads) void matrix_nms_emit_kernel(const MatrixNmsArgs a) {
  __shared__ uint64_t s_sort[kSortCap];
  __shared__ uint32_t s_alive;
  const uint32_t tid = threadIdx.x;
  const size_t img = blockIdx.x;
  const uint32_t n = a.r_n[img];
  const size_t base = img * a.stride;
  if (tid == 0) s_alive = 0;
  __syncthreads();
  for (uint32_t r0 = 0; r0 < n; r0 += kMatThreads) {          // (block-uniform trip count)
    const uint32_t r = r0 + tid;
    float s = 0.0f;
    uint32_t p = 0;
    if (r < n) {
      s = a.r_score[base + r] * mat_order_value(a.r_decay[base + r]);
      p = a.r_pos[base + r];
    }
    const bool alive = r < n && s >= a.min_score;             // (a NaN is not)
    const uint32_t slot = wave_append_slot(&s_alive, alive);
    if (alive) s_sort[slot] = (static_cast<uint64_t>(__float_as_uint(s)) << 32) | static_cast<uint32_t>(~p);
  }
  __syncthreads();
  const uint32_t n_alive = __builtin_amdgcn_readfirstlane(s_alive);
  sort_keys_desc<kSortCap>(s_sort, n_alive);
  const uint32_t ndet = static_cast<uint32_t>(a.ndet);
  const uint32_t emit = n_alive < ndet ? n_alive : ndet;
  const float *in_b = a.boxes + img * a.count * 4;
  const float *in_c = a.classes + img * a.count;
  for (uint32_t t = tid; t < ndet; t += kMatThreads) {
    const size_t o = img * ndet + t;
    float s = 0.0f, c = 0.0f;
    float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int32_t idx = -1;
    if (t < emit) {
      const uint64_t k = s_sort[t];
      const uint32_t p = ~static_cast<uint32_t>(k);
      s = __uint_as_float(static_cast<uint32_t>(k >> 32));
      b = make_float4(in_b[p * 4], in_b[p * 4 + 1], in_b[p * 4 + 2], in_b[p * 4 + 3]);   // (no alignment is promised)
      c = in_c[p];
      idx = static_cast<int32_t>(p);
    }
    a.out_scores[o] = s;
    a.out_boxes[o * 4] = b.x; a.out_boxes[o * 4 + 1] = b.y; a.out_boxes[o * 4 + 2] = b.z; a.out_boxes[o * 4 + 3] = b.w;
    a.out_classes[o] = c;
    if (a.out_indices) a.out_indices[o] = idx;
  }
}

}  // namespace odtk
