// tal.hpp -- task-aligned target assignment (TOOD, Feng et al., ICCV 2021; the assigner of PP-YOLOE and YOLOv8) for every pyramid
// level of the whole batch: the third assigner next to the fixed-IoU rule of targets.hpp and ATSS (atss.hpp), with the same outputs
// (depth, box_target, optional one-hot class map in the [A, *, H, W] layout the loss consumes).  Unlike those two it looks at what
// the network predicts: the positives of a box are the anchors with the largest t = s^alpha * u^beta, s the class score the
// network gives the box's class at the anchor, u the IoU of the box it predicts there with the ground truth.  Axis-aligned boxes only.
//
// The definition (every step ONE float32 operation in the written order, no contraction -- the library is built with
// -ffp-contract=off; tests/tal_ref.py restates it in numpy and is held to the kernels bit for bit):
//   inputs   per image the target rows (x, y, w, h, class); per level the class logits [B, A * C, H, W] and box deltas
//            [B, A * 4, H, W] in the head dtype (fp32 / bf16 / fp16, NCHW or channels_last), widened to float32 exactly; the level's
//            base anchors and stride.  topk in 1..ODTK_ATSS_MAX_TOPK, integer exponents alpha in 0..4 and beta in 1..8.
//   1. a row is valid when its class is a whole number in 0..C-1; every other row is padding (class < 0 as everywhere else, and
//      class >= C, which could not index a logit).  Its box: x1 = x, x2 = x + w - 1 (atss_box).
//   2. candidates of a row: every anchor (level l, slot a, cell y, x) whose cell centre xc * stride + 0.5 * stride + 0.5
//      (atss_cell_centre) lies more than 0.01 inside the box on all four sides -- ATSS's step 3 test; a NaN fails it.
//   3. s = 1.0f / (1.0f + exp_cr(-logit)), the logit of channel a * C + class.
//   4. the predicted box, operation for operation what select_decode.hpp and box.py:delta2box compute, without the clamp to the
//      image: w = ax2 - ax1 + 1, cx = ax1 + 0.5 * w, pcx = d0 * w + cx, pw = exp_cr(d2) * w,
//      P = (pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1).
//   5. u = atss_iou(P, box): the +1 pixel convention and the NaN rules of tmin_nan / tmax_nan.
//   6. m = 1.0f; alpha times m = m * s; then beta times m = m * u, left to right.  A NaN m is never chosen; m == 0 IS eligible (a
//      cold start gets its positives that way).  m is >= 0 or NaN; a negative zero (an empty intersection over a union that
//      rounding made negative) counts as zero.
//   7. the row selects its min(topk, number of non-NaN candidates) candidates with the largest m over ALL levels together; ties go
//      to the lower global anchor index g = level_base[l] + (a * H + y) * W + x (the memory order of depth, levels in call order).
//   8. an anchor selected by several rows goes to the row with the largest float32 u, ties to the earliest row.
//   9. depth = class + 1 / 0 (there is no ignore band), box_target = box2delta(box, anchor) in the operation order of
//      atss_assign_kernel / 0, cls_target = one-hot / 0; every element of every output is written.
//
// Three launches, no atomics, the same bits on every run:
//   tal_select_kernel   one workgroup per (image, target row).  Per level the rectangle of cells whose centres lie inside the box
//                       is found by bisection on the centre test itself (the test is monotone in the cell index, so the
//                       rectangle is exact, not a guess); only that rectangle, times A, is walked.  Every lane forms the packed key
//                       (bits of m) << 32 | ~g -- m >= 0, so its bit pattern orders like its value, and ~g below it breaks ties
//                       as step 7 wants.  The candidates are streamed ONCE: keys above the running k-th best are appended to an LDS
//                       staging buffer (ballot + a prefix over the waves' counts, no LDS atomics); when the next trip might not
//                       fit, the buffer is reduced to its best topk -- topk rounds of the DPP wave maximum and a cross-wave step --
//                       and the k-th best becomes the threshold.  The same reduction finishes.  Record per row: the selected g,
//                       their u (evaluated again by the same inline function, so the same bits) and the count.
//   tal_fill_kernel     zeros to depth, box_target and (where wanted) cls_target of all levels: 16-byte stores, a segment table.
//   tal_scatter_kernel  one thread per (image, row, selected entry): it compares its g with the entries of the image's other rows
//                       (staged through LDS kTalRound rows at a time) and writes the anchor's outputs only if it wins by step 8.
// Measured: tools/tal_probe.py.
#pragma once

#include "common.hpp"
#include "prefilter.hpp"   // element types F32 / BF16 / F16, load_raw
#include "atss.hpp"        // atss_box, atss_iou, atss_cell_centre
#include "../../include/odtk_hip.h"

namespace odtk {

constexpr int kTalThreads = 512;                      // tal_select_kernel
constexpr int kTalWaves = kTalThreads / kWave;
constexpr int kTalStage = 4096;                       // keys the staging buffer holds (32 KiB of LDS)
constexpr int kTalFillThreads = 256;
constexpr int kTalFillSegments = 3 * ODTK_MAX_LEVELS;
constexpr int kTalScatterThreads = 256;
constexpr int kTalRound = 128;                        // target rows whose records the scatter stages in LDS at a time
static_assert(kTalStage >= 2 * kTalThreads && ODTK_ATSS_MAX_TOPK == 16, "a trip must fit behind a reduced buffer; the scatter splits idx by 16");

// workspace: one record per (image, target row), [B][n_max]; every record is written by every call (padding rows: cnt = 0)
struct alignas(16) TalRecord {
  uint32_t g[ODTK_ATSS_MAX_TOPK];       // the selected global anchor indices, best first
  float u[ODTK_ATSS_MAX_TOPK];          // their IoU of the predicted box with the row's box
  int32_t cnt, pad_[3];
};
static_assert(sizeof(TalRecord) == 144, "the workspace query counts 144 bytes per target row");

struct TalLevel {
  const void *cls, *box;  // [B, A * C, H, W], [B, A * 4, H, W] in the head dtype
  float *cls_target;      // [B, A, C, H, W] or null
  float *box_target;      // [B, A, 4, H, W]
  float *depth;           // [B, A, 1, H, W]
  int height, width;
  float stride;
  int channels_last;
  uint32_t base, pad_;    // g of the level's first anchor
  float anchors[ODTK_MAX_ANCHORS * 4];
};

struct TalArgs {
  TalLevel lv[ODTK_MAX_LEVELS];
  const float *targets;   // [B, n_max, 5] = (x, y, w, h, class)
  TalRecord *records;     // [B, n_max]
  int n_levels, n_max, num_anchors, num_classes, topk, alpha, beta;
};
static_assert(sizeof(TalArgs) <= 4096, "kernel arguments travel by value");

struct TalFillArgs {
  float *ptr[kTalFillSegments];
  unsigned long long count[kTalFillSegments];     // floats
  uint32_t block_begin[kTalFillSegments + 1];
  int n_segments;
};

// step 1: the class of a valid row, or -1
__device__ __forceinline__ int tal_class(float c, int num_classes) {
  if (!(c >= 0.0f && c < 2147483648.0f) || c != floorf(c)) return -1;
  const int k = static_cast<int>(c);
  return k < num_classes ? k : -1;
}

// Step 2 along one axis.  The centre grows with the cell index and rounding is monotone, so `centre - lo > 0.01` turns from false
// to true once and `hi - centre > 0.01` from true to false once: both ends by bisection on the test itself.  NaN: an empty range.
__device__ __forceinline__ int tal_first_inside(float lo, float stride, int cells) {
  int a = 0, b = cells;                                       // the test fails below a and holds from b on
  while (a < b) {
    const int mid = a + ((b - a) >> 1);
    if (atss_cell_centre(mid, stride) - lo > 0.01f) b = mid; else a = mid + 1;
  }
  return a;
}
__device__ __forceinline__ int tal_end_inside(float hi, float stride, int cells) {
  int a = 0, b = cells;                                       // the test holds below a and fails from b on
  while (a < b) {
    const int mid = a + ((b - a) >> 1);
    if (hi - atss_cell_centre(mid, stride) > 0.01f) a = mid + 1; else b = mid;
  }
  return a;
}

// steps 3 to 6 for one anchor of image b: the metric m and the overlap u
template <typename T>
__device__ __forceinline__ void tal_eval(const TalLevel &lv, int b, int num_anchors, int num_classes, int an, int y, int x, int cls,
                                         const float *q, int alpha, int beta, float *m_out, float *u_out) {
  const uint64_t hw = static_cast<uint64_t>(lv.height) * static_cast<uint64_t>(lv.width);
  const uint64_t pix = static_cast<uint64_t>(y) * static_cast<uint64_t>(lv.width) + static_cast<uint64_t>(x);
  const uint64_t cch = static_cast<uint64_t>(num_anchors) * static_cast<uint64_t>(num_classes), bch = static_cast<uint64_t>(num_anchors) * 4u;
  const uint64_t c = static_cast<uint64_t>(an) * static_cast<uint64_t>(num_classes) + static_cast<uint64_t>(cls);
  const uint64_t cls_off = static_cast<uint64_t>(b) * cch * hw + (lv.channels_last ? pix * cch + c : c * hw + pix);
  const float logit = load_raw<T>(lv.cls, cls_off);
  float d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint64_t ch = static_cast<uint64_t>(an) * 4u + static_cast<uint64_t>(k);
    d[k] = load_raw<T>(lv.box, static_cast<uint64_t>(b) * bch * hw + (lv.channels_last ? pix * bch + ch : ch * hw + pix));
  }
  const float s = 1.0f / (1.0f + exp_cr(-logit));
  // select_decode.hpp: grid = [x, y, x, y] * stride + anchors[a], then box.py:100-103 and :108-111 without the clamp
  const float *anc = lv.anchors + 4 * an;
  const float fx = static_cast<float>(x) * lv.stride, fy = static_cast<float>(y) * lv.stride;
  const float ax1 = fx + anc[0], ay1 = fy + anc[1], ax2 = fx + anc[2], ay2 = fy + anc[3];
  const float w = ax2 - ax1 + 1.0f, h = ay2 - ay1 + 1.0f;
  const float cx = ax1 + 0.5f * w, cy = ay1 + 0.5f * h;
  const float pcx = d[0] * w + cx, pcy = d[1] * h + cy;
  const float pw = exp_cr(d[2]) * w, ph = exp_cr(d[3]) * h;
  const float u = atss_iou(pcx - 0.5f * pw, pcy - 0.5f * ph, pcx + 0.5f * pw - 1.0f, pcy + 0.5f * ph - 1.0f, q);
  float m = 1.0f;
  for (int i = 0; i < alpha; ++i) m = m * s;
  for (int i = 0; i < beta; ++i) m = m * u;
  *m_out = m;
  *u_out = u;
}

// g -> its level
__device__ __forceinline__ int tal_level_of(const TalArgs &a, uint32_t g) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < ODTK_MAX_LEVELS; ++i)
    if (i < a.n_levels && g >= a.lv[i].base) l = i;
  return l;
}

template <typename T>
__global__ __launch_bounds__(kTalThreads) void tal_select_kernel(const TalArgs a) {
  __shared__ uint64_t s_buf[kTalStage];                       // staged keys, in no particular order (keys are unique: g is in them)
  __shared__ uint64_t s_top[ODTK_ATSS_MAX_TOPK];              // the buffer's best keys, descending
  __shared__ uint64_t s_wmax[2 * kTalWaves];                  // (two of each: a round writes while stragglers still read the last)
  __shared__ uint32_t s_wcnt[2 * kTalWaves];

  const int row = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const size_t at = static_cast<size_t>(b) * a.n_max + row;
  const float *tg = a.targets + at * 5;
  TalRecord *rec = a.records + at;
  const int cls = tal_class(tg[4], a.num_classes);
  if (cls < 0) {                                              // padding (uniform over the workgroup)
    if (tid == 0) rec->cnt = 0;
    return;
  }
  float q[5];
  atss_box(tg, q);

  uint32_t n = 0;                                             // keys in s_buf; the same in every thread
  uint64_t thr = 0;                                           // keys have to exceed it (a real key is never 0: g < 2^31)
  int kept = 0;                                               // keys in s_top after reduce()

  // s_buf[0, n) -> its best min(topk, n) keys in s_top and at the front of s_buf; a full set raises the threshold
  auto reduce = [&]() {
    __syncthreads();
    uint64_t last = ~0ull;
    int cnt = 0;
    for (int k = 0; k < a.topk; ++k) {
      uint64_t best = 0;
      for (uint32_t j = tid; j < n; j += kTalThreads) {
        const uint64_t v = s_buf[j];
        if (v < last && v > best) best = v;
      }
      best = wave_max_u64(best);
      uint64_t *slot = s_wmax + (k & 1) * kTalWaves;
      if (lane == 0) slot[wave] = best;
      __syncthreads();
      best = 0;
#pragma unroll
      for (int w = 0; w < kTalWaves; ++w) best = slot[w] > best ? slot[w] : best;
      if (best == 0) break;                                   // fewer keys than topk (uniform)
      if (tid == 0) s_top[k] = best;
      last = best;
      ++cnt;
    }
    __syncthreads();
    if (tid < cnt) s_buf[tid] = s_top[tid];
    n = static_cast<uint32_t>(cnt);
    kept = cnt;
    if (cnt == a.topk) thr = last;
    __syncthreads();
  };

  uint32_t trip = 0;
  for (int l = 0; l < a.n_levels; ++l) {
    const TalLevel &lv = a.lv[l];
    const int x0 = tal_first_inside(q[0], lv.stride, lv.width), x1 = tal_end_inside(q[2], lv.stride, lv.width);
    const int y0 = tal_first_inside(q[1], lv.stride, lv.height), y1 = tal_end_inside(q[3], lv.stride, lv.height);
    if (x0 >= x1 || y0 >= y1) continue;                       // (uniform)
    const uint32_t nx = static_cast<uint32_t>(x1 - x0), cells = nx * static_cast<uint32_t>(y1 - y0);
    const uint32_t total = cells * static_cast<uint32_t>(a.num_anchors);          // <= the level's anchors < 2^31
    for (uint32_t first = 0; first < total; first += kTalThreads, ++trip) {
      if (n + kTalThreads > kTalStage) reduce();              // (uniform)
      const uint32_t i = first + static_cast<uint32_t>(tid);
      uint64_t key = 0;
      if (i < total) {
        const uint32_t an = i / cells, r = i - an * cells;
        const uint32_t yy = r / nx, xx = r - yy * nx;
        const int y = y0 + static_cast<int>(yy), x = x0 + static_cast<int>(xx);
        float m, u;
        tal_eval<T>(lv, b, a.num_anchors, a.num_classes, static_cast<int>(an), y, x, cls, q, a.alpha, a.beta, &m, &u);
        if (m == m) {
          m = m + 0.0f;                                       // -0.0 -> +0.0
          const uint32_t g = lv.base + (an * static_cast<uint32_t>(lv.height) + static_cast<uint32_t>(y)) * static_cast<uint32_t>(lv.width) +
                             static_cast<uint32_t>(x);
          key = (static_cast<uint64_t>(__float_as_uint(m)) << 32) | static_cast<uint32_t>(~g);
        }
      }
      const bool keep = key > thr;
      const uint64_t mask = __ballot(keep);
      uint32_t *slot = s_wcnt + (trip & 1u) * kTalWaves;
      if (lane == 0) slot[wave] = static_cast<uint32_t>(__popcll(mask));
      __syncthreads();
      uint32_t before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < kTalWaves; ++w) {
        const uint32_t c = slot[w];
        all += c;
        before += w < wave ? c : 0u;
      }
      if (keep) s_buf[n + before + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)))] = key;
      n += all;
    }
  }
  reduce();
  if (tid < kept) {
    const uint32_t g = ~static_cast<uint32_t>(s_top[tid]);
    const int l = tal_level_of(a, g);
    const TalLevel &lv = a.lv[l];
    const uint32_t local = g - lv.base, hw = static_cast<uint32_t>(lv.height) * static_cast<uint32_t>(lv.width);
    const uint32_t an = local / hw, pix = local - an * hw;
    const uint32_t y = pix / static_cast<uint32_t>(lv.width), x = pix - y * static_cast<uint32_t>(lv.width);
    float m, u;
    tal_eval<T>(lv, b, a.num_anchors, a.num_classes, static_cast<int>(an), static_cast<int>(y), static_cast<int>(x), cls, q, a.alpha, a.beta, &m, &u);
    rec->g[tid] = g;
    rec->u[tid] = u;
  }
  if (tid == 0) rec->cnt = kept;
}

__global__ __launch_bounds__(kTalFillThreads) void tal_fill_kernel(const TalFillArgs a) {
  const int s = level_of<kTalFillSegments>(a.block_begin, a.n_segments);
  float *p = a.ptr[s];
  const unsigned long long n = a.count[s];
  const uint32_t blk = blockIdx.x - a.block_begin[s], blocks = a.block_begin[s + 1] - a.block_begin[s];
  // floats in front of the first 16-byte boundary, whole vectors, floats behind the last
  unsigned long long head = ((16u - (reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2;
  head = head < n ? head : n;
  const unsigned long long vectors = (n - head) >> 2, tail = n - head - 4 * vectors;
  float4 *v = reinterpret_cast<float4 *>(p + head);
  for (unsigned long long i = static_cast<unsigned long long>(blk) * kTalFillThreads + threadIdx.x; i < vectors;
       i += static_cast<unsigned long long>(blocks) * kTalFillThreads)
    v[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (blk == 0) {
    if (threadIdx.x < head) p[threadIdx.x] = 0.0f;
    if (threadIdx.x < tail) p[head + 4 * vectors + threadIdx.x] = 0.0f;
  }
}

__global__ __launch_bounds__(kTalScatterThreads) void tal_scatter_kernel(const TalArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_g[kTalRound * ODTK_ATSS_MAX_TOPK];   // entries of a round's rows; ~0: none
  __shared__ float s_u[kTalRound * ODTK_ATSS_MAX_TOPK];

  const int b = blockIdx.y, tid = threadIdx.x;
  const TalRecord *recs = a.records + static_cast<size_t>(b) * a.n_max;
  const unsigned long long idx = static_cast<unsigned long long>(blockIdx.x) * kTalScatterThreads + tid;
  const unsigned long long row64 = idx >> 4;
  const int k = static_cast<int>(idx & 15u);
  const int row = row64 < static_cast<unsigned long long>(a.n_max) ? static_cast<int>(row64) : -1;
  bool mine = false;
  uint32_t g = ~0u;
  float u = 0.0f;
  if (row >= 0 && k < recs[row].cnt) {
    mine = true;
    g = recs[row].g[k];
    u = recs[row].u[k];
  }
  bool lost = false;
  for (int base = 0; base < a.n_max; base += kTalRound) {
    const int rows = a.n_max - base < kTalRound ? a.n_max - base : kTalRound;
    __syncthreads();
    for (int i = tid; i < kTalRound * ODTK_ATSS_MAX_TOPK; i += kTalScatterThreads) {
      const int r = i >> 4, j = i & 15;
      const bool live = r < rows && j < recs[base + r].cnt;
      s_g[i] = live ? recs[base + r].g[j] : ~0u;
      s_u[i] = live ? recs[base + r].u[j] : 0.0f;
    }
    __syncthreads();
    if (!mine) continue;
    for (int i = 0; i < rows * (ODTK_ATSS_MAX_TOPK / 4); ++i) {
      const uint4 v = reinterpret_cast<const uint4 *>(s_g)[i];                            // the same address in every lane
      if ((v.x != g) & (v.y != g) & (v.z != g) & (v.w != g)) continue;
      const int other = base + (i >> 2);
      if (other == row) continue;
      const int j = 4 * i + (v.x == g ? 0 : v.y == g ? 1 : v.z == g ? 2 : 3);          // (a row holds a g once)
      const float ou = s_u[j];
      if (ou > u || (ou == u && other < row)) lost = true;                               // step 8
    }
  }
  if (!mine || lost) return;

  const int l = tal_level_of(a, g);
  const TalLevel &lv = a.lv[l];
  const uint32_t local = g - lv.base, hw = static_cast<uint32_t>(lv.height) * static_cast<uint32_t>(lv.width);
  const uint32_t an = local / hw, pix = local - an * hw;
  const uint32_t y = pix / static_cast<uint32_t>(lv.width), x = pix - y * static_cast<uint32_t>(lv.width);
  const float *tg = a.targets + (static_cast<size_t>(b) * a.n_max + row) * 5;
  float q[5];
  atss_box(tg, q);
  const float gx = static_cast<float>(x) * lv.stride, gy = static_cast<float>(y) * lv.stride;
  const float ax1 = gx + lv.anchors[an * 4 + 0], ay1 = gy + lv.anchors[an * 4 + 1];
  const float ax2 = gx + lv.anchors[an * 4 + 2], ay2 = gy + lv.anchors[an * 4 + 3];
  // box2delta, in the operation order of atss_assign_kernel (targets.hpp:106-113)
  const float aw = ax2 - ax1 + 1.0f, ah = ay2 - ay1 + 1.0f;
  const float acx = ax1 + 0.5f * aw, acy = ay1 + 0.5f * ah;
  const float bw = q[2] - q[0] + 1.0f, bh = q[3] - q[1] + 1.0f;
  const float bcx = q[0] + 0.5f * bw, bcy = q[1] + 0.5f * bh;
  const size_t cell = static_cast<size_t>(b) * a.num_anchors + an;
  float *box = lv.box_target + cell * 4 * hw + pix;
  box[0] = (bcx - acx) / aw;
  box[static_cast<size_t>(hw)] = (bcy - acy) / ah;
  box[2 * static_cast<size_t>(hw)] = logf(bw / aw);
  box[3 * static_cast<size_t>(hw)] = logf(bh / ah);
  lv.depth[cell * hw + pix] = tg[4] + 1.0f;
  if (lv.cls_target) lv.cls_target[(cell * a.num_classes + static_cast<size_t>(tg[4])) * hw + pix] = 1.0f;
}

}  // namespace odtk
