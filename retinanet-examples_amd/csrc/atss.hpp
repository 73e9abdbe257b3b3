// atss.hpp -- ATSS target assignment (adaptive training sample selection, Zhang et al., CVPR 2020) for every pyramid level of
// the whole batch: the alternative to the fixed-IoU rule of targets.hpp, with the same outputs (depth, box_target, optional
// one-hot class map in the [A, *, H, W] layout the loss consumes).  Axis-aligned boxes only.
//
// The definition (every step float32, one operation per step, no contraction -- the library is built with -ffp-contract=off --
// except where float64 is named):
//   box      x1 = x, x2 = x + w - 1, area = (x2 - x1 + 1) * (y2 - y1 + 1), centre bcx = x1 + 0.5 * (x2 - x1 + 1)   (targets.hpp)
//   cell     centre px = xc * stride + 0.5 * stride + 0.5, shared by the A anchors of the cell (exact in float32)
//   1. per box and level: the min(k, H * W) cells with the smallest d2 = dx * dx + dy * dy (dx = px - bcx), ties to the lower
//      yc * W + xc, NaN never chosen.  The box's candidates = all A anchors of those cells, listed (level, rank, anchor) ascending.
//   2. v_i = IoU(candidate i, box) widened to float64; mean and sample variance (n - 1; 0 for n == 1) summed left to right in
//      list order; t = mean + sqrt(var).
//   3. candidate i is positive iff v_i >= t (float64; NaN: no) and the cell centre lies more than 0.01 inside the box on all
//      four sides (NaN: no).
//   4. an anchor positive for several boxes goes to the largest float32 IoU, ties to the earliest box.
//   5. depth = class + 1 / 0 (there is no ignore band), box_target = box2delta / 0, cls_target = one-hot / 0; every element of
//      every output is written.
//
// Two launches, no atomics, every output written once:
//   atss_stats_kernel   one wave per (image, target row): per level k rounds of a wave-minimum over the packed key
//                       (bits of d2) << 32 | cell -- d2 >= 0, so its bit pattern orders like its value, and the cell index
//                       below it breaks ties as the definition wants.  The k * A IoUs of the level go to LDS in list order; one
//                       lane then does the two sequential float64 sums.  Record per row: t, and per level the candidate cells
//                       and their bounding rows and columns.
//   atss_assign_kernel  shaped like snap_to_anchors_levels_kernel: one thread per anchor, the level table in the kernel
//                       arguments, the level's records of the rows staged through LDS kAtssRound at a time.  A thread looks at a box only
//                       when the box's candidate bounding box contains its cell (nearly never), then: candidate? IoU (the same
//                       inline function as the first launch, so the same bits), steps 3 and 4.
//
// Candidates: the first launch looks at a window of 8 x 8 cells around the box centre (one cell per lane, the key computed
// once) and takes its answer only when a run-time test proves it equal to the full scan (atss_window below); otherwise -- a
// centre well outside the grid, distances that float32 no longer tells apart, a level too narrow to hold k cells in the
// window -- it scans every cell of the level, k rounds of H * W / 64 key evaluations per lane.  Levels of up to 64 cells are
// scanned in full straight away (one cell per lane as well).  Measured: tools/atss_probe.py.
#pragma once

#include "common.hpp"
#include "fastdiv.hpp"
#include "../../include/odtk_hip.h"

namespace odtk {

constexpr int kAtssThreads = 256;   // atss_assign_kernel
constexpr int kAtssRound = 128;     // target rows whose records are staged in LDS at a time (more rows: further rounds)

// workspace: one record per (image, level, target row), [B][L][n_max] -- the rows of a level lie next to each other, so the
// dense launch stages a round of them with coalesced loads.  Padding rows: never written, never read.
struct alignas(16) AtssRecord {
  double t;                             // mean + std of the row's candidates' IoUs over ALL levels (the same in each of its records); NaN: none
  int32_t cnt, pad_;                    // candidate cells of this level (min(k, H * W), 0 for NaN distances)
  int32_t win[4];                       // their first / last row, first / last column (empty: 1, 0, 1, 0); 16-byte aligned: one LDS read
  int32_t cell[ODTK_ATSS_MAX_TOPK];     // yc * W + xc, nearest first
};
constexpr int kAtssRecordWords = 24;
static_assert(sizeof(AtssRecord) == 4 * kAtssRecordWords, "the workspace query counts 96 bytes per target row and level");

struct AtssLevel {
  float *cls_target;      // [B, A, C, H, W] or null
  float *box_target;      // [B, A, 4, H, W]
  float *depth;           // [B, A, 1, H, W]
  int height, width;
  float stride;
  FastDiv by_width;
  float anchors[ODTK_MAX_ANCHORS * 4];
};

struct AtssArgs {
  AtssLevel lv[ODTK_MAX_LEVELS];
  uint32_t block_begin[ODTK_MAX_LEVELS + 1];   // atss_assign_kernel: first workgroup of each level
  const float *targets;                        // [B, n_max, 5] = (x, y, w, h, class), class < 0 marks padding
  AtssRecord *records;                         // [B, n_levels, n_max]
  FastDiv by_anchors;
  int n_levels, n_max, num_anchors, num_classes, topk;
};
static_assert(sizeof(AtssArgs) <= 4096, "kernel arguments travel by value");

// x1, y1, x2, y2, area of a target row (targets.hpp:71-73)
__device__ __forceinline__ void atss_box(const float *r, float q[5]) {
  q[0] = r[0]; q[1] = r[1];
  q[2] = r[0] + r[2] - 1.0f; q[3] = r[1] + r[3] - 1.0f;
  q[4] = (q[2] - q[0] + 1.0f) * (q[3] - q[1] + 1.0f);
}

// IoU of an anchor and a box, +1 pixel convention (targets.hpp:49, :84-89)
__device__ __forceinline__ float atss_iou(float ax1, float ay1, float ax2, float ay2, const float *q) {
  const float a_area = (ax2 - ax1 + 1.0f) * (ay2 - ay1 + 1.0f);
  float w = tmin_nan(ax2, q[2]) - tmax_nan(ax1, q[0]) + 1.0f;
  float h = tmin_nan(ay2, q[3]) - tmax_nan(ay1, q[1]) + 1.0f;
  w = w < 0.0f ? 0.0f : w;
  h = h < 0.0f ? 0.0f : h;
  const float inter = w * h;
  return inter / (a_area + q[4] - inter);
}

// centre of the cell's anchors along one axis
__device__ __forceinline__ float atss_cell_centre(int c, float stride) { return static_cast<float>(c) * stride + 0.5f * stride + 0.5f; }

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) { return ~wave_max_u64(~v); }

// the packed key of a cell: d2 >= 0, so its bit pattern orders like its value; the cell index below it breaks ties.  NaN: all ones
__device__ __forceinline__ uint64_t atss_key(float dx, float dy, uint32_t cell) {
  const float d2 = dx * dx + dy * dy;
  return d2 != d2 ? ~0ull : (static_cast<uint64_t>(__float_as_uint(d2)) << 32) | cell;
}

// The window of the statistics launch: kAtssWindow x kAtssWindow cells (clipped to the level) around the cell the box centre
// falls into.  WHERE it lies is a guess and proves nothing; the result of scanning only the window is taken when, and only
// when, the following holds -- otherwise the level is scanned in full:
//   sound   the box centre lies between the centres of the first column left of the window and the first column right of it
//           (where they exist), and likewise for the rows.  Then every column left of the window is at least as far from the
//           box centre as the adjacent one, |px - bcx| grows with the distance from the window, and -- rounding is monotone --
//           so do the float32 values dx = px - bcx and dx * dx; the same on the right, above and below.
//   bound   = the smallest dx * dx / dy * dy of those (up to four) adjacent columns and rows, computed with the kernel's own
//           operations.  A cell outside the window lies in an outside column or an outside row, so its d2 = fl(dx2 + dy2) >=
//           its dx2 >= bound, or >= its dy2 >= bound (the other term is >= 0 and the sum rounds monotonically).
//   the window holds min(k, H * W) cells with d2 < bound, strictly.
// Then every cell outside ranks strictly after those min(k, H * W) cells whatever its index, so the level's nearest cells
// are the window's, in the same order -- for a level 1 or 2 cells wide (the window is the level's width there, with no outside
// column) as for a centre outside the grid (one side has no outside column; if the far cells tie, the strict test fails and the
// level is scanned in full).  NaN or infinite distances fail `sound` or the strict test.  tests/atss_ref.py restates the rule on
// the host; tests/test_atss.py holds it to the full scan by brute force.
constexpr int kAtssWindow = 8;
struct AtssWindow { int r0, r1, c0, c1; float bound; bool sound; };

__device__ __forceinline__ int atss_window_start(float centre, float stride, int cells) {
  const int span = cells < kAtssWindow ? cells : kAtssWindow;
  const float first = floorf((centre - 0.5f) / stride - 0.5f) - static_cast<float>(kAtssWindow / 2 - 1);
  const float last = static_cast<float>(cells - span);
  return !(first >= 0.0f) ? 0 : static_cast<int>(first > last ? last : first);      // NaN: 0
}

__device__ __forceinline__ AtssWindow atss_window(float bcx, float bcy, float stride, int height, int width) {
  AtssWindow w;
  w.c0 = atss_window_start(bcx, stride, width);
  w.r0 = atss_window_start(bcy, stride, height);
  w.c1 = w.c0 + (width < kAtssWindow ? width : kAtssWindow) - 1;
  w.r1 = w.r0 + (height < kAtssWindow ? height : kAtssWindow) - 1;
  w.sound = true;
  w.bound = __uint_as_float(0x7f800000u);
  if (w.c0 > 0) { const float e = atss_cell_centre(w.c0 - 1, stride); w.sound = w.sound && bcx >= e; const float d = e - bcx; w.bound = fminf(w.bound, d * d); }
  if (w.c1 < width - 1) { const float e = atss_cell_centre(w.c1 + 1, stride); w.sound = w.sound && bcx <= e; const float d = e - bcx; w.bound = fminf(w.bound, d * d); }
  if (w.r0 > 0) { const float e = atss_cell_centre(w.r0 - 1, stride); w.sound = w.sound && bcy >= e; const float d = e - bcy; w.bound = fminf(w.bound, d * d); }
  if (w.r1 < height - 1) { const float e = atss_cell_centre(w.r1 + 1, stride); w.sound = w.sound && bcy <= e; const float d = e - bcy; w.bound = fminf(w.bound, d * d); }
  return w;
}

struct AtssPick { int cnt, r0, r1, c0, c1; };   // candidate cells of a level so far, their first / last row and column

// one more candidate cell (every lane of the wave calls it with the same cell)
__device__ __forceinline__ void atss_note(AtssPick &p, uint32_t cell, const FastDiv &by_width, int *s_cell, int lane) {
  uint32_t xc;
  const int yc = static_cast<int>(fastdivmod(cell, by_width, &xc)), x = static_cast<int>(xc);
  if (p.cnt == 0) { p.r0 = p.r1 = yc; p.c0 = p.c1 = x; }
  p.r0 = yc < p.r0 ? yc : p.r0; p.r1 = yc > p.r1 ? yc : p.r1;
  p.c0 = x < p.c0 ? x : p.c0; p.c1 = x > p.c1 ? x : p.c1;
  if (lane == 0) s_cell[p.cnt] = static_cast<int>(cell);
  ++p.cnt;
}

__global__ __launch_bounds__(kWave) void atss_stats_kernel(const AtssArgs a) {
  __shared__ float s_iou[ODTK_MAX_LEVELS * ODTK_ATSS_MAX_TOPK * ODTK_MAX_ANCHORS];   // the candidates' IoUs in list order
  __shared__ int s_cell[ODTK_ATSS_MAX_TOPK];

  const int row = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const size_t at = static_cast<size_t>(b) * a.n_max + row;
  const float *tg = a.targets + at * 5;
  if (!(tg[4] > -1.0f)) return;                               // padding (wave-uniform)
  float q[5];
  atss_box(tg, q);
  const float bcx = q[0] + 0.5f * (q[2] - q[0] + 1.0f), bcy = q[1] + 0.5f * (q[3] - q[1] + 1.0f);
  AtssRecord *rec = a.records + static_cast<size_t>(b) * a.n_levels * a.n_max + row;   // + l * n_max: the level's record

  int listed = 0;                                             // candidate cells of the levels before this one
  for (int l = 0; l < a.n_levels; ++l) {
    const AtssLevel &lv = a.lv[l];
    const uint32_t hw = static_cast<uint32_t>(lv.height) * static_cast<uint32_t>(lv.width);
    const int want = static_cast<uint32_t>(a.topk) < hw ? a.topk : static_cast<int>(hw);
    __syncthreads();                                          // s_cell: the previous level's IoUs have read it
    AtssPick pick = {0, 1, 0, 1, 0};
    bool settled = false;
    if (hw > static_cast<uint32_t>(kWave)) {
      // the window: one cell per lane, its key computed once
      const AtssWindow win = atss_window(bcx, bcy, lv.stride, lv.height, lv.width);
      const int c = win.c0 + (lane & (kAtssWindow - 1)), r = win.r0 + (lane >> 3);
      uint64_t mine = ~0ull;
      if (c <= win.c1 && r <= win.r1)
        mine = atss_key(atss_cell_centre(c, lv.stride) - bcx, atss_cell_centre(r, lv.stride) - bcy, static_cast<uint32_t>(r * lv.width + c));
      uint64_t best = 0;
      for (; pick.cnt < want; ) {
        best = wave_min_u64(mine);
        if (best == ~0ull) break;
        if (mine == best) mine = ~0ull;
        atss_note(pick, static_cast<uint32_t>(best), lv.by_width, s_cell, lane);
      }
      settled = win.sound && pick.cnt == want && __uint_as_float(static_cast<uint32_t>(best >> 32)) < win.bound;
      if (!settled) pick = {0, 1, 0, 1, 0};
    }
    if (!settled) {
      // the full scan: per round the smallest key after the last one (keys are unique: the cell is in them)
      uint64_t last = 0;
      for (; pick.cnt < want; ) {
        uint64_t best = ~0ull;
        for (uint32_t i = lane; i < hw; i += kWave) {
          uint32_t xc;
          const uint32_t yc = fastdivmod(i, lv.by_width, &xc);
          const uint64_t key = atss_key(atss_cell_centre(static_cast<int>(xc), lv.stride) - bcx,
                                        atss_cell_centre(static_cast<int>(yc), lv.stride) - bcy, i);
          if ((pick.cnt == 0 || key > last) && key < best) best = key;
        }
        best = wave_min_u64(best);
        if (best == ~0ull) break;                             // only NaN distances are left
        last = best;
        atss_note(pick, static_cast<uint32_t>(best), lv.by_width, s_cell, lane);
      }
    }
    const int cnt = pick.cnt;
    if (lane == 0) {
      AtssRecord &out = rec[static_cast<size_t>(l) * a.n_max];
      out.cnt = cnt;
      out.win[0] = pick.r0; out.win[1] = pick.r1; out.win[2] = pick.c0; out.win[3] = pick.c1;
    }
    __syncthreads();
    for (uint32_t i = lane; i < static_cast<uint32_t>(cnt * a.num_anchors); i += kWave) {
      uint32_t an;
      const uint32_t j = fastdivmod(i, a.by_anchors, &an);
      uint32_t xc;
      const uint32_t yc = fastdivmod(static_cast<uint32_t>(s_cell[j]), lv.by_width, &xc);
      const float gx = static_cast<float>(xc) * lv.stride, gy = static_cast<float>(yc) * lv.stride;
      if (an == 0) rec[static_cast<size_t>(l) * a.n_max].cell[j] = s_cell[j];
      s_iou[listed * a.num_anchors + i] = atss_iou(gx + lv.anchors[an * 4 + 0], gy + lv.anchors[an * 4 + 1],
                                                   gx + lv.anchors[an * 4 + 2], gy + lv.anchors[an * 4 + 3], q);
    }
    listed += cnt;
  }
  __syncthreads();
  if (lane == 0) {
    const int n = listed * a.num_anchors;
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum = sum + static_cast<double>(s_iou[i]);
    const double mean = sum / static_cast<double>(n);
    double ss = 0.0;
    for (int i = 0; i < n; ++i) {
      const double d = static_cast<double>(s_iou[i]) - mean;
      ss = ss + d * d;
    }
    const double var = n > 1 ? ss / static_cast<double>(n - 1) : 0.0;
    const double t = n > 0 ? mean + sqrt(var) : __longlong_as_double(0x7ff8000000000000ll);
    for (int l = 0; l < a.n_levels; ++l) rec[static_cast<size_t>(l) * a.n_max].t = t;
  }
}

__global__ __launch_bounds__(kAtssThreads) void atss_assign_kernel(const AtssArgs a) {
  __shared__ AtssRecord s_rec[kAtssRound];                    // this level's records of the VALID rows of this round, in order
  __shared__ float s_box[kAtssRound * 6];                     // their x1, y1, x2, y2, area, class
  __shared__ int s_pos[kAtssRound];                           // row of the round -> its place among the valid ones, or -1
  __shared__ int s_n;

  const int l = level_of<ODTK_MAX_LEVELS>(a.block_begin, a.n_levels);
  const AtssLevel &lv = a.lv[l];
  const int b = blockIdx.y;
  const float *tg = a.targets + static_cast<size_t>(b) * a.n_max * 5;
  const AtssRecord *recs = a.records + (static_cast<size_t>(b) * a.n_levels + l) * a.n_max;
  const int hw = lv.height * lv.width;
  const int cell = static_cast<int>(blockIdx.x - a.block_begin[l]) * kAtssThreads + static_cast<int>(threadIdx.x);   // (anchor, y, x) flattened
  const bool live = cell < a.num_anchors * hw;
  const int an = live ? cell / hw : 0, pix = live ? cell - an * hw : 0;
  const int y = pix / lv.width, x = pix - y * lv.width;
  const float gx = static_cast<float>(x) * lv.stride, gy = static_cast<float>(y) * lv.stride;
  const float ax1 = gx + lv.anchors[an * 4 + 0], ay1 = gy + lv.anchors[an * 4 + 1];
  const float ax2 = gx + lv.anchors[an * 4 + 2], ay2 = gy + lv.anchors[an * 4 + 3];
  const float px = atss_cell_centre(x, lv.stride), py = atss_cell_centre(y, lv.stride);

  bool have = false;
  float best = 0.0f;
  float bq[5] = {0, 0, 0, 0, 0};   // x1, y1, x2, y2, class of the box this anchor goes to
  for (int base = 0; base < a.n_max; base += kAtssRound) {
    // compact the valid rows of this round in order, with this level's part of their records: one wave, ballot
    __syncthreads();
    if (threadIdx.x < kWave) {
      int n = 0;
      const int end = base + kAtssRound < a.n_max ? base + kAtssRound : a.n_max;
      for (int i0 = base; i0 < end; i0 += kWave) {
        const int i = i0 + static_cast<int>(threadIdx.x);
        float r[5] = {0, 0, 0, 0, -1};
        if (i < end) {
#pragma unroll
          for (int k = 0; k < 5; ++k) r[k] = tg[static_cast<size_t>(i) * 5 + k];
        }
        const bool valid = r[4] > -1.0f;
        const uint64_t m = __ballot(valid);
        if (valid) {
          const int p = n + __popcll(m & ((1ull << threadIdx.x) - 1ull));
          float q[5];
          atss_box(r, q);
#pragma unroll
          for (int k = 0; k < 5; ++k) s_box[p * 6 + k] = q[k];
          s_box[p * 6 + 5] = r[4];
          s_pos[i - base] = p;
        } else if (i < end) {
          s_pos[i - base] = -1;
        }
        n += __popcll(m);
      }
      if (threadIdx.x == 0) s_n = n;
    }
    __syncthreads();
    {
      // the records of the round's valid rows, word by word with every thread: consecutive threads read consecutive words
      const int end = base + kAtssRound < a.n_max ? base + kAtssRound : a.n_max;
      const uint32_t *src = reinterpret_cast<const uint32_t *>(recs + base);
      uint32_t *dst = reinterpret_cast<uint32_t *>(s_rec);
      for (int i = static_cast<int>(threadIdx.x); i < (end - base) * kAtssRecordWords; i += kAtssThreads) {
        const int row = i / kAtssRecordWords, p = s_pos[row];
        if (p >= 0) dst[p * kAtssRecordWords + (i - row * kAtssRecordWords)] = src[i];
      }
    }
    __syncthreads();
    const int n = s_n;
    for (int i = 0; i < n; ++i) {
      const AtssRecord &rec = s_rec[i];
      const int4 win = *reinterpret_cast<const int4 *>(rec.win);                // ONE read, no short circuit: four dependent LDS round trips otherwise
      if ((y < win.x) | (y > win.y) | (x < win.z) | (x > win.w)) continue;
      bool cand = false;
      for (int k = 0; k < rec.cnt; ++k) cand = cand || rec.cell[k] == pix;
      if (!cand) continue;
      const float *q = s_box + i * 6;
      const float ov = atss_iou(ax1, ay1, ax2, ay2, q);
      if (!(static_cast<double>(ov) >= rec.t)) continue;                        // NaN on either side: not positive
      if (!(px - q[0] > 0.01f && py - q[1] > 0.01f && q[2] - px > 0.01f && q[3] - py > 0.01f)) continue;
      if (!have || ov > best) {                                                  // largest IoU, the earliest box on a tie
        have = true;
        best = ov;
        bq[0] = q[0]; bq[1] = q[1]; bq[2] = q[2]; bq[3] = q[3]; bq[4] = q[5];
      }
    }
  }
  if (!live) return;
  const size_t img = static_cast<size_t>(b) * a.num_anchors;
  float *box = lv.box_target + (img + an) * 4 * hw + pix;

  int hot = -1;                 // class channel that gets the 1
  float dl[4] = {0, 0, 0, 0}, dval = 0.0f;
  if (have) {
    // box2delta, in the operation order of targets.hpp:106-113
    const float aw = ax2 - ax1 + 1.0f, ah = ay2 - ay1 + 1.0f;
    const float acx = ax1 + 0.5f * aw, acy = ay1 + 0.5f * ah;
    const float bw = bq[2] - bq[0] + 1.0f, bh = bq[3] - bq[1] + 1.0f;
    const float bcx = bq[0] + 0.5f * bw, bcy = bq[1] + 0.5f * bh;
    dl[0] = (bcx - acx) / aw;
    dl[1] = (bcy - acy) / ah;
    dl[2] = logf(bw / aw);
    dl[3] = logf(bh / ah);
    dval = bq[4] + 1.0f;
    hot = static_cast<int>(bq[4]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) box[static_cast<size_t>(k) * hw] = dl[k];
  lv.depth[(img + an) * hw + pix] = dval;
  if (lv.cls_target) {
    float *cls = lv.cls_target + (img + an) * a.num_classes * hw + pix;
    for (int c = 0; c < a.num_classes; ++c) cls[static_cast<size_t>(c) * hw] = (c == hot) ? 1.0f : 0.0f;
  }
}

}  // namespace odtk
