// cell_loss.hpp -- the machine the opt-in training losses share: the IoU-family box losses (box_iou_loss.hpp), the Gaussian box
// losses of rotated boxes (rotated_box_loss.hpp) and the quality / varifocal class losses (quality_loss.hpp).  Each of them is a
// sum over the anchor cells of every pyramid level of the batch, per level a pair (sum of the terms, number of foreground anchors):
//   - the level table and the anchor SIZES travel in the kernel arguments (CellLossArgs / CellLossLevel); level_of (common.hpp)
//     finds a workgroup's level, the workgroups of level l being [block_begin[l], block_begin[l + 1]);
//   - forward: every workgroup leaves its pair in the workspace (store_block_pair), then level_pair_reduce_kernel adds the pairs
//     of a level up in one fixed order.  No atomics: the same bits on every run;
//   - backward: one launch in the order the gradient lies in memory, every element written.
// The two box-loss families are one lane per anchor cell and differ in the per-anchor term only: cell_loss_forward_kernel /
// cell_loss_backward_kernel take it as a policy.  A new per-cell box loss supplies such a policy -- a struct with
//     kParams                                   deltas per anchor
//     Grad                                      the type its term computes in (float / double)
//     load<T>(L, A, ia, an, pix, p, t)          the cell's predicted and target deltas as float32
//     term<kGrad>(p, t, aw, ah, kind, grad)     L of one anchor; kGrad: also dL/dp
//     grad_value(g, grad)                       upstream gradient x dL/dp as the float32 that is stored (a zero always +0)
//     store_cell<T>(base, cell, v)              the cell's kParams consecutive elements of a channels_last gradient
// next to its definition (the numeric contract stays in the header of the loss), its kinds in box_iou_fill's check and an entry
// point over cell_loss_levels_forward / _backward in train.hip.  A loss that walks other elements than anchor cells (the quality
// losses stream the logits) keeps its own kernel and shares the arguments, level_of, store_block_pair and the reduce.
#pragma once

#include "loss.hpp"   // store_elem, block_sum; element types; fastdiv

namespace odtk {

constexpr int kCellLossThreads = 256;

struct CellLossLevel {
  const void *box;          // [B, A*kParams, H, W] predicted deltas, element type T
  const float *depth;       // [B, A, 1, H, W]
  const float *box_target;  // [B, A, kParams, H, W]
  void *dbox;               // backward: gradient, dtype / layout of box
  const float *g;           // backward: device scalar d(out)/d(sum) of this level (null: 0)
  uint32_t hw, cells;       // H*W, B*A*H*W (kParams * cells < 2^31: host)
  uint32_t channels_last, pad_;
  FastDiv by_hw, by_anchors;
  float aw[ODTK_MAX_ANCHORS], ah[ODTK_MAX_ANCHORS];
};

struct CellLossArgs {
  CellLossLevel lv[ODTK_MAX_LEVELS];
  uint32_t block_begin[ODTK_MAX_LEVELS + 1];
  double *partial;          // forward: [gridDim.x][2] = (sum, fg) per workgroup
  uint32_t n_levels, num_anchors, kind, pad_;
};

// The end of a forward workgroup: its (sum, fg) into the workspace.
__device__ __forceinline__ void store_block_pair(double loss, double fg, double *s_red, double *partial) {
  const double s = block_sum(loss, s_red);
  const double f = block_sum(fg, s_red);
  if (threadIdx.x == 0) {
    partial[2 * static_cast<size_t>(blockIdx.x)] = s;
    partial[2 * static_cast<size_t>(blockIdx.x) + 1] = f;
  }
}

// Workgroup l adds up the pairs of level l: thread t takes workgroups t, t + 256, ... in order, then the wave / block tree.
struct LevelPairReduceArgs {
  const double *partial;
  double *sums;                                // [n_levels][2] = (sum, fg)
  uint32_t block_begin[ODTK_MAX_LEVELS + 1];
};

__global__ __launch_bounds__(kCellLossThreads) void level_pair_reduce_kernel(const LevelPairReduceArgs a) {
  __shared__ double s_red[kCellLossThreads / kWave];
  const uint32_t l = blockIdx.x, b1 = a.block_begin[l + 1];
  double s = 0.0, f = 0.0;
  for (uint32_t b = a.block_begin[l] + threadIdx.x; b < b1; b += kCellLossThreads) {
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

// Lanes in depth's order (image, anchor, pixel): the depth read is coalesced; a foreground lane gathers its deltas.
template <typename T, typename Loss>
__global__ __launch_bounds__(kCellLossThreads) void cell_loss_forward_kernel(const CellLossArgs a) {
  __shared__ double s_red[kCellLossThreads / kWave];
  const int l = level_of<ODTK_MAX_LEVELS>(a.block_begin, a.n_levels);
  const CellLossLevel &L = a.lv[l];
  const uint32_t cell = (blockIdx.x - a.block_begin[l]) * kCellLossThreads + threadIdx.x;   // (image * A + an) * hw + pix
  double loss = 0.0, fg = 0.0;
  if (cell < L.cells && L.depth[cell] > 0.0f) {
    uint32_t pix, an;
    const uint32_t ia = fastdivmod(cell, L.by_hw, &pix);
    fastdivmod(ia, L.by_anchors, &an);
    float p[Loss::kParams], t[Loss::kParams];
    Loss::template load<T>(L, a.num_anchors, ia, an, pix, p, t);
    loss = Loss::template term<false>(p, t, L.aw[an], L.ah[an], a.kind, nullptr);
    fg = 1.0;
  }
  store_block_pair(loss, fg, s_red, a.partial);
}

// Lanes in the order d(deltas) lies in memory: NCHW (image, anchor, pixel), kParams plane stores of consecutive elements per
// wave; NHWC (image, pixel, anchor), the cell's kParams elements by Loss::store_cell, a wave's stores one run.
template <typename T, typename Loss>
__global__ __launch_bounds__(kCellLossThreads) void cell_loss_backward_kernel(const CellLossArgs a) {
  constexpr uint32_t kParams = Loss::kParams;
  const int l = level_of<ODTK_MAX_LEVELS>(a.block_begin, a.n_levels);
  const CellLossLevel &L = a.lv[l];
  const uint32_t cell = (blockIdx.x - a.block_begin[l]) * kCellLossThreads + threadIdx.x;
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
  float out[kParams] = {};
  if (L.depth[ia * L.hw + pix] > 0.0f) {
    const float g = L.g ? *L.g : 0.0f;
    float p[kParams], t[kParams];
    typename Loss::Grad grad[kParams];
    Loss::template load<T>(L, A, ia, an, pix, p, t);
    Loss::template term<true>(p, t, L.aw[an], L.ah[an], a.kind, grad);
#pragma unroll
    for (uint32_t k = 0; k < kParams; ++k) out[k] = Loss::grad_value(g, grad[k]);
  }
  if (L.channels_last) {
    Loss::template store_cell<T>(L.dbox, cell, out);
  } else {
    const uint32_t plane = ia * kParams * L.hw + pix;
#pragma unroll
    for (uint32_t k = 0; k < kParams; ++k) store_elem<T>(L.dbox, plane + k * L.hw, out[k]);
  }
}

}  // namespace odtk
