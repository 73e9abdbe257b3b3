// train.hip -- target assignment (odtk_snap_to_anchors*, odtk_atss_assign_levels, odtk_tal_assign_levels) and the focal + smooth-L1 loss: launch shapes,
// odtk_debug_loss_*, odtk_retina_loss_*; the IoU-family box losses (odtk_box_iou_loss_levels_*); the quality / varifocal
// classification losses (odtk_quality_loss_levels_*); the Gaussian box losses of rotated boxes (odtk_rotated_box_loss_levels_*);
// the optimisation step and the gradient norm (odtk_optim_sgd_step, odtk_optim_grad_norm*).
#include <cmath>
#include <cstring>
#include <mutex>

#include "runtime.hpp"
#include "targets.hpp"
#include "atss.hpp"
#include "tal.hpp"
#include "loss.hpp"
#include "box_iou_loss.hpp"   // (all three over cell_loss.hpp)
#include "quality_loss.hpp"
#include "rotated_box_loss.hpp"
#include "optim.hpp"

namespace {

// Launch shape of the loss kernels (odtk_debug_loss_tuning; defaults = the measured best):
// workgroup size, resident workgroups per CU the logit walk is capped at, 16-byte vectors a lane loads per trip.
struct LossTuning {
  int threads, per_cu, unroll, box_blocks;
  int per_wave, window, box_rows;   // odtk_debug_loss_layout: per-wave sums (workspace form only), contiguous trips, the backward's
                                    // box-delta walk in memory order (csrc/loss.hpp LossArgs)
  int form;   // filled by loss_tuning_snapshot from g_loss_form (odtk_debug_loss_form): 1 = vectors of negatives take focal_plain
};
// [16-bit heads, fp32 heads][forward with atomics, backward, forward through a workspace] = threads, logit workgroups per
// CU and level, vectors per trip, box workgroups per level; measured with tools/loss_probe.py (profiles/r03_loss_probe.txt)
enum { kLossFwd = 0, kLossBwd = 1, kLossFwdWs = 2 };
std::mutex g_loss_tuning_mu;
// Round 6 (profiles/r06_loss_layout_probe.txt): the backward walks contiguous trips (window 1) with 256-thread workgroups and
// writes d(deltas) in memory order -- fp32 50.6 -> 42.6-43.1 us, bf16 34.3 -> 27.4 us.
// The forward through the workspace walks contiguous trips too (fp32: two vectors per trip); per-wave sums stay off (walk -1.3 us,
// reduce launch +0.8 us: nothing).
LossTuning g_loss_tuning[2][3] = {{{512, 1, 2, 64, 0, 0, 1, 0}, {256, 4, 1, 256, 0, 1, 1, 0}, {256, 4, 1, 256, 0, 1, 1, 0}},
                                  {{512, 1, 4, 64, 0, 0, 1, 0}, {256, 8, 2, 1024, 0, 1, 1, 0}, {256, 4, 2, 256, 0, 1, 1, 0}}};

// Arithmetic form of the classification walk with gamma = 2 (csrc/loss.hpp focal_plain): 0 = every element through the
// symmetric focal_term (rounds 3-4), 1 = vectors that hold no positive element and no logit beyond kPlainMax through
// focal_plain.  Same sums to ~1e-8, same gradients to ~1e-6 of the largest (both well inside the tested bars).
int g_loss_form = ODTK_LOSS_FORM_DEFAULT;

LossTuning loss_tuning_snapshot(int dtype, int which) {
  std::lock_guard<std::mutex> lock(g_loss_tuning_mu);
  LossTuning t = g_loss_tuning[dtype == ODTK_F32][which];
  t.form = g_loss_form;
  return t;
}

// fills the kernel arguments of one level; returns the number of workgroups it wants (0 on error, *rc set)
unsigned retina_loss_fill(odtk::LossArgs &la, int which, const void *cls, const void *box, const float *depth,
                          const float *box_target, int batch, int A, int C, int height, int width, int nb, int dtype,
                          int channels_last, float alpha, float gamma, float beta, double *sums, const float *g_cls,
                          const float *g_box, void *dcls, void *dbox, const LossTuning &t, int *rc) {
  const bool backward = which == kLossBwd;
  *rc = ODTK_ERR_INVALID;
  if (!cls || !box || !depth || !box_target || batch <= 0 || A <= 0 || C <= 0 || height <= 0 || width <= 0 || nb <= 0) return 0;
  if (channels_last != 0 && channels_last != 1) return 0;
  if ((reinterpret_cast<uintptr_t>(cls) | reinterpret_cast<uintptr_t>(box)) & 15u) return 0;   // 16-B vector loads
  if (backward && (!dcls || !dbox || ((reinterpret_cast<uintptr_t>(dcls) | reinterpret_cast<uintptr_t>(dbox)) & 15u))) return 0;
  const unsigned long long n = 1ull * batch * A * C * height * width;
  if (n >= (1ull << 32)) return 0;
  if (1ull * batch * A * nb * height * width >= (1ull << 32)) return 0;
  std::memset(&la, 0, sizeof la);
  la.cls = cls; la.box = box; la.depth = depth; la.box_target = box_target;
  la.acc = sums; la.g_cls = g_cls; la.g_box = g_box; la.dcls = dcls; la.dbox = dbox;
  la.batch = batch; la.num_anchors = A; la.num_classes = C; la.hw = static_cast<uint32_t>(height) * width; la.nb = nb;
  la.channels_last = channels_last;
  la.alpha = alpha; la.gamma = gamma; la.beta = beta;
  la.by_channels = odtk::fastdiv_make(static_cast<uint32_t>(A) * C);
  la.by_hw = odtk::fastdiv_make(la.hw);
  la.by_classes = odtk::fastdiv_make(C);
  la.by_anchors = odtk::fastdiv_make(A);
  const unsigned threads = t.threads, unroll = t.unroll;
  const unsigned per = dtype == ODTK_F32 ? 4u : 8u;
  // at least two trips of `unroll` vectors per lane where the level is large enough
  unsigned long long cls_blocks = (n / per + threads * unroll * 2ull - 1) / (threads * unroll * 2ull);
  if (cls_blocks < 1) cls_blocks = 1;
  // forward: every block ends in (up to) three double atomics on the SAME three words of its level, ~11 ns each when
  // they queue up (MI355X_MICROARCH.md "fanin") -- 4096 blocks cost 40 us of pure queueing per launch, and the ~2 800
  // box-delta blocks of round 2 (one cell per lane, two atomics each) cost ~30 us on their own: the forward launch
  // keeps both kinds of workgroup few (a lane walks several vectors / cells); backward has no such tail.
  // The cap is PER LEVEL: dealing one budget to the levels in proportion to their size (P3 = 3/4 of the logits) was
  // measured slower -- 768 atomics on P3's word instead of 256 (profiles/r03_loss_probe_proportional_dealing.txt).
  const unsigned long long block_cap = 256ull * t.per_cu;
  if (cls_blocks > block_cap) cls_blocks = block_cap;
  unsigned long long box_blocks = (1ull * batch * A * height * width + threads - 1) / threads;
  if (box_blocks > static_cast<unsigned>(t.box_blocks)) box_blocks = t.box_blocks;
  la.cls_blocks = static_cast<uint32_t>(cls_blocks);
  la.per_wave = (which == kLossFwdWs && t.per_wave) ? 1u : 0u;
  la.window = t.window ? 1u : 0u;
  la.box_rows = t.box_rows ? 1u : 0u;
  *rc = ODTK_OK;
  return static_cast<unsigned>(cls_blocks + box_blocks);
}

template <typename T, bool kBackward>
void retina_loss_dispatch(const odtk::LossLevelsArgs &la, unsigned total, const LossTuning &t, hipStream_t stream) {
  const dim3 grid(total), block(t.threads);
#ifdef ODTK_LOSS_ABLATIONS   // build flag of tools/loss_form_probe.py only (make ablations): never in the shipped library
  if constexpr (std::is_same_v<T, odtk::F32> && !kBackward) {
    // timing ablations of form 1 (wrong results on purpose; tools/loss_form_probe.py): fp32 forward, four vectors per trip
    if (t.form == 2) { timed_launch(ODTK_KERNEL_LOSS, odtk::retina_loss_kernel<T, false, 4, 2>, grid, block, 0, stream, la); return; }
    if (t.form == 3) { timed_launch(ODTK_KERNEL_LOSS, odtk::retina_loss_kernel<T, false, 4, 3>, grid, block, 0, stream, la); return; }
    if (t.form == 4) { timed_launch(ODTK_KERNEL_LOSS, odtk::retina_loss_kernel<T, false, 4, 4>, grid, block, 0, stream, la); return; }
    if (t.form == 6) { timed_launch(ODTK_KERNEL_LOSS, odtk::retina_loss_kernel<T, false, 4, 6>, grid, block, 0, stream, la); return; }
    if (t.form == 7) { timed_launch(ODTK_KERNEL_LOSS, odtk::retina_loss_kernel<T, false, 4, 7>, grid, block, 0, stream, la); return; }
  }
#endif
  if (t.form) {
    switch (t.unroll) {
      case 1: timed_launch(ODTK_KERNEL_LOSS, odtk::retina_loss_kernel<T, kBackward, 1, 1>, grid, block, 0, stream, la); break;
      case 2: timed_launch(ODTK_KERNEL_LOSS, odtk::retina_loss_kernel<T, kBackward, 2, 1>, grid, block, 0, stream, la); break;
      default: timed_launch(ODTK_KERNEL_LOSS, odtk::retina_loss_kernel<T, kBackward, 4, 1>, grid, block, 0, stream, la); break;
    }
    return;
  }
  switch (t.unroll) {
    case 1: timed_launch(ODTK_KERNEL_LOSS, odtk::retina_loss_kernel<T, kBackward, 1, 0>, grid, block, 0, stream, la); break;
    case 2: timed_launch(ODTK_KERNEL_LOSS, odtk::retina_loss_kernel<T, kBackward, 2, 0>, grid, block, 0, stream, la); break;
    default: timed_launch(ODTK_KERNEL_LOSS, odtk::retina_loss_kernel<T, kBackward, 4, 0>, grid, block, 0, stream, la); break;
  }
}

// which: kLossFwd (atomics into `sums`, pre-zeroed), kLossBwd, kLossFwdWs (per-workgroup sums into `partial`, then the
// reduce launch writes `sums`).  With partial == nullptr and kLossFwdWs: returns the number of workgroups (size query).
int retina_loss_levels_launch(int which, int n_levels, const odtk_loss_level_t *levels, int batch, int A, int C, int nb,
                              int dtype, float alpha, float gamma, float beta, double *sums, const float *g_cls,
                              const float *g_box, double *partial, bool query, hipStream_t stream,
                              const LossTuning *tuning = nullptr) {
  if (n_levels <= 0 || n_levels > ODTK_MAX_LEVELS || !levels) return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  const bool backward = which == kLossBwd;
  // ONE snapshot of the launch shape per call: the size query and the launch of the workspace form must agree even if
  // odtk_debug_loss_tuning runs on another thread in between
  const LossTuning t = tuning ? *tuning : loss_tuning_snapshot(dtype, which);
  odtk::LossLevelsArgs la;
  std::memset(&la, 0, sizeof la);
  la.n_levels = n_levels;
  unsigned total = 0;
  for (int l = 0; l < n_levels; ++l) {
    int rc;
    const unsigned blocks = retina_loss_fill(la.lv[l], which, levels[l].cls, levels[l].box, levels[l].depth, levels[l].box_target,
                                             batch, A, C, levels[l].height, levels[l].width, nb, dtype, levels[l].channels_last,
                                             alpha, gamma, beta, sums ? sums + 3 * l : nullptr, g_cls ? g_cls + l : nullptr,
                                             g_box ? g_box + l : nullptr, levels[l].dcls, levels[l].dbox, t, &rc);
    if (rc != ODTK_OK) return rc;
    la.lv[l].partial = which == kLossFwdWs ? partial : nullptr;
    la.block_begin[l] = total;
    total += blocks;
  }
  for (int l = n_levels; l <= ODTK_MAX_LEVELS; ++l) la.block_begin[l] = total;
  if (query) return static_cast<int>(total);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    backward ? retina_loss_dispatch<T, true>(la, total, t, stream) : retina_loss_dispatch<T, false>(la, total, t, stream);
  });
  ODTK_HIP_TRY(hipGetLastError());
  if (which == kLossFwdWs) {
    odtk::LossReduceArgs ra;
    std::memset(&ra, 0, sizeof ra);
    ra.partial = partial;
    ra.per = t.per_wave ? static_cast<uint32_t>(t.threads) / 64u : 1u;
    ra.sums = sums;
    for (int l = 0; l <= ODTK_MAX_LEVELS; ++l) ra.block_begin[l] = la.block_begin[l];
    timed_launch(ODTK_KERNEL_LOSS_REDUCE, odtk::loss_reduce_kernel, dim3(n_levels), dim3(odtk::kLossReduceThreads), 0, stream, ra);
    ODTK_HIP_TRY(hipGetLastError());
  }
  return ODTK_OK;
}

// one level = a one-entry level table through the same kernel
int retina_loss_launch(bool backward, const void *cls, const void *box, const float *depth, const float *box_target,
                       int batch, int A, int C, int height, int width, int nb, int dtype, int channels_last, float alpha,
                       float gamma, float beta, double *sums, const float *g_cls, const float *g_box, void *dcls,
                       void *dbox, hipStream_t stream) {
  odtk_loss_level_t lv;
  std::memset(&lv, 0, sizeof lv);
  lv.cls = cls; lv.box = box; lv.depth = depth; lv.box_target = box_target;
  lv.dcls = dcls; lv.dbox = dbox;
  lv.height = height; lv.width = width; lv.channels_last = channels_last;
  return retina_loss_levels_launch(backward ? kLossBwd : kLossFwd, 1, &lv, batch, A, C, nb, dtype, alpha, gamma, beta, sums, g_cls, g_box,
                                   nullptr, false, stream);
}

// The kernel arguments of odtk_box_iou_loss_levels_* (csrc/box_iou_loss.hpp; nb = 4 box parameters per anchor) and of
// odtk_rotated_box_loss_levels_* (csrc/rotated_box_loss.hpp; nb = 6) from the ABI's level table; everything the entry points
// promise to check is checked here, on the host.  `pointers`: false for the workspace query, which looks at no data pointer.
int box_iou_fill(odtk::CellLossArgs &ba, bool backward, bool pointers, int n_levels, const odtk_loss_level_t *levels,
                 const float *const *anchors, int batch, int A, int dtype, int kind, const float *g, unsigned *total_blocks,
                 unsigned nb = 4) {
  if (n_levels <= 0 || n_levels > ODTK_MAX_LEVELS || !levels || !anchors || batch < 1 || A < 1 || A > ODTK_MAX_ANCHORS)
    return ODTK_ERR_INVALID;
  if (nb == 4 ? (kind != ODTK_BOX_LOSS_IOU && kind != ODTK_BOX_LOSS_GIOU && kind != ODTK_BOX_LOSS_DIOU)
              : (kind != ODTK_ROTATED_BOX_LOSS_PROBIOU && kind != ODTK_ROTATED_BOX_LOSS_KLD))
    return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  std::memset(&ba, 0, sizeof ba);
  ba.n_levels = n_levels;
  ba.num_anchors = A;
  ba.kind = kind;
  unsigned long long total = 0;
  for (int l = 0; l < n_levels; ++l) {
    const odtk_loss_level_t &lv = levels[l];
    odtk::CellLossLevel &bl = ba.lv[l];
    if (lv.height <= 0 || lv.width <= 0 || (lv.channels_last != 0 && lv.channels_last != 1) || !anchors[l]) return ODTK_ERR_INVALID;
    const unsigned long long cells = 1ull * batch * A * lv.height * lv.width;
    if (nb * cells >= (1ull << 31)) return ODTK_ERR_INVALID;    // the kernels index the deltas with 32 bits
    for (int i = 0; i < A; ++i) {
      const float *an = anchors[l] + 4 * i;
      const float aw = an[2] - an[0] + 1.0f, ah = an[3] - an[1] + 1.0f;
      if (!std::isfinite(aw) || !std::isfinite(ah) || !(aw > 0.0f) || !(ah > 0.0f)) return ODTK_ERR_INVALID;
      bl.aw[i] = aw;
      bl.ah[i] = ah;
    }
    if (pointers) {
      if (!lv.box || !lv.depth || !lv.box_target || (backward && !lv.dbox)) return ODTK_ERR_INVALID;
      // channels_last: one 16- / 8-byte vector per cell of four, three 8- / 4-byte pieces per cell of six; otherwise the
      // element's own alignment
      const uintptr_t vec = nb == 4 ? (dtype == ODTK_F32 ? 15u : 7u) : (dtype == ODTK_F32 ? 7u : 3u);
      const uintptr_t mask = lv.channels_last ? vec : (dtype == ODTK_F32 ? 3u : 1u);
      if ((reinterpret_cast<uintptr_t>(lv.box) | (backward ? reinterpret_cast<uintptr_t>(lv.dbox) : 0u)) & mask) return ODTK_ERR_INVALID;
      if ((reinterpret_cast<uintptr_t>(lv.depth) | reinterpret_cast<uintptr_t>(lv.box_target)) & 3u) return ODTK_ERR_INVALID;
    }
    bl.box = lv.box; bl.depth = lv.depth; bl.box_target = lv.box_target;
    bl.dbox = backward ? lv.dbox : nullptr;
    bl.g = (backward && g) ? g + l : nullptr;
    bl.hw = static_cast<uint32_t>(lv.height) * lv.width;
    bl.cells = static_cast<uint32_t>(cells);
    bl.channels_last = lv.channels_last;
    bl.by_hw = odtk::fastdiv_make(bl.hw);
    bl.by_anchors = odtk::fastdiv_make(A);
    ba.block_begin[l] = static_cast<uint32_t>(total);
    total += (cells + odtk::kCellLossThreads - 1) / odtk::kCellLossThreads;
  }
  for (int l = n_levels; l <= ODTK_MAX_LEVELS; ++l) ba.block_begin[l] = static_cast<uint32_t>(total);
  *total_blocks = static_cast<unsigned>(total);                   // <= 6 * 2^29 / 256
  return ODTK_OK;
}

// The kernel arguments of odtk_quality_loss_levels_* (csrc/quality_loss.hpp): the box side of every level through box_iou_fill (its
// checks are the box loss's own), then the logits.  Launch shape as the focal walk's: 256 threads, at least
// two trips per lane where the level is large enough, at most 256 * per_cu workgroups per level -- so a trip's stride stays below
// 2^21 vectors and the walk's 32-bit vector index cannot wrap.
int quality_fill(odtk::QualityArgs &qa, bool backward, bool pointers, int n_levels, const odtk_loss_level_t *levels,
                 const float *const *anchors, int batch, int A, int C, int dtype, int kind, float alpha, float gamma, const float *g,
                 unsigned *total_blocks) {
  if (kind != ODTK_CLS_LOSS_QFL && kind != ODTK_CLS_LOSS_VFL) return ODTK_ERR_INVALID;
  if (!std::isfinite(gamma) || gamma < 1.0f || !std::isfinite(alpha) || alpha < 0.0f || C < 1) return ODTK_ERR_INVALID;
  odtk::CellLossArgs ba;
  unsigned box_blocks = 0;
  const int rc = box_iou_fill(ba, false, pointers, n_levels, levels, anchors, batch, A, dtype, ODTK_BOX_LOSS_IOU, nullptr, &box_blocks);
  if (rc != ODTK_OK) return rc;
  std::memset(&qa, 0, sizeof qa);
  qa.n_levels = n_levels; qa.num_anchors = A; qa.num_classes = C; qa.kind = kind;
  qa.alpha = alpha; qa.gamma = gamma;
  const unsigned per = dtype == ODTK_F32 ? 4u : 8u, unroll = dtype == ODTK_F32 ? 2u : 1u;
  const unsigned long long cap = 256ull * (backward && dtype == ODTK_F32 ? 8 : 4);
  unsigned long long total = 0;
  for (int l = 0; l < n_levels; ++l) {
    const odtk_loss_level_t &lv = levels[l];
    odtk::QualityLevel &ql = qa.lv[l];
    const unsigned long long n = 1ull * ba.lv[l].cells * C;
    if (n >= (1ull << 32)) return ODTK_ERR_INVALID;              // the walk indexes the logits with 32 bits
    if (pointers) {
      if (!lv.cls || (backward && !lv.dcls)) return ODTK_ERR_INVALID;
      if ((reinterpret_cast<uintptr_t>(lv.cls) | (backward ? reinterpret_cast<uintptr_t>(lv.dcls) : 0u)) & 15u) return ODTK_ERR_INVALID;   // 16-B vectors
    }
    ql.b = ba.lv[l];
    ql.b.g = (backward && g) ? g + l : nullptr;
    ql.cls = lv.cls;
    ql.dcls = backward ? lv.dcls : nullptr;
    ql.n = static_cast<uint32_t>(n);
    ql.by_channels = odtk::fastdiv_make(static_cast<uint32_t>(A) * C);
    ql.by_classes = odtk::fastdiv_make(C);
    unsigned long long blocks = (n / per + odtk::kQualityThreads * unroll * 2ull - 1) / (odtk::kQualityThreads * unroll * 2ull);
    if (blocks < 1) blocks = 1;
    if (blocks > cap) blocks = cap;
    qa.block_begin[l] = static_cast<uint32_t>(total);
    total += blocks;
  }
  for (int l = n_levels; l <= ODTK_MAX_LEVELS; ++l) qa.block_begin[l] = static_cast<uint32_t>(total);
  *total_blocks = static_cast<unsigned>(total);
  return ODTK_OK;
}

template <bool kBackward>
void quality_dispatch(int dtype, const odtk::QualityArgs &qa, unsigned total, hipStream_t stream) {
  const dim3 grid(total), block(odtk::kQualityThreads);
  if (dtype == ODTK_F32) timed_launch(ODTK_KERNEL_LOSS, odtk::quality_loss_kernel<odtk::F32, kBackward, 2>, grid, block, 0, stream, qa);
  else if (dtype == ODTK_BF16) timed_launch(ODTK_KERNEL_LOSS, odtk::quality_loss_kernel<odtk::BF16, kBackward, 1>, grid, block, 0, stream, qa);
  else timed_launch(ODTK_KERNEL_LOSS, odtk::quality_loss_kernel<odtk::F16, kBackward, 1>, grid, block, 0, stream, qa);
}

// The walk of a per-cell box loss (csrc/cell_loss.hpp) with the policy `Loss`: one lane per anchor cell, either direction.
template <typename Loss, bool kBackward>
void box_loss_dispatch(int dtype, const odtk::CellLossArgs &ba, unsigned total, hipStream_t stream) {
  dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if constexpr (kBackward)
      timed_launch(ODTK_KERNEL_LOSS, odtk::cell_loss_backward_kernel<T, Loss>, dim3(total), dim3(odtk::kCellLossThreads), 0, stream, ba);
    else
      timed_launch(ODTK_KERNEL_LOSS, odtk::cell_loss_forward_kernel<T, Loss>, dim3(total), dim3(odtk::kCellLossThreads), 0, stream, ba);
  });
}

// The forward of odtk_{box_iou,rotated_box,quality}_loss_levels_*: `rc` and `args` are what the family's validator (box_iou_fill /
// quality_fill) returned and filled for a walk of `total` workgroups.  Two-phase: without a workspace, the bytes the workgroups'
// pairs need; with one, walk(stream) and then the fixed-order sum of every level's pairs into `sums`.
template <typename Args, typename Walk>
int cell_loss_levels_forward(int rc, Args &args, unsigned total, int n_levels, double *sums, void *workspace, size_t workspace_size,
                             int too_small,   // ODTK_ERR_INVALID for the box losses: their code predates the use of ODTK_ERR_WORKSPACE and is ABI
                             hipStream_t stream, Walk walk) {
  if (rc != ODTK_OK) return rc;
  const size_t need = align_up(static_cast<size_t>(total) * 2 * sizeof(double));
  if (!workspace) return static_cast<int>(need);                       // two-phase convention of the reference's plugins
  if (workspace_size < need) return too_small;
  if (!sums || ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(sums)) & 7u)) return ODTK_ERR_INVALID;
  args.partial = static_cast<double *>(workspace);
  walk(stream);
  ODTK_HIP_TRY(hipGetLastError());
  odtk::LevelPairReduceArgs ra;
  std::memset(&ra, 0, sizeof ra);
  ra.partial = args.partial;
  ra.sums = sums;
  for (int l = 0; l <= ODTK_MAX_LEVELS; ++l) ra.block_begin[l] = args.block_begin[l];
  timed_launch(ODTK_KERNEL_LOSS_REDUCE, odtk::level_pair_reduce_kernel, dim3(n_levels), dim3(odtk::kCellLossThreads), 0, stream, ra);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

// The backward of the same entry points: the validator's verdict, the upstream gradients' alignment, one launch.
template <typename Walk>
int cell_loss_levels_backward(int rc, const float *grad_sums, Walk walk) {
  if (rc != ODTK_OK) return rc;
  if (reinterpret_cast<uintptr_t>(grad_sums) & 3u) return ODTK_ERR_INVALID;
  walk();
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

// The kernel arguments of odtk_optim_sgd_step / odtk_optim_grad_norm* (csrc/optim.hpp) from the ABI's tensor list: the prefix table of
// the chunks and the alignment bit of every tensor.  `norm`: only grad and numel of a descriptor count.
int optim_fill(odtk::OptimArgs &oa, int n_tensors, const odtk_optim_tensor_t *tensors, bool norm, unsigned *total_blocks) {
  if (n_tensors < 1 || n_tensors > ODTK_MAX_OPTIM_TENSORS || !tensors) return ODTK_ERR_INVALID;
  std::memset(&oa, 0, sizeof oa);
  oa.n_tensors = static_cast<uint32_t>(n_tensors);
  unsigned long long total = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const odtk_optim_tensor_t &t = tensors[i];
    if (t.numel < 0) return ODTK_ERR_INVALID;
    const uintptr_t all = reinterpret_cast<uintptr_t>(t.grad) |
                          (norm ? 0u : reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.momentum) | reinterpret_cast<uintptr_t>(t.ema));
    if (t.numel > 0 && (!t.grad || (!norm && (!t.param || !t.momentum)))) return ODTK_ERR_INVALID;
    if (all & 3u) return ODTK_ERR_INVALID;
    oa.t[i] = t;
    if (!(all & 15u)) oa.vec_mask |= 1ull << i;
    oa.block_begin[i] = static_cast<uint32_t>(total);
    total += (static_cast<unsigned long long>(t.numel) + ODTK_OPTIM_CHUNK - 1) / ODTK_OPTIM_CHUNK;
    if (total > 0x7fffffffull) return ODTK_ERR_INVALID;
  }
  for (int i = n_tensors; i <= ODTK_MAX_OPTIM_TENSORS; ++i) oa.block_begin[i] = static_cast<uint32_t>(total);
  *total_blocks = static_cast<unsigned>(total);
  return ODTK_OK;
}

}  // namespace

extern "C" {

int odtk_debug_loss_tuning(int which, int fp32_heads, int threads, int blocks_per_cu, int unroll, int box_blocks) {
  if (which < 0 || which > 2 || threads < 64 || threads > odtk::kLossMaxThreads || threads % 64 || blocks_per_cu < 1 ||
      blocks_per_cu > 64 || (unroll != 1 && unroll != 2 && unroll != 4) || box_blocks < 1 || box_blocks > 16384)
    return ODTK_ERR_INVALID;
  std::lock_guard<std::mutex> lock(g_loss_tuning_mu);
  LossTuning &t = g_loss_tuning[fp32_heads != 0][which];
  t.threads = threads; t.per_cu = blocks_per_cu; t.unroll = unroll; t.box_blocks = box_blocks;   // (the layout switches stay)
  return ODTK_OK;
}

int odtk_debug_loss_layout(int which, int fp32_heads, int per_wave, int window, int box_rows) {
  if (which < 0 || which > 2 || (per_wave != 0 && per_wave != 1) || (window != 0 && window != 1) || (box_rows != 0 && box_rows != 1))
    return ODTK_ERR_INVALID;
  if (per_wave && which != kLossFwdWs) return ODTK_ERR_INVALID;   // per-wave sums exist in the workspace form only
  std::lock_guard<std::mutex> lock(g_loss_tuning_mu);
  LossTuning &t = g_loss_tuning[fp32_heads != 0][which];
  t.per_wave = per_wave; t.window = window; t.box_rows = box_rows;
  return ODTK_OK;
}

int odtk_debug_loss_tuning_get(int which, int fp32_heads, int out[7]) {
  if (which < 0 || which > 2 || !out) return ODTK_ERR_INVALID;
  std::lock_guard<std::mutex> lock(g_loss_tuning_mu);
  const LossTuning &t = g_loss_tuning[fp32_heads != 0][which];
  out[0] = t.threads; out[1] = t.per_cu; out[2] = t.unroll; out[3] = t.box_blocks;
  out[4] = t.per_wave; out[5] = t.window; out[6] = t.box_rows;
  return ODTK_OK;
}

int odtk_debug_loss_form_get(void) {
  std::lock_guard<std::mutex> lock(g_loss_tuning_mu);
  return g_loss_form;
}

int odtk_debug_loss_form(int form) {
#ifdef ODTK_LOSS_ABLATIONS
  if (form < 0 || form > 7 || form == 5) return ODTK_ERR_INVALID;
#else
  if (form != 0 && form != 1) return ODTK_ERR_INVALID;   // the ablation forms (wrong sums on purpose) are not compiled in
#endif
  std::lock_guard<std::mutex> lock(g_loss_tuning_mu);
  g_loss_form = form;
  return ODTK_OK;
}

int odtk_snap_to_anchors(int batch_size, const float *targets, int n_max, const float *anchors, int num_anchors,
                         int num_classes, int height, int width, int stride, float iou_background,
                         float iou_foreground, float *cls_target, float *box_target, float *depth, void *stream) {
  if (batch_size <= 0 || n_max < 0 || num_anchors <= 0 || num_anchors > ODTK_MAX_ANCHORS || num_classes <= 0 ||
      height <= 0 || width <= 0)
    return ODTK_ERR_INVALID;
  if (!anchors || !box_target || !depth || (n_max > 0 && !targets)) return ODTK_ERR_INVALID;   // cls_target may be null
  const long long cells = 1ll * num_anchors * height * width;
  if (cells > 0x7fffffffll) return ODTK_ERR_INVALID;        // the kernel indexes cells with int
  odtk::SnapArgs sa;
  std::memset(&sa, 0, sizeof sa);
  sa.targets = targets;
  sa.cls_target = cls_target;
  sa.box_target = box_target;
  sa.depth = depth;
  sa.n_max = n_max;
  sa.num_anchors = num_anchors;
  sa.num_classes = num_classes;
  sa.height = height;
  sa.width = width;
  sa.stride = static_cast<float>(stride);
  sa.iou_bg = iou_background;
  sa.iou_fg = iou_foreground;
  std::memcpy(sa.anchors, anchors, sizeof(float) * 4 * num_anchors);
  const unsigned blocks = static_cast<unsigned>((cells + odtk::kSnapThreads - 1) / odtk::kSnapThreads);
  {
    KernelTimer t(ODTK_KERNEL_TARGETS, static_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(odtk::snap_to_anchors_kernel, dim3(blocks, batch_size), dim3(odtk::kSnapThreads), 0,
                       static_cast<hipStream_t>(stream), sa);
  }
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

int odtk_snap_to_anchors_levels(int batch_size, const float *targets, int n_max, int n_levels,
                                const odtk_snap_level_t *levels, int num_anchors, int num_classes,
                                float iou_background, float iou_foreground, void *stream) {
  if (batch_size <= 0 || n_max < 0 || n_levels <= 0 || n_levels > ODTK_MAX_LEVELS || !levels || num_anchors <= 0 ||
      num_anchors > ODTK_MAX_ANCHORS || num_classes <= 0 || (n_max > 0 && !targets))
    return ODTK_ERR_INVALID;
  odtk::SnapLevelsArgs la;
  std::memset(&la, 0, sizeof la);
  la.n_levels = n_levels;
  unsigned total = 0;
  for (int l = 0; l < n_levels; ++l) {
    const odtk_snap_level_t &lv = levels[l];
    if (!lv.anchors || !lv.box_target || !lv.depth || lv.height <= 0 || lv.width <= 0) return ODTK_ERR_INVALID;
    odtk::SnapArgs &sa = la.lv[l];
    sa.targets = targets;
    sa.cls_target = lv.cls_target;
    sa.box_target = lv.box_target;
    sa.depth = lv.depth;
    sa.n_max = n_max;
    sa.num_anchors = num_anchors;
    sa.num_classes = num_classes;
    sa.height = lv.height;
    sa.width = lv.width;
    sa.stride = static_cast<float>(lv.stride);
    sa.iou_bg = iou_background;
    sa.iou_fg = iou_foreground;
    std::memcpy(sa.anchors, lv.anchors, sizeof(float) * 4 * num_anchors);
    la.block_begin[l] = total;
    const long long cells = 1ll * num_anchors * lv.height * lv.width;
    if (cells > 0x7fffffffll) return ODTK_ERR_INVALID;
    total += static_cast<unsigned>((cells + odtk::kSnapThreads - 1) / odtk::kSnapThreads);
  }
  for (int l = n_levels; l <= ODTK_MAX_LEVELS; ++l) la.block_begin[l] = total;
  timed_launch(ODTK_KERNEL_TARGETS, odtk::snap_to_anchors_levels_kernel, dim3(total, batch_size), dim3(odtk::kSnapThreads), 0,
               static_cast<hipStream_t>(stream), la);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

int odtk_snap_to_anchors_rotated_levels(int batch_size, const float *gt_axis, const float *gt_quads, const float *gt_class,
                                        int n_max, int n_levels, const odtk_snap_rot_level_t *levels, int num_anchors,
                                        int num_classes, float iou_background, float iou_foreground, void *stream) {
  if (batch_size <= 0 || n_max < 0 || n_levels <= 0 || n_levels > ODTK_MAX_LEVELS || !levels || num_anchors <= 0 ||
      num_classes <= 0 || (n_max > 0 && (!gt_axis || !gt_quads || !gt_class)))
    return ODTK_ERR_INVALID;
  odtk::SnapRotLevelsArgs la;
  std::memset(&la, 0, sizeof la);
  la.n_levels = n_levels;
  unsigned total = 0;
  for (int l = 0; l < n_levels; ++l) {
    const odtk_snap_rot_level_t &lv = levels[l];
    if (!lv.anchors_axis || !lv.anchors_quads || !lv.box_target || !lv.depth || lv.height <= 0 || lv.width <= 0) return ODTK_ERR_INVALID;
    odtk::SnapRotArgs &sa = la.lv[l];
    sa.gt_axis = gt_axis; sa.gt_quads = gt_quads; sa.gt_class = gt_class;
    sa.anchors_axis = lv.anchors_axis; sa.anchors_rot = lv.anchors_quads;
    sa.cls_target = lv.cls_target; sa.box_target = lv.box_target; sa.depth = lv.depth;
    sa.n_max = n_max; sa.num_anchors = num_anchors; sa.num_classes = num_classes;
    sa.height = lv.height; sa.width = lv.width;
    sa.stride = static_cast<float>(lv.stride);
    sa.iou_bg = iou_background; sa.iou_fg = iou_foreground;
    la.block_begin[l] = total;
    const long long cells = 1ll * num_anchors * lv.height * lv.width;
    if (cells > 0x7fffffffll) return ODTK_ERR_INVALID;
    total += static_cast<unsigned>((cells + odtk::kSnapThreads - 1) / odtk::kSnapThreads);
  }
  for (int l = n_levels; l <= ODTK_MAX_LEVELS; ++l) la.block_begin[l] = total;
  timed_launch(ODTK_KERNEL_TARGETS, odtk::snap_to_anchors_rotated_levels_kernel, dim3(total, batch_size), dim3(odtk::kSnapThreads), 0,
               static_cast<hipStream_t>(stream), la);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

int odtk_atss_assign_levels(int batch_size, const float *targets, int n_max, int n_levels, const odtk_snap_level_t *levels,
                            int num_anchors, int num_classes, int topk, void *workspace, size_t workspace_size, void *stream) {
  // grid.y carries the image in both launches
  if (batch_size <= 0 || batch_size > 65535 || n_max < 0 || n_levels <= 0 || n_levels > ODTK_MAX_LEVELS || num_anchors <= 0 ||
      num_anchors > ODTK_MAX_ANCHORS || num_classes <= 0 || topk < 1 || topk > ODTK_ATSS_MAX_TOPK)
    return ODTK_ERR_INVALID;
  const unsigned long long rows = 1ull * batch_size * n_max * n_levels;     // one record per image, level and target row
  if (rows * sizeof(odtk::AtssRecord) > 0x7fffff00ull) return ODTK_ERR_INVALID;      // the size query answers in an int
  const size_t need = align_up(rows ? rows * sizeof(odtk::AtssRecord) : 1);
  if (!workspace) return static_cast<int>(need);                                      // two-phase convention of the reference's plugins
  if (workspace_size < need) return ODTK_ERR_WORKSPACE;
  if (!levels || (n_max > 0 && !targets) || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return ODTK_ERR_INVALID;
  odtk::AtssArgs aa;
  std::memset(&aa, 0, sizeof aa);
  aa.targets = targets;
  aa.records = static_cast<odtk::AtssRecord *>(workspace);
  aa.by_anchors = odtk::fastdiv_make(num_anchors);
  aa.n_levels = n_levels;
  aa.n_max = n_max;
  aa.num_anchors = num_anchors;
  aa.num_classes = num_classes;
  aa.topk = topk;
  unsigned long long total = 0;
  for (int l = 0; l < n_levels; ++l) {
    const odtk_snap_level_t &lv = levels[l];
    if (!lv.anchors || !lv.box_target || !lv.depth || lv.height <= 0 || lv.width <= 0 || lv.stride <= 0) return ODTK_ERR_INVALID;
    const long long cells = 1ll * num_anchors * lv.height * lv.width;
    if (cells > 0x7fffffffll) return ODTK_ERR_INVALID;        // the kernels index cells with int
    odtk::AtssLevel &al = aa.lv[l];
    al.cls_target = lv.cls_target;
    al.box_target = lv.box_target;
    al.depth = lv.depth;
    al.height = lv.height;
    al.width = lv.width;
    al.stride = static_cast<float>(lv.stride);
    al.by_width = odtk::fastdiv_make(static_cast<uint32_t>(lv.width));
    std::memcpy(al.anchors, lv.anchors, sizeof(float) * 4 * num_anchors);
    aa.block_begin[l] = static_cast<uint32_t>(total);
    total += static_cast<unsigned long long>((cells + odtk::kAtssThreads - 1) / odtk::kAtssThreads);
  }
  if (total > 0x7fffffffull) return ODTK_ERR_INVALID;
  for (int l = n_levels; l <= ODTK_MAX_LEVELS; ++l) aa.block_begin[l] = static_cast<uint32_t>(total);
  if (n_max > 0) {
    timed_launch(ODTK_KERNEL_ATSS_STATS, odtk::atss_stats_kernel, dim3(n_max, batch_size), dim3(odtk::kWave), 0,
                 static_cast<hipStream_t>(stream), aa);
    ODTK_HIP_TRY(hipGetLastError());
  }
  timed_launch(ODTK_KERNEL_TARGETS, odtk::atss_assign_kernel, dim3(static_cast<unsigned>(total), batch_size), dim3(odtk::kAtssThreads), 0,
               static_cast<hipStream_t>(stream), aa);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

int odtk_tal_assign_levels(int batch_size, const float *targets, int n_max, int n_levels, const odtk_snap_level_t *levels,
                           const odtk_loss_level_t *heads, int num_anchors, int num_classes, int dtype, int topk, int alpha, int beta,
                           void *workspace, size_t workspace_size, void *stream) {
  // grid.y carries the image in the selection and the scatter
  if (batch_size <= 0 || batch_size > 65535 || n_max < 0 || n_levels <= 0 || n_levels > ODTK_MAX_LEVELS || num_anchors <= 0 ||
      num_anchors > ODTK_MAX_ANCHORS || num_classes < 1 || topk < 1 || topk > ODTK_ATSS_MAX_TOPK || alpha < 0 || alpha > 4 || beta < 1 ||
      beta > 8)
    return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  const unsigned long long rows = 1ull * batch_size * n_max;                  // one record per image and target row
  if (rows * sizeof(odtk::TalRecord) > 0x7fffff00ull) return ODTK_ERR_INVALID;        // the size query answers in an int
  const size_t need = align_up(rows ? rows * sizeof(odtk::TalRecord) : 1);
  if (!workspace) return static_cast<int>(need);                                      // two-phase convention of the reference's plugins
  if (workspace_size < need) return ODTK_ERR_WORKSPACE;
  if (!levels || !heads || (n_max > 0 && !targets) || (reinterpret_cast<uintptr_t>(workspace) & 15u) ||
      (reinterpret_cast<uintptr_t>(targets) & 3u))
    return ODTK_ERR_INVALID;
  odtk::TalArgs ta;
  odtk::TalFillArgs fa;
  std::memset(&ta, 0, sizeof ta);
  std::memset(&fa, 0, sizeof fa);
  ta.targets = targets;
  ta.records = static_cast<odtk::TalRecord *>(workspace);
  ta.n_levels = n_levels;
  ta.n_max = n_max;
  ta.num_anchors = num_anchors;
  ta.num_classes = num_classes;
  ta.topk = topk;
  ta.alpha = alpha;
  ta.beta = beta;
  const uintptr_t element = dtype == ODTK_F32 ? 3u : 1u;
  unsigned long long anchors_total = 0, fill_blocks = 0;
  for (int l = 0; l < n_levels; ++l) {
    const odtk_snap_level_t &lv = levels[l];
    const odtk_loss_level_t &hd = heads[l];
    if (!lv.anchors || !lv.box_target || !lv.depth || !hd.cls || !hd.box || lv.height <= 0 || lv.width <= 0 || lv.stride <= 0 ||
        (hd.channels_last != 0 && hd.channels_last != 1))
      return ODTK_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(hd.cls) | reinterpret_cast<uintptr_t>(hd.box)) & element) return ODTK_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(lv.box_target) | reinterpret_cast<uintptr_t>(lv.depth) | reinterpret_cast<uintptr_t>(lv.cls_target)) & 3u)
      return ODTK_ERR_INVALID;
    const unsigned long long pixels = 1ull * lv.height * lv.width;
    if (pixels > 0x7fffffffull || pixels * num_anchors > 0x7fffffffull) return ODTK_ERR_INVALID;   // the kernels index a level's anchors with 32 bits
    const unsigned long long cells = pixels * num_anchors;
    odtk::TalLevel &tl = ta.lv[l];
    tl.cls = hd.cls;
    tl.box = hd.box;
    tl.cls_target = lv.cls_target;
    tl.box_target = lv.box_target;
    tl.depth = lv.depth;
    tl.height = lv.height;
    tl.width = lv.width;
    tl.stride = static_cast<float>(lv.stride);
    tl.channels_last = hd.channels_last;
    tl.base = static_cast<uint32_t>(anchors_total);
    std::memcpy(tl.anchors, lv.anchors, sizeof(float) * 4 * num_anchors);
    anchors_total += cells;
    if (anchors_total > 0x7fffffffull) return ODTK_ERR_INVALID;                       // g, the global anchor index, has 31 bits
    // the fill: depth, box_target and cls_target of the level, at most four vectors per lane and 4096 workgroups per segment
    float *const out[3] = {lv.depth, lv.box_target, lv.cls_target};
    const unsigned long long per[3] = {1ull, 4ull, static_cast<unsigned long long>(num_classes)};
    for (int k = 0; k < 3; ++k) {
      if (!out[k]) continue;
      if (per[k] > (1ull << 62) / (batch_size * cells)) return ODTK_ERR_INVALID;      // an output no address space holds
      const unsigned long long count = batch_size * cells * per[k];
      unsigned long long blocks = (count / 4 + 4ull * odtk::kTalFillThreads - 1) / (4ull * odtk::kTalFillThreads);
      blocks = blocks < 1 ? 1 : blocks > 4096 ? 4096 : blocks;
      fa.ptr[fa.n_segments] = out[k];
      fa.count[fa.n_segments] = count;
      fa.block_begin[fa.n_segments] = static_cast<uint32_t>(fill_blocks);
      fill_blocks += blocks;
      ++fa.n_segments;
    }
  }
  for (int s = fa.n_segments; s <= odtk::kTalFillSegments; ++s) fa.block_begin[s] = static_cast<uint32_t>(fill_blocks);
  if (n_max > 0) {
    dispatch_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      timed_launch(ODTK_KERNEL_ATSS_STATS, odtk::tal_select_kernel<T>, dim3(n_max, batch_size), dim3(odtk::kTalThreads), 0,
                   static_cast<hipStream_t>(stream), ta);
    });
    ODTK_HIP_TRY(hipGetLastError());
  }
  timed_launch(ODTK_KERNEL_TARGETS, odtk::tal_fill_kernel, dim3(static_cast<unsigned>(fill_blocks)), dim3(odtk::kTalFillThreads), 0,
               static_cast<hipStream_t>(stream), fa);
  ODTK_HIP_TRY(hipGetLastError());
  if (n_max > 0) {
    const unsigned blocks = static_cast<unsigned>((1ull * n_max * ODTK_ATSS_MAX_TOPK + odtk::kTalScatterThreads - 1) / odtk::kTalScatterThreads);
    timed_launch(ODTK_KERNEL_TARGETS, odtk::tal_scatter_kernel, dim3(blocks, batch_size), dim3(odtk::kTalScatterThreads), 0,
                 static_cast<hipStream_t>(stream), ta);
    ODTK_HIP_TRY(hipGetLastError());
  }
  return ODTK_OK;
}

int odtk_retina_loss_forward(const void *cls, const void *box, const float *depth, const float *box_target,
                             int batch_size, int num_anchors, int num_classes, int height, int width, int box_params,
                             int dtype, int channels_last, float alpha, float gamma, float beta, double *sums,
                             void *stream) {
  if (!sums) return ODTK_ERR_INVALID;
  ODTK_HIP_TRY(hipMemsetAsync(sums, 0, 3 * sizeof(double), static_cast<hipStream_t>(stream)));
  return retina_loss_launch(false, cls, box, depth, box_target, batch_size, num_anchors, num_classes, height, width,
                            box_params, dtype, channels_last, alpha, gamma, beta, sums, nullptr, nullptr, nullptr, nullptr,
                            static_cast<hipStream_t>(stream));
}

int odtk_retina_loss_backward(const void *cls, const void *box, const float *depth, const float *box_target,
                              int batch_size, int num_anchors, int num_classes, int height, int width, int box_params,
                              int dtype, int channels_last, float alpha, float gamma, float beta,
                              const float *grad_cls_sum, const float *grad_box_sum, void *dcls, void *dbox,
                              void *stream) {
  if (!dcls || !dbox) return ODTK_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(dcls) | reinterpret_cast<uintptr_t>(dbox)) & 15u) return ODTK_ERR_INVALID;
  return retina_loss_launch(true, cls, box, depth, box_target, batch_size, num_anchors, num_classes, height, width,
                            box_params, dtype, channels_last, alpha, gamma, beta, nullptr, grad_cls_sum, grad_box_sum, dcls,
                            dbox, static_cast<hipStream_t>(stream));
}

int odtk_retina_loss_levels_forward(int n_levels, const odtk_loss_level_t *levels, int batch_size, int num_anchors,
                                    int num_classes, int box_params, int dtype, float alpha, float gamma, float beta,
                                    double *sums, void *stream) {
  if (!sums || n_levels <= 0 || n_levels > ODTK_MAX_LEVELS) return ODTK_ERR_INVALID;
  ODTK_HIP_TRY(hipMemsetAsync(sums, 0, 3 * sizeof(double) * n_levels, static_cast<hipStream_t>(stream)));
  return retina_loss_levels_launch(kLossFwd, n_levels, levels, batch_size, num_anchors, num_classes, box_params, dtype, alpha,
                                   gamma, beta, sums, nullptr, nullptr, nullptr, false, static_cast<hipStream_t>(stream));
}

int odtk_retina_loss_levels_forward_ws(int n_levels, const odtk_loss_level_t *levels, int batch_size, int num_anchors,
                                       int num_classes, int box_params, int dtype, float alpha, float gamma, float beta,
                                       double *sums, void *workspace, size_t workspace_size, void *stream) {
  if (n_levels <= 0 || n_levels > ODTK_MAX_LEVELS) return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  const LossTuning t = loss_tuning_snapshot(dtype, kLossFwdWs);
  const int blocks = retina_loss_levels_launch(kLossFwdWs, n_levels, levels, batch_size, num_anchors, num_classes, box_params,
                                               dtype, alpha, gamma, beta, nullptr, nullptr, nullptr, nullptr, true, nullptr, &t);
  if (blocks < 0) return blocks;
  const size_t need = (static_cast<size_t>(blocks) * (t.per_wave ? t.threads / 64 : 1) * 3 * sizeof(double) + 255) & ~static_cast<size_t>(255);
  if (!workspace) return static_cast<int>(need);                       // two-phase convention of the reference's plugins
  if (!sums) return ODTK_ERR_INVALID;
  if (workspace_size < need) return ODTK_ERR_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 7u) return ODTK_ERR_INVALID;
  return retina_loss_levels_launch(kLossFwdWs, n_levels, levels, batch_size, num_anchors, num_classes, box_params, dtype, alpha,
                                   gamma, beta, sums, nullptr, nullptr, static_cast<double *>(workspace), false,
                                   static_cast<hipStream_t>(stream), &t);
}

int odtk_retina_loss_levels_backward(int n_levels, const odtk_loss_level_t *levels, int batch_size, int num_anchors,
                                     int num_classes, int box_params, int dtype, float alpha, float gamma, float beta,
                                     const float *grad_cls_sums, const float *grad_box_sums, void *stream) {
  return retina_loss_levels_launch(kLossBwd, n_levels, levels, batch_size, num_anchors, num_classes, box_params, dtype, alpha,
                                   gamma, beta, nullptr, grad_cls_sums, grad_box_sums, nullptr, false, static_cast<hipStream_t>(stream));
}

int odtk_box_iou_loss_levels_forward(int n_levels, const odtk_loss_level_t *levels, const float *const *anchors, int batch_size,
                                     int num_anchors, int dtype, int kind, double *sums, void *workspace, size_t workspace_size,
                                     void *stream) {
  odtk::CellLossArgs ba;
  unsigned total = 0;
  const int rc = box_iou_fill(ba, false, workspace != nullptr, n_levels, levels, anchors, batch_size, num_anchors, dtype, kind, nullptr, &total);
  return cell_loss_levels_forward(rc, ba, total, n_levels, sums, workspace, workspace_size, ODTK_ERR_INVALID, static_cast<hipStream_t>(stream),
                                  [&](hipStream_t s) { box_loss_dispatch<odtk::BoxIouLoss, false>(dtype, ba, total, s); });
}

int odtk_box_iou_loss_levels_backward(int n_levels, const odtk_loss_level_t *levels, const float *const *anchors, int batch_size,
                                      int num_anchors, int dtype, int kind, const float *grad_sums, void *stream) {
  odtk::CellLossArgs ba;
  unsigned total = 0;
  const int rc = box_iou_fill(ba, true, true, n_levels, levels, anchors, batch_size, num_anchors, dtype, kind, grad_sums, &total);
  return cell_loss_levels_backward(rc, grad_sums, [&] { box_loss_dispatch<odtk::BoxIouLoss, true>(dtype, ba, total, static_cast<hipStream_t>(stream)); });
}

int odtk_quality_loss_levels_forward(int n_levels, const odtk_loss_level_t *levels, const float *const *anchors, int batch_size,
                                     int num_anchors, int num_classes, int dtype, int kind, float alpha, float gamma, double *sums,
                                     void *workspace, size_t workspace_size, void *stream) {
  odtk::QualityArgs qa;
  unsigned total = 0;
  const int rc = quality_fill(qa, false, workspace != nullptr, n_levels, levels, anchors, batch_size, num_anchors, num_classes, dtype,
                              kind, alpha, gamma, nullptr, &total);
  return cell_loss_levels_forward(rc, qa, total, n_levels, sums, workspace, workspace_size, ODTK_ERR_WORKSPACE, static_cast<hipStream_t>(stream),
                                  [&](hipStream_t s) { quality_dispatch<false>(dtype, qa, total, s); });
}

int odtk_quality_loss_levels_backward(int n_levels, const odtk_loss_level_t *levels, const float *const *anchors, int batch_size,
                                      int num_anchors, int num_classes, int dtype, int kind, float alpha, float gamma,
                                      const float *grad_sums, void *stream) {
  odtk::QualityArgs qa;
  unsigned total = 0;
  const int rc = quality_fill(qa, true, true, n_levels, levels, anchors, batch_size, num_anchors, num_classes, dtype, kind, alpha, gamma,
                              grad_sums, &total);
  return cell_loss_levels_backward(rc, grad_sums, [&] { quality_dispatch<true>(dtype, qa, total, static_cast<hipStream_t>(stream)); });
}

int odtk_rotated_box_loss_levels_forward(int n_levels, const odtk_loss_level_t *levels, const float *const *anchors, int batch_size,
                                         int num_anchors, int dtype, int kind, double *sums, void *workspace, size_t workspace_size,
                                         void *stream) {
  odtk::CellLossArgs ba;
  unsigned total = 0;
  const int rc = box_iou_fill(ba, false, workspace != nullptr, n_levels, levels, anchors, batch_size, num_anchors, dtype, kind, nullptr,
                              &total, 6);
  return cell_loss_levels_forward(rc, ba, total, n_levels, sums, workspace, workspace_size, ODTK_ERR_INVALID, static_cast<hipStream_t>(stream),
                                  [&](hipStream_t s) { box_loss_dispatch<odtk::RotatedBoxLoss, false>(dtype, ba, total, s); });
}

int odtk_rotated_box_loss_levels_backward(int n_levels, const odtk_loss_level_t *levels, const float *const *anchors, int batch_size,
                                          int num_anchors, int dtype, int kind, const float *grad_sums, void *stream) {
  odtk::CellLossArgs ba;
  unsigned total = 0;
  const int rc = box_iou_fill(ba, true, true, n_levels, levels, anchors, batch_size, num_anchors, dtype, kind, grad_sums, &total, 6);
  return cell_loss_levels_backward(rc, grad_sums, [&] { box_loss_dispatch<odtk::RotatedBoxLoss, true>(dtype, ba, total, static_cast<hipStream_t>(stream)); });
}

int odtk_optim_grad_norm_chained(int n_tensors, const odtk_optim_tensor_t *tensors, const float *grad_scale, float max_norm, void *state,
                                 int prior_slots, int last, void *workspace, size_t workspace_size, void *stream) {
  odtk::OptimArgs oa;
  unsigned total = 0;
  const int rc = optim_fill(oa, n_tensors, tensors, true, &total);
  if (rc != ODTK_OK) return rc;
  if (prior_slots < 0 || (last != 0 && last != 1) || 1ull * prior_slots + total > 0x7fffffffull / sizeof(double)) return ODTK_ERR_INVALID;
  if (last && (!std::isfinite(max_norm) || !(max_norm > 0.0f))) return ODTK_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(grad_scale) & 3u) return ODTK_ERR_INVALID;
  const size_t slots = static_cast<size_t>(prior_slots) + total;
  const size_t need = align_up(slots ? slots * sizeof(double) : 1);
  if (!workspace) return static_cast<int>(need);                       // two-phase convention of the reference's plugins
  if (workspace_size < need) return ODTK_ERR_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 7u) return ODTK_ERR_INVALID;
  if (last && (!state || (reinterpret_cast<uintptr_t>(state) & 3u))) return ODTK_ERR_INVALID;
  oa.grad_scale = grad_scale;
  oa.slots = static_cast<double *>(workspace) + prior_slots;
  if (total) {                                                         // (a list of empty tensors fills no slot)
    timed_launch(ODTK_KERNEL_LOSS_REDUCE, odtk::optim_grad_norm_kernel, dim3(total), dim3(odtk::kOptimThreads), 0,
                 static_cast<hipStream_t>(stream), oa);
    ODTK_HIP_TRY(hipGetLastError());
  }
  if (last) {
    odtk::OptimFinishArgs fa;
    std::memset(&fa, 0, sizeof fa);
    fa.slots = static_cast<const double *>(workspace);
    fa.n_slots = static_cast<uint32_t>(slots);
    fa.max_norm = max_norm;
    fa.state = static_cast<odtk::OptimState *>(state);
    timed_launch(ODTK_KERNEL_LOSS_REDUCE, odtk::optim_grad_norm_finish_kernel, dim3(1), dim3(odtk::kOptimFinishThreads), 0,
                 static_cast<hipStream_t>(stream), fa);
    ODTK_HIP_TRY(hipGetLastError());
  }
  return ODTK_OK;
}

int odtk_optim_grad_norm(int n_tensors, const odtk_optim_tensor_t *tensors, const float *grad_scale, float max_norm, void *state,
                         void *workspace, size_t workspace_size, void *stream) {
  return odtk_optim_grad_norm_chained(n_tensors, tensors, grad_scale, max_norm, state, 0, 1, workspace, workspace_size, stream);
}

int odtk_optim_sgd_step(int n_tensors, const odtk_optim_tensor_t *tensors, float lr, float momentum, float weight_decay, int first,
                        float one_minus_decay, const float *grad_scale, const float *found_inf, const void *norm_state, void *stream) {
  odtk::OptimArgs oa;
  unsigned total = 0;
  const int rc = optim_fill(oa, n_tensors, tensors, false, &total);
  if (rc != ODTK_OK) return rc;
  if (!std::isfinite(lr) || !std::isfinite(momentum) || !std::isfinite(weight_decay) || (first != 0 && first != 1)) return ODTK_ERR_INVALID;
  if (!(one_minus_decay >= 0.0f && one_minus_decay <= 1.0f)) return ODTK_ERR_INVALID;            // (a NaN fails both comparisons)
  if ((reinterpret_cast<uintptr_t>(grad_scale) | reinterpret_cast<uintptr_t>(found_inf) | reinterpret_cast<uintptr_t>(norm_state)) & 3u)
    return ODTK_ERR_INVALID;
  oa.lr = lr; oa.momentum = momentum; oa.wd = weight_decay; oa.one_minus_decay = one_minus_decay;
  oa.first = first;
  oa.grad_scale = grad_scale; oa.found_inf = found_inf;
  oa.norm_state = static_cast<const odtk::OptimState *>(norm_state);
  if (!total) return ODTK_OK;                                          // nothing but empty tensors
  timed_launch(ODTK_KERNEL_EPILOGUE, odtk::optim_sgd_step_kernel, dim3(total), dim3(odtk::kOptimThreads), 0,
               static_cast<hipStream_t>(stream), oa);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

}  // extern "C"
