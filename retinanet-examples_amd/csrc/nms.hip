// nms.hip -- NMS (axis-aligned, rotated staged), Soft-NMS, Matrix NMS, box voting, candidate concatenation, the merge of tiled inference and odtk_iou; nms_impl is what odtk_detect calls (internal.hpp).
#include <cmath>
#include <cstring>

#include "internal.hpp"
#include "iou.hpp"
#include "nms.hpp"
#include "soft_nms.hpp"
#include "matrix_nms.hpp"
#include "box_vote.hpp"
#include "tile.hpp"

namespace {

template <int NB, bool kGlobalKeys, int kStage = 0>
int nms_launch(const odtk::NmsArgs &na, int batch, size_t lds, hipStream_t stream) {
  // opt this kernel in to the full 160 KiB of LDS (once per device)
  const int rc = allow_dynamic_lds(reinterpret_cast<const void *>(&odtk::nms_kernel<NB, kGlobalKeys, kStage>), 160 * 1024,
                                   "hipFuncSetAttribute(nms_kernel)");
  if (rc != ODTK_OK) return rc;
  timed_launch(kStage == 1 ? ODTK_KERNEL_NMS_ORDER : ODTK_KERNEL_NMS, odtk::nms_kernel<NB, kGlobalKeys, kStage>, dim3(batch),
               dim3(odtk::kNmsThreads), lds, stream, na);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

// rotated boxes: first round in order -> pairwise suppression matrix on the whole chip -> resolve (csrc/nms.hpp)
template <bool kGlobalKeys>
int nms_rotated_staged(odtk::NmsArgs na, int batch, size_t lds, hipStream_t stream) {
  int rc = nms_launch<6, kGlobalKeys, 1>(na, batch, lds, stream);
  if (rc != ODTK_OK) return rc;
  odtk::SupArgs sa;
  sa.first_box = na.first_box; sa.first_cls = na.first_cls; sa.first_n = na.first_n; sa.sup = na.sup;
  sa.m_max = na.m_max; sa.thresh = na.thresh; sa.flags = na.flags;
  auto matrix = [&](uint32_t m_launch, uint32_t m_done, const uint32_t *done) {
    sa.m_launch = m_launch; sa.m_done = m_done; sa.done = done;
    const unsigned nblk = m_launch / 64;
    timed_launch(ODTK_KERNEL_NMS_MATRIX, odtk::rotated_sup_matrix_kernel, dim3(nblk * (nblk + 1) / 2 * (64 / odtk::kSupRows), batch),
                 dim3(odtk::kSupThreads), 0, stream, sa);
  };
  if (na.m_first >= na.m_max) {                              // the matrix is small: one step
    na.step = 0;
    matrix(na.m_max, 0, nullptr);
    ODTK_HIP_TRY(hipGetLastError());
    return nms_launch<6, kGlobalKeys, 2>(na, batch, lds, stream);
  }
  // two-step speculation: the pairs of the first m_first candidates, a resolve that stops there; only the images it did not
  // finish pay for the rest of the matrix and a second resolve (the other workgroups of those two launches leave at once)
  matrix(na.m_first, 0, nullptr);
  ODTK_HIP_TRY(hipGetLastError());
  na.step = 1;
  rc = nms_launch<6, kGlobalKeys, 2>(na, batch, lds, stream);
  if (rc != ODTK_OK) return rc;
  matrix(na.m_max, na.m_first, na.done);
  ODTK_HIP_TRY(hipGetLastError());
  na.step = 2;
  return nms_launch<6, kGlobalKeys, 2>(na, batch, lds, stream);
}

// ... and what the first of two matrix launches covers: 2.5 x detections_per_im (a detector whose boxes are well separated
// examines 1.5 .. 2.5 x as many candidates as it keeps), at least four chunks
uint32_t rotated_matrix_first(uint32_t m_max, int ndet) {
  size_t m = static_cast<size_t>(ndet) * 5 / 2;
  if (m < 256) m = 256;
  m = (m + 63) / 64 * 64;
  return m > m_max ? m_max : static_cast<uint32_t>(m);
}

// candidates of the first round the rotated suppression matrix covers: 8 x detections_per_im (the lazy pull of a typical
// image examines 1.5 .. 7 x as many candidates as it keeps), whole 64-candidate chunks, at most one round
// ... and as many as the resolve kernel can hold in LDS: it keeps the matrix (m x m / 64 words) where the polygon clip's
// columns will be once the first pair beyond the matrix is clipped (`ways` x 4 KiB: 704 candidates at 16 ways)
uint32_t rotated_matrix_rows(size_t count, int ndet, int ways) {
  size_t m = static_cast<size_t>(ndet) * 8;
  if (m > count) m = count;
  if (m > static_cast<size_t>(odtk::kNmsRound)) m = odtk::kNmsRound;
  m = (m + 63) / 64 * 64;
  const size_t room = static_cast<size_t>(ways) * odtk::kClipSlotsPerWave * sizeof(float2);
  while (m > 64 && m * (m / 64) * sizeof(uint64_t) > room) m -= 64;
  return static_cast<uint32_t>(m);
}

// Soft-NMS (csrc/soft_nms.hpp): one workgroup per image, boxes and classes in count x 20 bytes of dynamic LDS
template <bool kGaussian>
int soft_nms_launch(const odtk::SoftNmsArgs &sa, int batch, hipStream_t stream) {
  const size_t lds = odtk::soft_nms_lds_bytes(sa.count);
  const int rc = allow_dynamic_lds(reinterpret_cast<const void *>(&odtk::soft_nms_kernel<kGaussian>), odtk::soft_nms_lds_bytes(ODTK_MAX_NMS_COUNT),
                                   "hipFuncSetAttribute(soft_nms_kernel)");
  if (rc != ODTK_OK) return rc;
  timed_launch(ODTK_KERNEL_NMS, odtk::soft_nms_kernel<kGaussian>, dim3(batch), dim3(odtk::kSoftThreads), lds, stream, sa);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

}  // namespace

int nms_impl(int batch, const void *const *inputs, void *const *outputs, int n_outputs, size_t count,
             int ndet, float thresh, uint32_t flags, void *workspace, size_t workspace_size, hipStream_t stream,
             uint32_t sorted_run_len, const uint32_t *run_valid) {
  if (batch <= 0 || count == 0 || count > ODTK_MAX_NMS_COUNT_SCRATCH || ndet <= 0 || ndet > ODTK_MAX_NMS_DETECTIONS)
    return ODTK_ERR_INVALID;
  // up to ODTK_MAX_NMS_COUNT candidates per image everything is LDS-resident and the kernel needs no global scratch
  // (a token size keeps the reference's two-phase calling convention working unchanged); beyond that the key list
  // of every image lives in the workspace
  const int nb = (flags & ODTK_FLAG_ROTATED) ? 6 : 4;
  // ... or when the LDS-resident form does not fit next to a long kept list (detections_per_im in the thousands), or -- rotated
  // -- would leave fewer than 8 of the 16 waves a polygon-clip column (they are what evaluates box pairs)
  const odtk::NmsLds local(static_cast<uint32_t>(count > ODTK_MAX_NMS_COUNT ? 1 : count), ndet, nb, false);
  const bool global_keys = count > ODTK_MAX_NMS_COUNT || local.total > odtk::NmsLds::kLdsBudget || (nb == 6 && local.ways < 8);
  const size_t keys_bytes = global_keys ? align_up(sizeof(uint64_t) * static_cast<size_t>(batch) * count) : kAlign;
  // rotated: [first-round boxes | classes | counts | suppression matrix] behind the keys
  const uint32_t m_max = nb == 6 ? rotated_matrix_rows(count, ndet, odtk::NmsLds(static_cast<uint32_t>(global_keys ? 1 : count), ndet, nb, global_keys).ways) : 0u;
  const size_t off_fb = keys_bytes;
  const size_t off_fc = off_fb + (nb == 6 ? align_up(sizeof(float) * 6 * batch * m_max) : 0);
  const size_t off_fn = off_fc + (nb == 6 ? align_up(sizeof(float) * batch * m_max) : 0);
  const size_t off_fk = off_fn + (nb == 6 ? align_up(sizeof(uint32_t) * batch) : 0);
  const size_t off_fs = off_fk + (nb == 6 ? align_up(sizeof(uint64_t) * batch * odtk::kNmsRound) : 0);
  const size_t off_sup = off_fs + (nb == 6 ? align_up(sizeof(uint32_t) * 16 * batch) : 0);
  const size_t off_done = off_sup + (nb == 6 ? align_up(sizeof(uint64_t) * batch * m_max * (m_max / 64)) : 0);
  const size_t need = off_done + (nb == 6 ? align_up(sizeof(uint32_t) * batch) : 0);
  if (need > 0x7fffffffull) return ODTK_ERR_INVALID;
  if (!workspace || !workspace_size) return static_cast<int>(need);
  if (workspace_size < need) return ODTK_ERR_WORKSPACE;
  if (!inputs || !outputs || n_outputs < 3) return ODTK_ERR_INVALID;
  for (int i = 0; i < 3; ++i)
    if (!inputs[i] || !outputs[i]) return ODTK_ERR_INVALID;
  odtk::NmsArgs na;
  std::memset(&na, 0, sizeof na);
  na.scores = static_cast<const float *>(inputs[0]);
  na.boxes = static_cast<const float *>(inputs[1]);
  na.classes = static_cast<const float *>(inputs[2]);
  na.out_scores = static_cast<float *>(outputs[0]);
  na.out_boxes = static_cast<float *>(outputs[1]);
  na.out_classes = static_cast<float *>(outputs[2]);
  na.out_indices = n_outputs > 3 ? static_cast<int32_t *>(outputs[3]) : nullptr;
  na.count = static_cast<uint32_t>(count);
  na.run_len = sorted_run_len;
  na.run_valid = run_valid;
  na.ndet = ndet;
  na.thresh = thresh;
  na.flags = flags;
  na.batched_push = 1u;
  na.trace = g_trace ? g_trace + 8 * 64 : nullptr;          // after the select_decode slots
  na.key_scratch = global_keys ? static_cast<uint64_t *>(workspace) : nullptr;
  const size_t lds = odtk::NmsLds(na.count, ndet, nb, global_keys).total;   // same carve-up the kernel computes
  if (lds > 160 * 1024) return ODTK_ERR_INVALID;
  if (nb == 6) {
    char *ws = static_cast<char *>(workspace);
    na.first_box = reinterpret_cast<float *>(ws + off_fb);
    na.first_cls = reinterpret_cast<float *>(ws + off_fc);
    na.first_n = reinterpret_cast<uint32_t *>(ws + off_fn);
    na.first_keys = reinterpret_cast<unsigned long long *>(ws + off_fk);
    na.first_state = reinterpret_cast<uint32_t *>(ws + off_fs);
    na.sup = reinterpret_cast<unsigned long long *>(ws + off_sup);
    na.m_max = m_max;
    na.m_first = rotated_matrix_first(m_max, ndet);
    na.done = reinterpret_cast<uint32_t *>(ws + off_done);
    return global_keys ? nms_rotated_staged<true>(na, batch, lds, stream) : nms_rotated_staged<false>(na, batch, lds, stream);
  }
  return global_keys ? nms_launch<4, true>(na, batch, lds, stream) : nms_launch<4, false>(na, batch, lds, stream);
}

extern "C" {

int odtk_nms(int batch_size, const void *const *inputs, void *const *outputs, size_t count,
             int detections_per_im, float nms_thresh, void *workspace, size_t workspace_size, void *stream) {
  return nms_impl(batch_size, inputs, outputs, 3, count, detections_per_im, nms_thresh, 0u, workspace,
                  workspace_size, static_cast<hipStream_t>(stream));
}

int odtk_nms_rotate(int batch_size, const void *const *inputs, void *const *outputs, size_t count,
                    int detections_per_im, float nms_thresh, void *workspace, size_t workspace_size,
                    void *stream) {
  return nms_impl(batch_size, inputs, outputs, 3, count, detections_per_im, nms_thresh, ODTK_FLAG_ROTATED,
                  workspace, workspace_size, static_cast<hipStream_t>(stream));
}

int odtk_nms_ex(int batch_size, const void *const *inputs, void *const *outputs, int n_outputs, size_t count,
                int detections_per_im, float nms_thresh, uint32_t flags, void *workspace,
                size_t workspace_size, void *stream) {
  return nms_impl(batch_size, inputs, outputs, n_outputs, count, detections_per_im, nms_thresh, flags,
                  workspace, workspace_size, static_cast<hipStream_t>(stream));
}

int odtk_nms_sorted_runs(int batch_size, const void *const *inputs, void *const *outputs, int n_outputs, size_t count,
                         int run_len, const uint32_t *run_valid, int detections_per_im, float nms_thresh, uint32_t flags,
                         void *workspace, size_t workspace_size, void *stream) {
  if (run_len <= 0 || count % static_cast<size_t>(run_len) != 0 || count / run_len > 8) return ODTK_ERR_INVALID;
  if (workspace && workspace_size && !run_valid) return ODTK_ERR_INVALID;
  return nms_impl(batch_size, inputs, outputs, n_outputs, count, detections_per_im, nms_thresh, flags, workspace, workspace_size,
                  static_cast<hipStream_t>(stream), static_cast<uint32_t>(run_len), run_valid);
}

// everything is validated here, on the host, before anything touches the device
int odtk_soft_nms(int batch_size, const void *const *inputs, void *const *outputs, int n_outputs, size_t count,
                  int detections_per_im, float nms_thresh, int method, float sigma, float min_score, uint32_t flags,
                  void *workspace, size_t workspace_size, void *stream) {
  if (batch_size <= 0 || count == 0 || detections_per_im <= 0 || detections_per_im > ODTK_MAX_NMS_DETECTIONS) return ODTK_ERR_INVALID;
  if (method != ODTK_SOFT_NMS_LINEAR && method != ODTK_SOFT_NMS_GAUSSIAN) return ODTK_ERR_INVALID;
  if (!std::isfinite(sigma) || !(sigma > 0.0f) || !std::isfinite(min_score) || !(min_score > 0.0f)) return ODTK_ERR_INVALID;
  if (flags & ~(ODTK_FLAG_ROTATED | ODTK_FLAG_LOGITS | ODTK_FLAG_ROTATED_NMS_FIXED_ANGLE)) return ODTK_ERR_INVALID;
  if (flags & ODTK_FLAG_ROTATED) return ODTK_ERR_UNSUPPORTED;
  if (count > ODTK_MAX_NMS_COUNT) return ODTK_ERR_UNSUPPORTED;
  // nothing lives in global scratch: a token size keeps the two-phase calling convention
  const size_t need = kAlign;
  if (!workspace || !workspace_size) return static_cast<int>(need);
  if (workspace_size < need) return ODTK_ERR_WORKSPACE;
  if (!inputs || !outputs || n_outputs < 3) return ODTK_ERR_INVALID;
  for (int i = 0; i < 3; ++i)
    if (!inputs[i] || !outputs[i]) return ODTK_ERR_INVALID;
  odtk::SoftNmsArgs sa;
  std::memset(&sa, 0, sizeof sa);
  sa.scores = static_cast<const float *>(inputs[0]);
  sa.boxes = static_cast<const float *>(inputs[1]);
  sa.classes = static_cast<const float *>(inputs[2]);
  sa.out_scores = static_cast<float *>(outputs[0]);
  sa.out_boxes = static_cast<float *>(outputs[1]);
  sa.out_classes = static_cast<float *>(outputs[2]);
  sa.out_indices = n_outputs > 3 ? static_cast<int32_t *>(outputs[3]) : nullptr;
  sa.count = static_cast<uint32_t>(count);
  sa.ndet = detections_per_im;
  sa.thresh = nms_thresh;
  sa.sigma = sigma;
  sa.min_score = min_score;
  return method == ODTK_SOFT_NMS_GAUSSIAN ? soft_nms_launch<true>(sa, batch_size, static_cast<hipStream_t>(stream))
                                          : soft_nms_launch<false>(sa, batch_size, static_cast<hipStream_t>(stream));
}

// everything is validated here, on the host, before anything touches the device
int odtk_matrix_nms(int batch_size, const void *const *inputs, void *const *outputs, int n_outputs, size_t count,
                    int detections_per_im, int pre_top, int method, float sigma, float min_score, uint32_t flags,
                    void *workspace, size_t workspace_size, void *stream) {
  if (batch_size <= 0 || count == 0 || count > ODTK_MAX_NMS_COUNT_SCRATCH || detections_per_im <= 0 ||
      detections_per_im > ODTK_MAX_NMS_DETECTIONS || pre_top <= 0 || pre_top > ODTK_MAX_MATRIX_NMS_PRE)
    return ODTK_ERR_INVALID;
  if (method != ODTK_MATRIX_NMS_LINEAR && method != ODTK_MATRIX_NMS_GAUSSIAN) return ODTK_ERR_INVALID;
  if (!std::isfinite(sigma) || !(sigma > 0.0f) || !std::isfinite(min_score) || !(min_score > 0.0f)) return ODTK_ERR_INVALID;
  if (flags & ~(ODTK_FLAG_ROTATED | ODTK_FLAG_LOGITS | ODTK_FLAG_ROTATED_NMS_FIXED_ANGLE)) return ODTK_ERR_INVALID;
  if (flags & ODTK_FLAG_ROTATED) return ODTK_ERR_UNSUPPORTED;
  // workspace: [keys of the positive candidates | the participants in rank order: boxes, classes, scores, positions, cmax, decay | n]
  const size_t batch = static_cast<size_t>(batch_size);
  const size_t stride = (static_cast<size_t>(pre_top) + odtk::kMatCols - 1) / odtk::kMatCols * odtk::kMatCols;
  const size_t off_box = align_up(sizeof(uint64_t) * batch * count);
  const size_t off_cls = off_box + align_up(sizeof(float) * 4 * batch * stride);
  const size_t per = align_up(sizeof(float) * batch * stride);
  const size_t off_n = off_cls + 5 * per;
  const size_t need = off_n + align_up(sizeof(uint32_t) * batch);
  if (need > 0x7fffffffull) return ODTK_ERR_INVALID;
  if (!workspace || !workspace_size) return static_cast<int>(need);
  if (workspace_size < need) return ODTK_ERR_WORKSPACE;
  if (!inputs || !outputs || n_outputs < 3) return ODTK_ERR_INVALID;
  for (int i = 0; i < 3; ++i)
    if (!inputs[i] || !outputs[i]) return ODTK_ERR_INVALID;
  odtk::MatrixNmsArgs ma;
  std::memset(&ma, 0, sizeof ma);
  ma.scores = static_cast<const float *>(inputs[0]);
  ma.boxes = static_cast<const float *>(inputs[1]);
  ma.classes = static_cast<const float *>(inputs[2]);
  ma.out_scores = static_cast<float *>(outputs[0]);
  ma.out_boxes = static_cast<float *>(outputs[1]);
  ma.out_classes = static_cast<float *>(outputs[2]);
  ma.out_indices = n_outputs > 3 ? static_cast<int32_t *>(outputs[3]) : nullptr;
  char *ws = static_cast<char *>(workspace);
  ma.keys = reinterpret_cast<unsigned long long *>(ws);
  ma.r_box = reinterpret_cast<float *>(ws + off_box);
  ma.r_cls = reinterpret_cast<float *>(ws + off_cls);
  ma.r_score = reinterpret_cast<float *>(ws + off_cls + per);
  ma.r_pos = reinterpret_cast<uint32_t *>(ws + off_cls + 2 * per);
  ma.r_cmax = reinterpret_cast<uint32_t *>(ws + off_cls + 3 * per);
  ma.r_decay = reinterpret_cast<uint32_t *>(ws + off_cls + 4 * per);
  ma.r_n = reinterpret_cast<uint32_t *>(ws + off_n);
  ma.count = static_cast<uint32_t>(count);
  ma.stride = static_cast<uint32_t>(stride);
  ma.pre_top = static_cast<uint32_t>(pre_top);
  ma.ndet = detections_per_im;
  ma.sigma = sigma;
  ma.min_score = min_score;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // pair tiles: 64 columns x 256 rows; the ones above the diagonal or beyond an image's participants leave at once
  const unsigned tiles = static_cast<unsigned>((stride / odtk::kMatCols) * ((stride + odtk::kMatRows - 1) / odtk::kMatRows));
  const dim3 pair_grid(static_cast<unsigned>(batch_size), tiles), pair_block(odtk::kMatPairThreads);
  timed_launch(ODTK_KERNEL_NMS, odtk::matrix_nms_rank_kernel, dim3(batch_size), dim3(odtk::kMatThreads), 0, s, ma);
  timed_launch(ODTK_KERNEL_NMS, odtk::matrix_nms_pairs_kernel<0>, pair_grid, pair_block, 0, s, ma);
  if (method == ODTK_MATRIX_NMS_GAUSSIAN) timed_launch(ODTK_KERNEL_NMS, odtk::matrix_nms_pairs_kernel<2>, pair_grid, pair_block, 0, s, ma);
  else timed_launch(ODTK_KERNEL_NMS, odtk::matrix_nms_pairs_kernel<1>, pair_grid, pair_block, 0, s, ma);
  timed_launch(ODTK_KERNEL_NMS, odtk::matrix_nms_emit_kernel, dim3(batch_size), dim3(odtk::kMatThreads), 0, s, ma);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

// everything is validated here, on the host, before anything touches the device
int odtk_box_vote(int batch_size, const void *const *inputs, const int32_t *kept, void *out_boxes, size_t count,
                  int detections_per_im, float vote_thresh, uint32_t flags, void *stream) {
  if (batch_size <= 0 || count == 0 || count > ODTK_MAX_NMS_COUNT_SCRATCH || detections_per_im <= 0 ||
      detections_per_im > ODTK_MAX_NMS_DETECTIONS)
    return ODTK_ERR_INVALID;
  if (!std::isfinite(vote_thresh) || !(vote_thresh > 0.0f) || !(vote_thresh <= 1.0f)) return ODTK_ERR_INVALID;
  if (flags & ~(ODTK_FLAG_ROTATED | ODTK_FLAG_LOGITS | ODTK_FLAG_ROTATED_NMS_FIXED_ANGLE)) return ODTK_ERR_INVALID;
  if (!inputs || !inputs[0] || !inputs[1] || !inputs[2] || !kept || !out_boxes) return ODTK_ERR_INVALID;
  if (flags & ODTK_FLAG_ROTATED) return ODTK_ERR_UNSUPPORTED;
  odtk::BoxVoteArgs va;
  std::memset(&va, 0, sizeof va);
  va.scores = static_cast<const float *>(inputs[0]);
  va.boxes = static_cast<const float *>(inputs[1]);
  va.classes = static_cast<const float *>(inputs[2]);
  va.kept = kept;
  va.out_boxes = static_cast<float *>(out_boxes);
  va.count = static_cast<uint32_t>(count);
  va.ndet = detections_per_im;
  va.thresh = vote_thresh;
  const unsigned groups = (static_cast<unsigned>(detections_per_im) + odtk::kVoteWaves - 1) / odtk::kVoteWaves;
  const int per_launch = 65535;                                  // images per launch: the grid's y extent
  for (int first = 0; first < batch_size; first += per_launch) {
    const int n = batch_size - first < per_launch ? batch_size - first : per_launch;
    odtk::BoxVoteArgs part = va;
    part.scores += static_cast<size_t>(first) * count;
    part.boxes += static_cast<size_t>(first) * count * 4;
    part.classes += static_cast<size_t>(first) * count;
    part.kept += static_cast<size_t>(first) * detections_per_im;
    part.out_boxes += static_cast<size_t>(first) * detections_per_im * 4;
    timed_launch(ODTK_KERNEL_NMS, odtk::box_vote_kernel, dim3(groups, static_cast<unsigned>(n)), dim3(odtk::kVoteThreads), 0,
                 static_cast<hipStream_t>(stream), part);
  }
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

int odtk_concat_candidates(int batch_size, int n_parts, const odtk_candidates_t *parts, void *const *outputs, uint32_t flags,
                           void *stream) {
  if (batch_size <= 0 || n_parts < 1 || n_parts > odtk::kConcatMaxParts || !parts) return ODTK_ERR_INVALID;
  if (flags & ~(ODTK_FLAG_ROTATED | ODTK_FLAG_LOGITS | ODTK_FLAG_ROTATED_NMS_FIXED_ANGLE)) return ODTK_ERR_INVALID;
  if (!outputs || !outputs[0] || !outputs[1] || !outputs[2]) return ODTK_ERR_INVALID;
  odtk::ConcatArgs ca;
  std::memset(&ca, 0, sizeof ca);
  size_t total = 0;
  for (int i = 0; i < n_parts; ++i) {
    const odtk_candidates_t &c = parts[i];
    if (!c.scores || !c.boxes || !c.classes || c.count == 0 || c.count > ODTK_MAX_NMS_COUNT_SCRATCH || c.mirror_width < 0)
      return ODTK_ERR_INVALID;
    ca.scores[i] = c.scores; ca.boxes[i] = c.boxes; ca.classes[i] = c.classes;
    ca.offset[i] = static_cast<uint32_t>(total);
    ca.mirror[i] = static_cast<float>(c.mirror_width - 1);
    if (c.mirror_width > 0) ca.mirrored |= 1u << i;
    total += c.count;
    if (total > ODTK_MAX_NMS_COUNT_SCRATCH) return ODTK_ERR_INVALID;
  }
  if (flags & ODTK_FLAG_ROTATED) return ODTK_ERR_UNSUPPORTED;
  for (int i = n_parts; i <= odtk::kConcatMaxParts; ++i) ca.offset[i] = static_cast<uint32_t>(total);
  ca.total = static_cast<uint32_t>(total);
  ca.n_parts = n_parts;
  ca.out_scores = static_cast<float *>(outputs[0]);
  ca.out_boxes = static_cast<float *>(outputs[1]);
  ca.out_classes = static_cast<float *>(outputs[2]);
  ca.elements = static_cast<uint64_t>(batch_size) * total;
  uint64_t blocks = (ca.elements + odtk::kConcatThreads - 1) / odtk::kConcatThreads;
  if (blocks > 256 * 16) blocks = 256 * 16;                  // grid-stride beyond 16 workgroups per CU
  timed_launch(ODTK_KERNEL_NMS, odtk::concat_candidates_kernel, dim3(static_cast<unsigned>(blocks)), dim3(odtk::kConcatThreads), 0,
               static_cast<hipStream_t>(stream), ca);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

int odtk_merge_tile_candidates(int n_tiles, const odtk_tile_t *tiles, const void *const *inputs, void *const *outputs, size_t count,
                               int batch, int slots, int tile_h, int tile_w, int height, int width, float border, uint32_t flags,
                               void *stream) {
  if (n_tiles < 1 || n_tiles > ODTK_MAX_TILES || !tiles || count == 0 || batch <= 0 || slots <= 0) return ODTK_ERR_INVALID;
  if (tile_h <= 0 || tile_w <= 0 || height <= 0 || width <= 0) return ODTK_ERR_INVALID;
  if (count > ODTK_MAX_NMS_COUNT_SCRATCH || static_cast<unsigned long long>(slots) * count > ODTK_MAX_NMS_COUNT_SCRATCH) return ODTK_ERR_INVALID;
  if (!std::isfinite(border) || border < 0.0f) return ODTK_ERR_INVALID;
  if (flags & ~(ODTK_FLAG_ROTATED | ODTK_FLAG_LOGITS | ODTK_FLAG_ROTATED_NMS_FIXED_ANGLE)) return ODTK_ERR_INVALID;
  if (!inputs || !inputs[0] || !inputs[1] || !inputs[2] || !outputs || !outputs[0] || !outputs[1] || !outputs[2]) return ODTK_ERR_INVALID;
  for (int i = 0; i < n_tiles; ++i) {
    if (tiles[i].image >= batch) return ODTK_ERR_INVALID;
    if (tiles[i].image >= 0 && (tiles[i].slot < 0 || tiles[i].slot >= slots)) return ODTK_ERR_INVALID;
  }
  if (flags & ODTK_FLAG_ROTATED) return ODTK_ERR_UNSUPPORTED;
  static_assert(sizeof(odtk::TileMergeArgs) <= 4096, "kernel arguments travel by value");
  odtk::TileMergeArgs ma;
  std::memset(&ma, 0, sizeof ma);
  ma.scores = static_cast<const uint32_t *>(inputs[0]);
  ma.boxes = static_cast<const uint32_t *>(inputs[1]);
  ma.classes = static_cast<const uint32_t *>(inputs[2]);
  ma.out_scores = static_cast<uint32_t *>(outputs[0]);
  ma.out_boxes = static_cast<uint32_t *>(outputs[1]);
  ma.out_classes = static_cast<uint32_t *>(outputs[2]);
  ma.count = static_cast<uint32_t>(count);
  ma.total = static_cast<uint32_t>(static_cast<unsigned long long>(slots) * count);
  ma.tile_h = tile_h;
  ma.tile_w = tile_w;
  ma.height = height;
  ma.width = width;
  ma.border = border;
  std::memcpy(ma.tiles, tiles, sizeof(odtk_tile_t) * n_tiles);
  const unsigned groups = static_cast<unsigned>((count + odtk::kTileThreads - 1) / odtk::kTileThreads);
  const dim3 grid(groups, static_cast<unsigned>(n_tiles)), block(odtk::kTileThreads);
  if (border > 0.0f) timed_launch(ODTK_KERNEL_NMS, odtk::merge_tile_candidates_kernel<true>, grid, block, 0, static_cast<hipStream_t>(stream), ma);
  else timed_launch(ODTK_KERNEL_NMS, odtk::merge_tile_candidates_kernel<false>, grid, block, 0, static_cast<hipStream_t>(stream), ma);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

int odtk_iou(const void *const *inputs, void *const *outputs, int num_boxes, int num_anchors, void *stream) {
  if (num_boxes < 0 || num_anchors < 0) return ODTK_ERR_INVALID;
  const long long pairs = 1ll * num_boxes * num_anchors;
  if (pairs == 0) return ODTK_OK;                            // empty side: nothing to write
  if (!inputs || !outputs || !inputs[0] || !inputs[1] || !outputs[0]) return ODTK_ERR_INVALID;
  if (pairs > 0x7fffffffll) return ODTK_ERR_INVALID;
  const int threads = 256;
  long long blocks = (pairs + threads - 1) / threads;
  if (blocks > 256 * 16) blocks = 256 * 16;                  // grid-stride beyond 16 workgroups per CU
  {
    KernelTimer t(ODTK_KERNEL_IOU, static_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(odtk::iou_pairs_kernel, dim3(static_cast<unsigned>(blocks)), dim3(threads), 0,
                       static_cast<hipStream_t>(stream), static_cast<const float *>(inputs[0]),
                       static_cast<const float *>(inputs[1]), static_cast<float *>(outputs[0]), num_boxes,
                       num_anchors);
  }
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

}  // extern "C"
