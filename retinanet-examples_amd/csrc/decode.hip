// decode.hip -- decode and selection: workspace layout, the ODTK_SELECT_* knobs, odtk_decode*,
// odtk_prefilter_thresholds and odtk_detect (decode, then nms.hip's nms_impl over decode's own output).
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "internal.hpp"
#include "prefilter.hpp"
#include "select_decode.hpp"

namespace {

struct DecodeLayout {
  size_t sel_off, counts_off, key_off[ODTK_MAX_LEVELS], surv_off[ODTK_MAX_LEVELS], total;
  uint32_t cnt_off[ODTK_MAX_LEVELS], n[ODTK_MAX_LEVELS], spans[ODTK_MAX_LEVELS], parts[ODTK_MAX_LEVELS];
  uint32_t span_tiles, span_elems, budget;
};
static_assert(sizeof(odtk::DecodeArgs) <= 4096 && sizeof(odtk::ScanArgs) <= 4096, "kernel arguments travel by value");

// top_n <= 4096: the standard select_decode (32 KiB static sort buffer); beyond: the variant with 128 KiB of dynamic LDS
uint32_t sort_cap_for(int top_n) { return top_n <= odtk::kSortCap ? odtk::kSortCap : odtk::kSortCapBig; }

// select_decode's cooperative route (csrc/select_decode.hpp): how long a workgroup waits for the partners of its segment, in ticks
// of the 100 MHz wall clock, before the segment falls back to the tournament.  ODTK_SELECT_COOP_TICKS: 0 = route off (A/B),
// 1 = every barrier times out at once unless the partners are already there (exercises the fall-back), default 1000 = 10 us:
// measured where the kernel runs -- inside Model.forward, level streams on, 200 traced steps = 3200 shared segments
// (profiles/r06_select_routes_instep.txt) -- every segment went the cooperative route and workgroup 0 sat 2.1 us (p50) / 3.1 us
// (p99) / 3.4 us (max) between "slice fetched" and "barrier passed", its own histogram atomics included; the same with a 5 us
// bound.  10 us is three times the longest wait seen; a partner that is NOT resident costs its segment 10 us, not round 5's 30.
uint32_t select_coop_ticks() {
  static const uint32_t v = [] {
    const char *e = std::getenv("ODTK_SELECT_COOP_TICKS");
    const long x = e ? std::atol(e) : 1000;
    return static_cast<uint32_t>(x < 0 ? 0 : (x > 1000000 ? 1000000 : x));
  }();
  return v;
}

// ODTK_SELECT_RANK=1: select_decode orders the selected keys by COUNTING (histogram bases + in-bin ranks) and decodes each where
// it lies (csrc/select_decode.hpp, round 6) instead of the rank-merge sort + decode loop of rounds 4-5.  Same result
// (the GPU suite passes either way); NOT the default: measured slower on the bench's bf16 heads, whose boundary score is a
// plateau of 300-500 equal 16-bit scores (37.4 vs 30.0 us in the step; profiles/r06_select_rank_by_counting.txt).
uint32_t select_rank_sort() {
  static const uint32_t v = [] { const char *e = std::getenv("ODTK_SELECT_RANK"); return (e && e[0] == '1') ? 1u : 0u; }();
  return v;
}

// Workspace of a decode call: [segment state | sub-list lengths | candidate pool: kSpanCap keys per span | survivor lists].
// A span = 1 (fp32) or 2 (16-bit) tiles of 16 384 scores of ONE image; its four prefilter waves own kWaveStage keys each, so
// no list can overflow into another and nothing is reserved at run time.  A wave with more raw hits than that marks its
// list kListOverflow and select_decode re-reads the span's raw scores: capacity is a speed knob, never a result.
int decode_layout(int batch, int n_levels, const odtk_level_t *levels, int A, int C, int top_n, int dtype, DecodeLayout *out) {
  size_t off = 0;
  out->sel_off = off;
  off += align_up(sizeof(odtk::SelSeg) * static_cast<size_t>(batch) * n_levels);
  out->span_tiles = dtype == ODTK_F32 ? 1u : odtk::kSpanTiles16;
  out->span_elems = out->span_tiles * odtk::kTile;
  out->budget = sort_cap_for(top_n);                       // keys a workgroup of the tournament route passes on: one sort buffer
  size_t lists = 0;
  for (int l = 0; l < n_levels; ++l) {
    const unsigned long long n = 1ull * A * C * levels[l].height * levels[l].width;
    if (n == 0 || n > 0x7fff0000ull) return ODTK_ERR_INVALID;
    out->n[l] = static_cast<uint32_t>(n);
    out->spans[l] = static_cast<uint32_t>((n + out->span_elems - 1) / out->span_elems);
    // workgroups select_decode provides per segment: one per kSpansPerPart spans (they leave at once unless the segment
    // holds more than kKeysPerPart candidates each), and enough of them for a slice's sub-list lengths to fit in LDS
    uint32_t parts = (out->spans[l] + odtk::kSpansPerPart - 1) / odtk::kSpansPerPart;
    if (parts > odtk::kMaxParts) parts = odtk::kMaxParts;
    const uint32_t fit = (out->spans[l] * odtk::kScanWaves + odtk::kCntSlots - 1) / odtk::kCntSlots;
    if (parts < fit) parts = fit;
    out->parts[l] = parts < 1 ? 1 : parts;
    if (lists + static_cast<size_t>(batch) * out->spans[l] * odtk::kScanWaves > 0xffffffffull) return ODTK_ERR_INVALID;
    out->cnt_off[l] = static_cast<uint32_t>(lists);
    lists += static_cast<size_t>(batch) * out->spans[l] * odtk::kScanWaves;
  }
  out->counts_off = off;
  off += align_up(sizeof(uint32_t) * lists);
  for (int l = 0; l < n_levels; ++l) {
    out->key_off[l] = off;
    off += align_up(sizeof(uint64_t) * static_cast<size_t>(batch) * out->spans[l] * odtk::kSpanCap);
  }
  for (int l = 0; l < n_levels; ++l) {
    out->surv_off[l] = off;
    off += align_up(sizeof(uint64_t) * static_cast<size_t>(batch) * out->parts[l] * out->budget);
  }
  out->total = off;
  return ODTK_OK;
}

// Conservative raw-domain prefilter for ODTK_FLAG_LOGITS: every x with score_of(x) >= thresh has
// x >= logit_lower_bound(thresh).  The margin covers the rounding of the sigmoid to bf16/f16
// (relative 2^-8) and any non-monotonicity of expf by orders of magnitude; elements that pass it
// are then tested exactly, so a looser bound only costs a few extra exp() evaluations.
float logit_lower_bound(float thresh) {
  if (!(thresh > 0.0f)) return -INFINITY;                 // sigmoid > 0 >= thresh: everything passes
  const double t = static_cast<double>(thresh) * (1.0 - 1.0 / 64.0);
  if (t >= 1.0) return 0.0f;                              // only saturated scores can pass
  return static_cast<float>(std::log(t / (1.0 - t)) - 0.01);
}

int decode_levels_impl(int batch, int n_levels, const odtk_level_t *levels, int A, int C, int dtype,
                       uint32_t flags, float thresh, int top_n, void *const *outputs, int n_outputs,
                       void *workspace, size_t workspace_size, hipStream_t stream, uint32_t *run_valid = nullptr) {
  if (batch <= 0 || n_levels <= 0 || n_levels > ODTK_MAX_LEVELS || !levels) return ODTK_ERR_INVALID;
  if (A <= 0 || A > ODTK_MAX_ANCHORS || C <= 0 || top_n <= 0 || top_n > ODTK_MAX_TOP_N) return ODTK_ERR_INVALID;
  for (int l = 0; l < n_levels; ++l)
    if (levels[l].height <= 0 || levels[l].width <= 0) return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  size_t scan_lds = 0;                                     // per-channel threshold table of the prefilter (floats)
  for (int l = 0; l < n_levels; ++l) {
    if (levels[l].channels_last != 0 && levels[l].channels_last != 1) return ODTK_ERR_INVALID;
    if (levels[l].cls_bias) {
      if (dtype == ODTK_F32 || !(flags & ODTK_FLAG_LOGITS) || !levels[l].channels_last || (A * C) % 8 != 0)
        return ODTK_ERR_UNSUPPORTED;
      scan_lds = align_up(static_cast<size_t>(A) * C * sizeof(float));
      if (scan_lds > 48 * 1024) return ODTK_ERR_UNSUPPORTED;
      if (reinterpret_cast<uintptr_t>(levels[l].cls_thresholds) & 15u) return ODTK_ERR_INVALID;
    }
  }

  DecodeLayout lay;
  int rc = decode_layout(batch, n_levels, levels, A, C, top_n, dtype, &lay);
  if (rc != ODTK_OK) return rc;
  if (!workspace || !workspace_size) {
    if (lay.total > 0x7fffffffull) return ODTK_ERR_INVALID;   // the int return cannot carry it
    return static_cast<int>(lay.total);
  }
  if (workspace_size < lay.total) return ODTK_ERR_WORKSPACE;
  if (!outputs || n_outputs < 3 || !outputs[0] || !outputs[1] || !outputs[2]) return ODTK_ERR_INVALID;
  for (int l = 0; l < n_levels; ++l) {
    if (!levels[l].cls || !levels[l].box || !levels[l].anchors) return ODTK_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(levels[l].cls) & 15u) return ODTK_ERR_INVALID;   // 16-B vector loads
  }

  char *ws = static_cast<char *>(workspace);
  odtk::ScanArgs sa;
  std::memset(&sa, 0, sizeof sa);
  odtk::DecodeArgs da;
  std::memset(&da, 0, sizeof da);
  const uint32_t per_load = dtype == ODTK_F32 ? 4u : 8u;
  bool aligned = true;                                     // every image of every level starts on a 16-byte boundary
  uint32_t scan_blocks = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (lay.n[l] % per_load) aligned = false;
    sa.lv[l].cls = levels[l].cls;
    sa.lv[l].key_off = (lay.key_off[l] - lay.key_off[0]) / sizeof(uint64_t);
    sa.lv[l].cnt_off = lay.cnt_off[l];
    sa.lv[l].n = lay.n[l];
    sa.lv[l].blk_begin = scan_blocks;
    sa.lv[l].spans = lay.spans[l];
    sa.lv[l].seg_base = static_cast<uint32_t>(l) * batch;
    sa.lv[l].channels = static_cast<uint32_t>(A) * C;
    sa.lv[l].hw = static_cast<uint32_t>(levels[l].height) * levels[l].width;
    sa.lv[l].channels_last = static_cast<uint32_t>(levels[l].channels_last);
    sa.lv[l].by_channels = odtk::fastdiv_make(static_cast<uint32_t>(A) * C);
    sa.lv[l].bias = levels[l].cls_bias;
    sa.lv[l].table = levels[l].cls_bias ? levels[l].cls_thresholds : nullptr;
    if (static_cast<unsigned long long>(scan_blocks) + 1ull * batch * lay.spans[l] > 0x7fffffffull) return ODTK_ERR_INVALID;
    scan_blocks += static_cast<uint32_t>(batch) * lay.spans[l];

    da.lv[l].cls = levels[l].cls;
    da.lv[l].box = levels[l].box;
    da.lv[l].key_off = sa.lv[l].key_off;
    da.lv[l].surv_off = (lay.surv_off[l] - lay.surv_off[0]) / sizeof(uint64_t);
    da.lv[l].cnt_off = lay.cnt_off[l];
    da.lv[l].n = lay.n[l];
    da.lv[l].spans = lay.spans[l];
    da.lv[l].height = levels[l].height;
    da.lv[l].width = levels[l].width;
    da.lv[l].stride = static_cast<float>(levels[l].stride);
    da.lv[l].channels_last = static_cast<uint32_t>(levels[l].channels_last);
    da.lv[l].cls_bias = levels[l].cls_bias;
    da.lv[l].box_bias = levels[l].box_bias;
    std::memcpy(da.lv[l].anchors, levels[l].anchors, sizeof(float) * 4 * A);
    da.parts[l] = lay.parts[l];
    da.part_begin[l] = l == 0 ? 0u : da.part_begin[l - 1] + da.parts[l - 1] * static_cast<uint32_t>(batch);
  }
  da.part_begin[n_levels] = da.part_begin[n_levels - 1] + da.parts[n_levels - 1] * static_cast<uint32_t>(batch);
  for (int l = n_levels + 1; l <= ODTK_MAX_LEVELS; ++l) da.part_begin[l] = da.part_begin[n_levels];
  sa.counts = reinterpret_cast<uint32_t *>(ws + lay.counts_off);
  sa.cand = reinterpret_cast<uint64_t *>(ws + lay.key_off[0]);
  sa.sel = reinterpret_cast<odtk::SelSeg *>(ws + lay.sel_off);
  sa.n_levels = n_levels;
  sa.batch = batch;
  sa.span = static_cast<int>(lay.span_tiles);
  sa.thresh = thresh;
  sa.raw_lo = logit_lower_bound(thresh);

  da.sel = sa.sel;
  da.surv = reinterpret_cast<uint64_t *>(ws + lay.surv_off[0]);
  da.counts = sa.counts;
  da.cand = sa.cand;
  da.budget = lay.budget;
  da.span_elems = lay.span_elems;
  da.aligned = aligned ? 1u : 0u;
  da.coop_ticks = select_coop_ticks();
  da.rank_sort = select_rank_sort();
  da.raw_lo = sa.raw_lo;
  da.by_channels = odtk::fastdiv_make(static_cast<uint32_t>(A) * C);
  da.out_scores = static_cast<float *>(outputs[0]);
  da.out_boxes = static_cast<float *>(outputs[1]);
  da.out_classes = static_cast<float *>(outputs[2]);
  da.out_indices = n_outputs > 3 ? static_cast<int32_t *>(outputs[3]) : nullptr;
  da.run_valid = run_valid;
  da.n_levels = n_levels;
  da.batch = batch;
  da.num_anchors = A;
  da.num_classes = C;
  da.top_n = top_n;
  da.thresh = thresh;
  da.trace = g_trace;

  // Two launches, nothing to clear in front of them: the prefilter writes every sub-list length and zeroes the segment
  // state select_decode's tournament route counts in (rounds 1-3 cleared counters and histograms with a launch of their own).
  const uint32_t sel_blocks = da.part_begin[n_levels];
  const uint32_t sort_cap = sort_cap_for(top_n);
  const bool rotated = (flags & ODTK_FLAG_ROTATED) != 0, logits = (flags & ODTK_FLAG_LOGITS) != 0;
  return dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return logits ? launch_decode<T, true>(rotated, aligned, scan_blocks, sel_blocks, sort_cap, scan_lds, sa, da, stream)
                  : launch_decode<T, false>(rotated, aligned, scan_blocks, sel_blocks, sort_cap, scan_lds, sa, da, stream);
  });
}

int decode_single(bool rotated, int batch, const void *const *inputs, void *const *outputs, size_t height,
                  size_t width, size_t scale, size_t A, size_t C, const float *anchors, size_t anchors_len,
                  float thresh, int top_n, void *workspace, size_t workspace_size, void *stream) {
  if (height == 0 || width == 0 || height > 0x7fffffff || width > 0x7fffffff || scale > 0x7fffffff)
    return ODTK_ERR_INVALID;
  if (A == 0 || A > ODTK_MAX_ANCHORS || anchors_len != 4 * A || (!anchors && workspace && workspace_size))
    return ODTK_ERR_INVALID;
  if (C == 0 || C > 0x7fffffff) return ODTK_ERR_INVALID;
  const bool query = !workspace || !workspace_size;
  if (!query && (!inputs || !inputs[0] || !inputs[1])) return ODTK_ERR_INVALID;
  odtk_level_t lv;
  std::memset(&lv, 0, sizeof lv);
  lv.cls = query ? nullptr : inputs[0];
  lv.box = query ? nullptr : inputs[1];
  lv.height = static_cast<int32_t>(height);
  lv.width = static_cast<int32_t>(width);
  lv.stride = static_cast<int32_t>(scale);
  lv.anchors = anchors;
  return decode_levels_impl(batch, 1, &lv, static_cast<int>(A), static_cast<int>(C), ODTK_F32,
                            rotated ? ODTK_FLAG_ROTATED : 0u, thresh, top_n, outputs, 3, workspace,
                            workspace_size, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

int odtk_decode(int batch_size, const void *const *inputs, void *const *outputs, size_t height, size_t width,
                size_t scale, size_t num_anchors, size_t num_classes, const float *anchors, size_t anchors_len,
                float score_thresh, int top_n, void *workspace, size_t workspace_size, void *stream) {
  return decode_single(false, batch_size, inputs, outputs, height, width, scale, num_anchors, num_classes,
                       anchors, anchors_len, score_thresh, top_n, workspace, workspace_size, stream);
}

int odtk_decode_rotate(int batch_size, const void *const *inputs, void *const *outputs, size_t height,
                       size_t width, size_t scale, size_t num_anchors, size_t num_classes, const float *anchors,
                       size_t anchors_len, float score_thresh, int top_n, void *workspace, size_t workspace_size,
                       void *stream) {
  return decode_single(true, batch_size, inputs, outputs, height, width, scale, num_anchors, num_classes,
                       anchors, anchors_len, score_thresh, top_n, workspace, workspace_size, stream);
}

int odtk_prefilter_thresholds(const float *cls_bias, int channels, int dtype, float score_thresh, float *table, void *stream) {
  if (!cls_bias || !table || channels <= 0 || channels % 8 != 0) return ODTK_ERR_INVALID;
  if (dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(table) & 15u) return ODTK_ERR_INVALID;
  const float raw_thr = logit_lower_bound(score_thresh);
  const unsigned blocks = (static_cast<unsigned>(channels) + 255u) / 256u;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == ODTK_BF16)
    hipLaunchKernelGGL(odtk::prefilter_table_kernel<odtk::BF16>, dim3(blocks), dim3(256), 0, s, cls_bias, static_cast<uint32_t>(channels), raw_thr,
                       static_cast<uint32_t>(dtype), table);
  else
    hipLaunchKernelGGL(odtk::prefilter_table_kernel<odtk::F16>, dim3(blocks), dim3(256), 0, s, cls_bias, static_cast<uint32_t>(channels), raw_thr,
                       static_cast<uint32_t>(dtype), table);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

int odtk_decode_levels(int batch_size, int n_levels, const odtk_level_t *levels, int num_anchors,
                       int num_classes, int dtype, uint32_t flags, float score_thresh, int top_n,
                       void *const *outputs, int n_outputs, void *workspace, size_t workspace_size,
                       void *stream) {
  return decode_levels_impl(batch_size, n_levels, levels, num_anchors, num_classes, dtype, flags,
                            score_thresh, top_n, outputs, n_outputs, workspace, workspace_size,
                            static_cast<hipStream_t>(stream));
}

int odtk_detect(int batch_size, int n_levels, const odtk_level_t *levels, int num_anchors, int num_classes,
                int dtype, uint32_t flags, float score_thresh, int top_n, float nms_thresh,
                int detections_per_im, void *const *outputs, void *workspace, size_t workspace_size,
                void *stream) {
  if (batch_size <= 0 || n_levels <= 0 || n_levels > ODTK_MAX_LEVELS || top_n <= 0) return ODTK_ERR_INVALID;
  const int nb = (flags & ODTK_FLAG_ROTATED) ? 6 : 4;
  const size_t count = static_cast<size_t>(n_levels) * top_n;
  // workspace = [decode scratch | cat scores | cat boxes | cat classes]
  const int dec = decode_levels_impl(batch_size, n_levels, levels, num_anchors, num_classes, dtype, flags,
                                     score_thresh, top_n, nullptr, 0, nullptr, 0, nullptr);
  if (dec < 0) return dec;
  const int nms_ws = nms_impl(batch_size, nullptr, nullptr, 3, count, detections_per_im, nms_thresh, flags, nullptr, 0, nullptr);
  if (nms_ws < 0) return nms_ws;
  const size_t off_s = align_up(static_cast<size_t>(dec));
  const size_t off_b = off_s + align_up(sizeof(float) * batch_size * count);
  const size_t off_c = off_b + align_up(sizeof(float) * batch_size * count * nb);
  const size_t off_n = off_c + align_up(sizeof(float) * batch_size * count);
  const size_t off_v = off_n + align_up(static_cast<size_t>(nms_ws));                // positive scores per (image, level) list
  const size_t total = off_v + align_up(sizeof(uint32_t) * batch_size * n_levels);
  if (!workspace || !workspace_size) return total > 0x7fffffffull ? ODTK_ERR_INVALID : static_cast<int>(total);
  if (workspace_size < total) return ODTK_ERR_WORKSPACE;
  if (!outputs) return ODTK_ERR_INVALID;
  char *ws = static_cast<char *>(workspace);
  void *cat[3] = {ws + off_s, ws + off_b, ws + off_c};
  uint32_t *run_valid = reinterpret_cast<uint32_t *>(ws + off_v);
  int rc = decode_levels_impl(batch_size, n_levels, levels, num_anchors, num_classes, dtype, flags, score_thresh,
                              top_n, cat, 3, workspace, static_cast<size_t>(dec), static_cast<hipStream_t>(stream), run_valid);
  if (rc != ODTK_OK) return rc;
  // the candidates are decode_levels' own output: n_levels runs of top_n, each already in NMS order, run_valid of them positive
  return nms_impl(batch_size, cat, outputs, 3, count, detections_per_im, nms_thresh, flags, ws + off_n,
                  static_cast<size_t>(nms_ws), static_cast<hipStream_t>(stream), static_cast<uint32_t>(top_n), run_valid);
}

}  // extern "C"
