/*
 * odtk_hip.h -- C ABI of the MI355X (gfx950) post-processing library  libodtk_hip.so
 *
 * Drop-in boundary for the per-anchor hot path of NVIDIA/retinanet-examples (ODTK):
 * box decode + threshold/top-k prefilter, batched class-aware NMS, and the rotated-bbox
 * decode / IoU / NMS variants.  Every entry point is `extern "C"`, takes plain pointers and
 * sizes, never allocates device memory, never synchronises the host with the device, never
 * throws, and only ENQUEUES work on the caller's HIP stream.
 *
 * Conventions shared by all entry points
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - all tensor pointers are DEVICE pointers; `anchors` is a HOST pointer (copied by value
 *     into the kernel arguments -- nothing is uploaded, nothing outlives the call).
 *   - two-phase workspace query, cub style, exactly like the reference
 *     (csrc/cuda/decode.cu:53-72, nms.cu:87-105): call with workspace == NULL or
 *     workspace_size == 0 -> the return value is the number of scratch bytes required
 *     (> 0); call again with a buffer of at least that size -> returns ODTK_OK (0).
 *   - errors are negative return values (the reference never checked a CUDA error and threw
 *     std::runtime_error("Workspace is too small!") across the boundary, utils.h:55-57).
 *   - the workspace is scratch: contents before the call are irrelevant (nothing is cleared by a launch of
 *     its own: the first kernel of a call writes every word the second reads), a call may not
 *     share its workspace with another call that is in flight on a different stream.
 *   - outputs are fully written (zero padded tails); they need not be pre-zeroed.
 *
 * Semantics are those of the reference's CPU path odtk/box.py (the normative ones, see
 * DESIGN.md): candidates are `score >= score_thresh`, ordered score-descending with ties
 * broken by ascending flat NCHW index (decode) / ascending candidate position (nms);
 * boxes are clamped on both sides to [0, size*stride-1]; NMS uses the +1 pixel convention
 * and suppresses iff same class and not (IoU <= nms_thresh).
 */
#ifndef ODTK_HIP_H
#define ODTK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ODTK_OK                0
#define ODTK_ERR_INVALID      -1   /* bad argument (null pointer, size 0, limit exceeded) */
#define ODTK_ERR_WORKSPACE    -2   /* workspace smaller than the size query reports       */
#define ODTK_ERR_HIP          -3   /* a HIP runtime call failed; see odtk_last_hip_error() */
#define ODTK_ERR_UNSUPPORTED  -4   /* dtype / layout combination not implemented          */

#define ODTK_MAX_LEVELS    6       /* pyramid levels per call (P3..P7 = 5); keeps kernargs < 4 KiB */
#define ODTK_MAX_ANCHORS   32      /* anchors per cell (9 axis-aligned, 27 rotated)       */
#define ODTK_ATSS_MAX_TOPK 16      /* nearest cells per box and level that ATSS may ask for */
#define ODTK_MAX_TOP_N     16384   /* per-level top_n (<= 4096: 32 KiB LDS sort; beyond: a 128 KiB variant) */
#define ODTK_MAX_NMS_COUNT 7680    /* candidates per image nms keeps LDS-resident (5 x 1000 by default);  */
#define ODTK_MAX_NMS_COUNT_SCRATCH (1 << 22) /* beyond that, up to this, the key list lives in the workspace   */
#define ODTK_MAX_NMS_DETECTIONS 2048 /* detections_per_im (100 by default)                */

/* element types of the head tensors */
#define ODTK_F32   0
#define ODTK_BF16  1
#define ODTK_F16   2

/* flags */
#define ODTK_FLAG_ROTATED        1u   /* 6-parameter boxes [x1,y1,x2,y2,sin,cos]                       */
#define ODTK_FLAG_LOGITS         2u   /* cls holds logits: sigmoid is fused into the prefilter          */
#define ODTK_FLAG_ROTATED_NMS_FIXED_ANGLE 4u /* rotated nms: use each box's OWN angle (the reference   */
                                      /* rotates both quads by the lower-scored box's angle,            */
                                      /* csrc/cuda/nms_iou.cu:192; that is the default here too)        */

const char *odtk_version(void);
/* ABI guard.  sizeof() of a struct type of this header AS THE LIBRARY WAS COMPILED: which = 0 odtk_level_t,
 * 1 odtk_snap_level_t, 2 odtk_snap_rot_level_t, 3 odtk_loss_level_t, 5 odtk_image_t, 6 odtk_augment_t, 7 odtk_rotation_t,
 * 9 odtk_candidates_t, 11 odtk_tile_t, 14 odtk_mosaic_tile_t, 15 odtk_mosaic_t, 17 odtk_optim_tensor_t; -1 for any other value (4, 8, 10,
 * 12, 13 and 16 stay unassigned: tests/test_abi_host.py, tests/test_free_rotate.py, tests/test_box_vote.py and later ones probe them as unknown ids).  A binding compiled (or
 * mirrored) against another revision of this header would pass level arrays of the wrong stride: both bindings compare
 * their own sizeof with this at load time and refuse to load on a mismatch (odtk/_C.py, csrc/odtk_binding.cpp). */
int odtk_abi_struct_size(int which);
/* hipGetErrorString of the last HIP failure seen by this thread ("" if none). */
const char *odtk_last_hip_error(void);

/*
 * odtk_decode / odtk_decode_rotate -- one pyramid level, whole batch.
 * Replaces  int odtk::cuda::decode(...)         csrc/cuda/decode.h:30-35  (decode.cu:44-171)
 *      and  int odtk::cuda::decode_rotate(...)  csrc/cuda/decode_rotate.h:30-35
 * Same argument order and meaning; `const std::vector<float>& anchors` becomes
 * (anchors, anchors_len) and cudaStream_t becomes a hipStream_t.
 *   inputs[0]  scores  float32 [batch, num_anchors*num_classes, height, width]  contiguous NCHW
 *   inputs[1]  deltas  float32 [batch, num_anchors*{4|6},       height, width]
 *   outputs[0] scores  float32 [batch, top_n]
 *   outputs[1] boxes   float32 [batch, top_n, {4|6}]
 *   outputs[2] classes float32 [batch, top_n]
 *   anchors    host float[anchors_len], anchors_len == 4*num_anchors (axis-aligned set,
 *              also for rotated -- csrc/cuda/decode_rotate.cu:139, box.py:258-259)
 */
int odtk_decode(int batch_size, const void *const *inputs, void *const *outputs,
                size_t height, size_t width, size_t scale, size_t num_anchors, size_t num_classes,
                const float *anchors, size_t anchors_len, float score_thresh, int top_n,
                void *workspace, size_t workspace_size, void *stream);

int odtk_decode_rotate(int batch_size, const void *const *inputs, void *const *outputs,
                       size_t height, size_t width, size_t scale, size_t num_anchors, size_t num_classes,
                       const float *anchors, size_t anchors_len, float score_thresh, int top_n,
                       void *workspace, size_t workspace_size, void *stream);

/*
 * odtk_nms / odtk_nms_rotate -- whole batch, one workgroup per image.
 * Replaces  int odtk::cuda::nms(...)         csrc/cuda/nms.h:28-31      (nms.cu:82-160)
 *      and  int odtk::cuda::nms_rotate(...)  csrc/cuda/nms_iou.h:28-31  (nms_iou.cu:260-322)
 *   inputs[0]  scores  float32 [batch, count]          (<= 0 entries are padding)
 *   inputs[1]  boxes   float32 [batch, count, {4|6}]
 *   inputs[2]  classes float32 [batch, count]
 *   outputs[0..2]      float32 [batch, detections_per_im], [.., {4|6}], [..]
 * Workspace: ALWAYS query (two-phase convention).  Axis-aligned with count <= ODTK_MAX_NMS_COUNT: everything is
 * LDS-resident and the query returns a token size -- unless detections_per_im is in the thousands and the kept list
 * leaves no room, then, as for larger counts (the reference has no cap, nms.cu:82-160), batch * count * 8 bytes for
 * the key lists.  Rotated: additionally the first round in NMS order and its pairwise suppression matrix
 * (m x m bits per image, m = min(count, 8 * detections_per_im, 1024) rounded up to 64): the rotated NMS is three to
 * five launches (first round -> matrix on the whole chip -> resolve; csrc/nms.hpp).
 */
int odtk_nms(int batch_size, const void *const *inputs, void *const *outputs,
             size_t count, int detections_per_im, float nms_thresh,
             void *workspace, size_t workspace_size, void *stream);

int odtk_nms_rotate(int batch_size, const void *const *inputs, void *const *outputs,
                    size_t count, int detections_per_im, float nms_thresh,
                    void *workspace, size_t workspace_size, void *stream);

/*
 * odtk_iou -- pairwise rotated-rectangle IoU (training-side target assignment).
 * Replaces  int odtk::cuda::iou(...)  csrc/cuda/nms_iou.h:33-35 (nms_iou.cu:324-387).
 *   inputs[0]  boxes   float32 [num_boxes, 4 corners, 2]
 *   inputs[1]  anchors float32 [num_anchors, 4 corners, 2]
 *   outputs[0] iou     float32 [num_anchors, num_boxes]   (layout of csrc/extensions.cpp:64-66)
 */
int odtk_iou(const void *const *inputs, void *const *outputs, int num_boxes, int num_anchors,
             void *stream);

/* ------------------------------------------------------------------------------------------
 * Extended entry points (no reference equivalent): the MI355X-first batched forms.
 * ---------------------------------------------------------------------------------------- */

typedef struct odtk_level {
  const void *cls;          /* [batch, A*C, H, W] scores (or logits with ODTK_FLAG_LOGITS)   */
  const void *box;          /* [batch, A*nb, H, W] deltas                                    */
  int32_t height, width;    /* H, W of this level                                            */
  int32_t stride;           /* pixels per cell (the reference's `scale`)                     */
  int32_t channels_last;    /* 0: NCHW-contiguous, 1: NHWC-contiguous (torch.channels_last)  */
  const float *anchors;     /* HOST float[4*A]                                               */
  /* Optional per-channel bias of the heads' last convolutions, folded into the kernels so that the
   * caller can skip its bias pass over the largest activation of the network (both may be NULL):
   *   cls_bias  DEVICE float32 [A*C]: logit = float(cls) + cls_bias[channel] in fp32, then the sigmoid.
   *             Needs ODTK_FLAG_LOGITS, a 16-bit dtype, channels_last = 1 and A*C a multiple of 8;
   *             otherwise ODTK_ERR_UNSUPPORTED.
   *   box_bias  DEVICE float32 [A*nb]: delta = float(box) + box_bias[a*nb + k] in fp32. */
  const float *cls_bias;
  const float *box_bias;
  /* Optional (may be NULL), with cls_bias: the prefilter's per-channel threshold table for THIS cls_bias, score_thresh and
   * dtype, prepared once by odtk_prefilter_thresholds (an engine does it when it folds its weights).  Without it every
   * workgroup of the prefilter derives the table from cls_bias before its first load.  The table carries what it was made
   * for; one made for another threshold / dtype / channel count is ignored.  A table made from OTHER bias values is the
   * caller's bug (remake it whenever cls_bias changes). */
  const float *cls_thresholds;
} odtk_level_t;

/* odtk_prefilter_thresholds -- fills `table` (DEVICE, 16-byte aligned, ODTK_THRESHOLD_TABLE_FLOATS(channels) floats) for
 * odtk_level_t::cls_thresholds.  cls_bias: DEVICE float32 [channels]; dtype: ODTK_BF16 / ODTK_F16; channels % 8 == 0. */
#define ODTK_THRESHOLD_TABLE_FLOATS(channels) ((size_t)(channels) + 8)
int odtk_prefilter_thresholds(const float *cls_bias, int channels, int dtype, float score_thresh, float *table, void *stream);

/*
 * odtk_decode_levels -- ALL pyramid levels x whole batch in one enqueue (2 kernel launches: prefilter,
 * select + decode; no host synchronisation; the reference needs >= 5 launches + 1 host sync per image per
 * level, decode.cu:86-168).  Outputs are written directly in the concatenated layout that
 * `torch.cat(per_level, 1)` produces in the reference (odtk/model.py:164):
 *   outputs[0] scores  float32 [batch, n_levels*top_n]
 *   outputs[1] boxes   float32 [batch, n_levels*top_n, {4|6}]
 *   outputs[2] classes float32 [batch, n_levels*top_n]
 *   outputs[3] (optional, may be NULL) int32 [batch, n_levels*top_n] flat NCHW index of each
 *              detection inside its level (-1 padding) -- for index-level parity checks.
 * n_outputs is 3 or 4.
 */
int odtk_decode_levels(int batch_size, int n_levels, const odtk_level_t *levels,
                       int num_anchors, int num_classes, int dtype, uint32_t flags,
                       float score_thresh, int top_n,
                       void *const *outputs, int n_outputs,
                       void *workspace, size_t workspace_size, void *stream);

/*
 * odtk_nms_ex -- odtk_nms / odtk_nms_rotate selected by flags, plus an optional 4th output
 *   outputs[3] (may be NULL) int32 [batch, detections_per_im]: input position of each kept box.
 */
int odtk_nms_ex(int batch_size, const void *const *inputs, void *const *outputs, int n_outputs,
                size_t count, int detections_per_im, float nms_thresh, uint32_t flags,
                void *workspace, size_t workspace_size, void *stream);

/*
 * odtk_nms_sorted_runs -- odtk_nms_ex for a caller who KNOWS how its candidates are ordered: `count` = n_runs (<= 8) runs of
 * `run_len` candidates, each run sorted by (score desc, position asc) with its non-positive scores at the end -- what decode
 * writes per level and `torch.cat(per_level, 1)` lays side by side (reference odtk/model.py:153-164) -- and run_valid DEVICE
 * uint32 [batch, n_runs] = the entries with a positive score at the head of every run.  The kernel then takes its rounds as
 * prefixes of the runs (no compaction, no radix selection, no sort: csrc/nms.hpp "sorted runs"); odtk_detect calls the same
 * code with what its own decode wrote.  Same outputs as odtk_nms_ex on the same candidates; a run that is NOT sorted is the
 * caller's bug.  (Also what tools/nms_clustered_probe.py replays a trained detector's candidates through.)
 */
int odtk_nms_sorted_runs(int batch_size, const void *const *inputs, void *const *outputs, int n_outputs, size_t count,
                         int run_len, const uint32_t *run_valid, int detections_per_im, float nms_thresh, uint32_t flags,
                         void *workspace, size_t workspace_size, void *stream);

/*
 * odtk_soft_nms -- class-aware Soft-NMS (Bodla et al. 2017) on axis-aligned boxes; no reference equivalent.  Inputs, outputs
 * and the optional 4th int32 output as for odtk_nms_ex.  Per image, in float32: w = scores, a candidate is alive iff w > 0; at
 * most detections_per_im times the alive candidate with the largest w (ties: lowest position) is emitted with its CURRENT w
 * and retired, and every alive candidate j of its class is decayed with the IoU of odtk_nms (+1 pixel convention):
 *   ODTK_SOFT_NMS_LINEAR    if !(iou <= nms_thresh)  w_j *= 1 - iou
 *   ODTK_SOFT_NMS_GAUSSIAN  w_j *= exp((-(iou * iou)) / sigma)     (correctly rounded exp; nms_thresh is not used)
 * and stays alive iff w_j >= min_score.  Emitted scores are non-increasing; unused slots are zero (index -1).
 * sigma and min_score must be finite and > 0, method one of the two above: otherwise ODTK_ERR_INVALID, as for any undefined
 * flag bit.  ODTK_FLAG_ROTATED and count > ODTK_MAX_NMS_COUNT (the candidates of an image live in the registers and the LDS of
 * one workgroup; csrc/soft_nms.hpp) are ODTK_ERR_UNSUPPORTED.  Workspace: two-phase query as everywhere; a token size.
 * One launch, timed under ODTK_KERNEL_NMS.
 */
#define ODTK_SOFT_NMS_LINEAR   1
#define ODTK_SOFT_NMS_GAUSSIAN 2
int odtk_soft_nms(int batch_size, const void *const *inputs, void *const *outputs, int n_outputs,
                  size_t count, int detections_per_im, float nms_thresh, int method, float sigma, float min_score,
                  uint32_t flags, void *workspace, size_t workspace_size, void *stream);

/*
 * odtk_matrix_nms -- class-aware Matrix NMS (Wang et al., SOLOv2, 2020; mmdetection's mask_matrix_nms, PaddleDetection's
 * matrix_nms) on axis-aligned boxes; no reference equivalent.  Inputs, outputs and the optional 4th int32 output as for
 * odtk_nms_ex / odtk_soft_nms.  Every candidate's score is multiplied by one factor that comes from pairwise IoUs alone: nothing
 * is serial, and count may be anything in 1..ODTK_MAX_NMS_COUNT_SCRATCH.  Per image, in float32, no FMA contraction:
 *   participants  the candidates with score > 0 (NaN is not), ranked by score descending, ties by lowest input position; only
 *                 the first n = min(pre_top, #positive) take part, the rest are dropped.
 *   iou(a, b)     the IoU of odtk_soft_nms, operation for operation: +1 pixel, torch max / min / clamp NaN rules,
 *                 inter / ((area_a + area_b) - inter).  Bitwise symmetric.
 *   cmax_i        max(+0, iou(k, i)) over the participants k of i's class ranked before i, evaluated as
 *                 `acc = iou > acc ? iou : acc` from acc = 0: a NaN IoU is skipped, whatever the order.
 *   decay_j       min(1, d(i, j)) over the participants i of j's class ranked before j, evaluated as `acc = d < acc ? d : acc`
 *                 from acc = 1: a NaN or +inf d (a division by 1 - cmax_i = 0) decides nothing.
 *                   ODTK_MATRIX_NMS_LINEAR    d = (1 - iou(i, j)) / (1 - cmax_i)        two subtractions, one IEEE division
 *                   ODTK_MATRIX_NMS_GAUSSIAN  d = exp(((cmax_i * cmax_i) - (iou * iou)) / sigma)   four float32 operations and
 *                                             one correctly rounded exp; dividing by sigma as odtk_soft_nms does: sigma = 0.5
 *                                             is mmdetection's sigma = 2.0
 *                 The first participant of a class has decay 1.  mmdetection takes the minimum of the whole column of its decay
 *                 matrix instead; row 0 of that matrix (cmax = 0) holds 1 - iou or exp(-iou^2 / sigma), never above 1, so the
 *                 two agree.
 *   output        s'_j = score_j * decay_j, one multiplication; j is alive iff s'_j >= min_score.  The alive participants are
 *                 emitted in order of s' descending, ties by lowest input position, at most detections_per_im of them, each
 *                 with s', its unchanged box, its class and (4th output) its input position.  Unused slots are zero (index -1).
 * There is no nms_thresh.  max and min do not depend on the order of evaluation: the same bits on every run.
 * ODTK_ERR_INVALID: a null pointer, batch_size < 1, count outside 1..ODTK_MAX_NMS_COUNT_SCRATCH, detections_per_im outside
 * 1..ODTK_MAX_NMS_DETECTIONS, pre_top outside 1..ODTK_MAX_MATRIX_NMS_PRE, a method that is neither of the two, sigma or min_score
 * not finite or not > 0, any undefined flag bit.  ODTK_FLAG_ROTATED is ODTK_ERR_UNSUPPORTED.  Everything is checked on the host
 * before anything touches HIP.  Workspace: two-phase query as everywhere (the positive candidates' keys, 8 bytes per candidate,
 * and 36 bytes per participant).  Four launches (csrc/matrix_nms.hpp: rank, cmax, decay, emit), no host synchronisation, timed
 * under ODTK_KERNEL_NMS.
 */
#define ODTK_MATRIX_NMS_LINEAR   1
#define ODTK_MATRIX_NMS_GAUSSIAN 2
#define ODTK_MAX_MATRIX_NMS_PRE  4096
int odtk_matrix_nms(int batch_size, const void *const *inputs, void *const *outputs, int n_outputs, size_t count,
                    int detections_per_im, int pre_top, int method, float sigma, float min_score, uint32_t flags,
                    void *workspace, size_t workspace_size, void *stream);

/*
 * odtk_box_vote -- box voting behind a suppression (Gidaris & Komodakis 2015; Detectron's bbox_vote) on axis-aligned boxes; no
 * reference equivalent.  Per image the inputs are the SUPPRESSION'S INPUT LIST -- inputs[0..2] = scores [batch, count], boxes
 * [batch, count, 4], classes [batch, count], float32, as odtk_nms takes them -- and kept, int32 [batch, detections_per_im]: the
 * 4th output of odtk_nms_ex / odtk_soft_nms, the input position of each emitted detection or -1.  For slot r with p = kept[r]:
 *   p < 0 or p >= count: out_boxes[r] is four zeros.  Otherwise the voters are
 *     J = { j : scores[j] > 0, classes[j] == classes[p], (j == p or iou(p, j) >= vote_thresh) }
 *   where iou is the float32 IoU of odtk_soft_nms, operation for operation: +1 pixel, torch max / min / clamp NaN rules,
 *   inter / ((area_j + area_p) - inter).  A NaN IoU is not >= anything, so that candidate is no voter; the kept candidate always
 *   votes for itself (given its score is > 0 and its class equals itself, which holds for every position a suppression emits).
 *   out_boxes[r][k] = (float)( (SUM_J (double)scores[j] * (double)boxes[j][k]) / (SUM_J (double)scores[j]) ),  k = 0..3:
 *   products and sums in double, the sums in ANY order (the library's order is fixed: the same bits on every run), one double
 *   division, one rounding to float32.
 * The weights are always the INPUT scores, also behind odtk_soft_nms, whose emitted score is the decayed one.  Scores, classes
 * and the order of the detections are not touched: only out_boxes, float32 [batch, detections_per_im, 4], is written.  It may
 * alias nothing the call reads; pass the suppression's INPUT boxes, not its output boxes.
 * ODTK_ERR_INVALID: a null pointer, batch_size < 1, count outside 1..ODTK_MAX_NMS_COUNT_SCRATCH, detections_per_im outside
 * 1..ODTK_MAX_NMS_DETECTIONS, vote_thresh not finite or outside (0, 1], any undefined flag bit.  ODTK_FLAG_ROTATED is
 * ODTK_ERR_UNSUPPORTED.  No workspace; everything is checked on the host before anything touches HIP.  One launch (one wave per
 * slot: csrc/box_vote.hpp), timed under ODTK_KERNEL_NMS.
 */
int odtk_box_vote(int batch_size, const void *const *inputs, const int32_t *kept, void *out_boxes, size_t count,
                  int detections_per_im, float vote_thresh, uint32_t flags, void *stream);

/*
 * odtk_concat_candidates -- several candidate lists of the same batch as one, along the candidate axis (what torch.cat(.., 1)
 * gives), un-mirroring the boxes of the lists that come from a horizontally flipped pass: the merge step of flip test-time
 * augmentation.  parts is a HOST array of n_parts entries (they travel by value in the launch); outputs[0..2] = scores
 * [batch, total], boxes [batch, total, 4], classes [batch, total] with total = the sum of the counts; part i occupies the
 * positions behind those of parts 0..i-1, so on score ties a suppression prefers the earlier part.
 * mirror_width = 0: the part is copied.  mirror_width = W > 0: the part was decoded from x.flip(-1) of a tensor W wide; for its
 * entries with score > 0   x1' = (float)(W - 1) - x2,  x2' = (float)(W - 1) - x1   (one float32 subtraction each), y, score and
 * class unchanged; entries with score <= 0 (or NaN) are copied unchanged.
 * ODTK_ERR_INVALID: a null pointer, batch_size < 1, n_parts outside 1..8, a count of 0, a count or a total above
 * ODTK_MAX_NMS_COUNT_SCRATCH, a negative mirror_width, any undefined flag bit.  ODTK_FLAG_ROTATED is ODTK_ERR_UNSUPPORTED.
 * No workspace; everything is checked on the host.  One elementwise launch, timed under ODTK_KERNEL_NMS.
 */
typedef struct odtk_candidates {
  const float *scores;      /* [batch, count]     */
  const float *boxes;       /* [batch, count, 4]  */
  const float *classes;     /* [batch, count]     */
  uint32_t count;
  int32_t mirror_width;     /* 0, or the width of the tensor whose flip this part was decoded from */
} odtk_candidates_t;
int odtk_concat_candidates(int batch_size, int n_parts, const odtk_candidates_t *parts, void *const *outputs, uint32_t flags,
                           void *stream);

/*
 * Tiled (sliced) inference of large images: the image is cut into overlapping tiles of ONE fixed size, the detector runs on the
 * tiles as a batch, the candidates move back into image coordinates and one suppression sees them all.  No reference equivalent.
 * A tile table is a HOST array of up to ODTK_MAX_TILES entries; it travels by value in the launch.
 */
#define ODTK_MAX_TILES 64             /* entries per call: they travel by value, kernargs stay < 4 KiB */
typedef struct odtk_tile {
  int32_t image;            /* image of the batch the tile is cut from; < 0: a padding entry (an all-zero tile, skipped by the merge) */
  int32_t slot;             /* the tile's position among the tiles of its image (odtk_merge_tile_candidates; the tiler ignores it)  */
  int32_t x, y;             /* origin of the tile in its image, pixels, >= 0                                                         */
} odtk_tile_t;              /* 16 bytes; odtk_abi_struct_size id 11 */

/*
 * odtk_tile_images -- x: device [batch, channels, height, width] of `dtype` (ODTK_F32 / BF16 / F16), NCHW-contiguous
 * (channels_last = 0) or NHWC-contiguous (channels_last = 1); out: device [n_tiles, channels, tile_h, tile_w], same dtype and format.
 *     out[i][c][r][q] = x[tiles[i].image][c][tiles[i].y + r][tiles[i].x + q]   where that lies inside the image, +0 elsewhere
 * and an entry with image < 0 is an all-zero tile (the padding of a last, short chunk: the engine sees one shape only).  A bit copy:
 * NaN payloads, -0.0 and infinities survive.  Every element of out is written; `slot` is ignored.
 * ODTK_ERR_INVALID: a null pointer, n_tiles outside 1..ODTK_MAX_TILES, channels outside 1..16, a non-positive size, channels_last
 * other than 0 / 1, image >= batch, a negative origin, channels * tile_h * tile_w or channels * height * width beyond 2^32 - 1, a
 * pointer that is not aligned to the element.  Another dtype is ODTK_ERR_UNSUPPORTED.  No workspace; everything is checked on
 * the host before anything touches HIP.  One elementwise launch (csrc/tile.hpp), timed under ODTK_KERNEL_EPILOGUE.
 */
int odtk_tile_images(const void *x, void *out, int batch, int channels, int height, int width, int dtype, int channels_last,
                     int n_tiles, const odtk_tile_t *tiles, int tile_h, int tile_w, void *stream);

/*
 * odtk_merge_tile_candidates -- the candidates of the tiles, in tile coordinates, into the candidate lists of their images.
 * inputs[0..2] = scores [n_tiles, count], boxes [n_tiles, count, 4], classes [n_tiles, count], float32: what odtk_decode_levels
 * hands over for the batch of tiles.  outputs[0..2] = [batch, slots * count], [batch, slots * count, 4], [batch, slots * count].
 * Entry i writes positions slot * count .. slot * count + count - 1 of row `image`, and nothing else; the caller covers every
 * (image, slot) exactly once over its calls, so nothing is cleared.  Entries with image < 0 are skipped.  Per candidate of entry i:
 *   its score is not > 0 (zero, negative, NaN): copied bit for bit -- score, box and class;
 *   otherwise, with border > 0, the candidate is CUT when any of
 *       tile.x > 0 && x1 < border                        tile.x + tile_w < width  && x2 > (float)(tile_w - 1) - border
 *       tile.y > 0 && y1 < border                        tile.y + tile_h < height && y2 > (float)(tile_h - 1) - border
 *     holds -- float32 comparisons on the tile-local coordinates, a NaN fails them all -- and becomes an empty slot: score +0, box
 *     four zeros, class 0 (what decode leaves in unused slots);
 *   otherwise x1 += (float)tile.x, y1 += (float)tile.y, x2 += (float)tile.x, y2 += (float)tile.y, one float32 addition each; score
 *     and class unchanged.
 * border == 0 switches the cut rule off.  The rule drops the truncated candidates that decode's clamp presses against an interior
 * tile side; with an overlap at least as wide as the objects the neighbouring tile holds each such object whole.
 * ODTK_ERR_INVALID: a null pointer, n_tiles outside 1..ODTK_MAX_TILES, a count of 0, a non-positive batch, slots or size,
 * slots * count above ODTK_MAX_NMS_COUNT_SCRATCH, image >= batch, slot outside 0..slots - 1, a border that is negative or not
 * finite, any undefined flag bit.  ODTK_FLAG_ROTATED is ODTK_ERR_UNSUPPORTED.  No workspace; everything is checked on the host
 * before anything touches HIP.  One elementwise launch (csrc/tile.hpp), timed under ODTK_KERNEL_NMS.
 */
int odtk_merge_tile_candidates(int n_tiles, const odtk_tile_t *tiles, const void *const *inputs, void *const *outputs, size_t count,
                               int batch, int slots, int tile_h, int tile_w, int height, int width, float border, uint32_t flags,
                               void *stream);

/*
 * odtk_detect -- decode_levels + nms back to back on one stream (the whole post-processing of
 * odtk/model.py:153-165 in 3 launches).  outputs as odtk_nms; workspace holds the candidates.
 */
int odtk_detect(int batch_size, int n_levels, const odtk_level_t *levels,
                int num_anchors, int num_classes, int dtype, uint32_t flags,
                float score_thresh, int top_n, float nms_thresh, int detections_per_im,
                void *const *outputs, void *workspace, size_t workspace_size, void *stream);

/*
 * odtk_bias_act -- fused convolution epilogue, in place, on a channels_last (NHWC) activation:
 *     y[p][c] = act( y[p][c] + bias[c] (+ residual[p][c]) ),   act = ReLU if relu != 0
 * y, residual: device [n_pixels, channels] of `dtype` (ODTK_F32/BF16/F16), 16-byte aligned;
 * bias: DEVICE float32 [channels].  No reference kernel equivalent: it replaces the separate
 * conv-bias / frozen-batch-norm / residual-add / ReLU passes of the reference's PyTorch graph
 * (odtk/backbones/layers.py:5-16, torchvision Bottleneck.forward, odtk/model.py:57-62) once the
 * frozen BN scale is folded into the convolution weights (see odtk/fused.py).
 */
int odtk_bias_act(void *y, const float *bias, const void *residual, size_t n_pixels, int channels,
                  int dtype, int relu, void *stream);

/*
 * odtk_bias_act_maxpool -- stem epilogue: out = maxpool3x3/s2/p1( act( y + bias[c] ) ) in one pass over a
 * channels_last activation (ResNet conv1 -> bn1 -> relu -> maxpool, reference odtk/backbones/resnet.py
 * via torchvision's ResNet.forward).  y: device [batch, height, width, channels], out: device
 * [batch, (height+1)/2, (width+1)/2, channels], both ODTK_BF16 or ODTK_F16, 16-byte aligned,
 * channels % 8 == 0; bias: DEVICE float32 [channels].  Bit-identical to odtk_bias_act followed by
 * torch's max_pool2d (the epilogue is monotone, so it commutes with the maximum).
 */
int odtk_bias_act_maxpool(const void *y, const float *bias, void *out, int batch_size, int height, int width,
                          int channels, int dtype, int relu, void *stream);

/*
 * odtk_upsample_nearest2x -- out[b][y][x][c] = x[b][y / 2][x / 2][c] for a channels_last activation (the FPN's top-down path,
 * reference odtk/backbones/fpn.py:45-61: F.interpolate(., scale_factor=2)).  x: device [batch, height, width, channels], out:
 * device [batch, 2*height, 2*width, channels], both of `dtype`, 16-byte aligned, channels * sizeof(dtype) a multiple of 16.
 * A plain stream (bytes are copied, never decoded): bit-identical to torch's nearest interpolation.
 */
int odtk_upsample_nearest2x(const void *x, void *out, int batch_size, int height, int width, int channels, int dtype,
                            void *stream);

/*
 * Pyramid canvas (odtk/fused.py: the head towers of the small pyramid levels as ONE convolution).  The levels lie side by side in
 * one channels_last tensor [batch, height, width, channels] of `dtype`, each in a rectangle (y0, x0, rect_height, rect_width) --
 * `rects`: HOST int[4 * n_rects], n_rects <= ODTK_MAX_LEVELS, every rectangle inside the canvas -- with zero pixels between them:
 * the gutters are the zero padding of every level's convolution.  canvas 16-byte aligned, channels * sizeof(dtype) a multiple of 16.
 *   odtk_canvas_clear  zeroes every pixel outside the rectangles (a convolution over the canvas writes act(bias + ...) there;
 *                      the next layer must read zeros again); pixels inside are not touched.
 *   odtk_canvas_pack   writes the whole canvas: rectangle i from `sources[i]` (HOST array of DEVICE pointers to packed
 *                      [batch, rect_height, rect_width, channels] tensors, 16-byte aligned), zeros elsewhere.
 * One launch each; plain streams of 16-byte vectors (bytes are copied, never decoded: any storage type).
 */
int odtk_canvas_clear(void *canvas, int batch_size, int height, int width, int channels, int dtype, const int *rects, int n_rects,
                      void *stream);
int odtk_canvas_pack(void *canvas, int batch_size, int height, int width, int channels, int dtype, const int *rects,
                     const void *const *sources, int n_rects, void *stream);

/*
 * odtk_stem_pack -- 2x2 space-to-depth pack of the network input for the ResNet stem, with the cast to the engine's dtype:
 *     out[n][y][x][(dy * 2 + dx) * 3 + c] = x[n][c][2 y + dy][2 x + dx]   for the 12 real channels, channels 12..15 = 0
 * x: device [batch, 3, height, width] of in_dtype (ODTK_F32 / BF16 / F16), NCHW-contiguous (channels_last = 0) or NHWC-contiguous
 * (channels_last = 1); height and width even.  out: device [batch, height / 2, width / 2, 16] of out_dtype (ODTK_BF16 / F16),
 * 16-byte aligned.  The 7x7 / stride-2 / pad-3 stem convolution over x equals a 4x4 / stride-1 convolution with padding (2 before,
 * 1 after) over `out` with the re-indexed weights w4[k][(dy*2+dx)*3+c][R][S] = w[k][c][2R+dy-1][2S+dx-1] (zero outside the 7x7
 * window): same products, 16-byte channel vectors instead of 3-element ones (odtk/fused.py).  Replaces the cast + layout pass of
 * the input; no reference kernel equivalent (the reference feeds torchvision's conv1, odtk/backbones/resnet.py).
 */
int odtk_stem_pack(const void *x, void *out, int batch_size, int height, int width, int in_dtype, int channels_last, int out_dtype,
                   void *stream);

/* Debug / test: the launch shape of the six streaming kernels above (bias_act fast and scalar, bias_act_maxpool, upsample,
 * canvas, stem_pack).  Every launcher caps its grid (4096, 8192 or 256 * 16 workgroups) and walks the rest with a grid-stride loop;
 * the caps are reached only by tensors of 70 .. 130 MB, and the max-pool's 64-bit index form only by 2^32 output vectors.
 *   grid_cap         0 = each launcher's own cap (default); 1 .. 65536 replaces the cap of EVERY one of those grids (odtk_bias_act's
 *                    fast form still rounds the capped grid UP to a multiple of its unit, so that the grid stride stays a multiple
 *                    of the row length)
 *   pool_wide_index  1 = odtk_bias_act_maxpool runs its 64-bit index form whatever the size; 0 = only at 2^32 output vectors (default)
 * -1 leaves a field as it is; any other value: ODTK_ERR_INVALID, nothing changes.  The results never depend on either field
 * (tests/test_gpu_engine_streams.py).  Process-wide, one relaxed atomic load per launch; never touches HIP.
 * odtk_debug_stream_tuning_get: out[0] = grid_cap, out[1] = pool_wide_index. */
int odtk_debug_stream_tuning(int grid_cap, int pool_wide_index);
int odtk_debug_stream_tuning_get(int out[2]);
/* What odtk_bias_act would launch for [n_pixels, channels] of `dtype` under the current odtk_debug_stream_tuning -- answered by the
 * host function the launcher itself calls.  out[0] = form (0 scalar kernel, 1 fast 16-byte-vector kernel), out[1] = workgroups (of
 * 256 lanes), out[2] = grid stride = out[1] * 256, in vectors (fast) or elements (scalar), out[3] = passes of lane 0 of workgroup 0
 * through the fast form's unrolled loop (4 vectors, one stride apart, per pass; 0 for the scalar form).  ODTK_ERR_INVALID: out
 * null, n_pixels == 0 or channels < 1; ODTK_ERR_UNSUPPORTED: another dtype.  Never touches HIP. */
int odtk_debug_bias_act_grid(size_t n_pixels, int channels, int dtype, unsigned out[4]);

/*
 * odtk_preprocess_images -- the network's input from decoded source images, one launch for the whole batch: bilinear resize,
 * optional mirror, zero padding to height x width, normalisation, channels_last.  Replaces, on the device, what the reference's
 * dataset workers do per image on the host (odtk/data.py:56-59 `im.resize(.., Image.BILINEAR)`, :88 the flip, :111-117 the
 * normalisation, :166-176 the padding of the batch) and what its DALI loader did on the GPU (odtk/dali.py); bit-identical to
 * the former: Pillow's 8-bit resampling is fixed-point integer arithmetic, and the weights arrive as tables computed on the
 * host in double (odtk/data.py: resample_weights).
 *   images      HOST odtk_image_t[batch_size] (copied by value into the kernel arguments, kernels of up to 64 images)
 *   src         DEVICE uint8, src_bytes long: the source pixels, R G B interleaved, 3 bytes per pixel; image i starts at
 *               src + src_offset, its rows are src_pitch bytes apart
 *   tables      DEVICE int32[tables_len].  One table per axis and (source length, target length) pair, at index t:
 *               tables[t + 2 o], tables[t + 2 o + 1] = first source index and number of taps n <= taps of output index o
 *               (o < target length), then tables[t + 2 * target + o * taps + i] = weight i of output o in units of 2^-22.
 *               pass(s)[o] = clamp((2^21 + sum_i s[first + i] * weight[i]) >> 22, 0, 255); the horizontal pass runs first and
 *               is rounded to bytes.  x_table / y_table = -1: that pass is skipped (requires source length == target length).
 *   norm_table  DEVICE [3][256] of `dtype`: the value of byte v in channel c
 *   out         DEVICE [batch_size, height, width, 3] of `dtype` (ODTK_F32 / BF16 / F16) = [batch, 3, height, width] with
 *               channels_last strides; out[b][y][x][c] = norm_table[c][resized_b[y][mirror ? out_width - 1 - x : x][c]] for
 *               y < out_height and x < out_width, +0.0 elsewhere.  Every element is written.
 * Everything is checked on the host before anything touches HIP, including that every image and every table lies inside
 * src_bytes / tables_len.  No workspace, no synchronisation.
 */
typedef struct odtk_image {
  uint64_t src_offset;                      /* bytes from src to the first pixel                        */
  int32_t src_width, src_height, src_pitch; /* pixels, pixels, bytes (>= 3 * src_width)                 */
  int32_t out_width, out_height;            /* size after the resize (<= width, height of the batch)    */
  int32_t mirror;                           /* 1: flip left-right AFTER the resize                      */
  int32_t x_table, y_table;                 /* index of the axis' table in `tables`, -1: pass skipped   */
  int32_t x_taps, y_taps;                   /* taps per output index of that table                      */
} odtk_image_t;
int odtk_preprocess_images(int batch_size, const odtk_image_t *images, const void *src, size_t src_bytes, const int32_t *tables,
                           size_t tables_len, const void *norm_table, void *out, int height, int width, int dtype, void *stream);

/*
 * odtk_augment_images -- odtk_preprocess_images with the training augmentations of the reference's dataset between the resize and
 * the normalisation (odtk/data.py:68-109 there: `im.rotate` by a quarter turn, FLIP_LEFT_RIGHT, ImageEnhance.Brightness / Contrast,
 * torchvision's adjust_hue, ImageEnhance.Color), bit-identical to Pillow on the host; per image, in this order:
 *   resize (as odtk_preprocess_images; images[i].mirror must be 0, the flip is part of the map)
 *   -> canvas[y][x] = resized[(map[5] + map[3] x + map[4] y) >> 16][(map[2] + map[0] x + map[1] y) >> 16] for x < canvas_width,
 *      y < canvas_height, black (0, 0, 0) where that index lies outside the resized image: Pillow's 16.16 fixed-point NEAREST affine
 *      transform; a transpose, the flip and the identity {65536, 0, 0, 0, 65536, 0} are maps of the same form (odtk/data.py:
 *      quarter_turn_map computes them on the host, in double)
 *   -> brightness, contrast, saturation: byte = (uint8)(d + factor * (byte - d)) in float32 (product, then sum), clamped to
 *      [0, 255] first unless 0 <= factor <= 1; d = 0 | the image's grey level int(mean of L + 0.5) over the canvas as it is after
 *      the brightness | L of the pixel, L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.  Hue (between contrast and saturation):
 *      RGB -> HSV, H += hue (wrapping byte), HSV -> RGB as Pillow's `convert` does them; it runs, lossy, also for hue = 0
 *   -> out[b][y][x][c] = norm_table[c][byte], +0.0 outside the canvas.  Every element is written.
 * An image with flags = 0 and the identity map comes out exactly as odtk_preprocess_images writes it.
 *   augments    HOST odtk_augment_t[batch_size], like images
 *   workspace   DEVICE scratch, 16-byte aligned: the resized bytes of every image and one 64-bit sum per image.  Two-phase:
 *               workspace == NULL returns the bytes needed for (batch_size, height, width).
 * Everything else as odtk_preprocess_images.  A short chain of launches on `stream` (the grey level of the contrast has to exist
 * before any output pixel does): resize to bytes, sum of L (only if some image has contrast on), gather + colours + table + pad.
 * Everything is checked on the host before anything touches HIP; a workspace that is too small is ODTK_ERR_INVALID.
 */
#define ODTK_AUGMENT_BRIGHTNESS 1u
#define ODTK_AUGMENT_CONTRAST   2u
#define ODTK_AUGMENT_HUE        4u
#define ODTK_AUGMENT_SATURATION 8u
typedef struct odtk_augment {
  int32_t canvas_width, canvas_height;      /* size after the turn (<= width, height of the batch)      */
  int32_t map[6];                           /* 16.16 fixed point, see above                             */
  uint32_t flags;                           /* ODTK_AUGMENT_*                                           */
  float brightness, contrast, saturation;   /* blend factors (finite), read only if their flag is set   */
  uint8_t hue;                              /* added to H modulo 256                                    */
  uint8_t pad_[3];                          /* zero                                                     */
} odtk_augment_t;
int odtk_augment_images(int batch_size, const odtk_image_t *images, const odtk_augment_t *augments, const void *src, size_t src_bytes,
                        const int32_t *tables, size_t tables_len, const void *norm_table, void *out, int height, int width, int dtype,
                        void *workspace, size_t workspace_bytes, void *stream);
/*
 * odtk_augment_images_ex -- odtk_augment_images plus a free rotation per image: `Image.rotate(angle, resample=Image.BILINEAR)` of
 * the turned image about its centre on its own canvas (no expand, black fill), bit-identical to Pillow on the host.  No reference
 * equivalent: the reference parses --augment-free-rotate and ignores it.
 *   rotations   HOST odtk_rotation_t[batch_size], like augments; NULL: exactly odtk_augment_images (same checks, same workspace).
 * For an image with enabled != 0, in this order:
 *   resize -> the index map of augments[i], which holds the quarter turn ONLY, onto the canvas (w x h = canvas_width x canvas_height)
 *   -> rotation on that canvas, which keeps its size.  `matrix` takes the centre of an output pixel to a point of the turned image
 *      (odtk/data.py: free_rotation_matrix computes it on the host, in double, as Image.rotate does); per output pixel (x, y), every
 *      step one IEEE double operation, never fused:
 *        xin = (m0 (x + 0.5) + m1 (y + 0.5)) + m2,  yin = (m3 (x + 0.5) + m4 (y + 0.5)) + m5;  black unless 0 <= xin < w, 0 <= yin < h
 *        xin -= 0.5, yin -= 0.5, X = floor(xin), Y = floor(yin), dx = xin - X, dy = yin - Y
 *        v1 = p[Y'][X0] + (p[Y'][X1] - p[Y'][X0]) dx   with X0, X1 = X, X + 1 clamped to [0, w - 1], Y' = Y clamped to [0, h - 1]
 *        v2 = the same on row Y + 1 if Y + 1 < h, else v1;   byte = (uint8)(v1 + (v2 - v1) dy), truncated, per channel
 *   -> flip left-right if `flip`
 *   -> the colour chain of odtk_augment_images on those bytes (the black corners are image pixels: they count in the contrast's
 *      grey level and are normalised as byte 0), table, pad.
 * An image with enabled == 0 (then flip must be 0) comes out exactly as odtk_augment_images writes it.
 *   workspace   as odtk_augment_images, and a second slot per image for the finished canvas bytes: two-phase with this entry point's
 *               own query (workspace == NULL), which may answer more than odtk_augment_images does.
 * One more launch in the chain, between the resize and the sum of L (two for more than 32 images): the finished canvas bytes of
 * every image go to its second slot, and the sum and the colour pass read them through the identity map.
 * Everything is checked on the host before anything touches HIP: the matrix of an enabled image is finite, the flags are 0 or 1.
 */
typedef struct odtk_rotation {
  double matrix[6];                         /* m0 .. m5, see above; read only if enabled                */
  int32_t enabled;                          /* 0 | 1                                                    */
  int32_t flip;                             /* 0 | 1: flip left-right AFTER the rotation                */
} odtk_rotation_t;
int odtk_augment_images_ex(int batch_size, const odtk_image_t *images, const odtk_augment_t *augments, const odtk_rotation_t *rotations,
                           const void *src, size_t src_bytes, const int32_t *tables, size_t tables_len, const void *norm_table, void *out,
                           int height, int width, int dtype, void *workspace, size_t workspace_bytes, void *stream);
/*
 * odtk_mosaic_images -- mosaic augmentation: every output image is a canvas on which up to four resized source images are pasted,
 * each cropped to its rectangle, on a fill colour; then the colour chain, the table and the pad of odtk_augment_images.
 * Bit-identical to Pillow on the host (`Image.new`, `resize`, `transpose`, `crop`, `paste`; odtk/data.py: mosaic_pixels).  No
 * reference equivalent.
 *   images      HOST odtk_image_t[n_images]: the SOURCES, resized as odtk_preprocess_images resizes them; `mirror` is allowed here.
 *               resized_s = the resized bytes of source s with its mirror applied, out_width x out_height.
 *   max_pixels  the largest out_width * out_height over `images`, stated by the caller (the workspace query reads no descriptor);
 *               checked against the descriptors in the real call: no source may have more.
 *   mosaics     HOST odtk_mosaic_t[batch_size], one per OUTPUT image.  Canvas pixel (x, y), x < canvas_width, y < canvas_height, of
 *               output image b is resized_s[y - dst_y + src_y][x - dst_x + src_x] for the highest-numbered used tile (source = s >= 0)
 *               whose destination rectangle [dst_x, dst_x + width) x [dst_y, dst_y + height) holds (x, y), and `fill` where none does.
 *   augments    HOST odtk_augment_t[batch_size] or NULL (no colours).  Only the colour operations are read: canvas_width and
 *               canvas_height must equal the mosaic's and the map must be the identity {65536, 0, 0, 0, 65536, 0}.
 *   -> the colour chain of odtk_augment_images on the canvas bytes (fill pixels are image pixels: they count in the contrast's grey
 *      level and go through the table), out[b][y][x][c] = norm_table[c][byte], +0.0 outside the canvas.  Every element is written.
 * An output image with one tile that covers its canvas from src (0, 0) comes out exactly as odtk_augment_images writes that source
 * alone (the flip in the map there, in `mirror` here).
 *   workspace   DEVICE scratch, 16-byte aligned.  Two-phase: workspace == NULL returns the bytes needed, a function of (batch_size,
 *               n_images, max_pixels, height, width) alone: one 64-bit sum per output image (as many words as there are output images
 *               or sources, whichever are more: the resize zeroes one word per source), one slot of 3 * max_pixels bytes per
 *               source, one slot of 3 * height * width bytes per output image for its finished canvas.
 * A chain of launches on `stream`, no synchronisation: resize of the sources to bytes (64 per launch), the composition (16 output
 * images per launch), the sum of L (only if some image has contrast on), colours + table + pad through the identity map.
 * Everything is checked on the host before anything touches HIP: null pointers and non-positive sizes, `source` outside
 * -1 .. n_images - 1, a used tile without pixels or with a rectangle outside the canvas or with src + size outside its source's
 * resized image, non-zero pad_, a canvas larger than height x width, everything odtk_preprocess_images checks for the sources, a
 * workspace that is too small or not 16-byte aligned: ODTK_ERR_INVALID; a bad dtype: ODTK_ERR_UNSUPPORTED.
 */
typedef struct odtk_mosaic_tile {
  int32_t source;                           /* index into images[], -1: tile unused (the other fields are not read) */
  int32_t dst_x, dst_y, width, height;      /* destination rectangle on the canvas                      */
  int32_t src_x, src_y;                     /* its top-left corner in the resized source                */
} odtk_mosaic_tile_t;       /* 28 bytes; odtk_abi_struct_size id 14 */
typedef struct odtk_mosaic {
  int32_t canvas_width, canvas_height;      /* <= width, height of the batch                            */
  odtk_mosaic_tile_t tiles[4];              /* pasted in this order: a later tile covers an earlier one */
  uint8_t fill[3];                          /* R, G, B where no tile lies                               */
  uint8_t pad_;                             /* zero                                                     */
} odtk_mosaic_t;            /* 124 bytes; odtk_abi_struct_size id 15 */
int odtk_mosaic_images(int batch_size, const odtk_mosaic_t *mosaics, const odtk_augment_t *augments, int n_images,
                       const odtk_image_t *images, int max_pixels, const void *src, size_t src_bytes, const int32_t *tables,
                       size_t tables_len, const void *norm_table, void *out, int height, int width, int dtype, void *workspace,
                       size_t workspace_bytes, void *stream);
/*
 * odtk_gemm_bias_act -- 1x1 (pointwise) convolution of a channels_last activation as ONE GEMM with
 * the whole epilogue fused:
 *     y[p][o] = act( sum_c x[p][c] * w[o][c] + bias[o] (+ residual[p][o]) ),   act = ReLU if relu != 0
 * x: device [m, k], w: device [n, k] (= the convolution weight [C_out, C_in, 1, 1]), y / residual:
 * device [m, n], all of `dtype` (ODTK_BF16/F16/F32), row-major, 16-byte aligned; bias: DEVICE float32
 * [n]; residual may be NULL and must not alias y.  The contraction runs on hipBLASLt (bound at run time,
 * see odtk_gemm_init); the first call for a shape times the library's candidate kernels on `stream`
 * (synchronises once), later calls only enqueue.  workspace: device scratch for the library (32 MiB is
 * plenty), caller-owned like every other buffer of this ABI.
 * Like odtk_bias_act it has no reference kernel equivalent: it replaces conv1x1 -> frozen BN ->
 * (+ skip) -> ReLU of the reference's PyTorch graph (torchvision Bottleneck.forward,
 * odtk/backbones/layers.py:5-16, odtk/backbones/fpn.py lateral convs) once BN is folded.
 * Returns ODTK_ERR_UNSUPPORTED when hipBLASLt cannot be bound or has no kernel for the problem.
 *
 * odtk_gemm_init -- bind hipBLASLt from `path` (NULL: the already mapped / default libhipblaslt.so.1).
 * Optional; odtk_gemm_bias_act binds the default on first use.  Inside a PyTorch process pass the
 * copy PyTorch ships (torch/lib/libhipblaslt.so) so that only one copy of the soname is in use.
 */
int odtk_gemm_init(const char *hipblaslt_path);
/*
 * Reproducible plans.  Which hipBLASLt solution a problem runs on is decided by a stopwatch at its first call; the choice is not
 * the same on every box, and two solutions add up in different orders.  odtk_gemm_plan_export writes one line per tuned problem
 * ("gemm m n k dtype relu residual solution-index"; returns the bytes the text needs, NUL included, and writes at most
 * `capacity`), odtk_gemm_plan_import takes such lines (others are ignored; returns how many it took): a problem first seen after
 * the import runs on the named solution without timing, if the library still offers it for the problem (otherwise it is timed as
 * usual and counted by odtk_gemm_plan_pin_misses).  The engine's plan file (odtk/fused.py: plan_state / load_plan, ODTK_CONV_PLAN)
 * carries these lines next to libodtk_conv.so's (include/odtk_conv.h).  No reference equivalent (one deterministic PyTorch graph,
 * odtk/model.py:125-165).
 */
size_t odtk_gemm_plan_export(char *text, size_t capacity);
int odtk_gemm_plan_import(const char *text);
int odtk_gemm_plan_pin_misses(void);
/*
 * For tests and tools: what makes the selection observable and forcible (tests/test_gpu_gemm_solutions.py).  None of them launches
 * anything or changes how a call selects.
 * odtk_debug_gemm_candidates -- the solutions a plan for the problem chooses from: the heuristic's candidates (up to 16) whose
 * state is success and whose workspace fits `workspace_size`, as solution indices in heuristic order.  Returns their number and
 * writes at most `capacity` of them (indices may be NULL when capacity is 0); 0 when the library offers nothing.  Built by the
 * code the planner itself uses.  ODTK_ERR_INVALID: m, n or k < 1, capacity < 0, NULL indices with capacity > 0;
 * ODTK_ERR_UNSUPPORTED: another dtype (both decided before the library is touched), or hipBLASLt cannot be bound;
 * ODTK_ERR_HIP: no device (the library's handle needs one).
 * odtk_gemm_plan_clear -- destroys every cached plan, forgets every imported line and zeroes the miss count: an import of one
 * line followed by one call then runs that problem on the named solution.
 * odtk_gemm_last_solution -- the solution index the most recent odtk_gemm_bias_act of the process ran (-1: none yet) and, in
 * *origin (may be NULL), how its plan was made.  The GEMM's counterpart of odtk_conv_last_plan in include/odtk_conv.h.
 */
#define ODTK_GEMM_ORIGIN_TIMED   0   /* the fastest candidate by the stopwatch                          */
#define ODTK_GEMM_ORIGIN_PINNED  1   /* named by an imported line                                       */
#define ODTK_GEMM_ORIGIN_CAPTURE 2   /* first usable candidate: first seen while a stream was captured  */
int odtk_debug_gemm_candidates(size_t m, int n, int k, int dtype, int relu, int residual, size_t workspace_size,
                               int *indices, int capacity);
void odtk_gemm_plan_clear(void);
int odtk_gemm_last_solution(int *origin);
int odtk_gemm_bias_act(void *y, const void *x, const void *w, const float *bias, const void *residual,
                       size_t m, int n, int k, int dtype, int relu,
                       void *workspace, size_t workspace_size, void *stream);
/*
 * odtk_bottleneck_seam -- the seam between two bottleneck blocks as ONE pass (csrc/seam.hpp): the last 1x1 convolution of a block
 * with its skip and ReLU, and the first 1x1 convolution of the next block with its ReLU, which reads the first one's output from
 * registers instead of from memory:
 *     out[p][c] = rne(relu( sum_k y2[p][k] * w3[c][k] + b3[c] + skip[p][c] ))          c < c_mid,  k < c_in
 *     z[p][n]   = rne(relu( sum_c out[p][c] * w1[n][c] + b1[n] ))                      n < c_next
 * fp32 sums, rne = round-to-nearest-even to `dtype`; the second product reads the ROUNDED out, so both outputs are what the two
 * odtk_gemm_bias_act calls it replaces define (up to the order of the fp32 sums).  y2 [m, c_in], skip and out [m, c_mid],
 * z [m, c_next], w3 [c_mid, c_in], w1 [c_next, c_mid]: device, row-major, `dtype` (ODTK_BF16 / ODTK_F16), 16-byte aligned;
 * b3 [c_mid] and b1 [c_next]: DEVICE float32.  The outputs must not alias each other or an input.
 * ODTK_ERR_INVALID: a null, aliased or misaligned pointer, a channel count < 1.  ODTK_ERR_UNSUPPORTED: another dtype, or channel
 * counts other than c_in = 64, c_mid = 256, c_next = 64 | 128 (ResNet-50/101/152's layer1 and its hand-over to layer2: the weights
 * of the later layers do not fit the LDS beside the tile).  No workspace; one launch, timed under ODTK_KERNEL_SEAM.
 * No reference equivalent as a kernel (torchvision Bottleneck.forward, reference odtk/backbones/resnet.py).
 */
int odtk_bottleneck_seam(void *out, void *z, const void *y2, const void *skip, const void *w3, const float *b3, const void *w1,
                         const float *b1, size_t m, int c_in, int c_mid, int c_next, int dtype, void *stream);

/*
 * odtk_tower_conv3x3 -- the 3x3 convolutions of the head towers as an own implicit-GEMM MFMA kernel (csrc/tower_conv.hpp):
 *     y[b][i][j][n] = rne(act( rne( sum_{kh, kw, c} x[b][i + kh - 1][j + kw - 1][c] * w[n][kh][kw][c] ) + bias[n] ))
 * stride 1, padding 1 (positions outside the image read as zero), fp32 sums in a fixed order (the same input gives the same bits
 * on every launch; the order of the library's 256 x 256 x 32 instance, whose finite results it reproduces bit for bit), rne =
 * round-to-nearest-even to `dtype`, act = ReLU if relu != 0: the two roundings of the convolution library's entry point (include/odtk_conv.h), whose
 * drop-in this is -- except that a NaN sum comes out as NaN, as odtk_bias_act hands it on.
 *   x [batch, height, width, c_in] and y [batch, height, width, c_out]: channels_last activations of `dtype` (ODTK_BF16 / ODTK_F16);
 *   w [c_out, 3, 3, c_in] (a torch weight in channels_last memory format) and bias [c_out]: of `dtype` too.  All device, 16-byte
 *   aligned; y must not be x.
 * ODTK_ERR_INVALID: a null or misaligned pointer, y == x, an extent or channel count < 1.  ODTK_ERR_UNSUPPORTED: another dtype,
 * c_in != 256 or c_out != 256, or batch * height * width >= 2^22 pixels (32-bit byte offsets).  No workspace, nothing allocated
 * or uploaded: one launch, capturable in a hipGraph, timed under ODTK_KERNEL_TOWER_CONV.
 * No reference equivalent as a kernel (the reference's heads are nn.Conv2d + ReLU: odtk/model.py:57-62).
 */
int odtk_tower_conv3x3(void *y, const void *x, const void *w, const void *bias, int batch_size, int height, int width, int c_in,
                       int c_out, int dtype, int relu, void *stream);
/* Debug / A-B: launch variant of odtk_tower_conv3x3, two bits.  Bit 0 (set by default): tile ids permuted so that the workgroups
 * sharing an L2 (ids equal mod 8) own consecutive tiles, whose halo rows overlap; clear: workgroup k owns tile k (0 .. 2 % slower).
 * Bit 1 (clear by default): the MFMA form.  Clear: v_mfma_f32_32x32x16 with the k grouping of the convolution library's
 * 256 x 256 x 32 instance -- the result equals that instance's bit for bit; set: v_mfma_f32_16x16x32 over 32 consecutive k, 8 %
 * faster, one output in 50 000 a bf16 step away (profiles/tower_conv_probe.txt).  Default 1.  -1 reads the current value; returns the
 * previous one, ODTK_ERR_INVALID for any other argument.  Process-wide; never touches HIP. */
int odtk_debug_tower_conv_variant(int variant);

/*
 * odtk_snap_to_anchors -- fused training-target assignment for ONE pyramid level of the whole batch.
 * Replaces the reference's pure-torch snap_to_anchors (odtk/box.py:134-189, called per image and
 * level from odtk/model.py:167-184): IoU of every anchor against every ground-truth box (+1 pixel
 * convention), first maximum wins, regression deltas (box2delta, box.py:67-78), depth
 * (-1 ignore / 0 background / class+1) and the one-hot class map.
 *   targets     float32 [batch, n_max, 5] = (x, y, w, h, class); rows with class < 0 are padding
 *   anchors     HOST float[4*num_anchors]
 *   cls_target  float32 [batch, A, C, H, W]   box_target [batch, A, 4, H, W]   depth [batch, A, 1, H, W]
 * Any n_max (rows go through LDS 1024 at a time).  cls_target may be NULL when the caller feeds
 * odtk_retina_loss_* (which derives the class target from depth) and does not need the one-hot map.
 */
int odtk_snap_to_anchors(int batch_size, const float *targets, int n_max, const float *anchors,
                         int num_anchors, int num_classes, int height, int width, int stride,
                         float iou_background, float iou_foreground,
                         float *cls_target, float *box_target, float *depth, void *stream);

/* ... and all pyramid levels in ONE launch (a level table in the kernel arguments; n_levels <= ODTK_MAX_LEVELS). */
typedef struct odtk_snap_level {
  const float *anchors;       /* HOST float[4*num_anchors] of this level's stride */
  float *cls_target;          /* [batch, A, C, H, W] or NULL */
  float *box_target;          /* [batch, A, 4, H, W] */
  float *depth;               /* [batch, A, 1, H, W] */
  int32_t height, width, stride, pad_;
} odtk_snap_level_t;
int odtk_snap_to_anchors_levels(int batch_size, const float *targets, int n_max, int n_levels,
                                const odtk_snap_level_t *levels, int num_anchors, int num_classes,
                                float iou_background, float iou_foreground, void *stream);

/*
 * odtk_atss_assign_levels -- ATSS target assignment (adaptive training sample selection, Zhang et al., CVPR 2020) for all pyramid
 * levels of the batch: the alternative to the fixed-IoU rule above, axis-aligned boxes only.  No reference equivalent; the
 * definition -- the contract -- is spelled out in csrc/atss.hpp and restated in numpy in tests/atss_ref.py:
 *   per box and level the `topk` cells whose centres are nearest to the box centre (ties: lower cell index) are its candidates,
 *   with all their anchors; t = mean + sample standard deviation of the candidates' IoUs over ALL levels (float64, summed in list
 *   order); a candidate is positive when its IoU >= t and its cell centre lies more than 0.01 inside the box; an anchor positive
 *   for several boxes goes to the largest IoU (ties: the earliest row).
 * Inputs and outputs as for the levels form of the fixed-IoU rule (its level descriptor is reused), except that
 * depth is class + 1 or 0 -- ATSS has no ignore band -- and that every element of every output is written by this call.  n_max == 0
 * or only padding rows: all outputs zero.  A small box that contains no cell centre gets no positives: that is ATSS.
 * Two launches (one wave per target row: candidates + threshold into the workspace; one thread per anchor: assignment), no
 * atomics, timed under ODTK_KERNEL_ATSS_STATS and ODTK_KERNEL_TARGETS.  Workspace: 96 bytes per target row and level (two-phase query).
 * ODTK_ERR_INVALID: null pointers, n_levels outside 1..ODTK_MAX_LEVELS, topk outside 1..ODTK_ATSS_MAX_TOPK, num_anchors outside
 * 1..ODTK_MAX_ANCHORS, non-positive sizes or strides, batch_size > 65535, levels or workspaces beyond 2^31 - 1.
 */
int odtk_atss_assign_levels(int batch_size, const float *targets, int n_max, int n_levels,
                            const odtk_snap_level_t *levels, int num_anchors, int num_classes, int topk,
                            void *workspace, size_t workspace_size, void *stream);

/*
 * odtk_tal_assign_levels -- task-aligned target assignment (TOOD, Feng et al., ICCV 2021; the assigner of PP-YOLOE and YOLOv8) for
 * all pyramid levels of the batch: the assigner that looks at what the network predicts, axis-aligned boxes only.  No reference
 * equivalent; the definition -- the contract -- is spelled out in csrc/tal.hpp and restated in numpy in tests/tal_ref.py:
 *   a row is valid when its class is a whole number in 0..num_classes-1; its candidates are all anchors whose cell centre lies more
 *   than 0.01 inside the box; m = s^alpha * u^beta by repeated float32 multiplication, s the sigmoid of the logit of the row's class
 *   at the anchor, u the IoU of the box the deltas decode to there (no clamp to the image) with the row's box; the row selects its
 *   `topk` candidates with the largest m over all levels together (NaN never, 0 eligible; ties: the lower global anchor index); an
 *   anchor selected by several rows goes to the largest u (ties: the earliest row).
 * `levels` (anchors, outputs, H, W, stride) as for ATSS; `heads` gives per level the class logits [batch, A*C, H, W] and box deltas
 * [batch, A*4, H, W] of element type `dtype`, as the convolutions wrote them (cls, box, channels_last; every other field is
 * ignored).  topk in 1..ODTK_ATSS_MAX_TOPK, alpha in 0..4, beta in 1..8.  depth is class + 1 or 0 -- no ignore band -- and every
 * element of every output is written by this call.  n_max == 0 or only padding rows: all outputs zero.
 * Three launches (one workgroup per target row: a streaming top-k selection into the workspace; zeros to the outputs; one thread
 * per selected entry: conflicts and the winners' targets), no atomics, timed under ODTK_KERNEL_ATSS_STATS (the selection) and
 * ODTK_KERNEL_TARGETS.  Workspace: 144 bytes per target row (two-phase query); too small: ODTK_ERR_WORKSPACE.
 * ODTK_ERR_INVALID: null pointers (cls_target excepted), n_levels outside 1..ODTK_MAX_LEVELS, num_anchors outside
 * 1..ODTK_MAX_ANCHORS, topk, alpha or beta out of range, num_classes < 1, non-positive sizes or strides, batch_size outside
 * 1..65535, a level or a total anchor count beyond 2^31 - 1, heads misaligned for their element.  Another dtype:
 * ODTK_ERR_UNSUPPORTED.  Everything is checked on the host before anything is enqueued.
 */
struct odtk_loss_level;
int odtk_tal_assign_levels(int batch_size, const float *targets, int n_max, int n_levels,
                           const odtk_snap_level_t *levels, const struct odtk_loss_level *heads,
                           int num_anchors, int num_classes, int dtype, int topk, int alpha, int beta,
                           void *workspace, size_t workspace_size, void *stream);

/*
 * odtk_snap_to_anchors_rotated_levels -- the same assignment for ROTATED boxes (reference odtk/box.py:192-252, whose overlap is
 * the pairwise polygon IoU csrc/cuda/nms_iou.cu:324-387), all pyramid levels of the batch in ONE launch: no [27*H*W, N] IoU
 * matrix, no per-image host loop.  The ground truth arrives as the reference's `rotate_boxes` leaves it (utils.py:33-82):
 *   gt_axis   float32 [batch, n_max, 6] = (x1, y1, x2, y2, sin, cos)      gt_quads  float32 [batch, n_max, 8] ordered corners
 *   gt_class  float32 [batch, n_max], rows with class < 0 are padding
 * and per level DEVICE tables of the anchors (generate_anchors_rotated: axis form [A, 4] and quads [A, 8]):
 *   cls_target [batch, A, C, H, W] (or NULL)   box_target [batch, A, 6, H, W]   depth [batch, A, 1, H, W]
 */
typedef struct odtk_snap_rot_level {
  const float *anchors_axis;  /* DEVICE float[4*num_anchors] */
  const float *anchors_quads; /* DEVICE float[8*num_anchors] */
  float *cls_target;          /* or NULL */
  float *box_target;
  float *depth;
  int32_t height, width, stride, pad_;
} odtk_snap_rot_level_t;
int odtk_snap_to_anchors_rotated_levels(int batch_size, const float *gt_axis, const float *gt_quads, const float *gt_class,
                                        int n_max, int n_levels, const odtk_snap_rot_level_t *levels, int num_anchors,
                                        int num_classes, float iou_background, float iou_foreground, void *stream);

/*
 * odtk_retina_loss_forward / odtk_retina_loss_backward -- fused, masked FocalLoss + SmoothL1 reduction of ONE
 * pyramid level for the whole batch (the step after target assignment in training).
 * Replaces, per level, reference odtk/model.py:193-209 + odtk/loss.py:13-31 (focal loss, smooth-L1, the two
 * masks, the three sums: ~20 elementwise torch kernels over the classification head and their autograd twins).
 *   cls         [batch, A*C, H, W] logits          dtype ODTK_F32 / BF16 / F16, NCHW or channels_last,
 *   box         [batch, A*box_params, H, W]        same dtype and layout as cls, 16-byte aligned
 *   depth       float32 [batch, A, 1, H, W]        -1 ignore / 0 background / class + 1 (odtk_snap_to_anchors)
 *   box_target  float32 [batch, A, box_params, H, W]
 * The one-hot class target is not an input: under the mask `depth >= 0` it equals `c == depth - 1`.
 * forward:  sums = DEVICE double[3], overwritten with { sum of masked focal losses, sum of masked smooth-L1
 *           losses, number of foreground anchors (depth > 0) }.
 * backward: grad_cls_sum / grad_box_sum = DEVICE float32 scalars (upstream gradients of the two sums; NULL = 0);
 *           dcls / dbox receive d(out)/d(cls) and d(out)/d(box) in the dtype and layout of cls / box.
 * Nothing is read back to the host.  batch*A*C*H*W must be < 2^32.
 */
int odtk_retina_loss_forward(const void *cls, const void *box, const float *depth, const float *box_target,
                             int batch_size, int num_anchors, int num_classes, int height, int width,
                             int box_params, int dtype, int channels_last, float alpha, float gamma, float beta,
                             double *sums, void *stream);
int odtk_retina_loss_backward(const void *cls, const void *box, const float *depth, const float *box_target,
                              int batch_size, int num_anchors, int num_classes, int height, int width,
                              int box_params, int dtype, int channels_last, float alpha, float gamma, float beta,
                              const float *grad_cls_sum, const float *grad_box_sum, void *dcls, void *dbox,
                              void *stream);

/*
 * odtk_retina_loss_levels_forward / _backward -- the same reduction for ALL pyramid levels of the batch in ONE launch
 * per direction (a training step: two launches instead of ten).  Per level: the tensors of odtk_retina_loss_*; every
 * level shares batch, num_anchors, num_classes, box_params, dtype.
 *   forward:  sums = DEVICE double[n_levels][3] (cls_sum, box_sum, foreground count per level), overwritten.
 *   backward: grad_cls_sums / grad_box_sums = DEVICE float32 [n_levels] (NULL = zeros); levels[l].dcls / .dbox receive
 *             the gradients (forward ignores them).
 */
typedef struct odtk_loss_level {
  const void *cls;            /* [batch, A*C, H, W] logits                                   */
  const void *box;            /* [batch, A*box_params, H, W]                                 */
  const float *depth;         /* float32 [batch, A, 1, H, W]                                 */
  const float *box_target;    /* float32 [batch, A, box_params, H, W]                        */
  void *dcls, *dbox;          /* backward outputs, dtype / layout of cls / box               */
  int32_t height, width;
  int32_t channels_last;      /* layout of cls and box: 0 NCHW, 1 NHWC                       */
  int32_t pad_;
} odtk_loss_level_t;

int odtk_retina_loss_levels_forward(int n_levels, const odtk_loss_level_t *levels, int batch_size, int num_anchors,
                                    int num_classes, int box_params, int dtype, float alpha, float gamma, float beta,
                                    double *sums, void *stream);
/* The forward through a workspace: every workgroup writes its three sums to the workspace and a second (tiny) launch adds
 * them up in a fixed order -- no atomics (the plain form above ends every workgroup in a double atomic on its level's
 * word, which bounds how many workgroups it can afford: DESIGN.md section 4) and a result that is bitwise reproducible
 * from run to run.  Two-phase: workspace == NULL returns the bytes needed for these shapes; `sums` is overwritten. */
int odtk_retina_loss_levels_forward_ws(int n_levels, const odtk_loss_level_t *levels, int batch_size, int num_anchors,
                                       int num_classes, int box_params, int dtype, float alpha, float gamma, float beta,
                                       double *sums, void *workspace, size_t workspace_size, void *stream);
int odtk_retina_loss_levels_backward(int n_levels, const odtk_loss_level_t *levels, int batch_size, int num_anchors,
                                     int num_classes, int box_params, int dtype, float alpha, float gamma, float beta,
                                     const float *grad_cls_sums, const float *grad_box_sums, void *stream);

/*
 * odtk_box_iou_loss_levels_forward / _backward -- IoU, GIoU or DIoU box-regression loss at the foreground anchors of ALL pyramid
 * levels of the batch: the opt-in alternative to the smooth-L1 sum above (Model.box_loss, `odtk train --box-loss`), axis-aligned
 * boxes only.  No reference equivalent; the definition -- the contract -- restated in torch in odtk/loss.py:box_iou_loss:
 *   one foreground anchor (depth > 0) of anchor slot a, (aw, ah) = (x2 - x1 + 1, y2 - y1 + 1) of the level's anchor table,
 *   p = the predicted deltas (head dtype -> float32), t = the target deltas; both boxes decoded relative to the anchor centre:
 *     CLIP = log(1000 / 16);  pw' = min(pw, CLIP), ph' = min(ph, CLIP)       (predictions only; gradient 0 beyond the clip)
 *     P: centre (px aw, py ah), size (exp(pw') aw, exp(ph') ah)             T: the same from t, unclipped
 *     inter = max(0, min(Px2, Tx2) - max(Px1, Tx1)) max(0, min(Py2, Ty2) - max(Py1, Ty1))     (corners: centre -+ size / 2)
 *     union = area(P) + area(T) - inter + eps,  iou = inter / union,  eps = 1e-7;  (ew, eh) = size of the box enclosing both
 *     ODTK_BOX_LOSS_IOU : L = 1 - iou
 *     ODTK_BOX_LOSS_GIOU: c = ew eh + eps,         L = 1 - iou + (c - union) / c
 *     ODTK_BOX_LOSS_DIOU: c2 = ew^2 + eh^2 + eps,  L = 1 - iou + ((Pcx - Tcx)^2 + (Pcy - Tcy)^2) / c2
 * The level descriptor of the smooth-L1 entry points is reused: `cls` / `dcls` are ignored and may be NULL, box has 4 parameters
 * per anchor by definition.  `anchors`: HOST array of n_levels pointers to HOST float[4 * num_anchors] (only the sizes are used).
 *   forward:  sums = DEVICE double[n_levels][2] = (sum of L over the level's foreground anchors, their number), overwritten.  The
 *             sum is accumulated in float64 in one fixed order (per-workgroup sums in the workspace, added up by a second, tiny
 *             launch): no atomics, the same bits on every run.  Workspace: two-phase query as everywhere.
 *   backward: grad_sums = DEVICE float32[n_levels] (NULL = zeros), read on the device; levels[l].dbox receives grad_sums[l] dL/dp
 *             at the foreground cells and +0 everywhere else -- every element is written -- in the dtype and layout of box,
 *             rounded once at the store.  At a tie (min / max / clamp, inter = 0, pw = CLIP) the gradient is that of one side.
 * A NaN delta at a foreground anchor gives a NaN sum; cells that are not foreground are never read from box.  Arithmetic: IEEE
 * float32 per anchor.  Everything is checked on the host before anything touches HIP.  ODTK_ERR_INVALID: a null pointer,
 * n_levels outside 1..ODTK_MAX_LEVELS, num_anchors outside 1..ODTK_MAX_ANCHORS, batch_size < 1, a non-positive size, an
 * undefined kind, an anchor whose width or height is not finite and > 0, a level with batch * A * 4 * H * W >= 2^31, a misaligned
 * pointer (channels_last: 16 bytes for fp32 heads, 8 for 16-bit ones), a workspace that is too small.  Another dtype is
 * ODTK_ERR_UNSUPPORTED.  One launch per direction over one lane per anchor cell (csrc/box_iou_loss.hpp), timed under
 * ODTK_KERNEL_LOSS; the forward's second launch under ODTK_KERNEL_LOSS_REDUCE.
 */
#define ODTK_BOX_LOSS_IOU   1
#define ODTK_BOX_LOSS_GIOU  2
#define ODTK_BOX_LOSS_DIOU  3
int odtk_box_iou_loss_levels_forward(int n_levels, const odtk_loss_level_t *levels, const float *const *anchors, int batch_size,
                                     int num_anchors, int dtype, int kind, double *sums, void *workspace, size_t workspace_size,
                                     void *stream);
int odtk_box_iou_loss_levels_backward(int n_levels, const odtk_loss_level_t *levels, const float *const *anchors, int batch_size,
                                      int num_anchors, int dtype, int kind, const float *grad_sums, void *stream);

/*
 * odtk_rotated_box_loss_levels_forward / _backward -- ProbIoU (arXiv 2106.06072) or KLD (arXiv 2106.01883) box-regression loss on
 * the Gaussians of ROTATED boxes, at the foreground anchors of ALL pyramid levels of the batch: the opt-in alternative to the
 * smooth-L1 sum on the six deltas (Model.box_loss, `odtk train --rotated-bbox --box-loss probiou|kld`).  No reference equivalent;
 * the definition -- the contract -- restated in torch in odtk/loss.py:rotated_box_loss:
 *   one foreground anchor (depth > 0) of anchor slot a, (aw, ah) = (x2 - x1 + 1, y2 - y1 + 1) of the level's AXIS anchor table,
 *   p = the six predicted deltas (head dtype -> float32), t = the six target deltas, (t4, t5) the box's (sin, cos); both boxes
 *   decoded relative to the anchor centre:
 *     CLIP = log(1000 / 16);  pw' = min(p2, CLIP), ph' = min(p3, CLIP)       (predictions only; gradient 0 beyond the clip)
 *     centre (p0 aw, p1 ah);  w = exp(pw') aw,  h = exp(ph') ah              target: the same from t, unclipped
 *     q = p4^2 + p5^2 + 1e-12;  cc = p5^2 / q,  ss = p4^2 / q,  sc = p4 p5 / q       (target: the same from t4, t5)
 *     a = (w^2 cc + h^2 ss) / 12     b = (w^2 ss + h^2 cc) / 12     c = -(w^2 - h^2) sc / 12
 *   [[a, c], [c, b]]: the covariance of the uniform distribution on the rotated rectangle, width axis (cos, -sin), height axis
 *   (sin, cos) as in odtk/box.py:rotate_boxes.  Index 1 the prediction, 2 the target; (dx, dy) = centre(P) - centre(T):
 *     ODTK_ROTATED_BOX_LOSS_PROBIOU: A = a1 + a2, B = b1 + b2, C = c1 + c2, D = A B - C^2
 *         BD = (B dx^2 + A dy^2 - 2 C dx dy) / (4 D) + 0.5 ln(36 D / (w h tw th))
 *         BD' = min(max(BD, 0), 100)     L = sqrt(1 - exp(-BD') + 1e-7)                     (gradient 0 where clamped)
 *     ODTK_ROTATED_BOX_LOSS_KLD:     d2 = (tw th / 12)^2
 *         K = 0.5 [(b2 a1 + a2 b1 - 2 c2 c1) / d2 + (b2 dx^2 + a2 dy^2 - 2 c2 dx dy) / d2 - 2] + (t2 + t3 - pw' - ph')
 *         K' = max(K, 0)                 L = 1 - 1 / (1 + ln(1 + K'))                       (gradient 0 where clamped)
 * min / max hand a NaN on: a NaN delta at a foreground anchor gives a NaN sum.  The loss does not depend on the length of
 * (p4, p5): its gradient on the pair is tangential and scales with 1 / sqrt(q); for w = h the angle gradient is 0.
 * The level descriptor of the smooth-L1 entry points is reused: `cls` / `dcls` are ignored and may be NULL, box has 6 parameters
 * per anchor.  `anchors`: HOST array of n_levels pointers to HOST float[4 * num_anchors], the axis tables (only the sizes are used).
 *   forward:  sums = DEVICE double[n_levels][2] = (sum of L over the level's foreground anchors, their number), overwritten;
 *             float64 in one fixed order through the workspace (two-phase query as everywhere): no atomics, the same bits on every run.
 *   backward: grad_sums = DEVICE float32[n_levels] (NULL = zeros), read on the device; levels[l].dbox receives grad_sums[l] dL/dp
 *             for all six deltas at the foreground cells and +0 everywhere else -- every element is written -- in the dtype and
 *             layout of box, rounded once at the store.
 * Cells that are not foreground are never read from box.  Arithmetic: the float32 deltas widened, IEEE double per anchor (BD and K
 * are small differences of O(1) terms; csrc/rotated_box_loss.hpp).  Everything is checked on the host
 * before anything touches HIP.  ODTK_ERR_INVALID: a null pointer, n_levels outside 1..ODTK_MAX_LEVELS, num_anchors outside
 * 1..ODTK_MAX_ANCHORS, batch_size < 1, a non-positive size, an undefined kind, an anchor whose width or height is not finite and
 * > 0, a level with batch * A * 6 * H * W >= 2^31, a misaligned pointer (channels_last: a cell is three pieces of 8 bytes for fp32
 * heads, of 4 for 16-bit ones), a workspace that is too small.  Another dtype is ODTK_ERR_UNSUPPORTED.  One launch per direction
 * over one lane per anchor cell (csrc/rotated_box_loss.hpp), timed under ODTK_KERNEL_LOSS; the forward's second launch under
 * ODTK_KERNEL_LOSS_REDUCE.
 */
#define ODTK_ROTATED_BOX_LOSS_PROBIOU  1
#define ODTK_ROTATED_BOX_LOSS_KLD      2
int odtk_rotated_box_loss_levels_forward(int n_levels, const odtk_loss_level_t *levels, const float *const *anchors, int batch_size,
                                         int num_anchors, int dtype, int kind, double *sums, void *workspace, size_t workspace_size,
                                         void *stream);
int odtk_rotated_box_loss_levels_backward(int n_levels, const odtk_loss_level_t *levels, const float *const *anchors, int batch_size,
                                          int num_anchors, int dtype, int kind, const float *grad_sums, void *stream);

/*
 * odtk_quality_loss_levels_forward / _backward -- Quality Focal Loss (GFL, arXiv 2006.04388 eq. 4) or Varifocal Loss (arXiv
 * 2008.13367 eq. 2, as mmdetection implements it) over the class logits of ALL pyramid levels of the batch: the opt-in
 * alternatives to the focal sum of odtk_retina_loss_* (Model.cls_loss, `odtk train --cls-loss`), axis-aligned boxes only.  No
 * reference equivalent; the definition -- the contract -- restated in torch in odtk/loss.py (quality_focal_loss, varifocal_loss,
 * box_quality, quality_target):
 *   x = a class logit (head dtype -> float32), s = sigmoid(x), sp = softplus(x); depth as everywhere (-1 / 0 / class + 1);
 *   q = 1 - (the ODTK_BOX_LOSS_IOU loss above of the anchor's predicted and target deltas), foreground anchors only: a constant
 *       of this loss (nothing flows into the box head), NaN where a delta is NaN;
 *   y = q where depth - 1 == class, else 0; elements of ignored anchors (depth < 0) contribute 0 and get gradient +0;
 *     ODTK_CLS_LOSS_QFL (gamma >= 1): L = |s - y|^gamma (sp - y x), with y x = 0 where y = 0 whatever the logit
 *     ODTK_CLS_LOSS_VFL (alpha >= 0): y > 0 (or NaN): L = y (sp - y x);  otherwise: L = alpha s^gamma sp
 * The level descriptor is reused once more: `dbox` is ignored and may be NULL (d(deltas) is never written); `anchors` as for the
 * box losses.  Every level shares batch, num_anchors, num_classes and dtype; cls and box share the layout.
 *   forward:  sums = DEVICE double[n_levels][2] = (sum of L over the elements of non-ignored anchors, number of foreground anchors),
 *             overwritten; float64 in one fixed order through the workspace (two-phase query as everywhere): the same bits on every run.
 *   backward: grad_sums = DEVICE float32[n_levels] (NULL = zeros), read on the device; levels[l].dcls receives grad_sums[l] dL/dx,
 *             every element written, in the dtype and layout of cls, rounded once at the store.
 * The box head is never read at a cell that is not foreground.  Everything is checked on the host before anything touches HIP.
 * ODTK_ERR_INVALID: what the box losses refuse, a null or misaligned cls / dcls (16 bytes), num_classes < 1, an undefined kind, a
 * gamma that is not finite or < 1, an alpha that is not finite or < 0, a level with batch * A * C * H * W >= 2^32.  A workspace
 * that is too small is ODTK_ERR_WORKSPACE, another dtype ODTK_ERR_UNSUPPORTED.  One streaming launch per direction
 * (csrc/quality_loss.hpp), timed under ODTK_KERNEL_LOSS; the forward's second launch under ODTK_KERNEL_LOSS_REDUCE.
 */
#define ODTK_CLS_LOSS_QFL   1
#define ODTK_CLS_LOSS_VFL   2
int odtk_quality_loss_levels_forward(int n_levels, const odtk_loss_level_t *levels, const float *const *anchors, int batch_size,
                                     int num_anchors, int num_classes, int dtype, int kind, float alpha, float gamma, double *sums,
                                     void *workspace, size_t workspace_size, void *stream);
int odtk_quality_loss_levels_backward(int n_levels, const odtk_loss_level_t *levels, const float *const *anchors, int batch_size,
                                      int num_anchors, int num_classes, int dtype, int kind, float alpha, float gamma,
                                      const float *grad_sums, void *stream);

/*
 * odtk_optim_sgd_step / odtk_optim_grad_norm -- the optimisation step of training as one streaming pass over the parameters
 * (odtk/optim.py: FusedSGD, ModelEMA; `odtk train --ema / --clip-grad-norm / --fused-step`), and the global L2 norm of the
 * gradients as one more pass.  No reference equivalent (the reference steps with torch.optim.SGD); the definition -- the contract --
 * restated in torch in odtk/optim.py (FusedSGD._step_reference), every operation in float32 and rounded on its own:
 *   skipped -- nothing is written -- when found_inf is given and *found_inf != 0, or norm_state is given and its skip word is set;
 *   otherwise per element, with p, buf, e the element of param, momentum, ema:
 *     g = grad;  g = g / *grad_scale (grad_scale given);  g = g * coef (norm_state given);  g = g + weight_decay * p (weight_decay != 0)
 *     buf = first ? g : (momentum * buf) + g;   p = p - (lr * buf);   e = e + one_minus_decay * (p - e) (the tensor's ema given)
 * which is torch's SGD (dampening 0, no Nesterov) behind GradScaler's unscale and clip_grad_norm_'s factor, and lerp for the EMA.
 *   tensors      HOST array of 1..ODTK_MAX_OPTIM_TENSORS descriptors of DEVICE float32 arrays of `numel` contiguous elements each;
 *                they travel by value in the launch (a model with more tensors takes several calls).  numel == 0 is legal and the
 *                tensor is skipped; `ema` may be NULL per tensor; `momentum` is not read when first != 0.  A tensor whose four
 *                pointers are all 16-byte aligned is walked with 16-byte accesses, any other element by element: the same bits.
 *   grad_scale, found_inf   DEVICE float32 scalars in torch.amp.GradScaler's layout, each may be NULL; never read on the host.
 *   norm_state   NULL, or the DEVICE state odtk_optim_grad_norm wrote: 16 bytes = float32 norm, float32 coef, uint32 skip, uint32 0.
 *   one_minus_decay   1 - the EMA's decay, in [0, 1].
 * odtk_optim_grad_norm: norm = float32(sqrt(sum over every element of double(g') * double(g'))) with g' = g / *grad_scale in float32
 * (grad_scale given), the value the step will use; the squares are exact in double and added in double in one fixed order (lane,
 * wave, workgroup, then one slot of the workspace per workgroup; the second launch is ONE workgroup that adds the slots up): the
 * same bits on every run, no atomics.  It writes norm, coef = min(1, max_norm / (norm + 1e-6f)) in float32 (clip_grad_norm_'s
 * factor; NaN stays NaN) and skip = (norm is not finite) to `state`.  Only `grad` and `numel` of a descriptor are read.
 * odtk_optim_grad_norm_chained is the same for a model of more than ODTK_MAX_OPTIM_TENSORS tensors: every call of the chain passes
 * the SAME workspace and the number of slots the calls before it filled (prior_slots; a call fills one slot per started chunk
 * of ODTK_OPTIM_CHUNK elements of each of its tensors, behind those), and the call with last != 0 adds all of them up in index
 * order and writes the state; max_norm and state are looked at in that call only.  odtk_optim_grad_norm is the chain of one.
 * Workspace (the norm): two-phase query as everywhere, 8 bytes per slot up to this call's last one; too small: ODTK_ERR_WORKSPACE.
 * Everything is checked on the host before anything touches HIP.  ODTK_ERR_INVALID: n_tensors outside 1..ODTK_MAX_OPTIM_TENSORS, a
 * NULL tensor list, a negative numel, a NULL param / grad / momentum (the norm: grad) in a tensor with numel > 0, a pointer that
 * is not aligned to its element, a first other than 0 / 1, an lr, momentum or weight_decay that is not finite, a one_minus_decay
 * outside [0, 1], a max_norm that is not finite or not > 0, a NULL state, a negative prior_slots, more than 2^31 - 1 chunks.
 * One launch per call of the step, timed under ODTK_KERNEL_EPILOGUE; the norm's launches are timed under
 * ODTK_KERNEL_LOSS_REDUCE.  No allocation, no host synchronisation: capturable in a hipGraph.
 */
#define ODTK_MAX_OPTIM_TENSORS 64     /* descriptors per call: they travel by value, kernargs stay < 4 KiB */
#define ODTK_OPTIM_CHUNK 4096         /* elements of one tensor a workgroup owns */
typedef struct odtk_optim_tensor {
  float *param;
  const float *grad;
  float *momentum;
  float *ema;                         /* may be NULL */
  int64_t numel;
} odtk_optim_tensor_t;      /* 40 bytes; odtk_abi_struct_size id 17 */
int odtk_optim_grad_norm(int n_tensors, const odtk_optim_tensor_t *tensors, const float *grad_scale, float max_norm, void *state,
                         void *workspace, size_t workspace_size, void *stream);
int odtk_optim_grad_norm_chained(int n_tensors, const odtk_optim_tensor_t *tensors, const float *grad_scale, float max_norm, void *state,
                                 int prior_slots, int last, void *workspace, size_t workspace_size, void *stream);
int odtk_optim_sgd_step(int n_tensors, const odtk_optim_tensor_t *tensors, float lr, float momentum, float weight_decay, int first,
                        float one_minus_decay, const float *grad_scale, const float *found_inf, const void *norm_state, void *stream);

/* ------------------------------------------------------------------------------------------
 * Measurement hooks (used by bench.py; off by default, zero cost when off).
 * While enabled, a kernel launch of this library carries a hipEvent pair (asynchronous -- still no
 * host synchronisation): the post-processing, target and loss kernels hand the pair to the launch
 * itself (hipExtLaunchKernelGGL), so the two events hold the dispatch's own begin / end timestamps --
 * the figures rocprofv3's kernel trace reports -- and so do, since round 4, the epilogue kernels (bias_act, the stem's
 * pool pass, the upsampling); only odtk_gemm_bias_act, whose kernels hipBLASLt launches itself, records the pair around
 * the call (marker packets: the dispatch latency is inside the figure on both sides).  odtk_profile_collect waits for the recorded events, accumulates per-kernel elapsed
 * milliseconds and launch counts, and clears the pool.  Kernel ids: */
#define ODTK_KERNEL_PREFILTER 0   /* prefilter_scan_kernel                         */
#define ODTK_KERNEL_SELECT    1   /* select_decode_kernel                          */
#define ODTK_KERNEL_NMS       2   /* nms_kernel                                    */
#define ODTK_KERNEL_IOU       3   /* iou_pairs_kernel                              */
#define ODTK_KERNEL_EPILOGUE  4   /* bias_act_kernel (+ its scalar tail form)      */
#define ODTK_KERNEL_TARGETS   5   /* snap_to_anchors_kernel                        */
#define ODTK_KERNEL_GEMM      6   /* hipBLASLt kernels behind odtk_gemm_bias_act    */
#define ODTK_KERNEL_LOSS      7   /* retina_loss_kernel (forward and backward)      */
#define ODTK_KERNEL_SELHIST   8   /* (rounds 2-3: the selection's histogram launch; no longer launched, id kept) */
#define ODTK_KERNEL_SELFILTER 9   /* (rounds 2-3: the selection's filter launch; no longer launched, id kept)    */
#define ODTK_KERNEL_NMS_ORDER 10  /* nms_kernel, stage 1 (rotated: the first round in order)   */
#define ODTK_KERNEL_NMS_MATRIX 11 /* rotated_sup_matrix_kernel (rotated: pairwise suppression) */
#define ODTK_KERNEL_POOL      12  /* bias_act_maxpool_kernel (the stem's bias + ReLU + max-pool pass)  */
#define ODTK_KERNEL_UPSAMPLE  13  /* upsample_nearest2x_kernel                                         */
#define ODTK_KERNEL_STEM_PACK 14  /* stem_pack_kernel (space-to-depth pack of the network input)        */
#define ODTK_KERNEL_LOSS_REDUCE 15 /* loss_reduce_kernel (second launch of the forward through a workspace)   */
#define ODTK_KERNEL_ATSS_STATS 16 /* atss_stats_kernel (ATSS: candidates + threshold; its dense launch counts as ODTK_KERNEL_TARGETS) */
#define ODTK_KERNEL_SEAM      17  /* bottleneck_seam_kernel (conv3 + skip + ReLU and the next conv1 in one pass)      */
#define ODTK_KERNEL_TOWER_CONV 18 /* tower_conv3x3_kernel (the head towers' 3x3 256 -> 256 convolution, implicit GEMM)        */
#define ODTK_KERNEL_COUNT     19
/* on: 0 = off, otherwise a bit mask of kernel ids (1 << ODTK_KERNEL_*), -1 = all.  An event pair
 * is a queue marker before and after the kernel: cheap for the 3 post-processing launches of a step,
 * measurably NOT free for the ~110 epilogue launches (about 10 % of an 8.7 ms step), so time those
 * only in a separate pass. */
int odtk_profile_enable(int on);
/* Debug: device buffer (>= 128 KiB, zero-filled) that select_decode / nms workgroups stamp with wall_clock64()
 * (100 MHz) at their phase boundaries -- coarse stamps in the first 64 KiB, select_decode's per-segment fine-phase stamps
 * (16 words per segment, up to 512 segments) in the second; NULL (default) disables.  Not for production use. */
int odtk_debug_set_trace(void *device_buffer);
/* Debug / tuning: launch shape of the loss kernels for one form (which = 0: forward with atomics, 1: backward, 2: forward
 * through a workspace) and head width (fp32_heads = 0: bf16 / fp16, 1: fp32): workgroup size (multiple of 64, <= 1024),
 * resident workgroups per CU the logit walk is capped at (1..64), 16-byte vectors per lane per trip (1, 2 or 4),
 * workgroups of the box-delta walk (1..16384); both workgroup caps are per pyramid level.  The defaults are the measured
 * best; results do not depend on the shape beyond the order of the partial sums.  Process-wide, not
 * thread-safe against concurrent loss launches; a workspace size queried before a change is stale after it. */
int odtk_debug_loss_tuning(int which, int fp32_heads, int threads, int blocks_per_cu, int unroll, int box_blocks);
/* Debug / A-B: memory layout of the loss kernels' logit walk, per form and head width as above.  per_wave (workspace form
 * only, which = 2): 1 = every wave writes its own three sums to the workspace (3 doubles per WAVE of the launch -- the size
 * query follows) and no workgroup barrier closes the walk; window: 0 = the vectors a lane loads per trip lie one grid
 * stride apart, 1 = a wave's vectors of a trip are contiguous in memory; box_rows (read by the backward on
 * channels_last heads): 1 (default) = the box-delta walk enumerates the cells in the order d(deltas) lies in memory and
 * writes one vector per cell, 0 = in depth's order, one element per store (rounds 2-5).  Results do not depend on any of
 * them beyond the order of the partial sums. */
int odtk_debug_loss_layout(int which, int fp32_heads, int per_wave, int window, int box_rows);
/* Debug: reads back what the two setters above hold for one form and head width: out = threads, blocks_per_cu, unroll,
 * box_blocks, per_wave, window, box_rows.  Before any setter ran these are the shipped defaults.  Never touches HIP; a bad
 * `which` or a NULL `out` returns ODTK_ERR_INVALID.  A caller that changes the launch shape snapshots it here first and puts
 * the snapshot back afterwards, so that no copy of the defaults lives outside the library. */
int odtk_debug_loss_tuning_get(int which, int fp32_heads, int out[7]);
/* Debug / A-B: arithmetic form of the classification walk of the loss kernels when gamma == 2 (csrc/loss.hpp).
 * 0: every logit through the symmetric form (one select on the target, one on the sign);  1: 16-byte vectors that hold no
 * positive element and no logit above 64 (all but ~1 in 1000) through the negatives-only form u = exp(x), q = u / (1 + u),
 * ce = ln(1 + u) -- the same three hardware transcendentals, about a third fewer full-rate operations; every other vector
 * and every other gamma as with 0.  Results agree to ~1e-8 (sums) / ~1e-6 of the largest gradient.  The default is
 * ODTK_LOSS_FORM_DEFAULT; process-wide, read once per launch.  2, 3, 4, 6, 7: TIMING ABLATIONS of form 1 for the fp32
 * forward (no depth gather / no arithmetic / no index arithmetic and no depth gather / no box-delta walk / no logit walk;
 * other launches as form 1) -- their sums are wrong on purpose, tools/loss_form_probe.py is their only user, and they
 * exist only in a library built with -DODTK_LOSS_ABLATIONS (`make ablations` -> build_ablate/): the shipped library
 * accepts 0 and 1.  Returns ODTK_ERR_INVALID for any other value. */
#define ODTK_LOSS_FORM_DEFAULT 1
int odtk_debug_loss_form(int form);
/* Debug: the form odtk_debug_loss_form last set (ODTK_LOSS_FORM_DEFAULT before any call).  Never touches HIP. */
int odtk_debug_loss_form_get(void);
int odtk_profile_collect(double total_ms[ODTK_KERNEL_COUNT], int launches[ODTK_KERNEL_COUNT]);

#ifdef __cplusplus
}
#endif
#endif /* ODTK_HIP_H */
