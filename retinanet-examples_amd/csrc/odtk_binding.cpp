// odtk_binding.cpp -- the reference's operator module (NVIDIA/retinanet-examples csrc/extensions.cpp:47-158, :184-201)
// re-homed on the MI355X C ABI (include/odtk_hip.h, libodtk_hip.so): a compiled torch extension exporting
//
//     decode(cls_head, box_head, anchors, scale, score_thresh, top_n, rotated=False) -> [scores, boxes, classes]
//     nms(scores, boxes, classes, nms_thresh, detections_per_im, rotated=False)     -> [scores, boxes, classes]
//     iou(boxes, anchors)                                                           -> [Tensor[num_anchors, num_boxes]]
//     Engine                                                                        -> placeholder (TensorRT dropped)
//
// with the reference's positional signatures, plus `detect` (all pyramid levels + NMS in one enqueue), `soft_nms`, `matrix_nms`, `box_vote`, `concat_candidates`, `tile_images`, `merge_tile_candidates`, `tal_assign_levels` and `rotated_box_loss_levels_forward` / `_backward`.  It is what
// INTEGRATION.md section 2 tells a maintainer of the reference to write: no kernel lives here -- every function
// checks its tensors like the reference does (CUDA + contiguous -> RuntimeError), allocates outputs and scratch with
// torch, and makes the two-phase C ABI call on torch's current HIP stream with the GIL released.  Built by
// __graft_entry__.build() as retinanet-examples_amd/odtk/_C_ext*.so (plain host C++, g++; links libodtk_hip.so);
// it is imported as odtk._C_ext next to the ctypes binding odtk/_C.py, which never hands work to it.
#include <torch/extension.h>
// PyTorch-ROCm keeps the device type named "cuda": the guard and stream accessors that honour that are the
// *MasqueradingAsCUDA forms (what hipify turns c10::cuda::CUDAGuard / getCurrentCUDAStream of the reference's
// extensions.cpp:62,99 into); the plain c10::hip:: forms reject a "cuda" device.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/odtk_hip.h"

namespace {

void require_gpu_contiguous(const torch::Tensor &t, const char *name) {       // extensions.cpp:42-44 CHECK_INPUT
  TORCH_CHECK(t.is_cuda(), name, " must be a CUDA tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be float32");
}

int checked(int rc, const char *what) {
  if (rc < 0) {
    std::string msg = std::string(what) + " failed: ";
    switch (rc) {
      case ODTK_ERR_INVALID: msg += "invalid argument"; break;
      case ODTK_ERR_WORKSPACE: msg += "Workspace is too small!"; break;        // the reference's message, utils.h:55-57
      case ODTK_ERR_UNSUPPORTED: msg += "unsupported dtype/layout"; break;
      default: msg += std::string("HIP error (") + odtk_last_hip_error() + ")";
    }
    throw std::runtime_error(msg);
  }
  return rc;
}

void *current_stream(const torch::Tensor &t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

// cub-style two-phase call (decode.cu:53-72): `call(workspace, size)` with (nullptr, 0) returns the bytes needed
template <typename Call>
void with_scratch(const torch::Tensor &like, const char *what, Call &&call) {
  const int size = checked(call(nullptr, 0), what);
  auto scratch = torch::empty({size > 0 ? size : 1}, like.options().dtype(torch::kUInt8));
  checked(call(scratch.data_ptr(), static_cast<size_t>(size)), what);
}

std::vector<torch::Tensor> decode(torch::Tensor cls_head, torch::Tensor box_head, std::vector<float> &anchors, int scale,
                                  float score_thresh, int top_n, bool rotated) {
  require_gpu_contiguous(cls_head, "cls_head");
  require_gpu_contiguous(box_head, "box_head");
  TORCH_CHECK(cls_head.dim() == 4 && box_head.dim() == 4 && !anchors.empty() && anchors.size() % 4 == 0, "decode: bad shapes");
  const int nb = rotated ? 6 : 4;
  const int64_t batch = cls_head.size(0), height = cls_head.size(2), width = cls_head.size(3);
  const size_t num_anchors = anchors.size() / 4, num_classes = cls_head.size(1) / num_anchors;
  TORCH_CHECK(box_head.size(0) == batch && box_head.size(1) == static_cast<int64_t>(num_anchors) * nb &&
              box_head.size(2) == height && box_head.size(3) == width, "box_head does not match cls_head");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(cls_head.device());
  auto opt = cls_head.options();
  auto scores = torch::empty({batch, top_n}, opt), boxes = torch::empty({batch, top_n, nb}, opt);
  auto classes = torch::empty({batch, top_n}, opt);
  const void *in[2] = {cls_head.data_ptr(), box_head.data_ptr()};
  void *out[3] = {scores.data_ptr(), boxes.data_ptr(), classes.data_ptr()};
  auto fn = rotated ? odtk_decode_rotate : odtk_decode;
  void *stream = current_stream(cls_head);
  {
    pybind11::gil_scoped_release nogil;
    with_scratch(cls_head, "decode", [&](void *ws, size_t size) {
      return fn(static_cast<int>(batch), ws ? in : nullptr, ws ? out : nullptr, height, width, scale, num_anchors, num_classes,
                anchors.data(), anchors.size(), score_thresh, top_n, ws, size, ws ? stream : nullptr);
    });
  }
  return {scores, boxes, classes};
}

std::vector<torch::Tensor> nms(torch::Tensor scores, torch::Tensor boxes, torch::Tensor classes, float nms_thresh,
                               int detections_per_im, bool rotated) {
  require_gpu_contiguous(scores, "scores");
  require_gpu_contiguous(boxes, "boxes");
  require_gpu_contiguous(classes, "classes");
  const int nb = rotated ? 6 : 4;
  TORCH_CHECK(scores.dim() == 2 && boxes.dim() == 3 && boxes.size(2) == nb && boxes.size(0) == scores.size(0) &&
              boxes.size(1) == scores.size(1) && classes.sizes() == scores.sizes(), "nms: inconsistent shapes");
  const int64_t batch = scores.size(0), count = scores.size(1);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(scores.device());
  auto opt = scores.options();
  auto out_scores = torch::empty({batch, detections_per_im}, opt), out_boxes = torch::empty({batch, detections_per_im, nb}, opt);
  auto out_classes = torch::empty({batch, detections_per_im}, opt);
  const void *in[3] = {scores.data_ptr(), boxes.data_ptr(), classes.data_ptr()};
  void *out[3] = {out_scores.data_ptr(), out_boxes.data_ptr(), out_classes.data_ptr()};
  auto fn = rotated ? odtk_nms_rotate : odtk_nms;
  void *stream = current_stream(scores);
  {
    pybind11::gil_scoped_release nogil;
    with_scratch(scores, "nms", [&](void *ws, size_t size) {
      return fn(static_cast<int>(batch), ws ? in : nullptr, ws ? out : nullptr, static_cast<size_t>(count), detections_per_im,
                nms_thresh, ws, size, ws ? stream : nullptr);
    });
  }
  return {out_scores, out_boxes, out_classes};
}

// Soft-NMS (odtk_soft_nms: no reference equivalent), the signature of odtk/_C.py:soft_nms
std::vector<torch::Tensor> soft_nms(torch::Tensor scores, torch::Tensor boxes, torch::Tensor classes, float nms_thresh,
                                    int detections_per_im, int method, float sigma, float min_score, bool return_indices) {
  require_gpu_contiguous(scores, "scores");
  require_gpu_contiguous(boxes, "boxes");
  require_gpu_contiguous(classes, "classes");
  TORCH_CHECK(scores.dim() == 2 && boxes.dim() == 3 && boxes.size(2) == 4 && boxes.size(0) == scores.size(0) &&
              boxes.size(1) == scores.size(1) && classes.sizes() == scores.sizes(), "soft_nms: inconsistent shapes");
  const int64_t batch = scores.size(0), count = scores.size(1);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(scores.device());
  auto opt = scores.options();
  std::vector<torch::Tensor> result = {torch::empty({batch, detections_per_im}, opt), torch::empty({batch, detections_per_im, 4}, opt),
                                       torch::empty({batch, detections_per_im}, opt)};
  if (return_indices) result.push_back(torch::empty({batch, detections_per_im}, opt.dtype(torch::kInt32)));
  const void *in[3] = {scores.data_ptr(), boxes.data_ptr(), classes.data_ptr()};
  void *out[4] = {result[0].data_ptr(), result[1].data_ptr(), result[2].data_ptr(), return_indices ? result[3].data_ptr() : nullptr};
  const int n_out = return_indices ? 4 : 3;
  void *stream = current_stream(scores);
  {
    pybind11::gil_scoped_release nogil;
    with_scratch(scores, "soft_nms", [&](void *ws, size_t size) {
      return odtk_soft_nms(static_cast<int>(batch), ws ? in : nullptr, ws ? out : nullptr, n_out, static_cast<size_t>(count),
                           detections_per_im, nms_thresh, method, sigma, min_score, 0u, ws, size, ws ? stream : nullptr);
    });
  }
  return result;
}

// Matrix NMS (odtk_matrix_nms: no reference equivalent), the signature of odtk/_C.py:matrix_nms
std::vector<torch::Tensor> matrix_nms(torch::Tensor scores, torch::Tensor boxes, torch::Tensor classes, int detections_per_im,
                                      int pre_top, int method, float sigma, float min_score, bool return_indices) {
  require_gpu_contiguous(scores, "scores");
  require_gpu_contiguous(boxes, "boxes");
  require_gpu_contiguous(classes, "classes");
  TORCH_CHECK(scores.dim() == 2 && boxes.dim() == 3 && boxes.size(2) == 4 && boxes.size(0) == scores.size(0) &&
              boxes.size(1) == scores.size(1) && classes.sizes() == scores.sizes(), "matrix_nms: inconsistent shapes");
  const int64_t batch = scores.size(0), count = scores.size(1);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(scores.device());
  auto opt = scores.options();
  std::vector<torch::Tensor> result = {torch::empty({batch, detections_per_im}, opt), torch::empty({batch, detections_per_im, 4}, opt),
                                       torch::empty({batch, detections_per_im}, opt)};
  if (return_indices) result.push_back(torch::empty({batch, detections_per_im}, opt.dtype(torch::kInt32)));
  const void *in[3] = {scores.data_ptr(), boxes.data_ptr(), classes.data_ptr()};
  void *out[4] = {result[0].data_ptr(), result[1].data_ptr(), result[2].data_ptr(), return_indices ? result[3].data_ptr() : nullptr};
  const int n_out = return_indices ? 4 : 3;
  void *stream = current_stream(scores);
  {
    pybind11::gil_scoped_release nogil;
    with_scratch(scores, "matrix_nms", [&](void *ws, size_t size) {
      return odtk_matrix_nms(static_cast<int>(batch), ws ? in : nullptr, ws ? out : nullptr, n_out, static_cast<size_t>(count),
                             detections_per_im, pre_top, method, sigma, min_score, 0u, ws, size, ws ? stream : nullptr);
    });
  }
  return result;
}

// box voting behind a suppression (odtk_box_vote: no reference equivalent), the signature of odtk/_C.py:box_vote
torch::Tensor box_vote(torch::Tensor scores, torch::Tensor boxes, torch::Tensor classes, torch::Tensor kept, float vote_thresh) {
  require_gpu_contiguous(scores, "scores");
  require_gpu_contiguous(boxes, "boxes");
  require_gpu_contiguous(classes, "classes");
  TORCH_CHECK(kept.is_cuda() && kept.is_contiguous() && kept.scalar_type() == torch::kInt32, "kept must be a contiguous int32 CUDA tensor");
  TORCH_CHECK(scores.dim() == 2 && boxes.dim() == 3 && boxes.size(2) == 4 && boxes.size(0) == scores.size(0) &&
              boxes.size(1) == scores.size(1) && classes.sizes() == scores.sizes() && kept.dim() == 2 && kept.size(0) == scores.size(0),
              "box_vote: inconsistent shapes");
  const int64_t batch = scores.size(0), count = scores.size(1), ndet = kept.size(1);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(scores.device());
  auto out = torch::empty({batch, ndet, 4}, scores.options());
  const void *in[3] = {scores.data_ptr(), boxes.data_ptr(), classes.data_ptr()};
  void *stream = current_stream(scores);
  {
    pybind11::gil_scoped_release nogil;
    checked(odtk_box_vote(static_cast<int>(batch), in, static_cast<const int32_t *>(kept.data_ptr()), out.data_ptr(),
                          static_cast<size_t>(count), static_cast<int>(ndet), vote_thresh, 0u, stream), "box_vote");
  }
  return out;
}

// candidate lists as one, mirrored passes un-mirrored (odtk_concat_candidates), the signature of odtk/_C.py:concat_candidates
std::vector<torch::Tensor> concat_candidates(std::vector<std::vector<torch::Tensor>> parts, std::vector<int> mirror_widths) {
  TORCH_CHECK(!parts.empty() && parts.size() == mirror_widths.size(), "concat_candidates: one mirror width per part");
  std::vector<odtk_candidates_t> table(parts.size());
  int64_t total = 0;
  const int64_t batch = parts[0].at(0).size(0);
  for (size_t i = 0; i < parts.size(); ++i) {
    TORCH_CHECK(parts[i].size() == 3, "concat_candidates: a part is (scores, boxes, classes)");
    const torch::Tensor &s = parts[i][0], &b = parts[i][1], &c = parts[i][2];
    require_gpu_contiguous(s, "scores");
    require_gpu_contiguous(b, "boxes");
    require_gpu_contiguous(c, "classes");
    TORCH_CHECK(s.dim() == 2 && s.size(0) == batch && b.dim() == 3 && b.size(0) == batch && b.size(1) == s.size(1) && b.size(2) == 4 &&
                c.sizes() == s.sizes() && s.device() == parts[0][0].device(), "concat_candidates: inconsistent shapes");
    table[i] = {static_cast<const float *>(s.data_ptr()), static_cast<const float *>(b.data_ptr()), static_cast<const float *>(c.data_ptr()),
                static_cast<uint32_t>(s.size(1)), mirror_widths[i]};
    total += s.size(1);
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(parts[0][0].device());
  auto opt = parts[0][0].options();
  std::vector<torch::Tensor> result = {torch::empty({batch, total}, opt), torch::empty({batch, total, 4}, opt), torch::empty({batch, total}, opt)};
  void *out[3] = {result[0].data_ptr(), result[1].data_ptr(), result[2].data_ptr()};
  void *stream = current_stream(parts[0][0]);
  {
    pybind11::gil_scoped_release nogil;
    checked(odtk_concat_candidates(static_cast<int>(batch), static_cast<int>(table.size()), table.data(), out, 0u, stream), "concat_candidates");
  }
  return result;
}

// the tile table of tiled inference: one (image, slot, y, x) per entry, the convention of odtk/_C.py
std::vector<odtk_tile_t> tile_table(const std::vector<std::vector<int>> &tiles, const char *what) {
  TORCH_CHECK(!tiles.empty() && tiles.size() <= ODTK_MAX_TILES, what, ": 1..", ODTK_MAX_TILES, " tiles per call");
  std::vector<odtk_tile_t> table(tiles.size());
  for (size_t i = 0; i < tiles.size(); ++i) {
    TORCH_CHECK(tiles[i].size() == 4, what, ": a tile is (image, slot, y, x)");
    table[i] = {tiles[i][0], tiles[i][1], tiles[i][3], tiles[i][2]};
  }
  return table;
}

// the tiler of tiled inference (odtk_tile_images), the signature of odtk/_C.py:tile_images
torch::Tensor tile_images(torch::Tensor x, std::vector<std::vector<int>> tiles, std::vector<int> size) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "x must be a 4-d CUDA tensor");
  TORCH_CHECK(size.size() == 2, "tile_images: size is (tile_h, tile_w)");
  const bool channels_last = !x.is_contiguous() && x.is_contiguous(at::MemoryFormat::ChannelsLast);
  TORCH_CHECK(x.is_contiguous() || channels_last, "x must be contiguous (NCHW or channels_last)");
  const auto st = x.scalar_type();
  TORCH_CHECK(st == torch::kFloat32 || st == torch::kBFloat16 || st == torch::kFloat16, "x must be float32, bfloat16 or float16");
  const int dtype = st == torch::kFloat32 ? ODTK_F32 : st == torch::kBFloat16 ? ODTK_BF16 : ODTK_F16;
  auto table = tile_table(tiles, "tile_images");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto out = torch::empty({static_cast<int64_t>(table.size()), x.size(1), size[0], size[1]},
                          x.options().memory_format(channels_last ? at::MemoryFormat::ChannelsLast : at::MemoryFormat::Contiguous));
  void *stream = current_stream(x);
  {
    pybind11::gil_scoped_release nogil;
    checked(odtk_tile_images(x.data_ptr(), out.data_ptr(), static_cast<int>(x.size(0)), static_cast<int>(x.size(1)),
                             static_cast<int>(x.size(2)), static_cast<int>(x.size(3)), dtype, channels_last ? 1 : 0,
                             static_cast<int>(table.size()), table.data(), size[0], size[1], stream), "tile_images");
  }
  return out;
}

// the merge of tiled inference (odtk_merge_tile_candidates), the signature of odtk/_C.py:merge_tile_candidates
std::vector<torch::Tensor> merge_tile_candidates(std::vector<torch::Tensor> parts, std::vector<std::vector<int>> tiles, int batch, int slots,
                                                 std::vector<int> size, std::vector<int> extent, float border,
                                                 std::optional<std::vector<torch::Tensor>> out) {
  TORCH_CHECK(parts.size() == 3 && size.size() == 2 && extent.size() == 2, "merge_tile_candidates: parts is (scores, boxes, classes), size and "
              "extent are (height, width)");
  require_gpu_contiguous(parts[0], "scores");
  require_gpu_contiguous(parts[1], "boxes");
  require_gpu_contiguous(parts[2], "classes");
  auto table = tile_table(tiles, "merge_tile_candidates");
  const int64_t n = static_cast<int64_t>(table.size());
  TORCH_CHECK(parts[0].dim() == 2 && parts[0].size(0) == n && parts[1].dim() == 3 && parts[1].size(0) == n &&
              parts[1].size(1) == parts[0].size(1) && parts[1].size(2) == 4 && parts[2].sizes() == parts[0].sizes() && batch > 0 && slots > 0,
              "merge_tile_candidates: inconsistent shapes");
  const int64_t count = parts[0].size(1), total = count * slots;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(parts[0].device());
  auto opt = parts[0].options();
  std::vector<torch::Tensor> result;
  if (out.has_value()) {
    result = *out;
    TORCH_CHECK(result.size() == 3, "merge_tile_candidates: out is (scores, boxes, classes)");
    for (const auto &t : result) require_gpu_contiguous(t, "out");
    TORCH_CHECK(result[0].dim() == 2 && result[0].size(0) == batch && result[0].size(1) == total && result[1].dim() == 3 &&
                result[1].size(0) == batch && result[1].size(1) == total && result[1].size(2) == 4 && result[2].sizes() == result[0].sizes() &&
                result[0].device() == parts[0].device(), "merge_tile_candidates: out does not match batch, slots and the parts");
  } else {
    result = {torch::zeros({batch, total}, opt), torch::zeros({batch, total, 4}, opt), torch::zeros({batch, total}, opt)};
  }
  const void *in[3] = {parts[0].data_ptr(), parts[1].data_ptr(), parts[2].data_ptr()};
  void *outp[3] = {result[0].data_ptr(), result[1].data_ptr(), result[2].data_ptr()};
  void *stream = current_stream(parts[0]);
  {
    pybind11::gil_scoped_release nogil;
    checked(odtk_merge_tile_candidates(static_cast<int>(n), table.data(), in, outp, static_cast<size_t>(count), batch, slots, size[0], size[1],
                                       extent[0], extent[1], border, 0u, stream), "merge_tile_candidates");
  }
  return result;
}

std::vector<torch::Tensor> iou(torch::Tensor boxes, torch::Tensor anchors) {
  require_gpu_contiguous(boxes, "boxes");
  require_gpu_contiguous(anchors, "anchors");
  const int num_boxes = static_cast<int>(boxes.numel() / 8), num_anchors = static_cast<int>(anchors.numel() / 8);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(boxes.device());
  auto out = torch::empty({num_anchors, num_boxes}, boxes.options());          // layout of extensions.cpp:64-66
  const void *in[2] = {boxes.data_ptr(), anchors.data_ptr()};
  void *outs[1] = {out.data_ptr()};
  void *stream = current_stream(boxes);
  {
    pybind11::gil_scoped_release nogil;
    checked(odtk_iou(in, outs, num_boxes, num_anchors, stream), "iou");
  }
  return {out};
}

// All pyramid levels + NMS in one enqueue (odtk_detect), for head tensors as the convolutions wrote them.
std::vector<torch::Tensor> detect(std::vector<torch::Tensor> cls_heads, std::vector<torch::Tensor> box_heads,
                                  std::vector<std::vector<float>> anchors, std::vector<int> strides, float score_thresh,
                                  int top_n, float nms_thresh, int detections_per_im, bool rotated, bool logits) {
  const size_t n = cls_heads.size();
  TORCH_CHECK(n >= 1 && n <= ODTK_MAX_LEVELS && box_heads.size() == n && anchors.size() == n && strides.size() == n,
              "detect: need 1..", ODTK_MAX_LEVELS, " levels with matching lists");
  const int nb = rotated ? 6 : 4;
  const auto dtype = cls_heads[0].scalar_type();
  const int dt = dtype == torch::kFloat32 ? ODTK_F32 : dtype == torch::kBFloat16 ? ODTK_BF16 : dtype == torch::kFloat16 ? ODTK_F16 : -1;
  TORCH_CHECK(dt >= 0, "detect: heads must be float32 / bfloat16 / float16");
  const int64_t batch = cls_heads[0].size(0);
  const int num_anchors = static_cast<int>(anchors[0].size() / 4);
  std::vector<odtk_level_t> levels(n);
  for (size_t i = 0; i < n; ++i) {
    const auto &c = cls_heads[i], &b = box_heads[i];
    TORCH_CHECK(c.is_cuda() && b.is_cuda() && c.dim() == 4 && b.dim() == 4 && c.scalar_type() == dtype && b.scalar_type() == dtype,
                "detect: level ", i, ": CUDA 4-d tensors of one dtype expected");
    // (a one-channel head or a 1 x 1 level is contiguous in BOTH readings and follows its partner: odtk/_C.py:_pair_layout)
    const bool c_nchw = c.is_contiguous(), c_nhwc = c.is_contiguous(at::MemoryFormat::ChannelsLast);
    const bool b_nchw = b.is_contiguous(), b_nhwc = b.is_contiguous(at::MemoryFormat::ChannelsLast);
    TORCH_CHECK(c_nchw || c_nhwc, "cls_head[", i, "] must be contiguous (NCHW or channels_last)");
    TORCH_CHECK((c_nchw && b_nchw) || (c_nhwc && b_nhwc), "box_head[", i, "] must share cls_head's memory format");
    const bool nchw = c_nchw && b_nchw;
    TORCH_CHECK(static_cast<int>(anchors[i].size()) == 4 * num_anchors && c.size(0) == batch && b.size(1) == num_anchors * nb, "detect: inconsistent level ", i);
    levels[i] = odtk_level_t{c.data_ptr(), b.data_ptr(), static_cast<int32_t>(c.size(2)), static_cast<int32_t>(c.size(3)), strides[i],
                             nchw ? 0 : 1, anchors[i].data(), nullptr, nullptr};
  }
  const int num_classes = static_cast<int>(cls_heads[0].size(1)) / num_anchors;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(cls_heads[0].device());
  auto opt = cls_heads[0].options().dtype(torch::kFloat32);
  auto scores = torch::empty({batch, detections_per_im}, opt), boxes = torch::empty({batch, detections_per_im, nb}, opt);
  auto classes = torch::empty({batch, detections_per_im}, opt);
  void *out[3] = {scores.data_ptr(), boxes.data_ptr(), classes.data_ptr()};
  const uint32_t flags = (rotated ? ODTK_FLAG_ROTATED : 0u) | (logits ? ODTK_FLAG_LOGITS : 0u);
  void *stream = current_stream(cls_heads[0]);
  {
    pybind11::gil_scoped_release nogil;
    with_scratch(cls_heads[0], "detect", [&](void *ws, size_t size) {
      return odtk_detect(static_cast<int>(batch), static_cast<int>(n), levels.data(), num_anchors, num_classes, dt, flags, score_thresh,
                         top_n, nms_thresh, detections_per_im, ws ? out : nullptr, ws, size, ws ? stream : nullptr);
    });
  }
  return {scores, boxes, classes};
}

// task-aligned target assignment (odtk_tal_assign_levels: no reference equivalent), the signature of odtk/_C.py:tal_assign_levels.
// The heads are taken as the convolutions wrote them: one dtype out of float32 / bfloat16 / float16, NCHW or channels_last.
std::vector<std::vector<std::optional<torch::Tensor>>> tal_assign_levels(torch::Tensor targets, std::vector<torch::Tensor> cls_heads,
                                                                         std::vector<torch::Tensor> box_heads,
                                                                         std::vector<std::vector<float>> anchors, int num_classes,
                                                                         std::vector<int> strides, int topk, int alpha, int beta,
                                                                         bool want_cls_target) {
  require_gpu_contiguous(targets, "targets");
  TORCH_CHECK(targets.dim() == 3 && targets.size(2) == 5, "targets must be [B, N, 5]");
  const size_t n = cls_heads.size();
  TORCH_CHECK(n >= 1 && n <= ODTK_MAX_LEVELS && box_heads.size() == n && anchors.size() == n && strides.size() == n,
              "tal_assign_levels: need 1..", ODTK_MAX_LEVELS, " levels with matching lists");
  const auto dtype = cls_heads[0].scalar_type();
  const int dt = dtype == torch::kFloat32 ? ODTK_F32 : dtype == torch::kBFloat16 ? ODTK_BF16 : dtype == torch::kFloat16 ? ODTK_F16 : -1;
  TORCH_CHECK(dt >= 0, "tal_assign_levels: heads must be float32 / bfloat16 / float16");
  const int64_t batch = targets.size(0);
  const int num_anchors = static_cast<int>(anchors[0].size() / 4);
  TORCH_CHECK(num_anchors >= 1 && num_classes >= 1, "tal_assign_levels: need anchors and classes");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(targets.device());
  auto opt = targets.options();
  std::vector<odtk_snap_level_t> levels(n);
  std::vector<odtk_loss_level_t> heads(n);
  std::vector<std::vector<std::optional<torch::Tensor>>> out(3);
  for (size_t i = 0; i < n; ++i) {
    const auto &c = cls_heads[i], &b = box_heads[i];
    TORCH_CHECK(c.is_cuda() && b.is_cuda() && c.dim() == 4 && b.dim() == 4 && c.scalar_type() == dtype && b.scalar_type() == dtype,
                "tal_assign_levels: level ", i, ": CUDA 4-d tensors of one dtype expected");
    const bool c_nchw = c.is_contiguous(), c_nhwc = c.is_contiguous(at::MemoryFormat::ChannelsLast);
    const bool b_nchw = b.is_contiguous(), b_nhwc = b.is_contiguous(at::MemoryFormat::ChannelsLast);
    TORCH_CHECK(c_nchw || c_nhwc, "cls_head[", i, "] must be contiguous (NCHW or channels_last)");
    TORCH_CHECK((c_nchw && b_nchw) || (c_nhwc && b_nhwc), "box_head[", i, "] must share cls_head's memory format");
    const int64_t h = c.size(2), w = c.size(3);
    TORCH_CHECK(static_cast<int>(anchors[i].size()) == 4 * num_anchors && c.size(0) == batch && b.size(0) == batch &&
                c.size(1) == static_cast<int64_t>(num_anchors) * num_classes && b.size(1) == static_cast<int64_t>(num_anchors) * 4 &&
                b.size(2) == h && b.size(3) == w, "tal_assign_levels: inconsistent level ", i);
    out[0].push_back(want_cls_target ? std::optional<torch::Tensor>(torch::empty({batch, num_anchors, num_classes, h, w}, opt)) : std::nullopt);
    out[1].push_back(torch::empty({batch, num_anchors, 4, h, w}, opt));
    out[2].push_back(torch::empty({batch, num_anchors, 1, h, w}, opt));
    levels[i] = odtk_snap_level_t{anchors[i].data(), want_cls_target ? static_cast<float *>(out[0][i]->data_ptr()) : nullptr,
                                  static_cast<float *>(out[1][i]->data_ptr()), static_cast<float *>(out[2][i]->data_ptr()),
                                  static_cast<int32_t>(h), static_cast<int32_t>(w), strides[i], 0};
    heads[i] = odtk_loss_level_t{c.data_ptr(), b.data_ptr(), nullptr, nullptr, nullptr, nullptr, static_cast<int32_t>(h),
                                 static_cast<int32_t>(w), (c_nchw && b_nchw) ? 0 : 1, 0};
  }
  void *stream = current_stream(targets);
  {
    pybind11::gil_scoped_release nogil;
    with_scratch(targets, "tal_assign_levels", [&](void *ws, size_t size) {
      return odtk_tal_assign_levels(static_cast<int>(batch), static_cast<const float *>(targets.data_ptr()), static_cast<int>(targets.size(1)),
                                    static_cast<int>(n), levels.data(), heads.data(), num_anchors, num_classes, dt, topk, alpha, beta, ws, size,
                                    ws ? stream : nullptr);
    });
  }
  return out;
}

// ProbIoU / KLD box losses of rotated boxes (odtk_rotated_box_loss_levels_*: no reference equivalent), the signatures of
// odtk/_C.py:rotated_box_loss_levels_forward / _backward.  The heads are taken as the convolutions wrote them.
struct RotatedLossLevels {
  std::vector<odtk_loss_level_t> levels;
  std::vector<const float *> tables;
  int batch = 0, num_anchors = 0, dtype = -1, kind = 0;
};

RotatedLossLevels rotated_loss_levels(const char *what, const std::vector<torch::Tensor> &box_heads, const std::vector<torch::Tensor> &depths,
                                      const std::vector<torch::Tensor> &box_targets, const std::vector<std::vector<float>> &anchors,
                                      const std::string &kind, const std::vector<torch::Tensor> *grads) {
  const size_t n = box_heads.size();
  TORCH_CHECK(n >= 1 && n <= ODTK_MAX_LEVELS && depths.size() == n && box_targets.size() == n && anchors.size() == n, what, ": need 1..",
              ODTK_MAX_LEVELS, " levels with matching lists");
  TORCH_CHECK(kind == "probiou" || kind == "kld", what, ": kind must be 'probiou' or 'kld', not '", kind, "'");
  RotatedLossLevels out;
  out.kind = kind == "probiou" ? ODTK_ROTATED_BOX_LOSS_PROBIOU : ODTK_ROTATED_BOX_LOSS_KLD;
  out.levels.resize(n);
  out.tables.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const auto &head = box_heads[i], &depth = depths[i], &target = box_targets[i];
    TORCH_CHECK(head.is_cuda() && depth.is_cuda() && target.is_cuda(), what, ": tensors must be on the GPU");
    TORCH_CHECK(head.dim() == 4 && depth.dim() == 5 && target.dim() == 5, what, ": box heads must be [B, A*6, H, W], depth [B, A, 1, H, W], "
                "box_target [B, A, 6, H, W]");
    const auto st = head.scalar_type();
    const int dt = st == torch::kFloat32 ? ODTK_F32 : st == torch::kBFloat16 ? ODTK_BF16 : st == torch::kFloat16 ? ODTK_F16 : -1;
    TORCH_CHECK(dt >= 0, what, ": box heads must be float32 / bfloat16 / float16");
    const bool nchw = head.is_contiguous(), nhwc = head.is_contiguous(at::MemoryFormat::ChannelsLast);
    TORCH_CHECK(nchw || nhwc, what, ": box heads must be dense NCHW or channels_last");
    const int64_t b = head.size(0), h = head.size(2), w = head.size(3), a = target.size(1);
    TORCH_CHECK(head.size(1) == 6 * a && depth.sizes() == torch::IntArrayRef({b, a, 1, h, w}) &&
                target.sizes() == torch::IntArrayRef({b, a, 6, h, w}), what, ": inconsistent shapes");
    TORCH_CHECK(depth.scalar_type() == torch::kFloat32 && target.scalar_type() == torch::kFloat32 && depth.is_contiguous() &&
                target.is_contiguous(), what, ": depth and box_target must be contiguous float32");
    if (i == 0) { out.batch = static_cast<int>(b); out.num_anchors = static_cast<int>(a); out.dtype = dt; }
    TORCH_CHECK(out.batch == b && out.num_anchors == a && out.dtype == dt, what, ": every level must share batch, anchors and dtype");
    TORCH_CHECK(static_cast<int64_t>(anchors[i].size()) == 4 * a, what, ": every level needs an [A, 4] anchor table");
    out.tables[i] = anchors[i].data();
    out.levels[i] = odtk_loss_level_t{nullptr, head.data_ptr(), static_cast<const float *>(depth.data_ptr()),
                                      static_cast<const float *>(target.data_ptr()), nullptr, grads ? (*grads)[i].data_ptr() : nullptr,
                                      static_cast<int32_t>(h), static_cast<int32_t>(w), nchw ? 0 : 1, 0};
  }
  return out;
}

torch::Tensor rotated_box_loss_levels_forward(std::vector<torch::Tensor> box_heads, std::vector<torch::Tensor> depths,
                                              std::vector<torch::Tensor> box_targets, std::vector<std::vector<float>> anchors,
                                              std::string kind) {
  const RotatedLossLevels lv = rotated_loss_levels("rotated_box_loss_levels_forward", box_heads, depths, box_targets, anchors, kind, nullptr);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(box_heads[0].device());
  auto sums = torch::empty({static_cast<int64_t>(lv.levels.size()), 2}, box_heads[0].options().dtype(torch::kFloat64));
  void *stream = current_stream(box_heads[0]);
  {
    pybind11::gil_scoped_release nogil;
    with_scratch(box_heads[0], "rotated_box_loss_levels_forward", [&](void *ws, size_t size) {
      return odtk_rotated_box_loss_levels_forward(static_cast<int>(lv.levels.size()), lv.levels.data(), lv.tables.data(), lv.batch,
                                                  lv.num_anchors, lv.dtype, lv.kind, static_cast<double *>(sums.data_ptr()), ws, size,
                                                  ws ? stream : nullptr);
    });
  }
  return sums;
}

std::vector<torch::Tensor> rotated_box_loss_levels_backward(std::vector<torch::Tensor> box_heads, std::vector<torch::Tensor> depths,
                                                            std::vector<torch::Tensor> box_targets, std::vector<std::vector<float>> anchors,
                                                            std::string kind, std::optional<torch::Tensor> grad_sums) {
  std::vector<torch::Tensor> dbox;
  for (const auto &head : box_heads) {
    dbox.push_back(torch::empty_like(head));
    TORCH_CHECK(dbox.back().strides() == head.strides(), "rotated_box_loss_levels_backward: could not allocate gradients in the heads' layout");
  }
  const RotatedLossLevels lv = rotated_loss_levels("rotated_box_loss_levels_backward", box_heads, depths, box_targets, anchors, kind, &dbox);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(box_heads[0].device());
  torch::Tensor g;
  if (grad_sums) {
    g = grad_sums->detach().to(box_heads[0].device(), torch::kFloat32).reshape({static_cast<int64_t>(lv.levels.size())}).contiguous();
  }
  void *stream = current_stream(box_heads[0]);
  {
    pybind11::gil_scoped_release nogil;
    checked(odtk_rotated_box_loss_levels_backward(static_cast<int>(lv.levels.size()), lv.levels.data(), lv.tables.data(), lv.batch,
                                                  lv.num_anchors, lv.dtype, lv.kind, grad_sums ? static_cast<const float *>(g.data_ptr()) : nullptr,
                                                  stream),
            "rotated_box_loss_levels_backward");
  }
  return dbox;
}

struct Engine {};   // csrc/engine.h: the TensorRT engine class -- not available on MI355X (BASELINE.json north_star)

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  namespace py = pybind11;
  m.doc() = "odtk._C on MI355X: decode / nms / iou of NVIDIA/retinanet-examples over libodtk_hip.so";
  // ABI guard: this module was compiled against ONE revision of include/odtk_hip.h; the library it found at load time must
  // have been compiled against the same struct layouts (a stale module would pass level arrays of the wrong stride)
  if (odtk_abi_struct_size(0) != static_cast<int>(sizeof(odtk_level_t)) ||
      odtk_abi_struct_size(1) != static_cast<int>(sizeof(odtk_snap_level_t)) ||
      odtk_abi_struct_size(2) != static_cast<int>(sizeof(odtk_snap_rot_level_t)) ||
      odtk_abi_struct_size(9) != static_cast<int>(sizeof(odtk_candidates_t)) ||
      odtk_abi_struct_size(11) != static_cast<int>(sizeof(odtk_tile_t)) ||
      odtk_abi_struct_size(17) != static_cast<int>(sizeof(odtk_optim_tensor_t)))
    throw py::import_error("odtk._C_ext was compiled against another revision of include/odtk_hip.h than libodtk_hip.so "
                           "(struct sizes differ): rebuild it -- make -C retinanet-examples_amd/csrc");
  py::class_<Engine>(m, "Engine")
      .def(py::init([](py::args, py::kwargs) -> Engine * {
        throw std::runtime_error("odtk._C.Engine: the TensorRT engine path is not available on MI355X");
      }))
      .def_static("load", [](const std::string &) -> Engine * {
        throw std::runtime_error("odtk._C.Engine.load: the TensorRT engine path is not available on MI355X");
      });
  m.def("decode", &decode, py::arg("cls_head"), py::arg("box_head"), py::arg("anchors"), py::arg("scale"), py::arg("score_thresh"),
        py::arg("top_n"), py::arg("rotated") = false);
  m.def("nms", &nms, py::arg("scores"), py::arg("boxes"), py::arg("classes"), py::arg("nms_thresh"), py::arg("detections_per_im"),
        py::arg("rotated") = false);
  m.def("soft_nms", &soft_nms, py::arg("scores"), py::arg("boxes"), py::arg("classes"), py::arg("nms_thresh"),
        py::arg("detections_per_im"), py::arg("method"), py::arg("sigma"), py::arg("min_score"), py::arg("return_indices") = false);
  m.def("matrix_nms", &matrix_nms, py::arg("scores"), py::arg("boxes"), py::arg("classes"), py::arg("ndetections"), py::arg("pre_top"),
        py::arg("method"), py::arg("sigma"), py::arg("min_score"), py::arg("return_indices") = false);
  m.def("box_vote", &box_vote, py::arg("scores"), py::arg("boxes"), py::arg("classes"), py::arg("kept"), py::arg("vote_thresh"));
  m.def("concat_candidates", &concat_candidates, py::arg("parts"), py::arg("mirror_widths"));
  m.def("tile_images", &tile_images, py::arg("x"), py::arg("tiles"), py::arg("size"));
  m.def("merge_tile_candidates", &merge_tile_candidates, py::arg("parts"), py::arg("tiles"), py::arg("batch"), py::arg("slots"), py::arg("size"),
        py::arg("extent"), py::arg("border"), py::arg("out") = py::none());
  m.def("iou", &iou, py::arg("boxes"), py::arg("anchors"));
  m.def("detect", &detect, py::arg("cls_heads"), py::arg("box_heads"), py::arg("anchors"), py::arg("strides"), py::arg("score_thresh"),
        py::arg("top_n"), py::arg("nms_thresh"), py::arg("detections_per_im"), py::arg("rotated") = false, py::arg("logits") = false);
  m.def("tal_assign_levels", &tal_assign_levels, py::arg("targets"), py::arg("cls_heads"), py::arg("box_heads"), py::arg("anchors_list"),
        py::arg("num_classes"), py::arg("strides"), py::arg("topk") = 13, py::arg("alpha") = 1, py::arg("beta") = 6,
        py::arg("want_cls_target") = true);
  m.def("rotated_box_loss_levels_forward", &rotated_box_loss_levels_forward, py::arg("box_heads"), py::arg("depths"), py::arg("box_targets"),
        py::arg("anchors_list"), py::arg("kind"));
  m.def("rotated_box_loss_levels_backward", &rotated_box_loss_levels_backward, py::arg("box_heads"), py::arg("depths"),
        py::arg("box_targets"), py::arg("anchors_list"), py::arg("kind"), py::arg("grad_sums") = py::none());
  m.def("version", [] { return std::string(odtk_version()); });
  // sizes of the ABI structs THIS module was compiled against: a module older than include/odtk_hip.h passes arrays of the
  // wrong stride (tests/test_compiled_binding.py compares them with the ctypes mirror on every CPU run)
  m.def("abi_sizes", [] {
    return py::dict(py::arg("level") = sizeof(odtk_level_t), py::arg("snap_level") = sizeof(odtk_snap_level_t),
                    py::arg("snap_rot_level") = sizeof(odtk_snap_rot_level_t), py::arg("optim_tensor") = sizeof(odtk_optim_tensor_t));
  });
}
