"""odtk._C -- the operator boundary of the reference (csrc/extensions.cpp:184-201), re-homed on
the MI355X C ABI (include/odtk_hip.h, libodtk_hip.so) through ctypes.

Exposes the reference's three free functions with the SAME positional signatures and return
conventions, so `from ._C import decode, nms, iou` in a box.py keeps working:

    decode(cls_head, box_head, anchors, scale, score_thresh, top_n, rotated=False) -> [scores, boxes, classes]
    nms(scores, boxes, classes, nms_thresh, detections_per_im, rotated=False)     -> [scores, boxes, classes]
    iou(boxes, anchors)                                                           -> [Tensor[num_anchors, num_boxes]]
    Engine                                                                        -> placeholder (TensorRT dropped)

plus the MI355X-first batched forms (`decode_levels`, `detect`) that cover all pyramid levels of
the whole batch in one enqueue, `soft_nms` (linear / Gaussian Soft-NMS), `matrix_nms` (linear / Gaussian Matrix NMS), `box_vote` (box voting behind a suppression) and
`concat_candidates` (the merge of flip test-time augmentation), `tile_images` and `merge_tile_candidates` (tiled inference of
large images): no reference equivalents.

There is NO CPU fallback: tensors must live on the GPU and the shared library must be present
(build it with `python __graft_entry__.py` or `make -C retinanet-examples_amd/csrc`); anything
else raises.  Work is only ENQUEUED on torch's current HIP stream -- no host synchronisation
(the reference blocks the host once per image per level, csrc/cuda/decode.cu:103).
"""
import ctypes
import threading
import os

import torch

_LIB_PATH = os.environ.get('ODTK_HIP_LIBRARY') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libodtk_hip.so')

OK, ERR_INVALID, ERR_WORKSPACE, ERR_HIP, ERR_UNSUPPORTED = 0, -1, -2, -3, -4
F32, BF16, F16 = 0, 1, 2
FLAG_ROTATED, FLAG_LOGITS, FLAG_ROTATED_NMS_FIXED_ANGLE = 1, 2, 4
MAX_LEVELS, MAX_ANCHORS, MAX_TOP_N, MAX_NMS_COUNT, MAX_NMS_COUNT_SCRATCH = 6, 32, 16384, 7680, 1 << 22
MAX_CONCAT_PARTS = 8
MAX_TILES = 64
MAX_OPTIM_TENSORS, OPTIM_CHUNK = 64, 4096   # = ODTK_MAX_OPTIM_TENSORS, ODTK_OPTIM_CHUNK of include/odtk_hip.h (tests/test_optim.py compares)
SOFT_NMS_LINEAR, SOFT_NMS_GAUSSIAN = 1, 2
MATRIX_NMS_LINEAR, MATRIX_NMS_GAUSSIAN = 1, 2
MAX_MATRIX_NMS_PRE = 4096
ATSS_MAX_TOPK = 16
BOX_LOSS_IOU, BOX_LOSS_GIOU, BOX_LOSS_DIOU = 1, 2, 3
BOX_LOSS_KINDS = {'iou': BOX_LOSS_IOU, 'giou': BOX_LOSS_GIOU, 'diou': BOX_LOSS_DIOU}
ROTATED_BOX_LOSS_PROBIOU, ROTATED_BOX_LOSS_KLD = 1, 2
ROTATED_BOX_LOSS_KINDS = {'probiou': ROTATED_BOX_LOSS_PROBIOU, 'kld': ROTATED_BOX_LOSS_KLD}
CLS_LOSS_QFL, CLS_LOSS_VFL = 1, 2
CLS_LOSS_KINDS = {'qfl': CLS_LOSS_QFL, 'vfl': CLS_LOSS_VFL}

_vp = ctypes.c_void_p
_vpp = ctypes.POINTER(ctypes.c_void_p)
_fp = ctypes.POINTER(ctypes.c_float)
_sz = ctypes.c_size_t


class LossLevel(ctypes.Structure):
    """odtk_loss_level_t"""
    _fields_ = [('cls', ctypes.c_void_p), ('box', ctypes.c_void_p), ('depth', ctypes.c_void_p), ('box_target', ctypes.c_void_p),
                ('dcls', ctypes.c_void_p), ('dbox', ctypes.c_void_p), ('height', ctypes.c_int32), ('width', ctypes.c_int32),
                ('channels_last', ctypes.c_int32), ('pad_', ctypes.c_int32)]


class SnapLevel(ctypes.Structure):
    """odtk_snap_level_t"""
    _fields_ = [('anchors', ctypes.POINTER(ctypes.c_float)), ('cls_target', ctypes.c_void_p), ('box_target', ctypes.c_void_p),
                ('depth', ctypes.c_void_p), ('height', ctypes.c_int32), ('width', ctypes.c_int32), ('stride', ctypes.c_int32),
                ('pad_', ctypes.c_int32)]


class SnapRotLevel(ctypes.Structure):
    """odtk_snap_rot_level_t"""
    _fields_ = [('anchors_axis', ctypes.c_void_p), ('anchors_quads', ctypes.c_void_p), ('cls_target', ctypes.c_void_p),
                ('box_target', ctypes.c_void_p), ('depth', ctypes.c_void_p), ('height', ctypes.c_int32), ('width', ctypes.c_int32),
                ('stride', ctypes.c_int32), ('pad_', ctypes.c_int32)]


class Level(ctypes.Structure):
    """odtk_level_t"""
    _fields_ = [('cls', _vp), ('box', _vp), ('height', ctypes.c_int32), ('width', ctypes.c_int32),
                ('stride', ctypes.c_int32), ('channels_last', ctypes.c_int32), ('anchors', _fp),
                ('cls_bias', _vp), ('box_bias', _vp), ('cls_thresholds', _vp)]


class Image(ctypes.Structure):
    """odtk_image_t"""
    _fields_ = [('src_offset', ctypes.c_uint64), ('src_width', ctypes.c_int32), ('src_height', ctypes.c_int32),
                ('src_pitch', ctypes.c_int32), ('out_width', ctypes.c_int32), ('out_height', ctypes.c_int32),
                ('mirror', ctypes.c_int32), ('x_table', ctypes.c_int32), ('y_table', ctypes.c_int32),
                ('x_taps', ctypes.c_int32), ('y_taps', ctypes.c_int32)]


class Augment(ctypes.Structure):
    """odtk_augment_t"""
    _fields_ = [('canvas_width', ctypes.c_int32), ('canvas_height', ctypes.c_int32), ('map', ctypes.c_int32 * 6),
                ('flags', ctypes.c_uint32), ('brightness', ctypes.c_float), ('contrast', ctypes.c_float),
                ('saturation', ctypes.c_float), ('hue', ctypes.c_uint8), ('pad_', ctypes.c_uint8 * 3)]


class Rotation(ctypes.Structure):
    """odtk_rotation_t"""
    _fields_ = [('matrix', ctypes.c_double * 6), ('enabled', ctypes.c_int32), ('flip', ctypes.c_int32)]


class MosaicTile(ctypes.Structure):
    """odtk_mosaic_tile_t"""
    _fields_ = [('source', ctypes.c_int32), ('dst_x', ctypes.c_int32), ('dst_y', ctypes.c_int32), ('width', ctypes.c_int32),
                ('height', ctypes.c_int32), ('src_x', ctypes.c_int32), ('src_y', ctypes.c_int32)]


class Mosaic(ctypes.Structure):
    """odtk_mosaic_t"""
    _fields_ = [('canvas_width', ctypes.c_int32), ('canvas_height', ctypes.c_int32), ('tiles', MosaicTile * 4),
                ('fill', ctypes.c_uint8 * 3), ('pad_', ctypes.c_uint8)]


class OptimTensor(ctypes.Structure):
    """odtk_optim_tensor_t"""
    _fields_ = [('param', _vp), ('grad', _vp), ('momentum', _vp), ('ema', _vp), ('numel', ctypes.c_int64)]


class Candidates(ctypes.Structure):
    """odtk_candidates_t"""
    _fields_ = [('scores', _vp), ('boxes', _vp), ('classes', _vp), ('count', ctypes.c_uint32), ('mirror_width', ctypes.c_int32)]


class Tile(ctypes.Structure):
    """odtk_tile_t"""
    _fields_ = [('image', ctypes.c_int32), ('slot', ctypes.c_int32), ('x', ctypes.c_int32), ('y', ctypes.c_int32)]


_SIGNATURES = {
    'odtk_version': (ctypes.c_char_p, []),
    'odtk_abi_struct_size': (ctypes.c_int, [ctypes.c_int]),
    'odtk_last_hip_error': (ctypes.c_char_p, []),
    'odtk_decode': (ctypes.c_int, [ctypes.c_int, _vpp, _vpp, _sz, _sz, _sz, _sz, _sz, _fp, _sz, ctypes.c_float,
                                   ctypes.c_int, _vp, _sz, _vp]),
    'odtk_decode_rotate': (ctypes.c_int, [ctypes.c_int, _vpp, _vpp, _sz, _sz, _sz, _sz, _sz, _fp, _sz,
                                          ctypes.c_float, ctypes.c_int, _vp, _sz, _vp]),
    'odtk_nms': (ctypes.c_int, [ctypes.c_int, _vpp, _vpp, _sz, ctypes.c_int, ctypes.c_float, _vp, _sz, _vp]),
    'odtk_nms_rotate': (ctypes.c_int, [ctypes.c_int, _vpp, _vpp, _sz, ctypes.c_int, ctypes.c_float, _vp, _sz, _vp]),
    'odtk_iou': (ctypes.c_int, [_vpp, _vpp, ctypes.c_int, ctypes.c_int, _vp]),
    'odtk_decode_levels': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Level), ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_float, ctypes.c_int,
                                          _vpp, ctypes.c_int, _vp, _sz, _vp]),
    'odtk_nms_ex': (ctypes.c_int, [ctypes.c_int, _vpp, _vpp, ctypes.c_int, _sz, ctypes.c_int, ctypes.c_float,
                                   ctypes.c_uint32, _vp, _sz, _vp]),
    'odtk_detect': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Level), ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_uint32, ctypes.c_float, ctypes.c_int, ctypes.c_float,
                                   ctypes.c_int, _vpp, _vp, _sz, _vp]),
    'odtk_snap_to_anchors': (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, _fp, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                            _vp, _vp, _vp, _vp]),
    'odtk_snap_to_anchors_levels': (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(SnapLevel),
                                                   ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, _vp]),
    'odtk_atss_assign_levels': (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(SnapLevel), ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, _vp, _sz, _vp]),
    'odtk_tal_assign_levels': (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(SnapLevel),
                                              ctypes.POINTER(LossLevel)] + [ctypes.c_int] * 6 + [_vp, _sz, _vp]),
    'odtk_retina_loss_forward': (ctypes.c_int, [_vp, _vp, _vp, _vp] + [ctypes.c_int] * 8 + [ctypes.c_float] * 3 + [_vp, _vp]),
    'odtk_retina_loss_backward': (ctypes.c_int, [_vp, _vp, _vp, _vp] + [ctypes.c_int] * 8 + [ctypes.c_float] * 3 +
                                  [_vp, _vp, _vp, _vp, _vp]),
    'odtk_retina_loss_levels_forward': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(LossLevel)] + [ctypes.c_int] * 5 +
                                        [ctypes.c_float] * 3 + [_vp, _vp]),
    'odtk_retina_loss_levels_forward_ws': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(LossLevel)] + [ctypes.c_int] * 5 +
                                           [ctypes.c_float] * 3 + [_vp, _vp, _sz, _vp]),
    'odtk_retina_loss_levels_backward': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(LossLevel)] + [ctypes.c_int] * 5 +
                                         [ctypes.c_float] * 3 + [_vp, _vp, _vp]),
    'odtk_box_iou_loss_levels_forward': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(LossLevel), ctypes.POINTER(_fp)] +
                                         [ctypes.c_int] * 4 + [_vp, _vp, _sz, _vp]),
    'odtk_box_iou_loss_levels_backward': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(LossLevel), ctypes.POINTER(_fp)] +
                                          [ctypes.c_int] * 4 + [_vp, _vp]),
    'odtk_rotated_box_loss_levels_forward': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(LossLevel), ctypes.POINTER(_fp)] +
                                             [ctypes.c_int] * 4 + [_vp, _vp, _sz, _vp]),
    'odtk_rotated_box_loss_levels_backward': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(LossLevel), ctypes.POINTER(_fp)] +
                                              [ctypes.c_int] * 4 + [_vp, _vp]),
    'odtk_quality_loss_levels_forward': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(LossLevel), ctypes.POINTER(_fp)] +
                                         [ctypes.c_int] * 5 + [ctypes.c_float] * 2 + [_vp, _vp, _sz, _vp]),
    'odtk_quality_loss_levels_backward': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(LossLevel), ctypes.POINTER(_fp)] +
                                          [ctypes.c_int] * 5 + [ctypes.c_float] * 2 + [_vp, _vp]),
    'odtk_optim_grad_norm': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(OptimTensor), _vp, ctypes.c_float, _vp, _vp, _sz, _vp]),
    'odtk_optim_grad_norm_chained': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(OptimTensor), _vp, ctypes.c_float, _vp, ctypes.c_int,
                                                    ctypes.c_int, _vp, _sz, _vp]),
    'odtk_optim_sgd_step': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(OptimTensor)] + [ctypes.c_float] * 3 + [ctypes.c_int, ctypes.c_float,
                                           _vp, _vp, _vp, _vp]),
    'odtk_bias_act': (ctypes.c_int, [_vp, _vp, _vp, _sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]),
    'odtk_profile_enable': (ctypes.c_int, [ctypes.c_int]),
    'odtk_debug_set_trace': (ctypes.c_int, [_vp]),
    'odtk_debug_loss_tuning': (ctypes.c_int, [ctypes.c_int] * 6),
    'odtk_debug_loss_layout': (ctypes.c_int, [ctypes.c_int] * 5),
    'odtk_debug_loss_form': (ctypes.c_int, [ctypes.c_int]),
    'odtk_debug_loss_tuning_get': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    'odtk_debug_loss_form_get': (ctypes.c_int, []),
    'odtk_bias_act_maxpool': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'odtk_snap_to_anchors_rotated_levels': (ctypes.c_int, [ctypes.c_int, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int,
                                                           ctypes.POINTER(SnapRotLevel), ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                           ctypes.c_float, _vp]),
    'odtk_prefilter_thresholds': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, _vp, _vp]),
    'odtk_upsample_nearest2x': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_void_p]),
    'odtk_canvas_clear': (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_void_p]),
    'odtk_canvas_pack': (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int), _vpp, ctypes.c_int,
                                        ctypes.c_void_p]),
    'odtk_stem_pack': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'odtk_debug_stream_tuning': (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    'odtk_debug_stream_tuning_get': (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    'odtk_debug_bias_act_grid': (ctypes.c_int, [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint)]),
    'odtk_preprocess_images': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(Image), _vp, _sz, _vp, _sz, _vp, _vp, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, _vp]),
    'odtk_augment_images': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(Image), ctypes.POINTER(Augment), _vp, _sz, _vp, _sz, _vp, _vp,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _sz, _vp]),
    'odtk_augment_images_ex': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(Image), ctypes.POINTER(Augment), ctypes.POINTER(Rotation), _vp, _sz,
                                              _vp, _sz, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _sz, _vp]),
    'odtk_mosaic_images': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(Mosaic), ctypes.POINTER(Augment), ctypes.c_int, ctypes.POINTER(Image),
                                          ctypes.c_int, _vp, _sz, _vp, _sz, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _sz, _vp]),
    'odtk_nms_sorted_runs': (ctypes.c_int, [ctypes.c_int, _vpp, _vpp, ctypes.c_int, _sz, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_float,
                                            ctypes.c_uint32, _vp, _sz, _vp]),
    'odtk_soft_nms': (ctypes.c_int, [ctypes.c_int, _vpp, _vpp, ctypes.c_int, _sz, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                     ctypes.c_float, ctypes.c_float, ctypes.c_uint32, _vp, _sz, _vp]),
    'odtk_matrix_nms': (ctypes.c_int, [ctypes.c_int, _vpp, _vpp, ctypes.c_int, _sz, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_float, ctypes.c_float, ctypes.c_uint32, _vp, _sz, _vp]),
    'odtk_box_vote': (ctypes.c_int, [ctypes.c_int, _vpp, _vp, _vp, _sz, ctypes.c_int, ctypes.c_float, ctypes.c_uint32, _vp]),
    'odtk_concat_candidates': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Candidates), _vpp, ctypes.c_uint32, _vp]),
    'odtk_tile_images': (ctypes.c_int, [_vp, _vp] + [ctypes.c_int] * 7 + [ctypes.POINTER(Tile), ctypes.c_int, ctypes.c_int, _vp]),
    'odtk_merge_tile_candidates': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(Tile), _vpp, _vpp, _sz] + [ctypes.c_int] * 6 +
                                   [ctypes.c_float, ctypes.c_uint32, _vp]),
    'odtk_gemm_init': (ctypes.c_int, [ctypes.c_char_p]),
    'odtk_gemm_plan_export': (ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]),
    'odtk_gemm_plan_import': (ctypes.c_int, [ctypes.c_char_p]),
    'odtk_gemm_plan_pin_misses': (ctypes.c_int, []),
    'odtk_debug_gemm_candidates': (ctypes.c_int, [ctypes.c_size_t] + [ctypes.c_int] * 5 + [ctypes.c_size_t, ctypes.POINTER(ctypes.c_int),
                                                  ctypes.c_int]),
    'odtk_gemm_plan_clear': (None, []),
    'odtk_gemm_last_solution': (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    'odtk_gemm_bias_act': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'odtk_bottleneck_seam': (ctypes.c_int, [ctypes.c_void_p] * 8 + [ctypes.c_size_t] + [ctypes.c_int] * 4 + [ctypes.c_void_p]),
    'odtk_tower_conv3x3': (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int] * 7 + [ctypes.c_void_p]),
    'odtk_debug_tower_conv_variant': (ctypes.c_int, [ctypes.c_int]),
    'odtk_profile_collect': (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]),
}

KERNEL_NAMES = ('prefilter_scan_kernel', 'select_decode_kernel', 'nms_kernel', 'iou_pairs_kernel', 'bias_act_kernel',
                'snap_to_anchors_kernel', 'gemm_bias_act', 'retina_loss_kernel', 'select_hist_kernel', 'select_filter_kernel',
                'nms_first_round_kernel', 'rotated_sup_matrix_kernel', 'bias_act_maxpool_kernel', 'upsample_nearest2x_kernel',
                'stem_pack_kernel', 'loss_reduce_kernel', 'atss_stats_kernel', 'bottleneck_seam_kernel', 'tower_conv3x3_kernel')
# HBM bytes the epilogue entry points move, per kernel name, while `traffic_count` is on (bench.py's epilogue_roofline: the
# algorithmic bytes of every call -- each element read once and written once, + the skip input -- divided by the kernel time)
traffic_count = False
traffic_bytes = {}


def _count(name, nbytes):
    if traffic_count:
        traffic_bytes[name] = traffic_bytes.get(name, 0) + int(nbytes)


_lib = None


def library():
    """The loaded libodtk_hip.so (raises -- loudly -- if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.isfile(_LIB_PATH):
            raise ImportError('odtk._C: %s is missing -- build the HIP library first '
                              '(python __graft_entry__.py, or make -C retinanet-examples_amd/csrc). '
                              'There is no CPU fallback.' % _LIB_PATH)
        lib = ctypes.CDLL(_LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        # ABI guard: the ctypes mirrors below must have the layout the library was compiled with (include/odtk_hip.h)
        for which, mirror in ((0, Level), (1, SnapLevel), (2, SnapRotLevel), (3, LossLevel), (5, Image), (6, Augment), (7, Rotation),
                              (9, Candidates), (11, Tile), (14, MosaicTile), (15, Mosaic), (17, OptimTensor)):
            if lib.odtk_abi_struct_size(which) != ctypes.sizeof(mirror):
                raise ImportError('odtk._C: %s was built from another revision of include/odtk_hip.h (sizeof struct %d: library %d, '
                                  'binding %d) -- rebuild it (make -C retinanet-examples_amd/csrc)'
                                  % (_LIB_PATH, which, lib.odtk_abi_struct_size(which), ctypes.sizeof(mirror)))
        _lib = lib
        # Debug knob (tools/loss_probe.py): ODTK_LOSS_TUNING="fwd32:threads,blocks_per_cu,unroll,box_blocks;bwd16:...;ws32:..."
        # (fwd = forward with atomics, bwd, ws = forward through a workspace) overrides the built-in launch shapes
        for part in filter(None, os.environ.get('ODTK_LOSS_TUNING', '').split(';')):
            side, _, vals = part.partition(':')
            side = side.strip()
            _check(lib.odtk_debug_loss_tuning({'fwd': 0, 'bwd': 1, 'ws': 2}[side[:-2]], int(side.endswith('32')),
                                              *(int(v) for v in vals.split(','))), 'ODTK_LOSS_TUNING')
        # ODTK_LOSS_FORM=0|1: arithmetic form of the gamma = 2 classification walk (include/odtk_hip.h: odtk_debug_loss_form).
        # Said out loud: a process-wide numerical switch must not be silent.  (The ablation forms 2..7 -- wrong sums on purpose --
        # exist only in a -DODTK_LOSS_ABLATIONS build; the shipped library refuses them here.)
        if os.environ.get('ODTK_LOSS_FORM', '') != '':
            import warnings
            warnings.warn('odtk._C: ODTK_LOSS_FORM=%s overrides the loss kernels\' arithmetic form for this process' % os.environ['ODTK_LOSS_FORM'])
            _check(lib.odtk_debug_loss_form(int(os.environ['ODTK_LOSS_FORM'])), 'ODTK_LOSS_FORM')
    return _lib


def exported_symbols():
    return [n for n in _SIGNATURES]


_ERR = {ERR_INVALID: 'invalid argument', ERR_WORKSPACE: 'Workspace is too small!',
        ERR_HIP: 'HIP error', ERR_UNSUPPORTED: 'unsupported dtype/layout'}


def _check(rc, what):
    if rc < 0:
        detail = library().odtk_last_hip_error().decode() if rc == ERR_HIP else ''
        raise RuntimeError('%s failed: %s%s' % (what, _ERR.get(rc, 'error %d' % rc), (' (%s)' % detail) if detail else ''))
    return rc


def _check_input(t, name):
    # csrc/extensions.cpp:42-44  CHECK_CUDA / CHECK_CONTIGUOUS -> RuntimeError
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('%s must be a CUDA tensor' % name)
    if not t.is_contiguous():
        raise RuntimeError('%s must be contiguous' % name)
    if t.dtype != torch.float32:
        raise RuntimeError('%s must be float32' % name)


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


_workspaces = {}
_workspaces_lock = threading.Lock()      # several host threads may enqueue on their own streams at once (include/odtk_hip.h)


def _workspace(device, nbytes, cache=_workspaces):
    """Scratch owned by the binding, cached per (device, stream): never shared between streams.
    While the stream is being captured into a hipGraph nothing is cached and nothing cached is used: the buffer of a
    captured call is allocated for that call and belongs to the graph (torch serves allocations made during a capture
    from the graph's private pool and keeps that pool alive exactly as long as the graph), so a graph never reads
    scratch that an eager call -- or another graph -- may grow, replace or overwrite, and the cache never holds
    memory of a graph that no longer exists.  -> (buffer, stream handle)"""
    stream = torch.cuda.current_stream(device)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device), stream.cuda_stream
    key = (device.index, stream.cuda_stream)
    with _workspaces_lock:
        ws = cache.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
            cache[key] = ws
    return ws, stream.cuda_stream


def _enqueue(fn, what, device, *args):
    """The two-phase call of the ABI on torch's current HIP stream of `device`: fn(*args, workspace, size, stream) with a null
    workspace answers the size it needs (every entry point does so before it looks at a data pointer: tests/test_abi_host.py),
    then the same call with the binding's scratch enqueues the work."""
    with torch.cuda.device(device):
        size = _check(fn(*args, None, 0, None), what + ' (workspace query)')
        ws, stream = _workspace(device, size)
        _check(fn(*args, ws.data_ptr(), ws.numel(), stream), what)


def _launch(fn, what, device, *args):
    """An ABI call that takes no workspace: fn(*args, stream) on torch's current HIP stream of `device`."""
    with torch.cuda.device(device):
        _check(fn(*args, torch.cuda.current_stream(device).cuda_stream), what)


def _detections(batch, n, nb, device, return_indices=False):
    """The outputs of a decode / nms call: [scores [B, n], boxes [B, n, nb], classes [B, n]] (+ int32 indices [B, n])."""
    out = [torch.empty((batch, n), dtype=torch.float32, device=device),
           torch.empty((batch, n, nb), dtype=torch.float32, device=device),
           torch.empty((batch, n), dtype=torch.float32, device=device)]
    if return_indices:
        out.append(torch.empty((batch, n), dtype=torch.int32, device=device))
    return out


def _anchor_array(anchors):
    flat = [float(v) for v in anchors]
    return (ctypes.c_float * len(flat))(*flat), len(flat)


def decode(cls_head, box_head, anchors, scale, score_thresh, top_n, rotated=False):
    """csrc/extensions.cpp:69-115.  `anchors` is the flat python list the reference passes
    (anchors.view(-1).tolist(), odtk/box.py:263-264)."""
    _check_input(cls_head, 'cls_head')
    _check_input(box_head, 'box_head')
    lib = library()
    nb = 6 if rotated else 4
    batch, channels, height, width = cls_head.shape
    arr, n = _anchor_array(anchors)
    num_anchors = n // 4
    if num_anchors == 0 or n % 4 or channels % num_anchors:
        raise RuntimeError('decode: %d anchor values do not describe the %d channels of cls_head' % (n, channels))
    num_classes = channels // num_anchors
    if box_head.shape != (batch, num_anchors * nb, height, width):
        raise RuntimeError('box_head shape %s does not match cls_head %s' % (tuple(box_head.shape), tuple(cls_head.shape)))
    out = _detections(batch, top_n, nb, cls_head.device)
    _enqueue(lib.odtk_decode_rotate if rotated else lib.odtk_decode, 'decode', cls_head.device, batch,
             _ptrs([cls_head, box_head]), _ptrs(out), height, width, int(scale), num_anchors, num_classes, arr, n,
             float(score_thresh), int(top_n))
    return out


def nms(scores, boxes, classes, nms_thresh, detections_per_im, rotated=False, return_indices=False):
    """csrc/extensions.cpp:117-158."""
    _check_input(scores, 'scores')
    _check_input(boxes, 'boxes')
    _check_input(classes, 'classes')
    lib = library()
    nb = 6 if rotated else 4
    batch, count = scores.shape
    if boxes.shape != (batch, count, nb) or classes.shape != (batch, count):
        raise RuntimeError('nms: inconsistent shapes')
    out = _detections(batch, detections_per_im, nb, scores.device, return_indices)
    _enqueue(lib.odtk_nms_ex, 'nms', scores.device, batch, _ptrs([scores, boxes, classes]), _ptrs(out), len(out), count,
             int(detections_per_im), float(nms_thresh), FLAG_ROTATED if rotated else 0)
    return out


def soft_nms(scores, boxes, classes, nms_thresh, detections_per_im, method, sigma, min_score, return_indices=False):
    """Class-aware Soft-NMS on axis-aligned boxes (include/odtk_hip.h: odtk_soft_nms; no reference equivalent): one launch.
    method: SOFT_NMS_LINEAR / SOFT_NMS_GAUSSIAN; emitted scores are the decayed ones."""
    _check_input(scores, 'scores')
    _check_input(boxes, 'boxes')
    _check_input(classes, 'classes')
    lib = library()
    batch, count = scores.shape
    if boxes.shape != (batch, count, 4) or classes.shape != (batch, count):
        raise RuntimeError('soft_nms: inconsistent shapes')
    out = _detections(batch, detections_per_im, 4, scores.device, return_indices)
    _enqueue(lib.odtk_soft_nms, 'soft_nms', scores.device, batch, _ptrs([scores, boxes, classes]), _ptrs(out), len(out), count,
             int(detections_per_im), float(nms_thresh), int(method), float(sigma), float(min_score), 0)
    return out


def matrix_nms(scores, boxes, classes, ndetections, pre_top, method, sigma, min_score, return_indices=False):
    """Class-aware Matrix NMS on axis-aligned boxes (include/odtk_hip.h: odtk_matrix_nms; no reference equivalent): four launches,
    any list length.  method: MATRIX_NMS_LINEAR / MATRIX_NMS_GAUSSIAN; emitted scores are the decayed ones."""
    _check_input(scores, 'scores')
    _check_input(boxes, 'boxes')
    _check_input(classes, 'classes')
    lib = library()
    batch, count = scores.shape
    if boxes.shape != (batch, count, 4) or classes.shape != (batch, count):
        raise RuntimeError('matrix_nms: inconsistent shapes')
    out = _detections(batch, ndetections, 4, scores.device, return_indices)
    _enqueue(lib.odtk_matrix_nms, 'matrix_nms', scores.device, batch, _ptrs([scores, boxes, classes]), _ptrs(out), len(out), count,
             int(ndetections), int(pre_top), int(method), float(sigma), float(min_score), 0)
    return out


def box_vote(scores, boxes, classes, kept, vote_thresh):
    """Box voting (include/odtk_hip.h: odtk_box_vote; no reference equivalent): one launch.  scores / boxes / classes are the
    suppression's INPUT list, kept [B, D] int32 its position output (`nms(.., return_indices=True)[3]`) -> boxes [B, D, 4]."""
    _check_input(scores, 'scores')
    _check_input(boxes, 'boxes')
    _check_input(classes, 'classes')
    if not isinstance(kept, torch.Tensor) or not kept.is_cuda or not kept.is_contiguous() or kept.dtype != torch.int32:
        raise RuntimeError('kept must be a contiguous int32 CUDA tensor')
    lib = library()
    batch, count = scores.shape
    if boxes.shape != (batch, count, 4) or classes.shape != (batch, count) or kept.dim() != 2 or kept.shape[0] != batch:
        raise RuntimeError('box_vote: inconsistent shapes')
    out = torch.empty((batch, kept.shape[1], 4), dtype=torch.float32, device=scores.device)
    _launch(lib.odtk_box_vote, 'box_vote', scores.device, batch, _ptrs([scores, boxes, classes]), kept.data_ptr(), out.data_ptr(),
            count, int(kept.shape[1]), float(vote_thresh), 0)
    return out


def concat_candidates(parts, mirror_widths):
    """Candidate lists as one along the candidate axis, the boxes of mirrored passes mapped back (include/odtk_hip.h:
    odtk_concat_candidates): one launch.  parts: up to 8 (scores [B, n_i], boxes [B, n_i, 4], classes [B, n_i]); mirror_widths:
    per part 0, or the width of the tensor whose horizontal flip the part was decoded from."""
    lib = library()
    if not parts or len(parts) != len(mirror_widths):
        raise RuntimeError('concat_candidates: one mirror width per part')
    table = (Candidates * len(parts))()
    batch, dev, total = parts[0][0].shape[0], parts[0][0].device, 0
    for entry, (s, b, c), width in zip(table, parts, mirror_widths):
        _check_input(s, 'scores')
        _check_input(b, 'boxes')
        _check_input(c, 'classes')
        if s.dim() != 2 or s.shape[0] != batch or b.shape != (batch, s.shape[1], 4) or c.shape != s.shape or s.device != dev:
            raise RuntimeError('concat_candidates: inconsistent shapes')
        entry.scores, entry.boxes, entry.classes = s.data_ptr(), b.data_ptr(), c.data_ptr()
        entry.count, entry.mirror_width = s.shape[1], int(width)
        total += s.shape[1]
    out = _detections(batch, total, 4, dev)
    _launch(lib.odtk_concat_candidates, 'concat_candidates', dev, batch, len(parts), table, _ptrs(out), 0)
    return out


def _tile_table(tiles, what):
    """The odtk_tile_t array of a list of (image, slot, y, x)."""
    if not 1 <= len(tiles) <= MAX_TILES:
        raise RuntimeError('%s: 1..%d tiles per call, not %d' % (what, MAX_TILES, len(tiles)))
    table = (Tile * len(tiles))()
    for entry, (image, slot, y, x) in zip(table, tiles):
        entry.image, entry.slot, entry.x, entry.y = int(image), int(slot), int(x), int(y)
    return table


_TILE_DTYPES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


def tile_images(x, tiles, size):
    """The tiler of tiled inference (include/odtk_hip.h: odtk_tile_images): one launch.  x [B, C, H, W], float32 / bfloat16 /
    float16, NCHW- or channels_last-contiguous; tiles: up to 64 (image, slot, y, x), image < 0 = an all-zero tile; size (th, tw)
    -> [len(tiles), C, th, tw] in x's dtype and memory format, zeros behind the image."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4:
        raise RuntimeError('x must be a 4-d CUDA tensor')
    channels_last = not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)
    if not (x.is_contiguous() or channels_last):
        raise RuntimeError('x must be contiguous (NCHW or channels_last)')
    if x.dtype not in _TILE_DTYPES:
        raise RuntimeError('x must be float32, bfloat16 or float16')
    lib = library()
    table = _tile_table(tiles, 'tile_images')
    th, tw = (int(v) for v in size)
    batch, channels, height, width = x.shape
    out = torch.empty((len(table), channels, th, tw), dtype=x.dtype, device=x.device,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    _launch(lib.odtk_tile_images, 'tile_images', x.device, x.data_ptr(), out.data_ptr(), batch, channels, height, width,
            _TILE_DTYPES[x.dtype], int(channels_last), len(table), table, th, tw)
    return out


def merge_tile_candidates(parts, tiles, batch, slots, size, extent, border, out=None):
    """The merge of tiled inference (include/odtk_hip.h: odtk_merge_tile_candidates): one launch.  parts: (scores [n, count], boxes
    [n, count, 4], classes [n, count]) of the n tiles; tiles: their (image, slot, y, x); size (th, tw); extent (H, W) of the images
    -> [scores [batch, slots * count], boxes [.., 4], classes]: `out` when given (entry i writes its `count` positions of row
    `image` and nothing else), otherwise new lists whose other positions are empty slots."""
    lib = library()
    scores, boxes, classes = parts
    _check_input(scores, 'scores')
    _check_input(boxes, 'boxes')
    _check_input(classes, 'classes')
    table = _tile_table(tiles, 'merge_tile_candidates')
    batch, slots = int(batch), int(slots)
    if scores.dim() != 2 or scores.shape[0] != len(table) or boxes.shape != (len(table), scores.shape[1], 4) or classes.shape != scores.shape \
            or batch < 1 or slots < 1:
        raise RuntimeError('merge_tile_candidates: inconsistent shapes')
    count = scores.shape[1]
    total = slots * count
    if out is None:
        out = [torch.zeros(shape, dtype=torch.float32, device=scores.device) for shape in ((batch, total), (batch, total, 4), (batch, total))]
    else:
        out = list(out)
        for t in out:
            _check_input(t, 'out')
        if len(out) != 3 or out[0].shape != (batch, total) or out[1].shape != (batch, total, 4) or out[2].shape != (batch, total) \
                or out[0].device != scores.device:
            raise RuntimeError('merge_tile_candidates: out does not match batch, slots and the parts')
    _launch(lib.odtk_merge_tile_candidates, 'merge_tile_candidates', scores.device, len(table), table, _ptrs([scores, boxes, classes]),
            _ptrs(out), count, batch, slots, int(size[0]), int(size[1]), int(extent[0]), int(extent[1]), float(border), 0)
    return out


def nms_sorted_runs(scores, boxes, classes, run_len, nms_thresh, detections_per_im, rotated=False):
    """`nms` for candidates that are n_runs = count / run_len runs, each already in NMS order with its non-positive scores at
    the end -- the concatenation of per-level `decode` outputs (include/odtk_hip.h: odtk_nms_sorted_runs).  Same result as
    `nms`, without its compaction / selection / sort rounds."""
    _check_input(scores, 'scores')
    _check_input(boxes, 'boxes')
    _check_input(classes, 'classes')
    lib = library()
    nb = 6 if rotated else 4
    batch, count = scores.shape
    if boxes.shape != (batch, count, nb) or classes.shape != (batch, count) or count % int(run_len):
        raise RuntimeError('nms_sorted_runs: inconsistent shapes')
    run_valid = (scores.view(batch, count // int(run_len), int(run_len)) > 0).sum(2).to(torch.int32).contiguous()
    out = _detections(batch, detections_per_im, nb, scores.device)
    _enqueue(lib.odtk_nms_sorted_runs, 'nms_sorted_runs', scores.device, batch, _ptrs([scores, boxes, classes]), _ptrs(out), 3,
             count, int(run_len), run_valid.data_ptr(), int(detections_per_im), float(nms_thresh), FLAG_ROTATED if rotated else 0)
    return out


def iou(boxes, anchors):
    """csrc/extensions.cpp:47-67: flat [N*8] box corners, flat [M*8] anchor corners -> [Tensor[M, N]]."""
    _check_input(boxes, 'boxes')
    _check_input(anchors, 'anchors')
    lib = library()
    num_boxes = boxes.numel() // 8
    num_anchors = anchors.numel() // 8
    out = torch.empty((num_anchors, num_boxes), dtype=torch.float32, device=boxes.device)
    _launch(lib.odtk_iou, 'iou', boxes.device, _ptrs([boxes, anchors]), _ptrs([out]), num_boxes, num_anchors)
    return [out]


_DTYPES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


def _pair_layout(c, b, cname, bname, what, prefer_channels_last=False):
    """Common memory format of a (cls_head, box_head) pair: 0 NCHW, 1 channels_last.  A tensor with ONE channel (a one-anchor,
    one-class head) or ONE pixel (a 1 x 1 level) is contiguous in both readings -- torch says so for either format -- and follows
    its partner instead of being pinned to NCHW (found by tools/decode_fuzz_long.py: A = C = 1 with channels_last heads was
    refused as 'mixed formats').  prefer_channels_last: take that reading when both tensors allow both (the bias fold wants it)."""
    def readings(t, name):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError('%s must be a CUDA tensor' % name)
        if t.dim() != 4:
            raise RuntimeError('%s must be 4-d [B, C, H, W]' % name)
        n, l = t.is_contiguous(), t.is_contiguous(memory_format=torch.channels_last)
        if not (n or l):
            raise RuntimeError('%s must be contiguous (NCHW or channels_last)' % name)
        return n, l
    cn, cl = readings(c, cname)
    bn, bl = readings(b, bname)
    if prefer_channels_last and cl and bl:
        return 1
    if cn and bn:
        return 0
    if cl and bl:
        return 1
    raise RuntimeError('%s%s and %s must share one memory format' % (what, cname, bname))


def prefilter_thresholds(cls_bias, dtype, score_thresh):
    """The prefilter's per-channel threshold table for `cls_bias` (float32 CUDA vector [A*C], A*C % 8 == 0), a 16-bit head
    dtype and a score threshold: made ONCE (an engine: when it folds its weights) and handed to decode_levels / detect as
    `cls_thresholds`, so that the ~3750 workgroups of the prefilter load 2880 ready bytes instead of deriving them from the
    bias before their first load.  A table made for other parameters is detected and not used."""
    if not cls_bias.is_cuda or cls_bias.dtype != torch.float32 or not cls_bias.is_contiguous() or cls_bias.numel() % 8:
        raise RuntimeError('prefilter_thresholds: cls_bias must be a contiguous float32 CUDA vector whose length is a multiple of 8')
    if dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError('prefilter_thresholds: 16-bit head dtypes only')
    table = torch.empty(cls_bias.numel() + 8, dtype=torch.float32, device=cls_bias.device)
    _launch(library().odtk_prefilter_thresholds, 'prefilter_thresholds', cls_bias.device, cls_bias.data_ptr(), cls_bias.numel(),
            _DTYPES[dtype], float(score_thresh), table.data_ptr())
    return table


def _levels(cls_heads, box_heads, anchors_list, strides, nb, cls_bias=None, box_bias=None, cls_thresholds=None):
    """Fill the odtk_level_t table.  Head tensors are taken AS THE CONVOLUTION WROTE THEM: float32 /
    bfloat16 / float16, NCHW or channels_last -- no .float(), no .contiguous() (reference
    model.py:160, box.py:263 make both copies)."""
    n = len(cls_heads)
    if not (n == len(box_heads) == len(anchors_list) == len(strides)) or n == 0 or n > MAX_LEVELS:
        raise RuntimeError('decode_levels: need 1..%d levels with matching lists' % MAX_LEVELS)
    batch = cls_heads[0].shape[0]
    dtype = cls_heads[0].dtype
    if dtype not in _DTYPES:
        raise RuntimeError('decode_levels: unsupported dtype %s' % dtype)
    arr = (Level * n)()
    keep = []
    num_anchors = None
    for i, (c, b, a, s) in enumerate(zip(cls_heads, box_heads, anchors_list, strides)):
        # (a 1 x 1 level or a one-channel head is NCHW- and NHWC-contiguous at once: it follows its partner; the bias fold wants
        #  the channels_last reading where both allow it)
        lay = _pair_layout(c, b, 'cls_head[%d]' % i, 'box_head[%d]' % i, '', prefer_channels_last=cls_bias is not None)
        if c.dtype != dtype or b.dtype != dtype:
            raise RuntimeError('decode_levels: all head tensors must share one dtype')
        flat = a.reshape(-1).tolist() if isinstance(a, torch.Tensor) else list(a)
        carr, ln = _anchor_array(flat)
        keep.append(carr)
        if num_anchors is None:
            num_anchors = ln // 4
        if ln != 4 * num_anchors or c.shape[0] != batch or b.shape != (batch, num_anchors * nb, c.shape[2], c.shape[3]):
            raise RuntimeError('decode_levels: inconsistent level %d' % i)
        arr[i].cls = c.data_ptr()
        arr[i].box = b.data_ptr()
        arr[i].height, arr[i].width = c.shape[2], c.shape[3]
        arr[i].stride = int(s)
        arr[i].channels_last = lay
        arr[i].anchors = ctypes.cast(carr, _fp)
        for name, bias, width in (('cls_bias', cls_bias, c.shape[1]), ('box_bias', box_bias, b.shape[1]),
                                  ('cls_thresholds', cls_thresholds if cls_bias is not None else None, c.shape[1] + 8)):
            if bias is None:
                continue
            t = bias[i] if isinstance(bias, (list, tuple)) else bias      # one tensor shared by all levels, or a list
            if t is None:
                continue
            if not t.is_cuda or t.dtype != torch.float32 or t.numel() != width or not t.is_contiguous():
                raise RuntimeError('decode_levels: %s must be a contiguous float32 CUDA vector of length %d' % (name, width))
            keep.append(t)
            setattr(arr[i], name, t.data_ptr())
    num_classes = cls_heads[0].shape[1] // num_anchors
    return arr, keep, batch, num_anchors, num_classes, _DTYPES[dtype]


def decode_levels(cls_heads, box_heads, anchors_list, strides, score_thresh, top_n, rotated=False,
                  return_indices=False, logits=False, cls_bias=None, box_bias=None, cls_thresholds=None):
    """All levels x whole batch in one enqueue; returns tensors already in the layout of
    `torch.cat(per_level, 1)` (odtk/model.py:164): [B, L*top_n], [B, L*top_n, nb], [B, L*top_n].
    logits=True: cls_heads hold raw logits and the sigmoid is fused into the prefilter.
    cls_bias / box_bias: float32 CUDA vectors [A*C] / [A*nb] (or per-level lists) -- the bias of the heads'
    last convolutions, added inside the kernels (cls_bias: logits, 16-bit channels_last heads only)."""
    lib = library()
    nb = 6 if rotated else 4
    arr, keep, batch, num_anchors, num_classes, dtype = _levels(cls_heads, box_heads, anchors_list, strides, nb,
                                                                cls_bias, box_bias, cls_thresholds)
    dev = cls_heads[0].device
    n = len(cls_heads)
    out = _detections(batch, n * top_n, nb, dev, return_indices)
    flags = (FLAG_ROTATED if rotated else 0) | (FLAG_LOGITS if logits else 0)
    _enqueue(lib.odtk_decode_levels, 'decode_levels', dev, batch, n, arr, num_anchors, num_classes, dtype, flags,
             float(score_thresh), int(top_n), _ptrs(out), len(out))
    return out


def detect(cls_heads, box_heads, anchors_list, strides, score_thresh, top_n, nms_thresh, detections_per_im,
           rotated=False, logits=False, cls_bias=None, box_bias=None, cls_thresholds=None):
    """decode_levels + nms back to back (the whole of odtk/model.py:140-165): three launches -- prefilter, select + decode, nms
    -- (rotated boxes: five to seven), no host synchronisation, one workspace."""
    lib = library()
    nb = 6 if rotated else 4
    arr, keep, batch, num_anchors, num_classes, dtype = _levels(cls_heads, box_heads, anchors_list, strides, nb,
                                                                cls_bias, box_bias, cls_thresholds)
    dev = cls_heads[0].device
    out = _detections(batch, detections_per_im, nb, dev)
    flags = (FLAG_ROTATED if rotated else 0) | (FLAG_LOGITS if logits else 0)
    _enqueue(lib.odtk_detect, 'detect', dev, batch, len(cls_heads), arr, num_anchors, num_classes, dtype, flags,
             float(score_thresh), int(top_n), float(nms_thresh), int(detections_per_im), _ptrs(out))
    return out


def snap_to_anchors(targets, anchors, num_classes, height, width, stride, iou_background, iou_foreground,
                    want_cls_target=True):
    """Fused target assignment of one pyramid level for the whole batch (reference box.py:134-189 per
    image).  targets: float32 CUDA [B, N, 5] (x, y, w, h, class; class < 0 = padding row).
    -> cls_target [B, A, C, H, W] (None with want_cls_target=False: the fused loss derives it from depth),
    box_target [B, A, 4, H, W], depth [B, A, 1, H, W]."""
    _check_input(targets, 'targets')
    if targets.dim() != 3 or targets.shape[2] != 5:
        raise RuntimeError('targets must be [B, N, 5]')
    arr, n = _anchor_array(anchors.reshape(-1).tolist() if isinstance(anchors, torch.Tensor) else anchors)
    a = n // 4
    b, n_max = targets.shape[0], targets.shape[1]
    dev = targets.device
    cls = torch.empty((b, a, num_classes, height, width), dtype=torch.float32, device=dev) if want_cls_target else None
    box_t = torch.empty((b, a, 4, height, width), dtype=torch.float32, device=dev)
    depth = torch.empty((b, a, 1, height, width), dtype=torch.float32, device=dev)
    _launch(library().odtk_snap_to_anchors, 'snap_to_anchors', dev, b, targets.data_ptr(), n_max, arr, a, int(num_classes),
            int(height), int(width), int(stride), float(iou_background), float(iou_foreground),
            cls.data_ptr() if cls is not None else None, box_t.data_ptr(), depth.data_ptr())
    return cls, box_t, depth


def _snap_level_count(what, anchors_list, sizes, strides):
    n = len(anchors_list)
    if not (n == len(sizes) == len(strides)) or n == 0 or n > MAX_LEVELS:
        raise RuntimeError('%s: need 1..%d levels with matching lists' % (what, MAX_LEVELS))
    return n


def _snap_targets(arr, b, a, num_classes, nb, sizes, strides, dev, want_cls_target):
    """Allocate every level's targets and enter them, with the level's geometry, into its descriptor (SnapLevel and SnapRotLevel
    name these fields alike) -> lists (cls_targets or Nones, box_targets [B, A, nb, H, W], depths)."""
    cls_t, box_t, depth_t = [], [], []
    for lv, (h, w), s in zip(arr, sizes, strides):
        cls_t.append(torch.empty((b, a, num_classes, h, w), dtype=torch.float32, device=dev) if want_cls_target else None)
        box_t.append(torch.empty((b, a, nb, h, w), dtype=torch.float32, device=dev))
        depth_t.append(torch.empty((b, a, 1, h, w), dtype=torch.float32, device=dev))
        lv.cls_target = cls_t[-1].data_ptr() if want_cls_target else None
        lv.box_target, lv.depth = box_t[-1].data_ptr(), depth_t[-1].data_ptr()
        lv.height, lv.width, lv.stride = int(h), int(w), int(s)
    return cls_t, box_t, depth_t


def snap_to_anchors_rotated_levels(gt_axis, gt_quads, gt_class, anchors_list, num_classes, sizes, strides, iou_background,
                                   iou_foreground, want_cls_target=True):
    """Rotated target assignment (reference box.py:192-252) for every pyramid level of the batch in ONE launch.
    gt_axis [B, N, 6], gt_quads [B, N, 8], gt_class [B, N] (< 0: padding) float32 CUDA -- the reference's `rotate_boxes` output;
    anchors_list: per level (axis [A, 4], quads [A, 8]) float32 CUDA tensors; sizes: per level (H, W).
    -> lists (cls_targets or Nones, box_targets [B, A, 6, H, W], depths)."""
    for t, name, last in ((gt_axis, 'gt_axis', 6), (gt_quads, 'gt_quads', 8)):
        _check_input(t, name)
        if t.dim() != 3 or t.shape[2] != last:
            raise RuntimeError('%s must be [B, N, %d]' % (name, last))
    _check_input(gt_class, 'gt_class')
    n = _snap_level_count('snap_to_anchors_rotated_levels', anchors_list, sizes, strides)
    b, n_max = gt_axis.shape[0], gt_axis.shape[1]
    if gt_quads.shape[:2] != (b, n_max) or tuple(gt_class.shape) != (b, n_max):
        raise RuntimeError('snap_to_anchors_rotated_levels: gt_axis / gt_quads / gt_class disagree')
    dev = gt_axis.device
    arr = (SnapRotLevel * n)()
    a = None
    for lv, (axis, quads) in zip(arr, anchors_list):
        _check_input(axis, 'anchors (axis form)')
        _check_input(quads, 'anchors (quads)')
        if a is None:
            a = axis.shape[0]
        if tuple(axis.shape) != (a, 4) or tuple(quads.shape) != (a, 8):
            raise RuntimeError('snap_to_anchors_rotated_levels: every level needs [A, 4] and [A, 8] anchor tables')
        lv.anchors_axis, lv.anchors_quads = axis.data_ptr(), quads.data_ptr()
    out = _snap_targets(arr, b, a, num_classes, 6, sizes, strides, dev, want_cls_target)
    _launch(library().odtk_snap_to_anchors_rotated_levels, 'snap_to_anchors_rotated_levels', dev, b, gt_axis.data_ptr(),
            gt_quads.data_ptr(), gt_class.data_ptr(), n_max, n, arr, a, int(num_classes), float(iou_background), float(iou_foreground))
    return out


def _snap_levels(what, targets, anchors_list, sizes, strides):
    """Checks shared by the level forms over [B, N, 5] targets; enters every level's HOST anchor table into its descriptor
    -> (descriptor array, the ctypes arrays it points into, number of levels, anchors per cell)."""
    _check_input(targets, 'targets')
    if targets.dim() != 3 or targets.shape[2] != 5:
        raise RuntimeError('targets must be [B, N, 5]')
    n = _snap_level_count(what, anchors_list, sizes, strides)
    arr = (SnapLevel * n)()
    keep = []
    a = None
    for lv, anchors in zip(arr, anchors_list):
        carr, ln = _anchor_array(anchors.reshape(-1).tolist() if isinstance(anchors, torch.Tensor) else anchors)
        if a is None:
            a = ln // 4
        if ln != 4 * a:
            raise RuntimeError('%s: every level needs the same number of anchors' % what)
        keep.append(carr)
        lv.anchors = ctypes.cast(carr, _fp)
    return arr, keep, n, a


def snap_to_anchors_levels(targets, anchors_list, num_classes, sizes, strides, iou_background, iou_foreground,
                           want_cls_target=True):
    """`snap_to_anchors` for every pyramid level in ONE launch.  anchors_list: per level [A, 4]; sizes: per level (H, W).
    -> lists (cls_targets or Nones, box_targets, depths)."""
    arr, keep, n, a = _snap_levels('snap_to_anchors_levels', targets, anchors_list, sizes, strides)
    b, n_max = targets.shape[0], targets.shape[1]
    dev = targets.device
    out = _snap_targets(arr, b, a, num_classes, 4, sizes, strides, dev, want_cls_target)
    _launch(library().odtk_snap_to_anchors_levels, 'snap_to_anchors_levels', dev, b, targets.data_ptr(), n_max, n, arr, a,
            int(num_classes), float(iou_background), float(iou_foreground))
    return out


def atss_assign_levels(targets, anchors_list, num_classes, sizes, strides, topk=9, want_cls_target=True):
    """ATSS target assignment for every pyramid level of the batch (csrc/atss.hpp; two launches and a workspace).  Arguments and
    results as `snap_to_anchors_levels`, with `topk` (1..ATSS_MAX_TOPK nearest cells per box and level) in place of the IoU
    thresholds; depth is class + 1 or 0."""
    arr, keep, n, a = _snap_levels('atss_assign_levels', targets, anchors_list, sizes, strides)
    if not 1 <= int(topk) <= ATSS_MAX_TOPK:
        raise RuntimeError('atss_assign_levels: topk must be in 1..%d' % ATSS_MAX_TOPK)
    b, n_max = targets.shape[0], targets.shape[1]
    dev = targets.device
    out = _snap_targets(arr, b, a, num_classes, 4, sizes, strides, dev, want_cls_target)
    _enqueue(library().odtk_atss_assign_levels, 'atss_assign_levels', dev, b, targets.data_ptr(), n_max, n, arr, a,
             int(num_classes), int(topk))
    return out


def tal_assign_levels(targets, cls_heads, box_heads, anchors_list, num_classes, strides, topk=13, alpha=1, beta=6, want_cls_target=True):
    """Task-aligned target assignment for every pyramid level of the batch (csrc/tal.hpp; three launches and a workspace).
    cls_heads / box_heads: per level the logits [B, A * C, H, W] and deltas [B, A * 4, H, W] as the convolutions wrote them -- one
    dtype out of float32 / bfloat16 / float16, NCHW or channels_last, no copy.  Results as `atss_assign_levels`."""
    n = len(cls_heads)
    if len(box_heads) != n:
        raise RuntimeError('tal_assign_levels: need 1..%d levels with matching lists' % MAX_LEVELS)
    sizes = [tuple(int(v) for v in c.shape[-2:]) if isinstance(c, torch.Tensor) and c.dim() == 4 else (0, 0) for c in cls_heads]
    arr, keep, n, a = _snap_levels('tal_assign_levels', targets, anchors_list, sizes, strides)
    if not 1 <= int(topk) <= ATSS_MAX_TOPK:
        raise RuntimeError('tal_assign_levels: topk must be in 1..%d' % ATSS_MAX_TOPK)
    if not (0 <= int(alpha) <= 4 and 1 <= int(beta) <= 8):
        raise RuntimeError('tal_assign_levels: alpha must be in 0..4 and beta in 1..8')
    b, n_max = targets.shape[0], targets.shape[1]
    dev = targets.device
    heads = (LossLevel * n)()
    dtype = None
    for hd, c, x, (h, w) in zip(heads, cls_heads, box_heads, sizes):
        lay = _pair_layout(c, x, 'cls_head', 'box_head', 'tal_assign_levels: ')
        if c.dtype not in _DTYPES or x.dtype != c.dtype or (dtype is not None and c.dtype != dtype):
            raise RuntimeError('tal_assign_levels: heads must share one dtype out of float32 / bfloat16 / float16')
        dtype = c.dtype
        if tuple(c.shape) != (b, a * int(num_classes), h, w) or tuple(x.shape) != (b, a * 4, h, w) or c.device != dev or x.device != dev:
            raise RuntimeError('tal_assign_levels: inconsistent shapes')
        hd.cls, hd.box, hd.height, hd.width, hd.channels_last = c.data_ptr(), x.data_ptr(), h, w, lay
    out = _snap_targets(arr, b, a, num_classes, 4, sizes, strides, dev, want_cls_target)
    _enqueue(library().odtk_tal_assign_levels, 'tal_assign_levels', dev, b, targets.data_ptr(), n_max, n, arr, heads, a,
             int(num_classes), _DTYPES[dtype], int(topk), int(alpha), int(beta))
    return out


def _loss_geometry(cls_head, box_head, depth, box_target):
    """Shared validation of the fused loss entry points -> (B, A, C, H, W, nb, dtype enum, channels_last)."""
    if not (cls_head.is_cuda and box_head.is_cuda and depth.is_cuda and box_target.is_cuda):
        raise RuntimeError('retina_loss: tensors must be on the GPU')
    if cls_head.dim() != 4 or box_head.dim() != 4 or depth.dim() != 5 or box_target.dim() != 5:
        raise RuntimeError('retina_loss: cls/box must be [B, ch, H, W], depth [B, A, 1, H, W], box_target [B, A, nb, H, W]')
    lay = _pair_layout(cls_head, box_head, 'cls_head', 'box_head', 'retina_loss: ')
    b, ch, h, w = cls_head.shape
    a, nb = box_target.shape[1], box_target.shape[2]
    if cls_head.dtype not in _DTYPES or box_head.dtype != cls_head.dtype:
        raise RuntimeError('retina_loss: heads must share one dtype out of float32 / bfloat16 / float16')
    if ch % a or depth.shape != (b, a, 1, h, w) or box_target.shape != (b, a, nb, h, w) or box_head.shape != (b, a * nb, h, w):
        raise RuntimeError('retina_loss: inconsistent shapes')
    if depth.dtype != torch.float32 or box_target.dtype != torch.float32 or not depth.is_contiguous() or not box_target.is_contiguous():
        raise RuntimeError('retina_loss: depth and box_target must be contiguous float32')
    return b, a, ch // a, h, w, nb, _DTYPES[cls_head.dtype], lay


def _loss_levels(cls_heads, box_heads, depths, box_targets, grads=None):
    n = len(cls_heads)
    if not (n == len(box_heads) == len(depths) == len(box_targets)) or n == 0 or n > MAX_LEVELS:
        raise RuntimeError('retina_loss_levels: need 1..%d levels with matching lists' % MAX_LEVELS)
    arr = (LossLevel * n)()
    geo = None
    for i in range(n):
        b, a, c, h, w, nb, dtype, lay = _loss_geometry(cls_heads[i], box_heads[i], depths[i], box_targets[i])
        if geo is None:
            geo = (b, a, c, nb, dtype)
        elif geo != (b, a, c, nb, dtype):
            raise RuntimeError('retina_loss_levels: every level must share batch, anchors, classes, box parameters and dtype')
        arr[i].cls, arr[i].box = cls_heads[i].data_ptr(), box_heads[i].data_ptr()
        arr[i].depth, arr[i].box_target = depths[i].data_ptr(), box_targets[i].data_ptr()
        arr[i].height, arr[i].width, arr[i].channels_last = h, w, lay
        if grads is not None:
            arr[i].dcls, arr[i].dbox = grads[0][i].data_ptr(), grads[1][i].data_ptr()
    return arr, n, geo


def retina_loss_levels_forward(cls_heads, box_heads, depths, box_targets, alpha, gamma, beta, reproducible=False):
    """All pyramid levels in ONE launch -> float64 CUDA tensor [L, 3] = per level (cls_sum, box_sum, #foreground).
    reproducible=True (what odtk/loss.py asks for since round 6): the workgroups' sums go through a workspace and a second, tiny
    launch adds them up in a fixed order (odtk_retina_loss_levels_forward_ws): no atomics, the same bits on every run, and the walk
    is 8 us shorter than with three double atomics at the end of every workgroup (fp32, 2 images of 800 x 1280: 26.2 + 4.2 us for the
    two launches against 34.6; profiles/r06_loss_layout_probe.txt)."""
    arr, n, (b, a, c, nb, dtype) = _loss_levels(cls_heads, box_heads, depths, box_targets)
    dev = cls_heads[0].device
    sums = torch.empty((n, 3), dtype=torch.float64, device=dev)
    args = (n, arr, b, a, c, nb, dtype, float(alpha), float(gamma), float(beta), sums.data_ptr())
    if reproducible:
        _enqueue(library().odtk_retina_loss_levels_forward_ws, 'retina_loss_levels_forward', dev, *args)
    else:
        _launch(library().odtk_retina_loss_levels_forward, 'retina_loss_levels_forward', dev, *args)
    return sums


def retina_loss_levels_backward(cls_heads, box_heads, depths, box_targets, alpha, gamma, beta, grad_cls_sums, grad_box_sums):
    """Gradients of sum_l (g_cls[l] * cls_sum[l] + g_box[l] * box_sum[l]) w.r.t. every head, ONE launch.
    grad_*: float32 CUDA vectors [L] (or None = zeros), read on the device."""
    dev = cls_heads[0].device
    dcls = _head_grads('retina_loss_levels_backward', cls_heads)
    dbox = _head_grads('retina_loss_levels_backward', box_heads)
    arr, n, (b, a, c, nb, dtype) = _loss_levels(cls_heads, box_heads, depths, box_targets, (dcls, dbox))
    g_cls, g_box = _grad_vector(grad_cls_sums, n, dev), _grad_vector(grad_box_sums, n, dev)
    _launch(library().odtk_retina_loss_levels_backward, 'retina_loss_levels_backward', dev, n, arr, b, a, c, nb, dtype,
            float(alpha), float(gamma), float(beta), g_cls.data_ptr() if g_cls is not None else None,
            g_box.data_ptr() if g_box is not None else None)
    return dcls, dbox


def _box_iou_levels(what, box_heads, depths, box_targets, anchors_list, kind, grads=None, nb=4, kinds=BOX_LOSS_KINDS):
    """Validation and level table shared by the IoU-family box losses (nb = 4 parameters per anchor) and the Gaussian losses of
    rotated boxes (nb = 6, kinds = ROTATED_BOX_LOSS_KINDS) -> (descriptors, anchor pointers, the ctypes arrays they point into,
    levels, batch, anchors, dtype enum, kind enum)."""
    n = len(box_heads)
    if not (n == len(depths) == len(box_targets) == len(anchors_list)) or n == 0 or n > MAX_LEVELS:
        raise RuntimeError('%s: need 1..%d levels with matching lists' % (what, MAX_LEVELS))
    if kind not in kinds:
        raise RuntimeError("%s: kind must be %s, not %r" % (what, "'iou', 'giou' or 'diou'" if nb == 4 else "'probiou' or 'kld'", kind))
    arr = (LossLevel * n)()
    tables = (_fp * n)()
    keep, geo = [], None
    for i, (head, depth, target, anchors) in enumerate(zip(box_heads, depths, box_targets, anchors_list)):
        if not (head.is_cuda and depth.is_cuda and target.is_cuda):
            raise RuntimeError('%s: tensors must be on the GPU' % what)
        if head.dim() != 4 or depth.dim() != 5 or target.dim() != 5 or head.dtype not in _DTYPES:
            raise RuntimeError('%s: box heads must be [B, A*%d, H, W] float32 / bfloat16 / float16, depth [B, A, 1, H, W], '
                               'box_target [B, A, %d, H, W]' % (what, nb, nb))
        b, ch, h, w = head.shape
        a = target.shape[1]
        if head.is_contiguous():
            lay = 0
        elif head.is_contiguous(memory_format=torch.channels_last):
            lay = 1
        else:
            raise RuntimeError('%s: box heads must be dense NCHW or channels_last' % what)
        if ch != nb * a or tuple(depth.shape) != (b, a, 1, h, w) or tuple(target.shape) != (b, a, nb, h, w):
            raise RuntimeError('%s: inconsistent shapes' % what)
        if depth.dtype != torch.float32 or target.dtype != torch.float32 or not depth.is_contiguous() or not target.is_contiguous():
            raise RuntimeError('%s: depth and box_target must be contiguous float32' % what)
        if geo is None:
            geo = (b, a, _DTYPES[head.dtype])
        elif geo != (b, a, _DTYPES[head.dtype]):
            raise RuntimeError('%s: every level must share batch, anchors and dtype' % what)
        carr, ln = _anchor_array(anchors.reshape(-1).tolist() if isinstance(anchors, torch.Tensor) else anchors)
        if ln != 4 * a:
            raise RuntimeError('%s: every level needs an [A, 4] anchor table' % what)
        keep.append(carr)
        tables[i] = ctypes.cast(carr, _fp)
        arr[i].box, arr[i].depth, arr[i].box_target = head.data_ptr(), depth.data_ptr(), target.data_ptr()
        arr[i].height, arr[i].width, arr[i].channels_last = h, w, lay
        if grads is not None:
            arr[i].dbox = grads[i].data_ptr()
    return arr, tables, keep, n, geo[0], geo[1], geo[2], kinds[kind]


def _head_grads(what, heads):
    """Uninitialised gradients of `heads` in the heads' own layout (the kernels write every element)."""
    grads = [torch.empty_like(t) for t in heads]
    for g, t in zip(grads, heads):
        if g.stride() != t.stride():
            raise RuntimeError('%s: could not allocate gradients in the heads\' layout' % what)
    return grads


def _grad_vector(grad, n, dev):
    """An upstream gradient per level -> float32 vector [n] on `dev`, read on the device; None stays None (= zeros)."""
    return None if grad is None else grad.detach().to(device=dev, dtype=torch.float32).reshape(n).contiguous()


def _pair_sums_forward(what, dev, n, *args):
    """Enqueue the forward entry point odtk_<what> (two launches through the workspace) -> float64 [n, 2] = per level (sum, #foreground)."""
    sums = torch.empty((n, 2), dtype=torch.float64, device=dev)
    _enqueue(getattr(library(), 'odtk_' + what), what, dev, n, *args, sums.data_ptr())
    return sums


def _pair_sums_backward(what, dev, n, grad_sums, *args):
    g = _grad_vector(grad_sums, n, dev)
    _launch(getattr(library(), 'odtk_' + what), what, dev, n, *args, g.data_ptr() if g is not None else None)


def _box_loss_levels_forward(what, nb, kinds, box_heads, depths, box_targets, anchors_list, kind):
    arr, tables, keep, n, b, a, dtype, code = _box_iou_levels(what, box_heads, depths, box_targets, anchors_list, kind, None, nb, kinds)
    return _pair_sums_forward(what, box_heads[0].device, n, arr, tables, b, a, dtype, code)


def _box_loss_levels_backward(what, nb, kinds, box_heads, depths, box_targets, anchors_list, kind, grad_sums):
    dev = box_heads[0].device
    dbox = _head_grads(what, box_heads)
    arr, tables, keep, n, b, a, dtype, code = _box_iou_levels(what, box_heads, depths, box_targets, anchors_list, kind, dbox, nb, kinds)
    _pair_sums_backward(what, dev, n, grad_sums, arr, tables, b, a, dtype, code)
    return dbox


def box_iou_loss_levels_forward(box_heads, depths, box_targets, anchors_list, kind):
    """IoU / GIoU / DIoU box loss ('iou' | 'giou' | 'diou') at the foreground anchors of all pyramid levels (csrc/box_iou_loss.hpp)
    -> float64 CUDA tensor [L, 2] = per level (sum of the losses, #foreground).  anchors_list: per level [A, 4].  Two launches, no
    atomics: the same bits on every run."""
    return _box_loss_levels_forward('box_iou_loss_levels_forward', 4, BOX_LOSS_KINDS, box_heads, depths, box_targets, anchors_list, kind)


def box_iou_loss_levels_backward(box_heads, depths, box_targets, anchors_list, kind, grad_sums):
    """Gradients of sum_l grad_sums[l] * box_sum[l] w.r.t. every box head, in the heads' dtype and layout, ONE launch.
    grad_sums: float32 CUDA vector [L] (or None = zeros), read on the device."""
    return _box_loss_levels_backward('box_iou_loss_levels_backward', 4, BOX_LOSS_KINDS, box_heads, depths, box_targets, anchors_list, kind,
                                     grad_sums)


def rotated_box_loss_levels_forward(box_heads, depths, box_targets, anchors_list, kind):
    """ProbIoU / KLD box loss ('probiou' | 'kld') on the Gaussians of rotated boxes, at the foreground anchors of all pyramid
    levels (csrc/rotated_box_loss.hpp; the definition: odtk/loss.py:rotated_box_loss) -> float64 CUDA tensor [L, 2] = per level
    (sum of the losses, #foreground).  box_heads [B, A*6, H, W], box_targets [B, A, 6, H, W]; anchors_list: per level the AXIS
    table [A, 4] of the (axis, rotated) anchor pair.  Two launches, no atomics: the same bits on every run."""
    return _box_loss_levels_forward('rotated_box_loss_levels_forward', 6, ROTATED_BOX_LOSS_KINDS, box_heads, depths, box_targets,
                                    anchors_list, kind)


def rotated_box_loss_levels_backward(box_heads, depths, box_targets, anchors_list, kind, grad_sums):
    """Gradients of sum_l grad_sums[l] * box_sum[l] w.r.t. every box head (all six deltas), in the heads' dtype and layout, ONE
    launch.  grad_sums: float32 CUDA vector [L] (or None = zeros), read on the device."""
    return _box_loss_levels_backward('rotated_box_loss_levels_backward', 6, ROTATED_BOX_LOSS_KINDS, box_heads, depths, box_targets,
                                     anchors_list, kind, grad_sums)


def _quality_levels(what, cls_heads, box_heads, depths, box_targets, anchors_list, kind, alpha, gamma, grads=None):
    """Validation and level table of the quality / varifocal classification losses: the box side as the IoU-family box losses
    check it, then the logits -> (descriptors, anchor pointers, what they point into, levels, batch, anchors, classes, dtype enum,
    kind enum)."""
    if kind not in CLS_LOSS_KINDS:
        raise RuntimeError("%s: kind must be 'qfl' or 'vfl', not %r" % (what, kind))
    if not (float(gamma) >= 1 and float(gamma) < float('inf')) or not (float(alpha) >= 0 and float(alpha) < float('inf')):
        raise RuntimeError('%s: gamma must be finite and >= 1, alpha finite and >= 0 (not %r, %r)' % (what, gamma, alpha))
    if len(cls_heads) != len(box_heads):
        raise RuntimeError('%s: need 1..%d levels with matching lists' % (what, MAX_LEVELS))
    arr, tables, keep, n, b, a, dtype, _ = _box_iou_levels(what, box_heads, depths, box_targets, anchors_list, 'iou')
    classes = None
    for i, (cls_head, box_head) in enumerate(zip(cls_heads, box_heads)):
        lay = _pair_layout(cls_head, box_head, 'cls_head', 'box_head', what + ': ')
        if cls_head.dtype != box_head.dtype:
            raise RuntimeError('%s: heads must share one dtype out of float32 / bfloat16 / float16' % what)
        if cls_head.shape[0] != b or cls_head.shape[1] % a or tuple(cls_head.shape[2:]) != tuple(box_head.shape[2:]):
            raise RuntimeError('%s: inconsistent shapes' % what)
        if classes is None:
            classes = cls_head.shape[1] // a
        if cls_head.shape[1] != a * classes or classes < 1:
            raise RuntimeError('%s: every level must share the number of classes' % what)
        arr[i].cls, arr[i].channels_last = cls_head.data_ptr(), lay
        if grads is not None:
            arr[i].dcls = grads[i].data_ptr()
    return arr, tables, keep, n, b, a, classes, dtype, CLS_LOSS_KINDS[kind]


def quality_loss_levels_forward(cls_heads, box_heads, depths, box_targets, anchors_list, kind, alpha=0.75, gamma=2.0):
    """Quality focal ('qfl') or varifocal ('vfl') classification loss over the logits of all pyramid levels (csrc/quality_loss.hpp;
    the definition: odtk/loss.py) -> float64 CUDA tensor [L, 2] = per level (sum of the losses, #foreground).  The soft target --
    the IoU of the predicted and the assigned box at every foreground anchor -- is computed in the walk from box_heads / box_targets /
    anchors_list (per level [A, 4]).  Two launches, no atomics: the same bits on every run."""
    what = 'quality_loss_levels_forward'
    arr, tables, keep, n, b, a, c, dtype, code = _quality_levels(what, cls_heads, box_heads, depths, box_targets, anchors_list, kind, alpha, gamma)
    return _pair_sums_forward(what, cls_heads[0].device, n, arr, tables, b, a, c, dtype, code, float(alpha), float(gamma))


def quality_loss_levels_backward(cls_heads, box_heads, depths, box_targets, anchors_list, kind, alpha, gamma, grad_sums):
    """Gradients of sum_l grad_sums[l] * cls_sum[l] w.r.t. every class head, in the heads' dtype and layout, ONE launch (the box
    heads get none: the quality is a constant of this loss).  grad_sums: float32 CUDA vector [L] (or None = zeros), read on the device."""
    what, dev = 'quality_loss_levels_backward', cls_heads[0].device
    dcls = _head_grads(what, cls_heads)
    arr, tables, keep, n, b, a, c, dtype, code = _quality_levels(what, cls_heads, box_heads, depths, box_targets, anchors_list, kind, alpha,
                                                                 gamma, dcls)
    _pair_sums_backward(what, dev, n, grad_sums, arr, tables, b, a, c, dtype, code, float(alpha), float(gamma))
    return dcls


def retina_loss_forward(cls_head, box_head, depth, box_target, alpha, gamma, beta):
    """-> float64 CUDA tensor [3] = (sum of masked focal losses, sum of masked smooth-L1 losses, #foreground anchors)
    of one level (reference model.py:193-209 + loss.py:13-31 in one pass; csrc/loss.hpp)."""
    b, a, c, h, w, nb, dtype, lay = _loss_geometry(cls_head, box_head, depth, box_target)
    sums = torch.empty(3, dtype=torch.float64, device=cls_head.device)
    _launch(library().odtk_retina_loss_forward, 'retina_loss_forward', cls_head.device, cls_head.data_ptr(), box_head.data_ptr(),
            depth.data_ptr(), box_target.data_ptr(), b, a, c, h, w, nb, dtype, lay, float(alpha), float(gamma), float(beta),
            sums.data_ptr())
    return sums


def retina_loss_backward(cls_head, box_head, depth, box_target, alpha, gamma, beta, grad_cls_sum, grad_box_sum):
    """Gradients of (g_cls * cls_sum + g_box * box_sum) w.r.t. the two heads, in the heads' dtype and layout.
    grad_*: float32 CUDA scalars (or None = 0), read on the device."""
    b, a, c, h, w, nb, dtype, lay = _loss_geometry(cls_head, box_head, depth, box_target)
    dev = cls_head.device

    def scalar(g):
        if g is None:
            return None
        g = g.detach().to(device=dev, dtype=torch.float32).reshape(1)
        return g

    g_cls, g_box = scalar(grad_cls_sum), scalar(grad_box_sum)
    dcls = torch.empty_like(cls_head)                   # preserves the (dense) memory format
    dbox = torch.empty_like(box_head)
    if dcls.stride() != cls_head.stride() or dbox.stride() != box_head.stride():
        raise RuntimeError('retina_loss_backward: could not allocate gradients in the heads\' layout')
    _launch(library().odtk_retina_loss_backward, 'retina_loss_backward', dev, cls_head.data_ptr(), box_head.data_ptr(),
            depth.data_ptr(), box_target.data_ptr(), b, a, c, h, w, nb, dtype, lay, float(alpha), float(gamma), float(beta),
            g_cls.data_ptr() if g_cls is not None else None, g_box.data_ptr() if g_box is not None else None,
            dcls.data_ptr(), dbox.data_ptr())
    return dcls, dbox


def _channels_last(t, or_one_pixel=False):
    """channels_last -- or, where the caller allows it, a 1 x 1 map (whose strides torch reports either way)."""
    return t.is_contiguous(memory_format=torch.channels_last) or (or_one_pixel and t.shape[2] * t.shape[3] == 1)


def _bias_vector(bias, c):
    return bias.dtype == torch.float32 and bias.numel() == c and bias.is_cuda


def bias_act_(y, bias, residual=None, relu=True):
    """In place on a channels_last activation: y = act(y + bias[c] (+ residual)).  `bias` is a float32
    device vector [C].  Replaces the separate bias / frozen-BN / residual-add / ReLU passes.
    The sums are float32, rounded once (to nearest even) to y's dtype.  The ReLU is `o > 0 ? o : (isnan(o) ? o : +0.0)`: a NaN goes
    through, and a sum of -0.0 becomes +0.0 -- torch.relu keeps the -0.0, so the two differ in that one sign bit
    (tests/engine_streams_ref.py restates the kernel's rule)."""
    if not y.is_cuda or y.dim() != 4 or y.dtype not in _DTYPES:
        raise RuntimeError('bias_act_: y must be a 4-d CUDA tensor of float32/bfloat16/float16')
    n, c, h, w = y.shape
    if not _channels_last(y, True):
        raise RuntimeError('bias_act_: y must be channels_last')
    if not _bias_vector(bias, c):
        raise RuntimeError('bias_act_: bias must be a float32 CUDA vector of length C')
    if residual is not None and (residual.shape != y.shape or residual.dtype != y.dtype or not _channels_last(residual, True)):
        raise RuntimeError('bias_act_: residual must match y (shape, dtype, channels_last)')
    _launch(library().odtk_bias_act, 'bias_act', y.device, y.data_ptr(), bias.data_ptr(),
            residual.data_ptr() if residual is not None else None, n * h * w, c, _DTYPES[y.dtype], 1 if relu else 0)
    _count('bias_act_kernel', y.numel() * y.element_size() * (3 if residual is not None else 2))
    return y


def bias_act_maxpool(y, bias, relu=True):
    """maxpool3x3/s2/p1(act(y + bias[c])) of a channels_last bf16/fp16 activation in one pass (the ResNet
    stem after conv1); bit-identical to bias_act_ followed by F.max_pool2d(., 3, 2, 1)."""
    if not y.is_cuda or y.dim() != 4 or y.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError('bias_act_maxpool: y must be a 4-d CUDA tensor of bfloat16/float16')
    n, c, h, w = y.shape
    if not _channels_last(y) or c % 8:
        raise RuntimeError('bias_act_maxpool: y must be channels_last with channels % 8 == 0')
    if not _bias_vector(bias, c):
        raise RuntimeError('bias_act_maxpool: bias must be a float32 CUDA vector of length C')
    out = torch.empty((n, c, (h + 1) // 2, (w + 1) // 2), dtype=y.dtype, device=y.device, memory_format=torch.channels_last)
    _launch(library().odtk_bias_act_maxpool, 'bias_act_maxpool', y.device, y.data_ptr(), bias.data_ptr(), out.data_ptr(), n, h, w, c,
            _DTYPES[y.dtype], 1 if relu else 0)
    _count('bias_act_maxpool_kernel', (y.numel() + out.numel()) * y.element_size())
    return out


def upsample2x(x):
    """Nearest-neighbour 2x upsampling of a channels_last CUDA activation (the FPN's top-down path); bit-identical to
    F.interpolate(x, scale_factor=2) in channels_last.  One HIP stream kernel instead of torch's upsample + layout copy."""
    if not x.is_cuda or x.dim() != 4 or x.dtype not in _DTYPES:
        raise RuntimeError('upsample2x: x must be a 4-d CUDA tensor of float32/bfloat16/float16')
    n, c, h, w = x.shape
    if not _channels_last(x) or (c * x.element_size()) % 16:
        raise RuntimeError('upsample2x: x must be channels_last with channels * element size a multiple of 16 bytes')
    out = torch.empty((n, c, 2 * h, 2 * w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    _launch(library().odtk_upsample_nearest2x, 'upsample2x', x.device, x.data_ptr(), out.data_ptr(), n, h, w, c, _DTYPES[x.dtype])
    _count('upsample_nearest2x_kernel', (x.numel() + out.numel()) * x.element_size())
    return out


def _canvas_args(canvas, rects, what):
    if not canvas.is_cuda or canvas.dim() != 4 or canvas.dtype not in _DTYPES:
        raise RuntimeError('%s: canvas must be a 4-d CUDA tensor of float32/bfloat16/float16' % what)
    n, c, h, w = canvas.shape
    if not _channels_last(canvas) or (c * canvas.element_size()) % 16:
        raise RuntimeError('%s: canvas must be channels_last with channels * element size a multiple of 16 bytes' % what)
    if len(rects) > MAX_LEVELS:
        raise RuntimeError('%s: at most %d rectangles' % (what, MAX_LEVELS))
    flat = [int(v) for r in rects for v in r]
    if len(flat) != 4 * len(rects):
        raise RuntimeError('%s: a rectangle is (y0, x0, height, width)' % what)
    return n, c, h, w, (ctypes.c_int * max(len(flat), 1))(*flat)


def canvas_clear_(canvas, rects):
    """In place: zero every pixel of the channels_last `canvas` outside `rects` = [(y0, x0, height, width), ...] (the gutters of the
    engine's pyramid canvas; include/odtk_hip.h: odtk_canvas_clear).  One launch; pixels inside the rectangles are not touched."""
    n, c, h, w, arr = _canvas_args(canvas, rects, 'canvas_clear_')
    _launch(library().odtk_canvas_clear, 'canvas_clear', canvas.device, canvas.data_ptr(), n, h, w, c, _DTYPES[canvas.dtype], arr,
            len(rects))
    return canvas


def canvas_pack(levels, rects, height, width):
    """The pyramid canvas [B, C, height, width] (channels_last) of the channels_last activations `levels`: level i in rectangle
    rects[i] = (y0, x0, height_i, width_i), zeros elsewhere (include/odtk_hip.h: odtk_canvas_pack).  One launch."""
    first = levels[0]
    n, c = first.shape[:2]
    if len(levels) != len(rects):
        raise RuntimeError('canvas_pack: one rectangle per level')
    for t, r in zip(levels, rects):
        if (not t.is_cuda or t.dim() != 4 or t.dtype != first.dtype or t.device != first.device or tuple(t.shape) != (n, c, r[2], r[3])
                or not _channels_last(t)):
            raise RuntimeError('canvas_pack: every level must be a channels_last [B, C, h, w] CUDA tensor of one dtype filling its rectangle')
    canvas = torch.empty((n, c, height, width), dtype=first.dtype, device=first.device, memory_format=torch.channels_last)
    n, c, h, w, arr = _canvas_args(canvas, rects, 'canvas_pack')
    _launch(library().odtk_canvas_pack, 'canvas_pack', canvas.device, canvas.data_ptr(), n, h, w, c, _DTYPES[canvas.dtype], arr,
            _ptrs(list(levels)), len(rects))
    return canvas


def stem_pack(x, dtype):
    """2x2 space-to-depth pack of the network input [B, 3, H, W] (float32 / bfloat16 / float16, NCHW- or channels_last-contiguous, H and
    W even) into [B, 16, H/2, W/2] channels_last of `dtype` (bf16 / fp16): channel (dy*2+dx)*3+c of pixel (y, x) is x[:, c, 2y+dy, 2x+dx],
    channels 12..15 are zero (include/odtk_hip.h: odtk_stem_pack).  The cast and the layout change of the input, in one pass."""
    if not x.is_cuda or x.dim() != 4 or x.shape[1] != 3 or x.dtype not in _DTYPES or dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError('stem_pack: x must be a [B, 3, H, W] CUDA tensor of float32/bfloat16/float16, dtype bfloat16/float16')
    n, _, h, w = x.shape
    if h % 2 or w % 2:
        raise RuntimeError('stem_pack: height and width must be even')
    if x.is_contiguous():
        cl = 0
    elif x.is_contiguous(memory_format=torch.channels_last):
        cl = 1
    else:
        raise RuntimeError('stem_pack: x must be contiguous (NCHW or channels_last)')
    out = torch.empty((n, 16, h // 2, w // 2), dtype=dtype, device=x.device, memory_format=torch.channels_last)
    _launch(library().odtk_stem_pack, 'stem_pack', x.device, x.data_ptr(), out.data_ptr(), n, h, w, _DTYPES[x.dtype], cl, _DTYPES[dtype])
    return out


STREAM_TUNING_FIELDS = ('grid_cap', 'pool_wide_index')


def stream_tuning(grid_cap=-1, pool_wide_index=-1):
    """Debug / test: the launch shape of the engine's streaming kernels (include/odtk_hip.h: odtk_debug_stream_tuning).  grid_cap
    0 = every launcher's own grid cap, 1 .. 65536 replaces them all; pool_wide_index 1 = bias_act_maxpool with 64-bit index
    arithmetic; -1 leaves a field alone.  Process-wide; never touches the GPU."""
    _check(library().odtk_debug_stream_tuning(int(grid_cap), int(pool_wide_index)), 'stream_tuning')


def stream_tuning_state():
    """What stream_tuning holds, as a dict over STREAM_TUNING_FIELDS; stream_tuning(**state) puts it back."""
    out = (ctypes.c_int * 2)()
    _check(library().odtk_debug_stream_tuning_get(out), 'stream_tuning_state')
    return dict(zip(STREAM_TUNING_FIELDS, (int(v) for v in out)))


def bias_act_grid(n_pixels, channels, dtype):
    """What bias_act_ launches for [n_pixels, channels] of the torch `dtype` under the current stream_tuning -> dict(form =
    'scalar' / 'fast', blocks, stride, trips) (include/odtk_hip.h: odtk_debug_bias_act_grid).  Never touches the GPU."""
    out = (ctypes.c_uint * 4)()
    _check(library().odtk_debug_bias_act_grid(int(n_pixels), int(channels), _DTYPES[dtype], out), 'bias_act_grid')
    return {'form': ('scalar', 'fast')[out[0]], 'blocks': int(out[1]), 'stride': int(out[2]), 'trips': int(out[3])}


def _image_args(what, src, images, tables, table, height, width, batch=None):
    """Shared by preprocess_images / augment_images / mosaic_images: checks src, tables and table, coerces `images` to a ctypes array
    and allocates the output (`batch` images; default: as many as `images`) -> (images, out, the arguments the entry points take
    from src on)."""
    if not src.is_cuda or src.dtype != torch.uint8 or not src.is_contiguous():
        raise RuntimeError('%s: src must be a contiguous uint8 CUDA tensor' % what)
    if tables.device != src.device or tables.dtype != torch.int32 or not tables.is_contiguous():
        raise RuntimeError('%s: tables must be a contiguous int32 tensor on the device of src' % what)
    if table.device != src.device or table.dtype not in _DTYPES or tuple(table.shape) != (3, 256) or not table.is_contiguous():
        raise RuntimeError('%s: table must be a contiguous [3, 256] float32/bfloat16/float16 tensor on the device of src' % what)
    if not isinstance(images, ctypes.Array):
        images = (Image * len(images))(*images)
    out = torch.empty((len(images) if batch is None else batch, 3, height, width), dtype=table.dtype, device=src.device,
                      memory_format=torch.channels_last)
    return images, out, (src.data_ptr(), src.numel(), tables.data_ptr() if tables.numel() else None, tables.numel(),
                         table.data_ptr(), out.data_ptr(), height, width, _DTYPES[table.dtype])


def preprocess_images(src, images, tables, table, height, width):
    """The network's input from decoded source images in one launch (include/odtk_hip.h: odtk_preprocess_images): Pillow-exact
    bilinear resize, mirror, zero padding to height x width, normalisation, channels_last.
    src: uint8 CUDA tensor holding the source pixels (R G B interleaved); images: a ctypes array (or sequence) of `Image`, HOST
    memory; tables: int32 CUDA tensor of the resampling tables (odtk/data.py: resample_weights; may be empty when no image is
    resized); table: [3, 256] CUDA tensor of float32 / bfloat16 / float16, whose dtype is the output's.
    -> [len(images), 3, height, width] with channels_last strides."""
    images, out, args = _image_args('preprocess_images', src, images, tables, table, height, width)
    _launch(library().odtk_preprocess_images, 'preprocess_images', src.device, len(images), images, *args)
    return out


def augment_images(src, images, augments, tables, table, height, width, rotations=None):
    """`preprocess_images` with the training augmentations between the resize and the normalisation (include/odtk_hip.h:
    odtk_augment_images): quarter turn and flip as an index map, brightness, contrast, hue, saturation, Pillow-exact.
    augments: a ctypes array (or sequence) of `Augment`, one per image, HOST memory; the rest as `preprocess_images`.
    rotations: None, or a ctypes array (or sequence) of `Rotation`, one per image, HOST memory: the free rotation between the turn
    and the flip (odtk_augment_images_ex).
    -> [len(images), 3, height, width] with channels_last strides."""
    images, out, args = _image_args('augment_images', src, images, tables, table, height, width)
    if not isinstance(augments, ctypes.Array):
        augments = (Augment * len(augments))(*augments)
    if len(augments) != len(images):
        raise RuntimeError('augment_images: %d images but %d augment descriptors' % (len(images), len(augments)))
    if rotations is None:
        _enqueue(library().odtk_augment_images, 'augment_images', src.device, len(images), images, augments, *args)
        return out
    if not isinstance(rotations, ctypes.Array):
        rotations = (Rotation * len(rotations))(*rotations)
    if len(rotations) != len(images):
        raise RuntimeError('augment_images: %d images but %d rotation descriptors' % (len(images), len(rotations)))
    _enqueue(library().odtk_augment_images_ex, 'augment_images', src.device, len(images), images, augments, rotations, *args)
    return out


def mosaic_images(src, images, mosaics, augments, tables, table, height, width):
    """Mosaic augmentation on the device (include/odtk_hip.h: odtk_mosaic_images): `images` are the SOURCES (resized as
    `preprocess_images` resizes them, `mirror` allowed), `mosaics` one `Mosaic` per OUTPUT image that pastes up to four of them, each
    cropped to its rectangle, on a canvas of the fill colour; then the colour operations of `augments` (one `Augment` per output
    image with the mosaic's canvas and the identity map, or None: no colours), the table and the pad, Pillow-exact.
    mosaics, augments: ctypes arrays (or sequences), HOST memory; the rest as `preprocess_images`.
    -> [len(mosaics), 3, height, width] with channels_last strides."""
    if not isinstance(mosaics, ctypes.Array):
        mosaics = (Mosaic * len(mosaics))(*mosaics)
    images, out, args = _image_args('mosaic_images', src, images, tables, table, height, width, batch=len(mosaics))
    if augments is not None:
        if not isinstance(augments, ctypes.Array):
            augments = (Augment * len(augments))(*augments)
        if len(augments) != len(mosaics):
            raise RuntimeError('mosaic_images: %d output images but %d augment descriptors' % (len(mosaics), len(augments)))
    max_pixels = max((im.out_width * im.out_height for im in images), default=0)
    _enqueue(library().odtk_mosaic_images, 'mosaic_images', src.device, len(mosaics), mosaics, augments, len(images), images, max_pixels,
             *args)
    return out


_GEMM_WORKSPACE = {}     # a dictionary of its own: the 32 MiB GEMM buffer and the decode scratch never replace each other
_GEMM_READY = []


def _gemm_setup(device):
    """Bind hipBLASLt (the copy PyTorch ships, so that one copy of the soname serves the process) and keep one 32 MiB
    scratch buffer per (device, stream) -- GEMMs on different streams may run at the same time; `_workspace`'s rules
    (its lock; a captured call gets a buffer of its own).  -> (buffer, stream handle)"""
    if not gemm_available():
        raise RuntimeError('gemm_bias_act: hipBLASLt could not be bound (odtk_gemm_init failed)')
    return _workspace(device, 32 << 20, _GEMM_WORKSPACE)


def gemm_available():
    """True when hipBLASLt could be bound (it ships with ROCm and with PyTorch-ROCm).  When it cannot, the
    fused graph keeps its 1x1 convolutions on MIOpen + the HIP epilogue -- slower, same results."""
    if not _GEMM_READY:
        shipped = os.path.join(os.path.dirname(torch.__file__), 'lib', 'libhipblaslt.so')
        path = shipped if os.path.exists(shipped) else None
        rc = library().odtk_gemm_init(path.encode() if path else None)
        _GEMM_READY.append(rc == OK)
    return _GEMM_READY[0]


def gemm_bias_act(x, weight, bias, residual=None, relu=True):
    """1x1 convolution of a channels_last activation as one hipBLASLt GEMM with bias (+ residual)
    (+ ReLU) in its epilogue: returns act(conv1x1(x, weight) + bias (+ residual)), channels_last.
    x [B, Cin, H, W] channels_last, weight [Cout, Cin] (or [Cout, Cin, 1, 1]), bias float32 [Cout]."""
    if not x.is_cuda or x.dim() != 4 or x.dtype not in _DTYPES:
        raise RuntimeError('gemm_bias_act: x must be a 4-d CUDA tensor of float32/bfloat16/float16')
    b, k, h, w = x.shape
    n = weight.shape[0]
    if weight.numel() != n * k or weight.dtype != x.dtype or not weight.is_contiguous() and not weight.is_contiguous(
            memory_format=torch.channels_last):
        raise RuntimeError('gemm_bias_act: weight must be a dense [Cout, Cin(, 1, 1)] tensor of x.dtype')
    if not _channels_last(x, True):
        raise RuntimeError('gemm_bias_act: x must be channels_last')
    if not _bias_vector(bias, n):
        raise RuntimeError('gemm_bias_act: bias must be a float32 CUDA vector of length Cout')
    y = torch.empty((b, n, h, w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    if residual is not None and (residual.shape != y.shape or residual.dtype != y.dtype or not _channels_last(residual, True)):
        raise RuntimeError('gemm_bias_act: residual must match the output (shape, dtype, channels_last)')
    with torch.cuda.device(x.device):
        ws, stream = _gemm_setup(x.device)
        _check(library().odtk_gemm_bias_act(y.data_ptr(), x.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                                            residual.data_ptr() if residual is not None else None,
                                            b * h * w, n, k, _DTYPES[x.dtype], 1 if relu else 0,
                                            ws.data_ptr(), ws.numel(), stream), 'gemm_bias_act')
    return y


def bottleneck_seam(y2, skip, w3, b3, w1, b1):
    """The seam between two bottleneck blocks as one HIP pass (csrc/seam.hpp): -> (out, z) with
    out = relu(conv1x1(y2, w3) + b3 + skip) and z = relu(conv1x1(out, w1) + b1), both channels_last -- what two
    `gemm_bias_act` calls compute, without reading `out` back.  y2 [B, 64, H, W] and skip [B, 256, H, W] channels_last, bfloat16 or
    float16; w3 [256, 64(, 1, 1)], w1 [64 | 128, 256(, 1, 1)] of that dtype; b3, b1 float32.  Other shapes raise."""
    if not y2.is_cuda or y2.dim() != 4 or y2.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError('bottleneck_seam: y2 must be a 4-d CUDA tensor of bfloat16/float16')
    b, k, h, w = y2.shape
    c, n = w3.shape[0], w1.shape[0]
    for name, wt, rows, cols in (('w3', w3, c, k), ('w1', w1, n, c)):
        if wt.numel() != rows * cols or wt.shape[1] != cols or wt.dtype != y2.dtype or wt.device != y2.device or not (
                wt.is_contiguous() or wt.is_contiguous(memory_format=torch.channels_last)):
            raise RuntimeError('bottleneck_seam: %s must be a dense [%d, %d(, 1, 1)] tensor of y2.dtype' % (name, rows, cols))
    if skip.shape != (b, c, h, w) or skip.dtype != y2.dtype or skip.device != y2.device or not _channels_last(skip, True) \
            or not _channels_last(y2, True):
        raise RuntimeError('bottleneck_seam: y2 and skip must be channels_last, skip [B, %d, H, W] of y2.dtype' % c)
    if not _bias_vector(b3, c) or not _bias_vector(b1, n):
        raise RuntimeError('bottleneck_seam: b3 / b1 must be float32 CUDA vectors of length %d / %d' % (c, n))
    out = torch.empty((b, c, h, w), dtype=y2.dtype, device=y2.device, memory_format=torch.channels_last)
    z = torch.empty((b, n, h, w), dtype=y2.dtype, device=y2.device, memory_format=torch.channels_last)
    _launch(library().odtk_bottleneck_seam, 'bottleneck_seam', y2.device, out.data_ptr(), z.data_ptr(), y2.data_ptr(), skip.data_ptr(),
            w3.data_ptr(), b3.data_ptr(), w1.data_ptr(), b1.data_ptr(), b * h * w, k, c, n, _DTYPES[y2.dtype])
    _count('bottleneck_seam_kernel', (y2.numel() + skip.numel() + out.numel() + z.numel()) * y2.element_size())
    return out, z


def tower_conv3x3(x, weight, bias, relu=True):
    """act(conv2d(x, weight, padding=1) + bias) of a channels_last bf16 / fp16 activation by the library's own implicit-GEMM MFMA
    kernel (csrc/tower_conv.hpp; include/odtk_hip.h: odtk_tower_conv3x3): the head towers' 3x3, stride 1, 256 -> 256 convolutions.
    x [B, 256, H, W] channels_last, weight [256, 256, 3, 3] channels_last, bias [256] of x.dtype.  Anything else raises."""
    if not x.is_cuda or x.dim() != 4 or x.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError('tower_conv3x3: x must be a 4-d CUDA tensor of bfloat16/float16')
    b, c, h, w = x.shape
    n = weight.shape[0]
    if (weight.dim() != 4 or tuple(weight.shape[1:]) != (c, 3, 3) or weight.dtype != x.dtype or weight.device != x.device
            or not weight.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError('tower_conv3x3: weight must be a channels_last [Cout, %d, 3, 3] tensor of x.dtype' % c)
    if not x.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError('tower_conv3x3: x must be channels_last')
    if bias.dtype != x.dtype or bias.numel() != n or bias.device != x.device or not bias.is_contiguous():
        raise RuntimeError('tower_conv3x3: bias must be a dense vector of length Cout of x.dtype')
    y = torch.empty((b, n, h, w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    if y.numel() == 0:
        return y
    _launch(library().odtk_tower_conv3x3, 'tower_conv3x3', x.device, y.data_ptr(), x.data_ptr(), weight.data_ptr(), bias.data_ptr(),
            b, h, w, c, n, _DTYPES[x.dtype], 1 if relu else 0)
    _count('tower_conv3x3_kernel', (x.numel() + y.numel()) * x.element_size())
    return y


# ---- libodtk_conv.so: k x k convolution with the bias + ReLU in its own epilogue (csrc/conv_ck.cpp) -----------------------------
_CONV_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libodtk_conv.so')
_conv_lib = []


def conv_library():
    """The loaded libodtk_conv.so, or None when it has not been built (the engine then keeps convolution + odtk_bias_act)."""
    if not _conv_lib:
        lib = None
        if os.path.isfile(_CONV_LIB_PATH) and not os.environ.get('ODTK_NO_CONV_LIBRARY'):
            lib = ctypes.CDLL(_CONV_LIB_PATH)
            lib.odtk_conv_bias_act.restype = ctypes.c_int
            lib.odtk_conv_bias_act.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 13 + [ctypes.c_void_p]
            lib.odtk_conv_bias_act_pads.restype = ctypes.c_int
            lib.odtk_conv_bias_act_pads.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 15 + [ctypes.c_void_p]
            lib.odtk_conv_bias_act_strided.restype = ctypes.c_int
            lib.odtk_conv_bias_act_strided.argtypes = ([ctypes.c_void_p] * 4 + [ctypes.c_int] * 13 + [ctypes.c_longlong] * 6 +
                                                       [ctypes.c_int] * 2 + [ctypes.c_void_p])
            lib.odtk_conv_last_plan.restype = ctypes.c_char_p
            lib.odtk_conv_last_plan.argtypes = []
            lib.odtk_conv_instance_count.restype = ctypes.c_int
            lib.odtk_conv_instance_count.argtypes = [ctypes.c_int]
            lib.odtk_conv_plan_export.restype = ctypes.c_size_t
            lib.odtk_conv_plan_export.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
            lib.odtk_conv_plan_import.restype = ctypes.c_int
            lib.odtk_conv_plan_import.argtypes = [ctypes.c_char_p]
        _conv_lib.append(lib)
    return _conv_lib[0]


def conv_available():
    return conv_library() is not None


def conv_bias_act(x, weight, bias, stride=(1, 1), padding=(1, 1), relu=True, out=None):
    """act(conv2d(x, weight) + bias) of a channels_last bf16 / fp16 activation in ONE launch: a composable_kernel implicit-GEMM
    convolution with the bias and the ReLU in its epilogue (include/odtk_conv.h: odtk_conv_bias_act).  x [B, Cin, H, W]
    channels_last, weight [Cout, Cin, kh, kw] channels_last (= K, Y, X, C in memory), bias [Cout] of x.dtype.  The first call
    for a problem times the library's instances on the current stream (one synchronisation each); later calls only enqueue.
    Raises RuntimeError (ODTK_ERR_UNSUPPORTED) when no instance takes the problem."""
    lib = conv_library()
    if lib is None:
        raise ImportError('odtk._C: %s is missing -- build it (python __graft_entry__.py, or make -C retinanet-examples_amd/csrc conv)'
                          % _CONV_LIB_PATH)
    if not x.is_cuda or x.dim() != 4 or x.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError('conv_bias_act: x must be a 4-d CUDA tensor of bfloat16/float16')
    b, c, h, w = x.shape
    k, c2, kh, kw = weight.shape
    if c2 != c or weight.dtype != x.dtype or not weight.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError('conv_bias_act: weight must be [Cout, Cin, kh, kw] of x.dtype, channels_last')
    if bias.dtype != x.dtype or bias.numel() != k or not bias.is_cuda or not bias.is_contiguous():
        raise RuntimeError('conv_bias_act: bias must be a CUDA vector of length Cout in the dtype of x')
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    # padding (before, after) per dimension: ((top, bottom), (left, right)) -- the space-to-depth stem needs (2, 1)
    (ph0, ph1), (pw0, pw1) = [(p, p) if isinstance(p, int) else p for p in (ph, pw)]
    ho, wo = (h + ph0 + ph1 - kh) // sh + 1, (w + pw0 + pw1 - kw) // sw + 1
    if out is None:
        y = torch.empty((b, k, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    else:                                                    # caller-owned output
        if tuple(out.shape) != (b, k, ho, wo) or out.dtype != x.dtype or out.device != x.device:
            raise RuntimeError('conv_bias_act: out must be a channels_last %s tensor of shape %s' % (x.dtype, (b, k, ho, wo)))
        y = out
    # channels_last tensors, or views of larger ones (a rectangle of the engine's pyramid canvas, a channel slice): the channel
    # stride is 1 and the library takes the other three (include/odtk_conv_strided.h -- it says which views it refuses)
    views = []
    for t, name in ((x, 'x'), (y, 'out')):
        sn, sc, srow, spix = t.stride()
        if t.shape[1] != 1 and sc != 1:
            raise RuntimeError('conv_bias_act: %s must be channels_last (or a view of a channels_last tensor)' % name)
        ch, hh, ww = t.shape[1], t.shape[2], t.shape[3]
        # (torch reports arbitrary strides for dimensions of size 1: take the packed ones there)
        spix = spix if ww > 1 else ch
        srow = srow if hh > 1 else ww * spix
        sn = sn if t.shape[0] > 1 else hh * srow
        views += [sn, srow, spix]
    _launch(lib.odtk_conv_bias_act_strided, 'conv_bias_act', x.device, y.data_ptr(), x.data_ptr(), weight.data_ptr(), bias.data_ptr(),
            b, c, h, w, k, kh, kw, sh, sw, ph0, pw0, ph1, pw1, *views, _DTYPES[x.dtype], 1 if relu else 0)
    return y


def conv_last_plan():
    """'#index time name' of the instance the last conv_bias_act call of this thread ran (measurement records)."""
    lib = conv_library()
    return lib.odtk_conv_last_plan().decode() if lib is not None else ''


def _export_text(fn):
    need = fn(None, 0)
    buf = ctypes.create_string_buffer(int(need))
    fn(buf, need)
    return buf.value.decode()


def library_plans_export():
    """The choices the two kernel libraries under the engine made by stopwatch in this process, as text lines: hipBLASLt
    solutions ('gemm ...', include/odtk_hip.h: odtk_gemm_plan_export) and convolution instances ('conv ...', include/odtk_conv.h:
    odtk_conv_plan_export)."""
    text = _export_text(library().odtk_gemm_plan_export)
    lib = conv_library()
    if lib is not None:
        text += _export_text(lib.odtk_conv_plan_export)
    return text


def library_plans_import(text):
    """-> (gemm lines taken, conv lines taken): problems not yet planned in this process run on the named solution / instance
    without being timed."""
    data = text.encode()
    gemm_available()                                          # (binds hipBLASLt: the import itself only records)
    n_gemm = library().odtk_gemm_plan_import(data)
    lib = conv_library()
    return n_gemm, (lib.odtk_conv_plan_import(data) if lib is not None else 0)


def gemm_plan_pin_misses():
    return library().odtk_gemm_plan_pin_misses()


GEMM_ORIGINS = ('timed', 'pinned', 'capture')          # include/odtk_hip.h: ODTK_GEMM_ORIGIN_*


def gemm_candidates(m, n, k, dtype, relu, residual, workspace_size=32 << 20):
    """Debug: the hipBLASLt solution indices a plan for the problem chooses from, in heuristic order (host only, nothing is
    launched).  `dtype` is a torch dtype; the default workspace is the 32 MiB `gemm_bias_act` passes."""
    if not gemm_available():
        raise RuntimeError('gemm_candidates: hipBLASLt could not be bound (odtk_gemm_init failed)')
    out = (ctypes.c_int * 16)()
    n_found = _check(library().odtk_debug_gemm_candidates(m, n, k, _DTYPES[dtype], 1 if relu else 0, 1 if residual else 0,
                                                          workspace_size, out, 16), 'gemm_candidates')
    return list(out[:min(n_found, 16)])


def gemm_plan_clear():
    """Debug: forget every cached GEMM plan, every imported `gemm` line and the miss count."""
    library().odtk_gemm_plan_clear()


def gemm_last_solution():
    """-> (solution index of the most recent gemm_bias_act of the process, or -1; 'timed' | 'pinned' | 'capture')."""
    origin = ctypes.c_int(0)
    index = library().odtk_gemm_last_solution(ctypes.byref(origin))
    return index, GEMM_ORIGINS[origin.value]


def loss_tuning(which, fp32_heads, threads, blocks_per_cu, unroll, box_blocks):
    """Debug / tuning: launch shape of the loss kernels of one form (0 forward with atomics, 1 backward, 2 forward through a
    workspace) and head width (include/odtk_hip.h: odtk_debug_loss_tuning)."""
    _check(library().odtk_debug_loss_tuning(int(which), int(bool(fp32_heads)), int(threads), int(blocks_per_cu),
                                            int(unroll), int(box_blocks)), 'loss_tuning')


def loss_layout(which, fp32_heads, per_wave=0, window=0, box_rows=1):
    """Debug / A-B: per-wave partial sums (workspace form only), contiguous trips of the loss kernels' logit walk, the backward's
    box-delta walk in memory order (include/odtk_hip.h: odtk_debug_loss_layout)."""
    _check(library().odtk_debug_loss_layout(int(which), int(bool(fp32_heads)), int(bool(per_wave)), int(bool(window)),
                                            int(bool(box_rows))), 'loss_layout')


LOSS_TUNING_FIELDS = ('threads', 'blocks_per_cu', 'unroll', 'box_blocks', 'per_wave', 'window', 'box_rows')


def loss_tuning_state(which, fp32_heads):
    """What loss_tuning / loss_layout hold for one form and head width, as a dict over LOSS_TUNING_FIELDS (include/odtk_hip.h:
    odtk_debug_loss_tuning_get); the shipped defaults until a setter ran.  Never touches the GPU."""
    out = (ctypes.c_int * 7)()
    _check(library().odtk_debug_loss_tuning_get(int(which), int(bool(fp32_heads)), out), 'loss_tuning_state')
    return dict(zip(LOSS_TUNING_FIELDS, out))


def loss_tuning_restore(which, fp32_heads, state):
    """Puts back what loss_tuning_state returned."""
    loss_tuning(which, fp32_heads, state['threads'], state['blocks_per_cu'], state['unroll'], state['box_blocks'])
    loss_layout(which, fp32_heads, state['per_wave'], state['window'], state['box_rows'])


def loss_form_state():
    """The arithmetic form loss_form last set (include/odtk_hip.h: odtk_debug_loss_form_get)."""
    return library().odtk_debug_loss_form_get()


LOSS_FORM_DEFAULT = 1      # = ODTK_LOSS_FORM_DEFAULT of include/odtk_hip.h (tests/test_abi_host.py compares the two)


def loss_form(form):
    """Debug / A-B: 0 = the symmetric element form everywhere, 1 (default) = vectors of negatives through the negatives-only
    form; 2..4 = timing ablations with wrong sums (include/odtk_hip.h: odtk_debug_loss_form)."""
    _check(library().odtk_debug_loss_form(int(form)), 'loss_form')


def _dense(t):
    """No gaps and no overlap: contiguous in the default or a channels_last order (what parameters and their gradients are)."""
    return (t.numel() == 0 or t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)) or
            (t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d)))


def optim_tensors(params, grads, momenta, emas=None):
    """The descriptor groups of odtk_optim_sgd_step / odtk_optim_grad_norm for lists of float32 CUDA tensors (`emas`: None, or a
    list whose entries may be None): [(OptimTensor array, count)] of at most MAX_OPTIM_TENSORS entries each.  The tensors must be
    dense (any memory format: the step is elementwise, and the four of a parameter share their strides)."""
    groups = []
    for first in range(0, len(params), MAX_OPTIM_TENSORS):
        count = min(MAX_OPTIM_TENSORS, len(params) - first)
        table = (OptimTensor * count)()
        for i in range(count):
            p, g, m = params[first + i], grads[first + i], momenta[first + i]
            e = emas[first + i] if emas is not None else None
            for t, name in ((p, 'param'), (g, 'grad'), (m, 'momentum'), (e, 'ema')):
                if t is None and name == 'ema':
                    continue
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.device == p.device):
                    raise RuntimeError('optim_tensors: %s must be a float32 CUDA tensor on the parameter\'s device' % name)
                if t.numel() != p.numel() or t.stride() != p.stride() or not _dense(t):
                    raise RuntimeError('optim_tensors: %s must be dense and share the parameter\'s shape and strides' % name)
            table[i] = OptimTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), e.data_ptr() if e is not None else None, p.numel())
        groups.append((table, count))
    return groups


OPTIM_STATE_FLOATS = 4      # the device state of odtk_optim_grad_norm: float32 norm, float32 coef, uint32 skip, uint32 0


def optim_grad_norm(groups, grad_scale, max_norm, state):
    """Global L2 norm of the (unscaled) gradients of `groups` (optim_tensors) -> `state` (float32 CUDA tensor of OPTIM_STATE_FLOATS
    elements: norm, coef, the skip word, 0), enqueued: one launch per group + one (include/odtk_hip.h: odtk_optim_grad_norm_chained).
    `grad_scale`: None or a float32 CUDA scalar."""
    if not (state.is_cuda and state.dtype == torch.float32 and state.is_contiguous() and state.numel() >= OPTIM_STATE_FLOATS):
        raise RuntimeError('optim_grad_norm: state must be a contiguous float32 CUDA tensor of %d elements' % OPTIM_STATE_FLOATS)
    lib, device = library(), state.device
    scale = _optim_scalar(grad_scale, device, 'grad_scale')
    # the slots the calls before group k filled: one per started chunk of each of their tensors
    prior = [0]
    for table, _ in groups:
        prior.append(prior[-1] + sum((int(t.numel) + OPTIM_CHUNK - 1) // OPTIM_CHUNK for t in table))
    with torch.cuda.device(device):
        table, count = groups[-1]                                   # the last call's query covers every slot of the chain
        size = _check(lib.odtk_optim_grad_norm_chained(count, table, scale, float(max_norm), state.data_ptr(), prior[-2], 1, None, 0, None),
                      'optim_grad_norm (workspace query)')
        ws, stream = _workspace(device, size)
        for k, (table, count) in enumerate(groups):
            _check(lib.odtk_optim_grad_norm_chained(count, table, scale, float(max_norm), state.data_ptr(), prior[k], int(k == len(groups) - 1),
                                                    ws.data_ptr(), ws.numel(), stream), 'optim_grad_norm')


def _optim_scalar(t, device, name):
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == device and t.dtype == torch.float32 and t.numel() == 1):
        raise RuntimeError('%s must be a float32 CUDA scalar on the parameters\' device' % name)
    return t.data_ptr()


def optim_sgd_step(groups, lr, momentum, weight_decay, first, one_minus_decay, grad_scale=None, found_inf=None, norm_state=None, device=None):
    """The fused SGD step over `groups` (optim_tensors), enqueued: one launch per group (include/odtk_hip.h: odtk_optim_sgd_step).
    `grad_scale`, `found_inf`: None or float32 CUDA scalars (torch.amp.GradScaler's); `norm_state`: None or what optim_grad_norm
    wrote.  Nothing is read back."""
    lib = library()
    args = [_optim_scalar(grad_scale, device, 'grad_scale'), _optim_scalar(found_inf, device, 'found_inf'),
            norm_state.data_ptr() if norm_state is not None else None]
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        for table, count in groups:
            _check(lib.odtk_optim_sgd_step(count, table, float(lr), float(momentum), float(weight_decay), int(bool(first)), float(one_minus_decay),
                                           *args, stream), 'optim_sgd_step')


TRACE_WORDS = 16384     # odtk_debug_set_trace: >= 128 KiB (include/odtk_hip.h): coarse stamps in the first 8192 words, select_decode's
                        # per-segment fine stamps (16 words per segment, up to 512 segments) in the second 8192


def debug_set_trace(trace):
    """Debug trace buffer of the select_decode / nms kernels (include/odtk_hip.h: odtk_debug_set_trace), or None to switch it
    off.  `trace`: a zero-filled int64 CUDA tensor of at least TRACE_WORDS elements -- checked HERE because the library cannot:
    a 64 KiB buffer (the size of round 3's trace) is overrun by select_decode's fine stamps, which corrupts whatever the
    allocator placed behind it or faults (round 6, call 12: "Memory access fault by GPU" at the end of an 18-minute run)."""
    if trace is None:
        return library().odtk_debug_set_trace(None)
    if not (trace.is_cuda and trace.dtype == torch.int64 and trace.is_contiguous() and trace.numel() >= TRACE_WORDS):
        raise ValueError('the trace buffer must be a contiguous int64 CUDA tensor of >= %d elements (128 KiB)' % TRACE_WORDS)
    return library().odtk_debug_set_trace(trace.data_ptr())


def profile_enable(on=True, kernels=None):
    """Bracket kernel launches of the library with hipEvent pairs on their launch stream.
    kernels: iterable of names from KERNEL_NAMES (default: all)."""
    if not on:
        mask = 0
    elif kernels is None:
        mask = -1
    else:
        mask = 0
        for k in kernels:
            mask |= 1 << KERNEL_NAMES.index(k)
    _check(library().odtk_profile_enable(mask), 'profile_enable')


def profile_collect():
    """{kernel name: (total ms, launches)} since the last collect (waits for the recorded events)."""
    ms = (ctypes.c_double * len(KERNEL_NAMES))()
    n = (ctypes.c_int * len(KERNEL_NAMES))()
    _check(library().odtk_profile_collect(ms, n), 'profile_collect')
    return {name: (ms[i], n[i]) for i, name in enumerate(KERNEL_NAMES)}


class Engine:
    """Placeholder for the reference's TensorRT engine class (csrc/engine.h): the TensorRT / DALI /
    DeepStream deployment path is out of scope on MI355X (BASELINE.json north_star)."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError('odtk._C.Engine: the TensorRT engine path is not available on MI355X')

    @staticmethod
    def load(path):
        raise NotImplementedError('odtk._C.Engine.load: the TensorRT engine path is not available on MI355X')
