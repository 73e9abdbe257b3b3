"""RetinaNet (https://arxiv.org/abs/1708.02002) on MI355X.

Public surface = the reference's `odtk.model.Model` (constructor arguments, `initialize`, `forward`
in train / eval mode, `save` / `load` with the same checkpoint keys, reference odtk/model.py), so
training scripts and checkpoints carry over.  What runs where:

  backbone + FPN + the two 5-conv heads + losses   stock PyTorch-ROCm modules (MIOpen owns the MFMA work)
  eval forward on a GPU (the default)               the BN-folded inference engine (odtk/fused.py: folded
                                                    weights, HIP bias/skip/ReLU epilogues, 1x1 convs as
                                                    fused GEMMs) + `odtk.box.detect`: sigmoid + decode of all
                                                    five levels + batched NMS, hand-written HIP, six launches,
                                                    no host sync, head tensors read in place.  Built lazily
                                                    from the current weights, rebuilt when they change.
  `fused_graph = False`                             the eager nn.Module graph (what training uses) + the same
                                                    fused post-processing
  `fused_postprocess = False`                       the reference's own op sequence (model.py:140-165)
                                                    on the same kernels, for A/B checks
  CPU tensors                                       eager graph + the pure-torch decode / nms branch of
                                                    odtk/box.py (BASELINE config 0: no GPU needed)
"""
import math
import os.path

import numpy as np
import torch
import torch.nn as nn

from . import backbones as backbones_mod
from . import box as box_ops
from .loss import (BOX_LOSS_KINDS, CLS_LOSS_KINDS, ROTATED_BOX_LOSS_KINDS, FocalLoss, SmoothL1Loss, anchor_wh, box_iou_loss, box_quality,
                   fused_pyramid_box_iou_loss, fused_pyramid_loss, fused_pyramid_quality_loss, fused_pyramid_rotated_box_loss,
                   quality_focal_loss, quality_target, rotated_box_loss, varifocal_loss)

DEFAULT_RATIOS = [1.0, 2.0, 0.5]
DEFAULT_SCALES = [4 * 2 ** (i / 3) for i in range(3)]
DEFAULT_ANGLES = [-np.pi / 6, 0, np.pi / 6]
CLASS_PRIOR = 0.01                       # initial foreground probability of every anchor


def conv_tower(out_channels, width=256, depth=4):
    """`depth` x (3x3 conv + ReLU) followed by the 3x3 output conv; shared by all pyramid levels.
    nn.Sequential indices (0, 2, 4, 6, 8 are convs) are part of the checkpoint format."""
    layers = []
    for _ in range(depth):
        layers.extend([nn.Conv2d(width, width, 3, padding=1), nn.ReLU()])
    layers.append(nn.Conv2d(width, out_channels, 3, padding=1))
    return nn.Sequential(*layers)


def _init_tower(tower):
    for layer in tower:
        if isinstance(layer, nn.Conv2d):
            nn.init.normal_(layer.weight, std=0.01)
            nn.init.zeros_(layer.bias)


def _init_prior(conv):
    nn.init.normal_(conv.weight, std=0.01)
    nn.init.constant_(conv.bias, -math.log((1 - CLASS_PRIOR) / CLASS_PRIOR))


class Model(nn.Module):
    CHECKPOINT_EXTRAS = ('iteration', 'optimizer', 'scheduler', 'ema')   # 'ema': ModelEMA.state_dict() (odtk/optim.py); 'state_dict' stays the raw weights

    def __init__(self, backbones='ResNet50FPN', classes=80, ratios=DEFAULT_RATIOS, scales=DEFAULT_SCALES,
                 angles=None, rotated_bbox=False, anchor_ious=[0.4, 0.5], config={}):
        super().__init__()
        names = backbones if isinstance(backbones, list) else [backbones]
        self.backbones = nn.ModuleDict({n: getattr(backbones_mod, n)() for n in names})
        self.name = 'RetinaNet'
        self.unused_modules = [u for n in names for u in self.backbones[n].features.unused_modules]
        self.stride = max(b.stride for b in self.backbones.values())

        self.classes = classes
        self.ratios, self.scales = ratios, scales
        self.rotated_bbox = rotated_bbox
        self.angles = angles if angles is not None else (DEFAULT_ANGLES if rotated_bbox else None)
        self.anchor_ious = anchor_ious
        self.anchors = {}                                   # stride -> base anchors, filled lazily

        # post-processing hyper-parameters are config entries, not CLI flags (reference model.py:49-52)
        self.threshold = config.get('threshold', 0.05)
        self.top_n = config.get('top_n', 1000)
        self.nms = config.get('nms', 0.5)
        self.detections = config.get('detections', 100)
        # Soft-NMS instead of the reference's hard rule (odtk/box.py:soft_nms): None, or a dict with `method` ('linear' /
        # 'gaussian'), `sigma` and `min_score` (default: `threshold`).  A run-time option: never written into checkpoints
        self.soft_nms = None
        # Matrix NMS instead (odtk/box.py:matrix_nms; not together with `soft_nms`): None, or a dict with `method` ('linear' /
        # 'gaussian', default 'gaussian'), `sigma`, `min_score` (default: `threshold`) and `pre_top` (default 2000).  It takes a
        # candidate list of any length.  A run-time option as well: never written into checkpoints
        self.matrix_nms = None
        # two more run-time options of inference, like `soft_nms` never constructor arguments and never written into checkpoints:
        # box voting behind the suppression (odtk/box.py:box_vote) -- None, or its IoU threshold in (0, 1] -- and test-time
        # augmentation -- None, or 'flip': the network also runs on the mirrored batch and one suppression sees both candidate lists
        self.box_voting = None
        self.tta = None
        # tiled inference of large images, one more run-time option of this kind: None, or a dict with `size` (th, tw) -- multiples
        # of the model's stride --, `overlap` (default a quarter of the size), `border` (default 0: the cut rule of
        # odtk/box.py:merge_tile_candidates is off) and `batch`, the tiles per pass of the network (default 8).  The image is cut
        # into overlapping tiles of that one size, the network runs on chunks of `batch` tiles, one suppression sees all candidates
        self.tile = None
        # how ground truth becomes training targets: 'iou' (the reference's fixed thresholds, `anchor_ious`) or 'atss' (adaptive
        # training sample selection over the `atss_topk` nearest cells per level, odtk/box.py:atss_assign_levels; axis-aligned
        # boxes only), or 'tal' (task-aligned assignment: per box the `tal_topk` candidate anchors with the largest
        # score^`tal_alpha` * IoU^`tal_beta` of what the network predicts there, odtk/box.py:tal_assign_levels; axis-aligned boxes
        # only).  Run-time options like `soft_nms`: not constructor arguments, never written into checkpoints
        self.assigner = 'iou'
        self.atss_topk = 9
        self.tal_topk, self.tal_alpha, self.tal_beta = 13, 1, 6
        # what the box regression is trained with: 'smooth_l1' (the reference's loss on the four deltas) or 'iou' | 'giou' | 'diou' on
        # the boxes the deltas decode to (odtk/loss.py:box_iou_loss, csrc/box_iou_loss.hpp; axis-aligned boxes only), or 'probiou' |
        # 'kld' on the Gaussians of the rotated boxes the six deltas decode to (odtk/loss.py:rotated_box_loss,
        # csrc/rotated_box_loss.hpp; `rotated_bbox` models only), times `box_loss_weight` (every kind but 'smooth_l1').  Run-time
        # options like `assigner`: never written into checkpoints
        self.box_loss = 'smooth_l1'
        self.box_loss_weight = 1.0
        # what the class scores are trained with: 'focal' (the reference's loss on a one-hot target) or 'qfl' | 'vfl', the quality
        # focal and varifocal losses on a soft target -- at a foreground anchor the IoU of the predicted and the assigned box
        # (odtk/loss.py:quality_focal_loss / varifocal_loss, csrc/quality_loss.hpp; axis-aligned boxes only).  A run-time option like
        # `box_loss`: never written into checkpoints
        self.cls_loss = 'focal'
        self.exporting = False
        self.fused_postprocess = True
        self.fused_graph = True                             # eval on a GPU runs the BN-folded engine (odtk/fused.py)
        self.fused_loss = True                              # training on a GPU: HIP focal / smooth-L1 reduction (csrc/loss.hpp)
        self.__dict__['_engine_cache'] = {}                 # (not a submodule: keeps state_dict / checkpoints unchanged)

        self.num_anchors = len(ratios) * len(scales) * (len(self.angles) if rotated_bbox else 1)
        box_params = 6 if rotated_bbox else 4               # rotated: (dx, dy, dw, dh, sin, cos)
        self.cls_head = conv_tower(classes * self.num_anchors)
        self.box_head = conv_tower(box_params * self.num_anchors)
        self.cls_criterion = FocalLoss()
        self.box_criterion = SmoothL1Loss(beta=0.11)

    def __repr__(self):
        return '\n'.join(['     model: {}'.format(self.name),
                          '  backbone: {}'.format(', '.join(self.backbones.keys())),
                          '   classes: {}, anchors: {}'.format(self.classes, self.num_anchors)])

    # ------------------------------------------------------------------ weights
    def initialize(self, pre_trained=None):
        """Fresh initialisation, or fine-tuning from a checkpoint whose last classification (and, for
        rotated boxes, regression) layer is re-initialised (reference model.py:80-123)."""
        if pre_trained:
            if not os.path.isfile(pre_trained):
                raise ValueError('No checkpoint {}'.format(pre_trained))
            print('Fine-tuning weights from {}...'.format(os.path.basename(pre_trained)))
            donor = torch.load(pre_trained, map_location='cpu')['state_dict']
            dropped = ['cls_head.8.'] + (['box_head.8.'] if self.rotated_bbox else [])
            state = self.state_dict()
            state.update({k: v for k, v in donor.items() if not any(k.startswith(d) for d in dropped)})
            self.load_state_dict(state)
        else:
            for backbone in self.backbones.values():
                backbone.initialize()
            _init_tower(self.cls_head)
            _init_tower(self.box_head)
        _init_prior(self.cls_head[-1])
        if self.rotated_bbox:
            _init_prior(self.box_head[-1])

    def freeze_unused_params(self):
        for name, param in self.named_parameters():
            if any(u in name for u in self.unused_modules):
                param.requires_grad = False

    def save(self, state):
        checkpoint = {'backbone': list(self.backbones.keys()), 'classes': self.classes, 'ratios': self.ratios,
                      'scales': self.scales, 'state_dict': self.state_dict()}
        if self.rotated_bbox and self.angles:
            checkpoint['angles'] = self.angles
        checkpoint.update({k: state[k] for k in self.CHECKPOINT_EXTRAS if k in state})
        torch.save(checkpoint, state['path'])

    @classmethod
    def load(cls, filename, rotated_bbox=False):
        if not os.path.isfile(filename):
            raise ValueError('No checkpoint {}'.format(filename))
        checkpoint = torch.load(filename, map_location='cpu')
        kwargs = {k: checkpoint[k] for k in ('ratios', 'scales', 'angles') if k in checkpoint}
        if rotated_bbox or 'angles' in checkpoint:
            kwargs['rotated_bbox'] = True
        model = cls(backbones=checkpoint['backbone'], classes=checkpoint['classes'], **kwargs)
        model.load_state_dict(checkpoint['state_dict'])
        return model, {k: checkpoint[k] for k in cls.CHECKPOINT_EXTRAS if k in checkpoint}

    def export(self, *args, **kwargs):
        raise NotImplementedError('TensorRT export is not available on MI355X (the DALI / TensorRT / DeepStream '
                                  'paths are dropped, BASELINE.json north_star)')

    def fuse(self, dtype=torch.bfloat16):
        """Inference engine with BN folded into the convolutions and the HIP epilogue (odtk/fused.py)."""
        from .fused import FusedRetinaNet
        return FusedRetinaNet(self, dtype)

    def _apply(self, fn, *args, **kwargs):
        self.__dict__['_engine_cache'].clear()              # .to() / .cuda() / .float(): new storages
        return super()._apply(fn, *args, **kwargs)

    def train(self, mode=True):
        self.__dict__['_engine_rescan'] = True              # next eval call re-reads WHICH tensors the model is made of
        return super().train(mode)

    def invalidate_engine(self):
        """Drop the cached inference engine (and its hipGraphs).  Needed after weight changes the cache cannot see: writes
        through `.data` (`p.data.copy_()`, EMA swaps -- a separate version counter) between two eval calls."""
        self.__dict__['_engine_cache'].clear()

    def inference_engine(self, dtype):
        """The cached BN-folded engine for `dtype`; None when this model has no fused form (several
        backbones, exotic blocks).  The engine is a SNAPSHOT of the weights, so it remembers the tensors it
        was folded from together with their version counters and storage addresses, and is rebuilt when
        any of them moved: optimizer steps and load_state_dict write in place (version bump), .to() /
        .cuda() swap storages (cache dropped in `_apply`)."""
        from .fused import FusedRetinaNet
        cache = self.__dict__['_engine_cache']
        hit = cache.get(dtype)
        if hit is not None:
            tensors, stamp, engine = hit
            if self.__dict__.pop('_engine_rescan', False):
                # after every train() / eval() switch: is the model still MADE OF the tensors the engine was folded from?
                # (a replaced submodule or Parameter keeps the old objects alive in `tensors`, version and address unchanged).
                # The module walk costs ~0.4 ms, so it is not repeated on every call; between two switches use invalidate_engine()
                current = list(self.parameters()) + list(self.buffers())
                if len(current) != len(tensors) or any(a is not b for a, b in zip(current, tensors)):
                    hit = None
            if hit is not None and [t._version for t in tensors] + [t.data_ptr() for t in tensors] == stamp:
                return engine
        if not FusedRetinaNet.supports(self):
            return None
        cache.clear()                                       # one engine at a time: it holds a copy of the weights
        tensors = list(self.parameters()) + list(self.buffers())
        engine = FusedRetinaNet(self, dtype)
        cache[dtype] = (tensors, [t._version for t in tensors] + [t.data_ptr() for t in tensors], engine)
        self.__dict__.pop('_engine_rescan', None)
        return engine

    # ------------------------------------------------------------------ forward
    def level_anchors(self, stride):
        if stride not in self.anchors:
            if self.rotated_bbox:
                self.anchors[stride] = box_ops.generate_anchors_rotated(stride, self.ratios, self.scales, self.angles)
            else:
                self.anchors[stride] = box_ops.generate_anchors(stride, self.ratios, self.scales)
        return self.anchors[stride]

    def heads(self, x):
        """Raw head tensors of every pyramid level: (cls logits x5, box deltas x5)."""
        pyramid = [feature for backbone in self.backbones.values() for feature in backbone(x)]
        return [self.cls_head(f) for f in pyramid], [self.box_head(f) for f in pyramid]

    def forward(self, x, rotated_bbox=None, graph=False):
        """Reference surface (model.py:131): training -> (cls_loss, box_loss) of (images, targets); eval -> (scores, boxes,
        classes).  graph=True (eval on a GPU, opt-in): the whole call -- engine + post-processing, ~300 launches -- is captured
        once per input geometry into ONE hipGraph and replayed (batch 1: launch-bound eager); the graph
        belongs to the engine and goes with it when the weights change."""
        if self.training:
            if graph:
                raise RuntimeError('Model.forward(graph=True) is an inference option (eval mode)')
            images, targets = x
            cls_heads, box_heads = self.heads(images)
            return self._compute_loss(images, cls_heads, box_heads, targets.float())

        if self.fused_graph and self.fused_postprocess and x.is_cuda and not self.exporting:
            # the default inference path: same function as the eager graph below up to the rounding of the
            # folded weights (tests/test_gpu_fused_model.py, tests/test_gpu_detection_parity.py)
            dtype = torch.get_autocast_dtype('cuda') if torch.is_autocast_enabled('cuda') else self.cls_head[0].weight.dtype
            engine = self.inference_engine(dtype)
            if engine is not None:
                if graph and self.tta is not None:
                    raise RuntimeError('Model.forward(graph=True) is not available with Model.tta (two passes of the engine)')
                if graph and self.tile is not None:
                    raise RuntimeError('Model.forward(graph=True) is not available with Model.tile (several passes of the engine)')
                return engine.replay(x) if graph else engine(x)
        if graph:
            raise RuntimeError('Model.forward(graph=True) needs the fused inference engine (eval mode, GPU tensors, a single '
                               'ResNet-FPN backbone)')

        if self.tile is not None and not self.exporting:
            return self.forward_tiled(x, self._tile_candidates)
        cls_heads, box_heads = self.heads(x)
        strides = [x.shape[-1] // c.shape[-1] for c in cls_heads]
        if self.exporting:
            self.strides = strides
            return [c.sigmoid() for c in cls_heads], box_heads
        for stride in strides:
            self.level_anchors(stride)
        if self.tta is not None:
            # the first pass is decoded before the second runs; one suppression over [pass 0 | mirrored pass mapped back]
            self.check_inference_options()
            first = self.candidates(cls_heads, box_heads, strides)
            del cls_heads, box_heads
            second = self.candidates(*self.heads(box_ops.flip_batch(x)), strides)
            return self.suppress_tta(first, second, x.shape[-1])
        return self.postprocess(cls_heads, box_heads, strides)

    def check_inference_options(self):
        """The run-time options `soft_nms`, `matrix_nms`, `box_voting`, `tta` and `tile` against the model (axis-aligned boxes only) and their
        domains."""
        if self.tta not in (None, 'flip'):
            raise ValueError("Model.tta must be None or 'flip', not {!r}".format(self.tta))
        for name, value in (('soft_nms', self.soft_nms), ('matrix_nms', self.matrix_nms), ('box_voting', self.box_voting), ('tta', self.tta), ('tile', self.tile)):
            if value is not None and self.rotated_bbox:
                raise ValueError('Model.{} is not available for rotated boxes'.format(name))
        if self.matrix_nms is not None:
            if self.soft_nms is not None:
                raise ValueError('Model.matrix_nms is not available together with Model.soft_nms')
            if not isinstance(self.matrix_nms, dict):
                raise ValueError("Model.matrix_nms must be None or a dict with 'method', 'sigma', 'min_score' and 'pre_top', not "
                                 '{!r}'.format(self.matrix_nms))
            box_ops._matrix_nms_dict(self.matrix_nms, self.threshold)
        if self.tile is not None:
            if self.tta is not None:
                raise ValueError('Model.tile is not available together with Model.tta')
            self.tile_options()

    def tile_options(self):
        """`Model.tile` checked and completed -> (size (th, tw), overlap (oy, ox), border, batch)."""
        tile = self.tile
        if not isinstance(tile, dict) or 'size' not in tile or set(tile) - {'size', 'overlap', 'border', 'batch'}:
            raise ValueError("Model.tile must be None or a dict with 'size' and optionally 'overlap', 'border' and 'batch', not "
                             '{!r}'.format(tile))
        size = box_ops._pair_of_ints(tile['size'], 'Model.tile: size')
        if min(size) < 1 or any(v % self.stride for v in size):
            raise ValueError("Model.tile: the size must be a positive multiple of the model's stride {}, not {}".format(self.stride, size))
        overlap = box_ops._pair_of_ints(tile['overlap'], 'Model.tile: overlap') if tile.get('overlap') is not None \
            else (size[0] // 4, size[1] // 4)
        if any(not 0 <= o < v for o, v in zip(overlap, size)):
            raise ValueError('Model.tile: the overlap must be in [0, size), not {} for size {}'.format(overlap, size))
        border = float(tile.get('border', 0) or 0)
        if not (math.isfinite(border) and border >= 0):
            raise ValueError('Model.tile: the border must be finite and not negative, not {!r}'.format(tile.get('border')))
        batch = tile.get('batch', 8)
        if int(batch) != batch or not 1 <= batch <= box_ops.MAX_TILES:
            raise ValueError('Model.tile: batch (tiles per pass of the network) must be in 1..{}, not {!r}'.format(box_ops.MAX_TILES, batch))
        return size, overlap, border, int(batch)

    def _tile_candidates(self, tiles):
        """One pass of the eager network on a batch of tiles -> their candidate list."""
        cls_heads, box_heads = self.heads(tiles)
        strides = [tiles.shape[-1] // c.shape[-1] for c in cls_heads]
        for stride in strides:
            self.level_anchors(stride)
        return self.candidates(cls_heads, box_heads, strides)

    def forward_tiled(self, x, candidates_of):
        """Tiled inference (`Model.tile`): the grid of x.shape[-2:], the tiles image-major in chunks of `batch` (the last chunk
        padded with zero tiles, so the network sees one shape only), per chunk the tiler, one pass of the network and its decode
        (`candidates_of`: tiles -> candidate list; a chunk is decoded before the next pass runs), the merge into the lists
        [B, T * L * top_n] of the whole images, and one suppression over them."""
        self.check_inference_options()
        size, overlap, border, chunk = self.tile_options()
        batch, height, width = x.shape[0], x.shape[-2], x.shape[-1]
        grid = box_ops.tile_grid(height, width, size, overlap)
        entries = [(image, slot, y, left) for image in range(batch) for slot, (y, left) in enumerate(grid)]
        merged = None
        for first in range(0, len(entries), chunk):
            part = entries[first:first + chunk]
            part = part + [(-1, 0, 0, 0)] * (chunk - len(part))
            found = candidates_of(box_ops.tile_images(x, part, size))
            if merged is None:
                count = found[0].shape[1]
                if self.soft_nms is not None and len(grid) * count > box_ops.MAX_SOFT_NMS_COUNT:
                    raise ValueError('Model.tile with Model.soft_nms: the merged list has {} candidates per image ({} tiles), Soft-NMS '
                                     'takes {}: lower top_n'.format(len(grid) * count, len(grid), box_ops.MAX_SOFT_NMS_COUNT))
                merged = [found[0].new_empty((batch, len(grid) * count), dtype=torch.float32),
                          found[0].new_empty((batch, len(grid) * count, 4), dtype=torch.float32),
                          found[0].new_empty((batch, len(grid) * count), dtype=torch.float32)]
            box_ops.merge_tile_candidates(found, part, batch, len(grid), size, (height, width), border, out=merged)
        return box_ops.suppress(*merged, self.nms, self.detections, soft_nms=self.soft_nms, vote=self.box_voting,
                                threshold=self.threshold, matrix_nms=self.matrix_nms)

    def candidates(self, cls_heads, box_heads, strides):
        """Raw head tensors of axis-aligned boxes -> one candidate list (scores [B, L * top_n], boxes [.., 4], classes)."""
        if self.fused_postprocess and cls_heads[0].is_cuda:
            return box_ops.candidates(cls_heads, box_heads, strides, self.anchors, self.threshold, self.top_n, logits=True)
        per_level = [box_ops.decode(c.sigmoid().contiguous(), b.contiguous(), s, self.threshold, self.top_n, self.anchors[s])
                     for c, b, s in zip(cls_heads, box_heads, strides)]
        return [torch.cat(parts, 1) for parts in zip(*per_level)]

    def suppress_tta(self, first, second, width):
        """The candidates of the pass on x and of the pass on its horizontal flip (`width` = x.shape[-1]) -> detections."""
        if self.soft_nms is not None and first[0].shape[1] + second[0].shape[1] > box_ops.MAX_SOFT_NMS_COUNT:
            raise ValueError('Model.tta with Model.soft_nms: the merged list has {} candidates per image, Soft-NMS takes {}: lower '
                             'top_n'.format(first[0].shape[1] + second[0].shape[1], box_ops.MAX_SOFT_NMS_COUNT))
        merged = box_ops.concat_candidates([first, second], [0, width])
        return box_ops.suppress(*merged, self.nms, self.detections, soft_nms=self.soft_nms, vote=self.box_voting,
                                threshold=self.threshold, matrix_nms=self.matrix_nms)

    def postprocess(self, cls_heads, box_heads, strides):
        """Raw head tensors -> (scores [B, D], boxes [B, D, 4|6], classes [B, D])."""
        self.check_inference_options()
        if self.fused_postprocess and cls_heads[0].is_cuda:
            # sigmoid + decode x5 + nms on the head tensors as the convolutions wrote them
            return box_ops.detect(cls_heads, box_heads, strides, self.anchors, self.threshold, self.top_n,
                                  self.nms, self.detections, self.rotated_bbox, logits=True, soft_nms=self.soft_nms,
                                  vote=self.box_voting, matrix_nms=self.matrix_nms)
        if self.box_voting is not None or self.matrix_nms is not None:
            return box_ops.suppress(*self.candidates(cls_heads, box_heads, strides), self.nms, self.detections,
                                    soft_nms=self.soft_nms, vote=self.box_voting, threshold=self.threshold,
                                    matrix_nms=self.matrix_nms)
        # the reference's sequence, call for call (model.py:140, :153-165); on CPU tensors this is the
        # pure-torch branch of odtk/box.py
        suppress = box_ops.nms_rotated if self.rotated_bbox else box_ops.nms
        if self.soft_nms is not None:
            def suppress(scores, boxes, classes, nms, detections):
                return box_ops.soft_nms(scores, boxes, classes, nms, detections, self.soft_nms.get('method', 'linear'),
                                        self.soft_nms.get('sigma', 0.5), self.soft_nms.get('min_score', self.threshold))
        per_level = [box_ops.decode(c.sigmoid().contiguous(), b.contiguous(), s, self.threshold, self.top_n,
                                    self.anchors[s], self.rotated_bbox)
                     for c, b, s in zip(cls_heads, box_heads, strides)]
        return suppress(*[torch.cat(parts, 1) for parts in zip(*per_level)], self.nms, self.detections)

    # ------------------------------------------------------------------ training loss
    def _extract_targets(self, targets, stride, size, want_cls_target=True):
        """Per-image target assignment of one level, stacked over the batch (reference model.py:167-184)."""
        anchors = self.level_anchors(stride)
        if targets.is_cuda and not self.rotated_bbox:
            # one fused HIP launch for the whole batch (csrc/targets.hpp) instead of ~25 torch ops per image
            return box_ops.snap_to_anchors_batched(targets, size[1], size[0], stride, anchors, self.classes,
                                                   self.anchor_ious, want_cls_target)
        assign = box_ops.snap_to_anchors_rotated if self.rotated_bbox else box_ops.snap_to_anchors
        if not self.rotated_bbox:
            anchors = anchors.to(targets.device)
        pixels = [extent * stride for extent in size[::-1]]             # [W, H] of the padded image
        per_image = [assign(t[t[:, -1] > -1], pixels, stride, anchors, self.classes, targets.device, self.anchor_ious)
                     for t in targets]
        return tuple(torch.stack(parts) for parts in zip(*per_image))

    def _compute_loss(self, x, cls_heads, box_heads, targets):
        """Focal + smooth-L1 losses summed over levels and normalised by the number of foreground
        anchors (reference model.py:186-210); `depth` is -1 ignore / 0 background / class+1.

        `cls_loss = 'qfl' | 'vfl'` replaces the focal term by the quality focal / varifocal loss on the soft target (odtk/loss.py),
        normalised in the same way.  On the fused path the quality pass then supplies the classification sums and the foreground
        count; `fused_pyramid_loss` is called only while `box_loss` is 'smooth_l1', for its box sum -- its classification half goes
        unused, as its box half does under an IoU-family `box_loss`.  `box_loss = 'probiou' | 'kld'` (rotated models) replaces the
        smooth-L1 term on the six deltas in the same way, by `rotated_box_loss` / `fused_pyramid_rotated_box_loss`."""
        cls_total, box_total, foreground = 0.0, 0.0, 0.0
        if self.assigner not in ('iou', 'atss', 'tal'):
            raise ValueError("Model.assigner must be 'iou', 'atss' or 'tal', not {!r}".format(self.assigner))
        iou_kind, gauss_kind, weight = None, None, None     # weight: of every box loss except smooth-L1
        if self.box_loss != 'smooth_l1':
            if self.box_loss not in BOX_LOSS_KINDS + ROTATED_BOX_LOSS_KINDS:
                raise ValueError("Model.box_loss must be 'smooth_l1', 'iou', 'giou' or 'diou' (axis-aligned boxes), 'probiou' or 'kld' "
                                 '(rotated boxes), not {!r}'.format(self.box_loss))
            if self.box_loss in BOX_LOSS_KINDS and self.rotated_bbox:
                raise ValueError('Model.box_loss = {!r} is not available for rotated boxes'.format(self.box_loss))
            if self.box_loss in ROTATED_BOX_LOSS_KINDS and not self.rotated_bbox:
                raise ValueError('Model.box_loss = {!r} needs a model of rotated boxes (rotated_bbox=True)'.format(self.box_loss))
            weight = self.box_loss_weight
            if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not (math.isfinite(weight) and weight > 0):
                raise ValueError('Model.box_loss_weight must be finite and > 0, not {!r}'.format(weight))
            if self.rotated_bbox:
                gauss_kind = self.box_loss
            else:
                iou_kind = self.box_loss
        quality_kind = None
        if self.cls_loss != 'focal':
            if self.cls_loss not in CLS_LOSS_KINDS:
                raise ValueError("Model.cls_loss must be 'focal', 'qfl' or 'vfl', not {!r}".format(self.cls_loss))
            if self.rotated_bbox:
                raise ValueError('Model.cls_loss = {!r} is not available for rotated boxes'.format(self.cls_loss))
            quality_kind = self.cls_loss
        if self.assigner != 'iou':
            if self.rotated_bbox:
                raise ValueError('Model.assigner = {!r} is not available for rotated boxes'.format(self.assigner))
            if len(cls_heads) > box_ops.MAX_LEVELS_PER_CALL:
                why = 'its threshold spans all of them' if self.assigner == 'atss' else 'a box ranks its candidates over all of them'
                raise ValueError('Model.assigner = {!r} takes at most {} pyramid levels ({}, so the call cannot be split), not {}'.format(
                    self.assigner, box_ops.MAX_LEVELS_PER_CALL, why, len(cls_heads)))
        strides = [x.shape[-1] / c.shape[-1] for c in cls_heads]
        sizes = [tuple(c.shape[-2:]) for c in cls_heads]
        anchors_list = [self.level_anchors(s) for s in strides]          # rotated models: (axis, rotated) pairs
        fused = self.fused_loss and cls_heads[0].is_cuda
        atss = None
        if self.assigner == 'atss':
            atss = box_ops.atss_assign_levels(targets, sizes, strides, anchors_list, self.classes, self.atss_topk, want_cls_target=not fused)
        elif self.assigner == 'tal':
            # the assignment reads the heads as constants (detached); from here on both paths consume it exactly as ATSS's
            atss = box_ops.tal_assign_levels(targets, [c.detach() for c in cls_heads], [b.detach() for b in box_heads], strides,
                                             anchors_list, self.classes, self.tal_topk, self.tal_alpha, self.tal_beta,
                                             want_cls_target=not fused)
        if fused:
            # targets of every level (ONE HIP launch for all of them; the class map is implied by depth and not even built), then focal
            # + smooth-L1 + masks + sums of ALL levels in one HIP pass -- and one more in backward (csrc/loss.hpp)
            if atss is not None:
                _, box_targets, depths = atss
            elif len(cls_heads) <= box_ops.MAX_LEVELS_PER_CALL:
                assign = box_ops.snap_to_anchors_rotated_levels if self.rotated_bbox else box_ops.snap_to_anchors_levels
                _, box_targets, depths = assign(targets, sizes, strides, anchors_list, self.classes, self.anchor_ious, want_cls_target=False)
            else:
                depths, box_targets = [], []
                for stride, size in zip(strides, sizes):
                    _, box_target, depth = self._extract_targets(targets, stride, size, False)
                    depths.append(depth)
                    box_targets.append(box_target)
            # -> (cls_sums, box_sums, fg), each from the pass that owns it.  The quality pass (csrc/quality_loss.hpp) supplies the
            # classification sums and the foreground count; the focal + smooth-L1 pass then runs only for its box sum (its
            # classification half goes unused: autograd hands it a zero gradient) and, with an IoU-family box loss, not at all:
            # nothing streams the logits twice.  The IoU-family and the Gaussian losses (csrc/box_iou_loss.hpp, csrc/
            # rotated_box_loss.hpp: rotated boxes, on the axis tables) are passes of their own over the foreground anchors; the
            # smooth-L1 sum of the focal pass then goes unused in the same way
            if quality_kind is not None:
                cls_sums, fg = fused_pyramid_quality_loss(cls_heads, box_heads, depths, box_targets, anchors_list, quality_kind)
            if quality_kind is None or iou_kind is None:
                focal_sums, box_sums, focal_fg = fused_pyramid_loss(cls_heads, box_heads, depths, box_targets, self.cls_criterion.alpha,
                                                                    self.cls_criterion.gamma, self.box_criterion.beta)
                if quality_kind is None:
                    cls_sums, fg = focal_sums, focal_fg
            if iou_kind is not None:
                box_sums, _ = fused_pyramid_box_iou_loss(box_heads, depths, box_targets, anchors_list, iou_kind)
            elif gauss_kind is not None:
                box_sums, _ = fused_pyramid_rotated_box_loss(box_heads, depths, box_targets, [a[0] for a in anchors_list], gauss_kind)
            foreground = fg.clamp(min=1).sum()              # per level, as the reference clamps (model.py:196)
            box_total = box_sums.sum() if weight is None else weight * box_sums.sum()
            return cls_sums.sum() / foreground, box_total / foreground
        for level, (cls_head, box_head) in enumerate(zip(cls_heads, box_heads)):
            if atss is not None:
                cls_target, box_target, depth = (per_level[level] for per_level in atss)
            else:
                cls_target, box_target, depth = self._extract_targets(targets, strides[level], cls_head.shape[-2:])
            foreground = foreground + (depth > 0).sum().float().clamp(min=1)
            if quality_kind is not None:
                # the soft target: the IoU of the predicted and the assigned box at the anchor's class, a constant of this loss
                quality = box_quality(box_head.view_as(box_target).float(), box_target, anchor_wh(anchors_list[level])).detach()
                soft = quality_target(depth, quality, cls_target.shape[2])
                criterion = quality_focal_loss if quality_kind == 'qfl' else varifocal_loss
                cls_loss = criterion(cls_head.view_as(cls_target).float(), soft)
            else:
                cls_loss = self.cls_criterion(cls_head.view_as(cls_target).float(), cls_target)
            cls_total = cls_total + (cls_loss * (depth >= 0).expand_as(cls_target).float()).sum()
            if iou_kind is not None:
                box_loss = box_iou_loss(box_head.view_as(box_target).float(), box_target, anchor_wh(anchors_list[level]), iou_kind)
                mask = (depth[:, :, 0] > 0).float()
            elif gauss_kind is not None:
                box_loss = rotated_box_loss(box_head.view_as(box_target).float(), box_target, anchor_wh(anchors_list[level][0]), gauss_kind)
                mask = (depth[:, :, 0] > 0).float()
            else:
                box_loss = self.box_criterion(box_head.view_as(box_target).float(), box_target)
                mask = (depth > 0).expand_as(box_target).float()
            box_total = box_total + (box_loss * mask).sum()
        if weight is not None:
            box_total = weight * box_total
        return cls_total / foreground, box_total / foreground
