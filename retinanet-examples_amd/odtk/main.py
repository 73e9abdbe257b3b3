#!/usr/bin/env python3
"""`odtk` command line (reference odtk/main.py): `train`, `infer`, `export` with the reference's flags.

What differs from the reference, and why:

  * one process per GPU either way, but both launch styles work: run plainly, the command spawns a worker per
    visible GPU like the reference (main.py:243-251); run under `torchrun` (RANK / WORLD_SIZE / LOCAL_RANK in
    the environment), each process is one worker and nothing is spawned.  `backend="nccl"` is RCCL on ROCm.
  * every worker loads the checkpoint itself instead of receiving a pickled, shared-memory model from the
    parent (main.py:244-245): no 150 MB pickle per rank, no CPU shared-memory segment behind GPU-resident
    weights.
  * `--with-apex` / `--with-dali` and TensorRT engines (`.plan` / `.engine`, `export` to anything) name
    dependencies the north star drops; they are accepted by the parser and refused with a clear error.
  * `--device-resize` (train, infer) is new: what DALI did for the reference -- resize, flip, pad, normalise on the GPU -- as one
    HIP launch per batch (odtk/data.py), bit-identical to the default loader.
  * `--device-augment` (train) is new as well: `--device-resize` plus the training augmentations (`--augment-rotate` and the four
    colour options) on the GPU, as a short chain of HIP launches per batch, bit-identical to Pillow on the host.
  * `--augment-free-rotate MIN MAX` (train), which the reference parses and ignores, rotates every training image by an angle drawn
    from the range, bilinear, on its own canvas, and its boxes with it; with `--device-augment` on the GPU, the same pixels.
  * `--mosaic P` (train) with `--mosaic-scale LO HI` is new: with probability P a training item is a mosaic of four images on one
    canvas (odtk/data.py: CocoDataset); with `--device-augment` the composition is one more HIP pass, the same pixels.  Axis-aligned
    boxes only, not with the turns or the free rotation.  Never stored in a checkpoint.
  * `--soft-nms {linear,gaussian}` (infer; train: its validation passes) with `--soft-nms-sigma` / `--soft-nms-min-score` is new:
    Soft-NMS (odtk/box.py:soft_nms, one HIP launch) instead of the reference's hard suppression.  Never stored in a checkpoint.
  * `--matrix-nms {linear,gaussian}` (infer; train: its validation passes) with `--matrix-nms-sigma` / `--matrix-nms-min-score` /
    `--matrix-nms-pre` is new: Matrix NMS (odtk/box.py:matrix_nms, four HIP launches) instead of the hard suppression; unlike
    Soft-NMS it takes the merged candidate lists of `--tta flip` and `--tile` at any length.  Never stored in a checkpoint.
  * `--assigner {iou,atss}` (train) with `--atss-topk` is new: ATSS target assignment (odtk/box.py:atss_assign_levels, two HIP
    launches) instead of the reference's fixed `--anchor-ious` rule; axis-aligned boxes only.  Never stored in a checkpoint: a
    resumed run has to be given the flag again.
  * `--assigner tal` (train) with `--tal-topk`, `--tal-alpha` and `--tal-beta` is new as well: task-aligned target assignment (TOOD;
    odtk/box.py:tal_assign_levels, three HIP launches).  A box takes as positives the `--tal-topk` anchors inside it with the largest
    score^alpha * IoU^beta of what the network predicts there; with `--cls-loss qfl|vfl --box-loss giou` it is the TOOD-style
    recipe.  Axis-aligned boxes only.  Never stored in a checkpoint: give the flags again when resuming.
  * `--box-voting value` and `--tta flip` (infer; train: its validation passes) are new: box voting behind the suppression
    (odtk/box.py:box_vote, one HIP launch: every kept box becomes the score-weighted mean of its class's candidates that overlap it
    by at least `value`) and test-time augmentation by the horizontal flip (the network also runs on the mirrored batch, one
    suppression over both candidate lists).  Axis-aligned boxes only; never stored in a checkpoint.
  * `--tile size` with `--tile-overlap px`, `--tile-border px` and `--tile-batch n` (infer; train: its validation passes) is new:
    tiled inference of large images (odtk/model.py:forward_tiled).  Every image of the batch is cut into overlapping square tiles
    of `size` pixels (a multiple of the model's stride; one HIP launch per chunk, csrc/tile.hpp), the network runs on chunks of
    `--tile-batch` tiles (default 8) -- one tensor shape whatever the image, so one plan of the engine --, the candidates move back
    into image coordinates (one more launch; `--tile-border` drops those that reach into the outermost pixels of an interior tile
    side, where the neighbouring tile sees the object whole) and one suppression sees them all.  Default overlap: a quarter of the
    size.  Axis-aligned boxes only, not together with `--tta`; never stored in a checkpoint.
  * `--box-loss {smooth-l1,iou,giou,diou}` (train) with `--box-loss-weight value` is new: the box regression is trained with an IoU,
    GIoU or DIoU loss on the boxes the deltas decode to (odtk/loss.py:box_iou_loss; a HIP pass of its own over the foreground
    anchors, csrc/box_iou_loss.hpp) instead of the reference's smooth-L1 on the four deltas, times the weight (default 1).
    Axis-aligned boxes only.  Never stored in a checkpoint: a resumed run has to be given the flags again.
  * `--cls-loss {focal,qfl,vfl}` (train) is new: the class scores are trained as localisation-quality estimates, with the quality
    focal loss (GFL) or the varifocal loss (VarifocalNet) on a soft target -- at a foreground anchor the IoU of the box the network
    predicts there and the box it was assigned (odtk/loss.py:quality_focal_loss / varifocal_loss; a HIP pass over the logits that
    computes the target in place, csrc/quality_loss.hpp) -- instead of the reference's focal loss on a one-hot target.  Inference
    is unchanged.  Axis-aligned boxes only.  Never stored in a checkpoint: a resumed run has to be given the flag again.
  * `--rotated-bbox --box-loss {probiou,kld}` (train) is new: rotated boxes are trained with the ProbIoU or the KLD loss on the
    Gaussians of the boxes the six deltas decode to (odtk/loss.py:rotated_box_loss; a HIP pass of its own over the foreground
    anchors, csrc/rotated_box_loss.hpp) instead of the reference's smooth-L1 on (dx, dy, dw, dh, sin, cos), times
    `--box-loss-weight`.  The loss sees the (sin, cos) pair only through its direction and charges a square box nothing for its
    angle.  Rotated boxes only; `iou`, `giou` and `diou` stay axis-aligned only.  Never stored in a checkpoint.
  * `--ema DECAY`, `--clip-grad-norm MAX` and `--fused-step` (train) are new: with any of them the optimisation step is
    odtk/optim.py's `FusedSGD` -- GradScaler's unscale and skip, the clip factor, weight decay, momentum, the update and the
    average in one HIP pass over the parameters (csrc/optim.hpp), the gradient norm in one more -- instead of torch.optim.SGD; the
    optimizer state in the checkpoint is the same either way.  `--ema` keeps an exponential moving average of the weights
    (decay min(DECAY, (1 + t) / (10 + t)) at step t): validation runs on it, the checkpoint carries it as `ema` beside the raw
    weights (resuming continues both; resuming without `--ema` drops it and says so), and `infer` / `export` load it unless
    `--no-ema` is given.  `--clip-grad-norm` scales the gradients so that their global L2 norm is at most MAX and skips a step whose
    norm is not finite; the report line and the scalar log gain `grad_norm`.  The flags themselves are not stored: give them again
    when resuming.
"""
import argparse
import os
import sys

import torch
import torch.cuda
import torch.distributed
import torch.multiprocessing

from . import infer, train
from .model import Model

ROTATED_BOX_LOSSES = ('probiou', 'kld')                # the --box-loss values that need --rotated-bbox (odtk/loss.py)

def _flag(name, kind=None, default=None, text='', **extra):
    """One row of the flag tables below: (name, argparse keyword arguments)."""
    spec = dict(extra, help=text)
    if kind is bool:
        spec['action'] = 'store_true'
        if default is not None:                                         # argparse.SUPPRESS: no attribute unless the switch is given
            spec['default'] = default
    else:
        spec.update(type=kind, default=default)
    return name, spec


_DROPPED = 'names a dependency this build drops; refused at run time'
_SIZES = [_flag('--batch', int, None, 'images per step over all GPUs (default: 2 per GPU)', metavar='size'),
          _flag('--resize', int, 800, 'short side after resizing', metavar='scale'),
          _flag('--max-size', int, 1333, 'cap on the long side after resizing', metavar='max')]
_COMMON = [_flag('--with-apex', bool, text=_DROPPED), _flag('--with-dali', bool, text=_DROPPED),
           _flag('--workers', int, 8, 'loader processes per GPU (the reference hard-codes 2; ~6 feed one MI355X)', metavar='num'),
           # not a flag of the reference: absent from the namespace unless given (read with getattr)
           _flag('--device-resize', bool, text='resize, flip, pad and normalise the images on the device, bit-identical to the '
                 'host loader (train: not with --augment-rotate or non-zero colour augmentations)', default=argparse.SUPPRESS),
           _flag('--soft-nms', str, argparse.SUPPRESS, 'Soft-NMS instead of hard suppression: neighbours of a kept box keep a decayed '
                 'score (train: in the validation passes; not with --rotated-bbox)', choices=['linear', 'gaussian']),
           _flag('--soft-nms-sigma', float, argparse.SUPPRESS, 'width of the gaussian decay (default 0.5)', metavar='value'),
           _flag('--soft-nms-min-score', float, argparse.SUPPRESS, 'decayed scores below this are dropped (default: the '
                 "model's score threshold)", metavar='value'),
           _flag('--matrix-nms', str, argparse.SUPPRESS, 'Matrix NMS instead of hard suppression: every score is decayed by one '
                 'factor from the pairwise IoUs of the best candidates; takes candidate lists of any length (train: in the validation '
                 'passes; not with --soft-nms or --rotated-bbox)', choices=['linear', 'gaussian']),
           _flag('--matrix-nms-sigma', float, argparse.SUPPRESS, 'width of the gaussian decay (default 0.5)', metavar='value'),
           _flag('--matrix-nms-min-score', float, argparse.SUPPRESS, 'decayed scores below this are dropped (default: the '
                 "model's score threshold)", metavar='value'),
           _flag('--matrix-nms-pre', int, argparse.SUPPRESS, 'candidates per image that take part, the best by score, in 1..4096 '
                 '(default 2000)', metavar='count'),
           _flag('--box-voting', float, argparse.SUPPRESS, 'box voting behind the suppression: every kept box becomes the score-weighted '
                 'mean of the candidates of its class that overlap it by at least this IoU, in (0, 1] (0.65 is customary; not with '
                 '--rotated-bbox)', metavar='value'),
           _flag('--tta', str, argparse.SUPPRESS, 'test-time augmentation: flip = the network also runs on the mirrored batch and one '
                 'suppression sees both candidate lists (about two forwards per batch; not with --rotated-bbox)', choices=['flip']),
           _flag('--tile', int, argparse.SUPPRESS, 'tiled inference of large images: cut every image into overlapping square tiles of this '
                 "many pixels (a multiple of the model's stride), run the network on the tiles and suppress once over all their candidates "
                 '(not with --rotated-bbox or --tta)', metavar='size'),
           _flag('--tile-overlap', int, argparse.SUPPRESS, 'pixels that neighbouring tiles share (default: a quarter of --tile)', metavar='px'),
           _flag('--tile-border', float, argparse.SUPPRESS, 'drop the candidates of a tile that reach into this many of its outermost pixels '
                 'on a side that is not an image side (default 0: keep all)', metavar='px'),
           _flag('--tile-batch', int, argparse.SUPPRESS, 'tiles per pass of the network (default 8, at most 64)', metavar='n')]

# same names, types and defaults as the reference's parser (main.py:15-118)
TRAIN_FLAGS = [
    _flag('--annotations', str, None, 'COCO-style annotation file', metavar='path', required=True),
    _flag('--images', str, '.', 'image directory', metavar='path'),
    _flag('--backbone', str, ['ResNet50FPN'], 'one backbone or several', nargs='+'),
    _flag('--classes', int, 80, 'number of object classes', metavar='num'),
    *_SIZES,
    _flag('--jitter', int, [640, 1024], 'range of short-side sizes drawn per image', nargs=2, metavar='min max'),
    _flag('--iters', int, 90000, 'training iterations', metavar='number'),
    _flag('--milestones', int, [60000, 80000], 'iterations at which the learning rate drops', nargs='*'),
    _flag('--schedule', float, 1, 'stretch factor for --iters and --milestones', metavar='scale'),
    _flag('--full-precision', bool, text='fp32 instead of mixed precision'),
    _flag('--lr', float, 0.01, 'peak learning rate', metavar='value'),
    _flag('--warmup', int, 1000, 'iterations of linear warm-up', metavar='iterations'),
    _flag('--gamma', float, 0.1, 'learning-rate factor at a milestone', metavar='value'),
    _flag('--override', bool, text='start from scratch even if the model file exists'),
    _flag('--val-annotations', str, None, 'annotation file of the validation set', metavar='path'),
    _flag('--val-images', str, None, 'image directory of the validation set', metavar='path'),
    _flag('--post-metrics', str, None, 'POST training metrics to this address', metavar='url'),
    _flag('--fine-tune', str, None, 'initialise from this checkpoint', metavar='path'),
    _flag('--logdir', str, None, 'directory for scalar logs', metavar='logdir'),
    _flag('--val-iters', int, 8000, 'iterations between two validations', metavar='number'),
    *_COMMON,
    _flag('--device-augment', bool, text='--device-resize, and the quarter turns and colour augmentations run on the device as '
          'well, bit-identical to the host loader', default=argparse.SUPPRESS),
    _flag('--augment-rotate', bool, text='random quarter turns'),
    _flag('--augment-free-rotate', float, [0, 0], 'rotate every training image about its centre by an angle drawn uniformly from '
          'this range of degrees, counter-clockwise positive, and its boxes with it (0 0: off; not with --device-resize alone)', nargs=2,
          metavar='value value'),
    _flag('--augment-brightness', float, 0.002, 'sigma of the brightness factor', metavar='value'),
    _flag('--augment-contrast', float, 0.002, 'sigma of the contrast factor', metavar='value'),
    _flag('--augment-hue', float, 0.0002, 'sigma of the hue shift', metavar='value'),
    _flag('--augment-saturation', float, 0.002, 'sigma of the saturation factor', metavar='value'),
    _flag('--regularization-l2', float, 0.0001, 'weight decay', metavar='value'),
    _flag('--rotated-bbox', bool, text='boxes are [x, y, w, h, theta]'),
    _flag('--anchor-ious', float, [0.4, 0.5], 'background / foreground overlap thresholds', nargs=2, metavar='value value'),
    _flag('--absolute-angle', bool, text='regress the absolute angle instead of -45..45 degrees'),
    # not flags of the reference: absent from the namespace unless given (read with getattr)
    _flag('--assigner', str, argparse.SUPPRESS, 'how ground truth becomes training targets: iou = the fixed --anchor-ious thresholds '
          '(default), atss = adaptive training sample selection, tal = task-aligned assignment by the predicted score and IoU (both '
          'not with --rotated-bbox).  Not stored in the checkpoint: give it again when resuming', choices=['iou', 'atss', 'tal']),
    _flag('--mosaic', float, argparse.SUPPRESS, 'probability with which a training item is a mosaic of four images on one canvas of '
          'the image\'s size (default 0: off; on the host, or with --device-augment on the device, the same pixels either way; not with '
          '--rotated-bbox, --augment-rotate, --augment-free-rotate or --device-resize alone).  Not stored in the checkpoint', metavar='P'),
    _flag('--mosaic-scale', float, argparse.SUPPRESS, 'range of the factor on the four images of a mosaic, 0 < LO <= HI <= 1 '
          '(default 0.5 1; needs --mosaic)', nargs=2, metavar=('LO', 'HI')),
    _flag('--atss-topk', int, argparse.SUPPRESS, 'nearest cells per box and pyramid level that ATSS considers, 1..16 (default 9; '
          'needs --assigner atss)', metavar='num'),
    _flag('--tal-topk', int, argparse.SUPPRESS, 'anchors a box takes as positives under task-aligned assignment, 1..16 (default 13; '
          'needs --assigner tal; give it again when resuming)', metavar='num'),
    _flag('--tal-alpha', int, argparse.SUPPRESS, 'exponent of the class score in the task-aligned metric, a whole number in 0..4 '
          '(default 1; needs --assigner tal; give it again when resuming)', metavar='n'),
    _flag('--tal-beta', int, argparse.SUPPRESS, 'exponent of the IoU in the task-aligned metric, a whole number in 1..8 (default 6; '
          'needs --assigner tal; give it again when resuming)', metavar='n'),
    _flag('--box-loss', str, argparse.SUPPRESS, 'what the box regression is trained with: smooth-l1 on the four deltas (default), or an '
          'iou / giou / diou loss on the boxes they decode to (not with --rotated-bbox), or a probiou / kld loss on the Gaussians of the '
          'rotated boxes the six deltas decode to (only with --rotated-bbox).  Not stored in the checkpoint: give it again '
          'when resuming', choices=['smooth-l1', 'iou', 'giou', 'diou', 'probiou', 'kld']),
    _flag('--box-loss-weight', float, argparse.SUPPRESS, 'factor on the box loss, finite and > 0 (default 1; needs --box-loss iou, '
          'giou, diou, probiou or kld)', metavar='value'),
    _flag('--ema', float, argparse.SUPPRESS, 'keep an exponential moving average of the weights with this decay, in (0, 1) (0.9998 is '
          'customary): it is what gets validated, it is saved beside the raw weights and `infer` loads it.  Give it again when resuming: '
          'without it a stored average is dropped', metavar='DECAY'),
    _flag('--clip-grad-norm', float, argparse.SUPPRESS, 'scale the gradients so that their global L2 norm is at most this, finite and '
          '> 0 (35 is customary); a step whose norm is not finite is skipped.  Not stored in the checkpoint: give it again when resuming',
          metavar='MAX'),
    _flag('--fused-step', bool, text='run the optimisation step as one HIP pass over the parameters (implied by --ema and '
          '--clip-grad-norm; same optimizer state in the checkpoint)', default=argparse.SUPPRESS),
    _flag('--cls-loss', str, argparse.SUPPRESS, 'what the class scores are trained with: focal on the one-hot target (default), or the '
          'quality focal (qfl) / varifocal (vfl) loss on the IoU of the predicted and the assigned box (not with --rotated-bbox).  Not '
          'stored in the checkpoint: give it again when resuming', choices=['focal', 'qfl', 'vfl']),
]
INFER_FLAGS = [
    _flag('--images', str, '.', 'image directory', metavar='path'),
    _flag('--annotations', str, None, 'annotation file: evaluate against it', metavar='annotations'),
    _flag('--output', str, ['detections.json'], 'JSON file(s) for the detections', nargs='+', metavar='file'),
    *_SIZES, *_COMMON,
    _flag('--full-precision', bool, text='fp32 instead of mixed precision'),
    _flag('--rotated-bbox', bool, text='the model predicts rotated boxes'),
    _flag('--no-ema', bool, text='use the raw weights of a checkpoint that also holds averaged ones (--ema of train); the default is '
          'the average', default=argparse.SUPPRESS),
]
EXPORT_FLAGS = [                                                   # parsed for compatibility; `export` itself is refused
    _flag('--size', int, [1280], nargs='+', metavar='height width'), _flag('--full-precision', bool), _flag('--int8', bool),
    _flag('--calibration-batches', int, 2, metavar='size'), _flag('--calibration-images', str, '', metavar='path'),
    _flag('--calibration-table', str, '', metavar='path'), _flag('--verbose', bool), _flag('--rotated-bbox', bool),
    _flag('--dynamic-batch-opts', int, [1, 8, 16], nargs=3, metavar='value value value'),
    _flag('--no-ema', bool, default=argparse.SUPPRESS),
]


def parse(args):
    parser = argparse.ArgumentParser(description='ODTK: Object Detection Toolkit.')
    parser.add_argument('--master', metavar='address:port', type=str, default='127.0.0.1:29500',
                        help='rendezvous of the per-GPU workers')
    commands = parser.add_subparsers(help='sub-command', dest='command')
    commands.required = True
    per_gpu = 2 * max(1, torch.cuda.device_count())
    for name, positional, flags, text in (
            ('train', [('model', 'checkpoint to write (and to resume from when it exists)')], TRAIN_FLAGS, 'train a network'),
            ('infer', [('model', 'checkpoint to load')], INFER_FLAGS, 'run inference'),
            ('export', [('model', 'checkpoint to load'), ('export', 'output file')], EXPORT_FLAGS,
             'TensorRT export (dropped: refused)')):
        sub = commands.add_parser(name, help=text)
        for arg, arg_text in positional:
            sub.add_argument(arg, type=str, help=arg_text)
        for flag, spec in flags:
            spec = dict(spec)
            if flag == '--batch':
                spec['default'] = per_gpu
            sub.add_argument(flag, **spec)
    parsed = parser.parse_args(args)
    soft = [f for f in ('soft_nms', 'soft_nms_sigma', 'soft_nms_min_score') if hasattr(parsed, f)]
    if soft and getattr(parsed, 'rotated_bbox', False):
        parser.error('--soft-nms is not available with --rotated-bbox')
    if soft and 'soft_nms' not in soft:
        parser.error('--soft-nms-sigma / --soft-nms-min-score need --soft-nms {linear,gaussian}')
    matrix = [f for f in ('matrix_nms', 'matrix_nms_sigma', 'matrix_nms_min_score', 'matrix_nms_pre') if hasattr(parsed, f)]
    if matrix and getattr(parsed, 'rotated_bbox', False):
        parser.error('--matrix-nms is not available with --rotated-bbox')
    if matrix and soft:
        parser.error('--matrix-nms is not available with --soft-nms')
    if matrix and 'matrix_nms' not in matrix:
        parser.error('--matrix-nms-sigma / --matrix-nms-min-score / --matrix-nms-pre need --matrix-nms {linear,gaussian}')
    if hasattr(parsed, 'matrix_nms_pre') and not 1 <= parsed.matrix_nms_pre <= 4096:
        parser.error('--matrix-nms-pre must be in 1..4096')
    for flag in ('box_voting', 'tta'):
        if hasattr(parsed, flag) and getattr(parsed, 'rotated_bbox', False):
            parser.error('--%s is not available with --rotated-bbox' % flag.replace('_', '-'))
    if hasattr(parsed, 'box_voting') and not 0 < parsed.box_voting <= 1:          # (a NaN fails both comparisons)
        parser.error('--box-voting must be in (0, 1]')
    if not hasattr(parsed, 'tile'):
        if any(hasattr(parsed, f) for f in ('tile_overlap', 'tile_border', 'tile_batch')):
            parser.error('--tile-overlap / --tile-border / --tile-batch need --tile size')
    else:
        if getattr(parsed, 'rotated_bbox', False):
            parser.error('--tile is not available with --rotated-bbox')
        if hasattr(parsed, 'tta'):
            parser.error('--tile is not available with --tta')
        if parsed.tile < 1:
            parser.error('--tile must be positive')
        if not 0 <= getattr(parsed, 'tile_overlap', 0) < parsed.tile:
            parser.error('--tile-overlap must be in [0, --tile)')
        if not 0 <= getattr(parsed, 'tile_border', 0.0) < float('inf'):           # (a NaN fails both comparisons)
            parser.error('--tile-border must be finite and not negative')
        if not 1 <= getattr(parsed, 'tile_batch', 8) <= 64:
            parser.error('--tile-batch must be in 1..64')
    if hasattr(parsed, 'atss_topk') and getattr(parsed, 'assigner', 'iou') != 'atss':
        parser.error('--atss-topk needs --assigner atss')
    if hasattr(parsed, 'atss_topk') and not 1 <= parsed.atss_topk <= 16:
        parser.error('--atss-topk must be in 1..16')
    if getattr(parsed, 'assigner', 'iou') == 'atss' and getattr(parsed, 'rotated_bbox', False):
        parser.error('--assigner atss is not available with --rotated-bbox')
    for flag, low, high in (('tal_topk', 1, 16), ('tal_alpha', 0, 4), ('tal_beta', 1, 8)):
        if hasattr(parsed, flag) and getattr(parsed, 'assigner', 'iou') != 'tal':
            parser.error('--%s needs --assigner tal' % flag.replace('_', '-'))
        if hasattr(parsed, flag) and not low <= getattr(parsed, flag) <= high:
            parser.error('--%s must be in %d..%d' % (flag.replace('_', '-'), low, high))
    if getattr(parsed, 'assigner', 'iou') == 'tal' and getattr(parsed, 'rotated_bbox', False):
        parser.error('--assigner tal is not available with --rotated-bbox')
    if hasattr(parsed, 'box_loss_weight'):
        if getattr(parsed, 'box_loss', 'smooth-l1') == 'smooth-l1':
            parser.error('--box-loss-weight needs --box-loss iou, giou, diou, probiou or kld')
        if not 0 < parsed.box_loss_weight < float('inf'):                         # (a NaN fails both comparisons)
            parser.error('--box-loss-weight must be finite and > 0')
    if getattr(parsed, 'box_loss', 'smooth-l1') in ROTATED_BOX_LOSSES:
        if not getattr(parsed, 'rotated_bbox', False):
            parser.error('--box-loss {} needs --rotated-bbox'.format(parsed.box_loss))
    elif getattr(parsed, 'box_loss', 'smooth-l1') != 'smooth-l1' and getattr(parsed, 'rotated_bbox', False):
        parser.error('--box-loss {} is not available with --rotated-bbox'.format(parsed.box_loss))
    if getattr(parsed, 'cls_loss', 'focal') != 'focal' and getattr(parsed, 'rotated_bbox', False):
        parser.error('--cls-loss {} is not available with --rotated-bbox'.format(parsed.cls_loss))
    if hasattr(parsed, 'ema') and not 0 < parsed.ema < 1:                          # (a NaN fails both comparisons)
        parser.error('--ema must be a decay in (0, 1)')
    if hasattr(parsed, 'clip_grad_norm') and not 0 < parsed.clip_grad_norm < float('inf'):
        parser.error('--clip-grad-norm must be finite and > 0')
    if hasattr(parsed, 'mosaic_scale') and not hasattr(parsed, 'mosaic'):
        parser.error('--mosaic-scale needs --mosaic P')
    if hasattr(parsed, 'mosaic'):
        if not 0 <= parsed.mosaic <= 1:                                           # (a NaN fails both comparisons)
            parser.error('--mosaic must be a probability in [0, 1]')
        low, high = getattr(parsed, 'mosaic_scale', (0.5, 1.0))
        if not 0 < low <= high <= 1:
            parser.error('--mosaic-scale must be a range with 0 < LO <= HI <= 1')
        for flag, given in (('--rotated-bbox', parsed.rotated_bbox), ('--augment-rotate', parsed.augment_rotate),
                            ('--augment-free-rotate', any(parsed.augment_free_rotate)),
                            ('--device-resize without --device-augment', getattr(parsed, 'device_resize', False)
                             and not getattr(parsed, 'device_augment', False))):
            if given:
                parser.error('--mosaic is not available with ' + flag)
    return parsed


def soft_nms_options(args, model):
    """What `--soft-nms*` ask for, as `Model.soft_nms` takes it (None: the flags were not given)."""
    if not hasattr(args, 'soft_nms'):
        return None
    return {'method': args.soft_nms, 'sigma': getattr(args, 'soft_nms_sigma', 0.5),
            'min_score': getattr(args, 'soft_nms_min_score', model.threshold)}


def matrix_nms_options(args, model):
    """What `--matrix-nms*` ask for, as `Model.matrix_nms` takes it (None: the flags were not given)."""
    if not hasattr(args, 'matrix_nms'):
        return None
    return {'method': args.matrix_nms, 'sigma': getattr(args, 'matrix_nms_sigma', 0.5),
            'min_score': getattr(args, 'matrix_nms_min_score', model.threshold), 'pre_top': getattr(args, 'matrix_nms_pre', 2000)}


def tile_options(args):
    """What `--tile*` ask for, as `Model.tile` takes it (None: the flags were not given)."""
    if not hasattr(args, 'tile'):
        return None
    tile = {'size': (args.tile, args.tile), 'border': getattr(args, 'tile_border', 0.0), 'batch': getattr(args, 'tile_batch', 8)}
    if hasattr(args, 'tile_overlap'):
        tile['overlap'] = (args.tile_overlap, args.tile_overlap)
    return tile


def load_model(args, verbose=False):
    """Fresh model (train on a new path, or --override), or a `.pth` / `.torch` checkpoint with its training
    state (reference main.py:121-152).  TensorRT plans are refused."""
    if args.command != 'train' and not os.path.isfile(args.model):
        raise RuntimeError('Model file {} does not exist!'.format(args.model))
    state = {}
    ext = os.path.splitext(args.model)[1]
    if args.command == 'train' and (not os.path.exists(args.model) or args.override):
        if verbose:
            print('Initializing model...')
        model = Model(backbones=args.backbone, classes=args.classes, rotated_bbox=args.rotated_bbox,
                      anchor_ious=args.anchor_ious)
        model.initialize(args.fine_tune)
    elif ext in ('.pth', '.torch'):
        if verbose:
            print('Loading model from {}...'.format(os.path.basename(args.model)))
        model, state = Model.load(filename=args.model, rotated_bbox=args.rotated_bbox)
        if args.command != 'train' and 'ema' in state:              # the averaged weights are what a trained checkpoint is used with
            if getattr(args, 'no_ema', False):
                if verbose:
                    print('Using the raw weights (--no-ema); the checkpoint also holds averaged ones.')
            else:
                model.load_state_dict(state['ema']['state_dict'])
                if verbose:
                    print('Using the averaged weights (EMA, {} updates) of the checkpoint.'.format(state['ema']['updates']))
    elif ext in ('.engine', '.plan'):
        raise RuntimeError('TensorRT engines are not supported on MI355X: "{}"'.format(args.model))
    else:
        raise RuntimeError('Invalid model format "{}"!'.format(ext))
    model.freeze_unused_params()                                   # (reference: unused params are frozen, :136,143)
    if verbose:
        print(model)
    state['path'] = args.model
    return model, state


def launched_by_torchrun():
    return 'RANK' in os.environ and 'WORLD_SIZE' in os.environ


def worker(rank, args, world, spawned=False):
    """One process, one GPU (or the CPU)."""
    if spawned:
        address, port = args.master.rsplit(':', 1)
        os.environ.update({'MASTER_ADDR': address, 'MASTER_PORT': port, 'WORLD_SIZE': str(world), 'RANK': str(rank)})
    if torch.cuda.is_available():
        local = int(os.environ.get('LOCAL_RANK', rank))
        if local >= torch.cuda.device_count():
            raise RuntimeError('rank %d (local rank %d) has no GPU: this host has %d -- one process per GPU' % (
                rank, local, torch.cuda.device_count()))
        torch.cuda.set_device(local)
    if world > 1 and not torch.distributed.is_initialized():
        torch.distributed.init_process_group(backend='nccl' if torch.cuda.is_available() else 'gloo',
                                             init_method='env://', world_size=world, rank=rank)
    if args.command != 'export' and args.batch % world != 0:
        raise RuntimeError('Batch size should be a multiple of the number of GPUs')

    model, state = load_model(args, verbose=(rank == 0))
    if model.angles is not None:
        args.rotated_bbox = True
    if args.command != 'export':
        model.soft_nms = soft_nms_options(args, model)
        if model.soft_nms is not None and args.rotated_bbox:
            raise RuntimeError('--soft-nms is not available for a model with rotated boxes')
        model.matrix_nms = matrix_nms_options(args, model)
        if model.matrix_nms is not None and args.rotated_bbox:
            raise RuntimeError('--matrix-nms is not available for a model with rotated boxes')
        model.box_voting, model.tta = getattr(args, 'box_voting', None), getattr(args, 'tta', None)
        for flag, value in (('--box-voting', model.box_voting), ('--tta', model.tta)):
            if value is not None and args.rotated_bbox:
                raise RuntimeError('%s is not available for a model with rotated boxes' % flag)
        model.tile = tile_options(args)
        if model.tile is not None:
            if args.rotated_bbox:
                raise RuntimeError('--tile is not available for a model with rotated boxes')
            if args.tile % model.stride:
                raise RuntimeError("--tile must be a multiple of the model's stride, {}".format(model.stride))
    if args.command == 'train':
        model.assigner, model.atss_topk = getattr(args, 'assigner', 'iou'), getattr(args, 'atss_topk', 9)
        model.tal_topk, model.tal_alpha, model.tal_beta = getattr(args, 'tal_topk', 13), getattr(args, 'tal_alpha', 1), getattr(args, 'tal_beta', 6)
        if model.assigner in ('atss', 'tal') and args.rotated_bbox:
            raise RuntimeError('--assigner {} is not available for a model with rotated boxes'.format(model.assigner))
        model.box_loss = getattr(args, 'box_loss', 'smooth-l1').replace('-', '_')
        model.box_loss_weight = getattr(args, 'box_loss_weight', 1.0)
        if model.box_loss in ROTATED_BOX_LOSSES:
            if not model.rotated_bbox:
                raise RuntimeError('--box-loss {} needs a model with rotated boxes (--rotated-bbox)'.format(args.box_loss))
        elif model.box_loss != 'smooth_l1' and args.rotated_bbox:
            raise RuntimeError('--box-loss {} is not available for a model with rotated boxes'.format(args.box_loss))
        model.cls_loss = getattr(args, 'cls_loss', 'focal')
        if model.cls_loss != 'focal' and args.rotated_bbox:
            raise RuntimeError('--cls-loss {} is not available for a model with rotated boxes'.format(args.cls_loss))
    try:
        if args.command == 'train':
            return train.train(model, state, args.images, args.annotations, args.val_images or args.images,
                               args.val_annotations, args.resize, args.max_size, args.jitter, args.batch,
                               int(args.iters * args.schedule), args.val_iters, args.lr, args.warmup,
                               [int(m * args.schedule) for m in args.milestones], args.gamma, rank, world=world,
                               mixed_precision=not args.full_precision, with_apex=args.with_apex, use_dali=args.with_dali,
                               metrics_url=args.post_metrics, logdir=args.logdir, verbose=(rank == 0),
                               rotate_augment=args.augment_rotate, augment_brightness=args.augment_brightness,
                               augment_contrast=args.augment_contrast, augment_hue=args.augment_hue,
                               augment_saturation=args.augment_saturation, regularization_l2=args.regularization_l2,
                               rotated_bbox=args.rotated_bbox, absolute_angle=args.absolute_angle,
                               num_workers=args.workers, device_resize=getattr(args, 'device_resize', False),
                               device_augment=getattr(args, 'device_augment', False),
                               augment_free_rotate=tuple(args.augment_free_rotate), mosaic=getattr(args, 'mosaic', 0.0),
                               mosaic_scale=tuple(getattr(args, 'mosaic_scale', (0.5, 1.0))), ema_decay=getattr(args, 'ema', None),
                               clip_grad_norm=getattr(args, 'clip_grad_norm', None), fused_step=getattr(args, 'fused_step', False))
        if args.command == 'infer':
            return infer.infer(model, args.images, args.output, args.resize, args.max_size, args.batch,
                               annotations=args.annotations, mixed_precision=not args.full_precision,
                               is_master=(rank == 0), world=world, with_apex=args.with_apex, use_dali=args.with_dali,
                               verbose=(rank == 0), rotated_bbox=args.rotated_bbox, num_workers=args.workers,
                               device_resize=getattr(args, 'device_resize', False))
        return model.export(args.size, args.dynamic_batch_opts)     # raises: TensorRT is dropped
    finally:
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()


def main(args=None):
    """Entry point for the odtk command."""
    args = parse(args or sys.argv[1:])
    if launched_by_torchrun():
        return worker(int(os.environ['RANK']), args, int(os.environ['WORLD_SIZE']))
    world = torch.cuda.device_count()
    if args.command == 'export' or world <= 1:
        return worker(0, args, 1)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')       # dmabuf IPC: what RCCL needs on this driver
    torch.multiprocessing.spawn(worker, args=(args, world, True), nprocs=world)


if __name__ == '__main__':
    main()
