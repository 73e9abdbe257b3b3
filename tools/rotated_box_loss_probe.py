#!/usr/bin/env python
"""What the Gaussian box losses of rotated boxes (csrc/rotated_box_loss.hpp; `Model.box_loss = 'probiou' | 'kld'`) cost in a
training step: the forward (the walk over one lane per anchor cell + the fixed-order sum, two launches) and the backward (one
launch) of each kind, next to the existing rotated loss launches (focal + smooth-L1 on the six deltas, csrc/loss.hpp) on the same
heads and targets.  Every launch is timed by the library's own event pair around the dispatch (odtk_profile_*), the candidates
alternating call by call after a warm-up, the median of `--iters` calls each.

Workload: the rotated BASELINE shape -- the pyramid of an 800 x 1280 image (strides 8..128: 100 x 160 down to 7 x 10 cells), 27
anchors (3 ratios x 3 scales x 3 angles), 80 classes, 2 images, targets from odtk_snap_to_anchors_rotated_levels with 8 and 64
boxes per image, predictions = targets + N(0, 0.15), fp32 and bf16 heads as the convolutions write them (channels_last).

    python tools/rotated_box_loss_probe.py [--iters 100] [--step-ms 34.4]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]
import torch  # noqa: E402
from odtk import _C, box  # noqa: E402
from odtk import train as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=100)
ap.add_argument('--batch', type=int, default=2)
ap.add_argument('--step-ms', type=float, default=34.4, help='the training step the cost is set against')
args = ap.parse_args()
assert args.iters >= 50

HEIGHT, WIDTH, CLASSES = 800, 1280, 80
STRIDES = [8, 16, 32, 64, 128]
SIZES = [((HEIGHT + s - 1) // s, (WIDTH + s - 1) // s) for s in STRIDES]
ANCHORS = [box.generate_anchors_rotated(s, [1.0, 2.0, 0.5], [4 * 2 ** (i / 3) for i in range(3)], [-math.pi / 6, 0.0, math.pi / 6])
           for s in STRIDES]
AXIS = [pair[0] for pair in ANCHORS]
A = AXIS[0].shape[0]
KINDS = ('probiou', 'kld')
NAMES = ('retina_loss_kernel', 'loss_reduce_kernel')     # ODTK_KERNEL_LOSS / ODTK_KERNEL_LOSS_REDUCE: both losses' launches


def say(*a):
    print(*a, flush=True)


def collect():
    torch.cuda.synchronize()
    got = _C.profile_collect()
    return {k: got[k] for k in NAMES}


def workload(boxes, dtype):
    source = T.SyntheticBatches(args.batch, HEIGHT, WIDTH, classes=CLASSES, max_boxes=boxes, seed=boxes, rotated=True)
    _, targets = source.batch()
    targets[:, :, :] = torch.cat([source.batch()[1][:, :1] for _ in range(boxes)], 1)      # every row a box: `boxes` per image
    targets = targets.cuda()
    assert int((targets[:, :, 5] > -1).sum()) == args.batch * boxes
    _, box_targets, depths = box.snap_to_anchors_rotated_levels(targets, SIZES, STRIDES, ANCHORS, CLASSES, [0.4, 0.5], want_cls_target=False)
    g = torch.Generator(device='cuda').manual_seed(boxes)
    box_heads = [(bt.reshape(args.batch, -1, *bt.shape[-2:]) + torch.randn(args.batch, A * 6, *bt.shape[-2:], device='cuda', generator=g)
                  * 0.15).to(dtype).contiguous(memory_format=torch.channels_last) for bt in box_targets]
    cls_heads = [(torch.randn(args.batch, A * CLASSES, h, w, device='cuda', generator=g) * 1.5 - 4.0).to(dtype)
                 .contiguous(memory_format=torch.channels_last) for h, w in SIZES]
    return cls_heads, box_heads, depths, box_targets


def line(name, samples):
    v = sorted(samples)
    med = statistics.median(v)
    say('  %-34s median %7.1f us  (min %7.1f, p90 %7.1f)  = %.3f %% of a %.1f ms step' % (
        name, med, v[0], v[int(0.9 * (len(v) - 1))], med / (args.step_ms * 1e3) * 100, args.step_ms))
    return med


say('pyramid %s, batch %d, %d anchors, %d classes, %d calls each' % (SIZES, args.batch, A, CLASSES, args.iters))
for boxes in (8, 64):
    for dtype in (torch.float32, torch.bfloat16):
        cls_heads, box_heads, depths, box_targets = workload(boxes, dtype)
        fg = sum(int((d > 0).sum()) for d in depths)
        cells = sum(d.numel() for d in depths)
        g_levels = torch.full((len(SIZES),), 1.0 / max(fg, 1), device='cuda')

        def smooth_fwd():
            return _C.retina_loss_levels_forward(cls_heads, box_heads, depths, box_targets, 0.25, 2.0, 0.11, reproducible=True)

        def smooth_bwd():
            return _C.retina_loss_levels_backward(cls_heads, box_heads, depths, box_targets, 0.25, 2.0, 0.11, g_levels, g_levels)

        calls = {'focal + smooth-L1 forward': smooth_fwd, 'focal + smooth-L1 backward': smooth_bwd}
        for kind in KINDS:
            calls[kind + ' forward'] = lambda kind=kind: _C.rotated_box_loss_levels_forward(box_heads, depths, box_targets, AXIS, kind)
            calls[kind + ' backward'] = lambda kind=kind: _C.rotated_box_loss_levels_backward(box_heads, depths, box_targets, AXIS, kind, g_levels)
        for fn in calls.values():
            for _ in range(5):
                fn()
        values = {kind: _C.rotated_box_loss_levels_forward(box_heads, depths, box_targets, AXIS, kind).cpu() for kind in KINDS}
        smooth = smooth_fwd().cpu()
        _C.profile_enable(True, NAMES)
        collect()
        walk = {k: [] for k in calls}
        reduce = {k: [] for k in calls if k.endswith('forward')}
        for _ in range(args.iters):
            for name, fn in calls.items():
                fn()
                got = collect()
                assert got['retina_loss_kernel'][1] == 1 and got['loss_reduce_kernel'][1] == (1 if name in reduce else 0), (name, got)
                walk[name].append(got['retina_loss_kernel'][0] * 1e3)
                if name in reduce:
                    reduce[name].append(got['loss_reduce_kernel'][0] * 1e3)
        _C.profile_enable(False)
        say('== %d boxes per image, %s heads (channels_last): %d foreground anchors of %d cells (%.2f %%)' % (
            boxes, str(dtype).replace('torch.', ''), fg, cells, 100.0 * fg / cells))
        say('  mean loss per foreground anchor: smooth-L1 %.4f (sum over 6 deltas), probiou %.4f, kld %.4f' % (
            float(smooth[:, 1].sum()) / max(fg, 1), *[float(values[k][:, 0].sum()) / max(fg, 1) for k in KINDS]))
        total = {}
        for name in calls:
            med = line(name + (' (walk)' if name in reduce else ''), walk[name])
            if name in reduce:
                med += line(name + ' (sum launch)', reduce[name])
            total[name] = med
        for kind in KINDS:
            both = total[kind + ' forward'] + total[kind + ' backward']
            existing = total['focal + smooth-L1 forward'] + total['focal + smooth-L1 backward']
            say('  %-7s forward + backward %.1f us = %.3f %% of a %.1f ms step; the existing loss launches, which keep running: %.1f us' % (
                kind, both, both / (args.step_ms * 1e3) * 100, args.step_ms, existing))
