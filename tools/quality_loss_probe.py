#!/usr/bin/env python
"""What the quality focal / varifocal classification loss (csrc/quality_loss.hpp; `Model.cls_loss`) costs: its forward (the walk over
the logits + the fixed-order sum, two launches) and its backward (one launch), for each kind, next to the focal + smooth-L1
launches (csrc/loss.hpp) in the same process on the same heads and targets.  Both walks move the same bytes -- every logit read once
forward, read and written once backward -- so the ratio of the two is the figure; the share of HBM peak is given for both.  Every
launch is timed by the library's own event pair around the dispatch (odtk_profile_*), the candidates alternating call by call after a
warm-up, the median of `--iters` calls each.

Workload: the pyramid of an 800 x 1280 image (strides 8..128), 9 anchors, 80 classes, the batch of `bench.py --mode train`
(2 images), targets from odtk_snap_to_anchors_levels with 8 and 64 boxes per image, predicted deltas = targets + N(0, 0.15), logits
N(-4, 1.5), fp32 and bf16 heads as the convolutions write them (channels_last).

`--step` instead times whole training steps of `bench.py --mode train`'s model (ResNet50FPN, synthetic batches) with the default
options and with `cls_loss qfl, box_loss giou, assigner atss`.

    python tools/quality_loss_probe.py [--iters 100] [--hbm-tbs 8.0]
    python tools/quality_loss_probe.py --step [--step-iters 30]
"""
import argparse
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
ap.add_argument('--hbm-tbs', type=float, default=8.0, help='HBM peak the shares are set against, TB/s')
ap.add_argument('--step', action='store_true', help='only whole training steps: default options against qfl + giou + atss')
ap.add_argument('--step-iters', type=int, default=30)
args = ap.parse_args()
assert args.iters >= 20

HEIGHT, WIDTH, CLASSES = 800, 1280, 80
STRIDES = [8, 16, 32, 64, 128]
SIZES = [((HEIGHT + s - 1) // s, (WIDTH + s - 1) // s) for s in STRIDES]
ANCHORS = [box.generate_anchors(s, [1.0, 2.0, 0.5], [4 * 2 ** (i / 3) for i in range(3)]) for s in STRIDES]
NAMES = ('retina_loss_kernel', 'loss_reduce_kernel')     # ODTK_KERNEL_LOSS / ODTK_KERNEL_LOSS_REDUCE: both losses' launches


def say(*a):
    print(*a, flush=True)


if args.step:
    import time
    from odtk.model import Model
    torch.manual_seed(0)
    model = Model('ResNet50FPN', classes=CLASSES).cuda().train()
    model.initialize(None)
    optimizer = torch.optim.SGD(model.parameters(), lr=1e-4, momentum=0.9)
    source = T.SyntheticBatches(args.batch, HEIGHT, WIDTH, classes=CLASSES, seed=0)
    data, target = source.batch()
    data, target = data.cuda(), target.cuda()
    options = {'default': ('focal', 'smooth_l1', 'iou'), 'qfl + giou + atss': ('qfl', 'giou', 'atss'), 'default again': ('focal', 'smooth_l1', 'iou')}
    for name, (cls_loss, box_loss, assigner) in options.items():
        model.cls_loss, model.box_loss, model.assigner = cls_loss, box_loss, assigner
        times = []
        for i in range(5 + args.step_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            optimizer.zero_grad(set_to_none=True)
            cls, boxl = model((data, target))
            (cls + boxl).backward()
            optimizer.step()
            torch.cuda.synchronize()
            if i >= 5:
                times.append((time.perf_counter() - t0) * 1e3)
        v = sorted(times)
        say('%-20s fp32 step, batch %d at %d x %d: median %.2f ms (min %.2f, p90 %.2f); losses %.4f / %.4f' % (
            name, args.batch, HEIGHT, WIDTH, statistics.median(v), v[0], v[int(0.9 * (len(v) - 1))], float(cls), float(boxl)))
    raise SystemExit(0)


def collect():
    torch.cuda.synchronize()
    got = _C.profile_collect()
    return {k: got[k] for k in NAMES}


def workload(boxes, dtype):
    source = T.SyntheticBatches(args.batch, HEIGHT, WIDTH, classes=CLASSES, max_boxes=boxes, seed=boxes)
    _, targets = source.batch()
    targets[:, :, :] = torch.cat([source.batch()[1][:, :1] for _ in range(boxes)], 1)      # every row a box: `boxes` per image
    targets = targets.cuda()
    _, box_targets, depths = box.snap_to_anchors_levels(targets, SIZES, STRIDES, ANCHORS, CLASSES, [0.4, 0.5], want_cls_target=False)
    g = torch.Generator(device='cuda').manual_seed(boxes)
    box_heads = [(bt.reshape(args.batch, -1, *bt.shape[-2:]) + torch.randn(args.batch, bt.shape[1] * 4, *bt.shape[-2:], device='cuda', generator=g)
                  * 0.15).to(dtype).contiguous(memory_format=torch.channels_last) for bt in box_targets]
    cls_heads = [(torch.randn(args.batch, 9 * CLASSES, h, w, device='cuda', generator=g) * 1.5 - 4.0).to(dtype)
                 .contiguous(memory_format=torch.channels_last) for h, w in SIZES]
    return cls_heads, box_heads, depths, box_targets


def line(name, samples, nbytes):
    v = sorted(samples)
    med = statistics.median(v)
    say('  %-38s median %7.1f us  (min %7.1f, p90 %7.1f)  %5.2f TB/s = %4.1f %% of %.1f TB/s' % (
        name, med, v[0], v[int(0.9 * (len(v) - 1))], nbytes / med * 1e-6, nbytes / med * 1e-6 / args.hbm_tbs * 100, args.hbm_tbs))
    return med


say('pyramid %s, batch %d, 9 anchors, %d classes, %d calls each' % (SIZES, args.batch, CLASSES, args.iters))
for boxes in (8, 64):
    for dtype in (torch.float32, torch.bfloat16):
        cls_heads, box_heads, depths, box_targets = workload(boxes, dtype)
        fg = sum(int((d > 0).sum()) for d in depths)
        logit_bytes = sum(t.numel() * t.element_size() for t in cls_heads)
        g_levels = torch.full((len(SIZES),), 1.0 / max(fg, 1), device='cuda')
        calls = {
            'focal + smooth-L1 forward': lambda: _C.retina_loss_levels_forward(cls_heads, box_heads, depths, box_targets, 0.25, 2.0, 0.11, reproducible=True),
            'focal + smooth-L1 backward': lambda: _C.retina_loss_levels_backward(cls_heads, box_heads, depths, box_targets, 0.25, 2.0, 0.11, g_levels, g_levels)}
        for kind in ('qfl', 'vfl'):
            calls[kind + ' forward'] = lambda kind=kind: _C.quality_loss_levels_forward(cls_heads, box_heads, depths, box_targets, ANCHORS, kind)
            calls[kind + ' backward'] = lambda kind=kind: _C.quality_loss_levels_backward(cls_heads, box_heads, depths, box_targets, ANCHORS, kind,
                                                                                        0.75, 2.0, g_levels)
        calls['qfl gamma 1.5 forward'] = lambda: _C.quality_loss_levels_forward(cls_heads, box_heads, depths, box_targets, ANCHORS, 'qfl', 0.75, 1.5)
        calls['qfl gamma 1.5 backward'] = lambda: _C.quality_loss_levels_backward(cls_heads, box_heads, depths, box_targets, ANCHORS, 'qfl', 0.75, 1.5,
                                                                                  g_levels)
        for fn in calls.values():
            for _ in range(5):
                fn()
        values = {kind: calls[kind + ' forward']().cpu() for kind in ('qfl', 'vfl')}
        focal = calls['focal + smooth-L1 forward']().cpu()
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
        say('== %d boxes per image, %s heads (channels_last): %d foreground anchors, %.1f MB of logits' % (
            boxes, str(dtype).replace('torch.', ''), fg, logit_bytes / 1e6))
        say('  classification loss per foreground anchor: focal %.4f, qfl %.4f, vfl %.4f' % (
            float(focal[:, 0].sum()) / max(fg, 1), *[float(values[k][:, 0].sum()) / max(fg, 1) for k in ('qfl', 'vfl')]))
        total = {}
        for name in calls:
            med = line(name + (' (walk)' if name in reduce else ''), walk[name], logit_bytes * (1 if name in reduce else 2))
            if name in reduce:
                sums = sorted(reduce[name])
                say('  %-38s median %7.1f us' % (name + ' (sum launch)', statistics.median(sums)))
                med += statistics.median(sums)
            total[name] = med
        for kind in ('qfl', 'vfl', 'qfl gamma 1.5'):
            say('  %-14s forward %.1f us = %.2f x the focal + smooth-L1 forward; backward %.1f us = %.2f x' % (
                kind, total[kind + ' forward'], total[kind + ' forward'] / total['focal + smooth-L1 forward'],
                total[kind + ' backward'], total[kind + ' backward'] / total['focal + smooth-L1 backward']))
