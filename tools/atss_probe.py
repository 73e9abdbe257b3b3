#!/usr/bin/env python
"""What ATSS target assignment costs next to the fixed-IoU rule it can replace: odtk_atss_assign_levels (two launches: the
statistics launch `atss_stats_kernel`, one wave per target row, and the dense launch, one thread per anchor) against
odtk_snap_to_anchors_levels (one launch) on the same targets.  Every launch is timed by the library's own event pair around the
dispatch (odtk_profile_*), the two rules alternating call by call, the median of `--iters` calls each.

Workload: the pyramid of an 800 x 1280 image (strides 8..128: 100 x 160 down to 7 x 10 cells), 9 anchors, 80 classes, the batch
of `bench.py --mode train` (2 images), 8 and 64 boxes per image, no class map (the fused loss derives it from depth).
The yardstick is the training step of that benchmark (README.md): ATSS should stay below 1 % of it.

    python tools/atss_probe.py [--iters 100] [--step-ms 34.4]
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
ap.add_argument('--topk', type=int, default=9)
ap.add_argument('--step-ms', type=float, default=34.4, help='the training step the cost is set against')
args = ap.parse_args()
assert args.iters >= 50

HEIGHT, WIDTH, CLASSES = 800, 1280, 80
STRIDES = [8, 16, 32, 64, 128]
SIZES = [((HEIGHT + s - 1) // s, (WIDTH + s - 1) // s) for s in STRIDES]
ANCHORS = [box.generate_anchors(s, [1.0, 2.0, 0.5], [4 * 2 ** (i / 3) for i in range(3)]) for s in STRIDES]
NAMES = ('snap_to_anchors_kernel', 'atss_stats_kernel')


def collect():
    torch.cuda.synchronize()
    got = _C.profile_collect()
    return {k: got[k] for k in NAMES}


print('pyramid %s, batch %d, %d anchors, %d classes, topk %d, %d calls each' % (SIZES, args.batch, ANCHORS[0].shape[0], CLASSES,
                                                                               args.topk, args.iters))
for boxes in (8, 64):
    source = T.SyntheticBatches(args.batch, HEIGHT, WIDTH, classes=CLASSES, max_boxes=boxes, seed=boxes)
    _, targets = source.batch()
    targets[:, :, :] = torch.cat([source.batch()[1][:, :1] for _ in range(boxes)], 1)      # every row a box: `boxes` per image
    targets = targets.cuda()
    assert int((targets[:, :, 4] > -1).sum()) == args.batch * boxes
    rules = {'iou': lambda: box.snap_to_anchors_levels(targets, SIZES, STRIDES, ANCHORS, CLASSES, [0.4, 0.5], want_cls_target=False),
             'atss': lambda: box.atss_assign_levels(targets, SIZES, STRIDES, ANCHORS, CLASSES, args.topk, want_cls_target=False)}
    positives = {}
    for rule, fn in rules.items():
        for _ in range(5):
            out = fn()
        positives[rule] = sum(int((d > 0).sum()) for d in out[2])
    _C.profile_enable(True, NAMES)
    collect()
    us = {'iou': [], 'atss stats': [], 'atss dense': [], 'atss': []}
    for _ in range(args.iters):
        rules['iou']()
        got = collect()
        assert got['snap_to_anchors_kernel'][1] == 1
        us['iou'].append(got['snap_to_anchors_kernel'][0] * 1e3)
        rules['atss']()
        got = collect()
        assert got['snap_to_anchors_kernel'][1] == 1 and got['atss_stats_kernel'][1] == 1
        us['atss stats'].append(got['atss_stats_kernel'][0] * 1e3)
        us['atss dense'].append(got['snap_to_anchors_kernel'][0] * 1e3)
        us['atss'].append(us['atss stats'][-1] + us['atss dense'][-1])
    _C.profile_enable(False)
    print('== %d boxes per image: positives iou %d, atss %d' % (boxes, positives['iou'], positives['atss']))
    for name, v in us.items():
        v = sorted(v)
        med = statistics.median(v)
        print('  %-12s median %7.1f us  (min %7.1f, p90 %7.1f)  = %.3f %% of a %.1f ms step' % (
            name, med, v[0], v[int(0.9 * (len(v) - 1))], med / (args.step_ms * 1e3) * 100, args.step_ms))
