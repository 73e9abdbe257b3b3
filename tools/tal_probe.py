#!/usr/bin/env python
"""What task-aligned target assignment costs next to ATSS: odtk_tal_assign_levels (three launches: the selection
`tal_select_kernel`, one workgroup per target row; the fill, zeros to every output; the scatter, one thread per selected entry)
against odtk_atss_assign_levels (two launches) on the same targets.  Every launch is timed by the library's own event pair
around the dispatch (odtk_profile_*): the selection under `atss_stats_kernel`, fill + scatter under `snap_to_anchors_kernel`; a
call without target rows runs the fill alone, which splits the two.  The two assigners alternate call by call, the median of
`--iters` calls each.

Workload: the heads of RN50FPN on an 800 x 1280 image (strides 8..128: 100 x 160 down to 7 x 10 cells), 9 anchors, 80 classes,
the batch of `bench.py --mode train` (2 images), random logits ~ N(0, 2) and deltas ~ N(0, 0.3) in `--dtype` and `--layout`, 8 and
64 boxes per image from SyntheticBatches, no class map (the fused loss derives it from depth) -- and ONE synthetic row that covers
the whole image (about 190 000 candidates: the worst case of the streaming selection).

    python tools/tal_probe.py [--iters 100] [--step-ms 34.4] [--dtype bfloat16] [--layout channels_last]
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
ap.add_argument('--topk', type=int, default=13)
ap.add_argument('--dtype', default='bfloat16', choices=['float32', 'bfloat16', 'float16'])
ap.add_argument('--layout', default='channels_last', choices=['nchw', 'channels_last'])
ap.add_argument('--step-ms', type=float, default=34.4, help='the training step the cost is set against')
args = ap.parse_args()
assert args.iters >= 20

HEIGHT, WIDTH, CLASSES = 800, 1280, 80
STRIDES = [8, 16, 32, 64, 128]
SIZES = [((HEIGHT + s - 1) // s, (WIDTH + s - 1) // s) for s in STRIDES]
ANCHORS = [box.generate_anchors(s, [1.0, 2.0, 0.5], [4 * 2 ** (i / 3) for i in range(3)]) for s in STRIDES]
NAMES = ('snap_to_anchors_kernel', 'atss_stats_kernel')
A = ANCHORS[0].shape[0]
FORMAT = torch.channels_last if args.layout == 'channels_last' else torch.contiguous_format
g = torch.Generator().manual_seed(1)
CLS = [(torch.randn(args.batch, A * CLASSES, h, w, generator=g) * 2).to(getattr(torch, args.dtype)).cuda().contiguous(memory_format=FORMAT)
       for h, w in SIZES]
BOX = [(torch.randn(args.batch, A * 4, h, w, generator=g) * 0.3).to(getattr(torch, args.dtype)).cuda().contiguous(memory_format=FORMAT)
       for h, w in SIZES]


def collect():
    torch.cuda.synchronize()
    got = _C.profile_collect()
    return {k: got[k] for k in NAMES}


def measure(label, targets):
    empty = targets[:, :0].contiguous()
    rules = {'atss': lambda: box.atss_assign_levels(targets, SIZES, STRIDES, ANCHORS, CLASSES, 9, want_cls_target=False),
             'tal': lambda: box.tal_assign_levels(targets, CLS, BOX, STRIDES, ANCHORS, CLASSES, args.topk, 1, 6, want_cls_target=False),
             'fill': lambda: box.tal_assign_levels(empty, CLS, BOX, STRIDES, ANCHORS, CLASSES, args.topk, 1, 6, want_cls_target=False)}
    positives = {}
    for rule, fn in rules.items():
        for _ in range(3):
            out = fn()
        positives[rule] = sum(int((d > 0).sum()) for d in out[2])
    _C.profile_enable(True, NAMES)
    collect()
    us = {'atss stats': [], 'atss dense': [], 'atss': [], 'tal select': [], 'tal fill': [], 'tal scatter': [], 'tal': []}
    for _ in range(args.iters):
        rules['atss']()
        got = collect()
        assert got['snap_to_anchors_kernel'][1] == 1 and got['atss_stats_kernel'][1] == 1
        us['atss stats'].append(got['atss_stats_kernel'][0] * 1e3)
        us['atss dense'].append(got['snap_to_anchors_kernel'][0] * 1e3)
        us['atss'].append(us['atss stats'][-1] + us['atss dense'][-1])
        rules['fill']()
        got = collect()
        assert got['snap_to_anchors_kernel'][1] == 1 and got['atss_stats_kernel'][1] == 0
        us['tal fill'].append(got['snap_to_anchors_kernel'][0] * 1e3)
        rules['tal']()
        got = collect()
        assert got['snap_to_anchors_kernel'][1] == 2 and got['atss_stats_kernel'][1] == 1
        us['tal select'].append(got['atss_stats_kernel'][0] * 1e3)
        us['tal scatter'].append(got['snap_to_anchors_kernel'][0] * 1e3 - us['tal fill'][-1])
        us['tal'].append(us['tal select'][-1] + got['snap_to_anchors_kernel'][0] * 1e3)
    _C.profile_enable(False)
    print('== %s: positives atss %d, tal %d' % (label, positives['atss'], positives['tal']))
    for name, v in us.items():
        v = sorted(v)
        med = statistics.median(v)
        print('  %-12s median %7.1f us  (min %7.1f, p90 %7.1f)  = %.3f %% of a %.1f ms step' % (
            name, med, v[0], v[int(0.9 * (len(v) - 1))], med / (args.step_ms * 1e3) * 100, args.step_ms))


print('pyramid %s, batch %d, %d anchors, %d classes, heads %s %s, topk %d, %d calls each' % (
    SIZES, args.batch, A, CLASSES, args.dtype, args.layout, args.topk, args.iters))
for boxes in (8, 64):
    source = T.SyntheticBatches(args.batch, HEIGHT, WIDTH, classes=CLASSES, max_boxes=boxes, seed=boxes)
    _, targets = source.batch()
    targets[:, :, :] = torch.cat([source.batch()[1][:, :1] for _ in range(boxes)], 1)      # every row a box: `boxes` per image
    targets = targets.cuda()
    assert int((targets[:, :, 4] > -1).sum()) == args.batch * boxes
    measure('%d boxes per image' % boxes, targets)
whole = torch.tensor([[[0.0, 0.0, float(WIDTH), float(HEIGHT), 3.0]]] * args.batch).cuda()
measure('one row that covers the whole image', whole)
