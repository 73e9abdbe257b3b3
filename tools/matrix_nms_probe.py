#!/usr/bin/env python
"""odtk_matrix_nms (linear and Gaussian, pre_top 2000) against the hard NMS and Soft-NMS on THE SAME candidates.  Every launch
is timed by the library's own event pair around the dispatch (odtk_profile_*; all of them are recorded under ODTK_KERNEL_NMS):
a hard or soft suppression is one launch, Matrix NMS four, whose times are summed ("kernels").  "span" is a device event pair
around the whole call: the kernels plus the gaps between the four launches.  The rules alternate call by call; medians of
`--iters` calls each.  The two inputs of tools/soft_nms_probe.py:

  trained : tests/golden/nms_trained_scenes_ties.npz (16 images of a trained detector, 100..2552 clustered candidates each)
  bench   : decode_levels' candidates from the benchmark's heads -- ResNet50FPN, randn images, batch 8, 800 x 1280, bf16, the last
            classification convolution rescaled as bench.py does -- 5 x 1000 per image

The split over the four launches comes from a kernel trace in a run of its own (the profiler slows the host):

    python tools/matrix_nms_probe.py [--iters 100] [--skip-bench | --only-bench]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/matrix_nms_probe.py --iters 20 --only-matrix [--skip-bench | --only-bench]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from odtk import _C, box  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=100)
ap.add_argument('--skip-bench', action='store_true')
ap.add_argument('--only-bench', action='store_true')
ap.add_argument('--only-matrix', action='store_true', help='Matrix NMS alone (for a kernel trace)')
ap.add_argument('--sigma', type=float, default=0.5)
ap.add_argument('--min-score', type=float, default=0.05)
ap.add_argument('--pre-top', type=int, default=2000)
args = ap.parse_args()


def timed(fn, launches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    total, n = _C.profile_collect()['nms_kernel']
    assert n == launches, (n, launches)
    return total * 1e3, start.elapsed_time(stop) * 1e3


def measure(name, scores, boxes, classes, nms, det, run_len):
    matrix = lambda m: lambda: _C.matrix_nms(scores, boxes, classes, det, args.pre_top, m, args.sigma, args.min_score)
    rules = {'matrix linear': (matrix(_C.MATRIX_NMS_LINEAR), 4), 'matrix gaussian': (matrix(_C.MATRIX_NMS_GAUSSIAN), 4)}
    if not args.only_matrix:
        rules = dict({'hard (odtk_nms_sorted_runs)': (lambda: _C.nms_sorted_runs(scores, boxes, classes, run_len, nms, det), 1),
                      'soft linear': (lambda: _C.soft_nms(scores, boxes, classes, nms, det, _C.SOFT_NMS_LINEAR, args.sigma, args.min_score), 1),
                      'soft gaussian': (lambda: _C.soft_nms(scores, boxes, classes, nms, det, _C.SOFT_NMS_GAUSSIAN, args.sigma, args.min_score), 1)},
                     **rules)
    kept = {}
    for rule, (fn, _) in rules.items():
        for _ in range(5):
            out = fn()
        kept[rule] = (out[0] > 0).sum(1)
    torch.cuda.synchronize()
    _C.profile_enable(True, ('nms_kernel',))
    _C.profile_collect()
    us = {rule: [] for rule in rules}
    for _ in range(args.iters):
        for rule, (fn, launches) in rules.items():
            us[rule].append(timed(fn, launches))
    _C.profile_enable(False)
    alive = (scores > 0).sum(1)
    print('== %s: %d images x %d candidates (%d..%d positive), %d detections, nms %.2f, sigma %.2f, min_score %.3f, pre_top %d, %d calls each'
          % (name, scores.shape[0], scores.shape[1], int(alive.min()), int(alive.max()), det, nms, args.sigma, args.min_score,
             args.pre_top, args.iters))
    first = next(iter(rules))
    base = statistics.median(k for k, _ in us[first])
    for rule, v in us.items():
        kernels, span = sorted(k for k, _ in v), sorted(s for _, s in v)
        print('  %-28s kernels: median %7.1f us (min %7.1f, p90 %7.1f)  span: median %7.1f us   x %.2f of %s   kept per image: %d..%d, %d in all'
              % (rule, statistics.median(kernels), kernels[0], kernels[int(0.9 * (len(kernels) - 1))], statistics.median(span),
                 statistics.median(kernels) / base, first, int(kept[rule].min()), int(kept[rule].max()), int(kept[rule].sum())))


if not args.only_bench:
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'nms_trained_scenes_ties.npz'))
    s, b, c = (torch.from_numpy(g[k]).cuda() for k in ('scores', 'boxes', 'classes'))
    measure('trained', s, b, c, float(g['nms']), int(g['detections']), run_len=s.shape[1] // 5)

if not args.skip_bench:
    import bench
    from odtk.model import Model
    torch.manual_seed(0)
    model = Model(backbones='ResNet50FPN', classes=80)
    model.initialize(None)
    model = model.cuda().to(memory_format=torch.channels_last).eval()
    x = torch.randn(8, 3, 800, 1280, generator=torch.Generator().manual_seed(0)).cuda().contiguous(memory_format=torch.channels_last)

    def heads(inp):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            return model.heads(inp)
    bench.calibrate_cls_head(model, heads, x, bench.SPEC_FRACTION, model.threshold)
    cls_heads, box_heads = heads(x)
    strides = [x.shape[-1] // t.shape[-1] for t in cls_heads]
    for st in strides:
        model.level_anchors(st)
    s, b, c = box.decode_levels(cls_heads, box_heads, strides, model.threshold, model.top_n, model.anchors, logits=True)
    del cls_heads, box_heads
    measure('bench heads (ResNet50FPN, batch 8, 800 x 1280, bf16)', s, b, c, model.nms, model.detections, run_len=model.top_n)
