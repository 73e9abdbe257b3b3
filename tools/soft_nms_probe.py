#!/usr/bin/env python
"""odtk_soft_nms (linear and Gaussian) against the hard NMS on THE SAME candidates: every launch timed by the library's own
event pair around the dispatch (odtk_profile_*; both kernels are recorded under ODTK_KERNEL_NMS), the three rules alternating
launch by launch, the median of `--iters` launches each.  Two inputs:

  trained : tests/golden/nms_trained_scenes_ties.npz (16 images of a trained detector, 100..2552 clustered candidates each);
            hard = odtk_nms_ex on arbitrary-order input, and odtk_nms_sorted_runs (what odtk_detect runs; 118 us in
            profiles/r06_nms_clustered.txt)
  bench   : decode_levels' candidates from the benchmark's heads -- ResNet50FPN, randn images, batch 8, 800 x 1280, bf16, the last
            classification convolution rescaled as bench.py does -- 5 x 1000 per image

    python tools/soft_nms_probe.py [--iters 100] [--skip-bench]
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
ap.add_argument('--sigma', type=float, default=0.5)
ap.add_argument('--min-score', type=float, default=0.05)
args = ap.parse_args()


def timed(fn):
    fn()
    torch.cuda.synchronize()
    total, n = _C.profile_collect()['nms_kernel']
    assert n == 1, n
    return total * 1e3


def measure(name, scores, boxes, classes, nms, det, run_len=None):
    rules = {'hard (odtk_nms_ex)': lambda: _C.nms(scores, boxes, classes, nms, det),
             'soft linear': lambda: _C.soft_nms(scores, boxes, classes, nms, det, _C.SOFT_NMS_LINEAR, args.sigma, args.min_score),
             'soft gaussian': lambda: _C.soft_nms(scores, boxes, classes, nms, det, _C.SOFT_NMS_GAUSSIAN, args.sigma, args.min_score)}
    if run_len:
        rules['hard (odtk_nms_sorted_runs)'] = lambda: _C.nms_sorted_runs(scores, boxes, classes, run_len, nms, det)
    kept = {}
    for rule, fn in rules.items():
        for _ in range(5):
            out = fn()
        kept[rule] = (out[0] > 0).sum(1)
    torch.cuda.synchronize()
    _C.profile_enable(True, ('nms_kernel',))
    _C.profile_collect()
    us = {rule: [] for rule in rules}
    for _ in range(args.iters):
        for rule, fn in rules.items():
            us[rule].append(timed(fn))
    _C.profile_enable(False)
    alive = (scores > 0).sum(1)
    print('== %s: %d images x %d candidates (%d..%d positive), %d detections, nms %.2f, sigma %.2f, min_score %.3f, %d launches each'
          % (name, scores.shape[0], scores.shape[1], int(alive.min()), int(alive.max()), det, nms, args.sigma, args.min_score, args.iters))
    base = statistics.median(us['hard (odtk_nms_ex)'])
    for rule, v in us.items():
        v = sorted(v)
        print('  %-28s median %7.1f us  (min %7.1f, p90 %7.1f)  x %.2f of odtk_nms_ex   kept per image: %d..%d, %d in all'
              % (rule, statistics.median(v), v[0], v[int(0.9 * (len(v) - 1))], statistics.median(v) / base,
                 int(kept[rule].min()), int(kept[rule].max()), int(kept[rule].sum())))


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
