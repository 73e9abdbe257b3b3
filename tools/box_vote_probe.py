#!/usr/bin/env python
"""box_vote_kernel and concat_candidates_kernel (csrc/box_vote.hpp) beside the NMS launch they follow, every launch timed by the
library's own event pair around the dispatch (odtk_profile_*; all three are recorded under ODTK_KERNEL_NMS, so each is launched
alone between two collects), the launches alternating, the median of `--iters` each.  Inputs, 100 detections, vote at 0.65:

  clustered : 8 images x 5 000 and x 10 000 candidates of tests/box_vote_ref.py's generator (80 classes, 60 clusters)
  trained   : tests/golden/nms_trained_scenes_ties.npz (16 images of a trained detector, up to 2552 clustered candidates each)

then, unless --skip-model, on ResNet50FPN at batch 8, 800 x 1280, bf16 with the benchmark's calibrated heads:

  detect    : box.detect with vote=0.65 against box.detect without it on the same head tensors (stream events around the call):
              the price of leaving odtk_detect's sorted-run NMS for the general one, plus the vote launch
  forward   : Model.forward through the engine, default against tta='flip' and tta + voting

    python tools/box_vote_probe.py [--iters 100] [--skip-model]

--ap does something else and nothing of the above: it trains tools/trained_ap.py's detector (tests/test_gpu_trained_ap.py: ResNet18FPN
on odtk/scenes.py, fp32, one seed) and scores the fp32 engine's detections on held-out scenes with that harness's COCO scorer
under hard NMS, + voting, + tta, + tta + voting.

    python tools/box_vote_probe.py --ap [--seed 0] [--iterations 2500] [--images 256]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd'), os.path.join(ROOT, 'tests')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import box_vote_ref  # noqa: E402
from odtk import _C, box  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=100)
ap.add_argument('--skip-model', action='store_true')
ap.add_argument('--vote', type=float, default=0.65)
ap.add_argument('--ap', action='store_true')
ap.add_argument('--seed', type=int, default=0)
ap.add_argument('--iterations', type=int, default=2500)
ap.add_argument('--images', type=int, default=256)
args = ap.parse_args()


def trained_ap():
    import time
    import test_gpu_trained_ap as T
    from odtk import scenes
    from odtk.cocoeval import COCOeval
    from odtk.data import CocoIndex
    from odtk.infer import detections_to_coco
    batch, size = 16, 512
    t0 = time.time()
    model, _ = T.train_detector(seed=args.seed, iterations=args.iterations, batch=batch, size=size)
    print('seed %d: ResNet18FPN trained for %d iterations in %.0f s; fp32 engine, %d held-out scenes of %d x %d, nms %.2f, %d detections'
          % (args.seed, args.iterations, time.time() - t0, args.images, size, size, model.nms, model.detections))
    configs = [('hard NMS', None, None), ('hard NMS + voting %.2f' % args.vote, args.vote, None), ('hard NMS + tta flip', None, 'flip'),
               ('hard NMS + tta flip + voting %.2f' % args.vote, args.vote, 'flip')]
    held_out = scenes.SceneBatches(batch, size, size, classes=T.CLASSES, seed=args.seed, device='cuda', start=T.HELD_OUT_START)
    all_targets, dets = [], {name: [] for name, _, _ in configs}
    for step in range(args.images // batch):
        x, targets = held_out.batch_at(step)
        x = x.contiguous(memory_format=torch.channels_last)
        ids = torch.arange(step * batch, (step + 1) * batch)
        all_targets.append(targets.cpu())
        for name, model.box_voting, model.tta in configs:
            with torch.no_grad():
                s, b, c = model(x)
            dets[name].extend(detections_to_coco(s.float().cpu(), b.float().cpu(), c.float().cpu(), ids, torch.ones(batch)))
    truth = CocoIndex(dataset=scenes.coco_ground_truth(torch.cat(all_targets), 0, T.CLASSES))
    print('%-40s %8s %8s %8s   detections (objects: %d)' % ('', 'AP', 'AP50', 'AP75', len(truth.dataset['annotations'])))
    for name, found in dets.items():
        ev = COCOeval(truth, truth.loadRes(found), 'bbox')
        ev.evaluate()
        ev.accumulate()
        stats = [float(v) for v in ev.summarize(out=lambda text: None)]
        print('%-40s %8.4f %8.4f %8.4f   %d' % (name, stats[0], stats[1], stats[2], len(found)))


if args.ap:
    trained_ap()
    sys.exit(0)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    total, n = _C.profile_collect()['nms_kernel']
    assert n == 1, n
    return total * 1e3


def line(name, v, base=None, unit='us'):
    v = sorted(v)
    med = statistics.median(v)
    print('  %-44s median %7.1f %s  (min %7.1f, p90 %7.1f)%s' % (name, med, unit, v[0], v[int(0.9 * (len(v) - 1))],
                                                                 '  x %.2f of the NMS launch' % (med / base) if base else ''))
    return med


def measure(name, scores, boxes, classes, nms, det):
    kept = _C.nms(scores, boxes, classes, nms, det, return_indices=True)[3]
    width = 1280
    launches = {'nms (odtk_nms_ex, with positions)': lambda: _C.nms(scores, boxes, classes, nms, det, return_indices=True),
                'box_vote_kernel': lambda: _C.box_vote(scores, boxes, classes, kept, args.vote),
                'concat_candidates_kernel (2 x this list)': lambda: _C.concat_candidates([(scores, boxes, classes)] * 2, [0, width])}
    for fn in launches.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    _C.profile_enable(True, ('nms_kernel',))
    _C.profile_collect()
    us = {k: [] for k in launches}
    for _ in range(args.iters):
        for k, fn in launches.items():
            us[k].append(timed(fn))
    _C.profile_enable(False)
    ref = box_vote_ref.vote_ref(*[t.cpu().numpy() for t in (scores, boxes, classes)], kept.cpu().numpy(), args.vote)
    used = kept.cpu().numpy() >= 0
    voters = ref[2][used]
    positive = (scores > 0).sum(1)
    print('== %s: %d images x %d candidates (%d..%d positive), %d detections (%d kept in all), nms %.2f, vote %.2f, %d launches each'
          % (name, scores.shape[0], scores.shape[1], int(positive.min()), int(positive.max()), det, int(used.sum()), nms, args.vote, args.iters))
    print('  voters per kept detection: mean %.1f, max %d; pairs examined per launch: %d' % (voters.mean(), voters.max(), int(used.sum()) * scores.shape[1]))
    base = None
    for k, v in us.items():
        med = line(k, v, base)
        base = base or med


def device(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


for count in (5000, 10000):
    measure('clustered', *device(box_vote_ref.clustered_case(7, 8, count, 80, 60, extent=512.0)), 0.5, 100)
measure('trained', *device(box_vote_ref.trained_candidates(os.path.join(ROOT, 'tests', 'golden'))), 0.5, 100)

if not args.skip_model:
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

    def stream_timed(fn, iters):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
        return out

    print('== box.detect on the bench heads (ResNet50FPN, batch 8, 800 x 1280, bf16, 5 x 1000 candidates per image), stream events')
    common = (cls_heads, box_heads, strides, model.anchors, model.threshold, model.top_n, model.nms, model.detections)
    plain = line('detect (odtk_detect: 3 launches)', stream_timed(lambda: box.detect(*common, logits=True), args.iters))
    voted = line('detect, vote=%.2f (4 launches)' % args.vote, stream_timed(lambda: box.detect(*common, logits=True, vote=args.vote), args.iters))
    print('  difference %.1f us per batch' % (voted - plain))
    del cls_heads, box_heads

    engine = model.inference_engine(torch.bfloat16)
    plan = os.path.join(ROOT, 'plans', 'rn50fpn_bf16_bs8_800x1280.json')
    if engine is not None and os.path.isfile(plan):
        engine.load_plan(json.load(open(plan)))

    def forward():
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            return model(x)
    print('== Model.forward through the engine, same input, stream events, %d calls each' % max(10, args.iters // 5))
    base = line('default', [v / 1e3 for v in stream_timed(forward, max(10, args.iters // 5))], unit='ms')
    model.tta = 'flip'
    tta = line("tta = 'flip'", [v / 1e3 for v in stream_timed(forward, max(10, args.iters // 5))], unit='ms')
    model.box_voting = args.vote
    both = line("tta = 'flip', box_voting = %.2f" % args.vote, [v / 1e3 for v in stream_timed(forward, max(10, args.iters // 5))], unit='ms')
    print('  tta / default = %.2f, tta + voting / default = %.2f' % (tta / base, both / base))
