#!/usr/bin/env python
"""What the IoU-family box loss (csrc/box_iou_loss.hpp; `Model.box_loss`) costs in a training step: its forward (the walk over one
lane per anchor cell + the fixed-order sum, two launches) and its backward (one launch), for each kind, next to the existing loss
launches (focal + smooth-L1, csrc/loss.hpp) on the same heads and targets.  Every launch is timed by the library's own event pair
around the dispatch (odtk_profile_*), the candidates alternating call by call after a warm-up, the median of `--iters` calls each.

Workload: the pyramid of an 800 x 1280 image (strides 8..128: 100 x 160 down to 7 x 10 cells), 9 anchors, 80 classes, the batch
of `bench.py --mode train` (2 images), targets from odtk_snap_to_anchors_levels with 8 and 64 boxes per image, predictions =
targets + N(0, 0.15), fp32 and bf16 heads as the convolutions write them (channels_last).

The smooth-L1 share of the existing forward launch is the difference between that launch with and without its box-delta workgroups;
the form without them exists only in the ablation build of the library (make -C retinanet-examples_amd/csrc ablations):
    ODTK_HIP_LIBRARY=build_ablate/libodtk_hip.so python tools/box_iou_loss_probe.py --smooth-l1-share

`--ap` instead trains the synthetic detector of tools/trained_ap.py (tests/test_gpu_trained_ap.py: ResNet18FPN on odtk/scenes.py) once
per box loss from the same seed and scores it on the same held-out scenes with the reference's post-processing: a record, not a test.

    python tools/box_iou_loss_probe.py [--iters 100] [--step-ms 34.4]
    python tools/box_iou_loss_probe.py --ap [--ap-iterations 1500] [--ap-seeds 0] [--ap-losses smooth_l1:1 giou:2]
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
ap.add_argument('--step-ms', type=float, default=34.4, help='the fp32 training step the cost is set against')
ap.add_argument('--smooth-l1-share', action='store_true', help='only the existing fp32 forward with and without its box-delta walk '
                '(needs the ablation build of the library)')
ap.add_argument('--ap', action='store_true', help='only the trained-AP comparison of the box losses')
ap.add_argument('--ap-iterations', type=int, default=1500)
ap.add_argument('--ap-images', type=int, default=128)
ap.add_argument('--ap-seeds', type=int, nargs='+', default=[0])
ap.add_argument('--ap-losses', nargs='+', default=['smooth_l1:1', 'giou:2'], help='box_loss:box_loss_weight, one training each')
args = ap.parse_args()
assert args.iters >= 50

HEIGHT, WIDTH, CLASSES = 800, 1280, 80
STRIDES = [8, 16, 32, 64, 128]
SIZES = [((HEIGHT + s - 1) // s, (WIDTH + s - 1) // s) for s in STRIDES]
ANCHORS = [box.generate_anchors(s, [1.0, 2.0, 0.5], [4 * 2 ** (i / 3) for i in range(3)]) for s in STRIDES]
NAMES = ('retina_loss_kernel', 'loss_reduce_kernel')     # ODTK_KERNEL_LOSS / ODTK_KERNEL_LOSS_REDUCE: both losses' launches


def say(*a):
    print(*a, flush=True)


def collect():
    torch.cuda.synchronize()
    got = _C.profile_collect()
    return {k: got[k] for k in NAMES}


def workload(boxes, dtype):
    source = T.SyntheticBatches(args.batch, HEIGHT, WIDTH, classes=CLASSES, max_boxes=boxes, seed=boxes)
    _, targets = source.batch()
    targets[:, :, :] = torch.cat([source.batch()[1][:, :1] for _ in range(boxes)], 1)      # every row a box: `boxes` per image
    targets = targets.cuda()
    assert int((targets[:, :, 4] > -1).sum()) == args.batch * boxes
    _, box_targets, depths = box.snap_to_anchors_levels(targets, SIZES, STRIDES, ANCHORS, CLASSES, [0.4, 0.5], want_cls_target=False)
    g = torch.Generator(device='cuda').manual_seed(boxes)
    box_heads = [(bt.reshape(args.batch, -1, *bt.shape[-2:]) + torch.randn(args.batch, bt.shape[1] * 4, *bt.shape[-2:], device='cuda', generator=g)
                  * 0.15).to(dtype).contiguous(memory_format=torch.channels_last) for bt in box_targets]
    cls_heads = [(torch.randn(args.batch, 9 * CLASSES, h, w, device='cuda', generator=g) * 1.5 - 4.0).to(dtype)
                 .contiguous(memory_format=torch.channels_last) for h, w in SIZES]
    return cls_heads, box_heads, depths, box_targets


def median_us(samples):
    v = sorted(samples)
    return statistics.median(v), v[0], v[int(0.9 * (len(v) - 1))]


def line(name, samples, extra=''):
    med, lo, p90 = median_us(samples)
    say('  %-34s median %7.1f us  (min %7.1f, p90 %7.1f)  = %.3f %% of a %.1f ms step%s' % (
        name, med, lo, p90, med / (args.step_ms * 1e3) * 100, args.step_ms, extra))
    return med


if args.ap:
    import time
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gpu_trained_ap as TA
    from odtk.model import Model
    say('COCO AP (IoU 0.50:0.95 | 0.50 | 0.75) against the true boxes of %d held-out scenes, fp32 eager graph + the reference\'s post-processing; '
        'ResNet18FPN trained %d iterations x batch 16 at 512x512 by odtk/train.py (fp32, HIP target assignment + fused loss), one training '
        'per box loss and seed' % (args.ap_images, args.ap_iterations))
    for seed in args.ap_seeds:
        for spec in args.ap_losses:
            kind, _, weight = spec.partition(':')

            def make(*a, kind=kind, weight=float(weight or 1), **k):
                model = Model(*a, **k)
                if kind != 'smooth_l1':
                    model.box_loss, model.box_loss_weight = kind, weight
                return model
            TA.Model = make                                  # train_detector builds its model itself
            t0 = time.time()
            model, history = TA.train_detector(seed=seed, iterations=args.ap_iterations, log_interval=max(50, args.ap_iterations // 10))
            TA.Model = Model
            t_train = time.time() - t0
            stats = TA.evaluate_paths(model, seed=seed, images=args.ap_images, with_gpu_paths=False)['reference']
            say('seed %d  %-12s AP %.4f | %.4f | %.4f   trained in %.0f s; loss (iteration, focal, box): %s' % (
                seed, spec, stats[0], stats[1], stats[2], t_train, '  '.join('%d: %.3f / %.3f' % (h[0], h[1], h[2]) for h in history[-3:])))
    raise SystemExit(0)

say('pyramid %s, batch %d, 9 anchors, %d classes, %d calls each' % (SIZES, args.batch, CLASSES, args.iters))

if args.smooth_l1_share:
    if _C.library().odtk_debug_loss_form(6) != 0:
        raise SystemExit('this library has no ablation forms: build it with `make -C retinanet-examples_amd/csrc ablations` and point '
                         'ODTK_HIP_LIBRARY at build_ablate/libodtk_hip.so')
    _C.loss_form(1)
    # forms 2..7 run four vectors per trip: the same launch shape for the whole kernel
    _C._check(_C.library().odtk_debug_loss_tuning(2, 1, 256, 4, 4, 256), 'loss_tuning')
    for boxes in (8, 64):
        cls_heads, box_heads, depths, box_targets = workload(boxes, torch.float32)
        fg = sum(int((d > 0).sum()) for d in depths)
        runs = {'whole launch (form 1)': 1, 'without the box-delta walk (form 6)': 6, 'without the logit walk (form 7)': 7}
        for form in runs.values():
            _C.loss_form(form)
            for _ in range(5):
                _C.retina_loss_levels_forward(cls_heads, box_heads, depths, box_targets, 0.25, 2.0, 0.11, reproducible=True)
        _C.profile_enable(True, NAMES)
        collect()
        us = {k: [] for k in runs}
        for _ in range(args.iters):
            for name, form in runs.items():
                _C.loss_form(form)
                _C.retina_loss_levels_forward(cls_heads, box_heads, depths, box_targets, 0.25, 2.0, 0.11, reproducible=True)
                got = collect()
                assert got['retina_loss_kernel'][1] == 1
                us[name].append(got['retina_loss_kernel'][0] * 1e3)
        _C.profile_enable(False)
        _C.loss_form(1)
        say('== %d boxes per image (%d foreground anchors), fp32 heads: the existing forward launch (focal + smooth-L1), four vectors per trip' % (boxes, fg))
        med = {name: line(name, v) for name, v in us.items()}
        say('  smooth-L1 share of the launch: %.1f us (whole - without the box-delta walk); the box-delta walk alone: %.1f us' % (
            med['whole launch (form 1)'] - med['without the box-delta walk (form 6)'], med['without the logit walk (form 7)']))
    raise SystemExit(0)

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
        for kind in ('iou', 'giou', 'diou'):
            calls[kind + ' forward'] = lambda kind=kind: _C.box_iou_loss_levels_forward(box_heads, depths, box_targets, ANCHORS, kind)
            calls[kind + ' backward'] = lambda kind=kind: _C.box_iou_loss_levels_backward(box_heads, depths, box_targets, ANCHORS, kind, g_levels)
        for fn in calls.values():
            for _ in range(5):
                fn()
        values = {kind: _C.box_iou_loss_levels_forward(box_heads, depths, box_targets, ANCHORS, kind).cpu() for kind in ('iou', 'giou', 'diou')}
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
        say('  mean loss per foreground anchor: smooth-L1 %.4f (sum over 4 deltas), iou %.4f, giou %.4f, diou %.4f' % (
            float(smooth[:, 1].sum()) / max(fg, 1), *[float(values[k][:, 0].sum()) / max(fg, 1) for k in ('iou', 'giou', 'diou')]))
        total = {}
        for name in calls:
            med = line(name + (' (walk)' if name in reduce else ''), walk[name])
            if name in reduce:
                med += line(name + ' (sum launch)', reduce[name])
            total[name] = med
        for kind in ('iou', 'giou', 'diou'):
            both = total[kind + ' forward'] + total[kind + ' backward']
            existing = total['focal + smooth-L1 forward'] + total['focal + smooth-L1 backward']
            say('  %-4s forward + backward %.1f us = %.3f %% of a %.1f ms step; the existing loss launches, which keep running: %.1f us' % (
                kind, both, both / (args.step_ms * 1e3) * 100, args.step_ms, existing))
