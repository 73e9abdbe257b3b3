"""Go / no-go probe of the head towers' own 3x3 convolution kernel (csrc/tower_conv.hpp, `odtk_tower_conv3x3`) against the routes
the engine has today, on the same random tensors in one process:

    python tools/tower_conv_probe.py [--calls 100] [--blocks 10] [--dtype bf16] [--plan plans/rn50fpn_bf16_bs8_800x1280.json]

Arms, alternating in blocks of calls/blocks event-timed samples each (a sample = 4 launches back to back, divided by 4):
  own      `_C.tower_conv3x3` as shipped: the 32x32x16 form, whose sums follow the library's 256 x 256 x 32 instance; tile ids
           permuted so that workgroups sharing an L2 own consecutive tiles
  own-lin  the same, workgroup k owns tile k (odtk_debug_tower_conv_variant(0))
  own-16   the 16x16x32 form (odtk_debug_tower_conv_variant(3)): 32 consecutive k per MFMA
  library  `_C.conv_bias_act` on the instance the committed plan pins for the problem (its conv lines are imported first; a
           problem the plan does not name is timed by the library itself at its first call, outside the measurement)
  miopen   F.conv2d + `_C.bias_act_` (the two-pass route)
Shapes: P3's tower layers 8 x 256 x 100 x 160 with ReLU and linear, the pyramid canvas 8 x 256 x 50 x 121, and -- for the
engine's pixel threshold -- P4 and P5 on their own (8 x 256 x 50 x 80, 8 x 256 x 25 x 40: 125 and 32 tiles).
Per arm: median, min .. max of all calls, the fastest and the slowest block median, TFLOP/s of the median.  The rule: a shape is
routed to the own kernel only if its SLOWEST block is faster than the FASTEST block of every other arm.  Random operands (the
chip clocks higher on zeros).  The record of a run lives in profiles/tower_conv_probe.txt."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'retinanet-examples_amd'))
from odtk import _C  # noqa: E402


REPS = 4   # launches per event pair: the queue stays filled, so a sample is kernel time and not the host's launch gap


def timed(fn, calls):
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / REPS)
    return times


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--blocks', type=int, default=10)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16'])
    ap.add_argument('--plan', default=os.path.join(ROOT, 'plans', 'rn50fpn_bf16_bs8_800x1280.json'))
    ap.add_argument('--shapes', default='8x100x160:1,8x100x160:0,8x50x121:1,8x50x80:1,8x25x40:1')
    args = ap.parse_args()
    dtype = {'bf16': torch.bfloat16, 'fp16': torch.float16}[args.dtype]
    lib = _C.library()
    if args.plan and _C.conv_available():
        with open(args.plan) as f:
            lines = [s for s in json.load(f).get('libraries', []) if s.startswith('conv ')]
        taken = _C.conv_library().odtk_conv_plan_import('\n'.join(lines).encode())
        print('plan %s: %d of %d conv lines taken' % (os.path.basename(args.plan), taken, len(lines)))
    print('%s on %s: %s, %d calls per arm in %d alternating blocks' % (os.path.basename(__file__), torch.cuda.get_device_name(0), args.dtype,
                                                                      args.calls, args.blocks))
    g = torch.Generator().manual_seed(11)
    cl = lambda t: t.to(dtype).cuda().contiguous(memory_format=torch.channels_last)
    wt = cl(torch.randn(256, 256, 3, 3, generator=g) * (2.0 / 2304) ** 0.5)
    bias32 = (torch.randn(256, generator=g) * 0.3).cuda()
    bias = bias32.to(dtype)
    per = max(1, args.calls // args.blocks)
    for spec in args.shapes.split(','):
        dims, relu = spec.split(':')
        b, h, w = (int(v) for v in dims.split('x'))
        relu = relu != '0'
        x = cl(torch.randn(b, 256, h, w, generator=g) * 0.5)
        m = b * h * w
        flop = 2.0 * m * 256 * 2304

        def own(variant):
            def run():
                return _C.tower_conv3x3(x, wt, bias, relu)

            def call():
                before = lib.odtk_debug_tower_conv_variant(variant)
                try:
                    return run()
                finally:
                    lib.odtk_debug_tower_conv_variant(before)
            return call

        arms = [('own', own(1)), ('own-lin', own(0)), ('own-16', own(3))]
        if _C.conv_available():
            arms.append(('library', lambda: _C.conv_bias_act(x, wt, bias, (1, 1), (1, 1), relu)))
        arms.append(('miopen', lambda: _C.bias_act_(F.conv2d(x, wt, None, 1, 1), bias32, None, relu)))
        outs = {}
        for name, fn in arms:                                            # warm-up (the library may time its instances here)
            for _ in range(3):
                outs[name] = fn()
        torch.cuda.synchronize()
        plan = _C.conv_last_plan() if _C.conv_available() else ''
        times = {name: [] for name, _ in arms}
        for _ in range(args.blocks):
            for name, fn in arms:
                times[name].append(timed(fn, per))
        print('%d x 256 x %d x %d, %s: M = %d = %d tiles, %.1f GFLOP%s' % (b, h, w, 'ReLU' if relu else 'linear', m, (m + 255) // 256, flop / 1e9,
                                                                           ('; library instance ' + plan.split(' ', 2)[0]) if plan else ''))
        stats = {}
        for name, _ in arms:
            flat = [t for blk in times[name] for t in blk]
            meds = [median(blk) for blk in times[name]]
            stats[name] = (median(flat), min(flat), max(flat), min(meds), max(meds))
            print('  %-8s median %7.1f us (%.1f .. %.1f)   blocks %.1f .. %.1f   %6.0f TFLOP/s' % ((name,) + stats[name] + (flop / stats[name][0] / 1e6,)))
        for name in ('own', 'own-lin', 'own-16'):
            others = [stats[o][3] for o, _ in arms if not o.startswith('own')]
            print('  %-8s slowest block %.1f us vs the other arms\' fastest block %.1f us: %s' % (
                name, stats[name][4], min(others), 'GO' if stats[name][4] < min(others) else 'no-go'))
        ref = outs['own'].float()
        for name in outs:
            if name != 'own':
                d = (outs[name].float() - ref).abs()
                print('  own vs %-8s %d of %d elements differ, max |diff| %.3g' % (name, int((d != 0).sum()), d.numel(), float(d.max())))


if __name__ == '__main__':
    main()
