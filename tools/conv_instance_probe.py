#!/usr/bin/env python
"""Every instance of libodtk_conv.so's list on ONE problem: time and name, fastest first (ODTK_CONV_INSTANCE forces an instance).
Next to it: the MIOpen convolution alone and MIOpen + odtk_bias_act on the same tensors.  --check: also whether each instance's
output on the integer-valued inputs of oracle/conv_exact.py equals the float64 reference bit for bit (exact / WRONG n elements).

    python tools/conv_instance_probe.py [--shape 8 256 100 160 256 3 1 1] [--top 12] [--check]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]
import torch
import torch.nn.functional as F
from odtk import _C
from oracle import conv_exact

ap = argparse.ArgumentParser()
ap.add_argument('--shape', type=int, nargs=8, default=[8, 256, 100, 160, 256, 3, 1, 1], help='batch c_in h w c_out k stride pad')
ap.add_argument('--top', type=int, default=12)
ap.add_argument('--dtype', default='bf16')
ap.add_argument('--check', action='store_true', help='compare every instance with the exact float64 reference (CPU: slow on large shapes)')
a = ap.parse_args()
b, c, h, w, k, ks, stride, pad = a.shape
dtype = {'bf16': torch.bfloat16, 'fp16': torch.float16}[a.dtype]
torch.backends.cudnn.benchmark = True
g = torch.Generator().manual_seed(0)
x = (torch.randn(b, c, h, w, generator=g) * 0.5).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
wt = (torch.randn(k, c, ks, ks, generator=g) * 0.05).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
bias = torch.randn(k, generator=g).to(dtype).cuda()
bias32 = bias.float()


def timed(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


for _ in range(3):
    F.conv2d(x, wt, None, stride, pad)
t_conv = timed(lambda: F.conv2d(x, wt, None, stride, pad))
t_two = timed(lambda: _C.bias_act_(F.conv2d(x, wt, None, stride, pad), bias32, None, True))
print('problem %s %s: MIOpen convolution alone %.1f us, + odtk_bias_act %.1f us' % (a.shape, a.dtype, t_conv, t_two))
n = _C.conv_library().odtk_conv_instance_count(_C._DTYPES[dtype])
if a.check:                                      # the exact problem of this shape: same tensors for every instance
    cls = (c, k, ks, ks, stride, stride, pad, pad, pad, pad)
    ex, ew, eb, pre = conv_exact.exact_problem(cls, (b, h, w))
    ex, ew = (t.to(dtype).cuda().contiguous(memory_format=torch.channels_last) for t in (ex, ew))
    eb, ref = eb.to(dtype).cuda(), pre.clamp(min=0).to(dtype).cuda()
rows = []
for i in range(n):
    os.environ['ODTK_CONV_INSTANCE'] = str(i)
    try:
        t = timed(lambda: _C.conv_bias_act(x, wt, bias, stride, pad, True), reps=5)
    except RuntimeError:
        continue
    verdict = ''
    if a.check:
        wrong = int((_C.conv_bias_act(ex, ew, eb, stride, pad, True).view(torch.int16) != ref.contiguous(memory_format=torch.channels_last).view(torch.int16)).sum())
        verdict = 'exact' if not wrong else 'WRONG %d' % wrong
    rows.append((t, i, _C.conv_last_plan().split(' ', 3)[-1], verdict))
os.environ.pop('ODTK_CONV_INSTANCE', None)
rows.sort()
print('%d of %d instances take the problem; fastest first:' % (len(rows), n))
for t, i, name, verdict in rows[:a.top]:
    print('%8.1f us  #%-3d %-10s %s' % (t, i, verdict, name))
if a.check:
    print('%d of %d accepting instances are exact' % (sum(r[3] == 'exact' for r in rows), len(rows)))
    for t, i, name, verdict in rows:
        if verdict != 'exact':
            print('  #%-3d %s %s' % (i, verdict, name))
