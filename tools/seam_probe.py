"""Probe of the bottleneck seam (csrc/seam.hpp) at the flagship shape: one `odtk_bottleneck_seam` call against the two
`odtk_gemm_bias_act` calls it replaces, back to back on the same buffers.

    python tools/seam_probe.py [--batch 8 --height 200 --width 320] [--calls 100] [--dtype bf16]

Per N2 (64: layer1's inner seams, 128: the hand-over to layer2.0): the median of `--calls` event-timed calls of each side, the
algorithmic bytes each moves (every tensor once; the pair reads `out` back) and the bytes/s that makes, plus how many elements of
the two results differ (both are correct roundings of fp32 sums taken in different orders).  The record of a run lives in
profiles/bottleneck_seam_probe.txt."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'retinanet-examples_amd'))
from odtk import _C  # noqa: E402


def median_us(fn, calls):
    for _ in range(5):
        fn()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=200)
    ap.add_argument('--width', type=int, default=320)
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16'])
    args = ap.parse_args()
    dtype = {'bf16': torch.bfloat16, 'fp16': torch.float16}[args.dtype]
    b, h, w = args.batch, args.height, args.width
    m, size = b * h * w, torch.finfo(dtype).bits // 8
    g = torch.Generator().manual_seed(3)
    cl = lambda t: t.to(dtype).cuda().contiguous(memory_format=torch.channels_last)
    y2, skip = cl(torch.randn(b, 64, h, w, generator=g)), cl(torch.randn(b, 256, h, w, generator=g))
    w3, b3 = cl(torch.randn(256, 64, 1, 1, generator=g) / 8), torch.randn(256, generator=g).cuda()
    print('%s on %s: M = %d pixels, %s, medians of %d calls (min .. max)' % (os.path.basename(__file__), torch.cuda.get_device_name(0), m,
                                                                          args.dtype, args.calls))
    for n2 in (64, 128):
        w1, b1 = cl(torch.randn(n2, 256, 1, 1, generator=g) / 16), torch.randn(n2, generator=g).cuda()
        pair = lambda: _C.gemm_bias_act(_C.gemm_bias_act(y2, w3, b3, skip, True), w1, b1, None, True)
        first = lambda: _C.gemm_bias_act(y2, w3, b3, skip, True)
        seam = lambda: _C.bottleneck_seam(y2, skip, w3, b3, w1, b1)
        out_pair = _C.gemm_bias_act(y2, w3, b3, skip, True)
        z_pair = _C.gemm_bias_act(out_pair, w1, b1, None, True)
        out_seam, z_seam = seam()
        torch.cuda.synchronize()
        bytes_seam = m * size * (64 + 256 + 256 + n2)
        bytes_pair = bytes_seam + m * size * 256
        rows = [('seam kernel', median_us(seam, args.calls), bytes_seam), ('two GEMMs', median_us(pair, args.calls), bytes_pair),
                ('  (first GEMM alone)', median_us(first, args.calls), m * size * (64 + 256 + 256))]
        # the dispatches' own begin / end stamps (odtk_profile_*: what a kernel trace reports), without the launch gaps
        stamps = {}
        for name, fn, kernel in (('seam', seam, 'bottleneck_seam_kernel'), ('pair', pair, 'gemm_bias_act')):
            _C.profile_collect()
            _C.profile_enable(True, [kernel])
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            ms, launches = _C.profile_collect()[kernel]
            _C.profile_enable(False)
            stamps[name] = ms * 1e3 / 20
        print('N2 = %d' % n2)
        for name, (med, lo, hi), nbytes in rows:
            print('  %-22s %8.1f us (%.1f .. %.1f)   %7.1f MB   %5.2f TB/s' % (name, med, lo, hi, nbytes / 1e6, nbytes / med / 1e6))
        print('  dispatch stamps, mean of 20: seam %.1f us (%.2f TB/s), pair %.1f us (%.2f TB/s)' % (
            stamps['seam'], bytes_seam / stamps['seam'] / 1e6, stamps['pair'], bytes_pair / stamps['pair'] / 1e6))
        print('  seam / pair = %.3f;  elements differing: out %d of %d (max %.3g), z %d of %d (max %.3g)' % (
            rows[0][1][0] / rows[1][1][0], int((out_seam != out_pair).sum()), out_seam.numel(),
            (out_seam.float() - out_pair.float()).abs().max().item(), int((z_seam != z_pair).sum()), z_seam.numel(),
            (z_seam.float() - z_pair.float()).abs().max().item()))


if __name__ == '__main__':
    main()
