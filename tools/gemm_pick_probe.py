#!/usr/bin/env python
"""Does the agreement of the bottleneck seam with the two GEMMs it replaces depend on WHICH hipBLASLt solution runs them?

At the shapes of tests/test_gpu_bottleneck_seam.py::test_engine_seam_path_matches_the_two_gemm_graph (2 x 32 x 32 pixels, layer1:
64 -> 256 -> 64 | 128, bf16, real-valued inputs) every candidate the heuristic offers for each of the two GEMMs is forced in turn
(odtk_gemm_plan_clear + one imported line, as tests/test_gpu_gemm_solutions.py does) and its output compared with the seam
kernel's: the number of differing elements per solution, and which solution the stopwatch picks in this process.  Every
candidate is a correct fp32 sum rounded once; the ones that add up in another order than the seam kernel round a few elements
to the neighbouring bf16 value.  Record: profiles/gemm_seam_pick_probe.txt.

    python tools/gemm_pick_probe.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]

import torch  # noqa: E402

from odtk import _C  # noqa: E402


def main():
    g = torch.Generator().manual_seed(11)
    b, h, w = 2, 32, 32
    m = b * h * w
    cl = lambda t: t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    for n2 in (64, 128):
        y2, skip = cl(torch.randn(b, 64, h, w, generator=g)), cl(torch.randn(b, 256, h, w, generator=g) * 0.3)
        w3 = cl(torch.randn(256, 64, 1, 1, generator=g) * (0.3 * 64 ** -0.5))
        w1 = cl(torch.randn(n2, 256, 1, 1, generator=g) * 256 ** -0.5)
        b3, b1 = (torch.randn(256, generator=g) * 0.3).cuda(), (torch.randn(n2, generator=g) * 0.3).cuda()
        out, z = _C.bottleneck_seam(y2, skip, w3, b3, w1, b1)
        for name, ref, args, (n, k, res) in (('out', out, (y2, w3, b3, skip, True), (256, 64, 1)),
                                            ('z', z, (out, w1, b1, None, True), (n2, 256, 0))):
            rows = []
            for index in _C.gemm_candidates(m, n, k, torch.bfloat16, True, bool(res)):
                _C.gemm_plan_clear()
                assert _C.library().odtk_gemm_plan_import(('gemm %d %d %d 1 1 %d %d\n' % (m, n, k, res, index)).encode()) == 1
                got = _C.gemm_bias_act(*args)
                torch.cuda.synchronize()
                assert _C.gemm_last_solution() == (index, 'pinned')
                rows.append('%d:%d' % (index, int((got != ref).sum())))
            _C.gemm_plan_clear()
            _C.gemm_bias_act(*args)
            print('n2=%d %s [m=%d n=%d k=%d] elements differing from the seam per solution: %s; timed pick %d' % (
                n2, name, m, n, k, ' '.join(rows), _C.gemm_last_solution()[0]), flush=True)


if __name__ == '__main__':
    main()
