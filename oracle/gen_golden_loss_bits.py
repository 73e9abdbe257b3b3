"""Raw bits of the per-anchor-cell loss families (IoU / GIoU / DIoU, ProbIoU / KLD, quality focal / varifocal) as the GPU
computes them: every `sums` tensor and every gradient tensor of odtk._C.*_loss_levels_forward / _backward on one seeded input
set, stored byte by byte in tests/golden/loss_family_bits.npz.  Both passes are deterministic by construction (no atomics, one
fixed summation order), so a refactor of the kernels, of their host drivers or of the ctypes layer has to reproduce the file
exactly: tests/test_gpu_loss_family_bits.py regenerates the inputs from the seed and compares with no tolerance.

Only the public functions of odtk._C are driven, so the script runs unchanged before and after such a refactor.  Needs a GPU:
    python oracle/gen_golden_loss_bits.py [--out tests/golden/loss_family_bits.npz]

The inputs are the smallest that take every path: batch 2, A = 3 (no power of two); two levels of 7 x 9 and 2 x 3 cells, i.e.
378 anchor cells (two workgroups of 256, the second partial) and 36, with a level boundary inside the grid; C = 5 classes, so that
fp32 (4 per vector) and 16-bit (8 per vector) vectors straddle class and pixel boundaries and the element counts 1890 and 180 leave
a scalar tail; about a quarter of the anchors foreground, some ignored (-1), and the second image of the second level without any
foreground; every kind, float32 / bfloat16 / float16 heads, NCHW and channels_last; gamma = 2 (the plain-vector route) and 1.5;
an upstream gradient per level, and None (all gradients +0)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'retinanet-examples_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SEED = 20261020
BATCH, ANCHORS, CLASSES = 2, 3, 5
SIZES = ((7, 9), (2, 3))
# [A, 4] anchor tables (x1, y1, x2, y2) of the two levels: ratios 1, 2, 0.5 at strides 8 and 32
ANCHOR_TABLES = ([[-16.0, -16.0, 15.0, 15.0], [-11.5, -22.5, 10.5, 21.5], [-22.5, -11.5, 21.5, 10.5]],
                 [[-64.0, -64.0, 63.0, 63.0], [-45.5, -90.5, 44.5, 89.5], [-90.5, -45.5, 89.5, 44.5]])
DTYPES = (('fp32', torch.float32), ('bf16', torch.bfloat16), ('fp16', torch.float16))
LAYOUTS = (('nchw', False), ('nhwc', True))
UPSTREAM = (0.37, -1.9)
QUALITY_ALPHA = 0.75
QUALITY_GAMMAS = (2.0, 1.5)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'loss_family_bits.npz')


def inputs():
    """-> float32 CPU tensors: depths, and per family the targets and the heads (before the cast to the head dtype)."""
    rng = np.random.RandomState(SEED)
    depths, targets4, targets6, box4, box6, logits = [], [], [], [], [], []
    for level, (h, w) in enumerate(SIZES):
        shape = (BATCH, ANCHORS, 1, h, w)
        role = rng.randint(0, 8, size=shape)                       # 0, 1: foreground; 2: ignored; else background
        depth = np.where(role < 2, rng.randint(1, CLASSES + 1, size=shape), np.where(role == 2, -1, 0)).astype(np.float32)
        if level == 1:
            depth[1] = np.minimum(depth[1], 0.0)                   # the second image: no foreground at all
        t4 = (rng.standard_normal((BATCH, ANCHORS, 4, h, w)) * 0.3).astype(np.float32)
        p4 = t4 + (rng.standard_normal(t4.shape) * 0.15).astype(np.float32)
        p4[:, ::2, 2, :, ::3] = 4.75                               # widths beyond the clip
        angle = rng.uniform(-np.pi, np.pi, size=(BATCH, ANCHORS, 1, h, w))
        t6 = np.concatenate([t4, np.sin(angle), np.cos(angle)], axis=2).astype(np.float32)
        p6 = t6 + (rng.standard_normal(t6.shape) * 0.15).astype(np.float32)
        p6[:, 1, 3, ::2] = 4.75                                    # heights beyond the clip
        x = (rng.standard_normal((BATCH, ANCHORS, CLASSES, h, w)) * 2 - 3).astype(np.float32)
        flat = x.reshape(-1)
        special = np.array([63.5, 64.5, 30.0, -30.0, 100.0, -100.0], dtype=np.float32)   # either side of the plain-vector limit
        at = np.linspace(0, flat.size - 1, 12).astype(np.int64)
        flat[at] = special[np.arange(at.size) % special.size]
        depths.append(torch.from_numpy(depth))
        targets4.append(torch.from_numpy(t4))
        targets6.append(torch.from_numpy(t6))
        box4.append(torch.from_numpy(p4.reshape(BATCH, ANCHORS * 4, h, w)))
        box6.append(torch.from_numpy(p6.reshape(BATCH, ANCHORS * 6, h, w)))
        logits.append(torch.from_numpy(x.reshape(BATCH, ANCHORS * CLASSES, h, w)))
    return depths, targets4, targets6, box4, box6, logits


def _heads(tensors, dtype, channels_last):
    out = [t.cuda().to(dtype) for t in tensors]
    return [t.contiguous(memory_format=torch.channels_last) for t in out] if channels_last else out


def _bits(t):
    """The tensor's values in logical order, byte by byte."""
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().copy()


def compute():
    """-> {name: uint8 array} of every sums and gradient tensor.  Needs a GPU."""
    from odtk import _C
    depths, targets4, targets6, box4, box6, logits = inputs()
    depths = [d.cuda() for d in depths]
    targets4, targets6 = [t.cuda() for t in targets4], [t.cuda() for t in targets6]
    anchors = [torch.tensor(t) for t in ANCHOR_TABLES]
    upstream = torch.tensor(UPSTREAM, dtype=torch.float32, device='cuda')
    out = {}

    def record(name, sums, backward):
        out[name + '.sums'] = _bits(sums)
        for tag, g in (('up', upstream), ('none', None)):
            for level, grad in enumerate(backward(g)):
                out['%s.grad_%s.%d' % (name, tag, level)] = _bits(grad)

    for dname, dtype in DTYPES:
        for lname, channels_last in LAYOUTS:
            fmt = '%s.%s' % (dname, lname)
            b4, b6, cls = (_heads(t, dtype, channels_last) for t in (box4, box6, logits))
            for kind in _C.BOX_LOSS_KINDS:
                record('box_iou.%s.%s' % (kind, fmt), _C.box_iou_loss_levels_forward(b4, depths, targets4, anchors, kind),
                       lambda g, kind=kind: _C.box_iou_loss_levels_backward(b4, depths, targets4, anchors, kind, g))
            for kind in _C.ROTATED_BOX_LOSS_KINDS:
                record('rotated.%s.%s' % (kind, fmt), _C.rotated_box_loss_levels_forward(b6, depths, targets6, anchors, kind),
                       lambda g, kind=kind: _C.rotated_box_loss_levels_backward(b6, depths, targets6, anchors, kind, g))
            for kind in _C.CLS_LOSS_KINDS:
                for gamma in QUALITY_GAMMAS:
                    record('quality.%s.gamma%g.%s' % (kind, gamma, fmt),
                           _C.quality_loss_levels_forward(cls, b4, depths, targets4, anchors, kind, QUALITY_ALPHA, gamma),
                           lambda g, kind=kind, gamma=gamma: _C.quality_loss_levels_backward(cls, b4, depths, targets4, anchors, kind,
                                                                                             QUALITY_ALPHA, gamma, g))
    torch.cuda.synchronize()
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    parser.add_argument('--out', default=GOLDEN)
    args = parser.parse_args()
    arrays = compute()
    np.savez_compressed(args.out, **arrays)
    print('wrote %s: %d arrays, %d bytes of tensors' % (args.out, len(arrays), sum(a.size for a in arrays.values())))


if __name__ == '__main__':
    main()
