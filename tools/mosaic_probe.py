#!/usr/bin/env python
"""What the mosaic chain costs on the device (include/odtk_hip.h: odtk_mosaic_images; csrc/mosaic.hpp): a batch of 8 canvases of
1280 x 800, each composed of four 640 x 400 sources resized by 1.5 .. 2.1 (so every quadrant is full and every tile is cropped),
all four colour operations on -- next to the chain WITHOUT a mosaic on the same canvases (odtk_augment_images: 8 sources resized
to 1280 x 800, what the parent commit ran) and that chain with a free rotation of every image (odtk_augment_images_ex, pass R).
The three are timed in turns, round after round, in one process (events around `--iters` back-to-back calls); the per-pass
figures come from the same program under `rocprofv3 --kernel-trace --stats` (tools/rocpd_stats.py).

  python tools/mosaic_probe.py [--iters 100] [--rounds 5] [--batch 8]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]
import numpy as np
import torch

from odtk import _C
from odtk import data as D

W, H, SW, SH = 1280, 800, 640, 400
COLOUR = (15, 1.1, 0.9, 1.2, 5)


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters                   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: a timing from anywhere else says nothing'
    rng = np.random.default_rng(0)
    source = lambda: torch.from_numpy(rng.integers(0, 256, (SH, SW, 3), dtype=np.uint8))
    table = D.normalisation_table(torch.bfloat16).cuda()

    # the mosaic batch
    pixels, geometry = [], []
    for b in range(args.batch):
        centre = (W // 4 + (W // 2) * b // args.batch, H // 4 + (H // 2) * (args.batch - 1 - b) // args.batch)
        sizes = [(int((1.5 + 0.2 * k) * SW), int((1.5 + 0.2 * k) * SH)) for k in range(4)]
        tiles = tuple((k, k) + D.mosaic_placement(k, sizes[k][0], sizes[k][1], centre[0], centre[1], W, H) for k in range(4))
        pixels.append([source() for _ in range(4)])
        geometry.append(D.MosaicGeometry(W, H, tuple(s + ((b + k) % 2,) for k, s in enumerate(sizes)), tiles, *COLOUR))
    mosaic = D.SourceBatch(D.SourceBatch.pack(pixels, geometry, 128))
    mosaic_up = mosaic.buffer.cuda()
    m_images = (_C.Image * len(mosaic.images)).from_buffer_copy(mosaic.images.tobytes())
    m_records = (_C.Mosaic * mosaic.batch).from_buffer_copy(mosaic.mosaics.tobytes())
    m_augments = (_C.Augment * mosaic.batch).from_buffer_copy(mosaic.augments.tobytes())
    run_mosaic = lambda: _C.mosaic_images(mosaic_up, m_images, m_records, m_augments, mosaic.tables(mosaic_up), table, mosaic.height, mosaic.width)

    # the same canvases without a mosaic (the parent's chain), and with a free rotation of every image (pass R)
    sources = [source() for _ in range(args.batch)]
    chains = {}
    for name, rotate in (('plain', False), ('rotated', True)):
        geometry = []
        for k in range(args.batch):
            cw, ch, coefficients = D.quarter_turn_map(W, H, 0, False, bool(k % 2) and not rotate)
            extra = (D.free_rotation_matrix(cw, ch, -30.0 + 60.0 * (k + 0.5) / args.batch), k % 2) if rotate else ()
            geometry.append((W, H, 0, cw, ch, coefficients) + COLOUR + extra)
        batch = D.SourceBatch(D.SourceBatch.pack(sources, geometry, 128))
        up = batch.buffer.cuda()
        images = (_C.Image * batch.batch).from_buffer_copy(batch.images.tobytes())
        augments = (_C.Augment * batch.batch).from_buffer_copy(batch.augments.tobytes())
        rotations = (_C.Rotation * batch.batch).from_buffer_copy(batch.rotations.tobytes()) if rotate else None
        chains[name] = (lambda up=up, images=images, augments=augments, rotations=rotations, batch=batch:
                        _C.augment_images(up, images, augments, batch.tables(up), table, batch.height, batch.width, rotations=rotations))
    runs = {'odtk_augment_images (no mosaic, the parent\'s chain)': chains['plain'], 'odtk_mosaic_images (4 sources per canvas)': run_mosaic,
            'odtk_augment_images_ex (free rotation of every image)': chains['rotated']}
    out = run_mosaic()
    print('batch %s bfloat16, canvases %d x %d; mosaic: %d sources of %d x %d resized by 1.5 .. 2.1; %d calls per timing, %d rounds in turns'
          % (list(out.shape), W, H, len(mosaic.images), SW, SH, args.iters, args.rounds))
    times = {name: [] for name in runs}
    for _ in range(args.rounds):
        for name, fn in runs.items():
            times[name].append(timed(fn, args.iters))
    for name, t in times.items():
        print('%-58s median %.1f us per batch (min %.1f, max %.1f)' % (name, statistics.median(t), min(t), max(t)))
    print('pass M moves %d bytes per batch (3 H W read + written per image) -> %.1f us at 8 TB/s' % (2 * 3 * W * H * args.batch, 2 * 3 * W * H * args.batch / 8e12 * 1e6))


if __name__ == '__main__':
    main()
