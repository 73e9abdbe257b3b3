#!/usr/bin/env python
"""Kernel time of the device-side input pipeline (odtk_preprocess_images, csrc/preprocess.hpp) on a COCO-shaped batch -- 8 images
of 640x480 -> 1066x800, which stride 128 pads to [8, 3, 896, 1152] -- next to its bound (algorithmic bytes: source pixels and
tables read once, the output written once, over the 8 TB/s HBM peak the other rooflines of this project use), and next to the
device stage it replaces: `normalise_batch` on the already resized [8, 896, 1152, 4] uint8 batch (a chain of torch operators that
does strictly less work: no resize).  Event-timed back to back; under `rocprofv3 --kernel-trace --stats` the same launches show
up as preprocess_images_kernel<2> / <4>.

`--augment` times the augmentation chain instead (odtk_augment_images, csrc/augment.hpp: resize to bytes, sum of L, gather + colour
chain + table + pad) on the same batch, with all five options on, next to the plain launch and to its own bound (source read, the
byte image written once and read twice, the output written).  It runs the chain with every image unturned, every image turned by
90 degrees (expand: the gather walks columns of the byte image) and with the loader's mix of turns.  With `--free-rotate` as well
it times odtk_augment_images_ex with EVERY image rotated by a free angle (one more pass: the finished canvas bytes written once
and read by the sum and the colour pass), each row next to the chain without the rotation in the same process; under
`rocprofv3 --kernel-trace --stats` the added pass shows up as augment_rotate_kernel next to preprocess_images_kernel<4, true>.

  python tools/device_resize_probe.py [--iters 200] [--batch 8] [--source 640x480] [--augment [--free-rotate]]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]
import numpy as np
import torch

from odtk import _C
from odtk import data as D

HBM_PEAK = 8.0e12


def timed(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters                   # us per call


def augment_probe(args, sources, ow, oh):
    colour = (15, 1.1, 0.9, 1.2, 5)
    plain = D.SourceBatch(D.SourceBatch.pack(sources, [(ow, oh, k % 2) for k in range(args.batch)], 128))
    plain_up = plain.buffer.cuda()
    plain_images = (_C.Image * plain.batch).from_buffer_copy(plain.images.tobytes())
    turns = {'no turn': lambda k: 0, 'all 90 degrees': lambda k: 90, 'mixed turns': lambda k: 90 * (k % 4)}
    for dtype in (torch.bfloat16, torch.float32):
        table = D.normalisation_table(dtype).cuda()
        us_plain = timed(lambda: _C.preprocess_images(plain_up, plain_images, plain.tables(plain_up), table, plain.height, plain.width), args.iters)
        print('%-8s preprocess_images (no augmentation) %.1f us per batch [%d, 3, %d, %d]' % (str(dtype).replace('torch.', ''), us_plain,
                                                                                             plain.batch, plain.height, plain.width))
        for colours, label in ((colour, 'five options'), ((0, 1.0, 1.0, 1.0, 0), 'turn and flip only')):
            for name, angle in turns.items():
                geometry = [(ow, oh, 0) + D.quarter_turn_map(ow, oh, angle(k), True, k % 2) + colours for k in range(args.batch)]
                batch = D.SourceBatch(D.SourceBatch.pack(sources, geometry, 128))
                uploaded = batch.buffer.cuda()
                images = (_C.Image * batch.batch).from_buffer_copy(batch.images.tobytes())
                augments = (_C.Augment * batch.batch).from_buffer_copy(batch.augments.tobytes())
                run = lambda: _C.augment_images(uploaded, images, augments, batch.tables(uploaded), table, batch.height, batch.width)
                out = run()
                if name == 'no turn' and not colours[0]:
                    assert torch.equal(out, _C.preprocess_images(plain_up, plain_images, plain.tables(plain_up), table, plain.height, plain.width))
                us = timed(run, args.iters)
                resized = 3 * ow * oh * args.batch
                moved = (sum(s.numel() for s in sources) + 4 * batch.tables_len + resized * (3 if colours[0] else 2) +
                         out.numel() * out.element_size() + table.numel() * table.element_size())
                bound = moved / HBM_PEAK * 1e6
                print('%-8s augment_images, %-18s %-14s [%d, 3, %d, %d]: %.1f us per batch (events, back to back, %d calls); algorithmic '
                      'bytes %d -> bound %.1f us at 8 TB/s (%.1f %% of that rate); %.2fx the plain launch'
                      % (str(dtype).replace('torch.', ''), label + ',', name, batch.batch, batch.height, batch.width, us, args.iters, moved,
                         bound, 100 * bound / us, us / us_plain))
                if not args.free_rotate:
                    continue
                # the same images, each rotated by its own angle between the turn and the flip
                geometry = []
                for k in range(args.batch):
                    cw, ch, coefficients = D.quarter_turn_map(ow, oh, angle(k), True, False)
                    geometry.append((ow, oh, 0, cw, ch, coefficients) + colours + (D.free_rotation_matrix(cw, ch, -30.0 + 60.0 * (k + 0.5) / args.batch), k % 2))
                rotated = D.SourceBatch(D.SourceBatch.pack(sources, geometry, 128))
                rotated_up = rotated.buffer.cuda()
                rotated_augments = (_C.Augment * rotated.batch).from_buffer_copy(rotated.augments.tobytes())
                rotations = (_C.Rotation * rotated.batch).from_buffer_copy(rotated.rotations.tobytes())
                run_rotated = lambda: _C.augment_images(rotated_up, images, rotated_augments, rotated.tables(rotated_up), table, rotated.height,
                                                        rotated.width, rotations=rotations)
                run_rotated()
                us_rotated = timed(run_rotated, args.iters)
                moved_rotated = moved + resized * 2                  # the canvas bytes written once, and the taps read
                print('%-8s   + free rotation of every image (-30 .. 30 degrees): %.1f us per batch, %.1f us more than the row above (%.2fx); '
                      'algorithmic bytes %d -> bound %.1f us at 8 TB/s'
                      % (str(dtype).replace('torch.', ''), us_rotated, us_rotated - us, us_rotated / us, moved_rotated, moved_rotated / HBM_PEAK * 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--source', default='640x480')
    ap.add_argument('--augment', action='store_true', help='time the augmentation chain (odtk_augment_images)')
    ap.add_argument('--free-rotate', action='store_true', help='with --augment: also time the chain with every image rotated by a free '
                    'angle (odtk_augment_images_ex)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: a timing from anywhere else says nothing'
    sw, sh = (int(v) for v in args.source.split('x'))
    ratio = 800 / min(sw, sh)
    if ratio * max(sw, sh) > 1333:
        ratio = 1333 / max(sw, sh)
    ow, oh = int(ratio * sw), int(ratio * sh)
    rng = np.random.default_rng(0)
    sources = [torch.from_numpy(rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)) for _ in range(args.batch)]
    if args.augment:
        return augment_probe(args, sources, ow, oh)
    buffer = D.SourceBatch.pack(sources, [(ow, oh, k % 2) for k in range(args.batch)], 128)
    batch = D.SourceBatch(buffer)
    uploaded = buffer.cuda()
    images = (_C.Image * batch.batch).from_buffer_copy(batch.images.tobytes())
    tables = batch.tables(uploaded)
    print('%d images %dx%d -> %dx%d, batch [%d, 3, %d, %d]; upload %d bytes (tables %d)' % (
        args.batch, sw, sh, ow, oh, args.batch, batch.height, batch.width, buffer.numel(), 4 * batch.tables_len))
    # the host path's batch for the same images: resized on the host, R G B valid
    packed = torch.zeros(args.batch, batch.height, batch.width, 4, dtype=torch.uint8)
    for k, s in enumerate(sources):
        resized = D.resize_bilinear(s.numpy(), (ow, oh))
        packed[k, :oh, :ow, :3] = torch.from_numpy(resized[:, ::-1].copy() if k % 2 else resized)
        packed[k, :oh, :ow, 3] = 255
    packed = packed.cuda()
    for dtype in (torch.bfloat16, torch.float32):
        table = D.normalisation_table(dtype).cuda()
        out = _C.preprocess_images(uploaded, images, tables, table, batch.height, batch.width)
        ref = D.normalise_batch(packed, table, dtype)
        assert torch.equal(out, ref) and out.stride() == ref.stride(), 'the two device stages disagree'
        us = timed(lambda: _C.preprocess_images(uploaded, images, tables, table, batch.height, batch.width), args.iters)
        us_chain = timed(lambda: D.normalise_batch(packed, table, dtype), args.iters)
        moved = 3 * sw * sh * args.batch + 4 * batch.tables_len + out.numel() * out.element_size() + table.numel() * table.element_size()
        bound = moved / HBM_PEAK * 1e6
        print('%-8s preprocess_images %.1f us per batch (events, back to back, %d calls); algorithmic bytes %d -> bound %.1f us at 8 TB/s, '
              'the kernel reaches %.1f %% of that rate; normalise_batch (torch operators, resized input) %.1f us; ratio %.2fx'
              % (str(dtype).replace('torch.', ''), us, args.iters, moved, bound, 100 * bound / us, us_chain, us_chain / us))


if __name__ == '__main__':
    main()
