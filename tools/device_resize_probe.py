#!/usr/bin/env python
"""Kernel time of the device-side input pipeline (odtk_preprocess_images, csrc/preprocess.hpp) on a COCO-shaped batch -- 8 images
of 640x480 -> 1066x800, which stride 128 pads to [8, 3, 896, 1152] -- next to its bound (algorithmic bytes: source pixels and
tables read once, the output written once, over the 8 TB/s HBM peak the other rooflines of this project use), and next to the
device stage it replaces: `normalise_batch` on the already resized [8, 896, 1152, 4] uint8 batch (a chain of torch operators that
does strictly less work: no resize).  Event-timed back to back; under `rocprofv3 --kernel-trace --stats` the same launches show
up as preprocess_images_kernel<2> / <4>.

  python tools/device_resize_probe.py [--iters 200] [--batch 8] [--source 640x480]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--source', default='640x480')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: a timing from anywhere else says nothing'
    sw, sh = (int(v) for v in args.source.split('x'))
    ratio = 800 / min(sw, sh)
    if ratio * max(sw, sh) > 1333:
        ratio = 1333 / max(sw, sh)
    ow, oh = int(ratio * sw), int(ratio * sh)
    rng = np.random.default_rng(0)
    sources = [torch.from_numpy(rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)) for _ in range(args.batch)]
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
