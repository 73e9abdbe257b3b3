#!/usr/bin/env python
"""Tiled inference (csrc/tile.hpp, Model.tile) on one GPU: one image of --size x --size (2048), tiles of --tile (512) with --overlap
(128) pixels shared -- 5 x 5 = 25 tiles, four passes of --batch (8) tiles, the last with 7 padding tiles -- ResNet50FPN in bf16
through the engine, the heads calibrated as the benchmark calibrates them.

  tiler    : tile_images_kernel on one chunk of 8 tiles and on all 25 tiles in one launch, timed by the library's own event pair
             (recorded under ODTK_KERNEL_EPILOGUE), against torch.stack of the same slices (stream events: several launches)
  merge    : merge_tile_candidates_kernel on one chunk (8 x 5 x 1000 candidates), event pair under ODTK_KERNEL_NMS, border 0 and 2
  nms      : odtk_nms_ex on the merged list (25 x 5000 slots per image, mostly empty) against the same call on the candidates of
             an untiled pass (5000 slots), event pairs
  forward  : Model.forward with Model.tile against the untiled forward of the same tensor (stream events)

    python tools/tile_probe.py [--iters 100] [--size 2048] [--tile 512] [--overlap 128] [--batch 8]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]
import torch  # noqa: E402
import bench  # noqa: E402
from odtk import _C, box  # noqa: E402
from odtk.model import Model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=100)
ap.add_argument('--size', type=int, default=2048)
ap.add_argument('--tile', type=int, default=512)
ap.add_argument('--overlap', type=int, default=128)
ap.add_argument('--batch', type=int, default=8)
args = ap.parse_args()


def line(name, v, unit='us'):
    v = sorted(v)
    med = statistics.median(v)
    print('  %-64s median %9.1f %s  (min %9.1f, p90 %9.1f)' % (name, med, unit, v[0], v[int(0.9 * (len(v) - 1))]))
    return med


def event_timed(fn, kernel, launches=1):
    """Median-ready list of the library's own event-pair times of `fn`'s launch(es) recorded under `kernel`, in us."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    _C.profile_enable(True, (kernel,))
    _C.profile_collect()
    out = []
    for _ in range(args.iters):
        fn()
        torch.cuda.synchronize()
        total, n = _C.profile_collect()[kernel]
        assert n == launches, (kernel, n)
        out.append(total * 1e3)
    _C.profile_enable(False)
    return out


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


size, overlap = (args.tile, args.tile), (args.overlap, args.overlap)
torch.manual_seed(0)
model = Model(backbones='ResNet50FPN', classes=80)
model.initialize(None)
model = model.cuda().to(memory_format=torch.channels_last).eval()
x = torch.randn(1, 3, args.size, args.size, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).cuda()
x = x.contiguous(memory_format=torch.channels_last)
grid = box.tile_grid(args.size, args.size, size, overlap)
entries = [(0, slot, y, left) for slot, (y, left) in enumerate(grid)]
chunk = entries[:args.batch]
print('ResNet50FPN, bf16 engine, x %s channels_last, tile %d, overlap %d: %d tiles, %d passes of %d'
      % (tuple(x.shape), args.tile, args.overlap, len(grid), -(-len(grid) // args.batch), args.batch))


def heads(inp):
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        return model.heads(inp)


first = box.tile_images(x, chunk, size)
bench.calibrate_cls_head(model, heads, first, bench.SPEC_FRACTION, model.threshold)

print('== tiler (%d bytes per tile)' % (first[0].numel() * first.element_size()))


def stacked(tiles):
    return torch.stack([x[0, :, y:y + args.tile, left:left + args.tile] for _, _, y, left in tiles])


assert torch.equal(stacked(chunk).view(torch.int16), first.view(torch.int16))
line('tile_images_kernel, %d tiles' % len(chunk), event_timed(lambda: box.tile_images(x, chunk, size), 'bias_act_kernel'))
line('torch.stack of %d slices (stream events)' % len(chunk), stream_timed(lambda: stacked(chunk), args.iters))
if len(entries) <= box.MAX_TILES:
    line('tile_images_kernel, %d tiles' % len(entries), event_timed(lambda: box.tile_images(x, entries, size), 'bias_act_kernel'))
    line('torch.stack of %d slices (stream events)' % len(entries), stream_timed(lambda: stacked(entries), args.iters))

engine = model.inference_engine(torch.bfloat16)


def forward():
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        return model(x)


with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
    found = [t.clone() for t in engine._postprocess(first, True)]
    untiled = [t.clone() for t in engine._postprocess(x, True)]
count = found[0].shape[1]
print('== merge: %d tiles x %d candidates (%d positive)' % (found[0].shape[0], count, int((found[0] > 0).sum())))
merged = [torch.zeros((1, len(grid) * count), device='cuda'), torch.zeros((1, len(grid) * count, 4), device='cuda'),
          torch.zeros((1, len(grid) * count), device='cuda')]
for border in (0.0, 2.0):
    line('merge_tile_candidates_kernel, border %g' % border, event_timed(
        lambda: box.merge_tile_candidates(found, chunk, 1, len(grid), size, (args.size, args.size), border, out=merged), 'nms_kernel'))

model.tile = {'size': size, 'overlap': overlap, 'batch': args.batch}
with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
    for first_entry in range(0, len(entries), args.batch):
        part = entries[first_entry:first_entry + args.batch]
        part = part + [(-1, 0, 0, 0)] * (args.batch - len(part))
        box.merge_tile_candidates(engine._postprocess(box.tile_images(x, part, size), True), part, 1, len(grid), size,
                                  (args.size, args.size), 0.0, out=merged)
print('== nms (odtk_nms_ex, nms %.2f, %d detections)' % (model.nms, model.detections))
for name, cand in (('merged list: %d slots, %d positive' % (merged[0].shape[1], int((merged[0] > 0).sum())), merged),
                   ('untiled pass: %d slots, %d positive' % (untiled[0].shape[1], int((untiled[0] > 0).sum())), untiled)):
    for _ in range(3):
        _C.nms(*cand, model.nms, model.detections)
    torch.cuda.synchronize()
    _C.profile_enable(True, ('nms_kernel', 'nms_first_round_kernel', 'rotated_sup_matrix_kernel'))
    _C.profile_collect()
    us = []
    for _ in range(args.iters):
        _C.nms(*cand, model.nms, model.detections)
        torch.cuda.synchronize()
        got = _C.profile_collect()
        us.append(sum(got[k][0] for k in ('nms_kernel', 'nms_first_round_kernel', 'rotated_sup_matrix_kernel')) * 1e3)
    _C.profile_enable(False)
    line(name, us)

print('== Model.forward through the engine, same tensor, stream events, %d calls each' % max(10, args.iters // 5))
tiled = line('Model.tile = %r' % (model.tile,), [v / 1e3 for v in stream_timed(forward, max(10, args.iters // 5))], unit='ms')
model.tile = None
plain = line('untiled', [v / 1e3 for v in stream_timed(forward, max(10, args.iters // 5))], unit='ms')
print('  tiled / untiled = %.2f (the tiles hold %.2f x the pixels of the image)' % (tiled / plain, len(grid) * args.tile ** 2 / args.size ** 2))
