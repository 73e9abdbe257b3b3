#!/usr/bin/env python
"""Where the time of the file-based loader goes (odtk/data.py): first-batch latency (worker start-up) vs steady rate,
for several worker counts, on N synthetic JPEGs; plus the per-stage cost in the main process -- for the host path (workers resize
with Pillow and ship the resized RGBA pixels) and for device_resize=True (workers ship the source pixels, one HIP launch resizes,
pads and normalises).

  PROBE_IMAGES=192  PROBE_REPEAT=1  PROBE_WORKERS=0,4,16,32  PROBE_SIZE=1280x800  PROBE_MODES=host,device
PROBE_REPEAT lists every file that many times (a longer pass without writing more files): the steady rate is taken over the SECOND
HALF of the pass, which must be well beyond what the workers prefetch (2 batches each) while the main process waits for the first
batch.  PROBE_SIZE is the size of the JPEGs.  At the default, resize=800 / max_size=1333 asks for the size the images already have and
Pillow returns a copy: the resize is NOT in the host path's figures.  PROBE_SIZE=640x480 (COCO's usual size, -> 1066x800) makes it real.

  python tools/loader_probe.py --augment
the same for TRAINING items with all five augmentations on (quarter turns, brightness, contrast, hue, saturation): the host path
(workers resize, turn and enhance with Pillow) against device_augment=True (workers ship source pixels and descriptors, the chain
of odtk_augment_images does the rest).

  python tools/loader_probe.py --augment --free-rotate
the same with augment_free_rotate=(-30, 30) on top: the host path rotates the resized image with Pillow (bilinear, in double), the
descriptor path ships six doubles per image and odtk_augment_images_ex rotates on the device.

  python tools/loader_probe.py --mosaic 1
training items with the four colour augmentations on (no quarter turns: mosaic refuses them) and mosaic=P: on the host path a worker
decodes four images, resizes each with Pillow and pastes them; with device_augment=True it ships the four source images and one
placement record, and odtk_mosaic_images composes on the device."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]
import numpy as np
import torch
from PIL import Image

from odtk.data import CocoDataset, DataIterator, normalise_batch

N = int(os.environ.get('PROBE_IMAGES', 192))
REPEAT = int(os.environ.get('PROBE_REPEAT', 1))
WIDTH, HEIGHT = (int(v) for v in os.environ.get('PROBE_SIZE', '1280x800').split('x'))
MOSAIC = float(sys.argv[sys.argv.index('--mosaic') + 1]) if '--mosaic' in sys.argv[1:] else 0.0
AUGMENT = '--augment' in sys.argv[1:] or MOSAIC > 0
FREE_ROTATE = AUGMENT and '--free-rotate' in sys.argv[1:]
OPTIONS = dict(training=True, rotate_augment=True, augment_brightness=0.002, augment_contrast=0.002, augment_hue=0.0002,
               augment_saturation=0.002) if AUGMENT else {}                # the sigmas are `odtk train`'s defaults
if FREE_ROTATE:
    OPTIONS['augment_free_rotate'] = (-30, 30)
if MOSAIC:
    OPTIONS.update(rotate_augment=False, mosaic=MOSAIC)
MODES = os.environ.get('PROBE_MODES', 'host,device').split(',')
scratch = tempfile.mkdtemp(prefix='odtk_probe_')
yy, xx = np.mgrid[0:HEIGHT, 0:WIDTH]
images = []
for k in range(N):
    base = np.stack([(xx + 3 * k) % 256, (yy * 2 + k) % 256, ((xx + yy) // 2) % 256], 2).astype(np.uint8)
    Image.fromarray(base, 'RGB').save(os.path.join(scratch, 'im%04d.jpg' % k), quality=90)
images = [{'id': r * N + k, 'file_name': 'im%04d.jpg' % k, 'width': WIDTH, 'height': HEIGHT} for r in range(REPEAT) for k in range(N)]
ann = os.path.join(scratch, 'ann.json')
json.dump({'images': images}, open(ann, 'w'))
cuda = torch.cuda.is_available()
sync = torch.cuda.synchronize if cuda else (lambda: None)
if cuda:
    torch.zeros(1, device='cuda')
print('host cores', os.cpu_count(), 'images', N * REPEAT, '(%d files)' % N, 'of %dx%d' % (WIDTH, HEIGHT), 'resize 800 max 1333 stride 128, batches of 8')

for mode in MODES:
    device_resize = mode == 'device'
    switch = {'device_augment' if AUGMENT else 'device_resize': device_resize}
    if AUGMENT:
        print('--- training items, %s augmentations on%s: %s' % ('four colour' if MOSAIC else 'five', ' and mosaic with probability %g' % MOSAIC if MOSAIC else
                                                               ' and free rotation by -30 .. 30 degrees' if FREE_ROTATE else '', ('device_augment=True: workers ship source pixels and descriptors' if device_resize
                                                                 else 'host path: workers resize, turn and enhance with Pillow')))
    else:
        print('--- %s' % ('device_resize=True: workers ship source pixels' if device_resize else 'host path: workers resize with Pillow'))
    ds = CocoDataset(scratch, 800, 1333, 128, ann, **switch, **OPTIONS)
    t = time.time(); items = [ds[i] for i in range(16)]; per_item = (time.time() - t) / 16
    t = time.time(); packed = [ds.collate_fn(items[:8]) for _ in range(4)][0][0]; per_collate = (time.time() - t) / 4
    it = DataIterator(scratch, 800, 1333, 8, 128, 1, ann, **dict(dict(training=False, num_workers=0, **switch), **OPTIONS))
    pinned = packed.pin_memory() if cuda else packed
    stage = (lambda: it._preprocess(pinned)) if device_resize else (lambda: normalise_batch(pinned.to(it.device, non_blocking=True), it.table))
    out = stage()
    sync(); t = time.time()
    for _ in range(10):
        out = stage()
    sync(); per_stage = (time.time() - t) / 10
    print('main process: item (decode%s + to uint8) %.1f ms, collate of 8 %.1f ms, upload (pinned) + device stage of 8 %.2f ms -> %s'
          % ('' if device_resize else ' + resize + augmentations' if AUGMENT else ' + resize', per_item * 1e3, per_collate * 1e3, per_stage * 1e3, tuple(out.shape)))
    print('bytes per batch of 8 through shared memory and PCIe: %d (%.2f MB)' % (packed.numel(), packed.numel() / 1e6))

    for workers in [int(w) for w in os.environ.get('PROBE_WORKERS', '0,4,16,32').split(',')]:
        it = DataIterator(scratch, 800, 1333, 8, 128, 1, ann, **dict(dict(training=False, num_workers=workers, **switch), **OPTIONS))
        t0 = time.time()
        stamps = []
        for data, *_ in it:
            if not stamps:
                sync()
            stamps.append(time.time() - t0)
        sync()
        total = time.time() - t0
        half = len(stamps) // 2
        print('%2d workers: first batch after %.2f s; second half of the pass %.1f img/s; whole pass %.1f img/s'
              % (workers, stamps[0], 8 * (len(stamps) - half) / max(total - stamps[half - 1], 1e-9), 8 * len(stamps) / total))
        del it                                                      # (training keeps its workers: let them go before the next count)
