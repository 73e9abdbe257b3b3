"""Mosaic augmentation on the GPU (csrc/mosaic.hpp: mosaic_compose_kernel, odtk_mosaic_images): the chain's output must equal the CPU
pipeline of tests/test_mosaic.py (SourceBatch.apply_cpu: mosaic_pixels, itself equal to Pillow, then augment_pixels) bit for bit over
every element of the padded batch, the pad's sign bit included, for the three output dtypes; an image of one tile must come out as
odtk_augment_images writes its source alone; and the loader must yield on the GPU what it yields on the CPU with the same seed.
Every case runs once."""
import random

import numpy as np
import pytest
import torch

from odtk import _C
from odtk import data as D
from test_device_augment import noise
from test_free_rotate import ANN, HERE

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
B, C, H, S = D.AUGMENT_BRIGHTNESS, D.AUGMENT_CONTRAST, D.AUGMENT_HUE, D.AUGMENT_SATURATION
ALL = (B | C | H | S, 1.3, 0.8, 1.6, 200)                          # flags, brightness, contrast, saturation, hue
PLAIN = (0, 1.0, 1.0, 1.0, 0)
COLOURS = dict(augment_brightness=0.3, augment_contrast=0.3, augment_hue=0.1, augment_saturation=0.3)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def item(canvas, sources, tiles, colour=ALL):
    """One mosaic item for SourceBatch.pack: sources = [(pixels, (out_width, out_height), mirror)], tiles = [(k, index into sources,
    dst_x, dst_y, width, height, src_x, src_y)] -> (the list of source tensors, MosaicGeometry)."""
    geometry = D.MosaicGeometry(canvas[0], canvas[1], tuple(tuple(size) + (int(mirror),) for _, size, mirror in sources), tuple(tiles), *colour)
    return [torch.from_numpy(p) for p, _, _ in sources], geometry


def quadrants(canvas, centre, sources, colour=ALL):
    """The item the loader builds: tile k = source k, placed by `mosaic_placement`; a tile without pixels is left out."""
    tiles = []
    for k, (_, size, _) in enumerate(sources):
        placement = D.mosaic_placement(k, size[0], size[1], centre[0], centre[1], *canvas)
        if placement[2] and placement[3]:
            tiles.append((k, k) + placement)
    return item(canvas, sources, tiles, colour)


def _arrays(batch):
    images = (_C.Image * len(batch.images)).from_buffer_copy(batch.images.tobytes())
    mosaics = (_C.Mosaic * batch.batch).from_buffer_copy(batch.mosaics.tobytes())
    augments = (_C.Augment * batch.batch).from_buffer_copy(batch.augments.tobytes())
    return images, mosaics, augments


def _run(buffer, dtype, colours=True, uploaded=None, table=None):
    batch = D.SourceBatch(buffer)
    uploaded = buffer.cuda() if uploaded is None else uploaded
    table = D.normalisation_table(dtype).cuda() if table is None else table
    images, mosaics, augments = _arrays(batch)
    return _C.mosaic_images(uploaded, images, mosaics, augments if colours else None, batch.tables(uploaded), table, batch.height, batch.width)


def _run_alone(source, geometry, stride, dtype):
    """odtk_augment_images on one source."""
    buffer = D.SourceBatch.pack([torch.from_numpy(source)], [geometry], stride)
    batch = D.SourceBatch(buffer)
    assert batch.mosaics is None
    uploaded = buffer.cuda()
    images = (_C.Image * 1).from_buffer_copy(batch.images.tobytes())
    augments = (_C.Augment * 1).from_buffer_copy(batch.augments.tobytes())
    return _C.augment_images(uploaded, images, augments, batch.tables(uploaded), D.normalisation_table(dtype).cuda(), batch.height, batch.width)


def _check(items, stride, dtypes=DTYPES):
    """Pack, run on the device for every dtype, compare bits with the CPU pipeline; -> the batch."""
    buffer = D.SourceBatch.pack([i[0] for i in items], [i[1] for i in items], stride)
    batch = D.SourceBatch(buffer)
    assert batch.mosaics is not None and batch.batch == len(items)
    for dtype in dtypes:
        out = _run(buffer, dtype)
        assert out.shape == (len(items), 3, batch.height, batch.width) and out.dtype == dtype
        assert out.is_contiguous(memory_format=torch.channels_last)
        got = _bits(out.permute(0, 2, 3, 1)).cpu()
        want = _bits(batch.apply_cpu(D.normalisation_table(dtype), dtype).permute(0, 2, 3, 1))
        differ = (got != want).flatten(1).sum(1).tolist()
        print(dtype, 'differing elements per image:', differ)
        assert not any(differ), (dtype, differ)                     # bits: the pad's sign bit included
        for k, record in enumerate(batch.mosaics):
            assert not got[k, int(record['canvas_height']):].any() and not got[k, :, int(record['canvas_width']):].any()
    return batch


def plain(size, flip, colour):
    """The geometry of an item that is no mosaic (CocoDataset._augment_item without a turn)."""
    return tuple(size) + (0,) + D.quarter_turn_map(size[0], size[1], 0, flip=flip) + tuple(colour)


def test_every_placement_case_in_one_batch():
    """Canvases of 70 x 45 (rows of 210 bytes: no whole words, no whole vectors), 64 x 48 and 1 x 7, padded to 96 x 64.  Sources
    (width x height): 53 x 37 -> 80 x 60 (up-scaled, mirrored, cropped both ways), 120 x 75 -> 40 x 25 (down by 3: the chunked
    vertical footprint; cropped in height), 20 x 10 unscaled (no table; smaller than its quadrant: fill shows; mirrored), 7 x 1 -> 1 x 1.
    The second image leaves tiles 0 and 2 unused and has two tiles that overlap, the higher index on top; the
    third is one column; the last two are no mosaics, with and without a flip.  Every colour operation is on: the contrast's grey
    level includes the fill."""
    s = [noise(53, 37, 'noise', 1), noise(120, 75, 'noise', 2), noise(20, 10, 'noise', 3), noise(7, 1, 'noise', 4),
         noise(64, 64, 'binary', 5), noise(1, 7, 'noise', 6), noise(33, 21, 'noise', 7)]
    items = [quadrants((70, 45), (30, 20), [(s[0], (80, 60), 1), (s[1], (40, 25), 0), (s[2], (20, 10), 1), (s[3], (1, 1), 0)]),
             item((64, 48), [(s[4], (50, 40), 0), (s[1], (60, 38), 1)], [(1, 0, 0, 0, 40, 30, 3, 2), (3, 1, 20, 10, 44, 38, 16, 0)],
                  (C, 1.0, 1.7, 1.0, 0)),
             item((1, 7), [(s[5], (1, 7), 0)], [(2, 0, 0, 2, 1, 5, 0, 1)]),
             (torch.from_numpy(s[6]), plain((50, 32), True, ALL)),
             (torch.from_numpy(s[6]), plain((33, 21), False, ALL))]
    batch = _check(items, 32)
    assert (batch.height, batch.width) == (64, 96) and len(batch.images) == 9
    assert batch.mosaics['tiles']['source'].tolist() == [[0, 1, 2, 3], [-1, 4, -1, 5], [-1, -1, 6, -1], [7, -1, -1, -1], [8, -1, -1, -1]]
    assert batch.images['mirror'].tolist() == [1, 0, 1, 0, 0, 1, 0, 1, 0]
    assert int(batch.images[2]['x_table']) == -1 and int(batch.images[2]['y_table']) == -1 and int(batch.images[1]['y_taps']) > 5
    # an image of one tile: what odtk_augment_images writes for its source alone, the flip in the map there
    for k, geometry in ((3, items[3][1]), (4, items[4][1])):
        for dtype in DTYPES:
            want = _run_alone(s[6], geometry, 32, dtype)
            got = _run(batch.buffer, dtype)[k:k + 1, :, :want.shape[2], :want.shape[3]]
            assert torch.equal(_bits(got.permute(0, 2, 3, 1)), _bits(want.permute(0, 2, 3, 1))), (k, dtype)


def _seventeen():
    rng = np.random.default_rng(17)
    items = []
    for b in range(17):
        sources = []
        for k in range(4):
            w, h = int(rng.integers(4, 10)), int(rng.integers(4, 8))
            size = (int(rng.integers(4, 10)), int(rng.integers(4, 8))) if k % 2 else (w, h)
            sources.append((noise(w, h, 'noise', 1000 + 4 * b + k), size, int(rng.integers(0, 2))))
        items.append(quadrants((16, 12), (int(rng.integers(4, 13)), int(rng.integers(3, 10))), sources, (C | S, 1.0, 0.5 + b / 17, 1.3, 0)))
    return items


def test_seventeen_images_take_more_than_one_launch_of_each_pass():
    """68 sources of 4 x 4 to 9 x 7 pixels (pass A: 64 per launch) on 17 canvases of 16 x 12 (pass M: 16 per launch)."""
    batch = _check(_seventeen(), 8)
    assert len(batch.images) == 68 > 64 and batch.batch == 17 > 16


def test_without_augment_descriptors():
    """augments = NULL: no colours -- what flags = 0 gives."""
    items = [(i[0], i[1]._replace(**dict(zip(('flags', 'brightness', 'contrast', 'saturation', 'hue'), PLAIN)))) for i in _seventeen()[:3]]
    buffer = D.SourceBatch.pack([i[0] for i in items], [i[1] for i in items], 8)
    batch = D.SourceBatch(buffer)
    for dtype in DTYPES:
        got = _bits(_run(buffer, dtype, colours=False).permute(0, 2, 3, 1)).cpu()
        assert torch.equal(got, _bits(batch.apply_cpu(D.normalisation_table(dtype), dtype).permute(0, 2, 3, 1))), dtype


def test_seeded_iterator_on_the_gpu_equals_the_cpu_device():
    args = (HERE, [96, 160], 220, 5, 32, 1, ANN)
    batches = []
    for device in ('cuda', 'cpu'):
        it = D.DataIterator(*args, training=True, num_workers=0, device=device, device_augment=True, mosaic=1.0, **COLOURS)
        assert 'mosaic: probability 1, scale 0.5 to 1' in repr(it)
        random.seed(31)
        torch.manual_seed(31)
        batches.append([tuple(t.clone() for t in b) for _ in range(2) for b in it])
        torch.cuda.synchronize()
    assert len(batches[0]) == len(batches[1]) == 2
    for (a, ta), (b, tb) in zip(*batches):
        assert a.is_cuda and not b.is_cuda and a.shape == b.shape and a.stride() == b.stride()
        assert torch.equal(_bits(a.permute(0, 2, 3, 1)).cpu(), _bits(b.permute(0, 2, 3, 1)))
        assert torch.equal(ta.cpu(), tb)


def test_the_chain_replays_from_one_graph():
    """A linear chain on one stream (A, M, B, C; no parallel branches): captured and replayed it gives the eager call's bits."""
    items = _seventeen()[:5]
    buffer = D.SourceBatch.pack([i[0] for i in items], [i[1] for i in items], 8)
    uploaded, table = buffer.cuda(), D.normalisation_table(torch.bfloat16).cuda()      # (no upload inside the capture)
    eager = _run(buffer, torch.bfloat16, uploaded=uploaded, table=table).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _run(buffer, torch.bfloat16, uploaded=uploaded, table=table)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(captured.permute(0, 2, 3, 1)), _bits(eager.permute(0, 2, 3, 1)))
