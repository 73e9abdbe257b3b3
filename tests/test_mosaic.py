"""Mosaic augmentation on the CPU (odtk/data.py: CocoDataset(mosaic=...), mosaic_placement, mosaic_tile_boxes, mosaic_pixels,
SourceBatch): the numpy restatement the device path is pinned to equals Pillow's composition byte for byte, the loader's host
path (Pillow) and its device path on the CPU yield the same batches, the boxes follow their tiles, the option changes nothing
while it is off, the refused combinations are refused, and the C ABI validates on the host.  The GPU half is
tests/test_gpu_mosaic.py."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from odtk import _C
from odtk import data as D
from odtk import main as cli
from test_device_augment import noise

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data')
ANN = os.path.join(HERE, 'annotations.json')
ANN_ROT = os.path.join(HERE, 'annotations_rotated.json')
COLOURS = dict(augment_brightness=0.3, augment_contrast=0.3, augment_hue=0.1, augment_saturation=0.3)


# -- pixels -----------------------------------------------------------------------------------------------------------------------
def pillow_mosaic(images, sizes, mirrors, centre, canvas):
    """The composition as the issue defines it, with Pillow alone: images = four PIL images, sizes = their (tw, th)."""
    (cx, cy), (W, H) = centre, canvas
    out = Image.new('RGB', (W, H), (114, 114, 114))
    for k, (im, (tw, th), mirror) in enumerate(zip(images, sizes, mirrors)):
        tile = im.resize((tw, th), Image.BILINEAR)
        if mirror:
            tile = tile.transpose(Image.FLIP_LEFT_RIGHT)
        if k == 0:
            dw, dh = min(tw, cx), min(th, cy)
            dst, src = (cx - dw, cy - dh), (tw - dw, th - dh)
        elif k == 1:
            dw, dh = min(tw, W - cx), min(th, cy)
            dst, src = (cx, cy - dh), (0, th - dh)
        elif k == 2:
            dw, dh = min(tw, cx), min(th, H - cy)
            dst, src = (cx - dw, cy), (tw - dw, 0)
        else:
            dw, dh = min(tw, W - cx), min(th, H - cy)
            dst, src = (cx, cy), (0, 0)
        if dw == 0 or dh == 0:
            continue
        out.paste(tile.crop((src[0], src[1], src[0] + dw, src[1] + dh)), dst)
    return np.array(out)


def numpy_mosaic(arrays, sizes, mirrors, centre, canvas):
    """The same through resize_bilinear, mosaic_placement and mosaic_pixels, without Pillow."""
    record = np.zeros((), dtype=D.MOSAIC_DTYPE)
    record['canvas_width'], record['canvas_height'], record['fill'] = canvas[0], canvas[1], D.MOSAIC_FILL
    record['tiles']['source'] = -1
    tiles = []
    for k, (pixels, size, mirror) in enumerate(zip(arrays, sizes, mirrors)):
        tile = D.resize_bilinear(pixels, size)
        tiles.append(tile[:, ::-1] if mirror else tile)
        placement = D.mosaic_placement(k, size[0], size[1], centre[0], centre[1], *canvas)
        if placement[2] and placement[3]:
            record['tiles'][k] = (k,) + placement
    return D.mosaic_pixels(tiles, record)


def _golden_images():
    return [np.array(Image.open(os.path.join(HERE, 'im%d.png' % k)).convert('RGB')) for k in range(5)]


PLACEMENTS = [                                                      # sizes of the four tiles, mirrors, centre, canvas
    ([(80, 60), (40, 25), (20, 10), (1, 1)], (1, 0, 1, 0), (30, 20), (70, 45)),       # larger and smaller than the quadrant, 1 x 1
    ([(9, 9), (30, 30), (9, 9), (30, 30)], (0, 1, 1, 0), (0, 12), (24, 31)),          # cx = 0: tiles 0 and 2 have no pixels
    ([(9, 9), (30, 30), (9, 9), (30, 30)], (1, 1, 0, 0), (11, 0), (24, 31)),          # cy = 0: tiles 0 and 1 have none
    ([(5, 7), (6, 3), (2, 2), (3, 8)], (0, 0, 0, 0), (0, 0), (1, 1)),                 # a canvas of one pixel
    ([(1, 1), (1, 1), (1, 1), (1, 1)], (1, 1, 1, 1), (8, 8), (16, 16)),               # 1 x 1 tiles on a canvas of fill
    ([(64, 64), (64, 64), (64, 64), (64, 64)], (0, 1, 0, 1), (32, 24), (64, 48)),     # every quadrant full
    ([(16, 12), (16, 12), (16, 12), (16, 12)], (1, 0, 0, 1), (16, 12), (32, 24))]     # tiles that fit exactly


@pytest.mark.parametrize('case', range(len(PLACEMENTS)))
def test_numpy_composition_equals_pillow_on_chosen_placements(case):
    sizes, mirrors, centre, canvas = PLACEMENTS[case]
    arrays = [noise(53, 37, 'noise', 1), noise(120, 75, 'noise', 2), noise(20, 10, 'binary', 3), noise(7, 1, 'noise', 4)]
    want = pillow_mosaic([Image.fromarray(a) for a in arrays], sizes, mirrors, centre, canvas)
    got = numpy_mosaic(arrays, sizes, mirrors, centre, canvas)
    assert got.shape == want.shape == (canvas[1], canvas[0], 3) and np.array_equal(got, want)
    if case == 4:
        assert (got == 114).all(axis=-1).sum() == 16 * 16 - 4


def test_numpy_composition_equals_pillow_on_seeded_placements():
    """The loader's own draws (scale, centre, mirrors) over the golden images and synthetic sources."""
    rng = random.Random(7)
    pool = _golden_images() + [noise(53, 37, 'noise', 11), noise(3, 5, 'noise', 12), noise(7, 1, 'binary', 13)]
    for _ in range(40):
        arrays = [pool[rng.randrange(len(pool))] for _ in range(4)]
        canvas = (rng.randint(1, 90), rng.randint(1, 70))
        g = rng.uniform(0.3, 1.0)
        sizes = [(max(1, int(g * rng.uniform(0.5, 2.0) * a.shape[1])), max(1, int(g * rng.uniform(0.5, 2.0) * a.shape[0]))) for a in arrays]
        centre = (int(rng.uniform(0.25, 0.75) * canvas[0]), int(rng.uniform(0.25, 0.75) * canvas[1]))
        mirrors = [rng.randint(0, 1) for _ in range(4)]
        want = pillow_mosaic([Image.fromarray(a) for a in arrays], sizes, mirrors, centre, canvas)
        assert np.array_equal(numpy_mosaic(arrays, sizes, mirrors, centre, canvas), want), (canvas, sizes, centre, mirrors)


def test_a_later_tile_covers_an_earlier_one():
    """The records of the C ABI are more general than the loader's quadrants: tiles may overlap, unused ones are skipped."""
    a, b = noise(6, 4, 'noise', 1), noise(5, 5, 'noise', 2)
    record = np.zeros((), dtype=D.MOSAIC_DTYPE)
    record['canvas_width'], record['canvas_height'], record['fill'] = 8, 6, (1, 2, 3)
    record['tiles']['source'] = -1
    record['tiles'][1] = (0, 0, 0, 6, 4, 0, 0)
    record['tiles'][3] = (1, 4, 2, 4, 4, 1, 1)
    out = D.mosaic_pixels([a, b], record)
    want = np.empty((6, 8, 3), np.uint8)
    want[:] = (1, 2, 3)
    want[:4, :6] = a
    want[2:6, 4:8] = b[1:5, 1:5]
    assert np.array_equal(out, want)


# -- the loader -------------------------------------------------------------------------------------------------------------------
def _epochs(seed, epochs=2, **options):
    it = D.DataIterator(HERE, [96, 160], 220, 5, 32, 1, ANN, training=True, num_workers=0, device='cpu', **options)
    random.seed(seed)
    torch.manual_seed(seed)
    return it, [tuple(t.clone() for t in b) for _ in range(epochs) for b in it]


def test_host_path_and_device_path_on_the_cpu_yield_the_same_batches():
    host_it, host = _epochs(31, mosaic=1.0, **COLOURS)
    device_it, device = _epochs(31, mosaic=1.0, device_augment=True, **COLOURS)
    assert 'mosaic: probability 1, scale 0.5 to 1' in repr(host_it) and 'mosaic' in repr(device_it)
    assert 'mosaic' not in repr(D.DataIterator(HERE, 96, 220, 5, 32, 1, ANN, training=True, num_workers=0, device='cpu'))
    assert len(host) == len(device) == 2
    for (a, ta), (b, tb) in zip(host, device):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ta, tb)
        assert (ta[..., 4] >= 0).any()                              # boxes came through
    # a mixed batch (some items are mosaics, some are not) packs the others as one-tile records: the same again
    for p in (0.5, 0.3):
        host, device = _epochs(5, mosaic=p, **COLOURS)[1], _epochs(5, mosaic=p, device_augment=True, **COLOURS)[1]
        for (a, ta), (b, tb) in zip(host, device):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ta, tb)


def test_a_mosaic_item_carries_its_sources_and_a_placement_record():
    ds = D.CocoDataset(HERE, [96, 160], 220, 32, annotations=ANN, training=True, device_augment=True, mosaic=1.0, mosaic_scale=(0.6, 0.9), **COLOURS)
    random.seed(3)
    pixels, geometry, target = ds[1]
    assert isinstance(geometry, D.MosaicGeometry) and isinstance(pixels, list) and 1 <= len(pixels) == len(geometry.sources) <= 4
    assert [t[0] for t in geometry.tiles] == sorted(t[0] for t in geometry.tiles) and geometry.tiles[0][0] == 0
    assert geometry.flags == 15 and target.shape[1] == 5
    # the canvas is the size the primary image is resized to: the draws before it are those of the plain loader
    random.seed(3)
    _, _, size = D.CocoDataset(HERE, [96, 160], 220, 32, annotations=ANN, training=True)._open(ds.ids[1])
    assert (geometry.width, geometry.height) == size
    buffer = D.SourceBatch.pack([pixels], [geometry], 32)
    batch = D.SourceBatch(buffer)
    assert batch.batch == 1 and len(batch.images) == len(pixels) and batch.rotations is None
    assert int(buffer.numpy()[:32].view(np.int32)[7]) > 0 and ctypes.sizeof(_C.Mosaic) == D.MOSAIC_DTYPE.itemsize == 124
    assert tuple(batch.augments[0]['map']) == (65536, 0, 0, 0, 65536, 0)
    assert (int(batch.augments[0]['canvas_width']), int(batch.augments[0]['canvas_height'])) == size


# -- boxes ------------------------------------------------------------------------------------------------------------------------
def _boxes(rows):
    return torch.tensor(rows, dtype=torch.float32)


def test_boxes_are_scaled_shifted_and_clipped_to_their_tile():
    # tile 3 of 40 x 30 at the centre (50, 40) of a 70 x 60 canvas: dst (50, 40), 20 x 20 of it from src (0, 0)
    placement = D.mosaic_placement(3, 40, 30, 50, 40, 70, 60)
    assert placement == (50, 40, 20, 20, 0, 0)
    moved, keep = D.mosaic_tile_boxes(_boxes([[4, 6, 10, 8], [20, 10, 40, 30], [50, 50, 10, 10]]), 0.5, 40, 0, placement)
    assert moved.dtype == torch.float64 and keep.tolist() == [True, True, False]
    assert moved[0].tolist() == [52.0, 43.0, 5.0, 4.0]              # inside: scaled by 0.5 and shifted by (50, 40)
    assert moved[1].tolist() == [60.0, 45.0, 10.0, 15.0]            # 20 x 15 at (60, 45) clipped to x < 70: 10 / 20 of the area
    assert moved[2, 2:].tolist() == [0.0, 0.0]                      # beyond the rectangle: clipped to nothing
    # tile 0 of 40 x 30 at the centre (25, 12): dst (0, 0), 25 x 12 from src (15, 18); the shift is dst - src = (-15, -18)
    placement = D.mosaic_placement(0, 40, 30, 25, 12, 70, 60)
    assert placement == (0, 0, 25, 12, 15, 18)
    moved, keep = D.mosaic_tile_boxes(_boxes([[20, 20, 10, 6], [10, 16, 10, 8]]), 1.0, 40, 0, placement)
    assert moved.tolist() == [[5.0, 2.0, 10.0, 6.0], [0.0, 0.0, 5.0, 6.0]] and keep.tolist() == [True, True]


def test_the_keep_conditions_at_their_edges():
    placement = (10, 10, 20, 20, 0, 0)                              # the destination rectangle is [10, 30) x [10, 30)
    rows = [[-4, 0, 5, 5],                                          # 1 px of its width is left: kept (1 * 5 = 0.2 of 25)
            [-4.25, 0, 5, 5],                                       # 0.75 px: dropped
            [0, -9, 5, 10],                                         # 1 px of its height, but 0.1 of its area: dropped
            [0, -4, 5, 5],                                          # exactly 1 px of height and exactly 0.2 of the area: kept
            [-8, 0, 10, 10],                                        # 2 x 10 of 10 x 10 = exactly 0.2: kept
            [-8.5, 0, 10, 10],                                      # 1.5 x 10 = 0.15: dropped
            [-16, -15, 20, 20],                                     # 4 x 5 = 20 of 400: dropped by the area alone
            [0, 0, 1, 1], [0, 0, 0.5, 8], [0, 0, 8, 0.99]]          # whole boxes: 1 px is enough, less is not
    moved, keep = D.mosaic_tile_boxes(_boxes(rows), 1.0, 20, 0, placement)
    assert keep.tolist() == [True, False, False, True, True, False, False, True, False, False]
    assert moved[0].tolist() == [10.0, 10.0, 1.0, 5.0] and moved[4].tolist() == [10.0, 10.0, 2.0, 10.0]
    assert D.MOSAIC_MIN_AREA == 0.2


def test_boxes_of_a_mirrored_tile_are_flipped_within_the_tile():
    # tile 1 of 30 x 20, mirrored, at the centre (10, 25) of a 50 x 40 canvas: dst (10, 5), all of it
    placement = D.mosaic_placement(1, 30, 20, 10, 25, 50, 40)
    assert placement == (10, 5, 30, 20, 0, 0)
    moved, keep = D.mosaic_tile_boxes(_boxes([[2, 3, 8, 4]]), 1.0, 30, 1, placement)
    assert moved.tolist() == [[10.0 + (30 - 2 - 8), 8.0, 8.0, 4.0]] and keep.tolist() == [True]
    # the flip uses the WHOLE tile's width, also when the tile is cropped (tile 0 keeps its right part)
    placement = D.mosaic_placement(0, 30, 20, 12, 20, 50, 40)
    assert placement == (0, 0, 12, 20, 18, 0)
    moved, keep = D.mosaic_tile_boxes(_boxes([[2, 3, 8, 4]]), 1.0, 30, 1, placement)
    assert moved.tolist() == [[2.0, 3.0, 8.0, 4.0]] and keep.tolist() == [True]      # x = 30 - 2 - 8 = 20, shifted by -18


def _tiny_dataset(tmp_path, boxes_per_image, **options):
    """Four 40 x 30 images (resize 30: ratio 1) whose annotations are `boxes_per_image`; class = the image's index."""
    images, annotations = [], []
    for k, boxes in enumerate(boxes_per_image):
        Image.fromarray(noise(40, 30, 'noise', 50 + k)).save(str(tmp_path / ('t%d.png' % k)))
        images.append({'id': 10 + k, 'file_name': 't%d.png' % k, 'width': 40, 'height': 30})
        for box in boxes:
            annotations.append({'id': len(annotations) + 1, 'image_id': 10 + k, 'category_id': k + 1, 'bbox': list(box), 'area': box[2] * box[3],
                                'iscrowd': 0})
    dataset = {'images': images, 'annotations': annotations, 'categories': [{'id': k + 1, 'name': 'c%d' % k} for k in range(len(images))]}
    return D.CocoDataset(str(tmp_path), 30, 100, 32, annotations=dataset, training=True, mosaic=1.0, **options)


def _replay_draws(ds, seed, scale):
    """The draws of one mosaic item in the issue's order (resize is no range: `_open` draws nothing)."""
    rng = random.Random(seed)
    assert rng.random() < 1.0
    g = rng.uniform(*scale)
    cx, cy = int(rng.uniform(0.25, 0.75) * 40), int(rng.uniform(0.25, 0.75) * 30)
    others = [ds.ids[rng.randrange(len(ds.ids))] for _ in range(3)]
    mirrors = [rng.randint(0, 1) for _ in range(4)]
    return g, cx, cy, others, mirrors, rng


def test_targets_follow_the_tiles_in_their_order(tmp_path):
    """Every image has a 6 px high box in each corner, 8 px wide on the left and 7 px on the right.  At g = 1 a tile fills its
    quadrant with the part of its image that touches the centre, at least 10 x 7 pixels: exactly the box in that corner is left
    (the others are clipped to nothing), and in a mirrored tile it is the box of the other side.  Image 12 has no annotation."""
    corners = [(0, 0, 8, 6), (33, 0, 7, 6), (0, 24, 8, 6), (33, 24, 7, 6)]
    ds = _tiny_dataset(tmp_path, [corners, corners + [(0, 0, 0.5, 0.5)], [], corners], mosaic_scale=(1.0, 1.0))
    mirrored = 0
    for seed in range(8):
        g, cx, cy, others, mirrors, rng = _replay_draws(ds, seed, (1.0, 1.0))
        random.seed(seed)
        pixels, target = ds[0]
        assert random.getstate() == rng.getstate()                  # exactly these draws, no more
        assert pixels.shape == (30, 40, 4) and g == 1.0
        want = []
        for k, image_id in enumerate([10] + others):
            if image_id == 12:
                continue
            right = k in (0, 2)                                     # the quadrant shows the tile's right part
            width = 7 if right != bool(mirrors[k]) else 8
            want.append([cx - width if right else cx, cy - 6 if k in (0, 1) else cy, width, 6, image_id - 10])
            mirrored += mirrors[k]
        assert target.tolist() == [[float(v) for v in row] for row in want], seed
    assert mirrored > 3


def test_nothing_left_gives_the_no_box_row(tmp_path):
    ds = _tiny_dataset(tmp_path, [[(5, 5, 1.5, 1.5)], [(20, 10, 1.2, 9)], [], [(0, 0, 1.9, 1.9)]], mosaic_scale=(0.5, 0.5))
    for seed in range(4):                                           # scaled by 0.5 every box is narrower than a pixel
        random.seed(seed)
        assert ds[seed % 4][1].tolist() == [[1.0, 1.0, 1.0, 1.0, -1.0]]


# -- off means untouched ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('options', [{}, dict(device_resize=True), dict(device_augment=True, rotate_augment=True, augment_free_rotate=(-20, 20), **COLOURS),
                                     dict(rotate_augment=True, **COLOURS)], ids=['host', 'device-resize', 'device-augment', 'host-augment'])
def test_mosaic_zero_takes_no_draw_and_changes_no_item(options):
    def items(**extra):
        ds = D.CocoDataset(HERE, [96, 160], 220, 32, annotations=ANN, training=True, **options, **extra)
        random.seed(11)
        return [ds[k] for k in range(len(ds))], random.getstate()

    def same(a, b):
        if isinstance(a, torch.Tensor):
            return torch.equal(a, b)
        if isinstance(a, (tuple, list)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return a == b

    (plain, plain_state), (off, off_state) = items(), items(mosaic=0.0, mosaic_scale=(0.3, 0.4))
    assert plain_state == off_state and same(plain, off)


def pack_cases(module):
    """name -> (sources, geometry, stride): batches without a mosaic, as the tests of the device path pack them.  `module`: the
    odtk.data to take quarter_turn_map / free_rotation_matrix from (tests/golden/mosaic_pack_parent.npz holds what the parent
    commit's `SourceBatch.pack` wrote for them)."""
    a, b, c = noise(37, 21, 'noise', 1), noise(16, 16, 'noise', 2), noise(9, 30, 'binary', 3)
    turned = (50, 30, 0) + module.quarter_turn_map(50, 30, 90, True, False) + (module.AUGMENT_HUE, 1.0, 1.0, 1.0, 9)
    flipped = (16, 16, 0) + module.quarter_turn_map(16, 16, 0, False, True) + (15, 1.3, 0.8, 1.6, 200)
    cw, ch, coefficients = module.quarter_turn_map(20, 60, 270, False, False)
    rotated = (20, 60, 0, cw, ch, coefficients, 3, 1.1, 0.9, 1.0, 0, module.free_rotation_matrix(cw, ch, -7.3), 1)
    return {'plain': ([a, b, c], [(50, 30, 1), (16, 16, 0), (9, 30, 1)], 32),
            'augmented': ([a, b, c], [turned, (16, 16, 1), flipped[:2] + (0,) + flipped[3:]], 32),
            'rotated': ([a, b, c], [turned, flipped, rotated], 8)}


def written_bytes(view):
    """Mask of the bytes of a packed buffer WITHOUT a mosaic that `pack` writes (the gaps that align the parts to 16 bytes are not
    written: the buffer is born uninitialised), from the buffer's own header and descriptors."""
    batch, _, _, tables_at, tables_len, augments_at, rotations_at, _ = (int(v) for v in view[:32].view(np.int32))
    mask = np.zeros(view.shape, dtype=bool)
    mask[:32 + batch * D.IMAGE_DTYPE.itemsize] = True
    if augments_at:
        mask[augments_at:augments_at + batch * D.AUGMENT_DTYPE.itemsize] = True
    if rotations_at:
        mask[rotations_at:rotations_at + batch * D.ROTATION_DTYPE.itemsize] = True
    mask[tables_at:tables_at + 4 * tables_len] = True
    for im in view[32:32 + batch * D.IMAGE_DTYPE.itemsize].view(D.IMAGE_DTYPE):
        mask[int(im['src_offset']):int(im['src_offset']) + int(im['src_pitch']) * int(im['src_height'])] = True
    return mask


def test_a_batch_without_a_mosaic_packs_to_the_parents_bytes(golden_dir):
    """tests/golden/mosaic_pack_parent.npz: what the parent commit's `SourceBatch.pack` wrote for `pack_cases` (its unwritten gaps
    zeroed).  Same length, same header, same written bytes in the same places; the eighth header word stays 0."""
    with np.load(os.path.join(golden_dir, 'mosaic_pack_parent.npz')) as parent:
        for name, (sources, geometry, stride) in pack_cases(D).items():
            view = D.SourceBatch.pack([torch.from_numpy(s) for s in sources], geometry, stride).numpy()
            want = parent[name]
            assert view.shape == want.shape and np.array_equal(view[:32], want[:32]), name
            mask = written_bytes(want)
            assert np.array_equal(mask, written_bytes(view)) and mask.sum() > 0.95 * mask.size, name
            assert np.array_equal(view[mask], want[mask]) and not want[~mask].any(), name
            assert int(view[:32].view(np.int32)[7]) == 0 and D.SourceBatch(torch.from_numpy(view)).mosaics is None


# -- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refused_combinations_raise_in_the_dataset():
    base = dict(annotations=ANN, training=True, mosaic=0.5)
    for bad in (dict(rotate_augment=True), dict(augment_free_rotate=(-5, 5)), dict(device_resize=True),
                dict(rotate_augment=True, device_augment=True), dict(augment_free_rotate=(0, 5), device_augment=True)):
        with pytest.raises(ValueError, match='mosaic'):
            D.CocoDataset(HERE, 128, 200, 32, **base, **bad)
    with pytest.raises(ValueError, match='mosaic'):
        D.RotatedCocoDataset(HERE, 128, 200, 32, annotations=ANN_ROT, training=True, mosaic=0.5)
    with pytest.raises(ValueError, match='mosaic'):
        D.RotatedDataIterator(HERE, 128, 200, 2, 32, 1, ANN_ROT, training=True, device='cpu', num_workers=0, mosaic=1.0)
    for bad in (dict(mosaic=-0.1), dict(mosaic=1.5), dict(mosaic=float('nan')), dict(mosaic=0.5, mosaic_scale=(0.0, 1.0)),
                dict(mosaic=0.5, mosaic_scale=(0.8, 0.5)), dict(mosaic=0.5, mosaic_scale=(0.5, 1.5)), dict(mosaic=0.5, mosaic_scale=(0.5,))):
        with pytest.raises(ValueError, match='mosaic'):
            D.CocoDataset(HERE, 128, 200, 32, annotations=ANN, training=True, **bad)
    # accepted: alone, with the colours, with device_augment (and device_resize beside it)
    for good in ({}, COLOURS, dict(device_augment=True), dict(device_augment=True, device_resize=True, **COLOURS)):
        assert D.CocoDataset(HERE, 128, 200, 32, **base, **good).mosaic == 0.5


def test_command_line(monkeypatch, capsys):
    base = ['train', 'm.pth', '--annotations', 'a.json']
    plain = vars(cli.parse(base))
    assert 'mosaic' not in plain and 'mosaic_scale' not in plain
    parsed = cli.parse(base + ['--mosaic', '0.75', '--mosaic-scale', '0.4', '0.9', '--device-augment'])
    assert parsed.mosaic == 0.75 and parsed.mosaic_scale == [0.4, 0.9]
    assert 'mosaic_scale' not in vars(cli.parse(base + ['--mosaic', '1']))
    for bad in (['--mosaic', '0.5', '--rotated-bbox'], ['--mosaic', '0.5', '--augment-rotate'], ['--mosaic', '0.5', '--augment-free-rotate', '-5', '5'],
                ['--mosaic', '0.5', '--device-resize'], ['--mosaic', '1.5'], ['--mosaic', '-0.1'], ['--mosaic', 'nan'],
                ['--mosaic', '0.5', '--mosaic-scale', '0', '1'], ['--mosaic', '0.5', '--mosaic-scale', '0.8', '0.5'],
                ['--mosaic', '0.5', '--mosaic-scale', '0.5', '1.5'], ['--mosaic-scale', '0.5', '1.0']):
        with pytest.raises(SystemExit):
            cli.parse(base + bad)
    capsys.readouterr()
    assert cli.parse(base + ['--mosaic', '0.5', '--device-resize', '--device-augment', '--augment-free-rotate', '0', '0']).mosaic == 0.5
    with pytest.raises(SystemExit):
        cli.parse(['infer', 'm.pth', '--mosaic', '0.5'])
    # it reaches the iterator, and only when given
    from odtk.model import Model
    seen = []

    def spy(self, *args, **kwargs):
        seen.append((kwargs.get('mosaic'), kwargs.get('mosaic_scale')))
        raise KeyboardInterrupt                                     # far enough

    monkeypatch.setattr(D.DataIterator, '__init__', spy)
    monkeypatch.setattr(cli, 'load_model', lambda args, verbose=False: (Model('ResNet18FPN', classes=3), {}))
    base = ['train', 'm.pth', '--annotations', ANN, '--images', HERE]
    for argv, want in ((base + ['--mosaic', '0.5', '--mosaic-scale', '0.6', '0.7'], (0.5, (0.6, 0.7))), (base + ['--mosaic', '1'], (1.0, (0.5, 1.0))),
                       (base, (None, None))):
        with pytest.raises(KeyboardInterrupt):
            cli.worker(0, cli.parse(argv), 1)
        assert seen[-1] == want, argv


# -- the C ABI on the host ----------------------------------------------------------------------------------------------------------
def test_entry_point_validates_without_a_gpu():
    lib = _C.library()
    assert lib.odtk_abi_struct_size(14) == ctypes.sizeof(_C.MosaicTile) == D.MOSAIC_TILE_DTYPE.itemsize == 28
    assert lib.odtk_abi_struct_size(15) == ctypes.sizeof(_C.Mosaic) == D.MOSAIC_DTYPE.itemsize == 124
    assert [lib.odtk_abi_struct_size(k) for k in (4, 8, 10, 12, 13, 16)] == [-1] * 6
    assert 'odtk_mosaic_images' in _C.exported_symbols()
    images, mosaics, augments = (_C.Image * 3)(), (_C.Mosaic * 2)(), (_C.Augment * 2)()
    for im in images:                                               # 8 x 4 sources resized to 16 x 4
        im.src_offset, im.src_width, im.src_height, im.src_pitch = 0, 8, 4, 24
        im.out_width, im.out_height, im.x_table, im.y_table, im.x_taps, im.y_taps = 16, 4, 0, -1, 3, 0
    images[2].mirror = 1                                            # allowed here
    for mo, au in zip(mosaics, augments):
        mo.canvas_width, mo.canvas_height, mo.fill = 20, 10, (ctypes.c_uint8 * 3)(114, 114, 114)
        for k, tile in enumerate(mo.tiles):
            tile.source = -1
        mo.tiles[0].source, mo.tiles[0].dst_x, mo.tiles[0].dst_y, mo.tiles[0].width, mo.tiles[0].height = 0, 4, 6, 16, 4
        mo.tiles[3].source, mo.tiles[3].dst_x, mo.tiles[3].dst_y, mo.tiles[3].width, mo.tiles[3].height = 2, 0, 0, 10, 3
        mo.tiles[3].src_x, mo.tiles[3].src_y = 6, 1
        au.canvas_width, au.canvas_height, au.map = 20, 10, (ctypes.c_int32 * 6)(65536, 0, 0, 0, 65536, 0)
        au.flags, au.brightness, au.contrast, au.saturation, au.hue = 15, 1.1, 0.9, 1.2, 3
    tables_len = 16 * 5
    src, tables, norm, out, workspace = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20      # never dereferenced on these paths

    def call(batch=2, mosaics=mosaics, augments=augments, n_images=3, images=images, max_pixels=64, src=src, src_bytes=96, tables=tables,
             tables_len=tables_len, norm=norm, out=out, height=32, width=32, dtype=_C.BF16, workspace=workspace, workspace_bytes=None):
        front = (batch, mosaics, augments, n_images, images, max_pixels, src, src_bytes, tables, tables_len, norm, out, height, width, dtype)
        need = lib.odtk_mosaic_images(*front, None, 0, None)
        if workspace is None or need < 0:
            return need
        return lib.odtk_mosaic_images(*front, workspace, need if workspace_bytes is None else need + workspace_bytes, None)

    # the query: a function of (batch_size, n_images, max_pixels, height, width) alone, the same with null and with dummy pointers
    need = call(workspace=None)
    assert need >= 2 * 8 + 3 * 3 * 64 + 2 * 3 * 32 * 32
    assert call(workspace=None, mosaics=None, augments=None, images=None, src=None, tables=None, norm=None, out=None) == need
    assert call(workspace=None, batch=3) > need and call(workspace=None, n_images=4) > need and call(workspace=None, max_pixels=500) > need
    assert call(workspace=None, height=64) > need and call(workspace=None, width=64) > need
    if not torch.cuda.is_available():                               # (never with a device: the pointers are dummies)
        assert call() == _C.ERR_HIP                                 # valid: it gets as far as the first launch
    assert call(augments=None, workspace=None) == need
    for bad in (dict(mosaics=None), dict(images=None), dict(src=None), dict(norm=None), dict(out=None), dict(batch=0), dict(n_images=0),
                dict(max_pixels=0), dict(height=0), dict(width=0), dict(batch=-1), dict(n_images=-2),
                dict(width=19), dict(height=9),                     # a canvas larger than the batch
                dict(max_pixels=63),                                # a source with more pixels than stated
                dict(n_images=2),                                   # a tile's source beyond the sources
                dict(src_bytes=95), dict(tables_len=tables_len - 1), dict(tables=None), dict(out=out + 1), dict(tables=tables + 2),
                dict(workspace_bytes=-1), dict(workspace=workspace + 8)):
        assert call(**bad) == _C.ERR_INVALID, bad
    assert call(dtype=7) == _C.ERR_UNSUPPORTED and call(dtype=7, workspace=None) == _C.ERR_UNSUPPORTED

    def with_field(target, field, value):
        before = getattr(target, field)
        if isinstance(before, ctypes.Array):                        # (a view of the field: keep a copy)
            before = type(before)(*before)
        setattr(target, field, value)
        result = call()
        setattr(target, field, before)
        return result

    first, last = mosaics[1].tiles[0], mosaics[1].tiles[3]
    for target, field, value in ((mosaics[1], 'canvas_width', 0), (mosaics[1], 'canvas_height', -1), (mosaics[1], 'canvas_width', 33), (mosaics[1], 'pad_', 1),
                                 (first, 'source', -2), (first, 'source', 3), (first, 'dst_x', -1), (first, 'dst_y', -1), (first, 'dst_x', 5),
                                 (first, 'dst_y', 7), (first, 'width', 0), (first, 'height', 0), (first, 'width', -3), (first, 'width', 17),
                                 (first, 'height', 5), (first, 'src_x', 1), (first, 'src_y', 1), (first, 'src_x', -1), (first, 'src_y', -1),
                                 (first, 'width', 0x7fffffff), (first, 'dst_x', 0x7fffffff), (last, 'src_x', 7), (last, 'src_y', 2),
                                 (images[1], 'mirror', 2), (images[1], 'out_width', 0), (images[1], 'x_taps', 0), (images[1], 'src_pitch', 23),
                                 (augments[1], 'canvas_width', 19), (augments[1], 'canvas_height', 11), (augments[1], 'flags', 16),
                                 (augments[1], 'brightness', float('nan')), (augments[1], 'saturation', float('inf')),
                                 (augments[1], 'map', (ctypes.c_int32 * 6)(-65536, 0, 19 * 65536, 0, 65536, 0)),    # a flip: not here
                                 (augments[1], 'pad_', (ctypes.c_uint8 * 3)(0, 1, 0))):
        assert with_field(target, field, value) == _C.ERR_INVALID, (field, value)
    if not torch.cuda.is_available():                               # an unused tile's other fields are not read
        assert with_field(mosaics[0].tiles[1], 'width', -7) == _C.ERR_HIP
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        _C.mosaic_images(torch.zeros(96, dtype=torch.uint8), images, mosaics, augments, torch.zeros(80, dtype=torch.int32),
                         D.normalisation_table(), 32, 32)
