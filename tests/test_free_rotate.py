"""Free-angle rotation augmentation, host half (odtk/data.py: free_rotation_matrix, rotate_bilinear, rotate_points, _rotate_boxes,
augment_free_rotate=(lo, hi)): Pillow's bilinear `Image.rotate` restated in numpy must equal Pillow byte for byte, the loader that
ships the rotation as a descriptor must yield exactly what the host path yields with the same seed, a range of (0, 0) must change
nothing, the boxes must land where the pixels do, and odtk_augment_images_ex must refuse bad records before it touches HIP.  The
GPU half is tests/test_gpu_free_rotate.py."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import torch
from PIL import Image

from odtk import _C
from odtk import box
from odtk import data as D
from odtk import main as cli

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data')
ANN = os.path.join(HERE, 'annotations.json')
ANN_ROT = os.path.join(HERE, 'annotations_rotated.json')
SIZES = [(37, 53), (64, 64), (5, 3), (1, 7), (120, 75)]             # (height, width)
ANGLES = [0, 1, -7.3, 13.37, 30, 45, -45, 89.999, 90, 123.456, 180, -0.001, 359.5]
OPTIONS = dict(rotate_augment=True, augment_brightness=0.3, augment_contrast=0.3, augment_hue=0.1, augment_saturation=0.3)
DATASETS = [(D.CocoDataset, ANN, {}), (D.RotatedCocoDataset, ANN, {}), (D.RotatedCocoDataset, ANN_ROT, {}),
            (D.RotatedCocoDataset, ANN_ROT, {'absolute_angle': True})]
DATASET_IDS = ['axis', 'rotated-plain-file', 'rotated', 'absolute']


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_rotation_equals_pillow(size):
    h, w = size
    pixels = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    pil = Image.fromarray(pixels)
    angles = ANGLES + np.random.default_rng(7).uniform(-180, 180, 60).tolist()
    for angle in angles:
        want = np.array(pil.rotate(angle, resample=Image.BILINEAR))
        got = D.rotate_bilinear(pixels, D.free_rotation_matrix(w, h, angle))
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert int((got != want).sum()) == 0, (size, angle)


def test_matrix_is_the_quarter_turns_and_the_identity_at_zero():
    assert D.free_rotation_matrix(5, 7, 0) == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0) == D.free_rotation_matrix(5, 7, 360.0)
    pixels = np.random.default_rng(3).integers(0, 256, (7, 5, 3), dtype=np.uint8)
    assert np.array_equal(D.rotate_bilinear(pixels, D.free_rotation_matrix(5, 7, 0)), pixels)
    assert np.array_equal(D.rotate_bilinear(pixels, D.free_rotation_matrix(5, 7, 180)), pixels[::-1, ::-1])
    assert D.ROTATION_DTYPE.itemsize == ctypes.sizeof(_C.Rotation) == 56


@pytest.mark.parametrize('cls,ann,extra', DATASETS, ids=DATASET_IDS)
def test_seeded_training_equals_the_host_path(cls, ann, extra):
    """Rotation, quarter turns, flip and the four colour options on: same targets, `random` in the same state after every item,
    and the CPU pipeline over the source pixels and the descriptors gives the host path's batch."""
    kwargs = dict(resize=[96, 160], max_size=220, stride=32, annotations=ann, training=True, augment_free_rotate=(-30, 30), **OPTIONS, **extra)
    host, dev = cls(HERE, **kwargs), cls(HERE, device_augment=True, **kwargs)
    table = D.normalisation_table()
    host_items, dev_items, flips, turns = [], [], set(), set()
    state = random.Random(97).getstate()
    for i in range(20):
        random.setstate(state)
        pixels, target = host[i % 5]
        after_host = random.getstate()
        random.setstate(state)
        source, geometry, dev_target = dev[i % 5]
        assert random.getstate() == after_host, 'item %d' % i
        state = after_host
        assert dev_target.dtype == torch.float32 and torch.equal(target, dev_target), 'item %d' % i
        assert len(geometry) == 13 and geometry[2] == 0 and pixels.shape[:2] == (geometry[4], geometry[3])
        flips.add(int(geometry[12]))
        turns.add(tuple(1 if c > 0 else -1 if c < 0 else 0 for c in geometry[5][:2]))
        host_items.append((pixels, target))
        dev_items.append((source, geometry, dev_target))
    assert flips == {0, 1} and len(turns) == 4                     # the map holds the turn alone: four of them, never mirrored
    for at in range(0, 20, 5):
        packed, targets = host.collate_fn(host_items[at:at + 5])
        buffer, dev_targets = dev.collate_fn(dev_items[at:at + 5])
        assert torch.equal(targets, dev_targets)
        batch = D.SourceBatch(buffer)
        assert batch.rotations is not None and all(batch.rotations['enabled'] == 1)
        assert (batch.height, batch.width) == tuple(packed.shape[1:3])
        want, got = D.normalise_batch(packed, table), batch.apply_cpu(table)
        assert torch.equal(want, got) and torch.equal(torch.signbit(want), torch.signbit(got)), at


def test_an_angle_of_zero_from_a_range_still_takes_the_rotation_path():
    ds = D.CocoDataset(HERE, 128, 200, 32, annotations=ANN, training=True, device_augment=True, augment_free_rotate=(0, 1e-300))
    random.seed(3)
    source, geometry, target = ds[0]
    assert len(geometry) == 13 and geometry[11][:2] == (1.0, 0.0)
    buffer, _ = ds.collate_fn([(source, geometry, target)])
    batch = D.SourceBatch(buffer)
    assert batch.rotations is not None and int(batch.rotations[0]['enabled']) == 1
    plain = D.SourceBatch(D.SourceBatch.pack([source], [geometry[:11]], 32))
    if geometry[12]:
        return                                                      # (the flip is not in the map: nothing to compare with)
    assert torch.equal(batch.apply_cpu(D.normalisation_table()), plain.apply_cpu(D.normalisation_table()))


@pytest.mark.parametrize('cls,ann,extra', DATASETS, ids=DATASET_IDS)
@pytest.mark.parametrize('device_augment', [False, True], ids=['host', 'descriptors'])
def test_off_is_off(cls, ann, extra, device_augment, monkeypatch):
    """(0, 0): the same items, the same packed bytes and the same state of `random` as without the keyword."""
    monkeypatch.setattr(D, '_batch_buffer', lambda shape: torch.zeros(shape, dtype=torch.uint8))      # (alignment gaps are not written)
    kwargs = dict(resize=[96, 160], max_size=220, stride=32, annotations=ann, training=True, device_augment=device_augment, **OPTIONS, **extra)
    results = []
    for more in ({}, {'augment_free_rotate': (0, 0)}, {'augment_free_rotate': [0.0, 0.0]}):
        ds = cls(HERE, **kwargs, **more)
        assert ds.augment_free_rotate is None
        random.seed(1234)
        items = [ds[i % 5] for i in range(10)]
        results.append((items, ds.collate_fn(items[:5]), random.getstate()))
    for items, (packed, targets), state in results[1:]:
        assert state == results[0][2]
        assert torch.equal(packed, results[0][1][0]) and torch.equal(targets, results[0][1][1])
        for a, b in zip(items, results[0][0]):
            assert len(a) == len(b) and torch.equal(a[0], b[0]) and torch.equal(a[-1], b[-1])
            if device_augment:
                assert a[1] == b[1] and len(a[1]) == 11
    if device_augment:
        header = results[1][1][0].numpy()[:32].view(np.int32)
        assert header[5] != 0 and header[6] == 0 and D.SourceBatch(results[1][1][0]).rotations is None


def test_the_iterator_takes_the_range_and_says_so():
    args = (HERE, [96, 160], 220, 5, 32, 1, ANN)
    off = D.DataIterator(*args, training=True, num_workers=0, device='cpu')
    assert 'free rotation' not in repr(off)
    batches = []
    for device_augment in (False, True):
        it = D.DataIterator(*args, training=True, num_workers=0, device='cpu', device_augment=device_augment, augment_free_rotate=(-30, 30), **OPTIONS)
        assert 'free rotation: -30 to 30 degrees' in repr(it) and it.dataset.augment_free_rotate == (-30.0, 30.0)
        random.seed(5)
        torch.manual_seed(5)
        batches.append([b for _ in range(2) for b in it])
    for (a, ta), (b, tb) in zip(*batches):
        assert a.shape == b.shape and a.stride() == b.stride() and torch.equal(a, b) and torch.equal(ta, tb)
    with pytest.raises(ValueError, match='augment_free_rotate'):
        D.DataIterator(*args, training=True, num_workers=0, device='cpu', device_resize=True, augment_free_rotate=(-5, 5))
    D.DataIterator(*args, training=True, num_workers=0, device='cpu', device_resize=True, augment_free_rotate=(0, 0))
    for bad in ((1, 2, 3), (5, -5), (0, float('inf'))):
        with pytest.raises(ValueError, match='augment_free_rotate'):
            D.CocoDataset(HERE, 128, 200, 32, annotations=ANN, training=True, augment_free_rotate=bad)


# -- boxes -----------------------------------------------------------------------------------------------------------------------
CANVAS = (96, 64)                                                   # (width, height)


def _dataset(cls, **extra):
    return cls(HERE, 128, 200, 32, annotations=ANN, training=True, augment_free_rotate=(-1, 1), **extra)


def _inside_quad(quad, xs, ys, grow):
    """Pixel centres (xs, ys) inside the convex quad [4, 2] (any orientation) grown by `grow` pixels."""
    quad = np.asarray(quad, dtype=np.float64)
    centre = quad.mean(0)
    inside = np.ones(len(xs), dtype=bool)
    for k in range(4):
        p, q = quad[k], quad[(k + 1) % 4]
        normal = np.array([q[1] - p[1], p[0] - q[0]])
        normal /= np.linalg.norm(normal)
        if np.dot(centre - p, normal) > 0:
            normal = -normal                                        # outward
        inside &= (xs - p[0]) * normal[0] + (ys - p[1]) * normal[1] <= grow
    return inside


@pytest.mark.parametrize('angle', [17, -33, 90])
def test_axis_aligned_boxes_follow_the_pixels(angle):
    """One pixel is the support of a bilinear tap: a pixel above 127 has more than half of its weight on painted pixels, so its
    centre lies within a pixel of the painted rectangle's image."""
    w, h = CANVAS
    ds = _dataset(D.CocoDataset)
    x0, y0, bw, bh = 30, 20, 36, 18
    pixels = np.zeros((h, w, 3), dtype=np.uint8)
    pixels[y0:y0 + bh, x0:x0 + bw] = 255
    im, boxes, categories = ds._free_rotate(Image.fromarray(pixels), torch.tensor([[x0, y0, bw, bh]], dtype=torch.float32), torch.zeros(1, 1), angle)
    assert boxes.dtype == torch.float32 and boxes.shape == (1, 4) and categories.shape == (1, 1)
    ys, xs = np.nonzero(np.array(im)[..., 0] > 127)
    assert len(xs) > 0.8 * bw * bh
    bx, by, bw2, bh2 = (float(v) for v in boxes[0])
    assert xs.min() + 0.5 >= bx - 1 and xs.max() + 0.5 <= bx + bw2 + 1 and ys.min() + 0.5 >= by - 1 and ys.max() + 0.5 <= by + bh2 + 1
    assert abs(xs.min() - bx) <= 1 and abs(xs.max() + 1 - (bx + bw2)) <= 1          # pixel k covers [k, k + 1]
    assert abs(ys.min() - by) <= 1 and abs(ys.max() + 1 - (by + bh2)) <= 1


@pytest.mark.parametrize('absolute', [False, True], ids=['folded', 'absolute'])
@pytest.mark.parametrize('angle', [17, -33, 90])
def test_rotated_boxes_follow_the_pixels(angle, absolute):
    w, h = CANVAS
    ds = _dataset(D.RotatedCocoDataset, absolute_angle=absolute)
    start = torch.tensor([[34.0, 22.0, 30.0, 14.0, 0.3]])
    _, quad = box.rotate_boxes(start.clone())
    quad = quad.view(4, 2).numpy().astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    painted = _inside_quad(quad, xx.ravel() + 0.5, yy.ravel() + 0.5, 0.0).reshape(h, w)
    pixels = np.zeros((h, w, 3), dtype=np.uint8)
    pixels[painted] = 255
    im, boxes, categories = ds._free_rotate(Image.fromarray(pixels), start.clone(), torch.zeros(1, 1), angle)
    assert boxes.dtype == torch.float32 and boxes.shape == (1, 5)
    _, moved = box.rotate_boxes(boxes.clone())
    ys, xs = np.nonzero(np.array(im)[..., 0] > 127)
    assert len(xs) > 0.8 * painted.sum()
    assert _inside_quad(moved.view(4, 2).numpy(), xs + 0.5, ys + 0.5, 1.0).all()
    assert not _inside_quad(moved.view(4, 2).numpy(), xs + 0.5, ys + 0.5, -1.5).all()          # ... and no larger than the pixels
    theta = float(boxes[0, 4])
    want = 0.3 + math.radians(angle % 360.0)
    if absolute:
        assert theta == pytest.approx(math.fmod(want, math.pi), abs=1e-6)
    else:
        assert -math.pi / 4 <= theta <= math.pi / 4 and math.sin(2 * (theta - want)) == pytest.approx(0, abs=1e-5)
        assert (float(boxes[0, 2]), float(boxes[0, 3])) == ((14.0, 30.0) if round(want / (math.pi / 2)) % 2 else (30.0, 14.0))
    cx, cy = float(boxes[0, 0] + boxes[0, 2] / 2), float(boxes[0, 1] + boxes[0, 3] / 2)
    assert abs(cx - (xs.mean() + 0.5)) < 1 and abs(cy - (ys.mean() + 0.5)) < 1


def test_boxes_pushed_out_of_the_canvas_are_dropped():
    w, h = CANVAS
    axis = _dataset(D.CocoDataset)
    boxes = torch.tensor([[1.0, 1.0, 6.0, 5.0], [40.0, 26.0, 12.0, 10.0], [90.0, 59.0, 5.0, 4.0]])
    categories = torch.tensor([[0.0], [1.0], [2.0]])
    kept, cats = axis._rotate_boxes(boxes.clone(), categories, 45, w, h)         # the corners of 96 x 64 leave the canvas at 45 degrees
    assert kept.shape == (1, 4) and cats.tolist() == [[1.0]]
    kept, cats = axis._rotate_boxes(boxes[::2].clone(), categories[::2], 45, w, h)
    assert torch.equal(kept, torch.ones(1, 4)) and torch.equal(cats, -torch.ones(1, 1))       # the "no box" row
    none_boxes, none_cats = axis._get_target(10 ** 9)
    assert torch.equal(kept, none_boxes) and torch.equal(cats, none_cats)
    # a box that stays partly inside is clipped to the canvas, and dropped once less than a pixel is left
    kept, cats = axis._rotate_boxes(torch.tensor([[0.0, 20.0, 10.0, 10.0]]), torch.zeros(1, 1), 180, w, h)
    assert kept.tolist() == [[86.0, 34.0, 10.0, 10.0]]
    kept, cats = axis._rotate_boxes(torch.tensor([[-9.5, 20.0, 10.0, 10.0]]), torch.zeros(1, 1), 0, w, h)
    assert cats.tolist() == [[-1.0]]
    kept, cats = axis._rotate_boxes(torch.tensor([[-9.0, 20.0, 10.0, 10.0]]), torch.zeros(1, 1), 0, w, h)
    assert kept.tolist() == [[0.0, 20.0, 1.0, 10.0]] and cats.tolist() == [[0.0]]

    rotated = _dataset(D.RotatedCocoDataset)
    boxes = torch.tensor([[1.0, 1.0, 6.0, 5.0, 0.1], [40.0, 26.0, 12.0, 10.0, -0.2], [90.0, 59.0, 5.0, 4.0, 0.0]])
    kept, cats = rotated._rotate_boxes(boxes.clone(), categories, 45, w, h)
    assert kept.shape == (1, 5) and cats.tolist() == [[1.0]]
    kept, cats = rotated._rotate_boxes(boxes[::2].clone(), categories[::2], 45, w, h)
    assert torch.equal(kept, torch.ones(1, 5)) and torch.equal(cats, -torch.ones(1, 1))


def test_theta_folds_at_a_quarter_of_pi():
    w, h = CANVAS
    ds = _dataset(D.RotatedCocoDataset)
    quarter = math.pi / 4
    for theta, angle, folded, swapped in ((0.0, 44.0, math.radians(44), False), (0.0, 46.0, math.radians(46) - math.pi / 2, True),
                                         (0.0, -44.0, -math.radians(44), False), (0.0, -46.0, math.pi / 2 - math.radians(46), True),
                                         (0.0, 45.0, quarter, False), (0.0, -45.0, -quarter, False),      # the ends belong to the range
                                         (0.2, 135.0, 0.2 + 3 * quarter - math.pi, False), (0.3, 70.0, 0.3 + math.radians(70) - math.pi / 2, True),
                                         (-0.1, 180.0, -0.1, False)):
        kept, _ = ds._rotate_boxes(torch.tensor([[40.0, 26.0, 12.0, 10.0, theta]]), torch.zeros(1, 1), angle, w, h)
        assert float(kept[0, 4]) == pytest.approx(folded, abs=1e-6), (theta, angle)
        assert -quarter - 1e-7 <= float(kept[0, 4]) <= quarter + 1e-7
        assert (float(kept[0, 2]), float(kept[0, 3])) == ((10.0, 12.0) if swapped else (12.0, 10.0)), (theta, angle)
        centre = (float(kept[0, 0] + kept[0, 2] / 2), float(kept[0, 1] + kept[0, 3] / 2))
        want = D.rotate_points(torch.tensor(46.0, dtype=torch.float64), torch.tensor(31.0, dtype=torch.float64), w, h, angle)
        assert centre == pytest.approx((float(want[0]), float(want[1])), abs=1e-4)
    absolute = _dataset(D.RotatedCocoDataset, absolute_angle=True)
    kept, _ = absolute._rotate_boxes(torch.tensor([[40.0, 26.0, 12.0, 10.0, 0.25]]), torch.zeros(1, 1), 100.0, w, h)
    assert float(kept[0, 4]) == pytest.approx(0.25 + math.radians(100), abs=1e-6) and kept[0, 2:4].tolist() == [12.0, 10.0]
    kept, _ = absolute._rotate_boxes(torch.tensor([[40.0, 26.0, 12.0, 10.0, 0.25]]), torch.zeros(1, 1), -10.0, w, h)
    assert float(kept[0, 4]) == pytest.approx(0.25 + math.radians(350) - 2 * math.pi, abs=1e-6)    # wrapped as `_turn_boxes` wraps


# -- the C ABI, without a GPU -------------------------------------------------------------------------------------------------------
def test_entry_point_validates_without_a_gpu():
    lib = _C.library()
    assert lib.odtk_abi_struct_size(7) == ctypes.sizeof(_C.Rotation) == 56 and lib.odtk_abi_struct_size(8) == -1
    assert 'odtk_augment_images_ex' in _C.exported_symbols()
    images, augments, rotations = (_C.Image * 2)(), (_C.Augment * 2)(), (_C.Rotation * 2)()
    for im, au, ro in zip(images, augments, rotations):
        im.src_offset, im.src_width, im.src_height, im.src_pitch = 0, 8, 4, 24
        im.out_width, im.out_height, im.x_table, im.y_table, im.x_taps, im.y_taps = 16, 4, 0, -1, 3, 0
        au.canvas_width, au.canvas_height, au.map = 4, 16, (ctypes.c_int32 * 6)(0, -65536, 15 * 65536, 65536, 0, 0)
        au.flags, au.brightness, au.contrast, au.saturation, au.hue = 15, 1.1, 0.9, 1.2, 3
        ro.matrix, ro.enabled, ro.flip = (ctypes.c_double * 6)(*D.free_rotation_matrix(4, 16, 12.5)), 1, 1
    tables_len = 16 * 5
    src, tables, norm, out, workspace = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20      # never dereferenced on these paths

    def call(batch=2, images=images, augments=augments, rotations=rotations, src=src, src_bytes=96, tables=tables, tables_len=tables_len,
             norm=norm, out=out, height=32, width=32, dtype=_C.BF16, workspace=workspace, workspace_bytes=None):
        need = lib.odtk_augment_images_ex(batch, images, augments, rotations, src, src_bytes, tables, tables_len, norm, out, height, width,
                                          dtype, None, 0, None)
        if workspace is None or need < 0:
            return need
        return lib.odtk_augment_images_ex(batch, images, augments, rotations, src, src_bytes, tables, tables_len, norm, out, height, width,
                                          dtype, workspace, need if workspace_bytes is None else need + workspace_bytes, None)

    def plain(batch=2, images=images, augments=augments, src=src, src_bytes=96, tables=tables, tables_len=tables_len, norm=norm, out=out,
              height=32, width=32, dtype=_C.BF16, workspace=workspace, workspace_bytes=None):
        need = lib.odtk_augment_images(batch, images, augments, src, src_bytes, tables, tables_len, norm, out, height, width, dtype, None, 0, None)
        if workspace is None or need < 0:
            return need
        return lib.odtk_augment_images(batch, images, augments, src, src_bytes, tables, tables_len, norm, out, height, width, dtype,
                                       workspace, need if workspace_bytes is None else need + workspace_bytes, None)

    # its own workspace query: a second slot per image; without records, the query and every refusal of odtk_augment_images
    need, need_plain = call(workspace=None), plain(workspace=None)
    assert need >= need_plain + 2 * 3 * 32 * 32 and call(workspace=None, rotations=None) == need_plain
    assert call(workspace=None, batch=4) > need
    refused = (dict(images=None), dict(augments=None), dict(src=None), dict(norm=None), dict(out=None), dict(batch=0), dict(height=0),
               dict(width=0), dict(width=3), dict(height=15), dict(src_bytes=95), dict(tables_len=tables_len - 1), dict(tables=None),
               dict(out=out + 1), dict(tables=tables + 2), dict(workspace_bytes=-1), dict(workspace=workspace + 8))
    for bad in refused:
        assert call(**bad) == _C.ERR_INVALID, bad
        assert call(rotations=None, **bad) == plain(**bad) == _C.ERR_INVALID, bad
    assert call(dtype=7) == call(dtype=7, rotations=None) == _C.ERR_UNSUPPORTED
    # a workspace that is enough for odtk_augment_images is not enough here
    assert lib.odtk_augment_images_ex(2, images, augments, rotations, src, 96, tables, tables_len, norm, out, 32, 32, _C.BF16, workspace,
                                      need_plain, None) == _C.ERR_INVALID
    for field, value in (('enabled', 2), ('enabled', -1), ('flip', 2), ('flip', -1)):
        before = getattr(rotations[1], field)
        setattr(rotations[1], field, value)
        assert call() == _C.ERR_INVALID, (field, value)
        setattr(rotations[1], field, before)
    for k in range(6):
        for value in (float('nan'), float('inf'), -float('inf')):
            before = rotations[0].matrix[k]
            rotations[0].matrix[k] = value
            assert call() == _C.ERR_INVALID, (k, value)
            rotations[0].matrix[k] = before
    rotations[1].enabled = 0                                        # flip without a rotation: the flip of such an image is in its map
    assert call() == _C.ERR_INVALID
    rotations[1].enabled = 1
    augments[1].canvas_width = 33                                   # ... and the augment records are still checked
    assert call() == _C.ERR_INVALID
    augments[1].canvas_width = 4
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        _C.augment_images(torch.zeros(96, dtype=torch.uint8), images, augments, torch.zeros(80, dtype=torch.int32),
                          D.normalisation_table(), 32, 32, rotations=rotations)


# -- the command line -------------------------------------------------------------------------------------------------------------
def test_cli_trains_with_the_rotation_on_both_paths(tmp_path, capsys, monkeypatch):
    """On the CPU, also where a GPU is present: the descriptor path is then the numpy one, and the two runs see the same batches."""
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(torch.cuda, 'device_count', lambda: 0)
    assert cli.parse(['train', 'm.pth', '--annotations', 'a.json']).augment_free_rotate == [0, 0]
    before = torch.get_num_threads()
    torch.set_num_threads(4)
    losses = []
    try:
        for k, more in enumerate(([], ['--device-augment'])):
            random.seed(11)
            torch.manual_seed(11)
            argv = ['train', str(tmp_path / ('m%d.pth' % k)), '--annotations', ANN, '--images', HERE, '--backbone', 'ResNet18FPN', '--classes', '3',
                    '--batch', '2', '--resize', '128', '--max-size', '160', '--jitter', '96', '128', '--warmup', '1', '--lr', '0.001',
                    '--full-precision', '--workers', '0', '--augment-rotate', '--augment-free-rotate', '-10', '10', '--iters', '2']
            done, _ = cli.main(argv + more)
            out = capsys.readouterr().out
            assert done == 2 and 'free rotation: -10 to 10 degrees' in out and 'device: 1 cpu' in out
            assert ('augmentations on: the host (numpy)' in out) == bool(more)
            losses.append(re.findall(r'focal loss: ([-0-9.naninf]+), box loss: ([-0-9.naninf]+)', out))
    finally:
        torch.set_num_threads(before)
    assert len(losses[0]) >= 1 and losses[0] == losses[1]
    assert all(math.isfinite(float(v)) for pair in losses[0] for v in pair)
