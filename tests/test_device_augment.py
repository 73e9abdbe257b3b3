"""Device-side training augmentations, host half (odtk/data.py: quarter_turn_map, index_map, blend, contrast_mean, rgb_to_hsv,
hsv_to_rgb, device_augment=True): Pillow's quarter turns and colour enhancements restated in numpy must equal Pillow bit for bit,
and the loader mode that ships source pixels with augment descriptors must yield exactly what the host path yields with the same
seed.  Every comparison is equality over every element.  The GPU half is tests/test_gpu_device_augment.py."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from odtk import _C
from odtk import data as D
from odtk import main as cli
from odtk.model import Model

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data')
ANN = os.path.join(HERE, 'annotations.json')
ANN_ROT = os.path.join(HERE, 'annotations_rotated.json')
ONE = np.float32(1)
BLEND_FACTORS = [0, 1, float(np.nextafter(ONE, np.float32(0))), float(np.nextafter(ONE, np.float32(2))), 0.3, 1.21, 2.5, 40]
ENHANCE_FACTORS = [0, 0.3, 0.77, 0.999, 1, 1.0001, 1.21, 1.9, 2.5]
TURN_SIZES = [(9, 2), (2, 9), (33, 32), (32, 33), (16, 16), (1, 9), (9, 1), (131, 97), (7, 7)]      # (width, height)
OPTIONS = dict(rotate_augment=True, augment_brightness=0.3, augment_contrast=0.3, augment_hue=0.1, augment_saturation=0.3)


def all_colours():
    """Every 8-bit triple once, as a 4096 x 4096 x 3 image."""
    g = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([g >> 16, (g >> 8) & 255, g & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def noise(width, height, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == 'noise':
        return rng.integers(0, 256, (height, width, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (height, width, 3), dtype=np.uint8) * 255).astype(np.uint8)


def boundary_images():
    """[(pixels, grey level Pillow's Contrast uses)]: grey images (L == the byte) whose mean of L is exactly k + 0.5, and one
    pixel's worth below it -- where int(mean + 0.5) changes."""
    out = []
    for (w, h), k in (((8, 6), 100), ((64, 50), 0), ((130, 34), 254), ((1066, 800), 127)):
        for below in (0, 1):
            grey = np.full(w * h, k, dtype=np.uint8)
            grey[:w * h // 2 - below] = k + 1                        # (w h / 2) bytes k + 1 and as many k: the mean is k + 1/2
            pixels = np.repeat(np.random.default_rng(k).permutation(grey).reshape(h, w, 1), 3, axis=2)
            out.append((pixels, k if below else k + 1))
    return out


def test_hsv_conversions_equal_pillow_on_all_colours():
    colours = all_colours()
    want_hsv = np.array(Image.fromarray(colours).convert('HSV'))
    want_rgb = np.array(Image.fromarray(colours, 'HSV').convert('RGB'))
    for at in range(0, 4096, 512):                                  # strips: the restatement holds doubles
        strip = colours[at:at + 512]
        assert np.array_equal(D.rgb_to_hsv(strip), want_hsv[at:at + 512]), at
        assert np.array_equal(D.hsv_to_rgb(strip), want_rgb[at:at + 512]), at


@pytest.mark.parametrize('factor', BLEND_FACTORS + [1 + 1e-12])
def test_blend_equals_pillow_on_all_byte_pairs(factor):
    d, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    want = np.array(Image.blend(Image.fromarray(d), Image.fromarray(x), factor))
    assert np.array_equal(D.blend(d, x, factor), want)


@pytest.mark.parametrize('kind', ['noise', 'binary'])
def test_enhancements_equal_pillow(kind):
    for k, (w, h) in enumerate([(37, 53), (64, 16), (1, 9)]):
        pixels = noise(w, h, kind, 10 + k)
        pil = Image.fromarray(pixels)
        for factor in ENHANCE_FACTORS:
            assert np.array_equal(D.adjust_brightness(pixels, factor), np.array(ImageEnhance.Brightness(pil).enhance(factor))), factor
            assert np.array_equal(D.adjust_contrast(pixels, factor), np.array(ImageEnhance.Contrast(pil).enhance(factor))), factor
            assert np.array_equal(D.adjust_saturation(pixels, factor), np.array(ImageEnhance.Color(pil).enhance(factor))), factor
        for factor in (-0.5, -0.2, 0, 0.004, 0.1, 0.5):
            assert np.array_equal(D.adjust_hue(pixels, D.hue_shift_byte(factor)), np.array(D._adjust_hue(pil, factor))), factor


def test_contrast_mean_at_the_half_integer_boundary():
    for pixels, want in boundary_images():
        pil = Image.fromarray(pixels)
        assert D.contrast_mean(pixels) == want
        assert np.array(ImageEnhance.Contrast(pil).enhance(0)).flat[0] == want          # factor 0: the degenerate image itself
        assert np.array_equal(D.adjust_contrast(pixels, 1.7), np.array(ImageEnhance.Contrast(pil).enhance(1.7)))


def test_quarter_turns_equal_pillow():
    for k, (w, h) in enumerate(TURN_SIZES):
        pixels = np.random.default_rng(k).integers(1, 256, (h, w, 3), dtype=np.uint8)     # no byte 0: black is the turn's
        pil = Image.fromarray(pixels)
        for angle in (0, 90, 180, 270):
            for expand in (False, True):
                for flip in (False, True):
                    want = pil.rotate(angle, expand=expand)
                    if flip:
                        want = want.transpose(Image.FLIP_LEFT_RIGHT)
                    cw, ch, coefficients = D.quarter_turn_map(w, h, angle, expand, flip)
                    assert (cw, ch) == want.size, (w, h, angle, expand)
                    assert np.array_equal(D.index_map(pixels, cw, ch, coefficients), np.array(want)), (w, h, angle, expand, flip)
    assert D.quarter_turn_map(5, 7, 0) == (5, 7, (65536, 0, 0, 0, 65536, 0))
    cw, ch, coefficients = D.quarter_turn_map(8, 2, 90)             # a non-square turn without expand cuts the corners: black
    assert (D.index_map(np.full((2, 8, 3), 9, dtype=np.uint8), cw, ch, coefficients) == 0).sum() == 3 * 12
    with pytest.raises(ValueError):
        D.quarter_turn_map(5, 7, 45)


@pytest.mark.parametrize('cls,ann,extra', [(D.CocoDataset, ANN, {}), (D.RotatedCocoDataset, ANN_ROT, {}),
                                           (D.RotatedCocoDataset, ANN_ROT, {'absolute_angle': True})], ids=['axis', 'rotated', 'absolute'])
def test_seeded_training_equals_the_host_path(cls, ann, extra):
    """All five options on: same targets, `random` in the same state after every item, and the CPU pipeline over the source
    pixels and the descriptors gives the host path's batch."""
    kwargs = dict(resize=[96, 160], max_size=220, stride=32, annotations=ann, training=True, **OPTIONS, **extra)
    host, dev = cls(HERE, **kwargs), cls(HERE, device_augment=True, **kwargs)
    table = D.normalisation_table()
    host_items, dev_items, maps, swapped, black = [], [], set(), 0, 0
    state = random.Random(4321).getstate()
    for i in range(40):
        random.setstate(state)
        pixels, target = host[i % 5]
        after_host = random.getstate()
        random.setstate(state)
        source, geometry, dev_target = dev[i % 5]
        assert random.getstate() == after_host, 'item %d' % i
        state = after_host
        assert torch.equal(target, dev_target), 'item %d' % i
        ow, oh, mirror, cw, ch, coefficients, flags = geometry[:7]
        assert source.shape[2] == 3 and mirror == 0 and flags == 15 and pixels.shape[:2] == (ch, cw)
        maps.add(tuple(1 if c > 0 else -1 if c < 0 else 0 for c in (coefficients[0], coefficients[1], coefficients[3], coefficients[4])))
        swapped += (cw, ch) == (oh, ow) and ow != oh
        black += (cw, ch) == (ow, oh) and ow != oh and coefficients[0] == 0
        host_items.append((pixels, target))
        dev_items.append((source, geometry, dev_target))
    assert len(maps) == 8                                           # four turns, each mirrored and not
    assert (swapped > 0) == cls.turn_expands and (black > 0) != cls.turn_expands
    for at in range(0, 40, 5):
        packed, targets = host.collate_fn(host_items[at:at + 5])
        buffer, dev_targets = dev.collate_fn(dev_items[at:at + 5])
        assert torch.equal(targets, dev_targets)
        batch = D.SourceBatch(buffer)
        assert batch.augments is not None and (batch.height, batch.width) == tuple(packed.shape[1:3])
        want, got = D.normalise_batch(packed, table), batch.apply_cpu(table)
        assert torch.equal(want, got) and torch.equal(torch.signbit(want), torch.signbit(got)), at


@pytest.mark.parametrize('cls,ann,extra', [(D.DataIterator, ANN, {}), (D.RotatedDataIterator, ANN_ROT, {}),
                                           (D.RotatedDataIterator, ANN_ROT, {'absolute_angle': True})], ids=['axis', 'rotated', 'absolute'])
def test_seeded_training_iterators_agree(cls, ann, extra):
    args = (HERE, [96, 160], 220, 5, 32, 1, ann)
    batches = []
    for device_augment in (False, True):
        it = cls(*args, training=True, num_workers=0, device='cpu', device_augment=device_augment, **OPTIONS, **extra)
        assert ('augmentations on: the host (numpy)' in repr(it)) == device_augment
        random.seed(77)
        torch.manual_seed(77)
        batches.append([b for _ in range(3) for b in it])
    assert len(batches[0]) == len(batches[1]) == 3
    for (a, ta), (b, tb) in zip(*batches):
        assert a.shape == b.shape and a.stride() == b.stride() and torch.equal(a, b) and torch.equal(ta, tb)


def test_inference_items_are_those_of_device_resize():
    plain = D.CocoDataset(HERE, 128, 200, 32, annotations=ANN, training=False, device_resize=True)
    augmented = D.CocoDataset(HERE, 128, 200, 32, annotations=ANN, training=False, device_augment=True)
    a, b = plain.collate_fn([plain[0], plain[1]]), augmented.collate_fn([augmented[0], augmented[1]])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    first, second = D.SourceBatch(a[0]), D.SourceBatch(b[0])       # (the buffers' alignment gaps are uninitialised)
    assert second.augments is None and np.array_equal(first.images, second.images)
    assert torch.equal(first.apply_cpu(D.normalisation_table()), second.apply_cpu(D.normalisation_table()))


def test_plain_and_augmented_images_share_a_batch():
    """A plain (out_width, out_height, mirror) geometry in an augmented batch gets the identity (or mirror) map and no flags."""
    a, b = noise(37, 21, 'noise', 1), noise(16, 16, 'noise', 2)
    turned = (50, 30, 0) + D.quarter_turn_map(50, 30, 90, True, False) + (D.AUGMENT_HUE, 1.0, 1.0, 1.0, 9)
    buffer = D.SourceBatch.pack([torch.from_numpy(a), torch.from_numpy(b)], [turned, (16, 16, 1)], 32)
    batch = D.SourceBatch(buffer)
    assert (batch.height, batch.width) == (64, 32) and ctypes.sizeof(_C.Augment) == D.AUGMENT_DTYPE.itemsize == 52
    assert tuple(batch.augments[1]['map']) == (-65536, 0, 15 * 65536, 0, 65536, 0) and batch.augments[1]['flags'] == 0
    out = batch.apply_cpu(D.normalisation_table())
    first = D.adjust_hue(np.array(Image.fromarray(a).resize((50, 30), Image.BILINEAR).rotate(90, expand=True)), 9)
    packed = torch.zeros(2, 64, 32, 4, dtype=torch.uint8)
    packed[0, :50, :30, :3], packed[0, :50, :30, 3] = torch.from_numpy(first), 255
    packed[1, :16, :16, :3], packed[1, :16, :16, 3] = torch.from_numpy(b[:, ::-1].copy()), 255
    assert torch.equal(out, D.normalise_batch(packed))


@pytest.mark.parametrize('option', ['rotate_augment', 'augment_brightness', 'augment_contrast', 'augment_hue', 'augment_saturation'])
def test_each_option_is_accepted(option):
    value = True if option == 'rotate_augment' else 0.01
    ds = D.CocoDataset(HERE, 128, 200, 32, annotations=ANN, training=True, device_augment=True, **{option: value})
    assert ds.device_augment and ds.device_resize
    random.seed(5)
    source, geometry, target = ds[0]
    assert len(geometry) == 11 and source.shape[2] == 3
    it = D.RotatedDataIterator(HERE, 128, 200, 2, 32, 1, ANN_ROT, training=True, device='cpu', num_workers=0, device_augment=True,
                               **{option: value})
    assert it.device_augment and it.dataset.device_augment


def test_cli_switch_is_absent_unless_given_and_reaches_the_iterator(monkeypatch):
    assert 'device_augment' not in vars(cli.parse(['train', 'm.pth', '--annotations', 'a.json']))
    assert cli.parse(['train', 'm.pth', '--annotations', 'a.json', '--device-augment']).device_augment is True
    with pytest.raises(SystemExit):
        cli.parse(['infer', 'm.pth', '--device-augment'])
    seen = []

    def spy(self, *args, **kwargs):
        seen.append((kwargs.get('device_augment'), kwargs.get('augment_hue')))
        raise KeyboardInterrupt                                     # far enough

    monkeypatch.setattr(D.DataIterator, '__init__', spy)
    monkeypatch.setattr(cli, 'load_model', lambda args, verbose=False: (Model('ResNet18FPN', classes=3), {}))
    base = ['train', 'm.pth', '--annotations', ANN, '--images', HERE, '--augment-hue', '0.1']
    for argv, want in ((base + ['--device-augment'], True), (base, False)):
        with pytest.raises(KeyboardInterrupt):
            cli.worker(0, cli.parse(argv), 1)
        assert seen[-1] == (want, 0.1), argv


def test_entry_point_validates_without_a_gpu():
    lib = _C.library()
    assert lib.odtk_abi_struct_size(6) == ctypes.sizeof(_C.Augment) == 52 and lib.odtk_abi_struct_size(5) == 48
    images, augments = (_C.Image * 2)(), (_C.Augment * 2)()
    for im, au in zip(images, augments):
        im.src_offset, im.src_width, im.src_height, im.src_pitch = 0, 8, 4, 24
        im.out_width, im.out_height, im.x_table, im.y_table, im.x_taps, im.y_taps = 16, 4, 0, -1, 3, 0
        au.canvas_width, au.canvas_height, au.map = 4, 16, (ctypes.c_int32 * 6)(0, -65536, 15 * 65536, 65536, 0, 0)
        au.flags, au.brightness, au.contrast, au.saturation, au.hue = 15, 1.1, 0.9, 1.2, 3
    tables_len = 16 * 5
    src, tables, norm, out, workspace = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20      # never dereferenced on these paths

    def call(batch=2, images=images, augments=augments, src=src, src_bytes=96, tables=tables, tables_len=tables_len, norm=norm, out=out,
             height=32, width=32, dtype=_C.BF16, workspace=workspace, workspace_bytes=None):
        need = lib.odtk_augment_images(batch, images, augments, src, src_bytes, tables, tables_len, norm, out, height, width, dtype,
                                       None, 0, None)
        if workspace is None or need < 0:
            return need
        return lib.odtk_augment_images(batch, images, augments, src, src_bytes, tables, tables_len, norm, out, height, width, dtype,
                                       workspace, need if workspace_bytes is None else need + workspace_bytes, None)

    need = call(workspace=None)
    assert need >= 2 * 3 * 32 * 32 + 16 and call(workspace=None, batch=4) > need
    for bad in (dict(images=None), dict(augments=None), dict(src=None), dict(norm=None), dict(out=None), dict(batch=0), dict(height=0),
                dict(width=0), dict(width=3), dict(height=15),      # a canvas larger than the batch
                dict(src_bytes=95), dict(tables_len=tables_len - 1), dict(tables=None), dict(out=out + 1), dict(tables=tables + 2),
                dict(workspace_bytes=-1), dict(workspace=workspace + 8)):
        assert call(**bad) == _C.ERR_INVALID, bad
    assert call(dtype=7) == _C.ERR_UNSUPPORTED
    for field, value in (('canvas_width', 0), ('canvas_height', 0), ('canvas_width', 33), ('flags', 16), ('flags', 1 << 31),
                         ('brightness', float('nan')), ('saturation', float('inf')),
                         ('map', (ctypes.c_int32 * 6)(0, -65536, 15 * 65536, 1 << 30, 0, 0)),       # 2^30 * 3 leaves 32 bits
                         ('map', (ctypes.c_int32 * 6)(0, -65536, 15 * 65536, 65536, 0, 0x7fffffff))):
        before = getattr(augments[1], field)
        setattr(augments[1], field, value)
        assert call() == _C.ERR_INVALID, (field, value)
        setattr(augments[1], field, before)
    images[1].mirror = 1                                            # the flip travels in the map
    assert call() == _C.ERR_INVALID
    images[1].mirror = 0
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        _C.augment_images(torch.zeros(96, dtype=torch.uint8), images, augments, torch.zeros(80, dtype=torch.int32),
                          D.normalisation_table(), 32, 32)
