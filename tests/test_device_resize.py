"""The device-side input pipeline, host half (odtk/data.py: resample_weights, SourceBatch, device_resize=True): Pillow's 8-bit
bilinear resampling restated in integers must equal Pillow bit for bit, and the loader mode that ships source-size pixels must
yield exactly what the host path yields -- the arrays the reference's data.py produced (tests/golden/data/expected.npz).  Every
comparison is equality over every pixel.  The GPU half is tests/test_gpu_device_resize.py."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from odtk import _C
from odtk import data as D
from odtk import main as cli
from odtk.model import Model

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data')
ANN = os.path.join(HERE, 'annotations.json')
ANN_ROT = os.path.join(HERE, 'annotations_rotated.json')


def resize_cases():
    """((source width, height), (target width, height)): named cases first, then 40 seeded random pairs."""
    cases = [((640, 480), (1066, 800)),                  # COCO-shaped up-scaling
             ((4000, 3000), (1066, 800)),                # down-scaling by 3.75 on both axes
             ((600, 700), (40, 50)),                     # down-scaling by 15 / 14
             ((640, 480), (700, 480)), ((640, 480), (640, 300)),       # width only, height only
             ((64, 48), (64, 48)),                       # unchanged
             ((1, 1), (7, 5)), ((2, 3), (9, 11)), ((1, 50), (13, 20)), ((50, 1), (20, 13)),
             ((300, 200), (1, 1)), ((5, 4), (1, 9))]
    rng = random.Random(20240607)
    cases += [((rng.randint(1, 300), rng.randint(1, 300)), (rng.randint(1, 300), rng.randint(1, 300))) for _ in range(40)]
    return cases


def source_image(width, height, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == 'noise':
        return rng.integers(0, 256, (height, width, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (height, width, 3), dtype=np.uint8) * 255).astype(np.uint8)      # clamp and rounding cases


@pytest.fixture(scope='module')
def expected():
    return np.load(os.path.join(HERE, 'expected.npz'))


@pytest.mark.parametrize('kind', ['noise', 'binary'])
def test_two_pass_resize_equals_pillow(kind):
    for k, (src, dst) in enumerate(resize_cases()):
        pixels = source_image(*src, kind, 100 + k)
        want = np.array(Image.fromarray(pixels).resize(dst, Image.BILINEAR))
        got = D.resize_bilinear(pixels, dst)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), (src, dst, int((got != want).sum()))


def test_weight_tables_have_pillows_shape():
    bounds, weights = D.resample_weights(480, 800)                  # up-scaling: the filter is not stretched, 3 taps
    assert bounds.dtype == np.int32 and weights.dtype == np.int32 and bounds.shape == (800, 2) and weights.shape == (800, 3)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 480).all() and (bounds[:, 1] >= 1).all()
    assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()      # the kernel's footprint relies on it
    assert (np.abs(weights.sum(1) - (1 << 22)) <= 2).all() and (weights >= 0).all()
    bounds, weights = D.resample_weights(3000, 800)                 # down-scaling by 3.75: support 3.75, 2 * 4 + 1 taps
    assert weights.shape == (800, 9) and bounds[:, 1].max() <= 9
    for o, (first, n) in enumerate(bounds):
        assert not weights[o, n:].any()
    same = D.resample_weights(50, 50)                               # Pillow skips such a pass; its weights would be the identity
    assert (same[0][:, 0] == np.arange(50)).all() and (same[1][:, 0] == 1 << 22).all() and not same[1][:, 1:].any()
    with pytest.raises(ValueError):
        D.resample_weights(0, 5)


def test_source_batch_round_trip_and_mirror():
    """pack -> descriptors, tables, pixels; apply_cpu = resize, then mirror, then pad with +0.0, then the table."""
    a, b = source_image(37, 21, 'noise', 1), source_image(16, 16, 'noise', 2)
    buffer = D.SourceBatch.pack([torch.from_numpy(a), torch.from_numpy(b)], [(50, 30, 1), (16, 16, 0)], 32)
    batch = D.SourceBatch(buffer)
    assert (batch.batch, batch.height, batch.width) == (2, 32, 64)
    assert ctypes.sizeof(_C.Image) == D.IMAGE_DTYPE.itemsize == 48
    assert np.array_equal(batch.source(0), a) and np.array_equal(batch.source(1), b)
    first, second = batch.images
    assert (first['x_table'], first['x_taps'], first['y_taps'], first['mirror']) == (0, 3, 3, 1)
    assert (second['x_table'], second['y_table']) == (-1, -1)       # both passes skipped: the pixels are copied
    tables = batch.tables().numpy()
    bounds, weights = D.resample_weights(37, 50)
    assert np.array_equal(tables[:100], bounds.reshape(-1)) and np.array_equal(tables[100:250], weights.reshape(-1))
    out = batch.apply_cpu(D.normalisation_table())
    assert out.shape == (2, 3, 32, 64) and out.is_contiguous(memory_format=torch.channels_last)
    want = np.array(Image.fromarray(a).resize((50, 30), Image.BILINEAR).transpose(Image.FLIP_LEFT_RIGHT))
    packed = torch.zeros(2, 32, 64, 4, dtype=torch.uint8)
    packed[0, :30, :50, :3], packed[0, :30, :50, 3] = torch.from_numpy(want), 255
    packed[1, :16, :16, :3], packed[1, :16, :16, 3] = torch.from_numpy(b), 255
    assert torch.equal(out, D.normalise_batch(packed))
    assert not torch.signbit(out).logical_and(out == 0).any()
    thin = source_image(1, 9, 'noise', 3)                           # one pixel wide and mirrored: the flip is a copy with a negative stride
    out = D.SourceBatch(D.SourceBatch.pack([torch.from_numpy(thin)], [(1, 9, 1)], 1)).apply_cpu(D.normalisation_table())
    assert torch.equal(out, _normalised(thin, 1)[None])


def _normalised(pixels, stride, table=None):
    h, w = pixels.shape[:2]
    up = lambda d: d + (stride - d % stride) % stride
    packed = torch.zeros(1, up(h), up(w), 4, dtype=torch.uint8)
    packed[0, :h, :w, :3], packed[0, :h, :w, 3] = torch.from_numpy(pixels), 255
    return D.normalise_batch(packed, table)[0]


def test_inference_items_and_batch_equal_the_reference(expected):
    ds = D.CocoDataset(HERE, resize=128, max_size=200, stride=32, annotations=ANN, training=False, device_resize=True)
    items = [ds[i] for i in range(5)]
    assert [it[1] for it in items[:4]] == [(172, 128, 0), (128, 170, 0), (128, 128, 0), (170, 128, 0)]   # up- and down-scaling
    for i, (pixels, (ow, oh, mirror), image_id, ratio) in enumerate(items):
        assert pixels.dtype == torch.uint8 and pixels.shape[2] == 3
        with Image.open(os.path.join(HERE, 'im%d.png' % i)) as im:
            assert pixels.shape[:2] == im.size[::-1]                # source size: nothing was resized on the way
        got = _normalised(D.resize_bilinear(pixels.numpy(), (ow, oh)), 32)
        assert torch.equal(got.contiguous(), torch.from_numpy(expected['infer_pixels_%d' % i])), 'image %d' % i
        assert image_id == int(expected['infer_id_%d' % i]) and ratio == float(expected['infer_ratio_%d' % i])
    buffer, ids, ratios = ds.collate_fn(items[:4])
    assert buffer.dtype == torch.uint8 and buffer.dim() == 1
    batch = D.SourceBatch(buffer).apply_cpu(D.normalisation_table())
    assert batch.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(batch.contiguous(), torch.from_numpy(expected['infer_batch']))
    assert not torch.signbit(batch).logical_and(batch == 0).any()
    assert ids.dtype == torch.int32 and torch.equal(ids, torch.from_numpy(expected['infer_batch_ids']))
    assert torch.equal(ratios, torch.from_numpy(expected['infer_batch_ratios']))
    # fewer bytes cross the process boundary than the resized RGBA batch of the host path
    host = D.CocoDataset(HERE, resize=800, max_size=1333, stride=128, annotations=ANN, training=False)
    dev = D.CocoDataset(HERE, resize=800, max_size=1333, stride=128, annotations=ANN, training=False, device_resize=True)
    assert dev.collate_fn([dev[0], dev[1]])[0].numel() * 4 < host.collate_fn([host[0], host[1]])[0].numel()


@pytest.mark.parametrize('workers', [0, 2])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16], ids=['fp32', 'fp16', 'bf16'])
def test_iterator_equals_the_host_path_batch_for_batch(expected, dtype, workers):
    args = (HERE, 128, 200, 4, 32, 1, ANN)
    host = D.DataIterator(*args, training=False, num_workers=workers, device='cpu', dtype=dtype)
    dev = D.DataIterator(*args, training=False, num_workers=workers, device='cpu', dtype=dtype, device_resize=True)
    assert len(host) == len(dev) == 2 and 'resize on' in repr(dev) and 'resize on' not in repr(host)
    seen = 0
    for (a, a_ids, a_ratios), (b, b_ids, b_ratios) in zip(host, dev):
        assert b.dtype == dtype and a.shape == b.shape and a.stride() == b.stride()
        assert torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))
        assert torch.equal(a_ids, b_ids) and torch.equal(a_ratios, b_ratios) and a_ratios.shape == b_ratios.shape
        if seen == 0 and dtype == torch.float32:
            assert torch.equal(b.contiguous(), torch.from_numpy(expected['infer_batch']))
        seen += 1
    assert seen == 2


@pytest.mark.parametrize('cls,ann,extra', [(D.CocoDataset, ANN, {}), (D.RotatedCocoDataset, ANN_ROT, {}),
                                           (D.RotatedCocoDataset, ANN_ROT, {'absolute_angle': True})], ids=['axis', 'rotated', 'absolute'])
def test_seeded_training_equals_the_host_path(cls, ann, extra):
    """resize=[96, 160] with flips: same images, same targets, and `random` is left in the same state after every item."""
    kwargs = dict(resize=[96, 160], max_size=220, stride=32, annotations=ann, training=True, **extra)
    host, dev = cls(HERE, **kwargs), cls(HERE, device_resize=True, **kwargs)
    table = D.normalisation_table()
    host_items, dev_items, mirrored = [], [], 0
    state = random.Random(4321).getstate()
    for i in range(15):
        random.setstate(state)
        pixels, target = host[i % 5]
        after_host = random.getstate()
        random.setstate(state)
        source, (ow, oh, mirror), dev_target = dev[i % 5]
        assert random.getstate() == after_host, 'item %d' % i
        state = after_host
        assert torch.equal(target, dev_target), 'item %d' % i
        assert pixels.shape[:2] == (oh, ow)
        resized = D.resize_bilinear(source.numpy(), (ow, oh))
        assert np.array_equal(resized[:, ::-1] if mirror else resized, pixels[..., :3].numpy()), 'item %d' % i
        mirrored += mirror
        host_items.append((pixels, target))
        dev_items.append((source, (ow, oh, mirror), dev_target))
    assert 0 < mirrored < 15
    for at in (0, 5, 10):
        packed, targets = host.collate_fn(host_items[at:at + 5])
        buffer, dev_targets = dev.collate_fn(dev_items[at:at + 5])
        assert torch.equal(targets, dev_targets)
        assert torch.equal(D.normalise_batch(packed, table), D.SourceBatch(buffer).apply_cpu(table))


def test_seeded_training_iterators_agree():
    args = (HERE, [96, 160], 220, 5, 32, 1, ANN)
    batches = []
    for device_resize in (False, True):
        it = D.DataIterator(*args, training=True, num_workers=0, device='cpu', device_resize=device_resize)
        random.seed(99)
        torch.manual_seed(99)                                       # the sampler's shuffle (none here) and nothing else
        batches.append([b for b in it])
    assert len(batches[0]) == len(batches[1]) == 1
    for (a, ta), (b, tb) in zip(*batches):
        assert a.shape == b.shape and a.stride() == b.stride() and torch.equal(a, b) and torch.equal(ta, tb)


@pytest.mark.parametrize('option', ['rotate_augment', 'augment_brightness', 'augment_contrast', 'augment_hue', 'augment_saturation'])
def test_excluded_augmentations_raise_and_name_the_option(option):
    value = True if option == 'rotate_augment' else 0.01
    with pytest.raises(ValueError, match=option):
        D.CocoDataset(HERE, 128, 200, 32, annotations=ANN, training=True, device_resize=True, **{option: value})
    with pytest.raises(ValueError, match=option):
        D.RotatedDataIterator(HERE, 128, 200, 2, 32, 1, ANN_ROT, training=True, device='cpu', num_workers=0, device_resize=True,
                              **{option: value})
    D.CocoDataset(HERE, 128, 200, 32, annotations=ANN, training=True, **{option: value})          # the host path takes them as before


def test_cli_switch_is_absent_unless_given_and_reaches_the_iterator(monkeypatch):
    assert 'device_resize' not in vars(cli.parse(['infer', 'm.pth']))
    assert 'device_resize' not in vars(cli.parse(['train', 'm.pth', '--annotations', 'a.json']))
    assert cli.parse(['infer', 'm.pth', '--device-resize']).device_resize is True
    assert cli.parse(['train', 'm.pth', '--annotations', 'a.json', '--device-resize']).device_resize is True
    with pytest.raises(SystemExit):
        cli.parse(['export', 'm.pth', 'm.plan', '--device-resize'])
    seen = []

    def spy(self, *args, **kwargs):
        seen.append(kwargs.get('device_resize'))
        raise KeyboardInterrupt                                     # far enough

    monkeypatch.setattr(D.DataIterator, '__init__', spy)
    monkeypatch.setattr(cli, 'load_model', lambda args, verbose=False: (Model('ResNet18FPN', classes=3), {}))
    for argv, want in ((['infer', 'm.pth', '--images', HERE, '--device-resize'], True), (['infer', 'm.pth', '--images', HERE], False),
                       (['train', 'm.pth', '--annotations', ANN, '--images', HERE, '--device-resize'], True),
                       (['train', 'm.pth', '--annotations', ANN, '--images', HERE], False)):
        with pytest.raises(KeyboardInterrupt):
            cli.worker(0, cli.parse(argv), 1)
        assert seen[-1] == want, argv
    with pytest.raises(RuntimeError, match='DALI'):                 # --with-dali stays refused, with its message
        cli.worker(0, cli.parse(['infer', 'm.pth', '--images', HERE, '--with-dali']), 1)


def test_cpu_inference_writes_the_same_detections(tmp_path, monkeypatch):
    model = Model('ResNet18FPN', classes=3)
    model.initialize(None)
    with torch.no_grad():
        model.cls_head[-1].bias.fill_(0.0)
    path = str(tmp_path / 'm.pth')
    model.save({'path': path})
    calls = []
    apply_cpu = D.SourceBatch.apply_cpu
    monkeypatch.setattr(D.SourceBatch, 'apply_cpu', lambda self, *a, **k: calls.append(self.batch) or apply_cpu(self, *a, **k))
    base = ['infer', path, '--images', HERE, '--annotations', ANN, '--batch', '2', '--resize', '128', '--max-size', '160',
            '--workers', '0', '--full-precision', '--output']
    cli.main(base + [str(tmp_path / 'host.json')])
    cli.main(base + [str(tmp_path / 'device.json'), '--device-resize'])
    if not torch.cuda.is_available():                               # (with a GPU the same switch runs the HIP kernel instead)
        assert calls == [2, 2, 1]
    host, device = json.load(open(tmp_path / 'host.json')), json.load(open(tmp_path / 'device.json'))
    assert len(host['annotations']) > 0 and host == device


def test_entry_point_validates_without_a_gpu():
    lib = _C.library()
    assert lib.odtk_abi_struct_size(5) == ctypes.sizeof(_C.Image) == 48
    images = (_C.Image * 2)()
    for im in images:
        im.src_offset, im.src_width, im.src_height, im.src_pitch = 0, 8, 4, 24
        im.out_width, im.out_height, im.x_table, im.y_table, im.x_taps, im.y_taps = 16, 4, 0, -1, 3, 0
    tables_len = 16 * 5
    src, tables, norm, out = 1 << 20, 2 << 20, 3 << 20, 4 << 20    # never dereferenced on these paths

    def call(batch=2, images=images, src=src, src_bytes=96, tables=tables, tables_len=tables_len, norm=norm, out=out, height=32, width=32,
             dtype=_C.BF16):
        return lib.odtk_preprocess_images(batch, images, src, src_bytes, tables, tables_len, norm, out, height, width, dtype, None)

    for bad in (dict(images=None), dict(src=None), dict(norm=None), dict(out=None), dict(batch=0), dict(height=0), dict(width=0),
                dict(width=15), dict(height=3),                     # an image larger than the batch
                dict(src_bytes=95),                                 # the last row would end outside the buffer
                dict(tables_len=tables_len - 1), dict(tables=None), dict(out=out + 1), dict(tables=tables + 2)):
        assert call(**bad) == _C.ERR_INVALID, bad
    assert call(dtype=7) == _C.ERR_UNSUPPORTED
    for field, value in (('src_width', 0), ('src_height', 0), ('out_width', 0), ('out_height', 0), ('src_pitch', 23), ('mirror', 2),
                         ('x_taps', 0), ('x_table', -1),            # a skipped pass needs equal sizes
                         ('x_table', -2), ('y_table', 0),           # a vertical table for 4 -> 4 rows with 0 taps
                         ('src_offset', 1)):
        before = getattr(images[1], field)
        setattr(images[1], field, value)
        assert call() == _C.ERR_INVALID, field
        setattr(images[1], field, before)
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        _C.preprocess_images(torch.zeros(96, dtype=torch.uint8), images, torch.zeros(80, dtype=torch.int32), D.normalisation_table(), 32, 32)
