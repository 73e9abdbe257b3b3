"""Device-side training augmentations on the GPU (csrc/augment.hpp, odtk_augment_images): the chain's output must equal the CPU
pipeline of tests/test_device_augment.py (SourceBatch.apply_cpu, itself equal to Pillow) bit for bit, over every element of the
padded batch, for the three output dtypes; the hue path is checked against Pillow directly on all 2^24 colours; the loader with
device_augment=True must yield what the host path yields with the same seed; and the launches only enqueue on the caller's stream."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

from odtk import _C
from odtk import data as D
from test_device_augment import ANN, ANN_ROT, HERE, OPTIONS, all_colours, boundary_images, noise

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
B, C, H, S = D.AUGMENT_BRIGHTNESS, D.AUGMENT_CONTRAST, D.AUGMENT_HUE, D.AUGMENT_SATURATION
ALL = (B | C | H | S, 1.3, 0.8, 1.6, 200)                          # flags, brightness, contrast, saturation, hue


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def geometry(size, angle=0, expand=False, flip=False, colour=(0, 1.0, 1.0, 1.0, 0)):
    """The long geometry tuple of SourceBatch.pack for a resized image of `size` = (width, height)."""
    return tuple(size) + (0,) + D.quarter_turn_map(size[0], size[1], angle, expand, flip) + tuple(colour)


def _run(buffer, dtype):
    batch = D.SourceBatch(buffer)
    uploaded = buffer.cuda()
    images = (_C.Image * batch.batch).from_buffer_copy(batch.images.tobytes())
    augments = (_C.Augment * batch.batch).from_buffer_copy(batch.augments.tobytes())
    return _C.augment_images(uploaded, images, augments, batch.tables(uploaded), D.normalisation_table(dtype).cuda(), batch.height, batch.width)


def _check(sources, geometries, stride, dtypes=DTYPES):
    """Pack, run on the device for every dtype, compare bits with the CPU pipeline; -> the batch."""
    buffer = D.SourceBatch.pack([torch.from_numpy(s) for s in sources], geometries, stride)
    batch = D.SourceBatch(buffer)
    for dtype in dtypes:
        out = _run(buffer, dtype)
        assert out.shape == (len(sources), 3, batch.height, batch.width) and out.dtype == dtype
        assert out.is_contiguous(memory_format=torch.channels_last)
        got = _bits(out.permute(0, 2, 3, 1)).cpu()
        want = _bits(batch.apply_cpu(D.normalisation_table(dtype), dtype).permute(0, 2, 3, 1))
        differ = (got != want).flatten(1).sum(1).tolist()
        assert not any(differ), (dtype, differ)                     # bits: the pad's sign bit included
        for k, aug in enumerate(batch.augments):                    # ... and said once more for the pad alone
            assert not got[k, int(aug['canvas_height']):].any() and not got[k, :, int(aug['canvas_width']):].any()
    return batch


def test_every_turn_and_flip_with_and_without_expand():
    """65 x 17 (one past a tile each way), 1 x 9, 9 x 1 and a resized 37 x 21 -> 50 x 30; without expand the 90 / 270 degree turns
    of a non-square image cut the corners: black pixels, normalised like any byte 0."""
    shapes = [((65, 17), (65, 17)), ((1, 9), (1, 9)), ((9, 1), (9, 1)), ((37, 21), (50, 30))]
    for expand in (False, True):
        sources, geometries = [], []
        for k, (src, dst) in enumerate(shapes):
            for angle in (0, 90, 180, 270):
                for flip in (False, True):
                    sources.append(noise(*src, 'noise', 40 + k) | 1)            # no byte 0: black is the turn's alone
                    geometries.append(geometry(dst, angle, expand, flip, ALL if angle == 90 else (0, 1.0, 1.0, 1.0, 0)))
        batch = _check(sources, geometries, 32)
        assert (batch.height, batch.width) == ((96, 96) if expand else (32, 96))
    cw, ch, coefficients = D.quarter_turn_map(50, 30, 90)
    assert (cw, ch) == (50, 30) and (D.index_map(np.ones((30, 50, 3), dtype=np.uint8), cw, ch, coefficients) == 0).mean() > 0.25


@pytest.mark.parametrize('kind', ['noise', 'binary'])
def test_each_operation_alone_and_all_together_next_to_plain_images(kind):
    one = np.float32(1)
    colours = [(B, 0.6, 1.0, 1.0, 0), (B, 1.4, 1.0, 1.0, 0), (B, 0.0, 1.0, 1.0, 0), (B, float(np.nextafter(one, np.float32(2))), 1.0, 1.0, 0),
               (C, 1.0, 0.5, 1.0, 0), (C, 1.0, 1.8, 1.0, 0), (C, 1.0, 0.0, 1.0, 0), (H, 1.0, 1.0, 1.0, 0), (H, 1.0, 1.0, 1.0, 37),
               (H, 1.0, 1.0, 1.0, 255), (S, 1.0, 1.0, 0.3, 0), (S, 1.0, 1.0, 2.2, 0), (S, 1.0, 1.0, float(np.nextafter(one, np.float32(0))), 0),
               ALL, (B | C | H | S, 0.7, 40.0, 0.0, 128)]
    sizes = [(65, 17), (40, 33), (16, 16)]
    sources = [noise(*sizes[k % 3], kind, 60 + k) for k in range(len(colours) + 2)]
    geometries = [geometry(sizes[k % 3], 0, False, k % 2 == 1, colour) for k, colour in enumerate(colours)]
    geometries += [sizes[len(colours) % 3] + (0,), sizes[(len(colours) + 1) % 3] + (1,)]       # plain: (out_width, out_height, mirror)
    buffer = D.SourceBatch.pack([torch.from_numpy(s) for s in sources], geometries, 32)
    _check(sources, geometries, 32)
    # no flag and the identity (or mirror) map: exactly what odtk_preprocess_images writes
    plain = D.SourceBatch(D.SourceBatch.pack([torch.from_numpy(s) for s in sources[-2:]], geometries[-2:], 32))
    images = (_C.Image * 2).from_buffer_copy(plain.images.tobytes())
    uploaded = plain.buffer.cuda()
    for dtype in DTYPES:
        want = _C.preprocess_images(uploaded, images, plain.tables(uploaded), D.normalisation_table(dtype).cuda(), plain.height, plain.width)
        got = _run(buffer, dtype)[-2:, :, :plain.height, :plain.width]
        assert torch.equal(_bits(got.permute(0, 2, 3, 1)), _bits(want.permute(0, 2, 3, 1)))


def test_rows_that_are_not_whole_vectors_and_a_chunked_down_scale_under_a_turn():
    thin, wide = noise(1, 50, 'noise', 5), noise(2, 3, 'binary', 6)
    _check([thin, wide], [geometry((13, 20), 180, False, True, ALL), geometry((9, 11), 0, False, False, ALL)], 1)     # width 13
    _check([thin, wide], [geometry((13, 20), 90, True, False, ALL), geometry((9, 11), 270, True, True, ALL)], 1)     # width 20, height 13
    big = noise(600, 700, 'noise', 7)                               # 600 x 700 -> 40 x 50: the vertical walk in chunks, then the gather
    _check([big, big, big], [geometry((40, 50), 90, True, False, ALL), geometry((40, 50), 90, False, True, ALL), geometry((40, 50), 270, True)], 32)


def test_all_colours_through_the_hue_path_equal_pillow():
    colours = all_colours()
    shift_factor = 37 / 255 + 1e-9                                  # `_adjust_hue` adds int(factor * 255) % 256 = 37
    assert D.hue_shift_byte(shift_factor) == 37
    want = np.array(D._adjust_hue(Image.fromarray(colours), shift_factor))
    buffer = D.SourceBatch.pack([torch.from_numpy(colours)], [geometry((4096, 4096), colour=(H, 1.0, 1.0, 1.0, 37))], 32)
    got = _run(buffer, torch.float32)[0].permute(1, 2, 0)
    table = D.normalisation_table().cuda().reshape(-1)
    index = torch.from_numpy(want).cuda().to(torch.int32) + torch.tensor([0, 256, 512], dtype=torch.int32, device='cuda')
    assert torch.equal(_bits(got), _bits(table[index]))


def test_contrast_mean_at_the_half_integer_boundary_and_across_launches():
    for pixels, grey in boundary_images():
        size = pixels.shape[1::-1]
        batch = _check([pixels, pixels], [geometry(size, colour=(C, 1.0, 0.0, 1.0, 0)), geometry(size, 180, colour=(C, 1.0, 1.7, 1.0, 0))], 2,
                       [torch.float32])
        assert D.contrast_mean(batch.source(0)) == grey
    # 70 images: two launches, one sum each, none mixed
    sources = [np.clip(noise(20 + k % 3, 12, 'noise', 200 + k).astype(np.int32) + 2 * k - 70, 0, 255).astype(np.uint8) for k in range(70)]
    assert len({D.contrast_mean(s) for s in sources}) > 30
    _check(sources, [geometry(s.shape[1::-1], colour=(C, 1.0, 0.0 if k % 2 else 0.5, 1.0, 0)) for k, s in enumerate(sources)], 32, [torch.bfloat16])


def _iterate(it, seed):
    random.seed(seed)
    out = [tuple(t.clone() for t in batch) for batch in it]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('workers', [0, 2])
@pytest.mark.parametrize('cls,ann,extra', [(D.DataIterator, ANN, {}), (D.RotatedDataIterator, ANN_ROT, {}),
                                           (D.RotatedDataIterator, ANN_ROT, {'absolute_angle': True})], ids=['axis', 'rotated', 'absolute'])
def test_seeded_training_iterator_equals_the_host_path(cls, ann, extra, workers):
    """Workers draw from their own `random` (seeded by the loader from torch's generator): the same torch seed gives both paths
    the same draws."""
    args = (HERE, [96, 160], 220, 5, 32, 1, ann)
    for seed in (21, 22)[:2 - workers // 2]:                        # (starting workers costs more than the batch)
        batches = []
        for device_augment in (False, True):
            it = cls(*args, training=True, num_workers=workers, device='cuda', device_augment=device_augment, **OPTIONS, **extra)
            assert ('augmentations on: the device' in repr(it)) == device_augment
            torch.manual_seed(seed)
            batches.append(_iterate(it, seed))
            del it
        assert len(batches[0]) == len(batches[1]) == 1
        for (a, ta), (b, tb) in zip(*batches):
            assert b.is_cuda and a.shape == b.shape and a.stride() == b.stride()
            assert torch.equal(_bits(a.permute(0, 2, 3, 1)), _bits(b.permute(0, 2, 3, 1)))
            assert torch.equal(ta, tb)


def test_side_stream_and_repeated_runs_give_the_same_bits():
    """The chain runs on the caller's stream (its workspace is per stream) and shares no state between calls: the same batch
    twice on the default stream and once on a side stream, the same bits each time."""
    sources = [noise(640, 480, 'noise', 1), noise(600, 700, 'noise', 2), noise(64, 48, 'binary', 3)]
    geometries = [geometry((1066, 800), 90, True, True, ALL), geometry((40, 50), 270, False, False, ALL), geometry((64, 48), 180, False, True, ALL)]
    buffer = D.SourceBatch.pack([torch.from_numpy(s) for s in sources], geometries, 128)
    first = _run(buffer, torch.bfloat16)
    second = _run(buffer, torch.bfloat16)
    torch.cuda.synchronize()
    assert torch.equal(_bits(first), _bits(second))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = _run(buffer, torch.bfloat16)
    side.synchronize()
    assert torch.equal(_bits(on_side), _bits(first))
    want = _bits(D.SourceBatch(buffer).apply_cpu(D.normalisation_table(torch.bfloat16), torch.bfloat16).permute(0, 2, 3, 1))
    assert torch.equal(_bits(first.permute(0, 2, 3, 1)).cpu(), want)

