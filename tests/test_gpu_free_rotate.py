"""Free-angle rotation on the GPU (csrc/augment.hpp: augment_rotate_kernel, odtk_augment_images_ex): the chain's output must equal
the CPU pipeline of tests/test_free_rotate.py (SourceBatch.apply_cpu, itself equal to Pillow) bit for bit over every element of the
padded batch, for the three output dtypes; an image without a rotation in such a batch must come out as odtk_augment_images writes
it; and the loader must yield on the GPU what it yields on the CPU with the same seed.  Every case runs once."""
import random

import numpy as np
import pytest
import torch

from odtk import _C
from odtk import data as D
from test_device_augment import noise
from test_free_rotate import ANN, ANN_ROT, HERE, OPTIONS

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
B, C, H, S = D.AUGMENT_BRIGHTNESS, D.AUGMENT_CONTRAST, D.AUGMENT_HUE, D.AUGMENT_SATURATION
ALL = (B | C | H | S, 1.3, 0.8, 1.6, 200)                          # flags, brightness, contrast, saturation, hue
PLAIN = (0, 1.0, 1.0, 1.0, 0)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def geometry(size, turn=0, expand=False, flip=False, colour=PLAIN, angle=None):
    """The geometry tuple of SourceBatch.pack for a resized image of `size` = (width, height): with `angle` the map is the turn
    alone and the rotation of the turned canvas and the flip follow; without, the flip is in the map."""
    cw, ch, coefficients = D.quarter_turn_map(size[0], size[1], turn, expand, flip and angle is None)
    g = tuple(size) + (0, cw, ch, coefficients) + tuple(colour)
    return g if angle is None else g + (D.free_rotation_matrix(cw, ch, angle), int(flip))


def _run(buffer, dtype):
    batch = D.SourceBatch(buffer)
    uploaded = buffer.cuda()
    images = (_C.Image * batch.batch).from_buffer_copy(batch.images.tobytes())
    augments = (_C.Augment * batch.batch).from_buffer_copy(batch.augments.tobytes())
    rotations = None
    if batch.rotations is not None:
        rotations = (_C.Rotation * batch.batch).from_buffer_copy(batch.rotations.tobytes())
    return _C.augment_images(uploaded, images, augments, batch.tables(uploaded), D.normalisation_table(dtype).cuda(), batch.height, batch.width,
                             rotations=rotations)


def _check(sources, geometries, stride, dtypes=DTYPES):
    """Pack, run on the device for every dtype, compare bits with the CPU pipeline; -> (the batch, the last output)."""
    buffer = D.SourceBatch.pack([torch.from_numpy(s) for s in sources], geometries, stride)
    batch = D.SourceBatch(buffer)
    assert batch.rotations is not None
    for dtype in dtypes:
        out = _run(buffer, dtype)
        assert out.shape == (len(sources), 3, batch.height, batch.width) and out.dtype == dtype
        assert out.is_contiguous(memory_format=torch.channels_last)
        got = _bits(out.permute(0, 2, 3, 1)).cpu()
        want = _bits(batch.apply_cpu(D.normalisation_table(dtype), dtype).permute(0, 2, 3, 1))
        differ = (got != want).flatten(1).sum(1).tolist()
        print(dtype, 'differing elements per image:', differ)
        assert not any(differ), (dtype, differ)                     # bits: the pad's sign bit included
        for k, aug in enumerate(batch.augments):
            assert not got[k, int(aug['canvas_height']):].any() and not got[k, :, int(aug['canvas_width']):].any()
    return batch, out


@pytest.mark.parametrize('expand', [False, True], ids=['same-canvas', 'expand'])
def test_every_rotation_case_in_one_batch(expand):
    """Sources of 37 x 53, 64 x 64, 5 x 3, 1 x 7 and 120 x 75 (height x width), resized by up to 2: 45 degrees, an enabled angle of
    0, 180, 90 on a non-square canvas, and -7.3 degrees over a quarter turn of 90 (on its own canvas, or expanded); flips on and
    off; every colour operation, the contrast's mean over the rotated canvas with its black corners.  A sixth image is not rotated."""
    sources = [noise(53, 37, 'noise', 1), noise(64, 64, 'noise', 2), noise(3, 5, 'noise', 3), noise(7, 1, 'noise', 4), noise(75, 120, 'noise', 5),
               noise(64, 64, 'binary', 6)]
    geometries = [geometry((80, 60), 0, expand, True, ALL, 45.0),
                  geometry((64, 64), 0, expand, False, (C, 1.0, 1.7, 1.0, 0), 0.0),
                  geometry((6, 10), 0, expand, True, ALL, 180.0),
                  geometry((14, 2), 0, expand, False, ALL, 90.0),
                  geometry((90, 130), 90, expand, True, ALL, -7.3),
                  geometry((50, 40), 270, expand, True, ALL)]
    batch, out = _check(sources, geometries, 32)
    assert batch.rotations['enabled'].tolist() == [1, 1, 1, 1, 1, 0] and batch.rotations['flip'].tolist() == [1, 0, 1, 0, 1, 0]
    assert (int(batch.augments[4]['canvas_width']), int(batch.augments[4]['canvas_height'])) == ((130, 90) if expand else (90, 130))
    # the image without a rotation: what odtk_augment_images writes for it alone
    alone = D.SourceBatch.pack([torch.from_numpy(sources[5])], geometries[5:], 32)
    assert D.SourceBatch(alone).rotations is None
    for dtype in DTYPES:
        want = _run(alone, dtype)
        got = _run(batch.buffer, dtype)[5:, :, :want.shape[2], :want.shape[3]]
        assert torch.equal(_bits(got.permute(0, 2, 3, 1)), _bits(want.permute(0, 2, 3, 1)))


@pytest.mark.parametrize('width', [16, 13], ids=['rows-of-whole-vectors', 'rows-not-whole-vectors'])
def test_both_store_paths_of_the_colour_pass(width):
    """16 pixels: a row is 192 / 96 bytes, whole 16-byte vectors; 13 pixels: 156 / 78 bytes, it is not."""
    sources = [noise(9, 11, 'noise', 7), noise(width, 5, 'noise', 8)]
    _check(sources, [geometry((width, 9), 0, False, True, ALL, 13.37), geometry((width - 3, 7), 180, False, False, ALL, -45.0)], 1)


def test_sixty_five_images_cross_the_chain_boundary():
    sources = [noise(8, 8, 'noise', 100 + k) for k in range(65)]
    geometries = [geometry((8, 8), (k % 4) * 90, False, k % 2 == 1, (C | S, 1.0, 0.5 + k / 65, 1.3, 0), -180.0 + 5.5 * k) for k in range(65)]
    _check(sources, geometries, 8, [torch.bfloat16])


@pytest.mark.parametrize('cls,ann,extra', [(D.DataIterator, ANN, {}), (D.RotatedDataIterator, ANN_ROT, {}),
                                           (D.RotatedDataIterator, ANN_ROT, {'absolute_angle': True})], ids=['axis', 'rotated', 'absolute'])
def test_seeded_iterator_on_the_gpu_equals_the_cpu_device(cls, ann, extra):
    args = (HERE, [96, 160], 220, 5, 32, 1, ann)
    batches = []
    for device in ('cuda', 'cpu'):
        it = cls(*args, training=True, num_workers=0, device=device, device_augment=True, augment_free_rotate=(-30, 30), **OPTIONS, **extra)
        assert 'free rotation: -30 to 30 degrees' in repr(it)
        random.seed(31)
        torch.manual_seed(31)
        batches.append([tuple(t.clone() for t in b) for _ in range(2) for b in it])
        torch.cuda.synchronize()
    assert len(batches[0]) == len(batches[1]) == 2
    for (a, ta), (b, tb) in zip(*batches):
        assert a.is_cuda and not b.is_cuda and a.shape == b.shape and a.stride() == b.stride()
        assert torch.equal(_bits(a.permute(0, 2, 3, 1)).cpu(), _bits(b.permute(0, 2, 3, 1)))
        assert torch.equal(ta.cpu(), tb)
