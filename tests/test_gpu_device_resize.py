"""The device-side input pipeline on the GPU (csrc/preprocess.hpp, odtk_preprocess_images): the kernel's output must equal the CPU
pipeline of tests/test_device_resize.py -- itself equal to Pillow -- bit for bit, over every element of the padded batch, for the
three output dtypes, mirrored and not; the loader with device_resize=True must yield what the host path yields and what the
reference's data.py produced (tests/golden/data/expected.npz); and the launch only enqueues on the caller's stream."""
import os
import random
import threading

import numpy as np
import pytest
import torch

from odtk import _C
from odtk import data as D
from odtk.model import Model
from test_device_resize import ANN, ANN_ROT, HERE, resize_cases, source_image

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
_resized = {}


def _case(k, kind):
    """(source pixels, target size, the CPU pipeline's resized pixels) of case k, computed once."""
    if (k, kind) not in _resized:
        src, dst = resize_cases()[k]
        pixels = source_image(*src, kind, 100 + k)
        _resized[(k, kind)] = (pixels, dst, D.resize_bilinear(pixels, dst))
    return _resized[(k, kind)]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _expected(resized, mirrors, height, width, dtype):
    """Mirror, pad with +0.0, normalise by table: [B, H, W, 3]."""
    table = D.normalisation_table(dtype).reshape(-1)
    out = torch.zeros(len(resized), height, width, 3, dtype=dtype)
    for k, (pixels, mirror) in enumerate(zip(resized, mirrors)):
        pixels = pixels[:, ::-1].copy() if mirror else pixels
        out[k, :pixels.shape[0], :pixels.shape[1]] = table[torch.from_numpy(pixels).long() + torch.tensor([0, 256, 512])]
    return out


def _run(buffer, dtype):
    batch = D.SourceBatch(buffer)
    uploaded = buffer.cuda()
    images = (_C.Image * batch.batch).from_buffer_copy(batch.images.tobytes())
    return _C.preprocess_images(uploaded, images, batch.tables(uploaded), D.normalisation_table(dtype).cuda(), batch.height, batch.width)


def _check_batch(cases, kind, mirrors, stride, dtype):
    sources, sizes, resized = zip(*(_case(k, kind) for k in cases))
    buffer = D.SourceBatch.pack([torch.from_numpy(s) for s in sources], [size + (m,) for size, m in zip(sizes, mirrors)], stride)
    out = _run(buffer, dtype)
    batch = D.SourceBatch(buffer)
    assert out.shape == (len(cases), 3, batch.height, batch.width) and out.dtype == dtype
    assert out.is_contiguous(memory_format=torch.channels_last)
    got = _bits(out.permute(0, 2, 3, 1)).cpu()
    want = _bits(_expected(resized, mirrors, batch.height, batch.width, dtype))
    assert torch.equal(got, want), (cases, kind, mirrors, int((got != want).sum()))     # bits: the pad's sign bit included
    for k, (w, h) in enumerate(sizes):                                                  # ... and said once more for the pad alone
        assert not got[k, h:].any() and not got[k, :, w:].any()


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('kind', ['noise', 'binary'])
def test_kernel_equals_the_cpu_pipeline_on_every_case(kind, dtype):
    """The whole case list of the CPU test, in batches of mixed sizes (up to 7 images, the padded size of the largest), every
    image once mirrored and once not."""
    n = len(resize_cases())
    rng = random.Random(7)
    order = list(range(n))
    rng.shuffle(order)
    for flip in (0, 1):
        for at in range(0, n, 7):
            cases = order[at:at + 7]
            _check_batch(cases, kind, [(k + flip) % 2 for k in cases], 32, dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16', 'fp16'])
def test_passes_both_one_none_and_the_chunked_vertical_walk_in_one_batch(dtype):
    """640x480 -> 1066x800 (both passes), width only, height only, unchanged (copied), and 600x700 -> 40x50: a tile's 16 rows draw
    on ~250 source rows, walked in chunks of the 40 that LDS holds; 4000x3000 -> 1066x800 is the realistic chunked case."""
    named = {case: k for k, case in enumerate(resize_cases())}
    cases = [named[c] for c in (((640, 480), (1066, 800)), ((640, 480), (700, 480)), ((640, 480), (640, 300)), ((64, 48), (64, 48)),
                                ((600, 700), (40, 50)), ((4000, 3000), (1066, 800)))]
    for mirrors in ([0, 1, 0, 1, 0, 1], [1, 0, 1, 0, 1, 0]):
        _check_batch(cases, 'noise', mirrors, 128, dtype)
    _check_batch(cases[1:5], 'binary', [1, 1, 0, 0], 1, dtype)      # width 700: 16-bit rows are not whole 16-byte vectors
    _check_batch([named[((2, 3), (9, 11))], named[((1, 50), (13, 20))]], 'noise', [1, 0], 1, dtype)      # width 13: nor are fp32 rows


def test_more_images_than_one_launch_carries():
    """Descriptors travel in the kernel arguments, 64 per launch: a batch of 70 is two launches writing one output."""
    cases = [k for k, (src, dst) in enumerate(resize_cases()) if max(src + dst) <= 300][:35] * 2
    _check_batch(cases, 'noise', [k % 2 for k in range(70)], 32, torch.bfloat16)


def _iterate(it, seed=None):
    if seed is not None:
        random.seed(seed)
    out = [tuple(t.clone() for t in batch) for batch in it]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('workers', [0, 2])
def test_inference_iterator_equals_the_host_path_and_the_reference(dtype, workers):
    args = (HERE, 128, 200, 4, 32, 1, ANN)
    host = _iterate(D.DataIterator(*args, training=False, num_workers=workers, device='cuda', dtype=dtype))
    it = D.DataIterator(*args, training=False, num_workers=workers, device='cuda', dtype=dtype, device_resize=True)
    assert 'the device' in repr(it)
    dev = _iterate(it)
    assert len(host) == len(dev) == 2
    for (a, a_ids, a_ratios), (b, b_ids, b_ratios) in zip(host, dev):
        assert b.is_cuda and b.dtype == dtype and a.shape == b.shape and a.stride() == b.stride()
        assert torch.equal(_bits(a.permute(0, 2, 3, 1)), _bits(b.permute(0, 2, 3, 1)))
        assert torch.equal(a_ids, b_ids) and torch.equal(a_ratios, b_ratios) and a_ratios.shape == b_ratios.shape
    if dtype == torch.float32:
        with np.load(os.path.join(HERE, 'expected.npz')) as expected:
            assert torch.equal(dev[0][0].cpu().contiguous(), torch.from_numpy(expected['infer_batch']))
            assert torch.equal(dev[0][1].cpu(), torch.from_numpy(expected['infer_batch_ids']))
            assert torch.equal(dev[0][2].cpu(), torch.from_numpy(expected['infer_batch_ratios']))


@pytest.mark.parametrize('cls,ann,extra', [(D.DataIterator, ANN, {}), (D.RotatedDataIterator, ANN_ROT, {'absolute_angle': True})],
                         ids=['axis', 'rotated'])
def test_seeded_training_iterator_equals_the_host_path(cls, ann, extra):
    args = (HERE, [96, 160], 220, 5, 32, 1, ann)
    for seed in (11, 12, 13):
        host = _iterate(cls(*args, training=True, num_workers=0, device='cuda', **extra), seed)
        dev = _iterate(cls(*args, training=True, num_workers=0, device='cuda', device_resize=True, **extra), seed)
        assert len(host) == len(dev) == 1
        for (a, ta), (b, tb) in zip(host, dev):
            assert a.shape == b.shape and a.stride() == b.stride() and torch.equal(_bits(a.permute(0, 2, 3, 1)), _bits(b.permute(0, 2, 3, 1)))
            assert torch.equal(ta, tb)


def test_detections_on_a_device_resized_batch_equal_those_on_the_host_batch():
    """Identical input bits -> identical detections: compared exactly, in fp32 and under the fp16 autocast `infer` uses.  MIOpen's
    find mode may pick convolution kernels that do not repeat their own result on the same tensor (tests/test_gpu_graph.py,
    profiles/r03_determinism_probe.txt), so, as there, the comparison runs with torch.backends.cudnn.deterministic = True."""
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(3)
        model = Model('ResNet18FPN', classes=3)
        model.initialize(None)
        with torch.no_grad():
            model.cls_head[-1].bias.fill_(0.0)                      # detections exist (random weights score 0.01 < 0.05 otherwise)
        model = model.to(memory_format=torch.channels_last).cuda().eval()
        args = (HERE, 128, 200, 4, 32, 1, ANN)
        host = _iterate(D.DataIterator(*args, training=False, num_workers=0, device='cuda'))
        dev = _iterate(D.DataIterator(*args, training=False, num_workers=0, device='cuda', device_resize=True))
        for amp in (False, True):
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16, enabled=amp):
                for (a, _, _), (b, _, _) in zip(host, dev):
                    assert torch.equal(a, b)
                    want = [t.clone() for t in model(a)]
                    got = model(b)
                    assert int((want[0] > 0).sum()) > 0
                    for w, g in zip(want, got):
                        assert torch.equal(w, g), amp
    finally:
        torch.backends.cudnn.deterministic = saved


def test_side_stream_and_two_threads_give_the_same_bits():
    """The launch runs on the caller's stream and shares no state between calls: the same batch on the default stream, on a side
    stream, and from two host threads on their own streams at once (the model is tests/test_gpu_threads.py)."""
    named = {case: k for k, case in enumerate(resize_cases())}
    picks = [named[((640, 480), (1066, 800))], named[((600, 700), (40, 50))], named[((64, 48), (64, 48))]]
    sources, sizes, _ = zip(*(_case(k, 'noise') for k in picks))
    buffers = [D.SourceBatch.pack([torch.from_numpy(s) for s in sources], [size + (m,) for size in sizes], 128) for m in (0, 1)]
    serial = [_run(b, torch.bfloat16) for b in buffers]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = _run(buffers[0], torch.bfloat16)
    side.synchronize()
    assert torch.equal(_bits(on_side), _bits(serial[0]))
    streams = [torch.cuda.Stream() for _ in buffers]
    errors, start = [], threading.Barrier(len(buffers))

    def run(t):
        try:
            torch.cuda.set_device(0)
            start.wait()
            with torch.cuda.stream(streams[t]):
                for it in range(50):
                    out = _run(buffers[t], torch.bfloat16)
                    if it % 10 == 9:
                        streams[t].synchronize()
                        if not torch.equal(_bits(out), _bits(serial[t])):
                            errors.append((t, it))
                            return
        except Exception as e:                                       # noqa: BLE001 -- reported below, with the thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(len(buffers))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
