"""The boundary's threading promise (include/odtk_hip.h): calls only ENQUEUE on the caller's stream and may be
made concurrently from several host threads on distinct streams and workspaces.  Four host threads, each with its own HIP
stream and its own inputs, run `detect` (prefilter -> select_decode -> nms) and the fused loss pair (all-level forward through
the workspace form + backward) 200 times -- through the ctypes binding and through the compiled `_C_ext` module -- and every
result must equal, bit for bit, what the same call returned serially.  Process-wide state this exercises: the profiler's
event pool (enabled in half of the threads' iterations), hipFuncSetAttribute bookkeeping, the binding's workspace cache
(a lock since round 4), the loss launch-shape table (one snapshot per call since round 4)."""
import threading

import pytest
import torch

from odtk import _C, box, synthetic

pytestmark = pytest.mark.gpu
RATIOS, SCALES = [1.0, 2.0, 0.5], [4 * 2 ** (i / 3) for i in range(3)]
N_THREADS, ITERS = 4, 200


def _inputs(seed):
    cls, dl, strides = synthetic.pyramid(2, 9, 20, 192, 256, 'clustered', seed, unique=False)
    lg = [torch.logit(c.clamp(1e-6, 1 - 1e-6)).cuda().bfloat16().contiguous(memory_format=torch.channels_last) for c in cls]
    db = [d.cuda().bfloat16().contiguous(memory_format=torch.channels_last) for d in dl]
    anchors = {s: box.generate_anchors(s, RATIOS, SCALES) for s in strides}
    g = torch.Generator().manual_seed(seed)
    depths = [torch.randint(-1, 21, (2, 9, 1) + tuple(c.shape[-2:]), generator=g).float().cuda() for c in cls]
    targets = [torch.randn((2, 9, 4) + tuple(c.shape[-2:]), generator=g).cuda() * 0.3 for c in cls]
    return lg, db, strides, anchors, depths, targets


def _work(inp, ext):
    lg, db, strides, anchors, depths, targets = inp
    if ext:
        from odtk import _C_ext
        det = _C_ext.detect(lg, db, [anchors[s].reshape(-1).tolist() for s in strides], strides, 0.05, 1000, 0.5, 100, False, True)
    else:
        det = box.detect(lg, db, strides, anchors, 0.05, 1000, 0.5, 100, logits=True)
    sums = _C.retina_loss_levels_forward(lg, db, depths, targets, 0.25, 2.0, 0.11, reproducible=True)
    gc = torch.full((len(lg),), 0.5, device='cuda')
    dcls, dbox = _C.retina_loss_levels_backward(lg, db, depths, targets, 0.25, 2.0, 0.11, gc, gc)
    return list(det) + [sums] + list(dcls) + list(dbox)


def test_profiler_and_trace_are_one_per_library():
    """The library is linked from one object per subsystem; the profiler and the trace pointer must be ONE state that all of
    them see: launches of the decode, nms, loss and engine sources all arrive in the same profile_collect, and the trace
    buffer set once is stamped by select_decode and by nms."""
    batch, n_levels = 2, 5
    cls, dl, strides = synthetic.pyramid(batch, 9, 20, 128, 192, 'clustered', 4242)
    assert len(strides) == n_levels
    anchors = {s: box.generate_anchors(s, RATIOS, SCALES) for s in strides}
    cls, dl = [c.cuda() for c in cls], [d.cuda() for d in dl]
    lg = [torch.logit(c.clamp(1e-6, 1 - 1e-6)).bfloat16().contiguous(memory_format=torch.channels_last) for c in cls]
    db = [d.bfloat16().contiguous(memory_format=torch.channels_last) for d in dl]
    g = torch.Generator().manual_seed(4242)
    depths = [torch.randint(-1, 21, (batch, 9, 1) + tuple(c.shape[-2:]), generator=g).float().cuda() for c in cls]
    targets = [torch.randn((batch, 9, 4) + tuple(c.shape[-2:]), generator=g).cuda() * 0.3 for c in cls]
    y = torch.randn(batch, 64, 16, 24, device='cuda').bfloat16().contiguous(memory_format=torch.channels_last)
    bias = torch.randn(64, device='cuda')
    trace = torch.zeros(_C.TRACE_WORDS, dtype=torch.int64, device='cuda')
    try:
        _C.profile_collect()                                         # whatever earlier tests left pending
        _C.profile_enable()
        box.detect(cls, dl, strides, anchors, 0.05, 1000, 0.5, 100)
        _C.retina_loss_levels_forward(lg, db, depths, targets, 0.25, 2.0, 0.11, reproducible=True)
        _C.bias_act_(y, bias)
        _C.upsample2x(y)
        first = _C.profile_collect()
        for name in ('prefilter_scan_kernel', 'select_decode_kernel', 'nms_kernel', 'retina_loss_kernel', 'loss_reduce_kernel',
                     'bias_act_kernel', 'upsample_nearest2x_kernel'):
            assert first[name][1] >= 1, (name, first)
        assert all(n == 0 for _, n in _C.profile_collect().values())
        _C.debug_set_trace(trace)
        box.detect(cls, dl, strides, anchors, 0.05, 1000, 0.5, 100)
        torch.cuda.synchronize()
        words = trace.cpu()
        assert bool((words[:8 * batch * n_levels] != 0).any()), 'select_decode: 8 words per (level, image) segment from word 0'
        nms = words[8 * 64:]                                         # nms: behind the select_decode slots, 8 words per workgroup,
        for b in range(batch):                                       # the first `batch` groups of 8 left free
            assert int(nms[(batch + b) * 8]) != 0, 'nms workgroup %d left no stamp' % b
    finally:
        _C.debug_set_trace(None)
        _C.profile_enable(False)
        _C.profile_collect()


@pytest.mark.parametrize('ext', [False, True], ids=['ctypes', 'compiled'])
def test_concurrent_calls_on_distinct_streams_equal_serial_results(ext):
    inputs = [_inputs(1000 + t) for t in range(N_THREADS)]
    serial = [_work(inp, ext) for inp in inputs]
    torch.cuda.synchronize()
    assert all(int((s[0] > 0).sum()) > 20 for s in serial)
    streams = [torch.cuda.Stream() for _ in range(N_THREADS)]
    errors = []
    start = threading.Barrier(N_THREADS)

    def run(t):
        try:
            torch.cuda.set_device(0)
            start.wait()
            with torch.cuda.stream(streams[t]):
                for it in range(ITERS):
                    if t % 2 == 0 and it % 50 == 0:
                        _C.profile_enable(it % 100 == 0)             # the profiler's pool is process-wide state too
                    out = _work(inputs[t], ext)
                    if it % 20 == 19 or it == ITERS - 1:
                        streams[t].synchronize()
                        for k, (a, b) in enumerate(zip(out, serial[t])):
                            if not torch.equal(a, b):
                                errors.append((t, it, k))
                                return
        except Exception as e:                                       # noqa: BLE001 -- reported below, with the thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(N_THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    _C.profile_enable(False)
    _C.profile_collect()
    torch.cuda.synchronize()
    assert not errors, errors
