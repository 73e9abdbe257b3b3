"""Soft-NMS on the device (csrc/soft_nms.hpp, odtk_soft_nms) against the checker (tests/soft_nms_ref.py), bit for bit on scores,
boxes, classes and input positions: every count at which the kernel's ownership pattern changes (one wave, one pass of the
workgroup, the full eight candidates per thread), more detections asked for than candidates alive, crowds whose scores sink
under the floor, ties, padding anywhere, a NaN IoU; then the bindings, streams, box.detect and the three inference branches of
Model.forward.  Gaussian cases are admitted by the checker's exp margin (a condition on the inputs, no tolerance)."""
import os

import numpy as np
import pytest
import torch

import soft_nms_ref
from odtk import _C, box
from odtk.model import Model

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
METHODS = {'linear': _C.SOFT_NMS_LINEAR, 'gaussian': _C.SOFT_NMS_GAUSSIAN}


def _equal_scores():
    s, b, c = soft_nms_ref.random_case(31, 2, 300, 4, padding=0.0)
    s[:] = F(0.5)
    return s, b, c


def _padding_front_middle_end():
    s, b, c = soft_nms_ref.random_case(32, 2, 200, 3, padding=0.0)
    s[:, :50], s[:, 100:120], s[:, 180:] = 0, -1, 0
    return s, b, c


def _nan_iou():
    s, b, c = soft_nms_ref.random_case(33, 1, 70, 2, padding=0.1)
    b[0, 5], b[0, 66] = [5, 5, 4, 9], [5, 5, 4, 9]               # area 0 twice: their IoU is 0 / 0
    c[0, 5] = c[0, 66] = 1
    s[0, 5], s[0, 66] = 0.99, 0.98
    return s, b, c


def _empty_image_beside_a_full_one():
    s, b, c = soft_nms_ref.random_case(34, 2, 1100, 5, padding=0.0)
    s[0] = 0
    return s, b, c


# name -> (candidates, detections_per_im).  random_case(seed, batch, count, classes, extent, padding)
CASES = {
    'count1': (lambda: soft_nms_ref.random_case(1, 3, 1, 1, padding=0.0), 100),
    'count63': (lambda: soft_nms_ref.random_case(2, 3, 63, 8), 100),
    'count64_one_class': (lambda: soft_nms_ref.random_case(3, 1, 64, 1), 100),
    'count65_one_detection': (lambda: soft_nms_ref.random_case(4, 3, 65, 8), 1),
    'count1023': (lambda: soft_nms_ref.random_case(5, 1, 1023, 80, extent=256.0), 300),
    'count1024_one_class': (lambda: soft_nms_ref.random_case(6, 3, 1024, 1, extent=256.0), 100),
    'count1025_one_class_300': (lambda: soft_nms_ref.random_case(7, 1, 1025, 1, extent=256.0), 300),
    'count5000': (lambda: soft_nms_ref.random_case(8, 3, 5000, 80, extent=512.0), 100),
    'count7680': (lambda: soft_nms_ref.random_case(9, 1, 7680, 80, extent=512.0), 300),
    'count7680_one_class': (lambda: soft_nms_ref.random_case(10, 1, 7680, 1, extent=1024.0, padding=0.5), 100),
    'crowd1500_on_32px': (lambda: soft_nms_ref.random_case(11, 1, 1500, 1, extent=32.0, padding=0.0), 300),
    'equal_scores': (_equal_scores, 300),
    'padding_front_middle_end': (_padding_front_middle_end, 100),
    'nan_iou': (_nan_iou, 100),
    'empty_image_beside_a_full_one': (_empty_image_beside_a_full_one, 100),
}
OPTIONS = {'linear': (0.3, 0.5, 0.2), 'gaussian': (0.5, 0.3, 0.1)}             # nms, sigma, min_score


def _device(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _assert_bits(out, ref, what):
    for o, r, name in zip(out[:3], ref, ('scores', 'boxes', 'classes')):
        got = o.cpu().numpy()
        assert got.shape == r.shape and np.array_equal(got.view(np.uint32), r.view(np.uint32)), (what, name)
    if len(out) > 3:
        assert np.array_equal(out[3].cpu().numpy(), ref[3]), (what, 'positions')


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
@pytest.mark.parametrize('case', list(CASES))
def test_kernel_equals_checker(case, method):
    make, ndet = CASES[case]
    arrays = make()
    nms, sigma, floor = OPTIONS[method]
    ref = soft_nms_ref.soft_nms_ref(*arrays, nms, ndet, method, sigma, floor)
    assert ref[4] >= soft_nms_ref.ADMIT_ULPS, (case, ref[4])
    out = _C.soft_nms(*_device(arrays), nms, ndet, METHODS[method], sigma, floor, return_indices=True)
    _assert_bits(out, ref, case)
    assert (np.diff(ref[0], axis=1) <= 0).all()
    if case == 'crowd1500_on_32px':
        assert 0 < int((ref[0] > 0).sum()) < ndet                  # the crowd ran out: scores sank under the floor
    if case == 'nan_iou':
        assert 5 in ref[3][0] and 66 not in ref[3][0]


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_trained_candidates(method):
    arrays, ref = soft_nms_ref.trained_reference(GOLDEN, method)
    assert ref[4] >= soft_nms_ref.ADMIT_ULPS, ref[4]
    out = _C.soft_nms(*_device(arrays), 0.5, 100, METHODS[method], 0.5, 0.05, return_indices=True)
    _assert_bits(out, ref, 'trained')
    out = box.soft_nms(*_device(arrays), 0.5, 100, method, 0.5, 0.05)
    assert len(out) == 3
    _assert_bits(out, ref, 'trained, box.soft_nms')


def test_bindings_streams_and_repeats_agree():
    from odtk import _C_ext
    arrays = _device(soft_nms_ref.random_case(41, 3, 2100, 6, extent=128.0))
    for method in (_C.SOFT_NMS_LINEAR, _C.SOFT_NMS_GAUSSIAN):
        first = _C.soft_nms(*arrays, 0.4, 150, method, 0.4, 0.1, return_indices=True)
        again = _C.soft_nms(*arrays, 0.4, 150, method, 0.4, 0.1, return_indices=True)      # immediately behind it
        ext = _C_ext.soft_nms(*arrays, 0.4, 150, method, 0.4, 0.1, True)
        ext3 = _C_ext.soft_nms(*arrays, 0.4, 150, method, 0.4, 0.1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            there = _C.soft_nms(*arrays, 0.4, 150, method, 0.4, 0.1, return_indices=True)
        side.synchronize()
        torch.cuda.synchronize()
        assert len(ext) == 4 and len(ext3) == 3 and ext[3].dtype == torch.int32
        assert int((first[0] > 0).sum()) > 150
        for other in (again, ext, ext3, there):
            assert all(torch.equal(a, b) for a, b in zip(first, other))


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_detect_equals_decode_levels_then_checker(method):
    with np.load(os.path.join(GOLDEN, 'pipeline_clustered_160x256.npz')) as z:
        g = {k: z[k] for k in z.files}
    strides = [int(s) for s in g['strides']]
    cls = [torch.from_numpy(g['cls%d' % i]).cuda() for i in range(len(strides))]
    dl = [torch.from_numpy(g['box%d' % i]).cuda() for i in range(len(strides))]
    anchors = {s: torch.from_numpy(g['anchors%d' % i]) for i, s in enumerate(strides)}
    threshold, top_n, nms, ndet = float(g['threshold']), int(g['top_n']), float(g['nms']), int(g['detections'])
    options = {'method': method, 'sigma': 0.5, 'min_score': 0.06}
    soft_thresh = 0.3                                            # (at the fixture's 0.5 the linear rule keeps the same 100 here)
    out = box.detect(cls, dl, strides, anchors, threshold, top_n, soft_thresh, ndet, soft_nms=options)
    cand = box.decode_levels(cls, dl, strides, threshold, top_n, anchors)
    assert all(np.array_equal(t.cpu().numpy(), g[k]) for t, k in zip((cand[0], cand[2]), ('cat_scores', 'cat_classes')))
    ref = soft_nms_ref.soft_nms_ref(*[t.cpu().numpy() for t in cand], soft_thresh, ndet, method, 0.5, 0.06)
    assert ref[4] >= soft_nms_ref.ADMIT_ULPS, ref[4]
    _assert_bits(out, ref, 'detect')
    hard = box.detect(cls, dl, strides, anchors, threshold, top_n, nms, ndet)
    assert all(torch.equal(h, n) for h, n in zip(hard, _C.nms(*cand, nms, ndet)))            # the hard path is what it was
    assert np.array_equal(hard[0].cpu().numpy(), g['out_scores']) and np.array_equal(hard[2].cpu().numpy(), g['out_classes'])
    assert not torch.equal(hard[0], out[0])
    with pytest.raises(ValueError, match='rotated'):
        box.detect(cls, dl, strides, anchors, threshold, top_n, nms, ndet, rotated=True, soft_nms=options)


def test_model_branches_honour_the_option_and_the_off_switch():
    """ResNet18FPN at 128 x 128 under bf16 autocast.  The eager network and the BN-folded engine are the same function only up
    to the rounding of the folded weights (tests/test_gpu_fused_model.py), so each branch is compared, bit for bit, with the
    checker on the candidates decoded from ITS OWN head tensors; the hipGraph replays the engine, so those two are equal.
    With soft_nms = None every branch returns what it returned before the option was ever set -- the captured graph too."""
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True                          # (convolutions reproduce run to run: tests/test_gpu_graph.py)
    try:
        torch.manual_seed(0)
        model = Model('ResNet18FPN', classes=8)
        model.initialize(None)
        model = model.cuda().to(memory_format=torch.channels_last).eval()
        with torch.no_grad():
            model.cls_head[-1].weight.mul_(60.0)                        # detections exist
        x = torch.randn(2, 3, 128, 128, device='cuda').contiguous(memory_format=torch.channels_last)
        options = {'method': 'gaussian', 'sigma': 0.5, 'min_score': 0.05}

        def call(branch):
            model.fused_graph = branch != 'eager'
            try:
                with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                    return [t.clone() for t in model(x, graph=branch == 'graph')]
            finally:
                model.fused_graph = True

        def reference(cls_heads, box_heads, cls_bias=None, box_bias=None):
            strides = [x.shape[-1] // c.shape[-1] for c in cls_heads]
            pairs = [box._pair(c, b) for c, b in zip(cls_heads, box_heads)]
            cand = _C.decode_levels([p[0] for p in pairs], [p[1] for p in pairs], [model.anchors[s] for s in strides], strides,
                                    model.threshold, model.top_n, logits=True, cls_bias=cls_bias, box_bias=box_bias)
            ref = soft_nms_ref.soft_nms_ref(*[t.cpu().numpy() for t in cand], model.nms, model.detections, 'gaussian', 0.5, 0.05)
            assert ref[4] >= soft_nms_ref.ADMIT_ULPS, ref[4]
            return ref

        before = {b: call(b) for b in ('eager', 'engine', 'graph')}
        assert all(torch.equal(a, b) for a, b in zip(before['engine'], before['graph']))
        assert int((before['engine'][0] > 0).sum()) > 20
        model.soft_nms = options
        soft = {b: call(b) for b in ('eager', 'engine', 'graph')}
        assert all(torch.equal(a, b) for a, b in zip(soft['engine'], soft['graph']))          # not the graph captured above
        assert not torch.equal(soft['engine'][0], before['engine'][0]) and not torch.equal(soft['eager'][0], before['eager'][0])
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            _assert_bits(soft['eager'], reference(*model.heads(x)), 'eager + HIP')
            engine = model.inference_engine(torch.bfloat16)
            _assert_bits(soft['engine'], reference(*engine.heads_without_last_bias(x)), 'engine')
        model.soft_nms = None
        for b in ('eager', 'engine', 'graph'):
            assert all(torch.equal(a, c) for a, c in zip(before[b], call(b))), b
        n_graphs = len(engine._graphs)
        model.soft_nms = dict(options, method='linear')                 # another rule: another graph
        assert all(torch.equal(a, b) for a, b in zip(call('engine'), call('graph')))
        assert model.inference_engine(torch.bfloat16) is engine and len(engine._graphs) == n_graphs + 1
    finally:
        torch.backends.cudnn.deterministic = saved
