"""Matrix NMS on the device (csrc/matrix_nms.hpp, odtk_matrix_nms) against the checker (tests/matrix_nms_ref.py), bit for bit on
scores, boxes, classes and input positions, for both rules: the counts around a wave, participant numbers around the edges of
the pair tile (64 columns x 256 rows) and across several tiles, one class (a dense matrix) and eighty, the `pre_top` cut, lists
beyond what the LDS-resident kernels take, the radix selection (more than 4096 positive scores), crowds that sink under the
floor, ties, padding anywhere, NaN IoUs, duplicates (cmax = 1); then the bindings, streams, box.detect with and without box
voting and the inference branches of Model.forward.  Gaussian cases are admitted by the checker's exp margin (a condition on
the inputs, no tolerance)."""
import os

import numpy as np
import pytest
import torch

import box_vote_ref
import matrix_nms_ref
import tile_ref
from matrix_nms_ref import random_case
from odtk import _C, box
from odtk.model import Model

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
METHODS = {'linear': _C.MATRIX_NMS_LINEAR, 'gaussian': _C.MATRIX_NMS_GAUSSIAN}


def _equal_scores(seed, count):
    def make():
        s, b, c = random_case(seed, 2, count, 4, extent=192.0, padding=0.0)
        s[:] = F(0.5)
        return s, b, c
    return make


def _padding_front_middle_end():
    s, b, c = random_case(32, 2, 200, 3, padding=0.0)
    s[:, :50], s[:, 100:120], s[:, 180:] = 0, -1, 0
    return s, b, c


def _nan_iou():
    s, b, c = random_case(33, 1, 70, 2, padding=0.1)
    b[0, 5], b[0, 66] = [5, 5, 4, 9], [5, 5, 4, 9]               # area 0 twice: their IoU is 0 / 0, cmax and d are skipped
    c[0, 5] = c[0, 66] = 1
    s[0, 5], s[0, 66] = 0.99, 0.98
    return s, b, c


def _duplicate_pair():
    s, b, c = random_case(35, 1, 90, 2, padding=0.1)
    b[0, 7] = b[0, 40] = [10, 12, 40, 50]                        # iou 1: cmax of the second is 1, its row divides by 1 - 1
    b[0, 60] = [10, 12, 40, 50]                                  # ... (1 - 1) / (1 - 1) for the third copy, (1 - iou) / 0 elsewhere
    c[0, 7] = c[0, 40] = c[0, 60] = 1
    s[0, 7], s[0, 40], s[0, 60] = 0.99, 0.98, 0.97
    return s, b, c


def _crowd():
    s, b, c = random_case(18, 2, 1500, 1, extent=3.0, padding=0.0)   # 3 x 3 pixel boxes at nine places: a copy's factor is 0 (or NaN)
    s[1] *= F(0.09)                                              # ... and an image whose scores all lie under the floor
    return s, b, c


def _empty_image_beside_a_full_one():
    s, b, c = random_case(34, 2, 1100, 5, padding=0.0)
    s[0] = 0
    return s, b, c


# name -> (candidates, detections_per_im, pre_top).  random_case(seed, batch, count, classes, extent, padding)
CASES = {
    'count1': (lambda: random_case(1, 3, 1, 1, padding=0.0), 100, 2000),
    'count63': (lambda: random_case(2, 3, 63, 8, padding=0.0), 100, 2000),
    'count64_one_class': (lambda: random_case(3, 1, 64, 1, padding=0.0), 100, 2000),
    'count65_one_detection': (lambda: random_case(4, 3, 65, 8, padding=0.0), 1, 2000),
    'n255_one_class': (lambda: random_case(5, 2, 255, 1, extent=128.0, padding=0.0), 300, 2000),
    'n256': (lambda: random_case(6, 2, 256, 3, extent=128.0, padding=0.0), 100, 2000),
    'n257_one_class': (lambda: random_case(7, 1, 257, 1, extent=128.0, padding=0.0), 300, 2000),
    'n1000_several_tiles_80_classes': (lambda: random_case(8, 3, 1000, 80, extent=64.0, padding=0.0), 300, 2000),
    'n1000_several_tiles_one_class': (lambda: random_case(9, 1, 1000, 1, extent=256.0, padding=0.0), 100, 2000),
    'pre_top_cuts_500_to_100': (lambda: random_case(10, 2, 500, 2, padding=0.1), 100, 100),
    'pre_top_cuts_inside_a_tile': (lambda: random_case(11, 2, 700, 2, extent=128.0, padding=0.0), 500, 300),
    'pre_top_4096_above_count': (lambda: random_case(12, 2, 100, 2, padding=0.2), 100, 4096),
    'pre_top_4096_one_class_on_48px': (lambda: random_case(13, 1, 4096, 1, extent=48.0, padding=0.0), 300, 4096),
    'count5000_80_classes': (lambda: random_case(14, 3, 5000, 80, extent=128.0), 100, 2000),
    'count9000_pre_top_1000': (lambda: random_case(15, 2, 9000, 80, extent=128.0), 100, 1000),
    'count7000_all_positive_pre_top_4096': (lambda: random_case(16, 1, 7000, 40, extent=128.0, padding=0.0), 200, 4096),
    'detections_above_alive': (lambda: random_case(17, 2, 40, 2, padding=0.5), 300, 2000),
    'crowd1500_on_nine_places': (_crowd, 300, 2000),
    'equal_scores': (_equal_scores(31, 300), 300, 2000),
    'equal_scores_6000_pre_top_500': (_equal_scores(36, 6000), 100, 500),
    'padding_front_middle_end': (_padding_front_middle_end, 100, 2000),
    'nan_iou': (_nan_iou, 100, 2000),
    'duplicate_pair': (_duplicate_pair, 100, 2000),
    'empty_image_beside_a_full_one': (_empty_image_beside_a_full_one, 100, 2000),
}
OPTIONS = {'linear': (0.5, 0.2), 'gaussian': (0.3, 0.1)}                       # sigma, min_score


def _device(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _host(tensors):
    return [t.cpu().numpy() for t in tensors]


def _assert_bits(out, ref, what):
    for o, r, name in zip(out[:3], ref, ('scores', 'boxes', 'classes')):
        got = o.cpu().numpy()
        assert got.shape == r.shape and np.array_equal(got.view(np.uint32), r.view(np.uint32)), (what, name)
    if len(out) > 3:
        assert np.array_equal(out[3].cpu().numpy(), ref[3]), (what, 'positions')


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
@pytest.mark.parametrize('case', list(CASES))
def test_kernel_equals_checker(case, method):
    make, ndet, pre_top = CASES[case]
    arrays = make()
    sigma, floor = OPTIONS[method]
    ref = matrix_nms_ref.matrix_nms_ref(*arrays, ndet, method, sigma, floor, pre_top)
    assert ref[4] >= matrix_nms_ref.ADMIT_ULPS, (case, ref[4])
    out = _C.matrix_nms(*_device(arrays), ndet, pre_top, METHODS[method], sigma, floor, return_indices=True)
    _assert_bits(out, ref, case)
    assert (np.diff(ref[0], axis=1) <= 0).all()
    positive = (arrays[0] > 0).sum(1)
    if case.startswith('pre_top_cuts'):
        uncut = matrix_nms_ref.matrix_nms_ref(*arrays, ndet, method, sigma, floor, 4096)
        assert (positive > pre_top).all() and not np.array_equal(uncut[3], ref[3])       # the cut changes the result
    if case in ('count9000_pre_top_1000', 'count7000_all_positive_pre_top_4096', 'equal_scores_6000_pre_top_500'):
        assert (positive > 4096).all()                                                   # the radix selection ran
    if case == 'detections_above_alive':
        assert 0 < int((ref[0] > 0).sum(1).max()) < ndet                                 # fewer alive than slots
    if case == 'crowd1500_on_nine_places':                                               # the crowd sank under the floor
        assert 0 < int((ref[0][0] > 0).sum()) <= 9 and not (ref[0][1] > 0).any() and (ref[3][1] == -1).all()
    if case == 'nan_iou':
        assert 5 in ref[3][0] and 66 in ref[3][0]                                        # a NaN IoU decays nothing
    if case == 'duplicate_pair':
        assert 7 in ref[3][0] and 40 not in ref[3][0] and 60 not in ref[3][0]


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_trained_candidates(method):
    arrays, ref = matrix_nms_ref.trained_matrix_reference(GOLDEN, method)
    assert ref[4] >= matrix_nms_ref.ADMIT_ULPS, ref[4]
    out = _C.matrix_nms(*_device(arrays), 100, 2000, METHODS[method], 0.5, 0.05, return_indices=True)
    _assert_bits(out, ref, 'trained')
    out = box.matrix_nms(*_device(arrays), 100, method, 0.5, 0.05, 2000)
    assert len(out) == 3
    _assert_bits(out, ref, 'trained, box.matrix_nms')


def test_bindings_streams_and_repeats_agree():
    from odtk import _C_ext
    arrays = _device(random_case(41, 3, 2100, 6, extent=128.0))
    for method in (_C.MATRIX_NMS_LINEAR, _C.MATRIX_NMS_GAUSSIAN):
        first = _C.matrix_nms(*arrays, 150, 1500, method, 0.4, 0.1, return_indices=True)
        again = _C.matrix_nms(*arrays, 150, 1500, method, 0.4, 0.1, return_indices=True)      # immediately behind it
        ext = _C_ext.matrix_nms(*arrays, 150, 1500, method, 0.4, 0.1, True)
        ext3 = _C_ext.matrix_nms(*arrays, 150, 1500, method, 0.4, 0.1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            there = _C.matrix_nms(*arrays, 150, 1500, method, 0.4, 0.1, return_indices=True)
        side.synchronize()
        torch.cuda.synchronize()
        assert len(ext) == 4 and len(ext3) == 3 and ext[3].dtype == torch.int32
        assert int((first[0] > 0).sum()) > 150
        for other in (again, ext, ext3, there):
            assert all(torch.equal(a, b) for a, b in zip(first, other))


def _pipeline():
    with np.load(os.path.join(GOLDEN, 'pipeline_clustered_160x256.npz')) as z:
        g = {k: z[k] for k in z.files}
    strides = [int(s) for s in g['strides']]
    cls = [torch.from_numpy(g['cls%d' % i]).cuda() for i in range(len(strides))]
    dl = [torch.from_numpy(g['box%d' % i]).cuda() for i in range(len(strides))]
    anchors = {s: torch.from_numpy(g['anchors%d' % i]) for i, s in enumerate(strides)}
    return g, cls, dl, strides, anchors


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_detect_equals_decode_levels_then_checker(method):
    g, cls, dl, strides, anchors = _pipeline()
    threshold, top_n, nms, ndet = float(g['threshold']), int(g['top_n']), float(g['nms']), int(g['detections'])
    options = {'method': method, 'sigma': 0.5, 'min_score': 0.06, 'pre_top': 1500}
    out = box.detect(cls, dl, strides, anchors, threshold, top_n, nms, ndet, matrix_nms=options)
    cand = box.decode_levels(cls, dl, strides, threshold, top_n, anchors)
    ref = matrix_nms_ref.matrix_nms_ref(*_host(cand), ndet, method, 0.5, 0.06, 1500)
    assert ref[4] >= matrix_nms_ref.ADMIT_ULPS, ref[4]
    _assert_bits(out, ref, 'detect')
    hard = box.detect(cls, dl, strides, anchors, threshold, top_n, nms, ndet)
    assert np.array_equal(hard[0].cpu().numpy(), g['out_scores']) and np.array_equal(hard[2].cpu().numpy(), g['out_classes'])
    assert not torch.equal(hard[0], out[0])
    # min_score defaults to the score threshold, pre_top to 2000, the method to gaussian
    default = box.detect(cls, dl, strides, anchors, threshold, top_n, nms, ndet, matrix_nms={})
    ref = matrix_nms_ref.matrix_nms_ref(*_host(cand), ndet, 'gaussian', 0.5, threshold, 2000)
    assert ref[4] >= matrix_nms_ref.ADMIT_ULPS, ref[4]
    _assert_bits(default, ref, 'detect, defaults')
    # box voting behind it, through the position output
    voted = box.detect(cls, dl, strides, anchors, threshold, top_n, nms, ndet, matrix_nms=options, vote=0.65)
    ref = matrix_nms_ref.matrix_nms_ref(*_host(cand), ndet, method, 0.5, 0.06, 1500)
    assert torch.equal(voted[0], out[0]) and torch.equal(voted[2], out[2])
    votes = box_vote_ref.vote_ref(*_host(cand), ref[3], 0.65)
    box_vote_ref.assert_votes(voted[1].cpu().numpy(), votes, ref[3], 'detect + vote')
    assert not torch.equal(voted[1], out[1])
    with pytest.raises(ValueError, match='rotated'):
        box.detect(cls, dl, strides, anchors, threshold, top_n, nms, ndet, rotated=True, matrix_nms=options)
    with pytest.raises(ValueError, match='exclude'):
        box.detect(cls, dl, strides, anchors, threshold, top_n, nms, ndet, matrix_nms=options, soft_nms={'method': 'linear'})


def test_model_branches_honour_the_option_and_the_off_switch():
    """ResNet18FPN on [2, 3, 128, 160] under bf16 autocast.  The eager network and the BN-folded engine are the same function only
    up to the rounding of the folded weights, so each branch is compared, bit for bit, with the checker on the candidates decoded
    from ITS OWN head tensors; the hipGraph replays the engine, so those two are equal.  With matrix_nms = None every branch
    returns what it returned before the option was ever set -- the captured graph too.  Then the option with `tta = 'flip'`
    (against the checker on the merged list) and with `tile` on a merged list of 10 000 candidates, which Soft-NMS refuses."""
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(0)
        model = Model('ResNet18FPN', classes=8)
        model.initialize(None)
        model = model.cuda().to(memory_format=torch.channels_last).eval()
        with torch.no_grad():
            model.cls_head[-1].weight.mul_(60.0)                        # detections exist
        x = torch.randn(2, 3, 128, 160, device='cuda').contiguous(memory_format=torch.channels_last)
        options = {'method': 'gaussian', 'sigma': 0.5, 'min_score': 0.05, 'pre_top': 1200}

        def call(branch):
            model.fused_graph = branch != 'eager'
            try:
                with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                    return [t.clone() for t in model(x, graph=branch == 'graph')]
            finally:
                model.fused_graph = True

        def own_candidates(branch, inp):
            """decode_levels on the branch's own head tensors of `inp`, decoded at once (the engine's next pass may overwrite them)."""
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                if branch == 'eager':
                    (cls_heads, box_heads), cls_bias, box_bias = model.heads(inp), None, None
                else:
                    cls_heads, box_heads, cls_bias, box_bias = model.inference_engine(torch.bfloat16).heads_without_last_bias(inp)
                strides = [inp.shape[-1] // c.shape[-1] for c in cls_heads]
                pairs = [box._pair(c, b) for c, b in zip(cls_heads, box_heads)]
                cand = _C.decode_levels([p[0] for p in pairs], [p[1] for p in pairs], [model.anchors[s] for s in strides], strides,
                                        model.threshold, model.top_n, logits=True, cls_bias=cls_bias, box_bias=box_bias)
            torch.cuda.synchronize()
            return cand

        def check(out, cand, what):
            ref = matrix_nms_ref.matrix_nms_ref(*cand, model.detections, 'gaussian', 0.5, 0.05, 1200)
            assert ref[4] >= matrix_nms_ref.ADMIT_ULPS, ref[4]
            _assert_bits(out, ref, what)

        before = {b: call(b) for b in ('eager', 'engine', 'graph')}
        assert all(torch.equal(a, b) for a, b in zip(before['engine'], before['graph']))
        assert int((before['engine'][0] > 0).sum()) > 20
        engine = model.inference_engine(torch.bfloat16)
        n_graphs = len(engine._graphs)

        model.matrix_nms = options
        matrix = {b: call(b) for b in ('eager', 'engine', 'graph')}
        assert all(torch.equal(a, b) for a, b in zip(matrix['engine'], matrix['graph']))      # not the graph captured above
        assert len(engine._graphs) == n_graphs + 1
        for b in ('eager', 'engine'):
            assert not torch.equal(matrix[b][0], before[b][0])          # not what the hard rule gives
            check(matrix[b], _host(own_candidates(b, x)), b)

        model.tta = 'flip'
        for b in ('eager', 'engine'):
            cand = box_vote_ref.concat_ref([_host(own_candidates(b, x)), _host(own_candidates(b, box.flip_batch(x)))], [0, x.shape[-1]])
            assert cand[0].shape[1] > _C.MAX_NMS_COUNT                  # 10 000 candidates: more than Soft-NMS takes
            check(call(b), cand, ('tta', b))
        model.tta = None

        model.tile = {'size': (128, 128), 'overlap': (32, 32), 'batch': 8}
        for b in ('eager', 'engine'):
            tiled = call(b)

            def decode(tiles, b=b):
                return own_candidates(b, tiles)
            merged = tile_ref.expected_merged(x, ((128, 128), (32, 32), 0.0, 8), decode)[0]
            assert merged[0].shape[1] > _C.MAX_NMS_COUNT
            check(tiled, merged, ('tile', b))
        model.matrix_nms, model.soft_nms = None, {'method': 'gaussian', 'sigma': 0.5, 'min_score': 0.05}
        with pytest.raises(ValueError, match='top_n'):                  # the same list is more than Soft-NMS takes
            call('engine')
        model.soft_nms, model.tile = None, None

        for b in ('eager', 'engine', 'graph'):
            assert all(torch.equal(a, c) for a, c in zip(before[b], call(b))), b
        assert model.inference_engine(torch.bfloat16) is engine and len(engine._graphs) == n_graphs + 1
        model.matrix_nms, model.soft_nms = options, {'method': 'linear'}
        with pytest.raises(ValueError, match='soft_nms'):
            call('engine')
    finally:
        torch.backends.cudnn.deterministic = saved
