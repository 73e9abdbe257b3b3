"""Box voting and the flip merge on the device (csrc/box_vote.hpp: odtk_box_vote, odtk_concat_candidates) against the checker
(tests/box_vote_ref.py): the exact weighted mean, bit for bit where the inputs admit it and within one float32 ulp elsewhere -- on
the smallest shapes at which the kernel can go wrong (one candidate, the wave boundary, fewer detections than a workgroup holds,
thousands of voters per detection), behind the hard NMS and both Soft-NMS rules on a trained detector's candidates, then the
bindings, streams, box.detect and the three inference branches of Model.forward."""
import os

import numpy as np
import pytest
import torch

import box_vote_ref
import soft_nms_ref
from odtk import _C, box
from odtk.model import Model

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
METHODS = {'linear': _C.SOFT_NMS_LINEAR, 'gaussian': _C.SOFT_NMS_GAUSSIAN}


def _device(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _host(tensors):
    return [t.cpu().numpy() for t in tensors]


def _same_bits(got, ref, what=''):
    got, ref = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(ref, dtype=F)
    assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), what


@pytest.mark.parametrize('case', list(box_vote_ref.CASES))
def test_kernel_equals_checker(case):
    make, nms, ndet, vote = box_vote_ref.CASES[case]
    arrays = make()
    dev = _device(arrays)
    hard = _C.nms(*dev, nms, ndet, return_indices=True)
    kept = hard[3].cpu().numpy()
    got = _C.box_vote(*dev, hard[3], vote)
    assert got.shape == (arrays[0].shape[0], ndet, 4) and got.dtype == torch.float32
    ref = box_vote_ref.cached_ref(('cpu', case), *arrays, kept, vote)       # (shared with tests/test_box_vote.py: the same kept list)
    bad, compared = box_vote_ref.assert_votes(got.cpu().numpy(), ref, kept, case)
    print('%s: %d of %d coordinates not admitted, up to %d voters' % (case, bad, compared, int(ref[2].max(initial=0))))
    assert not got.cpu().numpy()[kept < 0].any()
    if case == '7680_one_class':
        assert int(ref[2].max()) > 1000
    if case == 'nan_iou':
        slot = int(np.flatnonzero(kept[0] == 5)[0])
        assert 66 not in kept[0] and ref[2][0, slot] == 1
        _same_bits(got.cpu().numpy()[0, slot], arrays[1][0, 5])
    if case == 'vote_thresh_1':
        _same_bits(got.cpu().numpy(), hard[1].cpu().numpy())
    if case == 'empty_image_beside_a_full_one':
        assert (kept[0] < 0).all() and (kept[1] >= 0).any()


def test_unused_and_out_of_range_positions_give_zeros():
    arrays = box_vote_ref.clustered_case(50, 2, 40, 2, 2, padding=0.0)
    kept = np.array([[3, -1, 40, 7, -1, -1], [-1, 0, 39, 1 << 20, -5, 2]], np.int32)
    ref = box_vote_ref.vote_ref(*arrays, kept, 0.65)
    got = box.box_vote(*_device(arrays), torch.from_numpy(kept).cuda(), 0.65).cpu().numpy()
    box_vote_ref.assert_votes(got, ref, np.where((kept >= 0) & (kept < 40), kept, -1), 'positions')
    unused = (kept < 0) | (kept >= 40)
    assert not got[unused].any() and got[~unused].any(axis=1).all()


def test_trained_candidates_behind_hard_nms():
    arrays = box_vote_ref.trained_candidates(GOLDEN)
    dev = _device(arrays)
    hard = _C.nms(*dev, 0.5, 100, return_indices=True)
    kept = hard[3].cpu().numpy()
    ref = box_vote_ref.cached_ref('trained hard', *arrays, kept, 0.65)
    got = box.box_vote(*dev, hard[3], 0.65)
    bad, compared = box_vote_ref.assert_votes(got.cpu().numpy(), ref, kept, 'trained')
    print('trained, hard: %d of %d coordinates not admitted, up to %d voters' % (bad, compared, int(ref[2].max())))
    assert int(ref[2].max()) > 100
    tail = box.suppress(*dev, 0.5, 100, vote=0.65)
    assert torch.equal(tail[0], hard[0]) and torch.equal(tail[1], got) and torch.equal(tail[2], hard[2])


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_trained_candidates_behind_soft_nms(method):
    """The weights are the input scores, not the decayed ones the suppression emits."""
    arrays, soft = soft_nms_ref.trained_reference(GOLDEN, method)
    assert soft[4] >= soft_nms_ref.ADMIT_ULPS, soft[4]
    dev = _device(arrays)
    out = _C.soft_nms(*dev, 0.5, 100, METHODS[method], 0.5, 0.05, return_indices=True)
    assert np.array_equal(out[3].cpu().numpy(), soft[3])
    ref = box_vote_ref.cached_ref('trained ' + method, *arrays, soft[3], 0.65)
    got = box.box_vote(*dev, out[3], 0.65)
    box_vote_ref.assert_votes(got.cpu().numpy(), ref, soft[3], method)
    tail = box.suppress(*dev, 0.5, 100, soft_nms={'method': method, 'sigma': 0.5, 'min_score': 0.05}, vote=0.65)
    _same_bits(tail[0].cpu().numpy(), soft[0]), _same_bits(tail[2].cpu().numpy(), soft[2])
    assert torch.equal(tail[1], got)


def test_concat_candidates_equals_restatement():
    parts = box_vote_ref.concat_parts()
    dev = [_device(p) for p in parts]
    for widths in ([0, 0, 0], [0, 256, 0], [300, 0, 17], [1, 2, 3]):
        ref = box_vote_ref.concat_ref(parts, widths)
        for got in (_C.concat_candidates(dev, widths), box.concat_candidates(dev, widths)):
            assert got[0].shape == (3, 102) and got[1].shape == (3, 102, 4)
            for g, r in zip(got, ref):
                _same_bits(g.cpu().numpy(), r, widths)
    # eight parts, and a list longer than one pass of the launch's grid
    big = box_vote_ref.clustered_case(63, 2, 530001, 5, 40, extent=1024.0)
    eight = [big] + [tuple(a[:2] for a in parts[i % 3]) for i in range(7)]
    widths = [1333, 0, 5, 0, 640, 0, 0, 2]
    ref = box_vote_ref.concat_ref(eight, widths)
    got = _C.concat_candidates([_device(p) for p in eight], widths)
    for g, r in zip(got, ref):
        _same_bits(g.cpu().numpy(), r, 'eight parts')


def test_bindings_streams_and_repeats_agree():
    from odtk import _C_ext
    arrays = _device(box_vote_ref.clustered_case(41, 3, 2100, 6, 20))
    hard = _C.nms(*arrays, 0.5, 150, return_indices=True)
    first = _C.box_vote(*arrays, hard[3], 0.6)
    again = _C.box_vote(*arrays, hard[3], 0.6)                          # immediately behind it
    ext = _C_ext.box_vote(*arrays, hard[3], 0.6)
    parts, widths = [arrays, [t[:, :700].contiguous() for t in arrays]], [0, 512]
    merged = _C.concat_candidates(parts, widths)
    merged_again = _C.concat_candidates(parts, widths)
    merged_ext = _C_ext.concat_candidates(parts, widths)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = _C.box_vote(*arrays, hard[3], 0.6)
        merged_there = _C.concat_candidates(parts, widths)
    side.synchronize()
    torch.cuda.synchronize()
    assert not torch.equal(first, hard[1])
    for other in (again, ext, there):
        assert torch.equal(first, other)
    for other in (merged_again, merged_ext, merged_there):
        assert all(torch.equal(a, b) for a, b in zip(merged, other))


def test_detect_equals_decode_levels_then_checker():
    with np.load(os.path.join(GOLDEN, 'pipeline_clustered_160x256.npz')) as z:
        g = {k: z[k] for k in z.files}
    strides = [int(s) for s in g['strides']]
    cls = [torch.from_numpy(g['cls%d' % i]).cuda() for i in range(len(strides))]
    dl = [torch.from_numpy(g['box%d' % i]).cuda() for i in range(len(strides))]
    anchors = {s: torch.from_numpy(g['anchors%d' % i]) for i, s in enumerate(strides)}
    threshold, top_n, nms, ndet = float(g['threshold']), int(g['top_n']), float(g['nms']), int(g['detections'])
    out = box.detect(cls, dl, strides, anchors, threshold, top_n, nms, ndet, vote=0.65)
    cand = box.decode_levels(cls, dl, strides, threshold, top_n, anchors)
    assert all(np.array_equal(t.cpu().numpy(), g[k]) for t, k in zip((cand[0], cand[2]), ('cat_scores', 'cat_classes')))
    hard = box.detect(cls, dl, strides, anchors, threshold, top_n, nms, ndet)                  # the default path is what it was
    assert np.array_equal(hard[0].cpu().numpy(), g['out_scores']) and np.array_equal(hard[2].cpu().numpy(), g['out_classes'])
    general = _C.nms(*cand, nms, ndet, return_indices=True)
    assert all(torch.equal(h, n) for h, n in zip(hard, general))
    kept = general[3].cpu().numpy()
    ref = box_vote_ref.vote_ref(*_host(cand), kept, 0.65)
    assert torch.equal(out[0], hard[0]) and torch.equal(out[2], hard[2])
    box_vote_ref.assert_votes(out[1].cpu().numpy(), ref, kept, 'detect')
    assert not torch.equal(out[1], hard[1])
    with pytest.raises(ValueError, match='rotated'):
        box.detect(cls, dl, strides, anchors, threshold, top_n, nms, ndet, rotated=True, vote=0.65)


def test_model_branches_honour_the_options_and_the_off_switch():
    """ResNet18FPN at 128 x 128 under bf16 autocast, as tests/test_gpu_soft_nms.py.  The eager network and the BN-folded engine are
    the same function only up to the rounding of the folded weights, so each branch is compared with the checkers on the candidates
    decoded from ITS OWN head tensors of x and of x.flip(-1); the hipGraph replays the engine, so those two are equal.  With the
    options back at None every branch returns what it returned before they were ever set -- the captured graph too."""
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(0)
        model = Model('ResNet18FPN', classes=8)
        model.initialize(None)
        model = model.cuda().to(memory_format=torch.channels_last).eval()
        with torch.no_grad():
            model.cls_head[-1].weight.mul_(60.0)                        # detections exist
        x = torch.randn(2, 3, 128, 128, device='cuda').contiguous(memory_format=torch.channels_last)
        flipped = box.flip_batch(x)
        assert torch.equal(flipped, x.flip(-1)) and flipped.is_contiguous(memory_format=torch.channels_last)
        gaussian = {'method': 'gaussian', 'sigma': 0.5, 'min_score': 0.05}

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
                cls_heads, box_heads = [t.clone() for t in cls_heads], [t.clone() for t in box_heads]
                strides = [inp.shape[-1] // c.shape[-1] for c in cls_heads]
                pairs = [box._pair(c, b) for c, b in zip(cls_heads, box_heads)]
                cand = _C.decode_levels([p[0] for p in pairs], [p[1] for p in pairs], [model.anchors[s] for s in strides], strides,
                                        model.threshold, model.top_n, logits=True, cls_bias=cls_bias, box_bias=box_bias)
            torch.cuda.synchronize()
            return _host(cand)

        def check(out, branch, what):
            cand = own_candidates(branch, x)
            if model.tta is not None:
                cand = box_vote_ref.concat_ref([cand, own_candidates(branch, flipped)], [0, x.shape[-1]])
            if model.soft_nms is not None:
                s, b, c, kept, margin = soft_nms_ref.soft_nms_ref(*cand, model.nms, model.detections, 'gaussian', 0.5, 0.05)
                assert margin >= soft_nms_ref.ADMIT_ULPS, margin
            else:
                s, b, c, kept = _host(_C.nms(*_device(cand), model.nms, model.detections, return_indices=True))
            _same_bits(out[0].cpu().numpy(), s, (what, branch, 'scores'))
            _same_bits(out[2].cpu().numpy(), c, (what, branch, 'classes'))
            if model.box_voting is None:
                _same_bits(out[1].cpu().numpy(), b, (what, branch, 'boxes'))
            else:
                ref = box_vote_ref.vote_ref(*cand, kept, model.box_voting)
                box_vote_ref.assert_votes(out[1].cpu().numpy(), ref, kept, (what, branch))
                assert not np.array_equal(out[1].cpu().numpy(), b)

        before = {b: call(b) for b in ('eager', 'engine', 'graph')}
        assert all(torch.equal(a, b) for a, b in zip(before['engine'], before['graph']))
        assert int((before['engine'][0] > 0).sum()) > 20
        engine = model.inference_engine(torch.bfloat16)
        n_graphs = len(engine._graphs)

        model.box_voting = 0.65
        voted = {b: call(b) for b in ('eager', 'engine', 'graph')}
        assert all(torch.equal(a, b) for a, b in zip(voted['engine'], voted['graph']))       # not the graph captured above
        assert len(engine._graphs) == n_graphs + 1
        for b in ('eager', 'engine'):
            assert torch.equal(voted[b][0], before[b][0]) and not torch.equal(voted[b][1], before[b][1])
            check(voted[b], b, 'voting')

        model.box_voting, model.tta = None, 'flip'
        for b in ('eager', 'engine'):
            out = call(b)
            assert not torch.equal(out[0], before[b][0])
            check(out, b, 'tta')
        with pytest.raises(RuntimeError, match='tta'):
            call('graph')

        model.box_voting, model.soft_nms, model.top_n = 0.5, gaussian, 700
        for b in ('eager', 'engine'):
            check(call(b), b, 'tta + voting + soft-nms')
        model.top_n = 1000                                              # 2 x 5 x 1000 candidates: more than Soft-NMS takes
        for b in ('eager', 'engine'):
            with pytest.raises(ValueError, match='top_n'):
                call(b)

        model.box_voting, model.soft_nms, model.tta = None, None, None
        for b in ('eager', 'engine', 'graph'):
            assert all(torch.equal(a, c) for a, c in zip(before[b], call(b))), b
        assert model.inference_engine(torch.bfloat16) is engine and len(engine._graphs) == n_graphs + 1
    finally:
        torch.backends.cudnn.deterministic = saved
