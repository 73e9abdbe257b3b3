"""Box voting and flip test-time augmentation without a GPU: the pure-torch branches of odtk.box against the checker
(tests/box_vote_ref.py: exact weighted means, bit equality where the inputs admit it), the C entries' argument checks through
ctypes, the command line, and Model on CPU tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import box_vote_ref
import soft_nms_ref
from odtk import _C, box
from odtk import main as cli
from odtk.model import Model

F = np.float32
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def _t(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]


def _same_bits(a, b, what=''):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


def _hard_kept(arrays, nms, ndet):
    """The torch hard NMS with its new position output: what it returned before, plus positions that name the emitted boxes."""
    tensors = _t(arrays)
    plain = box._nms_cpu(*tensors, nms, ndet)
    full = box._nms_cpu(*tensors, nms, ndet, return_indices=True)
    assert len(plain) == 3 and len(full) == 4 and full[3].dtype == torch.int32
    assert all(torch.equal(a, b) for a, b in zip(plain, full))
    kept = full[3].numpy()
    for image in range(kept.shape[0]):
        used = kept[image] >= 0
        assert np.array_equal(used, full[0][image].numpy() > 0)
        _same_bits(arrays[1][image][kept[image][used]], full[1][image].numpy()[used])
        _same_bits(arrays[0][image][kept[image][used]], full[0][image].numpy()[used])
    return full


@pytest.mark.parametrize('case', list(box_vote_ref.CASES))
def test_torch_branch_equals_checker_on_clustered_candidates(case):
    make, nms, ndet, vote = box_vote_ref.CASES[case]
    arrays = make()
    hard = _hard_kept(arrays, nms, ndet)
    kept = hard[3].numpy()
    ref = box_vote_ref.cached_ref(('cpu', case), *arrays, kept, vote)
    got = box.box_vote(*_t(arrays), hard[3], vote)
    bad, compared = box_vote_ref.assert_votes(got.numpy(), ref, kept, case)
    print('%s: %d of %d coordinates not admitted, up to %d voters, %.0f %% of the coordinates moved'
          % (case, bad, compared, int(ref[2].max(initial=0)), 100.0 * float((got != hard[1])[kept >= 0].float().mean()) if compared else 0))
    tail = box.suppress(*_t(arrays), nms, ndet, vote=vote)
    assert torch.equal(tail[0], hard[0]) and torch.equal(tail[2], hard[2]) and torch.equal(tail[1], got)
    if case == '7680_one_class':
        assert int(ref[2].max()) > 1000                              # the double accumulation has something to add up
    if case == 'nan_iou':
        slot = int(np.flatnonzero(kept[0] == 5)[0])
        assert 66 not in kept[0] and ref[2][0, slot] == 1            # the other zero-area box is suppressed (NaN IoU) and no voter
        _same_bits(got.numpy()[0, slot], arrays[1][0, 5])
    if case == 'vote_thresh_1':
        assert int(ref[2].max()) == 1                                # no two boxes of the case are equal: everybody votes alone
        _same_bits(got.numpy(), hard[1].numpy())
    if case == 'equal_scores_and_duplicates':
        assert int(ref[2][kept >= 0].min()) >= 2                     # the duplicate always votes


def test_torch_branch_equals_checker_on_trained_candidates():
    arrays = box_vote_ref.trained_candidates(GOLDEN)
    hard = _hard_kept(arrays, 0.5, 100)
    kept = hard[3].numpy()
    ref = box_vote_ref.cached_ref('trained hard', *arrays, kept, 0.65)
    got = box.box_vote(*_t(arrays), hard[3], 0.65)
    bad, compared = box_vote_ref.assert_votes(got.numpy(), ref, kept, 'trained')
    assert int(ref[2].max()) > 100                                   # a trained detector's clusters: hundreds of voters
    assert float((got != hard[1])[kept >= 0].float().mean()) > 0.5   # ... and most coordinates move
    print('trained: %d of %d coordinates not admitted, up to %d voters' % (bad, compared, int(ref[2].max())))


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_torch_tail_behind_soft_nms(method):
    """The weights are the INPUT scores, also behind Soft-NMS, whose emitted scores are the decayed ones."""
    arrays = box_vote_ref.CASES['count257_vote05'][0]()
    soft = soft_nms_ref.soft_nms_ref(*arrays, 0.5, 101, method, 0.5, 0.05)
    assert soft[4] >= soft_nms_ref.ADMIT_ULPS
    options = {'method': method, 'sigma': 0.5, 'min_score': 0.05}
    out = box.suppress(*_t(arrays), 0.5, 101, soft_nms=options, vote=0.5)
    _same_bits(out[0].numpy(), soft[0])
    _same_bits(out[2].numpy(), soft[2])
    ref = box_vote_ref.vote_ref(*arrays, soft[3], 0.5)
    box_vote_ref.assert_votes(out[1].numpy(), ref, soft[3], method)
    assert not np.array_equal(out[1].numpy(), soft[1])
    plain = box.suppress(*_t(arrays), 0.5, 101, soft_nms=options)
    for o, r in zip(plain, soft[:3]):
        _same_bits(o.numpy(), r)


def test_unused_and_out_of_range_positions_give_zeros():
    arrays = box_vote_ref.clustered_case(50, 2, 40, 2, 2, padding=0.0)
    kept = np.array([[3, -1, 40, 7, -1, -1], [-1, 0, 39, 1 << 20, -5, 2]], np.int32)
    ref = box_vote_ref.vote_ref(*arrays, kept, 0.65)
    got = box.box_vote(*_t(arrays), torch.from_numpy(kept), 0.65).numpy()
    box_vote_ref.assert_votes(got, ref, np.where((kept >= 0) & (kept < 40), kept, -1), 'positions')
    unused = (kept < 0) | (kept >= 40)
    assert not got[unused].any() and got[~unused].any(axis=1).all()
    for bad in (0, -0.5, 1.5, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            box.box_vote(*_t(arrays), torch.from_numpy(kept), bad)


def test_torch_concat_equals_restatement():
    parts = box_vote_ref.concat_parts()
    for widths in ([0, 0, 0], [0, 256, 0], [300, 0, 17], [1, 2, 3]):
        ref = box_vote_ref.concat_ref(parts, widths)
        got = box.concat_candidates([_t(p) for p in parts], widths)
        assert got[0].shape == (3, 102) and got[1].shape == (3, 102, 4)
        for g, r in zip(got, ref):
            _same_bits(g.numpy(), r, widths)
    mirrored = box.concat_candidates([_t(parts[1])], [256])
    positive = parts[1][0] > 0
    assert np.array_equal(mirrored[1].numpy()[positive][:, 0], F(255) - parts[1][1][positive][:, 2])
    _same_bits(mirrored[1].numpy()[~positive], parts[1][1][~positive])
    twice = box.concat_candidates([mirrored], [256])                  # whole-pixel corners would come back exactly; these need not
    assert np.allclose(twice[1].numpy(), parts[1][1], atol=1e-4)
    with pytest.raises(ValueError):
        box.concat_candidates([_t(parts[0])] * 9, [0] * 9)
    with pytest.raises(ValueError):
        box.concat_candidates([_t(parts[0])], [-1])
    with pytest.raises(ValueError):
        box.concat_candidates([_t(parts[0])], [0, 0])


def test_abi_validates_before_touching_the_device():
    lib = _C.library()
    assert {'odtk_box_vote', 'odtk_concat_candidates'} <= set(_C.exported_symbols())
    assert lib.odtk_abi_struct_size(9) == ctypes.sizeof(_C.Candidates) == 32 and lib.odtk_abi_struct_size(10) == -1
    ins = (ctypes.c_void_p * 3)(1 << 20, 1 << 20, 1 << 20)            # never dereferenced on these paths
    some = 1 << 20

    def vote(batch=8, inputs=ins, kept=some, out=some, count=5000, ndet=100, thresh=0.65, flags=0):
        return lib.odtk_box_vote(batch, inputs, kept, out, count, ndet, thresh, flags, None)
    for bad in (dict(inputs=None), dict(inputs=(ctypes.c_void_p * 3)(some, None, some)), dict(kept=None), dict(out=None), dict(batch=0),
                dict(batch=-1), dict(count=0), dict(count=_C.MAX_NMS_COUNT_SCRATCH + 1), dict(ndet=0), dict(ndet=2049), dict(thresh=0.0),
                dict(thresh=-0.5), dict(thresh=1.0001), dict(thresh=float('nan')), dict(thresh=float('inf')), dict(flags=8),
                dict(flags=1 << 31), dict(flags=_C.FLAG_ROTATED | 16)):
        assert vote(**bad) == _C.ERR_INVALID, bad
    assert vote(flags=_C.FLAG_ROTATED) == _C.ERR_UNSUPPORTED

    outs = (ctypes.c_void_p * 3)(some, some, some)

    def table(n=2, count=1000, width=0, scores=some, boxes=some, classes=some):
        parts = (_C.Candidates * max(n, 1))()
        for p in parts:
            p.scores, p.boxes, p.classes, p.count, p.mirror_width = scores, boxes, classes, count, width
        return parts

    def concat(batch=8, n=2, parts=None, outputs=outs, flags=0, **how):
        return lib.odtk_concat_candidates(batch, n, table(n, **how) if parts is None else parts, outputs, flags, None)
    for bad in (dict(batch=0), dict(n=0), dict(n=9), dict(n=-1), dict(outputs=None), dict(outputs=(ctypes.c_void_p * 3)(some, some, None)),
                dict(count=0), dict(count=_C.MAX_NMS_COUNT_SCRATCH + 1), dict(n=8, count=_C.MAX_NMS_COUNT_SCRATCH // 8 + 1),
                dict(width=-1), dict(width=-(1 << 31)), dict(scores=None), dict(boxes=None), dict(classes=None), dict(flags=8),
                dict(flags=_C.FLAG_ROTATED | 32)):
        assert concat(**bad) == _C.ERR_INVALID, bad
    assert lib.odtk_concat_candidates(8, 2, None, outs, 0, None) == _C.ERR_INVALID
    assert concat(flags=_C.FLAG_ROTATED) == _C.ERR_UNSUPPORTED
    from odtk import _C_ext
    assert hasattr(_C_ext, 'box_vote') and hasattr(_C_ext, 'concat_candidates')
    cpu = (torch.rand(1, 5), torch.rand(1, 5, 4), torch.zeros(1, 5))
    for module in (_C, _C_ext):
        with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
            module.box_vote(*cpu, torch.zeros(1, 3, dtype=torch.int32), 0.65)
        with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
            module.concat_candidates([cpu], [0])


def test_command_line_flags():
    args = cli.parse(['infer', 'm.pth', '--box-voting', '0.65', '--tta', 'flip'])
    assert (args.box_voting, args.tta) == (0.65, 'flip')
    args = cli.parse(['train', 'm.pth', '--annotations', 'a.json', '--box-voting', '1', '--tta', 'flip'])
    assert (args.box_voting, args.tta) == (1.0, 'flip')
    plain = cli.parse(['infer', 'm.pth'])
    assert not hasattr(plain, 'box_voting') and not hasattr(plain, 'tta')
    model = Model('ResNet18FPN', classes=3)
    assert model.box_voting is None and model.tta is None
    for refused in (['infer', 'm.pth', '--box-voting', '0.65', '--rotated-bbox'], ['infer', 'm.pth', '--tta', 'flip', '--rotated-bbox'],
                    ['train', 'm.pth', '--annotations', 'a.json', '--rotated-bbox', '--tta', 'flip'],
                    ['infer', 'm.pth', '--box-voting', '0'], ['infer', 'm.pth', '--box-voting', '1.01'], ['infer', 'm.pth', '--box-voting', 'nan'],
                    ['infer', 'm.pth', '--box-voting', '-0.3'], ['infer', 'm.pth', '--tta', 'scale'], ['export', 'm.pth', 'e', '--tta', 'flip']):
        with pytest.raises(SystemExit):
            cli.parse(refused)


def _model_and_input():
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=3)
    model.initialize(None)
    model.eval()
    with torch.no_grad():
        model.cls_head[-1].weight.mul_(60.0)                           # detections exist
    return model, torch.randn(2, 3, 64, 96)


def _cpu_candidates(model, x):
    """The reference's sequence on the model's own head tensors of `x`: decode per level, concatenate."""
    with torch.no_grad():
        cls_heads, box_heads = model.heads(x)
    strides = [x.shape[-1] // c.shape[-1] for c in cls_heads]
    per_level = [box.decode(c.sigmoid().contiguous(), d.contiguous(), s, model.threshold, model.top_n, model.level_anchors(s))
                 for c, d, s in zip(cls_heads, box_heads, strides)]
    return [torch.cat(p, 1).numpy() for p in zip(*per_level)]


def test_model_on_cpu_tensors_honours_the_options_and_the_off_switch(tmp_path):
    model, x = _model_and_input()
    model.top_n = 300

    def run():
        with torch.no_grad():
            return [t.clone() for t in model(x)]

    def expect(cand, soft):
        """(scores, boxes, classes) of the tail on `cand`: the suppression's checker or the torch NMS, then the vote checker."""
        if soft is None:
            s, b, c, kept = (t.numpy() for t in _hard_kept(cand, model.nms, model.detections))
        else:
            s, b, c, kept, margin = soft_nms_ref.soft_nms_ref(*cand, model.nms, model.detections, soft['method'], soft['sigma'], soft['min_score'])
            assert margin >= soft_nms_ref.ADMIT_ULPS
        return s, c, kept, b

    default = run()
    cand = _cpu_candidates(model, x)
    assert int((default[0] > 0).sum()) > 20
    for d, e in zip(default, box.nms(*_t(cand), model.nms, model.detections)):
        assert torch.equal(d, e)

    model.box_voting = 0.65
    voted = run()
    s, c, kept, _ = expect(cand, None)
    _same_bits(voted[0].numpy(), s), _same_bits(voted[2].numpy(), c)
    box_vote_ref.assert_votes(voted[1].numpy(), box_vote_ref.vote_ref(*cand, kept, 0.65), kept, 'box_voting')
    assert torch.equal(voted[0], default[0]) and not torch.equal(voted[1], default[1])

    model.box_voting, model.tta = None, 'flip'
    flipped = run()
    merged = box_vote_ref.concat_ref([cand, _cpu_candidates(model, x.flip(-1))], [0, x.shape[-1]])
    assert merged[0].shape[1] == 2 * cand[0].shape[1]
    for f, e in zip(flipped, box.nms(*_t(merged), model.nms, model.detections)):
        assert torch.equal(f, e)
    assert not torch.equal(flipped[0], default[0])

    model.box_voting, model.soft_nms = 0.5, {'method': 'gaussian', 'sigma': 0.5, 'min_score': 0.05}
    everything = run()
    s, c, kept, _ = expect(merged, model.soft_nms)
    _same_bits(everything[0].numpy(), s), _same_bits(everything[2].numpy(), c)
    box_vote_ref.assert_votes(everything[1].numpy(), box_vote_ref.vote_ref(*merged, kept, 0.5), kept, 'tta + soft + voting')
    model.top_n = 1000                                                  # 2 x 5 x 1000 candidates: more than Soft-NMS takes
    with pytest.raises(ValueError, match='top_n'):
        run()
    model.top_n = 300

    model.rotated_bbox = True
    for options in ((0.65, None), (None, 'flip')):
        model.box_voting, model.tta, model.soft_nms = options + (None,)
        with pytest.raises(ValueError, match='rotated'):
            model.check_inference_options()
        with pytest.raises(ValueError, match='rotated'):
            model.postprocess([torch.zeros(1, 27, 2, 2)], [torch.zeros(1, 54, 2, 2)], [8])
    model.rotated_bbox = False
    model.box_voting, model.tta = 0.65, 'mirror'
    with pytest.raises(ValueError, match='tta'):
        run()
    model.box_voting, model.tta = 0.65, 'flip'
    path = str(tmp_path / 'm.pth')
    model.save({'path': path})
    assert not any('vot' in k or 'tta' in k for k in torch.load(path, map_location='cpu'))
    loaded = Model.load(path)[0]
    assert loaded.box_voting is None and loaded.tta is None

    model.box_voting, model.tta = None, None
    for d, e in zip(default, run()):
        assert torch.equal(d, e)
