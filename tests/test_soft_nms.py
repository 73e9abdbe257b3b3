"""Soft-NMS (linear and Gaussian; include/odtk_hip.h: odtk_soft_nms) without a GPU: hand-computed cases, odtk.box.soft_nms on
CPU tensors against the checker (tests/soft_nms_ref.py) bit for bit, the properties that tie it to the hard rule, the C ABI's
argument validation (it never touches the device) and the command-line flags."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import soft_nms_ref
from odtk import _C, box
from odtk import main as cli
from odtk.model import Model

F = np.float32
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def _run(scores, boxes, classes, method, nms=0.5, ndet=4, sigma=0.5, min_score=0.05):
    out = box.soft_nms(torch.tensor([scores], dtype=torch.float32), torch.tensor([boxes], dtype=torch.float32),
                       torch.tensor([classes], dtype=torch.float32), nms, ndet, method, sigma, min_score)
    return [o[0].numpy() for o in out]


def _same_bits(a, b, what=''):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


# one pixel high; widths 5 and a shift of 1: inter 4, union 6 -> IoU 2/3.  Widths 4 and a shift of 2: inter 2, union 6 -> 1/3
TWO_THIRDS = [[0, 0, 4, 0], [1, 0, 5, 0]]
ONE_THIRD = [[0, 0, 3, 0], [2, 0, 5, 0]]


def test_linear_by_hand():
    s, b, c = _run([0.9, 0.8], TWO_THIRDS, [3, 3], 'linear')
    _same_bits(s, [F(0.9), F(0.8) * (F(1) - F(4) / F(6)), 0, 0])             # above the threshold: decayed, not dropped
    _same_bits(b[:2], TWO_THIRDS)
    _same_bits(c, [3, 3, 0, 0])
    assert abs(float(s[1]) - 0.8 / 3) < 1e-7
    s, _, _ = _run([0.9, 0.8], ONE_THIRD, [3, 3], 'linear')
    _same_bits(s, [F(0.9), F(0.8), 0, 0])                                    # IoU <= nms: untouched
    s, _, _ = _run([0.9, 0.8], ONE_THIRD, [3, 3], 'linear', nms=0.25)
    _same_bits(s, [F(0.9), F(0.8) * (F(1) - F(2) / F(6)), 0, 0])


def test_gaussian_by_hand():
    for pair, iou in ((TWO_THIRDS, F(4) / F(6)), (ONE_THIRD, F(2) / F(6))):
        s, _, _ = _run([0.9, 0.8], pair, [3, 3], 'gaussian', sigma=0.5)
        factor = F(math.exp(float((-(iou * iou)) / F(0.5))))
        _same_bits(s, [F(0.9), F(0.8) * factor, 0, 0])
        assert abs(float(s[1]) - 0.8 * math.exp(-float(iou) ** 2 / 0.5)) < 1e-6
    # every same-class neighbour is decayed, whatever nms says
    a = _run([0.9, 0.8], ONE_THIRD, [3, 3], 'gaussian', nms=0.9)
    b = _run([0.9, 0.8], ONE_THIRD, [3, 3], 'gaussian', nms=0.1)
    _same_bits(a[0], b[0])


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_other_classes_are_untouched(method):
    s, b, c = _run([0.9, 0.8], TWO_THIRDS, [3, 4], method)
    _same_bits(s, [F(0.9), F(0.8), 0, 0])
    _same_bits(c, [3, 4, 0, 0])


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_neighbour_below_min_score_is_dropped(method):
    s, b, c = _run([0.9, 0.8], TWO_THIRDS, [3, 3], method, min_score=0.4)      # 0.267 (linear) / 0.329 (gaussian) < 0.4
    _same_bits(s, [F(0.9), 0, 0, 0])
    _same_bits(b[1:], np.zeros((3, 4)))
    s, _, _ = _run([0.9, 0.8], TWO_THIRDS, [3, 3], method, min_score=0.2)
    assert s[1] > 0.2 and s[2] == 0
    # a candidate that starts below min_score is alive (w > 0) until a pick of its class visits it
    s, _, _ = _run([0.9, 0.01], [[0, 0, 4, 0], [50, 0, 54, 0]], [3, 3], method, min_score=0.05)
    _same_bits(s, [F(0.9), 0, 0, 0])
    s, _, _ = _run([0.9, 0.01], [[0, 0, 4, 0], [50, 0, 54, 0]], [3, 4], method, min_score=0.05)
    _same_bits(s, [F(0.9), F(0.01), 0, 0])


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_equal_scores_resolve_to_the_lower_position(method):
    boxes = [[40, 0, 44, 0], [0, 0, 4, 0], [20, 0, 24, 0], [1, 0, 5, 0]]
    out = box._soft_nms_cpu(torch.tensor([[0.5, 0.7, 0.7, 0.7]]), torch.tensor([boxes], dtype=torch.float32),
                            torch.tensor([[1., 1., 1., 1.]]), 0.5, 4, method, 0.5, 0.05)
    # 1 before 2 before 3 at equal score; 3 is then decayed by 1 (IoU 2/3) and falls behind 0
    assert out[3][0].tolist() == [1, 2, 0, 3]
    assert out[0][0, 0] == out[0][0, 1] == F(0.7) and out[0][0, 2] == F(0.5) and 0 < out[0][0, 3] < 0.5


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_nan_iou_dies(method):
    # two degenerate boxes of area 0 (x2 = x1 - 1): inter 0, union 0 -> IoU NaN -> the decayed score is NaN -> not alive
    degenerate = [[5, 5, 4, 9], [5, 5, 4, 9], [30, 30, 34, 34]]
    s, b, c = _run([0.9, 0.8, 0.7], degenerate, [2, 2, 2], method)
    _same_bits(s, [F(0.9), F(0.7), 0, 0])
    _same_bits(b[:2], [degenerate[0], degenerate[2]])


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_cpu_branch_equals_checker_on_trained_candidates(method):
    (scores, boxes, classes), ref = soft_nms_ref.trained_reference(GOLDEN, method)
    assert int((scores > 0).sum(1).max()) == 2552
    assert ref[4] >= soft_nms_ref.ADMIT_ULPS, ref[4]          # the inputs admit a bit test (tests/soft_nms_ref.py)
    out = box._soft_nms_cpu(torch.from_numpy(scores), torch.from_numpy(boxes), torch.from_numpy(classes), 0.5, 100, method, 0.5, 0.05)
    for o, r, what in zip(out[:3], ref, ('scores', 'boxes', 'classes')):
        _same_bits(o.numpy(), r, what)
    assert np.array_equal(out[3].numpy(), ref[3])
    assert (np.diff(ref[0], axis=1) <= 0).all()                # emitted scores are non-increasing


@pytest.mark.parametrize('seed', range(20))
def test_cpu_branch_equals_checker_on_random_candidates(seed):
    rng = np.random.default_rng(1000 + seed)
    count, num_classes, ndet = int(rng.integers(1, 301)), int(rng.integers(1, 9)), int(rng.choice([1, 7, 100, 300]))
    scores, boxes, classes = soft_nms_ref.random_case(seed, 2, count, num_classes)
    for method, nms, sigma, floor in (('linear', 0.3, 0.5, 0.2), ('gaussian', 0.5, 0.3, 0.1)):
        ref = soft_nms_ref.soft_nms_ref(scores, boxes, classes, nms, ndet, method, sigma, floor)
        assert ref[4] >= soft_nms_ref.ADMIT_ULPS, (seed, ref[4])
        out = box.soft_nms(torch.from_numpy(scores), torch.from_numpy(boxes), torch.from_numpy(classes), nms, ndet, method, sigma, floor)
        assert len(out) == 3
        for o, r, what in zip(out, ref, ('scores', 'boxes', 'classes')):
            _same_bits(o.numpy(), r, (seed, method, what))
        assert (np.diff(ref[0], axis=1) <= 0).all()


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_equals_hard_nms_when_no_same_class_boxes_overlap(method):
    rng = np.random.default_rng(7)
    cells = rng.permutation(400)[:150]
    x, y = (cells % 20) * 10.0, (cells // 20) * 10.0
    boxes = np.stack([x, y, x + 8, y + 8], 1).astype(F)[None]                # 9 x 9 pixels on a 10-pixel grid: disjoint
    boxes = np.concatenate([boxes, boxes], 1)                                # ... and each once more, in ANOTHER class
    classes = np.concatenate([np.zeros(150), np.ones(150)]).astype(F)[None]
    scores = (0.06 + 0.9 * rng.random((1, 300))).astype(F)
    scores[0, ::7] = 0
    args = [torch.from_numpy(a) for a in (scores, boxes, classes)]
    for ndet in (50, 300):
        hard = box.nms(*args, 0.5, ndet)
        soft = box.soft_nms(*args, 0.5, ndet, method, 0.5, 0.05)
        for h, s in zip(hard, soft):
            _same_bits(s.numpy(), h.numpy())


def test_options_are_validated():
    args = (torch.rand(1, 4), torch.rand(1, 4, 4), torch.zeros(1, 4))
    for bad in (dict(method='hard'), dict(sigma=0), dict(sigma=float('inf')), dict(min_score=0), dict(min_score=float('nan'))):
        with pytest.raises(ValueError):
            box.soft_nms(*args, **bad)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        _C.soft_nms(*args, 0.5, 3, _C.SOFT_NMS_LINEAR, 0.5, 0.05)
    anchors = {8: box.generate_anchors(8, [1.0], [4.0])}
    with pytest.raises(ValueError, match='rotated'):
        box.detect([torch.rand(1, 4, 3, 3)], [torch.zeros(1, 6, 3, 3)], [8], anchors, rotated=True, soft_nms={'method': 'linear'})


def test_abi_validates_before_touching_the_device():
    lib = _C.library()

    def query(batch=8, n_out=3, count=5000, ndet=100, thresh=0.5, method=_C.SOFT_NMS_LINEAR, sigma=0.5, floor=0.05, flags=0):
        return lib.odtk_soft_nms(batch, None, None, n_out, count, ndet, thresh, method, sigma, floor, flags, None, 0, None)
    assert query() == 256 and query(method=_C.SOFT_NMS_GAUSSIAN, count=_C.MAX_NMS_COUNT, n_out=4) == 256     # a token size
    for bad in (dict(method=0), dict(method=3), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float('inf')), dict(sigma=float('nan')),
                dict(floor=0.0), dict(floor=-0.1), dict(floor=float('inf')), dict(floor=float('nan')), dict(flags=8), dict(flags=1 << 31),
                dict(flags=_C.FLAG_ROTATED | 16), dict(batch=0), dict(count=0), dict(ndet=0)):
        assert query(**bad) == _C.ERR_INVALID, bad
    assert query(flags=_C.FLAG_ROTATED) == _C.ERR_UNSUPPORTED
    assert query(count=_C.MAX_NMS_COUNT + 1) == _C.ERR_UNSUPPORTED
    buf = ctypes.create_string_buffer(64)
    ins = (ctypes.c_void_p * 3)(1 << 20, 1 << 20, 1 << 20)
    outs = (ctypes.c_void_p * 3)(1 << 20, 1 << 20, 1 << 20)
    assert lib.odtk_soft_nms(8, ins, outs, 3, 5000, 100, 0.5, 1, 0.5, 0.05, 0, ctypes.cast(buf, ctypes.c_void_p), 64, None) == _C.ERR_WORKSPACE
    assert lib.odtk_soft_nms(8, None, outs, 3, 5000, 100, 0.5, 1, 0.5, 0.05, 0, ctypes.cast(buf, ctypes.c_void_p), 256, None) == _C.ERR_INVALID
    assert 'odtk_soft_nms' in _C.exported_symbols()
    from odtk import _C_ext
    assert hasattr(_C_ext, 'soft_nms')
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        _C_ext.soft_nms(torch.rand(1, 5), torch.rand(1, 5, 4), torch.zeros(1, 5), 0.5, 3, 1, 0.5, 0.05)


def test_command_line_flags():
    args = cli.parse(['infer', 'm.pth', '--soft-nms', 'gaussian', '--soft-nms-sigma', '0.3', '--soft-nms-min-score', '0.01'])
    assert (args.soft_nms, args.soft_nms_sigma, args.soft_nms_min_score) == ('gaussian', 0.3, 0.01)
    model = Model('ResNet18FPN', classes=3)
    assert model.soft_nms is None
    assert cli.soft_nms_options(args, model) == {'method': 'gaussian', 'sigma': 0.3, 'min_score': 0.01}
    args = cli.parse(['train', 'm.pth', '--annotations', 'a.json', '--soft-nms', 'linear'])
    assert cli.soft_nms_options(args, model) == {'method': 'linear', 'sigma': 0.5, 'min_score': model.threshold}
    plain = cli.parse(['infer', 'm.pth'])
    assert not hasattr(plain, 'soft_nms') and cli.soft_nms_options(plain, model) is None
    for refused in (['infer', 'm.pth', '--soft-nms', 'linear', '--rotated-bbox'],
                    ['train', 'm.pth', '--annotations', 'a.json', '--rotated-bbox', '--soft-nms', 'gaussian'],
                    ['infer', 'm.pth', '--soft-nms-sigma', '0.3'], ['infer', 'm.pth', '--soft-nms', 'hard']):
        with pytest.raises(SystemExit):
            cli.parse(refused)


def test_model_cpu_branch_honours_the_option_and_checkpoints_do_not_carry_it(tmp_path):
    from odtk import synthetic
    cls, dl, strides = synthetic.pyramid(2, 9, 3, 64, 96, 'clustered', 11)
    logits = [torch.logit(c.clamp(1e-6, 1 - 1e-6)) for c in cls]
    model = Model('ResNet18FPN', classes=3)
    model.eval()
    for s in strides:
        model.level_anchors(s)
    plain = model.postprocess(logits, dl, strides)
    per_level = [box.decode(c.sigmoid().contiguous(), d.contiguous(), s, model.threshold, model.top_n, model.anchors[s])
                 for c, d, s in zip(logits, dl, strides)]
    cat = [torch.cat(p, 1) for p in zip(*per_level)]
    for x, y in zip(plain, box.nms(*cat, model.nms, model.detections)):
        assert torch.equal(x, y)
    model.soft_nms = {'method': 'gaussian', 'sigma': 0.25, 'min_score': 0.05}
    soft = model.postprocess(logits, dl, strides)
    ref = soft_nms_ref.soft_nms_ref(*[t.numpy() for t in cat], model.nms, model.detections, 'gaussian', 0.25, 0.05)
    assert ref[4] >= soft_nms_ref.ADMIT_ULPS
    for o, r in zip(soft, ref):
        _same_bits(o.numpy(), r)
    assert not torch.equal(soft[0], plain[0])
    model.rotated_bbox = True
    with pytest.raises(ValueError, match='rotated'):
        model.postprocess(logits, dl, strides)
    model.rotated_bbox = False
    path = str(tmp_path / 'm.pth')
    model.save({'path': path})
    assert not any('soft' in k for k in torch.load(path, map_location='cpu'))
    assert Model.load(path)[0].soft_nms is None
