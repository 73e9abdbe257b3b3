"""Matrix NMS without a GPU: the torch CPU branch (odtk.box._matrix_nms_cpu) against the checker (tests/matrix_nms_ref.py) bit for
bit, cases computed by hand, the checker against a float64 restatement of mmdetection's published formula, the C ABI's argument
checks through the workspace query, the command line, the Model options and the refusals of box.suppress / box.detect."""
import ctypes
import math

import numpy as np
import pytest
import torch

import box_vote_ref
import matrix_nms_ref
from matrix_nms_ref import random_case
from odtk import _C, box
from odtk import main as cli
from odtk.model import Model

F = np.float32


def _run(scores, boxes, classes, method, ndet=4, sigma=0.5, min_score=0.05, pre_top=2000):
    out = box._matrix_nms_cpu(torch.tensor([scores], dtype=torch.float32), torch.tensor([boxes], dtype=torch.float32),
                              torch.tensor([classes], dtype=torch.float32), ndet, method, sigma, min_score, pre_top)
    return [t[0].numpy() for t in out]


def _same_bits(a, b, what=''):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint8), b.view(np.uint32 if b.dtype.itemsize == 4 else np.uint8)), what


# A 10 x 10, B 10 x 5 inside it, C 10 x 4 inside B (the +1 pixel convention): iou(A, B) = 50 / 100, iou(A, C) = 40 / 100,
# iou(B, C) = 40 / 50; cmax(A) = 0, cmax(B) = 0.5
HAND = ([0.9, 0.8, 0.7], [[0, 0, 9, 9], [0, 0, 9, 4], [0, 0, 9, 3]], [2, 2, 2])


def test_linear_by_hand():
    one, ab, ac, bc = F(1), F(50) / F(100), F(40) / F(100), F(40) / F(50)
    d_b = (one - ab) / (one - F(0))
    d_c = min((one - ac) / (one - F(0)), (one - bc) / (one - ab))        # 0.6 from A's row, 0.4 from B's compensated row
    assert d_c == (one - bc) / (one - ab)
    s, b, c, i = _run(*HAND, 'linear')
    _same_bits(s, np.array([F(0.9), F(0.8) * d_b, F(0.7) * d_c, 0], F))
    assert i.tolist() == [0, 1, 2, -1] and c.tolist() == [2, 2, 2, 0]
    _same_bits(b, np.array(HAND[1] + [[0, 0, 0, 0]], F))
    # a floor above C's decayed score drops it; the others keep their places
    s, b, c, i = _run(*HAND, 'linear', min_score=0.3)
    assert i.tolist() == [0, 1, -1, -1] and s[2] == 0


def test_gaussian_by_hand():
    sigma, ab, ac, bc = F(0.5), F(50) / F(100), F(40) / F(100), F(40) / F(50)
    e = lambda cmax, iou: F(math.exp(float(((cmax * cmax) - (iou * iou)) / sigma)))
    d_b = e(F(0), ab)
    d_c = min(e(F(0), ac), e(ab, bc))
    assert d_c == e(ab, bc)
    s, b, c, i = _run(*HAND, 'gaussian')
    _same_bits(s, np.array([F(0.9), F(0.8) * d_b, F(0.7) * d_c, 0], F))
    assert i.tolist() == [0, 1, 2, -1]
    # the decayed scores decide the order: B sinks below C when its own score is only a little higher
    s, b, c, i = _run([0.9, 0.5, 0.49], [[0, 0, 9, 9], [0, 0, 9, 8], [20, 20, 29, 29]], [2, 2, 2], 'gaussian')
    assert i.tolist() == [0, 2, 1, -1] and s[1] == F(0.49)


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_disjoint_boxes_come_out_ranked_with_their_scores(method):
    rng = np.random.default_rng(3)
    n = 40
    x = (np.arange(n) * 20).astype(F)
    boxes = np.stack([x, x, x + 9, x + 9], 1)
    scores = (0.1 + 0.9 * rng.random(n)).astype(F)
    scores[[3, 17]] = 0                                           # padding
    classes = np.zeros(n, F)
    s, b, c, i = _run(scores.tolist(), boxes.tolist(), classes.tolist(), method, ndet=50)
    order = np.array(sorted([k for k in range(n) if scores[k] > 0], key=lambda k: (-scores[k], k)))
    assert i[:38].tolist() == order.tolist() and (i[38:] == -1).all()
    _same_bits(s[:38], scores[order])
    _same_bits(b[:38], boxes[order])


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_other_classes_do_not_decay_each_other(method):
    same = [[5, 5, 30, 40]] * 4
    s, b, c, i = _run([0.9, 0.8, 0.7, 0.6], same, [0, 1, 0, 1], method, min_score=0.2)
    assert i.tolist() == [0, 1, -1, -1]                           # the copies of a class sink to 0 (linear) / e^-2 times ...
    _same_bits(s[:2], np.array([0.9, 0.8], F))                    # ... the firsts of the two classes are untouched
    s, b, c, i = _run([0.9, 0.8, 0.7, 0.6], same, [0, 1, 2, 3], method)
    assert i.tolist() == [0, 1, 2, 3]
    _same_bits(s, np.array([0.9, 0.8, 0.7, 0.6], F))


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_cpu_branch_equals_checker_on_random_candidates(seed, method):
    classes, pre_top = ((1, 2000), (3, 150), (80, 2000))[seed]
    arrays = random_case(50 + seed, 2, 400, classes, extent=64.0)
    ref = matrix_nms_ref.matrix_nms_ref(*arrays, 120, method, 0.4, 0.1, pre_top)
    out = box._matrix_nms_cpu(*[torch.from_numpy(a) for a in arrays], 120, method, 0.4, 0.1, pre_top)
    for o, r, name in zip(out, ref, ('scores', 'boxes', 'classes', 'positions')):
        _same_bits(o.numpy(), r, (seed, method, name))
    public = box.matrix_nms(*[torch.from_numpy(a) for a in arrays], 120, method, 0.4, 0.1, pre_top)
    assert len(public) == 3 and all(torch.equal(p, o) for p, o in zip(public, out))


def test_cpu_branch_equals_checker_on_nan_duplicates_ties_and_padding():
    s, b, c = random_case(60, 1, 120, 2, padding=0.2)
    b[0, 5] = b[0, 66] = [5, 5, 4, 9]                             # area 0 twice: IoU 0 / 0
    b[0, 7] = b[0, 40] = b[0, 90] = [10, 12, 40, 50]              # copies: cmax = 1, d = 0 / 0 and x / 0
    c[0, [5, 66, 7, 40, 90]] = 1
    s[0, [5, 66, 7, 40, 90]] = [0.99, 0.98, 0.97, 0.97, 0.5]      # (a tie among the copies)
    s[0, 100] = np.nan
    for method in ('linear', 'gaussian'):
        ref = matrix_nms_ref.matrix_nms_ref(s, b, c, 100, method, 0.5, 0.2, 2000)
        out = box._matrix_nms_cpu(*[torch.from_numpy(a) for a in (s, b, c)], 100, method, 0.5, 0.2, 2000)
        for o, r, name in zip(out, ref, ('scores', 'boxes', 'classes', 'positions')):
            _same_bits(o.numpy(), r, (method, name))
        kept = ref[3][0].tolist()
        assert 5 in kept and 66 in kept and 7 in kept and 40 not in kept and 90 not in kept and 100 not in kept


def _mmdet_float64(scores, boxes, classes, method, sigma, pre_top):
    """mmdetection's mask_matrix_nms (mmdet/models/layers/matrix_nms.py) in float64 on box IoUs: sort, the upper triangle of the
    IoU matrix masked by the labels, column maximum (compensation), decay matrix, column minimum.  Its `sigma` multiplies where
    this project's divides: 1 / sigma is handed over.  -> (positions in rank order, decay coefficients)."""
    order = matrix_nms_ref.participants(scores, pre_top)
    b, labels = boxes[order].astype(np.float64), classes[order]
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    wh = np.clip(np.minimum(b[:, None, 2:], b[None, :, 2:]) - np.maximum(b[:, None, :2], b[None, :, :2]) + 1, 0, None)
    inter = wh[..., 0] * wh[..., 1]
    iou = np.triu(inter / (area[:, None] + area[None, :] - inter), 1)
    label_matrix = np.triu(labels[:, None] == labels[None, :], 1)
    decay_iou = iou * label_matrix
    compensate_iou = decay_iou.max(0)[:, None]
    if method == 'gaussian':
        mm_sigma = 1 / sigma
        decay_matrix = np.exp(-1 * mm_sigma * (decay_iou ** 2)) / np.exp(-1 * mm_sigma * (compensate_iou ** 2))
    else:
        decay_matrix = (1 - decay_iou) / (1 - compensate_iou)
    return order, decay_matrix.min(0)


# The checker's float32 decay against its own float64 run (decay_of(.., dtype=np.float64)) on the three candidate sets below,
# measured as max |f32 - f64| / f64: 1.76e-7, 1.47e-7, 1.01e-7 (linear) and 1.20e-7, 9.4e-8, 7.1e-8 (gaussian) -- two or three
# float32 roundings of 6e-8 each; the cancellations in 1 - iou and 1 - cmax amplify little on these boxes (whole-pixel corners,
# sides 2..23, no copies: an IoU below 1 stays below ~0.95).  The bound sits an order of magnitude over the largest measurement
# and five below what a wrong formula gives (the uncompensated decay differs by tens of percent).
MMDET_REL_BOUND = 2e-6


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
@pytest.mark.parametrize('seed,classes', [(70, 1), (71, 5), (72, 80)])
def test_checker_agrees_with_mmdetections_formula_in_float64(seed, classes, method):
    s, b, c = random_case(seed, 1, 500, classes, extent=64.0)
    s, b, c = s[0], b[0], c[0]
    # no copies: mmdetection divides by 1 - 1 = 0 there, which the definition skips by rule (the NaN cases are tested above)
    _, first = np.unique(b, axis=0, return_index=True)
    keep = np.sort(first)
    s, b, c = s[keep], b[keep], c[keep]
    assert keep.size > 400 and not np.isnan(b).any()
    order, decay32, _ = matrix_nms_ref.decay_of(s, b, c, method, 0.5, 2000)
    order64, decay64, _ = matrix_nms_ref.decay_of(s, b, c, method, 0.5, 2000, dtype=np.float64)
    order_mm, decay_mm = _mmdet_float64(s, b, c, method, 0.5, 2000)
    assert np.array_equal(order, order64) and np.array_equal(order, order_mm)
    own = np.abs(decay32.astype(np.float64) - decay64) / decay64
    print('checker float32 against float64: max relative difference %.3g' % own.max())
    assert own.max() <= MMDET_REL_BOUND
    assert np.abs(decay64 - decay_mm).max() <= 1e-12 * max(1.0, decay_mm.max())      # the same formula in the same arithmetic
    rel = np.abs(decay32.astype(np.float64) - decay_mm) / decay_mm
    print('checker float32 against mmdetection float64: max relative difference %.3g' % rel.max())
    assert rel.max() <= MMDET_REL_BOUND
    assert (decay_mm < 0.9).sum() > 10                            # the decay is at work on these boxes


def test_options_are_validated():
    args = (torch.rand(1, 4), torch.rand(1, 4, 4), torch.zeros(1, 4))
    for bad in (dict(method='hard'), dict(sigma=0), dict(sigma=float('inf')), dict(min_score=0), dict(min_score=float('nan')),
                dict(pre_top=0), dict(pre_top=4097), dict(pre_top=1.5)):
        with pytest.raises(ValueError):
            box.matrix_nms(*args, **bad)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        _C.matrix_nms(*args, 3, 2000, _C.MATRIX_NMS_LINEAR, 0.5, 0.05)
    anchors = {8: box.generate_anchors(8, [1.0], [4.0])}
    with pytest.raises(ValueError, match='rotated'):
        box.detect([torch.rand(1, 4, 3, 3)], [torch.zeros(1, 6, 3, 3)], [8], anchors, rotated=True, matrix_nms={'method': 'linear'})
    with pytest.raises(ValueError, match='exclude'):
        box.detect([torch.rand(1, 4, 3, 3)], [torch.zeros(1, 4, 3, 3)], [8], anchors, matrix_nms={}, soft_nms={'method': 'linear'})
    with pytest.raises(ValueError, match='exclude'):
        box.suppress(*args, matrix_nms={'method': 'linear'}, soft_nms={'method': 'linear'})
    for bad in ({'method': 'hard'}, {'sigma': -1}, {'pre_top': 5000}, {'min_score': 0}, {'threshold': 0.5}):
        with pytest.raises(ValueError):
            box.suppress(*args, matrix_nms=bad)
    # the CPU branch behind box.suppress: min_score defaults to `threshold`, the rule to gaussian, pre_top to 2000
    s, b, c = [torch.from_numpy(a) for a in box_vote_ref.clustered_case(80, 2, 60, 2, 3)]
    for got, want in zip(box.suppress(s, b, c, 0.5, 20, matrix_nms={}, threshold=0.07),
                         box._matrix_nms_cpu(s, b, c, 20, 'gaussian', 0.5, 0.07, 2000)):
        assert torch.equal(got, want)
    voted = box.suppress(s, b, c, 0.5, 20, matrix_nms={'method': 'linear'}, vote=0.65, threshold=0.07)
    plain = box._matrix_nms_cpu(s, b, c, 20, 'linear', 0.5, 0.07, 2000)
    assert torch.equal(voted[0], plain[0]) and torch.equal(voted[2], plain[2])
    assert torch.equal(voted[1], box.box_vote(s, b, c, plain[3], 0.65)) and not torch.equal(voted[1], plain[1])


def test_abi_validates_before_touching_the_device():
    lib = _C.library()

    def query(batch=8, n_out=3, count=5000, ndet=100, pre=2000, method=_C.MATRIX_NMS_LINEAR, sigma=0.5, floor=0.05, flags=0):
        return lib.odtk_matrix_nms(batch, None, None, n_out, count, ndet, pre, method, sigma, floor, flags, None, 0, None)
    size = query()
    assert size > 8 * 5000 * 8 and size % 256 == 0
    assert query(method=_C.MATRIX_NMS_GAUSSIAN, n_out=4) == size
    assert query(count=_C.MAX_NMS_COUNT + 1) > 0 and query(batch=1, count=_C.MAX_NMS_COUNT_SCRATCH) > 0     # no 7680 cap
    assert query(pre=1) > 0 and query(pre=_C.MAX_MATRIX_NMS_PRE) > size and query(ndet=2048) == size
    for bad in (dict(method=0), dict(method=3), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float('inf')), dict(sigma=float('nan')),
                dict(floor=0.0), dict(floor=-0.1), dict(floor=float('inf')), dict(floor=float('nan')), dict(flags=8), dict(flags=1 << 31),
                dict(flags=_C.FLAG_ROTATED | 16), dict(batch=0), dict(batch=-1), dict(count=0), dict(count=_C.MAX_NMS_COUNT_SCRATCH + 1),
                dict(ndet=0), dict(ndet=2049), dict(pre=0), dict(pre=-5), dict(pre=_C.MAX_MATRIX_NMS_PRE + 1)):
        assert query(**bad) == _C.ERR_INVALID, bad
    assert query(flags=_C.FLAG_ROTATED) == _C.ERR_UNSUPPORTED
    buf = ctypes.create_string_buffer(64)
    big = (ctypes.c_char * size)()
    ins = (ctypes.c_void_p * 3)(1 << 20, 1 << 20, 1 << 20)
    outs = (ctypes.c_void_p * 3)(1 << 20, 1 << 20, 1 << 20)
    tail = (3, 5000, 100, 2000, 1, 0.5, 0.05, 0)
    assert lib.odtk_matrix_nms(8, ins, outs, *tail, ctypes.cast(buf, ctypes.c_void_p), 64, None) == _C.ERR_WORKSPACE
    ws = ctypes.cast(big, ctypes.c_void_p)
    assert lib.odtk_matrix_nms(8, None, outs, *tail, ws, size, None) == _C.ERR_INVALID                      # null pointers
    assert lib.odtk_matrix_nms(8, ins, None, *tail, ws, size, None) == _C.ERR_INVALID
    assert lib.odtk_matrix_nms(8, (ctypes.c_void_p * 3)(1 << 20, None, 1 << 20), outs, *tail, ws, size, None) == _C.ERR_INVALID
    assert lib.odtk_matrix_nms(8, ins, (ctypes.c_void_p * 3)(1 << 20, 1 << 20, None), *tail, ws, size, None) == _C.ERR_INVALID
    assert lib.odtk_matrix_nms(8, ins, outs, 2, *tail[1:], ws, size, None) == _C.ERR_INVALID
    assert 'odtk_matrix_nms' in _C.exported_symbols()
    from odtk import _C_ext
    assert hasattr(_C_ext, 'matrix_nms')
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        _C_ext.matrix_nms(torch.rand(1, 5), torch.rand(1, 5, 4), torch.zeros(1, 5), 3, 2000, 1, 0.5, 0.05)


def test_command_line_flags():
    args = cli.parse(['infer', 'm.pth', '--matrix-nms', 'linear', '--matrix-nms-sigma', '0.3', '--matrix-nms-min-score', '0.01',
                      '--matrix-nms-pre', '1500'])
    assert (args.matrix_nms, args.matrix_nms_sigma, args.matrix_nms_min_score, args.matrix_nms_pre) == ('linear', 0.3, 0.01, 1500)
    model = Model('ResNet18FPN', classes=3)
    assert model.matrix_nms is None
    assert cli.matrix_nms_options(args, model) == {'method': 'linear', 'sigma': 0.3, 'min_score': 0.01, 'pre_top': 1500}
    args = cli.parse(['train', 'm.pth', '--annotations', 'a.json', '--matrix-nms', 'gaussian'])
    assert cli.matrix_nms_options(args, model) == {'method': 'gaussian', 'sigma': 0.5, 'min_score': model.threshold, 'pre_top': 2000}
    assert cli.soft_nms_options(args, model) is None
    plain = cli.parse(['infer', 'm.pth'])
    assert not any(hasattr(plain, f) for f in ('matrix_nms', 'matrix_nms_sigma', 'matrix_nms_min_score', 'matrix_nms_pre'))
    assert cli.matrix_nms_options(plain, model) is None
    for refused in (['infer', 'm.pth', '--matrix-nms', 'linear', '--rotated-bbox'],
                    ['train', 'm.pth', '--annotations', 'a.json', '--rotated-bbox', '--matrix-nms', 'gaussian'],
                    ['infer', 'm.pth', '--matrix-nms', 'linear', '--soft-nms', 'linear'],
                    ['infer', 'm.pth', '--matrix-nms-sigma', '0.3'], ['infer', 'm.pth', '--matrix-nms-min-score', '0.3'],
                    ['infer', 'm.pth', '--matrix-nms-pre', '100'], ['infer', 'm.pth', '--matrix-nms', 'hard'],
                    ['infer', 'm.pth', '--matrix-nms', 'linear', '--matrix-nms-pre', '0'],
                    ['infer', 'm.pth', '--matrix-nms', 'linear', '--matrix-nms-pre', '4097']):
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
    model.matrix_nms = {'method': 'gaussian', 'sigma': 0.25, 'pre_top': 900}
    out = model.postprocess(logits, dl, strides)
    ref = matrix_nms_ref.matrix_nms_ref(*[t.numpy() for t in cat], model.detections, 'gaussian', 0.25, model.threshold, 900)
    for o, r in zip(out, ref):
        _same_bits(o.numpy(), r)
    assert not torch.equal(out[0], plain[0])
    model.matrix_nms = None
    assert all(torch.equal(a, b) for a, b in zip(model.postprocess(logits, dl, strides), plain))
    for bad, match in (({'method': 'hard'}, 'method'), ({'sigma': 0}, 'sigma'), ({'pre_top': 0}, 'pre_top'), ({'nms': 0.5}, 'unknown'),
                       ('gaussian', 'dict')):
        model.matrix_nms = bad
        with pytest.raises(ValueError, match=match):
            model.postprocess(logits, dl, strides)
    model.matrix_nms, model.soft_nms = {'method': 'linear'}, {'method': 'linear'}
    with pytest.raises(ValueError, match='soft_nms'):
        model.postprocess(logits, dl, strides)
    model.soft_nms, model.rotated_bbox = None, True
    with pytest.raises(ValueError, match='rotated'):
        model.postprocess(logits, dl, strides)
    model.rotated_bbox = False
    path = str(tmp_path / 'm.pth')
    model.save({'path': path})
    assert not any('matrix' in k for k in torch.load(path, map_location='cpu'))
    assert Model.load(path)[0].matrix_nms is None
