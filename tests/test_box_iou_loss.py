"""IoU / GIoU / DIoU box losses (odtk/loss.py:box_iou_loss, include/odtk_hip.h: odtk_box_iou_loss_levels_*; `Model.box_loss`,
`odtk train --box-loss`) without a GPU: the torch restatement against closed forms worked out by hand and against numerical
differentiation, `Model._compute_loss` on CPU tensors against the hand-composed expression, the command line, and the host-side
argument checks of the two entry points (they precede anything that touches HIP)."""
import ctypes
import math

import pytest
import torch

from odtk import _C
from odtk import main as cli
from odtk.loss import BBOX_XFORM_CLIP, BOX_LOSS_KINDS, anchor_wh, box_iou_loss, focal_loss, smooth_l1_loss
from odtk.model import Model

KINDS = ('iou', 'giou', 'diou')


def _one(p, t, size, kind, dtype=torch.float64):
    """One anchor of size `size`: deltas p, t (4 numbers each) -> the loss as a 0-d tensor."""
    pred = torch.tensor(p, dtype=dtype).view(1, 1, 4, 1, 1)
    target = torch.tensor(t, dtype=dtype).view(1, 1, 4, 1, 1)
    return box_iou_loss(pred, target, torch.tensor([size], dtype=dtype), kind).reshape(())


def test_kinds():
    assert BOX_LOSS_KINDS == KINDS
    assert BBOX_XFORM_CLIP == math.log(1000.0 / 16)
    with pytest.raises(ValueError, match='kind'):
        _one([0.0] * 4, [0.0] * 4, (2.0, 2.0), 'ciou')


@pytest.mark.parametrize('kind', KINDS)
def test_identical_boxes(kind):
    for deltas, size in (([0.0, 0.0, 0.0, 0.0], (2.0, 2.0)), ([0.3, -0.2, 0.4, -0.7], (45.25, 22.63)), ([-1.5, 2.0, 1.2, 0.1], (812.0, 406.0))):
        for dtype in (torch.float64, torch.float32):
            assert abs(float(_one(deltas, deltas, size, kind, dtype))) <= 1e-6


def test_unit_offset_squares():
    """Two 2 x 2 squares, one shifted by 1 along x: inter 2, union 6, IoU 1/3; the enclosing box is 3 x 2 = the union (GIoU term 0),
    its squared diagonal 13, the centres 1 apart."""
    p, t, size = [0.5, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], (2.0, 2.0)
    assert float(_one(p, t, size, 'iou')) == pytest.approx(2 / 3, rel=1e-7)
    assert float(_one(p, t, size, 'giou')) == pytest.approx(2 / 3, rel=1e-7)
    assert float(_one(p, t, size, 'diou')) == pytest.approx(2 / 3 + 1 / 13, rel=1e-7)
    # the same along y, on a 2 x 4 anchor whose target is the 2 x 2 square (th = log 1/2), prediction shifted by 1 px: py = 1/4
    p, t, size = [0.0, 0.25, 0.0, math.log(0.5)], [0.0, 0.0, 0.0, math.log(0.5)], (2.0, 4.0)
    assert float(_one(p, t, size, 'iou')) == pytest.approx(2 / 3, rel=1e-7)
    assert float(_one(p, t, size, 'diou')) == pytest.approx(2 / 3 + 1 / 13, rel=1e-7)


def test_disjoint_boxes():
    """Two 2 x 2 squares whose centres are 5 apart along x (a gap of 3): IoU 0, union 8, enclosing box 7 x 2."""
    p, t, size = [2.5, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], (2.0, 2.0)
    assert float(_one(p, t, size, 'iou')) == pytest.approx(1.0, rel=1e-9)
    assert float(_one(p, t, size, 'giou')) == pytest.approx(1 + (14 - 8) / 14, rel=1e-7)
    assert float(_one(p, t, size, 'diou')) == pytest.approx(1 + 25 / (49 + 4), rel=1e-7)
    # disjoint boxes still have a gradient towards each other with giou / diou, none with iou
    for kind, moves in (('iou', False), ('giou', True), ('diou', True)):
        pred = torch.tensor(p, dtype=torch.float64).view(1, 1, 4, 1, 1).requires_grad_(True)
        box_iou_loss(pred, torch.zeros(1, 1, 4, 1, 1, dtype=torch.float64), torch.tensor([size], dtype=torch.float64), kind).sum().backward()
        assert (float(pred.grad[0, 0, 0]) > 0) == moves


@pytest.mark.parametrize('kind', KINDS)
def test_clip_of_the_predicted_sizes(kind):
    size, t = (32.0, 64.0), [0.1, -0.1, 0.2, 0.3]
    at = _one([0.2, 0.1, BBOX_XFORM_CLIP, 0.1], t, size, kind)
    for beyond in (BBOX_XFORM_CLIP + 0.5, 50.0):
        pred = torch.tensor([0.2, 0.1, beyond, 0.1], dtype=torch.float64).view(1, 1, 4, 1, 1).requires_grad_(True)
        loss = box_iou_loss(pred, torch.tensor(t, dtype=torch.float64).view(1, 1, 4, 1, 1), torch.tensor([size], dtype=torch.float64), kind)
        assert float(loss.detach()) == float(at)
        loss.sum().backward()
        assert float(pred.grad[0, 0, 2]) == 0.0 and float(pred.grad[0, 0, 3]) != 0.0       # (ph is below the clip)
    # the targets are not clipped
    assert float(_one(t, [0.1, -0.1, BBOX_XFORM_CLIP + 0.5, 0.3], size, kind)) != float(_one(t, [0.1, -0.1, BBOX_XFORM_CLIP, 0.3], size, kind))


@pytest.mark.parametrize('kind', KINDS)
def test_common_shift_changes_nothing(kind):
    size = (22.6, 45.3)
    p, t = [0.31, -0.12, 0.2, -0.3], [0.1, 0.05, -0.1, 0.1]
    base = float(_one(p, t, size, kind))
    for sx, sy in ((1.0, 0.0), (-0.75, 2.5), (13.0, -7.0)):
        moved = float(_one([p[0] + sx, p[1] + sy, p[2], p[3]], [t[0] + sx, t[1] + sy, t[2], t[3]], size, kind))
        assert moved == pytest.approx(base, rel=1e-12, abs=1e-13)


def _random_anchors(seed, n, noise):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.rand(n, 2, generator=g, dtype=torch.float64) * 790 + 22
    target = torch.randn(1, n, 4, 1, 1, generator=g, dtype=torch.float64) * torch.tensor([0.3, 0.3, 0.2, 0.2], dtype=torch.float64).view(1, 1, 4, 1, 1)
    pred = target + torch.randn(1, n, 4, 1, 1, generator=g, dtype=torch.float64) * noise
    return pred, target, sizes


@pytest.mark.parametrize('kind', KINDS)
def test_gradcheck(kind):
    for seed, noise in ((1, 0.15), (2, 1.0)):           # overlapping pairs; pairs that are partly disjoint (iou's clamp at 0)
        pred, target, sizes = _random_anchors(seed, 20, noise)
        assert torch.autograd.gradcheck(lambda p: box_iou_loss(p, target, sizes, kind), (pred.requires_grad_(True),), eps=1e-6, atol=1e-7,
                                        rtol=1e-5)


@pytest.mark.parametrize('kind', KINDS)
def test_float32_follows_float64(kind):
    """The arithmetic the kernel uses, in torch: float32 sums within 1e-6 relative of float64 (the bar of the GPU tests)."""
    for noise in (0.01, 0.15, 1.0):
        pred, target, sizes = _random_anchors(7, 2000, noise)
        want = float(box_iou_loss(pred, target, sizes, kind).sum())
        got = float(box_iou_loss(pred.float(), target.float(), sizes.float(), kind).double().sum())
        assert abs(got - want) <= 1e-6 * abs(want)


def test_shapes_and_anchor_sizes():
    anchors = torch.tensor([[-12.0, -12.0, 19.0, 19.0], [-7.3, -18.6, 14.3, 25.6]])
    assert torch.equal(anchor_wh(anchors), torch.tensor([[32.0, 32.0], [14.3 + 7.3 + 1, 25.6 + 18.6 + 1]]))
    out = box_iou_loss(torch.zeros(2, 2, 4, 3, 5), torch.zeros(2, 2, 4, 3, 5), anchor_wh(anchors), 'giou')
    assert out.shape == (2, 2, 3, 5) and out.dtype == torch.float32
    # a NaN delta reaches the loss of its anchor, whichever delta it is, and no other anchor
    for k in range(4):
        pred = torch.zeros(1, 2, 4, 1, 1)
        pred[0, 1, k] = float('nan')
        for kind in KINDS:
            out = box_iou_loss(pred, torch.zeros(1, 2, 4, 1, 1), anchor_wh(anchors), kind).reshape(2)
            assert math.isnan(float(out[1])) and not math.isnan(float(out[0])), (k, kind)


# ---------------------------------------------------------------------------------------------------------------- Model
def _model_batch():
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=3)
    model.initialize(None)
    model.train()
    g = torch.Generator().manual_seed(11)
    images = torch.randn(2, 3, 64, 96, generator=g)
    targets = torch.tensor([[[8.0, 8.0, 32.0, 32.0, 0.0], [40.0, 16.0, 45.0, 23.0, 2.0], [20.0, 20.0, 40.0, 40.0, 1.0]],
                            [[50.0, 4.0, 32.0, 32.0, 1.0], [4.0, 10.0, 23.0, 45.0, 0.0], [30.0, 14.0, 40.0, 40.0, 2.0]]])
    with torch.no_grad():
        cls_heads, box_heads = model.heads(images)
    # head values of a trained-ish net: the fresh box head predicts ~0, which sits on no tie but is dull
    box_heads = [b + 0.1 * torch.randn(b.shape, generator=g) for b in box_heads]
    return model, images, targets, cls_heads, box_heads


def _composed(model, images, targets, cls_heads, box_heads, kind, weight):
    """model.py's eager loss written out, with `kind` (None: the smooth-L1 criterion) for the boxes."""
    cls_total, box_total, foreground = 0.0, 0.0, 0.0
    n_fg = 0
    for cls_head, box_head in zip(cls_heads, box_heads):
        stride = images.shape[-1] / cls_head.shape[-1]
        cls_target, box_target, depth = model._extract_targets(targets, stride, cls_head.shape[-2:])
        n_fg += int((depth > 0).sum())
        foreground = foreground + (depth > 0).sum().float().clamp(min=1)
        cls_loss = focal_loss(cls_head.view_as(cls_target).float(), cls_target, 0.25, 2)
        cls_total = cls_total + (cls_loss * (depth >= 0).expand_as(cls_target).float()).sum()
        if kind is None:
            box_loss = smooth_l1_loss(box_head.view_as(box_target).float(), box_target, 0.11)
            box_total = box_total + (box_loss * (depth > 0).expand_as(box_target).float()).sum()
        else:
            anchors = model.level_anchors(stride)
            wh = torch.stack([anchors[:, 2] - anchors[:, 0] + 1, anchors[:, 3] - anchors[:, 1] + 1], 1)
            box_loss = box_iou_loss(box_head.view_as(box_target).float(), box_target, wh, kind)
            box_total = box_total + (box_loss * (depth[:, :, 0] > 0).float()).sum()
    assert n_fg >= 3                                               # the boxes were chosen to hit anchors
    if kind is None:
        return cls_total / foreground, box_total / foreground
    return cls_total / foreground, weight * box_total / foreground


def test_model_loss_on_the_cpu():
    model, images, targets, cls_heads, box_heads = _model_batch()
    assert (model.box_loss, model.box_loss_weight) == ('smooth_l1', 1.0)
    before = _composed(model, images, targets, cls_heads, box_heads, None, 1.0)
    for value in (None, 'smooth_l1'):                               # never set; set to the default
        if value is not None:
            model.box_loss = value
        got = model._compute_loss(images, cls_heads, box_heads, targets)
        assert torch.equal(got[0], before[0]) and torch.equal(got[1], before[1])
    seen = {}
    for kind in KINDS:
        for weight in (1.0, 2.5):
            model.box_loss, model.box_loss_weight = kind, weight
            got = model._compute_loss(images, cls_heads, box_heads, targets)
            want = _composed(model, images, targets, cls_heads, box_heads, kind, weight)
            assert torch.equal(got[0], before[0])
            torch.testing.assert_close(got[1], want[1], rtol=1e-6, atol=0)
            seen[kind, weight] = float(got[1])
        assert seen[kind, 2.5] == pytest.approx(2.5 * seen[kind, 1.0], rel=1e-6)
    assert len({round(v, 6) for v in seen.values()}) == len(seen) and all(0 < v < 10 for v in seen.values())
    assert float(before[1]) not in seen.values()


def test_model_loss_differentiates_on_the_cpu():
    model, images, targets, cls_heads, box_heads = _model_batch()
    model.box_loss = 'giou'
    heads = [b.clone().requires_grad_(True) for b in box_heads]
    model._compute_loss(images, cls_heads, heads, targets)[1].backward()
    assert any(float(h.grad.abs().max()) > 0 for h in heads) and all(torch.isfinite(h.grad).all() for h in heads)


def test_model_refusals():
    model, images, targets, cls_heads, box_heads = _model_batch()
    model.box_loss = 'ciou'
    with pytest.raises(ValueError, match='box_loss'):
        model._compute_loss(images, cls_heads, box_heads, targets)
    model.box_loss = 'giou'
    for weight in (0.0, -1.0, float('inf'), float('nan'), None, 'heavy'):
        model.box_loss_weight = weight
        with pytest.raises(ValueError, match='box_loss_weight'):
            model._compute_loss(images, cls_heads, box_heads, targets)
    model.box_loss_weight = 1.0
    model.rotated_bbox = True
    with pytest.raises(ValueError, match='rotated'):
        model._compute_loss(images, cls_heads, box_heads, targets)


def test_checkpoints_do_not_carry_the_option(tmp_path):
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=3)
    plain, giou = str(tmp_path / 'plain.pth'), str(tmp_path / 'giou.pth')
    model.save({'path': plain})
    model.box_loss, model.box_loss_weight = 'giou', 2.0
    model.save({'path': giou})
    a, b = torch.load(plain, map_location='cpu'), torch.load(giou, map_location='cpu')
    assert a.keys() == b.keys() and a['state_dict'].keys() == b['state_dict'].keys()
    assert not any('box_loss' in k for k in list(b) + list(b['state_dict']))
    loaded = Model.load(giou)[0]
    assert (loaded.box_loss, loaded.box_loss_weight) == ('smooth_l1', 1.0)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_command_line_flags():
    base = ['train', 'm.pth', '--annotations', 'a.json']
    plain = cli.parse(base)
    assert not hasattr(plain, 'box_loss') and not hasattr(plain, 'box_loss_weight')
    for kind in ('smooth-l1', 'iou', 'giou', 'diou'):
        args = cli.parse(base + ['--box-loss', kind])
        assert args.box_loss == kind and not hasattr(args, 'box_loss_weight')
        assert {k: v for k, v in vars(args).items() if k != 'box_loss'} == vars(plain)      # nothing else in the namespace moves
    args = cli.parse(base + ['--box-loss', 'giou', '--box-loss-weight', '2.5'])
    assert (args.box_loss, args.box_loss_weight) == ('giou', 2.5)
    assert cli.parse(base + ['--box-loss', 'smooth-l1', '--rotated-bbox']).box_loss == 'smooth-l1'
    for refused in (base + ['--box-loss-weight', '2'], base + ['--box-loss', 'smooth-l1', '--box-loss-weight', '2'],
                    base + ['--box-loss', 'giou', '--box-loss-weight', '0'], base + ['--box-loss', 'giou', '--box-loss-weight', '-1'],
                    base + ['--box-loss', 'giou', '--box-loss-weight', 'inf'], base + ['--box-loss', 'giou', '--box-loss-weight', 'nan'],
                    base + ['--box-loss', 'iou', '--rotated-bbox'], base + ['--box-loss', 'giou', '--rotated-bbox'],
                    base + ['--box-loss', 'diou', '--rotated-bbox'], base + ['--box-loss', 'ciou'],
                    ['infer', 'm.pth', '--box-loss', 'giou'], ['infer', 'm.pth', '--box-loss-weight', '2']):
        with pytest.raises(SystemExit):
            cli.parse(refused)
    for flag in ('--box-loss', '--box-loss-weight'):
        assert [spec['help'] for name, spec in cli.TRAIN_FLAGS if name == flag][0]
    assert 'resum' in [spec['help'] for name, spec in cli.TRAIN_FLAGS if name == '--box-loss'][0]
    assert '--box-loss' in cli.__doc__


# ---------------------------------------------------------------------------------------------------------------- C ABI, host side
SIZES = ((40, 56), (1, 3))
NEED = 2560                      # 158 + 1 workgroups of 256 cells, 16 bytes each, rounded up to 256


def _levels(sizes=SIZES, **fields):
    levels = (_C.LossLevel * len(sizes))()
    for lv, (h, w) in zip(levels, sizes):
        lv.box = lv.depth = lv.box_target = lv.dbox = 1 << 20                 # never dereferenced: every call here is refused
        lv.height, lv.width, lv.channels_last = h, w, 1
    for name, value in fields.items():
        setattr(levels[len(sizes) - 1], name, value)
    return levels


def _tables(n=2, a=9, box=(-12.0, -12.0, 19.0, 19.0), last=None):
    keep = [(ctypes.c_float * (4 * a))(*(list(box) * a)) for _ in range(n)]
    if last is not None:
        keep[-1][4 * (a - 1):4 * a] = last
    return (_C._fp * n)(*[ctypes.cast(k, _C._fp) for k in keep]), keep


def test_abi_validates_before_touching_the_device():
    lib = _C.library()
    assert {'odtk_box_iou_loss_levels_forward', 'odtk_box_iou_loss_levels_backward'} <= set(_C.exported_symbols())
    assert (_C.BOX_LOSS_IOU, _C.BOX_LOSS_GIOU, _C.BOX_LOSS_DIOU) == (1, 2, 3)
    assert lib.odtk_abi_struct_size(3) == ctypes.sizeof(_C.LossLevel) == 64       # the level descriptor is reused unchanged
    tables, keep = _tables()
    buf = ctypes.create_string_buffer(NEED + 16)
    ws = (ctypes.addressof(buf) + 15) & ~15

    def forward(n_levels=2, lv=None, tab=tables, batch=2, a=9, dtype=_C.F32, kind=_C.BOX_LOSS_GIOU, sums=1 << 20, ws=None, size=0):
        return lib.odtk_box_iou_loss_levels_forward(n_levels, _levels() if lv is None else lv, tab, batch, a, dtype, kind, sums, ws, size, None)

    def backward(n_levels=2, lv=None, tab=tables, batch=2, a=9, dtype=_C.F32, kind=_C.BOX_LOSS_GIOU, grads=1 << 20):
        return lib.odtk_box_iou_loss_levels_backward(n_levels, _levels() if lv is None else lv, tab, batch, a, dtype, kind, grads, None)

    # the two-phase query: a NULL workspace answers the bytes needed and looks at no data pointer
    assert forward() == NEED and forward(sums=None, lv=_levels(box=None, depth=None, box_target=None)) == NEED
    assert forward(n_levels=1) == 2560 and forward(batch=1, a=1, tab=_tables(2, 1)[0]) == 256     # 158; 9 + 1 workgroups
    for dtype in (_C.F32, _C.BF16, _C.F16):
        for kind in (1, 2, 3):
            assert forward(dtype=dtype, kind=kind) == NEED
    shared = [dict(n_levels=0), dict(n_levels=_C.MAX_LEVELS + 1), dict(a=0), dict(a=_C.MAX_ANCHORS + 1), dict(batch=0), dict(batch=-2),
              dict(kind=0), dict(kind=4), dict(kind=-1), dict(lv=ctypes.POINTER(_C.LossLevel)()), dict(tab=ctypes.POINTER(_C._fp)()),
              dict(lv=_levels(height=0)), dict(lv=_levels(width=-1)), dict(lv=_levels(channels_last=2)),
              dict(lv=_levels(((40, 56), (8192, 4096)))),                                   # 2 * 9 * 4 * H * W >= 2^31
              dict(tab=(_C._fp * 2)(ctypes.cast(keep[0], _C._fp), _C._fp()))]              # a level without an anchor table
    for last in ((0.0, 0.0, float('inf'), 1.0), (0.0, 0.0, 1.0, float('nan')), (0.0, 0.0, -1.0, 5.0), (0.0, 5.0, 5.0, 3.0),
                 (float('-inf'), 0.0, 1.0, 1.0)):
        shared.append(dict(tab=_tables(last=last)[0]))
    for bad in shared:
        assert forward(**bad) == _C.ERR_INVALID, bad                # already the query refuses these
        assert forward(ws=ws, size=NEED, **bad) == _C.ERR_INVALID, bad
        assert backward(**bad) == _C.ERR_INVALID, bad
    for call in (forward, lambda **kw: forward(ws=ws, size=NEED, **kw), backward):
        assert call(dtype=3) == _C.ERR_UNSUPPORTED and call(dtype=-1) == _C.ERR_UNSUPPORTED
    # with a workspace: the data pointers, the workspace itself
    for field in ('box', 'depth', 'box_target'):
        assert forward(ws=ws, size=NEED, lv=_levels(**{field: None})) == _C.ERR_INVALID, field
        assert backward(lv=_levels(**{field: None})) == _C.ERR_INVALID, field
    assert backward(lv=_levels(dbox=None)) == _C.ERR_INVALID
    assert forward(ws=ws, size=NEED, sums=None) == _C.ERR_INVALID
    assert forward(ws=ws, size=NEED - 1) == _C.ERR_INVALID and forward(ws=ws, size=0) == _C.ERR_INVALID     # too small
    assert forward(ws=ws + 4, size=NEED) == _C.ERR_INVALID and forward(ws=ws, size=NEED, sums=(1 << 20) + 4) == _C.ERR_INVALID
    # channels_last heads are read and written as one vector per cell: 16 bytes for fp32, 8 for the 16-bit types
    assert forward(ws=ws, size=NEED, lv=_levels(box=(1 << 20) + 8)) == _C.ERR_INVALID
    assert forward(ws=ws, size=NEED, dtype=_C.BF16, lv=_levels(box=(1 << 20) + 4)) == _C.ERR_INVALID
    assert backward(lv=_levels(dbox=(1 << 20) + 8)) == _C.ERR_INVALID
    assert backward(grads=(1 << 20) + 2) == _C.ERR_INVALID


def test_binding_refuses_cpu_tensors_and_bad_lists():
    head, depth, target = torch.zeros(1, 4, 2, 2), torch.zeros(1, 1, 1, 2, 2), torch.zeros(1, 1, 4, 2, 2)
    anchors = [torch.tensor([[0.0, 0.0, 7.0, 7.0]])]
    with pytest.raises(RuntimeError, match='GPU'):
        _C.box_iou_loss_levels_forward([head], [depth], [target], anchors, 'giou')
    with pytest.raises(RuntimeError, match='kind'):
        _C.box_iou_loss_levels_forward([head], [depth], [target], anchors, 'ciou')
    with pytest.raises(RuntimeError, match='levels'):
        _C.box_iou_loss_levels_forward([head] * 7, [depth] * 7, [target] * 7, anchors * 7, 'giou')
    with pytest.raises(RuntimeError, match='levels'):
        _C.box_iou_loss_levels_backward([head], [depth], [target], [], 'giou', None)
