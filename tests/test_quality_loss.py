"""Quality focal and varifocal classification losses (odtk/loss.py: box_quality, quality_target, quality_focal_loss, varifocal_loss;
include/odtk_hip.h: odtk_quality_loss_levels_*; `Model.cls_loss`, `odtk train --cls-loss`) without a GPU: the torch restatement
against the float64 numpy one written from the formulas (tests/quality_loss_ref.py), its autograd against the closed-form
gradients and central differences, the identities that pin it to the existing focal loss, `Model._compute_loss` on CPU tensors,
the command line, and the host-side argument checks of the two entry points (they precede anything that touches HIP)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import quality_loss_ref as ref
from odtk import _C
from odtk import main as cli
from odtk.loss import (CLS_LOSS_KINDS, anchor_wh, box_iou_loss, box_quality, focal_loss, quality_focal_loss, quality_target,
                       varifocal_loss)
from odtk.model import Model

GAMMAS = (2.0, 1.5, 1.0, 3.0)


def _close(got, want, tol=1e-12):
    """|got - want| <= tol (1 + |want|), elementwise: float64 rounding of sums of a few terms of size |want|."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= tol * (1 + np.abs(want))), float(np.abs(got - want).max())


def _elements(seed=0, n=4000):
    """Logits over +-12 with the special values mixed in, and soft targets: zeros, ones and a spread over (0, 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g, dtype=torch.float64) * 4
    x[:12] = torch.tensor([0.0, -0.0, 100.0, -100.0, 30.0, -30.0, 63.9, 64.1, -64.1, 1e-9, 700.0, -700.0], dtype=torch.float64)
    y = torch.rand(n, generator=g, dtype=torch.float64)
    y[::3] = 0.0
    y[1::7] = 1.0
    y[:12] = torch.tensor([0.5, 0.0, 0.3, 0.3, 1.0, 1.0, 0.0, 0.0, 0.7, 0.2, 0.0, 0.9], dtype=torch.float64)
    return x, y


def test_kinds():
    assert CLS_LOSS_KINDS == ('qfl', 'vfl')
    assert (_C.CLS_LOSS_QFL, _C.CLS_LOSS_VFL) == (1, 2) and _C.CLS_LOSS_KINDS == {'qfl': 1, 'vfl': 2}


@pytest.mark.parametrize('gamma', GAMMAS)
def test_torch_functions_follow_the_numpy_restatement(gamma):
    x, y = _elements()
    want, want_grad = ref.qfl(x.numpy(), y.numpy(), gamma)
    assert np.isfinite(want).all() and np.isfinite(want_grad).all()
    xg = x.clone().requires_grad_(True)
    got = quality_focal_loss(xg, y, gamma)
    assert got.dtype == torch.float64 and got.shape == x.shape
    _close(got.detach().numpy(), want)
    got.sum().backward()
    _close(xg.grad.numpy(), want_grad)                       # autograd == the closed form of the issue
    for alpha in (0.75, 0.25):
        want, want_grad = ref.vfl(x.numpy(), y.numpy(), alpha, gamma)
        xg = x.clone().requires_grad_(True)
        got = varifocal_loss(xg, y, alpha, gamma)
        _close(got.detach().numpy(), want)
        got.sum().backward()
        _close(xg.grad.numpy(), want_grad)


@pytest.mark.parametrize('gamma', (2.0, 1.5))
def test_gradients_against_central_differences(gamma):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(300, generator=g, dtype=torch.float64) * 3
    y = torch.rand(300, generator=g, dtype=torch.float64)
    y[::4] = 0.0
    h = 1e-6
    for fn in (lambda v: ref.qfl(v, y.numpy(), gamma), lambda v: ref.vfl(v, y.numpy(), 0.75, gamma)):
        numeric = (fn(x.numpy() + h)[0] - fn(x.numpy() - h)[0]) / (2 * h)
        assert np.abs(numeric - fn(x.numpy())[1]).max() <= 1e-8          # O(h^2) truncation + 1e-16 / h rounding
    assert torch.autograd.gradcheck(lambda v: quality_focal_loss(v, y, gamma), (x.clone().requires_grad_(True),), eps=1e-6, atol=1e-7,
                                    rtol=1e-5)
    assert torch.autograd.gradcheck(lambda v: varifocal_loss(v, y, 0.75, gamma), (x.clone().requires_grad_(True),), eps=1e-6, atol=1e-7,
                                    rtol=1e-5)


@pytest.mark.parametrize('gamma', GAMMAS)
def test_hard_targets_give_the_focal_loss(gamma):
    x, y = _elements(1)
    hard = (y > 0.5).double()
    _close(quality_focal_loss(x, hard, gamma).numpy(), (2 * focal_loss(x, hard, alpha=0.5, gamma=gamma)).numpy(), 1e-13)
    zeros = torch.zeros_like(x)
    for alpha in (0.75, 0.3):
        _close(varifocal_loss(x, zeros, alpha, gamma).numpy(), focal_loss(x, zeros, alpha=1 - alpha, gamma=gamma).numpy(), 1e-13)
    # with y = 0 the quality focal loss is sigmoid^gamma softplus: focal_plain's form with weight 1
    _close(quality_focal_loss(x, zeros, gamma).numpy(), (torch.sigmoid(x) ** gamma * torch.nn.functional.softplus(x, threshold=1e9)).numpy(),
           1e-13)


def test_box_quality_is_the_box_loss():
    g = torch.Generator().manual_seed(5)
    sizes = torch.rand(6, 2, generator=g) * 300 + 20
    for dtype in (torch.float32, torch.float64):
        target = (torch.randn(2, 6, 4, 3, 5, generator=g) * 0.3).to(dtype)
        pred = target + (torch.randn(2, 6, 4, 3, 5, generator=g) * 0.4).to(dtype)
        pred[0, :, 2] = 5.0                                   # beyond the clip
        pred[1, 0, 0] += 40.0                                 # disjoint boxes: q == 0
        pred[1, 1] = target[1, 1]                             # identical boxes
        q = box_quality(pred, target, sizes.to(dtype))
        assert q.dtype == dtype and q.shape == (2, 6, 3, 5)
        assert torch.equal(q, 1 - box_iou_loss(pred, target, sizes.to(dtype), 'iou'))
        # in [0, 1] up to the rounding of inter / union (identical boxes: a few ulp of the dtype either side of 1); not clamped, so
        # that it stays the box loss's own number
        ulp = 2.0 ** (-23 if dtype == torch.float32 else -52)
        assert float(q.min()) >= 0 and float(q.max()) <= 1 + 8 * ulp and bool((q[1, 0] == 0).all())
        assert float((1 - q[1, 1]).abs().max()) <= 1e-6
        if dtype == torch.float64:
            _close(q.numpy(), ref.box_quality(pred.numpy(), target.numpy(), sizes.numpy()))
    pred = torch.zeros(1, 2, 4, 1, 1)
    pred[0, 1, 3] = float('nan')
    q = box_quality(pred, torch.zeros(1, 2, 4, 1, 1), torch.tensor([[8.0, 8.0], [16.0, 8.0]])).reshape(2)
    assert math.isnan(float(q[1])) and float(q[0]) == pytest.approx(1.0, abs=1e-6)


def test_quality_target():
    depth = torch.tensor([-1.0, 0.0, 1.0, 3.0, 2.0, 4.0], dtype=torch.float64).view(1, 6, 1, 1, 1)
    q = torch.tensor([0.9, 0.8, 0.7, 0.6, 0.0, 0.5], dtype=torch.float64).view(1, 6, 1, 1)
    y = quality_target(depth, q, 3)
    assert y.shape == (1, 6, 3, 1, 1)
    want = [[0, 0, 0], [0, 0, 0], [0.7, 0, 0], [0, 0, 0.6], [0, 0.0, 0], [0, 0, 0]]      # depth 4: no such class
    assert torch.equal(y.view(6, 3), torch.tensor(want, dtype=torch.float64))
    assert np.array_equal(ref.quality_target(depth.numpy(), q.numpy(), 3).reshape(6, 3), np.array(want, dtype=np.float64))


def test_varifocal_branches():
    x = torch.tensor([-2.0, 0.5, 3.0], dtype=torch.float64)
    zero = torch.zeros(3, dtype=torch.float64)
    # a foreground element whose predicted box misses its target (q == 0) takes the negative branch ...
    _close(varifocal_loss(x, zero, 0.75, 2.0).numpy(), (0.75 * torch.sigmoid(x) ** 2 * torch.nn.functional.softplus(x)).numpy(), 1e-15)
    assert float(varifocal_loss(x, zero, 0.75, 2.0).min()) > 1e-3
    # ... the smallest positive quality the positive one: y (sp - y x) -> 0 with y, while the negative term does not
    tiny = torch.full((3,), 1e-30, dtype=torch.float64)
    assert float(varifocal_loss(x, tiny, 0.75, 2.0).max()) <= 1e-29
    # a NaN quality reaches the loss in both kinds
    nan = torch.full((3,), float('nan'), dtype=torch.float64)
    assert bool(torch.isnan(varifocal_loss(x, nan)).all()) and bool(torch.isnan(quality_focal_loss(x, nan)).all())
    assert np.isnan(ref.vfl(x.numpy(), nan.numpy())[0]).all() and np.isnan(ref.qfl(x.numpy(), nan.numpy())[0]).all()


def test_level_restatement_masks_ignored_anchors():
    """tests/quality_loss_ref.py:level against the torch functions composed as Model's eager path composes them."""
    g = torch.Generator().manual_seed(9)
    b, a, c, h, w = 2, 3, 5, 4, 3
    depth = torch.randint(-1, c + 1, (b, a, 1, h, w), generator=g).double()
    logits = torch.randn(b, a * c, h, w, generator=g, dtype=torch.float64) * 3
    logits.view(b, a, c, h, w)[(depth < 0).expand(b, a, c, h, w)] = float('nan')          # ignored: whatever the logit
    box_target = torch.randn(b, a, 4, h, w, generator=g, dtype=torch.float64) * 0.3
    deltas = (box_target + torch.randn(b, a, 4, h, w, generator=g, dtype=torch.float64) * 0.3).reshape(b, a * 4, h, w)
    sizes = torch.tensor([[32.0, 32.0], [45.0, 23.0], [23.0, 45.0]], dtype=torch.float64)
    for kind, fn in (('qfl', lambda x, y: quality_focal_loss(x, y, 1.5)), ('vfl', lambda x, y: varifocal_loss(x, y, 0.6, 1.5))):
        xg = logits.clone().requires_grad_(True)
        y = quality_target(depth, box_quality(deltas.view(b, a, 4, h, w), box_target, sizes), c)
        per = fn(xg.view(b, a, c, h, w), y)
        total = torch.where((depth >= 0).expand_as(per), per, torch.zeros((), dtype=torch.float64)).sum()
        total.backward()
        want_sum, want_fg, want_grad = ref.level(logits.numpy(), deltas.numpy(), box_target.numpy(), depth.numpy(), sizes.numpy(), kind, 0.6, 1.5)
        assert math.isfinite(want_sum) and want_fg == float((depth > 0).sum())
        assert abs(float(total.detach()) - want_sum) <= 1e-12 * abs(want_sum)
        _close(torch.nan_to_num(xg.grad, nan=0.0).numpy(), want_grad)      # (autograd multiplies the NaN of an ignored logit by 0)
        assert not want_grad[np.broadcast_to((depth < 0).numpy(), (b, a, c, h, w)).reshape(want_grad.shape)].any()


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
    box_heads = [b + 0.1 * torch.randn(b.shape, generator=g) for b in box_heads]
    return model, images, targets, cls_heads, box_heads


def _composed_default(model, images, targets, cls_heads, box_heads):
    """model.py's eager loss as it was before the option existed."""
    from odtk.loss import smooth_l1_loss
    cls_total, box_total, foreground = 0.0, 0.0, 0.0
    for cls_head, box_head in zip(cls_heads, box_heads):
        stride = images.shape[-1] / cls_head.shape[-1]
        cls_target, box_target, depth = model._extract_targets(targets, stride, cls_head.shape[-2:])
        foreground = foreground + (depth > 0).sum().float().clamp(min=1)
        cls_loss = focal_loss(cls_head.view_as(cls_target).float(), cls_target, 0.25, 2)
        cls_total = cls_total + (cls_loss * (depth >= 0).expand_as(cls_target).float()).sum()
        box_loss = smooth_l1_loss(box_head.view_as(box_target).float(), box_target, 0.11)
        box_total = box_total + (box_loss * (depth > 0).expand_as(box_target).float()).sum()
    return cls_total / foreground, box_total / foreground


def test_model_default_is_unchanged_on_the_cpu():
    model, images, targets, cls_heads, box_heads = _model_batch()
    assert model.cls_loss == 'focal'
    before = _composed_default(model, images, targets, cls_heads, box_heads)
    for value in (None, 'focal'):                                   # never set; set to the default
        if value is not None:
            model.cls_loss = value
        got = model._compute_loss(images, cls_heads, box_heads, targets)
        assert torch.equal(got[0], before[0]) and torch.equal(got[1], before[1])


@pytest.mark.parametrize('assigner', ('iou', 'atss'))
@pytest.mark.parametrize('kind', CLS_LOSS_KINDS)
def test_model_loss_on_the_cpu(kind, assigner):
    model, images, targets, cls_heads, box_heads = _model_batch()
    model.assigner = assigner
    focal = model._compute_loss(images, cls_heads, box_heads, targets)
    model.cls_loss = kind
    cls_in = [c.clone().requires_grad_(True) for c in cls_heads]
    box_in = [b.clone().requires_grad_(True) for b in box_heads]
    cls_loss, box_loss = model._compute_loss(images, cls_in, box_in, targets)
    assert math.isfinite(float(cls_loss.detach())) and float(cls_loss.detach()) > 0 and float(cls_loss.detach()) != float(focal[0])
    assert torch.equal(box_loss.detach(), focal[1])                 # the box loss does not move
    # the classification loss alone: the class heads get a gradient, the box heads nothing (q is a constant)
    cls_loss.backward()
    assert all(c.grad is not None and bool(torch.isfinite(c.grad).all()) for c in cls_in) and any(float(c.grad.abs().max()) > 0 for c in cls_in)
    assert all(b.grad is None or not b.grad.any() for b in box_in)
    if assigner == 'iou':
        # against the numpy restatement, level by level
        total, fg = 0.0, 0.0
        for cls_head, box_head in zip(cls_heads, box_heads):
            stride = images.shape[-1] / cls_head.shape[-1]
            _, box_target, depth = model._extract_targets(targets, stride, cls_head.shape[-2:])
            s, f, _ = ref.level(cls_head.numpy(), box_head.numpy(), box_target.numpy(), depth.numpy(),
                                anchor_wh(model.level_anchors(stride)).numpy(), kind)
            total, fg = total + s, fg + max(f, 1.0)
        assert fg >= 3 and abs(float(cls_loss.detach()) - total / fg) <= 1e-5 * total / fg        # float32 arithmetic against float64
    for also in ('giou', 'smooth_l1'):
        model.box_loss = also
        both = model._compute_loss(images, cls_heads, box_heads, targets)
        assert torch.equal(both[0], cls_loss.detach()) and math.isfinite(float(both[1]))


def test_model_refusals():
    model, images, targets, cls_heads, box_heads = _model_batch()
    for bad in ('gfl', 'QFL', None, 1):
        model.cls_loss = bad
        with pytest.raises(ValueError, match='cls_loss'):
            model._compute_loss(images, cls_heads, box_heads, targets)
    model.cls_loss = 'qfl'
    model.rotated_bbox = True
    with pytest.raises(ValueError, match='rotated'):
        model._compute_loss(images, cls_heads, box_heads, targets)


def test_checkpoints_do_not_carry_the_option(tmp_path):
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=3)
    plain, soft = str(tmp_path / 'plain.pth'), str(tmp_path / 'qfl.pth')
    model.save({'path': plain})
    model.cls_loss = 'qfl'
    model.save({'path': soft})
    a, b = torch.load(plain, map_location='cpu'), torch.load(soft, map_location='cpu')
    assert a.keys() == b.keys() and a['state_dict'].keys() == b['state_dict'].keys()
    assert not any('cls_loss' in k for k in list(b) + list(b['state_dict']))
    assert Model.load(soft)[0].cls_loss == 'focal'


# ---------------------------------------------------------------------------------------------------------------- command line
def test_command_line_flag():
    base = ['train', 'm.pth', '--annotations', 'a.json']
    plain = cli.parse(base)
    assert not hasattr(plain, 'cls_loss')
    for kind in ('focal', 'qfl', 'vfl'):
        args = cli.parse(base + ['--cls-loss', kind])
        assert args.cls_loss == kind
        assert {k: v for k, v in vars(args).items() if k != 'cls_loss'} == vars(plain)      # nothing else in the namespace moves
    args = cli.parse(base + ['--cls-loss', 'qfl', '--box-loss', 'giou', '--assigner', 'atss'])
    assert (args.cls_loss, args.box_loss, args.assigner) == ('qfl', 'giou', 'atss')
    assert cli.parse(base + ['--cls-loss', 'focal', '--rotated-bbox']).cls_loss == 'focal'
    for refused in (base + ['--cls-loss', 'qfl', '--rotated-bbox'], base + ['--cls-loss', 'vfl', '--rotated-bbox'],
                    base + ['--cls-loss', 'gfl'], base + ['--cls-loss'], ['infer', 'm.pth', '--cls-loss', 'qfl']):
        with pytest.raises(SystemExit):
            cli.parse(refused)
    text = [spec['help'] for name, spec in cli.TRAIN_FLAGS if name == '--cls-loss'][0]
    assert 'checkpoint' in text and 'resum' in text
    assert '--cls-loss' in cli.__doc__


# ---------------------------------------------------------------------------------------------------------------- C ABI, host side
SIZES = ((40, 56), (1, 3))
# fp32 forward: 2 * 9 * 80 * 40 * 56 / 4 = 806400 vectors -> 788 workgroups of 256 lanes x 2 vectors x 2 trips, + 2 for the 1080
# vectors of the 1 x 3 level; 16 bytes each, rounded up to 256
NEED = 12800


def _levels(sizes=SIZES, **fields):
    levels = (_C.LossLevel * len(sizes))()
    for lv, (h, w) in zip(levels, sizes):
        lv.cls = lv.box = lv.depth = lv.box_target = lv.dcls = 1 << 20          # never dereferenced: every call here is refused
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
    assert {'odtk_quality_loss_levels_forward', 'odtk_quality_loss_levels_backward'} <= set(_C.exported_symbols())
    assert lib.odtk_abi_struct_size(3) == ctypes.sizeof(_C.LossLevel) == 64       # the level descriptor is reused unchanged
    tables, keep = _tables()
    buf = ctypes.create_string_buffer(NEED + 16)
    ws = (ctypes.addressof(buf) + 15) & ~15

    def forward(n_levels=2, lv=None, tab=tables, batch=2, a=9, c=80, dtype=_C.F32, kind=_C.CLS_LOSS_QFL, alpha=0.75, gamma=2.0,
                sums=1 << 20, ws=None, size=0):
        return lib.odtk_quality_loss_levels_forward(n_levels, _levels() if lv is None else lv, tab, batch, a, c, dtype, kind, alpha, gamma,
                                                    sums, ws, size, None)

    def backward(n_levels=2, lv=None, tab=tables, batch=2, a=9, c=80, dtype=_C.F32, kind=_C.CLS_LOSS_QFL, alpha=0.75, gamma=2.0,
                 grads=1 << 20):
        return lib.odtk_quality_loss_levels_backward(n_levels, _levels() if lv is None else lv, tab, batch, a, c, dtype, kind, alpha, gamma,
                                                     grads, None)

    # the two-phase query: a NULL workspace answers the bytes needed and looks at no data pointer
    assert forward() == NEED
    assert forward(sums=None, lv=_levels(cls=None, box=None, depth=None, box_target=None, dcls=None)) == NEED
    assert forward(batch=1, a=1, c=3, tab=_tables(2, 1)[0]) == 256                 # 2 + 1 workgroups
    for dtype in (_C.F32, _C.BF16, _C.F16):
        for kind in (_C.CLS_LOSS_QFL, _C.CLS_LOSS_VFL):
            assert forward(dtype=dtype, kind=kind, gamma=1.0, alpha=0.0) > 0
    inf, nan = float('inf'), float('nan')
    shared = [dict(n_levels=0), dict(n_levels=_C.MAX_LEVELS + 1), dict(a=0), dict(a=_C.MAX_ANCHORS + 1), dict(batch=0), dict(c=0), dict(c=-3),
              dict(kind=0), dict(kind=3), dict(kind=-1), dict(gamma=0.5), dict(gamma=0.0), dict(gamma=-2.0), dict(gamma=inf), dict(gamma=nan),
              dict(alpha=-0.25), dict(alpha=inf), dict(alpha=-inf), dict(alpha=nan),
              dict(lv=ctypes.POINTER(_C.LossLevel)()), dict(tab=ctypes.POINTER(_C._fp)()),
              dict(lv=_levels(height=0)), dict(lv=_levels(width=-1)), dict(lv=_levels(channels_last=2)),
              dict(lv=_levels(((40, 56), (1024, 2048))), c=128),                             # 2 * 9 * 128 * H * W >= 2^32
              dict(lv=_levels(((40, 56), (8192, 4096))), c=1),                               # 2 * 9 * 4 * H * W >= 2^31: the box side
              dict(tab=(_C._fp * 2)(ctypes.cast(keep[0], _C._fp), _C._fp())),                # a level without an anchor table
              dict(tab=_tables(last=(0.0, 0.0, inf, 1.0))[0]), dict(tab=_tables(last=(0.0, 5.0, 5.0, 3.0))[0])]
    for bad in shared:
        assert forward(**bad) == _C.ERR_INVALID, bad                # already the query refuses these
        assert forward(ws=ws, size=NEED, **bad) == _C.ERR_INVALID, bad
        assert backward(**bad) == _C.ERR_INVALID, bad
    for call in (forward, lambda **kw: forward(ws=ws, size=NEED, **kw), backward):
        assert call(dtype=3) == _C.ERR_UNSUPPORTED and call(dtype=-1) == _C.ERR_UNSUPPORTED
    # with a workspace: the data pointers, the workspace itself
    for field in ('cls', 'box', 'depth', 'box_target'):
        assert forward(ws=ws, size=NEED, lv=_levels(**{field: None})) == _C.ERR_INVALID, field
        assert backward(lv=_levels(**{field: None})) == _C.ERR_INVALID, field
    assert backward(lv=_levels(dcls=None)) == _C.ERR_INVALID
    assert forward(ws=ws, size=NEED, sums=None) == _C.ERR_INVALID
    assert forward(ws=ws, size=NEED - 1) == _C.ERR_WORKSPACE and forward(ws=ws, size=0) == _C.ERR_WORKSPACE
    assert forward(ws=ws + 4, size=NEED) == _C.ERR_INVALID and forward(ws=ws, size=NEED, sums=(1 << 20) + 4) == _C.ERR_INVALID
    # the logits are read and the gradients written as 16-byte vectors
    assert forward(ws=ws, size=NEED, lv=_levels(cls=(1 << 20) + 8)) == _C.ERR_INVALID
    assert forward(ws=ws, size=NEED, dtype=_C.BF16, lv=_levels(cls=(1 << 20) + 8)) == _C.ERR_INVALID
    assert backward(lv=_levels(dcls=(1 << 20) + 8)) == _C.ERR_INVALID
    assert backward(grads=(1 << 20) + 2) == _C.ERR_INVALID
    # dbox is ignored: d(deltas) is never written
    assert forward(lv=_levels(dbox=None)) == NEED


def test_binding_refuses_cpu_tensors_and_bad_arguments():
    cls, head, depth, target = torch.zeros(1, 3, 2, 2), torch.zeros(1, 4, 2, 2), torch.zeros(1, 1, 1, 2, 2), torch.zeros(1, 1, 4, 2, 2)
    anchors = [torch.tensor([[0.0, 0.0, 7.0, 7.0]])]
    with pytest.raises(RuntimeError, match='GPU'):
        _C.quality_loss_levels_forward([cls], [head], [depth], [target], anchors, 'qfl')
    with pytest.raises(RuntimeError, match='kind'):
        _C.quality_loss_levels_forward([cls], [head], [depth], [target], anchors, 'focal')
    for alpha, gamma in ((0.75, 0.5), (0.75, float('nan')), (-1.0, 2.0), (float('inf'), 2.0)):
        with pytest.raises(RuntimeError, match='gamma'):
            _C.quality_loss_levels_forward([cls], [head], [depth], [target], anchors, 'vfl', alpha, gamma)
    with pytest.raises(RuntimeError, match='levels'):
        _C.quality_loss_levels_forward([cls] * 7, [head] * 7, [depth] * 7, [target] * 7, anchors * 7, 'qfl')
    with pytest.raises(RuntimeError, match='levels'):
        _C.quality_loss_levels_backward([cls, cls], [head], [depth], [target], anchors, 'qfl', 0.75, 2.0, None)
