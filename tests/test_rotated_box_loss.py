"""ProbIoU / KLD box losses of rotated boxes (odtk/loss.py:rotated_box_loss, include/odtk_hip.h: odtk_rotated_box_loss_levels_*;
`Model.box_loss`, `odtk train --rotated-bbox --box-loss probiou|kld`) without a GPU: the covariance convention against the corners
of `rotate_boxes`, the limits of the definition in float64, numerical differentiation, `Model` and command-line validation in
both directions of the rotated requirement, and the host-side argument checks of the two entry points (they precede anything that
touches HIP)."""
import ctypes
import math

import pytest
import torch

from odtk import _C, _C_ext, box
from odtk import main as cli
from odtk.loss import BBOX_XFORM_CLIP, ROTATED_BOX_LOSS_KINDS, anchor_wh, rotated_box_loss
from odtk.model import Model

KINDS = ('probiou', 'kld')
F64 = torch.float64


def _one(p, t, size, kind, dtype=F64):
    """One anchor of size `size`: deltas p, t (6 numbers each) -> the loss as a 0-d tensor."""
    pred = torch.tensor(p, dtype=dtype).view(1, 1, 6, 1, 1)
    target = torch.tensor(t, dtype=dtype).view(1, 1, 6, 1, 1)
    return rotated_box_loss(pred, target, torch.tensor([size], dtype=dtype), kind).reshape(())


def _grad(p, t, size, kind):
    pred = torch.tensor(p, dtype=F64).view(1, 1, 6, 1, 1).requires_grad_(True)
    rotated_box_loss(pred, torch.tensor(t, dtype=F64).view(1, 1, 6, 1, 1), torch.tensor([size], dtype=F64), kind).sum().backward()
    return pred.grad.view(6)


def _deltas(cx, cy, w, h, theta, size):
    """The deltas that decode to a w x h box turned by theta whose centre is (cx, cy) from the anchor centre."""
    return [cx / size[0], cy / size[1], math.log(w / size[0]), math.log(h / size[1]), math.sin(theta), math.cos(theta)]


def test_kinds():
    assert ROTATED_BOX_LOSS_KINDS == KINDS
    with pytest.raises(ValueError, match='kind'):
        _one([0.0] * 5 + [1.0], [0.0] * 5 + [1.0], (2.0, 2.0), 'gwd')


@pytest.mark.parametrize('theta', [0.0, 0.3, -0.3, math.pi / 4, -1.1, 2.5, -math.pi / 2])
@pytest.mark.parametrize('w,h', [(40.0, 10.0), (10.0, 40.0), (12.0, 31.0)])
def test_covariance_convention(theta, w, h):
    """Three times the covariance [[a, c], [c, b]] of the definition = the covariance of the four corners `rotate_boxes` returns
    for the same box: pins the sign of c (the cross term multiplies it with the centre offsets)."""
    quad = box.rotate_boxes(torch.tensor([[100.0, 50.0, w, h, theta]], dtype=F64))[1].view(4, 2)
    centred = quad - quad.mean(0)
    corners = centred.t() @ centred / 4
    cc, ss, sc = math.cos(theta) ** 2, math.sin(theta) ** 2, math.sin(theta) * math.cos(theta)
    a, b, c = (w * w * cc + h * h * ss) / 12, (w * w * ss + h * h * cc) / 12, -(w * w - h * h) * sc / 12
    want = torch.tensor([[a, c], [c, b]], dtype=F64) * 3
    torch.testing.assert_close(corners, want, rtol=1e-10, atol=1e-9)
    # ... and the definition uses that sign: against an isotropic target (c2 = 0) probiou's cross term is -2 c1 dx dy, so of two
    # offsets of the same length the one along the Gaussian's long diagonal (dx dy of the sign of c1) costs less
    if abs(c) > 1e-9:
        size = (16.0, 16.0)
        side = math.sqrt(w * h)
        t_plus = _deltas(0.0, 0.0, side, side, 0.0, size)
        along = float(_one(_deltas(3.0, 3.0, w, h, theta, size), t_plus, size, 'probiou'))
        across = float(_one(_deltas(3.0, -3.0, w, h, theta, size), t_plus, size, 'probiou'))
        assert (along < across) == (c > 0)                  # an offset along the long diagonal of the Gaussian costs less


@pytest.mark.parametrize('kind', KINDS)
def test_identical_boxes(kind):
    want = math.sqrt(1e-7) if kind == 'probiou' else 0.0
    for deltas, size in (([0.0, 0.0, 0.0, 0.0, 0.0, 1.0], (2.0, 2.0)), ([0.3, -0.2, 0.4, -0.7, math.sin(0.6), math.cos(0.6)], (45.25, 22.63)),
                         ([-1.5, 2.0, 1.2, 0.1, math.sin(-2.0), math.cos(-2.0)], (812.0, 406.0))):
        got = float(_one(deltas, deltas, size, kind))
        # float64 rounding: BD and K are O(1) differences of O(1) terms, so ~1e-15 absolute; through sqrt(1e-7 + x) that is
        # ~1e-15 / (2 sqrt(1e-7)) = 2e-12, through the kld's x / (1 + x) 1e-15
        assert abs(got - want) <= 1e-11, (got, want)
        assert float(_grad(deltas, deltas, size, kind).abs().max()) <= 1e-6          # the minimum


@pytest.mark.parametrize('kind', KINDS)
def test_square_box_has_no_angle_gradient(kind):
    size = (24.0, 24.0)                                       # a square anchor and dw = dh: w = h to the last bit
    t = _deltas(2.0, -1.0, 26.0, 13.0, 0.4, size)
    p = [3.5 / 24, 1.0 / 24, 0.25, 0.25, math.sin(-0.7), math.cos(-0.7)]
    g = _grad(p, t, size, kind)
    assert float(g[:4].abs().min()) > 1e-3
    # 0 up to the 1e-12 in q: cc + ss = 1 - 1e-12 / q, so a = b = w^2 (cc + ss) / 12 keeps a radial dependence of relative size
    # 1e-12 on the pair (|(p4, p5)| = 1 here); the gradient by the sizes is O(1), a factor 10 covers the chain in between
    assert float(g[4:].abs().max()) <= 1e-11 * float(g[:4].abs().max())
    # the loss itself does not see the angle either
    turned = p[:4] + [math.sin(1.9), math.cos(1.9)]
    assert float(_one(turned, t, size, kind)) == pytest.approx(float(_one(p, t, size, kind)), rel=1e-12)
    # ... while an elongated one has a tangential gradient: orthogonal to (p4, p5)
    p = _deltas(3.5, 1.0, 40.0, 12.0, -0.7, size)
    g = _grad(p, t, size, kind)
    assert float(g[4:].abs().max()) > 1e-3
    assert abs(float(g[4] * p[4] + g[5] * p[5])) <= 1e-10 * float(g[4:].abs().max())


@pytest.mark.parametrize('kind', KINDS)
def test_direction_norm_changes_nothing(kind):
    size = (22.6, 45.3)
    t = _deltas(1.0, 2.0, 30.0, 50.0, 0.9, size)
    p = _deltas(-2.0, 4.0, 36.0, 41.0, 0.5, size)
    base, g1 = float(_one(p, t, size, kind)), _grad(p, t, size, kind)
    # up to the 1e-12 in q: at length 0.1 it changes cc, ss and sc by 1e-12 / 0.01 = 1e-10 relative, and the loss and its
    # gradient are O(1)-conditioned in them -- a factor 100 for the chain gives the bar 1e-8
    for scale in (0.1, 10.0):
        scaled = p[:4] + [p[4] * scale, p[5] * scale]
        assert float(_one(scaled, t, size, kind)) == pytest.approx(base, rel=1e-8)
        g = _grad(scaled, t, size, kind)
        torch.testing.assert_close(g[:4], g1[:4], rtol=1e-8, atol=1e-12)
        torch.testing.assert_close(g[4:] * scale, g1[4:], rtol=1e-8, atol=1e-10)    # tangential, ~ 1 / sqrt(q)
    # the target's length does not matter either
    assert float(_one(p, t[:4] + [3 * t[4], 3 * t[5]], size, kind)) == pytest.approx(base, rel=1e-10)


@pytest.mark.parametrize('kind', KINDS)
def test_common_turn_changes_nothing(kind):
    """Both boxes turned by the same angle about the prediction's centre: the same loss.  In the convention of `rotate_boxes` a turn
    by phi maps an offset d to [[cos, sin], [-sin, cos]] d."""
    size = (31.0, 17.0)
    pc, tc = (4.0, -2.0), (7.5, 3.0)
    pw, ph, pa, tw, th, ta = 48.0, 15.0, 0.35, 40.0, 19.0, -0.2
    base = float(_one(_deltas(*pc, pw, ph, pa, size), _deltas(*tc, tw, th, ta, size), size, kind))
    assert base > 0.05
    for phi in (0.4, -1.3, math.pi / 2, 3.0):
        ox, oy = tc[0] - pc[0], tc[1] - pc[1]
        moved = (pc[0] + math.cos(phi) * ox + math.sin(phi) * oy, pc[1] - math.sin(phi) * ox + math.cos(phi) * oy)
        got = float(_one(_deltas(*pc, pw, ph, pa + phi, size), _deltas(*moved, tw, th, ta + phi, size), size, kind))
        assert got == pytest.approx(base, rel=1e-10), phi
    # a common shift changes nothing either
    got = float(_one(_deltas(pc[0] + 9, pc[1] - 5, pw, ph, pa, size), _deltas(tc[0] + 9, tc[1] - 5, tw, th, ta, size), size, kind))
    assert got == pytest.approx(base, rel=1e-10)


@pytest.mark.parametrize('kind', KINDS)
def test_clip_of_the_predicted_sizes(kind):
    size = (32.0, 64.0)
    t = [0.1, -0.1, 0.2, 0.3, math.sin(0.3), math.cos(0.3)]
    at = _one([0.2, 0.1, BBOX_XFORM_CLIP, 0.1, 0.5, 0.8], t, size, kind)
    for beyond in (BBOX_XFORM_CLIP + 0.5, 50.0):
        p = [0.2, 0.1, beyond, 0.1, 0.5, 0.8]
        assert float(_one(p, t, size, kind)) == float(at)
        g = _grad(p, t, size, kind)
        assert float(g[2]) == 0.0 and float(g[3]) != 0.0 and float(g[0]) != 0.0       # (ph is below the clip)
    p = [0.2, 0.1, 4.5, 7.0, 0.5, 0.8]
    g = _grad(p, t, size, kind)
    assert float(g[2]) == 0.0 and float(g[3]) == 0.0
    # the targets are not clipped
    assert float(_one(t, t[:2] + [BBOX_XFORM_CLIP + 0.5] + t[3:], size, kind)) != float(_one(t, t[:2] + [BBOX_XFORM_CLIP] + t[3:], size, kind))


def test_clamps_of_the_distance():
    size = (16.0, 16.0)
    t = _deltas(0.0, 0.0, 16.0, 16.0, 0.0, size)
    far = _deltas(4000.0, 0.0, 16.0, 16.0, 0.0, size)          # BD = 4000^2 / (8 * 16^2 / 12) >> 100
    assert float(_one(far, t, size, 'probiou')) == pytest.approx(math.sqrt(1 + 1e-7), rel=1e-12)
    assert float(_grad(far, t, size, 'probiou').abs().max()) == 0.0
    assert 0.9 < float(_one(far, t, size, 'kld')) < 1.0 and float(_grad(far, t, size, 'kld')[0]) > 0       # the kld has no upper clamp


def test_nan_propagates():
    sizes = anchor_wh(torch.tensor([[-12.0, -12.0, 19.0, 19.0], [-7.3, -18.6, 14.3, 25.6]]))
    unit = torch.zeros(1, 2, 6, 1, 1)
    unit[:, :, 5] = 1.0
    for k in range(6):
        pred = unit.clone()
        pred[0, 1, k] = float('nan')
        for kind in KINDS:
            out = rotated_box_loss(pred, unit, sizes, kind).reshape(2)
            assert math.isnan(float(out[1])) and not math.isnan(float(out[0])), (k, kind)
    out = rotated_box_loss(torch.zeros(2, 2, 6, 3, 5) + unit, torch.zeros(2, 2, 6, 3, 5) + unit, sizes, 'kld')
    assert out.shape == (2, 2, 3, 5) and out.dtype == torch.float32


def _random_anchors(seed, n, noise):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.rand(n, 2, generator=g, dtype=F64) * 790 + 22
    target = torch.randn(1, n, 6, 1, 1, generator=g, dtype=F64) * torch.tensor([0.3, 0.3, 0.2, 0.2, 0, 0], dtype=F64).view(1, 1, 6, 1, 1)
    theta = torch.rand(n, generator=g, dtype=F64) * 2 * math.pi - math.pi
    target[0, :, 4, 0, 0], target[0, :, 5, 0, 0] = theta.sin(), theta.cos()
    pred = target + torch.randn(1, n, 6, 1, 1, generator=g, dtype=F64) * noise
    return pred, target, sizes


@pytest.mark.parametrize('kind', KINDS)
def test_gradcheck(kind):
    for seed, noise in ((1, 0.15), (2, 0.6)):
        pred, target, sizes = _random_anchors(seed, 20, noise)
        assert torch.autograd.gradcheck(lambda p: rotated_box_loss(p, target, sizes, kind), (pred.requires_grad_(True),), eps=1e-6,
                                        atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize('kind', KINDS)
def test_float32_follows_float64(kind):
    """The arithmetic the kernel uses, in torch: float32 sums within 1e-6 relative of float64 at the GPU tests' noise (their bar)."""
    pred, target, sizes = _random_anchors(7, 2000, 0.15)
    pred, target, sizes = pred.float().double(), target.float().double(), sizes.float().double()
    want = float(rotated_box_loss(pred, target, sizes, kind).sum())
    got = float(rotated_box_loss(pred.float(), target.float(), sizes.float(), kind).double().sum())
    assert abs(got - want) <= 1e-6 * abs(want)


# ---------------------------------------------------------------------------------------------------------------- Model
def _heads_of(model):
    torch.manual_seed(0)
    images = torch.randn(1, 3, 64, 64)
    targets = torch.tensor([[[8.0, 8.0, 32.0, 20.0, 0.3, 0.0]]])
    with torch.no_grad():
        cls_heads, box_heads = model.heads(images)
    return images, targets, cls_heads, box_heads


def test_model_validation_in_both_directions():
    torch.manual_seed(0)
    axis = Model('ResNet18FPN', classes=3).train()
    images, targets, cls_heads, box_heads = _heads_of(axis)
    for kind in KINDS:
        axis.box_loss = kind
        with pytest.raises(ValueError, match='rotated'):
            axis._compute_loss(images, cls_heads, box_heads, targets[:, :, [0, 1, 2, 3, 5]])
    rotated = Model('ResNet18FPN', classes=3, rotated_bbox=True).train()
    assert rotated.num_anchors == 27 and (rotated.box_loss, rotated.box_loss_weight) == ('smooth_l1', 1.0)
    images, targets, cls_heads, box_heads = _heads_of(rotated)
    for kind in ('iou', 'giou', 'diou'):
        rotated.box_loss = kind
        with pytest.raises(ValueError, match='not available for rotated'):
            rotated._compute_loss(images, cls_heads, box_heads, targets)
    rotated.box_loss = 'gwd'
    with pytest.raises(ValueError, match='box_loss'):
        rotated._compute_loss(images, cls_heads, box_heads, targets)
    for kind in KINDS:
        rotated.box_loss = kind
        for weight in (0.0, -1.0, float('inf'), float('nan'), None, 'heavy', True):
            rotated.box_loss_weight = weight
            with pytest.raises(ValueError, match='box_loss_weight'):
                rotated._compute_loss(images, cls_heads, box_heads, targets)
        rotated.box_loss_weight = 2.0
        # accepted: validation passes and the rotated target assignment is reached, which has no CPU form
        with pytest.raises(RuntimeError, match='GPU'):
            rotated._compute_loss(images, cls_heads, box_heads, targets)


def test_checkpoints_do_not_carry_the_option(tmp_path):
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=3, rotated_bbox=True)
    plain, kld = str(tmp_path / 'plain.pth'), str(tmp_path / 'kld.pth')
    model.save({'path': plain})
    model.box_loss, model.box_loss_weight = 'kld', 2.0
    model.save({'path': kld})
    a, b = torch.load(plain, map_location='cpu'), torch.load(kld, map_location='cpu')
    assert a.keys() == b.keys() and a['state_dict'].keys() == b['state_dict'].keys()
    assert not any('box_loss' in k for k in list(b) + list(b['state_dict']))
    loaded = Model.load(kld)[0]
    assert loaded.rotated_bbox and (loaded.box_loss, loaded.box_loss_weight) == ('smooth_l1', 1.0)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_command_line_flags():
    base = ['train', 'm.pth', '--annotations', 'a.json']
    plain = cli.parse(base + ['--rotated-bbox'])
    for kind in KINDS:
        args = cli.parse(base + ['--rotated-bbox', '--box-loss', kind])
        assert args.box_loss == kind and args.rotated_bbox and not hasattr(args, 'box_loss_weight')
        assert {k: v for k, v in vars(args).items() if k != 'box_loss'} == vars(plain)      # nothing else in the namespace moves
        args = cli.parse(base + ['--box-loss', kind, '--box-loss-weight', '2.5', '--rotated-bbox'])
        assert (args.box_loss, args.box_loss_weight) == (kind, 2.5)
        for refused in (base + ['--box-loss', kind], base + ['--box-loss', kind, '--box-loss-weight', '2'],
                        base + ['--rotated-bbox', '--box-loss', kind, '--box-loss-weight', '0'],
                        base + ['--rotated-bbox', '--box-loss', kind, '--box-loss-weight', 'nan'],
                        ['infer', 'm.pth', '--rotated-bbox', '--box-loss', kind]):
            with pytest.raises(SystemExit):
                cli.parse(refused)
    for kind in ('iou', 'giou', 'diou'):                             # the existing refusal stays
        with pytest.raises(SystemExit):
            cli.parse(base + ['--rotated-bbox', '--box-loss', kind])
        assert cli.parse(base + ['--box-loss', kind]).box_loss == kind
    with pytest.raises(SystemExit):
        cli.parse(base + ['--rotated-bbox', '--box-loss', 'gwd'])
    text = [spec['help'] for name, spec in cli.TRAIN_FLAGS if name == '--box-loss'][0]
    assert 'probiou' in text and 'kld' in text and '--rotated-bbox' in text
    assert 'probiou' in cli.__doc__ and 'kld' in cli.__doc__


def test_parser_error_names_the_rotated_requirement(capsys):
    with pytest.raises(SystemExit):
        cli.parse(['train', 'm.pth', '--annotations', 'a.json', '--box-loss', 'probiou'])
    assert '--rotated-bbox' in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------------------- C ABI, host side
SIZES = ((40, 56), (1, 3))
NEED = 7680                      # 2 * 27 * 2240 / 256 = 472.5 -> 473 + 1 workgroups, 16 bytes each, rounded up to 256


def _levels(sizes=SIZES, **fields):
    levels = (_C.LossLevel * len(sizes))()
    for lv, (h, w) in zip(levels, sizes):
        lv.box = lv.depth = lv.box_target = lv.dbox = 1 << 20                 # never dereferenced: every call here is refused
        lv.height, lv.width, lv.channels_last = h, w, 1
    for name, value in fields.items():
        setattr(levels[len(sizes) - 1], name, value)
    return levels


def _tables(n=2, a=27, box_=(-12.0, -12.0, 19.0, 19.0), last=None):
    keep = [(ctypes.c_float * (4 * a))(*(list(box_) * a)) for _ in range(n)]
    if last is not None:
        keep[-1][4 * (a - 1):4 * a] = last
    return (_C._fp * n)(*[ctypes.cast(k, _C._fp) for k in keep]), keep


def test_both_bindings_expose_the_entry_points():
    assert {'odtk_rotated_box_loss_levels_forward', 'odtk_rotated_box_loss_levels_backward'} <= set(_C.exported_symbols())
    assert (_C.ROTATED_BOX_LOSS_PROBIOU, _C.ROTATED_BOX_LOSS_KLD) == (1, 2)
    assert _C.ROTATED_BOX_LOSS_KINDS == {'probiou': 1, 'kld': 2}
    for module in (_C, _C_ext):
        assert callable(module.rotated_box_loss_levels_forward) and callable(module.rotated_box_loss_levels_backward)
    head, depth, target = torch.zeros(1, 6, 2, 2), torch.zeros(1, 1, 1, 2, 2), torch.zeros(1, 1, 6, 2, 2)
    tensors = [torch.tensor([[0.0, 0.0, 7.0, 7.0]])]
    for module, anchors in ((_C, tensors), (_C_ext, [[0.0, 0.0, 7.0, 7.0]])):
        with pytest.raises(RuntimeError, match='GPU'):
            module.rotated_box_loss_levels_forward([head], [depth], [target], anchors, 'kld')
        with pytest.raises(RuntimeError, match='kind'):
            module.rotated_box_loss_levels_forward([head], [depth], [target], anchors, 'giou')
        with pytest.raises(RuntimeError, match='levels'):
            module.rotated_box_loss_levels_forward([head] * 7, [depth] * 7, [target] * 7, anchors * 7, 'kld')
        with pytest.raises(RuntimeError, match='levels'):
            module.rotated_box_loss_levels_backward([head], [depth], [target], [], 'probiou', None)


def test_abi_validates_before_touching_the_device():
    lib = _C.library()
    assert lib.odtk_abi_struct_size(3) == ctypes.sizeof(_C.LossLevel) == 64       # the level descriptor is reused unchanged
    tables, keep = _tables()
    buf = ctypes.create_string_buffer(NEED + 16)
    ws = (ctypes.addressof(buf) + 15) & ~15

    def forward(n_levels=2, lv=None, tab=tables, batch=2, a=27, dtype=_C.F32, kind=_C.ROTATED_BOX_LOSS_KLD, sums=1 << 20, ws=None, size=0):
        return lib.odtk_rotated_box_loss_levels_forward(n_levels, _levels() if lv is None else lv, tab, batch, a, dtype, kind, sums, ws, size, None)

    def backward(n_levels=2, lv=None, tab=tables, batch=2, a=27, dtype=_C.F32, kind=_C.ROTATED_BOX_LOSS_KLD, grads=1 << 20):
        return lib.odtk_rotated_box_loss_levels_backward(n_levels, _levels() if lv is None else lv, tab, batch, a, dtype, kind, grads, None)

    # the two-phase query: a NULL workspace answers the bytes needed and looks at no data pointer
    assert forward() == NEED and forward(sums=None, lv=_levels(box=None, depth=None, box_target=None)) == NEED
    assert forward(n_levels=1) == 7680 and forward(batch=1, a=1, tab=_tables(2, 1)[0]) == 256     # 473; 9 + 1 workgroups
    assert forward(a=_C.MAX_ANCHORS, tab=_tables(2, _C.MAX_ANCHORS)[0]) > NEED                   # 27 and up to 32 anchors fit
    for dtype in (_C.F32, _C.BF16, _C.F16):
        for kind in (1, 2):
            assert forward(dtype=dtype, kind=kind) == NEED
    shared = [dict(n_levels=0), dict(n_levels=_C.MAX_LEVELS + 1), dict(a=0), dict(a=_C.MAX_ANCHORS + 1), dict(batch=0), dict(batch=-2),
              dict(kind=0), dict(kind=3), dict(kind=-1), dict(lv=ctypes.POINTER(_C.LossLevel)()), dict(tab=ctypes.POINTER(_C._fp)()),
              dict(lv=_levels(height=0)), dict(lv=_levels(width=-1)), dict(lv=_levels(channels_last=2)),
              dict(lv=_levels(((40, 56), (4096, 1619)))),                                   # 2 * 27 * 6 * H * W >= 2^31
              dict(tab=(_C._fp * 2)(ctypes.cast(keep[0], _C._fp), _C._fp()))]              # a level without an anchor table
    assert 2 * 27 * 6 * 4096 * 1619 >= 1 << 31 > 2 * 27 * 6 * 4096 * 1618
    assert forward(lv=_levels(((40, 56), (4096, 1618)))) > 0                              # ... and just below the limit is taken
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
    # channels_last heads are read and written as three pieces per cell: 8 bytes each for fp32, 4 for the 16-bit types
    assert forward(ws=ws, size=NEED, lv=_levels(box=(1 << 20) + 4)) == _C.ERR_INVALID
    assert forward(ws=ws, size=NEED, dtype=_C.BF16, lv=_levels(box=(1 << 20) + 2)) == _C.ERR_INVALID
    assert backward(lv=_levels(dbox=(1 << 20) + 4)) == _C.ERR_INVALID
    assert backward(dtype=_C.F16, lv=_levels(dbox=(1 << 20) + 2)) == _C.ERR_INVALID
    assert backward(grads=(1 << 20) + 2) == _C.ERR_INVALID
    # NCHW: the element's own alignment
    nchw = dict(channels_last=0)
    assert forward(ws=ws, size=NEED, lv=_levels(box=(1 << 20) + 2, **nchw)) == _C.ERR_INVALID
    assert forward(ws=ws, size=NEED, dtype=_C.F16, lv=_levels(box=(1 << 20) + 1, **nchw)) == _C.ERR_INVALID
