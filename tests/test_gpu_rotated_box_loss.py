"""The ProbIoU / KLD box-loss kernels of rotated boxes (csrc/rotated_box_loss.hpp, odtk_rotated_box_loss_levels_*) on the GPU against
their definition: `odtk.loss.rotated_box_loss` evaluated in float64 on the CPU, masked by `depth > 0` and summed per level, with
autograd for the gradients.  Bars (those of tests/test_gpu_loss.py): sums within 1e-6 relative of float64, the foreground count
exact, gradients within 1e-5 of the level's largest reference gradient for fp32 heads, 1e-2 for bf16 and 2e-3 for fp16 (one
rounding of the stored gradient); for 16-bit heads the reference reads the rounded head values.  Prediction noise is the siblings'
sigma = 0.15, so no anchor sits on the sqrt(1e-7) knee of probiou (that limit is tested in float64 in tests/test_rotated_box_loss.py).
Every check prints, next to the kernel's figure, the error of the SAME torch definition evaluated in float32 on the CPU at the same
inputs.  That float32 evaluation does NOT hold the fp32 gradient bar for probiou (measured: worst 1.5e-4 of a largest gradient of
4.14 = 3.7e-5, on real assignments with 27 anchors; its gradient goes with BD^-1/2 and BD is a small difference of O(1) terms), and
a kernel in float32 per anchor measured the same 1.5e-4 -- and 1.6e-4 against the torch evaluation's 5.7e-6 on a level of three
cells, so no multiple of the float32 yardstick bounds a single anchor.  The kernels therefore evaluate each anchor in double; the
project's bars hold as they stand (measured with the double kernels: see DESIGN.md) and no bar was re-derived.  Shapes: those of tests/test_gpu_box_iou_loss.py;
27 anchors (3 ratios x 3 scales x 3 angles), 3 and 1."""
import math

import pytest
import torch

from odtk import _C, box
from odtk import loss as L
from odtk.model import Model

pytestmark = pytest.mark.gpu

KINDS = ('probiou', 'kld')
RATIOS, SCALES, ANGLES = [1.0, 2.0, 0.5], [4 * 2 ** (i / 3) for i in range(3)], [-math.pi / 6, 0.0, math.pi / 6]
LEVELS3 = [(8, 40, 56), (32, 7, 10), (128, 1, 3)]
LEVELS5 = [(8, 40, 56), (16, 20, 28), (32, 7, 10), (64, 4, 5), (128, 1, 3)]
LEVELS6 = LEVELS5 + [(256, 1, 1)]
FORMATS = [(torch.float32, False), (torch.float32, True), (torch.bfloat16, True), (torch.float16, True), (torch.float16, False)]
FORMAT_IDS = ['fp32-nchw', 'fp32-nhwc', 'bf16-nhwc', 'fp16-nhwc', 'fp16-nchw']
GRAD_TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 2e-3}
# (x, y, w, h, theta, class) in a 448 x 320 image: boxes near the anchors of strides 8, 16 and 32, two that only the large anchors of
# the small levels cover, angles of both signs, aspect ratios up to 1:4
BOXES = [[[24.0, 40.0, 33.0, 31.0, 0.15, 0.0], [200.0, 100.0, 45.0, 23.0, -0.5, 2.0], [100.0, 60.0, 130.0, 126.0, -0.2, 1.0],
          [-70.0, -190.0, 520.0, 500.0, 0.1, 1.0], [300.0, 200.0, 64.0, 66.0, 0.45, 0.0], [150.0, 220.0, 80.0, 20.0, 0.6, 2.0]],
         [[310.0, 150.0, 23.0, 45.0, 0.5, 1.0], [30.0, 30.0, 200.0, 100.0, -0.45, 2.0], [64.0, -192.0, 512.0, 512.0, -0.1, 0.0],
          [120.0, 200.0, 40.0, 41.0, -0.3, 2.0], [250.0, 40.0, 16.0, 64.0, -0.55, 1.0], [-1.0, -1.0, -1.0, -1.0, 0.0, -1.0]]]


def _anchors(levels, a):
    """Per level the (axis, rotated) pair of `generate_anchors_rotated`."""
    if a == 27:
        return [box.generate_anchors_rotated(s, RATIOS, SCALES, ANGLES) for s, _, _ in levels]
    return [box.generate_anchors_rotated(s, [1.0], [4.0], ANGLES if a == 3 else [0.0]) for s, _, _ in levels]


def _axis(anchors):
    return [pair[0] for pair in anchors]


def _snap(levels, a):
    """Real rotated assignments (about 1 % foreground) -> (anchor pairs, box_targets, depths)."""
    anchors = _anchors(levels, a)
    assert anchors[0][0].shape == (a, 4)
    targets = torch.tensor(BOXES, device='cuda')
    _, box_targets, depths = box.snap_to_anchors_rotated_levels(targets, [(h, w) for _, h, w in levels], [s for s, _, _ in levels], anchors, 3,
                                                                [0.4, 0.5], want_cls_target=False)
    return anchors, box_targets, depths


def _synthetic(levels, a, depth_of, seed=5):
    """Targets N(0, 0.3) with unit directions everywhere and a depth map per level from depth_of(level index, shape)."""
    g = torch.Generator().manual_seed(seed)
    anchors = _anchors(levels, a)
    box_targets = []
    for _, h, w in levels:
        bt = torch.randn(2, a, 6, h, w, generator=g) * 0.3
        theta = torch.rand(2, a, h, w, generator=g) * 2 * math.pi - math.pi
        bt[:, :, 4], bt[:, :, 5] = theta.sin(), theta.cos()
        box_targets.append(bt.cuda())
    depths = [depth_of(i, (2, a, 1, h, w)).cuda() for i, (_, h, w) in enumerate(levels)]
    return anchors, box_targets, depths


def _heads(box_targets, seed, dtype, channels_last, sigma=0.15, mutate=None):
    """Predictions = box_target + N(0, sigma), in the head's dtype and layout (the `_heads_like` recipe of tests/test_gpu_loss.py)."""
    g = torch.Generator().manual_seed(seed)
    heads = []
    for bt in box_targets:
        b, a, nb, h, w = bt.shape
        head = bt.cpu().reshape(b, a * nb, h, w) + torch.randn(b, a * nb, h, w, generator=g) * sigma
        if mutate is not None:
            head = mutate(head.reshape(b, a, nb, h, w)).reshape(b, a * nb, h, w)
        head = head.cuda().to(dtype)
        if channels_last:
            head = head.contiguous(memory_format=torch.channels_last)
        heads.append(head.requires_grad_(True))
    return heads


def _reference(heads, box_targets, depths, anchors, kind, upstream):
    """float64 on the CPU -> (sums [L], foreground [L], gradients per level in float64, shaped like the heads) and the yardstick
    per level: (|sum - float64 sum|, max |gradient - float64 gradient|) of the same torch definition in float32 at these inputs."""
    sums, fg, grads, yard = [], [], [], []
    for head, bt, depth, an, g in zip(heads, box_targets, depths, _axis(anchors), upstream):
        pred = head.detach().float().cpu().contiguous().double().requires_grad_(True)        # 16-bit heads: the rounded values
        mask = depth.cpu()[:, :, 0] > 0
        per_anchor = L.rotated_box_loss(pred.view(bt.shape), bt.cpu().double(), L.anchor_wh(an).double(), kind)
        total = (per_anchor * mask.double()).sum()
        (total * g).backward()
        single = pred.detach().float().requires_grad_(True)
        per_anchor32 = L.rotated_box_loss(single.view(bt.shape), bt.cpu(), L.anchor_wh(an), kind)
        total32 = torch.where(mask, per_anchor32, torch.zeros_like(per_anchor32)).double().sum()
        (total32 * g).backward()
        yard.append((abs(float(total32.detach()) - float(total.detach())), float((single.grad.double() - pred.grad).abs().max())))
        sums.append(float(total.detach()))
        fg.append(float(mask.sum()))
        grads.append(pred.grad)
    return sums, fg, grads, yard


def _bars(ref_sum, grad_scale, yard, dtype):
    """(bar of a level's sum, bar of its gradient): the project's own.  The float32 yardstick is printed next to them and bounds
    nothing: the kernels evaluate each anchor in double."""
    return 1e-6 * abs(ref_sum), GRAD_TOL[dtype] * grad_scale


def _poison(heads):
    """Leave NaNs in the blocks the allocator hands out next: a gradient element the kernel does not write shows."""
    junk = [torch.full_like(h, float('nan')) for h in heads]
    del junk


def _check(anchors, box_targets, depths, kind, dtype, channels_last, seed=3, sigma=0.15, heads=None, want_fg=None):
    heads = heads if heads is not None else _heads(box_targets, seed, dtype, channels_last, sigma)
    n = len(heads)
    axis = _axis(anchors)
    upstream = [(-1.9, 0.37, 1.0, -0.6, 2.25, 0.11)[i % 6] for i in range(n)]
    ref_sums, ref_fg, ref_grads, yard = _reference(heads, box_targets, depths, anchors, kind, upstream)
    got = _C.rotated_box_loss_levels_forward([h.detach() for h in heads], depths, box_targets, axis, kind)
    again = _C.rotated_box_loss_levels_forward([h.detach() for h in heads], depths, box_targets, axis, kind)
    assert got.dtype == torch.float64 and got.shape == (n, 2)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))         # the same bits on every run
    got = got.cpu()
    for l in range(n):
        bar = _bars(ref_sums[l], 0.0, yard[l], dtype)[0]
        print('level %d %s: sum %.9g want %.9g (off %.3g, float32 torch off %.3g, project bar %.3g, bar %.3g), fg %g'
              % (l, kind, float(got[l, 0]), ref_sums[l], abs(float(got[l, 0]) - ref_sums[l]), yard[l][0], 1e-6 * abs(ref_sums[l]), bar,
                 float(got[l, 1])))
        assert float(got[l, 1]) == ref_fg[l]
        assert abs(float(got[l, 0]) - ref_sums[l]) <= bar, (l, float(got[l, 0]), ref_sums[l])
    if want_fg is not None:
        assert [int(f) for f in ref_fg] == want_fg
    # the autograd form: the same sums (as float32), gradients in the heads' dtype and layout; it takes the anchor pairs as they are
    sums, fg = L.fused_pyramid_rotated_box_loss(heads, depths, box_targets, anchors, kind)
    assert torch.equal(sums.cpu(), got[:, 0].float()) and torch.equal(fg.cpu(), got[:, 1].float()) and not fg.requires_grad
    _poison(heads)
    (sums * torch.tensor(upstream, device='cuda')).sum().backward()
    for l, (head, ref, depth) in enumerate(zip(heads, ref_grads, depths)):
        mine = head.grad
        assert mine.dtype == dtype and mine.stride() == head.stride() and mine.shape == head.shape
        scale = float(ref.abs().max())
        worst = float((mine.float().cpu().double() - ref).abs().max())
        bar = _bars(0.0, scale, yard[l], dtype)[1]
        print('level %d %s: gradient worst %.3g of %.3g (float32 torch worst %.3g, project bar %.3g, bar %.3g)'
              % (l, kind, worst, scale, yard[l][1], GRAD_TOL[dtype] * scale, bar))
        assert worst <= bar, (l, worst, scale)                                   # scale == 0 (no foreground anchor): exactly zero
        # +0, bit for bit, wherever the anchor is not foreground
        b, a, _, h, w = depth.shape
        off = (depth <= 0).expand(b, a, 6, h, w).reshape(b, a * 6, h, w)
        bits = mine.view(torch.int32 if dtype == torch.float32 else torch.int16)
        assert int((bits[off] != 0).sum()) == 0
    return heads, got


@pytest.mark.parametrize('a', [27, 3, 1])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype,channels_last', FORMATS, ids=FORMAT_IDS)
def test_against_float64_on_assigned_targets(dtype, channels_last, kind, a):
    anchors, box_targets, depths = _snap(LEVELS3, a)
    fg = sum(int((d > 0).sum()) for d in depths)
    print('foreground anchors:', fg)
    assert fg >= 3
    _check(anchors, box_targets, depths, kind, dtype, channels_last)


@pytest.mark.parametrize('levels', [LEVELS3[:1], LEVELS5, LEVELS6], ids=['1-level', '5-levels', '6-levels'])
def test_level_counts(levels):
    assert len(LEVELS6) == _C.MAX_LEVELS
    anchors, box_targets, depths = _snap(levels, 27)
    _check(anchors, box_targets, depths, 'probiou', torch.float32, True)
    _check(anchors, box_targets, depths, 'kld', torch.float16, False)


def test_seven_levels_are_split_into_groups():
    """More levels than one launch takes: `fused_pyramid_rotated_box_loss` splits them; the loss has no state across levels."""
    levels = LEVELS6 + [(8, 40, 56)]
    assert len(levels) > _C.MAX_LEVELS
    anchors, box_targets, depths = _synthetic(levels, 27, lambda i, shape: (torch.arange(shape[0] * shape[1] * shape[3] * shape[4])
                                                                            .reshape(shape) % 5 == 0).float())
    for kind, (dtype, channels_last) in zip(KINDS, (FORMATS[1], FORMATS[2])):
        heads = _heads(box_targets, 8, dtype, channels_last)
        upstream = [0.5, -2.0, 1.25, 1.0, -0.3, 0.8, 1.7]
        ref_sums, ref_fg, ref_grads, yard = _reference(heads, box_targets, depths, anchors, kind, upstream)
        sums, fg = L.fused_pyramid_rotated_box_loss(heads, depths, box_targets, anchors, kind)
        assert sums.shape == (7,) and fg.shape == (7,) and [float(f) for f in fg.cpu()] == ref_fg and ref_fg[6] > 0
        first = _C.rotated_box_loss_levels_forward([h.detach() for h in heads[:6]], depths[:6], box_targets[:6], _axis(anchors)[:6], kind)
        last = _C.rotated_box_loss_levels_forward([h.detach() for h in heads[6:]], depths[6:], box_targets[6:], _axis(anchors)[6:], kind)
        assert torch.equal(sums, torch.cat([first[:, 0], last[:, 0]]).float())
        for l in range(7):
            assert abs(float(torch.cat([first, last])[l, 0]) - ref_sums[l]) <= _bars(ref_sums[l], 0.0, yard[l], dtype)[0]
        with pytest.raises(RuntimeError, match='levels'):
            _C.rotated_box_loss_levels_forward([h.detach() for h in heads], depths, box_targets, _axis(anchors), kind)
        (sums * torch.tensor(upstream, device='cuda')).sum().backward()
        for head, ref, y in zip(heads, ref_grads, yard):
            assert float((head.grad.float().cpu().double() - ref).abs().max()) <= _bars(0.0, float(ref.abs().max()), y, dtype)[1]


@pytest.mark.parametrize('dtype,channels_last', FORMATS, ids=FORMAT_IDS)
def test_synthetic_depth_maps(dtype, channels_last):
    # no foreground at all: sums exactly 0, gradients all-zero bits (ignored and background cells both)
    def nothing(i, shape):
        return -(torch.arange(shape[0] * shape[1] * shape[3] * shape[4]).reshape(shape) % 2).float()
    anchors, box_targets, depths = _synthetic(LEVELS3, 27, nothing)
    heads, got = _check(anchors, box_targets, depths, 'probiou', dtype, channels_last, want_fg=[0, 0, 0])
    assert int((got.view(torch.int64) != 0).sum()) == 0
    for head in heads:
        assert int((head.grad.view(torch.int32 if dtype == torch.float32 else torch.int16) != 0).sum()) == 0
    # every anchor foreground
    anchors, box_targets, depths = _synthetic(LEVELS3, 3, lambda i, shape: torch.full(shape, 2.0))
    for kind in KINDS:
        _check(anchors, box_targets, depths, kind, dtype, channels_last, want_fg=[2 * 3 * 40 * 56, 2 * 3 * 70, 2 * 3 * 3])
    # a single foreground anchor, in the last cell of the last level
    def last(i, shape):
        depth = torch.zeros(shape)
        if i == len(LEVELS3) - 1:
            depth.view(-1)[-1] = 3.0
        return depth
    for a, kind in ((27, 'kld'), (1, 'probiou')):
        anchors, box_targets, depths = _synthetic(LEVELS3, a, last)
        _check(anchors, box_targets, depths, kind, dtype, channels_last, want_fg=[0, 0, 1])


@pytest.mark.parametrize('kind', KINDS)
def test_predicted_sizes_beyond_the_clip(kind):
    def beyond(pred):                                        # [B, A, 6, H, W]: some dw and dh well beyond log(1000 / 16) = 4.135
        pred[:, ::2, 2, :, ::3] = 4.75
        pred[:, 1::3, 3, ::2] = 9.0
        return pred
    anchors, box_targets, depths = _synthetic(LEVELS3[1:], 27, lambda i, shape: (torch.arange(shape[0] * shape[1] * shape[3] * shape[4])
                                                                                  .reshape(shape) % 3 == 0).float())
    for dtype, channels_last in ((torch.float32, False), (torch.bfloat16, True)):
        heads = _heads(box_targets, 4, dtype, channels_last, mutate=beyond)
        heads, _ = _check(anchors, box_targets, depths, kind, dtype, channels_last, heads=heads)
        clipped = 0
        for head, depth in zip(heads, depths):               # no gradient through a clipped size
            b, a, _, h, w = depth.shape
            sizes = head.detach().reshape(b, a, 6, h, w)[:, :, 2:4]
            hit = (sizes > 4.5) & (depth > 0)
            clipped += int(hit.sum())
            assert int((head.grad.reshape(b, a, 6, h, w)[:, :, 2:4][hit] != 0).sum()) == 0
        assert clipped > 10


@pytest.mark.parametrize('dtype,channels_last', FORMATS, ids=FORMAT_IDS)
def test_cells_that_are_not_foreground_are_never_read(dtype, channels_last):
    anchors, box_targets, depths = _snap(LEVELS3, 27)
    axis = _axis(anchors)
    clean = _heads(box_targets, 9, dtype, channels_last)
    dirty = []
    for head, depth in zip(clean, depths):
        b, a, _, h, w = depth.shape
        off = (depth <= 0).expand(b, a, 6, h, w).reshape(b, a * 6, h, w)
        d = torch.where(off, torch.full_like(head.detach(), float('nan')), head.detach())
        if channels_last:
            d = d.contiguous(memory_format=torch.channels_last)
        assert d.stride() == head.stride() and int(torch.isnan(d).sum()) > 0
        dirty.append(d.requires_grad_(True))
    out = []
    for heads in (clean, dirty):
        sums = _C.rotated_box_loss_levels_forward([h.detach() for h in heads], depths, box_targets, axis, 'kld')
        s, _ = L.fused_pyramid_rotated_box_loss(heads, depths, box_targets, axis, 'kld')
        (s * torch.tensor([0.5, -2.0, 1.25], device='cuda')).sum().backward()
        out.append((sums, [h.grad for h in heads]))
    assert torch.equal(out[0][0].view(torch.int64), out[1][0].view(torch.int64)) and bool(torch.isfinite(out[1][0]).all())
    for mine, ref in zip(out[1][1], out[0][1]):
        assert bool(torch.isfinite(mine).all()) and torch.equal(mine, ref)
    # ... while a NaN delta at a foreground anchor reaches its level's sum, and only that one, whichever of the six it is
    level = max(range(3), key=lambda l: int((depths[l] > 0).sum()))
    b, a, _, h, w = depths[level].shape
    for k, kind in zip(range(6), KINDS * 3):
        only = torch.zeros(1, 1, 6, 1, 1, dtype=torch.bool, device='cuda')
        only[0, 0, k] = True
        hit = ((depths[level] > 0) & only).reshape(b, a * 6, h, w)
        bad = [t.detach().clone() for t in clean]
        bad[level] = torch.where(hit, torch.full_like(bad[level], float('nan')), bad[level])
        if channels_last:
            bad[level] = bad[level].contiguous(memory_format=torch.channels_last)
        sums = _C.rotated_box_loss_levels_forward(bad, depths, box_targets, axis, kind).cpu()
        assert [bool(torch.isnan(sums[l, 0])) for l in range(3)] == [l == level for l in range(3)], (k, kind)
        assert torch.equal(sums[:, 1], out[0][0].cpu()[:, 1])


def test_no_upstream_gradient_gives_zeros():
    anchors, box_targets, depths = _synthetic(LEVELS3, 3, lambda i, shape: torch.full(shape, 1.0))
    for dtype, channels_last in FORMATS:
        heads = [h.detach() for h in _heads(box_targets, 2, dtype, channels_last)]
        _poison(heads)
        grads = _C.rotated_box_loss_levels_backward(heads, depths, box_targets, _axis(anchors), 'probiou', None)
        for g, head in zip(grads, heads):
            assert g.dtype == dtype and g.stride() == head.stride()
            assert int((g.view(torch.int32 if dtype == torch.float32 else torch.int16) != 0).sum()) == 0


def test_exotic_strides_and_argument_checks():
    anchors, box_targets, depths = _snap(LEVELS3, 27)
    axis = _axis(anchors)
    heads = _heads(box_targets, 6, torch.float32, False)
    want = _C.rotated_box_loss_levels_forward([h.detach() for h in heads], depths, box_targets, axis, 'kld')
    sliced = [torch.cat([h.detach(), h.detach()], 3)[:, :, :, :h.shape[3]] for h in heads]          # neither NCHW nor channels_last
    assert not sliced[0].is_contiguous()
    sums, _ = L.fused_pyramid_rotated_box_loss(sliced, depths, box_targets, axis, 'kld')
    assert torch.equal(sums, want[:, 0].float())
    with pytest.raises(RuntimeError, match='dense'):
        _C.rotated_box_loss_levels_forward(sliced, depths, box_targets, axis, 'kld')
    with pytest.raises(ValueError, match='kind'):
        L.fused_pyramid_rotated_box_loss(heads, depths, box_targets, axis, 'giou')
    with pytest.raises(RuntimeError, match='shapes'):
        _C.rotated_box_loss_levels_forward([h.detach() for h in heads], depths[::-1], box_targets, axis, 'kld')
    with pytest.raises(RuntimeError, match='anchor table'):
        _C.rotated_box_loss_levels_forward([h.detach() for h in heads], depths, box_targets, _axis(_anchors(LEVELS3, 1)), 'kld')


def test_compiled_binding_gives_the_same_bits():
    from odtk import _C_ext
    anchors, box_targets, depths = _snap(LEVELS3, 27)
    axis = _axis(anchors)
    tables = [t.reshape(-1).tolist() for t in axis]
    g = torch.tensor([0.5, -2.0, 1.25], device='cuda')
    for kind, (dtype, channels_last) in zip(KINDS, (FORMATS[0], FORMATS[2])):
        heads = [h.detach() for h in _heads(box_targets, 12, dtype, channels_last)]
        a = _C.rotated_box_loss_levels_forward(heads, depths, box_targets, axis, kind)
        b = _C_ext.rotated_box_loss_levels_forward(heads, depths, box_targets, tables, kind)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and float(a[:, 1].sum()) >= 3
        _poison(heads)
        da = _C.rotated_box_loss_levels_backward(heads, depths, box_targets, axis, kind, g)
        db = _C_ext.rotated_box_loss_levels_backward(heads, depths, box_targets, tables, kind, g)
        for x, y, head in zip(da, db, heads):
            assert y.dtype == dtype and y.stride() == head.stride() and torch.equal(x, y) and float(x.float().abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- Model
def _model_and_batch():
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=3, rotated_bbox=True)
    model.initialize(None)
    model = model.cuda().train()
    g = torch.Generator().manual_seed(11)
    images = torch.randn(2, 3, 128, 128, generator=g).cuda()
    targets = torch.tensor([[[8.0, 8.0, 32.0, 32.0, 0.2, 0.0], [60.0, 16.0, 45.0, 23.0, -0.45, 2.0], [20.0, 40.0, 64.0, 66.0, 0.1, 1.0]],
                            [[50.0, 4.0, 32.0, 32.0, -0.15, 1.0], [4.0, 50.0, 23.0, 45.0, 0.5, 0.0], [30.0, 14.0, 90.0, 88.0, -0.3, 2.0]]]).cuda()
    return model, images, targets


def _heads_step(model, images, targets, cls_heads, box_heads):
    """Both losses and their gradient at every box head, from head tensors held fixed."""
    leaves = [b.detach().clone().requires_grad_(True) for b in box_heads]
    cls_loss, box_loss = model._compute_loss(images, [c.detach() for c in cls_heads], leaves, targets)
    box_loss.backward()
    return float(cls_loss.detach()), float(box_loss.detach()), [t.grad for t in leaves]


def _box_truth(model, images, targets, box_heads, kind, weight):
    """`Model._compute_loss`'s box term written out in float64 on the CPU -> (loss, its gradient at every box head)."""
    strides = [images.shape[-1] // b.shape[-1] for b in box_heads]
    anchors = [model.level_anchors(s) for s in strides]
    _, box_targets, depths = box.snap_to_anchors_rotated_levels(targets, [tuple(b.shape[-2:]) for b in box_heads], strides, anchors,
                                                                model.classes, model.anchor_ious, want_cls_target=False)
    leaves = [b.detach().cpu().double().requires_grad_(True) for b in box_heads]
    total, foreground = 0.0, 0.0
    for leaf, bt, depth, (axis, _) in zip(leaves, box_targets, depths, anchors):
        mask = depth.cpu()[:, :, 0] > 0
        total = total + (L.rotated_box_loss(leaf.view(bt.shape), bt.cpu().double(), L.anchor_wh(axis).double(), kind) * mask.double()).sum()
        foreground += max(float(mask.sum()), 1.0)
    loss = weight * total / foreground
    loss.backward()
    return float(loss.detach()), [leaf.grad for leaf in leaves]


@pytest.mark.parametrize('kind', KINDS)
def test_model_fused_and_eager_paths_agree(kind):
    model, images, targets = _model_and_batch()
    assert model.num_anchors == 27
    model.box_loss, model.box_loss_weight = kind, 1.5
    with torch.no_grad():
        cls_heads, box_heads = model.heads(images)
    g = torch.Generator().manual_seed(3)
    # head values of a trained-ish net, the assigned targets + N(0, 0.15): the fresh rotated box head predicts the prior bias
    # (-4.6) for all six deltas, boxes so far from their targets that probiou's exp(-BD) has no gradient left in float32
    strides = [images.shape[-1] // b.shape[-1] for b in box_heads]
    _, box_targets, _ = box.snap_to_anchors_rotated_levels(targets, [tuple(b.shape[-2:]) for b in box_heads], strides,
                                                           [model.level_anchors(s) for s in strides], model.classes, model.anchor_ious,
                                                           want_cls_target=False)
    box_heads = [(bt.reshape(b.shape) + 0.15 * torch.randn(b.shape, generator=g).cuda()).contiguous(memory_format=torch.channels_last)
                 for bt, b in zip(box_targets, box_heads)]
    assert model.fused_loss
    fused = _heads_step(model, images, targets, cls_heads, box_heads)
    model.fused_loss = False
    eager = _heads_step(model, images, targets, cls_heads, box_heads)
    truth = _box_truth(model, images, targets, box_heads, kind, 1.5)
    # the focal term is the default path's on both sides: each within 1e-6 of float64 (tests/test_gpu_loss.py), 2e-6 of each other
    print(kind, 'cls loss', fused[0], eager[0])
    assert abs(fused[0] - eager[0]) <= 2e-6 * abs(eager[0]) and eager[0] > 0
    # the box term: both paths against float64.  The fused path at the kernels' bars.  The eager path IS the float32 torch
    # evaluation: a dozen roundings of O(1) terms that cancel leave BD and K ~1e-6 absolute off, L = sqrt(BD) and its gradient
    # ~ BD^-1/2 turn that into 0.5e-6 / BD relative, and at sigma = 0.15 hardly an anchor has BD < 0.005: 1e-4 of the largest
    # gradient, 1e-5 of the loss (a mean over anchors)
    print(kind, 'box loss %.9g eager %.9g float64 %.9g' % (fused[1], eager[1], truth[0]))
    assert abs(fused[1] - truth[0]) <= 1e-6 * truth[0] and abs(eager[1] - truth[0]) <= 1e-5 * truth[0] and truth[0] > 0
    seen = 0
    for mine, ref, want in zip(fused[2], eager[2], truth[1]):
        scale = float(want.abs().max())
        worst = float((mine.cpu().double() - want).abs().max())
        yard = float((ref.cpu().double() - want).abs().max())
        print(kind, 'box head gradient: worst %.3g of %.3g (eager %.3g)' % (worst, scale, yard))
        assert worst <= 1e-5 * scale and yard <= 1e-4 * scale
        seen += scale > 1e-3                                 # (a live gradient, not the tail of a saturated exp)
    assert seen >= 1
    # the weight is a plain factor, and the default is another loss
    model.fused_loss, model.box_loss_weight = True, 3.0
    assert _heads_step(model, images, targets, cls_heads, box_heads)[1] == pytest.approx(2 * fused[1], rel=1e-6)
    model.box_loss, model.box_loss_weight = 'smooth_l1', 1.0
    assert abs(_heads_step(model, images, targets, cls_heads, box_heads)[1] - fused[1] / 1.5) > 1e-3 * fused[1]


@pytest.mark.parametrize('kind', KINDS)
def test_ten_steps_stay_finite(kind):
    model, images, targets = _model_and_batch()
    model.box_loss = kind
    optimizer = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
    losses = []
    for _ in range(10):
        optimizer.zero_grad(set_to_none=True)
        cls_loss, box_loss = model((images, targets))
        (cls_loss + box_loss).backward()
        optimizer.step()
        losses.append((float(cls_loss), float(box_loss)))
    print(kind, losses)
    assert all(math.isfinite(c) and math.isfinite(b) for c, b in losses)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert losses[0][1] > 0
