"""The IoU / GIoU / DIoU box-loss kernels (csrc/box_iou_loss.hpp, odtk_box_iou_loss_levels_*) on the GPU against their definition:
`odtk.loss.box_iou_loss` evaluated in float64 on the CPU, masked by `depth > 0` and summed per level, with autograd for the
gradients.  Bars (those of tests/test_gpu_loss.py): sums within 1e-6 relative of float64, the foreground count exact, gradients
within 1e-5 of the largest reference gradient for fp32 heads, 1e-2 for bf16 and 2e-3 for fp16 (one rounding of the stored
gradient); for 16-bit heads the reference reads the rounded head values.  Shapes: the smallest that reach every path -- a level of
several workgroups with an odd pixel count, one with fewer cells than a wave, one whose rows are no whole vectors; 9 anchors and 1."""
import pytest
import torch

from odtk import _C, box
from odtk import loss as L
from odtk.model import Model

pytestmark = pytest.mark.gpu

KINDS = ('iou', 'giou', 'diou')
RATIOS, SCALES = [1.0, 2.0, 0.5], [4 * 2 ** (i / 3) for i in range(3)]
LEVELS3 = [(8, 40, 56), (32, 7, 10), (128, 1, 3)]
LEVELS5 = [(8, 40, 56), (16, 20, 28), (32, 7, 10), (64, 4, 5), (128, 1, 3)]
LEVELS6 = LEVELS5 + [(256, 1, 1)]
FORMATS = [(torch.float32, False), (torch.float32, True), (torch.bfloat16, True), (torch.float16, True), (torch.float16, False)]
FORMAT_IDS = ['fp32-nchw', 'fp32-nhwc', 'bf16-nhwc', 'fp16-nhwc', 'fp16-nchw']
GRAD_TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 2e-3}
# (x, y, w, h, class) in a 448 x 320 image: boxes near the anchors of strides 8, 16 and 32, and two that only the large anchors of the
# small levels cover (they reach beyond the image, as those anchors do)
BOXES = [[[24.0, 40.0, 33.0, 31.0, 0.0], [200.0, 100.0, 45.0, 23.0, 2.0], [100.0, 60.0, 130.0, 126.0, 1.0], [-70.0, -190.0, 520.0, 500.0, 1.0],
          [300.0, 200.0, 64.0, 66.0, 0.0]],
         [[310.0, 150.0, 23.0, 45.0, 1.0], [30.0, 30.0, 200.0, 100.0, 2.0], [64.0, -192.0, 512.0, 512.0, 0.0], [120.0, 200.0, 40.0, 41.0, 2.0],
          [-1.0, -1.0, -1.0, -1.0, -1.0]]]


def _anchors(levels, a):
    if a == 9:
        return [box.generate_anchors(s, RATIOS, SCALES) for s, _, _ in levels]
    return [box.generate_anchors(s, [1.0], [4.0]) for s, _, _ in levels]


def _snap(levels, a):
    """Realistic targets (about 1 % foreground) from the fixed-IoU rule -> (anchors, box_targets, depths)."""
    anchors = _anchors(levels, a)
    targets = torch.tensor(BOXES, device='cuda')
    _, box_targets, depths = box.snap_to_anchors_levels(targets, [(h, w) for _, h, w in levels], [s for s, _, _ in levels], anchors, 3,
                                                        [0.4, 0.5], want_cls_target=False)
    return anchors, box_targets, depths


def _synthetic(levels, a, depth_of, seed=5):
    """Targets N(0, 0.3) everywhere and a depth map per level from depth_of(level index, shape)."""
    g = torch.Generator().manual_seed(seed)
    anchors = _anchors(levels, a)
    box_targets = [(torch.randn(2, a, 4, h, w, generator=g) * 0.3).cuda() for _, h, w in levels]
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
    """float64 on the CPU -> (sums [L], foreground [L], gradients per level in float64, shaped like the heads)."""
    sums, fg, grads = [], [], []
    for head, bt, depth, an, g in zip(heads, box_targets, depths, anchors, upstream):
        pred = head.detach().float().cpu().contiguous().double().requires_grad_(True)        # 16-bit heads: the rounded values
        mask = depth.cpu()[:, :, 0] > 0
        per_anchor = L.box_iou_loss(pred.view(bt.shape), bt.cpu().double(), L.anchor_wh(an).double(), kind)
        total = (per_anchor * mask.double()).sum()
        (total * g).backward()
        sums.append(float(total.detach()))
        fg.append(float(mask.sum()))
        grads.append(pred.grad)
    return sums, fg, grads


def _poison(heads):
    """Leave NaNs in the blocks the allocator hands out next: a gradient element the kernel does not write shows."""
    junk = [torch.full_like(h, float('nan')) for h in heads]
    del junk


def _check(anchors, box_targets, depths, kind, dtype, channels_last, seed=3, sigma=0.15, heads=None, want_fg=None):
    heads = heads if heads is not None else _heads(box_targets, seed, dtype, channels_last, sigma)
    n = len(heads)
    upstream = [(-1.9, 0.37, 1.0, -0.6, 2.25, 0.11)[i % 6] for i in range(n)]
    ref_sums, ref_fg, ref_grads = _reference(heads, box_targets, depths, anchors, kind, upstream)
    got = _C.box_iou_loss_levels_forward([h.detach() for h in heads], depths, box_targets, anchors, kind)
    again = _C.box_iou_loss_levels_forward([h.detach() for h in heads], depths, box_targets, anchors, kind)
    assert got.dtype == torch.float64 and got.shape == (n, 2)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))         # the same bits on every run
    got = got.cpu()
    for l in range(n):
        print('level %d %s: sum %.9g want %.9g, fg %g' % (l, kind, float(got[l, 0]), ref_sums[l], float(got[l, 1])))
        assert float(got[l, 1]) == ref_fg[l]
        assert abs(float(got[l, 0]) - ref_sums[l]) <= 1e-6 * abs(ref_sums[l]), (l, float(got[l, 0]), ref_sums[l])
    if want_fg is not None:
        assert [int(f) for f in ref_fg] == want_fg
    # the autograd form: the same sums (as float32), gradients in the heads' dtype and layout
    sums, fg = L.fused_pyramid_box_iou_loss(heads, depths, box_targets, anchors, kind)
    assert torch.equal(sums.cpu(), got[:, 0].float()) and torch.equal(fg.cpu(), got[:, 1].float()) and not fg.requires_grad
    _poison(heads)
    (sums * torch.tensor(upstream, device='cuda')).sum().backward()
    for l, (head, ref, depth) in enumerate(zip(heads, ref_grads, depths)):
        mine = head.grad
        assert mine.dtype == dtype and mine.stride() == head.stride() and mine.shape == head.shape
        scale = float(ref.abs().max())
        worst = float((mine.float().cpu().double() - ref).abs().max())
        print('level %d %s: gradient worst %.3g of %.3g' % (l, kind, worst, scale))
        assert worst <= GRAD_TOL[dtype] * scale, (l, worst, scale)               # scale == 0 (no foreground anchor): exactly zero
        # +0, bit for bit, wherever the anchor is not foreground
        b, a, _, h, w = depth.shape
        off = (depth <= 0).expand(b, a, 4, h, w).reshape(b, a * 4, h, w)
        bits = mine.view(torch.int32 if dtype == torch.float32 else torch.int16)
        assert int((bits[off] != 0).sum()) == 0
    return heads, got


@pytest.mark.parametrize('a', [9, 1])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype,channels_last', FORMATS, ids=FORMAT_IDS)
def test_against_float64_on_assigned_targets(dtype, channels_last, kind, a):
    anchors, box_targets, depths = _snap(LEVELS3, a)
    assert sum(int((d > 0).sum()) for d in depths) >= 3
    _check(anchors, box_targets, depths, kind, dtype, channels_last)


@pytest.mark.parametrize('levels', [LEVELS3[:1], LEVELS5, LEVELS6], ids=['1-level', '5-levels', '6-levels'])
def test_level_counts(levels):
    assert len(LEVELS6) == _C.MAX_LEVELS
    anchors, box_targets, depths = _snap(levels, 9)
    _check(anchors, box_targets, depths, 'giou', torch.float32, True)
    _check(anchors, box_targets, depths, 'diou', torch.float16, False)


@pytest.mark.parametrize('dtype,channels_last', FORMATS, ids=FORMAT_IDS)
def test_synthetic_depth_maps(dtype, channels_last):
    # no foreground at all: sums exactly 0, gradients all-zero bits (ignored and background cells both)
    def nothing(i, shape):
        return -(torch.arange(shape[0] * shape[1] * shape[3] * shape[4]).reshape(shape) % 2).float()
    anchors, box_targets, depths = _synthetic(LEVELS3, 9, nothing)
    heads, got = _check(anchors, box_targets, depths, 'giou', dtype, channels_last, want_fg=[0, 0, 0])
    assert int((got.view(torch.int64) != 0).sum()) == 0
    for head in heads:
        assert int((head.grad.view(torch.int32 if dtype == torch.float32 else torch.int16) != 0).sum()) == 0
    # every anchor foreground
    anchors, box_targets, depths = _synthetic(LEVELS3, 9, lambda i, shape: torch.full(shape, 2.0))
    for kind in KINDS:
        _check(anchors, box_targets, depths, kind, dtype, channels_last, want_fg=[2 * 9 * 40 * 56, 2 * 9 * 70, 2 * 9 * 3])
    # a single foreground anchor, in the last cell of the last level
    def last(i, shape):
        depth = torch.zeros(shape)
        if i == len(LEVELS3) - 1:
            depth.view(-1)[-1] = 3.0
        return depth
    for a in (9, 1):
        anchors, box_targets, depths = _synthetic(LEVELS3, a, last)
        _check(anchors, box_targets, depths, 'diou', dtype, channels_last, want_fg=[0, 0, 1])


@pytest.mark.parametrize('kind', KINDS)
def test_predicted_sizes_beyond_the_clip(kind):
    def beyond(pred):                                        # [B, A, 4, H, W]: some dw and dh well beyond log(1000 / 16) = 4.135
        pred[:, ::2, 2, :, ::3] = 4.75
        pred[:, 1::3, 3, ::2] = 9.0
        return pred
    anchors, box_targets, depths = _synthetic(LEVELS3[1:], 9, lambda i, shape: (torch.arange(shape[0] * shape[1] * shape[3] * shape[4])
                                                                                 .reshape(shape) % 3 == 0).float())
    for dtype, channels_last in ((torch.float32, False), (torch.bfloat16, True)):
        heads = _heads(box_targets, 4, dtype, channels_last, mutate=beyond)
        heads, _ = _check(anchors, box_targets, depths, kind, dtype, channels_last, heads=heads)
        clipped = 0
        for head, depth in zip(heads, depths):               # no gradient through a clipped size
            b, a, _, h, w = depth.shape
            sizes = head.detach().reshape(b, a, 4, h, w)[:, :, 2:]
            hit = (sizes > 4.5) & (depth > 0)
            clipped += int(hit.sum())
            assert int((head.grad.reshape(b, a, 4, h, w)[:, :, 2:][hit] != 0).sum()) == 0
        assert clipped > 10


@pytest.mark.parametrize('dtype,channels_last', FORMATS, ids=FORMAT_IDS)
def test_cells_that_are_not_foreground_are_never_read(dtype, channels_last):
    anchors, box_targets, depths = _snap(LEVELS3, 9)
    clean = _heads(box_targets, 9, dtype, channels_last)
    dirty = []
    for head, depth in zip(clean, depths):
        b, a, _, h, w = depth.shape
        off = (depth <= 0).expand(b, a, 4, h, w).reshape(b, a * 4, h, w)
        d = torch.where(off, torch.full_like(head.detach(), float('nan')), head.detach())
        if channels_last:
            d = d.contiguous(memory_format=torch.channels_last)
        assert d.stride() == head.stride() and int(torch.isnan(d).sum()) > 0
        dirty.append(d.requires_grad_(True))
    out = []
    for heads in (clean, dirty):
        sums = _C.box_iou_loss_levels_forward([h.detach() for h in heads], depths, box_targets, anchors, 'giou')
        s, _ = L.fused_pyramid_box_iou_loss(heads, depths, box_targets, anchors, 'giou')
        (s * torch.tensor([0.5, -2.0, 1.25], device='cuda')).sum().backward()
        out.append((sums, [h.grad for h in heads]))
    assert torch.equal(out[0][0].view(torch.int64), out[1][0].view(torch.int64)) and bool(torch.isfinite(out[1][0]).all())
    for mine, ref in zip(out[1][1], out[0][1]):
        assert bool(torch.isfinite(mine).all()) and torch.equal(mine, ref)
    # ... while a NaN delta at a foreground anchor reaches its level's sum, and only that one
    level = max(range(3), key=lambda l: int((depths[l] > 0).sum()))
    b, a, _, h, w = depths[level].shape
    hit = (depths[level] > 0).expand(b, a, 4, h, w).reshape(b, a * 4, h, w)
    bad = [h.detach().clone() for h in clean]
    bad[level] = torch.where(hit, torch.full_like(bad[level], float('nan')), bad[level])
    if channels_last:
        bad[level] = bad[level].contiguous(memory_format=torch.channels_last)
    sums = _C.box_iou_loss_levels_forward(bad, depths, box_targets, anchors, 'iou').cpu()
    assert [bool(torch.isnan(sums[l, 0])) for l in range(3)] == [l == level for l in range(3)]
    assert torch.equal(sums[:, 1], out[0][0].cpu()[:, 1])


def test_no_upstream_gradient_gives_zeros():
    anchors, box_targets, depths = _synthetic(LEVELS3, 9, lambda i, shape: torch.full(shape, 1.0))
    for dtype, channels_last in FORMATS:
        heads = [h.detach() for h in _heads(box_targets, 2, dtype, channels_last)]
        _poison(heads)
        grads = _C.box_iou_loss_levels_backward(heads, depths, box_targets, anchors, 'giou', None)
        for g, head in zip(grads, heads):
            assert g.dtype == dtype and g.stride() == head.stride()
            assert int((g.view(torch.int32 if dtype == torch.float32 else torch.int16) != 0).sum()) == 0


def test_exotic_strides_and_argument_checks():
    anchors, box_targets, depths = _snap(LEVELS3, 9)
    heads = _heads(box_targets, 6, torch.float32, False)
    want = _C.box_iou_loss_levels_forward([h.detach() for h in heads], depths, box_targets, anchors, 'diou')
    sliced = [torch.cat([h.detach(), h.detach()], 3)[:, :, :, :h.shape[3]] for h in heads]          # neither NCHW nor channels_last
    assert not sliced[0].is_contiguous()
    sums, _ = L.fused_pyramid_box_iou_loss(sliced, depths, box_targets, anchors, 'diou')
    assert torch.equal(sums, want[:, 0].float())
    with pytest.raises(RuntimeError, match='dense'):
        _C.box_iou_loss_levels_forward(sliced, depths, box_targets, anchors, 'diou')
    with pytest.raises(ValueError, match='kind'):
        L.fused_pyramid_box_iou_loss(heads, depths, box_targets, anchors, 'ciou')
    with pytest.raises(RuntimeError, match='shapes'):
        _C.box_iou_loss_levels_forward([h.detach() for h in heads], depths[::-1], box_targets, anchors, 'iou')
    with pytest.raises(RuntimeError, match='anchor table'):
        _C.box_iou_loss_levels_forward([h.detach() for h in heads], depths, box_targets, _anchors(LEVELS3, 1), 'iou')


# ---------------------------------------------------------------------------------------------------------------- Model
def _model_and_batch():
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=3)
    model.initialize(None)
    model = model.cuda().train()
    g = torch.Generator().manual_seed(11)
    images = torch.randn(2, 3, 64, 96, generator=g).cuda()
    targets = torch.tensor([[[8.0, 8.0, 32.0, 32.0, 0.0], [40.0, 16.0, 45.0, 23.0, 2.0], [20.0, 20.0, 40.0, 40.0, 1.0]],
                            [[50.0, 4.0, 32.0, 32.0, 1.0], [4.0, 10.0, 23.0, 45.0, 0.0], [30.0, 14.0, 40.0, 40.0, 2.0]]]).cuda()
    return model, images, targets


def _step(model, images, targets):
    model.zero_grad(set_to_none=True)
    cls_loss, box_loss = model((images, targets))
    (cls_loss + box_loss).backward()
    return cls_loss.detach().clone(), box_loss.detach().clone(), model.box_head[-1].weight.grad.detach().clone()


@pytest.mark.parametrize('kind', KINDS)
def test_model_fused_and_eager_paths_agree(kind):
    model, images, targets = _model_and_batch()
    model.box_loss, model.box_loss_weight = kind, 1.5
    assert model.fused_loss
    fused = _step(model, images, targets)
    model.fused_loss = False
    eager = _step(model, images, targets)
    for k in range(2):
        print(kind, 'loss', k, float(fused[k]), float(eager[k]))
        assert abs(float(fused[k]) - float(eager[k])) <= 1e-5 * abs(float(eager[k])) and float(eager[k]) > 0
    scale = float(eager[2].abs().max())
    worst = float((fused[2] - eager[2]).abs().max())
    print(kind, 'box head weight gradient: worst %.3g of %.3g' % (worst, scale))
    assert scale > 0 and worst <= 1e-4 * scale


def test_model_default_is_untouched():
    model, images, targets = _model_and_batch()
    never_set = _step(model, images, targets)
    model.box_loss, model.box_loss_weight = 'smooth_l1', 1.0
    explicit = _step(model, images, targets)
    assert torch.equal(never_set[0], explicit[0]) and torch.equal(never_set[1], explicit[1])      # the same bits
    model.box_loss = 'giou'
    assert not torch.equal(_step(model, images, targets)[1], never_set[1])


def test_model_groups_seven_levels():
    """More levels than one launch takes (several backbones): the pass is split, the loss has no state across levels."""
    model, images, targets = _model_and_batch()
    model.box_loss = 'giou'
    g = torch.Generator().manual_seed(1)
    x = torch.zeros(2, 3, 256, 256, device='cuda')
    sizes = [32, 16, 8, 4, 2, 1, 32]                                        # strides 8 .. 256, and stride 8 once more
    big = torch.tensor([[[8.0, 8.0, 32.0, 32.0, 0.0], [40.0, 16.0, 45.0, 23.0, 2.0], [20.0, 20.0, 130.0, 126.0, 1.0]],
                        [[50.0, 4.0, 64.0, 66.0, 1.0], [4.0, 10.0, 23.0, 45.0, 0.0], [-60.0, -60.0, 400.0, 380.0, 2.0]]]).cuda()
    cls_heads = [(torch.randn(2, 27, s, s, generator=g) - 3).cuda() for s in sizes]
    box_heads = [(torch.randn(2, 36, s, s, generator=g) * 0.2).cuda().requires_grad_(True) for s in sizes]
    assert len(sizes) > _C.MAX_LEVELS
    out = []
    for fused in (True, False):
        model.fused_loss = fused
        cls_loss, box_loss = model._compute_loss(x, cls_heads, box_heads, big)
        box_loss.backward()
        out.append((float(cls_loss.detach()), float(box_loss.detach()), [h.grad.clone() for h in box_heads]))
        for h in box_heads:
            h.grad = None
    assert abs(out[0][0] - out[1][0]) <= 1e-5 * abs(out[1][0]) and abs(out[0][1] - out[1][1]) <= 1e-5 * abs(out[1][1]) and out[1][1] > 0
    for mine, ref in zip(out[0][2], out[1][2]):
        assert float((mine - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    assert float(out[1][2][6].abs().max()) > 0                                # the seventh level carries foreground
