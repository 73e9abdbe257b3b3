"""The quality focal / varifocal loss kernels (csrc/quality_loss.hpp, odtk_quality_loss_levels_*) on the GPU against their definition:
tests/quality_loss_ref.py, float64 numpy on the same inputs (16-bit heads: the rounded values, converted exactly).  Bars (those of
tests/test_gpu_loss.py and tests/test_gpu_box_iou_loss.py): sums within 1e-6 relative of float64, the foreground count exact,
d(logits) within 1e-5 of the largest reference gradient for fp32 heads, 1e-2 for bf16 and 2e-3 for fp16 (one rounding of the stored
gradient).

Shapes: the smallest at which every route of the walk is taken -- 16 x 24 cells (several workgroups), 5 x 7 and 1 x 1 (H*W no
multiple of the vector: NCHW goes element by element), C = 80 (vectors inside one anchor's classes) and C = 3, 5 (no vector is:
channels_last goes element by element with carries), A = 9 and 1, element counts with a scalar tail (2 * 9 * 3 * 35 = 1890).

Contents.  Every loss term is >= 0, so the sums have no cancellation between elements; what a finite float64 reference allows:
+-100 and values either side of kPlainMax = 64 (63.5 / 64.5: exact in bf16) anywhere, -inf at negative elements (term and gradient
0), +inf and NaN in ignored cells only -- by the definition a counted +inf logit, or -inf at the element that is its anchor's
class, has an infinite loss.  The reference's finiteness is asserted for every case."""
import functools

import numpy as np
import pytest
import torch

import quality_loss_ref as ref
from odtk import _C, box
from odtk import loss as L
from odtk.model import Model

pytestmark = pytest.mark.gpu

KINDS = ('qfl', 'vfl')
RATIOS, SCALES = [1.0, 2.0, 0.5], [4 * 2 ** (i / 3) for i in range(3)]
LEVELS3 = ((8, 16, 24), (32, 5, 7), (128, 1, 1))
LEVELS5 = ((8, 16, 24), (16, 8, 12), (32, 5, 7), (64, 2, 3), (128, 1, 1))
LEVELS6 = LEVELS5 + ((256, 1, 1),)
LEVELS7 = LEVELS6 + ((8, 16, 24),)
FORMATS = [(torch.float32, False), (torch.float32, True), (torch.bfloat16, True), (torch.float16, True), (torch.float16, False)]
FORMAT_IDS = ['fp32-nchw', 'fp32-nhwc', 'bf16-nhwc', 'fp16-nhwc', 'fp16-nchw']
GRAD_TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 2e-3}
UPSTREAM = (-1.9, 0.37, 1.0, -0.6, 2.25, 0.11, 0.8)
# (x, y, w, h, class) in a 192 x 128 image: boxes near the anchors of strides 8 .. 32 and two that only the large anchors cover
BOXES = [[[24.0, 40.0, 33.0, 31.0, 0.0], [100.0, 60.0, 45.0, 23.0, 2.0], [60.0, 10.0, 110.0, 100.0, 1.0], [-70.0, -190.0, 520.0, 500.0, 1.0],
          [130.0, 80.0, 40.0, 36.0, 0.0]],
         [[150.0, 50.0, 23.0, 45.0, 1.0], [30.0, 30.0, 130.0, 66.0, 2.0], [64.0, -192.0, 512.0, 512.0, 0.0], [40.0, 70.0, 30.0, 31.0, 2.0],
          [-1.0, -1.0, -1.0, -1.0, -1.0]]]


def _anchors(levels, a):
    if a == 9:
        return [box.generate_anchors(s, RATIOS, SCALES) for s, _, _ in levels]
    return [box.generate_anchors(s, [1.0], [4.0]) for s, _, _ in levels]


@functools.lru_cache(maxsize=None)
def _targets(levels, a, c, source):
    """-> (anchors, box_targets, depths) on the CPU.  source: 'iou' / 'atss' = the assigners on BOXES; 'mixed' = a synthetic depth map
    with ignored, background and foreground cells (every class) next to each other, targets N(0, 0.3)."""
    anchors = _anchors(levels, a)
    sizes, strides = [(h, w) for _, h, w in levels], [s for s, _, _ in levels]
    if source == 'iou':
        _, box_targets, depths = box.snap_to_anchors_levels(torch.tensor(BOXES, device='cuda'), sizes, strides, anchors, c, [0.4, 0.5],
                                                            want_cls_target=False)
    elif source == 'atss':
        _, box_targets, depths = box.atss_assign_levels(torch.tensor(BOXES, device='cuda'), sizes, strides, anchors, c, 9, want_cls_target=False)
    else:
        g = torch.Generator().manual_seed(5)
        box_targets = [torch.randn(2, a, 4, h, w, generator=g) * 0.3 for h, w in sizes]
        depths = []
        for h, w in sizes:
            idx = torch.arange(2 * a * h * w).reshape(2, a, 1, h, w)
            role = idx % 7                                       # 0: ignored, 5: foreground of class idx % c, else background
            depths.append(torch.where(role == 0, -1.0, torch.where(role == 5, (idx % c + 1).float(), 0.0)))
    return anchors, [t.cpu() for t in box_targets], [d.cpu() for d in depths]


def _inputs(targets, c, seed, mode='noise', dirty=True, tame=False):
    """float32 CPU heads for `targets`: logits N(-3, 2) with the special values planted, deltas = targets + noise (mode 'noise': q spreads
    over (0, 1); 'equal': q = 1; 'off': shifted off the target, q = 0; 'clip': sizes beyond the clip).  dirty: NaN / +-inf / 1e30 logits in
    ignored cells ('nan': NaN and -inf only; 'tame': -3 in the same places and clean deltas, the twin 'nan' is compared with) and NaN deltas
    at every cell that is not foreground.  tame: no special values at all."""
    _, box_targets, depths = targets
    g = torch.Generator().manual_seed(seed)
    cls_heads, box_heads = [], []
    for bt, depth in zip(box_targets, depths):
        b, a, _, h, w = bt.shape
        x = torch.randn(b, a, c, h, w, generator=g) * 2 - 3
        is_target = depth - 1 == torch.arange(c, dtype=torch.float32).view(1, 1, c, 1, 1)
        ignored = (depth < 0).expand_as(x)
        if not tame:
            flat = x.view(-1)
            special = torch.tensor([100.0, -100.0, 63.5, 64.5, float('-inf'), 30.0, -30.0])
            at = torch.linspace(0, flat.numel() - 1, min(14, flat.numel() // 64)).long()   # a few: they must not drown the other terms
            flat[at] = special[torch.arange(at.numel()) % 7]
            # the elements that are their anchor's class: every second one gets a special value too (never an infinite one)
            hot = is_target.reshape(-1).nonzero().reshape(-1)
            flat[hot] = torch.where(torch.isinf(flat[hot]), torch.full_like(flat[hot], -100.0), flat[hot])
            # At such an element a logit x multiplies the float32 rounding of q (about 2e-7) by |x| in the loss: +-100 there belong on
            # a level whose sum is large enough to be well conditioned; a level of a few dozen elements gets moderate values
            values = [100.0, -100.0, 63.5, 64.5, 0.5, -2.0] if flat.numel() >= 2048 else [3.0, -6.0, 0.5, -2.0]
            flat[hot[::2]] = torch.tensor(values)[torch.arange(hot[::2].numel()) % len(values)]
        if dirty:
            values = {'nan': [float('nan'), float('-inf')], 'tame': [-3.0]}.get(dirty, [float('nan'), float('inf'), float('-inf'), 1e30])
            junk = torch.tensor(values)[torch.arange(x.numel()) % len(values)].view_as(x)
            x = torch.where(ignored & (torch.arange(x.numel()).view_as(x) % 3 != 0), junk, x)
        d = bt + torch.randn(bt.shape, generator=g) * (0.15 if mode != 'equal' else 0.0)
        if mode == 'off':
            d[:, :, 0] += 50.0
        elif mode == 'clip':
            d[:, ::2, 2, :, ::3] = 4.75
            d[:, :, 3, ::2] = 9.0
        if dirty and dirty != 'tame':
            d = torch.where((depth > 0).expand_as(d), d, torch.full_like(d, float('nan')))
        cls_heads.append(x.reshape(b, a * c, h, w))
        box_heads.append(d.reshape(b, a * 4, h, w))
    return cls_heads, box_heads


def _to_device(heads, dtype, channels_last, requires_grad=False):
    out = []
    for t in heads:
        t = t.cuda().to(dtype)
        if channels_last:
            t = t.contiguous(memory_format=torch.channels_last)
        out.append(t.requires_grad_(requires_grad))
    return out


def _reference(cls_heads, box_heads, targets, kind, alpha, gamma):
    """float64 numpy on the values the kernel reads -> (sums, foreground counts, gradients of the sums)."""
    anchors, box_targets, depths = targets
    out = [ref.level(c.detach().float().cpu().numpy(), b.detach().float().cpu().numpy(), bt.numpy(), d.numpy(), L.anchor_wh(an).numpy(), kind,
                     alpha, gamma) for c, b, bt, d, an in zip(cls_heads, box_heads, box_targets, depths, anchors)]
    assert all(np.isfinite(s) and np.isfinite(grad).all() for s, _, grad in out)          # the case is one the bars apply to
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def _poison(heads):
    """Leave NaNs in the blocks the allocator hands out next: a gradient element the kernel does not write shows."""
    junk = [torch.full_like(h, float('nan')) for h in heads]
    del junk


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _check(targets, c, kind, dtype, channels_last, alpha=0.75, gamma=2.0, seed=3, mode='noise', dirty=True, want_fg=None):
    anchors, box_targets, depths = targets
    cls_cpu, box_cpu = _inputs(targets, c, seed, mode, dirty)
    cls_heads, box_heads = _to_device(cls_cpu, dtype, channels_last, True), _to_device(box_cpu, dtype, channels_last, True)
    dev_targets, dev_depths = [t.cuda() for t in box_targets], [d.cuda() for d in depths]
    n = len(cls_heads)
    ref_sums, ref_fg, ref_grads = _reference(cls_heads, box_heads, targets, kind, alpha, gamma)
    args = ([t.detach() for t in cls_heads], [t.detach() for t in box_heads], dev_depths, dev_targets, anchors, kind, alpha, gamma)
    got, again = _C.quality_loss_levels_forward(*args), _C.quality_loss_levels_forward(*args)
    assert got.dtype == torch.float64 and got.shape == (n, 2)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))         # the same bits on every run
    got = got.cpu()
    for l in range(n):
        print('level %d %s: sum %.12g want %.12g (rel %.2g), fg %g' % (l, kind, float(got[l, 0]), ref_sums[l],
                                                                     abs(float(got[l, 0]) - ref_sums[l]) / max(abs(ref_sums[l]), 1e-300), float(got[l, 1])))
    for l in range(n):
        assert float(got[l, 1]) == ref_fg[l]
        assert abs(float(got[l, 0]) - ref_sums[l]) <= 1e-6 * abs(ref_sums[l]), (l, float(got[l, 0]), ref_sums[l])
    if want_fg is not None:
        assert [int(f) for f in ref_fg] == want_fg
    # the autograd form: the same sums (as float32), gradients in the heads' dtype and layout, none for the box heads
    sums, fg = L.fused_pyramid_quality_loss(cls_heads, box_heads, dev_depths, dev_targets, anchors, kind, alpha, gamma)
    assert torch.equal(sums.cpu(), got[:, 0].float()) and torch.equal(fg.cpu(), got[:, 1].float()) and not fg.requires_grad
    _poison(cls_heads)
    upstream = torch.tensor(UPSTREAM[:n], device='cuda')
    (sums * upstream).sum().backward()
    direct = _C.quality_loss_levels_backward(*args, upstream)
    for l, (head, grad64, depth) in enumerate(zip(cls_heads, ref_grads, depths)):
        mine = head.grad
        assert box_heads[l].grad is None
        assert mine.dtype == dtype and mine.stride() == head.stride() and mine.shape == head.shape
        assert torch.equal(_bits(mine), _bits(direct[l]))                      # the same bits on every run
        want = torch.from_numpy(grad64) * UPSTREAM[l]
        scale = float(want.abs().max())
        worst = float((mine.float().cpu().double() - want).abs().max())        # (a NaN left unwritten fails the comparison below)
        print('level %d %s: gradient worst %.3g of %.3g' % (l, kind, worst, scale))
        assert worst <= GRAD_TOL[dtype] * scale, (l, worst, scale)
        # +0, bit for bit, at every element of an ignored anchor, whatever its logit
        b, a, _, h, w = depth.shape
        off = (depth < 0).expand(b, a, c, h, w).reshape(b, a * c, h, w).cuda()
        assert int((_bits(mine)[off] != 0).sum()) == 0
    return got


CASES = [(9, 80, 'iou'), (1, 80, 'atss'), (9, 80, 'mixed'), (9, 3, 'mixed'), (1, 5, 'mixed')]


@pytest.mark.parametrize('a,c,source', CASES, ids=['a9-c80-iou', 'a1-c80-atss', 'a9-c80-mixed', 'a9-c3-mixed', 'a1-c5-mixed'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype,channels_last', FORMATS, ids=FORMAT_IDS)
def test_against_float64(dtype, channels_last, kind, a, c, source):
    targets = _targets(LEVELS3, a, c, source)
    n_fg = sum(int((d > 0).sum()) for d in targets[2])
    assert n_fg >= (3 if source != 'mixed' else 40)
    if (a, c) == (9, 3):
        assert (2 * 9 * 3 * 35) % 8 == 2                      # the 5 x 7 level ends in a scalar tail for every dtype
    _check(targets, c, kind, dtype, channels_last)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype,channels_last', [FORMATS[0], FORMATS[2], FORMATS[4]], ids=['fp32-nchw', 'bf16-nhwc', 'fp16-nchw'])
def test_general_gamma_and_alpha(dtype, channels_last, kind):
    for a, c in ((9, 80), (1, 5)):
        _check(_targets(LEVELS3, a, c, 'mixed'), c, kind, dtype, channels_last, alpha=0.4, gamma=1.5, seed=8)
    _check(_targets(LEVELS3, 9, 3, 'mixed'), 3, kind, dtype, channels_last, alpha=1.0, gamma=1.0, seed=9)


@pytest.mark.parametrize('levels', [LEVELS3[:1], LEVELS5, LEVELS6], ids=['1-level', '5-levels', '6-levels'])
def test_level_counts(levels):
    assert len(LEVELS6) == _C.MAX_LEVELS
    _check(_targets(levels, 9, 80, 'iou'), 80, 'qfl', torch.float32, True)
    _check(_targets(levels, 9, 3, 'mixed'), 3, 'vfl', torch.float16, False)


def test_seven_levels_are_grouped():
    targets = _targets(LEVELS7, 9, 3, 'mixed')
    anchors, box_targets, depths = targets
    cls_cpu, box_cpu = _inputs(targets, 3, 4)
    cls_heads, box_heads = _to_device(cls_cpu, torch.float32, True, True), _to_device(box_cpu, torch.float32, True)
    ref_sums, ref_fg, ref_grads = _reference(cls_heads, box_heads, targets, 'qfl', 0.75, 2.0)
    sums, fg = L.fused_pyramid_quality_loss(cls_heads, box_heads, [d.cuda() for d in depths], [t.cuda() for t in box_targets], anchors, 'qfl')
    assert sums.shape == (7,) and fg.cpu().tolist() == ref_fg
    (sums * torch.tensor(UPSTREAM, device='cuda')).sum().backward()
    for l in range(7):
        assert abs(float(sums[l].detach()) - ref_sums[l]) <= 1e-6 * abs(ref_sums[l])      # (float32 of the float64 sum: 6e-8)
        want = torch.from_numpy(ref_grads[l]) * UPSTREAM[l]
        assert float((cls_heads[l].grad.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    with pytest.raises(RuntimeError, match='levels'):
        _C.quality_loss_levels_forward([t.detach() for t in cls_heads], box_heads, [d.cuda() for d in depths], [t.cuda() for t in box_targets],
                                       anchors, 'qfl')


@pytest.mark.parametrize('mode', ['equal', 'off', 'clip'])
@pytest.mark.parametrize('kind', KINDS)
def test_quality_at_its_ends_and_beyond_the_clip(kind, mode):
    """q = 1 (prediction == target), q = 0 (prediction off the target: varifocal's negative branch at a foreground anchor), predicted
    sizes beyond the clip."""
    for (a, c), (dtype, channels_last) in (((9, 80), FORMATS[1]), ((9, 3), FORMATS[0]), ((1, 5), FORMATS[2])):
        targets = _targets(LEVELS3, a, c, 'mixed')
        if mode != 'clip':
            cls_cpu, box_cpu = _inputs(targets, c, 6, mode, dirty=False)
            for bh, bt, depth, an in zip(box_cpu, targets[1], targets[2], targets[0]):
                q = ref.box_quality(bh.view(bt.shape).numpy(), bt.numpy(), L.anchor_wh(an).numpy())[(depth[:, :, 0] > 0).numpy()]
                assert (np.abs(q - 1) <= 1e-9).all() if mode == 'equal' else (q == 0).all()
        _check(targets, c, kind, dtype, channels_last, seed=6, mode=mode)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype,channels_last', FORMATS, ids=FORMAT_IDS)
def test_ignored_logits_and_cells_that_are_not_foreground_change_nothing(dtype, channels_last, kind):
    """NaN logits in ignored cells leave the sums unchanged, bit for bit, and get gradient +0; NaN deltas at every cell that is not
    foreground change nothing either: those cells are never read.  (The twin run has -3 where this one has NaN or -inf: a logit beyond kPlainMax
    in an ignored cell contributes nothing either, but sends its vector, the counted elements of an NCHW vector included, through the
    other arithmetic form -- _check covers those against float64, not bit for bit.)"""
    for a, c in ((9, 80), (9, 3)):
        targets = _targets(LEVELS3, a, c, 'mixed')
        anchors, box_targets, depths = targets
        dev_targets, dev_depths = [t.cuda() for t in box_targets], [d.cuda() for d in depths]
        out = []
        for dirty in ('tame', 'nan'):
            cls_cpu, box_cpu = _inputs(targets, c, 7, dirty=dirty)
            assert (dirty == 'nan') == any(bool(torch.isnan(t).any()) for t in cls_cpu) == any(bool(torch.isnan(t).any()) for t in box_cpu)
            cls_heads, box_heads = _to_device(cls_cpu, dtype, channels_last), _to_device(box_cpu, dtype, channels_last)
            sums = _C.quality_loss_levels_forward(cls_heads, box_heads, dev_depths, dev_targets, anchors, kind)
            grads = _C.quality_loss_levels_backward(cls_heads, box_heads, dev_depths, dev_targets, anchors, kind, 0.75, 2.0,
                                                    torch.tensor(UPSTREAM[:3], device='cuda'))
            out.append((sums, grads))
        assert torch.equal(out[0][0].view(torch.int64), out[1][0].view(torch.int64)) and bool(torch.isfinite(out[1][0]).all())
        for clean, dirty, depth in zip(out[0][1], out[1][1], depths):
            assert bool(torch.isfinite(dirty).all())
            keep = (depth >= 0).expand(2, a, c, *depth.shape[3:]).reshape(dirty.shape).cuda()
            assert torch.equal(_bits(clean)[keep], _bits(dirty)[keep]) and int((_bits(dirty)[~keep] != 0).sum()) == 0
        # ... while a NaN delta at a foreground anchor reaches its level's sum, and only that one
        cls_cpu, box_cpu = _inputs(targets, c, 7, dirty=False)
        hit = (depths[1] > 0).expand(2, a, 4, 5, 7).reshape(2, a * 4, 5, 7)
        box_cpu[1] = torch.where(hit & (torch.arange(hit.numel()).view_as(hit) % 4 == 1), torch.full_like(box_cpu[1], float('nan')), box_cpu[1])
        sums = _C.quality_loss_levels_forward(_to_device(cls_cpu, dtype, channels_last), _to_device(box_cpu, dtype, channels_last), dev_depths,
                                              dev_targets, anchors, kind).cpu()
        assert [bool(torch.isnan(sums[l, 0])) for l in range(3)] == [False, True, False]
        assert torch.equal(sums[:, 1], out[0][0].cpu()[:, 1])


def test_no_upstream_gradient_gives_zeros():
    targets = _targets(LEVELS3, 9, 80, 'mixed')
    anchors, box_targets, depths = targets
    cls_cpu, box_cpu = _inputs(targets, 80, 2, dirty=True, tame=True)
    for dtype, channels_last in FORMATS:
        for kind in KINDS:
            cls_heads, box_heads = _to_device(cls_cpu, dtype, channels_last), _to_device(box_cpu, dtype, channels_last)
            _poison(cls_heads)
            for upstream in (None, torch.zeros(3, device='cuda')):
                grads = _C.quality_loss_levels_backward(cls_heads, box_heads, [d.cuda() for d in depths], [t.cuda() for t in box_targets], anchors,
                                                        kind, 0.75, 2.0, upstream)
                for g, head in zip(grads, cls_heads):
                    assert g.dtype == dtype and g.stride() == head.stride()
                    assert int((_bits(g) != 0).sum()) == 0


def _single_anchor_case(a=9, c=80, cls=37):
    """One foreground anchor per level of LEVELS3, every other anchor ignored, its other classes at -20 (1e-17 each): cls_sum is L(q)
    of that one element.  -> (depths, box_targets, logits, deltas, the cells), CPU float32."""
    g = torch.Generator().manual_seed(12)
    depths, box_targets, cls_cpu, box_cpu, where = [], [], [], [], []
    for i, (_, h, w) in enumerate(LEVELS3):
        depth = torch.full((2, a, 1, h, w), -1.0)
        cell = (1, (4 + i) % a, 0, h - 1, w // 2)
        depth[cell] = cls + 1.0
        bt = torch.randn(2, a, 4, h, w, generator=g) * 0.3
        d = bt + torch.randn(2, a, 4, h, w, generator=g) * 0.2
        if i == 1:
            d[cell[0], cell[1], 2, cell[3], cell[4]] = 4.5                       # beyond the clip: the box is exp(CLIP) anchors wide
        x = torch.randn(2, a, c, h, w, generator=g) * 2 - 3
        x[cell[0], cell[1], :, cell[3], cell[4]] = -20.0
        x[cell[0], cell[1], cls, cell[3], cell[4]] = (-3.0, -1.5, -2.5)[i]      # sigmoid well away from q: |s - q|^2 is well conditioned
        depths.append(depth), box_targets.append(bt), where.append(cell)
        cls_cpu.append(x.reshape(2, a * c, h, w)), box_cpu.append(d.reshape(2, a * 4, h, w))
    return depths, box_targets, cls_cpu, box_cpu, where


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype,channels_last', [FORMATS[0], FORMATS[1], FORMATS[2]], ids=['fp32-nchw', 'fp32-nhwc', 'bf16-nhwc'])
def test_the_quality_is_the_box_loss_own(dtype, channels_last, kind):
    """cls_sum minus the float64 share of the anchor's other classes is L(q) with q = 1 - the sum of odtk_box_iou_loss_levels_forward
    ('iou') on the same tensors -- the clip included -- within the bar on the sums; a q that is off by 1e-4 would be outside it."""
    a, c, cls = 9, 80, 37
    anchors = _anchors(LEVELS3, a)
    depths, box_targets, cls_cpu, box_cpu, where = _single_anchor_case(a, c, cls)
    cls_heads, box_heads = _to_device(cls_cpu, dtype, channels_last), _to_device(box_cpu, dtype, channels_last)
    dev_depths, dev_targets = [d.cuda() for d in depths], [t.cuda() for t in box_targets]
    sums = _C.quality_loss_levels_forward(cls_heads, box_heads, dev_depths, dev_targets, anchors, kind).cpu()
    iou = _C.box_iou_loss_levels_forward(box_heads, dev_depths, dev_targets, anchors, 'iou').cpu()
    fn = (lambda v, t: ref.qfl(v, t, 2.0)[0]) if kind == 'qfl' else (lambda v, t: ref.vfl(v, t, 0.75, 2.0)[0])
    for l, cell in enumerate(where):
        assert float(sums[l, 1]) == 1 == float(iou[l, 1])
        q = float(np.float32(1.0) - np.float32(float(iou[l, 0])))            # float32 arithmetic, as the walk's
        x = cls_heads[l].float().cpu().double().view(2, a, c, *depths[l].shape[3:])[cell[0], cell[1], :, cell[3], cell[4]].numpy()
        others = float(fn(x, np.zeros(c)).sum() - fn(x[cls], 0.0))
        want = float(fn(x[cls], q))
        got = float(sums[l, 0]) - others
        print('level %d %s: q %.9g, L(q) %.9g, cls_sum - negatives %.9g' % (l, kind, q, want, got))
        assert 0 < q < 1 and others < 1e-9 * want and abs(got - want) <= 1e-6 * float(sums[l, 0])
        assert abs(float(fn(x[cls], q + 1e-4)) - want) > 4e-6 * want           # the bar resolves q to 1e-4 or better


def test_exotic_strides_and_argument_checks():
    targets = _targets(LEVELS3, 9, 80, 'iou')
    anchors, box_targets, depths = targets
    cls_cpu, box_cpu = _inputs(targets, 80, 6)
    cls_heads, box_heads = _to_device(cls_cpu, torch.float32, False), _to_device(box_cpu, torch.float32, False)
    dev_depths, dev_targets = [d.cuda() for d in depths], [t.cuda() for t in box_targets]
    want = _C.quality_loss_levels_forward(cls_heads, box_heads, dev_depths, dev_targets, anchors, 'vfl')
    sliced = [torch.cat([h, h], 3)[:, :, :, :h.shape[3]] for h in cls_heads]          # neither NCHW nor channels_last
    mixed = [h.contiguous(memory_format=torch.channels_last) for h in box_heads]       # and the box heads in the other layout
    assert not sliced[0].is_contiguous()
    sums, _ = L.fused_pyramid_quality_loss(sliced, mixed, dev_depths, dev_targets, anchors, 'vfl')
    assert torch.equal(sums, want[:, 0].float())
    with pytest.raises(RuntimeError, match='contiguous'):
        _C.quality_loss_levels_forward(sliced, box_heads, dev_depths, dev_targets, anchors, 'vfl')
    with pytest.raises(RuntimeError, match='memory format'):
        _C.quality_loss_levels_forward(cls_heads[:1], mixed[:1], dev_depths[:1], dev_targets[:1], anchors[:1], 'vfl')
    with pytest.raises(ValueError, match='kind'):
        L.fused_pyramid_quality_loss(cls_heads, box_heads, dev_depths, dev_targets, anchors, 'focal')
    with pytest.raises(RuntimeError, match='dtype'):
        _C.quality_loss_levels_forward([h.half() for h in cls_heads], box_heads, dev_depths, dev_targets, anchors, 'qfl')
    with pytest.raises(RuntimeError, match='float32 / bfloat16 / float16'):
        _C.quality_loss_levels_forward([h.double() for h in cls_heads], [h.double() for h in box_heads], dev_depths, dev_targets, anchors, 'qfl')
    with pytest.raises(RuntimeError, match='shapes'):
        _C.quality_loss_levels_forward(cls_heads, box_heads, dev_depths[::-1], dev_targets, anchors, 'qfl')
    with pytest.raises(RuntimeError, match='classes'):
        _C.quality_loss_levels_forward([cls_heads[0], cls_heads[1][:, :9 * 40].contiguous(), cls_heads[2]], box_heads, dev_depths, dev_targets,
                                       anchors, 'qfl')
    for alpha, gamma in ((0.75, 0.99), (0.75, float('inf')), (-0.1, 2.0), (float('nan'), 2.0)):
        with pytest.raises(RuntimeError, match='gamma'):
            _C.quality_loss_levels_forward(cls_heads, box_heads, dev_depths, dev_targets, anchors, 'vfl', alpha, gamma)
    # the library itself refuses them too, and a short workspace, before any launch: the sums keep their bits
    lib, arr, tables, keep = _C.library(), *_C._quality_levels('test', cls_heads, box_heads, dev_depths, dev_targets, anchors, 'qfl', 0.75, 2.0)[:3]
    sums = torch.full((3, 2), -7.0, dtype=torch.float64, device='cuda')
    ws = torch.empty(1 << 16, dtype=torch.uint8, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def forward(dtype=_C.F32, kind=_C.CLS_LOSS_QFL, alpha=0.75, gamma=2.0, size=ws.numel()):
        return lib.odtk_quality_loss_levels_forward(3, arr, tables, 2, 9, 80, dtype, kind, alpha, gamma, sums.data_ptr(), ws.data_ptr(), size, stream)

    need = lib.odtk_quality_loss_levels_forward(3, arr, tables, 2, 9, 80, _C.F32, _C.CLS_LOSS_QFL, 0.75, 2.0, None, None, 0, None)
    assert 0 < need <= ws.numel()
    assert forward(dtype=5) == _C.ERR_UNSUPPORTED and forward(kind=3) == _C.ERR_INVALID and forward(gamma=0.5) == _C.ERR_INVALID
    assert forward(alpha=-1.0) == _C.ERR_INVALID and forward(size=need - 1) == _C.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((sums == -7.0).all())
    assert forward(size=need) == _C.OK
    torch.cuda.synchronize()
    assert torch.equal(sums.view(torch.int64), _C.quality_loss_levels_forward(cls_heads, box_heads, dev_depths, dev_targets, anchors, 'qfl')
                       .view(torch.int64))


# ---------------------------------------------------------------------------------------------------------------- Model
@functools.lru_cache(maxsize=None)
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


def _configure(model, cls_loss='focal', box_loss='smooth_l1', assigner='iou', fused=True):
    model.cls_loss, model.box_loss, model.box_loss_weight, model.assigner, model.fused_loss = cls_loss, box_loss, 1.0, assigner, fused


def _step(model, images, targets):
    model.zero_grad(set_to_none=True)
    cls_loss, box_loss = model((images, targets))
    (cls_loss + box_loss).backward()
    return (cls_loss.detach().clone(), box_loss.detach().clone(), model.cls_head[-1].weight.grad.detach().clone(),
            model.box_head[-1].weight.grad.detach().clone())


@pytest.mark.parametrize('assigner', ['iou', 'atss'])
@pytest.mark.parametrize('box_loss', ['giou', 'smooth_l1'])
@pytest.mark.parametrize('kind', KINDS)
def test_model_fused_and_eager_paths_agree(kind, box_loss, assigner):
    model, images, targets = _model_and_batch()
    try:
        _configure(model, kind, box_loss, assigner, True)
        fused = _step(model, images, targets)
        _configure(model, kind, box_loss, assigner, False)
        eager = _step(model, images, targets)
    finally:
        _configure(model)
    for k in range(2):
        print(kind, box_loss, assigner, 'loss', k, float(fused[k]), float(eager[k]))
        assert abs(float(fused[k]) - float(eager[k])) <= 1e-5 * abs(float(eager[k])) and float(eager[k]) > 0
    for k in (2, 3):
        scale = float(eager[k].abs().max())
        worst = float((fused[k] - eager[k]).abs().max())
        print(kind, box_loss, assigner, 'head weight gradient %d: worst %.3g of %.3g' % (k, worst, scale))
        assert scale > 0 and worst <= 1e-4 * scale


def test_model_default_is_untouched():
    model, images, targets = _model_and_batch()
    _configure(model)
    never_set = _step(model, images, targets)
    # what `_compute_loss` did before the option existed, composed by hand: the same bits
    model.zero_grad(set_to_none=True)
    cls_heads, box_heads = model.heads(images)
    strides = [images.shape[-1] / c.shape[-1] for c in cls_heads]
    _, box_targets, depths = box.snap_to_anchors_levels(targets, [tuple(c.shape[-2:]) for c in cls_heads], strides,
                                                        [model.level_anchors(s) for s in strides], model.classes, model.anchor_ious,
                                                        want_cls_target=False)
    cls_sums, box_sums, fg = L.fused_pyramid_loss(cls_heads, box_heads, depths, box_targets, 0.25, 2, 0.11)
    foreground = fg.clamp(min=1).sum()
    assert torch.equal(never_set[0], (cls_sums.sum() / foreground).detach()) and torch.equal(never_set[1], (box_sums.sum() / foreground).detach())
    model.cls_loss = 'focal'
    explicit = _step(model, images, targets)
    assert torch.equal(never_set[0], explicit[0]) and torch.equal(never_set[1], explicit[1])      # the same bits
    try:
        model.cls_loss = 'qfl'
        other = _step(model, images, targets)
    finally:
        _configure(model)
    assert not torch.equal(other[0], never_set[0]) and torch.equal(other[1], never_set[1])      # the box loss does not move
