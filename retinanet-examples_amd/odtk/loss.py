"""Training losses of RetinaNet on PyTorch-ROCm: the focal classification loss
(https://arxiv.org/abs/1708.02002) and the smooth-L1 box loss.  Both are elementwise (no reduction);
`Model._compute_loss` masks and sums them.  Values follow the reference's definitions
(reference odtk/loss.py:13-31: alpha = 0.25, gamma = 2, beta = 0.11).

`fused_level_loss` is the MI355X form of one level's share of `Model._compute_loss`
(reference model.py:193-209): focal loss, smooth-L1, both masks and the three sums in ONE hand-written HIP
pass over the head tensors as the convolutions wrote them, and ONE pass in backward (csrc/loss.hpp) -- an
`autograd.Function`, so it drops into the training graph; the torch modules below stay as the reference
implementation it is tested against (tests/test_gpu_loss.py) and as the CPU path.

`box_iou_loss` (IoU / GIoU / DIoU on the boxes the deltas decode to; no reference equivalent) is the opt-in alternative to the
smooth-L1 box loss (`Model.box_loss`): the definition in torch -- the CPU path and the tests' ground truth -- and
`fused_pyramid_box_iou_loss`, its HIP form over all pyramid levels (csrc/box_iou_loss.hpp).

`rotated_box_loss` (ProbIoU / KLD on the Gaussians of the rotated boxes the six deltas decode to; no reference equivalent) is the
same for rotated models (`Model.box_loss = 'probiou' | 'kld'`): the definition in torch and `fused_pyramid_rotated_box_loss`, its
HIP form (csrc/rotated_box_loss.hpp).

`quality_focal_loss` (GFL) and `varifocal_loss` (VarifocalNet) are the opt-in alternatives to the focal loss (`Model.cls_loss`;
no reference equivalent): the class score is trained towards a soft target -- at a foreground anchor, for the assigned class,
`box_quality`, the IoU of the predicted and the assigned box, a constant of the loss; 0 everywhere else (`quality_target`).  The
definition, per level, with s = sigmoid(x), sp = softplus(x), y the target:
    qfl: L = |s - y|^gamma (sp - y x)        (y x = 0 where y = 0)        vfl: L = y (sp - y x) where y > 0, else alpha s^gamma sp
masked by `depth >= 0` and summed.  The torch functions are the CPU / eager path; `fused_pyramid_quality_loss` is the HIP form
over all pyramid levels (csrc/quality_loss.hpp), which builds neither the quality map nor the target."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


def focal_loss(logits, target, alpha=0.25, gamma=2.0):
    """alpha_t * (1 - p_t)^gamma * BCE(logits, target), per element; target is a 0/1 map."""
    prob = torch.sigmoid(logits)
    positive = target == 1
    p_t = torch.where(positive, prob, 1 - prob)                      # probability of the true label
    alpha_t = alpha * target + (1.0 - alpha) * (1.0 - target)
    bce = F.binary_cross_entropy_with_logits(logits, target, reduction='none')
    return alpha_t * (1.0 - p_t) ** gamma * bce


def smooth_l1_loss(pred, target, beta=0.11):
    """|d| - beta/2 beyond beta, d^2 / (2 beta) inside; per element."""
    dist = torch.abs(pred - target)
    quadratic = 0.5 * dist ** 2 / beta
    linear = dist - 0.5 * beta
    return torch.where(dist >= beta, linear, quadratic)


BOX_LOSS_KINDS = ('iou', 'giou', 'diou')
BBOX_XFORM_CLIP = math.log(1000.0 / 16)      # Detectron's clip of the predicted log-sizes
BOX_IOU_EPS = 1e-7


def box_iou_loss(pred, target, anchor_sizes, kind):
    """IoU-family loss of the boxes that predicted and target deltas decode to; per anchor, axis-aligned boxes only.

    pred, target [B, A, 4, H, W] deltas (dx, dy, dw, dh); anchor_sizes [A, 2] = (x2 - x1 + 1, y2 - y1 + 1) of the level's anchor
    table; kind 'iou' | 'giou' | 'diou' -> [B, A, H, W].  Both boxes are decoded relative to the anchor centre (the cell position
    cancels), the predicted log-sizes clipped at BBOX_XFORM_CLIP; then torchvision's {,generalized_,distance_}box_iou_loss:
        iou = inter / (area(P) + area(T) - inter + eps)                L = 1 - iou
        giou: c = area of the enclosing box + eps                      L = 1 - iou + (c - union) / c
        diou: c2 = squared diagonal of the enclosing box + eps         L = 1 - iou + |centre(P) - centre(T)|^2 / c2
    The arithmetic runs in pred's dtype (float64 in: the tests' ground truth)."""
    if kind not in BOX_LOSS_KINDS:
        raise ValueError("box_iou_loss: kind must be 'iou', 'giou' or 'diou', not {!r}".format(kind))
    sizes = torch.as_tensor(anchor_sizes, dtype=pred.dtype, device=pred.device)
    aw, ah = sizes[:, 0].view(1, -1, 1, 1), sizes[:, 1].view(1, -1, 1, 1)

    def corners(d, clip):
        dw, dh = (d[:, :, 2].clamp(max=BBOX_XFORM_CLIP), d[:, :, 3].clamp(max=BBOX_XFORM_CLIP)) if clip else (d[:, :, 2], d[:, :, 3])
        cx, cy, w, h = d[:, :, 0] * aw, d[:, :, 1] * ah, dw.exp() * aw, dh.exp() * ah
        return cx, cy, w, h, cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h

    pcx, pcy, pw, ph, px1, py1, px2, py2 = corners(pred, True)
    tcx, tcy, tw, th, tx1, ty1, tx2, ty2 = corners(target.to(pred.dtype), False)
    inter = (torch.minimum(px2, tx2) - torch.maximum(px1, tx1)).clamp(min=0) * \
            (torch.minimum(py2, ty2) - torch.maximum(py1, ty1)).clamp(min=0)
    union = pw * ph + tw * th - inter + BOX_IOU_EPS
    loss = 1 - inter / union
    ew = torch.maximum(px2, tx2) - torch.minimum(px1, tx1)
    eh = torch.maximum(py2, ty2) - torch.minimum(py1, ty1)
    if kind == 'giou':
        c = ew * eh + BOX_IOU_EPS
        loss = loss + (c - union) / c
    elif kind == 'diou':
        c2 = ew ** 2 + eh ** 2 + BOX_IOU_EPS
        loss = loss + ((pcx - tcx) ** 2 + (pcy - tcy) ** 2) / c2
    return loss


def anchor_wh(anchors):
    """[A, 4] anchor table (x1, y1, x2, y2) -> [A, 2] = (x2 - x1 + 1, y2 - y1 + 1), what `box_iou_loss` decodes with."""
    anchors = torch.as_tensor(anchors, dtype=torch.float32).reshape(-1, 4)
    return torch.stack([anchors[:, 2] - anchors[:, 0] + 1, anchors[:, 3] - anchors[:, 1] + 1], 1)


ROTATED_BOX_LOSS_KINDS = ('probiou', 'kld')
ROTATED_DIRECTION_EPS = 1e-12
PROBIOU_EPS = 1e-7
PROBIOU_MAX_DISTANCE = 100.0


def rotated_box_loss(pred, target, anchor_sizes, kind):
    """ProbIoU / KLD loss of the Gaussians of the rotated boxes that predicted and target deltas decode to; per anchor.

    pred, target [B, A, 6, H, W] deltas (dx, dy, dw, dh, sin, cos); anchor_sizes [A, 2] = (x2 - x1 + 1, y2 - y1 + 1) of the
    level's AXIS anchor table (`anchor_wh(generate_anchors_rotated(...)[0])`); kind 'probiou' | 'kld' -> [B, A, H, W].  Both
    boxes are decoded relative to the anchor centre (the cell position cancels), the predicted log-sizes clipped at
    BBOX_XFORM_CLIP (no gradient beyond it):
        centre (d0 aw, d1 ah), w = exp(d2) aw, h = exp(d3) ah
        q = d4^2 + d5^2 + 1e-12;  cc = d5^2 / q, ss = d4^2 / q, sc = d4 d5 / q                     (no atan2, no sqrt)
        a = (w^2 cc + h^2 ss) / 12    b = (w^2 ss + h^2 cc) / 12    c = -(w^2 - h^2) sc / 12
    [[a, c], [c, b]] is the covariance of the uniform distribution on the rotated rectangle in the convention of
    odtk/box.py:rotate_boxes -- width axis (cos, -sin), height axis (sin, cos); three times it is the covariance of the four
    corners.  With 1 the prediction, 2 the target and (dx, dy) = centre(P) - centre(T):
        probiou: A = a1 + a2, B = b1 + b2, C = c1 + c2, D = A B - C^2
                 BD = (B dx^2 + A dy^2 - 2 C dx dy) / (4 D) + 0.5 ln(36 D / (w h tw th)), clamped to [0, 100]
                 L = sqrt(1 - exp(-BD) + 1e-7)                                         (arXiv 2106.06072)
        kld:     d2 = (tw th / 12)^2
                 K = 0.5 [(b2 a1 + a2 b1 - 2 c2 c1) / d2 + (b2 dx^2 + a2 dy^2 - 2 c2 dx dy) / d2 - 2] + ln(tw th / (w h)), clamped at 0
                 L = 1 - 1 / (1 + ln(1 + K))                                           (KL(N_pred || N_target), arXiv 2106.01883)
    The clamps hand a NaN on and have no gradient where they bind.  Direction norm: the loss does not depend on the length of
    (d4, d5), as the decode's atan2(sin, cos) does not; its gradient on the pair is tangential and scales with 1 / sqrt(q), and
    nothing here pulls the length towards 1.  For w = h the covariance is isotropic and the angle gradient vanishes: a square box
    is not charged for an angle nobody can see.  The arithmetic runs in pred's dtype (float64 in: the tests' ground truth)."""
    if kind not in ROTATED_BOX_LOSS_KINDS:
        raise ValueError("rotated_box_loss: kind must be 'probiou' or 'kld', not {!r}".format(kind))
    sizes = torch.as_tensor(anchor_sizes, dtype=pred.dtype, device=pred.device)
    aw, ah = sizes[:, 0].view(1, -1, 1, 1), sizes[:, 1].view(1, -1, 1, 1)

    def gauss(d, clip):
        lw, lh = (d[:, :, 2].clamp(max=BBOX_XFORM_CLIP), d[:, :, 3].clamp(max=BBOX_XFORM_CLIP)) if clip else (d[:, :, 2], d[:, :, 3])
        w, h = lw.exp() * aw, lh.exp() * ah
        q = d[:, :, 4] * d[:, :, 4] + d[:, :, 5] * d[:, :, 5] + ROTATED_DIRECTION_EPS
        cc, ss, sc = d[:, :, 5] * d[:, :, 5] / q, d[:, :, 4] * d[:, :, 4] / q, d[:, :, 4] * d[:, :, 5] / q
        w2, h2 = w * w, h * h
        return d[:, :, 0] * aw, d[:, :, 1] * ah, w, h, (w2 * cc + h2 * ss) / 12, (w2 * ss + h2 * cc) / 12, -(w2 - h2) * sc / 12, lw, lh

    pcx, pcy, pw, ph, a1, b1, c1, plw, plh = gauss(pred, True)
    tcx, tcy, tw, th, a2, b2, c2, tlw, tlh = gauss(target.to(pred.dtype), False)
    dx, dy = pcx - tcx, pcy - tcy
    if kind == 'probiou':
        A, B, C = a1 + a2, b1 + b2, c1 + c2
        D = A * B - C * C
        distance = (B * dx * dx + A * dy * dy - 2 * C * dx * dy) / (4 * D) + 0.5 * torch.log(36 * D / (pw * ph * tw * th))
        return torch.sqrt(1 - torch.exp(-distance.clamp(min=0, max=PROBIOU_MAX_DISTANCE)) + PROBIOU_EPS)
    sd = tw * th / 12
    inv = 1 / (sd * sd)
    trace = b2 * a1 + a2 * b1 - 2 * c2 * c1
    mahalanobis = b2 * dx * dx + a2 * dy * dy - 2 * c2 * dx * dy
    divergence = 0.5 * (trace * inv + mahalanobis * inv - 2) + (tlw + tlh - plw - plh)
    return 1 - 1 / (1 + torch.log1p(divergence.clamp(min=0)))


CLS_LOSS_KINDS = ('qfl', 'vfl')


def box_quality(pred, target, anchor_sizes):
    """The localisation quality the class score is trained towards under `Model.cls_loss = 'qfl' | 'vfl'`: the IoU of the boxes that
    predicted and target deltas decode to, as `1 - box_iou_loss(pred, target, anchor_sizes, 'iou')` -- the same clip, eps and
    decoding; [B, A, 4, H, W] twice -> [B, A, H, W] in [0, 1] (identical boxes: within a few ulp of 1; it is not clamped, so that it
    stays the box loss's own number), NaN where a delta is NaN.  Meaningful at foreground anchors only."""
    return 1 - box_iou_loss(pred, target, anchor_sizes, 'iou')


def quality_target(depth, quality, classes):
    """The soft class target y of the eager path: depth [B, A, 1, H, W] (-1 ignore / 0 background / class + 1), quality
    [B, A, H, W] -> [B, A, classes, H, W] with y = quality where depth - 1 == class and 0 everywhere else."""
    cls_index = torch.arange(classes, device=depth.device, dtype=depth.dtype).view(1, 1, -1, 1, 1)
    return torch.where(depth - 1 == cls_index, quality.unsqueeze(2), torch.zeros((), dtype=quality.dtype, device=quality.device))


def _softplus(x):
    """log(1 + exp(x)) without overflow, 0 at -inf, with sigmoid(x) as its gradient (F.softplus switches to x beyond a threshold,
    2e-9 off in float64)."""
    return torch.logaddexp(x, torch.zeros_like(x))


def quality_focal_loss(logits, quality_target, gamma=2.0):
    """Quality Focal Loss (GFL, arXiv 2006.04388, eq. 4), per element: |sigmoid(x) - y|^gamma (softplus(x) - y x), the binary cross
    entropy against the soft target y in [0, 1] scaled by the distance to it; gamma >= 1.  For y = 0 it is sigmoid(x)^gamma
    softplus(x) (y x counts as 0 there even for an infinite logit); for y in {0, 1} twice `focal_loss` with alpha = 0.5.  The arithmetic runs in the logits' dtype."""
    y = quality_target.to(logits.dtype)
    yx = torch.where(y == 0, torch.zeros((), dtype=logits.dtype, device=logits.device), y * logits)      # 0 * -inf is 0 here
    return (torch.sigmoid(logits) - y).abs() ** gamma * (_softplus(logits) - yx)


def varifocal_loss(logits, quality_target, alpha=0.75, gamma=2.0):
    """Varifocal Loss (VarifocalNet, arXiv 2008.13367, eq. 2, as mmdetection implements it), per element: y (softplus(x) - y x)
    where y > 0, the focal negative term alpha sigmoid(x)^gamma softplus(x) where y <= 0 (also a foreground anchor whose predicted
    box misses its target entirely).  A NaN y takes the first form, so it reaches the sum.  The arithmetic runs in the logits' dtype."""
    y = quality_target.to(logits.dtype)
    softplus = _softplus(logits)
    return torch.where(y <= 0, alpha * torch.sigmoid(logits) ** gamma * softplus, y * (softplus - y * logits))


class FocalLoss(nn.Module):
    def __init__(self, alpha=0.25, gamma=2):
        super().__init__()
        self.alpha, self.gamma = alpha, gamma

    def forward(self, pred_logits, target):
        return focal_loss(pred_logits, target, self.alpha, self.gamma)


class SmoothL1Loss(nn.Module):
    def __init__(self, beta=0.11):
        super().__init__()
        self.beta = beta

    def forward(self, pred, target):
        return smooth_l1_loss(pred, target, self.beta)


class _FusedLevelLoss(torch.autograd.Function):
    """(cls_head, box_head) -> (cls_sum, box_sum, foreground) for one pyramid level of the batch."""

    @staticmethod
    def forward(ctx, cls_head, box_head, depth, box_target, alpha, gamma, beta):
        from . import _C
        sums = _C.retina_loss_forward(cls_head, box_head, depth, box_target, alpha, gamma, beta)
        ctx.save_for_backward(cls_head, box_head, depth, box_target)
        ctx.hyper = (alpha, gamma, beta)
        out = sums.float()
        foreground = out[2]
        ctx.mark_non_differentiable(foreground)
        return out[0], out[1], foreground

    @staticmethod
    def backward(ctx, grad_cls_sum, grad_box_sum, _grad_foreground):
        from . import _C
        cls_head, box_head, depth, box_target = ctx.saved_tensors
        dcls, dbox = _C.retina_loss_backward(cls_head, box_head, depth, box_target, *ctx.hyper, grad_cls_sum, grad_box_sum)
        return dcls, dbox, None, None, None, None, None


def _as_written(t):
    return t if (t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)) else t.contiguous()


def _as_written_pair(cls_head, box_head):
    """Head tensors go to the kernels as the convolutions wrote them; anything exotic is normalised once."""
    pair = [_as_written(cls_head), _as_written(box_head)]
    if pair[0].is_contiguous() != pair[1].is_contiguous() and pair[0].shape[2] * pair[0].shape[3] > 1:
        pair[1] = pair[1].contiguous() if pair[0].is_contiguous() else pair[1].contiguous(memory_format=torch.channels_last)
    if pair[1].dtype != pair[0].dtype:
        pair[1] = pair[1].to(pair[0].dtype)
    return pair


def _in_level_groups(fn, lists, *rest):
    """One launch covers _C.MAX_LEVELS levels (several backbones: 5 levels each) and no loss has state across levels: for more,
    `fn(*lists, *rest)` on slices of the per-level lists, the per-level results concatenated.  None where one call covers them."""
    from . import _C
    m = _C.MAX_LEVELS
    if len(lists[0]) <= m:
        return None
    groups = [fn(*[per_level[i:i + m] for per_level in lists], *rest) for i in range(0, len(lists[0]), m)]
    return tuple(torch.cat(parts) for parts in zip(*groups))


def _anchor_tables(anchors_list, pairs=False):
    """Per level the [A, 4] anchor table as a tuple of floats: what an autograd node keeps instead of tensors.  pairs: a level may
    be the (axis, rotated) pair of generate_anchors_rotated, of which the axis table counts."""
    if pairs:
        anchors_list = [a[0] if isinstance(a, (tuple, list)) and len(a) == 2 and isinstance(a[0], torch.Tensor) else a for a in anchors_list]
    return tuple(tuple(float(v) for v in torch.as_tensor(a).reshape(-1).tolist()) for a in anchors_list)


class _FusedPyramidLoss(torch.autograd.Function):
    """(cls_heads..., box_heads...) of ALL levels -> (cls_sums [L], box_sums [L], foreground [L]); one launch each way."""

    @staticmethod
    def forward(ctx, n, alpha, gamma, beta, *tensors):
        from . import _C
        cls_heads, box_heads = tensors[:n], tensors[n:2 * n]
        depths, box_targets = tensors[2 * n:3 * n], tensors[3 * n:4 * n]
        # Through the workspace (per-workgroup sums, added up in a fixed order by a second, tiny launch; csrc/loss.hpp:
        # loss_reduce_kernel): no double atomics at the end of every workgroup -- the walk takes 25-27 us where the atomics
        # form takes 31-35, the reduce launch 4 (profiles/r06_loss_layout_probe.txt) -- and the loss is the same bits on every
        # run.
        sums = _C.retina_loss_levels_forward(cls_heads, box_heads, depths, box_targets, alpha, gamma, beta,
                                             reproducible=True).float()
        ctx.save_for_backward(*tensors)
        ctx.meta = (n, alpha, gamma, beta)
        cls_sums, box_sums, foreground = sums[:, 0].contiguous(), sums[:, 1].contiguous(), sums[:, 2].contiguous()
        ctx.mark_non_differentiable(foreground)
        return cls_sums, box_sums, foreground

    @staticmethod
    def backward(ctx, grad_cls_sums, grad_box_sums, _grad_foreground):
        from . import _C
        n, alpha, gamma, beta = ctx.meta
        t = ctx.saved_tensors
        dcls, dbox = _C.retina_loss_levels_backward(t[:n], t[n:2 * n], t[2 * n:3 * n], t[3 * n:4 * n], alpha, gamma, beta,
                                                    grad_cls_sums, grad_box_sums)
        return (None, None, None, None) + tuple(dcls) + tuple(dbox) + (None,) * (2 * n)


def fused_pyramid_loss(cls_heads, box_heads, depths, box_targets, alpha=0.25, gamma=2.0, beta=0.11):
    """`fused_level_loss` for every pyramid level at once: per-level (cls_sums [L], box_sums [L], foreground [L]) from ONE
    HIP launch forward and ONE backward (a training step: two launches where the per-level form needs ten)."""
    split = _in_level_groups(fused_pyramid_loss, (cls_heads, box_heads, depths, box_targets), alpha, gamma, beta)
    if split is not None:
        return split
    pairs = [_as_written_pair(c, b) for c, b in zip(cls_heads, box_heads)]
    n = len(pairs)
    return _FusedPyramidLoss.apply(n, alpha, gamma, beta, *[p[0] for p in pairs], *[p[1] for p in pairs],
                                   *[d.contiguous() for d in depths], *[t.contiguous() for t in box_targets])


def fused_level_loss(cls_head, box_head, depth, box_target, alpha=0.25, gamma=2.0, beta=0.11):
    """One level's (sum of masked focal losses, sum of masked smooth-L1 losses, number of foreground anchors).

    cls_head [B, A*C, H, W] logits and box_head [B, A*nb, H, W] as the convolutions wrote them (float32 /
    bfloat16 / float16, NCHW or channels_last -- no .float(), no .contiguous()); depth [B, A, 1, H, W] and
    box_target [B, A, nb, H, W] float32 from target assignment.  Equals, and differentiates like,

        cls = FocalLoss(alpha, gamma)(cls_head.view(B, A, C, H, W).float(), onehot(depth - 1))
        (cls * (depth >= 0)).sum(), (SmoothL1Loss(beta)(box_head.view_as(box_target).float(), box_target)
                                     * (depth > 0)).sum(), (depth > 0).sum()"""
    pair = _as_written_pair(cls_head, box_head)
    return _FusedLevelLoss.apply(pair[0], pair[1], depth.contiguous(), box_target.contiguous(), alpha, gamma, beta)


class _FusedPyramidPairLoss(torch.autograd.Function):
    """The per-cell losses of csrc/cell_loss.hpp: (heads..., depths..., box_targets...) of ALL levels -> (sums [L], foreground [L]);
    two launches forward (walk + fixed-order sum), one backward.  `forward_fn` / `backward_fn`: the pair of odtk._C functions;
    `tensors`: `groups` per-level lists of n tensors each, in the order the functions take them, followed there by `anchors_list`
    and `hyper`; list `grad_group` (the heads the loss is a function of) receives the gradient."""

    @staticmethod
    def forward(ctx, forward_fn, backward_fn, groups, grad_group, hyper, anchors_list, *tensors):
        n = len(tensors) // groups
        sums = forward_fn(*[tensors[k * n:(k + 1) * n] for k in range(groups)], anchors_list, *hyper).float()
        ctx.save_for_backward(*tensors)
        ctx.meta = (backward_fn, groups, grad_group, hyper, anchors_list)
        loss_sums, foreground = sums[:, 0].contiguous(), sums[:, 1].contiguous()
        ctx.mark_non_differentiable(foreground)
        return loss_sums, foreground

    @staticmethod
    def backward(ctx, grad_sums, _grad_foreground):
        backward_fn, groups, grad_group, hyper, anchors_list = ctx.meta
        t = ctx.saved_tensors
        n = len(t) // groups
        grads = backward_fn(*[t[k * n:(k + 1) * n] for k in range(groups)], anchors_list, *hyper, grad_sums)
        return (None,) * (6 + grad_group * n) + tuple(grads) + (None,) * ((groups - 1 - grad_group) * n)


def fused_pyramid_box_iou_loss(box_heads, depths, box_targets, anchors_list, kind):
    """`box_iou_loss` masked by `depth > 0` and summed, for every pyramid level at once: per-level (box_sums [L], foreground [L])
    from the HIP pass of csrc/box_iou_loss.hpp.  box_heads [B, A*4, H, W] as the convolutions wrote them (float32 / bfloat16 /
    float16, NCHW or channels_last); depths [B, A, 1, H, W] and box_targets [B, A, 4, H, W] float32 from target assignment;
    anchors_list: per level the [A, 4] anchor table.  Equals, and differentiates like, per level

        (box_iou_loss(box_head.view_as(box_target).float(), box_target, anchor_wh(anchors), kind) * (depth[:, :, 0] > 0)).sum()"""
    from . import _C
    if kind not in BOX_LOSS_KINDS:
        raise ValueError("fused_pyramid_box_iou_loss: kind must be 'iou', 'giou' or 'diou', not {!r}".format(kind))
    split = _in_level_groups(fused_pyramid_box_iou_loss, (box_heads, depths, box_targets, anchors_list), kind)
    if split is not None:
        return split
    return _FusedPyramidPairLoss.apply(_C.box_iou_loss_levels_forward, _C.box_iou_loss_levels_backward, 3, 0, (kind,),
                                       _anchor_tables(anchors_list), *[_as_written(t) for t in box_heads],
                                       *[d.contiguous() for d in depths], *[t.contiguous() for t in box_targets])


def fused_pyramid_rotated_box_loss(box_heads, depths, box_targets, anchors_list, kind):
    """`rotated_box_loss` masked by `depth > 0` and summed, for every pyramid level at once: per-level (box_sums [L], foreground
    [L]) from the HIP pass of csrc/rotated_box_loss.hpp.  box_heads [B, A*6, H, W] as the convolutions wrote them (float32 /
    bfloat16 / float16, NCHW or channels_last); depths [B, A, 1, H, W] and box_targets [B, A, 6, H, W] float32 from rotated target
    assignment; anchors_list: per level the AXIS table [A, 4] -- the [0] of the (axis, rotated) pair of generate_anchors_rotated;
    the pair itself is accepted too.  Equals, and differentiates like, per level

        (rotated_box_loss(box_head.view_as(box_target).float(), box_target, anchor_wh(axis), kind) * (depth[:, :, 0] > 0)).sum()

    The gradient on a level's (sin, cos) pair is tangential (see `rotated_box_loss`): the loss never changes the pair's length."""
    from . import _C
    if kind not in ROTATED_BOX_LOSS_KINDS:
        raise ValueError("fused_pyramid_rotated_box_loss: kind must be 'probiou' or 'kld', not {!r}".format(kind))
    split = _in_level_groups(fused_pyramid_rotated_box_loss, (box_heads, depths, box_targets, anchors_list), kind)
    if split is not None:
        return split
    return _FusedPyramidPairLoss.apply(_C.rotated_box_loss_levels_forward, _C.rotated_box_loss_levels_backward, 3, 0, (kind,),
                                       _anchor_tables(anchors_list, pairs=True), *[_as_written(t) for t in box_heads],
                                       *[d.contiguous() for d in depths], *[t.contiguous() for t in box_targets])


def fused_pyramid_quality_loss(cls_heads, box_heads, depths, box_targets, anchors_list, kind, alpha=0.75, gamma=2.0):
    """`quality_focal_loss` ('qfl') or `varifocal_loss` ('vfl') against the soft target, masked by `depth >= 0` and summed, for every
    pyramid level at once: per-level (cls_sums [L], foreground [L]) from the HIP pass of csrc/quality_loss.hpp.  cls_heads
    [B, A*C, H, W] and box_heads [B, A*4, H, W] as the convolutions wrote them (float32 / bfloat16 / float16, NCHW or channels_last);
    depths [B, A, 1, H, W] and box_targets [B, A, 4, H, W] float32 from target assignment; anchors_list: per level the [A, 4] anchor
    table.  `alpha` is varifocal's only.  Equals, and differentiates like, per level

        q = box_quality(box_head.view_as(box_target).float(), box_target, anchor_wh(anchors)).detach()
        (loss(cls_head.view(B, A, C, H, W).float(), quality_target(depth, q, C)) * (depth >= 0)).sum(), (depth > 0).sum()

    with no gradient into the box heads; neither the quality map nor the target is ever built."""
    from . import _C
    if kind not in CLS_LOSS_KINDS:
        raise ValueError("fused_pyramid_quality_loss: kind must be 'qfl' or 'vfl', not {!r}".format(kind))
    split = _in_level_groups(fused_pyramid_quality_loss, (cls_heads, box_heads, depths, box_targets, anchors_list), kind, alpha, gamma)
    if split is not None:
        return split
    pairs = [_as_written_pair(c, b.detach()) for c, b in zip(cls_heads, box_heads)]
    return _FusedPyramidPairLoss.apply(_C.quality_loss_levels_forward, _C.quality_loss_levels_backward, 4, 0,
                                       (kind, float(alpha), float(gamma)), _anchor_tables(anchors_list), *[p[0] for p in pairs],
                                       *[p[1] for p in pairs], *[d.contiguous() for d in depths], *[t.contiguous() for t in box_targets])
