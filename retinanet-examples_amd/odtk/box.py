"""odtk.box -- Python surface of the per-anchor post-processing path, MI355X edition.

Same function names, argument order and return conventions as the reference's odtk/box.py
(generate_anchors :8, generate_anchors_rotated :23, box2delta :67, delta2box :97, decode :255,
nms :312, nms_rotated :370), so `odtk.model.Model.forward` and user code keep calling
`decode(cls, box, stride, threshold, top_n, anchors, rotated)` and `nms(scores, boxes, classes,
nms, ndetections)` unchanged.

Differences, all deliberate:
  * GPU tensors ALWAYS run the hand-written HIP kernels (libodtk_hip.so via odtk._C); a missing
    library raises, nothing falls back silently.
  * CPU tensors take the pure-torch branch below (`_decode_cpu`, `_nms_cpu`) -- the reference's own
    "no GPU" plumbing path (box.py:266-309, :319-367; BASELINE config 0), with the integer divisions
    written as floor divisions (the reference's `/` on index tensors broke with torch >= 1.5) and the
    canonical tie order (stable sorts).  The reference dispatches on `torch.cuda.is_available()`;
    here the tensor's device decides.  Rotated boxes have no CPU path (the reference's is dead code:
    box.py:408 calls an undefined `iou`).
  * `decode_levels` / `detect` are additions: all pyramid levels x the whole batch in one
    enqueue, with no host synchronisation (GPU only).
  * `atss_assign_levels` is an addition: ATSS target assignment next to the reference's fixed-IoU
    `snap_to_anchors` (HIP kernels for GPU tensors, pure torch otherwise).
  * `tal_assign_levels` is an addition as well: task-aligned target assignment (TOOD), which ranks a box's candidate anchors by
    what the network predicts at them (HIP kernels for GPU tensors, pure torch otherwise).
"""

import math

import torch

from . import _C


def _grid_of_shapes(ratio_vals, scales_vals):
    """(scale, ratio) pairs in the reference's order: scale-major, ratio-minor (box.py:11-13)."""
    scales = torch.tensor([s for s in scales_vals for _ in ratio_vals], dtype=torch.float32).view(-1, 1)
    ratios = torch.tensor([r for _ in scales_vals for r in ratio_vals], dtype=torch.float32)
    return scales, ratios


def generate_anchors(stride, ratio_vals, scales_vals, angles_vals=None):
    """Base anchors [A, 4] = [x1, y1, x2, y2] around one stride x stride cell (reference box.py:8-20)."""
    scales, ratios = _grid_of_shapes(ratio_vals, scales_vals)
    cell = torch.full((ratios.numel(), 2), float(stride), dtype=torch.float32)
    side = torch.sqrt(cell[:, 0] * cell[:, 1] / ratios)
    extent = torch.stack([side, side * ratios], dim=1) * scales
    return torch.cat([0.5 * (cell - extent), 0.5 * (cell + extent)], dim=1)


def _order_quads(quads):
    """[Q, 4, 2] corner sets -> [tl, tr, br, bl] per quad (reference utils.py:15-31), batched."""
    by_x = torch.gather(quads, 1, torch.argsort(quads[:, :, 0], dim=1)[:, :, None].expand(-1, -1, 2))
    left, right = by_x[:, :2], by_x[:, 2:]
    left = torch.gather(left, 1, torch.argsort(left[:, :, 1], dim=1)[:, :, None].expand(-1, -1, 2))
    tl, bl = left[:, 0], left[:, 1]
    dist = torch.cdist(tl[:, None, :], right)[:, 0]                       # [Q, 2]
    far_first = torch.argsort(dist, dim=1, descending=True)
    right = torch.gather(right, 1, far_first[:, :, None].expand(-1, -1, 2))
    br, tr = right[:, 0], right[:, 1]
    return torch.stack([tl, tr, br, bl], dim=1)


def generate_anchors_rotated(stride, ratio_vals, scales_vals, angles_vals):
    """(axis-aligned [A, 4], rotated corner [A, 8]) anchors, angle-major (reference box.py:23-64).
    decode only consumes [0] (box.py:258-259); [1] feeds rotated target assignment."""
    scales, ratios = _grid_of_shapes(ratio_vals, scales_vals)
    n_shapes = ratios.numel()
    cell = torch.full((n_shapes, 2), float(stride), dtype=torch.float32)
    side = torch.round(torch.sqrt(cell[:, 0] * cell[:, 1] / ratios))
    extent = torch.stack([side, torch.round(side * ratios)], dim=1) * scales
    p0 = 0.5 * (cell - extent)
    p2 = 0.5 * (cell + extent) - 1
    span = p2 - p0
    p1 = p0 + span * torch.tensor([0.0, 1.0])
    p3 = p0 + span * torch.tensor([1.0, 0.0])

    angles = torch.tensor(angles_vals, dtype=torch.float32)
    n_ang = angles.numel()
    rot = torch.stack([torch.stack([torch.cos(angles), torch.sin(angles)], dim=1),
                       torch.stack([-torch.sin(angles), torch.cos(angles)], dim=1)], dim=1)   # [n_ang, 2, 2]
    half = stride / 2

    def spin(p):   # rotate about the cell centre (box.py:50-53), result [n_ang * n_shapes, 2]
        r = torch.matmul(rot, p.transpose(1, 0) - half + 0.5) + half - 0.5
        return r.permute(0, 2, 1).contiguous().view(-1, 2)

    axis = torch.cat([p0.repeat(n_ang, 1), p2.repeat(n_ang, 1)], dim=1)
    corners = _order_quads(torch.stack([spin(p0), spin(p1), spin(p2), spin(p3)], dim=1)).view(-1, 8)
    return axis, corners


def _split_anchor(anchors):
    size = anchors[:, 2:4] - anchors[:, :2] + 1
    return size, anchors[:, :2] + 0.5 * size


def box2delta(boxes, anchors):
    """Regression targets of `boxes` w.r.t. `anchors` (+1 pixel convention; reference box.py:67-78)."""
    a_size, a_ctr = _split_anchor(anchors)
    b_size, b_ctr = _split_anchor(boxes)
    return torch.cat([(b_ctr - a_ctr) / a_size, torch.log(b_size / a_size)], 1)


def box2delta_rotated(boxes, anchors):
    """As box2delta plus pass-through (sin, cos) columns (reference box.py:81-94)."""
    return torch.cat([box2delta(boxes[:, :4], anchors[:, :4]), boxes[:, 4:6]], 1)


def delta2box(deltas, anchors, size, stride):
    """Inverse of box2delta with the two-sided clamp to [0, size*stride-1] (reference box.py:97-111).
    Pure torch; the inference path does this inside the HIP decode kernel instead."""
    a_size, a_ctr = _split_anchor(anchors)
    ctr = deltas[:, :2] * a_size + a_ctr
    ext = torch.exp(deltas[:, 2:4]) * a_size
    upper = torch.tensor([size], device=deltas.device, dtype=deltas.dtype) * stride - 1
    lower = torch.zeros(2, device=deltas.device, dtype=deltas.dtype)
    lo = torch.max(lower, torch.min(ctr - 0.5 * ext, upper))
    hi = torch.max(lower, torch.min(ctr + 0.5 * ext - 1, upper))
    return torch.cat([lo, hi], 1)


def delta2box_rotated(deltas, anchors, size, stride):
    """delta2box + theta = atan2(sin, cos) (reference box.py:114-131)."""
    return torch.cat([delta2box(deltas[:, :4], anchors[:, :4], size, stride),
                      torch.atan2(deltas[:, 4], deltas[:, 5])[:, None]], 1)


def _cell_anchors(anchors, size, stride, dtype, device):
    """All anchors of a level in (anchor, y, x) order, [A*H*W, K] (K = 4 corners or 8 quad coords)."""
    xs = torch.arange(0, size[0], stride, device=device, dtype=dtype)
    ys = torch.arange(0, size[1], stride, device=device, dtype=dtype)
    gy, gx = torch.meshgrid(ys, xs, indexing='ij')
    k = anchors.shape[1]
    grid = torch.stack([gx, gy] * (k // 2), 2).unsqueeze(0)                       # [1, H, W, K]
    return (grid + anchors.view(-1, 1, 1, k).to(device=device, dtype=dtype)).reshape(-1, k)


def _targets_from_overlap(overlap, boxes_xyxy, classes, cell, num_anchors, height, width, num_classes, anchor_ious,
                          to_delta):
    """Shared tail of snap_to_anchors[_rotated] (reference box.py:165-189 / :228-252): best box per
    anchor -> regression target, depth (-1 ignore / 0 background / class+1) and one-hot class target,
    produced directly in [A, *, H, W] order."""
    overlap, best = overlap.max(1)
    box_target = to_delta(boxes_xyxy[best], cell)
    nb = box_target.shape[1]
    box_target = box_target.view(num_anchors, height, width, nb).permute(0, 3, 1, 2).contiguous()
    background = overlap < anchor_ious[0]
    foreground = overlap >= anchor_ious[1]
    best_cls = classes[best].view(-1)
    depth = torch.full_like(overlap, -1)
    depth[background] = 0
    depth[foreground] = best_cls[foreground] + 1
    onehot_idx = best_cls.long()
    onehot_idx[background] = num_classes                                          # background has no class
    cls_target = torch.zeros((cell.shape[0], num_classes + 1), device=overlap.device, dtype=boxes_xyxy.dtype)
    cls_target.scatter_(1, onehot_idx.view(-1, 1), 1)
    cls_target = cls_target[:, :num_classes].view(num_anchors, height, width, num_classes).permute(0, 3, 1, 2)
    return cls_target.contiguous(), box_target, depth.view(num_anchors, 1, height, width)


def snap_to_anchors(boxes, size, stride, anchors, num_classes, device, anchor_ious):
    """Training targets for one image and one pyramid level (reference box.py:134-189).

    boxes [N, 5] = (x, y, w, h, class); size = [W*stride, H*stride].  Returns
    cls_target [A, C, H, W], box_target [A, 4, H, W], depth [A, 1, H, W].  Pure torch like the
    reference's (which has no native op here) and device-agnostic; per-anchor values equal the
    reference's (it builds [A, W, H] and transposes, which changes no value)."""
    num_anchors = anchors.shape[0]
    width, height = int(size[0] / stride), int(size[1] / stride)
    if boxes.nelement() == 0:
        return (torch.zeros([num_anchors, num_classes, height, width], device=device),
                torch.zeros([num_anchors, 4, height, width], device=device),
                torch.zeros([num_anchors, 1, height, width], device=device))
    boxes, classes = boxes.split(4, dim=1)
    cell = _cell_anchors(anchors, size, stride, classes.dtype, device)
    xyxy = torch.cat([boxes[:, :2], boxes[:, :2] + boxes[:, 2:] - 1], 1)
    lo = torch.max(cell[:, None, :2], xyxy[:, :2])
    hi = torch.min(cell[:, None, 2:], xyxy[:, 2:])
    inter = torch.prod((hi - lo + 1).clamp(0), 2)
    area_b = torch.prod(xyxy[:, 2:] - xyxy[:, :2] + 1, 1)
    area_a = torch.prod(cell[:, 2:] - cell[:, :2] + 1, 1)
    overlap = inter / (area_a[:, None] + area_b - inter)
    return _targets_from_overlap(overlap, xyxy, classes, cell, num_anchors, height, width, num_classes, anchor_ious,
                                 box2delta)


def snap_to_anchors_batched(targets, width, height, stride, anchors, num_classes, anchor_ious, want_cls_target=True):
    """snap_to_anchors for every image of the batch in ONE fused HIP launch (GPU only).
    targets [B, N, 5] padded with class = -1 rows (reference data.py:154-161 format).
    Returns the stacked (cls_target [B,A,C,H,W], box_target [B,A,4,H,W], depth [B,A,1,H,W])."""
    _require_gpu(targets, 'snap_to_anchors_batched')
    return _C.snap_to_anchors(targets.float().contiguous(), anchors, num_classes, int(height), int(width),
                              int(stride), anchor_ious[0], anchor_ious[1], want_cls_target)


MAX_LEVELS_PER_CALL = _C.MAX_LEVELS


def snap_to_anchors_levels(targets, sizes, strides, anchors_list, num_classes, anchor_ious, want_cls_target=True):
    """snap_to_anchors_batched for every pyramid level in ONE fused HIP launch (GPU only; csrc/targets.hpp).
    sizes: per level (H, W) of the head tensors; -> lists (cls_targets | Nones, box_targets, depths)."""
    _require_gpu(targets, 'snap_to_anchors_levels')
    return _C.snap_to_anchors_levels(targets.float().contiguous(), anchors_list, num_classes, [(int(h), int(w)) for h, w in sizes],
                                     [int(s) for s in strides], anchor_ious[0], anchor_ious[1], want_cls_target)


def _atss_image(boxes, sizes, strides, anchors_list, num_classes, topk, want_cls_target):
    """ATSS for the valid rows [N, 5] of one image, pure torch, in the steps of csrc/atss.hpp -> per level (cls, box, depth)."""
    dev = boxes.device
    n = boxes.shape[0]
    if n == 0:
        return [(boxes.new_zeros((anchors.shape[0], num_classes, h, w)) if want_cls_target else None,
                 boxes.new_zeros((anchors.shape[0], 4, h, w)), boxes.new_zeros((anchors.shape[0], 1, h, w)))
                for (h, w), anchors in zip(sizes, anchors_list)]
    xy1 = boxes[:, :2]
    xy2 = boxes[:, :2] + boxes[:, 2:4] - 1
    xyxy = torch.cat([xy1, xy2], 1)
    b_size = xy2 - xy1 + 1
    b_area = b_size[:, 0] * b_size[:, 1]
    b_ctr = xy1 + 0.5 * b_size
    classes = boxes[:, 4]
    margin = torch.tensor(0.01, dtype=torch.float32, device=dev)

    # 1. candidates: per level the nearest cells (a stable ascending sort: ties to the lower cell, NaN last), all their anchors
    levels = []
    for (h, w), s, anchors in zip(sizes, strides, anchors_list):
        s = float(s)
        anchors = anchors.to(device=dev, dtype=torch.float32)
        px = torch.arange(w, device=dev, dtype=torch.float32) * s + 0.5 * s + 0.5
        py = torch.arange(h, device=dev, dtype=torch.float32) * s + 0.5 * s + 0.5
        dx, dy = px[None, :] - b_ctr[:, 0:1], py[None, :] - b_ctr[:, 1:2]
        d2 = ((dx * dx)[:, None, :] + (dy * dy)[:, :, None]).reshape(n, h * w)
        near, cells = torch.sort(d2, dim=1, stable=True)
        near, cells = near[:, :min(topk, h * w)], cells[:, :min(topk, h * w)]
        yc, xc = torch.div(cells, w, rounding_mode='floor'), cells % w
        gx, gy = xc.float() * s, yc.float() * s
        a1x, a1y = gx[:, :, None] + anchors[:, 0], gy[:, :, None] + anchors[:, 1]                    # [N, k, A]
        a2x, a2y = gx[:, :, None] + anchors[:, 2], gy[:, :, None] + anchors[:, 3]
        a_area = (a2x - a1x + 1) * (a2y - a1y + 1)
        iw = (torch.min(a2x, xy2[:, 0, None, None]) - torch.max(a1x, xy1[:, 0, None, None]) + 1).clamp(min=0)
        ih = (torch.min(a2y, xy2[:, 1, None, None]) - torch.max(a1y, xy1[:, 1, None, None]) + 1).clamp(min=0)
        inter = iw * ih
        iou = inter / (a_area + b_area[:, None, None] - inter)
        cx, cy = px[xc], py[yc]
        inside = ((cx - xy1[:, 0:1] > margin) & (cy - xy1[:, 1:2] > margin) &
                  (xy2[:, 0:1] - cx > margin) & (xy2[:, 1:2] - cy > margin))                       # [N, k]
        levels.append((cells, ~torch.isnan(near), iou, inside))

    # 2. threshold: float64 mean and sample deviation of the listed IoUs, summed one after the other in list order
    a = anchors_list[0].shape[0]
    listed = torch.cat([iou.reshape(n, -1) for _, _, iou, _ in levels], 1).double()
    chosen = torch.cat([ok[:, :, None].expand(-1, -1, a).reshape(n, -1) for _, ok, _, _ in levels], 1)
    count = chosen.sum(1)
    total = torch.zeros(n, dtype=torch.float64, device=dev)
    for i in range(listed.shape[1]):
        total = torch.where(chosen[:, i], total + listed[:, i], total)
    mean = total / count.double()
    squares = torch.zeros(n, dtype=torch.float64, device=dev)
    for i in range(listed.shape[1]):
        d = listed[:, i] - mean
        squares = torch.where(chosen[:, i], squares + d * d, squares)
    var = torch.where(count > 1, squares / (count - 1).double(), torch.zeros_like(squares))
    thresh = torch.where(count > 0, mean + torch.sqrt(var), torch.full_like(mean, float('nan')))

    out = []
    for (h, w), s, anchors, (cells, ok, iou, inside) in zip(sizes, strides, anchors_list, levels):
        # 3. positives; 4. an anchor goes to the largest IoU, the earliest box on a tie
        positive = (iou.double() >= thresh[:, None, None]) & (ok & inside)[:, :, None]            # [N, k, A]
        flat = cells[:, :, None] + torch.arange(a, device=dev)[None, None, :] * (h * w)            # index into [A, H, W]
        owner = torch.full((a * h * w,), -1, dtype=torch.long, device=dev)
        best = torch.zeros(a * h * w, dtype=torch.float32, device=dev)
        for g in range(n):
            idx, ov = flat[g][positive[g]], iou[g][positive[g]]
            take = (owner[idx] < 0) | (ov > best[idx])
            owner[idx[take]] = g
            best[idx[take]] = ov[take]
        # 5. outputs in [A, *, H, W] order
        hit = (owner >= 0).nonzero().view(-1)
        box_target = torch.zeros((a * h * w, 4), dtype=torch.float32, device=dev)
        depth = torch.zeros(a * h * w, dtype=torch.float32, device=dev)
        if hit.numel():
            cell = _cell_anchors(anchors, [w * float(s), h * float(s)], float(s), torch.float32, dev)
            box_target[hit] = box2delta(xyxy[owner[hit]], cell[hit])
            depth[hit] = classes[owner[hit]] + 1
        cls_target = None
        if want_cls_target:
            cls_target = torch.zeros((a * h * w, num_classes + 1), dtype=torch.float32, device=dev)
            if hit.numel():
                label = classes[owner[hit]].long()
                label[(label < 0) | (label >= num_classes)] = num_classes
                cls_target[hit, label] = 1
            cls_target = cls_target[:, :num_classes].view(a, h, w, num_classes).permute(0, 3, 1, 2).contiguous()
        out.append((cls_target, box_target.view(a, h, w, 4).permute(0, 3, 1, 2).contiguous(), depth.view(a, 1, h, w)))
    return out


def atss_assign_levels(targets, sizes, strides, anchors_list, num_classes, topk=9, want_cls_target=True):
    """ATSS target assignment (adaptive training sample selection, Zhang et al., CVPR 2020) for every image and pyramid level:
    the alternative to the fixed-IoU rule of `snap_to_anchors*`, axis-aligned boxes only.  Per box and level the `topk` cells
    whose centres are nearest to the box centre are its candidates, with all their anchors; an IoU of at least the mean + the
    standard deviation of the box's candidates over all levels, and a cell centre inside the box, make a candidate positive; an
    anchor positive for several boxes goes to the largest IoU.  The exact definition is in csrc/atss.hpp.
    A small box may contain no cell centre and then gets no positive anchor at all: that is ATSS.

    targets [B, N, 5] = (x, y, w, h, class), class < 0 rows are padding; sizes: per level (H, W) of the head tensors.
    GPU tensors go to the HIP kernels; any other tensor takes the pure-torch branch, which follows the same definition.
    -> lists (cls_targets [B, A, C, H, W] | Nones, box_targets [B, A, 4, H, W], depths [B, A, 1, H, W]); depth is class + 1
    or 0 (there is no ignore band)."""
    topk = int(topk)
    if not 1 <= topk <= _C.ATSS_MAX_TOPK:
        raise ValueError('atss_assign_levels: topk must be in 1..%d' % _C.ATSS_MAX_TOPK)
    if len(sizes) > MAX_LEVELS_PER_CALL:
        raise ValueError('atss_assign_levels: at most %d levels (the threshold spans all of them, so the call cannot be split)'
                         % MAX_LEVELS_PER_CALL)
    sizes = [(int(h), int(w)) for h, w in sizes]
    targets = targets.float()
    if targets.is_cuda:
        return _C.atss_assign_levels(targets.contiguous(), anchors_list, num_classes, sizes, [int(s) for s in strides], topk,
                                     want_cls_target)
    return _atss_assign_torch(targets, sizes, strides, anchors_list, num_classes, topk, want_cls_target)


def _atss_assign_torch(targets, sizes, strides, anchors_list, num_classes, topk, want_cls_target):
    """The pure-torch branch of atss_assign_levels (any device)."""
    per_image = [_atss_image(t[t[:, -1] > -1], sizes, strides, anchors_list, num_classes, topk, want_cls_target) for t in targets]
    cls_t, box_t, depth_t = [], [], []
    for l, (h, w) in enumerate(sizes):
        a = anchors_list[l].shape[0]
        cls_t.append(torch.stack([img[l][0] for img in per_image]) if want_cls_target and per_image else
                     (targets.new_zeros((0, a, num_classes, h, w)) if want_cls_target else None))
        box_t.append(torch.stack([img[l][1] for img in per_image]) if per_image else targets.new_zeros((0, a, 4, h, w)))
        depth_t.append(torch.stack([img[l][2] for img in per_image]) if per_image else targets.new_zeros((0, a, 1, h, w)))
    return cls_t, box_t, depth_t


def _exp_cr(x):
    """float32 exp rounded once from the double result: csrc/common.hpp exp_cr."""
    return torch.exp(x.double()).float()


def _tal_image(boxes, cls_heads, box_heads, strides, anchors_list, num_classes, topk, alpha, beta, want_cls_target):
    """Task-aligned assignment for the valid rows [N, 5] of one image, pure torch, in the steps of csrc/tal.hpp.  cls_heads /
    box_heads: per level float32 [A * C, H, W] / [A * 4, H, W] -> per level (cls, box, depth)."""
    dev = boxes.device
    n = boxes.shape[0]
    sizes = [tuple(c.shape[-2:]) for c in cls_heads]
    counts = [anchors.shape[0] * h * w for (h, w), anchors in zip(sizes, anchors_list)]
    owner = torch.full((sum(counts),), -1, dtype=torch.long, device=dev)
    xyxy = torch.cat([boxes[:, :2], boxes[:, :2] + boxes[:, 2:4] - 1], 1)
    classes = boxes[:, 4]
    if n:
        x1, y1, x2, y2 = (xyxy[:, i, None, None, None] for i in range(4))                             # [N, 1, 1, 1]
        area = (x2 - x1 + 1) * (y2 - y1 + 1)
        margin = torch.tensor(0.01, dtype=torch.float32, device=dev)
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        metric, overlap, candidate = [], [], []
        for (h, w), s, anchors, cls_head, box_head in zip(sizes, strides, anchors_list, cls_heads, box_heads):
            s = float(s)
            a = anchors.shape[0]
            anchors = anchors.to(device=dev, dtype=torch.float32)
            # 2. candidates: the cell centre more than 0.01 inside the box on all four sides
            px = torch.arange(w, device=dev, dtype=torch.float32) * s + 0.5 * s + 0.5
            py = torch.arange(h, device=dev, dtype=torch.float32) * s + 0.5 * s + 0.5
            inside = ((px[None, None, None, :] - x1 > margin) & (py[None, None, :, None] - y1 > margin) &
                      (x2 - px[None, None, None, :] > margin) & (y2 - py[None, None, :, None] > margin))  # [N, 1, H, W]
            # 3. the score of the row's class
            logit = cls_head.reshape(a, num_classes, h, w)[:, classes.long()].permute(1, 0, 2, 3)       # [N, A, H, W]
            score = 1.0 / (1.0 + _exp_cr(-logit))
            # 4. the predicted box (delta2box without the clamp)
            d = box_head.reshape(a, 4, h, w)
            fx = torch.arange(w, device=dev, dtype=torch.float32)[None, None, :] * s
            fy = torch.arange(h, device=dev, dtype=torch.float32)[None, :, None] * s
            ax1, ay1 = fx + anchors[:, 0, None, None], fy + anchors[:, 1, None, None]                   # [A, 1 | H, W | 1]
            ax2, ay2 = fx + anchors[:, 2, None, None], fy + anchors[:, 3, None, None]
            aw, ah = ax2 - ax1 + 1, ay2 - ay1 + 1
            cx, cy = ax1 + 0.5 * aw, ay1 + 0.5 * ah
            pcx, pcy = d[:, 0] * aw + cx, d[:, 1] * ah + cy
            pw, ph = _exp_cr(d[:, 2]) * aw, _exp_cr(d[:, 3]) * ah
            p1x, p1y, p2x, p2y = pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1
            # 5. the overlap (torch.min / torch.max propagate NaN, like tmin_nan / tmax_nan)
            p_area = (p2x - p1x + 1) * (p2y - p1y + 1)
            iw = torch.min(p2x[None], x2.expand(n, a, h, w)) - torch.max(p1x[None], x1.expand(n, a, h, w)) + 1
            ih = torch.min(p2y[None], y2.expand(n, a, h, w)) - torch.max(p1y[None], y1.expand(n, a, h, w)) + 1
            iw, ih = torch.where(iw < 0, zero, iw), torch.where(ih < 0, zero, ih)
            inter = iw * ih
            u = inter / (p_area[None] + area - inter)
            # 6. the metric
            m = torch.ones_like(u)
            for _ in range(alpha):
                m = m * score
            for _ in range(beta):
                m = m * u
            metric.append(m.reshape(n, -1))
            overlap.append(u.reshape(n, -1))
            candidate.append(inside.expand(n, a, h, w).reshape(n, -1))
        metric, overlap, candidate = torch.cat(metric, 1), torch.cat(overlap, 1), torch.cat(candidate, 1)
        # 7. per row the topk largest metrics (a stable descending sort: ties to the lower global index); NaN never, 0 eligible
        eligible = candidate & ~torch.isnan(metric)
        ranked, order = torch.sort(torch.where(eligible, metric + 0.0, torch.full_like(metric, -1.0)), dim=1, descending=True, stable=True)
        ranked, order = ranked[:, :topk], order[:, :topk]
        # 8. a contested anchor goes to the largest overlap, the earliest row on a tie
        best = torch.zeros(owner.shape[0], dtype=torch.float32, device=dev)
        for g in range(n):
            idx = order[g][ranked[g] >= 0]
            ov = overlap[g][idx]
            take = (owner[idx] < 0) | (ov > best[idx])
            owner[idx[take]] = g
            best[idx[take]] = ov[take]
    # 9. outputs in [A, *, H, W] order
    out, first = [], 0
    for (h, w), s, anchors, count in zip(sizes, strides, anchors_list, counts):
        a = anchors.shape[0]
        mine = owner[first:first + count]
        first += count
        hit = (mine >= 0).nonzero().view(-1)
        box_target = torch.zeros((count, 4), dtype=torch.float32, device=dev)
        depth = torch.zeros(count, dtype=torch.float32, device=dev)
        cls_target = torch.zeros((count, num_classes), dtype=torch.float32, device=dev) if want_cls_target else None
        if hit.numel():
            cell = _cell_anchors(anchors, [w * float(s), h * float(s)], float(s), torch.float32, dev)
            box_target[hit] = box2delta(xyxy[mine[hit]], cell[hit])
            depth[hit] = classes[mine[hit]] + 1
            if want_cls_target:
                cls_target[hit, classes[mine[hit]].long()] = 1
        if want_cls_target:
            cls_target = cls_target.view(a, h, w, num_classes).permute(0, 3, 1, 2).contiguous()
        out.append((cls_target, box_target.view(a, h, w, 4).permute(0, 3, 1, 2).contiguous(), depth.view(a, 1, h, w)))
    return out


def tal_assign_levels(targets, cls_heads, box_heads, strides, anchors_list, num_classes, topk=13, alpha=1, beta=6,
                      want_cls_target=True):
    """Task-aligned target assignment (TOOD, Feng et al., ICCV 2021; the assigner of PP-YOLOE and YOLOv8) for every image and
    pyramid level: the assigner that looks at what the network predicts, axis-aligned boxes only.  The candidates of a box are
    the anchors whose cell centre lies inside it; each gets the metric s^alpha * u^beta -- s the class score the network gives the
    box's class there, u the IoU of the box it predicts there with the ground truth --, the box takes its `topk` best over all
    levels, and an anchor taken by several boxes goes to the largest u.  The exact definition is in csrc/tal.hpp.
    A box that contains no cell centre gets no positive anchor at all.

    targets [B, N, 5] = (x, y, w, h, class), rows whose class is not a whole number in 0..num_classes-1 are padding; cls_heads /
    box_heads: per level the logits [B, A * C, H, W] and deltas [B, A * 4, H, W] -- pass them detached; alpha in 0..4 and beta in
    1..8 are whole numbers.  GPU tensors go to the HIP kernels as the convolutions wrote them (float32 / bfloat16 / float16, NCHW or
    channels_last, no copy); any other tensor takes the pure-torch branch, which follows the same definition.
    -> lists (cls_targets [B, A, C, H, W] | Nones, box_targets [B, A, 4, H, W], depths [B, A, 1, H, W]); depth is class + 1
    or 0 (there is no ignore band)."""
    topk, alpha, beta = int(topk), int(alpha), int(beta)
    if not 1 <= topk <= _C.ATSS_MAX_TOPK:
        raise ValueError('tal_assign_levels: topk must be in 1..%d' % _C.ATSS_MAX_TOPK)
    if not 0 <= alpha <= 4:
        raise ValueError('tal_assign_levels: alpha must be in 0..4')
    if not 1 <= beta <= 8:
        raise ValueError('tal_assign_levels: beta must be in 1..8')
    if len(cls_heads) > MAX_LEVELS_PER_CALL:
        raise ValueError('tal_assign_levels: at most %d levels (a box ranks its candidates over all of them, so the call cannot '
                         'be split)' % MAX_LEVELS_PER_CALL)
    if not (len(cls_heads) == len(box_heads) == len(strides) == len(anchors_list)) or not cls_heads:
        raise ValueError('tal_assign_levels: one class head, box head, stride and anchor table per level')
    targets = targets.float()
    if targets.is_cuda:
        pairs = [_pair(c.detach(), b.detach()) for c, b in zip(cls_heads, box_heads)]
        return _C.tal_assign_levels(targets.contiguous(), [p[0] for p in pairs], [p[1] for p in pairs], anchors_list, num_classes,
                                    [int(s) for s in strides], topk, alpha, beta, want_cls_target)
    return _tal_assign_torch(targets, cls_heads, box_heads, strides, anchors_list, num_classes, topk, alpha, beta, want_cls_target)


def _tal_assign_torch(targets, cls_heads, box_heads, strides, anchors_list, num_classes, topk, alpha, beta, want_cls_target):
    """The pure-torch branch of tal_assign_levels (any device); 16-bit heads are widened to float32, which is exact."""
    cls_heads, box_heads = [c.detach().float() for c in cls_heads], [b.detach().float() for b in box_heads]
    per_image = []
    for i, t in enumerate(targets):
        c = t[:, 4]
        valid = (c >= 0) & (c < num_classes) & (c == torch.floor(c))
        per_image.append(_tal_image(t[valid], [h[i] for h in cls_heads], [h[i] for h in box_heads], strides, anchors_list, num_classes,
                                    topk, alpha, beta, want_cls_target))
    cls_t, box_t, depth_t = [], [], []
    for l, head in enumerate(cls_heads):
        a, (h, w) = anchors_list[l].shape[0], head.shape[-2:]
        cls_t.append(torch.stack([img[l][0] for img in per_image]) if want_cls_target and per_image else
                     (targets.new_zeros((0, a, num_classes, h, w)) if want_cls_target else None))
        box_t.append(torch.stack([img[l][1] for img in per_image]) if per_image else targets.new_zeros((0, a, 4, h, w)))
        depth_t.append(torch.stack([img[l][2] for img in per_image]) if per_image else targets.new_zeros((0, a, 1, h, w)))
    return cls_t, box_t, depth_t


def rotate_boxes(boxes, points=False):
    """(x, y, w, h, theta) targets -> ([x1, y1, x2, y2, sin, cos], ordered corner quads [N, 8])
    (reference utils.py:33-82; `points=True` takes (x1, y1, x2, y2, theta))."""
    theta = boxes[:, 4]
    cos, sin = torch.cos(theta), torch.sin(theta)
    if points:
        x1, y1, x2, y2 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
        cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
    else:
        x1, y1 = boxes[:, 0], boxes[:, 1]
        x2, y2 = x1 + boxes[:, 2], y1 + boxes[:, 3]
        cx, cy = x1 + boxes[:, 2] / 2, y1 + boxes[:, 3] / 2
    quads = []
    for px, py in ((x1, y1), (x2, y1), (x2, y2), (x1, y2)):
        dx, dy = px - cx, py - cy
        quads.append(torch.stack([cos * dx + sin * dy + cx, -sin * dx + cos * dy + cy], 1))
    axis = torch.cat([boxes[:, :2], boxes[:, :2] + boxes[:, 2:4] - 1, sin[:, None], cos[:, None]], 1)
    return axis, _order_quads(torch.stack(quads, 1)).view(-1, 8)


def snap_to_anchors_rotated(boxes, size, stride, anchors, num_classes, device, anchor_ious):
    """Rotated training targets (reference box.py:192-252): overlap = polygon IoU between the
    ground-truth quads and the rotated anchor quads, computed by the HIP `iou` op (GPU only -- the
    reference has no CPU implementation of it either, box.py:220-223)."""
    anchors_axis, anchors_rotated = anchors
    num_anchors = anchors_rotated.shape[0]
    width, height = int(size[0] / stride), int(size[1] / stride)
    if boxes.nelement() == 0:
        return (torch.zeros([num_anchors, num_classes, height, width], device=device),
                torch.zeros([num_anchors, 6, height, width], device=device),
                torch.zeros([num_anchors, 1, height, width], device=device))
    boxes, classes = boxes.split(5, dim=1)
    boxes_axis, boxes_quads = rotate_boxes(boxes)
    boxes_axis, boxes_quads = boxes_axis.to(device), boxes_quads.to(device)
    cell_axis = _cell_anchors(anchors_axis, size, stride, torch.float32, device)
    cell_quads = _cell_anchors(anchors_rotated, size, stride, torch.float32, device)
    _require_gpu(boxes_quads, 'snap_to_anchors_rotated')
    overlap = _C.iou(boxes_quads.contiguous().view(-1), cell_quads.contiguous().view(-1))[0]
    return _targets_from_overlap(overlap, boxes_axis, classes, cell_axis, num_anchors, height, width, num_classes,
                                 anchor_ious, box2delta_rotated)


_ROTATED_ANCHOR_TABLES = {}


def snap_to_anchors_rotated_levels(targets, sizes, strides, anchors_list, num_classes, anchor_ious, want_cls_target=True):
    """snap_to_anchors_rotated for every image and every pyramid level in ONE fused HIP launch (GPU only; csrc/targets.hpp):
    no [27*H*W, N] IoU matrix, no per-image loop.  targets [B, N, 6] = (x, y, w, h, theta, class), class = -1 rows are padding
    (reference data.py format); anchors_list: per level the (axis, rotated) pair of generate_anchors_rotated; sizes: per level
    (H, W) of the head tensors.  The few per-box torch ops of the reference's `rotate_boxes` (cos / sin, corner ordering) run
    once for the whole batch.  -> lists (cls_targets | Nones, box_targets [B, A, 6, H, W], depths [B, A, 1, H, W])."""
    _require_gpu(targets, 'snap_to_anchors_rotated_levels')
    targets = targets.float()
    b, n, _ = targets.shape
    flat = targets.reshape(b * n, 6)
    axis, quads = rotate_boxes(flat[:, :5])
    tables = []
    for (anchors_axis, anchors_rotated), s in zip(anchors_list, strides):
        key = (targets.device, anchors_axis.data_ptr(), anchors_rotated.data_ptr())
        hit = _ROTATED_ANCHOR_TABLES.get(key)
        if hit is None:                                           # device copies of the (tiny) anchor tables, made once
            hit = (anchors_axis.to(targets.device, torch.float32).contiguous(), anchors_rotated.to(targets.device, torch.float32).contiguous(),
                   anchors_axis, anchors_rotated)                  # (the host tensors are kept alive: their addresses are the key)
            _ROTATED_ANCHOR_TABLES[key] = hit
        tables.append(hit[:2])
    return _C.snap_to_anchors_rotated_levels(axis.view(b, n, 6).contiguous(), quads.view(b, n, 8).contiguous(), flat[:, 5].reshape(b, n).contiguous(),
                                             tables, num_classes, [(int(h), int(w)) for h, w in sizes], [int(s) for s in strides],
                                             anchor_ious[0], anchor_ious[1], want_cls_target)


def _require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError('odtk.box.%s: tensors must be on the GPU (only the axis-aligned decode / nms have a '
                           'pure-torch CPU branch)' % what)


def _decode_cpu(cls_heads, box_heads, stride, threshold, top_n, anchors):
    """CPU branch of `decode` (reference box.py:266-309): per image keep `score >= threshold`, take the
    `top_n` best in (score desc, flat NCHW index asc) order, decode their boxes with `delta2box`."""
    cls_heads, box_heads = cls_heads.float(), box_heads.float()
    anchors = anchors.to(cls_heads.device, torch.float32)
    batch, channels, height, width = cls_heads.shape
    num_anchors = anchors.shape[0]
    num_classes = channels // num_anchors
    scores_out = cls_heads.new_zeros((batch, top_n))
    boxes_out = cls_heads.new_zeros((batch, top_n, 4))
    classes_out = cls_heads.new_zeros((batch, top_n))
    flat_scores = cls_heads.reshape(batch, -1)
    deltas_by_cell = box_heads.reshape(batch, num_anchors, 4, height, width)
    for image in range(batch):
        row = flat_scores[image]
        candidates = torch.nonzero(row >= threshold).view(-1)                 # ascending flat index
        if candidates.numel() == 0:
            continue
        ranked = torch.argsort(row[candidates], descending=True, stable=True)[:top_n]
        index = candidates[ranked]
        k = index.numel()
        a, c, y, x = torch.unravel_index(index, (num_anchors, num_classes, height, width))
        cell = torch.stack([x, y, x, y], 1).to(torch.float32) * stride + anchors[a]
        scores_out[image, :k] = row[index]
        boxes_out[image, :k] = delta2box(deltas_by_cell[image, a, :, y, x], cell, [width, height], stride)
        classes_out[image, :k] = c.to(torch.float32)
    return scores_out, boxes_out, classes_out


def _nms_cpu(all_scores, all_boxes, all_classes, nms, ndetections, return_indices=False):
    """CPU branch of `nms` (reference box.py:319-367): greedy, class-aware, +1 pixel IoU.  The reference
    compacts its arrays after every kept box; here one `alive` mask over the score-sorted candidates does
    the same bookkeeping: the i-th kept box is the i-th alive entry, and it retires every alive entry that
    fails the reference's survivor test `score > s_i  or  IoU <= nms  or  class != c_i`.
    return_indices: a fourth value, int32 [B, D], the input position of every kept box (-1: unused slot)."""
    all_scores, all_boxes, all_classes = all_scores.float(), all_boxes.float(), all_classes.float()
    batch = all_scores.shape[0]
    scores_out = all_scores.new_zeros((batch, ndetections))
    boxes_out = all_scores.new_zeros((batch, ndetections, 4))
    classes_out = all_scores.new_zeros((batch, ndetections))
    index_out = torch.full((batch, ndetections), -1, dtype=torch.int32)
    for image in range(batch):
        positive = torch.nonzero(all_scores[image] > 0).view(-1)
        if positive.numel() == 0:
            continue
        order = positive[torch.argsort(all_scores[image, positive], descending=True, stable=True)]
        scores, boxes, classes = all_scores[image, order], all_boxes[image, order], all_classes[image, order]
        area = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
        alive = torch.ones_like(scores, dtype=torch.bool)
        kept = 0
        while kept < ndetections:
            remaining = torch.nonzero(alive).view(-1)
            if kept >= remaining.numel():
                break
            i = int(remaining[kept])
            lo = torch.max(boxes[:, :2], boxes[i, :2])
            hi = torch.min(boxes[:, 2:], boxes[i, 2:])
            inter = torch.prod((hi - lo + 1).clamp(0), 1)
            survives = (scores > scores[i]) | (inter / (area + area[i] - inter) <= nms) | (classes != classes[i])
            survives[i] = True
            alive &= survives
            kept += 1
        winners = torch.nonzero(alive).view(-1)[:kept]
        scores_out[image, :kept] = scores[winners]
        boxes_out[image, :kept] = boxes[winners]
        classes_out[image, :kept] = classes[winners]
        index_out[image, :kept] = order[winners].to(torch.int32)
    if return_indices:
        return scores_out, boxes_out, classes_out, index_out
    return scores_out, boxes_out, classes_out


def _soft_nms_cpu(all_scores, all_boxes, all_classes, nms, ndetections, method, sigma, min_score):
    """CPU branch of `soft_nms`: Soft-NMS (Bodla et al. 2017), class-aware, with `_nms_cpu`'s +1 pixel IoU in its operation order.
    Working scores w start as the scores (alive iff w > 0); up to `ndetections` times the alive candidate with the largest w
    (ties: lowest position) is emitted with its current w and retired, and every alive candidate of its class is decayed --
    linear: w *= 1 - IoU where not IoU <= nms; gaussian: w *= exp(-(IoU * IoU) / sigma) -- and stays alive iff w >= min_score."""
    all_scores, all_boxes, all_classes = all_scores.float(), all_boxes.float(), all_classes.float()
    batch = all_scores.shape[0]
    scores_out = all_scores.new_zeros((batch, ndetections))
    boxes_out = all_scores.new_zeros((batch, ndetections, 4))
    classes_out = all_scores.new_zeros((batch, ndetections))
    index_out = torch.full((batch, ndetections), -1, dtype=torch.int32)
    sigma = torch.tensor(sigma, dtype=torch.float32)
    for image in range(batch):
        boxes, classes = all_boxes[image], all_classes[image]
        w = all_scores[image].clone()
        alive = w > 0
        area = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
        for kept in range(ndetections):
            if not bool(alive.any()):
                break
            ranked = torch.where(alive, w, torch.full_like(w, -1))
            i = int(torch.nonzero(ranked == ranked.max()).view(-1)[0])   # largest w, lowest position
            scores_out[image, kept], boxes_out[image, kept], classes_out[image, kept] = w[i], boxes[i], classes[i]
            index_out[image, kept] = i
            alive[i] = False
            visit = alive & (classes == classes[i])
            lo = torch.max(boxes[:, :2], boxes[i, :2])
            hi = torch.min(boxes[:, 2:], boxes[i, 2:])
            inter = torch.prod((hi - lo + 1).clamp(0), 1)
            iou = inter / (area + area[i] - inter)
            if method == 'gaussian':
                # (float64 exp rounded once: what csrc/common.hpp's exp_cr is)
                decayed = w * torch.exp(((-(iou * iou)) / sigma).double()).float()
            else:
                decayed = torch.where(~(iou <= nms), w * (1 - iou), w)
            w = torch.where(visit, decayed, w)
            alive &= ~visit | (w >= min_score)
    return scores_out, boxes_out, classes_out, index_out


def _matrix_nms_cpu(all_scores, all_boxes, all_classes, ndetections, method, sigma, min_score, pre_top):
    """CPU branch of `matrix_nms`: Matrix NMS (Wang et al., SOLOv2, 2020), class-aware, float32 with `_soft_nms_cpu`'s +1 pixel
    IoU in its operation order.  Per image the candidates with score > 0 are ranked (score descending, ties by position) and the
    first `pre_top` take part.  With iou[i, j] over the participants and pair(i, j) = i ranks before j and both have one class:
      cmax[j]  = max(0, iou[i, j] over pair(i, j))                 (a NaN IoU is skipped)
      d[i, j]  = (1 - iou[i, j]) / (1 - cmax[i])                   linear
               = exp((cmax[i] * cmax[i] - iou[i, j] * iou[i, j]) / sigma)   gaussian (the double exp rounded once)
      decay[j] = min(1, d[i, j] over pair(i, j))                   (a NaN or +inf d is skipped)
    and participant j comes out with score * decay[j] where that is >= min_score, ordered by it (ties by position)."""
    all_scores, all_boxes, all_classes = all_scores.float(), all_boxes.float(), all_classes.float()
    batch = all_scores.shape[0]
    scores_out = all_scores.new_zeros((batch, ndetections))
    boxes_out = all_scores.new_zeros((batch, ndetections, 4))
    classes_out = all_scores.new_zeros((batch, ndetections))
    index_out = torch.full((batch, ndetections), -1, dtype=torch.int32)
    sigma = torch.tensor(sigma, dtype=torch.float32)
    for image in range(batch):
        order = torch.sort(all_scores[image], descending=True, stable=True)[1]
        order = order[all_scores[image][order] > 0][:pre_top]                    # (a NaN is not > 0)
        n = int(order.numel())
        if n == 0:
            continue
        scores, boxes, classes = all_scores[image][order], all_boxes[image][order], all_classes[image][order]
        area = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
        lo = torch.max(boxes[:, None, :2], boxes[None, :, :2])
        hi = torch.min(boxes[:, None, 2:], boxes[None, :, 2:])
        wh = (hi - lo + 1).clamp(0)
        inter = wh[..., 0] * wh[..., 1]
        iou = inter / ((area[None, :] + area[:, None]) - inter)
        rank = torch.arange(n)
        pair = (rank[:, None] < rank[None, :]) & (classes[:, None] == classes[None, :])
        cmax = torch.where(pair & (iou > 0), iou, torch.zeros_like(iou)).amax(0)
        if method == 'gaussian':
            d = torch.exp((((cmax * cmax)[:, None] - iou * iou) / sigma).double()).float()
        else:
            d = (1 - iou) / (1 - cmax)[:, None]
        decay = torch.where(pair & (d < 1), d, torch.ones_like(d)).amin(0)
        decayed = scores * decay
        alive = torch.nonzero(decayed >= min_score).view(-1)
        alive = alive[torch.sort(order[alive], stable=True)[1]]                  # by position, then (stable) by decayed score
        alive = alive[torch.sort(decayed[alive], descending=True, stable=True)[1]][:ndetections]
        kept = int(alive.numel())
        scores_out[image, :kept], boxes_out[image, :kept], classes_out[image, :kept] = decayed[alive], boxes[alive], classes[alive]
        index_out[image, :kept] = order[alive].to(torch.int32)
    return scores_out, boxes_out, classes_out, index_out


def decode(all_cls_head, all_box_head, stride=1, threshold=0.05, top_n=1000, anchors=None, rotated=False):
    """Box decoding and filtering for one pyramid level (reference box.py:255-309).

    cls [B, A*C, H, W] post-sigmoid, box [B, A*{4|6}, H, W] -> scores [B, top_n],
    boxes [B, top_n, {4|6}], classes [B, top_n] (score-descending, zero padded)."""
    if rotated:
        anchors = anchors[0]
    if not all_cls_head.is_cuda:
        if rotated:
            _require_gpu(all_cls_head, 'decode(rotated=True)')
        return _decode_cpu(all_cls_head, all_box_head, stride, threshold, top_n, anchors)
    return _C.decode(all_cls_head.float().contiguous(), all_box_head.float().contiguous(),
                     anchors.reshape(-1).tolist(), stride, threshold, top_n, rotated)


def nms(all_scores, all_boxes, all_classes, nms=0.5, ndetections=100):
    """Batched class-aware greedy NMS (reference box.py:312-367)."""
    if not all_scores.is_cuda:
        return _nms_cpu(all_scores, all_boxes, all_classes, nms, ndetections)
    return _C.nms(all_scores.float().contiguous(), all_boxes.float().contiguous(),
                  all_classes.float().contiguous(), nms, ndetections, False)


SOFT_NMS_METHODS = {'linear': _C.SOFT_NMS_LINEAR, 'gaussian': _C.SOFT_NMS_GAUSSIAN}
MAX_SOFT_NMS_COUNT = _C.MAX_NMS_COUNT              # candidates per image odtk_soft_nms takes


def _soft_nms_options(method, sigma, min_score):
    if method not in SOFT_NMS_METHODS:
        raise ValueError("soft_nms: method must be 'linear' or 'gaussian', not %r" % (method,))
    sigma, min_score = float(sigma), float(min_score)
    if not (math.isfinite(sigma) and sigma > 0 and math.isfinite(min_score) and min_score > 0):
        raise ValueError('soft_nms: sigma and min_score must be finite and > 0')
    return method, sigma, min_score


def soft_nms(all_scores, all_boxes, all_classes, nms=0.5, ndetections=100, method='linear', sigma=0.5, min_score=0.001):
    """Batched class-aware Soft-NMS on axis-aligned boxes (no reference equivalent; definition at `_soft_nms_cpu`): neighbours of
    a kept box have their scores decayed instead of being dropped; the returned scores are the decayed ones, non-increasing."""
    method, sigma, min_score = _soft_nms_options(method, sigma, min_score)
    if not all_scores.is_cuda:
        return _soft_nms_cpu(all_scores, all_boxes, all_classes, nms, ndetections, method, sigma, min_score)[:3]
    return _C.soft_nms(all_scores.float().contiguous(), all_boxes.float().contiguous(), all_classes.float().contiguous(),
                       nms, ndetections, SOFT_NMS_METHODS[method], sigma, min_score)


MATRIX_NMS_METHODS = {'linear': _C.MATRIX_NMS_LINEAR, 'gaussian': _C.MATRIX_NMS_GAUSSIAN}
MAX_MATRIX_NMS_PRE = _C.MAX_MATRIX_NMS_PRE         # participants per image odtk_matrix_nms ranks


def _matrix_nms_options(method, sigma, min_score, pre_top):
    if method not in MATRIX_NMS_METHODS:
        raise ValueError("matrix_nms: method must be 'linear' or 'gaussian', not %r" % (method,))
    sigma, min_score = float(sigma), float(min_score)
    if not (math.isfinite(sigma) and sigma > 0 and math.isfinite(min_score) and min_score > 0):
        raise ValueError('matrix_nms: sigma and min_score must be finite and > 0')
    if isinstance(pre_top, bool) or int(pre_top) != pre_top or not 1 <= pre_top <= MAX_MATRIX_NMS_PRE:
        raise ValueError('matrix_nms: pre_top must be a whole number in 1..%d, not %r' % (MAX_MATRIX_NMS_PRE, pre_top))
    return method, sigma, min_score, int(pre_top)


def _matrix_nms_dict(matrix_nms, threshold):
    """The options of a `matrix_nms` dict, validated: (method, sigma, min_score, pre_top)."""
    unknown = set(matrix_nms) - {'method', 'sigma', 'min_score', 'pre_top'}
    if unknown:
        raise ValueError('matrix_nms: unknown option(s) %s' % ', '.join(sorted(unknown)))
    return _matrix_nms_options(matrix_nms.get('method', 'gaussian'), matrix_nms.get('sigma', 0.5),
                               matrix_nms.get('min_score', threshold), matrix_nms.get('pre_top', 2000))


def matrix_nms(all_scores, all_boxes, all_classes, ndetections=100, method='gaussian', sigma=0.5, min_score=0.001, pre_top=2000):
    """Batched class-aware Matrix NMS on axis-aligned boxes (no reference equivalent; definition at `_matrix_nms_cpu`): every
    score is decayed by one factor that comes from the pairwise IoUs of the `pre_top` best candidates; the returned scores are the
    decayed ones, non-increasing.  There is no IoU threshold, and no limit on the length of the candidate list."""
    method, sigma, min_score, pre_top = _matrix_nms_options(method, sigma, min_score, pre_top)
    if not all_scores.is_cuda:
        return _matrix_nms_cpu(all_scores, all_boxes, all_classes, ndetections, method, sigma, min_score, pre_top)[:3]
    return _C.matrix_nms(all_scores.float().contiguous(), all_boxes.float().contiguous(), all_classes.float().contiguous(),
                         ndetections, pre_top, MATRIX_NMS_METHODS[method], sigma, min_score)


def _vote_option(vote):
    vote = float(vote)
    if not (math.isfinite(vote) and 0 < vote <= 1):
        raise ValueError('box voting: the threshold must be finite and in (0, 1], not %r' % (vote,))
    return vote


def _box_vote_cpu(all_scores, all_boxes, all_classes, kept, vote_thresh):
    """Pure-torch branch of `box_vote`: `_soft_nms_cpu`'s float32 IoU in its operation order, the weighted mean in float64."""
    all_scores, all_boxes, all_classes = all_scores.float(), all_boxes.float(), all_classes.float()
    batch, count = all_scores.shape
    out = all_scores.new_zeros((batch, kept.shape[1], 4))
    position = torch.arange(count, device=all_scores.device)
    for image in range(batch):
        scores, boxes, classes = all_scores[image], all_boxes[image], all_classes[image]
        area = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
        for slot, p in enumerate(kept[image].tolist()):
            if p < 0 or p >= count:
                continue
            lo = torch.max(boxes[:, :2], boxes[p, :2])
            hi = torch.min(boxes[:, 2:], boxes[p, 2:])
            inter = torch.prod((hi - lo + 1).clamp(0), 1)
            iou = inter / (area + area[p] - inter)
            voters = (scores > 0) & (classes == classes[p]) & ((iou >= vote_thresh) | (position == p))
            w = scores[voters].double()
            out[image, slot] = ((w[:, None] * boxes[voters].double()).sum(0) / w.sum()).float()
    return out


def box_vote(all_scores, all_boxes, all_classes, kept, vote_thresh=0.65):
    """Box voting behind a suppression (Gidaris & Komodakis 2015; no reference equivalent; definition in include/odtk_hip.h:
    odtk_box_vote): every kept box becomes the score-weighted mean of the candidates of its class that overlap it by at least
    `vote_thresh` (+1 pixel IoU), itself included.  all_scores / all_boxes / all_classes: the suppression's INPUT list (the weights
    are its scores, also behind Soft-NMS); kept [B, D] int32: the input position of each emitted detection or -1, as
    `_C.nms(.., return_indices=True)` and `_C.soft_nms(.., return_indices=True)` return it -> boxes [B, D, 4] (unused slots: zeros).
    GPU tensors go to the HIP kernel (one launch); any other tensor takes the pure-torch float64 branch."""
    vote_thresh = _vote_option(vote_thresh)
    if not all_scores.is_cuda:
        return _box_vote_cpu(all_scores, all_boxes, all_classes, kept, vote_thresh)
    return _C.box_vote(all_scores.float().contiguous(), all_boxes.float().contiguous(), all_classes.float().contiguous(),
                       kept.to(torch.int32).contiguous(), vote_thresh)


def concat_candidates(parts, mirror_widths):
    """Several candidate lists (scores [B, n_i], boxes [B, n_i, 4], classes [B, n_i]) as one along the candidate axis, the merge of
    flip test-time augmentation (include/odtk_hip.h: odtk_concat_candidates).  mirror_widths: per part 0, or the width W of the
    tensor whose horizontal flip the part was decoded from: its boxes with a score > 0 are mapped back, x1' = (W - 1) - x2 and
    x2' = (W - 1) - x1 in float32.  GPU tensors: one HIP launch; any other tensor: the same in torch."""
    parts = [tuple(t.float() for t in part) for part in parts]
    widths = [int(w) for w in mirror_widths]
    if not 1 <= len(parts) <= _C.MAX_CONCAT_PARTS or len(widths) != len(parts) or min(widths) < 0:
        raise ValueError('concat_candidates: 1..%d parts, one non-negative mirror width each' % _C.MAX_CONCAT_PARTS)
    if parts[0][0].is_cuda:
        return _C.concat_candidates([tuple(t.contiguous() for t in part) for part in parts], widths)
    unmirrored = []
    for (scores, boxes, classes), width in zip(parts, widths):
        if width > 0:
            edge = torch.tensor(width - 1, dtype=torch.float32)
            positive = scores > 0
            x1, x2 = torch.where(positive, edge - boxes[..., 2], boxes[..., 0]), torch.where(positive, edge - boxes[..., 0], boxes[..., 2])
            boxes = torch.stack([x1, boxes[..., 1], x2, boxes[..., 3]], -1)
        unmirrored.append((scores, boxes, classes))
    return [torch.cat(t, 1) for t in zip(*unmirrored)]


def flip_batch(x):
    """x.flip(-1) in x's memory format (the engine's plans and graphs are keyed by it)."""
    flipped = x.flip(-1)
    if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
        flipped = flipped.contiguous(memory_format=torch.channels_last)
    return flipped


MAX_TILES = _C.MAX_TILES                           # tile entries per call of `tile_images` / `merge_tile_candidates`


def _pair_of_ints(value, name):
    pair = (value, value) if isinstance(value, int) else tuple(value)
    if len(pair) != 2 or any(int(v) != v for v in pair):
        raise ValueError('%s must be an integer or a pair of integers, not %r' % (name, value))
    return int(pair[0]), int(pair[1])


def tile_grid(height, width, size, overlap):
    """The origins (y, x), row-major, of the tiles of `size` = (th, tw) that cover a height x width image with `overlap` =
    (oy, ox) pixels shared by neighbours, 0 <= overlap < size.  Per axis, with step = size - overlap: an extent <= size has the one
    origin 0 (the tile is zero-padded behind the image); otherwise 0, step, 2 step, ... while origin + size < extent, then one last
    origin extent - size: the last tile is shifted back, never padded."""
    size, overlap = _pair_of_ints(size, 'size'), _pair_of_ints(overlap, 'overlap')
    if height < 1 or width < 1 or min(size) < 1:
        raise ValueError('tile_grid: sizes must be positive')
    axes = []
    for extent, tile, over in zip((int(height), int(width)), size, overlap):
        if not 0 <= over < tile:
            raise ValueError('tile_grid: the overlap must be in [0, size), not %d for size %d' % (over, tile))
        origins = [0]
        if extent > tile:
            origins = list(range(0, extent - tile, tile - over)) + [extent - tile]
        axes.append(origins)
    return [(y, x) for y in axes[0] for x in axes[1]]


def _tile_entries(tiles, what, batch=None):
    tiles = [tuple(int(v) for v in t) for t in tiles]
    if not 1 <= len(tiles) <= MAX_TILES or any(len(t) != 4 for t in tiles):
        raise ValueError('%s: 1..%d tiles (image, slot, y, x) per call' % (what, MAX_TILES))
    if any(t[2] < 0 or t[3] < 0 for t in tiles) or (batch is not None and any(t[0] >= batch for t in tiles)):
        raise ValueError('%s: a tile names an image past the batch or a negative origin' % what)
    return tiles


def tile_images(x, tiles, size):
    """The tiler of tiled inference (definition in include/odtk_hip.h: odtk_tile_images).  x [B, C, H, W]; tiles: up to 64 entries
    (image, slot, y, x) -- the window of `image` at origin (y, x); image < 0: an all-zero tile, the padding of a short chunk; `slot`
    is ignored here; size (th, tw) -> [len(tiles), C, th, tw] in x's dtype and memory format, +0 wherever a window leaves its image.
    A bit copy.  GPU tensors (float32 / bfloat16 / float16): one HIP launch; any other tensor: the same in torch."""
    th, tw = _pair_of_ints(size, 'size')
    if x.dim() != 4 or th < 1 or tw < 1:
        raise ValueError('tile_images: x is [B, C, H, W] and the size positive')
    tiles = _tile_entries(tiles, 'tile_images', x.shape[0])
    channels_last = not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)
    if x.is_cuda:
        if not 1 <= x.shape[1] <= 16:
            raise ValueError('tile_images: 1..16 channels, not %d' % x.shape[1])
        return _C.tile_images(x if channels_last else x.contiguous(), tiles, (th, tw))
    out = torch.zeros((len(tiles), x.shape[1], th, tw), dtype=x.dtype, device=x.device)
    if channels_last:
        out = out.contiguous(memory_format=torch.channels_last)
    for i, (image, _, y, left) in enumerate(tiles):
        rows, cols = min(th, x.shape[2] - y), min(tw, x.shape[3] - left)
        if image >= 0 and rows > 0 and cols > 0:
            out[i, :, :rows, :cols] = x[image, :, y:y + rows, left:left + cols]
    return out


def merge_tile_candidates(parts, tiles, batch, slots, size, extent, border=0.0, out=None):
    """The merge of tiled inference (definition in include/odtk_hip.h: odtk_merge_tile_candidates).  parts: (scores [n, count], boxes
    [n, count, 4], classes [n, count]) decoded from the n tiles, in tile coordinates; tiles: their entries (image, slot, y, x), image
    < 0 skipped; size (th, tw); extent (H, W) of the images.  Entry i fills positions slot * count .. slot * count + count - 1 of row
    `image` of (scores [batch, slots * count], boxes [.., 4], classes): candidates with a score > 0 move by the tile's origin (one
    float32 addition per coordinate) unless `border` > 0 cuts them -- they reach into the outermost `border` pixels of a tile side
    that is not an image side -- which leaves an empty slot; everything else is copied bit for bit.  `out`: lists to write into
    (several calls that together cover every (image, slot)); without it new lists whose other positions are empty slots.
    GPU tensors: one HIP launch; any other tensor: the same in torch."""
    (th, tw), (height, width) = _pair_of_ints(size, 'size'), _pair_of_ints(extent, 'extent')
    border, batch, slots = float(border), int(batch), int(slots)
    if not (math.isfinite(border) and border >= 0):
        raise ValueError('merge_tile_candidates: the border must be finite and not negative, not %r' % (border,))
    if min(th, tw, height, width, batch, slots) < 1:
        raise ValueError('merge_tile_candidates: batch, slots and sizes must be positive')
    tiles = _tile_entries(tiles, 'merge_tile_candidates', batch)
    if any(t[0] >= 0 and not 0 <= t[1] < slots for t in tiles):
        raise ValueError('merge_tile_candidates: a slot outside 0..%d' % (slots - 1))
    scores, boxes, classes = (t.float() for t in parts)
    count = scores.shape[1]
    if scores.shape != (len(tiles), count) or boxes.shape != (len(tiles), count, 4) or classes.shape != scores.shape or count < 1:
        raise ValueError('merge_tile_candidates: the parts are (scores [n, count], boxes [n, count, 4], classes [n, count]) of the n tiles')
    if slots * count > _C.MAX_NMS_COUNT_SCRATCH:
        raise ValueError('merge_tile_candidates: %d candidates per image, the limit is %d' % (slots * count, _C.MAX_NMS_COUNT_SCRATCH))
    if scores.is_cuda:
        return _C.merge_tile_candidates((scores.contiguous(), boxes.contiguous(), classes.contiguous()), tiles, batch, slots, (th, tw),
                                        (height, width), border, out)
    if out is None:
        out = [scores.new_zeros((batch, slots * count)), scores.new_zeros((batch, slots * count, 4)), scores.new_zeros((batch, slots * count))]
    edge = torch.tensor(border, dtype=torch.float32)
    far_x, far_y = torch.tensor(tw - 1, dtype=torch.float32) - edge, torch.tensor(th - 1, dtype=torch.float32) - edge
    for i, (image, slot, y, left) in enumerate(tiles):
        if image < 0:
            continue
        s, b, c = scores[i], boxes[i], classes[i]
        positive = s > 0
        cut = torch.zeros_like(positive)
        if border > 0:
            if left > 0:
                cut |= b[:, 0] < edge
            if y > 0:
                cut |= b[:, 1] < edge
            if left + tw < width:
                cut |= b[:, 2] > far_x
            if y + th < height:
                cut |= b[:, 3] > far_y
        cut &= positive
        moved = torch.where(positive[:, None], b + torch.tensor([left, y, left, y], dtype=torch.float32), b)
        span = slice(slot * count, (slot + 1) * count)
        out[0][image, span] = torch.where(cut, torch.zeros_like(s), s)
        out[1][image, span] = torch.where(cut[:, None], torch.zeros_like(b), moved)
        out[2][image, span] = torch.where(cut, torch.zeros_like(c), c)
    return out


def suppress(all_scores, all_boxes, all_classes, nms=0.5, ndetections=100, soft_nms=None, vote=None, threshold=0.05, matrix_nms=None):
    """The tail of the post-processing on ONE candidate list of axis-aligned boxes: hard NMS, or Soft-NMS when `soft_nms` is a dict
    (`method`, `sigma`, `min_score`: default `threshold`), or Matrix NMS when `matrix_nms` is a dict (`method`, `sigma`,
    `min_score`: default `threshold`, `pre_top`: default 2000), then box voting at IoU `vote` when that is not None.
    -> (scores [B, D], boxes [B, D, 4], classes [B, D]).  GPU tensors: one launch for the suppression (Matrix NMS: four) and one
    for the vote."""
    if matrix_nms is not None and soft_nms is not None:
        raise ValueError('suppress: Soft-NMS and Matrix NMS exclude each other')
    want = vote is not None
    if want:
        vote = _vote_option(vote)
    cuda = all_scores.is_cuda
    if cuda:
        all_scores, all_boxes, all_classes = (t.float().contiguous() for t in (all_scores, all_boxes, all_classes))
    if soft_nms is not None:
        method, sigma, min_score = _soft_nms_options(soft_nms.get('method', 'linear'), soft_nms.get('sigma', 0.5),
                                                     soft_nms.get('min_score', threshold))
        if cuda:
            out = _C.soft_nms(all_scores, all_boxes, all_classes, nms, ndetections, SOFT_NMS_METHODS[method], sigma, min_score, want)
        else:
            out = _soft_nms_cpu(all_scores, all_boxes, all_classes, nms, ndetections, method, sigma, min_score)
    elif matrix_nms is not None:
        method, sigma, min_score, pre_top = _matrix_nms_dict(matrix_nms, threshold)
        if cuda:
            out = _C.matrix_nms(all_scores, all_boxes, all_classes, ndetections, pre_top, MATRIX_NMS_METHODS[method], sigma, min_score, want)
        else:
            out = _matrix_nms_cpu(all_scores, all_boxes, all_classes, ndetections, method, sigma, min_score, pre_top)
    elif cuda:
        out = _C.nms(all_scores, all_boxes, all_classes, nms, ndetections, False, want)
    else:
        out = _nms_cpu(all_scores, all_boxes, all_classes, nms, ndetections, want)
    if not want:
        return tuple(out[:3])
    return out[0], box_vote(all_scores, all_boxes, all_classes, out[3], vote), out[2]


def nms_rotated(all_scores, all_boxes, all_classes, nms=0.5, ndetections=100):
    """NMS on [x1, y1, x2, y2, sin, cos] boxes with polygon IoU (reference box.py:370-375)."""
    _require_gpu(all_scores, 'nms_rotated')
    return _C.nms(all_scores.float().contiguous(), all_boxes.float().contiguous(),
                  all_classes.float().contiguous(), nms, ndetections, True)


def _as_written(t):
    """Hand a head tensor to the HIP path as the convolution wrote it: float32 / bfloat16 / float16 in
    NCHW or channels_last need NO copy; anything else is converted once."""
    if t.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        t = t.float()
    if not (t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)):
        t = t.contiguous()
    return t


def _pair(c, b):
    c, b = _as_written(c), _as_written(b)
    if b.dtype != c.dtype:
        b = b.to(c.dtype)
    if c.is_contiguous() != b.is_contiguous():      # one memory format per level
        b = b.contiguous() if c.is_contiguous() else b.contiguous(memory_format=torch.channels_last)
    return c, b


def decode_levels(cls_heads, box_heads, strides, threshold, top_n, anchors_per_stride, rotated=False, logits=False):
    """All levels at once: equals `[torch.cat(t, 1) for t in zip(*[decode(...) per level])]`
    (reference model.py:153-164) in one enqueue.  logits=True fuses the sigmoid (model.py:140)."""
    anchors = [anchors_per_stride[s][0] if rotated else anchors_per_stride[s] for s in strides]
    for t in cls_heads:
        _require_gpu(t, 'decode_levels')
    pairs = [_pair(c, b) for c, b in zip(cls_heads, box_heads)]
    return _C.decode_levels([p[0] for p in pairs], [p[1] for p in pairs], anchors, strides, threshold, top_n,
                            rotated, logits=logits)


def _decode_groups(pairs, anchors, strides, threshold, top_n, logits, cls_bias, box_bias, cls_thresholds):
    """decode_levels of axis-aligned (cls, box) pairs in groups of MAX_LEVELS levels (the level table of one call) -> one
    candidate list."""
    def bias_of(bias, lo, hi):
        return bias[lo:hi] if isinstance(bias, (list, tuple)) else bias
    parts = []
    for lo in range(0, len(pairs), _C.MAX_LEVELS):
        hi = min(lo + _C.MAX_LEVELS, len(pairs))
        parts.append(_C.decode_levels([p[0] for p in pairs[lo:hi]], [p[1] for p in pairs[lo:hi]], anchors[lo:hi],
                                      strides[lo:hi], threshold, top_n, False, logits=logits,
                                      cls_bias=bias_of(cls_bias, lo, hi), box_bias=bias_of(box_bias, lo, hi),
                                      cls_thresholds=cls_thresholds if len(pairs) <= _C.MAX_LEVELS else None))
    return parts[0] if len(parts) == 1 else [torch.cat(t, 1) for t in zip(*parts)]


def candidates(cls_heads, box_heads, strides, anchors_per_stride, threshold=0.05, top_n=1000, logits=False, cls_bias=None,
               box_bias=None, cls_thresholds=None):
    """The first half of `detect` on its own, axis-aligned boxes: (scores [B, L * top_n], boxes [B, L * top_n, 4], classes) of all
    levels, reading the head tensors in place (GPU only) -- what the passes of test-time augmentation hand to
    `concat_candidates` and `suppress`."""
    for t in cls_heads:
        _require_gpu(t, 'candidates')
    pairs = [_pair(c, b) for c, b in zip(cls_heads, box_heads)]
    return _decode_groups(pairs, [anchors_per_stride[s] for s in strides], strides, threshold, top_n, logits, cls_bias, box_bias,
                          cls_thresholds)


def detect(cls_heads, box_heads, strides, anchors_per_stride, threshold=0.05, top_n=1000, nms=0.5,
           ndetections=100, rotated=False, logits=False, cls_bias=None, box_bias=None, cls_thresholds=None, soft_nms=None, vote=None,
           matrix_nms=None):
    """sigmoid (logits=True) + decode of all levels + nms: the whole inference post-processing of the
    reference (model.py:140-165) in one enqueue of three launches (rotated: five to seven), reading the head tensors in place.
    cls_bias / box_bias: the heads' last-conv biases, added inside the kernels (see _C.decode_levels); cls_thresholds: the
    prefilter's threshold table for that cls_bias, made once by _C.prefilter_thresholds (optional).
    soft_nms: None, or a dict with `method` ('linear' / 'gaussian'), `sigma` and `min_score` -- the suppression is then Soft-NMS
    (`soft_nms` above) on decode_levels' candidates: three launches as well.
    matrix_nms: None, or a dict with `method`, `sigma`, `min_score` and `pre_top` -- the suppression is then Matrix NMS
    (`matrix_nms` above) on decode_levels' candidates: six launches.  Not together with `soft_nms`.
    vote: None, or the IoU threshold of box voting (`box_vote` above) behind the suppression, hard or soft: decode_levels, the
    general NMS with its position output, the vote -- four launches."""
    if soft_nms is not None and rotated:
        raise ValueError('detect: Soft-NMS is not available for rotated boxes')
    if matrix_nms is not None and rotated:
        raise ValueError('detect: Matrix NMS is not available for rotated boxes')
    if matrix_nms is not None and soft_nms is not None:
        raise ValueError('detect: Soft-NMS and Matrix NMS exclude each other')
    if vote is not None and rotated:
        raise ValueError('detect: box voting is not available for rotated boxes')
    anchors = [anchors_per_stride[s][0] if rotated else anchors_per_stride[s] for s in strides]
    for t in cls_heads:
        _require_gpu(t, 'detect')
    pairs = [_pair(c, b) for c, b in zip(cls_heads, box_heads)]
    if soft_nms is not None or vote is not None or matrix_nms is not None:
        return suppress(*_decode_groups(pairs, anchors, strides, threshold, top_n, logits, cls_bias, box_bias, cls_thresholds),
                        nms, ndetections, soft_nms=soft_nms, vote=vote, threshold=threshold, matrix_nms=matrix_nms)
    if len(pairs) > _C.MAX_LEVELS:
        # a model with several backbones has 5 levels per backbone (reference model.py:138): the level table of one call
        # holds MAX_LEVELS, so decode in groups and hand the concatenation to nms (its candidate count is not capped)
        def bias_of(bias, lo, hi):
            return bias[lo:hi] if isinstance(bias, (list, tuple)) else bias
        parts = []
        for lo in range(0, len(pairs), _C.MAX_LEVELS):
            hi = min(lo + _C.MAX_LEVELS, len(pairs))
            parts.append(_C.decode_levels([p[0] for p in pairs[lo:hi]], [p[1] for p in pairs[lo:hi]], anchors[lo:hi],
                                          strides[lo:hi], threshold, top_n, rotated, logits=logits,
                                          cls_bias=bias_of(cls_bias, lo, hi), box_bias=bias_of(box_bias, lo, hi)))
        return _C.nms(*[torch.cat(t, 1) for t in zip(*parts)], nms, ndetections, rotated)
    return _C.detect([p[0] for p in pairs], [p[1] for p in pairs], anchors, strides, threshold, top_n, nms,
                     ndetections, rotated, logits=logits, cls_bias=cls_bias, box_bias=box_bias, cls_thresholds=cls_thresholds)
