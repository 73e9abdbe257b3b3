"""CPU oracle of the rotated target assignment (TEST INFRASTRUCTURE ONLY; never imported by the product package).

snap_to_anchors_rotated restates the reference's odtk/box.py:192-252 from three parts:
  * rotate_boxes / cell anchors: plain torch-CPU fp32, the reference's arithmetic (utils.py:15-82, box.py:213-218);
  * the overlap of ALL (anchor cell, box) pairs: c_oracle.iou_pairs, pinned bit for bit to the reference's device code
    compiled for the CPU and to the HIP `iou` op (tests/test_oracle_native_ref.py, tests/test_gpu_rotated.py);
  * the tail (first maximum, deltas, depth, class map): box_oracle.snap_tail, shared with the axis-aligned oracle.
Nothing is skipped on distance here: a pair the fused kernel's reject zeroes wrongly shows up as a difference.

deltas_f64 is the float64 value of the regression deltas of given fp32 (winner box, cell anchor) pairs: the truth the
fp32 chains of the oracle and of the kernel are both measured against (delta_error_bound).
"""
import numpy as np
import torch

from . import box_oracle, c_oracle


def _order_quads(quads):
    """[Q, 4, 2] corner sets -> [tl, tr, br, bl] per quad (utils.py:15-31), batched."""
    by_x = torch.gather(quads, 1, torch.argsort(quads[:, :, 0], dim=1)[:, :, None].expand(-1, -1, 2))
    left, right = by_x[:, :2], by_x[:, 2:]
    left = torch.gather(left, 1, torch.argsort(left[:, :, 1], dim=1)[:, :, None].expand(-1, -1, 2))
    tl, bl = left[:, 0], left[:, 1]
    dist = torch.cdist(tl[:, None, :], right)[:, 0]
    right = torch.gather(right, 1, torch.argsort(dist, dim=1, descending=True)[:, :, None].expand(-1, -1, 2))
    br, tr = right[:, 0], right[:, 1]
    return torch.stack([tl, tr, br, bl], dim=1)


def rotate_boxes(boxes):
    """utils.py:33-82 for (x, y, w, h, theta) rows -> (axis form [N, 6] = x1, y1, x2, y2, sin, cos; ordered quads [N, 8])."""
    boxes = boxes.float()
    theta = boxes[:, 4]
    cos, sin = torch.cos(theta), torch.sin(theta)
    x1, y1 = boxes[:, 0], boxes[:, 1]
    x2, y2 = x1 + boxes[:, 2], y1 + boxes[:, 3]
    cx, cy = x1 + boxes[:, 2] / 2, y1 + boxes[:, 3] / 2
    quads = []
    for px, py in ((x1, y1), (x2, y1), (x2, y2), (x1, y2)):
        dx, dy = px - cx, py - cy
        quads.append(torch.stack([cos * dx + sin * dy + cx, -sin * dx + cos * dy + cy], 1))
    axis = torch.cat([boxes[:, :2], boxes[:, :2] + boxes[:, 2:4] - 1, sin[:, None], cos[:, None]], 1)
    return axis, _order_quads(torch.stack(quads, 1)).reshape(-1, 8)


def box2delta_rotated(boxes, anchors):
    """box.py:81-94: box2delta on the axis forms, (sin, cos) passed through."""
    return torch.cat([box_oracle.box2delta(boxes[:, :4], anchors[:, :4]), boxes[:, 4:6]], 1)


def overlaps_from_quads(quads, size, stride, anchors_rotated):
    """Polygon IoU of every (anchor cell, box quad) pair, [A*H*W, N], cells in (a, y, x) order."""
    cell_quads = box_oracle.cell_anchors(anchors_rotated, size, stride)
    return torch.from_numpy(c_oracle.iou_pairs(quads.contiguous().numpy().reshape(-1, 8), cell_quads.numpy()))


def snap_from_rotated(axis, quads, classes, size, stride, anchors, num_classes, anchor_ious):
    """The assignment from rotate_boxes' output (axis [N, 6], quads [N, 8], classes [N, 1]): what the fused kernel is handed."""
    anchors_axis, anchors_rotated = anchors
    A = anchors_rotated.shape[0]
    W, H = int(size[0] / stride), int(size[1] / stride)
    if axis.shape[0] == 0:
        return (torch.zeros(A, num_classes, H, W), torch.zeros(A, 6, H, W), torch.zeros(A, 1, H, W),
                torch.full((A, H, W), -1, dtype=torch.int64), torch.zeros(A, H, W))
    cell_axis = box_oracle.cell_anchors(anchors_axis, size, stride)
    overlap = overlaps_from_quads(quads, size, stride, anchors_rotated)
    return box_oracle.snap_tail(overlap, axis, classes, cell_axis, A, H, W, num_classes, anchor_ious, box2delta_rotated)


def snap_to_anchors_rotated(boxes, size, stride, anchors, num_classes, anchor_ious):
    """box.py:192-252.  boxes [N, 6] = (x, y, w, h, theta, class); size = [W*stride, H*stride]; anchors = the (axis [A, 4],
    rotated [A, 8]) pair of generate_anchors_rotated.
    -> cls_target [A, C, H, W], box_target [A, 6, H, W], depth [A, 1, H, W], winner index [A, H, W] (-1 without boxes),
    overlap of the winner [A, H, W]."""
    boxes = boxes.float().view(-1, 6)
    axis, quads = rotate_boxes(boxes[:, :5])
    return snap_from_rotated(axis, quads, boxes[:, 5:6], size, stride, anchors, num_classes, anchor_ious)


def deltas_f64(winner, anchor):
    """winner [M, 4 or 6] fp32 corner form (+ sin, cos), anchor [M, 4] fp32 -> float64 deltas [M, 4 or 6]: the first four
    evaluated in float64 from the fp32 inputs (box.py:67-78, +1 pixel convention), sin and cos passed through."""
    b, a = np.asarray(winner, np.float64), np.asarray(anchor, np.float64)
    with np.errstate(all='ignore'):                  # non-finite and degenerate boxes are legitimate inputs
        a_wh = a[:, 2:4] - a[:, :2] + 1
        a_ctr = a[:, :2] + 0.5 * a_wh
        b_wh = b[:, 2:4] - b[:, :2] + 1
        b_ctr = b[:, :2] + 0.5 * b_wh
        out = np.concatenate([(b_ctr - a_ctr) / a_wh, np.log(b_wh / a_wh)], 1)
    return np.concatenate([out, b[:, 4:6]], 1)


def delta_error_bound(winner, anchor, k):
    """What an fp32 evaluation of the four deltas may differ from deltas_f64 by, [M, 4]: each fp32 operation adds half an
    ulp (2^-24 relative) of ITS OWN result.  Centre deltas: the two centres carry errors relative to |b_ctr| and |a_ctr|,
    the division scales them by 1 / a_wh and adds its own rounding: k * 2^-24 * ((|b_ctr| + |a_ctr|) / a_wh + |delta|).
    Log deltas: the ratio has a relative error of a few 2^-24, which log turns into an absolute one, plus the rounding of
    the result: k * 2^-24 * (1 + |delta|), plus logf's documented <= 1 ulp of the result (2^-23 * |delta|)."""
    b, a = np.asarray(winner, np.float64), np.asarray(anchor, np.float64)
    d = deltas_f64(winner, anchor)
    u = 2.0 ** -24
    with np.errstate(all='ignore'):
        a_wh = a[:, 2:4] - a[:, :2] + 1
        a_ctr = a[:, :2] + 0.5 * a_wh
        b_ctr = b[:, :2] + 0.5 * (b[:, 2:4] - b[:, :2] + 1)
        ctr = k * u * ((np.abs(b_ctr) + np.abs(a_ctr)) / np.abs(a_wh) + np.abs(d[:, :2]))
        log = k * u * (1 + np.abs(d[:, 2:4])) + 2 * u * np.abs(d[:, 2:4])
    return np.concatenate([ctr, log], 1)
