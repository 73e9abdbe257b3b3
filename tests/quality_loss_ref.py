"""The quality focal and varifocal classification losses (`Model.cls_loss = 'qfl' | 'vfl'`) restated in float64 numpy, from the
formulas alone -- independent of odtk/loss.py, which tests/test_quality_loss.py holds against this, and of the kernels
(csrc/quality_loss.hpp), whose ground truth on the GPU this is (tests/test_gpu_quality_loss.py).

    depth: -1 ignore / 0 background / class + 1;  x: a class logit;  s = sigmoid(x), sp = softplus(x)
    q (foreground anchors) = IoU of the boxes the predicted and the target deltas decode to, relative to the anchor centre, the
        predicted log-sizes clipped at log(1000 / 16), eps = 1e-7 in the union, written as 1 - (1 - iou)
    y = q where depth - 1 == class, else 0; elements of ignored anchors contribute 0 and get gradient 0
    qfl: L = |s - y|^gamma (sp - y x), y x = 0 where y = 0;   dL/dx = gamma |s - y|^(gamma-1) sign(s - y) s (1 - s) (sp - y x) + |s - y|^gamma (s - y)
    vfl: y > 0 (or NaN): L = y (sp - y x), dL/dx = y (s - y);   otherwise L = alpha s^gamma sp, dL/dx = alpha s^gamma (gamma (1 - s) sp + s)
"""
import math

import numpy as np

CLIP = math.log(1000.0 / 16)
EPS = 1e-7


def softplus(x):
    return np.logaddexp(0.0, x)


def sigmoid(x):
    return np.exp(-np.logaddexp(0.0, -x))


def box_quality(pred, target, sizes):
    """pred, target [B, A, 4, H, W] deltas, sizes [A, 2] -> q [B, A, H, W]."""
    pred, target, sizes = (np.asarray(v, dtype=np.float64) for v in (pred, target, sizes))
    aw, ah = sizes[:, 0].reshape(1, -1, 1, 1), sizes[:, 1].reshape(1, -1, 1, 1)
    with np.errstate(invalid='ignore', over='ignore'):
        w, h = np.exp(np.minimum(pred[:, :, 2], CLIP)) * aw, np.exp(np.minimum(pred[:, :, 3], CLIP)) * ah
        tw, th = np.exp(target[:, :, 2]) * aw, np.exp(target[:, :, 3]) * ah
        cx, cy, tcx, tcy = pred[:, :, 0] * aw, pred[:, :, 1] * ah, target[:, :, 0] * aw, target[:, :, 1] * ah
        iw = np.minimum(cx + 0.5 * w, tcx + 0.5 * tw) - np.maximum(cx - 0.5 * w, tcx - 0.5 * tw)
        ih = np.minimum(cy + 0.5 * h, tcy + 0.5 * th) - np.maximum(cy - 0.5 * h, tcy - 0.5 * th)
        inter = np.maximum(iw, 0.0) * np.maximum(ih, 0.0)
        union = w * h + tw * th - inter + EPS
        return 1.0 - (1.0 - inter / union)


def quality_target(depth, quality, classes):
    """depth [B, A, 1, H, W], quality [B, A, H, W] -> y [B, A, classes, H, W]."""
    depth = np.asarray(depth, dtype=np.float64)
    c = np.arange(classes, dtype=np.float64).reshape(1, 1, -1, 1, 1)
    return np.where(depth - 1.0 == c, np.asarray(quality, dtype=np.float64)[:, :, None], 0.0)


def qfl(x, y, gamma=2.0):
    """-> (L, dL/dx), elementwise."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        s, ce = sigmoid(x), softplus(x) - np.where(y == 0.0, 0.0, y * x)          # y x = 0 where y = 0, whatever the logit
        u = s - y
        loss = np.abs(u) ** gamma * ce
        grad = gamma * np.abs(u) ** (gamma - 1.0) * np.sign(u) * s * (1.0 - s) * ce + np.abs(u) ** gamma * u
    return loss, grad


def vfl(x, y, alpha=0.75, gamma=2.0):
    """-> (L, dL/dx), elementwise."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        s, sp = sigmoid(x), softplus(x)
        negative = y <= 0.0
        loss = np.where(negative, alpha * s ** gamma * sp, y * (sp - y * x))
        grad = np.where(negative, alpha * s ** gamma * (gamma * (1.0 - s) * sp + s), y * (s - y))
    return loss, grad


def level(logits, deltas, box_target, depth, sizes, kind, alpha=0.75, gamma=2.0):
    """One pyramid level: logits [B, A*C, H, W], deltas [B, A*4, H, W], box_target [B, A, 4, H, W], depth [B, A, 1, H, W], sizes [A, 2]
    -> (cls_sum, foreground, d(cls_sum)/d(logits) shaped like logits)."""
    depth = np.asarray(depth, dtype=np.float64)
    b, a, _, h, w = depth.shape
    x = np.asarray(logits, dtype=np.float64).reshape(b, a, -1, h, w)
    q = box_quality(np.asarray(deltas, dtype=np.float64).reshape(b, a, 4, h, w), box_target, sizes)
    q = np.where(depth[:, :, 0] > 0, q, 0.0)                 # only foreground anchors have one
    y = quality_target(depth, q, x.shape[2])
    loss, grad = qfl(x, y, gamma) if kind == 'qfl' else vfl(x, y, alpha, gamma)
    keep = np.broadcast_to(depth >= 0, x.shape)
    loss, grad = np.where(keep, loss, 0.0), np.where(keep, grad, 0.0)
    return float(loss.sum()), float((depth > 0).sum()), grad.reshape(np.asarray(logits).shape)
