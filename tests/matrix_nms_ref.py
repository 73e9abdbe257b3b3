"""The checker of the Matrix NMS tests: the definition (include/odtk_hip.h: odtk_matrix_nms) restated in numpy float32 over the
full n x n matrices of the participants, independent of odtk.box._matrix_nms_cpu.  Every float32 operation of the definition
is one numpy float32 operation here, in the same order, and the two reductions are written as the definition states them:
`acc = iou > acc ? iou : acc` and `acc = d < acc ? d : acc`, row after row.  The Gaussian factor is the double exp rounded once.

As in soft_nms_ref, a Gaussian case can be compared BIT FOR BIT only if none of its exp results lies within a few double ulps
of a float32 rounding boundary: `matrix_nms_ref` returns the smallest such distance it met over the pairs of the definition, in
double ulps, and a bit test asks `soft_nms_ref.ADMIT_ULPS` of its inputs.  A condition on the inputs, never a tolerance."""
import math

import numpy as np

from soft_nms_ref import ADMIT_ULPS, random_case, trained_reference   # noqa: F401  (the tests take them from here)

F = np.float32


def _clamp0(v):
    return np.where(v < 0, v.dtype.type(0), v)                  # torch's clamp(0): a NaN stays


def _boundary_distance_ulps(d):
    """Distances of the doubles `d` to the nearest float32 rounding boundary, in ulps of each `d` (inf where there is none)."""
    with np.errstate(all='ignore'):
        f = d.astype(F)
        up, dn = np.nextafter(f, F(np.inf)), np.nextafter(f, F(-np.inf))
        hi = (f.astype(np.float64) + up.astype(np.float64)) / 2
        lo = (f.astype(np.float64) + dn.astype(np.float64)) / 2
        dist = np.minimum(hi - d, d - lo) / np.spacing(d)
    return np.where(np.isfinite(f) & np.isfinite(up) & (f > 0), dist, np.inf)


def participants(scores, pre_top):
    """Input positions of the participants in rank order: score > 0, score descending, ties by lowest position, the first pre_top."""
    pos = np.flatnonzero(scores > 0)                            # (a NaN is not)
    return pos[np.lexsort((pos, -scores[pos]))][:pre_top]


def decay_of(scores, boxes, classes, method, sigma, pre_top, dtype=F):
    """The participants' positions (rank order), their decay factors in `dtype` arithmetic (float32: the definition; float64: what
    the float32 rounding is measured against) and the smallest exp margin."""
    assert method in ('linear', 'gaussian')
    T = dtype
    scores = np.ascontiguousarray(scores, dtype=F)
    order = participants(scores, pre_top)
    n = order.size
    b, c = np.ascontiguousarray(boxes, dtype=F)[order].astype(T), np.ascontiguousarray(classes, dtype=F)[order]
    one, sigma = T(1), T(sigma)
    margin = math.inf
    with np.errstate(all='ignore'):
        area = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
        lx, ly = np.maximum(b[:, None, 0], b[None, :, 0]), np.maximum(b[:, None, 1], b[None, :, 1])
        hx, hy = np.minimum(b[:, None, 2], b[None, :, 2]), np.minimum(b[:, None, 3], b[None, :, 3])
        inter = _clamp0(hx - lx + one) * _clamp0(hy - ly + one)
        iou = inter / ((area[None, :] + area[:, None]) - inter)          # [row i, column j]
        assert iou.dtype == T
        del lx, ly, hx, hy, inter
        pair = np.triu(np.ones((n, n), bool), 1) & (c[:, None] == c[None, :])   # row i ranks before column j, one class
        cmax = np.zeros(n, T)
        for i in range(n):                                       # acc = iou > acc ? iou : acc
            m = pair[i] & (iou[i] > cmax)
            cmax[m] = iou[i][m]
        if method == 'linear':
            d = (one - iou) / (one - cmax)[:, None]
        else:
            x = ((cmax * cmax)[:, None] - iou * iou) / sigma
            d64 = np.exp(x.astype(np.float64))
            d = d64.astype(T)
            if T is F:
                real = pair & (x != 0) & ~np.isnan(x)            # exp(+-0) is exactly 1
                if real.any():
                    margin = float(_boundary_distance_ulps(d64[real]).min())
            del x, d64
        assert d.dtype == T
        decay = np.ones(n, T)
        for i in range(n):                                       # acc = d < acc ? d : acc
            m = pair[i] & (d[i] < decay)
            decay[m] = d[i][m]
    return order, decay, margin


def matrix_nms_image(scores, boxes, classes, ndet, method, sigma, min_score, pre_top):
    """One image.  scores [n], boxes [n, 4], classes [n] float32 -> (scores [ndet], boxes [ndet, 4], classes [ndet], positions
    [ndet] int32 (-1 = unused), smallest distance of an exp result to a float32 rounding boundary in double ulps (inf: none))."""
    scores, boxes, classes = (np.ascontiguousarray(a, dtype=F) for a in (scores, boxes, classes))
    out_s, out_b, out_c = np.zeros(ndet, F), np.zeros((ndet, 4), F), np.zeros(ndet, F)
    out_i = np.full(ndet, -1, np.int32)
    order, decay, margin = decay_of(scores, boxes, classes, method, sigma, pre_top)
    with np.errstate(all='ignore'):
        decayed = scores[order] * decay
    assert decayed.dtype == F
    alive = np.flatnonzero(decayed >= F(min_score))
    alive = alive[np.lexsort((order[alive], -decayed[alive]))][:ndet]    # decayed score descending, ties by lowest position
    k = alive.size
    out_s[:k], out_b[:k], out_c[:k], out_i[:k] = decayed[alive], boxes[order[alive]], classes[order[alive]], order[alive]
    return out_s, out_b, out_c, out_i, margin


def matrix_nms_ref(scores, boxes, classes, ndet, method, sigma, min_score, pre_top):
    """Batch form: [B, n] / [B, n, 4] / [B, n] -> (scores [B, ndet], boxes [B, ndet, 4], classes [B, ndet], positions [B, ndet],
    smallest exp margin over the batch in double ulps)."""
    parts = [matrix_nms_image(s, b, c, ndet, method, sigma, min_score, pre_top) for s, b, c in zip(scores, boxes, classes)]
    return tuple(np.stack([p[k] for p in parts]) for k in range(4)) + (min([p[4] for p in parts], default=math.inf),)


_trained = {}


def trained_matrix_reference(golden_dir, method):
    """(inputs, checker outputs) for the trained detector's candidates (the fixture soft_nms_ref.trained_reference loads) at
    sigma 0.5, min_score 0.05, 100 detections, pre_top 2000; computed once per process."""
    if method not in _trained:
        inputs = trained_reference(golden_dir, 'linear')[0]
        _trained[method] = (inputs, matrix_nms_ref(*inputs, 100, method, 0.5, 0.05, 2000))
    return _trained[method]
