"""The checker of the Soft-NMS tests: the definition (include/odtk_hip.h: odtk_soft_nms), restated round by round in numpy float32
(elementwise over the candidates a round visits) and independent of odtk.box._soft_nms_cpu.  Every float32 operation of the definition is one numpy float32 operation here, in
the same order; the Gaussian factor is `np.float32(math.exp(float(x)))`, the double exp rounded once.

A double exp is only good to about an ulp, on the host as on the device, so a Gaussian case can be compared BIT FOR BIT only
if none of its exp results lies within a few double ulps of a float32 rounding boundary (the midpoint of two neighbouring
float32 values): `soft_nms_ref` returns the smallest such distance it met, in double ulps, and `ADMIT_ULPS` is what a bit
test asks of its inputs.  This is a condition on the inputs, never a tolerance on the outputs."""
import math

import numpy as np

ADMIT_ULPS = 8.0
F = np.float32


def _boundary_distance_ulps(d):
    """Distance of the double `d` to the nearest float32 rounding boundary, in ulps of `d`."""
    f = F(d)
    if not np.isfinite(f):
        return math.inf
    up, dn = np.nextafter(f, F(np.inf)), np.nextafter(f, F(-np.inf))
    hi = (float(f) + float(up)) / 2 if np.isfinite(up) else math.inf
    lo = (float(f) + float(dn)) / 2
    return min(hi - d, d - lo) / math.ulp(d)


def soft_nms_image(scores, boxes, classes, thresh, ndet, method, sigma, min_score):
    """One image.  scores [n], boxes [n, 4], classes [n] float32 -> (scores [ndet], boxes [ndet, 4], classes [ndet], positions
    [ndet] int32 (-1 = unused), smallest distance of an exp result to a float32 rounding boundary in double ulps (inf: none))."""
    assert method in ('linear', 'gaussian')
    scores, boxes, classes = (np.ascontiguousarray(a, dtype=F) for a in (scores, boxes, classes))
    thresh, sigma, min_score, one = F(thresh), F(sigma), F(min_score), F(1)
    out_s, out_b, out_c = np.zeros(ndet, F), np.zeros((ndet, 4), F), np.zeros(ndet, F)
    out_i = np.full(ndet, -1, np.int32)
    w = scores.copy()
    alive = w > 0
    margin = math.inf
    with np.errstate(all='ignore'):
        area = (boxes[:, 2] - boxes[:, 0] + one) * (boxes[:, 3] - boxes[:, 1] + one)
        for r in range(ndet):
            # pick: largest w, lowest position (argmax returns the first of equal maxima)
            idx = np.flatnonzero(alive)
            if idx.size == 0:
                break
            i = idx[np.argmax(w[idx])]
            out_s[r], out_b[r], out_c[r], out_i[r] = w[i], boxes[i], classes[i], i
            alive[i] = False
            # decay: every alive candidate of the pick's class (one float32 operation per line and element)
            js = np.flatnonzero(alive & (classes == classes[i]))
            if js.size == 0:
                continue
            lx, ly = np.maximum(boxes[js, 0], boxes[i, 0]), np.maximum(boxes[js, 1], boxes[i, 1])
            hx, hy = np.minimum(boxes[js, 2], boxes[i, 2]), np.minimum(boxes[js, 3], boxes[i, 3])
            inter = _clamp0(hx - lx + one) * _clamp0(hy - ly + one)
            iou = inter / (area[js] + area[i] - inter)
            assert iou.dtype == F
            if method == 'linear':
                hit = ~(iou <= thresh)
                w[js[hit]] = w[js[hit]] * (one - iou[hit])
            else:
                sq = iou * iou
                x = (-sq) / sigma
                factor = np.ones(js.size, F)                     # math.exp(+-0.0) is exactly 1.0
                for k in np.flatnonzero(x != 0):                 # (a NaN is != 0)
                    if np.isnan(x[k]):
                        factor[k] = np.nan
                        continue
                    d = math.exp(float(x[k]))
                    margin = min(margin, _boundary_distance_ulps(d))
                    factor[k] = F(d)
                w[js] = w[js] * factor
            alive[js] = w[js] >= min_score
    return out_s, out_b, out_c, out_i, margin


def _clamp0(v):
    return np.where(v < 0, F(0), v)                             # torch's clamp(0): a NaN stays


def soft_nms_ref(scores, boxes, classes, thresh, ndet, method, sigma, min_score):
    """Batch form: [B, n] / [B, n, 4] / [B, n] -> (scores [B, ndet], boxes [B, ndet, 4], classes [B, ndet], positions [B, ndet],
    smallest exp margin over the batch in double ulps)."""
    parts = [soft_nms_image(s, b, c, thresh, ndet, method, sigma, min_score) for s, b, c in zip(scores, boxes, classes)]
    return tuple(np.stack([p[k] for p in parts]) for k in range(4)) + (min([p[4] for p in parts], default=math.inf),)


def random_case(seed, batch, count, num_classes, extent=96.0, padding=0.25):
    """Seeded candidates for the tests: `count` boxes per image with whole-pixel corners inside an `extent`-pixel square (so
    same-class boxes overlap often), `num_classes` classes, distinct scores in (0.05, 1) except that about `padding` of the
    positions -- anywhere in the list -- hold padding (score 0 or negative)."""
    rng = np.random.default_rng(seed)
    xy = np.floor(rng.random((batch, count, 2)) * extent)
    wh = np.floor(rng.random((batch, count, 2)) * extent / 3) + 2
    boxes = np.concatenate([xy, xy + wh], 2).astype(F)
    classes = rng.integers(0, num_classes, (batch, count)).astype(F)
    scores = (0.05 + 0.95 * rng.random((batch, count))).astype(F)
    pad = rng.random((batch, count)) < padding
    scores[pad] = np.where(rng.random(int(pad.sum())) < 0.5, F(0), F(-1))
    return scores, boxes, classes


_trained = {}


def trained_reference(golden_dir, method):
    """(inputs, checker outputs) for the trained detector's candidates (tests/golden/nms_trained_scenes_ties.npz: 16 images, up
    to 2552 candidates each) at nms 0.5, sigma 0.5, min_score 0.05, 100 detections; computed once per process."""
    import os
    if method not in _trained:
        with np.load(os.path.join(golden_dir, 'nms_trained_scenes_ties.npz')) as z:
            inputs = (z['scores'], z['boxes'], z['classes'])
        _trained[method] = (inputs, soft_nms_ref(*inputs, 0.5, 100, method, 0.5, 0.05))
    return _trained[method]
