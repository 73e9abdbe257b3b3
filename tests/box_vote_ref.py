"""The checker of the box-voting tests: the definition (include/odtk_hip.h: odtk_box_vote), restated in numpy and independent of
odtk.box.  The IoU is numpy float32, one operation per line as in tests/soft_nms_ref.py; the weighted mean of the voters is computed
EXACTLY (fractions.Fraction over the voters' float32 values, which are dyadic rationals) and rounded once to float32.

The definition leaves the order of the double-precision sums free, so an implementation may differ from the exact quotient.  With
v voters, M = sum s_j |b_jk| / sum s_j, every product exact in double (24 x 24 bits), numerator and denominator each carry at most
v roundings of relative size 2^-53 of the partial sums' magnitudes and the division one more: the double result is within
(2 v + 2) 2^-53 M of the exact quotient, under 2^-41 M for v <= 2048 (zeros added for non-voters are exact).  A coordinate is
ADMITTED when its exact value lies at least 2^-38 M -- eight times that bound -- from the nearest float32 rounding boundary: then
every such implementation rounds to the same float32.  Admitted coordinates must match bit for bit, the others within one float32
ulp; a bit test asserts `MAX_VOTERS` and `MAX_INADMISSIBLE` of its inputs.  These are conditions on the inputs, never a tolerance
on what was admitted.

Also here: the numpy restatement of the flip merge (odtk_concat_candidates) and the generator of clustered candidates -- boxes in
clusters of overlapping same-class boxes, as a trained detector emits them, so that detections have tens to thousands of voters
(soft_nms_ref.random_case's boxes almost never reach IoU 0.65: 1.0 - 1.1 voters per detection)."""
import os
from fractions import Fraction

import numpy as np

F = np.float32
MAX_VOTERS = 2048
MAX_INADMISSIBLE = 0.01                       # share of a case's compared coordinates
ADMIT = Fraction(1, 2 ** 38)                  # x M: distance to the nearest rounding boundary a coordinate needs


def _clamp0(v):
    return np.where(v < 0, F(0), v)           # torch's clamp(0): a NaN stays


def _exact_sum(values):
    """Exact sum of python floats as a Fraction (they are dyadic: one common power-of-two denominator)."""
    pairs = [float(v).as_integer_ratio() for v in values]
    den = max([d for _, d in pairs], default=1)
    return Fraction(sum(n * (den // d) for n, d in pairs), den)


def _round_f32(q):
    """(the float32 nearest to the Fraction q, ties to even; the distance of q to the nearest rounding boundary, a Fraction)."""
    f = F(float(q))                           # a double rounding can only be off by one float32: corrected below
    for _ in range(2):
        up, dn = np.nextafter(f, F(np.inf)), np.nextafter(f, F(-np.inf))
        hi, lo = (Fraction(float(f)) + Fraction(float(up))) / 2, (Fraction(float(f)) + Fraction(float(dn))) / 2
        even = (int(np.array(f).view(np.uint32)) & 1) == 0
        if q > hi or (q == hi and not even):
            f = up
        elif q < lo or (q == lo and not even):
            f = dn
        else:
            break
    return f, min(hi - q, q - lo)


def vote_image(scores, boxes, classes, kept, vote_thresh):
    """One image.  -> (boxes [d, 4] float32 correctly rounded, admitted [d, 4] bool, voters [d] int)."""
    scores, boxes, classes = (np.ascontiguousarray(a, dtype=F) for a in (scores, boxes, classes))
    n, d = scores.shape[0], len(kept)
    out, admitted, voters = np.zeros((d, 4), F), np.ones((d, 4), bool), np.zeros(d, np.int64)
    thr, one = F(vote_thresh), F(1)
    position = np.arange(n)
    with np.errstate(all='ignore'):
        area = (boxes[:, 2] - boxes[:, 0] + one) * (boxes[:, 3] - boxes[:, 1] + one)
        for r, p in enumerate(int(k) for k in kept):
            if p < 0 or p >= n:
                continue
            lx, ly = np.maximum(boxes[:, 0], boxes[p, 0]), np.maximum(boxes[:, 1], boxes[p, 1])
            hx, hy = np.minimum(boxes[:, 2], boxes[p, 2]), np.minimum(boxes[:, 3], boxes[p, 3])
            inter = _clamp0(hx - lx + one) * _clamp0(hy - ly + one)
            iou = inter / (area + area[p] - inter)
            assert iou.dtype == F
            js = np.flatnonzero((scores > 0) & (classes == classes[p]) & ((iou >= thr) | (position == p)))
            voters[r] = js.size
            assert js.size, 'a kept position must have a positive score and a class that equals itself'
            s = [float(v) for v in scores[js]]
            weight = _exact_sum(s)
            for k in range(4):
                b = [float(v) for v in boxes[js, k]]
                q = _exact_sum([si * bi for si, bi in zip(s, b)]) / weight        # (float32 x float32 is exact in double)
                m = _exact_sum([si * abs(bi) for si, bi in zip(s, b)]) / weight
                out[r, k], distance = _round_f32(q)
                admitted[r, k] = distance >= ADMIT * m
    return out, admitted, voters


def vote_ref(scores, boxes, classes, kept, vote_thresh):
    """Batch form: [B, n] / [B, n, 4] / [B, n] / kept [B, d] -> (boxes [B, d, 4], admitted [B, d, 4], voters [B, d])."""
    parts = [vote_image(s, b, c, k, vote_thresh) for s, b, c, k in zip(scores, boxes, classes, np.asarray(kept))]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3))


def assert_votes(got, ref, kept, what):
    """`got` [B, d, 4] float32 against vote_ref's result: the input conditions, bit equality where admitted, one ulp elsewhere."""
    boxes, admitted, voters = ref
    got = np.ascontiguousarray(got, dtype=F)
    assert got.shape == boxes.shape, (what, got.shape, boxes.shape)
    used = np.asarray(kept) >= 0
    assert int(voters.max(initial=0)) <= MAX_VOTERS, (what, int(voters.max()))
    compared = 4 * int(used.sum())
    inadmissible = int((~admitted).sum())
    assert inadmissible <= MAX_INADMISSIBLE * compared, (what, inadmissible, compared)
    same = got.view(np.uint32) == boxes.view(np.uint32)
    assert same[admitted].all(), (what, 'admitted coordinates differ', int((~same & admitted).sum()),
                                  got[~same & admitted][:4], boxes[~same & admitted][:4])
    near = same | (got == np.nextafter(boxes, F(np.inf))) | (got == np.nextafter(boxes, F(-np.inf)))
    assert near.all(), (what, 'beyond one ulp', got[~near][:4], boxes[~near][:4])
    return inadmissible, compared


def concat_ref(parts, mirror_widths):
    """The flip merge: parts of (scores [B, n_i], boxes [B, n_i, 4], classes [B, n_i]) as one list; a part with a width W > 0 has
    the boxes of its entries with score > 0 mapped back, x1' = (W - 1) - x2 and x2' = (W - 1) - x1 in float32."""
    merged = []
    for (scores, boxes, classes), width in zip(parts, mirror_widths):
        scores, boxes, classes = (np.ascontiguousarray(a, dtype=F) for a in (scores, boxes, classes))
        if width > 0:
            edge, positive = F(width - 1), scores > 0
            flipped = boxes.copy()
            flipped[..., 0] = np.where(positive, edge - boxes[..., 2], boxes[..., 0])
            flipped[..., 2] = np.where(positive, edge - boxes[..., 0], boxes[..., 2])
            boxes = flipped
        merged.append((scores, boxes, classes))
    return tuple(np.concatenate(t, 1) for t in zip(*merged))


def clustered_case(seed, batch, count, num_classes, clusters, extent=256.0, jitter=3.0, padding=0.25):
    """Seeded candidates in `clusters` clusters per image: jittered copies of a cluster's box, 90 % of them of the cluster's class,
    scores in (0.05, 1), about `padding` of the positions -- anywhere -- holding padding (score 0 or negative)."""
    rng = np.random.default_rng(seed)
    cxy = rng.random((batch, clusters, 2)) * extent; cwh = 16 + rng.random((batch, clusters, 2)) * extent / 4
    ccls = rng.integers(0, num_classes, (batch, clusters)); which = rng.integers(0, clusters, (batch, count)); ix = np.arange(batch)[:, None]
    xy = cxy[ix, which] + rng.normal(0, jitter, (batch, count, 2)); wh = cwh[ix, which] + rng.normal(0, jitter, (batch, count, 2))
    boxes = np.concatenate([xy, xy + np.maximum(wh, 1)], 2).astype(np.float32)
    classes = ccls[ix, which].astype(np.float32); other = rng.random((batch, count)) < 0.1
    classes[other] = rng.integers(0, num_classes, int(other.sum())).astype(np.float32)
    scores = (0.05 + 0.95 * rng.random((batch, count))).astype(np.float32); pad = rng.random((batch, count)) < padding
    scores[pad] = np.where(rng.random(int(pad.sum())) < 0.5, np.float32(0), np.float32(-1))
    return scores, boxes, classes


def concat_parts():
    """Three parts of unequal counts for the flip-merge tests, the first with padding at the front, in the middle and at the end."""
    a = clustered_case(60, 3, 37, 3, 3, padding=0.0)
    a[0][:, :9], a[0][:, 15:20], a[0][:, 30:] = 0, -1, 0             # padding at the front, in the middle and at the end
    a[0][1, 12] = np.nan                                              # (not > 0: copied as it is)
    b = clustered_case(61, 3, 64, 3, 3)
    c = clustered_case(62, 3, 1, 3, 1, padding=0.0)
    return [a, b, c]


def _empty_image_beside_a_full_one():
    s, b, c = clustered_case(21, 2, 700, 3, 6, padding=0.0)
    s[0] = 0
    return s, b, c


def _nan_iou():
    s, b, c = clustered_case(22, 1, 70, 2, 3, padding=0.1)
    b[0, 5], b[0, 66] = [5, 5, 4, 9], [5, 5, 4, 9]               # area 0 twice: their IoU is 0 / 0, the kept one votes alone
    c[0, 5] = c[0, 66] = 1
    s[0, 5], s[0, 66] = 0.99, 0.98
    return s, b, c


def _equal_scores_and_duplicates():
    s, b, c = clustered_case(23, 2, 300, 2, 4, padding=0.0)
    s[:] = F(0.5)
    # corners on eighths of a pixel: with equal weights the mean of 2, 4, .. such values is a float32 itself, where full-mantissa
    # corners would put every second mean of two exactly ON a rounding boundary (a tie), which the admission rule excludes
    b[:] = np.round(b * 8) / 8
    b[:, 150:] = b[:, :150]                                        # every box twice
    c[:, 150:] = c[:, :150]
    return s, b, c


# name -> (candidates, nms threshold of the suppression in front, detections_per_im, vote threshold).  The counts: one candidate;
# the wave boundary; a few strides of a wave; more detections than candidates; the workload's 5 x 1000 with 80 classes; 7681 = the
# suppression's workspace route; thousands of voters per detection.  Detection counts 1, 3 and 101 are fewer than, and no multiple
# of, the four detections of a workgroup.
CASES = {
    'count1': (lambda: clustered_case(1, 2, 1, 1, 1, padding=0.0), 0.5, 1, 0.65),
    'count63': (lambda: clustered_case(2, 2, 63, 2, 2), 0.5, 3, 0.65),
    'count64': (lambda: clustered_case(3, 2, 64, 2, 2), 0.5, 101, 0.65),
    'count65': (lambda: clustered_case(4, 2, 65, 2, 2), 0.5, 3, 0.65),
    'count257_vote05': (lambda: clustered_case(5, 2, 257, 3, 4), 0.5, 101, 0.5),
    'count1025_300': (lambda: clustered_case(6, 1, 1025, 4, 12), 0.5, 300, 0.65),
    'count5000_80_classes': (lambda: clustered_case(7, 3, 5000, 80, 60, extent=512.0), 0.5, 100, 0.65),
    'count7681': (lambda: clustered_case(8, 1, 7681, 8, 40, extent=512.0), 0.5, 100, 0.65),
    'count10000_vote08_300': (lambda: clustered_case(9, 1, 10000, 8, 50, extent=512.0), 0.5, 300, 0.8),
    '7680_one_class': (lambda: clustered_case(10, 1, 7680, 1, 3), 0.5, 101, 0.65),
    'empty_image_beside_a_full_one': (_empty_image_beside_a_full_one, 0.5, 100, 0.65),
    'nan_iou': (_nan_iou, 0.5, 100, 0.65),
    'equal_scores_and_duplicates': (_equal_scores_and_duplicates, 0.5, 101, 0.65),
    'vote_thresh_1': (lambda: clustered_case(24, 2, 400, 2, 3), 0.5, 100, 1.0),
}


def trained_candidates(golden_dir):
    """The trained detector's candidates (tests/golden/nms_trained_scenes_ties.npz: 16 images, up to 2552 candidates each)."""
    with np.load(os.path.join(golden_dir, 'nms_trained_scenes_ties.npz')) as z:
        return z['scores'], z['boxes'], z['classes']


_cache = {}


def cached_ref(key, scores, boxes, classes, kept, vote_thresh):
    """vote_ref once per process and `key` (the caller's name for these inputs AND this kept list); the result is shared
    between the tests that need it and must not be changed."""
    kept = np.asarray(kept)
    hit = _cache.get(key)
    if hit is None or not np.array_equal(hit[0], kept):
        hit = _cache[key] = (kept.copy(), vote_ref(scores, boxes, classes, kept, vote_thresh))
    return hit[1]
