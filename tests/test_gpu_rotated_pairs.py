"""The rotated box-pair test (csrc/rotated_iou.hpp) on the GPU, at every place that evaluates it, on the directed inputs of
tests/rotated_pairs_ref.py -- the boundary of the distance reject, improper kept quads, (sin, cos) far from unit norm, clips
that emit more than 8 vertices, NaN intersections and unions, non-finite fields.  tests/test_rotated_pairs.py proves on the
CPU that those inputs reach what they claim to.

Everything is compared against the C oracle (c_oracle.nms / rotated_overlap / iou_pairs), which has no reject and clips every
pair: kept indices equal, every output bit equal.  The float32 restatement of the reject is used here only to CHOOSE which
pairs of a generator go into a layout (the ones next to the boundary first); it never decides an expected value.

NaN: the pairwise IoU is compared by NaN mask plus the bits of everything that is not NaN (a NaN produced by 0 / 0 or
inf - inf has the sign bit set on an x86 host and clear on the GPU; neither carries a payload).  NMS outputs are copies of
input fields, so they are compared bit for bit, NaN included.

Which of the call sites evaluated a pair is fixed by the candidate's RANK in its image (scores are tie-free):
  * rotated_sup_matrix_kernel covers the pairs among the first m_max ranks of the first round,
      m_max = min(8 * ndet, count, 1024) rounded up to 64                      (nms.hip: rotated_matrix_rows)
    in one launch, or -- when m_first = max(256, ceil64(2.5 * ndet)) < m_max   (nms.hip: rotated_matrix_first) -- in two: the
    tiles whose column block ends at or below m_first first, the rest only for images that kept fewer than ndet boxes
    among their first m_first candidates;
  * behind m_max the resolve kernel walks the round (all candidates when count <= kNmsRound = 1024) in chunks of 64 ranks:
    a chunk is first pulled against the whole kept list (`rows` = false branch of pair_phase), then its own pairs
    (i < j, both alive) are evaluated (`rows` = true branch)."""
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle
from odtk import _C
import rotated_pairs_ref as ref

pytestmark = pytest.mark.gpu

K_NMS_ROUND = 1024


def matrix_rows(count, ndet):
    """nms.hip: rotated_matrix_rows (the LDS clamp -- m * (m / 64) * 8 bytes <= 16 clip regions of 4 KiB -- included)."""
    m = min(8 * ndet, count, K_NMS_ROUND)
    m = (m + 63) // 64 * 64
    while m > 64 and m * (m // 64) * 8 > 16 * 4096:
        m -= 64
    return m


def matrix_first(m_max, ndet):
    """nms.hip: rotated_matrix_first."""
    return min(m_max, (max(256, ndet * 5 // 2) + 63) // 64 * 64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gpu_nms(scores, boxes, classes, thr, ndet, own):
    s, b, c = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (scores, boxes, classes))
    batch, count = scores.shape
    if not own:
        out = _C.nms(s, b, c, thr, ndet, True, return_indices=True)
    else:
        lib = _C.library()
        out = [torch.empty(batch, ndet, device='cuda'), torch.empty(batch, ndet, 6, device='cuda'),
               torch.empty(batch, ndet, device='cuda'), torch.empty(batch, ndet, dtype=torch.int32, device='cuda')]
        flags = _C.FLAG_ROTATED | _C.FLAG_ROTATED_NMS_FIXED_ANGLE
        size = lib.odtk_nms_ex(batch, None, None, 4, count, ndet, thr, flags, None, 0, None)      # two-phase: query, then call
        assert size > 0
        ws = torch.empty(size, dtype=torch.uint8, device='cuda')
        rc = lib.odtk_nms_ex(batch, _C._ptrs([s, b, c]), _C._ptrs(out), 4, count, ndet, thr, flags, ws.data_ptr(), size,
                             torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def assert_equals_oracle(out, scores, boxes, classes, thr, ndet, own):
    want = c_oracle.nms(scores, boxes, classes, thr, ndet, rotated=True, own_angle=own)
    got_i = out[3].astype(np.int64)
    if not np.array_equal(got_i, want[3]):
        img = int(np.flatnonzero((got_i != want[3]).any(1))[0])
        raise AssertionError('kept indices differ in %d images, first image %d (thr %g, own %s):\n  got  %s\n  want %s' % (
            (got_i != want[3]).any(1).sum(), img, thr, own, got_i[img], want[3][img]))
    for h, r in zip(out[:3], want[:3]):
        assert np.array_equal(bits(h), bits(r))
    return want


# ---------------------------------------------------------------------------------------------------------------------
# which pairs of the generators a test takes
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def generator(name, own):
    """(m, j, cats) -- cats: disjoint index sets of the pairs a call site must not miss (next to the boundary of the reject,
    kept quads that are not proper, verdicts that depend on the mode, degenerate clips by kind, non-finite fields).  Read-only."""
    m, j = ref.all_generators(own)[name]
    far, bound, proper = ref.far_apart_terms(m, j, own)
    with np.errstate(all='ignore'):
        ratio = far.astype(np.float64) / bound.astype(np.float64)
    if name == 'degenerate':
        st = np.array([c_oracle.rotated_overlap_stats(a, b, own)[1:] for a, b in zip(m, j)])
        over, nan_i, nan_u, cross = st[:, 0] > 8, st[:, 1] != 0, st[:, 2] != 0, st[:, 3] != 0
        masks = [over & cross, over & ~cross, nan_i & nan_u, nan_i & ~nan_u & ~over]
    elif name == 'own_angle':
        masks = [ref.far_apart(m, j, 0.0, True) != ref.far_apart(m, j, 0.0, False)]
    elif name == 'improper':
        masks = [~proper & (ratio > 1.0)]
    elif name == 'nonfinite':
        masks = [np.ones(len(m), bool)]
    else:
        masks = [np.abs(ratio - 1.0) <= 0.05]
    cats = tuple(np.flatnonzero(k) for k in masks if k.any())
    for a in (m, j) + cats:
        a.setflags(write=False)
    return m, j, cats


def _thin(idx, n):
    return idx[np.linspace(0, len(idx) - 1, n).astype(int)] if n else idx[:0]


def take(name, own, n):
    """n pairs of one generator (all of it if it has fewer): up to three quarters from the index sets above, in equal shares,
    each evenly thinned; the rest from the other pairs, evenly thinned."""
    m, j, cats = generator(name, own)
    if len(m) <= n:
        return m, j
    hot = np.zeros(len(m), bool)
    for c in cats:
        hot[c] = True
    rest = np.flatnonzero(~hot)
    left = min(int(hot.sum()), max(n * 3 // 4, n - len(rest)))
    picked = []
    for ci, c in enumerate(sorted(cats, key=len)):             # (the small sets first: what they cannot fill goes to the others)
        q = min(len(c), left // (len(cats) - ci))
        picked.append(_thin(c, q))
        left -= q
    n_hot = sum(len(p) for p in picked)
    idx = np.concatenate(picked + [_thin(rest, n - n_hot)])
    assert len(idx) == n and len(set(idx.tolist())) == n
    return m[idx], j[idx]


def mixed_pairs(own, n):
    """n pairs, a sixth from every generator."""
    parts = [take(name, own, n // 6 + 1) for name in ('boundary', 'norm', 'improper', 'own_angle', 'degenerate', 'nonfinite')]
    m, j = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    idx = np.linspace(0, len(m) - 1, n).astype(int)
    assert len(set(idx)) == n
    return m[idx], j[idx]


# ---------------------------------------------------------------------------------------------------------------------
# matrix site
# ---------------------------------------------------------------------------------------------------------------------
def pairs_per_image(m, j, k, seed):
    """Images of k pairs each: the same class within a pair, distinct classes across the pairs of an image, tie-free scores
    with m above j, candidates at shuffled positions.  Slots of the last image that have no pair get score 0."""
    rng = np.random.default_rng(seed)
    n = len(m)
    batch, count = (n + k - 1) // k, 2 * k
    scores, boxes, classes = np.zeros((batch, count), np.float32), np.zeros((batch, count, 6), np.float32), np.zeros((batch, count), np.float32)
    for b in range(batch):
        vals = (rng.permutation(count) + 1).astype(np.float32) / np.float32(count + 1)
        pos = rng.permutation(count)
        for p in range(min(k, n - b * k)):
            hi, lo = max(vals[2 * p], vals[2 * p + 1]), min(vals[2 * p], vals[2 * p + 1])
            pm, pj = pos[2 * p], pos[2 * p + 1]
            scores[b, pm], scores[b, pj] = hi, lo
            boxes[b, pm], boxes[b, pj] = m[b * k + p], j[b * k + p]
            classes[b, pm] = classes[b, pj] = p
    return scores, boxes, classes


@pytest.mark.parametrize('own', [False, True])
@pytest.mark.parametrize('name', ['boundary', 'norm', 'improper', 'own_angle', 'degenerate', 'nonfinite'])
def test_matrix_site_equals_oracle(name, own):
    """Few candidates per image (count = 16 <= m_max = 64): every pair is evaluated by rotated_sup_matrix_kernel."""
    k = 8
    m, j = take(name, own, 2400)
    scores, boxes, classes = pairs_per_image(m, j, k, 7)
    count, ndet = 2 * k, 2 * k
    assert count <= matrix_rows(count, ndet) == 64 and matrix_first(64, ndet) == 64          # one matrix launch covers the image
    assert scores.shape[0] <= 320
    for thr in (0.0, 0.3, 1.0, -0.1):
        out = gpu_nms(scores, boxes, classes, thr, ndet, own)
        want = assert_equals_oracle(out, scores, boxes, classes, thr, ndet, own)
        if thr < 0 and name == 'boundary':
            # the reject is off: every j goes, the far ones included (finite proper quads: overlap >= 0 > thr) -- but for the
            # few tiny boxes at 1e5 whose fp32 shoelace areas cancel to 0 (0 / 0: NaN suppresses nothing)
            n_nan = sum(np.isnan(c_oracle.rotated_overlap(a, b, own)) for a, b in zip(m, j))
            assert n_nan <= 4 and (want[3] >= 0).sum() == len(m) + n_nan
            assert ref.far_apart(m, j, 0.0, own).sum() >= 256 and not ref.far_apart(m, j, thr, own).any()


# ---------------------------------------------------------------------------------------------------------------------
# in-workgroup queue sites
# ---------------------------------------------------------------------------------------------------------------------
def anchor_and_duplicates(n, seed):
    """A 90 x 60 box at an angle and n - 1 copies of it shifted by up to 3 px: overlap with the original > 0.85 in either mode."""
    rng = np.random.default_rng(seed)
    cx, cy = rng.uniform(100.0, 900.0, 2)
    a = rng.uniform(-3.0, 3.0)
    d = rng.uniform(-3.0, 3.0, (n, 2))
    d[0] = 0
    return ref.box6(cx + d[:, 0], cy + d[:, 1], 90.0, 60.0, np.sin(a), np.cos(a))


def ranked_image(ranked_boxes, ranked_classes, count, rng):
    """Candidates given in rank order -> (scores, boxes, classes) of one image at shuffled positions, tie-free scores."""
    n = len(ranked_boxes)
    scores, boxes, classes = np.zeros(count, np.float32), np.zeros((count, 6), np.float32), np.zeros(count, np.float32)
    pos = rng.permutation(count)[:n]
    scores[pos] = np.float32(1.0) - np.arange(n, dtype=np.float32) * np.float32(1.0 / 1024)
    boxes[pos], classes[pos] = ranked_boxes, ranked_classes
    return scores, boxes, classes


def ranks_of(scores):
    order = np.argsort(-scores, kind='stable')
    rank = np.empty(len(scores), np.int64)
    rank[order] = np.arange(len(scores))
    return rank


@pytest.mark.parametrize('own', [False, True])
@pytest.mark.parametrize('site', ['rows', 'kept'])
def test_queue_sites_equal_oracle(site, own):
    """ndet = 8 gives m_max = min(64, count, 1024) = 64: the suppression matrix ends at rank 64.  Ranks 0..63 are one box of
    class 0 and 63 near-copies of it (the matrix removes them; one kept box).  Everything from rank 64 on -- count <=
    kNmsRound, so the whole image is ONE round -- is resolved chunk by chunk (c0 = 64, 128, ...) through pair_phase:
      'rows'  m and j lie in the same chunk [64, 128): both survive the pull (no kept box of their class), so the pair is
              evaluated by the rows = true branch;
      'kept'  m lies in chunk [64, 128) and is kept there, j in chunk [128, 192): the pull of that chunk against the kept
              list evaluates the pair in the rows = false branch.
    The other ranks are more near-copies of the class-0 box (they die in the pull and keep nothing).  Three pairs per image:
    1 + 2 * 3 = 7 < ndet kept boxes at most, so the NMS never stops before a pair's verdict shows."""
    ndet, per, batch = 8, 3, 128
    count = 160 if site == 'rows' else 200
    m_max = matrix_rows(count, ndet)
    assert m_max == 64 and 8 * ndet <= 64 and count <= K_NMS_ROUND and 1 + 2 * per < ndet
    m, j = mixed_pairs(own, per * batch)
    rng = np.random.default_rng(11)
    S, Bx, C, where = [], [], [], []
    for b in range(batch):
        n_rank = count - 7                                    # (a few slots stay empty: score 0)
        rb = anchor_and_duplicates(n_rank, 100 + b)
        rc = np.zeros(n_rank, np.float32)
        for p in range(per):
            rm = 64 + 3 + 21 * p                              # 67, 88, 109
            rj = rm + 1 + 5 * p if site == 'rows' else 128 + 2 + 23 * p + (b % 3)
            rb[rm], rb[rj] = m[b * per + p], j[b * per + p]
            rc[rm] = rc[rj] = 1 + p
            where.append((b, rm, rj))
        s, bx, c = ranked_image(rb, rc, count, rng)
        rank = ranks_of(s)
        for p in range(per):                                  # the position arithmetic the docstring derives
            pm = int(np.flatnonzero((c == 1 + p) & (s > 0))[0]), int(np.flatnonzero((c == 1 + p) & (s > 0))[1])
            r_m, r_j = sorted((rank[pm[0]], rank[pm[1]]))
            assert r_m >= m_max and r_j >= m_max
            assert (r_m // 64 == r_j // 64 == 1) if site == 'rows' else (r_m // 64 == 1 and r_j // 64 == 2)
        S.append(s), Bx.append(bx), C.append(c)
    scores, boxes, classes = np.stack(S), np.stack(Bx), np.stack(C)
    for thr in (0.0, 0.3, -0.1):
        out = gpu_nms(scores, boxes, classes, thr, ndet, own)
        want = assert_equals_oracle(out, scores, boxes, classes, thr, ndet, own)
        assert ((want[3] >= 0).sum(1) < ndet).all()           # no image ran out of detections: every verdict is visible
        assert ((want[2] == 0) & (want[3] >= 0)).sum(1).max() == 1   # the copies all went


# ---------------------------------------------------------------------------------------------------------------------
# two-step matrix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('own', [False, True])
def test_two_step_matrix_equals_oracle(own):
    """ndet = 40, count = 384: m_max = min(320, 384) = 320 and m_first = max(256, 100) = 256 < m_max, so the matrix is written
    in two launches.  Three kinds of images in one batch:
      S   340 candidates, at most 1 + 2 * 19 = 39 < ndet of them can be kept: the first resolve stops at rank 256 with
          kept < ndet, the second matrix launch writes the tiles of column block [256, 320) and the second resolve redoes the
          round.  Eleven pairs have m at a rank below 256 and j in [256, 320); eight have both in [256, 320): row blocks 0..3
          and row block 4 of the second launch's tiles.  Ranks 320..339 go through the chunk loop.
      F   19 pairs at ranks 0..37, then 62 far-apart boxes of classes of their own: 40 boxes are kept within the first
          256 candidates, the first resolve finishes the image (done = 1) and the second launch skips it.
      G   24 candidates only (12 pairs): the round is shorter than m_first, the first step covers it whole."""
    ndet, count = 40, 384
    m_max = matrix_rows(count, ndet)
    m_first = matrix_first(m_max, ndet)
    assert (m_max, m_first) == (320, 256)
    n_s, n_f, n_g = 20, 6, 6
    m, j = mixed_pairs(own, 19 * n_s + 19 * n_f + 12 * n_g)
    rng = np.random.default_rng(13)
    S, Bx, C, kinds = [], [], [], []
    at = 0
    order = ['S'] * n_s + ['F'] * n_f + ['G'] * n_g
    order = [order[i] for i in np.random.default_rng(5).permutation(len(order))]
    for b, kind in enumerate(order):
        if kind == 'S':
            rb = anchor_and_duplicates(340, 300 + b)
            rc = np.zeros(340, np.float32)
            slots = [(10 + 20 * i, 256 + 2 * i) for i in range(11)] + [(280 + 4 * q, 281 + 4 * q + (q & 1)) for q in range(8)]
            assert all(rm < rj and 256 <= rj < 320 for rm, rj in slots) and sum(rm >= 256 for rm, _ in slots) == 8
            assert len(set(sum(slots, ()))) == 38
        elif kind == 'F':
            far = ref.box6(5000.0 + 400.0 * np.arange(62), -3000.0, 50.0, 30.0, np.sin(0.5), np.cos(0.5))
            rb = np.concatenate([np.zeros((38, 6), np.float32), far])
            rc = np.concatenate([np.zeros(38, np.float32), 100 + np.arange(62, dtype=np.float32)])
            slots = [(2 * p, 2 * p + 1) for p in range(19)]
        else:
            rb, rc = np.zeros((24, 6), np.float32), np.zeros(24, np.float32)
            slots = [(2 * p, 2 * p + 1) for p in range(12)]
        for p, (rm, rj) in enumerate(slots):
            rb[rm], rb[rj] = m[at], j[at]
            rc[rm] = rc[rj] = 1 + p
            at += 1
        s, bx, c = ranked_image(rb, rc, count, rng)
        S.append(s), Bx.append(bx), C.append(c), kinds.append(kind)
    assert at == len(m)
    scores, boxes, classes = np.stack(S), np.stack(Bx), np.stack(C)
    kinds = np.array(kinds)
    for thr in (0.0, 0.3):
        out = gpu_nms(scores, boxes, classes, thr, ndet, own)
        want = assert_equals_oracle(out, scores, boxes, classes, thr, ndet, own)
        kept = (want[3] >= 0).sum(1)
        assert (kept[kinds == 'S'] < ndet).all() and (kept[kinds == 'G'] < ndet).all()     # S needs the second step
        assert (kept[kinds == 'F'] == ndet).all()
        for b in np.flatnonzero(kinds == 'F'):                # ... and F finishes inside the first m_first ranks
            assert ranks_of(scores[b])[want[3][b]].max() < m_first


# ---------------------------------------------------------------------------------------------------------------------
# pairwise IoU
# ---------------------------------------------------------------------------------------------------------------------
def raw_quads():
    """Corner quads that no [x1, y1, x2, y2, sin, cos] box can express."""
    sq = np.array([10, 10, 50, 10, 50, 40, 10, 40], np.float32)
    q = [sq,
         sq.reshape(4, 2)[::-1].reshape(8),                                        # reversed vertex order
         np.array([10, 10, 50, 40, 50, 10, 10, 40], np.float32),                   # self-intersecting bow-tie
         np.array([16, 16, 32, 16, 48, 16, 24, 40], np.float32),                   # three collinear corners
         np.array([0, 0, 8, 8, 16, 16, 0, 16], np.float32),
         np.array([24, 24, 24, 24, 24, 24, 24, 24], np.float32),                   # all four corners equal
         np.array([30, 20, 30, 20, 30, 20, 30, 20], np.float32),
         np.array([12, 12, 44, 12, 44, 36, 12, 36], np.float32)]
    for k in range(8):                                                             # a NaN in one coordinate
        nan = sq.copy()
        nan[k] = np.nan
        q.append(nan)
    inf = sq.copy()
    inf[2] = np.inf
    q.append(inf)
    return np.stack(q)


def assert_iou_equals_oracle(boxes, anchors):
    out = _C.iou(torch.from_numpy(boxes).cuda().reshape(-1), torch.from_numpy(anchors).cuda().reshape(-1))[0].cpu().numpy()
    want = c_oracle.iou_pairs(boxes, anchors)
    assert out.shape == want.shape == (len(anchors), len(boxes))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out), nan)                 # NaN by mask (module docstring) ...
    assert np.array_equal(bits(out)[~nan], bits(want)[~nan])  # ... every other value bit for bit
    return want


@pytest.mark.parametrize('name', ['boundary', 'norm', 'improper', 'own_angle', 'degenerate', 'nonfinite'])
def test_pairwise_iou_equals_oracle(name):
    """The corner quads of the generators' boxes (each turned by its own angle), all of one side against all of the other, in
    both orders of subject and clipper, with the raw quads on both sides."""
    m, j = take(name, True, 90)
    with np.errstate(all='ignore'):                            # (non-finite fields, coordinates of 2^62)
        qm = np.stack([c_oracle.box6_to_quad(b) for b in m]).reshape(-1, 8).astype(np.float32)
        qj = np.stack([c_oracle.box6_to_quad(b) for b in j]).reshape(-1, 8).astype(np.float32)
    a, b = np.concatenate([qm, raw_quads()]), np.concatenate([qj, raw_quads()])
    assert len(a) * len(b) <= 12000
    w1 = assert_iou_equals_oracle(a, b)
    w2 = assert_iou_equals_oracle(b, a)
    if name == 'degenerate':                                   # the pairs themselves sit on the diagonal: the cap and the NaN rules ran
        st = [c_oracle.rotated_overlap_stats(x, y, True) for x, y in zip(m, j)]
        assert sum(s[1] > 8 for s in st) >= 16 and sum(s[2] for s in st) >= 16 and sum(s[2] and s[3] for s in st) >= 4
        assert (np.diag(w1)[:len(m)] == 1.0).sum() >= 4
    if name == 'nonfinite':
        assert np.isnan(w1).any() and np.isnan(w2).any()
