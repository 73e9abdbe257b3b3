"""The checker of ATSS target assignment (odtk.box.atss_assign_levels, csrc/atss.hpp): the definition restated in numpy, on its
own -- nothing of odtk/box.py's torch branch is used -- plus the cases and the comparison rule that tests/test_atss.py (CPU
tensors) and tests/test_gpu_atss.py (the kernels) share.

There is no reference implementation to compare with, so the definition is the contract: every float32 step below is ONE numpy
float32 operation in the written order, the float64 part (mean, sample variance, threshold) is Python floats summed one after
the other in list order, and the candidates come from a full scan of every level (a stable argsort of all H * W distances).

Comparison rule (`compare`): depth, cls_target and the zero pattern of box_target exactly; the centre deltas (columns 0, 1) bit
for bit; the log deltas (columns 2, 3) within rtol = atol = 1e-6, the bound tests/test_gpu_target_shapes.py uses for them (the
three logs -- numpy, torch, the device -- may differ in the last place)."""
import functools
import math

import numpy as np

F = np.float32
RATIOS = [1.0, 2.0, 0.5]
SCALES = [4 * 2 ** (i / 3) for i in range(3)]
MAX_TOPK, MAX_ANCHORS, MAX_LEVELS = 16, 32, 6        # ODTK_ATSS_MAX_TOPK, ODTK_MAX_ANCHORS, ODTK_MAX_LEVELS
ROUND = 128                                          # kAtssRound: records staged in LDS at a time by the dense launch


def base_anchors(stride, ratios=RATIOS, scales=SCALES):
    """[A, 4] float32 base anchors around one stride x stride cell, scale-major (symmetric about the cell centre)."""
    out = []
    for sc in scales:
        for r in ratios:
            side = math.sqrt(stride * stride / r)
            w, h = side * sc, side * r * sc
            out.append([0.5 * (stride - w), 0.5 * (stride - h), 0.5 * (stride + w), 0.5 * (stride + h)])
    return np.asarray(out, dtype=F)


def _iou(a1x, a1y, a2x, a2y, x1, y1, x2, y2, area):
    """float32, +1 pixel convention; minimum / maximum propagate NaN like the kernel's tmin_nan / tmax_nan."""
    a_area = (a2x - a1x + F(1)) * (a2y - a1y + F(1))
    w = np.minimum(a2x, x2) - np.maximum(a1x, x1) + F(1)
    h = np.minimum(a2y, y2) - np.maximum(a1y, y1) + F(1)
    w = np.where(w < 0, F(0), w)
    h = np.where(h < 0, F(0), h)
    inter = w * h
    return inter / (a_area + area - inter)


def atss_reference(targets, levels, anchors, num_classes, topk):
    """targets [B, n_max, 5] float32 (x, y, w, h, class; class < 0: padding); levels [(H, W, stride)]; anchors per level [A, 4].
    -> dict(cls, box, depth: per level [B, A, C | 4 | 1, H, W] float32; and the facts the tests assert on: `assigned` anchors,
    anchors `contested` by two or more boxes, candidates `centre_rejected` (IoU over the threshold, cell centre not inside),
    `boxes_without_positives`, `assigned_per_level`, valid `boxes`)."""
    targets = np.asarray(targets, dtype=F)
    batch = targets.shape[0]
    a_count = anchors[0].shape[0]
    cls_t = [np.zeros((batch, a_count, num_classes, h, w), F) for h, w, _ in levels]
    box_t = [np.zeros((batch, a_count, 4, h, w), F) for h, w, _ in levels]
    depth_t = [np.zeros((batch, a_count, 1, h, w), F) for h, w, _ in levels]
    facts = dict(assigned=0, contested=0, centre_rejected=0, boxes_without_positives=0, boxes=0,
                 assigned_per_level=[0] * len(levels))
    with np.errstate(all='ignore'):
        for b in range(batch):
            rows = [r for r in targets[b] if r[4] > -1]       # (classes are whole numbers: the same rows as class >= 0)
            owner = [np.full((a_count, h * w), -1, np.int64) for h, w, _ in levels]
            best = [np.zeros((a_count, h * w), F) for h, w, _ in levels]
            claims = [np.zeros((a_count, h * w), np.int64) for h, w, _ in levels]
            for g, r in enumerate(rows):
                facts['boxes'] += 1
                x1, y1 = r[0], r[1]
                x2, y2 = r[0] + r[2] - F(1), r[1] + r[3] - F(1)
                area = (x2 - x1 + F(1)) * (y2 - y1 + F(1))
                bcx, bcy = x1 + F(0.5) * (x2 - x1 + F(1)), y1 + F(0.5) * (y2 - y1 + F(1))
                cand = []                                      # per level: (cells nearest first, IoU [k, A], centre inside [k])
                for (h, w, s), anc in zip(levels, anchors):
                    s = F(s)
                    px = np.arange(w).astype(F) * s + F(0.5) * s + F(0.5)
                    py = np.arange(h).astype(F) * s + F(0.5) * s + F(0.5)
                    dx, dy = px - bcx, py - bcy
                    d2 = ((dx * dx)[None, :] + (dy * dy)[:, None]).reshape(-1)
                    order = np.argsort(d2, kind='stable')[:min(topk, h * w)]     # full scan; ties to the lower cell; NaN last
                    order = order[~np.isnan(d2[order])]
                    yc, xc = order // w, order % w
                    gx, gy = xc.astype(F) * s, yc.astype(F) * s
                    iou = _iou(gx[:, None] + anc[None, :, 0], gy[:, None] + anc[None, :, 1], gx[:, None] + anc[None, :, 2],
                               gy[:, None] + anc[None, :, 3], x1, y1, x2, y2, area).astype(F)
                    cx, cy = px[xc], py[yc]
                    inside = (cx - x1 > F(0.01)) & (cy - y1 > F(0.01)) & (x2 - cx > F(0.01)) & (y2 - cy > F(0.01))
                    cand.append((order, iou, inside))
                listed = [float(v) for _, iou, _ in cand for v in iou.reshape(-1)]
                n = len(listed)
                positives = 0
                if n:
                    total = 0.0
                    for v in listed:
                        total = total + v
                    mean = total / n
                    squares = 0.0
                    for v in listed:
                        squares = squares + (v - mean) * (v - mean)
                    var = squares / (n - 1) if n > 1 else 0.0
                    thresh = mean + math.sqrt(var) if var == var else float('nan')
                    for l, (order, iou, inside) in enumerate(cand):
                        over = iou.astype(np.float64) >= thresh               # float64 comparison; NaN on either side: False
                        for j, a in np.argwhere(over):
                            cell = order[j]
                            if not inside[j]:
                                facts['centre_rejected'] += 1
                                continue
                            positives += 1
                            claims[l][a, cell] += 1
                            if owner[l][a, cell] < 0 or iou[j, a] > best[l][a, cell]:
                                owner[l][a, cell], best[l][a, cell] = g, iou[j, a]
                facts['boxes_without_positives'] += positives == 0
            for l, ((h, w, s), anc) in enumerate(zip(levels, anchors)):
                s = F(s)
                facts['contested'] += int((claims[l] >= 2).sum())
                hits = np.argwhere(owner[l] >= 0)
                facts['assigned'] += len(hits)
                facts['assigned_per_level'][l] += len(hits)
                for a, cell in hits:
                    r = rows[owner[l][a, cell]]
                    yc, xc = cell // w, cell % w
                    gx, gy = F(xc) * s, F(yc) * s
                    ax1, ay1, ax2, ay2 = gx + anc[a, 0], gy + anc[a, 1], gx + anc[a, 2], gy + anc[a, 3]
                    x1, y1 = r[0], r[1]
                    x2, y2 = r[0] + r[2] - F(1), r[1] + r[3] - F(1)
                    aw, ah = ax2 - ax1 + F(1), ay2 - ay1 + F(1)
                    acx, acy = ax1 + F(0.5) * aw, ay1 + F(0.5) * ah
                    bw, bh = x2 - x1 + F(1), y2 - y1 + F(1)
                    bcx, bcy = x1 + F(0.5) * bw, y1 + F(0.5) * bh
                    box_t[l][b, a, :, yc, xc] = [(bcx - acx) / aw, (bcy - acy) / ah, np.log(bw / aw), np.log(bh / ah)]
                    depth_t[l][b, a, 0, yc, xc] = r[4] + F(1)
                    if 0 <= int(r[4]) < num_classes:
                        cls_t[l][b, a, int(r[4]), yc, xc] = 1
    return dict(cls=cls_t, box=box_t, depth=depth_t, **facts)


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, dtype=F)


def compare(got, ref, want_cls=True, what=''):
    """`got` = the (cls_targets | Nones, box_targets, depths) lists of atss_assign_levels against atss_reference's dict."""
    cls_g, box_g, depth_g = got
    for l in range(len(ref['depth'])):
        tag = '%s level %d' % (what, l)
        assert np.array_equal(_np(depth_g[l]).view(np.uint32), ref['depth'][l].view(np.uint32)), tag + ': depth'
        if want_cls:
            assert np.array_equal(_np(cls_g[l]).view(np.uint32), ref['cls'][l].view(np.uint32)), tag + ': cls_target'
        else:
            assert cls_g[l] is None, tag
        box, rbox = _np(box_g[l]), ref['box'][l]
        assert box.shape == rbox.shape, tag
        assert np.array_equal(box.view(np.uint32) == 0, rbox.view(np.uint32) == 0), tag + ': zero pattern of box_target'
        assert np.array_equal(box[:, :, :2].view(np.uint32), rbox[:, :, :2].view(np.uint32)), tag + ': centre deltas'
        assert np.allclose(box[:, :, 2:], rbox[:, :, 2:], rtol=1e-6, atol=1e-6), tag + ': log deltas'


# ------------------------------------------------------------------------------------------- the window rule, on the host
WINDOW = 8                                           # kAtssWindow


def _centres(n, s):
    return np.arange(n).astype(F) * s + F(0.5) * s + F(0.5)


def distances(bcx, bcy, h, w, stride):
    """d2 [P, H * W] float32 of P box centres to every cell of the level, in the definition's operations."""
    s = F(stride)
    dx, dy = _centres(w, s)[None, :] - bcx[:, None], _centres(h, s)[None, :] - bcy[:, None]
    return ((dx * dx)[:, None, :] + (dy * dy)[:, :, None]).reshape(len(bcx), h * w)


def full_scan(bcx, bcy, h, w, stride):
    """-> (cells [P, H * W] nearest first, ties to the lower cell, NaN last; their d2)."""
    with np.errstate(all='ignore'):
        d2 = distances(bcx, bcy, h, w, stride)
    order = np.argsort(d2, axis=1, kind='stable')
    return order, np.take_along_axis(d2, order, 1)


def window_scan(bcx, bcy, h, w, stride):
    """The statistics kernel's window (csrc/atss.hpp: atss_window) for P box centres, restated in numpy float32:
    -> (cells [P, n] of the window nearest first, their d2, `sound` [P], `bound` [P]).  The kernel takes the first k' =
    min(k, H * W) of them iff sound, the window holds k' cells and d2 of the k'-th < bound; otherwise it scans the level in full."""
    s = F(stride)
    with np.errstate(all='ignore'):
        def start(centre, cells):
            span = min(cells, WINDOW)
            first = np.floor((centre - F(0.5)) / s - F(0.5)) - F(WINDOW // 2 - 1)
            last = F(cells - span)
            return np.where(~(first >= 0), 0, np.where(first > last, last, first)).astype(np.int64), span
        (c0, wc), (r0, hc) = start(bcx, w), start(bcy, h)
        c1, r1 = c0 + wc - 1, r0 + hc - 1
        px, py = _centres(w, s), _centres(h, s)
        sound = np.ones(len(bcx), bool)
        bound = np.full(len(bcx), np.inf, F)
        for centre, lo, hi, edge, n in ((bcx, c0, c1, px, w), (bcy, r0, r1, py, h)):
            before, after = edge[np.maximum(lo - 1, 0)], edge[np.minimum(hi + 1, n - 1)]
            sound &= (lo == 0) | (centre >= before)
            sound &= (hi == n - 1) | (centre <= after)
            d = before - centre
            bound = np.where(lo > 0, np.fmin(bound, d * d), bound)
            d = after - centre
            bound = np.where(hi < n - 1, np.fmin(bound, d * d), bound)
        d2 = distances(bcx, bcy, h, w, stride)
    rows = r0[:, None, None] + np.arange(hc)[None, :, None]
    cols = c0[:, None, None] + np.arange(wc)[None, None, :]
    cells = (rows * w + cols).reshape(len(bcx), hc * wc)               # ascending cell index
    inside = np.take_along_axis(d2, cells, 1)
    order = np.argsort(inside, axis=1, kind='stable')
    return np.take_along_axis(cells, order, 1), np.take_along_axis(inside, order, 1), sound, bound.astype(F)


# ---------------------------------------------------------------------------------------------------------------- cases
DEFAULT_LEVELS = [(32, 40, 8), (16, 20, 16), (8, 10, 32), (4, 5, 64), (2, 3, 128)]      # a 256 x 320 padded image
SIX_LEVELS = [(24, 28, 4), (12, 14, 8), (6, 7, 16), (3, 4, 32), (2, 2, 64), (1, 1, 128)]


def random_targets(seed, batch, n_max, extent=(320, 256), fill=0.8, classes=5, interleave=True):
    """[B, n_max, 5]: boxes of mixed sizes inside `extent` = (width, height), class -1 rows in between."""
    rng = np.random.RandomState(seed)
    t = np.full((batch, n_max, 5), -1, F)
    for b in range(batch):
        for i in range(n_max):
            if interleave and rng.rand() > fill:
                continue
            w = float(np.exp(rng.uniform(np.log(6), np.log(extent[0] * 0.9))))
            h = float(np.clip(w * np.exp(rng.uniform(-0.7, 0.7)), 4, extent[1] * 0.95))
            x, y = rng.uniform(0, max(extent[0] - w, 1)), rng.uniform(0, max(extent[1] - h, 1))
            t[b, i] = [x, y, w, h, rng.randint(classes)]
    return t


def _rows(*rows, n_max=None, batch=1):
    t = np.full((batch, n_max or len(rows), 5), -1, F)
    for i, r in enumerate(rows):
        t[0, i] = r
    return t


def _anchors(levels, ratios=RATIOS, scales=SCALES):
    return [base_anchors(s, ratios, scales) for _, _, s in levels]


def _case(targets, levels=DEFAULT_LEVELS, topk=9, classes=5, anchors=None, want_cls=True, random=False):
    return dict(targets=np.asarray(targets, F), levels=levels, anchors=anchors or _anchors(levels), classes=classes, topk=topk,
                want_cls=want_cls, random=random)


def _empty_next_to_full():
    t = random_targets(21, 2, 12, interleave=False)
    t[0, :, 4] = -1
    return t


CASES = {
    # the default pyramid, batch 3, every k
    'default_k1': lambda: _case(random_targets(11, 3, 14), topk=1, random=True),
    'default_k9': lambda: _case(random_targets(12, 3, 14), topk=9, random=True),
    'default_k16': lambda: _case(random_targets(13, 3, 14), topk=16, random=True),
    'default_no_cls': lambda: _case(random_targets(14, 3, 10), want_cls=False, random=True),
    'crowd': lambda: _case(random_targets(15, 2, 40, interleave=False), classes=80, random=True),
    'single_level': lambda: _case(random_targets(16, 2, 6, extent=(160, 112)), levels=[(14, 20, 8)]),
    'six_levels': lambda: _case(random_targets(17, 2, 8, extent=(112, 96)), levels=SIX_LEVELS, random=True),
    # levels with fewer cells than k (2 x 3, 2 x 2) and a 1 x 1 level
    'few_cells': lambda: _case(random_targets(18, 2, 5, extent=(128, 128)), levels=[(2, 3, 64), (2, 2, 64), (1, 1, 128)], topk=9),
    'one_anchor': lambda: _case(random_targets(19, 2, 8), anchors=_anchors(DEFAULT_LEVELS, [1.0], [4.0])),
    'max_anchors': lambda: _case(random_targets(20, 1, 6), levels=DEFAULT_LEVELS[1:],
                                 anchors=_anchors(DEFAULT_LEVELS[1:], [1.0, 2.0, 0.5, 3.0], [2 * 2 ** (i / 8) for i in range(8)])),
    'n_max_0': lambda: _case(np.zeros((2, 0, 5), F)),
    'all_padding': lambda: _case(np.full((2, 7, 5), -1, F)),
    'interleaved_padding': lambda: _case(random_targets(22, 3, 30, fill=0.4)),
    'round_minus_1': lambda: _case(random_targets(23, 1, ROUND - 1, fill=0.9), levels=DEFAULT_LEVELS[1:], classes=80),
    'round_exact': lambda: _case(random_targets(24, 1, ROUND, interleave=False), levels=DEFAULT_LEVELS[1:], classes=80),
    'round_plus_1': lambda: _case(random_targets(25, 1, ROUND + 1, fill=0.9), levels=DEFAULT_LEVELS[1:], classes=80),
    'three_rounds': lambda: _case(random_targets(26, 2, 2 * ROUND + 9, fill=0.7), levels=DEFAULT_LEVELS[1:], classes=80),
    'empty_next_to_full': lambda: _case(_empty_next_to_full()),
    'corners': lambda: _case(_rows([0, 0, 40, 30, 0], [280, 0, 40, 30, 1], [0, 226, 40, 30, 2], [280, 226, 40, 30, 3],
                                   [0, 0, 9, 9, 4], [311, 247, 9, 9, 0])),
    'centre_outside': lambda: _case(_rows([-90, 40, 60, 50, 0], [330, 100, 80, 60, 1], [100, -120, 70, 90, 2],
                                          [150, 300, 40, 200, 3], [-400, -300, 500, 400, 4], [2000, 1500, 64, 64, 0])),
    'three_pixels': lambda: _case(_rows([100, 100, 3, 3, 1], [19, 19, 3, 3, 2], [60, 70, 90, 80, 0])),
    'whole_image': lambda: _case(_rows([0, 0, 320, 256, 2], [96, 64, 128, 128, 1])),
    'identical_boxes': lambda: _case(_rows([64, 48, 120, 100, 1], [64, 48, 120, 100, 3], [10, 10, 50, 60, 0])),
    'shifted_by_one': lambda: _case(_rows([64, 48, 120, 100, 1], [65, 48, 120, 100, 3], [64, 49, 120, 100, 2])),
    'zero_width': lambda: _case(_rows([100, 80, 0, 60, 1], [40, 40, 80, 0, 2], [150, 100, 70, 70, 0])),
    'nan_coordinate': lambda: _case(_rows([float('nan'), 80, 50, 60, 1], [40, 40, 80, float('nan'), 2], [150, 100, 70, 70, 0],
                                          [30, float('nan'), 64, 64, 3])),
    'near_1e4': lambda: _case(_rows([9990.3, 10010.7, 61.5, 47.25, 1], [9700.2, 9895.1, 200.4, 180.9, 0], [9984, 9984, 333, 310, 1],
                                    [10050.5, 9999.5, 120, 130, 0]), levels=[(158, 159, 64), (79, 80, 128)], classes=2),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (the case, the checker's outputs for it); built once per process and left unchanged."""
    c = CASES[name]()
    return c, atss_reference(c['targets'], c['levels'], c['anchors'], c['classes'], c['topk'])
