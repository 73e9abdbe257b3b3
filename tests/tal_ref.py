"""The checker of task-aligned target assignment (odtk.box.tal_assign_levels, csrc/tal.hpp): the definition restated in numpy, on
its own -- nothing of odtk/box.py is used -- plus the cases and the comparison rule that tests/test_tal.py (CPU tensors) and
tests/test_gpu_tal.py (the kernels) share.

There is no reference implementation to compare with, so the definition is the contract (csrc/tal.hpp has it in full): every
float32 step below is ONE numpy float32 operation in the written order; exp_cr is the float64 exponential rounded once.

  1. a row is valid when its class is a whole number in 0..C-1; its box is x1 = x, x2 = x + w - 1
  2. its candidates: every anchor whose cell centre xc * stride + 0.5 * stride + 0.5 lies more than 0.01 inside the box (NaN: no)
  3. s = 1 / (1 + exp_cr(-logit)) of channel a * C + class
  4. the predicted box: delta2box without the clamp to the image
  5. u = IoU(predicted box, box), +1 pixel convention, minimum / maximum propagate NaN
  6. m = 1; alpha times m = m * s; beta times m = m * u.  NaN is never chosen, 0 is eligible (and -0 counts as 0)
  7. the row selects its min(topk, non-NaN candidates) largest m over all levels, ties to the lower global anchor index
  8. an anchor selected by several rows goes to the largest u, ties to the earliest row
  9. depth = class + 1 / 0, box_target = box2delta / 0, cls_target = one-hot / 0

Comparison rule (`compare`, that of atss_ref.compare): depth, cls_target and the zero pattern of box_target exactly; the centre
deltas (columns 0, 1) bit for bit; the log deltas (columns 2, 3) within rtol = atol = 1e-6 (the three logs -- numpy, torch, the
device -- may differ in the last place)."""
import functools
import math

import numpy as np

F = np.float32
RATIOS = [1.0, 2.0, 0.5]
SCALES = [4 * 2 ** (i / 3) for i in range(3)]
MAX_TOPK = 16                                        # ODTK_ATSS_MAX_TOPK
STAGE, THREADS, ROUND = 4096, 512, 128               # kTalStage, kTalThreads, kTalRound (csrc/tal.hpp)


def base_anchors(stride, ratios=RATIOS, scales=SCALES):
    """[A, 4] float32 base anchors around one stride x stride cell, scale-major."""
    out = []
    for sc in scales:
        for r in ratios:
            side = math.sqrt(stride * stride / r)
            w, h = side * sc, side * r * sc
            out.append([0.5 * (stride - w), 0.5 * (stride - h), 0.5 * (stride + w), 0.5 * (stride + h)])
    return np.asarray(out, dtype=F)


def exp_cr(x):
    return np.exp(x.astype(np.float64)).astype(F)


def _iou(a1x, a1y, a2x, a2y, x1, y1, x2, y2, area):
    a_area = (a2x - a1x + F(1)) * (a2y - a1y + F(1))
    w = np.minimum(a2x, x2) - np.maximum(a1x, x1) + F(1)
    h = np.minimum(a2y, y2) - np.maximum(a1y, y1) + F(1)
    w = np.where(w < 0, F(0), w)
    h = np.where(h < 0, F(0), h)
    inter = w * h
    return inter / (a_area + area - inter)


def valid_class(c, num_classes):
    return bool(c >= 0 and c < num_classes and c == np.floor(c))


def tal_reference(targets, levels, anchors, cls_heads, box_heads, num_classes, topk, alpha, beta):
    """targets [B, n_max, 5] float32; levels [(H, W, stride)]; anchors per level [A, 4]; cls_heads / box_heads per level float32
    [B, A * C, H, W] / [B, A * 4, H, W] (the widened values of the heads).
    -> dict(cls, box, depth: per level [B, A, C | 4 | 1, H, W] float32; and the facts the tests assert on: `assigned` anchors,
    anchors `contested` by two or more rows, rows with `ties_at_the_kth` (the last selected and the first unselected candidate have
    the same metric), `boxes_without_positives`, `rows_with_fewer_than_k` (at least one, fewer than topk eligible candidates),
    `nan_candidates`, `zero_metric_selected` entries, `assigned_per_level`, valid `boxes`, `max_candidates` of a row; per valid row
    in order (image, row, candidate g ascending, selected g best first, number of non-NaN candidates) in `rows`)."""
    targets = np.asarray(targets, dtype=F)
    batch = targets.shape[0]
    a_count = anchors[0].shape[0]
    cls_t = [np.zeros((batch, a_count, num_classes, h, w), F) for h, w, _ in levels]
    box_t = [np.zeros((batch, a_count, 4, h, w), F) for h, w, _ in levels]
    depth_t = [np.zeros((batch, a_count, 1, h, w), F) for h, w, _ in levels]
    level_base = np.cumsum([0] + [a_count * h * w for h, w, _ in levels])
    facts = dict(assigned=0, contested=0, ties_at_the_kth=0, boxes_without_positives=0, rows_with_fewer_than_k=0, nan_candidates=0,
                 zero_metric_selected=0, boxes=0, max_candidates=0, assigned_per_level=[0] * len(levels), rows=[])
    with np.errstate(all='ignore'):
        for b in range(batch):
            total = int(level_base[-1])
            owner = np.full(total, -1, np.int64)
            best = np.zeros(total, F)
            claims = np.zeros(total, np.int64)
            for i, r in enumerate(targets[b]):
                if not valid_class(r[4], num_classes):
                    continue
                facts['boxes'] += 1
                k = int(r[4])
                x1, y1 = r[0], r[1]
                x2, y2 = r[0] + r[2] - F(1), r[1] + r[3] - F(1)
                area = (x2 - x1 + F(1)) * (y2 - y1 + F(1))
                gs, ms, us = [], [], []
                for l, ((h, w, s), anc) in enumerate(zip(levels, anchors)):
                    s = F(s)
                    px = np.arange(w).astype(F) * s + F(0.5) * s + F(0.5)
                    py = np.arange(h).astype(F) * s + F(0.5) * s + F(0.5)
                    inside = ((px - x1 > F(0.01)) & (x2 - px > F(0.01)))[None, :] & ((py - y1 > F(0.01)) & (y2 - py > F(0.01)))[:, None]
                    a, yc, xc = np.nonzero(np.broadcast_to(inside[None], (a_count, h, w)))      # (a, y, x) ascending = g ascending
                    if not len(a):
                        continue
                    logit = cls_heads[l][b].reshape(a_count, num_classes, h, w)[a, k, yc, xc].astype(F)
                    d = box_heads[l][b].reshape(a_count, 4, h, w)[a, :, yc, xc].astype(F)         # [n, 4]
                    score = F(1) / (F(1) + exp_cr(-logit))
                    fx, fy = xc.astype(F) * s, yc.astype(F) * s
                    ax1, ay1, ax2, ay2 = fx + anc[a, 0], fy + anc[a, 1], fx + anc[a, 2], fy + anc[a, 3]
                    aw, ah = ax2 - ax1 + F(1), ay2 - ay1 + F(1)
                    cx, cy = ax1 + F(0.5) * aw, ay1 + F(0.5) * ah
                    pcx, pcy = d[:, 0] * aw + cx, d[:, 1] * ah + cy
                    pw, ph = exp_cr(d[:, 2]) * aw, exp_cr(d[:, 3]) * ah
                    u = _iou(pcx - F(0.5) * pw, pcy - F(0.5) * ph, pcx + F(0.5) * pw - F(1), pcy + F(0.5) * ph - F(1),
                             x1, y1, x2, y2, area).astype(F)
                    m = np.ones(len(a), F)
                    for _ in range(alpha):
                        m = m * score
                    for _ in range(beta):
                        m = m * u
                    gs.append(level_base[l] + (a * h + yc) * w + xc)
                    ms.append(m.astype(F))
                    us.append(u)
                g = np.concatenate(gs) if gs else np.zeros(0, np.int64)
                m = np.concatenate(ms) if ms else np.zeros(0, F)
                u = np.concatenate(us) if us else np.zeros(0, F)
                facts['max_candidates'] = max(facts['max_candidates'], len(g))
                nan = np.isnan(m)
                facts['nan_candidates'] += int(nan.sum())
                ge, me, ue = g[~nan], m[~nan] + F(0), u[~nan]
                order = np.lexsort((ge, -me))                                                    # m descending, then g ascending
                take = order[:min(topk, len(order))]
                facts['boxes_without_positives'] += len(take) == 0
                facts['rows_with_fewer_than_k'] += 0 < len(order) < topk
                facts['zero_metric_selected'] += int((me[take] == 0).sum())
                if len(order) > len(take) and me[order[len(take) - 1]] == me[order[len(take)]]:
                    facts['ties_at_the_kth'] += 1
                facts['rows'].append((b, i, g, ge[take], len(ge)))
                for j in take:
                    claims[ge[j]] += 1
                    if owner[ge[j]] < 0 or ue[j] > best[ge[j]]:
                        owner[ge[j]], best[ge[j]] = i, ue[j]
            facts['contested'] += int((claims >= 2).sum())
            for l, ((h, w, s), anc) in enumerate(zip(levels, anchors)):
                s = F(s)
                mine = owner[level_base[l]:level_base[l + 1]]
                hits = np.nonzero(mine >= 0)[0]
                facts['assigned'] += len(hits)
                facts['assigned_per_level'][l] += len(hits)
                for local in hits:
                    r = targets[b][mine[local]]
                    a, cell = local // (h * w), local % (h * w)
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
                    cls_t[l][b, a, int(r[4]), yc, xc] = 1
    return dict(cls=cls_t, box=box_t, depth=depth_t, **facts)


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, dtype=F)


def compare(got, ref, want_cls=True, what=''):
    """`got` = the (cls_targets | Nones, box_targets, depths) lists of tal_assign_levels against tal_reference's dict."""
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


# ---------------------------------------------------------------------------------------------------------------- cases
LEVELS = [(8, 12, 8), (4, 6, 16), (2, 3, 32)]        # a 64 x 96 image
STREAM_LEVELS = [(40, 40, 2)] + LEVELS               # one extra level of 40 x 40 cells: 14 400 anchors with A = 9
CLASSES, BATCH = 3, 2


def _anchors(levels, one=False):
    return [base_anchors(s, [1.0], [4.0]) if one else base_anchors(s) for _, _, s in levels]


def random_heads(seed, levels, a, classes=CLASSES, batch=BATCH):
    """Logits ~ N(0, 2), deltas ~ N(0, 0.3), per level float32 [B, A * C | A * 4, H, W]."""
    rng = np.random.RandomState(seed)
    return ([(rng.randn(batch, a * classes, h, w) * 2).astype(F) for h, w, _ in levels],
            [(rng.randn(batch, a * 4, h, w) * 0.3).astype(F) for h, w, _ in levels])


def random_targets(seed, n_max, batch=BATCH, extent=(96, 64), classes=CLASSES, low=8.0, high=None):
    rng = np.random.RandomState(seed)
    t = np.zeros((batch, n_max, 5), F)
    for b in range(batch):
        for i in range(n_max):
            w = float(np.exp(rng.uniform(np.log(low), np.log(high or extent[0] * 0.9))))
            h = float(np.clip(w * np.exp(rng.uniform(-0.6, 0.6)), 4, extent[1] * 0.95))
            t[b, i] = [rng.uniform(0, max(extent[0] - w, 1)), rng.uniform(0, max(extent[1] - h, 1)), w, h, rng.randint(classes)]
    return t


def _rows(*images, n_max=None):
    n = n_max or max(len(rows) for rows in images)
    t = np.full((len(images), n, 5), -1, F)
    for b, rows in enumerate(images):
        for i, r in enumerate(rows):
            t[b, i] = r
    return t


def _case(targets, heads=None, levels=LEVELS, one=False, topk=13, alpha=1, beta=6, want_cls=True, seed=1, classes=CLASSES):
    targets = np.asarray(targets, F)
    anchors = _anchors(levels, one)
    cls_heads, box_heads = heads or random_heads(seed, levels, anchors[0].shape[0], classes, targets.shape[0])
    return dict(targets=targets, levels=levels, anchors=anchors, cls=cls_heads, box=box_heads, classes=classes, topk=topk, alpha=alpha,
                beta=beta, want_cls=want_cls)


def _constant_heads(levels, a, logit, deltas, batch=BATCH, classes=CLASSES):
    cls_heads = [np.full((batch, a * classes, h, w), logit, F) for h, w, _ in levels]
    box_heads = [np.tile(np.asarray(deltas, F).reshape(1, 1, 4, 1, 1), (batch, a, 1, h, w)).reshape(batch, a * 4, h, w) for h, w, _ in levels]
    return cls_heads, box_heads


def _off_target_heads(levels, a):
    """Random logits; deltas that move every predicted box far off any ground truth: u = 0 everywhere."""
    cls_heads, box_heads = random_heads(31, levels, a)
    for x in box_heads:
        x.reshape(x.shape[0], a, 4, *x.shape[2:])[:, :, 0] = 50
    return cls_heads, box_heads


def _non_finite_heads(levels, a):
    cls_heads, box_heads = random_heads(32, levels, a)
    rng = np.random.RandomState(33)
    for x in cls_heads + box_heads:
        flat = x.reshape(-1)
        where = rng.choice(flat.size, max(flat.size // 8, 3), replace=False)
        flat[where] = rng.choice(np.asarray([np.nan, np.inf, -np.inf], F), len(where))
    return cls_heads, box_heads


def _many_rows():
    t = random_targets(41, 130, low=9.0, high=22.0)
    assert t.shape[1] > ROUND
    return t


BOX = [20, 10, 50, 40]
CASES = {
    # random boxes with random heads
    'random_a9': lambda: _case(random_targets(11, 6), seed=2),
    'random_a1': lambda: _case(random_targets(12, 6), one=True, seed=3),
    'random_no_cls': lambda: _case(random_targets(13, 5), want_cls=False, seed=4),
    # a box over the whole image and one extra level of 40 x 40 cells: more candidates than several staging rounds hold
    'whole_image_stream': lambda: _case(_rows([[0, 0, 96, 96, 1], [30, 20, 40, 30, 2]], [[0, 0, 96, 96, 0]]), levels=STREAM_LEVELS, seed=5),
    # a box with no cell centre inside, next to boxes that have some
    'no_centre': lambda: _case(_rows([[1, 1, 3, 3, 0], BOX + [1]], [[40, 20, 30, 30, 2]]), seed=6),
    # fewer candidates than topk: 9 + 1 + 1 anchors with A = 1
    'fewer_than_k': lambda: _case(_rows([[10, 10, 20, 20, 1]], [[50, 30, 20, 20, 0]]), one=True, topk=16, seed=7),
    # ties: all logits equal, all deltas zero (the predicted box is the anchor; every anchor that lies inside the box has the same u)
    'ties': lambda: _case(_rows([[8, 4, 80, 56, 1], [17, 16, 64, 32, 2]], [[0, 0, 96, 64, 0]]), one=True,
                          heads=_constant_heads(LEVELS, 1, 0.3, [0, 0, 0, 0])),
    'ties_a9': lambda: _case(_rows([[8, 4, 80, 56, 1], [17, 16, 64, 32, 2]], [[0, 0, 96, 64, 0]]),
                             heads=_constant_heads(LEVELS, 9, -1.0, [0, 0, 0, 0])),
    # u = 0 everywhere: the topk lowest indices are taken
    'zero_metric': lambda: _case(_rows([BOX + [1], [40, 8, 50, 50, 0]], [[10, 10, 70, 40, 2]]), heads=_off_target_heads(LEVELS, 9)),
    # two overlapping boxes of different classes, and two identical rows
    'contested': lambda: _case(_rows([BOX + [1], BOX + [2], [30, 16, 50, 40, 0]], [[10, 10, 60, 40, 2], [20, 14, 60, 40, 1]]), seed=8),
    # NaN and +-inf logits and deltas at an eighth of the positions
    'non_finite': lambda: _case(random_targets(14, 5), heads=_non_finite_heads(LEVELS, 9)),
    # padding rows between valid ones, a row with class == C, a class that is no whole number; no rows; only padding
    'padding': lambda: _case(_rows([[-1, -1, -1, -1, -1], BOX + [1], [30, 10, 40, 40, CLASSES], [5, 5, 60, 50, 1.5], [40, 20, 40, 30, 0]],
                                   [[10, 10, 40, 40, 2], [-1, -1, -1, -1, -1], [0, 0, 0, 0, -1], [50, 8, 40, 50, 1]]), seed=9),
    'n_max_0': lambda: _case(np.zeros((BATCH, 0, 5), F)),
    'all_padding': lambda: _case(np.full((BATCH, 7, 5), -1, F)),
    # more rows than the scatter stages in one round
    'many_rows': lambda: _case(_many_rows(), seed=10),
    # exponents and topk
    'alpha_0': lambda: _case(random_targets(15, 5), alpha=0, seed=11),
    'beta_1': lambda: _case(random_targets(16, 5), beta=1, seed=12),
    'alpha_4_beta_8': lambda: _case(random_targets(17, 5), alpha=4, beta=8, seed=13),
    'topk_1': lambda: _case(random_targets(18, 5), topk=1, seed=14),
    'topk_16': lambda: _case(random_targets(19, 5), topk=16, seed=15),
}
DTYPES = ('float32', 'bfloat16', 'float16')


def heads_in(c, dtype):
    """The case's heads as torch tensors GENERATED in `dtype` (float32 values rounded to it once), per level -> (cls, box)."""
    import torch
    kind = getattr(torch, dtype)
    return [torch.from_numpy(x).to(kind) for x in c['cls']], [torch.from_numpy(x).to(kind) for x in c['box']]


@functools.lru_cache(maxsize=None)
def case(name, dtype='float32'):
    """-> (the case, the checker's outputs for its heads in `dtype`, widened); built once per process and left unchanged."""
    c = CASES[name]()
    if dtype != 'float32':
        cls_heads, box_heads = heads_in(c, dtype)
        c = dict(c, cls=[x.float().numpy() for x in cls_heads], box=[x.float().numpy() for x in box_heads])
    return c, tal_reference(c['targets'], c['levels'], c['anchors'], c['cls'], c['box'], c['classes'], c['topk'], c['alpha'], c['beta'])
