"""Every staging round, decision edge and launch geometry of the target-assignment kernels (csrc/targets.hpp) against the CPU
oracle of the same operation on the same inputs.

snap_to_anchors_kernel / snap_to_anchors_levels_kernel are held to oracle/box_oracle.py:snap_to_anchors, the rotated kernel to
oracle/targets_oracle.py (all-pairs polygon IoU by oracle/c_oracle.py, which is pinned bit for bit to the reference's device code
and to the HIP `iou` op).  The rotated kernel is handed `rotate_boxes`' output computed on the CPU (the oracle's own restatement),
so both sides start from the same bits: cos / sin of the host and of the device may differ by an ulp, which is a property of
torch, not of the kernel under test (tests/test_targets.py runs the whole path on the device against the fixtures).

What is compared (`_compare`), for every image and level of every case, no cell excluded:
  depth, cls_target   bit for bit;
  box_target          NaN at the oracle's NaN positions, +-inf where the oracle has them, exactly 0 where the oracle is exactly 0;
                      the finite rest within rtol = atol = 1e-6 (axis-aligned) / 1e-5 (rotated, the four deltas) of the fp32 oracle,
                      sin and cos bit for bit;
                      and within 2 K of oracle/targets_oracle.py:delta_error_bound of the float64 deltas of the oracle's winner
                      (the kernel is the oracle's chain of fp32 operations with another log).
K = 3 is the smallest integer under which the fp32 oracle itself stays inside the bound on every case of this file
(test_cases_are_not_vacuous asserts that it does; the oracle's worst ratio at K = 1 is 2.15, on a log delta of axis_rows_2049:
the two widths carry two roundings each and the division a fifth; the centre deltas reach 1.76).

The cases are built by plain functions (CASES); test_cases_are_not_vacuous checks with the oracle alone, on the CPU, that they
contain what they are meant to contain (all three decisions, winners from every staging round, zero and non-zero overlaps on
both sides of the reject margin, a sub-pixel box beyond the margin that still overlaps, the intended threshold decisions).
Outputs are allocated over NaN-filled memory, so a cell the kernel does not write shows up."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import box_oracle, targets_oracle

RATIOS = [1.0, 2.0, 0.5]
SCALES = [4 * 2 ** (i / 3) for i in range(3)]
ANGLES = [-math.pi / 6, 0, math.pi / 6]
MAX_ANCHORS, MAX_LEVELS = 32, 6                     # ODTK_MAX_ANCHORS, ODTK_MAX_LEVELS (asserted against odtk._C on the GPU)
AXIS_ROUND, ROT_ROUND = 1024, 128                   # kSnapMaxBoxes, kSnapRotBoxes: rows staged in LDS at a time
K_ORACLE = 3
GEOMETRY = [(1, 1), (40, 25), (5, 7), (1, 300), (17, 16), (16, 16)]      # (H, W); hw <, ==, just past 256; not monotone
GEOMETRY_STRIDES = [64, 8, 32, 4, 16, 16]


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32, copy=False)).view(np.uint32)


class Case:
    """targets [B, n_max, 5 | 6] with class = -1 padding rows; levels [(H, W, stride)]; anchors per level: [A, 4], or the
    ([A, 4], [A, 8]) pair for rotated boxes."""

    def __init__(self, rotated, targets, levels, anchors, classes, ious=(0.4, 0.5), **notes):
        self.rotated, self.targets, self.levels, self.anchors = rotated, targets.float().contiguous(), levels, anchors
        self.classes, self.ious, self.notes = classes, [float(v) for v in ious], notes
        if rotated:                                   # what the kernel is handed: rotate_boxes of EVERY row, padding included
            b, n = self.targets.shape[:2]
            axis, quads = targets_oracle.rotate_boxes(self.targets.reshape(b * n, 6)[:, :5])
            self.gt_axis, self.gt_quads = axis.view(b, n, 6).contiguous(), quads.view(b, n, 8).contiguous()
            self.gt_class = self.targets[:, :, 5].contiguous()

    @functools.lru_cache(maxsize=None)
    def oracle(self):
        """[image][level] -> dict(cls, box, depth, winner, overlap, winbox [cells, 4 | 6], anchor [cells, 4]); `winner` indexes the
        image's VALID rows (rows with class > -1, in order)."""
        out = []
        for b in range(self.targets.shape[0]):
            valid = self.targets[b, :, -1] > -1
            per_level = []
            for (h, w, s), anchors in zip(self.levels, self.anchors):
                size = [w * s, h * s]
                if self.rotated:
                    axis = self.gt_axis[b][valid]
                    r = targets_oracle.snap_from_rotated(axis, self.gt_quads[b][valid], self.gt_class[b][valid][:, None], size, s,
                                                         anchors, self.classes, self.ious)
                    xyxy, anc = axis, box_oracle.cell_anchors(anchors[0], size, s)
                else:
                    rows = self.targets[b][valid]
                    r = box_oracle.snap_to_anchors(rows, size, s, anchors, self.classes, self.ious, return_winner=True)
                    xyxy, anc = torch.cat([rows[:, :2], rows[:, :2] + rows[:, 2:4] - 1], 1), box_oracle.cell_anchors(anchors, size, s)
                d = dict(zip(('cls', 'box', 'depth', 'winner', 'overlap'), r), anchor=anc)
                d['winbox'] = xyxy[d['winner'].view(-1)] if int(valid.sum()) else None
                per_level.append(d)
            out.append(per_level)
        return out

    def valid_index(self, b):
        """positions in the padded list of image b's valid rows: oracle winner -> row index."""
        return (self.targets[b, :, -1] > -1).nonzero().view(-1)


# ------------------------------------------------------------------------------------------------------------------------------
# anchors and random boxes
# ------------------------------------------------------------------------------------------------------------------------------
def _axis_anchors(stride, a):
    from odtk import box
    if a == 9:
        return box.generate_anchors(stride, RATIOS, SCALES)
    if a == 1:
        return box.generate_anchors(stride, RATIOS, SCALES)[4:5].contiguous()
    assert a == MAX_ANCHORS
    return box.generate_anchors(stride, [0.5, 1.0, 2.0, 3.0], [2 * 2 ** (i / 4) for i in range(8)])


def _rot_anchors(stride, a):
    from odtk import box
    axis, quads = box.generate_anchors_rotated(stride, RATIOS, SCALES, ANGLES)
    if a == 1:
        return axis[4:5].contiguous(), quads[4:5].contiguous()          # a -30 degree anchor
    assert a == 27
    return axis, quads


def _random_boxes(gen, n, wpx, hpx, classes, rotated, lo=10.0, hi=110.0):
    xy = torch.rand(n, 2, generator=gen) * torch.tensor([wpx * 1.0, hpx * 1.0]) - torch.tensor([wpx * 0.2, hpx * 0.2])
    wh = torch.rand(n, 2, generator=gen) * (hi - lo) + lo
    cols = [xy, wh]
    if rotated:
        cols.append((torch.rand(n, 1, generator=gen) - 0.5) * 2.4)
    cols.append(torch.randint(0, classes, (n, 1), generator=gen).float())
    return torch.cat(cols, 1)


def _anchor_box(level, anchors, row, y, x, cls, rotated):
    """A ground-truth row that coincides with anchor `row` of cell (y, x): IoU (nearly) 1, nothing random beats it."""
    h, w, s = level
    ax = (anchors[0] if rotated else anchors)[row]
    x1, y1 = float(ax[0]) + x * s, float(ax[1]) + y * s
    if rotated:                                        # quads span x .. x + w (rotate_boxes), the axis form x .. x + w - 1
        q = anchors[1][row].view(4, 2)
        assert float(q[0, 1]) == float(q[1, 1]), 'needs an anchor of angle 0'
        return torch.tensor([float(q[0, 0]) + x * s, float(q[0, 1]) + y * s, float(q[2, 0] - q[0, 0]), float(q[2, 1] - q[0, 1]), 0.0, cls])
    return torch.tensor([x1, y1, float(ax[2] - ax[0]) + 1, float(ax[3] - ax[1]) + 1, cls])


# ------------------------------------------------------------------------------------------------------------------------------
# staging rounds and compaction
# ------------------------------------------------------------------------------------------------------------------------------
AXIS_ROWS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049]
ROT_ROWS = [0, 1, 63, 64, 65, 127, 128, 129, 256, 257, 300]
SPECIAL_ROWS = (63, 64, 127, 128, 1023, 1024)


def _staging_case(rotated, n, seed):
    """Four images over the same n rows: all valid (its last row coincides with an anchor: the last round can win) | valid rows only
    in the last round (every earlier round compacts to 0 rows) | padding interleaved: every third row and rows 63, 64, 127, 128,
    1023, 1024 valid, the padding rows keep their coordinates | all padding."""
    gen = torch.Generator().manual_seed(seed)
    rnd = ROT_ROUND if rotated else AXIS_ROUND
    classes = 6
    level = (4, 6, 16) if rotated else (5, 7, 16)
    anchors = _rot_anchors(16, 27) if rotated else _axis_anchors(16, 9)
    h, w, s = level
    rows = _random_boxes(gen, n, w * s, h * s, classes, rotated, 8.0, 64.0)
    if n > 1:
        cell = n % (h * w)
        rows[n - 1] = _anchor_box(level, anchors, 13 if rotated else 4, cell // w, cell % w, classes - 1, rotated)
    width = rows.shape[1]
    targets = rows[None].repeat(4, 1, 1)
    first = ((n - 1) // rnd) * rnd if n else 0
    keep = torch.zeros(n, dtype=torch.bool)
    keep[first if first else max(n - 3, 0):] = True
    targets[1][~keep] = -1.0
    keep = torch.arange(n) % 3 == 1
    for i in SPECIAL_ROWS:
        if i < n:
            keep[i] = True
    targets[2][~keep, width - 1] = -1.0
    targets[3] = -1.0
    return Case(rotated, targets, [level], [anchors], classes, rounds=rnd, planted_last=n > 1)


def _duplicate_case(rotated, seed):
    """An exact duplicate of a winning box in each later round, with another class: the FIRST must win.  A better box (one that
    coincides with an anchor) as the last row of the last round: the last round must be able to win."""
    gen = torch.Generator().manual_seed(seed)
    rnd = ROT_ROUND if rotated else AXIS_ROUND
    classes, n = 7, 2 * rnd + 40
    level = (4, 6, 16) if rotated else (5, 7, 16)
    anchors = _rot_anchors(16, 27) if rotated else _axis_anchors(16, 9)
    h, w, s = level
    rows = _random_boxes(gen, n, w * s, h * s, classes, rotated, 8.0, 64.0)
    src = 5
    rows[src] = _anchor_box(level, anchors, 13 if rotated else 4, 1, 2, 2, rotated)     # wins its cell for certain
    for r, at in enumerate((rnd + 17, 2 * rnd + 3)):
        rows[at] = rows[src]
        rows[at, -1] = 3 + r
    rows[n - 1] = _anchor_box(level, anchors, 13 if rotated else 4, 3, 4, 6, rotated)
    targets = rows[None].repeat(2, 1, 1)
    targets[1, :rnd] = -1.0                             # image 1: the first copy is gone, the copy of round 1 is now the first
    return Case(rotated, targets, [level], [anchors], classes, rounds=rnd, duplicate=(src, rnd + 17, 2 * rnd + 3), cell=(1, 2),
                row=13 if rotated else 4, last_cell=(3, 4))


# ------------------------------------------------------------------------------------------------------------------------------
# decision edges (hand-built anchors)
# ------------------------------------------------------------------------------------------------------------------------------
UNIT_ANCHOR = torch.tensor([[0.0, 0.0, 9.0, 9.0]])          # area 100 under the +1 convention


def _threshold_case(ious):
    """Level 2 x 3, stride 16, one anchor (0, 0, 9, 9) per cell.  A box (x, y, 10, k) on a cell has IoU 10 k / 100 with it: k = 5 is
    exactly 0.5, k = 4 exactly float32(0.4), k = 3 0.3.  One box per cell, classes 0 and C - 1 among them."""
    c = 5
    rows = [[0, 0, 10, 5, c - 1], [16, 0, 10, 4, 0], [32, 0, 10, 3, 2], [0, 16, 10, 4, c - 1], [16, 16, 10, 5, 0], [32, 16, 10, 10, 1]]
    return Case(False, torch.tensor(rows, dtype=torch.float32)[None], [(2, 3, 16)], [UNIT_ANCHOR], c, ious,
                overlaps=[0.5, 0.4, 0.3, 0.4, 0.5, 1.0])


def _tie_case():
    """Different boxes with exactly the same IoU on a cell (mirror images about the anchor): the first in the list wins; image 1 has
    them in the other order.  The deltas of the two differ by 0.4: far above any bar."""
    a = [-2.0, 0, 10, 10, 1]
    b = [2.0, 0, 10, 10, 3]
    c = [16.0, 14.0, 10, 10, 0]
    d = [16.0, 18.0, 10, 10, 4]
    t = torch.tensor([[a, b, c, d, [-1.0] * 5], [d, [-1.0] * 5, c, b, a]], dtype=torch.float32)
    return Case(False, t, [(2, 3, 16)], [UNIT_ANCHOR], 5, (0.4, 0.5), ties=True)


def _far_rows(rotated, n, classes):
    rows = []
    for i in range(n):
        r = [5000.0 + 97 * i, 7000.0 - 41 * i, 20.0 + i, 30.0 + 2 * i]
        rows.append(r + ([0.3 * i - 0.5] if rotated else []) + [float((i * 3 + 1) % classes)])
    return torch.tensor(rows, dtype=torch.float32)


def _all_zero_case(rotated):
    """Every box far from every anchor: all background, cls_target all zero, box_target = the deltas towards the FIRST valid row at
    every cell (image 1: row 0 is padding).  The centre deltas towards any other row differ by more than 0.1."""
    rows = _far_rows(rotated, 150 if rotated else 1100, 4)
    t = rows[None].repeat(2, 1, 1)
    t[1, 0] = -1.0
    anchors = _rot_anchors(16, 27) if rotated else _axis_anchors(16, 9)
    return Case(rotated, t, [(5, 7, 16)], [anchors], 4, all_zero=True)


def _nan_case(rotated):
    """Image 0: a row with a NaN coordinate in the middle of the list.  Image 1: a row with a NaN coordinate AFTER a box that coincides
    with an anchor.  Image 2: NaN in the width; image 3: +inf coordinates."""
    gen = torch.Generator().manual_seed(31)
    level = (3, 4, 16)
    anchors = _rot_anchors(16, 27) if rotated else _axis_anchors(16, 9)
    rows = _random_boxes(gen, 5, 64, 48, 5, rotated, 16.0, 90.0)
    t = rows[None].repeat(4, 1, 1)
    t[0, 2, 0] = float('nan')
    t[1, 0] = _anchor_box(level, anchors, 13 if rotated else 4, 1, 1, 4, rotated)
    t[1, 3, 1] = float('nan')
    t[2, 4, 2] = float('nan')
    t[3, 1, 0] = float('inf')
    t[3, 2, 3] = float('inf')
    return Case(rotated, t, [level], [anchors], 5, nan=True)


def _degenerate_case(rotated):
    """Axis-aligned: zero and negative widths / heights among ordinary boxes.  Rotated: widths of 0.5 px, 2^-10 px and 0 px ON the
    anchors (the flag "an edge shorter than one pixel" sends every pair with them through the full clip)."""
    gen = torch.Generator().manual_seed(32)
    level = (3, 4, 16)
    rows = _random_boxes(gen, 8, 64, 48, 5, rotated, 16.0, 90.0)
    if rotated:
        rows[1, 2], rows[3, 2], rows[5, 3], rows[6, 2] = 0.5, 0.0, 0.5, 2.0 ** -10
        rows[6, 4] = 0.0
        t = rows[None].repeat(2, 1, 1)
        t[1, :, 2:4] = torch.tensor([[0.5, 40.0], [0.0, 40.0], [40.0, 0.5], [0.0, 0.0], [0.5, 0.5], [40.0, 0.0], [2.0 ** -10, 30.0], [0.25, 60.0]])
        return Case(True, t, [level], [_rot_anchors(16, 27)], 5, degenerate=True)
    rows[1, 2], rows[2, 3], rows[4, 2], rows[5, 3] = 0.0, 0.0, -6.0, -1.0
    t = rows[None].repeat(2, 1, 1)
    t[1, :, 2:4] = torch.tensor([[0.0, 30.0], [30.0, 0.0], [0.0, 0.0], [-4.0, 30.0], [30.0, -4.0], [-4.0, -4.0], [1.0, 1.0], [-1.0, 50.0]])
    return Case(False, t, [level], [_axis_anchors(16, 9)], 5, degenerate=True)


# ------------------------------------------------------------------------------------------------------------------------------
# rotated distance reject
# ------------------------------------------------------------------------------------------------------------------------------
def reject_margin(reach):
    return 2.0 + 1e-3 * reach + 4e-6 * reach * reach


def _bbox(q):
    q = np.asarray(q, np.float64).reshape(4, 2)
    return q[:, 0].min(), q[:, 1].min(), q[:, 0].max(), q[:, 1].max()


def gap_and_margin(anchor_quad, box_quad):
    """The kernel's `gap` and reject margin of a pair, in float64 from the fp32 quads."""
    a, b = _bbox(anchor_quad), _bbox(box_quad)
    gap = max(a[0] - b[2], b[0] - a[2], a[1] - b[3], b[1] - a[3])
    reach = max(abs(v) for v in a) + max(abs(v) for v in b)
    return gap, reject_margin(reach)


def _edges_at_least_one_pixel(quad):
    """the kernel's condition for skipping the clip on distance, in its own fp32 arithmetic"""
    q = quad.view(4, 2)
    e = q.roll(-1, 0) - q
    return bool(((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]).min() >= 1.0))


def _reject_case(off):
    """Anchor 0 of cell (0, 0) is the square off .. off + 31 (anchor 1: the same square turned by 30 degrees, 200 px further).  Every
    image holds a decoy far beyond the margin (overlap exactly 0) in front of ONE probe box, so a probe with any overlap at all wins
    the cell; iou_bg is 1e-7, so it also flips the cell from background to ignored.  Probes: 40 x 24 boxes, unrotated and turned by
    0.5 rad, at bounding-box gaps of -3 .. 8 px on all four sides and at gaps just below and just above the margin (at 1e5 px
    only left of and above the square, towards the origin: a probe to the right or below takes `reach` with it and its gap never
    exceeds the margin there); from 1e4 px on small and thin boxes a few pixels away, to which the clip's fp32 rounding gives a real,
    non-zero overlap although the bounding boxes do not touch; and at 1e3 px two boxes 2^-10 px wide beyond the margin that the
    clip still gives an overlap."""
    off = float(off)
    sq = torch.tensor([[off, off, off + 31, off, off + 31, off + 31, off, off + 31]])
    c, s = math.cos(math.pi / 6), math.sin(math.pi / 6)
    ctr = off + 215.5
    turned = [(ctr + c * dx + s * dy, ctr - s * dx + c * dy) for dx, dy in ((-15.5, -15.5), (15.5, -15.5), (15.5, 15.5), (-15.5, 15.5))]
    order = sorted(turned)                                               # tl, tr, br, bl as rotate_boxes orders them
    tl, bl = sorted(order[:2], key=lambda p: p[1])
    tr, br = sorted(order[2:], key=lambda p: p[1])
    quads = torch.cat([sq, torch.tensor([[v for p in (tl, tr, br, bl) for v in p]], dtype=torch.float32)])
    axis = torch.tensor([[off, off, off + 31, off + 31], [off + 200, off + 200, off + 231, off + 231]])

    def probe(side, g, theta=0.0, w=40.0, h=24.0):
        """a w x h box (its quad spans w x h) on one side of the square -- right, left, below, above -- whose BOUNDING box is g away"""
        bw, bh = w * math.cos(theta) + h * abs(math.sin(theta)), w * abs(math.sin(theta)) + h * math.cos(theta)
        ex, ey = (bw - w) / 2, (bh - h) / 2
        x, y = {0: (off + 31 + g + ex, off + 3.0), 1: (off - g - w - ex, off + 5.0), 2: (off + 2.0, off + 31 + g + ey),
                3: (off - 4.0, off - g - h - ey)}[side]
        return [x, y, w, h, theta, float(side)]

    def at_margin(side):
        """the gap at which gap == margin on this side (the margin grows with the gap: reach contains the box), by bisection"""

        def excess(g):
            quad = targets_oracle.rotate_boxes(torch.tensor([probe(side, g)[:5]]))[1][0].numpy()
            gap, margin = gap_and_margin(sq[0].numpy(), quad)
            return gap - margin
        # a probe AWAY from the origin (right, below) takes reach with it: beyond ~6e4 px 4e-6 reach^2 outgrows every gap on those sides.
        # Towards the origin (left, above) reach stays ~2 off, and at 1e5 px a gap of ~1.6e5 px exceeds the margin
        lo, hi = 0.0, next((h for h in (5.0e4, 2.0e5) if excess(h) > 0), None)
        if hi is None:
            return None
        for _ in range(60):
            mid = (lo + hi) / 2
            lo, hi = (mid, hi) if excess(mid) <= 0 else (lo, mid)
        return hi

    probes = []
    for side in range(4):
        gaps = [-3.0, -1.0, -0.25, 1.5, 2.0, 2.01, 2.5, 3.0, 8.0]
        edge = at_margin(side)
        if edge is not None:
            gaps += [edge * 0.9, edge - 0.5, edge - 0.05, edge + 0.05, edge + 0.5, edge * 1.3]
        probes += [probe(side, g) for g in gaps]
        probes += [probe(side, g, 0.5 if side % 2 else -0.5) for g in gaps if g not in (2.01, 3.0)]
        if off >= 1e4:      # small and thin boxes a few pixels away: the clip's line equations lose them in rounding at these coordinates
            for w, h, theta in ((1.5, 60.0, 0.5), (1.5, 60.0, 1.3), (2.0, 2.0, -0.5), (200.0, 2.0, 0.01)):
                probes += [probe(side, g, theta, w, h) for g in (0.1, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 8.0)]
    if off == 1000.0:                                                    # found by search with the oracle: beyond the margin, overlap 3e-5
        probes.append([1015.0, 1061.0, 2.0 ** -10, 40.0, 0.0, 3.0])
        probes.append([1072.9, 1011.0, 2.0 ** -10, 40.0, 1.2, 0.0])
    # the decoy is beyond the margin: at 1e5 px that takes a box towards the origin, 1.85e5 px to the left
    decoy = [off + 6000.0, off - 5000.0, 50.0, 30.0, 0.2, 3.0] if off < 5e4 else [off - 1.85e5, off + 5.0, 50.0, 30.0, 0.2, 3.0]
    t = torch.tensor([[decoy, p] for p in probes], dtype=torch.float32)
    return Case(True, t, [(1, 2, 64)], [(axis, quads)], 4, (1e-7, 0.5), reject=True)


# ------------------------------------------------------------------------------------------------------------------------------
# launch geometry
# ------------------------------------------------------------------------------------------------------------------------------
def _geometry_case(rotated, a, batch, seed):
    """ODTK_MAX_LEVELS levels in non-monotone size order; images with 12, 0, 5, ... rows; boxes up to the size of the largest level."""
    gen = torch.Generator().manual_seed(seed)
    classes = 5
    levels = [(h, w, s) for (h, w), s in zip(GEOMETRY, GEOMETRY_STRIDES)]
    anchors = [(_rot_anchors if rotated else _axis_anchors)(s, a) for s in GEOMETRY_STRIDES]
    n_max = 16
    t = torch.full((batch, n_max, 6 if rotated else 5), -1.0)
    for b in range(batch):
        n = (12, 0, 5, 14, 1)[b % 5] if batch > 1 else 12
        rows = _random_boxes(gen, n, 330, 330, classes, rotated, 6.0, 200.0)
        if n:
            rows[0, :2] = torch.tensor([1190.0 - 40 * b, -3.0])            # the far end of the 1 x 300 level
            rows[0, 2:4] = torch.tensor([9.0, 11.0]) if not rotated else torch.tensor([14.0, 13.0])
        t[b, (b % 2):(b % 2) + n] = rows                                    # odd images start with a padding row
    return Case(rotated, t, levels, anchors, classes, geometry=True)


CASES = {}
for _n in AXIS_ROWS:
    CASES['axis_rows_%d' % _n] = functools.partial(_staging_case, False, _n, 100 + _n)
for _n in ROT_ROWS:
    CASES['rot_rows_%d' % _n] = functools.partial(_staging_case, True, _n, 200 + _n)
CASES.update({
    'axis_duplicate': functools.partial(_duplicate_case, False, 41), 'rot_duplicate': functools.partial(_duplicate_case, True, 42),
    'axis_thresholds': functools.partial(_threshold_case, (0.4, 0.5)), 'axis_thresholds_bg_eq_fg_04': functools.partial(_threshold_case, (0.4, 0.4)),
    'axis_thresholds_bg_eq_fg_05': functools.partial(_threshold_case, (0.5, 0.5)), 'axis_ties': _tie_case,
    'axis_all_zero': functools.partial(_all_zero_case, False), 'rot_all_zero': functools.partial(_all_zero_case, True),
    'axis_nan': functools.partial(_nan_case, False), 'rot_nan': functools.partial(_nan_case, True),
    'axis_degenerate': functools.partial(_degenerate_case, False), 'rot_degenerate': functools.partial(_degenerate_case, True),
    'rot_reject_0': functools.partial(_reject_case, 0), 'rot_reject_1e3': functools.partial(_reject_case, 1e3),
    'rot_reject_1e4': functools.partial(_reject_case, 1e4), 'rot_reject_1e5': functools.partial(_reject_case, 1e5),
    'axis_geometry_a1_b17': functools.partial(_geometry_case, False, 1, 17, 51), 'axis_geometry_a9_b5': functools.partial(_geometry_case, False, 9, 5, 52),
    'axis_geometry_a32_b1': functools.partial(_geometry_case, False, MAX_ANCHORS, 1, 53),
    'rot_geometry_a1_b17': functools.partial(_geometry_case, True, 1, 17, 54), 'rot_geometry_a27_b5': functools.partial(_geometry_case, True, 27, 5, 55),
    'rot_geometry_a27_b1': functools.partial(_geometry_case, True, 27, 1, 56),
})
RANDOMISED = [n for n in CASES if '_rows_' in n and not n.endswith('_0') and not n.endswith('_1')] + \
    ['axis_duplicate', 'rot_duplicate'] + [n for n in CASES if 'geometry' in n]


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------------------------------------
def _delta_ratio(box_cells, ora, rotated):
    """max over the finite deltas of |value - float64| / delta_error_bound(K = 1); box_cells [cells, 4 | 6] in (a, y, x) order."""
    if ora['winbox'] is None:
        return 0.0
    want = targets_oracle.deltas_f64(ora['winbox'].numpy(), ora['anchor'].numpy())[:, :4]
    bound = targets_oracle.delta_error_bound(ora['winbox'].numpy(), ora['anchor'].numpy(), 1)
    got = box_cells[:, :4].astype(np.float64)
    ok = np.isfinite(want) & np.isfinite(got) & np.isfinite(bound) & (bound > 0)
    with np.errstate(all='ignore'):
        return float((np.abs(got - want)[ok] / bound[ok]).max()) if ok.any() else 0.0


def _cells(box_t):
    """[A, nb, H, W] -> [A*H*W, nb]"""
    return np.ascontiguousarray(box_t.detach().cpu().numpy().transpose(0, 2, 3, 1)).reshape(-1, box_t.shape[1])


def _compare(c, b, l, cls, box_t, depth, where):
    ora = c.oracle()[b][l]
    where = '%s image %d level %d' % (where, b, l)
    assert np.array_equal(_bits(depth), _bits(ora['depth'])), where + ': depth'
    if cls is not None:
        assert np.array_equal(_bits(cls), _bits(ora['cls'])), where + ': cls_target'
    got, want = box_t.cpu().numpy(), ora['box'].numpy()
    assert got.shape == want.shape, where
    assert np.array_equal(np.isnan(got), np.isnan(want)), where + ': NaN positions of box_target'
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), where + ': infinite deltas'
    assert np.array_equal(got == 0, want == 0), where + ': exact zeros of box_target'
    fin = np.isfinite(want)
    if c.rotated:
        assert np.array_equal(_bits(box_t[:, 4:6]), _bits(ora['box'][:, 4:6])), where + ': sin / cos'
        fin[:, 4:6] = False
    tol = 1e-5 if c.rotated else 1e-6
    assert np.allclose(got[fin], want[fin], rtol=tol, atol=tol), where + ': box_target against the fp32 oracle, worst %g' % np.abs(got[fin] - want[fin]).max()
    ratio = _delta_ratio(_cells(box_t), ora, c.rotated)
    assert ratio <= 2 * K_ORACLE, where + ': box_target is %.2f bounds from the float64 deltas' % ratio


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the cases contain what they are meant to contain, and the bound's K
# ------------------------------------------------------------------------------------------------------------------------------
def _decisions(c):
    """(foreground, ignored, background) cells of image 0: the image with every row valid"""
    d = torch.cat([lv['depth'].view(-1) for lv in c.oracle()[0]])
    return int((d > 0).sum()), int((d < 0).sum()), int((d == 0).sum())


def test_cases_are_not_vacuous():
    """With the oracle alone (no GPU).  K_ORACLE = 3: the worst ratio of the fp32 oracle to delta_error_bound(K = 1) over all
    cases was measured as 2.15 (torch's vectorised CPU log may move it by an ulp's worth from one CPU generation to another)."""
    worst = 0.0
    for name in CASES:
        c = case(name)
        for im in c.oracle():
            for lv in im:
                worst = max(worst, _delta_ratio(_cells(lv['box']), lv, c.rotated))
    assert worst <= K_ORACLE, worst

    for name in RANDOMISED:
        fg, ign, bg = _decisions(case(name))
        assert fg > 0 and ign > 0 and bg > 0, (name, fg, ign, bg)

    # winners from every staging round (image 0: all rows valid), the planted last row among them
    for name, c in ((n, case(n)) for n in CASES if '_rows_' in n or 'duplicate' in n):
        n, rnd = c.targets.shape[1], c.notes['rounds']
        if n == 0:
            continue
        lv = c.oracle()[0][0]
        assert {int(v) for v in (lv['winner'].view(-1) // rnd).unique()} == set(range((n + rnd - 1) // rnd)), name
        if c.notes.get('planted_last'):
            assert int((lv['winner'] == n - 1).sum()) > 0 and float(lv['overlap'][lv['winner'] == n - 1].max()) > 0.9, name
        # image 1 holds rows of the last round only, image 2 has valid rows at the special indices, image 3 none
        if '_rows_' in name:
            idx = c.valid_index(1)
            assert len(idx) and (int(idx.min()) // rnd == (n - 1) // rnd)
            idx2 = set(c.valid_index(2).tolist())
            assert all(i in idx2 for i in SPECIAL_ROWS if i < n) and len(c.valid_index(3)) == 0
            if n > 2:
                assert len(idx2) < n

    # duplicates: the first copy wins its cell, in both images; the last row wins its cell
    for name in ('axis_duplicate', 'rot_duplicate'):
        c = case(name)
        (src, second, third), (y, x), row = c.notes['duplicate'], c.notes['cell'], c.notes['row']
        rnd = c.notes['rounds']
        assert torch.equal(c.targets[0, src, :-1], c.targets[0, second, :-1]) and torch.equal(c.targets[0, src, :-1], c.targets[0, third, :-1])
        assert len({float(c.targets[0, i, -1]) for i in (src, second, third)}) == 3
        o0, o1 = c.oracle()[0][0], c.oracle()[1][0]
        assert int(c.valid_index(0)[o0['winner'][row, y, x]]) == src and float(o0['depth'][row, 0, y, x]) == float(c.targets[0, src, -1]) + 1
        assert int(c.valid_index(1)[o1['winner'][row, y, x]]) == second and float(o1['depth'][row, 0, y, x]) == float(c.targets[0, second, -1]) + 1
        ly, lx = c.notes['last_cell']
        assert int(c.valid_index(0)[o0['winner'][row, ly, lx]]) == c.targets.shape[1] - 1

    # thresholds: exactly the intended decisions
    cells = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    for name, want in (('axis_thresholds', ['fg', 'ign', 'bg', 'ign', 'fg', 'fg']), ('axis_thresholds_bg_eq_fg_04', ['fg', 'fg', 'bg', 'fg', 'fg', 'fg']),
                       ('axis_thresholds_bg_eq_fg_05', ['fg', 'bg', 'bg', 'bg', 'fg', 'fg'])):
        c = case(name)
        o = c.oracle()[0][0]
        for i, ((y, x), w) in enumerate(zip(cells, want)):
            assert float(o['overlap'][0, y, x]) == float(np.float32(c.notes['overlaps'][i])), (name, i)
            cl = int(c.targets[0, i, 4])
            assert float(o['depth'][0, 0, y, x]) == {'fg': cl + 1, 'ign': -1, 'bg': 0}[w], (name, i)
            assert float(o['cls'][0, cl, y, x]) == (0.0 if w == 'bg' else 1.0) and float(o['cls'][0, :, y, x].sum()) == (0.0 if w == 'bg' else 1.0)
    assert {int(v) for v in case('axis_thresholds').targets[0, :, 4]} >= {0, 4}                  # class 0 and class C - 1

    # ties: equal overlaps of different boxes, the first of the list wins
    c = case('axis_ties')
    for b, first in ((0, {(0, 0): 0, (1, 1): 2}), (1, {(0, 0): 2, (1, 1): 0})):
        o = c.oracle()[b][0]
        rows = c.targets[b][c.valid_index(b)]
        alone = torch.stack([box_oracle.snap_to_anchors(r[None], [48, 32], 16, UNIT_ANCHOR, 5, c.ious, return_winner=True)[4] for r in rows])
        for (y, x), f in first.items():
            top = (alone[:, 0, y, x] == alone[:, 0, y, x].max()).nonzero().view(-1).tolist()
            assert len(top) == 2 and top[0] == f and int(o['winner'][0, y, x]) == f and float(alone[f, 0, y, x]) > 0.5, (b, y, x, top)
            assert not torch.equal(rows[top[0]], rows[top[1]])

    # all overlaps zero: background everywhere, deltas towards the first valid row, which differ from the next row's by > 0.1
    for name in ('axis_all_zero', 'rot_all_zero'):
        c = case(name)
        for b, first in ((0, 0), (1, 0)):
            o = c.oracle()[b][0]
            assert not o['overlap'].any() and not o['depth'].any() and not o['cls'].any() and not o['winner'].any(), name
            assert int(c.valid_index(b)[0]) == (0 if b == 0 else 1)
        assert float((c.oracle()[0][0]['box'] - c.oracle()[1][0]['box'])[:, :2].abs().min()) > 0.1     # 1e4 times the bar

    # NaN rows: the NaN box wins every cell, ignored everywhere, its class channel hot; after an IoU ~1 box NaN still wins
    c = case('axis_nan')
    for b, row in ((0, 2), (1, 3)):
        o = c.oracle()[b][0]
        assert (o['winner'] == row).all() and (o['depth'] == -1).all() and torch.isnan(o['overlap']).all() and torch.isnan(o['box']).any()
        assert (o['cls'][:, int(c.targets[b, row, 4])] == 1).all() and float(o['cls'].sum()) == o['depth'].numel()
    assert not torch.isnan(case('axis_nan').oracle()[1][0]['box']).all()
    # rotated: a non-finite coordinate makes the whole quad non-finite, the polygon IoU of every pair with it NaN, and the row wins
    # every cell as above (image 2: NaN width; image 3: two rows with +inf, the first of them wins)
    c = case('rot_nan')
    for b, row in ((0, 2), (1, 3), (2, 4), (3, 1)):
        o = c.oracle()[b][0]
        assert not torch.isfinite(c.gt_quads[b, row]).any()
        assert (o['winner'] == row).all() and (o['depth'] == -1).all() and torch.isnan(o['overlap']).all(), b
        assert torch.isnan(o['box'][:, :4]).any() and not torch.isnan(o['box'][:, :4]).all()
        assert (o['cls'][:, int(c.targets[b, row, 5])] == 1).all() and float(o['cls'].sum()) == o['depth'].numel()

    # degenerate rotated boxes overlap anchors (the full clip decides something); axis-aligned ones produce -inf and NaN deltas
    assert any(float(im[0]['overlap'].max()) > 0 for im in case('rot_degenerate').oracle())
    d = torch.cat([im[0]['box'].view(-1) for im in case('axis_degenerate').oracle()])
    assert torch.isinf(d).any() or torch.isnan(d).any()

    # the reject cases: per offset, probes with zero and with non-zero overlap on BOTH sides of ... the margin where the margin can
    # be reached; a probe with gap > 0 and non-zero overlap exists beyond 1e4 px; the winner of cell (0, 0, 0) is the probe there
    for name in ('rot_reject_0', 'rot_reject_1e3', 'rot_reject_1e4', 'rot_reject_1e5'):
        c = case(name)
        aq = c.anchors[0][1][0].numpy()
        stats = {'zero': 0, 'nonzero': 0, 'below_nonzero': 0, 'above': 0, 'below': 0, 'probe_wins': 0, 'just_above': 0, 'just_below': 0}
        for b in range(c.targets.shape[0]):
            o = c.oracle()[b][0]
            gap, margin = gap_and_margin(aq, c.gt_quads[b, 1].numpy())
            dgap, dmargin = gap_and_margin(aq, c.gt_quads[b, 0].numpy())
            assert dgap > 1.1 * dmargin                                        # the decoy is rejected, and rightly so:
            assert float(targets_oracle.overlaps_from_quads(c.gt_quads[b, :1], [128, 64], 64, c.anchors[0][1])[0, 0]) == 0
            ov, win = float(o['overlap'][0, 0, 0]), int(o['winner'][0, 0, 0])
            assert win == (1 if ov > 0 else 0)
            stats['zero' if ov == 0 else 'nonzero'] += 1
            stats['probe_wins'] += win
            stats['above' if gap > margin else 'below'] += 1
            stats['just_above'] += int(0 < gap - margin <= 1)
            stats['just_below'] += int(0 <= margin - gap < 1)
            stats['below_nonzero'] += int(0 < gap <= margin and ov > 0 and _edges_at_least_one_pixel(c.gt_quads[b, 1]))
            if gap > margin and float(c.targets[b, 1, 2]) >= 1.0:
                assert ov == 0, (name, b, gap, margin, ov)                     # a rightful reject
        assert stats['zero'] and stats['nonzero'] and stats['below'] and stats['probe_wins'], (name, stats)
        # within one pixel of the margin on either side of it, on at least two sides of the square (at 1e5 px: left and above)
        assert stats['above'] >= 8 and stats['just_above'] >= 4 and stats['just_below'] >= 4, (name, stats)
        if name in ('rot_reject_1e4', 'rot_reject_1e5'):
            assert stats['below_nonzero'], (name, stats)                       # what `gap > 0` would zero wrongly
    # the sub-pixel boxes beyond the margin that the clip still gives an overlap: what the short-edge flag is for
    c = case('rot_reject_1e3')
    aq, hits = c.anchors[0][1][0].numpy(), 0
    for b in range(c.targets.shape[0]):
        gap, margin = gap_and_margin(aq, c.gt_quads[b, 1].numpy())
        if float(c.targets[b, 1, 2]) < 1.0:
            assert gap > margin and float(c.oracle()[b][0]['overlap'][0, 0, 0]) > 0 and int(c.oracle()[b][0]['winner'][0, 0, 0]) == 1
            hits += 1
    assert hits == 2

    # geometry: six levels, the three anchor counts, the three batch sizes
    seen = {(c.rotated, (c.anchors[0][0] if c.rotated else c.anchors[0]).shape[0], c.targets.shape[0]) for c in (case(n) for n in CASES if 'geometry' in n)}
    assert seen == {(False, 1, 17), (False, 9, 5), (False, MAX_ANCHORS, 1), (True, 1, 17), (True, 27, 5), (True, 27, 1)}
    assert len(GEOMETRY) == MAX_LEVELS and sorted(h * w for h, w in GEOMETRY) != [h * w for h, w in GEOMETRY]


# ------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------
def _poison(shapes):
    """NaN-filled blocks of the sizes the next call allocates, handed back to the caching allocator: its outputs start as NaN."""
    junk = [torch.full(s, float('nan'), device='cuda') for s in shapes]
    del junk


def _run(c, level_ids, want_cls, single_entry=False):
    """The kernel on the given levels of the case, in ONE launch -> (cls list | Nones, box list, depth list).  single_entry: the
    one-level entry point odtk_snap_to_anchors (axis-aligned boxes only)."""
    from odtk import _C
    b = c.targets.shape[0]
    levels = [c.levels[l] for l in level_ids]
    sizes, strides = [(h, w) for h, w, _ in levels], [s for _, _, s in levels]
    a = (c.anchors[0][0] if c.rotated else c.anchors[0]).shape[0]
    nb = 6 if c.rotated else 4
    shapes = [(b, a, k, h, w) for h, w in sizes for k in ((c.classes, nb, 1) if want_cls else (nb, 1))]
    _poison(shapes)
    if c.rotated:
        tables = [(c.anchors[l][0].cuda().contiguous(), c.anchors[l][1].cuda().contiguous()) for l in level_ids]
        out = _C.snap_to_anchors_rotated_levels(c.gt_axis.cuda(), c.gt_quads.cuda(), c.gt_class.cuda(), tables, c.classes, sizes, strides,
                                                c.ious[0], c.ious[1], want_cls)
    elif single_entry:
        (l,) = level_ids
        one = _C.snap_to_anchors(c.targets.cuda(), c.anchors[l], c.classes, sizes[0][0], sizes[0][1], strides[0], c.ious[0], c.ious[1], want_cls)
        out = ([one[0]], [one[1]], [one[2]])
    else:
        out = _C.snap_to_anchors_levels(c.targets.cuda(), [c.anchors[l] for l in level_ids], c.classes, sizes, strides, c.ious[0], c.ious[1], want_cls)
    torch.cuda.synchronize()
    assert all((t is None) == (not want_cls) for t in out[0])
    return out


def _check(c, out, level_ids, where):
    for i, l in enumerate(level_ids):
        for b in range(c.targets.shape[0]):
            _compare(c, b, l, None if out[0][i] is None else out[0][i][b], out[1][i][b], out[2][i][b], where)


def _same_bits(x, y, where):
    for i, (p, q) in enumerate(zip(x, y)):
        for u, v in zip(p, q):
            assert (u is None and v is None) or torch.equal(u.view(torch.int32), v.view(torch.int32)), '%s: output %d' % (where, i)


SINGLE_LEVEL = [n for n in CASES if 'geometry' not in n]


@pytest.mark.gpu
@pytest.mark.parametrize('want_cls', [True, False], ids=['cls', 'nocls'])
@pytest.mark.parametrize('name', SINGLE_LEVEL)
def test_kernel_equals_the_oracle(name, want_cls):
    """Staging rounds, compaction, decision edges and the distance reject: every case through the levels entry point (one level),
    axis-aligned ones through odtk_snap_to_anchors too, with and without the class map; the two entry points write the same bits."""
    from odtk import _C
    assert (_C.MAX_ANCHORS, _C.MAX_LEVELS) == (MAX_ANCHORS, MAX_LEVELS)
    c = case(name)
    out = _run(c, [0], want_cls)
    _check(c, out, [0], name + ' (levels entry)')
    if not c.rotated:
        one = _run(c, [0], want_cls, single_entry=True)
        _check(c, one, [0], name + ' (single entry)')
        _same_bits(out, one, name)


@pytest.mark.gpu
@pytest.mark.parametrize('want_cls', [True, False], ids=['cls', 'nocls'])
@pytest.mark.parametrize('name', [n for n in CASES if 'geometry' in n])
def test_launch_geometry(name, want_cls):
    """ODTK_MAX_LEVELS levels in non-monotone order in one launch == the oracle == the per-level launches (bit for bit), for
    A in {1, 9, ODTK_MAX_ANCHORS} / {1, 27} and B in {1, 5, 17}; (H, W) from one cell to hw just past 256 and a 1 x 300 row."""
    c = case(name)
    ids = list(range(len(c.levels)))
    out = _run(c, ids, want_cls)
    _check(c, out, ids, name + ' (all levels)')
    for l in ids:
        one = _run(c, [l], want_cls)
        _same_bits([[t[l]] for t in out], one, '%s level %d alone' % (name, l))
        if not c.rotated:
            single = _run(c, [l], want_cls, single_entry=True)
            _same_bits(one, single, '%s level %d through odtk_snap_to_anchors' % (name, l))
    # another order of the same levels: the table is searched by block_begin, not by size
    perm = [3, 0, 5, 1, 4, 2]
    again = _run(c, perm, want_cls)
    _same_bits([[t[l] for l in perm] for t in out], again, name + ' permuted')


@pytest.mark.gpu
def test_a_seventh_level_is_refused():
    """ODTK_MAX_LEVELS + 1 levels: an error before anything is launched, from both levels entry points."""
    for name in ('axis_geometry_a9_b5', 'rot_geometry_a1_b17'):
        c = case(name)
        with pytest.raises(RuntimeError, match='levels'):
            _run(c, list(range(MAX_LEVELS)) + [0], True)
