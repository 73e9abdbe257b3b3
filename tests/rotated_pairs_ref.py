"""Directed inputs for the rotated box-pair test (csrc/rotated_iou.hpp) and a float32 restatement of its distance reject.

Every generator is deterministic and returns (m, j): two [n, 6] float32 arrays of [x1, y1, x2, y2, sin, cos] boxes, m the kept
box and j the lower-scored one.  `far_apart_terms` / `far_apart` restate `rotated_far_apart` operation by operation in numpy
float32 (the library is built without FMA contraction, so every float32 operation there is one float32 operation here).  The
restatement is used for two things only: to PLACE pairs on either side of the reject's boundary and to COUNT how many landed
where.  It never decides an expected result -- those come from the C oracle (oracle/c/odtk_oracle.c) alone, which has no reject.

No GPU is used here."""
import numpy as np

F = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# the reject, restated
# ---------------------------------------------------------------------------------------------------------------------
def far_apart_terms(m, j, own_angle):
    """-> (far, bound, proper) of rotated_far_apart, float32 [n] / bool [n]; bound = rr * 1.001 + 2 + 4e-6 * reach^2."""
    m, j = np.asarray(m, F).reshape(-1, 6), np.asarray(j, F).reshape(-1, 6)
    with np.errstate(all='ignore'):
        sm = m[:, 4] if own_angle else j[:, 4]
        cm = m[:, 5] if own_angle else j[:, 5]
        wm, hm = m[:, 2] - m[:, 0], m[:, 3] - m[:, 1]
        kj = np.abs(j[:, 4]) + np.abs(j[:, 5])
        km = np.abs(sm) + np.abs(cm)
        rr = F(0.5) * ((np.abs(j[:, 2] - j[:, 0]) + np.abs(j[:, 3] - j[:, 1])) * kj + (np.abs(wm) + np.abs(hm)) * km)
        sxm, sym = m[:, 0] + m[:, 2], m[:, 1] + m[:, 3]
        # fmaxf returns the other operand when one is NaN: np.fmax
        far = F(0.5) * np.fmax(np.abs((j[:, 0] + j[:, 2]) - sxm), np.abs((j[:, 1] + j[:, 3]) - sym))
        reach = F(0.5) * (np.abs(sxm) + np.abs(sym)) + far + rr
        proper = (wm * km >= F(1.5)) & (hm * km >= F(1.5))
        bound = rr * F(1.001) + F(2.0) + F(4e-6) * reach * reach
    assert far.dtype == F and bound.dtype == F
    return far, bound, proper


def far_apart(m, j, thr, own_angle):
    """rotated_far_apart(m, j, thr, own_angle) for every pair: bool [n]."""
    far, bound, proper = far_apart_terms(m, j, own_angle)
    if not F(thr) >= F(0.0):
        return np.zeros(far.shape, bool)
    with np.errstate(all='ignore'):
        return proper & (far > bound)


# ---------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------
def box6(cx, cy, w, h, s, c):
    """[x1, y1, x2, y2, sin, cos] float32 from centre / size (float64 arithmetic, rounded once)."""
    cx, cy, w, h, s, c = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (cx, cy, w, h, s, c)))
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, s, c], -1).astype(F).reshape(-1, 6)


DIRECTIONS = ((1, 0), (0, 1), (1, 1), (-1, 0), (0, -1), (-1, 1), (1, -1), (-1, -1))


def boundary_offset(mcx, mcy, mw, mh, ms, mc, jw, jh, js, jc, own_angle, t, root=0):
    """Centre distance d (along x, along y, or along both) at which far = t * bound, in real arithmetic: bound is quadratic
    in d through reach, so there are two such distances (root 0: where the reject starts to fire; root 1: where, at large
    coordinates, the 4e-6 * reach^2 term overtakes it again) or none (-> None: the reject cannot fire for this kept box)."""
    km = abs(ms) + abs(mc) if own_angle else abs(js) + abs(jc)
    kj = abs(js) + abs(jc)
    rr = 0.5 * ((abs(jw) + abs(jh)) * kj + (abs(mw) + abs(mh)) * km)
    a0, c0 = rr * 1.001 + 2.0, abs(mcx) + abs(mcy) + rr
    # d = t * (a0 + 4e-6 * (c0 + d)^2)
    qa, qb, qc = 4e-6 * t, 8e-6 * t * c0 - 1.0, t * (a0 + 4e-6 * c0 * c0)
    disc = qb * qb - 4 * qa * qc
    if disc <= 0:
        return None
    return (-qb - np.sqrt(disc)) / (2 * qa) if root == 0 else (-qb + np.sqrt(disc)) / (2 * qa)


def _place(rows, mcx, mcy, mw, mh, ms, mc, jw, jh, js, jc, own_angle, t, direction, root=0):
    d = boundary_offset(mcx, mcy, mw, mh, ms, mc, jw, jh, js, jc, own_angle, t, root)
    if d is None:
        return False
    rows.append((box6(mcx, mcy, mw, mh, ms, mc)[0], box6(mcx + d * direction[0], mcy + d * direction[1], jw, jh, js, jc)[0]))
    return True


def _stack(rows):
    return np.stack([r[0] for r in rows]).astype(F), np.stack([r[1] for r in rows]).astype(F)


# offsets relative to the boundary: a fine ladder right at it, and a sweep over the +-5 % window the tests count in
T_SWEEP = tuple(1.0 + s * d for d in (3e-7, 1e-6, 1e-5, 1e-4, 1e-3, 5e-3, 0.01, 0.02, 0.03, 0.045) for s in (-1, 1))
ANGLES = (0.0, 0.4, 1.2, 2.0, 2.9, -0.7, -1.9, -2.6, 3.6, -4.5, 6.9, -6.5)      # all four quadrants, and beyond +-pi


def boundary_pairs(own_angle):
    """Centre offsets swept across the boundary of the reject (placed for the given own_angle mode) along x, along y and
    diagonally; kept-box centres of magnitude 1e1, 1e3, 1e4 and -- the far root -- j at 1e5; sizes 2..1000 px; angles in all
    four quadrants and beyond +-pi.  A part of the pairs are thin, long, axis-aligned boxes laid end to end along the sweep:
    for them |sin| + |cos| = |(sin, cos)| and w + h ~ w, the radius bound is tight, and pairs just inside the boundary
    really overlap (the only geometry in which they can: see test_rotated_pairs.py)."""
    rng = np.random.default_rng(20240 + int(own_angle))
    rows = []
    for mag in (1e1, 1e3, 1e4, 1e5):
        for di, direction in enumerate(DIRECTIONS):
            for ti, t in enumerate(T_SWEEP):
                sx, sy = rng.choice((-1.0, 1.0), 2)
                # 1e5: the kept box sits at a few 1e4 (beyond |cx| + |cy| ~ 6e4 the reject never fires) and j at the far root
                base = mag if mag < 1e5 else 2.2e4
                mcx, mcy = sx * base * rng.uniform(0.5, 1.0), sy * base * rng.uniform(0.5, 1.0)
                root = 1 if mag == 1e5 else 0
                # general position: log-uniform sizes, any angle
                mw, mh, jw, jh = np.exp(rng.uniform(np.log(2.0), np.log(1000.0), 4))
                am, aj = ANGLES[(di + ti) % len(ANGLES)], ANGLES[(di + 5 * ti + 3) % len(ANGLES)]
                _place(rows, mcx, mcy, mw, mh, np.sin(am), np.cos(am), jw, jh, np.sin(aj), np.cos(aj), own_angle, t, direction, root)
                # thin boxes end to end along an axis (exact (0, 1) / (1, 0) sin-cos; the quarter turn swaps the roles of w, h)
                if direction[0] == 0 or direction[1] == 0:
                    along_x = direction[1] == 0
                    long_m, long_j = rng.uniform(300.0, 1000.0), rng.uniform(2.0, 1000.0)
                    thin_m, thin_j = rng.uniform(2.0, 3.0, 2)
                    for quarter in (False, True):
                        lay = along_x != quarter
                        mw_, mh_ = (long_m, thin_m) if lay else (thin_m, long_m)
                        jw_, jh_ = (long_j, thin_j) if lay else (thin_j, long_j)
                        s, c = (1.0, 0.0) if quarter else (0.0, 1.0)
                        _place(rows, mcx, mcy, mw_, mh_, s, c, jw_, jh_, s, c, own_angle, t, direction, root)
                        if mag <= 1e3 and t < 1.0:       # ... and once more a little further inside: these overlap for certain
                            _place(rows, mcx, mcy, mw_, mh_, s, c, jw_, jh_, s, c, own_angle, 0.955 + 0.04 * (ti / len(T_SWEEP)), direction, root)
    # a kept box at 1e5 on both axes: no offset reaches the boundary (the margin outgrows the distance); swept anyway
    for ti, t in enumerate(T_SWEEP):
        mw, mh, jw, jh = np.exp(rng.uniform(np.log(2.0), np.log(1000.0), 4))
        d = 0.5 * (mw + mh + jw + jh) * t
        rows.append((box6(1e5, -1e5, mw, mh, 0.0, 1.0)[0], box6(1e5 + d, -1e5, jw, jh, 0.0, 1.0)[0]))
    return _stack(rows)


NORMS = (0.01, 0.1, 0.6, 1.4, 10.0)


def _sincos_variants():
    out = []
    for n in NORMS:
        for a in (0.0, 0.6, 2.3, -1.1):
            out.append((n * np.sin(a), n * np.cos(a)))
    out += [(0.0, 0.0), (0.8, 0.0), (-3.0, 0.0), (0.0, 0.5), (0.0, 7.0), (0.6, -0.8), (0.0, -1.0), (-0.3, -2.0)]
    return out


def norm_pairs(own_angle):
    """(sin, cos) of norm 0.01, 0.1, 0.6, 1.4 and 10 -- the network does not normalise it --, (0, 0), (s, 0), (0, c) and a
    negative cos, on m and on j independently, with the centre offset on both sides of the boundary and well inside it."""
    rng = np.random.default_rng(31 + int(own_angle))
    var = _sincos_variants()
    rows = []
    for vi, (ms, mc) in enumerate(var):
        for vj, (js, jc) in enumerate(var):
            if (vi * 7 + vj) % 3:                    # a third of the combinations
                continue
            mw, mh, jw, jh = rng.uniform(4.0, 120.0, 4)
            mcx, mcy = rng.uniform(-300.0, 300.0, 2)
            for k, t in enumerate((0.2, 0.6, 0.97, 0.9999, 1.0001, 1.03)):
                _place(rows, mcx, mcy, mw, mh, ms, mc, jw, jh, js, jc, own_angle, t, DIRECTIONS[(vi + vj + k) % 8])
    return _stack(rows)


def own_angle_pairs():
    """m and j with very different angles AND very different (sin, cos) norms, so that the two modes give different quads and
    different radius bounds: placed at the boundary of either mode, and at centre distances between the two."""
    rng = np.random.default_rng(47)
    rows = []
    for am in ANGLES:
        for aj in ANGLES[::3]:
            for nm, nj in ((1.0, 1.0), (10.0, 0.1), (0.1, 10.0), (1.4, 0.6), (10.0, 1.0), (3.0, 0.3)):
                mw, mh, jw, jh = rng.uniform(6.0, 200.0, 4)
                mcx, mcy = rng.uniform(-500.0, 500.0, 2)
                args = (mcx, mcy, mw, mh, nm * np.sin(am), nm * np.cos(am), jw, jh, nj * np.sin(aj + 1.3), nj * np.cos(aj + 1.3))
                d_own, d_j = boundary_offset(*args, True, 1.0), boundary_offset(*args, False, 1.0)
                direction = DIRECTIONS[len(rows) % 8]
                for d in (0.98 * d_own, 1.02 * d_own, 0.98 * d_j, 1.02 * d_j, 0.5 * (d_own + d_j), 0.3 * min(d_own, d_j),
                          0.9 * max(d_own, d_j)):
                    rows.append((box6(*args[:6])[0], box6(mcx + d * direction[0], mcy + d * direction[1], *args[6:])[0]))
    return _stack(rows)


def improper_pairs(own_angle):
    """Quads that are not `proper`: w < 0, h < 0, both, w = 0, h = 0, and w * km just below / just above 1.5 -- on the kept
    box (first half) and on j (second half) -- near the other box, around the boundary and far beyond it."""
    rng = np.random.default_rng(59 + int(own_angle))
    sizes = [(-40.0, 30.0), (25.0, -60.0), (-35.0, -45.0), (0.0, 50.0), (40.0, 0.0), (0.0, 0.0), (0.0, 0.0), (0.0, 0.0), (-3.0, 2.0),
             (1.499, 20.0), (1.501, 20.0), (20.0, 1.499), (20.0, 1.501), (1.0, 1.0), (-200.0, 150.0), (120.0, -90.0)]
    rows = []
    for on_m in (True, False):
        for (w, h) in sizes:
            for ai, a in enumerate(ANGLES[:8]):
                ow, oh = rng.uniform(10.0, 150.0, 2)
                oa = ANGLES[(ai + 5) % len(ANGLES)]
                mcx, mcy = rng.uniform(-400.0, 400.0, 2)
                # w * km: the thresholds are meant at km = 1, i.e. an exact (0, 1) / (1, 0) pair for those sizes
                # (in the reference's mode km is taken from j: BOTH boxes get the exact pair then)
                edge = 1.0 < abs(w) < 2.0 or 1.0 < abs(h) < 2.0
                s, c = ((0.0, 1.0) if ai % 2 else (1.0, 0.0)) if edge else (np.sin(a), np.cos(a))
                os_, oc = ((1.0, 0.0) if ai % 4 < 2 else (0.0, -1.0)) if edge else (np.sin(oa), np.cos(oa))
                m_args = (w, h, s, c) if on_m else (ow, oh, os_, oc)
                j_args = (ow, oh, os_, oc) if on_m else (w, h, s, c)
                for k, t in enumerate((0.0, 0.15, 0.5, 0.98, 1.02, 1.5, 3.0, 10.0)):
                    _place(rows, mcx, mcy, *m_args, *j_args, own_angle, max(t, 1e-9), DIRECTIONS[(ai + k) % 8])
    return _stack(rows)


def _grid_box(rng, n):
    x1, y1 = rng.integers(0, 5, n), rng.integers(0, 5, n)
    w, h = rng.integers(1, 6 - x1), rng.integers(1, 6 - y1)
    quarter = rng.integers(0, 2, n)
    return np.stack([8.0 * x1, 8.0 * y1, 8.0 * (x1 + w), 8.0 * (y1 + h), quarter, 1 - quarter], 1).astype(F)


def degenerate_pairs():
    """Axis-aligned and quarter-turn boxes on an integer grid (coordinates 8 * {0..5}, sizes of whole cells, (sin, cos)
    exactly (0, 1) or (1, 0)): what a quantised or clamped decode produces, and where the clip degenerates -- vertices on
    clip lines, parallel coincident edges (0 / 0 and x / 0 intersections), more than 8 emitted vertices.  Random pairs of the
    grid; the same grid scaled by 2^59 (exact; products of two coordinates overflow fp32, so `uni` becomes NaN as well); then
    the named sub-cases for every square / rectangle of the grid."""
    rng = np.random.default_rng(73)
    m, j = _grid_box(rng, 14000), _grid_box(rng, 14000)
    hm, hj = _grid_box(rng, 1500), _grid_box(rng, 1500)
    hm[:, :4] *= F(2.0 ** 59)
    hj[:, :4] *= F(2.0 ** 59)
    ms, js = [m, hm], [j, hj]

    def add(a, b):
        ms.append(np.asarray(a, F).reshape(-1, 6))
        js.append(np.asarray(b, F).reshape(-1, 6))

    up, turn = (0.0, 1.0), (1.0, 0.0)
    for x in range(0, 4):
        for y in range(0, 4):
            for w in range(1, 6 - x):
                for h in range(1, 6 - y):
                    X1, Y1, X2, Y2 = 8.0 * x, 8.0 * y, 8.0 * (x + w), 8.0 * (y + h)
                    b = (X1, Y1, X2, Y2)
                    for sc_m in (up, turn):
                        for sc_j in (up, turn):
                            add(b + sc_m, b + sc_j)                                              # identical / the same box at 0 and 90 degrees
                            add(b + sc_m, (X2, Y1, X2 + 8.0 * w, Y2) + sc_j)                     # touching edges (side by side)
                            add(b + sc_m, (X1, Y2, X2, Y2 + 8.0 * h) + sc_j)                     # touching edges (stacked)
                            add(b + sc_m, (X1, Y1, X2 + 8.0, Y2 + 8.0) + sc_j)                   # shared same-numbered corner
                            add((X1, Y1, X2 + 8.0, Y2 + 8.0) + sc_m, b + sc_j)
                            add((X1, Y1, X2 + 16.0, Y2) + sc_m, (X1 + 8.0, Y1, X2 + 8.0, Y2) + sc_j)   # shared edge lines, overlapping
                            add((X1, Y1, X2 + 8.0, Y2 + 16.0) + sc_m, (X1, Y1 + 8.0, X2, Y2 + 8.0) + sc_j)   # inside, sharing an edge
                            add((X1, Y1 + 8.0, X2, Y2 + 8.0) + sc_m, (X1, Y1, X2 + 8.0, Y2 + 16.0) + sc_j)
    return np.concatenate(ms), np.concatenate(js)


def nonfinite_pairs():
    """NaN, +inf or -inf in one coordinate, or in sin or cos, of m or of j; the other box is finite and either overlaps the
    finite version of the pair or lies far from it.  (Scores and classes stay finite; no field is ever an index.)"""
    rows = []
    bases = [((100.0, 80.0, 60.0, 40.0, np.sin(0.3), np.cos(0.3)), (110.0, 90.0, 50.0, 70.0, np.sin(-0.9), np.cos(-0.9))),
             ((24.0, 24.0, 16.0, 16.0, 0.0, 1.0), (24.0, 24.0, 16.0, 16.0, 1.0, 0.0)),
             ((-50.0, 300.0, 30.0, 90.0, np.sin(2.0), np.cos(2.0)), (4000.0, -2500.0, 80.0, 20.0, np.sin(1.0), np.cos(1.0)))]
    for mb, jb in bases:
        m0, j0 = box6(*mb)[0], box6(*jb)[0]
        for on_m in (True, False):
            for field in range(6):
                for v in (np.nan, np.inf, -np.inf):
                    m, j = m0.copy(), j0.copy()
                    (m if on_m else j)[field] = v
                    rows.append((m, j))
    return _stack(rows)


def all_generators(own_angle):
    """name -> (m, j) for the given mode (the placement of the boundary depends on it)."""
    return {'boundary': boundary_pairs(own_angle), 'norm': norm_pairs(own_angle), 'improper': improper_pairs(own_angle),
            'own_angle': own_angle_pairs(), 'degenerate': degenerate_pairs(), 'nonfinite': nonfinite_pairs()}
