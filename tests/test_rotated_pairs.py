"""The distance reject in front of the rotated polygon clip (csrc/rotated_iou.hpp: rotated_far_apart) and the inputs that pin
it, on the CPU.

Two things are established here, without a GPU, so that tests/test_gpu_rotated_pairs.py can rely on them:

  soundness   whenever the reject AS WRITTEN (tests/rotated_pairs_ref.py restates it in float32, operation by operation)
              fires for a pair, the C oracle -- which has no reject and clips every pair -- does not suppress that pair;
  coverage    the directed generators really reach what they claim to: both sides of the reject's boundary, improper kept
              quads that DO suppress a far-away box (the pairs the `proper` guard exists for), clips that emit more than 8
              vertices, NaN intersections, NaN unions.  These are conditions on the INPUTS, asserted, not logged.

What cannot be had, and why (figures from this file's own counts):

  * A pair within 5 % of the boundary cannot have an overlap above 0.3 (let alone 1.0) if its quads are well-formed.  The
    boundary is far >= 0.95 * (rr * 1.001 + 2), rr >= r_j + r_m with equality only for axis-aligned thin boxes laid end to
    end; there the overlapping length is L <= 0.5 (W + w) - far <= 0.025 (W + w), so overlap = L / (W + w - L) <= 0.026.
    "At least 64 not-rejected boundary pairs with an oracle overlap above thr" is therefore asserted at thr = 0 only; the
    reject does not look at thr beyond its sign, so a reject that fired too often is caught there for every thr >= 0.
    (The improper generator does have such pairs -- a kept POINT suppresses whatever it meets -- and they are counted.)
  * With own_angle off both quads are turned by j's angle, the grid's boxes stay parallel rectangles, and no clip edge
    ever emits more than 8 vertices (0 of ~22 000 pairs); the cap is reached with own_angle on (and by the pairwise IoU,
    which takes the corner quads of that mode)."""
import functools

import numpy as np
import pytest

from oracle import c_oracle
import rotated_pairs_ref as ref

GENERATORS = ('boundary', 'norm', 'improper', 'own_angle', 'degenerate', 'nonfinite')
THRESHOLDS = (0.0, 0.3, 1.0)


@functools.lru_cache(maxsize=None)
def _case(name, own):
    """(m, j, overlap, max emitted, inter NaN, uni NaN, later edge crosses) of one generator; computed once, never modified."""
    m, j = ref.all_generators(own)[name]
    st = [c_oracle.rotated_overlap_stats(a, b, own) for a, b in zip(m, j)]
    cols = [np.array([s[k] for s in st]) for k in range(5)]
    # the statistics entry point returns the overlap of the plain one, bit for bit (NaN included)
    plain = np.array([c_oracle.rotated_overlap(a, b, own) for a, b in zip(m[::7], j[::7])], np.float32)
    assert np.array_equal(plain.view(np.uint32), cols[0][::7].astype(np.float32).view(np.uint32))
    for a in (m, j) + tuple(cols):
        a.setflags(write=False)
    return (m, j) + tuple(cols)


def test_restatement_matches_a_scalar_reading_of_the_kernel_source():
    """The vectorised restatement against a literal scalar transcription of rotated_far_apart's lines (np.float32 scalars)."""
    F = np.float32
    m, j = ref.all_generators(True)['norm']
    m2, j2 = ref.all_generators(False)['improper']
    for own, (mm, jj) in ((True, (m[::5], j[::5])), (False, (m2[::5], j2[::5]))):
        far, bound, proper = ref.far_apart_terms(mm, jj, own)
        for i, (a, b) in enumerate(zip(mm, jj)):
            with np.errstate(all='ignore'):
                sm, cm = (a[4], a[5]) if own else (b[4], b[5])
                wm, hm = a[2] - a[0], a[3] - a[1]
                kj, km = abs(b[4]) + abs(b[5]), abs(sm) + abs(cm)
                rr = F(0.5) * ((abs(b[2] - b[0]) + abs(b[3] - b[1])) * kj + (abs(wm) + abs(hm)) * km)
                sxm, sym = a[0] + a[2], a[1] + a[3]
                f = F(0.5) * np.fmax(abs((b[0] + b[2]) - sxm), abs((b[1] + b[3]) - sym))
                reach = F(0.5) * (abs(sxm) + abs(sym)) + f + rr
                bd = rr * F(1.001) + F(2.0) + F(4e-6) * reach * reach
            assert f.dtype == F and bd.dtype == F
            assert np.array_equal(np.array([f, bd]).view(np.uint32), np.array([far[i], bound[i]]).view(np.uint32))
            assert bool(proper[i]) == bool(wm * km >= F(1.5) and hm * km >= F(1.5))


@pytest.mark.parametrize('own', [False, True])
@pytest.mark.parametrize('name', GENERATORS)
def test_reject_as_written_is_sound(name, own):
    m, j, ov = _case(name, own)[:3]
    for thr in THRESHOLDS:
        rejected = ref.far_apart(m, j, thr, own)
        with np.errstate(invalid='ignore'):
            suppressed = ov > np.float32(thr)
        bad = np.flatnonzero(rejected & suppressed)
        assert bad.size == 0, 'rejected but suppressed by the full clip: %s' % [(m[i], j[i], ov[i]) for i in bad[:3]]
    assert not ref.far_apart(m, j, -0.1, own).any() and not ref.far_apart(m, j, np.nan, own).any()   # thr < 0 | NaN: reject off


@pytest.mark.parametrize('own', [False, True])
def test_boundary_generator_lands_on_both_sides(own):
    m, j, ov = _case('boundary', own)[:3]
    far, bound, proper = ref.far_apart_terms(m, j, own)
    ratio = far.astype(np.float64) / bound.astype(np.float64)
    assert proper.all()
    for thr in THRESHOLDS:
        rejected = ref.far_apart(m, j, thr, own)
        # thr = 0, 0.3: within 5 % of the boundary on either side; thr = 1.0: the rejected ones above it by no more than 5 %
        # (a rejected pair IS above the boundary, so one window serves both readings)
        window = np.abs(ratio - 1.0) <= 0.05
        assert (rejected & window & (ratio > 1.0)).sum() >= 256
        assert (~rejected & window).sum() >= 256
    # right AT the boundary: both verdicts within one part in 1e5 of it
    near = np.abs(ratio - 1.0) <= 1e-5
    rejected = ref.far_apart(m, j, 0.0, own)
    assert (near & rejected).sum() >= 32 and (near & ~rejected).sum() >= 32
    # not-rejected boundary pairs that the full clip suppresses (see the module docstring for thr > 0)
    assert (~rejected & (np.abs(ratio - 1.0) <= 0.05) & (ov > 0.0)).sum() >= 64
    # coordinate magnitudes 1e1 .. 1e5, sizes 2 .. 1000 px, angles in all four quadrants
    # (of the kept box's centre: 1e1, 1e3, 1e4; 1e5 is where j lies at the far root of a kept box at a few 1e4)
    centre = np.maximum(np.abs(m[:, 0] + m[:, 2]), np.abs(m[:, 1] + m[:, 3])) / 2
    for lo, hi in ((5, 10), (5e2, 1e3), (5e3, 1e4)):
        assert (((centre >= lo) & (centre <= hi)) & rejected).sum() >= 16, (lo, hi)
    assert ((np.abs(j[:, :4]).max(1) >= 8e4) & rejected).sum() >= 16
    size = np.concatenate([m[:, 2] - m[:, 0], m[:, 3] - m[:, 1], j[:, 2] - j[:, 0], j[:, 3] - j[:, 1]])
    assert size.min() >= 1.99 and size.min() < 3 and size.max() > 900 and size.max() <= 1000.01
    for sign_s in (-1, 1):
        for sign_c in (-1, 1):
            assert ((np.sign(m[:, 4]) == sign_s) & (np.sign(m[:, 5]) == sign_c)).sum() >= 16


@pytest.mark.parametrize('own', [False, True])
def test_improper_generator_holds_the_pairs_the_guard_exists_for(own):
    m, j, ov = _case('improper', own)[:3]
    far, bound, proper = ref.far_apart_terms(m, j, own)
    beyond = far > bound
    guarded = ~proper & beyond & (ov > 0.0)               # without `proper &&` the reject would fire; the oracle suppresses
    assert guarded.sum() >= 64, guarded.sum()
    assert not ref.far_apart(m[guarded], j[guarded], 0.0, own).any()
    # all the classes of improper kept quads are there, on both sides of 1.5
    wm, hm = m[:, 2] - m[:, 0], m[:, 3] - m[:, 1]
    assert ((wm < 0) & (hm > 0)).sum() >= 32 and ((hm < 0) & (wm > 0)).sum() >= 32 and ((wm < 0) & (hm < 0)).sum() >= 32
    assert ((wm == 0) & (hm > 0)).sum() >= 32 and ((hm == 0) & (wm > 0)).sum() >= 32
    assert ((wm > 1.49) & (wm < 1.5) & ~proper).sum() >= 16 and ((wm > 1.5) & (wm < 1.51) & proper).sum() >= 16
    assert ((hm > 1.49) & (hm < 1.5) & ~proper).sum() >= 16 and ((hm > 1.5) & (hm < 1.51) & proper).sum() >= 16
    wj = j[:, 2] - j[:, 0]
    assert (wj < 0).sum() >= 32 and (wj == 0).sum() >= 32   # ... and the same set on j (which the guard does not look at)


def test_norm_and_own_angle_generators_separate_the_two_modes():
    m, j = ref.all_generators(True)['norm'][0], ref.all_generators(True)['norm'][1]
    norms = np.hypot(np.concatenate([m[:, 4], j[:, 4]]).astype(np.float64), np.concatenate([m[:, 5], j[:, 5]]).astype(np.float64))
    for n in ref.NORMS:
        assert (np.abs(norms / n - 1.0) < 1e-3).sum() >= 32, n
    assert (norms == 0).sum() >= 16
    assert ((m[:, 4] != 0) & (m[:, 5] == 0)).sum() >= 16 and ((m[:, 4] == 0) & (m[:, 5] != 0)).sum() >= 16 and (m[:, 5] < 0).sum() >= 16
    # own-angle generator: pairs on which the reject's verdict depends on the mode, in both directions, and pairs that
    # the oracle suppresses in one mode only
    m, j, ov_own = _case('own_angle', True)[:3]
    ov_j = _case('own_angle', False)[2]
    r_own, r_j = ref.far_apart(m, j, 0.0, True), ref.far_apart(m, j, 0.0, False)
    assert (r_own & ~r_j).sum() >= 64 and (~r_own & r_j).sum() >= 64
    assert ((ov_own > 0) != (ov_j > 0)).sum() >= 64
    # pairs that a reject which always took j's (sin, cos) would wrongly drop when own_angle is set
    assert (r_j & (ov_own > 0)).sum() >= 64


def test_degenerate_generator_reaches_the_cap_and_the_nan_rules():
    m, j, ov, nq, nan_i, nan_u, cross = _case('degenerate', True)
    finite = np.abs(m[:, :4]).max(1) < 1e6
    # integer grid, exact quarter turns
    assert np.array_equal(m[finite, :4] % 8, np.zeros_like(m[finite, :4])) and np.array_equal(j[finite, :4] % 8, np.zeros_like(j[finite, :4]))
    assert set(map(tuple, np.concatenate([m[:, 4:], j[:, 4:]]))) == {(0.0, 1.0), (1.0, 0.0)}
    assert ((nq > 8) & finite).sum() >= 64, (nq > 8).sum()
    assert ((nq > 8) & cross & finite).sum() >= 32, ((nq > 8) & cross).sum()
    assert nq.max() >= 12
    assert nan_i.sum() >= 64 and (nan_i & finite).sum() >= 64
    assert (nan_i & nan_u).sum() >= 16 and np.all(ov[nan_i & nan_u] == 1.0)
    assert np.all(ov[nan_i & ~nan_u] == 0.0)
    # the named sub-cases
    same = np.all(m[:, :4] == j[:, :4], 1) & finite
    assert (same & np.all(m[:, 4:] == j[:, 4:], 1)).sum() >= 64                                  # identical boxes
    square = same & ((m[:, 2] - m[:, 0]) == (m[:, 3] - m[:, 1]))
    assert (square & (m[:, 4] != j[:, 4]) & (nq >= 10)).sum() >= 16                              # the same square at 0 and 90 degrees
    # reference mode: parallel rectangles never go over the cap (module docstring); the NaN rules are still reached
    nq0, nan0, nanu0 = _case('degenerate', False)[3:6]
    assert nq0.max() <= 8
    assert nan0.sum() >= 64 and (nan0 & nanu0).sum() >= 16


def test_nonfinite_generator_has_every_field_on_both_boxes():
    m, j = ref.nonfinite_pairs()
    for a, other in ((m, j), (j, m)):
        assert np.isfinite(other[~np.isfinite(a).all(1)]).all()
        for f in range(6):
            col = a[:, f]
            assert np.isnan(col).sum() >= 3 and (col == np.inf).sum() >= 3 and (col == -np.inf).sum() >= 3
    for own in (False, True):                              # nothing non-finite is ever "far apart": the full path decides
        used = m if own else m[:, :4]                     # (the kept box's own sin / cos are not read in the reference's mode)
        bad = ~np.isfinite(used).all(1) | ~np.isfinite(j).all(1)
        assert bad.sum() >= 90 and not ref.far_apart(m[bad], j[bad], 0.0, own).any()
