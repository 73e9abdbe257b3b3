"""The per-anchor-cell loss families (IoU / GIoU / DIoU, ProbIoU / KLD, quality focal / varifocal) reproduce, bit for bit, what the
library computed before their kernels, host drivers and ctypes functions were folded into one framework (csrc/cell_loss.hpp):
every `sums` tensor and every gradient of odtk._C.*_loss_levels_forward / _backward on the seeded inputs of
oracle/gen_golden_loss_bits.py against tests/golden/loss_family_bits.npz, recorded on an MI355X at the commit before the fold.

Both passes are deterministic by construction (no atomics, one fixed summation order), so equality of the bytes is the bar: there is no
tolerance.  The shapes (two levels of 7 x 9 and 2 x 3 cells, batch 2, 3 anchors, 5 classes) are the smallest that take every path;
the generator's docstring lists them."""
import os

import numpy as np
import pytest

from oracle import gen_golden_loss_bits as gen

pytestmark = pytest.mark.gpu

FAMILIES = ('box_iou', 'rotated', 'quality')
KINDS = {'box_iou': 3, 'rotated': 2, 'quality': 2 * len(gen.QUALITY_GAMMAS)}


@pytest.fixture(scope='module')
def computed():
    return gen.compute()


@pytest.fixture(scope='module')
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, 'loss_family_bits.npz')) as z:
        return {k: z[k] for k in z.files}


def test_golden_covers_every_case(golden, computed):
    """Every kind x dtype x layout has its sums and, with and without an upstream gradient, one gradient per level."""
    assert set(computed) == set(golden)
    per_case = 1 + 2 * len(gen.SIZES)
    assert len(golden) == sum(KINDS.values()) * len(gen.DTYPES) * len(gen.LAYOUTS) * per_case
    # the inputs do what the shapes are for: foreground on both levels, none in the last image, and gradients that are not all zero
    sums = golden['box_iou.iou.fp32.nchw.sums'].view(np.float64).reshape(len(gen.SIZES), 2)
    assert sums[:, 1].tolist() == [91.0, 6.0] and (sums[:, 0] > 0).all()
    assert golden['box_iou.iou.fp32.nchw.grad_up.1'].any() and not golden['box_iou.iou.fp32.nchw.grad_none.1'].any()


@pytest.mark.parametrize('family', FAMILIES)
def test_same_bits_as_before_the_fold(family, golden, computed):
    names = sorted(k for k in golden if k.startswith(family + '.'))
    assert names
    differing = [k for k in names if golden[k].shape != computed[k].shape or not np.array_equal(golden[k], computed[k])]
    assert not differing, '%d of %d arrays differ: %s' % (len(differing), len(names), differing[:8])
