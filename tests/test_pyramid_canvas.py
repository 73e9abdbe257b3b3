"""The pyramid canvas without a GPU (odtk/fused.py: pyramid_canvas_layout, FusedRetinaNet._canvas_towers): the layout's invariants
for any input size, and the canvas path against the per-level path on an fp32 engine run with plain torch on the CPU."""
import itertools

import pytest
import torch

from odtk import fused
from odtk.model import Model


def _levels(height, width, first=4, last=7):
    """Extents of the pyramid levels P`first`..P`last` of an input (each level is the ceiling half of the one above, from stride 8)."""
    h, w = -(-height // 8), -(-width // 8)
    out = []
    for level in range(3, last + 1):
        if level >= first:
            out.append((h, w))
        h, w = -(-h // 2), -(-w // 2)
    return out


SIZES = [(128, 128), (800, 1280), (1333, 800), (800, 1333), (127, 129), (301, 77), (64, 640), (640, 64), (1, 1), (2049, 33)]


@pytest.mark.parametrize('gutter', [0, 1, 2, 3])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_layout_invariants(size, gutter):
    for first, last in [(4, 7), (5, 7), (4, 5), (3, 7), (4, 4), (4, 8)]:
        shapes = _levels(*size, first=first, last=last)
        (height, width), origins = fused.pyramid_canvas_layout(shapes, gutter)
        assert len(origins) == len(shapes) and origins[0] == (0, 0)
        rects = [(y, x, y + h, x + w) for (y, x), (h, w) in zip(origins, shapes)]
        for y0, x0, y1, x1 in rects:                                  # inside the canvas
            assert 0 <= y0 < y1 <= height and 0 <= x0 < x1 <= width
        assert height == max(r[2] for r in rects) and width == max(r[3] for r in rects)      # and the canvas is no larger than needed
        for a, b in itertools.combinations(rects, 2):                 # disjoint and at least `gutter` apart along one axis
            apart_y = max(b[0] - a[2], a[0] - b[2])
            apart_x = max(b[1] - a[3], a[1] - b[3])
            assert max(apart_y, apart_x) >= gutter, (shapes, origins)
        # every pixel within `gutter` of a level belongs to that level, to no level, or lies outside the canvas (a painted check)
        paint = torch.full((height, width), -1, dtype=torch.long)
        for i, (y0, x0, y1, x1) in enumerate(rects):
            assert (paint[y0:y1, x0:x1] == -1).all()
            paint[y0:y1, x0:x1] = i
        for i, (y0, x0, y1, x1) in enumerate(rects):
            halo = paint[max(y0 - gutter, 0):y1 + gutter, max(x0 - gutter, 0):x1 + gutter]
            assert ((halo == i) | (halo == -1)).all(), (shapes, origins)


def test_layout_of_the_flagship_shape():
    """P4..P7 of 800 x 1280: P4 on the left, P5 over (P6, P7) on the shelf -- 50 x 121, 6050 pixels for 5330 of levels."""
    shapes = [(50, 80), (25, 40), (13, 20), (7, 10)]
    assert fused.pyramid_canvas_layout(shapes, 1) == ((50, 121), [(0, 0), (0, 81), (26, 81), (26, 102)])
    with pytest.raises(ValueError):
        fused.pyramid_canvas_layout([], 1)
    with pytest.raises(ValueError):
        fused.pyramid_canvas_layout([(4, 0)], 1)


def _heads(engine, x):
    with torch.no_grad():
        cls, box = engine.heads(x)
        cls2, box2, cls_bias, box_bias = engine.heads_without_last_bias(x)
    return cls + box, cls2 + box2


@pytest.mark.parametrize('size', [(128, 128), (96, 160), (160, 64)], ids=lambda s: '%dx%d' % s)
def test_canvas_path_equals_per_level_path_fp32_cpu(size):
    """Same engine, canvas forced on against off.  The two paths sum the same products in orders the convolution picks per shape, so
    the bar is the one tests/test_gpu_fused_model.py::test_fold_conv_bn_is_exact_in_fp32_cpu sets for re-associated fp32 sums: 1e-5
    relative to each head tensor's largest magnitude."""
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=6).eval()
    model.initialize(None)
    with torch.no_grad():                                            # (initialize() leaves the towers near zero: give them weights)
        for head in (model.cls_head, model.box_head):
            for m in head:
                if isinstance(m, torch.nn.Conv2d):
                    m.weight.normal_(0, 0.05)
                    m.bias.normal_(0, 0.5)
    engine = fused.FusedRetinaNet(model, torch.float32)
    x = torch.randn(2, 3, *size, generator=torch.Generator().manual_seed(1))
    engine.pyramid_canvas = False
    off = _heads(engine, x)
    assert engine._canvas_gutter([x] * 5) is None
    engine.pyramid_canvas = True                                     # the default: CPU tensors keep the per-level path
    assert engine._canvas_gutter([torch.zeros(1, 8, 4, 4)] * 5) is None
    engine.pyramid_canvas = 'always'
    assert engine._canvas_gutter([torch.zeros(1, 8, 4, 4)] * 5) == 1
    on = _heads(engine, x)
    for got, ref in zip(on[0] + on[1], off[0] + off[1]):
        assert got.shape == ref.shape and got.dtype == ref.dtype
        assert got.is_contiguous(memory_format=torch.channels_last) or got.shape[2] * got.shape[3] == 1 or got.is_contiguous()
        scale = ref.abs().max().item()
        assert scale > 0
        assert (got - ref).abs().max().item() <= 1e-5 * scale, ((got - ref).abs().max().item(), scale)
    # P3 does not go through the canvas: the same calls, the same bits
    n = len(off[0]) // 2
    for k in (0, n):
        assert torch.equal(on[0][k], off[0][k]) and torch.equal(on[1][k], off[1][k])


def test_canvas_does_not_apply_to_other_towers():
    """The gutters stand in for "same" padding of stride-1 convolutions only: anything else keeps the per-level path."""
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=6).eval()
    model.initialize(None)
    engine = fused.FusedRetinaNet(model, torch.float32)
    engine.pyramid_canvas = 'always'
    feats = [torch.zeros(1, 256, s, s) for s in (16, 8, 4, 2, 1)]
    assert engine._canvas_gutter(feats) == 1
    assert engine._canvas_gutter(feats[:2]) is None                  # a single level below P3: nothing to pack
    engine.cls_head[1].stride = (2, 2)
    assert engine._canvas_gutter(feats) is None
    engine.cls_head[1].stride = (1, 1)
    engine.box_head[0].padding = (0, 0)
    assert engine._canvas_gutter(feats) is None
