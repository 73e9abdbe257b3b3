"""The engine's fourth convolution route (odtk/fused.py: `_Conv._tower_takes`): the head towers' 3x3 256 -> 256 layers through the
library's own kernel (`odtk_tower_conv3x3`), switched by `FusedRetinaNet.tower_conv` / ODTK_TOWER_CONV."""
import os
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]

gpu = pytest.mark.gpu


def _model(backbone):
    from odtk.model import Model
    torch.manual_seed(0)
    model = Model(backbone, classes=8)
    model.initialize(None)
    for m in model.modules():                       # non-trivial frozen statistics
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.8, 1.2); m.bias.data.normal_(0, 0.1)
    model = model.cuda().to(memory_format=torch.channels_last).eval()
    with torch.no_grad():
        model.cls_head[-1].weight.mul_(60.0)        # detections exist
    return model


def _tower_launches(fn):
    from odtk import _C
    _C.profile_collect()
    _C.profile_enable(True, ['tower_conv3x3_kernel'])
    try:
        result = fn()
        torch.cuda.synchronize()
        counts = _C.profile_collect()
    finally:
        _C.profile_enable(False)
    return result, counts['tower_conv3x3_kernel'][1]


def test_eligibility_is_decided_per_layer_and_the_switch_reaches_every_layer(monkeypatch):
    """No GPU: which layers the own kernel may take (3x3, stride 1, padding 1, 256 -> 256, 16-bit), the pixel threshold, the
    engine's switch."""
    from odtk import fused
    from odtk.model import Model
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=8)
    model.initialize(None)
    engine = fused.FusedRetinaNet(model.eval(), torch.bfloat16)
    ok = sorted(n for n, m in engine.named_modules() if isinstance(m, fused._Conv) and m.tower_ok)
    # the towers' four hidden layers of both heads and the three smoothing convolutions; not the heads' last layers (72 / 36
    # outputs), not pyramid6 / pyramid7 (stride 2), nothing of the backbone (ResNet18: 64 .. 512 channels, 256 only with stride 2 or ...)
    expected = ['box_head.%d' % i for i in range(4)] + ['cls_head.%d' % i for i in range(4)] + ['smooth.%d' % i for i in range(3)]
    assert [n for n in ok if not n.startswith('layers.')] == sorted(expected)
    for n in ok:
        if n.startswith('layers.'):
            m = dict(engine.named_modules())[n]
            assert tuple(m.weight.shape) == (256, 256, 3, 3) and tuple(m.stride) == (1, 1)
    assert not fused.FusedRetinaNet(model, torch.float32).cls_head[0].tower_ok
    conv = engine.cls_head[0]
    x = torch.zeros(1, 256, 4, 4, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert not conv._tower_takes(x)                                          # a CPU tensor never does
    assert engine.tower_conv == (os.environ.get('ODTK_TOWER_CONV', '1') != '0')
    engine.tower_conv = False
    assert not any(m.tower_conv for m in engine.modules() if isinstance(m, fused._Conv))
    engine.tower_conv = True
    assert all(m.tower_conv for m in engine.modules() if isinstance(m, fused._Conv))
    assert fused._Conv.tower_min_pixels == 100000
    big = torch.zeros(8, 256, 100, 160, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert 8 * 100 * 160 >= fused._Conv.tower_min_pixels > 8 * 50 * 121 and not conv._tower_takes(big)      # (P3 yes, the canvas no; CPU: never)


def _head_error(heads, eager):
    """Largest |head - fp32 eager head| over every level of both heads, relative to that tensor's largest magnitude."""
    worst = 0.0
    for got, ref in zip(heads[0] + heads[1], eager[0] + eager[1]):
        scale = float(ref.abs().max()) + 1e-6
        worst = max(worst, float((got.float() - ref).abs().max()) / scale)
    return worst


@gpu
def test_engine_route_lies_inside_the_envelope_of_the_library_instances(monkeypatch):
    """ResNet18FPN (the heads are 256 wide on every backbone), 64 x 64, batch 2, bf16; the pixel threshold lowered to 0 so that P3
    (8 x 8) and the canvas of the levels below it run through the own kernel.  The towers are compared on ONE set of pyramid
    features (computed once by the engine) against the fp32 eager heads on those features, so that the figures are the towers' own:

      * own kernel (switch on): 16 launches of tower_conv3x3_kernel per pass (4 hidden layers x 2 heads x {P3, canvas});
      * switch off: no launch of it, the library's instance as the stopwatch / plan picks it -- the parent's graph;
      * switch off and three other instances that accept the tower problem forced in turn (ODTK_CONV_INSTANCE).

    The own route's worst error must not exceed the worst of the library runs: the envelope is measured, no tolerance is set by
    hand.  Measured on MI355X (relative to each head tensor's largest magnitude; printed with -s; profiles/tower_conv_probe.txt):
    own 0.00652885, library as planned 0.00652885, instances #0, #1, #2 forced 0.00652885 each -- the worst element is the same
    in all five runs: the routes differ at most in the order of the fp32 sums (the kernel's default form sums as the library's
    256 x 256 x 32 instance does; its 16x16x32 form, measured earlier, gave 0.00719441 in all five runs of that session)."""
    from odtk import _C, fused
    monkeypatch.setattr(fused._Conv, 'tower_min_pixels', 0)
    monkeypatch.setattr(fused._Conv, 'route_mode', 'library')              # no stopwatch: every k x k layer the library takes is routed to it
    model = _model('ResNet18FPN')
    engine = fused.FusedRetinaNet(model, dtype=torch.bfloat16)
    assert engine.tower_conv
    x = torch.randn(2, 3, 64, 64, device='cuda')
    with torch.no_grad():
        engine.forward(x)                                                    # plan pass, library warm-up
        feats = [f.clone() for f in engine.features(x)]
        assert tuple(feats[0].shape) == (2, 256, 8, 8)
        eager = ([model.cls_head(f.float()) for f in feats], [model.box_head(f.float()) for f in feats])

        def towers():
            with torch.autocast('cuda', enabled=False):
                cls, box = engine._towers(feats, True)
            return [t.clone() for t in cls], [t.clone() for t in box]

        own, n_own = _tower_launches(towers)
        assert n_own == 16, n_own
        engine.tower_conv = False
        off, n_off = _tower_launches(towers)
        assert n_off == 0
        again, _ = _tower_launches(towers)
        assert all(torch.equal(a, b) for a, b in zip(off[0] + off[1], again[0] + again[1]))
        errors = {'own': _head_error(own, eager), 'library (as planned)': _head_error(off, eager)}
        # three other instances that take the towers' problem at P3's shape
        layer = engine.cls_head[0]
        _C.conv_bias_act(feats[0], layer.weight, layer.bias_lp, 1, 1, True)
        planned = int(_C.conv_last_plan().split()[0].lstrip('#'))
        total = _C.conv_library().odtk_conv_instance_count(_C.BF16)
        forced = []
        for index in range(total):
            if index == planned:
                continue
            monkeypatch.setenv('ODTK_CONV_INSTANCE', str(index))
            try:
                _C.conv_bias_act(feats[0], layer.weight, layer.bias_lp, 1, 1, True)
            except RuntimeError as e:
                assert 'unsupported' in str(e).lower(), e
                continue
            assert _C.conv_last_plan().startswith('#%d ' % index), (index, _C.conv_last_plan())   # the forced instance ran P3's problem
            forced.append(index)
            errors['library #%d' % index] = _head_error(towers(), eager)
            if len(forced) == 3:
                break
        monkeypatch.delenv('ODTK_CONV_INSTANCE')
        assert len(forced) == 3, forced
        engine.tower_conv = True
    for name, err in errors.items():
        print('[tower-conv] engine envelope: %-22s worst head error %.6g' % (name, err))
    envelope = max(v for k, v in errors.items() if k != 'own')
    assert errors['own'] <= envelope, errors


@gpu
def test_engine_switch_is_part_of_the_graph_key(monkeypatch):
    """Launch counts with the switch on and off, a graph replay equals the eager call on both sides, and the switch makes a new
    graph.  How far the detections move between the two sides is printed, not bounded (the envelope test above is the bound)."""
    from odtk import fused
    monkeypatch.setattr(fused._Conv, 'tower_min_pixels', 0)
    monkeypatch.setattr(fused._Conv, 'route_mode', 'library')              # no stopwatch: every k x k layer the library takes is routed to it
    engine = fused.FusedRetinaNet(_model('ResNet18FPN'), dtype=torch.bfloat16)
    x = torch.randn(2, 3, 64, 64, device='cuda')
    with torch.no_grad():
        engine.forward(x)
        on, n_on = _tower_launches(lambda: [t.clone() for t in engine.forward(x)])
        engine.tower_conv = False
        off, n_off = _tower_launches(lambda: [t.clone() for t in engine.forward(x)])
        engine.tower_conv = True
        # the towers' 16, the three smoothing convolutions and layer3's one 256 -> 256 convolution without a skip (block 1's first)
        assert n_on == 20 and n_off == 0, (n_on, n_off)
        assert int((on[0] > 0).sum()) > 20
        print('[tower-conv] engine: scores differing %d of %d (max %.3g), classes differing %d' % (
            int((on[0] != off[0]).sum()), on[0].numel(), float((on[0] - off[0]).abs().max()), int((on[2] != off[2]).sum())))
        replayed = engine.replay(x)
        assert all(torch.equal(a, b) for a, b in zip(on, replayed))
        n_graphs = len(engine._graphs)
        engine.tower_conv = False
        assert all(torch.equal(a, b) for a, b in zip(off, engine.replay(x))) and len(engine._graphs) == n_graphs + 1
