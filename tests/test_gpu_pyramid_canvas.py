"""The pyramid canvas on the GPU (odtk/fused.py: _canvas_towers; include/odtk_conv_strided.h: odtk_conv_bias_act_strided;
include/odtk_hip.h: odtk_canvas_clear / odtk_canvas_pack): the convolution library on views of larger buffers, the two canvas
kernels against torch, and the engine with the canvas on against the per-level path."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]

pytestmark = pytest.mark.gpu


def _tower_layer(dtype, k=256, c=256, seed=11):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(k, c, 3, 3, generator=g) * (2.0 / (c * 9)) ** 0.5).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
    b = (torch.randn(k, generator=g) * 0.3).to(dtype).cuda()
    return w, b, g


def _forced_instance(monkeypatch, x, w, b, relu):
    """Runs the packed entry once as planned, then pins the instance it ran for every later call (ODTK_CONV_INSTANCE)."""
    from odtk import _C
    _C.conv_bias_act(x, w, b, 1, 1, relu)
    index = int(_C.conv_last_plan().split()[0].lstrip('#'))
    monkeypatch.setenv('ODTK_CONV_INSTANCE', str(index))
    return index


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('k', [256, 72, 36], ids=['256to256', '256to72', '256to36'])
def test_strided_entry_equals_the_packed_entry_bit_for_bit(monkeypatch, dtype, k):
    """x: a rectangle of a larger channels_last buffer (a level of the canvas).  y: a view of a larger buffer as far as the prebuilt
    instances honour one -- a channel slice, i.e. a wider PIXEL stride.  Same instance forced on both sides: the same bits, and
    every byte of the output buffer outside the view is left alone."""
    from odtk import _C
    assert _C.conv_available()
    w, b, g = _tower_layer(dtype, k=k)
    big = torch.randn(2, 256, 50, 121, generator=g).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
    y0, x0, h, wd = 26, 81, 13, 20
    view = big[:, :, y0:y0 + h, x0:x0 + wd]
    assert not view.is_contiguous(memory_format=torch.channels_last)
    packed = view.contiguous(memory_format=torch.channels_last)
    _forced_instance(monkeypatch, packed, w, b, True)
    ref = _C.conv_bias_act(packed, w, b, 1, 1, True)
    plan_ref = _C.conv_last_plan().split()[0]
    got = _C.conv_bias_act(view, w, b, 1, 1, True)                              # strided x, packed y
    assert _C.conv_last_plan().split()[0] == plan_ref
    assert torch.equal(got, ref)
    # strided x AND strided y: channels [8, 8 + k) of a wider buffer (a multiple of 8 channels), filled with a sentinel first
    total = (k + 8 + 7) // 8 * 8 + 8
    wide = torch.full((2, total, h, wd), 7.0, dtype=dtype, device='cuda').contiguous(memory_format=torch.channels_last)
    out = wide[:, 8:8 + k]
    assert out.stride(1) == 1 and out.stride(3) == total
    _C.conv_bias_act(view, w, b, 1, 1, True, out=out)
    torch.cuda.synchronize()
    assert _C.conv_last_plan().split()[0] == plan_ref
    assert torch.equal(out, ref)
    assert bool((wide[:, :8] == 7.0).all()) and bool((wide[:, 8 + k:] == 7.0).all())    # bytes outside the view: untouched
    assert torch.equal(big[:, :, y0:y0 + h, x0:x0 + wd], packed)                          # and the input buffer is only read


def test_an_output_rectangle_is_refused_never_miswritten(monkeypatch):
    """The prebuilt instances address their output as ONE run of batch * out_h * out_w pixels at the pixel stride (composable_kernel's
    transform_conv_fwd_to_gemm.hpp, MakeCDescriptor_M_N: row and image strides of the output are not carried), and
    IsSupportedArgument does not look at them.  A rectangle of a wider buffer as OUTPUT therefore cannot be bit-equal to the packed
    entry with these instances; the entry refuses it (ODTK_ERR_UNSUPPORTED) before anything is launched and the buffer keeps every
    byte -- the engine packs the canvas with odtk_canvas_pack instead of convolving into it."""
    from odtk import _C
    w, b, g = _tower_layer(torch.bfloat16)
    x = torch.randn(2, 256, 13, 20, generator=g).bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    big = torch.full((2, 256, 50, 121), 3.0, dtype=torch.bfloat16, device='cuda').contiguous(memory_format=torch.channels_last)
    before = big.clone()
    with pytest.raises(RuntimeError, match='unsupported'):
        _C.conv_bias_act(x, w, b, 1, 1, True, out=big[:, :, 26:39, 81:101])
    torch.cuda.synchronize()
    assert torch.equal(big, before)
    # misaligned views are invalid, not unsupported: a pixel stride that is no multiple of 8 elements
    odd = torch.zeros(2, 260, 13, 20, dtype=torch.bfloat16, device='cuda').contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match='invalid'):
        _C.conv_bias_act(odd[:, 2:258], w, b, 1, 1, True)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32, torch.float16], ids=['bf16', 'fp32', 'fp16'])
def test_canvas_clear_and_pack_match_torch(dtype):
    from odtk import _C, fused
    g = torch.Generator().manual_seed(2)
    for shapes, channels, gutter in [([(50, 80), (25, 40), (13, 20), (7, 10)], 256, 1), ([(8, 8), (4, 4), (2, 2), (1, 1)], 64, 1),
                                     ([(5, 7), (3, 4), (2, 2)], 8, 2)]:
        (height, width), origins = fused.pyramid_canvas_layout(shapes, gutter)
        rects = [(y, x, h, w) for (y, x), (h, w) in zip(origins, shapes)]
        inside = torch.zeros(1, 1, height, width, dtype=torch.bool, device='cuda')
        for y, x, h, w in rects:
            inside[:, :, y:y + h, x:x + w] = True
        canvas = torch.randn(3, channels, height, width, generator=g).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
        ref = torch.where(inside, canvas, torch.zeros_like(canvas))
        got = _C.canvas_clear_(canvas, rects)
        assert got is canvas and torch.equal(canvas, ref)
        levels = [torch.randn(3, channels, h, w, generator=g).to(dtype).cuda().contiguous(memory_format=torch.channels_last) for h, w in shapes]
        packed = _C.canvas_pack(levels, rects, height, width)
        ref = torch.zeros_like(packed)
        for t, (y, x, h, w) in zip(levels, rects):
            ref[:, :, y:y + h, x:x + w] = t
        assert packed.is_contiguous(memory_format=torch.channels_last) and torch.equal(packed, ref)
    with pytest.raises(RuntimeError):
        _C.canvas_clear_(canvas, [(0, 0, height + 1, 1)])                      # a rectangle outside the canvas
    assert torch.equal(_C.canvas_clear_(canvas.clone(memory_format=torch.preserve_format), []), torch.zeros_like(canvas))


def _model(backbone, classes, seed=0):
    from odtk.model import Model
    torch.manual_seed(seed)
    model = Model(backbone, classes=classes).cuda().eval()
    model.initialize(None)
    return model


@pytest.mark.parametrize('backbone,size', [('ResNet18FPN', (256, 320)), ('ResNet50FPN', (256, 384))], ids=['rn18', 'rn50'])
def test_engine_with_the_canvas_against_the_per_level_path(backbone, size):
    """bf16 engines, one plan, canvas on against off.  P3 does not go through the canvas: bit-equal.  The other levels run the same
    convolutions on another geometry (another instance, another summation order): within the bound tests/test_gpu_conv_library.py
    sets between convolution routes.  The detections keep their shapes."""
    from odtk import fused
    model = _model(backbone, 20)
    x = torch.randn(2, 3, *size, device='cuda')
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True                                   # (the layers left on MIOpen must reproduce themselves)
    try:
        engine = fused.FusedRetinaNet(model, torch.bfloat16)
        assert engine.pyramid_canvas is True
        with torch.no_grad():
            engine.plan(x)
            on_c, on_b = engine.heads(x)
            det_on = engine(x)
            engine.pyramid_canvas = False
            off_c, off_b = engine.heads(x)
            det_off = engine(x)
            engine.pyramid_canvas = True
            engine.level_streams = False                                        # one stream: the same bits as beside P3
            seq_c, seq_b = engine.heads(x)
    finally:
        torch.backends.cudnn.deterministic = saved
    assert any(len(k) == 4 and k[2:] not in [tuple(t.shape[2:]) for t in off_c] for k in engine.cls_head[0].route), 'no canvas shape was routed'
    for level, (got, ref) in enumerate(zip(on_c + on_b, off_c + off_b)):
        assert got.shape == ref.shape and got.dtype == ref.dtype and got.is_contiguous(memory_format=torch.channels_last) == \
            ref.is_contiguous(memory_format=torch.channels_last)
        if level % len(on_c) == 0:
            assert torch.equal(got, ref), 'P3 changed'
        else:
            scale = float(ref.float().abs().max())
            err = float((got.float() - ref.float()).abs().max())
            print('level %d: max |diff| %.4g, scale %.4g' % (level % len(on_c) + 3, err, scale))
            assert err <= 0.03 * scale + 1e-3, (level, err, scale)
    for got, ref in zip(seq_c + seq_b, on_c + on_b):
        assert torch.equal(got, ref)
    for a, b in zip(det_on, det_off):
        assert a.shape == b.shape and a.dtype == b.dtype


def test_graph_replay_with_the_canvas_returns_what_the_eager_call_returns():
    from odtk import fused
    model = _model('ResNet18FPN', 6)
    x = torch.randn(2, 3, 256, 320, device='cuda')
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        engine = fused.FusedRetinaNet(model, torch.bfloat16)
        assert engine._canvas_gutter([torch.zeros(2, 256, s, s, device='cuda', dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
                                      for s in (32, 16, 8, 4, 2)]) == 1
        with torch.no_grad():
            eager = engine(x)
            first = engine.replay(x)
            x2 = torch.randn(2, 3, 256, 320, device='cuda')
            second = engine.replay(x2)                                          # the graph's canvases are its own: another input, replayed
            eager2 = engine(x2)
            again = engine.replay(x)
    finally:
        torch.backends.cudnn.deterministic = saved
    for a, b in zip(eager, first):
        assert torch.equal(a, b)
    for a, b in zip(eager2, second):
        assert torch.equal(a, b)
    for a, b in zip(eager, again):
        assert torch.equal(a, b)


_CHILD = r'''
import hashlib, json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, 'retinanet-examples_amd'))
import torch
from odtk import fused
from odtk.model import Model
torch.backends.cudnn.deterministic = True   # the layers the plan leaves on MIOpen must reproduce themselves (tests/test_conv_plan.py)
torch.manual_seed(0)
model = Model('ResNet50FPN', classes=80).eval()
model.initialize(None)
model = model.cuda().to(memory_format=torch.channels_last)
e = fused.FusedRetinaNet(model, torch.bfloat16)
taken = e.load_plan(json.load(open(%(plan)r)))
x = torch.randn(8, 3, 800, 1280, generator=torch.Generator().manual_seed(3)).cuda().contiguous(memory_format=torch.channels_last)
with torch.no_grad():
    e.plan(x)
    cls, box = e.heads(x)
h = hashlib.sha256()
for t in cls + box:
    h.update(t.float().cpu().numpy().tobytes())
canvas = sorted(k for k in e.cls_head[0].route)
print(json.dumps({'digest': h.hexdigest(), 'plan_hash': e.plan_hash(), 'taken': list(taken), 'canvas': bool(e.pyramid_canvas),
                  'measured': sum(1 for m in e.modules() if isinstance(m, fused._Conv) for v in m.route.values() if v[1] is not None)}))
'''


def test_committed_plan_gives_the_same_head_tensors_in_two_processes():
    """The committed plan names no canvas problem: the engine follows the layers' recorded decisions and the convolution library
    adopts the planned sibling's instance (50 x 80 for the 50 x 121 canvas) -- no stopwatch, so two fresh processes agree bit for bit."""
    from odtk import _C
    assert _C.conv_available()
    plan = os.path.join(ROOT, 'plans', 'rn50fpn_bf16_bs8_800x1280.json')
    outs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT, 'plan': plan}], capture_output=True, text=True, timeout=900,
                           env={k: v for k, v in os.environ.items() if k not in ('ODTK_PYRAMID_CANVAS', 'ODTK_CONV_PLAN', 'ODTK_CONV_ROUTE')})
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    first, second = outs
    assert first['canvas'] and first['measured'] == 0 and second['measured'] == 0
    assert first['taken'] == second['taken'] and first['taken'][1] > 0
    assert first['plan_hash'] == second['plan_hash']
    assert first['digest'] == second['digest']
