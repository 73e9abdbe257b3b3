"""Task-aligned target assignment on the device (csrc/tal.hpp, odtk_tal_assign_levels) against the checker (tests/tal_ref.py)
under its comparison rule: depth, cls_target and the zero pattern of box_target exactly, the centre deltas bit for bit, the log
deltas within rtol = atol = 1e-6.  tests/test_tal.py::test_cases_are_not_vacuous checks, with the checker alone, that every case
exercises what it names.  16-bit heads are generated in their dtype and the checker sees the widened values.  Outputs are
allocated over NaN-filled memory, so an element a kernel does not write shows up."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import tal_ref
from odtk import _C, box
from odtk import main as cli
from odtk.model import Model

pytestmark = pytest.mark.gpu


def _dirty(c):
    """NaN into the blocks the caching allocator hands out next for this case's outputs."""
    b = c['targets'].shape[0]
    held = []
    for (h, w, _), anchors in zip(c['levels'], c['anchors']):
        a = anchors.shape[0]
        for channels in (c['classes'], 4, 1):
            held += [torch.full((b, a, channels, h, w), float('nan'), device='cuda') for _ in range(2)]
    del held


def _heads(c, dtype, channels_last):
    cls_heads, box_heads = tal_ref.heads_in(c, dtype)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    return [x.cuda().contiguous(memory_format=fmt) for x in cls_heads], [x.cuda().contiguous(memory_format=fmt) for x in box_heads]


def run(c, dtype='float32', channels_last=False, assign=box.tal_assign_levels, dirty=True):
    cls_heads, box_heads = _heads(c, dtype, channels_last)
    if dirty:
        _dirty(c)
    return assign(torch.from_numpy(c['targets']).cuda(), cls_heads, box_heads, [s for _, _, s in c['levels']],
                  [torch.from_numpy(a) for a in c['anchors']], c['classes'], c['topk'], c['alpha'], c['beta'], c['want_cls'])


@pytest.mark.parametrize('channels_last', [False, True], ids=['nchw', 'channels_last'])
@pytest.mark.parametrize('dtype', tal_ref.DTYPES)
@pytest.mark.parametrize('name', list(tal_ref.CASES))
def test_kernels_equal_the_checker(name, dtype, channels_last):
    c, ref = tal_ref.case(name, dtype)
    got = run(c, dtype, channels_last)
    assert all(t.is_cuda for t in got[1] + got[2])
    tal_ref.compare(got, ref, c['want_cls'], '%s %s' % (name, dtype))


@pytest.mark.parametrize('name', ['random_a9', 'non_finite', 'ties_a9', 'zero_metric', 'padding'])
def test_torch_branch_on_gpu_tensors_equals_the_kernels(name):
    """The pure-torch branch is device-agnostic: on the same GPU tensors it gives what the kernels give."""
    c, ref = tal_ref.case(name)
    got = run(c, assign=box._tal_assign_torch, dirty=False)
    assert all(t.is_cuda for t in got[1] + got[2])
    tal_ref.compare(got, ref, c['want_cls'], name)
    kernels = run(c)
    for mine, theirs in zip(got[2], kernels[2]):
        assert torch.equal(mine, theirs)


@pytest.mark.parametrize('dtype,channels_last', [('float32', False), ('bfloat16', True)])
def test_compiled_binding_equals_the_ctypes_binding(dtype, channels_last):
    from odtk import _C_ext
    c, ref = tal_ref.case('contested', dtype)
    cls_heads, box_heads = _heads(c, dtype, channels_last)
    got = _C_ext.tal_assign_levels(torch.from_numpy(c['targets']).cuda(), cls_heads, box_heads, [a.reshape(-1).tolist() for a in c['anchors']],
                                   c['classes'], [s for _, _, s in c['levels']], c['topk'], c['alpha'], c['beta'], True)
    tal_ref.compare(got, ref, True, 'compiled binding')
    none = _C_ext.tal_assign_levels(torch.from_numpy(c['targets']).cuda(), cls_heads, box_heads, [a.reshape(-1).tolist() for a in c['anchors']],
                                    c['classes'], [s for _, _, s in c['levels']], want_cls_target=False)
    tal_ref.compare(none, ref, False, 'compiled binding, no class map')


def test_repeatable_back_to_back_and_on_a_side_stream():
    c, ref = tal_ref.case('many_rows')
    first = run(c)
    second = run(c, dirty=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run(c, dirty=False)
    side.synchronize()
    torch.cuda.synchronize()
    tal_ref.compare(first, ref, c['want_cls'])
    for other in (second, third):
        for part, again in zip(first, other):
            for x, y in zip(part, again):
                assert np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))


def test_workspace_smaller_than_the_query_is_refused():
    lib = _C.library()
    c, _ = tal_ref.case('random_a1')
    targets = torch.from_numpy(c['targets']).cuda()
    b, n_max = targets.shape[:2]
    cls_heads, box_heads = _heads(c, 'float32', False)
    n = len(c['levels'])
    levels, heads = (_C.SnapLevel * n)(), (_C.LossLevel * n)()
    keep, outputs = [], []
    a = c['anchors'][0].shape[0]
    for lv, hd, (h, w, s), anchors, cls_head, box_head in zip(levels, heads, c['levels'], c['anchors'], cls_heads, box_heads):
        table = (ctypes.c_float * (4 * a))(*anchors.reshape(-1).tolist())
        keep.append(table)
        box_t, depth = torch.full((b, a, 4, h, w), 7.0, device='cuda'), torch.full((b, a, 1, h, w), 7.0, device='cuda')
        outputs += [box_t, depth]
        lv.anchors = ctypes.cast(table, ctypes.POINTER(ctypes.c_float))
        lv.box_target, lv.depth, lv.height, lv.width, lv.stride = box_t.data_ptr(), depth.data_ptr(), h, w, s
        hd.cls, hd.box, hd.channels_last = cls_head.data_ptr(), box_head.data_ptr(), 0
    args = (b, targets.data_ptr(), n_max, n, levels, heads, a, c['classes'], _C.F32, c['topk'], c['alpha'], c['beta'])
    need = lib.odtk_tal_assign_levels(*args, None, 0, None)
    assert need == (b * n_max * 144 + 255) // 256 * 256
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.odtk_tal_assign_levels(*args, ws.data_ptr(), need - 1, stream) == _C.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outputs)                                  # nothing was launched
    assert lib.odtk_tal_assign_levels(*args, ws.data_ptr(), need, stream) == _C.OK
    torch.cuda.synchronize()
    assert not any(bool((t == 7).any()) for t in outputs)


# ---------------------------------------------------------------------------------------------------------------- Model
@functools.lru_cache(maxsize=None)
def _model_and_batch():
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=3)
    model.initialize(None)
    model = model.cuda().train()
    g = torch.Generator().manual_seed(11)
    images = torch.randn(2, 3, 64, 96, generator=g).cuda()
    targets = torch.tensor([[[8.0, 8.0, 32.0, 32.0, 0.0], [40.0, 16.0, 45.0, 23.0, 2.0], [20.0, 20.0, 40.0, 40.0, 1.0]],
                            [[50.0, 4.0, 32.0, 32.0, 1.0], [4.0, 10.0, 23.0, 45.0, 0.0], [30.0, 14.0, 40.0, 40.0, 2.0]]]).cuda()
    return model, images, targets


def _configure(model, cls_loss='focal', box_loss='smooth_l1', assigner='iou', fused=True):
    model.cls_loss, model.box_loss, model.box_loss_weight, model.assigner, model.fused_loss = cls_loss, box_loss, 1.0, assigner, fused


def _step(model, images, targets):
    model.zero_grad(set_to_none=True)
    cls_loss, box_loss = model((images, targets))
    (cls_loss + box_loss).backward()
    return (cls_loss.detach().clone(), box_loss.detach().clone(), model.cls_head[-1].weight.grad.detach().clone(),
            model.box_head[-1].weight.grad.detach().clone())


@pytest.mark.parametrize('cls_loss,box_loss', [('qfl', 'giou'), ('vfl', 'giou'), ('focal', 'smooth_l1')])
def test_model_fused_and_eager_paths_agree(cls_loss, box_loss):
    """A training step with assigner = 'tal': the assignment is identical on both paths, so only the loss arithmetic differs -- to
    the tolerances of tests/test_gpu_quality_loss.py::test_model_fused_and_eager_paths_agree (1e-5 of the losses, 1e-4 of the
    largest head weight gradient)."""
    model, images, targets = _model_and_batch()
    try:
        _configure(model, cls_loss, box_loss, 'tal', True)
        fused = _step(model, images, targets)
        _configure(model, cls_loss, box_loss, 'tal', False)
        eager = _step(model, images, targets)
        _configure(model, cls_loss, box_loss, 'atss', True)
        atss = _step(model, images, targets)
    finally:
        _configure(model)
    for k in range(2):
        print(cls_loss, box_loss, 'loss', k, float(fused[k]), float(eager[k]))
        assert abs(float(fused[k]) - float(eager[k])) <= 1e-5 * abs(float(eager[k])) and float(eager[k]) > 0
    for k in (2, 3):
        scale = float(eager[k].abs().max())
        worst = float((fused[k] - eager[k]).abs().max())
        print(cls_loss, box_loss, 'head weight gradient %d: worst %.3g of %.3g' % (k, worst, scale))
        assert scale > 0 and worst <= 1e-4 * scale
    assert not torch.equal(fused[0], atss[0])                                           # and it is not ATSS's assignment


def test_train_through_the_command_line(tmp_path, capsys, monkeypatch):
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data')
    calls = []
    real = box.tal_assign_levels

    def spy(*args, **kwargs):
        calls.append(tuple(args[6:9]) + (all(not t.requires_grad for t in list(args[1]) + list(args[2])),))
        return real(*args, **kwargs)
    monkeypatch.setattr(box, 'tal_assign_levels', spy)
    path = str(tmp_path / 'tiny.pth')
    done, _ = cli.main(['train', path, '--iters', '2', '--annotations', os.path.join(data, 'annotations.json'), '--images', data,
                        '--backbone', 'ResNet18FPN', '--classes', '3', '--batch', '2', '--resize', '128', '--max-size', '160',
                        '--jitter', '96', '128', '--warmup', '2', '--lr', '0.001', '--workers', '0', '--assigner', 'tal',
                        '--tal-topk', '7', '--tal-beta', '4', '--cls-loss', 'vfl', '--box-loss', 'giou'])
    out = capsys.readouterr().out
    assert done == 2 and '[2/2] focal loss:' in out
    assert calls == [(7, 1, 4, True), (7, 1, 4, True)]
    assert not any('tal' in k or 'assigner' in k for k in torch.load(path, map_location='cpu'))
