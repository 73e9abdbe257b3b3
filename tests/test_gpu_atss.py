"""ATSS target assignment on the device (csrc/atss.hpp, odtk_atss_assign_levels) against the checker (tests/atss_ref.py) under the
comparison rule of tests/test_atss.py: depth, cls_target and the zero pattern of box_target exactly, the centre deltas bit for
bit, the log deltas within rtol = atol = 1e-6.  tests/test_atss.py::test_cases_are_not_vacuous checks, with the checker alone,
that the cases contain conflicts, centre rejections, boxes without positives and every staging round.
Outputs are allocated over NaN-filled memory, so an element a kernel does not write shows up."""
import ctypes
import os

import numpy as np
import pytest
import torch

import atss_ref
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


def run(c, assign=box.atss_assign_levels, dirty=True):
    if dirty:
        _dirty(c)
    return assign(torch.from_numpy(c['targets']).cuda(), [(h, w) for h, w, _ in c['levels']], [s for _, _, s in c['levels']],
                  [torch.from_numpy(a) for a in c['anchors']], c['classes'], c['topk'], c['want_cls'])


@pytest.mark.parametrize('name', list(atss_ref.CASES))
def test_kernels_equal_the_checker(name):
    c, ref = atss_ref.case(name)
    got = run(c)
    assert all(t.is_cuda for t in got[1] + got[2])
    atss_ref.compare(got, ref, c['want_cls'], name)


@pytest.mark.parametrize('name', ['default_k9', 'nan_coordinate', 'few_cells'])
def test_torch_branch_on_gpu_tensors_equals_the_kernels(name):
    """The pure-torch branch is device-agnostic: on the same GPU tensors it gives what the kernels give."""
    c, ref = atss_ref.case(name)
    got = run(c, assign=box._atss_assign_torch, dirty=False)
    assert all(t.is_cuda for t in got[1] + got[2])
    atss_ref.compare(got, ref, c['want_cls'], name)
    kernels = run(c)
    for mine, theirs in zip(got[2], kernels[2]):
        assert torch.equal(mine, theirs)


def test_repeatable_back_to_back_and_on_a_side_stream():
    c, ref = atss_ref.case('crowd')
    first = run(c)
    second = run(c, dirty=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run(c, dirty=False)
    side.synchronize()
    torch.cuda.synchronize()
    atss_ref.compare(first, ref, c['want_cls'])
    for other in (second, third):
        for part, again in zip(first, other):
            for x, y in zip(part, again):
                assert np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))


def test_workspace_smaller_than_the_query_is_refused():
    lib = _C.library()
    c, _ = atss_ref.case('single_level')
    targets = torch.from_numpy(c['targets']).cuda()
    b, n_max = targets.shape[:2]
    (h, w, s), anchors = c['levels'][0], c['anchors'][0]
    a = anchors.shape[0]
    table = (ctypes.c_float * (4 * a))(*anchors.reshape(-1).tolist())
    box_t, depth = torch.full((b, a, 4, h, w), 7.0, device='cuda'), torch.full((b, a, 1, h, w), 7.0, device='cuda')
    level = (_C.SnapLevel * 1)()
    level[0].anchors = ctypes.cast(table, ctypes.POINTER(ctypes.c_float))
    level[0].box_target, level[0].depth, level[0].height, level[0].width, level[0].stride = box_t.data_ptr(), depth.data_ptr(), h, w, s
    args = (b, targets.data_ptr(), n_max, 1, level, a, c['classes'], c['topk'])
    need = lib.odtk_atss_assign_levels(*args, None, 0, None)
    assert need == (b * n_max * 96 + 255) // 256 * 256
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.odtk_atss_assign_levels(*args, ws.data_ptr(), need - 1, stream) == _C.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((box_t == 7).all()) and bool((depth == 7).all())                       # nothing was launched
    assert lib.odtk_atss_assign_levels(*args, ws.data_ptr(), need, stream) == _C.OK
    torch.cuda.synchronize()
    assert not bool((depth == 7).any()) and not bool((box_t == 7).any())


def _step(model, data, target):
    model.zero_grad(set_to_none=True)
    cls_loss, box_loss = model([data, target])
    (cls_loss + box_loss).backward()
    return float(cls_loss.detach()), float(box_loss.detach()), [p.grad for p in model.parameters() if p.grad is not None]


def test_model_training_step():
    """ResNet18FPN, 2 x 3 x 128 x 128: with ATSS the fused loss equals the unfused one within the tolerance
    tests/test_gpu_loss.py::test_model_training_step_fused_loss_equals_torch_loss uses for that comparison (2e-6 relative), the
    gradients are finite; with the IoU rule the losses are bit-equal to a model whose attribute was never touched."""
    from odtk import train as T
    data, target = T.SyntheticBatches(2, 128, 128, classes=6, max_boxes=6, seed=5, device='cuda').batch()

    def fresh():
        torch.manual_seed(0)
        m = Model('ResNet18FPN', classes=6)
        m.initialize(None)
        return m.cuda().train()
    flags = (torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic)
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    try:
        untouched = _step(fresh(), data, target)
        m = fresh()
        m.assigner = 'atss'
        fused = _step(m, data, target)
        m.fused_loss = False
        unfused = _step(m, data, target)
        m.fused_loss = True
        m.assigner = 'iou'
        back = _step(m, data, target)
    finally:
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = flags
    print('atss fused', fused[:2], 'unfused', unfused[:2], 'iou', untouched[:2])
    assert abs(fused[0] - unfused[0]) <= 2e-6 * abs(unfused[0]) and abs(fused[1] - unfused[1]) <= 2e-6 * abs(unfused[1]), (fused[:2], unfused[:2])
    assert fused[2] and all(bool(torch.isfinite(g).all()) for g in fused[2] + unfused[2])
    assert fused[1] > 0 and fused[:2] != untouched[:2]                                 # ATSS found positives, and they are not the IoU rule's
    assert back[:2] == untouched[:2]


def test_train_through_the_command_line(tmp_path, capsys, monkeypatch):
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data')
    calls = []
    real = box.atss_assign_levels

    def spy(*args, **kwargs):
        calls.append(args[5])
        return real(*args, **kwargs)
    monkeypatch.setattr(box, 'atss_assign_levels', spy)
    path = str(tmp_path / 'tiny.pth')
    done, _ = cli.main(['train', path, '--iters', '2', '--annotations', os.path.join(data, 'annotations.json'), '--images', data,
                        '--backbone', 'ResNet18FPN', '--classes', '3', '--batch', '2', '--resize', '128', '--max-size', '160',
                        '--jitter', '96', '128', '--warmup', '2', '--lr', '0.001', '--workers', '0', '--assigner', 'atss',
                        '--atss-topk', '7'])
    out = capsys.readouterr().out
    assert done == 2 and '[2/2] focal loss:' in out
    assert calls == [7, 7]
    assert not any('atss' in k or 'assigner' in k for k in torch.load(path, map_location='cpu'))
