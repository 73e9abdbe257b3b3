"""ATSS target assignment off the GPU: odtk.box.atss_assign_levels on CPU tensors (its pure-torch branch) against the checker
(tests/atss_ref.py) on every case the device test runs, what the cases are meant to contain, the C ABI's refusals, the command
line, and Model's plumbing -- the option is a run-time attribute that never reaches a checkpoint.

The statistics kernel finds a box's candidates in a window of 8 x 8 cells where a run-time test allows it (csrc/atss.hpp:
atss_window); the host form of that rule (tests/atss_ref.py:window_scan) is held to the full scan by brute force here."""
import ctypes

import numpy as np
import pytest
import torch

import atss_ref
from odtk import _C, box
from odtk import main as cli
from odtk.model import Model

RANDOM = [name for name in atss_ref.CASES if atss_ref.CASES[name]().get('random')]


def run(c, device='cpu', assign=box.atss_assign_levels):
    return assign(torch.from_numpy(c['targets']).to(device), [(h, w) for h, w, _ in c['levels']], [s for _, _, s in c['levels']],
                  [torch.from_numpy(a) for a in c['anchors']], c['classes'], c['topk'], c['want_cls'])


@pytest.mark.parametrize('name', list(atss_ref.CASES))
def test_torch_branch_equals_the_checker(name):
    c, ref = atss_ref.case(name)
    got = run(c)
    for l, (h, w, _) in enumerate(c['levels']):
        b, a = c['targets'].shape[0], c['anchors'][l].shape[0]
        assert tuple(got[1][l].shape) == (b, a, 4, h, w) and tuple(got[2][l].shape) == (b, a, 1, h, w)
    atss_ref.compare(got, ref, c['want_cls'], name)


def test_cases_are_not_vacuous():
    """With the checker alone: a kernel that assigns nothing, never meets a conflict or never applies the centre test cannot pass."""
    facts = {name: atss_ref.case(name)[1] for name in atss_ref.CASES}
    assert any(f['contested'] > 0 for f in facts.values())
    assert any(f['centre_rejected'] > 0 for f in facts.values())
    assert any(f['boxes_without_positives'] > 0 for f in facts.values())
    assert len(RANDOM) >= 5
    for name in RANDOM:
        assert sum(n > 0 for n in facts[name]['assigned_per_level']) >= 3, (name, facts[name]['assigned_per_level'])
    for name in ('n_max_0', 'all_padding'):
        assert facts[name]['assigned'] == 0 and facts[name]['boxes'] == 0
    for name in ('corners', 'centre_outside', 'three_pixels', 'whole_image', 'zero_width', 'nan_coordinate', 'near_1e4', 'few_cells',
                 'one_anchor', 'max_anchors', 'single_level', 'three_rounds'):
        assert facts[name]['assigned'] > 0, name
    assert atss_ref.case('max_anchors')[0]['anchors'][0].shape[0] == atss_ref.MAX_ANCHORS == _C.MAX_ANCHORS
    assert len(atss_ref.case('six_levels')[0]['levels']) == atss_ref.MAX_LEVELS == _C.MAX_LEVELS
    assert atss_ref.MAX_TOPK == _C.ATSS_MAX_TOPK
    # the staging rounds of the dense launch: one row short of a round, a full one, one more, and more than two rounds of rows
    assert [atss_ref.case(n)[0]['targets'].shape[1] for n in ('round_minus_1', 'round_exact', 'round_plus_1')] == [
        atss_ref.ROUND - 1, atss_ref.ROUND, atss_ref.ROUND + 1]
    assert atss_ref.case('three_rounds')[0]['targets'].shape[1] > 2 * atss_ref.ROUND
    assert facts['round_exact']['boxes'] == atss_ref.ROUND
    # on the largest level of the default pyramid the statistics kernel's window rule admits some boxes and refuses others
    took = []
    for name in ('default_k9', 'centre_outside'):
        c, _ = atss_ref.case(name)
        rows = c['targets'][0][c['targets'][0][:, 4] > -1]
        x2, y2 = rows[:, 0] + rows[:, 2] - np.float32(1), rows[:, 1] + rows[:, 3] - np.float32(1)
        bcx = rows[:, 0] + np.float32(0.5) * (x2 - rows[:, 0] + np.float32(1))
        bcy = rows[:, 1] + np.float32(0.5) * (y2 - rows[:, 1] + np.float32(1))
        h, w, s = c['levels'][0]
        assert h * w > 64
        _, d2, sound, bound = atss_ref.window_scan(bcx, bcy, h, w, s)
        took += list(sound & (d2[:, c['topk'] - 1] < bound))
    assert any(took) and not all(took)
    # identical boxes: the earlier row wins every anchor both claim (classes 1 and 3 -> depth 2, never 4)
    c, ref = atss_ref.case('identical_boxes')
    assert ref['contested'] > 0
    assert all(not (d == 4).any() for d in ref['depth']) and any((d == 2).any() for d in ref['depth'])
    # an image without boxes next to a full one
    c, ref = atss_ref.case('empty_next_to_full')
    assert all(not d[0].any() for d in ref['depth']) and any(d[1].any() for d in ref['depth'])
    # the box whose every coordinate is far outside, and the NaN boxes, get nothing; ATSS has no ignore band
    assert facts['nan_coordinate']['boxes_without_positives'] == 3
    assert all((d >= 0).all() for f in facts.values() for d in f['depth'])


def _lattices(h, w, stride):
    """Box centres on two fine lattices (a quarter of a stride apart; the second shifted off the dyadic values) that reach two
    strides beyond the grid on every side."""
    for shift in (0.0, 0.37 + stride / 8):
        xs = np.arange(-2 * stride, (w + 2) * stride + 1e-6, stride / 4) + shift
        ys = np.arange(-2 * stride, (h + 2) * stride + 1e-6, stride / 4) + shift
        gx, gy = np.meshgrid(xs, ys)
        yield gx.reshape(-1).astype(np.float32), gy.reshape(-1).astype(np.float32)


def test_window_rule_equals_the_full_scan():
    """Wherever the kernel would take the window's answer, it is the full scan's answer: grids from 1 x 1 to 12 x 12 (1 x N and
    N x 1 among them), every k, centres inside and up to two strides outside.  And the rule is no dead letter: inside a grid
    wider and higher than the window it admits every centre at every k."""
    stride = 8
    taken = full = 0
    for h in range(1, 13):
        for w in range(1, 13):
            for bcx, bcy in _lattices(h, w, stride):
                order, _ = atss_ref.full_scan(bcx, bcy, h, w, stride)
                cells, d2, sound, bound = atss_ref.window_scan(bcx, bcy, h, w, stride)
                in_grid = (bcx >= 0.5) & (bcx <= w * stride + 0.5) & (bcy >= 0.5) & (bcy <= h * stride + 0.5)
                for k in range(1, atss_ref.MAX_TOPK + 1):
                    want = min(k, h * w)
                    if cells.shape[1] < want:
                        full += len(bcx)
                        continue
                    ok = sound & (d2[:, want - 1] < bound)
                    assert np.array_equal(cells[ok, :want], order[ok, :want]), (h, w, k)
                    taken += int(ok.sum())
                    full += int((~ok).sum())
                    if h > atss_ref.WINDOW and w > atss_ref.WINDOW:
                        assert ok[in_grid].all(), (h, w, k)
    assert taken > 10 * full > 0, (taken, full)
    # a centre so far out that float32 no longer tells the cells of a row apart: the far cells tie, the rule must refuse
    far = np.asarray([3e9], np.float32)
    cells, d2, sound, bound = atss_ref.window_scan(far, np.asarray([40.0], np.float32), 12, 12, stride)
    assert not (sound & (d2[:, 8] < bound)).any()
    order, _ = atss_ref.full_scan(far, np.asarray([40.0], np.float32), 12, 12, stride)
    assert not np.array_equal(cells[0, :9], order[0, :9])


def test_arguments_are_checked():
    c, _ = atss_ref.case('single_level')
    for topk in (0, 17, -1):
        with pytest.raises(ValueError, match='topk'):
            run(dict(c, topk=topk))
    seven = dict(c, levels=c['levels'] * 7, anchors=c['anchors'] * 7)
    with pytest.raises(ValueError, match='levels'):
        run(seven)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        run(c, assign=lambda t, sizes, strides, anchors, classes, topk, want: _C.atss_assign_levels(t, anchors, classes, sizes, strides, topk, want))


def test_abi_validates_before_touching_the_device():
    lib = _C.library()
    assert 'odtk_atss_assign_levels' in _C.exported_symbols()
    anchors = (ctypes.c_float * 36)(*[0.0] * 36)
    levels = (_C.SnapLevel * 2)()
    for lv, (h, w, s) in zip(levels, ((4, 5, 8), (2, 3, 16))):
        lv.anchors = ctypes.cast(anchors, ctypes.POINTER(ctypes.c_float))
        lv.box_target, lv.depth, lv.height, lv.width, lv.stride = 1 << 20, 1 << 20, h, w, s

    def call(batch=2, targets=1 << 20, n_max=10, n_levels=2, lv=levels, a=9, classes=3, topk=9, ws=None, size=0):
        return lib.odtk_atss_assign_levels(batch, targets, n_max, n_levels, lv, a, classes, topk, ws, size, None)
    assert call() == 2 * 10 * 2 * 96 and call(n_max=0) == 256 and call(batch=1, n_max=8, n_levels=1) == 768      # 96 bytes per row and level
    for bad in (dict(batch=0), dict(batch=65536), dict(n_max=-1), dict(n_levels=0), dict(n_levels=_C.MAX_LEVELS + 1), dict(a=0),
                dict(a=_C.MAX_ANCHORS + 1), dict(classes=0), dict(topk=0), dict(topk=_C.ATSS_MAX_TOPK + 1),
                dict(batch=60000, n_max=80000)):
        assert call(**bad) == _C.ERR_INVALID, bad
    buf = ctypes.create_string_buffer(2 * 10 * 2 * 96 + 16)
    ws = (ctypes.addressof(buf) + 15) & ~15
    assert call(ws=ws, size=2 * 10 * 2 * 96 - 1) == _C.ERR_WORKSPACE
    assert call(ws=ws, size=2 * 10 * 2 * 96, targets=None) == _C.ERR_INVALID
    assert call(ws=ws, size=2 * 10 * 2 * 96, lv=None) == _C.ERR_INVALID
    assert call(ws=ws + 8, size=2 * 10 * 2 * 96) == _C.ERR_INVALID                    # records are 16-byte aligned
    for field, value in (('box_target', None), ('depth', None), ('height', 0), ('width', -1), ('stride', 0), ('anchors', None),
                         ('height', 1 << 30)):
        broken = (_C.SnapLevel * 2)()
        for dst, src in zip(broken, levels):
            ctypes.pointer(dst)[0] = src
        setattr(broken[1], field, ctypes.POINTER(ctypes.c_float)() if field == 'anchors' else value)
        assert call(ws=ws, size=2 * 10 * 2 * 96, lv=broken) == _C.ERR_INVALID, field


def test_command_line_flags():
    base = ['train', 'm.pth', '--annotations', 'a.json']
    plain = cli.parse(base)
    assert not hasattr(plain, 'assigner') and not hasattr(plain, 'atss_topk')
    args = cli.parse(base + ['--assigner', 'atss'])
    assert args.assigner == 'atss' and not hasattr(args, 'atss_topk')
    assert {k: v for k, v in vars(args).items() if k != 'assigner'} == vars(plain)      # nothing else in the namespace moves
    args = cli.parse(base + ['--assigner', 'atss', '--atss-topk', '5'])
    assert (args.assigner, args.atss_topk) == ('atss', 5)
    assert cli.parse(base + ['--assigner', 'iou']).assigner == 'iou'
    for refused in (base + ['--atss-topk', '5'], base + ['--assigner', 'iou', '--atss-topk', '5'],
                    base + ['--assigner', 'atss', '--rotated-bbox'], base + ['--assigner', 'nearest'],
                    base + ['--assigner', 'atss', '--atss-topk', '0'], base + ['--assigner', 'atss', '--atss-topk', '17'],
                    ['infer', 'm.pth', '--assigner', 'atss']):
        with pytest.raises(SystemExit):
            cli.parse(refused)
    train_parser_help = [spec['help'] for flag, spec in cli.TRAIN_FLAGS if flag == '--assigner'][0]
    assert 'resum' in train_parser_help


def _batch(seed=5, size=128, classes=4):
    from odtk import train as T
    return T.SyntheticBatches(2, size, size, classes=classes, max_boxes=5, seed=seed).batch()


def test_model_refusals():
    data, target = _batch()
    model = Model('ResNet18FPN', classes=4).train()
    assert (model.assigner, model.atss_topk) == ('iou', 9)
    heads = [torch.zeros(2, 9 * 4, 16 >> l, 16 >> l) for l in range(5)], [torch.zeros(2, 9 * 4, 16 >> l, 16 >> l) for l in range(5)]
    model.assigner = 'nearest'
    with pytest.raises(ValueError, match='assigner'):
        model._compute_loss(data, *heads, target)
    model.assigner = 'atss'
    model.rotated_bbox = True
    with pytest.raises(ValueError, match='rotated'):
        model._compute_loss(data, *heads, target)
    model.rotated_bbox = False
    seven = [[torch.zeros(2, 9 * 4, 2, 2)] * (box.MAX_LEVELS_PER_CALL + 1)] * 2
    with pytest.raises(ValueError, match='levels'):
        model._compute_loss(data, *seven, target)
    model.atss_topk = 17
    with pytest.raises(ValueError, match='topk'):
        model._compute_loss(data, *heads, target)


def test_checkpoints_do_not_carry_the_option(tmp_path):
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=4)
    keys = set(model.state_dict())
    plain, atss = str(tmp_path / 'plain.pth'), str(tmp_path / 'atss.pth')
    model.save({'path': plain})
    model.assigner, model.atss_topk = 'atss', 5
    model.save({'path': atss})
    assert set(model.state_dict()) == keys
    a, b = torch.load(plain, map_location='cpu'), torch.load(atss, map_location='cpu')
    assert a.keys() == b.keys() and a['state_dict'].keys() == b['state_dict'].keys()
    assert not any('atss' in k or 'assigner' in k for k in list(b) + list(b['state_dict']))
    loaded = Model.load(atss)[0]
    assert (loaded.assigner, loaded.atss_topk) == ('iou', 9)


def test_two_training_steps_on_the_cpu():
    """ResNet18FPN, two optimizer steps with each assigner from the same initial weights: finite losses, and not the IoU rule's."""
    losses = {}
    for assigner in ('iou', 'atss'):
        torch.manual_seed(0)
        model = Model('ResNet18FPN', classes=4)
        model.initialize(None)
        model.train()
        model.assigner = assigner
        optimizer = torch.optim.SGD(model.parameters(), lr=0.01)
        steps = []
        for step in range(2):
            data, target = _batch(seed=7 + step)
            optimizer.zero_grad()
            cls_loss, box_loss = model([data, target])
            (cls_loss + box_loss).backward()
            optimizer.step()
            steps.append((float(cls_loss.detach()), float(box_loss.detach())))
        losses[assigner] = steps
    assert all(np.isfinite(v) for steps in losses.values() for pair in steps for v in pair), losses
    assert all(a != b for a, b in zip(losses['iou'], losses['atss'])), losses
    assert all(box_loss > 0 for _, box_loss in losses['atss']), losses          # ATSS found positives
