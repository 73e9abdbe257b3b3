"""Task-aligned target assignment off the GPU: odtk.box.tal_assign_levels on CPU tensors (its pure-torch branch) against the
checker (tests/tal_ref.py) on every case the device test runs, what the cases are meant to contain, the C ABI's refusals, the
command line, and Model's plumbing -- the options are run-time attributes that never reach a checkpoint."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tal_ref
from odtk import _C, box
from odtk import main as cli
from odtk.model import Model


def run(c, device='cpu', assign=box.tal_assign_levels, heads=None):
    cls_heads, box_heads = heads or ([torch.from_numpy(x) for x in c['cls']], [torch.from_numpy(x) for x in c['box']])
    return assign(torch.from_numpy(c['targets']).to(device), [x.to(device) for x in cls_heads], [x.to(device) for x in box_heads],
                  [s for _, _, s in c['levels']], [torch.from_numpy(a) for a in c['anchors']], c['classes'], c['topk'], c['alpha'],
                  c['beta'], c['want_cls'])


@pytest.mark.parametrize('name', list(tal_ref.CASES))
def test_torch_branch_equals_the_checker(name):
    c, ref = tal_ref.case(name)
    got = run(c)
    for l, (h, w, _) in enumerate(c['levels']):
        b, a = c['targets'].shape[0], c['anchors'][l].shape[0]
        assert tuple(got[1][l].shape) == (b, a, 4, h, w) and tuple(got[2][l].shape) == (b, a, 1, h, w)
    tal_ref.compare(got, ref, c['want_cls'], name)


def test_torch_branch_widens_16_bit_heads():
    c, ref = tal_ref.case('random_a9', 'bfloat16')
    tal_ref.compare(run(c, heads=tal_ref.heads_in(c, 'bfloat16')), ref, c['want_cls'])


def _depth_by_index(ref, image):
    """depth of `image` by global anchor index."""
    return np.concatenate([d[image].reshape(-1) for d in ref['depth']])


def test_cases_are_not_vacuous():
    """With the checker alone: each case exercises what it names."""
    facts = {name: tal_ref.case(name)[1] for name in tal_ref.CASES}
    for name in ('random_a9', 'random_a1', 'random_no_cls'):
        assert sum(n > 0 for n in facts[name]['assigned_per_level']) >= 2, (name, facts[name]['assigned_per_level'])
    # the streaming path: more candidates than the staging buffer holds at ANY capacity up to 8 192, so several reductions
    c, ref = tal_ref.case('whole_image_stream')
    assert c['levels'][0][:2] == (40, 40) and c['anchors'][0].shape[0] == 9
    assert ref['max_candidates'] >= 14400 > 8192 >= tal_ref.STAGE and ref['assigned'] > 0
    assert facts['no_centre']['boxes_without_positives'] == 1 and facts['no_centre']['boxes'] == 3
    c, ref = tal_ref.case('fewer_than_k')
    assert c['topk'] == 16 and c['anchors'][0].shape[0] == 1 and ref['rows_with_fewer_than_k'] > 0
    assert all(0 < len(sel) < 16 and len(sel) == len(cand) for _, _, cand, sel, eligible in ref['rows'])
    for name in ('ties', 'ties_a9'):
        c, ref = tal_ref.case(name)
        assert ref['ties_at_the_kth'] > 0, name
    # the lowest indices win a tie: with one anchor per cell, equal logits and zero deltas, a row's selected entries that share the
    # k-th metric are the lowest candidates among ALL that share it -- here checked on the plainest row, where every candidate ties
    c, ref = tal_ref.case('zero_metric')
    assert ref['zero_metric_selected'] > 0
    for _, _, cand, sel, eligible in ref['rows']:
        assert len(cand) > c['topk'] and np.array_equal(sel, np.sort(cand)[:c['topk']])
    c, ref = tal_ref.case('contested')
    assert ref['contested'] > 0
    # rows 0 and 1 of image 0 are the same box with classes 1 and 2, so the same u at every anchor: the earlier row wins every
    # anchor both select (depth 2, never 3); row 2 is another box that overlaps them
    selected = {row: set(sel.tolist()) for image, row, _, sel, _ in ref['rows'] if image == 0}
    both = sorted(selected[0] & selected[1])
    depth = _depth_by_index(ref, 0)
    assert len(both) > 0 and not (depth[both] == 3).any() and (depth[both] == 2).any()
    assert (depth == 3).any() and (depth == 1).any() and (selected[2] & (selected[0] | selected[1]))
    c, ref = tal_ref.case('non_finite')
    assert ref['nan_candidates'] > 0 and ref['assigned'] > 0 and any(eligible < len(cand) for _, _, cand, _, eligible in ref['rows'])
    for _, _, cand, sel, eligible in ref['rows']:
        assert len(sel) == min(c['topk'], eligible) and len(set(sel.tolist())) == len(sel)
    c, ref = tal_ref.case('padding')
    assert ref['boxes'] == 4 and c['targets'][0, 2, 4] == c['classes'] and ref['assigned'] > 0
    assert all(not (d == c['classes'] + 1).any() and not (d == 2.5).any() for d in ref['depth'])
    for name in ('n_max_0', 'all_padding'):
        assert facts[name]['assigned'] == 0 and facts[name]['boxes'] == 0
    c, ref = tal_ref.case('many_rows')
    assert c['targets'].shape[1] == 130 > tal_ref.ROUND and ref['boxes'] == 2 * 130 and ref['contested'] > 0
    settings = {(tal_ref.case(n)[0]['alpha'], tal_ref.case(n)[0]['beta'], tal_ref.case(n)[0]['topk']) for n in tal_ref.CASES}
    assert {(0, 6, 13), (1, 1, 13), (4, 8, 13), (1, 6, 1), (1, 6, 16)} <= settings
    for name in ('alpha_0', 'beta_1', 'alpha_4_beta_8', 'topk_1', 'topk_16'):
        assert facts[name]['assigned'] > 0, name
    assert all((d >= 0).all() for f in facts.values() for d in f['depth'])           # no ignore band
    assert tal_ref.MAX_TOPK == _C.ATSS_MAX_TOPK


def test_the_exponents_matter():
    """alpha = 0 ranks by the overlap alone, so flipping the logits' sign changes nothing; with alpha = 1 it does."""
    c, ref = tal_ref.case('alpha_0')
    flipped = run(c, heads=([-torch.from_numpy(x) for x in c['cls']], [torch.from_numpy(x) for x in c['box']]))
    tal_ref.compare(flipped, ref, c['want_cls'])
    c, ref = tal_ref.case('random_a9')
    flipped = run(c, heads=([-torch.from_numpy(x) for x in c['cls']], [torch.from_numpy(x) for x in c['box']]))
    assert any(not np.array_equal(f.numpy(), d) for f, d in zip(flipped[2], ref['depth']))


def test_arguments_are_checked():
    c, _ = tal_ref.case('random_a1')
    for field, values in (('topk', (0, 17, -1)), ('alpha', (-1, 5)), ('beta', (0, 9))):
        for value in values:
            with pytest.raises(ValueError, match=field):
                run(dict(c, **{field: value}))
    seven = dict(c, levels=[c['levels'][0]] * 7, anchors=[c['anchors'][0]] * 7, cls=[c['cls'][0]] * 7, box=[c['box'][0]] * 7)
    with pytest.raises(ValueError, match='levels'):
        run(seven)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        _C.tal_assign_levels(torch.from_numpy(c['targets']), [torch.from_numpy(x) for x in c['cls']], [torch.from_numpy(x) for x in c['box']],
                             [torch.from_numpy(a) for a in c['anchors']], c['classes'], [s for _, _, s in c['levels']])


def test_abi_validates_before_touching_the_device():
    lib = _C.library()
    assert 'odtk_tal_assign_levels' in _C.exported_symbols() and hasattr(lib, 'odtk_tal_assign_levels')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert 'odtk_tal_assign_levels' in open(os.path.join(root, 'include', 'odtk_hip.h')).read()
    # exports.map hides only the compiler's per-source objects: every extern "C" symbol of the header is exported
    assert 'local: __hip_cuid_*' in open(os.path.join(root, 'retinanet-examples_amd', 'csrc', 'exports.map')).read()
    assert lib.odtk_abi_struct_size(1) == ctypes.sizeof(_C.SnapLevel) and lib.odtk_abi_struct_size(3) == ctypes.sizeof(_C.LossLevel) == 64
    assert lib.odtk_abi_struct_size(13) == -1                                           # both descriptors are reused: no new struct
    anchors = (ctypes.c_float * 36)(*[0.0] * 36)
    levels, heads = (_C.SnapLevel * 2)(), (_C.LossLevel * 2)()
    for lv, hd, (h, w, s) in zip(levels, heads, ((4, 5, 8), (2, 3, 16))):
        lv.anchors = ctypes.cast(anchors, ctypes.POINTER(ctypes.c_float))
        lv.box_target, lv.depth, lv.height, lv.width, lv.stride = 1 << 20, 1 << 20, h, w, s
        hd.cls, hd.box = 1 << 20, 1 << 20

    def call(batch=2, targets=1 << 20, n_max=10, n_levels=2, lv=levels, hd=heads, a=9, classes=3, dtype=_C.F32, topk=13, alpha=1, beta=6,
             ws=None, size=0):
        return lib.odtk_tal_assign_levels(batch, targets, n_max, n_levels, lv, hd, a, classes, dtype, topk, alpha, beta, ws, size, None)
    need = 2 * 10 * 144
    assert call() == (need + 255) // 256 * 256 and call(n_max=0) == 256 and call(batch=1, n_max=16, n_levels=1) == 16 * 144   # 144 bytes per row
    for bad in (dict(batch=0), dict(batch=65536), dict(n_max=-1), dict(n_levels=0), dict(n_levels=_C.MAX_LEVELS + 1), dict(a=0),
                dict(a=_C.MAX_ANCHORS + 1), dict(classes=0), dict(topk=0), dict(topk=_C.ATSS_MAX_TOPK + 1), dict(alpha=-1), dict(alpha=5),
                dict(beta=0), dict(beta=9), dict(batch=60000, n_max=800000)):
        assert call(**bad) == _C.ERR_INVALID, bad
    assert call(dtype=7) == _C.ERR_UNSUPPORTED
    size = (need + 255) // 256 * 256
    buf = ctypes.create_string_buffer(size + 16)
    ws = (ctypes.addressof(buf) + 15) & ~15
    assert call(ws=ws, size=size - 1) == _C.ERR_WORKSPACE
    assert call(ws=ws, size=size, targets=None) == _C.ERR_INVALID
    assert call(ws=ws, size=size, lv=None) == _C.ERR_INVALID
    assert call(ws=ws, size=size, hd=None) == _C.ERR_INVALID
    assert call(ws=ws + 8, size=size) == _C.ERR_INVALID                                # records are 16-byte aligned

    def copies():
        lv2, hd2 = (_C.SnapLevel * 2)(), (_C.LossLevel * 2)()
        for dst, src in zip(lv2, levels):
            ctypes.pointer(dst)[0] = src
        for dst, src in zip(hd2, heads):
            ctypes.pointer(dst)[0] = src
        return lv2, hd2
    for field, value in (('box_target', None), ('depth', None), ('height', 0), ('width', -1), ('stride', 0), ('anchors', None),
                         ('height', 1 << 30), ('width', 1 << 28)):
        lv2, hd2 = copies()
        setattr(lv2[1], field, ctypes.POINTER(ctypes.c_float)() if field == 'anchors' else value)
        assert call(ws=ws, size=size, lv=lv2, hd=hd2) == _C.ERR_INVALID, field
    for field, value, dtype in (('cls', None, _C.F32), ('box', None, _C.F32), ('channels_last', 2, _C.F32), ('cls', (1 << 20) + 2, _C.F32),
                                ('box', (1 << 20) + 1, _C.BF16), ('cls', (1 << 20) + 1, _C.F16)):
        lv2, hd2 = copies()
        setattr(hd2[0], field, value)
        assert call(ws=ws, size=size, lv=lv2, hd=hd2, dtype=dtype) == _C.ERR_INVALID, field
    # the total anchor count: two levels that fit on their own, but not together
    lv2, hd2 = copies()
    for lv in lv2:
        lv.height, lv.width = 1 << 14, 1 << 13                                         # 9 * 2^27 anchors each
    assert call(ws=ws, size=size, lv=lv2, hd=hd2) == _C.ERR_INVALID
    # the heads' own height / width fields are ignored
    lv2, hd2 = copies()
    hd2[0].height = -5
    assert call(ws=ws, size=size - 1, lv=lv2, hd=hd2) == _C.ERR_WORKSPACE


def test_command_line_flags():
    base = ['train', 'm.pth', '--annotations', 'a.json']
    plain = cli.parse(base)
    assert not any(hasattr(plain, f) for f in ('assigner', 'tal_topk', 'tal_alpha', 'tal_beta'))
    args = cli.parse(base + ['--assigner', 'tal'])
    assert args.assigner == 'tal' and not any(hasattr(args, f) for f in ('tal_topk', 'tal_alpha', 'tal_beta', 'atss_topk'))
    assert {k: v for k, v in vars(args).items() if k != 'assigner'} == vars(plain)      # nothing else in the namespace moves
    args = cli.parse(base + ['--assigner', 'tal', '--tal-topk', '10', '--tal-alpha', '0', '--tal-beta', '3'])
    assert (args.assigner, args.tal_topk, args.tal_alpha, args.tal_beta) == ('tal', 10, 0, 3)
    args = cli.parse(base + ['--assigner', 'tal', '--cls-loss', 'vfl', '--box-loss', 'giou'])
    assert (args.assigner, args.cls_loss, args.box_loss) == ('tal', 'vfl', 'giou')
    assert cli.parse(base + ['--assigner', 'atss', '--atss-topk', '5']).atss_topk == 5
    refused = [base + [flag, '2'] for flag in ('--tal-topk', '--tal-alpha', '--tal-beta')]
    refused += [base + ['--assigner', other, flag, '2'] for other in ('iou', 'atss') for flag in ('--tal-topk', '--tal-alpha', '--tal-beta')]
    refused += [base + ['--assigner', 'tal', flag, value] for flag, value in (('--tal-topk', '0'), ('--tal-topk', '17'), ('--tal-alpha', '-1'),
                                                                            ('--tal-alpha', '5'), ('--tal-beta', '0'), ('--tal-beta', '9'),
                                                                            ('--tal-alpha', '0.5'))]
    refused += [base + ['--assigner', 'tal', '--rotated-bbox'], base + ['--assigner', 'tal', '--atss-topk', '5'],
                ['infer', 'm.pth', '--assigner', 'tal'], ['infer', 'm.pth', '--tal-topk', '5']]
    for argv in refused:
        with pytest.raises(SystemExit):
            cli.parse(argv)
    for flag in ('--assigner', '--tal-topk', '--tal-alpha', '--tal-beta'):
        assert 'resum' in [spec['help'] for name, spec in cli.TRAIN_FLAGS if name == flag][0], flag
    assert '--assigner tal' in cli.__doc__ and 'resum' in cli.__doc__


def _batch(seed=5, size=128, classes=4):
    from odtk import train as T
    return T.SyntheticBatches(2, size, size, classes=classes, max_boxes=5, seed=seed).batch()


def test_model_defaults_and_refusals():
    data, target = _batch()
    model = Model('ResNet18FPN', classes=4).train()
    assert (model.assigner, model.tal_topk, model.tal_alpha, model.tal_beta) == ('iou', 13, 1, 6)
    heads = [torch.zeros(2, 9 * 4, 16 >> l, 16 >> l) for l in range(5)], [torch.zeros(2, 9 * 4, 16 >> l, 16 >> l) for l in range(5)]
    model.assigner = 'nearest'
    with pytest.raises(ValueError, match='assigner'):
        model._compute_loss(data, *heads, target)
    model.assigner = 'tal'
    model.rotated_bbox = True
    with pytest.raises(ValueError, match='rotated'):
        model._compute_loss(data, *heads, target)
    model.rotated_bbox = False
    seven = [[torch.zeros(2, 9 * 4, 2, 2)] * (box.MAX_LEVELS_PER_CALL + 1)] * 2
    with pytest.raises(ValueError, match='levels'):
        model._compute_loss(data, *seven, target)
    for field, value in (('tal_topk', 17), ('tal_alpha', 5), ('tal_beta', 0)):
        setattr(model, field, value)
        with pytest.raises(ValueError, match=field[4:]):
            model._compute_loss(data, *heads, target)
        setattr(model, field, {'tal_topk': 13, 'tal_alpha': 1, 'tal_beta': 6}[field])
    cls_loss, box_loss = model._compute_loss(data, *heads, target)                      # a cold start: equal scores, zero deltas
    assert np.isfinite(float(cls_loss)) and float(box_loss) > 0


def test_checkpoints_do_not_carry_the_options(tmp_path):
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=4)
    keys = set(model.state_dict())
    plain, tal = str(tmp_path / 'plain.pth'), str(tmp_path / 'tal.pth')
    model.save({'path': plain})
    model.assigner, model.tal_topk, model.tal_alpha, model.tal_beta = 'tal', 5, 2, 3
    model.save({'path': tal})
    assert set(model.state_dict()) == keys
    a, b = torch.load(plain, map_location='cpu'), torch.load(tal, map_location='cpu')
    assert a.keys() == b.keys() and a['state_dict'].keys() == b['state_dict'].keys()
    assert not any('tal' in k.split('.') or k.startswith('tal') or 'assigner' in k for k in list(b) + list(b['state_dict']))
    loaded = Model.load(tal)[0]
    assert (loaded.assigner, loaded.tal_topk, loaded.tal_alpha, loaded.tal_beta) == ('iou', 13, 1, 6)


def test_two_training_steps_on_the_cpu():
    """ResNet18FPN, two optimizer steps of the TOOD-style recipe (qfl + giou) with each assigner from the same initial weights:
    finite losses, and task-aligned assignment's are not ATSS's."""
    losses = {}
    for assigner in ('atss', 'tal'):
        torch.manual_seed(0)
        model = Model('ResNet18FPN', classes=4)
        model.initialize(None)
        model.train()
        model.assigner, model.cls_loss, model.box_loss = assigner, 'qfl', 'giou'
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
    assert all(a != b for a, b in zip(losses['atss'], losses['tal'])), losses
    assert all(box_loss > 0 for _, box_loss in losses['tal']), losses                   # the assigner found positives
