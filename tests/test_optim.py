"""The fused optimisation step without a GPU: FusedSGD's torch restatement of the definition (`_step_reference`) against the numpy
checker tests/optim_ref.py bit for bit, the command-line options, the host side of the C ABI (every refusal before anything
touches HIP), checkpoints that continue weights, momentum and average exactly, and ModelEMA's swap."""
import copy
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import optim_ref as R
from odtk import _C
from odtk import main as cli
from odtk import train as T
from odtk.model import Model
from odtk.optim import FusedSGD, ModelEMA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, MOMENTUM = 0.01, 0.9


class _Params(torch.nn.Module):
    def __init__(self, shapes, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.items = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes])


def _arrays(tensors):
    return [None if t is None else t.detach().numpy().copy() for t in tensors]


@pytest.mark.parametrize('wd,ema,scale,clip', list(itertools.product([0.0, 1e-4], [False, True], [None, 65536.0], [None, 0.5])))
def test_reference_branch_is_the_definition(wd, ema, scale, clip):
    """Five steps (the first and four later ones) of every option combination, bit for bit."""
    module = _Params([(37,), (5, 3), (2, 3, 3, 3)], 1)
    params = list(module.parameters())
    opt = FusedSGD(params, lr=LR, momentum=MOMENTUM, weight_decay=wd, max_norm=clip)
    average = ModelEMA(module, 0.99) if ema else None
    if ema:
        opt.bind_ema(average)
    P, B = _arrays(params), [None] * len(params)
    E = [p.copy() if ema else None for p in P]
    g = torch.Generator().manual_seed(2)
    for t in range(5):
        grads = [torch.randn(p.shape, generator=g) * (scale or 1.0) for p in params]
        for p, grad in zip(params, grads):
            p.grad = grad.clone()
        if scale:
            opt.grad_scale, opt.found_inf = torch.tensor(scale), torch.tensor(0.0)
        opt.step()
        P, B, E, norm, coef = R.step_all(P, _arrays(grads), B, E, LR, MOMENTUM, wd, np.float32(1.0 - R.decay_at(0.99, t)), scale, clip)
        for i, p in enumerate(params):
            assert R.same_bits(p.detach().numpy(), P[i]) and R.same_bits(opt.state[p]['momentum_buffer'].numpy(), B[i]), (t, i)
            if ema:
                assert R.same_bits(average.of(p).numpy(), E[i]), (t, i)
        if clip:
            assert R.same_bits(opt.last_grad_norm.numpy(), norm) and coef < 1
    assert average is None or average.updates == 5


def test_special_values_behave_as_in_the_checker():
    """-0, inf and NaN gradients with found_inf = 0 go through the arithmetic (only a non-finite NORM skips); a set found_inf and,
    under clipping, a NaN gradient leave everything as it was."""
    special = torch.tensor([-0.0, 0.0, float('inf'), -float('inf'), float('nan'), 1.0, -2.5])
    for first in (True, False):
        module = _Params([(7,)], 3)
        p = module.items[0]
        opt = FusedSGD([p], lr=LR, momentum=MOMENTUM, weight_decay=0.0)
        average = ModelEMA(module, 0.9)
        opt.bind_ema(average)
        P, B, E = _arrays([p]), [None], _arrays([p])
        grads = ([torch.ones(7)] if not first else []) + [special]
        for t, grad in enumerate(grads):
            p.grad = grad.clone()
            opt.found_inf = torch.tensor(0.0)
            opt.step()
            P, B, E, _, _ = R.step_all(P, _arrays([grad]), B, E, LR, MOMENTUM, 0.0, np.float32(1.0 - R.decay_at(0.9, t)))
        assert R.same_values(p.detach().numpy(), P[0]) and R.same_values(opt.state[p]['momentum_buffer'].numpy(), B[0])
        assert R.same_values(average.of(p).numpy(), E[0])
        assert np.signbit(B[0][0]) == first                        # -0 stays -0 on a first step; (0.9 * 1) + -0 is 0.9
    # skipped: found_inf set, or a NaN under clipping
    for found_inf, clip in ((1.0, None), (0.0, 1.0)):
        module = _Params([(7,)], 3)
        p = module.items[0]
        opt = FusedSGD([p], lr=LR, momentum=MOMENTUM, weight_decay=1e-4, max_norm=clip)
        average = ModelEMA(module, 0.9)
        opt.bind_ema(average)
        p.grad = torch.ones(7)
        opt.step()
        before = [t.clone() for t in (p.detach(), opt.state[p]['momentum_buffer'], average.of(p))]
        p.grad = special.clone()
        opt.found_inf = torch.tensor(found_inf)
        opt.step()
        assert all(R.same_bits(a.numpy(), b.detach().numpy()) for a, b in zip(before, (p, opt.state[p]['momentum_buffer'], average.of(p))))
        assert average.updates == 2                                 # a skipped step still counts
        if clip:
            assert np.isnan(float(opt.last_grad_norm))


def test_ema_decay_schedule():
    module = _Params([(3,)], 0)
    average = ModelEMA(module, 0.9998)
    assert [average.decay_at(t) for t in (0, 1, 90)] == [0.1, 2 / 11, 0.91] and average.decay_at(10 ** 6) == 0.9998
    assert R.same_bits(np.float32(average.one_minus_decay()), np.float32(1.0 - 0.1))
    for bad in (0.0, 1.0, -0.5, float('nan')):
        with pytest.raises(ValueError):
            ModelEMA(module, bad)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            FusedSGD(module.parameters(), lr=LR, max_norm=bad)


def test_options_parse_and_refuse():
    base = ['train', 'model.pth', '--annotations', 'a.json']
    args = cli.parse(base + ['--ema', '0.9998', '--clip-grad-norm', '35', '--fused-step'])
    assert args.ema == 0.9998 and args.clip_grad_norm == 35.0 and args.fused_step is True
    plain = cli.parse(base)
    assert not any(hasattr(plain, f) for f in ('ema', 'clip_grad_norm', 'fused_step'))
    assert cli.parse(['infer', 'model.pth', '--no-ema']).no_ema is True and not hasattr(cli.parse(['infer', 'model.pth']), 'no_ema')
    assert cli.parse(['export', 'model.pth', 'out.onnx', '--no-ema']).no_ema is True
    for bad in (['--clip-grad-norm', '0'], ['--clip-grad-norm', '-1'], ['--clip-grad-norm', 'inf'], ['--clip-grad-norm', 'nan'],
                ['--ema', '0'], ['--ema', '1'], ['--ema', '1.5'], ['--ema', '-0.1'], ['--ema', 'nan']):
        with pytest.raises(SystemExit):
            cli.parse(base + bad)
    for flag in ('--ema', '--clip-grad-norm'):
        assert 'resum' in [spec['help'] for name, spec in cli.TRAIN_FLAGS if name == flag][0]
    assert all(flag in cli.__doc__ for flag in ('--ema', '--clip-grad-norm', '--fused-step', '--no-ema'))


def _tensor(numel=8, param=16, grad=16, momentum=16, ema=None):
    return _C.OptimTensor(param, grad, momentum, ema, numel)


def test_abi_on_the_host():
    lib = _C.library()
    assert {'odtk_optim_grad_norm', 'odtk_optim_grad_norm_chained', 'odtk_optim_sgd_step'} <= set(_C.exported_symbols())
    assert lib.odtk_abi_struct_size(17) == ctypes.sizeof(_C.OptimTensor) == 40 and lib.odtk_abi_struct_size(16) == -1
    header = open(os.path.join(ROOT, 'include', 'odtk_hip.h')).read()
    assert int(re.search(r'#define ODTK_MAX_OPTIM_TENSORS (\d+)', header).group(1)) == _C.MAX_OPTIM_TENSORS == 64
    assert int(re.search(r'#define ODTK_OPTIM_CHUNK (\d+)', header).group(1)) == _C.OPTIM_CHUNK

    def step(tensors, n=None, lr=0.1, momentum=0.9, wd=1e-4, first=0, omd=0.5):
        table = (_C.OptimTensor * max(len(tensors), 1))(*tensors)
        return lib.odtk_optim_sgd_step(len(tensors) if n is None else n, table, lr, momentum, wd, first, omd, None, None, None, None)

    def norm(tensors, n=None, max_norm=1.0, state=16, workspace=None, size=0):
        table = (_C.OptimTensor * max(len(tensors), 1))(*tensors)
        return lib.odtk_optim_grad_norm(len(tensors) if n is None else n, table, None, max_norm, state, workspace, size, None)

    nan, inf = float('nan'), float('inf')
    # the two-phase query: 8 bytes per started chunk, rounded up to 256; empty tensors are legal and fill no slot
    assert norm([_tensor(_C.OPTIM_CHUNK * 40 + 1)]) == 512 and norm([_tensor(5), _tensor(0, None, None, None)]) == 256
    assert norm([_tensor(0)]) == 256
    assert lib.odtk_optim_grad_norm_chained(1, (_C.OptimTensor * 1)(_tensor(5)), None, 1.0, 16, 63, 1, None, 0, None) == 512
    buf = ctypes.create_string_buffer(64)
    assert norm([_tensor(5)], workspace=ctypes.cast(buf, ctypes.c_void_p), size=64) == _C.ERR_WORKSPACE
    # every refusal, with null streams and no GPU
    refused = [
        step([_tensor(param=None)]), step([_tensor(grad=None)]), step([_tensor(momentum=None)]), norm([_tensor(grad=None)]),
        step([_tensor(-1)]), norm([_tensor(-1)]),
        step([]), norm([]), step([_tensor()], n=65), norm([_tensor()], n=65), step([_tensor()], n=-1),
        lib.odtk_optim_sgd_step(1, None, 0.1, 0.9, 0.0, 0, 0.0, None, None, None, None),
        step([_tensor()], lr=nan), step([_tensor()], lr=inf), step([_tensor()], momentum=nan), step([_tensor()], momentum=-inf),
        step([_tensor()], wd=nan), step([_tensor()], wd=inf),
        step([_tensor()], omd=-0.001), step([_tensor()], omd=1.001), step([_tensor()], omd=nan),
        step([_tensor()], first=2),
        norm([_tensor()], max_norm=0.0), norm([_tensor()], max_norm=-1.0), norm([_tensor()], max_norm=inf), norm([_tensor()], max_norm=nan),
        step([_tensor(param=18)]), step([_tensor(ema=17)]), norm([_tensor(grad=2)]),
        lib.odtk_optim_grad_norm_chained(1, (_C.OptimTensor * 1)(_tensor(5)), None, 1.0, 16, -1, 1, None, 0, None),
    ]
    assert refused == [_C.ERR_INVALID] * len(refused)
    # the norm looks at grad and numel only; a full table of 64 is accepted
    assert norm([_tensor(8, None, 16, None)] * 64) == 64 * 8
    buf = ctypes.create_string_buffer(512)
    aligned = (ctypes.addressof(buf) + 255) // 256 * 256
    assert norm([_tensor(5)], state=None, workspace=aligned, size=256) == _C.ERR_INVALID    # a null state is found before the launch


def _tiny_model(seed=0):
    torch.manual_seed(seed)
    model = Model('ResNet18FPN', classes=3)
    model.initialize(None)
    return model


def _batches(n):
    source = T.SyntheticBatches(2, 128, 128, classes=3, max_boxes=4, seed=3)
    return [source.batch() for _ in range(n)]


def test_checkpoint_continues_weights_momentum_and_average_exactly(tmp_path, capsys):
    start, batches, cpu = _tiny_model(), _batches(5), torch.device('cpu')
    options = dict(lr=0.001, warmup=2, verbose=False, log_interval=100, ema_decay=0.99, clip_grad_norm=35.0)
    split, whole = str(tmp_path / 'split.pth'), str(tmp_path / 'whole.pth')
    assert T.train_batches(copy.deepcopy(start), {}, batches[:3], 3, cpu, save_path=split, **options) == 3
    model, state = Model.load(split)
    assert set(state) == {'iteration', 'optimizer', 'scheduler', 'ema'} and state['ema']['updates'] == 3 and state['ema']['decay'] == 0.99
    assert not torch.equal(state['ema']['state_dict']['cls_head.0.weight'], model.state_dict()['cls_head.0.weight'])   # the raw weights are saved
    assert T.train_batches(model, state, batches[3:], 5, cpu, save_path=split, **options) == 5
    assert T.train_batches(copy.deepcopy(start), {}, batches, 5, cpu, save_path=whole, **options) == 5
    a, b = torch.load(split, map_location='cpu'), torch.load(whole, map_location='cpu')
    assert a['iteration'] == b['iteration'] == 5 and a['ema']['updates'] == b['ema']['updates'] == 5
    for x, y in ((a['state_dict'], b['state_dict']), (a['ema']['state_dict'], b['ema']['state_dict'])):
        assert list(x) == list(y) and all(torch.equal(x[k], y[k]) for k in x)
    assert a['optimizer']['state'].keys() == b['optimizer']['state'].keys() and len(a['optimizer']['state']) > 10
    assert all(torch.equal(a['optimizer']['state'][k]['momentum_buffer'], b['optimizer']['state'][k]['momentum_buffer']) for k in a['optimizer']['state'])
    assert a['scheduler'] == b['scheduler']

    # resuming with --ema from a checkpoint without an average starts it at the current weights with updates = 0 ...
    model, state = Model.load(split)
    del state['ema']
    _, _, optimizer, _ = T.prepare(model, cpu, state=state, ema_decay=0.5)
    assert optimizer.ema.updates == 0 and all(torch.equal(optimizer.ema.of(p), p.detach()) for p in model.parameters())
    # ... and resuming without it drops a stored one and says so, in one line; the optimizer is then the reference's
    capsys.readouterr()
    model, state = Model.load(split)
    _, _, optimizer, _ = T.prepare(model, cpu, state=state)
    said = capsys.readouterr().out
    assert type(optimizer) is torch.optim.SGD and said.count('\n') == 1 and 'EMA' in said and 'dropped' in said
    assert len(optimizer.state) == len(a['optimizer']['state'])     # a FusedSGD checkpoint loaded into plain SGD


def test_sgd_and_fused_sgd_read_each_others_state():
    def pair(kind):
        module = _Params([(6,), (4, 2)], 5)
        make = FusedSGD if kind == 'fused' else torch.optim.SGD
        return module, make(module.parameters(), lr=LR, momentum=MOMENTUM, weight_decay=1e-4)

    g = torch.Generator().manual_seed(9)
    grads = [[torch.randn(6, generator=g), torch.randn(4, 2, generator=g)] for _ in range(4)]

    def run(module, opt, steps):
        for grad in steps:
            for p, v in zip(module.parameters(), grad):
                p.grad = v.clone()
            opt.step()

    for first, second in (('sgd', 'fused'), ('fused', 'sgd')):
        module, opt = pair(first)
        run(module, opt, grads[:2])
        state = copy.deepcopy(opt.state_dict())
        assert all(set(s) == {'momentum_buffer'} for s in state['state'].values()) and len(state['state']) == 2
        other_module, other = pair(second)
        other_module.load_state_dict(module.state_dict())
        other.load_state_dict(state)
        run(module, opt, grads[2:])
        run(other_module, other, grads[2:])
        for p, q in zip(module.parameters(), other_module.parameters()):
            assert torch.allclose(p, q, rtol=1e-6, atol=1e-7)
            assert torch.allclose(opt.state[p]['momentum_buffer'], other.state[q]['momentum_buffer'], rtol=1e-6, atol=1e-7)
        assert other.state_dict()['param_groups'][0].keys() == opt.state_dict()['param_groups'][0].keys()


def test_swapped_serves_the_average_and_puts_the_weights_back():
    model = _tiny_model(1).eval()
    with torch.no_grad():
        model.cls_head[-1].bias.fill_(0.0)                          # detections exist
    average = ModelEMA(model, 0.9)
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=MOMENTUM)
    opt.bind_ema(average)
    g = torch.Generator().manual_seed(4)
    for _ in range(2):
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g) * p.detach().abs().mean()
        opt.step()
    opt.zero_grad(set_to_none=True)
    x = torch.randn(1, 3, 128, 128, generator=g)
    fresh = Model('ResNet18FPN', classes=3).eval()
    fresh.load_state_dict(average.state_dict()['state_dict'])
    before = [p.detach().clone() for p in model.parameters()]
    calls = []
    model.invalidate_engine = lambda: calls.append(1)
    with torch.no_grad():
        raw = model(x)
        want = fresh(x)
        with average.swapped(model) as inside:
            assert inside is model and len(calls) == 1
            got = model(x)
        assert len(calls) == 2
        again = model(x)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and not all(torch.equal(a, b) for a, b in zip(got, raw))
    assert all(torch.equal(a, b) for a, b in zip(again, raw))
    assert all(torch.equal(a.view(torch.int32), p.detach().view(torch.int32)) for a, p in zip(before, model.parameters()))
    state = average.state_dict()
    assert set(state) == {'decay', 'updates', 'state_dict'} and state['updates'] == 2 and list(state['state_dict']) == list(model.state_dict())
    other = ModelEMA(fresh, 0.5)
    other.load_state_dict(state)
    assert other.updates == 2 and other.decay == 0.5 and all(torch.equal(other.shadow[k], average.shadow[k]) for k in average.shadow)
