"""The fused optimisation step on an MI355X (csrc/optim.hpp; odtk/optim.py: FusedSGD, ModelEMA): the kernels against the numpy
checker tests/optim_ref.py, bit for bit, over every launch shape -- one to three launches, empty tensors, every alignment of the four
arrays, every option --, the skip on overflow, the norm against the correctly rounded sum, torch.amp.GradScaler's hand-over, a
hipGraph of the calls, the trajectory against torch's own optimizer, and `odtk train --ema --clip-grad-norm` / `odtk infer` end to end."""
import ctypes
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch

import optim_ref as R
from odtk import _C
from odtk import main as cli
from odtk import train as train_module
from odtk.model import Model
from odtk.optim import FusedSGD, ModelEMA

pytestmark = pytest.mark.gpu

C = _C.OPTIM_CHUNK
NUMELS = [1, 3, 4, 63, 64, 65, C - 1, C, C + 1, 2 * C + 5]
LR, MOMENTUM = 0.01, 0.9
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data')
ANN = os.path.join(DATA, 'annotations.json')


def _placed(values, offset):
    """`values` on the device, `offset` floats behind a 16-byte boundary."""
    store = torch.empty(values.size + 8, dtype=torch.float32, device='cuda')
    assert store.data_ptr() % 16 == 0
    view = store[offset:offset + values.size]
    view.copy_(torch.from_numpy(values))
    return view


class Case:
    """A tensor list on the device and its numpy twin.  offsets[i] = the misalignment of (param, grad, momentum, ema) of tensor i."""

    def __init__(self, numels, offsets, seed, ema):
        rng = np.random.default_rng(seed)
        self.numels, self.offsets, self.rng = numels, offsets, rng
        self.P = [rng.standard_normal(n).astype(np.float32) for n in numels]
        self.B = [None] * len(numels)
        self.E = [p + rng.standard_normal(p.size).astype(np.float32) * np.float32(0.01) if ema else None for p in self.P]
        self.p = [_placed(v, o[0]) for v, o in zip(self.P, offsets)]
        self.m = [_placed(np.zeros(n, np.float32), o[2]) for n, o in zip(numels, offsets)]
        self.e = [_placed(v, o[3]) for v, o in zip(self.E, offsets)] if ema else None
        self.g = None

    def grads(self, scale=1.0, spread=0):
        G = []
        for n in self.numels:
            g = self.rng.standard_normal(n) * scale
            if spread:
                g = g * np.exp2(self.rng.integers(-spread, spread + 1, n))
            G.append(g.astype(np.float32))
        self.G = G
        self.g = [_placed(v, o[1]) for v, o in zip(G, self.offsets)]
        return G

    def groups(self):
        return _C.optim_tensors(self.p, self.g, self.m, self.e)

    def device_arrays(self):
        return ([t.cpu().numpy() for t in self.p], [t.cpu().numpy() for t in self.m],
                [t.cpu().numpy() for t in self.e] if self.e is not None else None)


def _scalar(value):
    return torch.tensor(float(value), dtype=torch.float32, device='cuda')


def _run_steps(case, steps, wd, scale, clip, omd):
    """`steps` steps on the device and in the checker; every array is compared after every step."""
    state = torch.zeros(4, dtype=torch.float32, device='cuda') if clip else None
    grad_scale = _scalar(scale) if scale else None
    found_inf = _scalar(0) if scale else None
    for t in range(steps):
        G = case.grads(scale or 1.0)
        groups = case.groups()
        norm = None
        if clip:
            _C.optim_grad_norm(groups, grad_scale, clip, state)
        _C.optim_sgd_step(groups, LR, MOMENTUM, wd, t == 0, omd, grad_scale, found_inf, state, device=torch.device('cuda', 0))
        if clip:
            norm, coef = (np.float32(v) for v in state[:2].cpu().numpy())
            want = R.grad_norm(G, scale)
            assert R.ulps_apart(norm, want) <= 1, (t, norm, want)
            assert R.same_bits(coef, R.clip_coef(norm, clip)), (t, coef)
        case.P, case.B, case.E, _, _ = R.step_all(case.P, G, case.B, case.E, LR, MOMENTUM, wd, omd, scale, clip, norm=norm)
        p, m, e = case.device_arrays()
        for i in range(len(case.numels)):
            what = (t, i, case.numels[i], case.offsets[i])
            assert R.same_bits(p[i], case.P[i]), ('param',) + what
            assert R.same_bits(m[i], case.B[i]), ('momentum',) + what
            if e is not None:
                assert R.same_bits(e[i], case.E[i]), ('ema',) + what


def _numels(count, with_empty=True):
    numels = [NUMELS[i % len(NUMELS)] for i in range(count)]
    if with_empty and count > 2:
        numels[count // 2] = 0
    return numels


@pytest.mark.parametrize('count', [1, 64, 65, 130])
def test_step_over_one_to_three_launches(count):
    """1, 64, 65 and 130 tensors = one, one, two and three launches, a zero-numel tensor among them, all options on."""
    case = Case(_numels(count), [(0, 0, 0, 0)] * count, 100 + count, True)
    case.grads()
    assert len(case.groups()) == (count + 63) // 64
    _run_steps(case, 3, 1e-4, 65536.0, 5.0, np.float32(1.0 - R.decay_at(0.99, 3)))


def test_step_at_every_alignment_of_the_four_arrays():
    """Each of param, grad, momentum and ema 0..3 floats behind a 16-byte boundary, independently: 256 tensors, the vector form
    (all four aligned), the element form and every mixture; sizes around the chunk so that both forms meet a partial vector."""
    offsets = list(itertools.product(range(4), repeat=4))
    numels = [[65, C + 1, 3, 2 * C + 5][i % 4] for i in range(len(offsets))]
    case = Case(numels, offsets, 7, True)
    _run_steps(case, 3, 1e-4, None, 5.0, np.float32(0.25))


@pytest.mark.parametrize('wd,ema,scale,clip', list(itertools.product([0.0, 1e-4], [False, True], [None, 65536.0], [None, 2.0])))
def test_step_option_matrix(wd, ema, scale, clip):
    case = Case(_numels(11), [(0, 0, 0, 0)] * 5 + [(1, 2, 3, 0)] * 6, 11, ema)
    _run_steps(case, 3, wd, scale, clip, np.float32(0.1))


@pytest.mark.parametrize('why', ['found_inf', 'nan_under_clipping'])
def test_skip_on_overflow_writes_nothing(why):
    case = Case(_numels(70), [(0, 0, 0, 0)] * 35 + [(0, 1, 0, 0)] * 35, 3, True)
    _run_steps(case, 1, 1e-4, None, None, np.float32(0.1))          # (momentum buffers that hold something)
    G = case.grads()
    state = None
    if why == 'nan_under_clipping':
        case.g[40][0] = float('nan')
        state = torch.zeros(4, dtype=torch.float32, device='cuda')
        _C.optim_grad_norm(case.groups(), None, 5.0, state)
    before = [[t.clone() for t in ts] for ts in (case.p, case.m, case.e)]
    _C.optim_sgd_step(case.groups(), LR, MOMENTUM, 1e-4, False, 0.1, None, _scalar(1) if why == 'found_inf' else _scalar(0), state,
                      device=torch.device('cuda', 0))
    if state is not None:
        assert math.isnan(float(state[0])) and int(state.view(torch.int32)[2]) == 1
    for olds, news in zip(before, (case.p, case.m, case.e)):
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(olds, news))


@pytest.mark.parametrize('scale', [None, 1024.0])
def test_norm_is_the_correctly_rounded_one(scale):
    """Values over 12 binades, tensors up to 2C + 5 elements, two launches + the finish: within 1 float32 ulp of
    sqrt(fsum of the exact squares) -- the squares are exact in double, the double sums err far below half a float32 ulp, only
    the final square root and cast can straddle a rounding boundary --, coef from the formula, the same bits on a second run."""
    count = 70
    case = Case(_numels(count), [(0, i % 4, 0, 0) for i in range(count)], 5, False)
    G = case.grads(scale or 1.0, spread=6)
    state = torch.zeros(2, 4, dtype=torch.float32, device='cuda')
    for run in range(2):
        _C.optim_grad_norm(case.groups(), _scalar(scale) if scale else None, 35.0, state[run])
    got = state.cpu().numpy()
    want = R.grad_norm(G, scale)
    print('norm: device %r, checker %r' % (got[0, 0], want))
    assert R.ulps_apart(got[0, 0], want) <= 1
    assert R.same_bits(got[0, 1], R.clip_coef(got[0, 0], 35.0)) and got[0, 1] < 1
    assert R.same_bits(got[0], got[1]) and got[0].view(np.uint32)[2] == 0
    # all-zero gradients: norm 0, coef 1
    for g in case.g:
        g.zero_()
    _C.optim_grad_norm(case.groups(), None, 35.0, state[0])
    assert state[0].cpu().numpy().view(np.uint32).tolist() == [0, np.float32(1).view(np.uint32), 0, 0]


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.b = torch.nn.Conv2d(8, 4, 3, padding=1)

    def forward(self, x):
        return self.b(torch.relu(self.a(x)))


def test_grad_scaler_hands_scale_and_found_inf_over():
    torch.manual_seed(0)
    net = _Net().cuda()
    opt = FusedSGD(net.parameters(), lr=LR, momentum=MOMENTUM, weight_decay=1e-4)
    ema = ModelEMA(net, 0.99)
    opt.bind_ema(ema)
    scaler = torch.amp.GradScaler('cuda', init_scale=1024.0)
    x = torch.randn(2, 3, 16, 16, device='cuda')
    params = list(net.parameters())
    P = [p.detach().cpu().numpy().copy() for p in params]
    E = [p.copy() for p in P]
    with torch.autocast('cuda', dtype=torch.float16):
        loss = net(x).float().pow(2).mean()
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
    assert not hasattr(opt, 'grad_scale') and scaler.get_scale() == 1024.0
    G = [p.grad.cpu().numpy() for p in params]                      # still scaled: nothing unscaled them in place
    P, B, E, _, _ = R.step_all(P, G, [None] * len(P), E, LR, MOMENTUM, 1e-4, np.float32(1.0 - R.decay_at(0.99, 0)), 1024.0)
    for i, p in enumerate(params):
        assert R.same_bits(p.detach().cpu().numpy(), P[i]) and R.same_bits(opt.state[p]['momentum_buffer'].cpu().numpy(), B[i])
        assert R.same_bits(ema.of(p).cpu().numpy(), E[i])
    assert ema.updates == 1
    # a forced inf loss: the weights stay, the scale halves
    before = [[t.detach().clone() for t in ts] for ts in (params, [opt.state[p]['momentum_buffer'] for p in params], [ema.of(p) for p in params])]
    opt.zero_grad(set_to_none=True)
    with torch.autocast('cuda', dtype=torch.float16):
        loss = net(x).float().pow(2).mean() * float('inf')
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == 512.0 and ema.updates == 2
    after = (params, [opt.state[p]['momentum_buffer'] for p in params], [ema.of(p) for p in params])
    for olds, news in zip(before, after):
        assert all(torch.equal(a.view(torch.int32), b.detach().view(torch.int32)) for a, b in zip(olds, news))


def _graph_node_types(graph):
    """hipGraphNodeType of every node of a captured torch graph (0 = kernel), through the HIP runtime the process has loaded."""
    path = [line.split()[-1] for line in open('/proc/self/maps') if 'libamdhip64' in line][0]
    hip = ctypes.CDLL(path)
    raw = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) == 0
    types = []
    for node in nodes:
        kind = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) == 0
        types.append(kind.value)
    return types


def test_norm_and_step_capture_into_a_graph_of_kernel_nodes():
    count = 70                                                       # two launches of each kernel + the finish
    numels = _numels(count)

    def fresh():
        case = Case(numels, [(0, 0, 0, 0)] * count, 21, True)
        case.grads(64.0)
        return case, torch.zeros(4, dtype=torch.float32, device='cuda')

    def enqueue(case, state, scale):
        groups = case.groups()
        _C.optim_grad_norm(groups, scale, 5.0, state)
        _C.optim_sgd_step(groups, LR, MOMENTUM, 1e-4, True, 0.1, scale, None, state, device=torch.device('cuda', 0))

    scale = _scalar(64.0)
    eager, eager_state = fresh()
    enqueue(eager, eager_state, scale)
    torch.cuda.synchronize()
    case, state = fresh()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        enqueue(case, state, scale)
    types = _graph_node_types(graph)
    assert len(types) == 5 and set(types) == {0}, types             # 2 norm walks + finish + 2 steps, kernels all
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(state.view(torch.int32), eager_state.view(torch.int32))
    for a, b in zip(eager.device_arrays(), case.device_arrays()):
        assert all(R.same_bits(x, y) for x, y in zip(a, b))


def test_trajectory_against_torch_sgd_clip_and_lerp():
    """20 steps of a two-layer conv net, clip + EMA: FusedSGD against torch.optim.SGD + clip_grad_norm_ + _foreach_lerp_ from the same
    start.  Closeness, not bits (torch's kernels may contract): the fused float32 trajectory lies no further from the same recipe
    in float64 than twice what torch's float32 trajectory does -- both are correctly ordered float32 evaluations of one formula."""
    torch.manual_seed(1)
    x = torch.randn(4, 3, 16, 16)
    start = _Net().state_dict()
    clip, decay, steps = 0.05, 0.99, 20

    def run(kind):
        dtype, device = (torch.float64, 'cpu') if kind == 'float64' else (torch.float32, 'cuda')
        net = _Net().to(dtype)
        net.load_state_dict({k: v.to(dtype) for k, v in start.items()})
        net = net.to(device)
        params = list(net.parameters())
        data = x.to(device=device, dtype=dtype)
        if kind == 'fused':
            opt = FusedSGD(params, lr=0.05, momentum=MOMENTUM, weight_decay=1e-4, max_norm=clip)
            ema = ModelEMA(net, decay)
            opt.bind_ema(ema)
        else:
            opt = torch.optim.SGD(params, lr=0.05, momentum=MOMENTUM, weight_decay=1e-4, **({'foreach': True} if device == 'cuda' else {}))
            shadow = [p.detach().clone() for p in params]
        norms = []
        for t in range(steps):
            opt.zero_grad(set_to_none=True)
            net(data).pow(2).mean().backward()
            if kind != 'fused':
                norms.append(float(torch.nn.utils.clip_grad_norm_(params, clip)))
            opt.step()
            if kind != 'fused':
                torch._foreach_lerp_(shadow, [p.detach() for p in params], 1.0 - R.decay_at(decay, t))
        if kind == 'fused':
            shadow = [ema.of(p) for p in params]
        return [t.detach().double().cpu() for t in params + shadow], norms

    exact, norms = run('float64')
    assert min(norms) > clip                                         # every step is clipped
    distance = {kind: max(float((a - b).abs().max()) for a, b in zip(run(kind)[0], exact)) for kind in ('torch', 'fused')}
    print('largest |float32 - float64| over weights and EMA after %d steps: torch %.3e, fused %.3e' % (steps, distance['torch'], distance['fused']))
    assert distance['fused'] <= 2 * distance['torch'], distance


def test_train_with_ema_and_clipping_then_infer_through_the_command_line(tmp_path, capsys, monkeypatch):
    tags = []
    real = train_module.ScalarLog.add_scalar
    monkeypatch.setattr(train_module.ScalarLog, 'add_scalar', lambda self, tag, value, it: (tags.append((tag, float(value))), real(self, tag, value, it))[1])
    path = str(tmp_path / 'tiny.pth')
    common = ['--annotations', ANN, '--images', DATA, '--backbone', 'ResNet18FPN', '--classes', '3', '--batch', '2',
              '--resize', '128', '--max-size', '160', '--jitter', '96', '128', '--warmup', '2', '--lr', '0.001', '--workers', '0']
    done, _ = cli.main(['train', path, '--iters', '6', '--ema', '0.99', '--clip-grad-norm', '35', '--logdir', str(tmp_path / 'log')] + common)
    out = capsys.readouterr().out
    assert done == 6 and '[6/6] focal loss:' in out and 'grad norm:' in out
    logged = dict(tags)
    assert all(math.isfinite(logged[k]) for k in ('focal_loss', 'box_loss', 'grad_norm')) and logged['grad_norm'] > 0
    model, state = Model.load(path)
    assert state['ema']['updates'] == 6 and state['iteration'] == 6
    checkpoint = torch.load(path, map_location='cpu')
    raw, averaged = checkpoint['state_dict'], checkpoint['ema']['state_dict']
    assert list(raw) == list(averaged) and not torch.equal(raw['cls_head.0.weight'], averaged['cls_head.0.weight'])

    # lift the class prior in both sets of weights: detections exist
    for weights in (checkpoint['state_dict'], checkpoint['ema']['state_dict']):
        weights['cls_head.8.bias'].fill_(0.0)
    lifted, only_ema = str(tmp_path / 'lifted.pth'), str(tmp_path / 'only_ema.pth')
    torch.save(checkpoint, lifted)
    torch.save({**{k: v for k, v in checkpoint.items() if k != 'ema'}, 'state_dict': checkpoint['ema']['state_dict']}, only_ema)
    found = {}
    # MIOpen's find mode may pick convolution kernels that do not reproduce from run to run (tests/test_gpu_graph.py): two runs on
    # the same weights are compared bit for bit here, so the comparison runs deterministic
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    for tag, file, extra in (('default', lifted, []), ('raw', lifted, ['--no-ema']), ('ema', only_ema, [])):
        out_file = str(tmp_path / (tag + '.json'))
        cli.main(['infer', file, '--images', DATA, '--annotations', ANN, '--output', out_file, '--batch', '2', '--resize', '128', '--max-size', '160',
                  '--workers', '0'] + extra)
        found[tag] = json.load(open(out_file))['annotations']
    text = capsys.readouterr().out
    assert 'averaged weights' in text and '--no-ema' in text
    assert len(found['default']) >= 5 and found['default'] == found['ema'] and found['default'] != found['raw']


def test_without_the_flags_the_optimizer_is_the_reference_one():
    def optimizer_of(**extra):
        model = Model('ResNet18FPN', classes=3)
        model.initialize(None)
        return train_module.prepare(model, torch.device('cuda', 0), **extra)[2]

    optimizer = optimizer_of()
    assert isinstance(optimizer, torch.optim.SGD) and not isinstance(optimizer, FusedSGD) and not hasattr(optimizer, 'ema')
    for extra in ({'ema_decay': 0.99}, {'clip_grad_norm': 35.0}, {'fused_step': True}):
        optimizer = optimizer_of(**extra)
        assert isinstance(optimizer, FusedSGD) and (optimizer.ema is not None) == ('ema_decay' in extra)
