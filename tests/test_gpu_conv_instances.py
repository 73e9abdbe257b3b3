"""Every instance of libodtk_conv.so (csrc/conv_ck.cpp) that can reach a problem, against an exact float64 reference.

An instance reaches a problem by the stopwatch, by adopt_sibling, as the first that fits under a stream capture, by
odtk_conv_plan_import from plans/*.json, or by ODTK_CONV_INSTANCE.  All five are right if and only if every instance that accepts
a problem computes it, so this file forces each one in turn (ODTK_CONV_INSTANCE) instead of testing what a stopwatch picked:

  * test_plan_named_instances_are_exact: each (class, instance) pair the committed plans name, at three small extents, with and
    without ReLU, bit for bit on integer-valued inputs, and within the two-roundings bound on real-valued ones;
  * test_every_supporting_instance_is_exact: all instances of the list on every class of the plans (and one more), both dtypes;
  * test_views_every_supporting_instance: the head-tower classes again through the views the engine uses.

The inputs (oracle/conv_exact.py) are small integers: every partial sum is exactly representable in bf16 / fp16 / fp32, so the
summation order, the CShuffle rounding and the epilogue's rounding change nothing and the comparison needs NO tolerance -- a
dropped tap, a wrong pad or a neighbour pixel read instead of padding moves an output by an integer.

The parser and generator tests run without a GPU.  Lines starting with `[conv-instances]` (run with -s) are the record behind
profiles/conv_instance_sweep.txt."""
import os
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]

from oracle import conv_exact as ce  # noqa: E402

gpu = pytest.mark.gpu

# (n, h, w) of the input.  13 x 20 at n = 2: 520 output pixels at stride 1 = more than one M tile of every instance plus a partial
# one.  7 x 11 at n = 3: odd extents, 231 pixels = one partial tile of the 256-row instances.  25 x 40 at n = 2: 2000 pixels, eight-odd
# tiles of the largest.  For the stride-2 classes these are INPUT extents: odd (13, 7, 11, 25) and even (20, 40) inputs both occur.
EXTENTS = [(2, 13, 20), (3, 7, 11), (2, 25, 40)]
SWEEP_EXTENTS = (2, 13, 20)
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
CODES = {torch.bfloat16: 1, torch.float16: 2}
EPS = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}

PLAN_PAIRS = ce.plan_pairs()
PLAN_CLASSES = ce.plan_classes()
SWEEP_CLASSES = PLAN_CLASSES + [c for c in ce.EXTRA_CLASSES if c not in PLAN_CLASSES]
TOWER_CLASSES = [(256, k, 3, 3, 1, 1, 1, 1, 1, 1) for k in (256, 36, 720)]


# ---- without a GPU: the parser and the generator -------------------------------------------------------------------------------

def test_parser_finds_the_conv_lines_of_every_plan():
    files = ce.plan_files()
    assert files, 'no plan file under plans/'
    for path in files:
        lines = ce.parse_conv_lines(path)
        assert lines, '%s: the parser found no conv line' % os.path.basename(path)
        import json
        with open(path) as f:
            raw = [s for s in json.load(f)['libraries'] if s.startswith('conv ')]
        assert len(lines) == len(raw)
        for line, text in zip(lines, raw):
            c, k, r, s, u, v, ph, pw, ph1, pw1 = line['cls']
            # the fields put back in export_plans' order give the line back: nothing was shifted or dropped
            again = 'conv %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s' % (
                line['dtype'], line['n'], c, line['h'], line['w'], k, r, s, u, v, ph, pw, ph1, pw1, line['index'], line['name'])
            assert again == text
            assert line['dtype'] in ce.DTYPE_CODES and line['index'] >= 0 and line['name'].startswith('DeviceGroupedConvFwd')
            assert min(c, k, r, s, u, v) >= 1 and min(ph, pw, ph1, pw1) >= 0
    assert len({key for key, _ in PLAN_PAIRS}) == len(PLAN_PAIRS) >= len(PLAN_CLASSES) >= 1


@pytest.mark.parametrize('cls', SWEEP_CLASSES, ids=ce.class_id)
def test_generator_stays_exact_for_every_class(cls):
    """The condition of the exact comparison, on the reference alone: integers, max |acc| and |acc + bias| <= 256, both sides of
    the ReLU present, and every weight position (c, r, s) non-zero for some output channel (no tap goes unobserved)."""
    for extents in EXTENTS:
        x, wt, bias, pre = ce.exact_problem(cls, extents)          # (asserts the bound itself)
        assert set(x.unique().tolist()) == {-1.0, 0.0, 1.0} and set(wt.unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert float(bias.abs().max()) <= 32 and bool((bias == bias.round()).all())
        assert bool((wt != 0).any(0).all()), 'a weight position is zero for every output channel'
        assert tuple(pre.shape) == (extents[0], cls[1]) + ce.out_extent(cls, *extents[1:])
        for dtype in DTYPES.values():                                # and the 16-bit types hold every value
            assert torch.equal(pre.to(dtype).double(), pre)


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------

def _to_device(t, dtype):
    """The upload of an activation / weight / bias (one place, so that a sensitivity run can corrupt it)."""
    t = t.to(dtype).cuda()
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t


_device_cache = {}


def _exact_on_device(cls, extents, dtype):
    """x, w, bias and the references with and without ReLU in `dtype` on the GPU, once per (class, extents, dtype)."""
    key = ('exact', cls, tuple(extents), dtype)
    if key not in _device_cache:
        x, wt, bias, pre = ce.exact_problem(cls, extents)
        zeros = float((pre <= 0).double().mean())
        assert 0.35 <= zeros <= 0.65 and bool((pre > 0).any()) and bool((pre <= 0).any())
        refs = {False: pre, True: pre.clamp(min=0)}
        for ref in refs.values():
            assert float(ref.abs().max()) <= ce.BOUND and torch.equal(ref.to(dtype).double(), ref)     # exact in the 16-bit type
        _device_cache[key] = (_to_device(x, dtype), _to_device(wt, dtype), _to_device(bias, dtype),
                              {relu: _to_device(ref, dtype) for relu, ref in refs.items()})
    return _device_cache[key]


def _conv(cls, x, w, b, relu, out=None):
    from odtk import _C
    u, v, ph, pw, ph1, pw1 = cls[4:]
    return _C.conv_bias_act(x, w, b, (u, v), ((ph, ph1), (pw, pw1)), relu, out=out)


_faulted = []


def _forced(monkeypatch, index, cls, x, w, b, relu, out=None):
    """The problem on instance `index` -> (y, name), or (None, None) when the instance declines (ODTK_ERR_UNSUPPORTED).  Any other
    error -- a HIP error above all -- propagates: nothing is retried."""
    from odtk import _C
    if _faulted:
        pytest.fail('an earlier forced launch of this session failed with %r: nothing more is launched' % _faulted[0])
    monkeypatch.setenv('ODTK_CONV_INSTANCE', str(index))
    try:
        y = _conv(cls, x, w, b, relu, out)
    except RuntimeError as e:
        if 'unsupported' in str(e).lower():
            return None, None
        _faulted.append('#%d on %s: %s' % (index, ce.class_id(cls), e))
        raise
    plan = _C.conv_last_plan()
    assert plan.startswith('#%d ' % index), 'instance #%d was forced, %r ran' % (index, plan)
    return y, plan.split(' ', 3)[-1]


def _bits_differ(got, ref):
    """None when `got` equals `ref` bit for bit (both of one 16-bit dtype), else (count, first (n, c, y, x), got, reference)."""
    if got.shape == ref.shape and torch.equal(got.view(torch.int16), ref.view(torch.int16)):
        return None
    assert got.shape == ref.shape, (got.shape, ref.shape)
    found = ce.first_difference(got.double().cpu(), ref.double().cpu())
    return found or (int((got.view(torch.int16) != ref.view(torch.int16)).sum()), 'sign of zero', -0.0, 0.0)


def _instance_count(dtype):
    from odtk import _C
    assert _C.conv_available(), 'libodtk_conv.so is missing on a GPU box: build it (make -C retinanet-examples_amd/csrc conv)'
    n = _C.conv_library().odtk_conv_instance_count(CODES[dtype])
    assert n > 0
    return n


_real_cache = {}


def _real_on_device(cls, extents, dtype):
    key = (cls, tuple(extents), dtype)
    if key not in _real_cache:
        x, wt, bias = ce.real_inputs(cls, extents, dtype)
        _, pre = ce.reference(cls, x, wt, bias)
        _real_cache[key] = (_to_device(x, dtype), _to_device(wt, dtype), _to_device(bias, dtype), pre.cuda(),
                            float(bias.float().abs().max()))
    return _real_cache[key]


@gpu
@pytest.mark.parametrize('pair', PLAN_PAIRS, ids=lambda p: '%s-#%d-%s' % (ce.class_id(p[0][0]), p[0][1], {1: 'bf16', 2: 'fp16'}[p[0][2]]))
def test_plan_named_instances_are_exact(monkeypatch, pair):
    """What bench.py pins.  No extents had to be replaced: every pair of the plan accepts all three reduced problems."""
    (cls, index, code), name = pair
    dtype = ce.DTYPE_CODES[code]
    assert index < _instance_count(dtype), 'the plan names instance #%d, this build has %d' % (index, _instance_count(dtype))
    failures = []
    for extents in EXTENTS:
        x, w, b, refs = _exact_on_device(cls, extents, dtype)
        for relu in (True, False):
            y, ran = _forced(monkeypatch, index, cls, x, w, b, relu)
            assert y is not None, '#%d declines %s at (n, h, w) = %s although the plan pins it for this class' % (index, ce.class_id(cls), extents)
            assert ran == name, ('the plan no longer fits the build -- bench.py would time instead of pinning: instance #%d is\n  %s\n'
                                 'the plan names\n  %s' % (index, ran, name))
            torch.cuda.synchronize()
            assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
            if relu:
                assert not bool((y < 0).any()), 'negative output under ReLU'
            bad = _bits_differ(y, refs[relu])
            if bad:
                failures.append('%s relu=%d: %d elements differ, first at (n, c, y, x) = %s: got %g, reference %g' % ((extents, relu) + bad))
        # the same pair on real-valued inputs: the two roundings to the 16-bit type, at the bound test_gpu_conv_library.py sets
        xr, wr, br, pre, bias_max = _real_on_device(cls, extents, dtype)
        for relu in (True, False):
            y, _ = _forced(monkeypatch, index, cls, xr, wr, br, relu)
            ref = pre.clamp(min=0) if relu else pre
            err = (y.double() - ref).abs()
            tol = EPS[dtype] * ref.abs() + EPS[dtype] * bias_max + 1e-3
            if not bool((err <= tol).all()):
                worst = int((err - tol).argmax())
                failures.append('%s relu=%d real-valued: excess %.3g at ref %.4g, got %.4g' % (
                    extents, relu, float((err - tol).flatten()[worst]), float(ref.flatten()[worst]), float(y.double().flatten()[worst])))
    assert not failures, '#%d %s on %s:\n  ' % (index, name, ce.class_id(cls)) + '\n  '.join(failures)


def _sweep(monkeypatch, cls, dtype, launch):
    """launch(index) -> None (declined) or (name, None or a difference).  Every instance of the list once; all failures together."""
    total = _instance_count(dtype)
    accepting, failures = [], []
    for index in range(total):
        result = launch(index)
        if result is None:
            continue
        accepting.append(index)
        name, bad = result
        if bad:
            failures.append('#%d %s: %d elements differ, first at (n, c, y, x) = %s: got %g, reference %g' % ((index, name) + tuple(bad)))
    torch.cuda.synchronize()
    return total, accepting, failures


@gpu
@pytest.mark.parametrize('dtype', list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize('cls', SWEEP_CLASSES, ids=ce.class_id)
def test_every_supporting_instance_is_exact(monkeypatch, cls, dtype):
    """adopt_sibling, the first fit under a capture and a stopwatch that picks differently on another box are all covered by this:
    whichever instance accepts the class must compute it."""
    t0 = time.perf_counter()
    x, w, b, refs = _exact_on_device(cls, SWEEP_EXTENTS, dtype)
    t1 = time.perf_counter()

    def launch(index):
        y, name = _forced(monkeypatch, index, cls, x, w, b, True)
        if y is None:
            return None
        bad = _bits_differ(y, refs[True])
        if not bad and bool((y < 0).any()):
            bad = (int((y < 0).sum()), 'negative under ReLU', float(y.min()), 0.0)
        return name, bad

    total, accepting, failures = _sweep(monkeypatch, cls, dtype, launch)
    t2 = time.perf_counter()
    print('\n[conv-instances] sweep %-26s %s: %3d of %d instances accept (n, h, w) = %s; reference %.2f s, %d forced launches %.2f s'
          % (ce.class_id(cls), {v: k for k, v in DTYPES.items()}[dtype], len(accepting), total, SWEEP_EXTENTS, t1 - t0, total, t2 - t1))
    assert not failures, '%d of %d accepting instances are wrong on %s:\n  ' % (len(failures), len(accepting), ce.class_id(cls)) + '\n  '.join(failures)
    assert accepting, 'no instance accepts %s in %s' % (ce.class_id(cls), dtype)
    named = sorted(i for (c, i, code), _ in PLAN_PAIRS if c == cls and ce.DTYPE_CODES[code] == dtype)
    assert set(named) <= set(accepting), 'the plan names %s for this class, of which %s decline' % (named, sorted(set(named) - set(accepting)))


@gpu
@pytest.mark.parametrize('view', ['x_rectangle', 'y_channel_slice'])
@pytest.mark.parametrize('dtype', list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize('cls', TOWER_CLASSES, ids=ce.class_id)
def test_views_every_supporting_instance(monkeypatch, cls, dtype, view):
    """The head-tower classes through the views the engine uses (include/odtk_conv_strided.h).
    x_rectangle: x is a 13 x 20 rectangle at an offset of a wider channels_last canvas whose every other element is 7, not 0 -- an
    instance that reads a neighbour where it should apply its own zero padding produces another integer.
    y_channel_slice: y is channels [8, 8 + c_out) of a wider buffer (a pixel stride above c_out); the slice must equal the
    reference and the sentinel around it must survive."""
    t0 = time.perf_counter()
    n, h, wd = SWEEP_EXTENTS
    x, w, b, refs = _exact_on_device(cls, SWEEP_EXTENTS, dtype)
    ref = refs[True]
    k = cls[1]
    if view == 'x_rectangle':
        y0, x0 = 5, 9
        canvas = torch.full((n, cls[0], 24, 40), 7.0, dtype=dtype, device='cuda').contiguous(memory_format=torch.channels_last)
        canvas[:, :, y0:y0 + h, x0:x0 + wd] = x
        before = canvas.clone()
        xin = canvas[:, :, y0:y0 + h, x0:x0 + wd]
        assert not xin.is_contiguous(memory_format=torch.channels_last) and torch.equal(xin, x)
        assert all(s % 8 == 0 for s in (xin.stride(0), xin.stride(2), xin.stride(3))) and xin.data_ptr() % 16 == 0

        def launch(index):
            y, name = _forced(monkeypatch, index, cls, xin, w, b, True)
            return None if y is None else (name, _bits_differ(y, ref))
    else:
        total_c = (k + 8 + 7) // 8 * 8 + 8
        sentinel = -3.0
        wide = torch.empty((n, total_c, h, wd), dtype=dtype, device='cuda').contiguous(memory_format=torch.channels_last)
        out = wide[:, 8:8 + k]
        assert out.stride(1) == 1 and out.stride(3) == total_c > k and out.data_ptr() % 16 == 0

        def launch(index):
            wide.fill_(sentinel)
            y, name = _forced(monkeypatch, index, cls, x, w, b, True, out=out)
            if y is None:
                return None
            bad = _bits_differ(out, ref)
            if not bad and not (bool((wide[:, :8] == sentinel).all()) and bool((wide[:, 8 + k:] == sentinel).all())):
                outside = torch.ones_like(wide, dtype=torch.bool)
                outside[:, 8:8 + k] = False
                hit = (wide != sentinel) & outside
                at = tuple(int(i) for i in hit.nonzero()[0])
                bad = (int(hit.sum()), 'outside the slice, buffer ' + str(at), float(wide[at]), sentinel)
            return name, bad

    total, accepting, failures = _sweep(monkeypatch, cls, dtype, launch)
    if view == 'x_rectangle':
        assert torch.equal(canvas, before), 'the input canvas was written to'
    print('\n[conv-instances] %-15s %-20s %s: %3d of %d instances accept; %.2f s'
          % (view, ce.class_id(cls), {v: kk for kk, v in DTYPES.items()}[dtype], len(accepting), total, time.perf_counter() - t0))
    assert not failures, '%d of %d accepting instances are wrong on %s as %s:\n  ' % (
        len(failures), len(accepting), ce.class_id(cls), view) + '\n  '.join(failures)
    assert accepting, 'no instance accepts %s in %s through the view' % (ce.class_id(cls), dtype)
