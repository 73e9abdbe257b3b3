"""Every hipBLASLt solution that can reach a problem of odtk_gemm_bias_act (csrc/gemm_lt.hpp), against an exact float64 reference.

Which solution computes a 1x1 convolution is decided at run time: the fastest of the heuristic's candidates by a stopwatch, the one
a `gemm` line of plans/*.json names, or the first usable one when the shape is first seen under a stream capture.  All three are
right if and only if every candidate that can reach a problem computes it, so this file forces each candidate in turn
(odtk_gemm_plan_clear + odtk_gemm_plan_import of one line; odtk_debug_gemm_candidates lists them, odtk_gemm_last_solution says what
ran) instead of testing what a stopwatch picked:

  * test_every_offered_solution_is_exact: every candidate of every class x dtype at m = 1, 231, 2039, with and without ReLU and
    residual, bit for bit on integer-valued inputs; the plan-cache hit gives the same bits;
  * test_plan_named_solutions_are_exact: every `gemm` line of the committed plans on its own solution, at the smallest multiple
    2039 * 2^j of the period at which the heuristic still offers it (else at the line's own m);
  * test_every_offered_solution_on_real_values: every candidate against float64 at the bound of an fp32 sum in any order;
  * test_selection_paths: the stopwatch, a pin that misses, and a first call under a capture;
  * test_comparison_notices_one_wrong_element: the comparison is not vacuous.

The inputs (oracle/gemm_exact.py) are small integers: every partial sum and every stage of the epilogue is exactly representable in
bf16 / fp16 / fp32, so the comparison needs NO tolerance.  The parser and generator tests run without a GPU.  Lines starting with
`[gemm-solutions]` (run with -s) are the record behind profiles/gemm_solution_sweep.txt."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]

from oracle import gemm_exact as ge  # noqa: E402

gpu = pytest.mark.gpu

# m = 1: the 1 x 1 P7 level of one small image.  231: one partial tile of a 256-row macro tile.  2039: a prime -- several whole
# tiles plus a partial one for every tile height up to 256.
M_SIZES = [1, 231, 2039]
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
NAMES = {v: k for k, v in DTYPES.items()}
CODES = {v: k for k, v in ge.DTYPE_CODES.items()}
INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
UNIT = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12, torch.float32: 2.0 ** -24}       # u_T: 2 u_T |v| bounds one rounding of v to T
WORKSPACE_BYTES = 32 << 20                      # what odtk/_C.py: gemm_bias_act passes
GUARD = 4096                                    # elements before and after y that must keep the sentinel
SENTINEL = -1024.0                              # exact in every dtype, outside the exact problems' range of +-256
OK, ERR_UNSUPPORTED = 0, -4

CLASSES = ge.classes()
PLAN_LINES = ge.plan_lines()


# ---- without a GPU: the parser and the generator -------------------------------------------------------------------------------

def test_parser_finds_the_gemm_lines_of_every_plan():
    import json
    from oracle import conv_exact as ce
    files = ce.plan_files()
    assert files, 'no plan file under plans/'
    for path in files:
        lines = ge.parse_gemm_lines(path)
        assert lines, '%s: the parser found no gemm line' % os.path.basename(path)
        with open(path) as f:
            raw = [s for s in json.load(f)['libraries'] if s.startswith('gemm ')]
        assert len(lines) == len(raw)
        for line, text in zip(lines, raw):
            # the fields put back in plan_export's order give the line back: nothing was shifted or dropped
            assert ge.format_line(line['m'], line['n'], line['k'], line['dtype'], line['relu'], line['residual'], line['index']) == text
            assert line['dtype'] in ge.DTYPE_CODES and line['relu'] in (0, 1) and line['residual'] in (0, 1)
            assert min(line['m'], line['n'], line['k']) >= 1 and line['index'] >= 0 and line['cls'] == (line['n'], line['k'])
    # ... and that order is the one plan_export prints and plan_import scans (csrc/gemm_lt.hpp)
    source = open(os.path.join(ROOT, 'retinanet-examples_amd', 'csrc', 'gemm_lt.hpp')).read()
    printed = re.search(r'snprintf\(line, sizeof line, "(gemm [^"\\]*)\\n",\s*static_cast<unsigned long long>\(std::get<0>\(kv\.first\)\),'
                        r'\s*std::get<1>\(kv\.first\), std::get<2>\(kv\.first\), std::get<3>\(kv\.first\), std::get<4>\(kv\.first\), '
                        r'std::get<5>\(kv\.first\),\s*kv\.second\)', source)
    assert printed, 'plan_export no longer prints the PinKey (m, n, k, dtype, relu, residual) followed by the solution index'
    assert re.sub(r'%(llu|u)', '%d', printed.group(1)) == ge.LINE_FORMAT
    assert 'sscanf(p, "%s", &m, &n, &k, &dtype, &relu, &res, &idx)' % printed.group(1) in source
    assert 'using PinKey = std::tuple<uint64_t, uint32_t, uint32_t, int, int, int>;      // m, n, k, dtype, relu, residual' in source
    assert len(ge.plan_classes()) >= 1 and set(ge.EXTRA_CLASSES) <= set(CLASSES) and len(set(CLASSES)) == len(CLASSES)


@pytest.mark.parametrize('cls', CLASSES, ids=ge.class_id)
def test_generator_stays_exact_for_every_class(cls):
    """The condition of the exact comparison, on the reference alone: integers of magnitude <= 256 at every stage, the ReLU clamps a
    share in [0.35, 0.65] (m >= 231; both sides present at m = 1), every weight position is non-zero for some output channel, and
    every dtype holds every value."""
    n, k = cls
    for m in M_SIZES:
        x, wt, bias, residual, refs = ge.exact_problem(cls, m)                 # (asserts the bound itself)
        worst, low, high = ge.check_generator_bound(refs, m)
        assert worst <= ge.BOUND and (m < 231 or 0.35 <= low <= high <= 0.65)
        assert tuple(x.shape) == (m, k) and tuple(wt.shape) == (n, k) and tuple(bias.shape) == (n,) and tuple(residual.shape) == (m, n)
        assert set(x.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(wt.unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert m == 1 or set(x.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert float(bias.abs().max()) <= 32 and bool((bias == bias.round()).all())
        assert float(residual.abs().max()) <= 16 and bool((residual == residual.round()).all())
        assert bool((wt != 0).any(0).all()), 'a weight position is zero for every output channel'
        for pair in refs.values():
            for ref in pair.values():
                assert tuple(ref.shape) == (m, n)
                for dtype in DTYPES.values():
                    assert torch.equal(ref.to(dtype).double(), ref)


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------

class _Problem:
    """One problem on the device: x [m, k], w [n, k], bias float32 [n], residual [m, n] and, per (relu, residual), the reference
    in `dtype`: [m, n], or one period of it ([2039, n]) when x and the residual repeat with that period."""

    def __init__(self, cls, m, dtype, x, w, bias, residual, refs):
        self.cls, self.m, self.dtype, self.x, self.w, self.bias, self.residual, self.refs = cls, m, dtype, x, w, bias, residual, refs
        self.n, self.k = cls


_device_cache = {}
_stats = {'pairs': 0, 'indices': set()}
_faulted = []
_workspace = []


def _lib():
    from odtk import _C
    assert _C.gemm_available(), 'hipBLASLt could not be bound on a GPU box'
    return _C.library()


def _exact_on_device(cls, m, dtype):
    key = ('exact', cls, m, dtype)
    if key not in _device_cache:
        x, wt, bias, residual, refs = ge.exact_problem(cls, m)
        on_device = {}
        for relu in (False, True):
            for with_res in (False, True):
                ref = refs['residual' if with_res else 'bias'][relu]
                assert float(ref.abs().max()) <= ge.BOUND and torch.equal(ref.to(dtype).double(), ref)        # rounding once changes nothing
                on_device[(relu, with_res)] = ref.to(dtype).cuda()
        _device_cache[key] = _Problem(cls, m, dtype, x.to(dtype).cuda(), wt.to(dtype).cuda(), bias.float().cuda(),
                                      residual.to(dtype).cuda(), on_device)
    return _device_cache[key]


def _candidates(m, n, k, dtype, relu, with_res):
    """The solution indices a plan for the problem chooses from, in heuristic order (host only)."""
    lib = _lib()
    out = (ctypes.c_int * 16)()
    count = lib.odtk_debug_gemm_candidates(m, n, k, CODES[dtype], int(relu), int(with_res), WORKSPACE_BYTES, out, 16)
    assert 0 <= count <= 16, 'odtk_debug_gemm_candidates returned %d' % count
    assert lib.odtk_debug_gemm_candidates(m, n, k, CODES[dtype], int(relu), int(with_res), WORKSPACE_BYTES, None, 0) == count
    found = list(out[:count])
    assert len(set(found)) == len(found), 'the heuristic offers a solution twice: %s' % found
    return found


def _fresh_output(prob):
    """y [m, n], NaN-filled, inside a larger buffer that holds the sentinel."""
    size = prob.m * prob.n
    buf = torch.full((GUARD + size + GUARD,), SENTINEL, dtype=prob.dtype, device='cuda')
    y = buf[GUARD:GUARD + size].view(prob.m, prob.n)
    y.fill_(float('nan'))
    assert y.data_ptr() % 16 == 0
    return buf, y


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _call(prob, y, relu, with_res, w=None, bias=None, residual=None):
    """odtk_gemm_bias_act through the C ABI on the current stream -> its return code."""
    lib = _lib()
    if not _workspace:
        _workspace.append(torch.empty(WORKSPACE_BYTES, dtype=torch.uint8, device='cuda'))
    ws = _workspace[0]
    w = prob.w if w is None else w
    bias = prob.bias if bias is None else bias
    residual = prob.residual if residual is None else residual
    assert tuple(residual.shape) == (prob.m, prob.n) and tuple(prob.x.shape) == (prob.m, prob.k) and tuple(w.shape) == (prob.n, prob.k)
    assert all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (prob.x, w, bias, residual, y))
    return lib.odtk_gemm_bias_act(y.data_ptr(), prob.x.data_ptr(), w.data_ptr(), bias.data_ptr(),
                                  residual.data_ptr() if with_res else None, prob.m, prob.n, prob.k, CODES[prob.dtype], int(relu),
                                  ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)


def _launched(prob, relu, with_res, what, **other):
    """One eager call into a fresh output -> (buf, y), or None when the library declines (ODTK_ERR_UNSUPPORTED).  Any other error
    -- a HIP error above all -- is remembered and propagates: nothing more is launched in the session."""
    if _faulted:
        pytest.fail('an earlier launch of this session failed with %r: nothing more is launched' % _faulted[0])
    buf, y = _fresh_output(prob)
    try:
        rc = _call(prob, y, relu, with_res, **other)
        if rc == ERR_UNSUPPORTED:
            return None
        if rc != OK:
            raise RuntimeError('odtk_gemm_bias_act returned %d' % rc)
        torch.cuda.synchronize()
    except RuntimeError as e:
        _faulted.append('%s: %s' % (what, e))
        raise
    return buf, y


def _forced(index, prob, relu, with_res, **other):
    """The problem on solution `index`: plan_clear -> import one line -> call -> (buf, y), or None when the library declines."""
    from odtk import _C
    lib = _lib()
    _C.gemm_plan_clear()
    line = ge.format_line(prob.m, prob.n, prob.k, CODES[prob.dtype], relu, with_res, index)
    assert lib.odtk_gemm_plan_import((line + '\n').encode()) == 1
    out = _launched(prob, relu, with_res, 'solution %d forced by %r' % (index, line), **other)
    if out is None:
        return None
    assert _C.gemm_last_solution() == (index, 'pinned'), 'solution %d was forced, %s ran' % (index, _C.gemm_last_solution())
    assert _C.gemm_plan_pin_misses() == 0
    _stats['pairs'] += 1
    _stats['indices'].add(index)
    return out


def _bits_differ(got, ref):
    """None when `got` [m, n] equals `ref` bit for bit (one dtype; 16-bit types as int16, fp32 as int32), else (number of differing
    elements, first differing (row, channel), got there, reference there).  A `ref` of fewer rows is periodic: got[r] must equal
    ref[r mod period]."""
    assert got.dtype == ref.dtype and got.dim() == 2 and got.shape[1] == ref.shape[1], (got.shape, ref.shape)
    as_int = INT_VIEW[got.dtype]
    m, period = got.shape[0], ref.shape[0]
    whole, rest = divmod(m, period)
    if m == period:
        same = torch.equal(got.view(as_int), ref.view(as_int))
    else:
        assert m > period
        head = got[:whole * period].view(whole, period, -1).view(as_int) == ref.view(as_int)[None]
        same = bool(head.all()) and torch.equal(got[whole * period:].view(as_int), ref[:rest].view(as_int))
    if same:
        return None
    full = ref if m == period else torch.cat([ref.repeat(whole, 1), ref[:rest]])
    diff = (got.view(as_int) != full.view(as_int)).flatten()
    row, channel = divmod(int(diff.nonzero()[0]), got.shape[1])
    return int(diff.sum()), (row, channel), float(got[row, channel]), float(full[row, channel])


def _report(cls, dtype, m, relu, with_res, index, bad):
    return '%s %s m=%d relu=%d residual=%d solution %d: %d elements differ, first at (row, channel) = %s: got %r, want %r' % (
        (ge.class_id(cls), NAMES[dtype], m, relu, with_res, index) + tuple(bad))


def _print_totals(with_indices=False):
    text = '[gemm-solutions] so far in this session: %d (problem, solution) pairs forced, %d distinct solution indices' % (
        _stats['pairs'], len(_stats['indices']))
    if with_indices:                                                           # as ranges: 618384-618392 618396 ...
        runs = []
        for index in sorted(_stats['indices']):
            if runs and index == runs[-1][1] + 1:
                runs[-1][1] = index
            else:
                runs.append([index, index])
        text += ': ' + ' '.join('%d' % a if a == b else '%d-%d' % (a, b) for a, b in runs)
    print(text)


@gpu
@pytest.mark.parametrize('dtype', list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize('cls', CLASSES, ids=ge.class_id)
def test_every_offered_solution_is_exact(cls, dtype):
    """The stopwatch on another box, a plan from another run and the first fit under a capture are all covered by this: whichever
    candidate the heuristic offers for the problem must compute it."""
    n, k = cls
    failures = []
    for m in M_SIZES:
        prob = _exact_on_device(cls, m, dtype)
        listed = {}
        for relu in (True, False):
            for with_res in (False, True):
                found = _candidates(m, n, k, dtype, relu, with_res)
                assert found, 'the heuristic offers nothing for %s %s m=%d relu=%d residual=%d' % (ge.class_id(cls), NAMES[dtype], m, relu, with_res)
                listed[(int(relu), int(with_res))] = found
                ref = prob.refs[(relu, with_res)]
                for index in found:
                    out = _forced(index, prob, relu, with_res)
                    if out is None:
                        failures.append('%s %s m=%d relu=%d residual=%d solution %d: offered, then declined' % (
                            ge.class_id(cls), NAMES[dtype], m, relu, with_res, index))
                        continue
                    buf, y = out
                    bad = _bits_differ(y, ref)
                    if bad:
                        failures.append(_report(cls, dtype, m, relu, with_res, index, bad))
                    if not _guards_intact(buf):
                        failures.append('%s %s m=%d relu=%d residual=%d solution %d: wrote outside y' % (
                            ge.class_id(cls), NAMES[dtype], m, relu, with_res, index))
                    from odtk import _C
                    again = _launched(prob, relu, with_res, 'solution %d, plan-cache hit' % index)           # no clear, no import
                    assert again is not None and _C.gemm_last_solution() == (index, 'pinned')
                    if not torch.equal(again[1].view(INT_VIEW[dtype]), y.view(INT_VIEW[dtype])) or not _guards_intact(again[0]):
                        failures.append('%s %s m=%d relu=%d residual=%d solution %d: the plan-cache hit gives other bits' % (
                            ge.class_id(cls), NAMES[dtype], m, relu, with_res, index))
        if len({tuple(v) for v in listed.values()}) == 1:
            print('\n[gemm-solutions] %-10s %s m=%-4d (relu, residual) any  : %s' % (ge.class_id(cls), NAMES[dtype], m, listed[(1, 0)]), end='')
        else:
            for (relu, with_res), found in sorted(listed.items()):
                print('\n[gemm-solutions] %-10s %s m=%-4d (relu, residual) (%d, %d): %s' % (ge.class_id(cls), NAMES[dtype], m, relu, with_res, found), end='')
    print()
    assert not failures, '%d wrong results on %s %s:\n  ' % (len(failures), ge.class_id(cls), NAMES[dtype]) + '\n  '.join(failures)


def _periodic_on_device(base, m):
    """`base` (PERIOD rows) repeated to m rows on the device; the references stay those of one period."""
    whole, rest = divmod(m, ge.PERIOD)
    if (whole, rest) == (1, 0):
        return base
    grow = lambda t: torch.cat([t.repeat(whole, 1), t[:rest]]).contiguous()
    return _Problem(base.cls, m, base.dtype, grow(base.x), base.w, base.bias, grow(base.residual), base.refs)


@gpu
@pytest.mark.parametrize('line', PLAN_LINES, ids=lambda l: '%s-m%d-r%d%d-#%d' % (ge.class_id(l['cls']), l['m'], l['relu'], l['residual'], l['index']))
def test_plan_named_solutions_are_exact(line):
    """What bench.py pins: every `gemm` line of the committed plans on the solution it names, at its own dtype, relu and residual.
    Above 2039 rows the activation and the residual repeat with period 2039 (2039 * 256 > 512 000: no two rows that a power-of-two
    tile could confuse are equal by construction), so the exact reference is the 2039-row reference repeated."""
    cls, dtype, index = line['cls'], ge.DTYPE_CODES[line['dtype']], line['index']
    n, k = cls
    relu, with_res = bool(line['relu']), bool(line['residual'])
    at_own = _candidates(line['m'], n, k, dtype, relu, with_res)
    assert index in at_own, ('the plan no longer fits the library -- bench.py would time instead of pinning: %r names solution %d, the '
                             'heuristic offers %s' % (ge.format_line(line['m'], n, k, line['dtype'], relu, with_res, index), index, at_own))
    m = line['m']
    reduced = ge.PERIOD
    while reduced <= line['m']:
        if index in _candidates(reduced, n, k, dtype, relu, with_res):
            m = reduced
            break
        reduced *= 2
    print('\n[gemm-solutions] plan line %-36r runs at m = %d%s' % (
        ge.format_line(line['m'], n, k, line['dtype'], relu, with_res, index), m, '' if m != line['m'] else ' (its own)'))
    prob = _periodic_on_device(_exact_on_device(cls, ge.PERIOD, dtype), m)
    out = _forced(index, prob, relu, with_res)
    assert out is not None, 'solution %d declines the problem although the heuristic offers it' % index
    buf, y = out
    bad = _bits_differ(y, prob.refs[(relu, with_res)])
    assert not bad, _report(cls, dtype, m, relu, with_res, index, bad)
    assert _guards_intact(buf), 'solution %d wrote outside y' % index


_real_cache = {}


def _real_on_device(cls, m, dtype):
    """Real-valued inputs on the device, the float64 reference with residual and ReLU, and the bound
    2 u |ref| + 2 (k + 2) 2^-24 S with S = sum |x w| + |bias| + |residual|: the standard bound of an fp32 sum of k + 2 terms in any
    order ((k + 2) 2^-24 S, to first order) followed by one rounding to the output type (u |ref|), doubled."""
    key = (cls, m, dtype)
    if key not in _real_cache:
        x, wt, bias, residual = ge.real_inputs(cls, m, dtype)
        ref = ge.references(x, wt, bias, residual)['residual'][True]
        scale = ge.magnitude_sum(x, wt, bias, residual)
        bound = 2.0 * UNIT[dtype] * ref.abs() + 2.0 * (cls[1] + 2) * 2.0 ** -24 * scale
        prob = _Problem(cls, m, dtype, x.cuda(), wt.cuda(), bias.float().cuda(), residual.cuda(), {})
        _real_cache[key] = (prob, ref.cuda(), bound.cuda())
    return _real_cache[key]


@gpu
@pytest.mark.parametrize('dtype', list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize('cls', CLASSES, ids=ge.class_id)
def test_every_offered_solution_on_real_values(cls, dtype):
    """Each candidate once at m = 2039 with ReLU and residual against float64: the accumulation is an fp32 sum (in whatever order)
    rounded once.  Nobody has widened this bound to fit; the worst ratio of error to bound is printed."""
    n, k = cls
    m = ge.PERIOD
    prob, ref, bound = _real_on_device(cls, m, dtype)
    found = _candidates(m, n, k, dtype, True, True)
    assert found
    failures, worst = [], (0.0, None)
    for index in found:
        out = _forced(index, prob, True, True)
        if out is None:
            failures.append('solution %d: offered, then declined' % index)
            continue
        buf, y = out
        err = (y.double() - ref).abs()
        ratio = float((err / bound).nan_to_num(nan=float('inf')).max())
        worst = max(worst, (ratio, index))
        if not bool((err <= bound).all()) or not _guards_intact(buf):
            at = int((err / bound).nan_to_num(nan=float('inf')).argmax())
            failures.append('solution %d: error / bound = %.3g at (row, channel) = %s: got %r, reference %r, bound %.3g%s' % (
                index, ratio, divmod(at, n), float(y.flatten()[at]), float(ref.flatten()[at]), float(bound.flatten()[at]),
                '' if _guards_intact(buf) else '; wrote outside y'))
    print('\n[gemm-solutions] real values %-10s %s m=%d: %d candidates, worst error / bound = %.3f (solution %s)'
          % (ge.class_id(cls), NAMES[dtype], m, len(found), worst[0], worst[1]))
    assert not failures, '%s %s m=%d on real values:\n  ' % (ge.class_id(cls), NAMES[dtype], m) + '\n  '.join(failures)


def _assert_exact(prob, out, relu, with_res, what):
    assert out is not None, what + ': declined'
    buf, y = out
    bad = _bits_differ(y, prob.refs[(relu, with_res)])
    assert not bad, what + ': ' + _report(prob.cls, prob.dtype, prob.m, relu, with_res, -1, bad)
    assert _guards_intact(buf), what + ': wrote outside y'


@gpu
def test_selection_paths():
    """The three ways a production call selects, on problems no other test of the file uses (m = 509, 523, 541)."""
    from odtk import _C
    lib = _lib()
    dtype, relu, with_res = torch.bfloat16, True, True
    # (a) no pin: the stopwatch
    prob = _exact_on_device((256, 64), 509, dtype)
    found = _candidates(prob.m, prob.n, prob.k, dtype, relu, with_res)
    _C.gemm_plan_clear()
    out = _launched(prob, relu, with_res, 'timed')
    index, origin = _C.gemm_last_solution()
    assert origin == 'timed' and index in found and _C.gemm_plan_pin_misses() == 0, (index, origin, found)
    _assert_exact(prob, out, relu, with_res, '(a) timed, solution %d' % index)
    # (b) a pin the heuristic does not offer: one miss, then the stopwatch
    prob = _exact_on_device((64, 256), 523, dtype)
    found = _candidates(prob.m, prob.n, prob.k, dtype, relu, with_res)
    absent = 7
    while absent in found:
        absent += 1
    _C.gemm_plan_clear()
    assert lib.odtk_gemm_plan_import((ge.format_line(prob.m, prob.n, prob.k, CODES[dtype], relu, with_res, absent) + '\n').encode()) == 1
    out = _launched(prob, relu, with_res, 'pin miss')
    index, origin = _C.gemm_last_solution()
    assert origin == 'timed' and index in found and _C.gemm_plan_pin_misses() == 1, (index, origin, found, _C.gemm_plan_pin_misses())
    _assert_exact(prob, out, relu, with_res, '(b) after a pin miss, solution %d' % index)
    # (c) first seen inside a capture: the first usable candidate, not remembered as tuned
    prob = _exact_on_device((512, 128), 541, dtype)
    found = _candidates(prob.m, prob.n, prob.k, dtype, relu, with_res)
    _C.gemm_plan_clear()
    if _faulted:
        pytest.fail('an earlier launch of this session failed with %r: nothing more is launched' % _faulted[0])
    buf, y = _fresh_output(prob)
    assert _workspace                                                          # (the library's scratch exists before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):                                          # (captures on a side stream)
            rc = _call(prob, y, relu, with_res)
        assert rc == OK, rc
        assert _C.gemm_last_solution() == (found[0], 'capture'), (_C.gemm_last_solution(), found)

        def replay(what):
            buf.fill_(SENTINEL)
            y.fill_(float('nan'))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            _assert_exact(prob, (buf, y), relu, with_res, what)
        replay('(c) replay of the capture, solution %d' % found[0])
        out = _launched(prob, relu, with_res, 'eager after the capture')
        index, origin = _C.gemm_last_solution()
        assert origin == 'timed' and index in found, (index, origin, found)
        _assert_exact(prob, out, relu, with_res, '(c) eager call after the capture, solution %d' % index)
        replay('(c) replay after the eager call')
    except RuntimeError as e:
        _faulted.append('capture: %s' % e)
        raise
    finally:
        del graph
    print('\n[gemm-solutions] selection paths: timed, pin miss -> timed, capture -> %d = candidates[0] -> timed %d' % (found[0], index))


@gpu
def test_comparison_notices_one_wrong_element():
    """The comparison helper on a GEMM whose input differs from the reference's in ONE element: a flipped weight moves the rows whose
    activation at that channel is non-zero, a changed bias entry a whole channel, a changed residual element exactly one output."""
    cls, m, dtype, relu, with_res = (24, 40), 231, torch.bfloat16, False, True
    prob = _exact_on_device(cls, m, dtype)
    ref = prob.refs[(relu, with_res)]
    index = _candidates(m, cls[0], cls[1], dtype, relu, with_res)[0]
    buf, y = _forced(index, prob, relu, with_res)
    assert _bits_differ(y, ref) is None
    o, c, row = 17, 33, 200
    w = prob.w.clone()
    w[o, c] = 1.0 if float(w[o, c]) == 0.0 else -float(w[o, c])
    touched = int((prob.x[:, c] != 0).sum())
    assert 0 < touched < m
    bad = _bits_differ(_forced(index, prob, relu, with_res, w=w)[1], ref)
    assert bad and bad[0] == touched and bad[1][1] == o, bad
    bias = prob.bias.clone()
    bias[o] += 1.0
    bad = _bits_differ(_forced(index, prob, relu, with_res, bias=bias)[1], ref)
    assert bad and bad[0] == m and bad[1] == (0, o) and bad[2] == bad[3] + 1.0, bad
    residual = prob.residual.clone()
    residual[row, o] += 1.0
    bad = _bits_differ(_forced(index, prob, relu, with_res, residual=residual)[1], ref)
    assert bad and bad[0] == 1 and bad[1] == (row, o) and bad[2] == bad[3] + 1.0, bad
    # ... and a sign of zero or an unwritten element (NaN) is a difference too
    other = ref.clone()
    other[3, 5] = float('nan')
    assert _bits_differ(other, ref)[:2] == (1, (3, 5))
    zero = torch.zeros(2, 8, dtype=dtype, device='cuda')
    assert _bits_differ(-zero, zero)[0] == 16
    print()
    _print_totals(with_indices=True)
