"""Exact problems for odtk_gemm_bias_act (csrc/gemm_lt.hpp: the 1x1 convolutions on hipBLASLt), shared by
tests/test_gpu_gemm_solutions.py and any probe.  Pure CPU: nothing here touches the GPU or the library.

    y[p][o] = act( sum_c x[p][c] * w[o][c] + bias[o] (+ residual[p][o]) )          x [m, k], w [n, k], y / residual [m, n]

A class is (n, k) = (output channels, input channels).  The inputs are oracle/conv_exact.py's for the 1x1 convolution class
(k, n, 1, 1, 1, 1, 0, 0, 0, 0) at the extents (1, 1, m): x in {-1, 0, 1}, w sparse +-1 (at most ~1024 non-zero products per
output), the bias an integer in [-32, 32]; the residual is an integer in [-16, 16].  Every product, every partial sum and every
stage of the epilogue is then an integer of magnitude <= 256: exact in bf16 (8 significant bits), fp16, fp32 and the fp32
accumulator in any order of summation, so a correct solution EQUALS the float64 reference rounded to the dtype, bit for bit.  A bias
applied along the wrong axis, a beta * C that reads another buffer or a wrong row in a partial tile moves an output by an integer."""
import json
import os

import torch

from oracle import conv_exact as ce

BOUND = ce.BOUND
DTYPE_CODES = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}     # include/odtk_hip.h: ODTK_F32, ODTK_BF16, ODTK_F16
EXTRA_CLASSES = [(24, 40)]                       # no multiple of any tile: the odd case of tests/test_gpu_fused.py
PERIOD = 2039                                    # a prime: the row count the large problems repeat with
LINE_FORMAT = 'gemm %d %d %d %d %d %d %d'        # plan_export (csrc/gemm_lt.hpp): m n k dtype relu residual solution-index


def parse_gemm_lines(path):
    """The `gemm` lines of a plan file's "libraries" list, in the field order of plan_export (csrc/gemm_lt.hpp):
    gemm m n k dtype relu residual solution-index   ->  list of dicts."""
    with open(path) as f:
        plan = json.load(f)
    out = []
    for line in plan.get('libraries', []):
        tok = line.split(' ')
        if tok[0] != 'gemm':
            continue
        if len(tok) != 8:
            raise ValueError('%s: malformed gemm line %r' % (path, line))
        m, n, k, dtype, relu, residual, index = (int(t) for t in tok[1:])
        out.append({'plan': os.path.basename(path), 'm': m, 'n': n, 'k': k, 'dtype': dtype, 'relu': relu, 'residual': residual,
                    'index': index, 'cls': (n, k)})
    return out


def format_line(m, n, k, dtype, relu, residual, index):
    """One line as plan_export writes it and plan_import reads it."""
    return LINE_FORMAT % (m, n, k, dtype, 1 if relu else 0, 1 if residual else 0, index)


def plan_lines():
    return [line for path in ce.plan_files() for line in parse_gemm_lines(path)]


def plan_classes():
    """Distinct (n, k) of the committed plans, sorted."""
    return sorted({line['cls'] for line in plan_lines()})


def classes():
    """The plan classes and the extra ones: what the solution sweep runs."""
    found = plan_classes()
    return found + [c for c in EXTRA_CLASSES if c not in found]


def class_id(cls):
    return '%dto%d' % (cls[1], cls[0])


def conv_class(cls):
    n, k = cls
    return (k, n, 1, 1, 1, 1, 0, 0, 0, 0)


def exact_inputs(cls, m):
    """x [m, k] in {-1, 0, 1}, w [n, k] sparse +-1, bias [n] integers in [-32, 32] (conv_exact.exact_inputs on the 1x1 class at
    the extents (1, 1, m)) and residual [m, n] integers in [-16, 16].  float64."""
    n, k = cls
    x, wt, bias = ce.exact_inputs(conv_class(cls), (1, 1, m))
    g = ce._generator(conv_class(cls), (1, 1, m), 'residual')
    residual = torch.randint(-16, 17, (m, n), generator=g).double()
    return x[0, :, 0, :].t().contiguous(), wt.view(n, k).contiguous(), bias, residual


def real_inputs(cls, m, dtype):
    """conv_exact.real_inputs on the same class (activations ~ N(0, 0.5), He-scaled weights, bias ~ N(0, 0.3)) plus a residual
    ~ N(0, 0.3), all rounded to `dtype`."""
    n, k = cls
    x, wt, bias = ce.real_inputs(conv_class(cls), (1, 1, m), dtype)
    g = ce._generator(conv_class(cls), (1, 1, m), 'real residual')
    residual = (torch.randn(m, n, generator=g) * 0.3).to(dtype)
    return x[0, :, 0, :].t().contiguous(), wt.view(n, k).contiguous(), bias, residual


def reference(x, wt, bias, residual):
    """(acc, acc + bias, acc + bias + residual) in float64 on the CPU.  `+ 0.0` turns a -0.0 into the +0.0 every sum that starts
    from a zeroed accumulator gives."""
    acc = x.double().cpu() @ wt.double().cpu().t() + 0.0
    pre = acc + bias.double().cpu().view(1, -1) + 0.0
    return acc, pre, pre + residual.double().cpu() + 0.0


def references(x, wt, bias, residual):
    """{stage: {relu: float64 [m, n]}} for the stages 'acc', 'bias' (acc + bias) and 'residual' (acc + bias + residual), each
    without and with the ReLU.  The GEMM itself computes the last two."""
    acc, pre, full = reference(x, wt, bias, residual)
    return {name: {False: t, True: t.clamp(min=0)} for name, t in (('acc', acc), ('bias', pre), ('residual', full))}


def magnitude_sum(x, wt, bias, residual):
    """S = sum_c |x w| + |bias| + |residual| per output, float64: the scale of the rounding bound of a sum in any order."""
    return x.double().cpu().abs() @ wt.double().cpu().abs().t() + bias.double().cpu().abs().view(1, -1) + residual.double().cpu().abs()


def check_generator_bound(refs, m):
    """The condition of the exact comparison, on the reference alone: every stage is integer-valued with magnitude <= 256, and the
    ReLU has something to do on both epilogues the GEMM runs: it clamps a share in [0.35, 0.65] of the outputs for m >= 231; at
    smaller m (one row) both sides must merely be present.  -> (largest magnitude, smallest share, largest share)."""
    worst, shares = 0.0, []
    for name, pair in refs.items():
        t = pair[False]
        assert bool((t == t.round()).all()), 'the exact problem is not integer-valued at stage %r' % name
        worst = max(worst, float(t.abs().max()))
        if name == 'acc':
            continue
        clamped = float((t <= 0).double().mean())
        assert bool((t > 0).any()) and bool((t <= 0).any()), 'the ReLU after %r has only one side at m = %d' % (name, m)
        if m >= 231:
            assert 0.35 <= clamped <= 0.65, 'the ReLU after %r clamps a share of %.3f at m = %d' % (name, clamped, m)
        shares.append(clamped)
    assert worst <= BOUND, 'generator bound broken: the largest magnitude is %g > %d' % (worst, BOUND)
    return worst, min(shares), max(shares)


_cache = {}


def exact_problem(cls, m):
    """(x, w, bias, residual, references) in float64 on the CPU, computed once per (class, m) and shared: callers must not modify
    them.  Asserts the generator's bound."""
    key = (cls, m)
    if key not in _cache:
        x, wt, bias, residual = exact_inputs(cls, m)
        refs = references(x, wt, bias, residual)
        check_generator_bound(refs, m)
        _cache[key] = (x, wt, bias, residual, refs)
    return _cache[key]
