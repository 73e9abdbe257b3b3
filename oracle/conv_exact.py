"""Exact convolution problems for libodtk_conv.so (csrc/conv_ck.cpp), shared by tests/test_gpu_conv_instances.py and
tools/conv_instance_probe.py --check.  Pure CPU: nothing here touches the GPU or the library.

Integer-valued inputs make the comparison exact.  x is in {-1, 0, 1}, w in {-1, 0, 1}, the bias an integer in [-32, 32], so every
product and every partial sum is an integer; as long as |acc| and |acc + bias| stay <= 256 each of them is representable in bf16
(8 significant bits hold every integer up to 256; fp16 up to 2048) and in the fp32 accumulator, so no order of summation, no
rounding of the accumulator to the 16-bit type and no second rounding after the bias changes a bit.  The result of a correct
kernel EQUALS the float64 reference; a wrong tap, pad or neighbour pixel moves an output by an integer.

A class is (c_in, c_out, kh, kw, stride_h, stride_w, pad_h, pad_w, pad_h_end, pad_w_end): what adopt_sibling matches on."""
import glob
import json
import os
import zlib

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, 'plans')
BOUND = 256                                                     # integers up to here are exact in bf16
DTYPE_CODES = {1: torch.bfloat16, 2: torch.float16}             # include/odtk_hip.h: ODTK_BF16, ODTK_F16
EXTRA_CLASSES = [(64, 128, 3, 3, 2, 2, 1, 1, 1, 1)]             # reached by Model backbones (ResNet18/34 layer2), in no plan


def parse_conv_lines(path):
    """The `conv` lines of a plan file's "libraries" list, in the field order of export_plans (csrc/conv_ck.cpp):
    conv dtype n c h w k r s u v ph pw ph1 pw1 index name...   ->  list of dicts."""
    with open(path) as f:
        plan = json.load(f)
    out = []
    for line in plan.get('libraries', []):
        tok = line.split(' ', 16)
        if tok[0] != 'conv':
            continue
        if len(tok) != 17:
            raise ValueError('%s: malformed conv line %r' % (path, line))
        dtype, n, c, h, w, k, r, s, u, v, ph, pw, ph1, pw1, index = (int(t) for t in tok[1:16])
        out.append({'plan': os.path.basename(path), 'dtype': dtype, 'n': n, 'h': h, 'w': w, 'index': index, 'name': tok[16],
                    'cls': (c, k, r, s, u, v, ph, pw, ph1, pw1)})
    return out


def plan_files():
    return sorted(glob.glob(os.path.join(PLANS, '*.json')))


def plan_lines():
    return [line for path in plan_files() for line in parse_conv_lines(path)]


def plan_classes():
    """Distinct classes of the committed plans, sorted."""
    return sorted({line['cls'] for line in plan_lines()})


def plan_pairs():
    """Distinct (class, instance index, dtype code) of the committed plans -> instance name, sorted."""
    pairs = {}
    for line in plan_lines():
        key = (line['cls'], line['index'], line['dtype'])
        if pairs.setdefault(key, line['name']) != line['name']:
            raise ValueError('plans name instance #%d of dtype %d twice with different names' % (line['index'], line['dtype']))
    return sorted(pairs.items())


def class_id(cls):
    c, k, r, s, u, v, ph, pw, ph1, pw1 = cls
    pads = 'p%d' % ph if ph == pw == ph1 == pw1 else 'p%d.%d.%d.%d' % (ph, ph1, pw, pw1)
    return '%dto%d_%dx%d_s%d_%s' % (c, k, r, s, u, pads)


def out_extent(cls, h, w):
    c, k, r, s, u, v, ph, pw, ph1, pw1 = cls
    return (h + ph + ph1 - r) // u + 1, (w + pw + pw1 - s) // v + 1


def _generator(cls, extents, salt):
    return torch.Generator().manual_seed(zlib.crc32(repr((cls, extents, salt)).encode()))


def exact_inputs(cls, extents):
    """x [n, c, h, w] uniform in {-1, 0, 1}; w [k, c, r, s] = +-1 with probability p_w = min(1, 1024 / (c r s 2/3)), else 0 (so at
    most ~1024 non-zero products per output: a sum of standard deviation <= 32); bias [k] integers in [-32, 32].  float64."""
    c, k, r, s = cls[:4]
    n, h, w = extents
    g = _generator(cls, extents, 'exact')
    x = torch.randint(-1, 2, (n, c, h, w), generator=g).double()
    p_w = min(1.0, 1024.0 / (c * r * s * 2.0 / 3.0))
    sign = torch.randint(0, 2, (k, c, r, s), generator=g).double() * 2.0 - 1.0
    wt = torch.where(torch.rand(k, c, r, s, generator=g) < p_w, sign, torch.zeros(()).double())
    bias = torch.randint(-32, 33, (k,), generator=g).double()
    return x, wt, bias


def real_inputs(cls, extents, dtype):
    """The real-valued generator of tests/test_gpu_conv_library.py (activations ~ N(0, 0.5), He-scaled weights, bias ~ N(0, 0.3)),
    rounded to `dtype`: what the rounding comparison runs on."""
    c, k, r, s = cls[:4]
    n, h, w = extents
    g = _generator(cls, extents, 'real')
    x = (torch.randn(n, c, h, w, generator=g) * 0.5).to(dtype)
    wt = (torch.randn(k, c, r, s, generator=g) * (2.0 / (c * r * s)) ** 0.5).to(dtype)
    bias = (torch.randn(k, generator=g) * 0.3).to(dtype)
    return x, wt, bias


def reference(cls, x, wt, bias):
    """(acc, acc + bias) in float64 on the CPU: F.conv2d over the explicitly zero-padded input."""
    u, v, ph, pw, ph1, pw1 = cls[4:]
    padded = F.pad(x.double().cpu(), (pw, pw1, ph, ph1))
    acc = F.conv2d(padded, wt.double().cpu(), None, (u, v), 0)
    return acc, acc + bias.double().cpu().view(1, -1, 1, 1)


def check_generator_bound(acc, pre):
    """The condition of the generator, on the reference alone: every value an instance may hold is an integer of magnitude <= 256,
    and the ReLU has something to do (about half of the outputs are clamped)."""
    assert bool((acc == acc.round()).all()) and bool((pre == pre.round()).all()), 'the exact problem is not integer-valued'
    worst = max(float(acc.abs().max()), float(pre.abs().max()))
    assert worst <= BOUND, 'generator bound broken: max |acc|, |acc + bias| = %g > %d' % (worst, BOUND)
    zeros = float((pre <= 0).double().mean())
    assert 0.35 <= zeros <= 0.65, 'ReLU clamps a share of %.3f of the outputs: the case does not exercise both sides' % zeros
    return worst, zeros


_cache = {}


def exact_problem(cls, extents):
    """x, w, bias and the reference before the activation (float64, CPU), computed once per (class, extents) and shared: callers
    must not modify them."""
    key = (cls, tuple(extents))
    if key not in _cache:
        x, wt, bias = exact_inputs(cls, extents)
        acc, pre = reference(cls, x, wt, bias)
        check_generator_bound(acc, pre)
        _cache[key] = (x, wt, bias, pre)
    return _cache[key]


def first_difference(got, ref):
    """(number of differing elements, first differing (n, channel, row, column), got there, reference there) or None."""
    diff = got != ref
    count = int(diff.sum())
    if not count:
        return None
    at = tuple(int(i) for i in diff.nonzero()[0])
    return count, at, float(got[at]), float(ref[at])
