"""odtk_tower_conv3x3 (csrc/tower_conv.hpp): the head towers' 3x3, stride 1, 256 -> 256 convolution as the library's own
implicit-GEMM MFMA kernel.

Bit for bit against the integer-valued problems of oracle/conv_exact.py (no order of summation and neither of the two roundings
changes a bit there: a wrong tap, a neighbour image's pixel read instead of padding or a K-tile read early moves an output by an
integer), at extents chosen for the kernel's 256-pixel tile: a single pixel (eight of nine taps outside), one row, one column, less
than a tile, a tile that spans the end of image 0 and the start of image 1, exactly three tiles, five tiles with a partial last one,
rows longer than a tile.  Every case walks all 36 K-tiles.  Then the real-valued problem within the two-roundings bound of
tests/test_gpu_conv_instances.py, determinism, a bounded screen of repeated launches, a sensitivity check and the ABI's refusals."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'retinanet-examples_amd')]

from oracle import conv_exact as ce  # noqa: E402

gpu = pytest.mark.gpu

CLS = (256, 256, 3, 3, 1, 1, 1, 1, 1, 1)
EXTENTS = [(1, 1, 1), (1, 1, 40), (1, 40, 1), (2, 3, 5), (2, 9, 31), (3, 16, 16), (2, 17, 33), (1, 2, 300)]
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
EPS = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}


def _extents_id(e):
    return '%dx%dx%d' % e


def _to_device(t, dtype):
    t = t.to(dtype).cuda()
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t


_cache = {}


def _exact_on_device(extents, dtype):
    """x, w, bias, a zero bias and the four references (bias | zero bias) x (ReLU | linear) in `dtype` on the GPU, once."""
    key = (tuple(extents), dtype)
    if key not in _cache:
        x, wt, bias, pre = ce.exact_problem(CLS, extents)
        acc = pre - bias.view(1, -1, 1, 1)
        refs = {(True, True): pre.clamp(min=0), (True, False): pre, (False, True): acc.clamp(min=0), (False, False): acc}
        for ref in refs.values():
            assert float(ref.abs().max()) <= ce.BOUND and torch.equal(ref.to(dtype).double(), ref)
        _cache[key] = (_to_device(x, dtype), _to_device(wt, dtype), _to_device(bias, dtype), _to_device(torch.zeros_like(bias), dtype),
                       {k: _to_device(v, dtype) for k, v in refs.items()})
    return _cache[key]


def _differs(got, ref):
    if got.shape == ref.shape and torch.equal(got.view(torch.int16), ref.view(torch.int16)):
        return None
    assert got.shape == ref.shape, (got.shape, ref.shape)
    found = ce.first_difference(got.double().cpu(), ref.double().cpu())
    return found or (int((got.view(torch.int16) != ref.view(torch.int16)).sum()), 'sign of zero', -0.0, 0.0)


# ---- without a GPU -------------------------------------------------------------------------------------------------------------------

def test_reference_notices_two_swapped_taps():
    """Sensitivity of the exact comparison: with two taps of the weights swapped the reference itself changes, so a kernel that
    walks the taps in a wrong order cannot pass."""
    x, wt, bias, pre = ce.exact_problem(CLS, (2, 9, 31))
    for a, b in (((0, 0), (0, 1)), ((1, 1), (2, 2)), ((0, 2), (2, 0))):
        swapped = wt.clone()
        swapped[:, :, a[0], a[1]], swapped[:, :, b[0], b[1]] = wt[:, :, b[0], b[1]], wt[:, :, a[0], a[1]]
        _, other = ce.reference(CLS, x, swapped, bias)
        changed = float((other != pre).double().mean())
        assert changed > 0.5, 'swapping taps %s and %s changes only a share of %.3f of the outputs' % (a, b, changed)


def test_binding_refuses_without_a_device_what_the_kernel_does_not_take():
    from odtk import _C
    assert 'odtk_tower_conv3x3' in _C.exported_symbols() and 'tower_conv3x3_kernel' in _C.KERNEL_NAMES
    assert _C.KERNEL_NAMES.index('tower_conv3x3_kernel') == len(_C.KERNEL_NAMES) - 1
    fn = _C.library().odtk_tower_conv3x3
    ok = dict(y=0x1000, x=0x2000, w=0x3000, bias=0x4000, batch=1, height=4, width=4, c_in=256, c_out=256, dtype=_C.BF16, relu=1)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a['y'], a['x'], a['w'], a['bias'], a['batch'], a['height'], a['width'], a['c_in'], a['c_out'], a['dtype'], a['relu'], None)

    # (validation happens before anything touches the device: the pointers are never dereferenced)
    for name in ('y', 'x', 'w', 'bias'):
        assert call(**{name: None}) == _C.ERR_INVALID, name
        assert call(**{name: ok[name] + 8}) == _C.ERR_INVALID, name + ' misaligned'
    assert call(y=ok['x']) == _C.ERR_INVALID
    for name in ('batch', 'height', 'width', 'c_in', 'c_out'):
        assert call(**{name: 0}) == _C.ERR_INVALID, name
    assert call(dtype=_C.F32) == _C.ERR_UNSUPPORTED
    for c_in, c_out in ((128, 256), (256, 128), (256, 720), (512, 512), (264, 256)):
        assert call(c_in=c_in, c_out=c_out) == _C.ERR_UNSUPPORTED, (c_in, c_out)
    assert call(batch=64, height=256, width=256) == _C.ERR_UNSUPPORTED              # 2^22 pixels: beyond the 32-bit byte offsets
    assert _C.library().odtk_debug_tower_conv_variant(4) == _C.ERR_INVALID
    assert _C.library().odtk_debug_tower_conv_variant(-1) == 1


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('dtype', list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize('extents', EXTENTS, ids=_extents_id)
def test_exact_problems_bit_for_bit(extents, dtype):
    from odtk import _C
    x, w, b, zero, refs = _exact_on_device(extents, dtype)
    failures = []
    for with_bias in (True, False):
        for relu in (True, False):
            y = _C.tower_conv3x3(x, w, b if with_bias else zero, relu)
            torch.cuda.synchronize()
            assert y.dtype == dtype and y.shape == refs[(with_bias, relu)].shape and y.is_contiguous(memory_format=torch.channels_last)
            bad = _differs(y, refs[(with_bias, relu)])
            if bad:
                failures.append('bias=%d relu=%d: %d elements differ, first at (n, c, y, x) = %s: got %g, reference %g'
                                % ((with_bias, relu) + tuple(bad)))
    assert not failures, '%s %s:\n  ' % (extents, dtype) + '\n  '.join(failures)


@gpu
@pytest.mark.parametrize('dtype', list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize('variant', [0, 2, 3], ids=['tile-k', '16x16x32-tile-k', '16x16x32'])
def test_every_variant_is_exact(variant, dtype):
    """The default (1) is the 32x32x16 form with permuted tile ids; the others -- workgroup k owns tile k, and the 16x16x32 form
    with both tile orders -- on every extent, with and without ReLU."""
    from odtk import _C
    lib = _C.library()
    before = lib.odtk_debug_tower_conv_variant(variant)
    assert before == 1
    failures = []
    try:
        for extents in EXTENTS:
            x, w, b, _, refs = _exact_on_device(extents, dtype)
            for relu in (True, False):
                y = _C.tower_conv3x3(x, w, b, relu)
                if _differs(y, refs[(True, relu)]):
                    failures.append((extents, relu))
        torch.cuda.synchronize()
    finally:
        lib.odtk_debug_tower_conv_variant(before)
    assert not failures, failures


@gpu
@pytest.mark.parametrize('dtype', list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize('extents', [(2, 9, 31), (2, 17, 33)], ids=_extents_id)
def test_real_valued_problem_within_the_two_roundings_bound(extents, dtype):
    from odtk import _C
    x, wt, bias = ce.real_inputs(CLS, extents, dtype)
    _, pre = ce.reference(CLS, x, wt, bias)
    bias_max = float(bias.float().abs().max())
    xd, wd, bd, pre = _to_device(x, dtype), _to_device(wt, dtype), _to_device(bias, dtype), pre.cuda()
    for relu in (True, False):
        y = _C.tower_conv3x3(xd, wd, bd, relu)
        ref = pre.clamp(min=0) if relu else pre
        err = (y.double() - ref).abs()
        tol = EPS[dtype] * ref.abs() + EPS[dtype] * bias_max + 1e-3
        print('\n[tower-conv] real-valued %s %s relu=%d: max err %.3g, max err / tol %.3f'
              % (extents, dtype, relu, float(err.max()), float((err / tol).max())))
        assert bool((err <= tol).all()), 'relu=%d: excess %.3g' % (relu, float((err - tol).max()))
        again = _C.tower_conv3x3(xd, wd, bd, relu)                       # the same input, the same bits
        assert torch.equal(y.view(torch.int16), again.view(torch.int16))


@gpu
def test_twenty_launches_all_equal_the_reference():
    """A bounded screen for a staged buffer read early (which shows as rare wrong tiles): twenty launches, each compared."""
    from odtk import _C
    x, w, b, _, refs = _exact_on_device((2, 17, 33), torch.bfloat16)
    outs = [_C.tower_conv3x3(x, w, b, True) for _ in range(20)]
    torch.cuda.synchronize()
    wrong = [i for i, y in enumerate(outs) if _differs(y, refs[(True, True)])]
    assert not wrong, 'launches %s differ from the reference' % wrong


@gpu
def test_nan_is_handed_on_and_other_shapes_raise():
    from odtk import _C
    x, w, b, _, refs = _exact_on_device((2, 3, 5), torch.bfloat16)
    xn = x.clone()
    xn[1, 7, 1, 2] = float('nan')
    y = _C.tower_conv3x3(xn, w, b, True)
    hit = torch.isnan(y)
    # the 3 x 3 neighbourhood of the pixel, in every output channel whose weights are non-zero there; nothing in image 0
    assert bool(hit[1, :, 0:3, 1:4].any()) and not bool(hit[0].any()) and not bool(hit[1, :, :, 4:].any())
    assert not _differs(y[0], refs[(True, True)][0])
    with pytest.raises(RuntimeError):
        _C.tower_conv3x3(x[:, :128].contiguous(memory_format=torch.channels_last), w[:, :128].contiguous(memory_format=torch.channels_last), b)
    with pytest.raises(RuntimeError):
        _C.tower_conv3x3(x.float(), w.float(), b.float())
    with pytest.raises(RuntimeError):
        _C.tower_conv3x3(x.contiguous(), w, b)                            # NCHW
    fn = _C.library().odtk_tower_conv3x3
    out = torch.empty_like(x)
    args = (x.shape[0], x.shape[2], x.shape[3], 256, 256, _C.BF16, 1, None)
    assert fn(out.data_ptr(), x.data_ptr() + 2, w.data_ptr(), b.data_ptr(), *args) == _C.ERR_INVALID
    assert fn(out.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), x.shape[0], x.shape[2], x.shape[3], 256, 256, _C.BF16, 1,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert not _differs(out, refs[(True, True)])
