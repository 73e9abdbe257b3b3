"""The six streaming kernels of csrc/epilogue.hpp (bias_act fast and scalar, bias_act_maxpool, upsample_nearest2x, canvas_fill,
stem_pack) and their launchers in csrc/engine.hip against the plain restatements of tests/engine_streams_ref.py, on every launch
path and at the edge values: each grid-stride loop wrapping (odtk_debug_stream_tuning caps the grids, so tensors of a few kilobytes
walk the paths production reaches at 70 .. 130 MB), the fast bias_act form's unrolled loop with rows that are no power of two, the
scalar / fast boundary, the max-pool's 64-bit index form, every border of the pool window and of the canvas rectangles, the
alignment fallback of the stem pack, and ties, overflow, subnormals, NaNs and signed zeros through every cast.

Every call goes through the C ABI on the current stream.  Every buffer is a view into a flat allocation filled with a sentinel byte,
64 KiB of it on either side, and the guards are compared after every call: a store outside a tensor is a failure of the test.
Comparison: bits equal; where the restatement is a NaN the result must be a NaN.  tests/test_engine_streams_ref.py shows (without a
GPU) that every case named here takes the path its name claims.
"""
import contextlib
import ctypes
import zlib

import numpy as np
import pytest
import torch

import engine_streams_ref as ref
from odtk import _C

pytestmark = pytest.mark.gpu

GUARD = 64 << 10
SENTINEL = 0xA5
CODE = {'fp32': _C.F32, 'bf16': _C.BF16, 'fp16': _C.F16}
TORCH = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
SIZE = {'fp32': 4, 'bf16': 2, 'fp16': 2}


class Buf:
    """`nbytes` at `offset` bytes past a 16-byte boundary, inside a sentinel-filled allocation with GUARD bytes on either side."""

    def __init__(self, nbytes, offset=0, data=None):
        self.begin, self.nbytes = GUARD + offset, nbytes
        self.flat = torch.full((GUARD + 16 + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
        assert self.flat.data_ptr() % 16 == 0
        self.ptr = self.flat.data_ptr() + self.begin
        if data is not None:
            self.write(data)

    @classmethod
    def of(cls, array, offset=0):
        array = np.ascontiguousarray(array)
        return cls(array.nbytes, offset, array)

    def write(self, array):
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        assert raw.size == self.nbytes
        self.flat[self.begin:self.begin + self.nbytes].copy_(torch.from_numpy(raw.copy()))

    def read(self, dtype, shape):
        return self.flat[self.begin:self.begin + self.nbytes].cpu().numpy().view(dtype).reshape(shape).copy()

    def check_guards(self, what):
        lo, hi = self.flat[:self.begin], self.flat[self.begin + self.nbytes:]
        assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), '%s: a store outside the tensor' % what


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    if rc == _C.ERR_HIP:
        pytest.exit('%s: HIP error %s -- nothing more is started on this device' % (what, _C.library().odtk_last_hip_error().decode()), 3)
    assert rc == 0, '%s returned %d' % (what, rc)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a fault of the device is sticky: end the session instead of launching the remaining cases on it
        pytest.exit('%s: %s -- nothing more is started on this device' % (what, e), 3)


@contextlib.contextmanager
def tuned(grid_cap=-1, pool_wide_index=-1):
    found = _C.stream_tuning_state()
    try:
        _C.stream_tuning(grid_cap, pool_wide_index)
        yield
    finally:
        _C.stream_tuning(**found)
        assert _C.stream_tuning_state() == found


def _randn_bits(rng, shape, dtype, scale=2.0):
    return ref.round_bits((rng.standard_normal(shape) * scale).astype(np.float32), dtype)


def _run_bias_act(y_bits, bias, res_bits, relu, dtype, what):
    pixels, channels = y_bits.shape
    y, b = Buf.of(y_bits), Buf.of(np.asarray(bias, dtype=np.float32))
    r = Buf.of(res_bits) if res_bits is not None else None
    _ok(_C.library().odtk_bias_act(y.ptr, b.ptr, r.ptr if r else None, pixels, channels, CODE[dtype], int(relu), _stream()), what)
    for buf in (y, b) + ((r,) if r else ()):
        buf.check_guards(what)
    if r:
        assert np.array_equal(r.read(ref.BITS[dtype], y_bits.shape), res_bits), '%s: the residual was written' % what
    ref.assert_bits(y.read(ref.BITS[dtype], y_bits.shape), ref.bias_act(y_bits, bias, res_bits, relu, dtype), dtype, what)


# ---- bias_act ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dtype', ref.bias_act_case_ids(), ids=['%s-%s' % c for c in ref.bias_act_case_ids()])
def test_bias_act_on_every_launch_path(name, dtype):
    """Every case of engine_streams_ref.BIAS_ACT_CASES x residual x ReLU.  The library's own grid query must still name the path the
    case stands for (tests/test_engine_streams_ref.py checks the whole table without a GPU)."""
    channels, pixels, cap, claim = ref.bias_act_case(name, dtype)
    rng = np.random.default_rng(zlib.crc32(('%s-%s' % (name, dtype)).encode()))
    with tuned(grid_cap=cap):
        assert ref.describe_grid(_C.bias_act_grid(pixels, channels, TORCH[dtype]), channels, pixels, dtype) == claim
        for with_res in (False, True):
            for relu in (False, True):
                y = _randn_bits(rng, (pixels, channels), dtype)
                res = _randn_bits(rng, (pixels, channels), dtype) if with_res else None
                bias = rng.standard_normal(channels).astype(np.float32)
                _run_bias_act(y, bias, res, relu, dtype, 'bias_act %s %s res=%d relu=%d' % (name, dtype, with_res, relu))


@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('form', ['scalar', 'fast'])
def test_bias_act_special_values(form, dtype):
    """The table of engine_streams_ref.bias_act_special crossed against its bias table (pixel p holds x[p] in all 16 channels,
    channel c adds bias[c]): signed zeros, cancellation, infinities and inf - inf, NaNs of both signs, ties in both directions,
    overflow of the storage type, subnormal results -- once through each kernel form, with and without a residual and the ReLU."""
    x, bias = ref.bias_act_special(dtype)
    reps = 1 if form == 'scalar' else -(-16 * ref.PER[dtype] // len(x))          # fast: n / per >= 256
    xs = np.tile(x, reps)
    assert _C.bias_act_grid(len(xs), 16, TORCH[dtype])['form'] == form
    y = np.repeat(xs[:, None], 16, axis=1)
    res = np.stack([np.roll(xs, c + 1) for c in range(16)], axis=1)
    for res_bits in (None, res):
        for relu in (False, True):
            _run_bias_act(y, bias, res_bits, relu, dtype,
                          'bias_act special values %s %s res=%d relu=%d' % (form, dtype, res_bits is not None, relu))


# ---- bias_act_maxpool ----------------------------------------------------------------------------------------------------------
def _run_pool(y_bits, bias, relu, dtype, what):
    batch, h, w, c = y_bits.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    y, b, out = Buf.of(y_bits), Buf.of(bias), Buf(batch * ho * wo * c * 2)
    _ok(_C.library().odtk_bias_act_maxpool(y.ptr, b.ptr, out.ptr, batch, h, w, c, CODE[dtype], int(relu), _stream()), what)
    for buf in (y, b, out):
        buf.check_guards(what)
    assert np.array_equal(y.read(np.uint16, y_bits.shape), y_bits), '%s: the input was written' % what
    ref.assert_bits(out.read(np.uint16, (batch, ho, wo, c)), ref.bias_act_maxpool(y_bits, bias, relu, dtype), dtype, what)


def _pool_fillings(rng, batch, h, w, c, dtype):
    """randn; a ramp growing with y * w + x (the maximum of every window in its last row and column; 0 .. 255, exact in bf16) and
    its negation (in its first); all-negative values (a padding value that won would show as 0)."""
    ramp = np.arange(h * w, dtype=np.float32).reshape(1, h, w, 1) * np.ones((batch, 1, 1, c), dtype=np.float32)
    yield 'randn', _randn_bits(rng, (batch, h, w, c), dtype), (False, True)
    yield 'ramp', ref.round_bits(ramp, dtype), (False, True)
    yield 'falling ramp', ref.round_bits(-ramp, dtype), (False, True)
    yield 'negative', ref.round_bits(-1 - np.abs(rng.standard_normal((batch, h, w, c))).astype(np.float32), dtype), (False,)


@pytest.mark.parametrize('wide', [0, 1], ids=['index32', 'index64'])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_bias_act_maxpool_borders(dtype, wide):
    """Every extent of engine_streams_ref.POOL_EXTENTS (one row, one column, 2 x 2, even x odd, ...), three fillings, with and
    without the ReLU -- through the 32-bit index form and (pool_wide_index = 1) the 64-bit one, which no tensor that fits in
    memory reaches otherwise."""
    rng = np.random.default_rng(11 + wide)
    with tuned(pool_wide_index=wide):
        for batch, c in ref.POOL_BATCH_CHANNELS:
            for h, w in ref.POOL_EXTENTS:
                for filling, y, relus in _pool_fillings(rng, batch, h, w, c, dtype):
                    bias = np.zeros(c, dtype=np.float32) if filling == 'negative' else rng.standard_normal(c).astype(np.float32)
                    for relu in relus:
                        _run_pool(y, bias, relu, dtype, 'bias_act_maxpool %s %dx%dx%dx%d %s relu=%d wide=%d' % (dtype, batch, c, h, w, filling, relu, wide))


@pytest.mark.parametrize('wide', [0, 1], ids=['index32', 'index64'])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_bias_act_maxpool_under_a_grid_cap(dtype, wide):
    """engine_streams_ref.POOL_CAPPED: one workgroup for the whole tensor; the second shape makes every lane run its loop body more
    than once."""
    rng = np.random.default_rng(13)
    for batch, c, h, w, cap, _ in ref.POOL_CAPPED:
        with tuned(grid_cap=cap, pool_wide_index=wide):
            for relu in (False, True):
                _run_pool(_randn_bits(rng, (batch, h, w, c), dtype), rng.standard_normal(c).astype(np.float32), relu, dtype,
                          'bias_act_maxpool %s %dx%dx%dx%d cap=%d relu=%d wide=%d' % (dtype, batch, c, h, w, cap, relu, wide))


# ---- upsample2x ----------------------------------------------------------------------------------------------------------------
def _counter(n, dtype, start):
    """n distinct bit patterns: a counter (wrapping for the 16-bit types only beyond 65536 elements)."""
    bits = ref.BITS[dtype]
    return ((np.arange(n, dtype=np.uint64) + start) & np.uint64(np.iinfo(bits).max)).astype(bits)


@pytest.mark.parametrize('cap', [0, 1, 3])
@pytest.mark.parametrize('dtype', ref.DTYPES)
def test_upsample2x_places_every_vector(dtype, cap):
    """Distinct bit patterns in, the output allocated over sentinel bytes: a misplaced or unwritten 16-byte vector shows.  A plain
    copy: the comparison is on bits, NaN patterns included."""
    with tuned(grid_cap=cap):
        for batch in (1, 3):
            for h, w in ref.UPSAMPLE_EXTENTS:
                for row_bytes in ref.ROW_BYTES:
                    c = row_bytes // SIZE[dtype]
                    what = 'upsample2x %s %dx%dx%dx%d cap=%d' % (dtype, batch, c, h, w, cap)
                    x_bits = _counter(batch * h * w * c, dtype, 0x7f00).reshape(batch, h, w, c)
                    x, out = Buf.of(x_bits), Buf(4 * x_bits.nbytes)
                    _ok(_C.library().odtk_upsample_nearest2x(x.ptr, out.ptr, batch, h, w, c, CODE[dtype], _stream()), what)
                    x.check_guards(what)
                    out.check_guards(what)
                    assert np.array_equal(out.read(ref.BITS[dtype], (batch, 2 * h, 2 * w, c)), ref.upsample2x(x_bits)), what


# ---- stem_pack -----------------------------------------------------------------------------------------------------------------
def _stem_input(rng, batch, h, w, in_dtype, shift):
    """The logical image [batch, 3, h, w] as bits: randn scaled into the normal range, with the special table at known places."""
    bits = _randn_bits(rng, (batch, 3, h, w), in_dtype, scale=1.5)
    flat = bits.reshape(-1)
    ref.place_table(flat, ref.stem_special(in_dtype), shift)
    return flat.reshape(batch, 3, h, w)


def _run_stem(x_bits, in_dtype, out_dtype, layout, offset, what):
    batch, _, h, w = x_bits.shape
    memory = x_bits if layout == 'nchw' else x_bits.transpose(0, 2, 3, 1)
    x, out = Buf.of(memory, offset), Buf(batch * (h // 2) * (w // 2) * 32)
    assert x.ptr % 16 == offset
    _ok(_C.library().odtk_stem_pack(x.ptr, out.ptr, batch, h, w, CODE[in_dtype], int(layout == 'nhwc'), CODE[out_dtype], _stream()), what)
    x.check_guards(what)
    out.check_guards(what)
    got = out.read(np.uint16, (batch, h // 2, w // 2, 16))
    assert not got[..., 12:].any(), '%s: channels 12..15 must be all-zero bits' % what
    ref.assert_bits(got, ref.stem_pack(x_bits, in_dtype, out_dtype), out_dtype, what)


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('in_dtype', ref.DTYPES)
def test_stem_pack_layouts_alignments_and_the_cast(in_dtype, layout):
    """Every extent x batch x output type x alignment of the input pointer: 16, 8 (the float2 path's minimum) and 4 bytes (its
    fallback) for fp32, 16 and 2 for the 16-bit types.  The values carry ties of both directions, overflow, subnormal results, signed
    zeros, infinities and the NaN patterns 0x7fc00000, 0x7f800001, 0xff800001, 0x7fbfffff, 0xffffffff (fp32; their 16-bit
    counterparts otherwise): each must come out a NaN in both output types."""
    rng = np.random.default_rng(17)
    shift = 0
    for out_dtype in ('bf16', 'fp16'):
        for batch in (1, 3):
            for h, w in ref.STEM_EXTENTS:
                for offset in ((0, 8, 4) if in_dtype == 'fp32' else (0, 2)):
                    shift += 5
                    _run_stem(_stem_input(rng, batch, h, w, in_dtype, shift), in_dtype, out_dtype, layout, offset,
                              'stem_pack %s->%s %s %dx3x%dx%d input at +%d' % (in_dtype, out_dtype, layout, batch, h, w, offset))


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('in_dtype', ref.DTYPES)
def test_stem_pack_under_a_grid_cap(in_dtype, layout):
    """engine_streams_ref.STEM_CAPPED: one workgroup; at 3 x (64, 96) every lane runs its loop body 18 times."""
    rng = np.random.default_rng(19)
    for batch, h, w, cap, _ in ref.STEM_CAPPED:
        with tuned(grid_cap=cap):
            for out_dtype in ('bf16', 'fp16'):
                for offset in ((0, 4) if in_dtype == 'fp32' else (0,)):
                    _run_stem(_stem_input(rng, batch, h, w, in_dtype, 3), in_dtype, out_dtype, layout, offset,
                              'stem_pack %s->%s %s %dx3x%dx%d input at +%d cap=%d' % (in_dtype, out_dtype, layout, batch, h, w, offset, cap))


# ---- canvas pack and clear -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap', [0, 1])
@pytest.mark.parametrize('dtype', ref.DTYPES)
def test_canvas_pack_and_clear_rectangles(dtype, cap):
    """engine_streams_ref.canvas_layouts: a rectangle flush against each edge, the whole canvas, no rectangle, and the full six with
    a 1 x 1 among them.  Sources and the canvas hold distinct bit patterns (NaN patterns among them); pack must place every vector
    and zero the rest, clear must zero the rest and leave every bit inside alone."""
    lib = _C.library()
    bits = ref.BITS[dtype]
    with tuned(grid_cap=cap):
        for batch in (1, 2):
            for row_bytes in (16, 48):
                c = row_bytes // SIZE[dtype]
                for name, (height, width, rects) in ref.canvas_layouts().items():
                    what = 'canvas %s %s batch %d, %d channels, cap=%d' % (name, dtype, batch, c, cap)
                    flat = (ctypes.c_int * max(4 * len(rects), 1))(*[v for r in rects for v in r])
                    sources, start = [], 0x7f00
                    for _, _, h, w in rects:
                        sources.append(_counter(batch * h * w * c, dtype, start).reshape(batch, h, w, c))
                        start += sources[-1].size
                    bufs = [Buf.of(s) for s in sources]
                    canvas = Buf(batch * height * width * row_bytes)
                    ptrs = (ctypes.c_void_p * max(len(rects), 1))(*[b.ptr for b in bufs])
                    _ok(lib.odtk_canvas_pack(canvas.ptr, batch, height, width, c, CODE[dtype], flat, ptrs, len(rects), _stream()), what + ' pack')
                    for b in bufs + [canvas]:
                        b.check_guards(what + ' pack')
                    got = canvas.read(bits, (batch, height, width, c))
                    assert np.array_equal(got, ref.canvas_pack(batch, height, width, c, rects, sources, bits)), what + ' pack'
                    before = _counter(batch * height * width * c, dtype, 0x7b00).reshape(batch, height, width, c)
                    canvas.write(before)
                    _ok(lib.odtk_canvas_clear(canvas.ptr, batch, height, width, c, CODE[dtype], flat, len(rects), _stream()), what + ' clear')
                    canvas.check_guards(what + ' clear')
                    assert np.array_equal(canvas.read(bits, before.shape), ref.canvas_clear(before, rects)), what + ' clear'
