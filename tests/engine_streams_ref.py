"""Plain restatements of the engine's six streaming kernels (csrc/epilogue.hpp), in numpy on bit patterns, and the tables of cases
tests/test_engine_streams_ref.py (no GPU: the restatements against torch's CPU operators, every case shown not to be vacuous) and
tests/test_gpu_engine_streams.py (the kernels against the restatements) share.

A tensor is an array of BITS: uint32 for 'fp32', uint16 for 'bf16' / 'fp16'.  Every fp32 operation is written once, in the
kernel's order; the single rounding to the storage type is done by hand: bf16 = round-to-nearest-even on the bit pattern with a NaN
staying a NaN, fp16 = numpy.float16.  Comparison rule (assert_bits): bits equal; where the restatement is a NaN the result must be
a NaN and its payload is free.

bias_act's ReLU is the kernel's documented rule  o > 0 ? o : (isnan(o) ? o : +0.0): a NaN goes through and -0.0 becomes +0.0.
torch.relu keeps -0.0; the restatement follows the kernel.
"""
import numpy as np

DTYPES = ('fp32', 'bf16', 'fp16')
BITS = {'fp32': np.uint32, 'bf16': np.uint16, 'fp16': np.uint16}
PER = {'fp32': 4, 'bf16': 8, 'fp16': 8}            # elements of a 16-byte vector
MAX_LEVELS = 6                                      # ODTK_MAX_LEVELS
F32 = np.float32


# ---- number formats ------------------------------------------------------------------------------------------------------------
def widen(bits, dtype):
    """bits of `dtype` -> float32 (exact)."""
    bits = np.asarray(bits)
    if dtype == 'fp32':
        return bits.astype(np.uint32).view(F32)
    if dtype == 'bf16':
        return (bits.astype(np.uint32) << np.uint32(16)).view(F32)
    with np.errstate(invalid='ignore'):                     # (a signalling NaN raises the flag)
        return bits.astype(np.uint16).view(np.float16).astype(F32)


def round_bits(f, dtype):
    """float32 -> bits of `dtype`, ONE rounding to nearest even; a NaN stays a NaN."""
    f = np.ascontiguousarray(f, dtype=F32)
    if dtype == 'fp32':
        return f.view(np.uint32).copy()
    if dtype == 'fp16':
        with np.errstate(over='ignore', invalid='ignore'):
            return f.astype(np.float16).view(np.uint16).copy()
    b = f.view(np.uint32).astype(np.uint64)
    nan = (b & 0x7fffffff) > 0x7f800000
    r = (b + 0x7fff + ((b >> 16) & 1)) >> 16
    r = np.where(nan, (b >> 16) | 0x40, r)          # sign kept, quiet bit set
    return r.astype(np.uint16)


def is_nan_bits(bits, dtype):
    bits = np.asarray(bits).astype(np.uint32)
    if dtype == 'fp32':
        return (bits & 0x7fffffff) > 0x7f800000
    if dtype == 'bf16':
        return (bits & 0x7fff) > 0x7f80
    return (bits & 0x7fff) > 0x7c00


def assert_bits(got, ref, dtype, what=''):
    """got == ref bit for bit, except where ref is a NaN: there got must be a NaN (any payload)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, '%s: %s %s against %s %s' % (what, got.shape, got.dtype, ref.shape, ref.dtype)
    nan = is_nan_bits(ref, dtype)
    bad = np.where(nan, ~is_nan_bits(got, dtype), got != ref)
    if bad.any():
        at = np.argwhere(bad)
        first = tuple(int(v) for v in at[0])
        raise AssertionError('%s: %d of %d elements differ; first at %s: got 0x%x, restatement 0x%x%s'
                             % (what, len(at), bad.size, first, int(got[first]), int(ref[first]),
                                ' (a NaN)' if bool(nan[first]) else ''))


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
def _relu(o):
    return np.where(o > 0, o, np.where(np.isnan(o), o, F32(0.0))).astype(F32)


def bias_act(y_bits, bias, res_bits, relu, dtype):
    """y [pixels, channels] bits, bias float32 [channels], res as y or None -> bits of act((y + bias[c]) + res)."""
    with np.errstate(over='ignore', invalid='ignore'):
        o = widen(y_bits, dtype) + np.asarray(bias, dtype=F32)[None, :]
        if res_bits is not None:
            o = o + widen(res_bits, dtype)
        if relu:
            o = _relu(o)
    return round_bits(o, dtype)


def order_keys(bits16):
    """sign-magnitude 16-bit float bits -> order-preserving int16 keys (+0 above -0, +NaN above +inf, -NaN below -inf); an involution."""
    h = np.asarray(bits16).astype(np.uint16)
    sign = (h >> np.uint16(15)).astype(bool)
    return np.where(sign, h ^ np.uint16(0x7fff), h).astype(np.uint16).view(np.int16)


def bias_act_maxpool(y_bits, bias, relu, dtype):
    """y [batch, h, w, c] bits (bf16 / fp16) -> [batch, (h+1)/2, (w+1)/2, c] bits of act(max over the clamped 3x3 / stride 2 window
    + bias[c]).  The maximum is taken on the keys (so +0 beats -0); any NaN of the window wins."""
    y_bits = np.asarray(y_bits)
    _, h, w, _ = y_bits.shape
    keys = order_keys(y_bits)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    stack = []
    for dy in range(3):
        rows = np.clip(2 * np.arange(ho) - 1 + dy, 0, h - 1)
        for dx in range(3):
            cols = np.clip(2 * np.arange(wo) - 1 + dx, 0, w - 1)
            stack.append(keys[:, rows][:, :, cols])
    stack = np.stack(stack)
    kmax, kmin = stack.max(0), stack.min(0)
    neg_inf_key = order_keys(np.array([0xff80 if dtype == 'bf16' else 0xfc00], dtype=np.uint16))[0]
    kk = np.where(kmin < neg_inf_key, kmin, kmax)                    # below -inf's key: a negative NaN
    m = widen(kk.view(np.uint16) ^ np.where(kk < 0, np.uint16(0x7fff), np.uint16(0)).astype(np.uint16), dtype)
    with np.errstate(over='ignore', invalid='ignore'):
        o = m + np.asarray(bias, dtype=F32)[None, None, None, :]
        if relu:
            o = _relu(o)
    return round_bits(o, dtype)


def upsample2x(x_bits):
    """[batch, h, w, c] bits -> [batch, 2h, 2w, c]: out[b][y][x] = in[b][y / 2][x / 2]."""
    return np.repeat(np.repeat(np.asarray(x_bits), 2, axis=1), 2, axis=2)


def canvas_pack(batch, height, width, channels, rects, sources, bits):
    """zeros [batch, height, width, channels] with rectangle i = (y0, x0, h, w) filled from sources[i] [batch, h, w, channels]."""
    out = np.zeros((batch, height, width, channels), dtype=bits)
    for (y0, x0, h, w), src in zip(rects, sources):
        out[:, y0:y0 + h, x0:x0 + w] = src
    return out


def canvas_clear(canvas_bits, rects):
    """zero outside the rectangles, every bit inside left alone."""
    out = np.zeros_like(canvas_bits)
    for y0, x0, h, w in rects:
        out[:, y0:y0 + h, x0:x0 + w] = canvas_bits[:, y0:y0 + h, x0:x0 + w]
    return out


def stem_pack(x_bits, in_dtype, out_dtype):
    """x [batch, 3, height, width] bits (the LOGICAL image, whatever its memory layout) -> [batch, height/2, width/2, 16] bits:
    out[n][y][x][(dy * 2 + dx) * 3 + c] = cast(x[n][c][2 y + dy][2 x + dx]), channels 12..15 all-zero bits."""
    x_bits = np.asarray(x_bits)
    b, _, h, w = x_bits.shape
    cast = round_bits(widen(x_bits, in_dtype), out_dtype)
    out = np.zeros((b, h // 2, w // 2, 16), dtype=np.uint16)
    for dy in range(2):
        for dx in range(2):
            for c in range(3):
                out[:, :, :, (dy * 2 + dx) * 3 + c] = cast[:, c, dy::2, dx::2]
    return out


# ---- bias_act: the launch the library makes, restated for the claims of the case table -----------------------------------------
# name -> (channels, pixels, dtypes, grid_cap, claims per dtype).  A claim: form, `idle` (workgroups with nothing to do), `unrolled`
# (lane 0 of workgroup 0 enters the 4-vector loop), `wraps` (a lane runs its loop body more than once), `rounded` (the grid is a
# multiple of unit = vpr / gcd(vpr, 256) > 1, as the fast form needs).  tests/test_engine_streams_ref.py holds every claim against
# odtk_debug_bias_act_grid.
def _claim(form, idle=False, unrolled=False, wraps=False, rounded=False):
    return dict(form=form, idle=idle, unrolled=unrolled, wraps=wraps, rounded=rounded)


_S, _16 = _claim('scalar'), ('bf16', 'fp16')
BIAS_ACT_CASES = {
    # scalar by channel count
    'c7_p9': (7, 9, DTYPES, 0, {d: _S for d in DTYPES}),
    'c36_p70': (36, 70, DTYPES, 0, {'bf16': _S, 'fp16': _S, 'fp32': _claim('fast', idle=True, rounded=True)}),   # 36 % 4 == 0: fp32 is fast
    # scalar by size, and the n / per >= 256 boundary
    'c256_p1': (256, 1, DTYPES, 0, {d: _S for d in DTYPES}),
    'cper_p255': ('per', 255, DTYPES, 0, {d: _S for d in DTYPES}),
    'cper_p256': ('per', 256, DTYPES, 0, {d: _claim('fast') for d in DTYPES}),
    # fast, power-of-two row: 2 x 64 x 17 x 23
    'c64_p782': (64, 2 * 17 * 23, DTYPES, 0, {d: _claim('fast', unrolled=True, wraps=True) for d in DTYPES}),
    # fast, unit > 1: tail only, workgroups with nothing to do
    'c720_p45': (720, 45, _16, 0, {d: _claim('fast', idle=True, rounded=True) for d in _16}),
    # fast, unit > 1, unrolled loop entered: 2 x 720 x 16 x 16 and 36 channels of fp32 (vpr 9)
    'c720_p512': (720, 2 * 16 * 16, _16, 0, {d: _claim('fast', unrolled=True, wraps=True, rounded=True) for d in _16}),
    'c36_p1024': (36, 1024, ('fp32',), 0, {'fp32': _claim('fast', unrolled=True, wraps=True, rounded=True)}),
    # scalar loop wraps under a cap
    'c7_p300_cap2': (7, 300, DTYPES, 2, {d: _claim('scalar', wraps=True) for d in DTYPES}),
}
# the fast shapes again under grid_cap 1 and 3: the grid is rounded UP to the unit after the cap
for _cap in (1, 3):
    BIAS_ACT_CASES['c64_p782_cap%d' % _cap] = (64, 782, DTYPES, _cap, {d: _claim('fast', unrolled=True, wraps=True) for d in DTYPES})
    BIAS_ACT_CASES['c720_p45_cap%d' % _cap] = (720, 45, _16, _cap, {d: _claim('fast', idle=True, rounded=True) for d in _16})
    BIAS_ACT_CASES['c720_p512_cap%d' % _cap] = (720, 512, _16, _cap, {d: _claim('fast', unrolled=True, wraps=True, rounded=True) for d in _16})
    BIAS_ACT_CASES['c36_p1024_cap%d' % _cap] = (36, 1024, ('fp32',), _cap, {'fp32': _claim('fast', unrolled=True, wraps=True, rounded=True)})


def bias_act_case(name, dtype):
    channels, pixels, dtypes, cap, claims = BIAS_ACT_CASES[name]
    assert dtype in dtypes
    return (PER[dtype] if channels == 'per' else channels), pixels, cap, claims[dtype]


def bias_act_case_ids():
    return [(name, d) for name, case in BIAS_ACT_CASES.items() for d in case[2]]


def describe_grid(grid, channels, pixels, dtype):
    """odtk_debug_bias_act_grid's answer (dict form / blocks / stride / trips) -> the claim it amounts to."""
    n = channels * pixels
    per = PER[dtype]
    work = n // per if grid['form'] == 'fast' else n
    assert grid['stride'] == grid['blocks'] * 256
    rounded = False
    if grid['form'] == 'fast':
        vpr = channels // per
        assert channels % per == 0 and grid['stride'] % vpr == 0, 'the grid stride must be a multiple of the row length'
        unit = vpr // np.gcd(vpr, 256)
        rounded = unit > 1 and grid['blocks'] % unit == 0 and grid['blocks'] > 0
    return _claim(grid['form'], idle=(grid['blocks'] - 1) * 256 >= work, unrolled=grid['trips'] > 0, wraps=work > grid['stride'],
                  rounded=bool(rounded))


# ---- special values ------------------------------------------------------------------------------------------------------------
def _f32_bits(values):
    return np.array(values, dtype=F32).view(np.uint32)


_NAN32 = np.array([0x7fc00000, 0x7f800001, 0xff800001, 0x7fbfffff, 0xffffffff], dtype=np.uint32)   # quiet, payload in the low half, ...
STEM_NAN_BITS = {'fp32': _NAN32, 'bf16': np.array([0x7fc0, 0x7f81, 0xff81, 0x7fbf, 0xffff], dtype=np.uint16),
                 'fp16': np.array([0x7e00, 0x7c01, 0xfc01, 0x7dff, 0xffff], dtype=np.uint16)}


def bias_act_special(dtype):
    """-> (x bits [P] of `dtype`, bias float32 [C], C a multiple of 8): the test runs y[p][c] = x[p] against bias[c], the whole cross.
    Rows: +-0, +-1, +-inf, NaNs of both signs, the largest finite, the smallest subnormal, and per storage type the operands of sums
    that tie up, tie down, overflow to inf, and round to a subnormal."""
    two = lambda e: float(2.0 ** e)
    if dtype == 'fp32':
        x = np.concatenate([_f32_bits([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 3.4028234663852886e38, -3.4028234663852886e38]),
                            np.array([0x00000001, 0x80000001, 0x00800000, 0x7fc00000, 0xffc00000, 0x7f800001], dtype=np.uint32),
                            _f32_bits([1.0 + two(-23), 16777216.0])])
        bias = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, two(-24), 3 * two(-24), 3.4028234663852886e38, two(103), -two(-127), 1.0]
    elif dtype == 'bf16':
        #          +0      -0      1       -1      +inf    -inf    max     -max    min sub -min sub +NaN   -NaN    sNaN    1+2^-7  2^-126
        x = np.array([0x0000, 0x8000, 0x3f80, 0xbf80, 0x7f80, 0xff80, 0x7f7f, 0xff7f, 0x0001, 0x8001, 0x7fc0, 0xffc0, 0x7f81, 0x3f81, 0x0080],
                     dtype=np.uint16)
        # 2^-8: half a step at 1 (1 ties DOWN to 1, 1 + 2^-7 ties UP to 1 + 2^-6); 2^119: half a step at the largest finite (ties to
        # inf), 2^118 stays finite; -2^-127 on 2^-126: the subnormal 2^-127; 2^-134: half the smallest subnormal (ties to 0)
        bias = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, two(-8), two(119), two(118), -two(-127), two(-134), 3 * two(-134)]
    else:
        #          +0      -0      1       -1      +inf    -inf    max     -max    min sub -min sub +NaN   -NaN    sNaN    1+2^-10 2^-14
        x = np.array([0x0000, 0x8000, 0x3c00, 0xbc00, 0x7c00, 0xfc00, 0x7bff, 0xfbff, 0x0001, 0x8001, 0x7e00, 0xfe00, 0x7c01, 0x3c01, 0x0400],
                     dtype=np.uint16)
        # 2^-11: half a step at 1; 16 on 65504 = 65520: ties to inf, 15 stays finite; -2^-15 on 2^-14: the subnormal 2^-15; 2^-25: half
        # the smallest subnormal (ties to 0), 3 * 2^-25 ties up to 2 * 2^-24
        bias = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, two(-11), 16.0, 15.0, -two(-15), two(-25), 3 * two(-25)]
    bias = np.array(bias, dtype=F32)
    nan_bias = np.array([0x7fc00000, 0xffc00000], dtype=np.uint32).view(F32)
    bias = np.concatenate([bias, nan_bias, np.zeros(16 - len(bias) - 2, dtype=F32)])
    assert len(bias) == 16
    return x.astype(BITS[dtype]), bias


def stem_special(in_dtype):
    """Input bit patterns of `in_dtype` for stem_pack's cast: ties of both directions for each output type, overflow to inf,
    subnormal results, +-0, +-inf and the NaN patterns."""
    two = lambda e: float(2.0 ** e)
    if in_dtype == 'fp32':
        vals = _f32_bits([0.0, -0.0, np.inf, -np.inf,
                          1 + two(-8), 1 + two(-7) + two(-8), -(1 + two(-8)), -(1 + two(-7) + two(-8)),           # bf16 ties: down, up
                          1 + two(-11), 1 + two(-10) + two(-11), -(1 + two(-11)), -(1 + two(-10) + two(-11)),     # fp16 ties: down, up
                          65520.0, -65520.0, 65519.0, 1e38,                                                       # fp16: inf, inf, max, inf
                          two(-15), two(-24), two(-25), 3 * two(-25), two(-25) * 1.5,                              # fp16 subnormals and their ties
                          two(-127), two(-133), two(-134), 3 * two(-134), two(-149)])                              # bf16 subnormals and their ties
        vals = np.concatenate([vals, np.array([0x7f7f8000, 0xff7f8000, 0x7f7f7fff], dtype=np.uint32), _NAN32])   # bf16: inf, -inf, max
    elif in_dtype == 'bf16':
        # to fp16: 2^-25 ties down to 0, 3 * 2^-25 ties up, 2^-15 a subnormal, 65536 and 1e38 overflow, 65280 stays finite
        vals = np.array([0x0000, 0x8000, 0x7f80, 0xff80, 0x3f80, 0x3f81, 0x3300, 0x33c0, 0x3800, 0xb300, 0x4780, 0xc780, 0x477f, 0x7e96,
                         0x0001, 0x0040], dtype=np.uint16)
        vals = np.concatenate([vals, STEM_NAN_BITS['bf16']])
    else:
        # to bf16: 1 + 2^-8 ties down, 1 + 2^-7 + 2^-8 ties up (and negated); nothing overflows or goes subnormal in bf16
        vals = np.array([0x0000, 0x8000, 0x7c00, 0xfc00, 0x3c00, 0x3c04, 0x3c0c, 0xbc04, 0xbc0c, 0x7bff, 0xfbff, 0x0001, 0x8001, 0x03ff],
                        dtype=np.uint16)
        vals = np.concatenate([vals, STEM_NAN_BITS['fp16']])
    return vals.astype(BITS[in_dtype])


def place_table(flat_bits, table, shift):
    """Writes the table (rolled by `shift`) into the flat tensor at evenly spread positions; -> the positions.  A tensor smaller
    than the table takes as much of it as it has elements."""
    n = min(flat_bits.size, len(table))
    at = np.unique(np.linspace(0, flat_bits.size - 1, n).astype(np.int64))
    flat_bits[at] = np.roll(table, shift)[:len(at)]
    return at


def tie_kind(exact, out_bits, dtype):
    """For float64 sums `exact` and their rounded bits: +1 where the sum lies exactly halfway between two neighbouring values of
    `dtype` and went to the one larger in magnitude, -1 where it went to the smaller, 0 elsewhere (16-bit types)."""
    exact = np.asarray(exact, dtype=np.float64)
    bits = np.asarray(out_bits).astype(np.uint16)
    mag = bits & np.uint16(0x7fff)
    with np.errstate(invalid='ignore', over='ignore'):
        got = widen(out_bits, dtype).astype(np.float64)
        finite = np.isfinite(exact) & np.isfinite(got)
        up = widen(np.where(mag < 0x7fff, bits + np.uint16(1), bits).astype(np.uint16), dtype).astype(np.float64)
        down = widen(np.where(mag > 0, bits - np.uint16(1), bits).astype(np.uint16), dtype).astype(np.float64)
        went_down = finite & (mag < 0x7fff) & np.isfinite(up) & (np.abs(exact) > np.abs(got)) & (np.abs(exact) - np.abs(got) == np.abs(up) - np.abs(exact))
        went_up = finite & (mag > 0) & (np.abs(exact) < np.abs(got)) & (np.abs(got) - np.abs(exact) == np.abs(exact) - np.abs(down))
    return went_up.astype(np.int8) - went_down.astype(np.int8)


# ---- the other kernels' cases --------------------------------------------------------------------------------------------------
POOL_EXTENTS = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 9), (9, 1), (2, 7), (7, 2), (3, 3), (4, 5), (7, 9), (16, 16)]
POOL_BATCH_CHANNELS = [(1, 8), (3, 24)]
# (batch, channels, height, width, grid_cap, wraps): 3 x 24 x 7 x 9 is 3 * 4 * 5 * 3 = 180 output vectors, which one workgroup of 256
# lanes covers without wrapping; 3 x 24 x 16 x 16 (576 vectors) is the one whose loop body runs more than once per lane
POOL_CAPPED = [(3, 24, 7, 9, 1, False), (3, 24, 16, 16, 1, True)]
UPSAMPLE_EXTENTS = [(1, 1), (1, 5), (5, 1), (3, 4), (13, 20)]
ROW_BYTES = (16, 48, 512)
STEM_EXTENTS = [(2, 2), (2, 6), (6, 2), (4, 10), (64, 96)]
# (batch, height, width, grid_cap, wraps): 3 x (4, 10) is 30 output pixels -- one workgroup, no wrap; 3 x (64, 96) is 4608
STEM_CAPPED = [(3, 4, 10, 1, False), (3, 64, 96, 1, True)]


def pool_work(batch, channels, height, width):
    return batch * ((height + 1) // 2) * ((width + 1) // 2) * (channels // 8)


def stream_blocks(work, per_block, own_cap, grid_cap):
    """The grid of a streaming launcher: ceil(work / per_block) workgroups, at most its own cap, or the debug cap in its place."""
    return min(-(-work // per_block), grid_cap or own_cap)


def canvas_layouts():
    """name -> (height, width, rects): one rectangle flush against each edge, the whole canvas, none, and six with a 1 x 1 among
    them and gutters of 1 and 2 pixels."""
    h, w = 9, 14
    six = [(0, 0, 5, 6), (0, 7, 3, 3), (0, 12, 1, 1), (4, 7, 2, 2), (4, 10, 1, 3), (7, 0, 2, 4)]
    layouts = {'top': (h, w, [(0, 3, 2, 5)]), 'bottom': (h, w, [(6, 4, 3, 6)]), 'left': (h, w, [(2, 0, 4, 3)]),
               'right': (h, w, [(1, 9, 5, 5)]), 'whole': (h, w, [(0, 0, h, w)]), 'none': (h, w, []), 'six': (h, w, six)}
    assert len(six) == MAX_LEVELS
    return layouts
