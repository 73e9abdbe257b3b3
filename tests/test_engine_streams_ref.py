"""Without a GPU: (1) the restatements of tests/engine_streams_ref.py against torch's CPU operators on finite random data, (2) every
case tests/test_gpu_engine_streams.py names shown not to be vacuous -- through the library's own grid query for bias_act, by the
launchers' grid arithmetic for the other kernels, by inspection of the special-value tables -- and (3) the tuning entry point
(odtk_debug_stream_tuning / _get / odtk_debug_bias_act_grid): set, get, restore, refusals, and today's grids for real layer shapes."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import engine_streams_ref as ref
from odtk import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}


def _tensor(bits, dtype):
    """bits -> torch tensor of the dtype (same shape)."""
    bits = np.ascontiguousarray(bits)
    return torch.from_numpy(bits.view(np.int32 if dtype == 'fp32' else np.int16).copy()).view(TORCH[dtype])


def _bits(t, dtype):
    return t.contiguous().view(torch.int32 if dtype == 'fp32' else torch.int16).numpy().view(ref.BITS[dtype])


def _randn_bits(rng, shape, dtype, scale=2.0):
    return ref.round_bits((rng.standard_normal(shape) * scale).astype(np.float32), dtype)


@pytest.fixture
def restored_tuning():
    found = _C.stream_tuning_state()
    yield found
    _C.stream_tuning(**found)
    assert _C.stream_tuning_state() == found


# ---- (1) the restatements against torch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_the_hand_rounding_is_torchs_cast(dtype):
    """10^5 values across the whole exponent range (subnormals of the storage type, overflow, both signs), the special table of the
    stem pack, and every tie of the 16-bit type near 1: round_bits == torch's .to(dtype) bit for bit, NaN for NaN."""
    rng = np.random.default_rng(1)
    with np.errstate(over='ignore'):
        f = (rng.standard_normal(100000) * np.exp2(rng.integers(-150, 128, 100000))).astype(np.float32)
    step = 2.0 ** (-8 if dtype == 'bf16' else -11)
    f = np.concatenate([f, 1 + step * np.arange(1, 64, 2, dtype=np.float32), ref.widen(ref.stem_special('fp32'), 'fp32')])
    want = _bits(torch.from_numpy(f).to(TORCH[dtype]), dtype)
    got = ref.round_bits(f, dtype)
    ref.assert_bits(got, want, dtype, 'round_bits ' + dtype)
    assert ref.is_nan_bits(got, dtype).sum() == np.isnan(f).sum() == 5
    assert np.array_equal(ref.widen(got, dtype)[~np.isnan(f)], _tensor(want, dtype).float().numpy()[~np.isnan(f)])


@pytest.mark.parametrize('dtype', ref.DTYPES)
def test_bias_act_restatement_against_torch(dtype):
    rng = np.random.default_rng(2)
    y, res = _randn_bits(rng, (70, 36), dtype), _randn_bits(rng, (70, 36), dtype)
    bias = rng.standard_normal(36).astype(np.float32)
    for r in (None, res):
        for relu in (False, True):
            o = _tensor(y, dtype).float() + torch.from_numpy(bias)
            if r is not None:
                o = o + _tensor(r, dtype).float()
            if relu:
                o = torch.relu(o)                     # (differs from the kernel's rule only in the sign of a -0.0 sum: none here)
                assert not ((o == 0) & torch.signbit(o)).any()
            assert np.array_equal(ref.bias_act(y, bias, r, relu, dtype), _bits(o.to(TORCH[dtype]), dtype))


def test_relu_rule_of_the_restatement():
    """The one documented difference from torch.relu: a sum of -0.0 becomes +0.0; a NaN goes through; both as the kernel says."""
    y = np.array([[0x80000000, 0x7fc00000, 0xbf800000, 0x3f800000]], dtype=np.uint32)            # -0.0, NaN, -1, 1
    out = ref.bias_act(y, np.array([-0.0] * 4, dtype=np.float32), None, True, 'fp32')
    assert out[0, 0] == 0 and ref.is_nan_bits(out, 'fp32')[0, 1] and out[0, 2] == 0 and out[0, 3] == 0x3f800000
    assert torch.signbit(torch.relu(torch.tensor(-0.0)))                                          # torch keeps the sign


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_maxpool_restatement_against_torch(dtype):
    """F.max_pool2d on the float-widened epilogue output, at every extent the GPU test uses."""
    rng = np.random.default_rng(3)
    for batch, c in ref.POOL_BATCH_CHANNELS:
        for h, w in ref.POOL_EXTENTS:
            y = _randn_bits(rng, (batch, h, w, c), dtype)
            bias = rng.standard_normal(c).astype(np.float32)
            for relu in (False, True):
                e = _tensor(ref.bias_act(y.reshape(-1, c), bias, None, relu, dtype).reshape(y.shape), dtype).float()
                want = F.max_pool2d(e.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(TORCH[dtype])
                assert np.array_equal(ref.bias_act_maxpool(y, bias, relu, dtype), _bits(want, dtype)), (batch, c, h, w, relu)


def test_maxpool_restatement_on_zeros_and_nans():
    """+0 beats -0 (the key order), and any NaN of the window wins, whatever its sign."""
    y = np.full((1, 3, 3, 8), 0x8000, dtype=np.uint16)                    # -0.0 everywhere
    y[0, 1, 1, 0] = 0x0000                                                # one +0.0: channel 0 of every window of the 2 x 2 output sees it
    y[0, 0, 0, 1], y[0, 2, 2, 2] = 0x7fc0, 0xffc1                         # a positive NaN in the first window, a negative in the last
    out = ref.bias_act_maxpool(y, np.full(8, -0.0, dtype=np.float32), False, 'bf16')
    assert (out[..., 0] == 0x0000).all() and (out[..., 3:] == 0x8000).all()
    nan = ref.is_nan_bits(out, 'bf16')
    assert nan[0, 0, 0, 1] and nan[..., 1].sum() == 1 and nan[0, 1, 1, 2] and nan[..., 2].sum() == 1


@pytest.mark.parametrize('dtype', ref.DTYPES)
def test_upsample_canvas_and_stem_restatements_against_torch(dtype):
    rng = np.random.default_rng(4)
    x = _randn_bits(rng, (3, 5, 4, 8), dtype)
    want = F.interpolate(_tensor(x, dtype).float().permute(0, 3, 1, 2), scale_factor=2).permute(0, 2, 3, 1).to(TORCH[dtype])
    assert np.array_equal(ref.upsample2x(x), _bits(want, dtype))
    # the canvas: zeros plus slice assignment
    for name, (height, width, rects) in ref.canvas_layouts().items():
        for y0, x0, h, w in rects:
            assert 0 <= y0 and 0 <= x0 and h > 0 and w > 0 and y0 + h <= height and x0 + w <= width, name
        sources = [_randn_bits(rng, (2, h, w, 8), dtype) for _, _, h, w in rects]
        packed = ref.canvas_pack(2, height, width, 8, rects, sources, ref.BITS[dtype])
        t = torch.zeros(2, height, width, 8, dtype=TORCH[dtype])
        for (y0, x0, h, w), s in zip(rects, sources):
            t[:, y0:y0 + h, x0:x0 + w] = _tensor(s, dtype)
        assert np.array_equal(packed, _bits(t, dtype))
        dirty = _randn_bits(rng, (2, height, width, 8), dtype)
        cleared = ref.canvas_clear(dirty, rects)
        inside = packed != 0                                            # (randn never yields a zero here)
        assert np.array_equal(cleared[inside], dirty[inside]) and not cleared[~inside].any()
    # the stem pack: the permute / reshape of test_stem_pack_is_space_to_depth_plus_cast, then the cast
    xb = _randn_bits(rng, (2, 3, 6, 10), dtype, scale=1.5)
    xt = _tensor(xb, dtype).float()
    for out_dtype in ('bf16', 'fp16'):
        want = xt.view(2, 3, 3, 2, 5, 2).permute(0, 3, 5, 1, 2, 4).reshape(2, 12, 3, 5)
        want = torch.cat([want, torch.zeros(2, 4, 3, 5)], 1).to(TORCH[out_dtype]).permute(0, 2, 3, 1)
        assert np.array_equal(ref.stem_pack(xb, dtype, out_dtype), _bits(want, out_dtype))


# ---- (2) no case is vacuous ----------------------------------------------------------------------------------------------------
def _todays_grid(pixels, channels, dtype, cap=0):
    """bias_act's launch as it was before the cap could be replaced, restated: -> (form, blocks)."""
    per, n = ref.PER[dtype], pixels * channels
    if channels % per == 0 and n // per >= 256:
        vpr = channels // per
        unit = vpr // math.gcd(vpr, 256)
        blocks = min(-(-(n // per) // 1024), cap or 256 * 16)
        return 'fast', -(-blocks // unit) * unit
    return 'scalar', min(-(-n // 256), cap or 4096)


@pytest.mark.parametrize('name,dtype', ref.bias_act_case_ids(), ids=['%s-%s' % c for c in ref.bias_act_case_ids()])
def test_every_bias_act_case_takes_the_path_it_names(name, dtype, restored_tuning):
    """odtk_debug_bias_act_grid -- the host function the launcher itself calls -- under the case's cap: the form, the idle
    workgroups, the unrolled trips (> 0 or == 0), the wrap and the rounding to the unit are what the table claims; and the same shape
    without (or with) the cap is the launch the restated arithmetic gives."""
    channels, pixels, cap, claim = ref.bias_act_case(name, dtype)
    for c in {0, cap}:
        _C.stream_tuning(grid_cap=c)
        grid = _C.bias_act_grid(pixels, channels, TORCH[dtype])
        assert (grid['form'], grid['blocks']) == _todays_grid(pixels, channels, dtype, c), (name, dtype, c, grid)
        if c == cap:
            assert ref.describe_grid(grid, channels, pixels, dtype) == claim, (name, dtype, grid)
    if claim['form'] == 'fast':
        # the invariant of the fast form, and the trips against a walk of lane 0's loop
        stride, n_vec = grid['stride'], channels * pixels // ref.PER[dtype]
        assert stride % (channels // ref.PER[dtype]) == 0
        q = trips = 0
        while q + 3 * stride < n_vec:
            q, trips = q + 4 * stride, trips + 1
        assert trips == grid['trips']


def test_the_bias_act_table_covers_what_the_issue_names():
    """Across the table: both forms; the boundary straddled; the unrolled loop with a power-of-two row AND with unit > 1; idle
    workgroups; a wrap of the scalar loop; a capped grid that the rounding lifts back to the unit."""
    claims = [(name, d, ref.bias_act_case(name, d)) for name, d in ref.bias_act_case_ids()]
    def some(**want):
        return any(all(claim[k] == v for k, v in want.items()) for _, _, (_, _, _, claim) in claims)
    assert some(form='scalar', wraps=True) and some(form='fast', unrolled=True, rounded=False) and some(form='fast', unrolled=True, rounded=True)
    assert some(form='fast', unrolled=False, idle=True, rounded=True) and some(form='fast', unrolled=False, idle=False)
    assert ref.bias_act_case('cper_p255', 'bf16')[3]['form'] == 'scalar' and ref.bias_act_case('cper_p256', 'bf16')[3]['form'] == 'fast'
    assert any(cap == 1 and claim['rounded'] for _, _, (_, _, cap, claim) in claims)


def test_the_other_kernels_wrap_exactly_where_claimed():
    """Work against workgroups x 256 lanes, by each launcher's grid arithmetic."""
    for batch, c, h, w, cap, wraps in ref.POOL_CAPPED:
        work = ref.pool_work(batch, c, h, w)
        assert (work > ref.stream_blocks(work, 256, 256 * 32, cap) * 256) == wraps
    for batch, h, w, cap, wraps in ref.STEM_CAPPED:
        work = batch * (h // 2) * (w // 2)
        assert (work > ref.stream_blocks(work, 256, 256 * 32, cap) * 256) == wraps
    assert any(c[-1] for c in ref.POOL_CAPPED) and any(c[-1] for c in ref.STEM_CAPPED)
    # without a cap nothing here wraps: the cap is what reaches the loops
    for batch, c in ref.POOL_BATCH_CHANNELS:
        for h, w in ref.POOL_EXTENTS:
            work = ref.pool_work(batch, c, h, w)
            assert work <= ref.stream_blocks(work, 256, 256 * 32, 0) * 256
    # upsample and canvas: ~4 vectors per lane, so the largest shapes wrap even uncapped, and every cap wraps somewhere
    for cap in (0, 1, 3):
        wrapped = [4 * b * h * w * (rb // 16) > ref.stream_blocks(4 * b * h * w * (rb // 16), 1024, 256 * 16, cap) * 256
                   for b in (1, 3) for h, w in ref.UPSAMPLE_EXTENTS for rb in ref.ROW_BYTES]
        assert any(wrapped) and not all(wrapped)
    for cap in (0, 1):
        wrapped = [b * h * w * (rb // 16) > ref.stream_blocks(b * h * w * (rb // 16), 1024, 256 * 16, cap) * 256
                   for b in (1, 2) for rb in (16, 48) for h, w, _ in ref.canvas_layouts().values()]
        assert any(wrapped) and not all(wrapped)


def test_the_canvas_layouts_are_what_they_name():
    layouts = ref.canvas_layouts()
    h, w = layouts['whole'][:2]
    (top,), (bottom,), (left,), (right,) = (layouts[k][2] for k in ('top', 'bottom', 'left', 'right'))
    assert top[0] == 0 and bottom[0] + bottom[2] == h and left[1] == 0 and right[1] + right[3] == w
    assert layouts['whole'][2] == [(0, 0, h, w)] and layouts['none'][2] == []
    six = layouts['six'][2]
    assert len(six) == ref.MAX_LEVELS == _C.MAX_LEVELS and (1, 1) in [(r[2], r[3]) for r in six]
    cover = np.zeros((h, w), dtype=int)
    for y0, x0, rh, rw in six:
        cover[y0:y0 + rh, x0:x0 + rw] += 1
    assert cover.max() == 1                                             # no two rectangles overlap
    gaps = set()                                                         # gutters between horizontal / vertical neighbours
    for a in six:
        for b in six:
            if a is not b and a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and b[1] >= a[1] + a[3]:
                gaps.add(b[1] - (a[1] + a[3]))
            if a is not b and a[1] < b[1] + b[3] and b[1] < a[1] + a[3] and b[0] >= a[0] + a[2]:
                gaps.add(b[0] - (a[0] + a[2]))
    assert {1, 2} <= gaps and 0 not in gaps


@pytest.mark.parametrize('dtype', ref.DTYPES)
def test_bias_act_special_table_holds_what_it_names(dtype):
    x, bias = ref.bias_act_special(dtype)
    y = np.repeat(x[:, None], 16, axis=1)
    out = ref.bias_act(y, bias, None, False, dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        xf, of = ref.widen(x, dtype).astype(np.float64)[:, None], ref.widen(out, dtype)
        exact = xf + bias.astype(np.float64)[None, :]                   # (exact: float64 holds every sum of the table)
    zero = (of == 0)
    assert (zero & np.signbit(of)).any() and (zero & ~np.signbit(of)).any()                       # -0 (from -0 + -0) and +0
    assert (zero & (xf != 0)).any()                                                                # exact cancellation
    assert np.isposinf(of).any() and np.isneginf(of).any()
    assert (np.isnan(of) & np.isinf(xf) & np.isinf(bias)[None, :]).any()                           # inf - inf
    nan_out = out[ref.is_nan_bits(out, dtype)]
    top = 31 if dtype == 'fp32' else 15
    assert ((nan_out >> top) == 0).any() and ((nan_out >> top) == 1).any()                         # NaNs of both signs
    assert (np.isnan(ref.widen(x, dtype)).sum() >= 2) and np.isnan(bias).sum() == 2
    largest = {'fp32': 0x7f7fffff, 'bf16': 0x7f7f, 'fp16': 0x7bff}[dtype]
    assert (out == largest).any() and (out == 1).any()                                             # largest finite, smallest subnormal
    # the ReLU sees -0, NaN and negatives
    relu = ref.bias_act(y, bias, None, True, dtype)
    assert not ((ref.widen(relu, dtype) == 0) & np.signbit(ref.widen(relu, dtype))).any()
    assert np.array_equal(ref.is_nan_bits(relu, dtype), ref.is_nan_bits(out, dtype))
    if dtype != 'fp32':
        ties = ref.tie_kind(exact, out, dtype)
        assert (ties == 1).any() and (ties == -1).any()                                            # a tie in each direction
        assert (np.isfinite(exact) & np.isinf(of)).any()                                           # overflow of the storage type
        expo = {'bf16': 0x7f80, 'fp16': 0x7c00}[dtype]
        subnormal = ((out & expo) == 0) & ((out & 0x7fff) != 0)
        assert (subnormal & (exact != of)).any() or (subnormal & (xf != exact)).any()              # a SUM that comes out subnormal
        assert (subnormal & (np.abs(xf) >= ref.widen(np.array([{'bf16': 0x0080, 'fp16': 0x0400}[dtype]], dtype=np.uint16), dtype)[0])).any()


@pytest.mark.parametrize('in_dtype', ref.DTYPES)
def test_stem_special_table_holds_what_it_names(in_dtype):
    table = ref.stem_special(in_dtype)
    assert len(set(table.tolist())) == len(table)
    f = ref.widen(table, in_dtype)
    with np.errstate(invalid='ignore'):
        exact = f.astype(np.float64)                                    # (a signalling NaN raises the flag)
    assert np.array_equal(table[np.isnan(f)], ref.STEM_NAN_BITS[in_dtype])
    if in_dtype == 'fp32':
        assert table[np.isnan(f)].tolist() == [0x7fc00000, 0x7f800001, 0xff800001, 0x7fbfffff, 0xffffffff]
    for out_dtype in ('bf16', 'fp16'):
        out = ref.round_bits(f, out_dtype)
        of = ref.widen(out, out_dtype)
        assert np.array_equal(ref.is_nan_bits(out, out_dtype), np.isnan(f))                       # each NaN comes out a NaN
        assert {0x0000, 0x8000} <= set(out.tolist()) and np.isposinf(of[np.isposinf(f)]).all() and np.isneginf(of[np.isneginf(f)]).all()
        if out_dtype == in_dtype:
            ref.assert_bits(out, table, out_dtype, 'a cast to itself')                             # a copy (a NaN's payload apart)
            continue
        ties = ref.tie_kind(exact, out, out_dtype)
        expo = {'bf16': 0x7f80, 'fp16': 0x7c00}[out_dtype]
        subnormal = ((out & expo) == 0) & ((out & 0x7fff) != 0)
        overflow = np.isfinite(f) & np.isinf(of)
        if in_dtype == 'fp32' or out_dtype == 'fp16':
            assert (ties == 1).any() and (ties == -1).any() and overflow.any() and subnormal.any(), (in_dtype, out_dtype)
        else:                                                            # fp16 -> bf16: every fp16 value is a normal, finite bf16 one
            assert (ties == 1).any() and (ties == -1).any() and not overflow.any()
    # the table reaches the tensors: the smallest image takes a part of it, rolled on from case to case; the others take all of it
    flat = np.zeros(12, dtype=ref.BITS[in_dtype])
    assert len(ref.place_table(flat, table, 5)) == 12 and np.array_equal(flat, np.roll(table, 5)[:12])
    flat = np.zeros(3 * 4 * 10, dtype=ref.BITS[in_dtype])
    at = ref.place_table(flat, table, 3)
    assert len(at) == len(table) and sorted(flat[at].tolist()) == sorted(table.tolist())


# ---- (3) the tuning entry point ------------------------------------------------------------------------------------------------
def test_stream_tuning_sets_gets_restores_and_refuses(restored_tuning):
    lib = _C.library()
    assert restored_tuning == {'grid_cap': 0, 'pool_wide_index': 0}                               # the shipped default
    _C.stream_tuning(grid_cap=3)
    assert _C.stream_tuning_state() == {'grid_cap': 3, 'pool_wide_index': 0}
    _C.stream_tuning(pool_wide_index=1)                                                           # -1 leaves the other field alone
    assert _C.stream_tuning_state() == {'grid_cap': 3, 'pool_wide_index': 1}
    _C.stream_tuning(65536, 0)
    assert _C.stream_tuning_state() == {'grid_cap': 65536, 'pool_wide_index': 0}
    _C.stream_tuning(7, 1)
    for bad in ((-2, 0), (65537, 0), (0, 2), (0, -2), (-2, -2), (1 << 20, 1)):
        assert lib.odtk_debug_stream_tuning(*bad) == _C.ERR_INVALID, bad
        assert _C.stream_tuning_state() == {'grid_cap': 7, 'pool_wide_index': 1}, bad            # nothing changed
    with pytest.raises(RuntimeError):
        _C.stream_tuning(grid_cap=70000)
    assert lib.odtk_debug_stream_tuning_get(None) == _C.ERR_INVALID
    out = (ctypes.c_uint * 4)()
    assert lib.odtk_debug_bias_act_grid(0, 8, _C.BF16, out) == _C.ERR_INVALID
    assert lib.odtk_debug_bias_act_grid(4, 0, _C.BF16, out) == _C.ERR_INVALID
    assert lib.odtk_debug_bias_act_grid(4, 8, _C.BF16, None) == _C.ERR_INVALID
    assert lib.odtk_debug_bias_act_grid(4, 8, 9, out) == _C.ERR_UNSUPPORTED
    _C.stream_tuning(0, 0)
    assert _C.stream_tuning_state() == {'grid_cap': 0, 'pool_wide_index': 0}


def test_default_tuning_gives_todays_grids_for_the_engines_layers(restored_tuning):
    """Three activation shapes of the flagship plan (bf16, batch 8, 800 x 1280): with grid_cap = 0 the query returns the launch the
    library made before the cap could be replaced -- the smallest head level, a middle one, and one beyond the 4096-workgroup cap."""
    plan = json.load(open(os.path.join(ROOT, 'plans', 'rn50fpn_bf16_bs8_800x1280.json')))
    shapes = {key for layer in plan['layers'].values() for key in layer}
    _C.stream_tuning(0, 0)
    want = {'act:8x256x7x10': ('fast', 18, 1), 'act:8x512x50x80': ('fast', 2000, 1), 'act:8x256x200x320': ('fast', 4096, 4)}
    for key, (form, blocks, trips) in want.items():
        assert key in shapes
        b, c, h, w = (int(v) for v in key.split(':')[1].split('x'))
        grid = _C.bias_act_grid(b * h * w, c, torch.bfloat16)
        assert grid == {'form': form, 'blocks': blocks, 'stride': blocks * 256, 'trips': trips}, (key, grid)
        assert (form, blocks) == _todays_grid(b * h * w, c, 'bf16')
