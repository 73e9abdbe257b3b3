"""Every launch shape of the loss kernels (csrc/loss.hpp) against a float64 restatement written here.

csrc/loss.hpp is one template over many code paths -- element type, direction, gamma == 2 or general, NCHW or channels_last, 1 / 2 / 4
vectors per trip, two arithmetic forms, two trip layouts (`window`), per-workgroup or per-wave partial sums (`per_wave`), two orders
of the backward's box-delta walk (`box_rows`), a fast and a carry path per vector and a scalar tail -- and the header says that
results do not depend on any of them beyond the order of the partial sums.  tests/test_gpu_loss.py runs the shipped launch shapes
only; this file runs a list that covers every value of every knob (and whatever the library reports as its defaults), on the
smallest level sizes that reach each path, and holds all of them to the bars loss.hpp states:

  forward   each of the two sums within 1e-6 relative of float64, the foreground count exact;
  backward  fp32 heads: within 1e-5 of the largest reference gradient, and exactly 0 where the reference is exactly 0;
            16-bit heads: the stored value between round(ref - 1e-5 scale) and round(ref + 1e-5 scale), one ulp of the element
            type outward -- an fp32 gradient that meets the fp32 bar, then one rounding;
  across launch shapes (fixed form, element type, layout): d(logits) and d(deltas) are the same BITS as with the first shape;
      (this found d(deltas) changing with box_rows in the sign of its zeros -- the vector-store walk wrote +0 where the element
      walks wrote g x 0, and for fp16 the compiler folded g x grad into the conversion in one walk only: loss.hpp box_grad_value);
  every output element is written: all launches go through the C ABI with buffers of this file, NaN-filled beforehand and followed
  by a NaN-filled guard of 256 bytes that must stay NaN; the workspace is exactly as large as the size query says.

The reference (`reference`) is independent of the kernels and of odtk/loss.py: the reference's loss.py:13-31 and model.py:193-209
restated in numpy float64 with the gradients written out by hand, on the head tensors as stored (16-bit values upcast exactly) and
with alpha / gamma / beta as the C ABI receives them (floats).  NaN / +-inf logits are not used here
(test_gpu_loss.py::test_loss_forms_agree_and_special_logits has their pattern; a float64 sum with them says nothing).

The process-wide launch shape and arithmetic form are read back (odtk_debug_loss_tuning_get / odtk_debug_loss_form_get) before
every test of this file and put back after it, whatever happened in between."""
import functools

import numpy as np
import pytest
import torch

ALPHA, BETA = 0.25, float(np.float32(0.11))            # as the kernels receive them: float arguments of the C ABI
G_CLS, G_BOX = float(np.float32(0.37)), float(np.float32(-1.9))      # upstream gradients (float32 device scalars)
FWD, BWD, WS = 0, 1, 2
GUARD_BYTES = 256

# name -> (B, A, C, H, W, box_params); each is the smallest that reaches its path (asserted in test_shapes_reach_their_paths)
SHAPES = {
    'one_cell': (1, 1, 1, 1, 1, 4),       # n_vec == 0: only the scalar tail; every divisor 1; the one anchor is foreground
    'tail': (1, 3, 5, 1, 3, 4),           # n = 45: tail of 1 (fp32) / 5 (16-bit); C % kPer and hw % kPer != 0: carries in both layouts
    'mixed': (2, 9, 20, 5, 7, 4),         # hw = 35: NCHW mixes fast and carry vectors, C = 20 does for channels_last 16-bit
    'rotated': (2, 27, 3, 3, 4, 6),       # box_params != 4: the element-store branch of the memory-order box-delta walk
    'trips': (3, 9, 20, 20, 28, 4),       # 75 600 / 37 800 vectors: 64 threads x 256 blocks walk > 2 trips, the last one partial
}
CASES = [(name, 2.0) for name in SHAPES] + [('mixed', 1.5), ('tail', 1.5)]
CASE_IDS = ['%s-gamma%g' % c for c in CASES]
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
SPECIAL_LOGITS = (64.0, -64.0, 64.5, 88.0, -88.0, 100.0, -100.0)     # finite values where the forms switch; exact in bf16 and fp16

# (threads, blocks_per_cu, unroll, box_blocks, per_wave, window, box_rows); blocks_per_cu None = the library's default for that
# kernel and head width.  per_wave reaches the workspace form only, box_rows the backward only.  Covers every value of every knob,
# every pair unroll x window, an odd number of waves (192 threads), and at 64 x 1 the per-level block cap on `trips`.
LAUNCH_SHAPES = [
    (64, 1, 1, 1, 0, 0, 1),
    (64, 1, 1, 256, 1, 1, 0),
    (64, 1, 2, 256, 0, 1, 1),
    (64, None, 2, 1, 1, 0, 0),
    (64, 1, 4, 1, 1, 1, 1),
    (256, None, 4, 256, 0, 0, 0),
    (256, 1, 1, 1, 1, 1, 1),
    (256, None, 2, 256, 1, 0, 1),
    (192, 1, 2, 1, 1, 1, 0),
    (1024, 1, 1, 256, 0, 0, 1),
    (1024, None, 2, 1, 1, 1, 0),
    (1024, 1, 4, 256, 1, 1, 1),
    (1024, None, 4, 1, 0, 0, 0),
]


def test_launch_shape_list_covers_every_knob():
    cols = list(zip(*LAUNCH_SHAPES))
    assert {64, 256, 1024} <= set(cols[0]) and {1, None} == set(cols[1]) and {1, 2, 4} == set(cols[2])
    assert {1, 256} == set(cols[3]) and {0, 1} == set(cols[4]) == set(cols[5]) == set(cols[6])
    assert {(u, w) for u in (1, 2, 4) for w in (0, 1)} == {(s[2], s[5]) for s in LAUNCH_SHAPES}
    assert any((s[0] // 64) % 2 == 1 and s[0] > 64 and s[4] == 1 for s in LAUNCH_SHAPES)        # per-wave sums, odd wave count


# ------------------------------------------------------------------------------------------------------------------------------
# inputs (CPU, deterministic) and the float64 reference
# ------------------------------------------------------------------------------------------------------------------------------

def _round_to(a32, dtype):
    """float32 numpy -> the value an element of `dtype` holds (round to nearest even, torch's own conversion), as float32"""
    return torch.from_numpy(np.ascontiguousarray(a32)).to(dtype).float().numpy()


def make_inputs(shape, dtype, seed):
    """-> logits [B, A, C, H, W], deltas [B, A, NB, H, W] (float32 arrays holding values of `dtype`), depth [B, A, 1, H, W],
    box_target [B, A, NB, H, W] (float32)."""
    b, a, c, h, w, nb = shape
    rng = np.random.RandomState(seed)
    cells = b * a * h * w
    # depth: ~5 % ignored (-1), ~3 % foreground with a random class, the rest background; all three kinds wherever they fit
    u = rng.rand(cells)
    depth = np.zeros(cells, np.float32)
    depth[u < 0.05] = -1.0
    fg = u > 0.97
    depth[fg] = rng.randint(1, c + 1, int(fg.sum())).astype(np.float32)
    if cells >= 3:
        three = rng.permutation(cells)[:3]
        depth[three[0]], depth[three[1]], depth[three[2]] = -1.0, 0.0, float(rng.randint(1, c + 1))
    else:
        depth[:] = float(rng.randint(1, c + 1))
    depth = depth.reshape(b, a, 1, h, w)
    # logits: randn * 3 - 3, with the finite values where the arithmetic forms switch sprinkled over ~1 % of them and next to
    # positives in both memory orders (the neighbouring pixel: NCHW; the neighbouring class: channels_last)
    x = (rng.randn(b, a, c, h, w) * 3.0 - 3.0).astype(np.float32)
    flat = x.reshape(-1)
    n = flat.size
    if n >= 8:
        where = rng.permutation(n)[:max(4, n // 100)]
        flat[where] = np.asarray(SPECIAL_LOGITS, np.float32)[rng.randint(0, len(SPECIAL_LOGITS), where.size)]
    pos = np.argwhere(depth[:, :, 0] > 0)                                    # (image, anchor, y, x) of the foreground cells
    for j, (bi, ai, yi, xi) in enumerate(pos[:: max(1, len(pos) // 24)]):
        ci = int(depth[bi, ai, 0, yi, xi]) - 1
        p = yi * w + xi
        xv = x[bi, ai].reshape(c, h * w)
        for k, (dc, dp) in enumerate(((0, 1), (0, -1), (1, 0), (-1, 0))):
            if 0 <= ci + dc < c and 0 <= p + dp < h * w:
                xv[ci + dc, p + dp] = SPECIAL_LOGITS[(j + k) % len(SPECIAL_LOGITS)]
    x = _round_to(x, dtype)
    # deltas: the target + 0.15 randn; in foreground cells some |d| exactly beta (either sign) and some exactly 0
    tgt = (rng.randn(b, a, nb, h, w) * 0.3).astype(np.float32)
    box = _round_to(tgt + (rng.randn(b, a, nb, h, w) * 0.15).astype(np.float32), dtype)
    for j, (bi, ai, yi, xi) in enumerate(pos):
        for k in range(nb):
            kind = (j + k) % 6
            if kind == 0:
                tgt[bi, ai, k, yi, xi] = box[bi, ai, k, yi, xi]              # d == 0 (a 16-bit value is a float32 value)
            elif kind in (1, 2):
                box[bi, ai, k, yi, xi] = 0.0
                tgt[bi, ai, k, yi, xi] = -np.float32(BETA) if kind == 1 else np.float32(BETA)     # d == +beta / -beta, exactly
    return x, box, depth, tgt


def _sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def reference(x, box, depth, tgt, gamma, g_cls, g_box, real=np.float64):
    """loss.py:13-31 combined as model.py:193-209, in `real` arithmetic -> (cls_sum, box_sum, foreground), d(logits), d(deltas).

        p = sigmoid(x);  pt = t p + (1 - t)(1 - p);  alpha_t = t alpha + (1 - t)(1 - alpha)
        BCE(x, t) = max(x, 0) - x t + log(1 + exp(-|x|))
        loss = alpha_t (1 - pt)^gamma BCE                                   masked by depth >= 0
        d loss / dx = alpha_t sgn (1 - pt)^gamma (gamma pt BCE + (1 - pt)),  sgn = +1 (t = 0), -1 (t = 1)
            (d(1 - pt)/dx = sgn pt (1 - pt),  dBCE/dx = p - t = sgn (1 - pt))
        smooth-L1: d = pred - target; |d| >= beta: |d| - beta / 2, gradient sign(d); else d^2 / (2 beta), gradient d / beta
                                                                             masked by depth > 0
    The one-hot target is model.py's: t = 1 at class depth - 1 of a foreground anchor.  `1 - p` is evaluated as sigmoid(-x), which
    is the same number without the cancellation.  The sums are always accumulated in float64."""
    b, a, c, h, w = x.shape
    x = x.astype(real)
    alpha, gam, beta = real(ALPHA), real(gamma), real(BETA)
    t = (np.arange(c, dtype=np.float32).reshape(1, 1, c, 1, 1) == depth - 1.0) & (depth > 0)
    p, one_minus_p = _sigmoid(x), _sigmoid(-x)
    pt = np.where(t, p, one_minus_p)
    one_minus_pt = np.where(t, one_minus_p, p)
    bce = np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))
    alpha_t = np.where(t, alpha, real(1) - alpha)
    mod = one_minus_pt ** gam
    cls_mask = np.broadcast_to(depth >= 0, x.shape)
    cls_loss = np.where(cls_mask, alpha_t * mod * bce, real(0))
    sgn = np.where(t, real(-1), real(1))
    dcls = np.where(cls_mask, real(g_cls) * alpha_t * sgn * mod * (gam * pt * bce + one_minus_pt), real(0))
    d = box.astype(real) - tgt.astype(real)
    ad = np.abs(d)
    box_mask = np.broadcast_to(depth > 0, d.shape)
    box_loss = np.where(box_mask, np.where(ad >= beta, ad - real(0.5) * beta, real(0.5) * ad * ad / beta), real(0))
    dbox = np.where(box_mask, real(g_box) * np.where(ad >= beta, np.sign(d), d / beta), real(0))
    sums = (float(cls_loss.astype(np.float64).sum()), float(box_loss.astype(np.float64).sum()), float((depth > 0).sum()))
    return sums, dcls, dbox


def _step(v16, up):
    """the neighbour of every element of a 16-bit float tensor, one ulp towards +inf (up) or -inf"""
    bits = v16.view(torch.int16).to(torch.int32)
    key = torch.where(bits >= 0, bits, -(bits & 0x7fff))                      # monotone in the value; +0 and -0 -> 0
    key = key + (1 if up else -1)
    bits = torch.where(key >= 0, key, (-key) | 0x8000)
    return ((bits + 0x8000) % 0x10000 - 0x8000).to(torch.int16).view(v16.dtype)


def bracket(ref64, dtype, scale):
    """what the 16-bit backward may store: [round(ref - 1e-5 scale) - 1 ulp, round(ref + 1e-5 scale) + 1 ulp], as float64"""
    r = torch.from_numpy(ref64)
    lo = _step((r - 1e-5 * scale).to(dtype), up=False).double()
    hi = _step((r + 1e-5 * scale).to(dtype), up=True).double()
    return lo, hi


def test_the_ulp_step_is_the_neighbouring_value():
    for dtype in (torch.bfloat16, torch.float16):
        v = torch.tensor([0.0, -0.0, 1.0, -1.0, 0.37, -1.9, 6e-8 if dtype == torch.float16 else 1e-38], dtype=dtype)
        up, down = _step(v, True), _step(v, False)
        assert bool((up.double() > v.double()).all()) and bool((down.double() < v.double()).all())
        assert torch.equal(_step(up, False).double(), v.double()) and torch.equal(_step(down, True).double(), v.double())
        one = torch.tensor([1.0], dtype=dtype)
        assert float(_step(one, True)) == 1.0 + float(torch.finfo(dtype).eps)


class Case:
    """One level: inputs as stored, the float64 reference, what the gradients may be.  Built once, never changed."""

    def __init__(self, name, gamma, dtype_name, shape=None, seed=None, g_cls=G_CLS, g_box=G_BOX):
        self.name, self.gamma, self.dtype_name, self.dtype = name, gamma, dtype_name, DTYPES[dtype_name]
        self.shape = shape or SHAPES[name]
        self.g_cls, self.g_box = g_cls, g_box
        seed = seed if seed is not None else 1000 + 7 * list(SHAPES).index(name) + int(gamma * 2)
        self.x, self.box, self.depth, self.tgt = make_inputs(self.shape, self.dtype, seed)
        self.sums, self.dcls, self.dbox = reference(self.x, self.box, self.depth, self.tgt, gamma, g_cls, g_box)
        self.scale = (float(np.abs(self.dcls).max()), float(np.abs(self.dbox).max()))


@functools.lru_cache(maxsize=None)
def case(name, gamma, dtype_name):
    return Case(name, gamma, dtype_name)


def _mem(arr5, channels_last):
    """[B, A, K, H, W] -> the flat order a head of that layout has in memory"""
    b, a, k, h, w = arr5.shape
    v = arr5.reshape(b, a * k, h, w)
    return np.ascontiguousarray(v.transpose(0, 2, 3, 1) if channels_last else v).reshape(-1)


def _kper(dtype_name):
    return 4 if dtype_name == 'fp32' else 8


@pytest.mark.parametrize('dtype_name', list(DTYPES))
def test_shapes_reach_their_paths(dtype_name):
    """The properties the shape table promises, from the inputs alone (no GPU): a later edit of a shape or of the input recipe
    cannot lose a path silently."""
    kper = _kper(dtype_name)
    n = {k: int(np.prod(s[:5])) for k, s in SHAPES.items()}
    assert n['one_cell'] == 1 and float(case('one_cell', 2.0, dtype_name).depth.reshape(-1)[0]) > 0        # tail only, foreground
    b, a, c, h, w, nb = SHAPES['tail']
    assert n['tail'] == 45 and n['tail'] % kper == (1 if kper == 4 else 5) and c % kper and (h * w) % kper
    b, a, c, h, w, nb = SHAPES['mixed']
    assert (h * w) % kper and h * w > 2 * kper                       # NCHW: vectors inside a plane row AND across its end
    assert c % 8 and c > 8 and c % 4 == 0                            # channels_last: 16-bit mixes, fp32 is all fast
    assert b * a * h * w < 1024                                      # more lanes than cells in a 1024-thread box-delta workgroup
    assert (n['mixed'] // kper) < 1024 * 4                           # more vector slots than vectors in one 1024 x 4 trip
    assert SHAPES['rotated'][5] != 4 and all(s[5] == 4 for k, s in SHAPES.items() if k != 'rotated')
    # trips: at 64 threads x 1 block per CU the per-level cap of 256 workgroups binds and the walk takes more than two whole trips
    # of every lane plus a partial one (restated from retina_loss_fill; tied to the library in the workspace size checks below)
    n_vec = n['trips'] // kper
    binding = [s for s in LAUNCH_SHAPES if s[0] == 64 and s[1] == 1 and -(-n_vec // (64 * s[2] * 2)) > 256
               and n_vec > 2 * 256 * 64 * s[2] and n_vec % (256 * 64 * s[2])]
    assert {s[5] for s in binding} == {0, 1}                         # with both trip layouts
    assert int(np.prod(SHAPES['trips'][:2])) * 20 * 28 == 15120
    assert max(n.values()) * 4 <= 1.25 * 2 ** 20                     # the biggest tensor is about 1.2 MB
    for name, gamma in CASES:
        cs = case(name, gamma, dtype_name)
        cells = cs.depth.size
        if cells >= 3:
            assert (cs.depth < 0).any() and (cs.depth == 0).any() and (cs.depth > 0).any()
        fgc = cs.depth[:, :, 0] > 0
        d = (cs.box - cs.tgt)[np.broadcast_to(fgc[:, :, None], cs.box.shape)]
        assert (d == 0).any() and (d == np.float32(BETA)).any() and (d == -np.float32(BETA)).any()
        if cs.x.size < 8:
            continue
        t = (np.arange(cs.shape[2]).reshape(1, 1, -1, 1, 1) == cs.depth - 1.0) & (cs.depth > 0)
        special = np.isin(cs.x, np.asarray(SPECIAL_LOGITS, np.float32))
        assert set(np.unique(cs.x[special])) == set(SPECIAL_LOGITS) or cs.x.size < 100
        if cs.x.size < 1000:
            continue
        for cl in (False, True):                                     # special values inside and outside vectors that hold a positive
            tv, sv = (_mem(m, cl)[: cs.x.size // kper * kper].reshape(-1, kper) for m in (t, special))
            assert (tv.any(1) & sv.any(1)).sum() >= 2 and (~tv.any(1) & sv.any(1)).sum() >= 2, (name, cl)


@pytest.mark.parametrize('dtype_name', list(DTYPES))
def test_float32_on_the_cpu_meets_the_bars_on_these_inputs(dtype_name):
    """The bars are reachable on the chosen inputs: the same restatement evaluated in float32 numpy (sums accumulated in float64, as
    the kernels do after <= 32 elements) against the float64 one.  If this fails the inputs are wrong, not the kernels.
    Observed worst case over all cases of this file: sums 5.1e-08 relative with fp32 heads, 4.6e-08 with bf16, 1.0e-07 with fp16
    (bar 1e-6); gradients 3.7e-07 of the largest with fp32 heads, 3.2e-07 with bf16, 3.9e-07 with fp16 (bar 1e-5); of the 16-bit
    values, rounded once from the float32 gradient, none outside its bracket."""
    worst_sum = worst_grad = 0.0
    outside = 0
    for name, gamma in CASES:
        cs = case(name, gamma, dtype_name)
        sums, dcls, dbox = reference(cs.x, cs.box, cs.depth, cs.tgt, gamma, cs.g_cls, cs.g_box, real=np.float32)
        assert dcls.dtype == np.float32 and dbox.dtype == np.float32
        assert sums[2] == cs.sums[2]
        for k in range(2):
            worst_sum = max(worst_sum, abs(sums[k] - cs.sums[k]) / max(abs(cs.sums[k]), 1e-300))
        for got, ref, scale in ((dcls, cs.dcls, cs.scale[0]), (dbox, cs.dbox, cs.scale[1])):
            worst_grad = max(worst_grad, float(np.abs(got - ref).max()) / max(scale, 1e-300))
            assert not (got[ref == 0] != 0).any()
            if dtype_name != 'fp32':
                lo, hi = bracket(ref, cs.dtype, scale)
                stored = torch.from_numpy(got).to(cs.dtype).double()
                outside += int(((stored < lo) | (stored > hi)).sum())
    print('float32 on the CPU, %s heads: sums %.2e relative, gradients %.2e of the largest, %d outside their bracket'
          % (dtype_name, worst_sum, worst_grad, outside))
    assert worst_sum <= 1e-6 and worst_grad <= 1e-5 and outside == 0


# ------------------------------------------------------------------------------------------------------------------------------
# the GPU side: buffers of this file, launches through the C ABI
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(autouse=True)
def launch_state():
    """Process-wide state of the loss kernels: all six launch shapes and the arithmetic form as found, put back whatever happens."""
    from odtk import _C
    pairs = [(which, fp32) for which in (FWD, BWD, WS) for fp32 in (0, 1)]
    found = {p: _C.loss_tuning_state(*p) for p in pairs}
    form = _C.loss_form_state()
    try:
        yield found
    finally:
        for p in pairs:
            _C.loss_tuning_restore(p[0], p[1], found[p])
        _C.loss_form(form)
        assert {p: _C.loss_tuning_state(*p) for p in pairs} == found and _C.loss_form_state() == form


def _guarded(n, dtype):
    """n elements of NaN and GUARD_BYTES more behind them -> (the whole buffer, the n elements, the guard)"""
    extra = GUARD_BYTES // torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((n + extra,), float('nan'), dtype=dtype, device='cuda')
    return buf, buf[:n], buf[n:]


def _untouched(guard):
    return bool(torch.isnan(guard).all())


class DeviceLevel:
    """One level of one layout on the device: the heads in memory order, the reference and the allowed gradients in the same order."""

    def __init__(self, cs, channels_last):
        self.cs, self.cl = cs, int(channels_last)
        def up(a, dt=None):
            t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return t.to(dt) if dt is not None else t

        self.cls, self.box = up(_mem(cs.x, channels_last), cs.dtype), up(_mem(cs.box, channels_last), cs.dtype)
        assert torch.equal(self.cls.float().cpu(), torch.from_numpy(_mem(cs.x, channels_last)))           # stored exactly
        assert torch.equal(self.box.float().cpu(), torch.from_numpy(_mem(cs.box, channels_last)))
        self.depth, self.tgt = up(cs.depth), up(cs.tgt)
        self.grads = []                                      # per gradient: reference, lowest and highest allowed, where exactly 0, scale
        for ref, scale in ((cs.dcls, cs.scale[0]), (cs.dbox, cs.scale[1])):
            ref = _mem(ref, channels_last)
            if cs.dtype == torch.float32:
                lo, hi = torch.from_numpy(ref - 1e-5 * scale), torch.from_numpy(ref + 1e-5 * scale)
            else:
                lo, hi = bracket(ref, cs.dtype, scale)
            self.grads.append((up(ref), lo.cuda(), hi.cuda(), up(ref == 0), scale))


@functools.lru_cache(maxsize=None)
def device_level(name, gamma, dtype_name, channels_last):
    return DeviceLevel(case(name, gamma, dtype_name), channels_last)


def _level_array(levels, grads=None):
    from odtk import _C
    arr = (_C.LossLevel * len(levels))()
    for i, lv in enumerate(levels):
        arr[i].cls, arr[i].box, arr[i].depth, arr[i].box_target = lv.cls.data_ptr(), lv.box.data_ptr(), lv.depth.data_ptr(), lv.tgt.data_ptr()
        arr[i].height, arr[i].width, arr[i].channels_last = lv.cs.shape[3], lv.cs.shape[4], lv.cl
        if grads is not None:
            arr[i].dcls, arr[i].dbox = grads[i][0][1].data_ptr(), grads[i][1][1].data_ptr()
    return arr


def _set_shape(which, fp32, shape, found):
    """-> the seven numbers the library now holds for (which, fp32)"""
    from odtk import _C
    threads, per_cu, unroll, box_blocks, per_wave, window, box_rows = shape
    per_cu = found[which, fp32]['blocks_per_cu'] if per_cu is None else per_cu
    _C.loss_tuning(which, fp32, threads, per_cu, unroll, box_blocks)
    _C.loss_layout(which, fp32, per_wave if which == WS else 0, window, box_rows)
    return tuple(_C.loss_tuning_state(which, fp32).values())


def _blocks(cs, state):
    """retina_loss_fill's workgroup count of one level, restated: at least two trips per lane, at most 256 x blocks_per_cu logit
    workgroups and box_blocks box-delta workgroups per level"""
    threads, per_cu, unroll, box_blocks = state[:4]
    b, a, c, h, w, nb = cs.shape
    n_vec = b * a * c * h * w // _kper(cs.dtype_name)
    cls_blocks = min(max(1, -(-n_vec // (threads * unroll * 2))), 256 * per_cu)
    return cls_blocks + min(-(-(b * a * h * w) // threads), box_blocks)


class Worst:
    def __init__(self):
        self.sum = self.grad = 0.0
        self.odd_per_wave = 0


def run_launch_shapes(levels, found, worst, form):
    """Every launch shape (and the defaults found) on `levels` (one launch covers them all): forward with atomics, forward through
    the workspace, backward; every assertion of this file's docstring.  The first failing launch ends the case."""
    from odtk import _C
    lib = _C.library()
    cs0 = levels[0].cs
    fp32 = int(cs0.dtype == torch.float32)
    n = len(levels)
    b, a, c, _, _, nb = cs0.shape
    dt = {'fp32': _C.F32, 'bf16': _C.BF16, 'fp16': _C.F16}[cs0.dtype_name]
    args = (n, None, b, a, c, nb, dt, ALPHA, cs0.gamma, BETA)
    stream = torch.cuda.current_stream().cuda_stream
    want = torch.tensor([lv.cs.sums for lv in levels], dtype=torch.float64)
    g_cls = torch.tensor([lv.cs.g_cls for lv in levels], dtype=torch.float32, device='cuda')
    g_box = torch.tensor([lv.cs.g_box for lv in levels], dtype=torch.float32, device='cuda')
    _C.loss_form(form)
    first = None
    for i, shape in enumerate([None] + LAUNCH_SHAPES):
        for which in (FWD, WS, BWD):
            state = _set_shape(which, fp32, shape, found) if shape is not None else tuple(found[which, fp32].values())
            if shape is None:
                _C.loss_tuning_restore(which, fp32, found[which, fp32])
            tag = '%s gamma %g %s %s form %d %s launch shape %s' % (cs0.name, cs0.gamma, cs0.dtype_name, 'nhwc' if levels[0].cl else 'nchw', form,
                                                                    ('forward', 'backward', 'forward-ws')[which], state)
            if which == BWD:
                grads = [[_guarded(t.numel(), t.dtype) for t in (lv.cls, lv.box)] for lv in levels]
                arr = _level_array(levels, grads)
                rc = lib.odtk_retina_loss_levels_backward(args[0], arr, *args[2:], g_cls.data_ptr(), g_box.data_ptr(), stream)
                assert rc == 0, '%s: rc %d %s' % (tag, rc, lib.odtk_last_hip_error())
                for l, lv in enumerate(levels):
                    for k, (ref, lo, hi, zero, scale) in enumerate(lv.grads):
                        _, got, guard = grads[l][k]
                        where = '%s level %d %s' % (tag, l, ('dcls', 'dbox')[k])
                        assert _untouched(guard), where
                        assert not bool(torch.isnan(got).any()), where                      # every element was written
                        g64 = got.double()
                        err = float((g64 - ref).abs().max())
                        worst.grad = max(worst.grad, err / max(scale, 1e-300))
                        bad = (g64 < lo) | (g64 > hi)
                        assert not bool(bad.any()), '%s: %d outside, worst error %.3e, largest gradient %.3e' % (where, int(bad.sum()), err, scale)
                        assert not bool(((g64 != 0) & zero).any()), where                           # ignored cells, non-foreground deltas
                bits = [g[1].view(torch.int32 if fp32 else torch.int16).clone() for lg in grads for g in lg]
                if first is None:
                    first = bits
                else:
                    for j, (x, y) in enumerate(zip(bits, first)):                           # the same element math, whoever computes it
                        assert torch.equal(x, y), '%s level %d %s: %d elements differ in bits from the first launch shape' % (
                            tag, j // 2, ('dcls', 'dbox')[j % 2], int((x != y).sum()))
                continue
            sums_buf, sums, sums_guard = _guarded(3 * n, torch.float64)
            arr = _level_array(levels)
            if which == FWD:
                rc = lib.odtk_retina_loss_levels_forward(args[0], arr, *args[2:], sums.data_ptr(), stream)
            else:
                need = lib.odtk_retina_loss_levels_forward_ws(args[0], arr, *args[2:], None, None, 0, None)
                total = sum(_blocks(lv.cs, state) for lv in levels)
                per = state[0] // 64 if state[4] else 1
                assert need == (total * per * 24 + 255) // 256 * 256, '%s: size query %d, %d workgroups x %d' % (tag, need, total, per)
                worst.odd_per_wave += int(total % 2 == 1 and state[4] == 1)
                ws_buf, ws, ws_guard = _guarded(need // 8, torch.float64)
                rc = lib.odtk_retina_loss_levels_forward_ws(args[0], arr, *args[2:], sums.data_ptr(), ws.data_ptr(), need, stream)
            assert rc == 0, '%s: rc %d %s' % (tag, rc, lib.odtk_last_hip_error())
            got = sums.cpu().view(n, 3)
            assert _untouched(sums_guard) and (which == FWD or _untouched(ws_guard)), tag
            assert bool(torch.isfinite(got).all()), '%s: %s' % (tag, got.tolist())
            for l in range(n):
                assert float(got[l, 2]) == float(want[l, 2]), '%s level %d: %s, want %s' % (tag, l, got[l].tolist(), want[l].tolist())
                for k in range(2):
                    rel = abs(float(got[l, k]) - float(want[l, k])) / max(abs(float(want[l, k])), 1e-300)
                    worst.sum = max(worst.sum, rel)
                    assert abs(float(got[l, k]) - float(want[l, k])) <= 1e-6 * abs(float(want[l, k])), '%s level %d sum %d: %.12g, want %.12g, %.2e relative' % (tag, l, k, float(got[l, k]), float(want[l, k]), rel)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype_name', list(DTYPES))
@pytest.mark.parametrize('name,gamma', CASES, ids=CASE_IDS)
def test_every_launch_shape_against_float64(name, gamma, dtype_name, launch_state):
    """One level, both layouts, both arithmetic forms, every launch shape: the three forms of the kernel against the float64
    restatement, bit-equal gradients across launch shapes, every output element written, no guard touched."""
    worst = Worst()
    for channels_last in (False, True):
        for form in (0, 1):
            run_launch_shapes([device_level(name, gamma, dtype_name, channels_last)], launch_state, worst, form)
    print('%s gamma %g %s: worst sum %.2e relative (bar 1e-6), worst gradient %.2e of the largest (bar 1e-5%s)'
          % (name, gamma, dtype_name, worst.sum, worst.grad, '' if dtype_name == 'fp32' else ', then one rounding'))
    if name == 'trips':
        assert worst.odd_per_wave > 0                        # per-wave sums with an odd number of workgroups were among them


PYRAMIDS = {'b1a3c5': (1, 3, 5, 4), 'b2a9c20': (2, 9, 20, 4)}
PYRAMID_SIZES = ((1, 1), (1, 3), (5, 7))                     # one_cell-, tail- and mixed-sized levels


@functools.lru_cache(maxsize=None)
def pyramid_levels(key, dtype_name, channels_last):
    b, a, c, nb = PYRAMIDS[key]
    out = []
    for l, (h, w) in enumerate(PYRAMID_SIZES):
        cs = Case('pyramid-%s-L%d' % (key, l), 2.0, dtype_name, shape=(b, a, c, h, w, nb), seed=500 + 10 * list(PYRAMIDS).index(key) + l,
                  g_cls=float(np.float32(0.37 + 0.5 * l)), g_box=float(np.float32(-1.9 + 1.3 * l)))
        out.append(DeviceLevel(cs, channels_last))
    return tuple(out)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype_name', list(DTYPES))
@pytest.mark.parametrize('key', list(PYRAMIDS))
def test_pyramid_launch_under_every_launch_shape(key, dtype_name, launch_state):
    """Three levels in ONE launch (block_begin bookkeeping, with per-wave sums too): every launch shape gives every level's own
    float64 results, with an upstream gradient of its own per level."""
    worst = Worst()
    for channels_last in (False, True):
        for form in (0, 1):
            run_launch_shapes(list(pyramid_levels(key, dtype_name, channels_last)), launch_state, worst, form)
    print('pyramid %s %s: worst sum %.2e relative (bar 1e-6), worst gradient %.2e of the largest (bar 1e-5%s)'
          % (key, dtype_name, worst.sum, worst.grad, '' if dtype_name == 'fp32' else ', then one rounding'))


@pytest.mark.gpu
def test_workspace_size_follows_the_launch_shape_and_a_stale_size_is_refused(launch_state):
    """Change the shape, query again: with per-wave sums the size follows threads / 64 per workgroup; the size of the earlier shape
    is too small now and is refused with ODTK_ERR_WORKSPACE before anything is launched (sums and workspace stay NaN)."""
    from odtk import _C
    lib = _C.library()
    lv = device_level('trips', 2.0, 'fp32', True)
    arr = _level_array([lv])
    b, a, c, _, _, nb = lv.cs.shape
    args = (1, arr, b, a, c, nb, _C.F32, ALPHA, 2.0, BETA)
    stream = torch.cuda.current_stream().cuda_stream
    sizes = {}
    for threads in (64, 192, 256, 1024):
        for per_wave in (0, 1):
            state = _set_shape(WS, 1, (threads, 1, 1, 1, per_wave, 1, 1), launch_state)
            sizes[threads, per_wave] = need = lib.odtk_retina_loss_levels_forward_ws(*args, None, None, 0, None)
            blocks = _blocks(lv.cs, state)
            assert need == (blocks * (threads // 64 if per_wave else 1) * 24 + 255) // 256 * 256, (threads, per_wave, need, blocks)
    assert sizes[1024, 1] > sizes[1024, 0] and sizes[192, 1] > sizes[192, 0] and sizes[64, 1] == sizes[64, 0]
    stale = sizes[1024, 0]
    _set_shape(WS, 1, (1024, 1, 1, 1, 1, 1, 1), launch_state)
    _, sums, sums_guard = _guarded(3, torch.float64)
    _, ws, ws_guard = _guarded(sizes[1024, 1] // 8, torch.float64)
    assert lib.odtk_retina_loss_levels_forward_ws(*args, sums.data_ptr(), ws.data_ptr(), stale, stream) == _C.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert _untouched(sums) and _untouched(ws) and _untouched(sums_guard) and _untouched(ws_guard)
    assert lib.odtk_retina_loss_levels_forward_ws(*args, sums.data_ptr(), ws.data_ptr(), sizes[1024, 1], stream) == 0
    got = sums.cpu()
    assert _untouched(sums_guard) and _untouched(ws_guard)
    for k in range(2):
        assert abs(float(got[k]) - lv.cs.sums[k]) <= 1e-6 * abs(lv.cs.sums[k])
    assert float(got[2]) == lv.cs.sums[2]
