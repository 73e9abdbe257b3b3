"""odtk_bottleneck_seam (csrc/seam.hpp): conv3 + skip + ReLU of a bottleneck block and conv1 + ReLU of the next one as one HIP pass.

Exactness, in the manner of oracle/conv_exact.py: y2, W3 and W1 are in {-1, 0, 1}, the biases and the skip are integers, so every
product and partial sum of both contractions is an integer.  |out| <= 256 is exact in bf16 and fp16 and in the fp32 accumulator, so
`out` EQUALS the float64 reference whatever the order of summation; z before its rounding is an integer below 2^24 (exact in fp32 in
any order) and below the dtype's maximum, so z EQUALS the reference rounded once to the dtype.  A swapped row / column, a missed
k-permutation of the accumulator-as-operand idiom or a wrong neighbour moves an output by an integer.
Shapes: the smallest that take every path -- 15 pixels (part of one wave tile, three idle waves), 234 (a whole workgroup trip and a
partial one: tiles 0..7, the last with 10 pixels), 32 * 5 + 1 (a one-pixel tile), 4 * 32 * 513 - 1 = 65663 (more 128-pixel trips than
the 512 / 256 resident workgroups of a 256-CU device: the persistent loop and its prefetch of the next tile run, and the last tile is
partial)."""
import functools

import pytest
import torch
import torch.nn as nn

from odtk import _C

C_IN, C_MID = 64, 256
SIZES = [15, 234, 32 * 5 + 1, 4 * 32 * 513 - 1]
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}


def _sparse_signs(g, rows, cols, keep):
    """{-1, 0, 1} with P(non-zero) = keep, signs even."""
    return (torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1) * (torch.rand(rows, cols, generator=g) < keep)


@functools.lru_cache(maxsize=None)
def _exact_case(m, pattern):
    """Integer inputs and the float64 reference for N2 = 128 (N2 = 64 takes the first 64 rows of W1 / b1 / z): computed once per
    (size, pattern), shared by both dtypes and both widths, never modified."""
    g = torch.Generator().manual_seed(1000 * len(pattern) + m)
    y2 = torch.randint(-1, 2, (m, C_IN), generator=g)
    skip = torch.randint(-64, 65, (m, C_MID), generator=g)
    b3 = torch.randint(-32, 33, (C_MID,), generator=g)
    b1 = torch.randint(-512, 513, (128,), generator=g)
    if pattern == 'identity_w3':            # out[c] = relu(y2[c % 64] + b3[c] + skip[c]): every channel block shows its own k
        w3 = (torch.arange(C_MID).view(-1, 1) % C_IN == torch.arange(C_IN).view(1, -1)).long()
    else:
        w3 = _sparse_signs(g, C_MID, C_IN, 0.5)
    if pattern == 'identity_w1':            # z[n] = relu(out[(5 n + 3) % 256] + b1[n]): a permutation, not symmetric
        w1 = ((5 * torch.arange(128).view(-1, 1) + 3) % C_MID == torch.arange(C_MID).view(1, -1)).long()
        b1 = torch.randint(-96, 33, (128,), generator=g)
    else:
        w1 = _sparse_signs(g, 128, C_MID, 0.25)
    pre_out = y2.double() @ w3.double().t() + b3.double() + skip.double()
    out = pre_out.clamp_min(0)
    pre_z = out @ w1.double().t() + b1.double()
    return {'y2': y2, 'skip': skip, 'w3': w3, 'b3': b3, 'w1': w1, 'b1': b1, 'pre_out': pre_out, 'out': out, 'pre_z': pre_z}


def _as_map(mat, dtype):
    """[M, C] integers / floats -> a channels_last [1, C, 1, M] device tensor of `dtype` (one pixel per row)."""
    m, c = mat.shape
    return mat.to(dtype).cuda().contiguous().view(1, 1, m, c).permute(0, 3, 1, 2)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _run_exact(m, pattern, n2, dtype):
    case = _exact_case(m, pattern)
    # the reference alone first: the bounds that make the comparison exact, and both ReLUs cut about half
    assert case['out'].abs().max().item() <= 256 and case['pre_out'].abs().max().item() <= 256
    pre_z = case['pre_z'][:, :n2]
    assert pre_z.abs().max().item() < 2 ** 24 and pre_z.abs().max().item() < torch.finfo(dtype).max
    for pre in (case['pre_out'], pre_z):
        neg = (pre < 0).double().mean().item()
        assert 0.3 < neg < 0.7, neg
    out, z = _C.bottleneck_seam(_as_map(case['y2'], dtype), _as_map(case['skip'], dtype), case['w3'].to(dtype).cuda(),
                                case['b3'].float().cuda(), case['w1'][:n2].to(dtype).cuda().contiguous(), case['b1'][:n2].float().cuda())
    assert out.shape == (1, C_MID, 1, m) and z.shape == (1, n2, 1, m) and out.dtype == dtype and z.dtype == dtype
    want_out = case['out'].to(dtype)
    assert torch.equal(want_out.double(), case['out'])                       # (representable: nothing was rounded)
    want_z = pre_z.clamp_min(0).float().to(dtype)                            # rne_T of the exact value
    got_out, got_z = _rows(out).cpu(), _rows(z).cpu()
    bad = (got_out != want_out).nonzero()
    assert bad.numel() == 0, ('out', bad.shape[0], bad[:4].tolist(), got_out[tuple(bad[0])].item(), want_out[tuple(bad[0])].item())
    bad = (got_z != want_z).nonzero()
    assert bad.numel() == 0, ('z', bad.shape[0], bad[:4].tolist(), got_z[tuple(bad[0])].item(), want_z[tuple(bad[0])].item())


@pytest.mark.gpu
@pytest.mark.parametrize('m', SIZES)
@pytest.mark.parametrize('n2', [64, 128])
@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_seam_equals_the_float64_reference_bit_for_bit(m, n2, dtype):
    _run_exact(m, 'random', n2, DTYPES[dtype])


@pytest.mark.gpu
@pytest.mark.parametrize('pattern', ['identity_w3', 'identity_w1'])
@pytest.mark.parametrize('n2', [64, 128])
@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_seam_identity_against_asymmetric_weights(pattern, n2, dtype):
    """An identity in one product and an asymmetric matrix in the other: a swapped row / column of either product, or W1 staged
    in natural order against the permuted rows of the accumulator, cannot cancel."""
    _run_exact(234, pattern, n2, DTYPES[dtype])


@pytest.mark.gpu
@pytest.mark.parametrize('n2', [64, 128])
def test_seam_matches_the_two_gemms_on_real_values(n2):
    """Real-valued bf16 inputs against the two odtk_gemm_bias_act calls the seam replaces, and against the fp32 restatement, at the
    bound tests/test_gpu_fused.py uses for gemm_bias_act: 2^-8 |ref| + 1e-2 (one bf16 rounding + the order of the fp32 sums).  Two
    correct roundings of sums taken in different orders may differ by one bf16 ulp; the bound admits that below 4 (ulp 2^-6), so
    the inputs are scaled to outputs of about 0.5 standard deviations (4 is eight of them)."""
    g = torch.Generator().manual_seed(11)
    b, h, w = 2, 37, 53
    cl = lambda t: t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)
    y2, skip = cl(torch.randn(b, C_IN, h, w, generator=g)), cl(torch.randn(b, C_MID, h, w, generator=g) * 0.3)
    w3 = cl(torch.randn(C_MID, C_IN, 1, 1, generator=g) * (0.3 * C_IN ** -0.5))
    w1 = cl(torch.randn(n2, C_MID, 1, 1, generator=g) * C_MID ** -0.5)
    b3, b1 = (torch.randn(C_MID, generator=g) * 0.3).cuda(), (torch.randn(n2, generator=g) * 0.3).cuda()
    out, z = _C.bottleneck_seam(y2, skip, w3, b3, w1, b1)
    assert out.is_contiguous(memory_format=torch.channels_last) and z.is_contiguous(memory_format=torch.channels_last)
    gemm_out = _C.gemm_bias_act(y2, w3, b3, skip, True)
    gemm_z = _C.gemm_bias_act(gemm_out, w1, b1, None, True)
    ref_out = (nn.functional.conv2d(y2.float(), w3.float()) + b3.view(1, -1, 1, 1) + skip.float()).relu()
    ref_z = (nn.functional.conv2d(out.float(), w1.float()) + b1.view(1, -1, 1, 1)).relu()      # (from the ROUNDED out it stored)
    for name, got, want in (('out vs gemm', out, gemm_out.float()), ('z vs gemm', z, gemm_z.float()), ('out vs fp32', out, ref_out),
                            ('z vs fp32', z, ref_z)):
        err = (got.float() - want).abs()
        tol = 2.0 ** -8 * want.abs() + 1e-2
        print('%s: max |err| %.3g, %d of %d elements differ' % (name, err.max().item(), int((err > 0).sum()), err.numel()))
        assert (err <= tol).all(), (name, float((err - tol).max()))
    assert torch.equal(out, _C.bottleneck_seam(y2, skip, w3, b3, w1, b1)[0])


def test_seam_entry_point_refuses_on_the_host():
    """Null, aliased or misaligned pointers: ODTK_ERR_INVALID; other dtypes and channel counts: ODTK_ERR_UNSUPPORTED -- all before
    anything touches HIP (the pointers are dummies)."""
    fn = _C.library().odtk_bottleneck_seam
    p = [4096 * (i + 1) for i in range(8)]                       # out, z, y2, skip, w3, b3, w1, b1

    def call(ptrs=p, m=100, c_in=64, c_mid=256, c_next=64, dtype=_C.BF16):
        return fn(*ptrs, m, c_in, c_mid, c_next, dtype, None)

    for i in range(8):
        assert call(p[:i] + [None] + p[i + 1:]) == _C.ERR_INVALID, i
    for dst, src in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3)):     # out == z, an output == an input
        q = list(p)
        q[dst] = q[src]
        assert call(q) == _C.ERR_INVALID, (dst, src)
    for i in (0, 1, 2, 3, 4, 6):                                  # 16-byte alignment of the 16-bit tensors
        assert call(p[:i] + [p[i] + 8] + p[i + 1:]) == _C.ERR_INVALID, i
    for i in (5, 7):                                              # the fp32 biases: their element
        assert call(p[:i] + [p[i] + 2] + p[i + 1:]) == _C.ERR_INVALID, i
    assert call(c_in=0) == _C.ERR_INVALID and call(c_next=-1) == _C.ERR_INVALID
    assert call(dtype=_C.F32) == _C.ERR_UNSUPPORTED and call(dtype=9) == _C.ERR_UNSUPPORTED
    for kw in ({'c_in': 128}, {'c_mid': 512}, {'c_next': 256}, {'c_next': 96}, {'c_in': 256, 'c_mid': 64}):
        assert call(**kw) == _C.ERR_UNSUPPORTED, kw
    assert call(m=0) == 0                                         # nothing to do (a supported call with pixels would launch)
    assert 'odtk_bottleneck_seam' in _C.exported_symbols() and 'bottleneck_seam_kernel' in _C.KERNEL_NAMES


# ---- the engine ---------------------------------------------------------------------------------------------------------------
def _model(backbone):
    from odtk.model import Model
    torch.manual_seed(0)
    model = Model(backbone, classes=8)
    model.initialize(None)
    for m in model.modules():                       # non-trivial frozen statistics
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.8, 1.2); m.bias.data.normal_(0, 0.1)
    model = model.cuda().to(memory_format=torch.channels_last).eval()
    with torch.no_grad():
        model.cls_head[-1].weight.mul_(60.0)        # detections exist
    return model


def _seam_launches(fn):
    _C.profile_collect()
    _C.profile_enable(True, ['bottleneck_seam_kernel', 'gemm_bias_act'])
    try:
        result = fn()
        torch.cuda.synchronize()
        counts = _C.profile_collect()
    finally:
        _C.profile_enable(False)
    return result, counts['bottleneck_seam_kernel'][1], counts['gemm_bias_act'][1]


@pytest.mark.gpu
def test_engine_seam_path_matches_the_two_gemm_graph():
    """ResNet50FPN on a 128 px image, seam on versus off: three seam launches replace six GEMMs, the detections (scores and classes)
    are the same, the head tensors agree within the tolerance of test_fused_graph_matches_eager_fp32, and a graph replay equals the
    eager call."""
    from odtk.fused import FusedRetinaNet
    engine = FusedRetinaNet(_model('ResNet50FPN'), dtype=torch.bfloat16)
    assert engine.seam_fusion and len(engine._seams) == 3
    x = torch.randn(2, 3, 128, 128, device='cuda')
    with torch.no_grad():
        engine.forward(x)                                                    # plan pass, library warm-up
        on, n_seam, n_gemm = _seam_launches(lambda: [t.clone() for t in engine.forward(x)])
        heads_on = engine.heads(x)
        engine.seam_fusion = False
        off, n_seam_off, n_gemm_off = _seam_launches(lambda: [t.clone() for t in engine.forward(x)])
        heads_off = engine.heads(x)
        engine.seam_fusion = True
        assert (n_seam, n_seam_off) == (3, 0) and n_gemm_off - n_gemm == 6, (n_seam, n_gemm, n_seam_off, n_gemm_off)
        assert int((on[0] > 0).sum()) > 50
        for a, b in zip(heads_on[0] + heads_on[1], heads_off[0] + heads_off[1]):
            scale = b.float().abs().max().item() + 1e-6
            err = (a.float() - b.float()).abs().max().item()
            print('head %s: max |seam - gemm| / scale = %.3g' % (tuple(a.shape), err / scale))
            assert err <= 2e-3 * scale, err / scale
        print('scores differing: %d, classes differing: %d, max |box| move %.3g' % (
            int((on[0] != off[0]).sum()), int((on[2] != off[2]).sum()), (on[1] - off[1]).abs().max().item()))
        assert torch.equal(on[0], off[0]) and torch.equal(on[2], off[2])
        replayed = engine.replay(x)
        assert all(torch.equal(a, b) for a, b in zip(on, replayed))
        n_graphs = len(engine._graphs)
        engine.seam_fusion = False                                           # the switch is part of the graph key
        assert all(torch.equal(a, b) for a, b in zip(off, engine.replay(x))) and len(engine._graphs) == n_graphs + 1


@pytest.mark.gpu
def test_basic_block_engine_launches_no_seam_kernel():
    from odtk.fused import FusedRetinaNet
    engine = FusedRetinaNet(_model('ResNet18FPN'), dtype=torch.bfloat16)
    assert not engine._seams
    x = torch.randn(2, 3, 128, 128, device='cuda')
    with torch.no_grad():
        engine.forward(x)
        _, n_seam, n_gemm = _seam_launches(lambda: engine.forward(x))
    assert n_seam == 0 and n_gemm > 0
