"""Tiled inference on the GPU: the two HIP kernels of csrc/tile.hpp against the numpy restatement of tests/tile_ref.py, bit for
bit, through both bindings; and Model.tile in the eager branch and in the engine."""
import numpy as np
import pytest
import torch

import tile_ref
from odtk import _C, box
from odtk.model import Model

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()]).cpu().numpy()


def _device(arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _image(shape, dtype, channels_last, seed):
    torch.manual_seed(seed)
    x = torch.randn(*shape)
    flat = x.view(-1)
    flat[3], flat[17], flat[40], flat[41], flat[100] = float('nan'), -0.0, float('inf'), float('-inf'), float('nan')
    x = x.to(dtype)
    if dtype == torch.float32:
        x.view(torch.int32).view(-1)[5] = 0x7fc01234                    # a NaN with a payload
    x = x.cuda()
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('channels', [3, 1])
def test_tiler_kernel_equals_restatement(dtype, channels_last, channels):
    x = _image((2, channels, 40, 56), dtype, channels_last, 1)
    size = (16, 24)
    grid = tile_ref.grid_ref(40, 56, size, (4, 8))
    tiles = [(image, slot, y, left) for image in range(2) for slot, (y, left) in enumerate(grid)]
    tiles = tiles[:7] + [(-1, 0, 0, 0)] + tiles[7:] + [(-1, 5, 3, 3)]    # padding entries in the middle and at the end
    out = box.tile_images(x, tiles, size)
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.shape == (len(tiles), channels, 16, 24)
    if channels > 1:
        assert out.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    tile_ref.assert_same_bits(_bits(out), tile_ref.tile_ref(_bits(x), tiles, size))
    # an image smaller than the tile, windows that leave it and windows wholly outside it
    small = _image((1, channels, 10, 12), dtype, channels_last, 2)
    tiles = [(0, 0, 0, 0), (0, 1, 4, 6), (0, 2, 9, 11), (0, 3, 10, 0), (0, 4, 0, 500)]
    out = box.tile_images(small, tiles, (16, 16))
    torch.cuda.synchronize()
    tile_ref.assert_same_bits(_bits(out), tile_ref.tile_ref(_bits(small), tiles, (16, 16)))


def test_tiler_kernel_with_more_than_one_workgroup_per_tile_and_64_entries():
    x = _image((3, 3, 70, 90), torch.bfloat16, True, 3)
    grid = tile_ref.grid_ref(70, 90, (48, 40), (13, 7))                  # 3 x 48 x 40 = 5760 elements per tile: six workgroups
    tiles = [(image, slot, y, left) for image in range(3) for slot, (y, left) in enumerate(grid)]
    tiles = (tiles * 8)[:64]
    out = box.tile_images(x, tiles, (48, 40))
    torch.cuda.synchronize()
    tile_ref.assert_same_bits(_bits(out), tile_ref.tile_ref(_bits(x), tiles, (48, 40)))


@pytest.mark.parametrize('count', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('border', [0.0, 1.0, 2.5])
def test_merge_kernel_equals_restatement(count, border):
    parts, tiles, how = tile_ref.merge_case(count, border, seed=count)
    got = box.merge_tile_candidates(_device(parts), tiles, **how)
    torch.cuda.synchronize()
    for g, w, name in zip(got, tile_ref.merge_ref(parts, tiles, **how), ('scores', 'boxes', 'classes')):
        tile_ref.assert_same_bits(g.cpu().numpy(), w, '%s, count %d, border %g' % (name, count, border))


def test_merge_kernel_writes_its_own_positions_only():
    parts, tiles, how = tile_ref.merge_case(65, 1.0, seed=9)
    shapes = ((2, 9 * 65), (2, 9 * 65, 4), (2, 9 * 65))
    out = [torch.full(s, -7.0, device='cuda') for s in shapes]
    some = [0, 4, 17]                                                     # three entries and a padding entry
    part = tuple(np.concatenate([p[some], p[:1]]) for p in parts)
    entries = [tiles[i] for i in some] + [(-1, 0, 0, 0)]
    back = box.merge_tile_candidates(_device(part), entries, out=out, **how)
    torch.cuda.synchronize()
    assert all(b is o for b, o in zip(back, out))
    want = tile_ref.merge_ref(part, entries, out=[np.full(s, -7.0, np.float32) for s in shapes], **how)
    for g, w in zip(out, want):
        tile_ref.assert_same_bits(g.cpu().numpy(), w)


def test_both_bindings_on_a_side_stream_called_twice():
    from odtk import _C_ext
    x = _image((2, 3, 40, 56), torch.bfloat16, True, 4)
    size = (16, 24)
    parts, tiles, how = tile_ref.merge_case(65, 2.5, seed=5)
    dev = _device(parts)
    args = (tiles, how['batch'], how['slots'], how['size'], how['extent'], how['border'])
    results = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for module in (_C, _C_ext, _C, _C_ext):
            results.append((module.tile_images(x, tiles, size), module.merge_tile_candidates(dev, *args)))
        out = [torch.full_like(t, -7.0) for t in results[0][1]]
        for module in (_C, _C_ext):
            module.merge_tile_candidates(dev, *args, out=out)
    side.synchronize()
    torch.cuda.synchronize()
    tile_ref.assert_same_bits(_bits(results[0][0]), tile_ref.tile_ref(_bits(x), tiles, size))
    want = tile_ref.merge_ref(parts, tiles, **how)
    for tiled, merged in results:
        assert torch.equal(tiled.view(torch.int16), results[0][0].view(torch.int16))
        assert tiled.is_contiguous(memory_format=torch.channels_last)
        for g, o, w in zip(merged, out, want):
            tile_ref.assert_same_bits(g.cpu().numpy(), w)
            tile_ref.assert_same_bits(o.cpu().numpy(), w)


def test_model_branches_honour_the_option_and_the_off_switch():
    """ResNet18FPN under bf16 autocast on [2, 3, 256, 256] channels_last, tile 128, overlap 32: 9 tiles per image, three passes of
    8, the last with 6 padding tiles.  The eager network and the BN-folded engine are the same function only up to the rounding
    of the folded weights, so each branch is compared with the restatement on the candidates decoded from ITS OWN head tensors of
    the restated chunks.  A hipGraph is refused; with the option back at None every branch -- the graph captured before too --
    returns what it returned before the option was ever set."""
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(0)
        model = Model('ResNet18FPN', classes=8)
        model.initialize(None)
        model = model.cuda().to(memory_format=torch.channels_last).eval()
        model.top_n = 100
        with torch.no_grad():
            model.cls_head[-1].weight.mul_(60.0)                        # detections exist
        x = torch.randn(2, 3, 256, 256, device='cuda').contiguous(memory_format=torch.channels_last)

        def call(branch):
            model.fused_graph = branch != 'eager'
            try:
                with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                    return [t.clone() for t in model(x, graph=branch == 'graph')]
            finally:
                model.fused_graph = True

        def own_candidates(branch):
            def decode(tiles):
                """decode_levels on the branch's own head tensors of `tiles`, at once (the engine's next pass may overwrite them)."""
                assert tiles.shape == (8, 3, 128, 128) and tiles.is_contiguous(memory_format=torch.channels_last)
                with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                    if branch == 'eager':
                        (cls_heads, box_heads), cls_bias, box_bias = model.heads(tiles), None, None
                    else:
                        cls_heads, box_heads, cls_bias, box_bias = model.inference_engine(torch.bfloat16).heads_without_last_bias(tiles)
                    strides = [tiles.shape[-1] // c.shape[-1] for c in cls_heads]
                    pairs = [box._pair(c, b) for c, b in zip(cls_heads, box_heads)]
                    cand = _C.decode_levels([p[0] for p in pairs], [p[1] for p in pairs], [model.anchors[s] for s in strides], strides,
                                            model.threshold, model.top_n, logits=True, cls_bias=cls_bias, box_bias=box_bias)
                torch.cuda.synchronize()
                return cand
            return decode

        def check(out, branch, border, **tail):
            merged, passes, padding = tile_ref.expected_merged(x, ((128, 128), (32, 32), border, 8), own_candidates(branch))
            assert (passes, padding) == (3, 6) and merged[0].shape == (2, 9 * 5 * model.top_n)
            want = box.suppress(*_device(merged), model.nms, model.detections, threshold=model.threshold, **tail)
            for g, w, name in zip(out, want, ('scores', 'boxes', 'classes')):
                tile_ref.assert_same_bits(g.cpu().numpy(), w.cpu().numpy(), (branch, border, name))
            return merged

        before = {b: call(b) for b in ('eager', 'engine', 'graph')}
        assert all(torch.equal(a, b) for a, b in zip(before['engine'], before['graph']))
        engine = model.inference_engine(torch.bfloat16)
        n_graphs = len(engine._graphs)

        model.tile = {'size': (128, 128), 'overlap': (32, 32), 'batch': 8}
        for b in ('eager', 'engine'):
            tiled = call(b)
            assert int((tiled[0] > 0).sum()) > 20 and not torch.equal(tiled[1], before[b][1])
            check(tiled, b, 0.0)
        with pytest.raises(RuntimeError, match='tile'):
            call('graph')
        with pytest.raises(RuntimeError, match='tile'):
            with torch.no_grad():
                engine.replay(x)
        assert len(engine._graphs) == n_graphs

        model.tile = {'size': 128, 'overlap': 32, 'border': 2.5}
        model.box_voting = 0.65
        check(call('engine'), 'engine', 2.5, vote=0.65)
        model.box_voting, model.soft_nms = None, {'method': 'gaussian', 'sigma': 0.5, 'min_score': 0.05}
        check(call('engine'), 'engine', 2.5, soft_nms=model.soft_nms)
        model.top_n = 200
        with pytest.raises(ValueError, match='top_n'):
            call('engine')
        model.top_n, model.soft_nms = 100, None
        model.tta = 'flip'
        with pytest.raises(ValueError, match='tta'):
            call('engine')
        model.tta = None

        model.tile = None
        after = {b: call(b) for b in ('eager', 'engine', 'graph')}
        assert len(engine._graphs) == n_graphs                           # the graph captured at the start is the one replayed
        for b in after:
            assert all(torch.equal(a, c) for a, c in zip(before[b], after[b])), b
    finally:
        torch.backends.cudnn.deterministic = saved
