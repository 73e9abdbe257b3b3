"""Tiled inference without a GPU: the grid, the torch branches of odtk/box.py against the numpy restatement of tests/tile_ref.py
(bit for bit), the host-side validation of the two C entries, the command line, and Model.tile on CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

import tile_ref
from odtk import _C, box
from odtk import main as cli
from odtk.model import Model


def _bits(t):
    """A float tensor as its raw integers (numpy)."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()]).numpy()


# ---------------------------------------------------------------------------------------------------------------- the grid
def test_grid_example_and_edges():
    assert tile_ref.axis_origins(256, 128, 32) == [0, 96, 128]
    assert box.tile_grid(256, 256, (128, 128), (32, 32)) == [(y, x) for y in (0, 96, 128) for x in (0, 96, 128)]
    assert box.tile_grid(100, 128, (128, 128), (32, 32)) == [(0, 0)]                   # extents < and == the size
    assert box.tile_grid(129, 100, (128, 128), (0, 0)) == [(0, 0), (1, 0)]             # one pixel more: a second, shifted tile
    assert box.tile_grid(10, 40, (16, 16), (15, 15))[:3] == [(0, 0), (0, 1), (0, 2)]   # overlap size - 1: step 1
    assert box.tile_grid(10, 40, (16, 16), (15, 15))[-1] == (0, 24)
    assert box.tile_grid(64, 64, 32, 0) == [(0, 0), (0, 32), (32, 0), (32, 32)]        # an integer means a square
    for bad in (dict(overlap=(16, 0)), dict(overlap=(-1, 0)), dict(size=(0, 16)), dict(height=0)):
        with pytest.raises(ValueError):
            box.tile_grid(**{**dict(height=40, width=56, size=(16, 24), overlap=(4, 8)), **bad})


@pytest.mark.parametrize('size,overlap', [((16, 24), (4, 8)), ((16, 16), (0, 0)), ((16, 16), (15, 15)), ((7, 5), (3, 4)), ((32, 48), (8, 1))])
def test_grid_equals_restatement_and_covers_every_pixel(size, overlap):
    for height in (1, size[0] - 1, size[0], size[0] + 1, 2 * size[0] - overlap[0], 40, 57):
        for width in (1, size[1], size[1] + 1, 56, 61):
            if height < 1 or width < 1:
                continue
            grid = box.tile_grid(height, width, size, overlap)
            assert grid == tile_ref.grid_ref(height, width, size, overlap), (height, width)
            assert len(set(grid)) == len(grid)
            covered = np.zeros((height, width), bool)
            for y, x in grid:
                assert y >= 0 and x >= 0
                if height >= size[0]:
                    assert y + size[0] <= height                   # no tile leaves an image at least as large as the tile
                if width >= size[1]:
                    assert x + size[1] <= width
                covered[y:y + size[0], x:x + size[1]] = True
            assert covered.all(), (height, width)
            ys = sorted({y for y, _ in grid})
            assert all(b - a <= size[0] - overlap[0] for a, b in zip(ys, ys[1:]))       # neighbours share at least the overlap


# ---------------------------------------------------------------------------------------------------------------- the tiler
def _special_pixels(x):
    flat = x.view(-1)
    flat[3], flat[17], flat[40], flat[41], flat[100] = float('nan'), -0.0, float('inf'), float('-inf'), float('nan')
    return x


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('channels_last', [False, True])
def test_torch_tiler_equals_restatement(dtype, channels_last):
    torch.manual_seed(1)
    x = _special_pixels(torch.randn(2, 3, 40, 56)).to(dtype)
    if dtype == torch.float32:
        raw = x.view(torch.int32)
        raw.view(-1)[5] = 0x7fc01234                                   # a NaN with a payload
        raw.view(-1)[6] = -0x7f8edcc                                   # ... and a negative one (0xf8071234)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    size, overlap = (16, 24), (4, 8)
    grid = box.tile_grid(40, 56, size, overlap)
    tiles = [(image, slot, y, left) for image in range(2) for slot, (y, left) in enumerate(grid)]
    tiles = tiles[:7] + [(-1, 0, 0, 0)] + tiles[7:] + [(-1, 5, 3, 3)]   # padding entries in the middle and at the end
    assert len(tiles) <= box.MAX_TILES
    out = box.tile_images(x, tiles, size)
    assert out.dtype == dtype and out.shape == (len(tiles), 3, 16, 24)
    assert out.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    tile_ref.assert_same_bits(_bits(out), tile_ref.tile_ref(_bits(x), tiles, size))
    assert not _bits(out)[7].any() and not _bits(out)[-1].any()


def test_torch_tiler_pads_an_image_smaller_than_the_tile():
    torch.manual_seed(2)
    x = _special_pixels(torch.randn(1, 3, 10, 12))
    tiles = [(0, 0, 0, 0), (0, 1, 4, 6), (0, 2, 9, 11), (0, 3, 10, 0), (0, 4, 0, 500)]     # the last two lie outside: all zeros
    out = box.tile_images(x, tiles, (16, 16))
    tile_ref.assert_same_bits(_bits(out), tile_ref.tile_ref(_bits(x), tiles, (16, 16)))
    assert box.tile_grid(10, 12, (16, 16), (4, 4)) == [(0, 0)]
    assert torch.equal(out[0, :, :10, :12].view(torch.int32), x[0].view(torch.int32)) and not _bits(out[0, :, 10:]).any()
    assert not _bits(out)[3:].any()
    one = box.tile_images(torch.randn(2, 1, 9, 9), [(1, 0, 2, 3)], (4, 4))                 # a single channel
    assert one.shape == (1, 1, 4, 4)
    for bad in ([], [(0, 0, 0, 0)] * 65, [(1, 0, 0, 0)], [(0, 0, -1, 0)], [(0, 0, 0, -1)], [(0, 0, 0)]):
        with pytest.raises(ValueError):
            box.tile_images(x, bad, (16, 16))


# ---------------------------------------------------------------------------------------------------------------- the merge
def _t(parts):
    return tuple(torch.from_numpy(np.ascontiguousarray(p)) for p in parts)


@pytest.mark.parametrize('count', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('border', [0.0, 1.0, 2.5])
def test_torch_merge_equals_restatement(count, border):
    parts, tiles, how = tile_ref.merge_case(count, border, seed=count)
    want = tile_ref.merge_ref(parts, tiles, **how)
    got = box.merge_tile_candidates(_t(parts), tiles, **how)
    for g, w, name in zip(got, want, ('scores', 'boxes', 'classes')):
        assert g.dtype == torch.float32
        tile_ref.assert_same_bits(g.numpy(), w, '%s, count %d, border %g' % (name, count, border))
    if count == 1000:
        positive = parts[0] > 0
        if border > 0:
            cut = int(positive.sum()) - int((want[0] > 0).sum())
            assert 0 < cut < int(positive.sum())                      # the rule cuts some candidates and keeps others
        else:
            assert int(positive.sum()) == int((want[0] > 0).sum())


def test_merge_rule_at_its_edges():
    """One candidate per case on a 3 x 3 grid: a box exactly at `border` / at (tile - 1) - border stays, one ulp beyond is cut, and
    only on the sides of a tile that are not sides of the image."""
    size, extent, border = (16, 24), (40, 56), 2.5
    grid = tile_ref.grid_ref(*extent, size, (4, 8))
    assert grid[4] == (12, 16) and grid[0] == (0, 0) and grid[8] == (24, 32)
    far_x, far_y = np.float32(23) - np.float32(2.5), np.float32(15) - np.float32(2.5)
    below = lambda v: np.nextafter(np.float32(v), np.float32(-1e9))
    above = lambda v: np.nextafter(np.float32(v), np.float32(1e9))
    cases = [  # (slot, box, kept?)
        (4, [2.5, 2.5, far_x, far_y], True), (4, [below(2.5), 5, 10, 10], False), (4, [5, below(2.5), 10, 10], False),
        (4, [5, 5, above(far_x), 10], False), (4, [5, 5, 10, above(far_y)], False), (4, [np.nan, 5, 10, 10], True),
        (4, [5, 5, np.nan, np.nan], True), (0, [0, 0, 10, 10], True), (0, [0, 0, 23, 10], False), (0, [0, 0, 10, 15], False),
        (8, [0, 5, 23, 15], False), (8, [5, 0, 23, 15], False), (8, [5, 5, 23, 15], True), (2, [5, 0, 23, 5], True), (2, [0, 5, 23, 5], False),
        (6, [0, 5, 10, 15], True), (6, [0, 0, 10, 15], False)]
    tiles = [(0, slot, *grid[slot]) for slot, _, _ in cases]
    scores = np.full((len(cases), 1), 0.5, np.float32)
    boxes = np.array([b for _, b, _ in cases], np.float32)[:, None, :]
    classes = np.full((len(cases), 1), 7, np.float32)
    for i, (slot, b, kept) in enumerate(cases):                        # one call per case: the cases share slots
        part = (scores[i:i + 1], boxes[i:i + 1], classes[i:i + 1])
        how = dict(batch=1, slots=9, size=size, extent=extent, border=border)
        got = box.merge_tile_candidates(_t(part), tiles[i:i + 1], **how)
        want = tile_ref.merge_ref(part, tiles[i:i + 1], **how)
        for g, w in zip(got, want):
            tile_ref.assert_same_bits(g.numpy(), w, str(cases[i]))
        assert bool(got[0][0, slot] > 0) == kept, cases[i]
        assert int((got[0] != 0).sum()) == int(kept)
        off = box.merge_tile_candidates(_t(part), tiles[i:i + 1], **{**how, 'border': 0})
        assert float(off[0][0, slot]) == 0.5                           # border 0: the rule is off


def test_merge_writes_its_own_positions_only():
    parts, tiles, how = tile_ref.merge_case(65, 1.0, seed=9)
    out = [torch.full((2, 9 * 65), -7.0), torch.full((2, 9 * 65, 4), -7.0), torch.full((2, 9 * 65), -7.0)]
    some = [0, 4, 17]                                                   # three entries and a padding entry
    part = tuple(np.concatenate([p[some], p[:1]]) for p in parts)
    entries = [tiles[i] for i in some] + [(-1, 0, 0, 0)]
    back = box.merge_tile_candidates(_t(part), entries, out=out, **how)
    assert all(b is o for b, o in zip(back, out))
    want = tile_ref.merge_ref(part, entries, out=[np.full(o.shape, -7.0, np.float32) for o in out], **how)
    for g, w in zip(out, want):
        tile_ref.assert_same_bits(g.numpy(), w)
    assert int((out[0] == -7.0).sum()) == (18 - 3) * 65
    for bad in (dict(border=-1.0), dict(border=float('nan')), dict(border=float('inf')), dict(slots=4), dict(batch=1), dict(slots=0)):
        with pytest.raises(ValueError):
            box.merge_tile_candidates(_t(parts), tiles, **{**how, **bad})


# ---------------------------------------------------------------------------------------------------------------- the C entries
def test_abi_validates_before_touching_the_device():
    lib = _C.library()
    assert {'odtk_tile_images', 'odtk_merge_tile_candidates'} <= set(_C.exported_symbols())
    assert hasattr(lib, 'odtk_tile_images') and hasattr(lib, 'odtk_merge_tile_candidates')
    assert lib.odtk_abi_struct_size(11) == ctypes.sizeof(_C.Tile) == 16 and lib.odtk_abi_struct_size(12) == -1
    assert _C.MAX_TILES == box.MAX_TILES == 64
    some = 1 << 20                                                       # never dereferenced on these paths

    def table(n=4, image=0, slot=0, ox=0, oy=0):
        tiles = (_C.Tile * max(n, 1))()
        for t in tiles:
            t.image, t.slot, t.x, t.y = image, slot, ox, oy
        return tiles

    def tile(x=some, out=some, batch=2, channels=3, height=40, width=56, dtype=_C.BF16, channels_last=1, n=4, tiles=0, th=16, tw=24, **entry):
        return lib.odtk_tile_images(x, out, batch, channels, height, width, dtype, channels_last, n, table(n, **entry) if tiles == 0 else tiles,
                                    th, tw, None)
    for bad in (dict(x=None), dict(out=None), dict(tiles=None), dict(n=0), dict(n=65), dict(n=-1), dict(channels=0), dict(channels=17),
                dict(batch=0), dict(height=0), dict(width=-3), dict(th=0), dict(tw=0), dict(image=2), dict(image=1 << 30), dict(ox=-1),
                dict(oy=-1), dict(oy=-(1 << 31)), dict(channels_last=2), dict(x=some + 1), dict(dtype=_C.F32, out=some + 2)):
        assert tile(**bad) == _C.ERR_INVALID, bad
    assert tile(dtype=3) == _C.ERR_UNSUPPORTED and tile(dtype=-1) == _C.ERR_UNSUPPORTED

    ins = (ctypes.c_void_p * 3)(some, some, some)
    outs = (ctypes.c_void_p * 3)(some, some, some)

    def merge(n=4, tiles=0, inputs=ins, outputs=outs, count=1000, batch=2, slots=9, th=16, tw=24, height=40, width=56, border=1.0, flags=0,
              **entry):
        return lib.odtk_merge_tile_candidates(n, table(n, **entry) if tiles == 0 else tiles, inputs, outputs, count, batch, slots, th, tw,
                                              height, width, border, flags, None)
    for bad in (dict(tiles=None), dict(inputs=None), dict(outputs=None), dict(inputs=(ctypes.c_void_p * 3)(some, None, some)),
                dict(outputs=(ctypes.c_void_p * 3)(some, some, None)), dict(n=0), dict(n=65), dict(count=0),
                dict(slots=9, count=_C.MAX_NMS_COUNT_SCRATCH // 9 + 1), dict(count=_C.MAX_NMS_COUNT_SCRATCH + 1, slots=1), dict(image=2),
                dict(slot=9), dict(slot=-1), dict(border=-0.5), dict(border=float('nan')), dict(border=float('inf')), dict(flags=8),
                dict(flags=1 << 31), dict(flags=_C.FLAG_ROTATED | 16), dict(batch=0), dict(slots=0), dict(th=0), dict(width=0)):
        assert merge(**bad) == _C.ERR_INVALID, bad
    assert merge(flags=_C.FLAG_ROTATED) == _C.ERR_UNSUPPORTED
    assert merge(flags=_C.FLAG_ROTATED, slot=9) == _C.ERR_INVALID

    from odtk import _C_ext
    assert hasattr(_C_ext, 'tile_images') and hasattr(_C_ext, 'merge_tile_candidates')
    cpu = (torch.rand(1, 5), torch.rand(1, 5, 4), torch.zeros(1, 5))
    for module in (_C, _C_ext):
        with pytest.raises(RuntimeError, match='CUDA tensor'):
            module.tile_images(torch.zeros(1, 3, 8, 8), [(0, 0, 0, 0)], (4, 4))
        with pytest.raises(RuntimeError, match='CUDA tensor'):
            module.merge_tile_candidates(cpu, [(0, 0, 0, 0)], 1, 1, (4, 4), (8, 8), 0.0)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_command_line_flags():
    args = cli.parse(['infer', 'm.pth', '--tile', '512'])
    assert args.tile == 512 and cli.tile_options(args) == {'size': (512, 512), 'border': 0.0, 'batch': 8}
    args = cli.parse(['infer', 'm.pth', '--tile', '512', '--tile-overlap', '128', '--tile-border', '2.5', '--tile-batch', '4', '--box-voting', '0.65',
                      '--soft-nms', 'linear'])
    assert cli.tile_options(args) == {'size': (512, 512), 'overlap': (128, 128), 'border': 2.5, 'batch': 4}
    args = cli.parse(['train', 'm.pth', '--annotations', 'a.json', '--tile', '256', '--tile-overlap', '0'])
    assert cli.tile_options(args) == {'size': (256, 256), 'overlap': (0, 0), 'border': 0.0, 'batch': 8}
    plain = cli.parse(['infer', 'm.pth'])
    assert not any(hasattr(plain, f) for f in ('tile', 'tile_overlap', 'tile_border', 'tile_batch')) and cli.tile_options(plain) is None
    assert Model('ResNet18FPN', classes=3).tile is None
    for refused in (['infer', 'm.pth', '--tile-overlap', '32'], ['infer', 'm.pth', '--tile-border', '2'], ['infer', 'm.pth', '--tile-batch', '4'],
                    ['infer', 'm.pth', '--tile', '512', '--rotated-bbox'], ['infer', 'm.pth', '--tile', '512', '--tta', 'flip'],
                    ['train', 'm.pth', '--annotations', 'a.json', '--tile', '512', '--tta', 'flip'], ['infer', 'm.pth', '--tile', '0'],
                    ['infer', 'm.pth', '--tile', '-128'], ['infer', 'm.pth', '--tile', '128', '--tile-overlap', '128'],
                    ['infer', 'm.pth', '--tile', '128', '--tile-overlap', '-1'], ['infer', 'm.pth', '--tile', '128', '--tile-border', '-1'],
                    ['infer', 'm.pth', '--tile', '128', '--tile-border', 'nan'], ['infer', 'm.pth', '--tile', '128', '--tile-batch', '0'],
                    ['infer', 'm.pth', '--tile', '128', '--tile-batch', '65'], ['infer', 'm.pth', '--tile', '12.5'],
                    ['export', 'm.pth', 'e', '--tile', '512']):
        with pytest.raises(SystemExit):
            cli.parse(refused)


# ---------------------------------------------------------------------------------------------------------------- the model
def _model_and_input():
    torch.manual_seed(0)
    model = Model('ResNet18FPN', classes=3)
    model.initialize(None)
    model.eval()
    with torch.no_grad():
        model.cls_head[-1].weight.mul_(60.0)                           # detections exist
    return model, torch.randn(2, 3, 256, 256)


def test_model_on_cpu_tensors_honours_the_option_and_the_off_switch(tmp_path):
    model, x = _model_and_input()
    model.top_n = 100

    def run():
        with torch.no_grad():
            return [t.clone() for t in model(x)]

    def candidates_of(tiles):
        with torch.no_grad():
            cls_heads, box_heads = model.heads(tiles)
            strides = [tiles.shape[-1] // c.shape[-1] for c in cls_heads]
            for s in strides:
                model.level_anchors(s)
            return model.candidates(cls_heads, box_heads, strides)

    def check(got, tile, **tail):
        merged, passes, padding = tile_ref.expected_merged(x, tile, candidates_of)
        assert (passes, padding) == (3, 6) and merged[0].shape == (2, 9 * 5 * model.top_n)
        want = box.suppress(*_t(merged), model.nms, model.detections, threshold=model.threshold, **tail)
        for g, w, name in zip(got, want, ('scores', 'boxes', 'classes')):
            tile_ref.assert_same_bits(g.numpy(), w.numpy(), name)
        return merged

    default = run()
    assert model.tile is None and int((default[0] > 0).sum()) > 20

    model.tile = {'size': (128, 128), 'overlap': (32, 32), 'batch': 8}
    tiled = run()
    merged = check(tiled, ((128, 128), (32, 32), 0.0, 8))
    assert int((tiled[0] > 0).sum()) > 20 and not torch.equal(tiled[1], default[1])
    model.tile = {'size': 128, 'overlap': 32}                           # an integer is a square; batch 8 is the default
    assert model.tile_options() == ((128, 128), (32, 32), 0.0, 8)
    model.tile = {'size': 128}
    assert model.tile_options() == ((128, 128), (32, 32), 0.0, 8)       # a quarter of the size

    model.tile = {'size': (128, 128), 'overlap': (32, 32), 'border': 2.5, 'batch': 8}
    model.box_voting = 0.65
    cut = check(run(), ((128, 128), (32, 32), 2.5, 8), vote=0.65)
    assert int((cut[0] > 0).sum()) < int((merged[0] > 0).sum())          # the rule dropped candidates
    model.box_voting, model.soft_nms = None, {'method': 'gaussian', 'sigma': 0.5, 'min_score': 0.05}
    assert 9 * 5 * model.top_n <= box.MAX_SOFT_NMS_COUNT
    check(run(), ((128, 128), (32, 32), 2.5, 8), soft_nms=model.soft_nms)
    model.top_n = 200                                                    # 9 x 5 x 200 candidates: more than Soft-NMS takes
    with pytest.raises(ValueError, match='top_n'):
        run()
    model.top_n, model.soft_nms = 100, None

    for bad in ({'size': (100, 128)}, {'size': (128, 64)}, {'size': 0}, {'size': 128, 'overlap': 128}, {'size': 128, 'overlap': (-1, 0)},
                {'size': 128, 'border': -1}, {'size': 128, 'border': float('nan')}, {'size': 128, 'batch': 0}, {'size': 128, 'batch': 65},
                {'overlap': 32}, {'size': 128, 'stride': 2}, 128):
        model.tile = bad
        with pytest.raises(ValueError, match='tile'):
            run()
    model.tile = {'size': 128}
    model.tta = 'flip'
    with pytest.raises(ValueError, match='tta'):
        run()
    model.tta, model.rotated_bbox = None, True
    with pytest.raises(ValueError, match='rotated'):
        model.check_inference_options()
    model.rotated_bbox = False
    with pytest.raises(RuntimeError, match='graph'):
        model(x, graph=True)

    path = str(tmp_path / 'm.pth')
    model.save({'path': path})
    assert not any('tile' in k for k in torch.load(path, map_location='cpu'))
    assert Model.load(path)[0].tile is None

    model.tile = None
    for d, e in zip(default, run()):
        assert torch.equal(d, e)


def test_infer_through_the_command_line(tmp_path):
    """`odtk infer --tile` end to end on the committed five-image data set, on the CPU: the flags reach Model.tile, the run writes
    detections, and they differ from the untiled run's."""
    import json
    import os
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data')
    model, _ = _model_and_input()
    path = str(tmp_path / 'm.pth')
    model.save({'path': path})
    common = ['--images', data, '--annotations', os.path.join(data, 'annotations.json'), '--batch', '2', '--resize', '256', '--max-size', '256', '--workers', '0', '--full-precision']
    before = torch.get_num_threads()
    torch.set_num_threads(4)
    try:
        docs = []
        for name, flags in (('plain', []), ('tiled', ['--tile', '128', '--tile-overlap', '32', '--tile-border', '2', '--tile-batch', '6'])):
            out = str(tmp_path / (name + '.json'))
            assert cli.main(['infer', path, '--output', out] + common + flags) is not None
            docs.append(json.load(open(out)))
        with pytest.raises(RuntimeError, match='stride'):
            cli.main(['infer', path, '--output', str(tmp_path / 'bad.json'), '--tile', '100'] + common)
    finally:
        torch.set_num_threads(before)
    assert len(docs[1]['images']) == 5 and len(docs[1]['annotations']) > 20
    assert docs[0]['annotations'] != docs[1]['annotations']
