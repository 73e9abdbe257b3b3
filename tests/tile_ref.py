"""Numpy restatement of tiled inference, independent of odtk/box.py: the grid, the tiler and the merge exactly as
include/odtk_hip.h defines them (odtk_tile_images, odtk_merge_tile_candidates).  The definitions leave no rounding freedom
-- a bit copy, float32 comparisons and one float32 addition per coordinate -- so every comparison against this file is bit for
bit (`bits` below), without a tolerance.

A tile entry is (image, slot, y, x), as odtk/box.py takes it; image < 0 is a padding entry."""
import numpy as np


def axis_origins(extent, size, overlap):
    """One axis of the grid: an extent <= size has the origin 0 alone; otherwise 0, step, 2 step, .. while origin + size < extent,
    followed by one last origin extent - size."""
    assert extent >= 1 and size >= 1 and 0 <= overlap < size
    if extent <= size:
        return [0]
    step, origins, origin = size - overlap, [], 0
    while origin + size < extent:
        origins.append(origin)
        origin += step
    origins.append(extent - size)
    return origins


def grid_ref(height, width, size, overlap):
    """Origins (y, x) in row-major order."""
    return [(y, x) for y in axis_origins(height, size[0], overlap[0]) for x in axis_origins(width, size[1], overlap[1])]


def chunks_ref(batch, grid, chunk):
    """The tiles of a batch image-major, in chunks of `chunk` entries (image, slot, y, x), the last padded with (-1, 0, 0, 0)."""
    entries = [(image, slot, y, x) for image in range(batch) for slot, (y, x) in enumerate(grid)]
    out = []
    for first in range(0, len(entries), chunk):
        part = entries[first:first + chunk]
        out.append(part + [(-1, 0, 0, 0)] * (chunk - len(part)))
    return out


def tile_ref(x, tiles, size):
    """x: integer array [B, C, H, W] holding the BITS of the pixels (int16 / int32 views) -> [len(tiles), C, th, tw] of the same
    type: the window of image `image` at (y, x), zero bits (+0) elsewhere and for padding entries."""
    assert x.dtype.kind in 'iu'
    th, tw = size
    out = np.zeros((len(tiles), x.shape[1], th, tw), x.dtype)
    for i, (image, _, y, left) in enumerate(tiles):
        if image < 0:
            continue
        rows, cols = max(0, min(th, x.shape[2] - y)), max(0, min(tw, x.shape[3] - left))    # the part of the window inside the image
        out[i, :, :rows, :cols] = x[image, :, y:y + rows, left:left + cols]
    return out


def merge_ref(parts, tiles, batch, slots, size, extent, border, out=None):
    """parts: float32 (scores [n, count], boxes [n, count, 4], classes [n, count]) -> [scores [batch, slots * count], boxes, classes];
    positions no entry covers keep what `out` held (new lists: zeros).  One candidate at a time, scalar float32 arithmetic."""
    scores, boxes, classes = (np.ascontiguousarray(p, np.float32) for p in parts)
    n, count = scores.shape
    assert n == len(tiles) and boxes.shape == (n, count, 4) and classes.shape == (n, count)
    th, tw = size
    height, width = extent
    border = np.float32(border)
    if out is None:
        out = [np.zeros((batch, slots * count), np.float32), np.zeros((batch, slots * count, 4), np.float32),
               np.zeros((batch, slots * count), np.float32)]
    far_x, far_y = np.float32(tw - 1) - border, np.float32(th - 1) - border
    zero = np.float32(0)
    for i, (image, slot, y, left) in enumerate(tiles):
        if image < 0:
            continue
        assert image < batch and 0 <= slot < slots
        tx, ty = np.float32(left), np.float32(y)
        for j in range(count):
            s, b, c = scores[i, j], boxes[i, j].copy(), classes[i, j]
            if s > zero:
                cut = False
                if border > zero:
                    cut = bool((left > 0 and b[0] < border) or (y > 0 and b[1] < border) or
                               (left + tw < width and b[2] > far_x) or (y + th < height and b[3] > far_y))
                if cut:
                    s, b, c = zero, np.zeros(4, np.float32), zero
                else:
                    b = np.array([b[0] + tx, b[1] + ty, b[2] + tx, b[3] + ty], np.float32)
            at = slot * count + j
            out[0][image, at], out[2][image, at] = s, c
            out[1][image, at] = b
    return out


def merge_case(count, border, seed, size=(16, 24), extent=(40, 56), overlap=(4, 8), batch=2):
    """Candidates of every tile of a batch, in tile coordinates, with the values the definition treats apart."""
    rng = np.random.RandomState(seed)
    grid = grid_ref(*extent, size, overlap)                   # 3 x 3: tiles on every image side and in the interior
    tiles = [(image, slot, y, x) for image in range(batch) for slot, (y, x) in enumerate(grid)]
    n, (th, tw) = len(tiles), size
    scores = rng.rand(n, count).astype(np.float32)
    kind = rng.randint(0, 12, (n, count))
    scores[kind == 0] = 0.0
    scores[kind == 1] = -rng.rand(int((kind == 1).sum())).astype(np.float32)
    scores[kind == 2] = np.nan
    scores[kind == 3] = -0.0
    x1, y1 = rng.uniform(0, tw - 1, (n, count)), rng.uniform(0, th - 1, (n, count))
    x2, y2 = x1 + rng.uniform(0, tw, (n, count)), y1 + rng.uniform(0, th, (n, count))
    boxes = np.stack([x1, y1, np.minimum(x2, tw - 1), np.minimum(y2, th - 1)], -1).astype(np.float32)
    edge = rng.randint(0, 16, (n, count))                              # coordinates exactly at, just inside and just outside the rule
    b32 = np.float32(border)
    for k, value in enumerate((b32, np.nextafter(b32, np.float32(-1)), np.nextafter(b32, np.float32(100)))):
        boxes[..., 0][edge == k] = value
        boxes[..., 1][edge == 3 + k] = value
    for axis, length, base in ((2, tw, 6), (3, th, 9)):
        far = np.float32(length - 1) - b32
        for k, value in enumerate((far, np.nextafter(far, np.float32(-1e9)), np.nextafter(far, np.float32(1e9)))):
            boxes[..., axis][edge == base + k] = value
    boxes[edge == 12] = np.nan                                         # NaN coordinates (with any score)
    boxes[..., 0][edge == 13] = np.nan
    boxes[..., 3][edge == 14] = np.inf
    classes = rng.randint(0, 80, (n, count)).astype(np.float32)
    classes[kind == 4] = np.nan
    return (scores, boxes, classes), tiles, dict(batch=batch, slots=len(grid), size=size, extent=extent, border=border)


def expected_merged(x, tile, candidates_of):
    """Restatement tiling -> `candidates_of(tiles tensor)` per chunk -> restatement merge: the merged lists (numpy) and the number
    of passes and of padding entries."""
    import torch
    size, overlap, border, chunk = tile
    grid = grid_ref(x.shape[2], x.shape[3], size, overlap)
    merged, passes, padding = None, 0, 0
    raw = x.contiguous().view({2: torch.int16, 4: torch.int32}[x.element_size()]).cpu().numpy()
    for part in chunks_ref(x.shape[0], grid, chunk):
        tiles = torch.from_numpy(tile_ref(raw, part, size)).view(x.dtype).to(x.device)
        if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
            tiles = tiles.contiguous(memory_format=torch.channels_last)
        found = [t.float().cpu().numpy() for t in candidates_of(tiles)]
        merged = merge_ref(found, part, x.shape[0], len(grid), size, x.shape[2:], border, out=merged)
        passes, padding = passes + 1, padding + sum(1 for t in part if t[0] < 0)
    return merged, passes, padding


def bits(a):
    """An array (numpy, or anything with .numpy()) as its raw integers."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def assert_same_bits(got, want, what=''):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()), 'elements differ')
