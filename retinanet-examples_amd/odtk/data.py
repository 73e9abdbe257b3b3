"""Images and COCO-style annotations in, device-resident batches out: the data format on the INPUT side of
the path (reference odtk/data.py; its DALI twin dali.py is dropped by the north star).

Same dataset semantics as the reference -- resize so that the short side is `resize` unless the long side
would exceed `max_size` (data.py:56-59), PIL bilinear resampling, ImageNet mean / std, zero padding (in
normalised space) up to a multiple of the stride and to the largest image of the batch, targets as
`[x, y, w, h(, theta), class]` rows padded with -1, ids + resize ratios for inference -- with a different
split of the work between the host and the GPU:

  * workers hand over **uint8** pixels.  A batch crosses PCIe as ONE `[B, H, W, 4]` uint8 tensor
    (R, G, B, valid): 4 bytes per pixel instead of the reference's 12 (three fp32 planes, normalised by the
    dataset workers one channel at a time, data.py:111-117).
  * normalisation happens on the device, as a 3 x 256-entry table lookup.  The table holds
    `((v / 255) - mean) / std` evaluated in float32 on the host in the reference's operation order, so the
    pixels are bit-identical to the reference's whatever the device's division or fusion rules are; pad
    pixels (valid == 0) become +0.0 exactly like `F.pad` of the normalised image.
  * the batch is born NHWC: `[B, H, W, 3]` viewed as `[B, 3, H, W]` IS a channels_last tensor, the layout
    the convolutions want (the reference builds NCHW and converts every batch, infer.py:75, train.py:96).

With `device_resize=True` the resize moves to the device as well: workers hand over the decoded SOURCE pixels (uint8 RGB, 3
bytes per pixel) with the tables of Pillow's fixed-point bilinear resampling (`resample_weights`), and one HIP launch per batch
(`odtk_preprocess_images`) resizes, mirrors, pads and normalises -- bit-identical to the host path, see `SourceBatch`.
`device_augment=True` is that hand-over plus the training augmentations: the workers draw the quarter turn, the flip and the
colour factors and ship them as descriptors; the turn (Pillow's fixed-point index map), brightness, contrast, hue and saturation
run on the device between the resize and the normalisation (`odtk_augment_images`), bit-identical to Pillow on the host.
`augment_free_rotate=(lo, hi)` adds a rotation by a free angle between the quarter turn and the flip: Pillow's bilinear
`Image.rotate` on the host, or, with `device_augment`, six doubles per image and one more pass on the device
(`odtk_augment_images_ex`), the same bytes (`free_rotation_matrix`, `rotate_bilinear`).
`mosaic=p` composes a training item, with probability p, of four images on one canvas of the primary image's size (`CocoDataset`):
Pillow's `resize`, `crop` and `paste` on the host, or, with `device_augment`, the four source images and one placement record per
output image and one more pass on the device (`odtk_mosaic_images`), the same bytes (`mosaic_pixels`).

`CocoIndex` is the part of `pycocotools.coco.COCO` (nvidia/cocoapi master, un-pinned and absent from this
image) that the reference touches: `dataset`, `imgs`, `getCatIds`, `getAnnIds`, `loadAnns`, `loadImgs`,
`loadRes`.
"""
import collections
import functools
import json
import math
import os
import random

import numpy as np
import torch
from PIL import Image, ImageEnhance
from torch.utils import data

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


class CocoIndex:
    """Annotation file -> lookup tables, in file order (pycocotools coco.py `createIndex`)."""

    def __init__(self, annotation_file=None, dataset=None):
        if dataset is None:
            if annotation_file is None:
                dataset = {}
            else:
                with open(annotation_file) as f:
                    dataset = json.load(f)
        if not isinstance(dataset, dict):
            raise TypeError('annotation file format {} not supported'.format(type(dataset)))
        self.dataset = dataset
        self.imgs = {im['id']: im for im in dataset.get('images', [])}
        self.cats = {c['id']: c for c in dataset.get('categories', [])}
        self.anns, self.imgToAnns = {}, {}
        for ann in dataset.get('annotations', []):
            self.anns[ann['id']] = ann
            self.imgToAnns.setdefault(ann['image_id'], []).append(ann)

    def getCatIds(self):
        """Category ids in FILE order (coco.py getCatIds with no filter) -- class index k of the network is
        the k-th entry, for training targets and for the detections' `category_id` alike."""
        return [c['id'] for c in self.dataset.get('categories', [])]

    def getImgIds(self):
        return list(self.imgs.keys())

    def getAnnIds(self, imgIds=()):
        ids = [imgIds] if not isinstance(imgIds, (list, tuple)) else imgIds
        if not ids:
            return [a['id'] for a in self.dataset.get('annotations', [])]
        return [a['id'] for i in ids for a in self.imgToAnns.get(i, [])]

    def loadAnns(self, ids=()):
        return [self.anns[i] for i in ids] if isinstance(ids, (list, tuple)) else [self.anns[ids]]

    def loadImgs(self, ids=()):
        return [self.imgs[i] for i in ids] if isinstance(ids, (list, tuple)) else [self.imgs[ids]]

    def loadRes(self, detections):
        """A result set over the same images (coco.py loadRes, bbox branch): every detection gets
        `area = w * h`, `id = position + 1`, `iscrowd = 0`.  Rotated detections keep their polygon but
        are indexed by their axis-aligned extent (mask rasterisation is not part of this port)."""
        known = set(self.imgs)
        anns = []
        for k, det in enumerate(detections):
            if det['image_id'] not in known:
                raise AssertionError('Results do not correspond to current coco set')
            ann = dict(det)
            ann['area'] = det['bbox'][2] * det['bbox'][3]
            ann['id'] = k + 1
            ann['iscrowd'] = 0
            anns.append(ann)
        out = {'images': list(self.dataset.get('images', [])), 'annotations': anns}
        if 'categories' in self.dataset:
            out['categories'] = self.dataset['categories']
        return CocoIndex(dataset=out)


def normalisation_table(dtype=torch.float32):
    """[3, 256]: `((v / 255) - mean) / std` in float32, the reference's operation order (data.py:112-117)."""
    v = torch.arange(256, dtype=torch.float32).div(255)
    rows = [v.clone().sub_(m).div_(s) for m, s in zip(MEAN, STD)]
    return torch.stack(rows).to(dtype)


def normalise_batch(packed, table=None, dtype=torch.float32):
    """`[B, H, W, 4]` uint8 (R, G, B, valid) on any device -> `[B, 3, H, W]` `dtype`, channels_last storage."""
    if table is None:
        table = normalisation_table(dtype)
    table = table.to(device=packed.device, dtype=dtype).reshape(-1)
    index = packed[..., :3].to(torch.int32) + torch.tensor([0, 256, 512], dtype=torch.int32, device=packed.device)
    pixels = torch.where(packed[..., 3:4] != 0, table[index], torch.zeros((), dtype=dtype, device=packed.device))
    return pixels.permute(0, 3, 1, 2)


def _batch_buffer(shape):
    """Uninitialised uint8 tensor for a collated batch.  Inside a loader worker it is born in shared memory, which is
    how the batch reaches the main process anyway (torch's default collate does the same): one first touch of the pages
    instead of two (private buffer, then the copy into a fresh shared segment)."""
    if data.get_worker_info() is None:
        return torch.empty(shape, dtype=torch.uint8)
    proto = torch.empty(0, dtype=torch.uint8)
    storage = proto._typed_storage()._new_shared(math.prod(shape), device=proto.device)
    return proto.new(storage).resize_(*shape)


# -- Pillow's 8-bit bilinear resampling, restated -----------------------------------------------------------------------------------
# `Image.resize(size, Image.BILINEAR)` on an 8-bit image is fixed-point integer arithmetic over weights computed in double.  The
# weights below are what the device path ships (include/odtk_hip.h: odtk_preprocess_images); applied with numpy they are the CPU
# implementation of the same pipeline.

RESAMPLE_BITS = 22                                                  # Pillow's PRECISION_BITS = 32 - 8 - 2


@functools.lru_cache(maxsize=512)
def resample_weights(in_size, out_size):
    """One axis of `Image.resize(.., Image.BILINEAR)`, `in_size` -> `out_size` pixels (default box, no reducing_gap):
    (bounds int32 [out_size, 2] = first source index and number of taps per output index, weights int32 [out_size, taps] in units
    of 2^-22, zero beyond a row's taps).  Every step in IEEE double and in Pillow's operation order: the triangle filter is
    stretched by max(in / out, 1), evaluated at `(i + first - center + 0.5) * (1 / stretch)` (a product with the reciprocal, not
    a quotient), the weights are normalised by their sum taken in index order and rounded to fixed point half away from zero."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError('resample_weights: sizes must be positive, got %d -> %d' % (in_size, out_size))
    scale = in_size / out_size
    stretch = max(scale, 1.0)
    support = 1.0 * stretch                                         # the triangle filter's own support is 1
    taps = int(math.ceil(support)) * 2 + 1
    inverse = 1.0 / stretch
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    first = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    count = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - first
    tap = np.arange(taps, dtype=np.int64)[None, :]
    t = np.abs(((tap + first[:, None]) - center[:, None] + 0.5) * inverse)
    w = np.where(t < 1.0, 1.0 - t, 0.0)
    w[tap >= count[:, None]] = 0.0
    total = np.zeros(out_size, dtype=np.float64)
    for i in range(taps):                                           # in index order, from 0.0 (x + 0.0 == x: the masked taps add nothing)
        total = total + w[:, i]
    with np.errstate(divide='ignore', invalid='ignore'):
        w = np.where(total[:, None] != 0.0, w / total[:, None], w)
    weights = np.trunc(w * float(1 << RESAMPLE_BITS) + np.where(w < 0.0, -0.5, 0.5)).astype(np.int32)
    bounds = np.stack([first, count], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    weights.setflags(write=False)
    return bounds, weights


def _resample_pass(pixels, bounds, weights, axis):
    """One pass along `axis` (0: vertical, 1: horizontal) of uint8 `[h, w, c]`: clamp((2^21 + sum src * weight) >> 22) per channel."""
    pixels = np.moveaxis(pixels, axis, 0).astype(np.int32)
    first, last = bounds[:, 0].astype(np.int64), pixels.shape[0] - 1
    acc = np.full((bounds.shape[0],) + pixels.shape[1:], 1 << (RESAMPLE_BITS - 1), dtype=np.int32)
    for i in range(weights.shape[1]):                               # weights beyond a row's taps are zero: the clamped index adds nothing
        acc += pixels[np.minimum(first + i, last)] * weights[:, i].reshape((-1,) + (1,) * (pixels.ndim - 1))
    return np.moveaxis(np.clip(acc >> RESAMPLE_BITS, 0, 255).astype(np.uint8), 0, axis)


def resize_bilinear(pixels, size):
    """`np.array(Image.fromarray(pixels).resize(size, Image.BILINEAR))` for uint8 `[h, w, c]`, `size = (width, height)`, without
    Pillow: the horizontal pass first, rounded to bytes, then the vertical pass on those bytes; a pass that would not change
    the length is skipped."""
    pixels = np.asarray(pixels)
    width, height = int(size[0]), int(size[1])
    if pixels.shape[1] != width:
        pixels = _resample_pass(pixels, *resample_weights(pixels.shape[1], width), axis=1)
    if pixels.shape[0] != height:
        pixels = _resample_pass(pixels, *resample_weights(pixels.shape[0], height), axis=0)
    return np.ascontiguousarray(pixels)


# -- Pillow's quarter turns and colour enhancements, restated ------------------------------------------------------------------------
# What `__getitem__` does to the resized image in training -- `Image.rotate` by a quarter turn, FLIP_LEFT_RIGHT, ImageEnhance's
# Brightness / Contrast / Color and `_adjust_hue` -- in numpy, every step in the number format Pillow's C uses.  They are the CPU
# implementation of `device_augment=True` and what the device path (include/odtk_hip.h: odtk_augment_images) is pinned to.

AUGMENT_BRIGHTNESS, AUGMENT_CONTRAST, AUGMENT_HUE, AUGMENT_SATURATION = 1, 2, 4, 8     # odtk_augment_t.flags
_FIX_ONE = 1 << 16


def _fix(v):
    """Pillow's FIX(): a double to 16.16 fixed point."""
    return int(math.floor(v * 65536.0 + 0.5))


def quarter_turn_map(width, height, angle, expand=False, flip=False):
    """`im.rotate(angle[, expand=True])` of a `width` x `height` image for angle in {0, 90, 180, 270}, then (flip) FLIP_LEFT_RIGHT, as
    an index map: -> (canvas width, canvas height, (a0, a1, a2, a3, a4, a5)) with
        out[y][x] = in[(a5 + a3 x + a4 y) >> 16][(a2 + a0 x + a1 y) >> 16],   black where that lies outside the image.
    180 degrees, and 90 / 270 with `expand` or on a square image, are transposes in Pillow; 90 / 270 otherwise is its NEAREST affine
    transform on the same canvas, evaluated in 16.16 fixed point from the matrix `Image.rotate` builds in double."""
    width, height, angle = int(width), int(height), int(angle) % 360
    if angle not in (0, 90, 180, 270):
        raise ValueError('quarter_turn_map: angle must be a multiple of 90, got %r' % angle)
    cw, ch = width, height
    if angle == 0:
        a = [_FIX_ONE, 0, 0, 0, _FIX_ONE, 0]
    elif angle == 180:
        a = [-_FIX_ONE, 0, (width - 1) * _FIX_ONE, 0, -_FIX_ONE, (height - 1) * _FIX_ONE]
    elif expand or width == height:
        cw, ch = height, width
        if angle == 90:                                             # ROTATE_90: out[y][x] = in[x][width - 1 - y]
            a = [0, -_FIX_ONE, (width - 1) * _FIX_ONE, _FIX_ONE, 0, 0]
        else:                                                       # ROTATE_270: out[y][x] = in[height - 1 - x][y]
            a = [0, _FIX_ONE, 0, -_FIX_ONE, 0, (height - 1) * _FIX_ONE]
    else:
        radians = -math.radians(angle)
        m = [round(math.cos(radians), 15), round(math.sin(radians), 15), 0.0,
             round(-math.sin(radians), 15), round(math.cos(radians), 15), 0.0]
        cx, cy = width / 2, height / 2
        m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
        m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy
        a = [_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]
    if flip:                                                        # after the turn: x -> canvas width - 1 - x, in integers
        a[2], a[0] = a[2] + a[0] * (cw - 1), -a[0]
        a[5], a[3] = a[5] + a[3] * (cw - 1), -a[3]
    return cw, ch, tuple(a)


def index_map(pixels, canvas_width, canvas_height, coefficients):
    """The gather of `quarter_turn_map` on uint8 `[h, w, c]` -> `[canvas_height, canvas_width, c]`."""
    pixels = np.asarray(pixels)
    a0, a1, a2, a3, a4, a5 = (int(v) for v in coefficients)
    x = np.arange(canvas_width, dtype=np.int64)[None, :]
    y = np.arange(canvas_height, dtype=np.int64)[:, None]
    xin, yin = (a2 + a0 * x + a1 * y) >> 16, (a5 + a3 * x + a4 * y) >> 16
    inside = (xin >= 0) & (xin < pixels.shape[1]) & (yin >= 0) & (yin < pixels.shape[0])
    out = pixels[np.clip(yin, 0, pixels.shape[0] - 1), np.clip(xin, 0, pixels.shape[1] - 1)]
    out[~inside] = 0
    return np.ascontiguousarray(out)


def free_rotation_matrix(width, height, angle):
    """The matrix `Image.rotate(angle)` builds for a `width` x `height` image turned about its centre on its own canvas, in double
    and in Pillow's operation order (the entries rounded to 15 places, as there): six coefficients (m0 .. m5) that take the centre
    of an OUTPUT pixel to a point of the input,  xin = m0 (x + 0.5) + m1 (y + 0.5) + m2,  yin = m3 (x + 0.5) + m4 (y + 0.5) + m5.
    `angle` in degrees, any real: positive is counter-clockwise on screen.  The device receives these six doubles."""
    angle = float(angle) % 360.0
    radians = -math.radians(angle)
    m = [round(math.cos(radians), 15), round(math.sin(radians), 15), 0.0,
         round(-math.sin(radians), 15), round(math.cos(radians), 15), 0.0]
    cx, cy = int(width) / 2, int(height) / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
    m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy
    return tuple(m)


def rotate_bilinear(pixels, matrix):
    """`np.array(Image.fromarray(pixels).rotate(angle, resample=Image.BILINEAR))` for uint8 `[h, w, c]` and `matrix` =
    `free_rotation_matrix(w, h, angle)`, without Pillow: its affine transform with the bilinear filter, every step one IEEE double
    operation in its order.  A pixel whose source point lies outside the image is black; inside, the two taps of a row are clamped
    to the row, the row below is used only if it exists, and the result is truncated to a byte."""
    pixels = np.asarray(pixels)
    h, w = pixels.shape[:2]
    m0, m1, m2, m3, m4, m5 = (float(v) for v in matrix)
    x = np.arange(w, dtype=np.float64)[None, :] + 0.5
    y = np.arange(h, dtype=np.float64)[:, None] + 0.5
    xin, yin = (m0 * x + m1 * y) + m2, (m3 * x + m4 * y) + m5
    inside = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
    xin, yin = xin - 0.5, yin - 0.5
    fx, fy = np.floor(xin), np.floor(yin)
    dx, dy = (xin - fx)[..., None], (yin - fy)[..., None]
    col, row = np.clip(fx, -1, w).astype(np.int64), np.clip(fy, -1, h).astype(np.int64)     # (inside: -1 <= floor < size)
    x0, x1 = np.clip(col, 0, w - 1), np.clip(col + 1, 0, w - 1)
    p = pixels.astype(np.float64)
    first, second = p[np.clip(row, 0, h - 1), x0], p[np.clip(row, 0, h - 1), x1]
    v1 = first + (second - first) * dx
    first, second = p[np.clip(row + 1, 0, h - 1), x0], p[np.clip(row + 1, 0, h - 1), x1]
    below = ((row + 1 >= 0) & (row + 1 < h))[..., None]
    v2 = np.where(below, first + (second - first) * dx, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.int64).astype(np.uint8)
    out[~inside] = 0
    return np.ascontiguousarray(out)


def rotate_points(x, y, width, height, angle):
    """Where `rotate_bilinear` (= `Image.rotate(angle)`) moves the points (x, y) of a `width` x `height` image: the inverse of the
    pixel map, out - c = [[cos a, sin a], [-sin a, cos a]] (in - c) about c = (width / 2, height / 2), with the matrix' rounded
    entries; float64 tensors in, float64 tensors out."""
    m = free_rotation_matrix(width, height, angle)
    cos, sin = m[0], m[3]
    cx, cy = int(width) / 2, int(height) / 2
    return cx + (cos * (x - cx) + sin * (y - cy)), cy + (cos * (y - cy) - sin * (x - cx))


def luma(pixels):
    """`convert('L')` of uint8 RGB `[..., 3]`: (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    p = np.asarray(pixels).astype(np.int64)
    return ((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(degenerate, pixels, factor):
    """`Image.blend(degenerate, image, factor)` per byte, in float32: t = d + alpha * (x - d); truncated to a byte when
    0 <= alpha <= 1, clamped to [0, 255] first otherwise (ImageEnhance's `enhance`)."""
    alpha = np.float32(factor)
    d = np.asarray(degenerate).astype(np.float32)
    diff = np.asarray(pixels).astype(np.int32) - np.asarray(degenerate).astype(np.int32)
    t = d + alpha * diff.astype(np.float32)                         # two roundings: product, then sum (no FMA)
    if not 0.0 <= alpha <= 1.0:
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.uint8)


def contrast_mean(pixels):
    """The byte `ImageEnhance.Contrast` blends towards: int(mean of L + 0.5), the mean taken as sum / count in double."""
    grey = luma(pixels)
    return int(int(grey.sum(dtype=np.int64)) / grey.size + 0.5)


def adjust_brightness(pixels, factor):
    return blend(np.zeros_like(pixels), pixels, factor)


def adjust_contrast(pixels, factor):
    return blend(np.full_like(pixels, contrast_mean(pixels)), pixels, factor)


def adjust_saturation(pixels, factor):
    return blend(np.repeat(luma(pixels)[..., None], 3, axis=-1), pixels, factor)


def _clip8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def rgb_to_hsv(pixels):
    """`convert('HSV')` of uint8 RGB `[..., 3]` (Pillow's rgb2hsv_row): float32 quotients, the hue assembled in double and
    rounded to float32, the products with 255 in double, truncated."""
    p = np.asarray(pixels)
    r, g, b = (p[..., k].astype(np.int32) for k in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    f32 = np.float32
    cr = np.where(grey, 1, maxc - minc).astype(f32)
    s = cr / np.where(grey, 1, maxc).astype(f32)
    rc, gc, bc = ((maxc - c).astype(f32) / cr for c in (r, g, b))
    rc64, gc64, bc64 = (c.astype(np.float64) for c in (rc, gc, bc))
    h = np.where(r == maxc, bc64 - gc64, np.where(g == maxc, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64)).astype(f32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(f32)
    hue = _clip8((h.astype(np.float64) * 255.0).astype(np.int64))
    sat = _clip8((s.astype(np.float64) * 255.0).astype(np.int64))
    return np.stack([np.where(grey, 0, hue), np.where(grey, 0, sat), maxc], axis=-1).astype(np.uint8)


def hsv_to_rgb(pixels):
    """`convert('RGB')` of uint8 HSV `[..., 3]` (Pillow's hsv2rgb_row), in double."""
    p = np.asarray(pixels)
    h, s, v = (p[..., k].astype(np.float64) for k in range(3))
    hh = h * 6.0 / 255.0
    i = np.floor(hh)
    f = hh - i
    fs = s / 255.0
    x = _clip8(np.rint(v * (1.0 - fs)))
    q = _clip8(np.rint(v * (1.0 - fs * f)))
    t = _clip8(np.rint(v * (1.0 - fs * (1.0 - f))))
    v8 = p[..., 2]
    sextant = i.astype(np.int64) % 6
    r = np.choose(sextant, [v8, q, x, x, t, v8])
    g = np.choose(sextant, [t, v8, v8, q, x, x])
    b = np.choose(sextant, [x, x, t, v8, v8, q])
    grey = p[..., 1] == 0
    return np.stack([np.where(grey, v8, r), np.where(grey, v8, g), np.where(grey, v8, b)], axis=-1).astype(np.uint8)


def hue_shift_byte(factor):
    """The byte `_adjust_hue` adds to the hue channel."""
    return int(factor * 255) % 256


def adjust_hue(pixels, shift):
    """`_adjust_hue`: RGB -> HSV, hue + `shift` (a byte, wrapping), HSV -> RGB.  Lossy even for a shift of 0."""
    hsv = rgb_to_hsv(pixels)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) & 255
    return hsv_to_rgb(hsv)


def augment_pixels(pixels, aug, rotation=None):
    """Resized uint8 RGB `[h, w, 3]` and one AUGMENT_DTYPE record -> the augmented canvas: turn and flip (the index map), then
    brightness, contrast, hue, saturation, in `__getitem__`'s order.  With an enabled ROTATION_DTYPE record the map holds the turn
    alone, and the free rotation (on the turned canvas) and the record's flip follow it, before the colours."""
    pixels = index_map(pixels, int(aug['canvas_width']), int(aug['canvas_height']), aug['map'])
    if rotation is not None and int(rotation['enabled']):
        pixels = rotate_bilinear(pixels, rotation['matrix'])
        if int(rotation['flip']):
            pixels = np.ascontiguousarray(pixels[:, ::-1])
    flags = int(aug['flags'])
    if flags & AUGMENT_BRIGHTNESS:
        pixels = adjust_brightness(pixels, aug['brightness'])
    if flags & AUGMENT_CONTRAST:
        pixels = adjust_contrast(pixels, aug['contrast'])
    if flags & AUGMENT_HUE:
        pixels = adjust_hue(pixels, int(aug['hue']))
    if flags & AUGMENT_SATURATION:
        pixels = adjust_saturation(pixels, aug['saturation'])
    return pixels


# -- mosaic: four images on one canvas ------------------------------------------------------------------------------------------------
# Tile k = 0..3 (top-left, top-right, bottom-left, bottom-right) is its image resized once, mirrored or not, touching the centre
# (cx, cy) with one corner and cropped to its quadrant.  `mosaic_placement` and `mosaic_tile_boxes` are shared by the host path and
# the device path; `mosaic_pixels` is the CPU implementation the device path (include/odtk_hip.h: odtk_mosaic_images) is pinned to.

MOSAIC_FILL = (114, 114, 114)                                       # the canvas where no tile lies
MOSAIC_MIN_AREA = 0.2                                               # a box stays only with this share of its scaled area left after the clip


def mosaic_placement(k, tile_width, tile_height, cx, cy, width, height):
    """Where tile `k` of `tile_width` x `tile_height` pixels goes on a `width` x `height` canvas with the centre (cx, cy):
    -> (dst_x, dst_y, dw, dh, src_x, src_y), the dw x dh pixels of the tile from (src_x, src_y) on pasted at (dst_x, dst_y)."""
    left, top = k in (0, 2), k in (0, 1)
    dw = min(tile_width, cx if left else width - cx)
    dh = min(tile_height, cy if top else height - cy)
    return (cx - dw if left else cx, cy - dh if top else cy, dw, dh, tile_width - dw if left else 0, tile_height - dh if top else 0)


def mosaic_tile_boxes(boxes, scale, tile_width, mirror, placement):
    """The boxes `[N, 4]` (x, y, w, h in source pixels) of one tile on the canvas, in float64: scaled, flipped within the tile if it
    is mirrored, shifted by dst - src and clipped to the tile's destination rectangle -> (boxes float64 [N, 4], keep bool [N]): a box
    stays if at least a pixel of its width and of its height and MOSAIC_MIN_AREA of its scaled area are left."""
    dx, dy, dw, dh, sx, sy = placement
    x, y, w, h = (boxes[:, k].double() * scale for k in range(4))
    if mirror:
        x = tile_width - x - w
    x, y = x + (dx - sx), y + (dy - sy)
    left, right = x.clamp(dx, dx + dw), (x + w).clamp(dx, dx + dw)
    top, bottom = y.clamp(dy, dy + dh), (y + h).clamp(dy, dy + dh)
    moved = torch.stack([left, top, right - left, bottom - top], 1)
    keep = (moved[:, 2] >= 1) & (moved[:, 3] >= 1) & (moved[:, 2] * moved[:, 3] >= MOSAIC_MIN_AREA * (w * h))
    return moved, keep


def mosaic_pixels(tiles, record):
    """`Image.new('RGB', canvas, fill)` and one `canvas.paste(tile.crop(..), dst)` per used tile of one MOSAIC_DTYPE record, without
    Pillow: `tiles[s]` is the resized (and mirrored) uint8 `[h, w, 3]` image that a tile names as its `source`; tiles are pasted in
    their order, so a later one covers an earlier one -> the canvas, uint8 `[canvas_height, canvas_width, 3]`."""
    canvas = np.empty((int(record['canvas_height']), int(record['canvas_width']), 3), dtype=np.uint8)
    canvas[:] = record['fill']
    for tile in record['tiles']:
        if int(tile['source']) < 0:
            continue
        dx, dy, w, h, sx, sy = (int(tile[f]) for f in ('dst_x', 'dst_y', 'width', 'height', 'src_x', 'src_y'))
        canvas[dy:dy + h, dx:dx + w] = np.asarray(tiles[int(tile['source'])])[sy:sy + h, sx:sx + w]
    return canvas


# The geometry of a mosaic item for `SourceBatch.pack`: the canvas, sources = ((out_width, out_height, mirror) per source image of the
# item), tiles = ((k, index into sources, dst_x, dst_y, width, height, src_x, src_y) per used tile) and the colour operations.  The
# item's pixels are the list of its source images.
MosaicGeometry = collections.namedtuple('MosaicGeometry', 'width height sources tiles flags brightness contrast saturation hue')


# -- a batch of source images in one buffer -----------------------------------------------------------------------------------------
AUGMENT_DTYPE = np.dtype([('canvas_width', '<i4'), ('canvas_height', '<i4'), ('map', '<i4', (6,)), ('flags', '<u4'),
                          ('brightness', '<f4'), ('contrast', '<f4'), ('saturation', '<f4'), ('hue', 'u1'), ('pad_', 'u1', (3,))])
                                                                    # odtk_augment_t (include/odtk_hip.h)
ROTATION_DTYPE = np.dtype([('matrix', '<f8', (6,)), ('enabled', '<i4'), ('flip', '<i4')])     # odtk_rotation_t (include/odtk_hip.h)
IMAGE_DTYPE =np.dtype([('src_offset', '<u8'), ('src_width', '<i4'), ('src_height', '<i4'), ('src_pitch', '<i4'),
                        ('out_width', '<i4'), ('out_height', '<i4'), ('mirror', '<i4'), ('x_table', '<i4'), ('y_table', '<i4'),
                        ('x_taps', '<i4'), ('y_taps', '<i4')])      # odtk_image_t (include/odtk_hip.h)
MOSAIC_TILE_DTYPE = np.dtype([('source', '<i4'), ('dst_x', '<i4'), ('dst_y', '<i4'), ('width', '<i4'), ('height', '<i4'),
                              ('src_x', '<i4'), ('src_y', '<i4')])  # odtk_mosaic_tile_t (include/odtk_hip.h)
MOSAIC_DTYPE = np.dtype([('canvas_width', '<i4'), ('canvas_height', '<i4'), ('tiles', MOSAIC_TILE_DTYPE, (4,)), ('fill', 'u1', (3,)),
                         ('pad_', 'u1')])                           # odtk_mosaic_t (include/odtk_hip.h)
_HEADER_WORDS = 8                                                   # int32: batch, height, width, tables at byte, tables length, augments at byte (0: none), rotations at byte (0: none), mosaics at byte (0: none)
_up16 = lambda n: (n + 15) // 16 * 16


class SourceBatch:
    """What a worker hands over with `device_resize=True`: ONE uint8 buffer per batch =
        header (8 int32) | odtk_image_t per image | the resampling tables of the batch (int32) | source pixels, 3 bytes each
    so that the source-size pixels, not the resized ones, cross shared memory and PCIe, in one upload.  `pack` writes it (inside
    a loader worker, straight into shared memory), `descriptors` / `tables` read it back, `apply_cpu` is the pipeline in numpy and
    torch: resize, mirror, pad, normalise -- the CPU implementation of `odtk_preprocess_images`.

    With `device_augment=True` the geometry tuples are longer (`CocoDataset._augment_item`) and the buffer carries one
    odtk_augment_t per image between the image descriptors and the tables (the header's sixth word says where): the index map of
    the quarter turn and the flip, and the colour operations.  The batch is then padded to the canvases AFTER the turn, and
    `apply_cpu` is the CPU implementation of `odtk_augment_images`.

    With `augment_free_rotate` the tuples of the rotated images carry two more entries, the matrix of `free_rotation_matrix` and the
    flip, and the buffer one odtk_rotation_t per image after the augment records (the header's seventh word says where; it is 0,
    and the buffer is what it was, when no image of the batch is rotated).  The map of such an image is the quarter turn alone:
    the free rotation and then the flip follow it on the turned canvas (`odtk_augment_images_ex`).

    With `mosaic` an item may bring up to four source images (`MosaicGeometry`).  The image descriptors and the pixels are then those
    of ALL sources of the batch, in item order, the augment records (identity map, the colours) stay one per OUTPUT image, and
    behind them come 16 bytes (the number of sources, 0, 0, 0) and one odtk_mosaic_t per output image that says which sources go
    where on its canvas (the header's eighth word says where; it is 0, and the buffer is what it was, when no item is a mosaic).
    An item of such a batch that is no mosaic becomes a record of one tile (`odtk_mosaic_images`)."""

    @staticmethod
    def pack(sources, geometry, stride):
        """sources: uint8 `[h, w, 3]` tensors; geometry: `(out_width, out_height, mirror)` per image, or (device_augment)
        `(out_width, out_height, 0, canvas_width, canvas_height, map, flags, brightness, contrast, saturation, hue)`, or (free
        rotation) that with `(matrix, flip)` appended; or (mosaic) a `MosaicGeometry`, whose entry of `sources` is the list of
        the item's source images.  From here on `geometry` describes the OUTPUT images and `resized` the source images: one each,
        the same, unless the batch has a mosaic."""
        up = lambda d: d + (stride - d % stride) % stride
        mosaics = None
        if any(isinstance(g, MosaicGeometry) for g in geometry):
            sources, geometry, resized, mosaics = SourceBatch._mosaic_records(sources, geometry)
        augmented = any(len(g) > 3 for g in geometry)
        if augmented:                                               # plain images of such a batch get the identity map
            geometry = [g if len(g) > 3 else g[:2] + (0,) + quarter_turn_map(g[0], g[1], 0, flip=g[2]) + (0, 1.0, 1.0, 1.0, 0)
                        for g in geometry]
        if mosaics is None:
            resized = [g[:3] for g in geometry]
        height = max(up(g[4] if augmented else g[1]) for g in geometry)
        width = max(up(g[3] if augmented else g[0]) for g in geometry)
        tables, where, length = [], {}, 0
        def table(in_size, out_size):
            nonlocal length
            if in_size == out_size:
                return -1, 0
            if (in_size, out_size) not in where:
                bounds, weights = resample_weights(in_size, out_size)
                where[(in_size, out_size)] = (length, weights.shape[1])
                tables.extend((bounds.reshape(-1), weights.reshape(-1)))
                length += bounds.size + weights.size
            return where[(in_size, out_size)]
        images = np.zeros(len(sources), dtype=IMAGE_DTYPE)
        for im, p, (ow, oh, mirror) in zip(images, sources, resized):
            h, w = p.shape[:2]
            im['src_width'], im['src_height'], im['src_pitch'] = w, h, 3 * w
            im['out_width'], im['out_height'], im['mirror'] = ow, oh, int(bool(mirror))
            im['x_table'], im['x_taps'] = table(w, ow)
            im['y_table'], im['y_taps'] = table(h, oh)
        augments = np.zeros(len(geometry) if augmented else 0, dtype=AUGMENT_DTYPE)
        for aug, g in zip(augments, geometry):
            aug['canvas_width'], aug['canvas_height'], aug['map'], aug['flags'] = g[3], g[4], g[5], g[6]
            aug['brightness'], aug['contrast'], aug['saturation'], aug['hue'] = g[7], g[8], g[9], g[10]
        rotated = any(len(g) > 11 for g in geometry)
        rotations = np.zeros(len(geometry) if rotated else 0, dtype=ROTATION_DTYPE)
        for rot, g in zip(rotations, geometry):
            if len(g) > 11:
                rot['matrix'], rot['enabled'], rot['flip'] = g[11], 1, int(bool(g[12]))
        augments_at = _up16(4 * _HEADER_WORDS + images.nbytes) if augmented else 0
        rotations_at = _up16(augments_at + augments.nbytes) if rotated else 0
        tables_at = _up16(max(augments_at, rotations_at, 4 * _HEADER_WORDS + images.nbytes) + (rotations.nbytes if rotated else augments.nbytes))
        mosaics_at = 0
        if mosaics is not None:                                     # 16 bytes (the number of source images, 0, 0, 0), then the records
            mosaics_at = _up16(augments_at + augments.nbytes)
            tables_at = _up16(mosaics_at + 16 + mosaics.nbytes)
        at = _up16(tables_at + 4 * length)
        for im in images:
            im['src_offset'] = at
            at = _up16(at + int(im['src_pitch']) * int(im['src_height']))
        buffer = _batch_buffer((at,))
        view = buffer.numpy()
        view[:4 * _HEADER_WORDS].view(np.int32)[:] = (len(geometry), height, width, tables_at, length, augments_at, rotations_at, mosaics_at)
        view[4 * _HEADER_WORDS:4 * _HEADER_WORDS + images.nbytes] = images.view(np.uint8)
        if augmented:
            view[augments_at:augments_at + augments.nbytes] = augments.view(np.uint8)
        if rotated:
            view[rotations_at:rotations_at + rotations.nbytes] = rotations.view(np.uint8)
        if mosaics is not None:
            view[mosaics_at:mosaics_at + 16].view(np.int32)[:] = (len(sources), 0, 0, 0)
            view[mosaics_at + 16:mosaics_at + 16 + mosaics.nbytes] = mosaics.view(np.uint8)
        if tables:
            view[tables_at:tables_at + 4 * length].view(np.int32)[:] = np.concatenate(tables)
        for im, p in zip(images, sources):
            start = int(im['src_offset'])
            view[start:start + p.numel()] = p.numpy().reshape(-1)
        return buffer

    @staticmethod
    def _mosaic_records(sources, geometry):
        """A batch with a mosaic item -> (the source images of all items in one list, one plain `device_augment` geometry per output
        image: its canvas, the identity map and its colours, `(out_width, out_height, mirror)` per source image, one MOSAIC_DTYPE
        record per output image).  An item that is no mosaic becomes a record of one tile that covers its canvas; its flip, which
        its map held, becomes the source's mirror."""
        flat, resized, canvases = [], [], []
        records = np.zeros(len(geometry), dtype=MOSAIC_DTYPE)
        records['tiles']['source'] = -1
        records['fill'] = MOSAIC_FILL
        for record, pixels, g in zip(records, sources, geometry):
            if isinstance(g, MosaicGeometry):
                width, height, colour = g.width, g.height, tuple(g[4:])
                for k, source, *rectangle in g.tiles:
                    record['tiles'][k] = (len(flat) + source,) + tuple(rectangle)
                flat.extend(pixels)
                resized.extend(g.sources)
            else:
                if len(g) > 11 or (len(g) > 3 and (tuple(g[3:5]) != tuple(g[:2]) or g[5][1] or g[5][3])):
                    raise ValueError('SourceBatch.pack: a batch with a mosaic cannot hold a turned or rotated image')
                width, height = g[:2]
                colour = (0, 1.0, 1.0, 1.0, 0) if len(g) == 3 else tuple(g[6:11])
                record['tiles'][0] = (len(flat), 0, 0, width, height, 0, 0)
                flat.append(pixels)
                resized.append((width, height, int(bool(g[2] if len(g) == 3 else g[5][0] < 0))))
            record['canvas_width'], record['canvas_height'] = width, height
            canvases.append((width, height, 0) + quarter_turn_map(width, height, 0) + colour)
        return flat, canvases, resized, records

    def __init__(self, buffer):
        """buffer: the packed uint8 tensor, in HOST memory (the descriptors are kernel arguments)."""
        self.buffer = buffer
        self.view = buffer.numpy()
        header = self.view[:4 * _HEADER_WORDS].view(np.int32)
        self.batch, self.height, self.width, self.tables_at, self.tables_len, augments_at, rotations_at, mosaics_at = (int(v) for v in header[:8])
        self.mosaics = None                                         # one MOSAIC_DTYPE record per output image when one of them is a mosaic
        n_images = self.batch                                       # source images: one per output image unless there are mosaics
        if mosaics_at:
            n_images = int(self.view[mosaics_at:mosaics_at + 4].view(np.int32)[0])
            self.mosaics = self.view[mosaics_at + 16:mosaics_at + 16 + self.batch * MOSAIC_DTYPE.itemsize].view(MOSAIC_DTYPE)
        self.images = self.view[4 * _HEADER_WORDS:4 * _HEADER_WORDS + n_images * IMAGE_DTYPE.itemsize].view(IMAGE_DTYPE)
        self.augments = None                                        # one AUGMENT_DTYPE record per image with `device_augment`
        if augments_at:
            self.augments = self.view[augments_at:augments_at + self.batch * AUGMENT_DTYPE.itemsize].view(AUGMENT_DTYPE)
        self.rotations = None                                       # one ROTATION_DTYPE record per image when one of them is rotated
        if rotations_at:
            self.rotations = self.view[rotations_at:rotations_at + self.batch * ROTATION_DTYPE.itemsize].view(ROTATION_DTYPE)

    def tables(self, buffer=None):
        """The int32 tables as a view of `buffer` (default: the host copy; pass the uploaded one for the device's view)."""
        buffer = self.buffer if buffer is None else buffer
        return buffer[self.tables_at:self.tables_at + 4 * self.tables_len].view(torch.int32)

    def source(self, k):
        im = self.images[k]
        start, h, w = int(im['src_offset']), int(im['src_height']), int(im['src_width'])
        return self.view[start:start + 3 * w * h].reshape(h, w, 3)

    def apply_cpu(self, table, dtype=torch.float32):
        """-> `[B, 3, H, W]` `dtype`, channels_last storage: what `odtk_preprocess_images` (with augment descriptors:
        `odtk_augment_images`, with rotation records `odtk_augment_images_ex`, with mosaic records `odtk_mosaic_images`) writes,
        computed on the host."""
        table = table.to(device='cpu', dtype=dtype).reshape(-1)
        out = torch.zeros((self.batch, self.height, self.width, 3), dtype=dtype)
        channel = torch.tensor([0, 256, 512])
        resized = []
        for k, im in enumerate(self.images):
            pixels = resize_bilinear(self.source(k), (int(im['out_width']), int(im['out_height'])))
            if im['mirror']:
                pixels = pixels[:, ::-1].copy()
            if self.mosaics is not None:                            # the sources first, then the canvases below
                resized.append(pixels)
                continue
            if self.augments is not None:
                pixels = augment_pixels(pixels, self.augments[k], None if self.rotations is None else self.rotations[k])
            out[k, :pixels.shape[0], :pixels.shape[1]] = table[torch.from_numpy(pixels).long() + channel]
        for k, record in enumerate(self.mosaics if self.mosaics is not None else ()):
            pixels = augment_pixels(mosaic_pixels(resized, record), self.augments[k])
            out[k, :pixels.shape[0], :pixels.shape[1]] = table[torch.from_numpy(pixels).long() + channel]
        return out.permute(0, 3, 1, 2)



def _adjust_hue(im, factor):
    """Shift the hue channel by `factor` turns (|factor| <= 0.5), wrapping: what torchvision's PIL
    `adjust_hue` does (the reference calls it, data.py:101-105; torchvision is absent here)."""
    if im.mode in ('L', '1', 'I', 'F'):
        return im
    h, s, v = im.convert('HSV').split()
    shifted = np.array(h, dtype=np.uint8)
    with np.errstate(over='ignore'):
        shifted += np.uint8(int(factor * 255) % 256)
    return Image.merge('HSV', (Image.fromarray(shifted, 'L'), s, v)).convert(im.mode)


class CocoDataset(data.dataset.Dataset):
    """One image (and its boxes) per item.  Items are `(pixels uint8 [h, w, 4] = R, G, B, 255, ...)`: normalisation and
    padding are done per BATCH (see the module docstring); everything else follows reference data.py:13-181.

    The random decisions of training are drawn from `random` in the reference's order (resize jitter,
    quarter-turn, flip, brightness, contrast, hue, saturation), so a seeded run makes the same choices.

    `augment_free_rotate=(lo, hi)`, in degrees: every training item is rotated about its centre, on its own canvas, by an angle drawn
    uniformly from the range, between the quarter turn and the flip (`Image.rotate(angle, resample=Image.BILINEAR)`; the corners it
    leaves empty are black image pixels) and its boxes move with it (`_rotate_boxes`).  (0, 0), the default, is off: no draw is taken.

    `mosaic=p`, `mosaic_scale=(lo, hi)`: with probability p (drawn behind the jitter draw; 0, the default, takes no draw) a training
    item is a mosaic (`_mosaic_plan`): a canvas of the primary image's resized size, grey (114), on which four images -- the primary
    and three drawn from the whole set -- each resized ONCE by its own ratio times g (g uniform in the scale range) and mirrored
    or not, touch a centre drawn in the middle half of the canvas with one corner and are cropped to their quadrant.  Boxes are
    clipped to their tile and stay with a pixel of width and height and MOSAIC_MIN_AREA of their area left; the colours follow on
    the canvas.  An item that is not a mosaic continues as without the option.  It refuses the quarter turns, the free rotation,
    rotated boxes and `device_resize` alone.

    `device_resize=True`: items are source pixels and the target geometry (`_source_item`); it refuses the quarter turns and the
    colour options and the free rotation.  `device_augment=True`: the same hand-over, and those travel as descriptors
    (`_augment_item`)."""

    box_fields = 4

    def __init__(self, path, resize, max_size, stride, annotations=None, training=False, rotate_augment=False,
                 augment_brightness=0.0, augment_contrast=0.0, augment_hue=0.0, augment_saturation=0.0, device_resize=False,
                 device_augment=False, augment_free_rotate=(0, 0), mosaic=0.0, mosaic_scale=(0.5, 1.0)):
        super().__init__()
        mosaic, mosaic_scale = float(mosaic), tuple(float(v) for v in mosaic_scale)
        if not 0.0 <= mosaic <= 1.0:
            raise ValueError('mosaic must be a probability in [0, 1], got %r' % (mosaic,))
        if len(mosaic_scale) != 2 or not 0.0 < mosaic_scale[0] <= mosaic_scale[1] <= 1.0:
            raise ValueError('mosaic_scale must be a range (lo, hi) with 0 < lo <= hi <= 1, got %r' % (mosaic_scale,))
        if mosaic:
            for name, value in (('rotate_augment', rotate_augment), ('augment_free_rotate', any(float(v) for v in augment_free_rotate)),
                                ('rotated boxes', self.box_fields != 4), ('device_resize without device_augment', device_resize and not device_augment)):
                if value:
                    raise ValueError('mosaic cannot be combined with %s' % name)
        self.mosaic, self.mosaic_scale = mosaic, mosaic_scale                                      # 0: off, no draw
        augment_free_rotate = tuple(float(v) for v in augment_free_rotate)
        if len(augment_free_rotate) != 2 or not all(math.isfinite(v) for v in augment_free_rotate) or augment_free_rotate[0] > augment_free_rotate[1]:
            raise ValueError('augment_free_rotate must be a finite range (lo, hi) in degrees with lo <= hi, got %r' % (augment_free_rotate,))
        if device_resize and not device_augment:
            # quarter turns and the colour augmentations act on the RESIZED PIL image in the reference: they stay on the host path
            for name, value in (('rotate_augment', rotate_augment), ('augment_brightness', augment_brightness),
                                ('augment_contrast', augment_contrast), ('augment_hue', augment_hue),
                                ('augment_saturation', augment_saturation),
                                ('augment_free_rotate', augment_free_rotate if any(augment_free_rotate) else ())):
                if value:
                    raise ValueError('device_resize=True cannot be combined with %s=%r: that augmentation works on the resized '
                                     'image on the host (use the default loader)' % (name, value))
        # device_augment: the source-pixel hand-over of device_resize, and the five augmentations travel as descriptors
        self.device_resize, self.device_augment = bool(device_resize or device_augment), bool(device_augment)
        self.path = os.path.expanduser(path)
        self.resize, self.max_size, self.stride = resize, max_size, stride
        self.mean, self.std = list(MEAN), list(STD)
        self.training = training
        self.rotate_augment = rotate_augment
        self.augment_brightness, self.augment_contrast = augment_brightness, augment_contrast
        self.augment_hue, self.augment_saturation = augment_hue, augment_saturation
        self.augment_free_rotate = augment_free_rotate if any(augment_free_rotate) else None       # None: off, no draw
        self.coco = CocoIndex(dataset=annotations) if isinstance(annotations, dict) else CocoIndex(annotations)
        self.ids = list(self.coco.imgs.keys())
        if 'categories' in self.coco.dataset:
            self.categories_inv = {k: i for i, k in enumerate(self.coco.getCatIds())}

    def __len__(self):
        return len(self.ids)

    # -- geometry ---------------------------------------------------------------------------------------
    def _open(self, image_id):
        """-> the decoded image, the resize ratio (with its jitter draw) and the size the ratio asks for."""
        name = self.coco.loadImgs(image_id)[0]['file_name']
        im = Image.open(os.path.join(self.path, name)).convert('RGB')
        resize = self.resize
        if isinstance(resize, (list, tuple)):
            resize = random.randint(resize[0], resize[-1])
        ratio = resize / min(im.size)
        if ratio * max(im.size) > self.max_size:
            ratio = self.max_size / max(im.size)
        return im, ratio, tuple(int(ratio * d) for d in im.size)

    def _open_resized(self, image_id):
        im, ratio, size = self._open(image_id)
        return im.resize(size, Image.BILINEAR), ratio

    def _quarter_turn(self, im, boxes, angle):
        """Rotate the image by `angle` in {90, 180, 270} on its own canvas and move the boxes with it
        (reference data.py:68-85)."""
        return im.rotate(angle), self._turn_boxes(boxes, angle, *im.size)

    turn_expands = False                                                # `Image.rotate(angle, expand=...)` of `_quarter_turn`

    def _turn_boxes(self, boxes, angle, width, height):
        """The boxes' half of `_quarter_turn`; `width`, `height`: the image BEFORE the turn."""
        x, y, w, h = (boxes[:, k].clone() for k in range(4))
        if angle == 90:
            boxes[:, 0] = y - height / 2 + width / 2
            boxes[:, 1] = width / 2 + height / 2 - x - w
            boxes[:, 2], boxes[:, 3] = h, w
        elif angle == 180:
            boxes[:, 0] = width - x - w
            boxes[:, 1] = height - y - h
        elif angle == 270:
            boxes[:, 0] = width / 2 + height / 2 - y - h
            boxes[:, 1] = x - width / 2 + height / 2
            boxes[:, 2], boxes[:, 3] = h, w
        return boxes

    def _free_rotate(self, im, boxes, categories, angle):
        """Rotate the image by `angle` degrees (any real) about its centre on its own canvas, bilinear, black corners, and move
        the boxes with it; boxes the rotation pushes out of the image are dropped with their categories."""
        return (im.rotate(angle, resample=Image.BILINEAR),) + self._rotate_boxes(boxes, categories, angle, *im.size)

    def _rotate_boxes(self, boxes, categories, angle, width, height):
        """The boxes' half of `_free_rotate` -> (boxes, categories); `width`, `height`: the canvas.  The four corners move with the
        pixels (`rotate_points`, in float64); the box becomes their enclosing axis-aligned box clipped to the canvas, and is dropped
        when less than a pixel of its width or height is left.  None left: the "no box" row of `_get_target`."""
        x, y, w, h = (boxes[:, k].double() for k in range(4))
        xs, ys = rotate_points(torch.stack([x, x + w, x, x + w], 1), torch.stack([y, y, y + h, y + h], 1), width, height, angle)
        left, right = xs.min(1).values.clamp(0, width), xs.max(1).values.clamp(0, width)
        top, bottom = ys.min(1).values.clamp(0, height), ys.max(1).values.clamp(0, height)
        moved = torch.stack([left, top, right - left, bottom - top], 1)
        return self._kept_boxes(moved, categories, (moved[:, 2] >= 1) & (moved[:, 3] >= 1))

    def _kept_boxes(self, boxes, categories, keep):
        if not bool(keep.any()):
            return torch.ones([1, self.box_fields]), torch.ones([1, 1]) * -1
        return boxes[keep].float(), categories[keep]

    def _flip(self, im, boxes):
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
        return im, self._flip_boxes(boxes, im.size[0])

    def _flip_boxes(self, boxes, width):
        boxes[:, 0] = width - boxes[:, 0] - boxes[:, 2]
        return boxes

    def _colour(self, im):
        if self.augment_brightness:
            im = ImageEnhance.Brightness(im).enhance(max(0, random.normalvariate(1, self.augment_brightness)))
        if self.augment_contrast:
            im = ImageEnhance.Contrast(im).enhance(max(0, random.normalvariate(1, self.augment_contrast)))
        if self.augment_hue:
            im = _adjust_hue(im, min(0.5, max(-0.5, random.normalvariate(0, self.augment_hue))))
        if self.augment_saturation:
            im = ImageEnhance.Color(im).enhance(max(0, random.normalvariate(1, self.augment_saturation)))
        return im

    # -- items --------------------------------------------------------------------------------------------
    def _source_item(self, image_id):
        """The item of `device_resize=True`: `(source pixels uint8 [h, w, 3], (out_width, out_height, mirror), ...)` -- the same
        draws from `random` in the same order as the host path (jitter, quarter turn, flip), the targets scaled and flipped as
        there; the image itself is resized and mirrored on the device."""
        im, ratio, size = self._open(image_id)
        pixels = torch.from_numpy(np.array(im, dtype=np.uint8))
        if not self.training:
            return pixels, size + (0,), image_id, ratio
        boxes, categories = self._get_target(image_id)
        boxes[:, :4] *= ratio
        random.randint(0, 3)                                            # the quarter turn's draw (rotate_augment is off here)
        mirror = random.randint(0, 1)
        if mirror:
            boxes = self._flip_boxes(boxes, size[0])
        return pixels, size + (mirror,), torch.cat([boxes, categories], dim=1)

    def _augment_item(self, image_id):
        """The training item of `device_augment=True`: `(source pixels, (out_width, out_height, 0, canvas_width, canvas_height, map,
        flags, brightness, contrast, saturation, hue), target)`.  Every draw from `random` happens here, in the host path's order
        (jitter, quarter turn, flip, brightness, contrast, hue, saturation) and with `_colour`'s clamps; the turn and the flip
        become the index map of `quarter_turn_map`, the colour operations flags and factors -- the pixels are untouched.  With
        `augment_free_rotate` the angle is drawn between the turn and the flip, the map holds the turn alone, and the tuple ends in
        `(free_rotation_matrix of the turned canvas, flip)`."""
        im, ratio, size = self._open(image_id)
        if self.mosaic and random.random() < self.mosaic:
            tiles, target = self._mosaic_plan(image_id, im, ratio, size)
            return self._mosaic_item(tiles, size, target)
        pixels = torch.from_numpy(np.array(im, dtype=np.uint8))
        boxes, categories = self._get_target(image_id)
        boxes[:, :4] *= ratio
        angle = random.randint(0, 3) * 90
        if self.rotate_augment and angle != 0:
            boxes = self._turn_boxes(boxes, angle, *size)
        else:
            angle = 0
        free = random.uniform(*self.augment_free_rotate) if self.augment_free_rotate else None
        mirror = random.randint(0, 1)
        cw, ch, coefficients = quarter_turn_map(size[0], size[1], angle, self.turn_expands, mirror and free is None)
        rotation = ()
        if free is not None:
            boxes, categories = self._rotate_boxes(boxes, categories, free, cw, ch)
            rotation = (free_rotation_matrix(cw, ch, free), mirror)
        if mirror:
            boxes = self._flip_boxes(boxes, cw)
        geometry = size + (0, cw, ch, coefficients) + self._colour_draws() + rotation
        return pixels, geometry, torch.cat([boxes, categories], dim=1)

    def _colour_draws(self):
        """`_colour`'s draws and clamps as descriptors -> (flags, brightness, contrast, saturation, hue)."""
        flags, brightness, contrast, saturation, hue = 0, 1.0, 1.0, 1.0, 0
        if self.augment_brightness:
            flags, brightness = flags | AUGMENT_BRIGHTNESS, max(0, random.normalvariate(1, self.augment_brightness))
        if self.augment_contrast:
            flags, contrast = flags | AUGMENT_CONTRAST, max(0, random.normalvariate(1, self.augment_contrast))
        if self.augment_hue:
            flags, hue = flags | AUGMENT_HUE, hue_shift_byte(min(0.5, max(-0.5, random.normalvariate(0, self.augment_hue))))
        if self.augment_saturation:
            flags, saturation = flags | AUGMENT_SATURATION, max(0, random.normalvariate(1, self.augment_saturation))
        return flags, brightness, contrast, saturation, hue

    # -- mosaic ---------------------------------------------------------------------------------------------
    def _mosaic_plan(self, image_id, im, ratio, size):
        """Every draw of a mosaic item behind its decision, in this order: the scale g, the centre, three more images (from the whole
        set; each with its own `_open` draw), four mirror draws -> (tiles, target).  tiles: `(k, decoded image, tile width, tile
        height, mirror, mosaic_placement)` for every tile that has pixels on the canvas `size`; target: the boxes of those tiles in
        tile order (`mosaic_tile_boxes`), or the "no box" row of `_get_target`."""
        g = random.uniform(*self.mosaic_scale)
        cx, cy = int(random.uniform(0.25, 0.75) * size[0]), int(random.uniform(0.25, 0.75) * size[1])
        opened = [(image_id, im, ratio, size)]
        for _ in range(3):
            other = self.ids[random.randrange(len(self.ids))]
            opened.append((other,) + self._open(other))
        mirrors = [random.randint(0, 1) for _ in range(4)]
        tiles, rows = [], []
        for k, (tile_id, tile_im, tile_ratio, tile_size) in enumerate(opened):
            tw, th = max(1, int(g * tile_size[0])), max(1, int(g * tile_size[1]))
            placement = mosaic_placement(k, tw, th, cx, cy, *size)
            if placement[2] == 0 or placement[3] == 0:
                continue
            tiles.append((k, tile_im, tw, th, mirrors[k], placement))
            boxes, categories = self._get_target(tile_id)
            real = categories[:, 0] >= 0                                 # (the "no box" row is no box)
            moved, keep = mosaic_tile_boxes(boxes[real], tile_ratio * g, tw, mirrors[k], placement)
            rows.append(torch.cat([moved[keep].float(), categories[real][keep]], dim=1))
        target = torch.cat(rows, dim=0) if rows else torch.zeros((0, self.box_fields + 1))
        if not target.shape[0]:
            target = torch.cat([torch.ones([1, self.box_fields]), torch.ones([1, 1]) * -1], dim=1)
        return tiles, target

    def _mosaic_host(self, tiles, size):
        """The canvas of `_mosaic_plan`'s tiles with Pillow: one resize per tile straight from its source, the mirror, crop, paste."""
        canvas = Image.new('RGB', size, MOSAIC_FILL)
        for _, im, tw, th, mirror, (dx, dy, dw, dh, sx, sy) in tiles:
            tile = im.resize((tw, th), Image.BILINEAR)
            if mirror:
                tile = tile.transpose(Image.FLIP_LEFT_RIGHT)
            canvas.paste(tile.crop((sx, sy, sx + dw, sy + dh)), (dx, dy))
        return canvas

    def _mosaic_item(self, tiles, size, target):
        """The mosaic item of `device_augment=True`: `(the tiles' source pixels, MosaicGeometry, target)`; the colour draws happen
        here, behind `_mosaic_plan`'s."""
        pixels = [torch.from_numpy(np.array(t[1], dtype=np.uint8)) for t in tiles]
        geometry = MosaicGeometry(size[0], size[1], tuple((tw, th, mirror) for _, _, tw, th, mirror, _ in tiles),
                                  tuple((t[0], n) + t[5] for n, t in enumerate(tiles)), *self._colour_draws())
        return pixels, geometry, target

    def __getitem__(self, index):
        image_id = self.ids[index]
        if self.device_augment and self.training:
            return self._augment_item(image_id)
        if self.device_resize:
            return self._source_item(image_id)
        if self.training and self.mosaic:                                   # the decision is drawn behind the jitter, before the resize
            im, ratio, size = self._open(image_id)
            if random.random() < self.mosaic:
                tiles, target = self._mosaic_plan(image_id, im, ratio, size)
                im = self._colour(self._mosaic_host(tiles, size))
                return torch.from_numpy(np.array(im.convert('RGBA'), dtype=np.uint8)), target
            im = im.resize(size, Image.BILINEAR)
        else:
            im, ratio = self._open_resized(image_id)
        target = None
        if self.training:
            boxes, categories = self._get_target(image_id)
            boxes[:, :4] *= ratio
            angle = random.randint(0, 3) * 90
            if self.rotate_augment and angle != 0:
                im, boxes = self._quarter_turn(im, boxes, angle)
            if self.augment_free_rotate:
                im, boxes, categories = self._free_rotate(im, boxes, categories, random.uniform(*self.augment_free_rotate))
            if random.randint(0, 1):
                im, boxes = self._flip(im, boxes)
            im = self._colour(im)
            target = torch.cat([boxes, categories], dim=1)
        # [h, w, 4] = R, G, B, 255: PIL writes the `valid` byte of the batch format, and collate then moves whole rows
        pixels = torch.from_numpy(np.array(im.convert('RGBA'), dtype=np.uint8))
        if self.training:
            return pixels, target
        return pixels, image_id, ratio

    def _get_target(self, image_id):
        """Boxes [N, 4|5] and class indices [N, 1] of one image; a single (1, ..., 1 | -1) row when it has
        none (reference data.py:130-152).  Annotations smaller than a pixel both ways are skipped."""
        boxes, categories = [], []
        for ann in self.coco.loadAnns(self.coco.getAnnIds(imgIds=image_id)):
            if ann['bbox'][2] < 1 and ann['bbox'][3] < 1:
                continue
            boxes.append(self._box_of(ann, image_id))
            cat = ann['category_id']
            if 'categories' in self.coco.dataset:
                cat = self.categories_inv[cat]
            categories.append(cat)
        if boxes:
            return torch.tensor(boxes, dtype=torch.float32), torch.tensor(categories, dtype=torch.float32).unsqueeze(1)
        return torch.ones([1, self.box_fields]), torch.ones([1, 1]) * -1

    def _box_of(self, ann, image_id):
        return list(ann['bbox'])

    # -- batches ------------------------------------------------------------------------------------------
    def collate_fn(self, batch):
        """-> (packed uint8 [B, H, W, 4], targets [B, N, box_fields + 1] padded with -1)   (training)
              (packed uint8 [B, H, W, 4], ids int32 [B], ratios float32 [B, 1, 1])          (inference)
        H, W = the largest image of the batch, each first rounded up to a multiple of the stride
        (reference data.py:119-121, 166-176)."""
        pixels = [item[0] for item in batch]
        stride = self.stride
        if self.device_resize:                                              # -> (SourceBatch buffer uint8 [bytes], ...) instead of packed
            packed = SourceBatch.pack(pixels, [item[1] for item in batch], stride)
            batch = [item[:1] + item[2:] for item in batch]
        else:
            up = lambda d: d + (stride - d % stride) % stride
            height = max(up(p.shape[0]) for p in pixels)
            width = max(up(p.shape[1]) for p in pixels)
            packed = _batch_buffer((len(pixels), height, width, 4))
            view = packed.numpy()
            for k, p in enumerate(pixels):
                h, w = p.shape[:2]
                view[k, :h, :w] = p.numpy()                                 # rows of 4 * w contiguous bytes
                view[k, :h, w:] = 0                                         # only the padding is cleared
                view[k, h:] = 0
        if self.training:
            targets = [item[1] for item in batch]
            rows = max(t.shape[0] for t in targets)
            padded = torch.full((len(targets), rows, self.box_fields + 1), -1.0)
            for k, t in enumerate(targets):
                padded[k, :t.shape[0]] = t
            return packed, padded
        ids = torch.tensor([item[1] for item in batch], dtype=torch.int32)
        ratios = torch.tensor([item[2] for item in batch], dtype=torch.float32).view(-1, 1, 1)
        return packed, ids, ratios


class RotatedCocoDataset(CocoDataset):
    """Boxes are `[x, y, w, h, theta]` (theta = 0 appended to plain boxes); quarter turns expand the canvas
    and, with `absolute_angle`, turn theta instead of swapping w and h; a flip negates theta
    (reference data.py:233-415)."""

    box_fields = 5

    def __init__(self, *args, absolute_angle=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.absolute_angle = absolute_angle

    def _box_of(self, ann, image_id):
        box = list(ann['bbox'])
        if len(box) == 4:
            box.append(0.0)
        assert len(box) == 5, 'Bounding box for id %i does not contain five entries.' % image_id
        return box

    turn_expands = True

    def _quarter_turn(self, im, boxes, angle):
        return im.rotate(angle, expand=True), self._turn_boxes(boxes, angle, *im.size)

    def _turn_boxes(self, boxes, angle, width, height):
        x, y, w, h, t = (boxes[:, k].clone() for k in range(5))
        if angle == 90:
            boxes[:, 0], boxes[:, 1] = y, width - x - w
        elif angle == 180:
            boxes[:, 0], boxes[:, 1] = width - x - w, height - y - h
        elif angle == 270:
            boxes[:, 0], boxes[:, 1] = height - y - h, x
        if angle in (90, 270) and not self.absolute_angle:
            boxes[:, 2], boxes[:, 3] = h, w
        if self.absolute_angle:
            t = t + math.radians(angle)
            t = torch.remainder(torch.abs(t), math.pi) * torch.sign(t)
        boxes[:, 4] = t
        return boxes

    def _rotate_boxes(self, boxes, categories, angle, width, height):
        """The centre moves with the pixels, w and h stay, theta grows by the angle (counter-clockwise, the sign of `_turn_boxes`);
        `absolute_angle` wraps theta as `_turn_boxes` does, otherwise theta is folded into [-pi / 4, pi / 4] by quarter turns of the
        box about its own centre (an odd number of them swaps w and h).  A box whose centre leaves the canvas is dropped."""
        x, y, w, h, t = (boxes[:, k].double() for k in range(5))
        cx, cy = rotate_points(x + w / 2, y + h / 2, width, height, angle)
        t = t + math.radians(float(angle) % 360.0)
        if self.absolute_angle:
            t = torch.remainder(torch.abs(t), math.pi) * torch.sign(t)
        else:
            quarters = torch.round(t / (math.pi / 2))
            t = t - quarters * (math.pi / 2)
            odd = torch.remainder(quarters, 2) == 1
            w, h = torch.where(odd, h, w), torch.where(odd, w, h)
        moved = torch.stack([cx - w / 2, cy - h / 2, w, h, t], 1)
        return self._kept_boxes(moved, categories, (cx >= 0) & (cx <= width) & (cy >= 0) & (cy <= height))

    def _flip_boxes(self, boxes, width):
        boxes = super()._flip_boxes(boxes, width)
        boxes[:, 4] = -boxes[:, 4]
        return boxes


class DataIterator:
    """Batches for one rank of a data-parallel job (reference data.py:184-230): `DistributedSampler` shards
    the images when `world > 1`, each rank loads `batch_size // world` of them per step, uploads the uint8
    batch and normalises it on its own GPU.  Yields `(data, targets)` in training and `(data, ids, ratios)`
    in inference, all on `device`; `data` is float `[B, 3, H, W]` with channels_last strides."""

    dataset_class = CocoDataset

    def __init__(self, path, resize, max_size, batch_size, stride, world, annotations, training=False,
                 rotate_augment=False, augment_brightness=0.0, augment_contrast=0.0, augment_hue=0.0,
                 augment_saturation=0.0, device=None, dtype=torch.float32, num_workers=2, rank=None, device_resize=False,
                 device_augment=False, **dataset_args):
        self.resize, self.max_size = resize, max_size
        self.device_resize, self.device_augment = bool(device_resize or device_augment), bool(device_augment)
        if device_resize:
            dataset_args = dict(dataset_args, device_resize=True)
        if device_augment:
            dataset_args = dict(dataset_args, device_augment=True)
        self.dataset = self.dataset_class(path, resize=resize, max_size=max_size, stride=stride,
                                          annotations=annotations, training=training, rotate_augment=rotate_augment,
                                          augment_brightness=augment_brightness, augment_contrast=augment_contrast,
                                          augment_hue=augment_hue, augment_saturation=augment_saturation,
                                          **dataset_args)
        self.ids = self.dataset.ids
        self.coco = self.dataset.coco
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
        self.device, self.dtype = torch.device(device), dtype
        self.table = normalisation_table(dtype).to(self.device)
        world = max(1, world)
        if batch_size % world:
            raise RuntimeError('Batch size should be a multiple of the number of GPUs')
        sampler_args = {} if rank is None else {'num_replicas': world, 'rank': rank}
        self.sampler = data.distributed.DistributedSampler(self.dataset, **sampler_args) if world > 1 else None
        self.dataloader = data.DataLoader(self.dataset, batch_size=batch_size // world, sampler=self.sampler,
                                          collate_fn=self.dataset.collate_fn, num_workers=num_workers,
                                          pin_memory=self.device.type == 'cuda',
                                          # training walks the data set epoch after epoch: keep the workers (starting one
                                          # costs ~0.2 s next to an initialised HIP runtime, profiles/r02_loader_probe.txt)
                                          persistent_workers=bool(training and num_workers > 0))

    def __repr__(self):
        lines = ['    loader: pytorch', '    resize: {}, max: {}'.format(self.resize, self.max_size)]
        if self.device_resize:
            lines.append('    resize on: {}'.format('the device (odtk_preprocess_images)' if self.device.type == 'cuda' else 'the host (numpy)'))
        if self.device_augment:
            lines.append('    augmentations on: {}'.format('the device (odtk_augment_images)' if self.device.type == 'cuda' else 'the host (numpy)'))
        if self.dataset.augment_free_rotate:
            lines.append('    free rotation: {:g} to {:g} degrees'.format(*self.dataset.augment_free_rotate))
        if self.dataset.mosaic:
            lines.append('    mosaic: probability {:g}, scale {:g} to {:g}'.format(self.dataset.mosaic, *self.dataset.mosaic_scale))
        return '\n'.join(lines)

    def __len__(self):
        return len(self.dataloader)

    def _preprocess(self, packed):
        """`device_resize=True` / `device_augment=True`: the batch from a `SourceBatch` buffer -- one upload and one HIP launch on a GPU (the descriptors
        are read from the host copy: they are kernel arguments), the same arithmetic in numpy on the CPU."""
        batch = SourceBatch(packed)
        if self.device.type != 'cuda':
            return batch.apply_cpu(self.table, self.dtype)
        from . import _C
        uploaded = packed.to(self.device, non_blocking=True)
        images = (_C.Image * len(batch.images)).from_buffer_copy(batch.images.tobytes())
        if batch.mosaics is not None:                               # resize of the sources to bytes, composition, (sum of L,) colour chain + table + pad
            mosaics = (_C.Mosaic * batch.batch).from_buffer_copy(batch.mosaics.tobytes())
            augments = (_C.Augment * batch.batch).from_buffer_copy(batch.augments.tobytes())
            return _C.mosaic_images(uploaded, images, mosaics, augments, batch.tables(uploaded), self.table, batch.height, batch.width)
        if batch.augments is not None:                              # resize to bytes, (sum of L,) gather + colour chain + table + pad
            augments = (_C.Augment * batch.batch).from_buffer_copy(batch.augments.tobytes())
            rotations = None                                        # (with them: + the free rotation, between the resize and the sum)
            if batch.rotations is not None:
                rotations = (_C.Rotation * batch.batch).from_buffer_copy(batch.rotations.tobytes())
            return _C.augment_images(uploaded, images, augments, batch.tables(uploaded), self.table, batch.height, batch.width,
                                     rotations=rotations)
        return _C.preprocess_images(uploaded, images, batch.tables(uploaded), self.table, batch.height, batch.width)

    def __iter__(self):
        for packed, *rest in self.dataloader:
            if self.device_resize:
                images = self._preprocess(packed)
            else:
                images = normalise_batch(packed.to(self.device, non_blocking=True), self.table, self.dtype)
            yield (images, *(t.to(self.device, non_blocking=True) for t in rest))


class RotatedDataIterator(DataIterator):
    """`DataIterator` over `RotatedCocoDataset` (reference data.py:418-484); takes `absolute_angle`."""

    dataset_class = RotatedCocoDataset
