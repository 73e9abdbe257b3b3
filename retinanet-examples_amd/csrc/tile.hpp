// tile.hpp -- tiled (sliced) inference of large images: the tiler that cuts a batch of images into overlapping tiles of one
// fixed size, and the merge that moves the tiles' candidates back into image coordinates.  No reference equivalent; the
// definitions are in include/odtk_hip.h (odtk_tile_images, odtk_merge_tile_candidates).
//
// Both kernels are elementwise, without atomics, LDS, barriers or scratch.  The tile table (up to ODTK_MAX_TILES entries of 16
// bytes) travels in the kernel arguments, and the entry of a workgroup is chosen by blockIdx.y: a uniform index, so the entry
// is read with scalar loads from the kernarg segment and never copied anywhere.
//
// tile_images_kernel.  grid (workgroups per tile, n_tiles); a lane walks the elements of its tile in OUTPUT memory order
// (coalesced stores; the loads are coalesced along the same innermost axis), splits the flat offset with two divisions by launch
// constants (fastdiv.hpp) and copies the element's BITS (uint16_t / uint32_t: nothing is decoded, so NaN payloads, -0.0 and
// infinities survive) or writes +0 where the window leaves the image or the entry is a padding entry (image < 0).
//
// merge_tile_candidates_kernel.  grid (ceil(count / 256), n_tiles); one lane per candidate: score, class and the four box
// scalars are read as bits (no alignment is promised), and written to row `image`, position slot * count + j.  A score that is
// not > 0 is copied; otherwise the cut rule (float32 compares on the tile-local coordinates) or one float32 addition per coordinate.
// Both kernels are templates, so each is compiled only into the object whose host code launches it (input.hip, nms.hip).
#pragma once

#include "common.hpp"
#include "fastdiv.hpp"
#include "../../include/odtk_hip.h"

namespace odtk {

constexpr int kTileThreads = 256;

struct TileArgs {
  const void *x;            // [batch, channels, height, width], NCHW- or NHWC-contiguous
  void *out;                // [n_tiles, channels, tile_h, tile_w], same format
  uint32_t channels, height, width, tile_h, tile_w;
  uint32_t per_tile;        // channels * tile_h * tile_w
  FastDiv inner, middle;    // NCHW: tile_w, tile_h; channels_last: channels, tile_w
  odtk_tile_t tiles[ODTK_MAX_TILES];
};

struct TileMergeArgs {
  const uint32_t *scores, *boxes, *classes;               // [n_tiles, count], [n_tiles, count, 4], [n_tiles, count]: float32 bits
  uint32_t *out_scores, *out_boxes, *out_classes;         // [batch, total], [batch, total, 4], [batch, total]
  uint32_t count;                                         // candidates per tile
  uint32_t total;                                         // slots * count: candidates per image of the output
  int32_t tile_h, tile_w, height, width;
  float border;
  odtk_tile_t tiles[ODTK_MAX_TILES];
};

template <typename U, bool ChannelsLast>
__global__ __launch_bounds__(kTileThreads) void tile_images_kernel(const TileArgs a) {
  const odtk_tile_t t = a.tiles[blockIdx.y];
  U *out = static_cast<U *>(a.out) + static_cast<uint64_t>(blockIdx.y) * a.per_tile;
  const uint64_t image_elements = static_cast<uint64_t>(a.channels) * a.height * a.width;
  const U *src = static_cast<const U *>(a.x) + (t.image < 0 ? 0ull : static_cast<uint64_t>(t.image) * image_elements);
  const uint32_t step = gridDim.x * kTileThreads;                  // (per_tile <= 0xf0000000: `e += step` cannot wrap)
  for (uint32_t e = blockIdx.x * kTileThreads + threadIdx.x; e < a.per_tile; e += step) {
    uint32_t c, r, q, rest;
    if (ChannelsLast) {
      rest = fastdivmod(e, a.inner, &c);                           // e = (r * tile_w + q) * channels + c
      r = fastdivmod(rest, a.middle, &q);
    } else {
      rest = fastdivmod(e, a.inner, &q);                           // e = (c * tile_h + r) * tile_w + q
      c = fastdivmod(rest, a.middle, &r);
    }
    const uint64_t sy = static_cast<uint64_t>(static_cast<uint32_t>(t.y)) + r, sx = static_cast<uint64_t>(static_cast<uint32_t>(t.x)) + q;
    U v = 0;
    if (t.image >= 0 && sy < a.height && sx < a.width)
      v = ChannelsLast ? src[(sy * a.width + sx) * a.channels + c] : src[(static_cast<uint64_t>(c) * a.height + sy) * a.width + sx];
    out[e] = v;
  }
}

// Cut: the launch has a border > 0 (without one the cut rule is compiled out)
template <bool Cut>
__global__ __launch_bounds__(kTileThreads) void merge_tile_candidates_kernel(const TileMergeArgs a) {
  const odtk_tile_t t = a.tiles[blockIdx.y];
  if (t.image < 0) return;                                         // a padding entry
  const uint32_t j = blockIdx.x * kTileThreads + threadIdx.x;
  if (j >= a.count) return;
  const uint64_t src = static_cast<uint64_t>(blockIdx.y) * a.count + j;
  const uint64_t dst = static_cast<uint64_t>(t.image) * a.total + static_cast<uint64_t>(t.slot) * a.count + j;
  uint32_t s = a.scores[src], c = a.classes[src];
  uint32_t b0 = a.boxes[src * 4], b1 = a.boxes[src * 4 + 1], b2 = a.boxes[src * 4 + 2], b3 = a.boxes[src * 4 + 3];
  if (__uint_as_float(s) > 0.0f) {                                 // (a NaN score is copied like a non-positive one)
    const float x1 = __uint_as_float(b0), y1 = __uint_as_float(b1), x2 = __uint_as_float(b2), y2 = __uint_as_float(b3);
    bool cut = false;
    if (Cut) {
      const float far_x = static_cast<float>(a.tile_w - 1) - a.border, far_y = static_cast<float>(a.tile_h - 1) - a.border;
      cut = (t.x > 0 && x1 < a.border) || (t.y > 0 && y1 < a.border) ||
            (static_cast<long long>(t.x) + a.tile_w < a.width && x2 > far_x) ||
            (static_cast<long long>(t.y) + a.tile_h < a.height && y2 > far_y);
    }
    if (cut) {
      s = c = b0 = b1 = b2 = b3 = 0u;                              // an empty slot, as decode leaves them
    } else {
      const float tx = static_cast<float>(t.x), ty = static_cast<float>(t.y);
      b0 = __float_as_uint(x1 + tx);
      b1 = __float_as_uint(y1 + ty);
      b2 = __float_as_uint(x2 + tx);
      b3 = __float_as_uint(y2 + ty);
    }
  }
  a.out_scores[dst] = s;
  a.out_classes[dst] = c;
  a.out_boxes[dst * 4] = b0; a.out_boxes[dst * 4 + 1] = b1; a.out_boxes[dst * 4 + 2] = b2; a.out_boxes[dst * 4 + 3] = b3;
}

}  // namespace odtk
