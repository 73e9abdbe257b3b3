// mosaic.hpp -- pass M of the mosaic chain (odtk_mosaic_images): up to four resized source images composed on one canvas per output
// image, bit-identical to `Image.new` + `crop` + `paste` of Pillow on the host (odtk/data.py: mosaic_pixels is this pass in numpy).
//
// The chain is the augmentation chain of augment.hpp with one more producer of the "finished canvas in a second slot":
//   A. preprocess_images_kernel<4, true> over the SOURCES (there are more of them than output images): resized bytes, mirror applied,
//      to one slot per source.
//   M. mosaic_compose_kernel (here): the finished canvas BYTES of every output image of the launch go to its canvas slot.  Canvas
//      pixel (x, y) is the pixel (x - dst_x + src_x, y - dst_y + src_y) of the resized source of the highest-numbered tile whose
//      destination rectangle holds (x, y), the fill colour where no tile does.  Its first thread zeroes the image's sum of L.
//   B, C. augment_luma_sum_kernel and augment_images_kernel read the canvas slot through the identity map: their code, and so the
//      colour chain's bits, are the ones of augment.hpp.  The fill is an image pixel: it counts in the contrast's grey level.
//
// Shape (the one of augment_rotate_kernel): a byte gather whose output rows are contiguous.  A thread owns four consecutive canvas
// pixels = 12 bytes = three aligned 32-bit stores (slots are 16-byte aligned, rows follow each other without a gap).  Membership is
// at most four rectangle tests per pixel, and along a row it changes at a tile's edge only, so a wave is uniform along most of
// it; the source bytes of neighbouring lanes are neighbours in the source row.  No LDS, no atomics, no scratch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/odtk_hip.h"

namespace odtk {

constexpr int kMosMaxImages = 16;                // descriptors per launch of pass M (144 bytes each, by value in the kernel arguments)
constexpr int kMosPixels = 4;                    // consecutive pixels per thread

struct MosTile {
  int32_t x0, y0, x1, y1;  // destination rectangle [x0, x1) x [y0, y1) on the canvas; x1 <= x0: the tile is unused
  int32_t ox, oy;          // src - dst: canvas (x, y) reads the resized source at (x + ox, y + oy)
  int32_t rw;              // width of the resized source = pixels per row of its slot
  int32_t source;          // index of the source = of its slot
};

struct MosImage {
  int32_t cw, ch;          // canvas; rows of the canvas slot are 3 * cw bytes apart
  uint32_t fill;           // 0x00BBGGRR
  int32_t pad_;
  MosTile tiles[4];
};

struct MosArgs {
  const uint8_t *bytes;    // resized bytes of source s = bytes + s * src_slot
  uint8_t *canvas;         // finished canvas bytes of output image b = canvas + b * canvas_slot
  unsigned long long *sums;  // one per output image, zeroed here for the sum of L (augment.hpp, pass B)
  uint64_t src_slot, canvas_slot;
  int32_t first;           // batch index of images[0]
  int32_t pad_;
  MosImage images[kMosMaxImages];
};

// Pass M.  grid = (ceil(largest canvas of the launch in pixels / (256 * kMosPixels)), 1, output images of the launch).
__global__ __launch_bounds__(256) void mosaic_compose_kernel(const MosArgs a) {
  const MosImage &im = a.images[blockIdx.z];
  if (blockIdx.x == 0 && threadIdx.x == 0) a.sums[a.first + blockIdx.z] = 0ull;
  const uint32_t pixels = static_cast<uint32_t>(im.cw) * static_cast<uint32_t>(im.ch);
  const uint32_t p0 = (blockIdx.x * 256u + threadIdx.x) * kMosPixels;
  if (p0 >= pixels) return;
  uint8_t *dst = a.canvas + static_cast<size_t>(a.first + blockIdx.z) * a.canvas_slot + static_cast<size_t>(p0) * 3u;
  int32_t y = static_cast<int32_t>(p0 / static_cast<uint32_t>(im.cw)), x = static_cast<int32_t>(p0 - static_cast<uint32_t>(y) * static_cast<uint32_t>(im.cw));
  uint32_t v[kMosPixels];
#pragma unroll
  for (int p = 0; p < kMosPixels; ++p) {
    v[p] = im.fill;
    if (p0 + p < pixels) {
      int hit = -1;                                                 // the highest-numbered tile that holds (x, y)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x >= im.tiles[k].x0 && x < im.tiles[k].x1 && y >= im.tiles[k].y0 && y < im.tiles[k].y1) hit = k;
      if (hit >= 0) {
        // selected field by field: an indexed copy of a descriptor in the kernel arguments would go through scratch
        int32_t ox = im.tiles[0].ox, oy = im.tiles[0].oy, rw = im.tiles[0].rw, source = im.tiles[0].source;
#pragma unroll
        for (int k = 1; k < 4; ++k)
          if (hit == k) ox = im.tiles[k].ox, oy = im.tiles[k].oy, rw = im.tiles[k].rw, source = im.tiles[k].source;
        // host-checked: (x + ox, y + oy) lies inside the resized source, and 3 * its pixels fit 31 bits
        const uint8_t *q = a.bytes + static_cast<size_t>(source) * a.src_slot +
                           (static_cast<uint32_t>(y + oy) * static_cast<uint32_t>(rw) + static_cast<uint32_t>(x + ox)) * 3u;
        v[p] = static_cast<uint32_t>(q[0]) | (static_cast<uint32_t>(q[1]) << 8) | (static_cast<uint32_t>(q[2]) << 16);
      }
    }
    if (++x == im.cw) x = 0, ++y;
  }
  static_assert(kMosPixels == 4, "12 bytes = three words");
  if (p0 + kMosPixels <= pixels) {                                  // slots are 16-byte aligned and p0 * 3 is a multiple of 12
    uint32_t *w = reinterpret_cast<uint32_t *>(dst);
    w[0] = v[0] | (v[1] << 24);
    w[1] = (v[1] >> 8) | (v[2] << 16);
    w[2] = (v[2] >> 16) | (v[3] << 8);
  } else {
#pragma unroll
    for (int p = 0; p < kMosPixels; ++p)
      if (p0 + p < pixels) {
        dst[3 * p] = static_cast<uint8_t>(v[p]);
        dst[3 * p + 1] = static_cast<uint8_t>(v[p] >> 8);
        dst[3 * p + 2] = static_cast<uint8_t>(v[p] >> 16);
      }
  }
}

}  // namespace odtk
