// preprocess.hpp -- the input side of the network in one launch per batch: Pillow-exact bilinear resize of uint8 RGB source
// images, optional mirror, zero padding to the batch size, normalisation by table, channels_last output (odtk_preprocess_images).
//
// What is reproduced, bit for bit, is `PIL.Image.resize(size, Image.BILINEAR)` on an 8-bit RGB image (reference odtk/data.py:56-59)
// followed by `transpose(FLIP_LEFT_RIGHT)` (data.py:88) and the per-channel `((v / 255) - mean) / std` (data.py:111-117, here the
// host-computed [3, 256] table of odtk/data.py: normalisation_table).  Pillow's 8-bit resampling is integer arithmetic:
//     pass(src)[o] = clamp((2^21 + sum_i src[first[o] + i] * k[o][i]) >> 22, 0, 255)            k = round(weight * 2^22)
// horizontally first, ROUNDED TO A BYTE, then vertically on those bytes.  The weights are computed on the host in double
// (odtk/data.py: resample_weights) and arrive as tables; this file only multiplies and adds integers, so nothing here depends on
// the device's floating point.  A pass whose source and target length agree is skipped by Pillow; here it runs with the single
// weight 2^22, and (2^21 + v * 2^22) >> 22 == v for every byte v: the same bits without a second code path.
//
// Shape: one workgroup = one tile of 16 rows x 64 pixels of one image of the padded batch.
//   1. the source rows the tile's 16 output rows draw on (their vertical footprint) are resampled HORIZONTALLY for the tile's 64
//      columns into LDS, 3 bytes per pixel -- the byte intermediate never goes through global memory.  A mirrored image reads the
//      resized column out_w - 1 - x: the flip comes after the resize, as in data.py (the fixed-point weights are not symmetric).
//   2. the VERTICAL pass runs out of LDS along W * 3: a row's weight is the same for every pixel and channel of the row, so a
//      thread takes 16 bytes' worth of consecutive output elements (4 fp32 / 8 bf16 or fp16), reads their 4 / 8 source bytes of
//      every footprint row with one LDS load, and ends in one 16-byte store.
//   3. footprints beyond kPreLdsRows rows (down-scaling by more than ~2) are walked in chunks of that many rows; the vertical sum
//      is an integer sum, so accumulating it across chunks is exact.
// Elements outside an image's out_h x out_w are +0.0 (all bits zero), like F.pad of the normalised image.
//
// BYTES = true is the same tile code as pass A of the augmentation chain (augment.hpp): the resized R G B bytes themselves go to
// the image's slot of the workspace, rows 3 * out_width bytes apart, instead of through the table; nothing is padded.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/odtk_hip.h"
#include "prefilter.hpp"   // vuint4

namespace odtk {

constexpr int kPreTileW = 64;                    // output pixels per tile row
constexpr int kPreTileH = 16;                    // output rows per tile
constexpr int kPreRowBytes = kPreTileW * 3;      // one LDS row: the tile's columns of one horizontally resampled source row
constexpr int kPreLdsRows = 40;                  // rows per chunk of the vertical footprint (16 rows of an up-scale need <= 18)
constexpr int kPreMaxImages = 64;                // descriptors per launch: they travel by value in the kernel arguments
constexpr int kPreUnit = 1 << 22;                // the weight 1.0 in Pillow's fixed point (PRECISION_BITS = 32 - 8 - 2)

struct PreArgs {
  const uint8_t *src;
  const int32_t *tables;
  const void *norm;        // [3][256] of the output's element type
  void *out;               // [batch, height, width, 3]
  int32_t height, width;
  int32_t first;           // batch index of images[0]
  int32_t vector_rows;     // every output row is a whole number of 16-byte vectors and starts on one
  uint8_t *bytes;          // BYTES only: slot of image b = bytes + b * slot, 16-byte aligned
  unsigned long long *sums;  // BYTES only: one per image of the batch, zeroed here for the sum of L (augment.hpp)
  uint64_t slot;
  odtk_image_t images[kPreMaxImages];
};

__device__ __forceinline__ int32_t pre_byte(int32_t acc) {
  const int32_t v = acc >> 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// first source index and tap count of output index `o` of one axis; `table` < 0: the pass is skipped (one tap, weight 2^22).
// Clamped to the source length, so a damaged table cannot send a load outside the image.
__device__ __forceinline__ void pre_bounds(const int32_t *tables, int32_t table, int32_t taps, int32_t in_size, int32_t o, int32_t *first,
                                           int32_t *n) {
  if (table < 0) {
    *first = o < in_size ? o : in_size - 1;
    *n = 1;
    return;
  }
  int32_t f = tables[table + 2 * o], c = tables[table + 2 * o + 1];
  f = f < 0 ? 0 : (f > in_size - 1 ? in_size - 1 : f);
  c = c < 0 ? 0 : (c > taps ? taps : c);
  *first = f;
  *n = c > in_size - f ? in_size - f : c;
}

template <int ES, bool BYTES = false>   // bytes per output element: 4 (fp32) or 2 (bf16 / fp16 -- the table holds the bits, nothing is
__global__ __launch_bounds__(256) void preprocess_images_kernel(const PreArgs a) {   // converted here); BYTES: 4, see above
  constexpr int EPT = 16 / ES;                                    // elements per 16-byte store
  constexpr int VPR = kPreRowBytes / EPT;                         // vectors per tile row
  constexpr int ITEMS = (kPreTileH * VPR + 255) / 256;            // vectors per thread
  using elem_t = std::conditional_t<ES == 4, uint32_t, uint16_t>;
  using word_t = std::conditional_t<ES == 4, uint32_t, uint64_t>; // EPT source bytes
  __shared__ __attribute__((aligned(16))) uint8_t rows[kPreLdsRows * kPreRowBytes];
  __shared__ elem_t norm[3 * 256];

  const int tid = static_cast<int>(threadIdx.x);
  const odtk_image_t &im = a.images[blockIdx.z];
  const int32_t ow = im.out_width, oh = im.out_height;
  const int32_t x0 = static_cast<int32_t>(blockIdx.x) * kPreTileW, y0 = static_cast<int32_t>(blockIdx.y) * kPreTileH;
  const bool live = x0 < ow && y0 < oh;                           // (workgroup-uniform) otherwise the tile is padding only
  const int32_t *tables = a.tables;

  if constexpr (BYTES) {
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) a.sums[a.first + blockIdx.z] = 0ull;
  } else {
    for (int i = tid; i < 3 * 256; i += 256) norm[i] = static_cast<const elem_t *>(a.norm)[i];
  }

  // this thread's vectors: tile row, first element in the row, vertical taps
  int32_t acc[ITEMS][EPT], ymin[ITEMS], yn[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int item = tid + it * 256;
    const int32_t y = y0 + item / VPR;
    ymin[it] = 0;
    yn[it] = 0;
    if (live && item < kPreTileH * VPR && y < oh) pre_bounds(tables, im.y_table, im.y_taps, im.src_height, y, &ymin[it], &yn[it]);
#pragma unroll
    for (int k = 0; k < EPT; ++k) acc[it][k] = 1 << 21;
  }

  // vertical footprint of the tile (first / count are non-decreasing in the output index)
  int32_t r0 = 0, r1 = 0;
  if (live) {
    int32_t f, n;
    pre_bounds(tables, im.y_table, im.y_taps, im.src_height, y0, &r0, &n);
    const int32_t yl = (y0 + kPreTileH < oh ? y0 + kPreTileH : oh) - 1;
    pre_bounds(tables, im.y_table, im.y_taps, im.src_height, yl, &f, &n);
    r1 = f + n;
  }

  // this thread's column of the horizontal pass
  const int32_t col = tid & (kPreTileW - 1);
  int32_t xmin = 0, xn = 0;
  const int32_t *kx = nullptr;
  if (live && x0 + col < ow) {
    const int32_t rx = im.mirror ? ow - 1 - (x0 + col) : x0 + col;
    pre_bounds(tables, im.x_table, im.x_taps, im.src_width, rx, &xmin, &xn);
    if (im.x_table >= 0) kx = tables + im.x_table + 2 * ow + rx * im.x_taps;
  }
  const uint8_t *image = a.src + im.src_offset;

  for (int32_t c0 = r0; c0 < r1; c0 += kPreLdsRows) {
    const int32_t cn = r1 - c0 < kPreLdsRows ? r1 - c0 : kPreLdsRows;
    __syncthreads();                                              // the previous chunk has been consumed (first trip: norm[] is written)
    if (xn > 0) {
      for (int32_t r = tid >> 6; r < cn; r += 256 / kPreTileW) {
        const uint8_t *p = image + static_cast<uint32_t>(c0 + r) * static_cast<uint32_t>(im.src_pitch) + static_cast<uint32_t>(xmin) * 3u;
        int32_t s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
        for (int32_t i = 0; i < xn; ++i) {
          const int32_t k = kx ? kx[i] : kPreUnit;
          s0 += static_cast<int32_t>(p[3 * i]) * k;
          s1 += static_cast<int32_t>(p[3 * i + 1]) * k;
          s2 += static_cast<int32_t>(p[3 * i + 2]) * k;
        }
        uint8_t *q = rows + r * kPreRowBytes + col * 3;
        q[0] = static_cast<uint8_t>(pre_byte(s0));
        q[1] = static_cast<uint8_t>(pre_byte(s1));
        q[2] = static_cast<uint8_t>(pre_byte(s2));
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int item = tid + it * 256;
      const int32_t y = y0 + item / VPR, e0 = (item % VPR) * EPT;
      const int32_t lo = ymin[it] > c0 ? ymin[it] : c0;
      const int32_t hi = ymin[it] + yn[it] < c0 + cn ? ymin[it] + yn[it] : c0 + cn;
      const int32_t *ky = im.y_table >= 0 ? tables + im.y_table + 2 * oh + y * im.y_taps - ymin[it] : nullptr;
      for (int32_t i = lo; i < hi; ++i) {
        const int32_t k = ky ? ky[i] : kPreUnit;
        const word_t w = *reinterpret_cast<const word_t *>(rows + (i - c0) * kPreRowBytes + e0);
#pragma unroll
        for (int e = 0; e < EPT; ++e) acc[it][e] += static_cast<int32_t>((w >> (8 * e)) & 0xffu) * k;
      }
    }
  }
  __syncthreads();                                                // norm[] is written (a tile of padding never entered the loop)

  if constexpr (BYTES) {
    static_assert(ES == 4 && EPT == 4, "four bytes per item");
    uint8_t *slot = a.bytes + static_cast<size_t>(a.first + blockIdx.z) * a.slot;
    const int32_t row_bytes = ow * 3;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int item = tid + it * 256;
      const int32_t y = y0 + item / VPR, first = x0 * 3 + (item % VPR) * EPT;
      if (item >= kPreTileH * VPR || y >= oh || first >= row_bytes) continue;
      uint8_t *dst = slot + static_cast<size_t>(y) * row_bytes + first;
      uint32_t w = 0;
#pragma unroll
      for (int e = 0; e < EPT; ++e) w |= static_cast<uint32_t>(pre_byte(acc[it][e])) << (8 * e);
      if ((row_bytes & 3) == 0) {                                   // rows start on a word, and so does `first`
        *reinterpret_cast<uint32_t *>(dst) = w;
      } else {
#pragma unroll
        for (int e = 0; e < EPT; ++e)
          if (first + e < row_bytes) dst[e] = static_cast<uint8_t>(w >> (8 * e));
      }
    }
    return;
  }
  elem_t *out = static_cast<elem_t *>(a.out) + static_cast<size_t>(a.first + blockIdx.z) * a.height * a.width * 3;
  const int32_t row_elems = a.width * 3;
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int item = tid + it * 256;
    const int32_t y = y0 + item / VPR, e0 = (item % VPR) * EPT;
    if (item >= kPreTileH * VPR || y >= a.height) continue;
    const uint32_t p0 = static_cast<uint32_t>(e0) / 3u, ch0 = static_cast<uint32_t>(e0) - 3u * p0;
    elem_t v[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const uint32_t t = ch0 + e;
      const int32_t px = x0 + static_cast<int32_t>(p0 + t / 3u);
      v[e] = (y < oh && px < ow) ? norm[(t % 3u) * 256u + static_cast<uint32_t>(pre_byte(acc[it][e]))] : elem_t(0);
    }
    const int32_t first = x0 * 3 + e0;                            // element of the output row
    elem_t *dst = out + static_cast<size_t>(y) * row_elems + first;
    if (a.vector_rows) {
      if (first < row_elems) {
        vuint4 o;
        if constexpr (ES == 4) {
          o = vuint4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = static_cast<uint32_t>(v[2 * e]) | (static_cast<uint32_t>(v[2 * e + 1]) << 16);
        }
        *reinterpret_cast<vuint4 *>(dst) = o;
      }
    } else {
#pragma unroll
      for (int e = 0; e < EPT; ++e)
        if (first + e < row_elems) dst[e] = v[e];
    }
  }
}

}  // namespace odtk
