// augment.hpp -- the training augmentations of the input side on the device (odtk_augment_images; mosaic.hpp adds pass M, the
// mosaic composition, as one more producer of the finished canvas that passes B and C read): quarter turn, flip, brightness,
// contrast, hue and saturation of the RESIZED image, then normalisation by table and zero padding, bit-identical to what the
// dataset workers do with Pillow on the host (odtk/data.py: __getitem__, restated in numpy there: quarter_turn_map, index_map,
// blend, contrast_mean, rgb_to_hsv, hsv_to_rgb -- this file follows those line by line).
//
// A chain of launches per batch, because the contrast's grey level is a mean over the whole image:
//   A. preprocess_images_kernel<4, true> (preprocess.hpp): the Pillow-exact resize, its bytes stored to the image's slot of the
//      workspace; the image's sum is zeroed by its first workgroup.
//   B. augment_luma_sum_kernel (only when an image of the launch has contrast on): sum of L over the canvas of
//      brightness(turn(bytes)); 64-bit integer partial sums, reduced in the wave, through LDS, then one 64-bit atomicAdd per
//      workgroup -- integer sums do not depend on the order.
//   C. augment_images_kernel: every element of [B, H, W, 3].  A thread owns 16 / ES consecutive pixels of one output row = three
//      16-byte vectors; each pixel is gathered through the image's index map, runs the colour chain and is looked up in the table.
//      Under a transposing map (90 / 270 degrees) a row of the canvas is a column of the byte image, and the gather reads it
//      straight from global memory: a variant that first copied the rectangle a workgroup's tile maps into to LDS (consecutive
//      lanes on consecutive bytes, LDS rows an odd number of bytes apart) was measured against it and was no faster
//      (profiles/r08_device_augment_kernel.txt), so it is not here.  Pass B avoids the question: a sum does not care for the
//      order, so under such a map its lanes walk the canvas by columns = along the byte image's rows.
//
// With a free rotation (odtk_augment_images_ex) one more pass runs between A and B:
//   R. augment_rotate_kernel: the finished canvas BYTES of every image of the launch -- the turn through the index map, then
//      `Image.rotate(angle, resample=BILINEAR)` on the turned canvas, then the flip -- go to a second slot of the workspace, and B
//      and C read that slot through the identity map: their code, and so the colour chain's bits, are the ones above.  An image
//      without a rotation is copied through its map (a gather of bytes: the same bytes B and C would have gathered themselves).
//      Pillow's bilinear affine transform is double arithmetic (odtk/data.py: rotate_bilinear is this pass in numpy): the centre
//      of an output pixel goes through the host-computed matrix, a point outside the image is black, otherwise two taps on each
//      of two rows (clamped to the image; the lower row only if it exists) are blended by the fractions and TRUNCATED to a byte.
//      A thread owns four consecutive pixels of the canvas (rows are contiguous) = 12 bytes = three aligned 32-bit stores.
//
// The index map is Pillow's affine_fixed: xin = (a2 + a0 x + a1 y) >> 16, yin = (a5 + a3 x + a4 y) >> 16 in 16.16 fixed point, black
// where (xin, yin) lies outside the resized image.  The host computes the six integers (also for the transposes and with the flip
// composed in), so there is one gather path.  Black pixels of the turn are image pixels: they are normalised like any byte 0 and
// count in the mean; the padding beyond the canvas is +0.0.
//
// Floating point: every operation below is a single IEEE operation in the format Pillow's C uses (float32 for the blends and the
// quotients of RGB -> HSV, double where its expressions hold a double literal), never fused: the library is built with
// -ffp-contract=off and the functions say so once more.  fp32 and fp64 division must be the correctly rounded ones (hipcc's
// default).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/odtk_hip.h"
#include "prefilter.hpp"   // vuint4
#include "preprocess.hpp"  // kPreMaxImages

namespace odtk {

constexpr int kAugRows = 16;                     // output rows per workgroup of pass C; 16 threads x (16 / ES) pixels per row
constexpr int kAugSumBlocks = 120;               // workgroups per image of pass B (rows are dealt round robin)

struct AugImage {
  int32_t cw, ch;          // canvas after the turn
  int32_t rw, rh;          // the resized image = what the slot holds, rows 3 * rw bytes apart
  int32_t map[6];
  uint32_t flags;
  float brightness, contrast, saturation;
  uint32_t hue;
};

struct AugArgs {
  const uint8_t *bytes;    // slot of image b = bytes + b * slot
  unsigned long long *sums;
  const void *norm;        // [3][256] of the output's element type
  void *out;               // [batch, height, width, 3]
  uint64_t slot;
  int32_t height, width;
  int32_t first;           // batch index of images[0]
  int32_t vector_rows;
  AugImage images[kPreMaxImages];
};

// `Image.blend(degenerate, image, alpha)` for one byte: float32 product, float32 sum, truncation; clamped first unless 0 <= alpha <= 1
// (then t lies between d and x and needs no clamp).
__device__ __forceinline__ int32_t aug_blend(int32_t d, int32_t x, float alpha, bool clamp) {
#pragma clang fp contract(off)
  const float product = alpha * static_cast<float>(x - d);
  float t = static_cast<float>(d) + product;
  if (clamp) t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
  return static_cast<int32_t>(t);
}

__device__ __forceinline__ int32_t aug_luma(int32_t r, int32_t g, int32_t b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ __forceinline__ int32_t aug_clip8(int32_t v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ int32_t aug_map_x(const AugImage &im, int32_t x, int32_t y) { return (im.map[2] + im.map[0] * x + im.map[1] * y) >> 16; }
__device__ __forceinline__ int32_t aug_map_y(const AugImage &im, int32_t x, int32_t y) { return (im.map[5] + im.map[3] * x + im.map[4] * y) >> 16; }

// pixel (x, y) of the canvas: the byte image through the index map, then brightness.  Host-checked: the sums fit 32 bits.
__device__ __forceinline__ void aug_fetch(const uint8_t *image, const AugImage &im, int32_t x, int32_t y, int32_t *r, int32_t *g, int32_t *b) {
  const int32_t xin = aug_map_x(im, x, y), yin = aug_map_y(im, x, y);
  *r = *g = *b = 0;
  if (xin >= 0 && xin < im.rw && yin >= 0 && yin < im.rh) {
    const uint8_t *p = image + (static_cast<uint32_t>(yin) * static_cast<uint32_t>(im.rw) + static_cast<uint32_t>(xin)) * 3u;
    *r = p[0];
    *g = p[1];
    *b = p[2];
  }
  if (im.flags & ODTK_AUGMENT_BRIGHTNESS) {
    const bool clamp = !(im.brightness >= 0.0f && im.brightness <= 1.0f);
    *r = aug_blend(0, *r, im.brightness, clamp);
    *g = aug_blend(0, *g, im.brightness, clamp);
    *b = aug_blend(0, *b, im.brightness, clamp);
  }
}

// `_adjust_hue`: Pillow's rgb2hsv_row, hue + shift (wrapping byte), hsv2rgb_row.
__device__ __forceinline__ void aug_hue(int32_t *pr, int32_t *pg, int32_t *pb, int32_t shift) {
#pragma clang fp contract(off)
  const int32_t r = *pr, g = *pg, b = *pb;
  const int32_t maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  if (maxc == minc) return;                                       // h = s = 0: grey stays grey whatever the shift
  const float cr = static_cast<float>(maxc - minc);
  const float s = cr / static_cast<float>(maxc);
  const float rc = static_cast<float>(maxc - r) / cr, gc = static_cast<float>(maxc - g) / cr, bc = static_cast<float>(maxc - b) / cr;
  float h;
  if (r == maxc)
    h = static_cast<float>(static_cast<double>(bc) - static_cast<double>(gc));
  else if (g == maxc)
    h = static_cast<float>(2.0 + static_cast<double>(rc) - static_cast<double>(bc));
  else
    h = static_cast<float>(4.0 + static_cast<double>(gc) - static_cast<double>(rc));
  double turn = static_cast<double>(h) / 6.0 + 1.0;               // in (0.8, 1.9): fmod(turn, 1) is an exact subtraction
  if (turn >= 1.0) turn = turn - 1.0;
  h = static_cast<float>(turn);
  const int32_t hue = (aug_clip8(static_cast<int32_t>(static_cast<double>(h) * 255.0)) + shift) & 255;
  const int32_t sat = aug_clip8(static_cast<int32_t>(static_cast<double>(s) * 255.0));
  if (sat == 0) {
    *pr = *pg = *pb = maxc;
    return;
  }
  const double v = static_cast<double>(maxc);
  const double hh = static_cast<double>(hue) * 6.0 / 255.0;
  const double fl = floor(hh);
  const double f = hh - fl;
  const double fs = static_cast<double>(sat) / 255.0;
  const int32_t p = aug_clip8(static_cast<int32_t>(rint(v * (1.0 - fs))));
  const int32_t q = aug_clip8(static_cast<int32_t>(rint(v * (1.0 - fs * f))));
  const int32_t t = aug_clip8(static_cast<int32_t>(rint(v * (1.0 - fs * (1.0 - f)))));
  switch (static_cast<int32_t>(fl) % 6) {
    case 0: *pr = maxc, *pg = t, *pb = p; break;
    case 1: *pr = q, *pg = maxc, *pb = p; break;
    case 2: *pr = p, *pg = maxc, *pb = t; break;
    case 3: *pr = p, *pg = q, *pb = maxc; break;
    case 4: *pr = t, *pg = p, *pb = maxc; break;
    default: *pr = maxc, *pg = p, *pb = q; break;
  }
}

constexpr int kRotMaxImages = 32;                // descriptors per launch of pass R (96 bytes each, by value in the kernel arguments)
constexpr int kRotPixels = 4;                    // consecutive pixels per thread of pass R

struct RotImage {
  double m[6];             // odtk_rotation_t.matrix
  int32_t cw, ch;          // canvas after the turn = what the rotation works on and what is written
  int32_t rw, rh;          // the resized image = what the source slot holds
  int32_t map[6];          // the turn (enabled) or the turn and the flip (not enabled)
  int32_t enabled, flip;
};

struct RotArgs {
  const uint8_t *bytes;    // resized bytes of image b = bytes + b * slot
  uint8_t *canvas;         // finished canvas bytes of image b = canvas + b * slot, rows 3 * cw bytes apart
  uint64_t slot;
  int32_t first;           // batch index of images[0]
  int32_t pad_;
  RotImage images[kRotMaxImages];
};

// pixel (x, y) of the TURNED canvas, 0 <= x < cw, 0 <= y < ch: the byte image through the index map, black outside it.
__device__ __forceinline__ void rot_tap(const uint8_t *image, const RotImage &im, int32_t x, int32_t y, double *r, double *g, double *b) {
  const int32_t xin = (im.map[2] + im.map[0] * x + im.map[1] * y) >> 16, yin = (im.map[5] + im.map[3] * x + im.map[4] * y) >> 16;
  *r = *g = *b = 0.0;
  if (xin >= 0 && xin < im.rw && yin >= 0 && yin < im.rh) {
    const uint8_t *p = image + (static_cast<uint32_t>(yin) * static_cast<uint32_t>(im.rw) + static_cast<uint32_t>(xin)) * 3u;
    *r = static_cast<double>(p[0]);
    *g = static_cast<double>(p[1]);
    *b = static_cast<double>(p[2]);
  }
}

// Pillow's BILINEAR(v, a, b, d): v = a + (b - a) * d, three roundings.
__device__ __forceinline__ double rot_lerp(double a, double b, double d) {
#pragma clang fp contract(off)
  const double diff = b - a;
  const double product = diff * d;
  return a + product;
}

// Pixel (x, y) of the rotated canvas -> 0x00BBGGRR.  Pillow's affine_transform + bilinear_filter32RGB, in double, never fused.
__device__ __forceinline__ uint32_t rot_pixel(const uint8_t *image, const RotImage &im, int32_t x, int32_t y) {
#pragma clang fp contract(off)
  const double xc = static_cast<double>(x) + 0.5, yc = static_cast<double>(y) + 0.5;
  const double ax = im.m[0] * xc, bx = im.m[1] * yc, ay = im.m[3] * xc, by = im.m[4] * yc;
  const double sx = ax + bx, sy = ay + by;
  double xin = sx + im.m[2], yin = sy + im.m[5];
  if (!(xin >= 0.0 && xin < static_cast<double>(im.cw) && yin >= 0.0 && yin < static_cast<double>(im.ch))) return 0u;
  xin = xin - 0.5;
  yin = yin - 0.5;
  const double fx = floor(xin), fy = floor(yin);
  const double dx = xin - fx, dy = yin - fy;
  const int32_t col = static_cast<int32_t>(fx), row = static_cast<int32_t>(fy);          // -1 <= col < cw, -1 <= row < ch
  const int32_t x0 = col < 0 ? 0 : col, x1 = col + 1 > im.cw - 1 ? im.cw - 1 : col + 1, y0 = row < 0 ? 0 : row;
  double r0, g0, b0, r1, g1, b1;
  rot_tap(image, im, x0, y0, &r0, &g0, &b0);
  rot_tap(image, im, x1, y0, &r1, &g1, &b1);
  const double vr = rot_lerp(r0, r1, dx), vg = rot_lerp(g0, g1, dx), vb = rot_lerp(b0, b1, dx);
  double wr = vr, wg = vg, wb = vb;
  if (row + 1 < im.ch) {                                          // (row + 1 >= 0 always)
    rot_tap(image, im, x0, row + 1, &r0, &g0, &b0);
    rot_tap(image, im, x1, row + 1, &r1, &g1, &b1);
    wr = rot_lerp(r0, r1, dx);
    wg = rot_lerp(g0, g1, dx);
    wb = rot_lerp(b0, b1, dx);
  }
  const uint32_t r = static_cast<uint32_t>(static_cast<int32_t>(rot_lerp(vr, wr, dy))) & 255u;
  const uint32_t g = static_cast<uint32_t>(static_cast<int32_t>(rot_lerp(vg, wg, dy))) & 255u;
  const uint32_t b = static_cast<uint32_t>(static_cast<int32_t>(rot_lerp(vb, wb, dy))) & 255u;
  return r | (g << 8) | (b << 16);
}

// Pass R.  grid = (ceil(largest canvas of the launch in pixels / (256 * kRotPixels)), 1, images of the launch).
__global__ __launch_bounds__(256) void augment_rotate_kernel(const RotArgs a) {
  const RotImage &im = a.images[blockIdx.z];
  const uint32_t pixels = static_cast<uint32_t>(im.cw) * static_cast<uint32_t>(im.ch);
  const uint32_t p0 = (blockIdx.x * 256u + threadIdx.x) * kRotPixels;
  if (p0 >= pixels) return;
  const uint8_t *image = a.bytes + static_cast<size_t>(a.first + blockIdx.z) * a.slot;
  uint8_t *dst = a.canvas + static_cast<size_t>(a.first + blockIdx.z) * a.slot + static_cast<size_t>(p0) * 3u;
  int32_t y = static_cast<int32_t>(p0 / static_cast<uint32_t>(im.cw)), x = static_cast<int32_t>(p0 - static_cast<uint32_t>(y) * static_cast<uint32_t>(im.cw));
  uint32_t v[kRotPixels];
#pragma unroll
  for (int p = 0; p < kRotPixels; ++p) {
    v[p] = 0u;
    if (p0 + p < pixels) {
      if (im.enabled) {
        v[p] = rot_pixel(image, im, im.flip ? im.cw - 1 - x : x, y);
      } else {
        double r, g, b;
        rot_tap(image, im, x, y, &r, &g, &b);
        v[p] = static_cast<uint32_t>(r) | (static_cast<uint32_t>(g) << 8) | (static_cast<uint32_t>(b) << 16);
      }
    }
    if (++x == im.cw) x = 0, ++y;
  }
  static_assert(kRotPixels == 4, "12 bytes = three words");
  if (p0 + kRotPixels <= pixels) {                                // slots are 16-byte aligned and p0 * 3 is a multiple of 12
    uint32_t *w = reinterpret_cast<uint32_t *>(dst);
    w[0] = v[0] | (v[1] << 24);
    w[1] = (v[1] >> 8) | (v[2] << 16);
    w[2] = (v[2] >> 16) | (v[3] << 8);
  } else {
#pragma unroll
    for (int p = 0; p < kRotPixels; ++p)
      if (p0 + p < pixels) {
        dst[3 * p] = static_cast<uint8_t>(v[p]);
        dst[3 * p + 1] = static_cast<uint8_t>(v[p] >> 8);
        dst[3 * p + 2] = static_cast<uint8_t>(v[p] >> 16);
      }
  }
}

// Pass B.  grid = (kAugSumBlocks, 1, images of the launch).
__global__ __launch_bounds__(256) void augment_luma_sum_kernel(const AugArgs a) {
  __shared__ unsigned long long partial[4];
  const AugImage &im = a.images[blockIdx.z];
  if (!(im.flags & ODTK_AUGMENT_CONTRAST)) return;                // (workgroup-uniform)
  const int tid = static_cast<int>(threadIdx.x);
  const uint8_t *image = a.bytes + static_cast<size_t>(a.first + blockIdx.z) * a.slot;
  unsigned long long sum = 0;
  const bool transposing = im.map[0] == 0;                        // the source column depends on y alone: lanes walk y
  const int32_t lines = transposing ? im.cw : im.ch, length = transposing ? im.ch : im.cw;
  for (int32_t line = static_cast<int32_t>(blockIdx.x); line < lines; line += static_cast<int32_t>(gridDim.x)) {
    uint32_t part = 0;                                            // <= 255 * ceil(length / 256) < 2^32
    for (int32_t at = tid; at < length; at += 256) {
      int32_t r, g, b;
      aug_fetch(image, im, transposing ? line : at, transposing ? at : line, &r, &g, &b);
      part += static_cast<uint32_t>(aug_luma(r, g, b));
    }
    sum += part;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if ((tid & 63) == 0) partial[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    const unsigned long long total = partial[0] + partial[1] + partial[2] + partial[3];
    if (total) atomicAdd(a.sums + a.first + blockIdx.z, total);
  }
}

// Pass C.  grid = (ceil(width / (16 * PPT)), ceil(height / kAugRows), images of the launch).
template <int ES>
__global__ __launch_bounds__(256) void augment_images_kernel(const AugArgs a) {
  constexpr int PPT = 16 / ES;                                    // pixels per thread: 3 * PPT elements = three 16-byte vectors
  using elem_t = std::conditional_t<ES == 4, uint32_t, uint16_t>;
  constexpr int TW = 16 * PPT;                                    // pixels per row of the workgroup's tile
  __shared__ elem_t norm[3 * 256];
  const int tid = static_cast<int>(threadIdx.x);
  for (int i = tid; i < 3 * 256; i += 256) norm[i] = static_cast<const elem_t *>(a.norm)[i];
  __syncthreads();

  const AugImage &im = a.images[blockIdx.z];
  const uint8_t *image = a.bytes + static_cast<size_t>(a.first + blockIdx.z) * a.slot;
  const int32_t x0 = static_cast<int32_t>(blockIdx.x) * TW + (tid & 15) * PPT;
  const int32_t y = static_cast<int32_t>(blockIdx.y) * kAugRows + (tid >> 4);
  if (y >= a.height || x0 >= a.width) return;

  // the grey level of the contrast: int(sum / count + 0.5) of the host (the quotient and the sum rounded to double) equals
  // (2 sum + count) / (2 count) in integers.  If sum / count < k + 1/2 it is below by at least 1 / (2 count) > 2^-31 (count =
  // cw * ch < 2^31 / 3 is checked on the host), while a double near 255 is spaced 2^-45: neither rounding can reach k + 1/2, resp.
  // k + 1; if sum / count >= k + 1/2 rounding keeps it there (k + 1/2 is a double).
  int32_t grey = 0;
  if (im.flags & ODTK_AUGMENT_CONTRAST) {
    const unsigned long long count = static_cast<unsigned long long>(im.cw) * static_cast<unsigned long long>(im.ch);
    grey = static_cast<int32_t>((2ull * a.sums[a.first + blockIdx.z] + count) / (2ull * count));
  }
  const bool clamp_c = !(im.contrast >= 0.0f && im.contrast <= 1.0f), clamp_s = !(im.saturation >= 0.0f && im.saturation <= 1.0f);

  elem_t v[3 * PPT];
#pragma unroll
  for (int p = 0; p < PPT; ++p) {
    const int32_t x = x0 + p;
    if (y < im.ch && x < im.cw) {
      int32_t r, g, b;
      aug_fetch(image, im, x, y, &r, &g, &b);
      if (im.flags & ODTK_AUGMENT_CONTRAST) {
        r = aug_blend(grey, r, im.contrast, clamp_c);
        g = aug_blend(grey, g, im.contrast, clamp_c);
        b = aug_blend(grey, b, im.contrast, clamp_c);
      }
      if (im.flags & ODTK_AUGMENT_HUE) aug_hue(&r, &g, &b, static_cast<int32_t>(im.hue));
      if (im.flags & ODTK_AUGMENT_SATURATION) {
        const int32_t l = aug_luma(r, g, b);
        r = aug_blend(l, r, im.saturation, clamp_s);
        g = aug_blend(l, g, im.saturation, clamp_s);
        b = aug_blend(l, b, im.saturation, clamp_s);
      }
      v[3 * p] = norm[r];
      v[3 * p + 1] = norm[256 + g];
      v[3 * p + 2] = norm[512 + b];
    } else {
      v[3 * p] = v[3 * p + 1] = v[3 * p + 2] = elem_t(0);
    }
  }

  elem_t *dst = static_cast<elem_t *>(a.out) + (static_cast<size_t>(a.first + blockIdx.z) * a.height + y) * a.width * 3 + static_cast<size_t>(x0) * 3;
  if (a.vector_rows) {                                            // width is a multiple of PPT: the thread's pixels all exist
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      vuint4 o;
      if constexpr (ES == 4) {
        o = vuint4{v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = static_cast<uint32_t>(v[8 * k + 2 * e]) | (static_cast<uint32_t>(v[8 * k + 2 * e + 1]) << 16);
      }
      reinterpret_cast<vuint4 *>(dst)[k] = o;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 3 * PPT; ++e)
      if (x0 + e / 3 < a.width) dst[e] = v[e];
  }
}

}  // namespace odtk
