// tower_conv_layout.hpp -- the index functions of the head towers' 3x3 convolution kernel (tower_conv.hpp), callable on the host:
// tests/test_tower_conv_layout.py compiles them into a stand-alone program and checks them exhaustively without a GPU.
//
// The convolution is a GEMM with a gathered operand: rows = 256 consecutive pixels of the flattened N*H*W run, columns = the 256
// output channels, K = 9 taps x 256 input channels, walked in 36 K-tiles of 64: K-tile kt is tap kt / 4, channels (kt % 4) * 64.
// Both operand tiles are [256 rows][64 k] 16-bit = 256 rows of 128 bytes = 8 chunks of 16 bytes each, 32 KiB.
//
// They reach the LDS by LDS-DMA (global_load_lds_dwordx4), whose destination is wave-uniform base + lane * 16: the image is linear
// in the order the lanes are numbered.  Piece (i, tid), i < 4, of the 512 threads lands at byte (i * 512 + tid) * 16, i.e. in row
// i * 64 + tid / 8 at PHYSICAL chunk tid % 8: one wave instruction fills 8 whole rows, and reads 8 whole 128-byte lines.
// The swizzle lives on the source address and on the ds_read address (the same involution on both sides): physical chunk =
// logical chunk ^ ((row / 2) % 8).  A ds_read_b128 of an MFMA 16x16x32 fragment (lane l: row l % 16, chunk 4 kk + l / 16) then
// finds the 16 lanes of each of the hardware's lane groups on 16 different 16-byte slots of the 256-byte bank row.
#pragma once

#include "fastdiv.hpp"

namespace odtk {
namespace tower {

constexpr uint32_t kThreads = 512;                  // 8 waves, 2 (pixels) x 4 (channels): 128 pixels x 64 channels per wave
constexpr uint32_t kTilePixels = 256, kChannels = 256, kBK = 64, kTaps = 9;
constexpr uint32_t kKTiles = kTaps * kChannels / kBK;                     // 36
constexpr uint32_t kRowBytes = kBK * 2, kOperandBytes = 256 * kRowBytes;   // 128, 32 KiB
constexpr uint32_t kBufferBytes = 2 * kOperandBytes;                       // pixels' tile, then the weights' tile
constexpr uint32_t kLdsBytes = 2 * kBufferBytes;                           // two buffers: 128 KiB (= the epilogue's 256 x 256 x 2)
constexpr uint32_t kPixelBytes = kChannels * 2;                            // one pixel of x or y: 512

// the swizzle: an involution on the chunk index of a row
ODTK_HD uint32_t swizzle(uint32_t row, uint32_t chunk) { return chunk ^ ((row >> 1) & 7u); }

// LDS-DMA piece (i, tid): where it lands in the operand's image, which row it belongs to, and which LOGICAL chunk of that row's
// 128 bytes its source is (the physical chunk is tid % 8)
ODTK_HD uint32_t piece_dst(uint32_t i, uint32_t tid) { return (i * kThreads + tid) * 16u; }
ODTK_HD uint32_t piece_wave_base(uint32_t i, uint32_t wave) { return (i * kThreads + wave * 64u) * 16u; }   // + lane * 16 by the hardware
ODTK_HD uint32_t piece_row(uint32_t i, uint32_t tid) { return i * 64u + (tid >> 3); }
ODTK_HD uint32_t piece_chunk(uint32_t tid) { return swizzle(tid >> 3, tid & 7u); }    // (i * 64 does not reach bits 1..3 of the row)

// ds_read_b128 of lane l for the 16-row block `block` of an operand image and k-step kk (32 k each): row, logical chunk, address
ODTK_HD uint32_t frag_row(uint32_t block, uint32_t lane) { return block * 16u + (lane & 15u); }
ODTK_HD uint32_t frag_chunk(uint32_t kk, uint32_t lane) { return kk * 4u + (lane >> 4); }
ODTK_HD uint32_t frag_addr(uint32_t block, uint32_t kk, uint32_t lane) {
  const uint32_t row = frag_row(block, lane);
  return row * kRowBytes + (swizzle(row, frag_chunk(kk, lane)) << 4);
}

// The same for the 32x32x16 MFMA ("form 1"): lane l holds row l % 32 and 8 consecutive k chosen by its half h = l / 32.  A K-tile
// is four k-steps of 16; which 8-element chunk of the tile's 64 a lane feeds to step s follows the convolution library's
// 256 x 256 x 32 instance, so that every fp32 sum is taken over the same k in the same instruction slot as there: within each
// 32-deep block the halves start 16 apart -- step s = 2 blk + r reads chunk 4 blk + 2 h + r, i.e. one MFMA sums k {0..7, 16..23}
// of the block and the next {8..15, 24..31}.  (Form 0, above, sums 32 consecutive k per MFMA.)
ODTK_HD uint32_t frag32_row(uint32_t block, uint32_t lane) { return block * 32u + (lane & 31u); }
ODTK_HD uint32_t frag32_chunk(uint32_t step, uint32_t lane) { return (step >> 1) * 4u + 2u * (lane >> 5) + (step & 1u); }
ODTK_HD uint32_t frag32_addr(uint32_t block, uint32_t step, uint32_t lane) {
  const uint32_t row = frag32_row(block, lane);
  return row * kRowBytes + (swizzle(row, frag32_chunk(step, lane)) << 4);
}

// K-tile -> tap and first channel; tap t = 3 kh + kw reads pixel (y + kh - 1, x + kw - 1)
ODTK_HD uint32_t ktile_tap(uint32_t kt) { return kt >> 2; }
ODTK_HD uint32_t ktile_channel(uint32_t kt) { return (kt & 3u) * kBK; }
ODTK_HD int32_t tap_pixel_offset(uint32_t tap, uint32_t width) {
  return (static_cast<int32_t>(tap / 3u) - 1) * static_cast<int32_t>(width) + (static_cast<int32_t>(tap % 3u) - 1);
}

// flat pixel p < n * h * w -> (image, y, x)
struct Pixel { uint32_t n, y, x; };
ODTK_HD Pixel pixel_of(uint32_t p, const FastDiv &by_w, const FastDiv &by_hw) {
  Pixel q;
  uint32_t rem;
  q.n = fastdivmod(p, by_hw, &rem);
  q.y = fastdivmod(rem, by_w, &q.x);
  return q;
}

// bit t set: tap t of the pixel lies inside ITS image (a tile crosses row ends and image ends: the neighbour in memory is then
// another row's or another image's pixel and must read as zero)
ODTK_HD uint32_t tap_mask(uint32_t y, uint32_t x, uint32_t height, uint32_t width) {
  const uint32_t rows = (y > 0u ? 1u : 0u) | 2u | (y + 1u < height ? 4u : 0u);      // bit kh
  const uint32_t cols = (x > 0u ? 1u : 0u) | 2u | (x + 1u < width ? 4u : 0u);       // bit kw
  uint32_t mask = 0u;
  for (uint32_t kh = 0; kh < 3u; ++kh)
    if ((rows >> kh) & 1u) mask |= cols << (3u * kh);
  return mask;
}

// The epilogue's image of the rounded tile: [256 pixels][32 chunks of 8 channels]; the chunk's low three bits are XORed with the
// pixel's, so that the 8-byte fragment writes of 16 pixels (512 bytes apart) spread over the banks.  The row-order read-back is
// linear in the PHYSICAL index: unit q = 512 it + tid is pixel q / 32, physical chunk q % 32.
ODTK_HD uint32_t out_chunk(uint32_t pixel, uint32_t chunk) { return (chunk & ~7u) | ((chunk ^ pixel) & 7u); }   // an involution too
ODTK_HD uint32_t out_addr(uint32_t pixel, uint32_t channel) {     // of the 8 bytes that hold channels channel .. channel + 3 (channel % 4 == 0)
  return pixel * kPixelBytes + out_chunk(pixel, channel >> 3) * 16u + (channel & 4u) * 2u;
}
// accumulator register r of lane l of the 16x16 tile (channel block nb, pixel block mb): the weights are the MFMA's A operand,
// so a lane holds 4 CONSECUTIVE channels of one pixel
ODTK_HD uint32_t acc_channel(uint32_t nb, uint32_t lane, uint32_t reg) { return nb * 16u + (lane >> 4) * 4u + reg; }
ODTK_HD uint32_t acc_pixel(uint32_t mb, uint32_t lane) { return mb * 16u + (lane & 15u); }
// ... and of the 32x32 tile (form 1): register r of lane l is row (r % 4) + 8 (r / 4) + 4 (l / 32), column l % 32
ODTK_HD uint32_t acc32_channel(uint32_t nb, uint32_t lane, uint32_t reg) { return nb * 32u + (reg & 3u) + 8u * (reg >> 2) + 4u * (lane >> 5); }
ODTK_HD uint32_t acc32_pixel(uint32_t mb, uint32_t lane) { return mb * 32u + (lane & 31u); }

}  // namespace tower
}  // namespace odtk
