// tower_conv.hpp -- the 3x3 convolutions of the head towers as an implicit-GEMM MFMA kernel:
//     y[p][n] = rne_T(act(fp32(rne_T(fp32 sum_{tap, c} x[p + tap][c] * w[n][tap][c])) + fp32(bias[n])))     c, n < 256
// for NHWC 16-bit activations, stride 1, padding 1 (taps outside the pixel's image read as zero), bias in the activation dtype:
// the two roundings of the convolution library's route (include/odtk_conv.h), a NaN accumulator handed on as odtk_bias_act does.
// No reference equivalent as a kernel (the reference runs nn.Conv2d + ReLU: odtk/model.py:57-62).
//
// One workgroup owns 256 consecutive pixels of the flattened N*H*W run and all 256 output channels; 8 waves as 2 (pixels) x 4
// (channels), 128 x 64 outputs per wave in 32 accumulators of v_mfma_f32_16x16x32.  K = 9 taps x 256 channels runs in 36 K-tiles of
// 64 in a fixed order (no split-K, no atomics: the same input gives the same bits on every launch).  The weights as the engine
// stores them, [c_out][kh][kw][c_in], are the K-contiguous second operand as they are; the pixels' operand is gathered: the
// source of each 16-byte piece is the pixel's base + the tap's offset + the channel offset, or one 16-byte block of zeros where
// the tap is outside the image or the pixel beyond the run -- chosen from a 9-bit mask per piece computed once in the prologue.
// No padded copy, no bounds branch in the loop, nothing to allocate.
//
// Both operands go global -> LDS by LDS-DMA into two 64 KiB buffers (the structure: stage tile kt + 1, compute tile kt, wait for
// every outstanding load, one workgroup barrier per K-tile: a staged buffer is never read before the wait + barrier that retire
// it, and never restaged before a barrier every reader has passed).  The index functions -- LDS image, swizzle, fragment
// addresses, tap mask -- are in tower_conv_layout.hpp, which the host can call (tests/test_tower_conv_layout.py).
// The weights are the MFMA's A operand (rows = channels) and the pixels its B operand (columns), so a lane's 4 accumulator
// registers are 4 consecutive channels of one pixel: 8 bytes after the first rounding.  The rounded tile crosses the LDS
// (128 KiB, free after the loop) and leaves in row order: every store instruction covers two whole pixels = eight 128-byte lines.
#pragma once

#include "common.hpp"
#include "seam.hpp"                // seam_pack2 / seam_unpack, the vector types
#include "tower_conv_layout.hpp"

namespace odtk {

typedef float tower_f32x4 __attribute__((ext_vector_type(4)));

// what a masked piece reads instead of a pixel
__device__ __attribute__((aligned(16))) uint32_t tower_zero_block[4];

template <typename T>
__device__ __forceinline__ tower_f32x4 tower_mfma(vuint4 a, vuint4 b, tower_f32x4 c) {
  if constexpr (std::is_same_v<T, BF16>)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(seam_bf16x8, a), __builtin_bit_cast(seam_bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(seam_f16x8, a), __builtin_bit_cast(seam_f16x8, b), c, 0, 0, 0);
}

template <typename T>
__device__ __forceinline__ seam_f32x16 tower_mfma32(vuint4 a, vuint4 b, seam_f32x16 c) {
  if constexpr (std::is_same_v<T, BF16>)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(seam_bf16x8, a), __builtin_bit_cast(seam_bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(seam_f16x8, a), __builtin_bit_cast(seam_f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ void tower_glds16(const unsigned char *src, unsigned char *lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                   (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}

// kForm: which MFMA sums which k (tower_conv_layout.hpp, "forms"): 1 = v_mfma_f32_32x32x16 with the k grouping of the convolution
// library's 256 x 256 x 32 instance, 0 = v_mfma_f32_16x16x32 over 32 consecutive k.  The forms differ only in the order of the fp32 sums.
// remap: tile ids permuted so that the workgroups that share an L2 (ids equal mod 8) own consecutive tiles, whose halo rows overlap
template <typename T, bool kRelu, int kForm>
__global__ __launch_bounds__(tower::kThreads) void tower_conv3x3_kernel(const unsigned char *__restrict__ x, const unsigned char *__restrict__ w,
                                                                        const uint16_t *__restrict__ bias, unsigned char *__restrict__ y,
                                                                        uint32_t m, uint32_t height, uint32_t width, FastDiv by_w,
                                                                        FastDiv by_hw, uint32_t remap) {
  using namespace tower;
  extern __shared__ __attribute__((aligned(1024))) unsigned char tower_lds[];      // the ONLY LDS object of the kernel

  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t tile = blockIdx.x;
  if (remap) {                                                // bijective for every grid size
    const uint32_t nwg = gridDim.x, q = nwg >> 3, r = nwg & 7u, xcd = tile & 7u;
    tile = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + (tile >> 3);
  }

  // ---- prologue: per piece, the pixel's byte offset (+ this thread's chunk) and the mask of its taps inside the image ----------
  const uint32_t chunk_bytes = piece_chunk(tid) * 16u;
  int32_t a_base[4];
  uint32_t a_mask[4];
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    const uint32_t p = tile * kTilePixels + piece_row(i, tid);
    a_base[i] = 0;
    a_mask[i] = 0u;
    if (p < m) {
      const Pixel px = pixel_of(p, by_w, by_hw);
      a_base[i] = static_cast<int32_t>(p * kPixelBytes + chunk_bytes);
      a_mask[i] = tap_mask(px.y, px.x, height, width);
    }
  }
  const unsigned char *w_src = w + static_cast<size_t>(piece_row(0, tid)) * (kTaps * kPixelBytes) + chunk_bytes;
  const unsigned char *zeros = reinterpret_cast<const unsigned char *>(tower_zero_block);

  auto stage = [&](uint32_t kt, uint32_t buffer) {
    const uint32_t tap = ktile_tap(kt);
    const int32_t k_bytes = tap_pixel_offset(tap, width) * static_cast<int32_t>(kPixelBytes) + static_cast<int32_t>(ktile_channel(kt) * 2u);
    unsigned char *dst = tower_lds + buffer * kBufferBytes;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const unsigned char *src = ((a_mask[i] >> tap) & 1u) ? x + static_cast<ptrdiff_t>(a_base[i] + k_bytes) : zeros;
      tower_glds16(src, dst + piece_wave_base(i, wave));
    }
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
      tower_glds16(w_src + static_cast<size_t>(i) * 64u * (kTaps * kPixelBytes) + kt * kRowBytes, dst + kOperandBytes + piece_wave_base(i, wave));
  };

  const uint32_t wr = wave >> 2, wc = wave & 3u;
  // [channel block][pixel block] of this wave's 64 x 128: 16 x 16 blocks (form 0) or 32 x 32 blocks (form 1)
  using Acc = std::conditional_t<kForm == 0, tower_f32x4[4][8], seam_f32x16[2][4]>;
  Acc acc;
  if constexpr (kForm == 0) {
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int b = 0; b < 8; ++b) acc[n][b] = tower_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  } else {
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[n][b][e] = 0.0f;
  }
  // fragment addresses: the row block goes into the instruction's offset field, the k-steps are registers
  uint32_t f[4];
  if constexpr (kForm == 0) {
    f[0] = frag_addr(0, 0, lane); f[1] = frag_addr(0, 1, lane); f[2] = f[3] = 0u;
  } else {
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) f[s] = frag32_addr(0, s, lane);
  }
  const uint32_t x_frag = wr * 128u * kRowBytes, w_frag = kOperandBytes + wc * 64u * kRowBytes;

  auto compute = [&](const unsigned char *buf) {
    if constexpr (kForm == 0) {
#pragma unroll
      for (uint32_t kk = 0; kk < 2; ++kk) {
        vuint4 wf[4], xf[8];
#pragma unroll
        for (uint32_t n = 0; n < 4; ++n) wf[n] = *reinterpret_cast<const vuint4 *>(buf + w_frag + n * 16u * kRowBytes + f[kk]);
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) xf[b] = *reinterpret_cast<const vuint4 *>(buf + x_frag + b * 16u * kRowBytes + f[kk]);
#pragma unroll
        for (uint32_t n = 0; n < 4; ++n)
#pragma unroll
          for (uint32_t b = 0; b < 8; ++b) acc[n][b] = tower_mfma<T>(wf[n], xf[b], acc[n][b]);
      }
    } else {
#pragma unroll
      for (uint32_t s = 0; s < 4; ++s) {
        vuint4 wf[2], xf[4];
#pragma unroll
        for (uint32_t n = 0; n < 2; ++n) wf[n] = *reinterpret_cast<const vuint4 *>(buf + w_frag + n * 32u * kRowBytes + f[s]);
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b) xf[b] = *reinterpret_cast<const vuint4 *>(buf + x_frag + b * 32u * kRowBytes + f[s]);
#pragma unroll
        for (uint32_t n = 0; n < 2; ++n)
#pragma unroll
          for (uint32_t b = 0; b < 4; ++b) acc[n][b] = tower_mfma32<T>(wf[n], xf[b], acc[n][b]);
      }
    }
  };

  stage(0, 0);
#pragma unroll 1
  for (uint32_t kt = 0; kt < kKTiles; kt += 2) {
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half) {               // buffer `half` holds K-tile kt + half
      // tile kt + half has landed (every wave waits for its own pieces, the barrier makes them everybody's), and every wave
      // has finished reading the other buffer (its reads are behind its MFMAs, which are behind this barrier)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (kt + half + 1 < kKTiles) stage(kt + half + 1, half ^ 1u);
      compute(tower_lds + half * kBufferBytes);
    }
  }

  // ---- epilogue: first rounding, through the LDS, bias + activation + second rounding in row order ----------------------------
  __syncthreads();                                            // every wave is done with the operands' buffers
  if constexpr (kForm == 0) {
#pragma unroll
    for (uint32_t n = 0; n < 4; ++n)
#pragma unroll
      for (uint32_t b = 0; b < 8; ++b) {
        const uint32_t at = out_addr(acc_pixel(wr * 8u + b, lane), acc_channel(wc * 4u + n, lane, 0));
        uint2 v;
        v.x = seam_pack2<T>(acc[n][b][0], acc[n][b][1]);
        v.y = seam_pack2<T>(acc[n][b][2], acc[n][b][3]);
        *reinterpret_cast<uint2 *>(tower_lds + at) = v;
      }
  } else {
#pragma unroll
    for (uint32_t n = 0; n < 2; ++n)
#pragma unroll
      for (uint32_t b = 0; b < 4; ++b)
#pragma unroll
        for (uint32_t g = 0; g < 4; ++g) {                    // registers 4 g .. 4 g + 3: four consecutive channels
          const uint32_t at = out_addr(acc32_pixel(wr * 4u + b, lane), acc32_channel(wc * 2u + n, lane, 4u * g));
          uint2 v;
          v.x = seam_pack2<T>(acc[n][b][4 * g], acc[n][b][4 * g + 1]);
          v.y = seam_pack2<T>(acc[n][b][4 * g + 2], acc[n][b][4 * g + 3]);
          *reinterpret_cast<uint2 *>(tower_lds + at) = v;
        }
  }
  __syncthreads();
  // unit q = 512 it + tid: pixel q / 32 = 16 it + tid / 32, physical chunk tid % 32 -- the logical chunk is the same in every trip
  const uint32_t pixel0 = tid >> 5, chunk = out_chunk(pixel0, tid & 31u);
  float bias8[8];
  {
    const vuint4 bv = *reinterpret_cast<const vuint4 *>(bias + chunk * 8u);
#pragma unroll
    for (int e = 0; e < 8; ++e) bias8[e] = seam_unpack<T>(bv[e >> 1], e & 1);
  }
#pragma unroll 4
  for (uint32_t it = 0; it < 16; ++it) {
    const uint32_t pixel = it * 16u + pixel0, p = tile * kTilePixels + pixel;
    const vuint4 v = *reinterpret_cast<const vuint4 *>(tower_lds + (it * kThreads + tid) * 16u);
    vuint4 r;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      float o[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float s = seam_unpack<T>(v[d], e) + bias8[2 * d + e];
        o[e] = kRelu ? (s > 0.0f ? s : (s != s ? s : 0.0f)) : s;      // NaN goes through, as odtk_bias_act
      }
      r[d] = seam_pack2<T>(o[0], o[1]);
    }
    if (p < m) *reinterpret_cast<vuint4 *>(y + static_cast<size_t>(p) * kPixelBytes + chunk * 16u) = r;
  }
}

}  // namespace odtk
