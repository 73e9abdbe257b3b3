// seam.hpp -- the seam between two bottleneck blocks of ResNet's layer1 as ONE pass: the last 1x1 convolution of a block
// (64 -> 256, + skip, ReLU) and the first 1x1 convolution of the next block (256 -> 64, or 256 -> 128 into layer2; ReLU):
//     out[p][c] = rne_T(relu(fp32 sum_k y2[p][k] * W3[c][k] + fp32(skip[p][c]) + b3[c]))          c < 256, k < 64
//     z[p][n]   = rne_T(relu(fp32 sum_c out[p][c] * W1[n][c] + b1[n]))                            n < N2 (64 | 128)
// (the second product reads the ROUNDED out: the values that are stored; the skip is added before the bias, as the GEMM's epilogue
// does, and the k-steps follow the GEMM's order: on the flagship shape both outputs equal the two GEMMs' bit for bit,
// profiles/bottleneck_seam_probe.txt).  As two GEMMs `out` is written (262 MB at the flagship shape), read back at once by the
// second GEMM and read a third time later as the next skip; here the middle read never leaves the registers.  No reference
// equivalent as a kernel (torchvision Bottleneck.forward, reference odtk/backbones/resnet.py).
//
// HBM-bound: (64 + 256 + 256 + N2) * sizeof(T) bytes per pixel; the arithmetic is about a tenth of the pass's MFMA time.
//
// One wave owns 32 pixels, the pixel on the MFMA lane (v_mfma_f32_32x32x16): for each of the eight 32-channel blocks
//     X  = W3_blk . y2^T            (4 MFMAs: A = 32 channels x 64, B = y2^T: lane (r, h) holds y2[pixel r][16 s + 8 h + 0..7])
//     X += skip + b3, ReLU, rounded pairwise to T: registers 8 s .. 8 s + 7 of a lane ARE the B fragment of k-step s of
//     Z^T += W1[:, blk] . X         (2 MFMAs per 32 outputs), and 16 contiguous bytes of the lane's row of `out`.
// The accumulator holds row (reg & 3) + 8 (reg >> 2) + 4 h of X in register reg of lane half h.  The rows of each weight tile are
// therefore permuted when the weights are staged: row rho of a tile is channel pi(rho) of its 32-channel block, pi = swap bits 2 and
// 3.  Then registers 8 u .. 8 u + 7 of lane half h are the CONTIGUOUS channels 16 u + 8 h + 0..7: a lane's piece of skip, `out` and
// `z` is one 16-byte vector, and W1's k index (which must follow X's permuted rows) is back in natural order.
// The weights lie in LDS in fragment order (a wave reads 64 consecutive 16-byte fragments: no bank conflicts), staged once per
// workgroup; the grid is persistent.  Activations travel between memory and the fragments in 32-pixel x 128-byte panels through
// 4 KB of LDS per wave (SeamPanel below), so that every global access covers whole 128-byte lines.  A panel's registers are
// re-loaded with the wave's NEXT tile as soon as the panel has been handed to the LDS: a whole tile (20 KB per wave) is in flight
// while one computes.
#pragma once

#include "common.hpp"
#include "prefilter.hpp"   // element types, vuint4, bf16/f16 conversions

namespace odtk {

typedef float seam_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 seam_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 seam_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 seam_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 seam_f16x2 __attribute__((ext_vector_type(2)));
typedef float seam_f32x2 __attribute__((ext_vector_type(2)));
typedef float seam_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSeamThreads = 256;                          // 4 waves: 128 pixels per workgroup and trip
constexpr int kSeamCin = 64, kSeamCmid = 256;

// LDS: W3 fragments [8 blocks][4 k-steps][64 lanes] x 16 B, W1 fragments [8 blocks][2 k-steps][N2 / 32 tiles][64 lanes] x 16 B,
// b3 [256] and b1 [N2] in fp32, and 4 KB per wave for the panels on their way between memory and the fragments (SeamPanel)
template <int N2>
constexpr size_t seam_lds_bytes() {
  return 8 * 4 * 64 * 16 + 8 * 2 * (N2 / 32) * 64 * 16 + (kSeamCmid + N2) * 4 + (kSeamThreads / 64) * 256 * 16;
}

__device__ __forceinline__ uint32_t seam_pi(uint32_t rho) {   // swap bits 2 and 3
  return (rho & ~12u) | ((rho & 4u) << 1) | ((rho & 8u) >> 1);
}

template <typename T>
__device__ __forceinline__ seam_f32x16 seam_mfma(vuint4 a, vuint4 b, seam_f32x16 c) {
  if constexpr (std::is_same_v<T, BF16>)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(seam_bf16x8, a), __builtin_bit_cast(seam_bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(seam_f16x8, a), __builtin_bit_cast(seam_f16x8, b), c, 0, 0, 0);
}

template <typename T>
__device__ __forceinline__ uint32_t seam_pack2(float lo, float hi) {    // round-to-nearest-even, two at a time
  if constexpr (std::is_same_v<T, BF16>)
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(seam_f32x2{lo, hi}, seam_bf16x2));
  else
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(seam_f32x2{lo, hi}, seam_f16x2));
}

template <typename T>
__device__ __forceinline__ float seam_unpack(uint32_t word, int half) {
  const uint32_t h = half ? word >> 16 : word & 0xffffu;
  return std::is_same_v<T, BF16> ? bf16_bits_to_float(h) : f16_bits_to_float(h);
}

// registers 8 u .. 8 u + 7 of an accumulator + bias (+ skip), ReLU -> eight T in 16 bytes
template <typename T, bool kSkip>
__device__ __forceinline__ vuint4 seam_epilogue(const seam_f32x16 &acc, int u, const float *bias8, vuint4 skip) {
  const seam_f32x4 b0 = *reinterpret_cast<const seam_f32x4 *>(bias8), b1 = *reinterpret_cast<const seam_f32x4 *>(bias8 + 4);
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float o = acc[8 * u + e];
    if (kSkip) o += seam_unpack<T>(skip[e >> 1], e & 1);     // the skip first, then the bias: the order of the GEMM's epilogue
    o += e < 4 ? b0[e & 3] : b1[e & 3];                      // (beta * C, then the bias vector), whose bits this pass reproduces
    v[e] = o > 0.0f ? o : (o != o ? o : 0.0f);             // NaN goes through, as torch.relu
  }
  vuint4 r;
#pragma unroll
  for (int d = 0; d < 4; ++d) r[d] = seam_pack2<T>(v[2 * d], v[2 * d + 1]);
  return r;
}

// One 32-pixel x 128-byte panel (64 channels of `out` / skip / z, or a whole y2 row) between global memory and a wave's fragments.
// Towards memory a panel is four 16-byte vectors per lane in "row order": vector i of lane l is unit e = 64 i + l, pixel e >> 3,
// 16-byte chunk e & 7 -- eight lanes cover one full 128-byte line, an instruction eight whole lines.  (Straight from the fragment
// layout -- lane = pixel, 16 bytes each -- an instruction touched 64 lines for 16 bytes each, and the pass ran at 2.5 TB/s.)
// Towards the MFMA a lane wants chunk c of ITS pixel r.  The panel crosses the wave's own 4 KB of LDS, chunk c of pixel p at unit
// 8 p + (c ^ ((p >> 1) & 7)): both sides are conflict-free, and a wave's LDS accesses execute in order, so no barrier is needed.
struct SeamPanel {
  vuint4 *stage;        // this wave's 256 units
  uint32_t row[4];      // unit of vector i in row order
  uint32_t pix[4];      // its pixel within the tile
  uint32_t chunk;       // its chunk (the same for the four)
  uint32_t frag_base, frag_swz;
  __device__ __forceinline__ SeamPanel(vuint4 *stage_, uint32_t lane) : stage(stage_) {
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t e = 64 * i + lane;
      pix[i] = e >> 3;
      row[i] = (e & ~7u) | ((e & 7u) ^ ((e >> 4) & 7u));
    }
    chunk = lane & 7u;
    const uint32_t r = lane & 31u;
    frag_base = 8 * r;
    frag_swz = (r >> 1) & 7u;
  }
  __device__ __forceinline__ uint32_t frag(uint32_t c) const { return frag_base + (c ^ frag_swz); }
};

// the four row-order loads of a panel: pixels tile * 32 + ..., clamped to the last one (a partial tile reads valid rows, stores none)
template <bool kStream>
__device__ __forceinline__ void seam_load_panel(vuint4 (&v)[4], const SeamPanel &pn, const uint16_t *base, uint32_t row_elems, uint32_t col,
                                                uint64_t tile, uint64_t m) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint64_t p = tile * 32 + pn.pix[i];
    p = p < m ? p : m - 1;
    const vuint4 *src = reinterpret_cast<const vuint4 *>(base + p * row_elems + col) + pn.chunk;
    v[i] = kStream ? __builtin_nontemporal_load(src) : *src;
  }
}

template <bool kFull>
__device__ __forceinline__ void seam_store_panel(const SeamPanel &pn, uint16_t *base, uint32_t row_elems, uint32_t col, uint64_t tile,
                                                 uint64_t m) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t p = tile * 32 + pn.pix[i];
    const vuint4 v = pn.stage[pn.row[i]];
    if (kFull || p < m) *(reinterpret_cast<vuint4 *>(base + p * row_elems + col) + pn.chunk) = v;
  }
}

// One tile of a wave.  In: the tile's y2 panel (yq) and four skip panels (sq) in registers, loaded a tile ago; out: the same
// registers hold tile `next` (each panel is re-loaded as soon as it has been handed to the LDS, so a whole tile stays in flight).
// kFull: all 32 pixels exist -- the stores are unconditional, and the compiler's count of the memory operations in flight exact
// (behind a branch it must assume the fewest, and every wait for a prefetched register also waited for the newest stores).
template <typename T, int N2, bool kFull>
__device__ __forceinline__ void seam_tile(const SeamPanel &pn, uint32_t lane, const vuint4 *s_w3, const vuint4 *s_w1, const float *s_b3,
                                          const float *s_b1, vuint4 (&yq)[4], vuint4 (&sq)[4][4], const uint16_t *y2, const uint16_t *skip,
                                          uint16_t *out, uint16_t *z, uint64_t tile, uint64_t next, uint64_t m) {
  constexpr int NT = N2 / 32;
  const uint32_t h = lane >> 5;
  vuint4 yf[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) pn.stage[pn.row[i]] = yq[i];
#pragma unroll
  for (int s = 0; s < 4; ++s) yf[s] = pn.stage[pn.frag(2 * s + h)];
  seam_load_panel<false>(yq, pn, y2, kSeamCin, 0, next, m);

  seam_f32x16 zacc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) zacc[t][e] = 0.0f;

#pragma unroll
  for (int q = 0; q < 4; ++q) {                              // 64 channels of out: two 32-channel blocks
    // the weight fragments do not change from tile to tile: without this fence the compiler hoists all of their LDS reads out of
    // the tile loop and holds 64 KB of weights in registers (512 per lane + scratch)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < 4; ++i) pn.stage[pn.row[i]] = sq[q][i];
    seam_load_panel<true>(sq[q], pn, skip, kSeamCmid, 64 * q, next, m);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int blk = 2 * q + b;
      seam_f32x16 x;
#pragma unroll
      for (int e = 0; e < 16; ++e) x[e] = 0.0f;
#pragma unroll
      for (int s = 0; s < 4; ++s) x = seam_mfma<T>(s_w3[(blk * 4 + s) * 64 + lane], yf[s], x);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const uint32_t at = pn.frag(4 * b + 2 * u + h);
        const vuint4 frag = seam_epilogue<T, true>(x, u, s_b3 + 32 * blk + 16 * u + 8 * h, pn.stage[at]);
        pn.stage[at] = frag;                                 // (the lane's own unit: read as skip, written as out)
#pragma unroll
        for (int t = 0; t < NT; ++t) zacc[t] = seam_mfma<T>(s_w1[((blk * 2 + u) * NT + t) * 64 + lane], frag, zacc[t]);
      }
    }
    seam_store_panel<kFull>(pn, out, kSeamCmid, 64 * q, tile, m);
  }
#pragma unroll
  for (int g = 0; g < NT / 2; ++g) {                         // 64 channels of z
    asm volatile("" ::: "memory");
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
        pn.stage[pn.frag(4 * b + 2 * u + h)] =
            seam_epilogue<T, false>(zacc[2 * g + b], u, s_b1 + 32 * (2 * g + b) + 16 * u + 8 * h, vuint4{0u, 0u, 0u, 0u});
    }
    seam_store_panel<kFull>(pn, z, N2, 64 * g, tile, m);
  }
}

template <typename T, int N2>
__global__ __launch_bounds__(kSeamThreads) void bottleneck_seam_kernel(const uint16_t *__restrict__ y2, const uint16_t *__restrict__ skip,
                                                                       const uint16_t *__restrict__ w3, const float *__restrict__ b3,
                                                                       const uint16_t *__restrict__ w1, const float *__restrict__ b1,
                                                                       uint16_t *__restrict__ out, uint16_t *__restrict__ z, uint64_t m) {
  constexpr int NT = N2 / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char seam_lds[];
  vuint4 *s_w3 = reinterpret_cast<vuint4 *>(seam_lds);                       // [(blk * 4 + s) * 64 + lane]
  vuint4 *s_w1 = s_w3 + 8 * 4 * 64;                                          // [((blk * 2 + s) * NT + t) * 64 + lane]
  float *s_b3 = reinterpret_cast<float *>(s_w1 + 8 * 2 * NT * 64);
  float *s_b1 = s_b3 + kSeamCmid;
  vuint4 *s_stage = reinterpret_cast<vuint4 *>(s_b1 + N2);                   // [wave][256]

  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  // ---- stage the weights in fragment order (rows permuted by pi) ---------------------------------------------------------------
  for (uint32_t f = tid; f < 8 * 4 * 64; f += kSeamThreads) {
    const uint32_t fl = f & 63u, s = (f >> 6) & 3u, blk = f >> 8;
    const uint32_t row = 32 * blk + seam_pi(fl & 31u), k = 16 * s + 8 * (fl >> 5);
    s_w3[f] = *reinterpret_cast<const vuint4 *>(w3 + row * kSeamCin + k);
  }
  for (uint32_t f = tid; f < 8 * 2 * NT * 64; f += kSeamThreads) {
    const uint32_t fl = f & 63u, t = (f >> 6) % NT, bs = (f >> 6) / NT;       // bs = blk * 2 + s: 16 channels of `out` each
    const uint32_t row = 32 * t + seam_pi(fl & 31u), k = 16 * bs + 8 * (fl >> 5);
    s_w1[f] = *reinterpret_cast<const vuint4 *>(w1 + row * kSeamCmid + k);
  }
  for (uint32_t c = tid; c < kSeamCmid + N2; c += kSeamThreads) s_b3[c] = c < kSeamCmid ? b3[c] : b1[c - kSeamCmid];
  __syncthreads();

  const uint64_t n_tiles = (m + 31) / 32, n_full = m / 32;                   // wave tiles of 32 pixels; at most one is partial
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * (kSeamThreads / 64);
  uint64_t tile = static_cast<uint64_t>(blockIdx.x) * (kSeamThreads / 64) + (tid >> 6);
  if (tile >= n_tiles) return;                                               // (after the only barrier)

  const SeamPanel pn(s_stage + (tid >> 6) * 256, lane);
  vuint4 yq[4], sq[4][4];
  seam_load_panel<false>(yq, pn, y2, kSeamCin, 0, tile, m);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    // keep the order of use: loads return in order and the tile waits for panel 0 first -- issued last (as the scheduler likes
    // to), it would make that wait one for everything in flight, in every trip
    asm volatile("" ::: "memory");
    seam_load_panel<true>(sq[q], pn, skip, kSeamCmid, 64 * q, tile, m);
  }
  asm volatile("" ::: "memory");
#pragma unroll 1
  for (; tile < n_full; tile += stride) {
    const uint64_t next = tile + stride < n_tiles ? tile + stride : tile;    // the last trip re-loads its own tile (unused)
    seam_tile<T, N2, true>(pn, lane, s_w3, s_w1, s_b3, s_b1, yq, sq, y2, skip, out, z, tile, next, m);
  }
  if (tile < n_tiles) seam_tile<T, N2, false>(pn, lane, s_w3, s_w1, s_b3, s_b1, yq, sq, y2, skip, out, z, tile, tile, m);
}

}  // namespace odtk
