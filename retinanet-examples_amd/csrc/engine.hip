// engine.hip -- what the inference engine runs between convolutions: bias + activation epilogues, the max-pool, nearest
// 2x upsampling, the pyramid canvas, the stem pack, the hipBLASLt GEMM (gemm_lt.hpp is included here only), the bottleneck seam
// (seam.hpp: two 1x1 convolutions of layer1 in one MFMA pass) and the head towers' 3x3 convolution (tower_conv.hpp).
#include <cstring>

#include "runtime.hpp"
#include "epilogue.hpp"
#include "gemm_lt.hpp"
#include "seam.hpp"
#include "tower_conv.hpp"

namespace {

// odtk_debug_stream_tuning: both fields in ONE word (a launch reads it once, relaxed): bits 0..16 = grid_cap (0: each launcher's own
// cap), bit 20 = pool_wide_index.
constexpr int kStreamCapMax = 65536, kStreamWideBit = 1 << 20;
std::atomic<int> g_stream_tuning{0};

inline int stream_tuning() { return g_stream_tuning.load(std::memory_order_relaxed); }

// The grid of a streaming kernel: `blocks` workgroups of work, at most the launcher's `own_cap` -- or the debug cap in its place.
inline uint64_t stream_grid(uint64_t blocks, uint64_t own_cap, int tuning) {
  const uint64_t cap = (tuning & (kStreamWideBit - 1)) ? static_cast<uint64_t>(tuning & (kStreamWideBit - 1)) : own_cap;
  return blocks > cap ? cap : blocks;
}

// What bias_act_launch does with n elements of rows of `channels`, `per` to a 16-byte vector: the ONE place that decides it (the
// launcher and odtk_debug_bias_act_grid both ask here).
struct BiasActPlan {
  bool fast;         // bias_act_kernel (16-byte vectors), else bias_act_scalar_kernel over all n elements
  uint32_t blocks;   // workgroups of 256 lanes
  uint32_t vpr;      // fast: vectors per row
  uint64_t n_vec;    // fast: vectors in all
  uint64_t stride;   // blocks * 256: the grid stride, in vectors (fast) or elements (scalar)
  uint64_t trips;    // fast: passes of lane 0 of workgroup 0 through the unrolled loop (4 vectors, `stride` apart, per pass)
};

BiasActPlan bias_act_plan(uint64_t n, uint32_t channels, int per_, int tuning) {
  const uint32_t per = static_cast<uint32_t>(per_);
  BiasActPlan p{};
  if (channels % per == 0 && n / per >= 256) {
    // fast form: grid stride (blocks * 256 lanes) must be a multiple of the row length in vectors
    p.fast = true;
    p.vpr = channels / per;
    p.n_vec = n / per;                                      // n is a multiple of channels, hence of per: no scalar tail
    uint32_t g = p.vpr, m = 256;                            // unit = vpr / gcd(vpr, 256) blocks
    while (m) { const uint32_t r_ = g % m; g = m; m = r_; }
    const uint32_t unit = p.vpr / g;
    uint64_t blocks = stream_grid((p.n_vec + 256ull * 4 - 1) / (256ull * 4), 256 * 16, tuning);   // ~4 vectors per lane, <= 16 workgroups per CU
    blocks = (blocks + unit - 1) / unit * unit;             // after the cap: the stride stays a multiple of the row
    p.blocks = static_cast<uint32_t>(blocks);
    p.stride = blocks * 256;
    constexpr uint64_t kUnroll = 4;                          // bias_act_kernel's
    p.trips = p.n_vec > (kUnroll - 1) * p.stride ? (p.n_vec - (kUnroll - 1) * p.stride + kUnroll * p.stride - 1) / (kUnroll * p.stride) : 0;
  } else {
    p.blocks = static_cast<uint32_t>(stream_grid((n + 255) / 256, 4096, tuning));
    p.stride = static_cast<uint64_t>(p.blocks) * 256;
  }
  return p;
}

template <typename T, bool kRes, bool kRelu>
int bias_act_launch(void *y, const float *bias, const void *res, uint64_t n, uint32_t channels, hipStream_t stream) {
  const BiasActPlan p = bias_act_plan(n, channels, T::kPerLoad, stream_tuning());
  if (p.fast)
    timed_launch(ODTK_KERNEL_EPILOGUE, odtk::bias_act_kernel<T, kRes, kRelu>, dim3(p.blocks), dim3(256), 0, stream, y, bias, res, p.n_vec,
                 p.vpr);
  else
    hipLaunchKernelGGL((odtk::bias_act_scalar_kernel<T, kRes, kRelu>), dim3(p.blocks), dim3(256), 0, stream, y, bias, res,
                       static_cast<uint64_t>(0), n, channels);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

template <typename T>
int bias_act_typed(void *y, const float *bias, const void *res, uint64_t n, uint32_t c, bool relu, hipStream_t s) {
  if (res) return relu ? bias_act_launch<T, true, true>(y, bias, res, n, c, s) : bias_act_launch<T, true, false>(y, bias, res, n, c, s);
  return relu ? bias_act_launch<T, false, true>(y, bias, res, n, c, s) : bias_act_launch<T, false, false>(y, bias, res, n, c, s);
}

int bias_act_dispatch(void *y, const float *bias, const void *res, uint64_t n, uint32_t c, int dtype, bool relu,
                      hipStream_t s) {
  return dispatch_dtype(dtype, [&](auto t) { return bias_act_typed<decltype(t)>(y, bias, res, n, c, relu, s); });
}

template <typename TIn>
int stem_pack_launch(const void *x, void *out, int batch, int height, int width, int channels_last, int out_dtype, hipStream_t stream) {
  const unsigned long long total = 1ull * batch * (height / 2) * (width / 2);
  const unsigned long long blocks = stream_grid((total + 255) / 256, 256 * 32, stream_tuning());
  const odtk::FastDiv by_wo = odtk::fastdiv_make(static_cast<uint32_t>(width / 2));
  const odtk::FastDiv by_howo = odtk::fastdiv_make(static_cast<uint32_t>(height / 2) * static_cast<uint32_t>(width / 2));
  if (out_dtype == ODTK_BF16)
    timed_launch(ODTK_KERNEL_STEM_PACK, odtk::stem_pack_kernel<TIn, odtk::BF16>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, x, out,
                 static_cast<uint32_t>(batch), static_cast<uint32_t>(height), static_cast<uint32_t>(width), static_cast<uint32_t>(channels_last), by_wo, by_howo);
  else
    timed_launch(ODTK_KERNEL_STEM_PACK, odtk::stem_pack_kernel<TIn, odtk::F16>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, x, out,
                 static_cast<uint32_t>(batch), static_cast<uint32_t>(height), static_cast<uint32_t>(width), static_cast<uint32_t>(channels_last), by_wo, by_howo);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

template <typename T, int N2>
int seam_launch(const void *y2, const void *skip, const void *w3, const float *b3, const void *w1, const float *b1, void *out, void *z,
                uint64_t m, hipStream_t stream) {
  constexpr size_t lds = odtk::seam_lds_bytes<N2>();
  const int rc = allow_dynamic_lds(reinterpret_cast<const void *>(&odtk::bottleneck_seam_kernel<T, N2>), lds, "bottleneck_seam_kernel LDS");
  if (rc != ODTK_OK) return rc;
  int device = 0, cus = 0;
  ODTK_HIP_TRY(hipGetDevice(&device));
  ODTK_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  // persistent: as many workgroups as the LDS lets a CU hold (160 KiB: two with 64 outputs, one with 128), each staging the weights once
  constexpr uint64_t per_group = odtk::kSeamThreads / 64 * 32;
  uint64_t blocks = (m + per_group - 1) / per_group;
  const uint64_t resident = static_cast<uint64_t>(cus > 0 ? cus : 1) * (160 * 1024 / lds);
  if (blocks > resident) blocks = resident;
  timed_launch(ODTK_KERNEL_SEAM, odtk::bottleneck_seam_kernel<T, N2>, dim3(static_cast<unsigned>(blocks)), dim3(odtk::kSeamThreads), lds, stream,
               static_cast<const uint16_t *>(y2), static_cast<const uint16_t *>(skip), static_cast<const uint16_t *>(w3), b3,
               static_cast<const uint16_t *>(w1), b1, static_cast<uint16_t *>(out), static_cast<uint16_t *>(z), m);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

// odtk_debug_tower_conv_variant: bit 0 = tile ids permuted by L2, bit 1 = the 16x16x32 form (otherwise the 32x32x16 form, whose sums
// follow the convolution library's instance)
std::atomic<int> g_tower_variant{1};

template <typename T, bool kRelu, int kForm>
int tower_conv_launch(void *y, const void *x, const void *w, const void *bias, uint32_t m, uint32_t height, uint32_t width, bool remap,
                      hipStream_t stream) {
  const int rc = allow_dynamic_lds(reinterpret_cast<const void *>(&odtk::tower_conv3x3_kernel<T, kRelu, kForm>), odtk::tower::kLdsBytes,
                                   "tower_conv3x3_kernel LDS");
  if (rc != ODTK_OK) return rc;
  const uint32_t tiles = (m + odtk::tower::kTilePixels - 1) / odtk::tower::kTilePixels;
  timed_launch(ODTK_KERNEL_TOWER_CONV, odtk::tower_conv3x3_kernel<T, kRelu, kForm>, dim3(tiles), dim3(odtk::tower::kThreads),
               odtk::tower::kLdsBytes, stream, static_cast<const unsigned char *>(x), static_cast<const unsigned char *>(w),
               static_cast<const uint16_t *>(bias), static_cast<unsigned char *>(y), m, height, width, odtk::fastdiv_make(width),
               odtk::fastdiv_make(height * width), remap ? 1u : 0u);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

template <typename T>
int tower_conv_typed(void *y, const void *x, const void *w, const void *bias, uint32_t m, uint32_t h, uint32_t wd, bool relu, int variant,
                     hipStream_t s) {
  const bool remap = variant & 1;
  if (variant & 2) return relu ? tower_conv_launch<T, true, 0>(y, x, w, bias, m, h, wd, remap, s) : tower_conv_launch<T, false, 0>(y, x, w, bias, m, h, wd, remap, s);
  return relu ? tower_conv_launch<T, true, 1>(y, x, w, bias, m, h, wd, remap, s) : tower_conv_launch<T, false, 1>(y, x, w, bias, m, h, wd, remap, s);
}

}  // namespace

extern "C" {

int odtk_debug_tower_conv_variant(int variant) {
  if (variant < -1 || variant > 3) return ODTK_ERR_INVALID;
  return variant < 0 ? g_tower_variant.load() : g_tower_variant.exchange(variant);
}

int odtk_debug_stream_tuning(int grid_cap, int pool_wide_index) {
  if (grid_cap < -1 || grid_cap > kStreamCapMax || pool_wide_index < -1 || pool_wide_index > 1) return ODTK_ERR_INVALID;
  int was = g_stream_tuning.load(std::memory_order_relaxed), now;
  do {
    now = (grid_cap < 0 ? was & (kStreamWideBit - 1) : grid_cap) | (pool_wide_index < 0 ? was & kStreamWideBit : pool_wide_index ? kStreamWideBit : 0);
  } while (!g_stream_tuning.compare_exchange_weak(was, now, std::memory_order_relaxed));
  return ODTK_OK;
}

int odtk_debug_stream_tuning_get(int out[2]) {
  if (!out) return ODTK_ERR_INVALID;
  const int tuning = stream_tuning();
  out[0] = tuning & (kStreamWideBit - 1);
  out[1] = (tuning & kStreamWideBit) != 0;
  return ODTK_OK;
}

int odtk_debug_bias_act_grid(size_t n_pixels, int channels, int dtype, unsigned out[4]) {
  if (!out || n_pixels == 0 || channels <= 0) return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  const BiasActPlan p = bias_act_plan(static_cast<uint64_t>(n_pixels) * channels, static_cast<uint32_t>(channels),
                                      dtype == ODTK_F32 ? odtk::F32::kPerLoad : odtk::BF16::kPerLoad, stream_tuning());
  out[0] = p.fast ? 1u : 0u;
  out[1] = p.blocks;
  out[2] = static_cast<unsigned>(p.stride);
  out[3] = p.trips > 0xffffffffull ? 0xffffffffu : static_cast<unsigned>(p.trips);
  return ODTK_OK;
}

int odtk_tower_conv3x3(void *y, const void *x, const void *w, const void *bias, int batch_size, int height, int width, int c_in, int c_out,
                       int dtype, int relu, void *stream) {
  if (!y || !x || !w || !bias || batch_size <= 0 || height <= 0 || width <= 0 || c_in <= 0 || c_out <= 0) return ODTK_ERR_INVALID;
  if (y == x) return ODTK_ERR_INVALID;
  if (dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  if (c_in != static_cast<int>(odtk::tower::kChannels) || c_out != static_cast<int>(odtk::tower::kChannels)) return ODTK_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(bias)) & 15u)
    return ODTK_ERR_INVALID;
  // 32-bit byte offsets into x and y: a pixel is 512 bytes
  const uint64_t m = static_cast<uint64_t>(batch_size) * static_cast<uint64_t>(height) * static_cast<uint64_t>(width);
  if (m * odtk::tower::kPixelBytes >= (1ull << 31)) return ODTK_ERR_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int variant = g_tower_variant.load(std::memory_order_relaxed);
  if (dtype == ODTK_BF16)
    return tower_conv_typed<odtk::BF16>(y, x, w, bias, static_cast<uint32_t>(m), static_cast<uint32_t>(height), static_cast<uint32_t>(width),
                                        relu != 0, variant, s);
  return tower_conv_typed<odtk::F16>(y, x, w, bias, static_cast<uint32_t>(m), static_cast<uint32_t>(height), static_cast<uint32_t>(width),
                                      relu != 0, variant, s);
}

int odtk_bottleneck_seam(void *out, void *z, const void *y2, const void *skip, const void *w3, const float *b3, const void *w1,
                         const float *b1, size_t m, int c_in, int c_mid, int c_next, int dtype, void *stream) {
  if (!out || !z || !y2 || !skip || !w3 || !b3 || !w1 || !b1 || c_in <= 0 || c_mid <= 0 || c_next <= 0) return ODTK_ERR_INVALID;
  if (out == z || out == y2 || out == skip || z == y2 || z == skip) return ODTK_ERR_INVALID;
  if (dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  if (c_in != odtk::kSeamCin || c_mid != odtk::kSeamCmid || (c_next != 64 && c_next != 128)) return ODTK_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(y2) | reinterpret_cast<uintptr_t>(skip) |
       reinterpret_cast<uintptr_t>(w3) | reinterpret_cast<uintptr_t>(w1)) & 15u)
    return ODTK_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(b3) | reinterpret_cast<uintptr_t>(b1)) & 3u) return ODTK_ERR_INVALID;
  if (m > (1ull << 40)) return ODTK_ERR_INVALID;
  if (m == 0) return ODTK_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == ODTK_BF16)
    return c_next == 64 ? seam_launch<odtk::BF16, 64>(y2, skip, w3, b3, w1, b1, out, z, m, s)
                        : seam_launch<odtk::BF16, 128>(y2, skip, w3, b3, w1, b1, out, z, m, s);
  return c_next == 64 ? seam_launch<odtk::F16, 64>(y2, skip, w3, b3, w1, b1, out, z, m, s)
                      : seam_launch<odtk::F16, 128>(y2, skip, w3, b3, w1, b1, out, z, m, s);
}

int odtk_bias_act(void *y, const float *bias, const void *residual, size_t n_pixels, int channels, int dtype,
                  int relu, void *stream) {
  if (!y || !bias || channels <= 0) return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(y) & 15u) || (reinterpret_cast<uintptr_t>(residual) & 15u)) return ODTK_ERR_INVALID;
  const uint64_t n = static_cast<uint64_t>(n_pixels) * channels;
  if (n == 0) return ODTK_OK;
  return bias_act_dispatch(y, bias, residual, n, static_cast<uint32_t>(channels), dtype, relu != 0,
                           static_cast<hipStream_t>(stream));
}

int odtk_bias_act_maxpool(const void *y, const float *bias, void *out, int batch_size, int height, int width,
                          int channels, int dtype, int relu, void *stream) {
  if (!y || !bias || !out || batch_size <= 0 || height <= 0 || width <= 0 || channels <= 0) return ODTK_ERR_INVALID;
  if (dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  if (channels % 8 != 0) return ODTK_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out)) & 15u) return ODTK_ERR_INVALID;
  if (1ull * height * width * channels >= (1ull << 32)) return ODTK_ERR_UNSUPPORTED;   // 32-bit offsets inside one image
  const uint32_t ho = (static_cast<uint32_t>(height) + 1) / 2, wo = (static_cast<uint32_t>(width) + 1) / 2;
  const uint64_t work = static_cast<uint64_t>(batch_size) * ho * wo * (channels / 8);
  const int tuning = stream_tuning();
  const uint64_t blocks = stream_grid((work + 255) / 256, 256 * 32, tuning);   // grid-stride beyond 32 workgroups per CU
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint16_t *in = static_cast<const uint16_t *>(y);
  uint16_t *o = static_cast<uint16_t *>(out);
  odtk::PoolDivisors dv;
  dv.groups = odtk::fastdiv_make(static_cast<uint32_t>(channels / 8));
  dv.wo = odtk::fastdiv_make(wo);
  dv.ho = odtk::fastdiv_make(ho);
  const bool small = work < (1ull << 32) && !(tuning & kStreamWideBit);   // else 64-bit index arithmetic (k32 = false)
#define ODTK_POOL_(T, R, S)                                                                                             \
  timed_launch(ODTK_KERNEL_POOL, odtk::bias_act_maxpool_kernel<T, R, S>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, in, \
               bias, o, static_cast<uint32_t>(batch_size), static_cast<uint32_t>(height),                             \
               static_cast<uint32_t>(width), static_cast<uint32_t>(channels), ho, wo, dv)
#define ODTK_POOL(T, R) do { if (small) ODTK_POOL_(T, R, true); else ODTK_POOL_(T, R, false); } while (0)
  if (dtype == ODTK_BF16) { if (relu) ODTK_POOL(odtk::BF16, true); else ODTK_POOL(odtk::BF16, false); }
  else { if (relu) ODTK_POOL(odtk::F16, true); else ODTK_POOL(odtk::F16, false); }
#undef ODTK_POOL_
#undef ODTK_POOL
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

int odtk_upsample_nearest2x(const void *x, void *out, int batch_size, int height, int width, int channels, int dtype,
                            void *stream) {
  if (!x || !out || batch_size <= 0 || height <= 0 || width <= 0 || channels <= 0) return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  const unsigned long long row_bytes = 1ull * channels * (dtype == ODTK_F32 ? 4 : 2);
  if (row_bytes % 16) return ODTK_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15u) return ODTK_ERR_INVALID;
  const unsigned long long groups = row_bytes / 16;
  const unsigned long long total = 4ull * batch_size * height * width * groups;
  if (total > 0xf0000000ull) return ODTK_ERR_INVALID;
  const unsigned long long blocks = stream_grid((total + 256ull * 4 - 1) / (256ull * 4), 256 * 16, stream_tuning());   // ~4 vectors per lane
  timed_launch(ODTK_KERNEL_UPSAMPLE, odtk::upsample_nearest2x_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
               static_cast<hipStream_t>(stream), static_cast<const odtk::vuint4 *>(x), static_cast<odtk::vuint4 *>(out),
               static_cast<uint32_t>(height), static_cast<uint32_t>(width), static_cast<uint32_t>(groups), static_cast<uint32_t>(total),
               odtk::fastdiv_make(static_cast<uint32_t>(groups)), odtk::fastdiv_make(2u * width), odtk::fastdiv_make(2u * height));
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

int odtk_canvas_pack(void *canvas, int batch_size, int height, int width, int channels, int dtype, const int *rects,
                     const void *const *sources, int n_rects, void *stream) {
  if (!canvas || !rects || batch_size <= 0 || height <= 0 || width <= 0 || channels <= 0 || n_rects < 0 || n_rects > ODTK_MAX_LEVELS)
    return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  const unsigned long long row_bytes = 1ull * channels * (dtype == ODTK_F32 ? 4 : 2);
  if (row_bytes % 16) return ODTK_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(canvas) & 15u) return ODTK_ERR_INVALID;
  const unsigned long long groups = row_bytes / 16;
  const unsigned long long total = 1ull * batch_size * height * width * groups;
  if (total > 0xf0000000ull) return ODTK_ERR_INVALID;
  odtk::CanvasArgs a{};
  a.n = static_cast<uint32_t>(n_rects);
  for (int l = 0; l < n_rects; ++l) {
    const int y0 = rects[4 * l], x0 = rects[4 * l + 1], h = rects[4 * l + 2], w = rects[4 * l + 3];
    if (y0 < 0 || x0 < 0 || h <= 0 || w <= 0 || y0 > height - h || x0 > width - w) return ODTK_ERR_INVALID;   // inside the canvas
    if (sources && (!sources[l] || (reinterpret_cast<uintptr_t>(sources[l]) & 15u))) return ODTK_ERR_INVALID;
    a.y0[l] = static_cast<uint32_t>(y0); a.x0[l] = static_cast<uint32_t>(x0);
    a.h[l] = static_cast<uint32_t>(h); a.w[l] = static_cast<uint32_t>(w);
    a.src[l] = sources ? static_cast<const odtk::vuint4 *>(sources[l]) : nullptr;
  }
  const unsigned long long blocks = stream_grid((total + 256ull * 4 - 1) / (256ull * 4), 256 * 16, stream_tuning());   // ~4 vectors per lane
  hipLaunchKernelGGL(odtk::canvas_fill_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<odtk::vuint4 *>(canvas), a, static_cast<uint32_t>(groups), static_cast<uint32_t>(total),
                     odtk::fastdiv_make(static_cast<uint32_t>(groups)), odtk::fastdiv_make(static_cast<uint32_t>(width)),
                     odtk::fastdiv_make(static_cast<uint32_t>(height)));
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

int odtk_canvas_clear(void *canvas, int batch_size, int height, int width, int channels, int dtype, const int *rects, int n_rects,
                      void *stream) {
  return odtk_canvas_pack(canvas, batch_size, height, width, channels, dtype, rects, nullptr, n_rects, stream);
}

int odtk_stem_pack(const void *x, void *out, int batch_size, int height, int width, int in_dtype, int channels_last, int out_dtype,
                   void *stream) {
  if (!x || !out || batch_size <= 0 || height <= 0 || width <= 0 || (height & 1) || (width & 1)) return ODTK_ERR_INVALID;
  if (channels_last != 0 && channels_last != 1) return ODTK_ERR_INVALID;
  if (in_dtype != ODTK_F32 && in_dtype != ODTK_BF16 && in_dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  if (out_dtype != ODTK_BF16 && out_dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(out) & 15u) return ODTK_ERR_INVALID;
  if (1ull * batch_size * (height / 2) * (width / 2) > 0xf0000000ull) return ODTK_ERR_INVALID;
  if (3ull * height * width >= (1ull << 32)) return ODTK_ERR_INVALID;       // 32-bit offsets inside one image
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dispatch_dtype(in_dtype, [&](auto t) {
    return stem_pack_launch<decltype(t)>(x, out, batch_size, height, width, channels_last, out_dtype, s);
  });
}

int odtk_gemm_init(const char *hipblaslt_path) { return odtk::lt::init(hipblaslt_path); }

size_t odtk_gemm_plan_export(char *text, size_t capacity) { return odtk::lt::plan_export(text, capacity); }
int odtk_gemm_plan_import(const char *text) { return odtk::lt::plan_import(text); }
int odtk_gemm_plan_pin_misses(void) { return odtk::lt::pin_misses(); }
void odtk_gemm_plan_clear(void) { odtk::lt::plan_clear(); }

int odtk_gemm_last_solution(int *origin) {
  std::lock_guard<std::mutex> lock(odtk::lt::mutex());
  if (origin) *origin = odtk::lt::last_solution()[1];
  return odtk::lt::last_solution()[0];
}

int odtk_debug_gemm_candidates(size_t m, int n, int k, int dtype, int relu, int residual, size_t workspace_size, int *indices,
                               int capacity) {
  if (m == 0 || n <= 0 || k <= 0 || capacity < 0 || (capacity > 0 && !indices)) return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  return odtk::lt::candidates(m, static_cast<uint32_t>(n), static_cast<uint32_t>(k), dtype, relu, residual, workspace_size,
                              indices, capacity);
}

int odtk_gemm_bias_act(void *y, const void *x, const void *w, const float *bias, const void *residual, size_t m,
                       int n, int k, int dtype, int relu, void *workspace, size_t workspace_size, void *stream) {
  if (!y || !x || !w || !bias || n <= 0 || k <= 0 || residual == y) return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) |
       reinterpret_cast<uintptr_t>(residual) | reinterpret_cast<uintptr_t>(workspace)) & 15u)
    return ODTK_ERR_INVALID;
  if (m == 0) return ODTK_OK;
  KernelTimer t(ODTK_KERNEL_GEMM, static_cast<hipStream_t>(stream));
  return odtk::lt::gemm_bias_act(y, x, w, bias, residual, m, static_cast<uint32_t>(n), static_cast<uint32_t>(k), dtype,
                                 relu, workspace, workspace_size, static_cast<hipStream_t>(stream));
}

}  // extern "C"
