// input.hip -- the input pipeline: odtk_preprocess_images (resize + flip + pad + normalise), odtk_augment_images,
// odtk_augment_images_ex (the same with a free rotation) and odtk_mosaic_images (four sources composed per canvas, pass M);
// odtk_tile_images (the tiler of tiled inference).
#include <cmath>
#include <cstring>

#include "runtime.hpp"
#include "preprocess.hpp"
#include "augment.hpp"
#include "mosaic.hpp"
#include "tile.hpp"

extern "C" {

// One axis of one image: the table (or the skipped pass) is consistent with the sizes and lies inside `tables`.
static bool preprocess_axis_ok(int32_t table, int32_t taps, int32_t in_size, int32_t out_size, size_t tables_len) {
  if (table < 0) return table == -1 && in_size == out_size;
  if (taps <= 0) return false;
  const unsigned long long need = 1ull * static_cast<uint32_t>(out_size) * (2ull + static_cast<uint32_t>(taps));
  return need < (1ull << 31) && static_cast<unsigned long long>(table) + need <= tables_len;
}

// The images of a batch against their buffers; `canvas` = false: the resized image is not held to height x width (it is turned later).
static int preprocess_images_ok(int batch_size, const odtk_image_t *images, size_t src_bytes, const int32_t *tables, size_t tables_len,
                                int height, int width, bool canvas) {
  for (int b = 0; b < batch_size; ++b) {
    const odtk_image_t &im = images[b];
    if (im.src_width <= 0 || im.src_height <= 0 || im.out_width <= 0 || im.out_height <= 0) return ODTK_ERR_INVALID;
    if (canvas && (im.out_width > width || im.out_height > height)) return ODTK_ERR_INVALID;
    if (im.mirror != 0 && im.mirror != 1) return ODTK_ERR_INVALID;
    if (im.src_pitch <= 0 || 3ll * im.src_width > im.src_pitch) return ODTK_ERR_INVALID;
    const unsigned long long extent = 1ull * (im.src_height - 1) * im.src_pitch + 3ull * im.src_width;   // 32-bit offsets inside one image
    if (extent >= (1ull << 31) || im.src_offset > src_bytes || extent > src_bytes - im.src_offset) return ODTK_ERR_INVALID;
    if ((im.x_table >= 0 || im.y_table >= 0) && !tables) return ODTK_ERR_INVALID;
    if (!preprocess_axis_ok(im.x_table, im.x_taps, im.src_width, im.out_width, tables_len) ||
        !preprocess_axis_ok(im.y_table, im.y_taps, im.src_height, im.out_height, tables_len))
      return ODTK_ERR_INVALID;
  }
  return ODTK_OK;
}

int odtk_preprocess_images(int batch_size, const odtk_image_t *images, const void *src, size_t src_bytes, const int32_t *tables,
                           size_t tables_len, const void *norm_table, void *out, int height, int width, int dtype, void *stream) {
  if (!images || !src || !norm_table || !out || batch_size <= 0 || height <= 0 || width <= 0) return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  const unsigned es = dtype == ODTK_F32 ? 4u : 2u;
  if ((reinterpret_cast<uintptr_t>(norm_table) | reinterpret_cast<uintptr_t>(out)) & (es - 1u)) return ODTK_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(tables) & 3u) return ODTK_ERR_INVALID;
  if (3ull * height * width >= (1ull << 31) || (height + odtk::kPreTileH - 1) / odtk::kPreTileH > 65535) return ODTK_ERR_INVALID;
  if (preprocess_images_ok(batch_size, images, src_bytes, tables, tables_len, height, width, true) != ODTK_OK) return ODTK_ERR_INVALID;
  static_assert(sizeof(odtk::PreArgs) <= 4096, "kernel arguments travel by value");
  odtk::PreArgs args;
  args.bytes = nullptr;
  args.sums = nullptr;
  args.slot = 0;
  args.src = static_cast<const uint8_t *>(src);
  args.tables = tables;
  args.norm = norm_table;
  args.out = out;
  args.height = height;
  args.width = width;
  args.vector_rows = ((3ull * width * es) % 16 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) ? 1 : 0;
  const dim3 tiles((width + odtk::kPreTileW - 1) / odtk::kPreTileW, (height + odtk::kPreTileH - 1) / odtk::kPreTileH);
  for (int first = 0; first < batch_size; first += odtk::kPreMaxImages) {   // one launch for batches of up to 64 images
    const int n = batch_size - first < odtk::kPreMaxImages ? batch_size - first : odtk::kPreMaxImages;
    args.first = first;
    std::memcpy(args.images, images + first, sizeof(odtk_image_t) * n);
    if (n < odtk::kPreMaxImages) std::memset(args.images + n, 0, sizeof(odtk_image_t) * (odtk::kPreMaxImages - n));
    const dim3 grid(tiles.x, tiles.y, static_cast<unsigned>(n));
    if (es == 4)
      hipLaunchKernelGGL(odtk::preprocess_images_kernel<4>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), args);
    else
      hipLaunchKernelGGL(odtk::preprocess_images_kernel<2>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), args);
    ODTK_HIP_TRY(hipGetLastError());
  }
  return ODTK_OK;
}

// odtk_augment_images (rotations == nullptr) and odtk_augment_images_ex.
static int augment_images(int batch_size, const odtk_image_t *images, const odtk_augment_t *augments, const odtk_rotation_t *rotations,
                          const void *src, size_t src_bytes, const int32_t *tables, size_t tables_len, const void *norm_table, void *out,
                          int height, int width, int dtype, void *workspace, size_t workspace_bytes, void *stream) {
  if (batch_size <= 0 || height <= 0 || width <= 0) return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  if (3ull * height * width >= (1ull << 31) || (height + odtk::kAugRows - 1) / odtk::kAugRows > 65535) return ODTK_ERR_INVALID;
  // workspace: one 64-bit sum per image | one slot per image for its resized bytes (as many pixels as the canvas at most)
  // | with rotations: one more slot per image for its finished canvas bytes
  const size_t slot = align_up(3ull * height * width), off_bytes = align_up(sizeof(unsigned long long) * batch_size);
  const size_t need = off_bytes + slot * batch_size * (rotations ? 2u : 1u);
  if (need > 0x7fffffffull) return ODTK_ERR_INVALID;
  if (!workspace) return static_cast<int>(need);
  if (!images || !augments || !src || !norm_table || !out) return ODTK_ERR_INVALID;
  if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return ODTK_ERR_INVALID;
  const unsigned es = dtype == ODTK_F32 ? 4u : 2u;
  if ((reinterpret_cast<uintptr_t>(norm_table) | reinterpret_cast<uintptr_t>(out)) & (es - 1u)) return ODTK_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(tables) & 3u) return ODTK_ERR_INVALID;
  if (preprocess_images_ok(batch_size, images, src_bytes, tables, tables_len, height, width, false) != ODTK_OK) return ODTK_ERR_INVALID;
  int32_t max_w = 0, max_h = 0;
  for (int b = 0; b < batch_size; ++b) {
    const odtk_image_t &im = images[b];
    const odtk_augment_t &au = augments[b];
    if (im.mirror != 0) return ODTK_ERR_INVALID;                  // the flip is part of the map
    if (3ull * im.out_width * im.out_height > slot) return ODTK_ERR_INVALID;
    if ((im.out_height + odtk::kPreTileH - 1) / odtk::kPreTileH > 65535) return ODTK_ERR_INVALID;
    if (au.canvas_width <= 0 || au.canvas_height <= 0 || au.canvas_width > width || au.canvas_height > height) return ODTK_ERR_INVALID;
    if (au.flags & ~(ODTK_AUGMENT_BRIGHTNESS | ODTK_AUGMENT_CONTRAST | ODTK_AUGMENT_HUE | ODTK_AUGMENT_SATURATION)) return ODTK_ERR_INVALID;
    if (au.pad_[0] | au.pad_[1] | au.pad_[2]) return ODTK_ERR_INVALID;
    if (((au.flags & ODTK_AUGMENT_BRIGHTNESS) && !std::isfinite(au.brightness)) || ((au.flags & ODTK_AUGMENT_CONTRAST) && !std::isfinite(au.contrast)) ||
        ((au.flags & ODTK_AUGMENT_SATURATION) && !std::isfinite(au.saturation)))
      return ODTK_ERR_INVALID;
    // the map is evaluated in 32-bit integers: it is affine, so its extremes over the canvas lie at the corners
    for (int axis = 0; axis < 2; ++axis)
      for (int corner = 0; corner < 4; ++corner) {
        const long long x = (corner & 1) ? au.canvas_width - 1 : 0, y = (corner & 2) ? au.canvas_height - 1 : 0;
        const long long px = 1ll * au.map[3 * axis] * x, py = 1ll * au.map[3 * axis + 1] * y;
        const long long limit = 0x7fffffffll;
        if (px > limit || px < -limit || py > limit || py < -limit) return ODTK_ERR_INVALID;
        const long long partial = au.map[3 * axis + 2] + px, v = partial + py;
        if (partial > limit || partial < -limit || v > limit || v < -limit) return ODTK_ERR_INVALID;
      }
    max_w = im.out_width > max_w ? im.out_width : max_w;
    max_h = im.out_height > max_h ? im.out_height : max_h;
    if (rotations) {
      const odtk_rotation_t &ro = rotations[b];
      if ((ro.enabled != 0 && ro.enabled != 1) || (ro.flip != 0 && ro.flip != 1) || (!ro.enabled && ro.flip)) return ODTK_ERR_INVALID;
      for (int k = 0; ro.enabled && k < 6; ++k)
        if (!std::isfinite(ro.matrix[k])) return ODTK_ERR_INVALID;
    }
  }
  static_assert(sizeof(odtk::PreArgs) <= 4096 && sizeof(odtk::AugArgs) <= 4096 && sizeof(odtk::RotArgs) <= 4096,
                "kernel arguments travel by value");
  hipStream_t s = static_cast<hipStream_t>(stream);
  odtk::PreArgs pre;
  pre.src = static_cast<const uint8_t *>(src);
  pre.tables = tables;
  pre.norm = nullptr;
  pre.out = nullptr;
  pre.height = max_h;
  pre.width = max_w;
  pre.vector_rows = 0;
  pre.bytes = static_cast<uint8_t *>(workspace) + off_bytes;
  pre.sums = static_cast<unsigned long long *>(workspace);
  pre.slot = slot;
  odtk::RotArgs rot;
  rot.bytes = pre.bytes;
  rot.canvas = pre.bytes + slot * batch_size;
  rot.slot = slot;
  rot.pad_ = 0;
  odtk::AugArgs aug;
  aug.bytes = rotations ? rot.canvas : pre.bytes;                 // passes B and C read the finished canvas, through the identity map
  aug.sums = pre.sums;
  aug.norm = norm_table;
  aug.out = out;
  aug.slot = slot;
  aug.height = height;
  aug.width = width;
  aug.vector_rows = ((3ull * width * es) % 16 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) ? 1 : 0;
  const unsigned group = 16u * (16u / es);                        // pixels per workgroup row of pass C
  for (int first = 0; first < batch_size; first += odtk::kPreMaxImages) {   // one chain for batches of up to 64 images
    const int n = batch_size - first < odtk::kPreMaxImages ? batch_size - first : odtk::kPreMaxImages;
    pre.first = aug.first = first;
    std::memset(pre.images, 0, sizeof(pre.images));
    std::memcpy(pre.images, images + first, sizeof(odtk_image_t) * n);
    std::memset(aug.images, 0, sizeof(aug.images));
    bool contrast = false;
    for (int i = 0; i < n; ++i) {
      const odtk_augment_t &au = augments[first + i];
      odtk::AugImage &d = aug.images[i];
      d.cw = au.canvas_width;
      d.ch = au.canvas_height;
      d.rw = images[first + i].out_width;
      d.rh = images[first + i].out_height;
      std::memcpy(d.map, au.map, sizeof(d.map));
      if (rotations) {
        const int32_t identity[6] = {65536, 0, 0, 0, 65536, 0};
        d.rw = au.canvas_width;
        d.rh = au.canvas_height;
        std::memcpy(d.map, identity, sizeof(d.map));
      }
      d.flags = au.flags;
      d.brightness = au.brightness;
      d.contrast = au.contrast;
      d.saturation = au.saturation;
      d.hue = au.hue;
      contrast = contrast || (au.flags & ODTK_AUGMENT_CONTRAST);
    }
    const dim3 tiles((max_w + odtk::kPreTileW - 1) / odtk::kPreTileW, (max_h + odtk::kPreTileH - 1) / odtk::kPreTileH, static_cast<unsigned>(n));
    hipLaunchKernelGGL((odtk::preprocess_images_kernel<4, true>), tiles, dim3(256), 0, s, pre);
    ODTK_HIP_TRY(hipGetLastError());
    for (int at = 0; rotations && at < n; at += odtk::kRotMaxImages) {   // its descriptors are larger: up to two launches
      const int m = n - at < odtk::kRotMaxImages ? n - at : odtk::kRotMaxImages;
      rot.first = first + at;
      std::memset(rot.images, 0, sizeof(rot.images));
      unsigned long long pixels = 0;
      for (int i = 0; i < m; ++i) {
        const odtk_augment_t &au = augments[first + at + i];
        const odtk_rotation_t &ro = rotations[first + at + i];
        odtk::RotImage &d = rot.images[i];
        std::memcpy(d.m, ro.matrix, sizeof(d.m));
        d.cw = au.canvas_width;
        d.ch = au.canvas_height;
        d.rw = images[first + at + i].out_width;
        d.rh = images[first + at + i].out_height;
        std::memcpy(d.map, au.map, sizeof(d.map));
        d.enabled = ro.enabled;
        d.flip = ro.flip;
        const unsigned long long count = 1ull * au.canvas_width * au.canvas_height;
        pixels = count > pixels ? count : pixels;
      }
      const unsigned per_group = 256u * odtk::kRotPixels;
      hipLaunchKernelGGL(odtk::augment_rotate_kernel, dim3(static_cast<unsigned>((pixels + per_group - 1) / per_group), 1, static_cast<unsigned>(m)),
                         dim3(256), 0, s, rot);
      ODTK_HIP_TRY(hipGetLastError());
    }
    if (contrast) {
      hipLaunchKernelGGL(odtk::augment_luma_sum_kernel, dim3(odtk::kAugSumBlocks, 1, static_cast<unsigned>(n)), dim3(256), 0, s, aug);
      ODTK_HIP_TRY(hipGetLastError());
    }
    const dim3 grid((width + group - 1) / group, (height + odtk::kAugRows - 1) / odtk::kAugRows, static_cast<unsigned>(n));
    if (es == 4)
      hipLaunchKernelGGL(odtk::augment_images_kernel<4>, grid, dim3(256), 0, s, aug);
    else
      hipLaunchKernelGGL(odtk::augment_images_kernel<2>, grid, dim3(256), 0, s, aug);
    ODTK_HIP_TRY(hipGetLastError());
  }
  return ODTK_OK;
}

int odtk_augment_images(int batch_size, const odtk_image_t *images, const odtk_augment_t *augments, const void *src, size_t src_bytes,
                        const int32_t *tables, size_t tables_len, const void *norm_table, void *out, int height, int width, int dtype,
                        void *workspace, size_t workspace_bytes, void *stream) {
  return augment_images(batch_size, images, augments, nullptr, src, src_bytes, tables, tables_len, norm_table, out, height, width, dtype,
                        workspace, workspace_bytes, stream);
}

int odtk_augment_images_ex(int batch_size, const odtk_image_t *images, const odtk_augment_t *augments, const odtk_rotation_t *rotations,
                           const void *src, size_t src_bytes, const int32_t *tables, size_t tables_len, const void *norm_table, void *out,
                           int height, int width, int dtype, void *workspace, size_t workspace_bytes, void *stream) {
  return augment_images(batch_size, images, augments, rotations, src, src_bytes, tables, tables_len, norm_table, out, height, width, dtype,
                        workspace, workspace_bytes, stream);
}

// Mosaic: passes A (over the sources), M (mosaic.hpp), B and C (augment.hpp, through the identity map).
int odtk_mosaic_images(int batch_size, const odtk_mosaic_t *mosaics, const odtk_augment_t *augments, int n_images,
                       const odtk_image_t *images, int max_pixels, const void *src, size_t src_bytes, const int32_t *tables,
                       size_t tables_len, const void *norm_table, void *out, int height, int width, int dtype, void *workspace,
                       size_t workspace_bytes, void *stream) {
  if (batch_size <= 0 || n_images <= 0 || max_pixels <= 0 || height <= 0 || width <= 0) return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  if (3ull * height * width >= (1ull << 31) || (height + odtk::kAugRows - 1) / odtk::kAugRows > 65535) return ODTK_ERR_INVALID;
  if (3ull * max_pixels >= (1ull << 31)) return ODTK_ERR_INVALID;
  // workspace: one 64-bit word per output image or source, whichever are more (pass A zeroes one per source, pass M the sum of
  // every output image) | one slot per source for its resized bytes | one slot per output image for its finished canvas bytes
  const size_t src_slot = align_up(3ull * max_pixels), canvas_slot = align_up(3ull * height * width);
  const size_t off_bytes = align_up(sizeof(unsigned long long) * (batch_size > n_images ? batch_size : n_images));
  const unsigned long long need = 1ull * off_bytes + 1ull * src_slot * n_images + 1ull * canvas_slot * batch_size;
  if (need > 0x7fffffffull) return ODTK_ERR_INVALID;
  if (!workspace) return static_cast<int>(need);
  if (!mosaics || !images || !src || !norm_table || !out) return ODTK_ERR_INVALID;
  if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return ODTK_ERR_INVALID;
  const unsigned es = dtype == ODTK_F32 ? 4u : 2u;
  if ((reinterpret_cast<uintptr_t>(norm_table) | reinterpret_cast<uintptr_t>(out)) & (es - 1u)) return ODTK_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(tables) & 3u) return ODTK_ERR_INVALID;
  if (preprocess_images_ok(n_images, images, src_bytes, tables, tables_len, height, width, false) != ODTK_OK) return ODTK_ERR_INVALID;
  int32_t max_w = 0, max_h = 0;
  for (int s = 0; s < n_images; ++s) {
    const odtk_image_t &im = images[s];
    if (1ull * im.out_width * im.out_height > static_cast<unsigned long long>(max_pixels)) return ODTK_ERR_INVALID;
    if ((im.out_height + odtk::kPreTileH - 1) / odtk::kPreTileH > 65535) return ODTK_ERR_INVALID;
    max_w = im.out_width > max_w ? im.out_width : max_w;
    max_h = im.out_height > max_h ? im.out_height : max_h;
  }
  for (int b = 0; b < batch_size; ++b) {
    const odtk_mosaic_t &mo = mosaics[b];
    if (mo.canvas_width <= 0 || mo.canvas_height <= 0 || mo.canvas_width > width || mo.canvas_height > height || mo.pad_) return ODTK_ERR_INVALID;
    for (int k = 0; k < 4; ++k) {
      const odtk_mosaic_tile_t &t = mo.tiles[k];
      if (t.source < -1 || t.source >= n_images) return ODTK_ERR_INVALID;
      if (t.source < 0) continue;
      if (t.width <= 0 || t.height <= 0 || t.dst_x < 0 || t.dst_y < 0 || t.src_x < 0 || t.src_y < 0) return ODTK_ERR_INVALID;
      if (1ll * t.dst_x + t.width > mo.canvas_width || 1ll * t.dst_y + t.height > mo.canvas_height) return ODTK_ERR_INVALID;
      if (1ll * t.src_x + t.width > images[t.source].out_width || 1ll * t.src_y + t.height > images[t.source].out_height) return ODTK_ERR_INVALID;
    }
    if (!augments) continue;
    const odtk_augment_t &au = augments[b];
    const int32_t identity[6] = {65536, 0, 0, 0, 65536, 0};
    if (au.canvas_width != mo.canvas_width || au.canvas_height != mo.canvas_height || std::memcmp(au.map, identity, sizeof identity)) return ODTK_ERR_INVALID;
    if (au.flags & ~(ODTK_AUGMENT_BRIGHTNESS | ODTK_AUGMENT_CONTRAST | ODTK_AUGMENT_HUE | ODTK_AUGMENT_SATURATION)) return ODTK_ERR_INVALID;
    if (au.pad_[0] | au.pad_[1] | au.pad_[2]) return ODTK_ERR_INVALID;
    if (((au.flags & ODTK_AUGMENT_BRIGHTNESS) && !std::isfinite(au.brightness)) || ((au.flags & ODTK_AUGMENT_CONTRAST) && !std::isfinite(au.contrast)) ||
        ((au.flags & ODTK_AUGMENT_SATURATION) && !std::isfinite(au.saturation)))
      return ODTK_ERR_INVALID;
  }
  static_assert(sizeof(odtk::MosArgs) <= 4096, "kernel arguments travel by value");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // A: the sources, 64 per launch
  odtk::PreArgs pre;
  pre.src = static_cast<const uint8_t *>(src);
  pre.tables = tables;
  pre.norm = nullptr;
  pre.out = nullptr;
  pre.height = max_h;
  pre.width = max_w;
  pre.vector_rows = 0;
  pre.bytes = static_cast<uint8_t *>(workspace) + off_bytes;
  pre.sums = static_cast<unsigned long long *>(workspace);
  pre.slot = src_slot;
  for (int first = 0; first < n_images; first += odtk::kPreMaxImages) {
    const int n = n_images - first < odtk::kPreMaxImages ? n_images - first : odtk::kPreMaxImages;
    pre.first = first;
    std::memset(pre.images, 0, sizeof(pre.images));
    std::memcpy(pre.images, images + first, sizeof(odtk_image_t) * n);
    const dim3 tiles((max_w + odtk::kPreTileW - 1) / odtk::kPreTileW, (max_h + odtk::kPreTileH - 1) / odtk::kPreTileH, static_cast<unsigned>(n));
    hipLaunchKernelGGL((odtk::preprocess_images_kernel<4, true>), tiles, dim3(256), 0, s, pre);
    ODTK_HIP_TRY(hipGetLastError());
  }
  // M: the canvases, 16 per launch
  odtk::MosArgs mos;
  mos.bytes = pre.bytes;
  mos.canvas = pre.bytes + src_slot * n_images;
  mos.sums = pre.sums;
  mos.src_slot = src_slot;
  mos.canvas_slot = canvas_slot;
  mos.pad_ = 0;
  for (int first = 0; first < batch_size; first += odtk::kMosMaxImages) {
    const int n = batch_size - first < odtk::kMosMaxImages ? batch_size - first : odtk::kMosMaxImages;
    mos.first = first;
    std::memset(mos.images, 0, sizeof(mos.images));                 // (an all-zero tile is unused: x1 <= x0)
    unsigned long long pixels = 0;
    for (int i = 0; i < n; ++i) {
      const odtk_mosaic_t &mo = mosaics[first + i];
      odtk::MosImage &d = mos.images[i];
      d.cw = mo.canvas_width;
      d.ch = mo.canvas_height;
      d.fill = static_cast<uint32_t>(mo.fill[0]) | (static_cast<uint32_t>(mo.fill[1]) << 8) | (static_cast<uint32_t>(mo.fill[2]) << 16);
      for (int k = 0; k < 4; ++k) {
        const odtk_mosaic_tile_t &t = mo.tiles[k];
        if (t.source < 0) continue;
        odtk::MosTile &m = d.tiles[k];
        m.x0 = t.dst_x;
        m.y0 = t.dst_y;
        m.x1 = t.dst_x + t.width;
        m.y1 = t.dst_y + t.height;
        m.ox = t.src_x - t.dst_x;
        m.oy = t.src_y - t.dst_y;
        m.rw = images[t.source].out_width;
        m.source = t.source;
      }
      const unsigned long long count = 1ull * mo.canvas_width * mo.canvas_height;
      pixels = count > pixels ? count : pixels;
    }
    const unsigned per_group = 256u * odtk::kMosPixels;
    hipLaunchKernelGGL(odtk::mosaic_compose_kernel, dim3(static_cast<unsigned>((pixels + per_group - 1) / per_group), 1, static_cast<unsigned>(n)),
                       dim3(256), 0, s, mos);
    ODTK_HIP_TRY(hipGetLastError());
  }
  // B, C: the finished canvases through the identity map, 64 per launch
  odtk::AugArgs aug;
  aug.bytes = mos.canvas;
  aug.sums = pre.sums;
  aug.norm = norm_table;
  aug.out = out;
  aug.slot = canvas_slot;
  aug.height = height;
  aug.width = width;
  aug.vector_rows = ((3ull * width * es) % 16 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) ? 1 : 0;
  const unsigned group = 16u * (16u / es);                        // pixels per workgroup row of pass C
  for (int first = 0; first < batch_size; first += odtk::kPreMaxImages) {
    const int n = batch_size - first < odtk::kPreMaxImages ? batch_size - first : odtk::kPreMaxImages;
    aug.first = first;
    std::memset(aug.images, 0, sizeof(aug.images));
    bool contrast = false;
    for (int i = 0; i < n; ++i) {
      const odtk_mosaic_t &mo = mosaics[first + i];
      odtk::AugImage &d = aug.images[i];
      d.cw = d.rw = mo.canvas_width;
      d.ch = d.rh = mo.canvas_height;
      d.map[0] = d.map[4] = 65536;
      d.brightness = d.contrast = d.saturation = 1.0f;
      if (augments) {
        const odtk_augment_t &au = augments[first + i];
        d.flags = au.flags;
        d.brightness = au.brightness;
        d.contrast = au.contrast;
        d.saturation = au.saturation;
        d.hue = au.hue;
        contrast = contrast || (au.flags & ODTK_AUGMENT_CONTRAST);
      }
    }
    if (contrast) {
      hipLaunchKernelGGL(odtk::augment_luma_sum_kernel, dim3(odtk::kAugSumBlocks, 1, static_cast<unsigned>(n)), dim3(256), 0, s, aug);
      ODTK_HIP_TRY(hipGetLastError());
    }
    const dim3 grid((width + group - 1) / group, (height + odtk::kAugRows - 1) / odtk::kAugRows, static_cast<unsigned>(n));
    if (es == 4)
      hipLaunchKernelGGL(odtk::augment_images_kernel<4>, grid, dim3(256), 0, s, aug);
    else
      hipLaunchKernelGGL(odtk::augment_images_kernel<2>, grid, dim3(256), 0, s, aug);
    ODTK_HIP_TRY(hipGetLastError());
  }
  return ODTK_OK;
}

// everything is validated here, on the host, before anything touches the device
int odtk_tile_images(const void *x, void *out, int batch, int channels, int height, int width, int dtype, int channels_last,
                     int n_tiles, const odtk_tile_t *tiles, int tile_h, int tile_w, void *stream) {
  if (!x || !out || !tiles || n_tiles < 1 || n_tiles > ODTK_MAX_TILES || channels < 1 || channels > 16) return ODTK_ERR_INVALID;
  if (batch <= 0 || height <= 0 || width <= 0 || tile_h <= 0 || tile_w <= 0) return ODTK_ERR_INVALID;
  if (channels_last != 0 && channels_last != 1) return ODTK_ERR_INVALID;
  for (int i = 0; i < n_tiles; ++i)
    if (tiles[i].image >= batch || tiles[i].x < 0 || tiles[i].y < 0) return ODTK_ERR_INVALID;
  if (dtype != ODTK_F32 && dtype != ODTK_BF16 && dtype != ODTK_F16) return ODTK_ERR_UNSUPPORTED;
  const unsigned es = dtype == ODTK_F32 ? 4u : 2u;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & (es - 1u)) return ODTK_ERR_INVALID;
  const unsigned long long per_tile = 1ull * channels * tile_h * tile_w;          // 32-bit offsets inside one tile and one image
  if (per_tile > 0xf0000000ull || 1ull * channels * height * width > 0xffffffffull) return ODTK_ERR_INVALID;
  static_assert(sizeof(odtk::TileArgs) <= 4096, "kernel arguments travel by value");
  odtk::TileArgs args;
  std::memset(&args, 0, sizeof args);
  args.x = x;
  args.out = out;
  args.channels = static_cast<uint32_t>(channels);
  args.height = static_cast<uint32_t>(height);
  args.width = static_cast<uint32_t>(width);
  args.tile_h = static_cast<uint32_t>(tile_h);
  args.tile_w = static_cast<uint32_t>(tile_w);
  args.per_tile = static_cast<uint32_t>(per_tile);
  args.inner = odtk::fastdiv_make(channels_last ? args.channels : args.tile_w);
  args.middle = odtk::fastdiv_make(channels_last ? args.tile_w : args.tile_h);
  std::memcpy(args.tiles, tiles, sizeof(odtk_tile_t) * n_tiles);
  unsigned long long blocks = (per_tile + odtk::kTileThreads * 4ull - 1) / (odtk::kTileThreads * 4ull);     // ~4 elements per lane
  if (blocks > 4096) blocks = 4096;
  const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(n_tiles)), block(odtk::kTileThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (es == 4 && channels_last) timed_launch(ODTK_KERNEL_EPILOGUE, odtk::tile_images_kernel<uint32_t, true>, grid, block, 0, s, args);
  else if (es == 4) timed_launch(ODTK_KERNEL_EPILOGUE, odtk::tile_images_kernel<uint32_t, false>, grid, block, 0, s, args);
  else if (channels_last) timed_launch(ODTK_KERNEL_EPILOGUE, odtk::tile_images_kernel<uint16_t, true>, grid, block, 0, s, args);
  else timed_launch(ODTK_KERNEL_EPILOGUE, odtk::tile_images_kernel<uint16_t, false>, grid, block, 0, s, args);
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

}  // extern "C"
