"""The index functions of the head towers' 3x3 convolution kernel (csrc/tower_conv_layout.hpp), checked exhaustively on the host:
the header is plain C++ on both sides, so a stand-alone program compiled here walks every lane, piece, fragment and K-tile.

  * the pieces one tile's LDS-DMA loads write (wave-uniform base + lane * 16, as the instruction defines its destination) form a
    permutation of the operand's 32 KiB image, and each piece holds the (row, logical chunk) its source address was computed for;
  * every fragment read (ds_read_b128 of lane l, row block, k-step) returns the (row, k) the MFMA 16x16x32 expects: row l % 16 of
    the block, k = 32 kk + 8 (l / 16) .. + 7 -- read through the image the pieces wrote;
  * the same for the 32x32x16 form, whose lane halves read the chunks in the grouping of the library's instance;
  * the 16 lanes of each hardware lane group of ds_read_b128 hit 16 different 16-byte slots of the 256-byte bank row;
  * K-tile kt is tap kt / 4, channels (kt % 4) * 64: the 36 tiles cover K = 2304 once, in order;
  * the tap mask equals a brute-force bounds test, and pixel_of the division, for every pixel of the extents the GPU test runs;
  * the epilogue's image: the accumulator registers of the 8 waves write every 8-byte unit of the 128 KiB tile exactly once, and the
    row-order read-back finds 8 consecutive channels of one pixel in each 16-byte unit.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'retinanet-examples_amd', 'csrc', 'tower_conv_layout.hpp')
EXTENTS = [(1, 1, 1), (1, 1, 40), (1, 40, 1), (2, 3, 5), (2, 9, 31), (3, 16, 16), (2, 17, 33), (1, 2, 300), (8, 8, 8)]

PROGRAM = r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include "%s"
using namespace odtk::tower;

int main() {
  long bad = 0, checked = 0;
  // ---- the LDS image of one operand tile: what (row, logical chunk) lies at each 16-byte slot ---------------------------------
  std::vector<int> slot_row(kOperandBytes / 16, -1), slot_chunk(kOperandBytes / 16, -1);
  for (uint32_t i = 0; i < 4; ++i)
    for (uint32_t tid = 0; tid < kThreads; ++tid) {
      const uint32_t wave = tid >> 6, lane = tid & 63u;
      const uint32_t dst = piece_wave_base(i, wave) + lane * 16u;          // the hardware's rule
      ++checked;
      if (dst != piece_dst(i, tid) || dst %% 16u || dst >= kOperandBytes) { ++bad; continue; }
      if (slot_row[dst / 16] != -1) ++bad;                                  // written twice
      slot_row[dst / 16] = piece_row(i, tid);
      slot_chunk[dst / 16] = piece_chunk(tid);
      // one wave instruction: 8 whole rows
      if (piece_row(i, tid) / 8 != piece_row(i, tid & ~63u) / 8) ++bad;
    }
  for (size_t s = 0; s < slot_row.size(); ++s) { ++checked; if (slot_row[s] < 0) ++bad; }
  {                                                                          // every (row, chunk) exactly once
    std::vector<int> seen(256 * 8, 0);
    for (size_t s = 0; s < slot_row.size(); ++s) if (slot_row[s] >= 0) ++seen[slot_row[s] * 8 + slot_chunk[s]];
    for (int v : seen) { ++checked; if (v != 1) ++bad; }
  }
  // ---- fragment reads ------------------------------------------------------------------------------------------------------------
  for (uint32_t block = 0; block < 16; ++block)
    for (uint32_t kk = 0; kk < 2; ++kk) {
      uint32_t slots[64];
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t a = frag_addr(block, kk, lane);
        ++checked;
        if (a %% 16u || a >= kOperandBytes) { ++bad; continue; }
        const int row = slot_row[a / 16], chunk = slot_chunk[a / 16];
        // the MFMA's map: row lane %% 16 of the block, k = 32 kk + 8 (lane / 16) + 0..7, i.e. logical chunk 4 kk + lane / 16
        if (row != (int)(block * 16 + (lane & 15u)) || chunk != (int)(4 * kk + (lane >> 4))) ++bad;
        slots[lane] = (a / 16u) %% 16u;
      }
      // lane groups of ds_read_b128: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, and the same + 32
      for (uint32_t g = 0; g < 4; ++g) {
        uint32_t used = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint32_t l = lane & 31u;
          const bool first = l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28);
          if ((lane >> 5) * 2 + (first ? 0 : 1) != g) continue;
          used |= 1u << slots[lane];
        }
        ++checked;
        if (used != 0xffffu) ++bad;
      }
    }
  // ---- fragment reads of the 32x32x16 form: row lane %% 32 of the block; over the four steps of a K-tile each lane half reads every
  // chunk of its two 16-deep halves of each 32-deep block once: step 2 blk + r -> chunk 4 blk + 2 h + r --------------------------
  for (uint32_t block = 0; block < 8; ++block) {
    for (uint32_t lane = 0; lane < 64; ++lane) {
      uint32_t seen = 0;
      for (uint32_t step = 0; step < 4; ++step) {
        const uint32_t a = frag32_addr(block, step, lane);
        ++checked;
        if (a %% 16u || a >= kOperandBytes) { ++bad; continue; }
        const int row = slot_row[a / 16], chunk = slot_chunk[a / 16];
        const uint32_t want = (step >> 1) * 4 + 2 * (lane >> 5) + (step & 1);
        if (row != (int)(block * 32 + (lane & 31u)) || chunk != (int)want || chunk != (int)frag32_chunk(step, lane)) ++bad;
        seen |= 1u << chunk;
      }
      // the two halves of a wave together cover the tile's eight chunks once
      if (seen != ((lane >> 5) ? 0xccu : 0x33u)) ++bad;
    }
    for (uint32_t step = 0; step < 4; ++step)
      for (uint32_t g = 0; g < 4; ++g) {                                     // the same lane groups, conflict-free
        uint32_t used = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint32_t l = lane & 31u;
          const bool first = l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28);
          if ((lane >> 5) * 2 + (first ? 0 : 1) != g) continue;
          used |= 1u << ((frag32_addr(block, step, lane) / 16u) %% 16u);
        }
        ++checked;
        if (used != 0xffffu) ++bad;
      }
  }
  // ---- K order -------------------------------------------------------------------------------------------------------------------
  for (uint32_t kt = 0; kt < kKTiles; ++kt) {
    ++checked;
    if (ktile_tap(kt) * kChannels + ktile_channel(kt) != kt * kBK) ++bad;
  }
  if (kKTiles * kBK != 9 * 256) ++bad;
  // ---- pixel decomposition and tap mask against brute force --------------------------------------------------------------------
  const int extents[][3] = {%s};
  for (const auto &e : extents) {
    const uint32_t n = e[0], h = e[1], w = e[2];
    const odtk::FastDiv by_w = odtk::fastdiv_make(w), by_hw = odtk::fastdiv_make(h * w);
    for (uint32_t p = 0; p < n * h * w; ++p) {
      const Pixel q = pixel_of(p, by_w, by_hw);
      ++checked;
      if (q.n != p / (h * w) || q.y != p %% (h * w) / w || q.x != p %% w) { ++bad; continue; }
      const uint32_t mask = tap_mask(q.y, q.x, h, w);
      for (uint32_t t = 0; t < 9; ++t) {
        const int yy = (int)q.y + (int)(t / 3) - 1, xx = (int)q.x + (int)(t %% 3) - 1;
        const bool inside = yy >= 0 && yy < (int)h && xx >= 0 && xx < (int)w;
        ++checked;
        if (((mask >> t) & 1u) != (inside ? 1u : 0u)) ++bad;
        // an inside tap's source is that pixel of the same image
        if (inside && (long)p + tap_pixel_offset(t, w) != (long)((q.n * h + yy) * w + xx)) ++bad;
      }
      if (mask >> 9) ++bad;
    }
  }
  // ---- the epilogue's image ------------------------------------------------------------------------------------------------------
  {
    std::vector<int> unit_pixel(kLdsBytes / 8, -1), unit_channel(kLdsBytes / 8, -1);
    for (uint32_t wave = 0; wave < 8; ++wave)
      for (uint32_t n = 0; n < 4; ++n)
        for (uint32_t b = 0; b < 8; ++b)
          for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t wr = wave >> 2, wc = wave & 3u;
            const uint32_t pixel = acc_pixel(wr * 8 + b, lane), channel = acc_channel(wc * 4 + n, lane, 0);
            const uint32_t at = out_addr(pixel, channel);
            ++checked;
            if (at %% 8u || at >= kLdsBytes || pixel >= 256 || channel + 3 >= 256 + 3) { ++bad; continue; }
            if (unit_pixel[at / 8] != -1) ++bad;
            unit_pixel[at / 8] = pixel;
            unit_channel[at / 8] = channel;
          }
    // the 32x32 form writes the same image: every 8-byte unit once, the same (pixel, channel) in it
    std::vector<int> hit(kLdsBytes / 8, 0);
    for (uint32_t wave = 0; wave < 8; ++wave)
      for (uint32_t n = 0; n < 2; ++n)
        for (uint32_t b = 0; b < 4; ++b)
          for (uint32_t g = 0; g < 4; ++g)
            for (uint32_t lane = 0; lane < 64; ++lane) {
              const uint32_t wr = wave >> 2, wc = wave & 3u;
              const uint32_t pixel = acc32_pixel(wr * 4 + b, lane), channel = acc32_channel(wc * 2 + n, lane, 4 * g);
              const uint32_t at = out_addr(pixel, channel);
              ++checked;
              if (at %% 8u || at >= kLdsBytes || (channel & 3u)) { ++bad; continue; }
              for (uint32_t e = 1; e < 4; ++e) if (acc32_channel(wc * 2 + n, lane, 4 * g + e) != channel + e) ++bad;
              if (unit_pixel[at / 8] != (int)pixel || unit_channel[at / 8] != (int)channel || hit[at / 8]++) ++bad;
            }
    for (int v : hit) if (v != 1) ++bad;
    for (uint32_t it = 0; it < 16; ++it)
      for (uint32_t tid = 0; tid < kThreads; ++tid) {
        const uint32_t q = it * kThreads + tid, pixel = it * 16 + (tid >> 5), chunk = out_chunk(tid >> 5, tid & 31u);
        ++checked;
        // the kernel computes the logical chunk once, from trip 0's pixel
        if (chunk != out_chunk(pixel, tid & 31u) || q / 32 != pixel) ++bad;
        for (uint32_t half = 0; half < 2; ++half)
          if (unit_pixel[q * 2 + half] != (int)pixel || unit_channel[q * 2 + half] != (int)(chunk * 8 + half * 4)) ++bad;
      }
  }
  std::printf("checked=%%ld bad=%%ld\n", checked, bad);
  return bad ? 1 : 0;
}
'''


def test_layout_functions_hold_for_every_lane_piece_fragment_and_pixel(tmp_path):
    src = tmp_path / 'layout.cpp'
    src.write_text(PROGRAM % (HEADER, ', '.join('{%d, %d, %d}' % e for e in EXTENTS)))
    exe = tmp_path / 'layout'
    subprocess.run(['g++', '-O1', '-std=c++17', '-o', str(exe), str(src)], check=True, timeout=120)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    fields = dict(f.split('=') for f in run.stdout.split())
    assert int(fields['bad']) == 0 and int(fields['checked']) > 50000, run.stdout
