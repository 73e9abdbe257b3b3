// select_decode.hpp -- kernel 2 of the decode path: per (level, image) segment, pick the top_n candidates
// (score desc, flat index asc) out of the prefilter's per-wave candidate sub-lists, sort them in LDS and decode
// their boxes.  ONE launch (round 4; rounds 2-3 ran a histogram launch and a filter launch in front of it).
//
// Replaces reference steps D4-D6 (csrc/cuda/decode.cu:108-167: gather + cub radix sort of all
// survivors, the box-decode device lambda, the tail fills) for all images and levels at once.
// Box arithmetic follows odtk/box.py:97-111 + :302 operation by operation (CPU path is
// normative: two-sided clamp).
//
// Selection is exact for ANY input and needs no state prepared by another launch:
//   * every workgroup of a segment adds up the segment's sub-list lengths (one coalesced read) and derives the SAME
//     number G of workgroups that take part: 1 up to kKeysPerPart candidates -- the normal case; the other workgroups
//     the host provided leave at once --, more for dense inputs or when a sub-list overflowed (kListOverflow: that
//     span is re-read from the raw scores, keys rebuilt on the fly, so list capacity never decides a result).
//   * G == 1: the workgroup walks all sub-lists (16 lanes per sub-list, 4 sub-lists = one span per wave instruction,
//     8 independent loads in flight per lane).  <= LDS sort capacity: everything is gathered and sorted.  More: a
//     threshold T with top_n <= #{key >= T} <= capacity comes from histogram passes over 2048 EQUAL bins of the
//     current key range (select_threshold; normally one pass: fp32 scores of one image share their exponent bits, a
//     linear digit over [key(thresh), key(1.0)] separates what an 11-bit MSD digit cannot; the range is clipped to
//     [min key, max key] between passes, so saturated scores go straight to the index bits), then one gather pass.
//   * G > 1 (tournament): workgroup g walks the spans s = g (mod G), keeps its LOCAL top `budget` >= top_n keys --
//     any key of the global top_n is in its slice's top_n -- and appends them to the segment's survivor list (one
//     returning atomic per workgroup); the workgroup that takes the last ticket (SelSeg::arrived; nobody waits)
//     selects among the <= G * budget survivors.
//   * the selected keys are narrowed to the smallest sortable size in LDS, sorted (bitonic, keys in registers, only
//     the cross-wave stages through LDS) and decoded.
// Keys are unique (they embed the index), so "keys >= T" is exactly top_n elements even when every score is equal.
#pragma once

#include "common.hpp"
#include "prefilter.hpp"
#include "../../include/odtk_hip.h"

namespace odtk {

constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / kWave;
constexpr int kSortCap = 4096;                  // keys sortable in LDS by the standard kernel (32 KiB)
constexpr int kSortCapBig = ODTK_MAX_TOP_N;     // ... by the top_n > 4096 variant (128 KiB of dynamic LDS)
constexpr int kRadixBits = 11;
constexpr int kRadixBins = 1 << kRadixBits;
constexpr uint32_t kKeysPerPart = 3072;         // candidates per workgroup: a slice then nearly always fits the sort buffer whole
constexpr uint32_t kCntSlots = 2048;            // sub-list lengths a workgroup keeps in LDS (512 spans)
constexpr uint32_t kSpansPerPart = 44;          // host: workgroups provided per segment = ceil(spans / this), <= kMaxParts
constexpr uint32_t kMaxParts = 64;
constexpr uint32_t kMaxInBin = 640;              // rank-by-counting: keys one histogram bin may hold ...
constexpr uint32_t kMaxInBinSquares = 500000;    // ... and the sum over the bins of their squared counts = in-bin comparisons (more: plateaus -> the rank-merge sort)
constexpr int kHistCopies = 4;                  // sub-histograms of select_threshold (standard kernel): lane l adds to copy l % 4

// LDS carve-up of select_decode_kernel (one dynamic allocation: more than the 64 KiB a kernel may declare statically)
template <int CAP>
struct SelLds {
  static constexpr int copies = CAP <= kSortCap ? kHistCopies : 1;       // (the 128 KiB sort buffer leaves room for one)
  static constexpr size_t keys = 0;
  static constexpr size_t hist = keys + sizeof(uint64_t) * CAP;
  static constexpr size_t cnt = hist + sizeof(uint32_t) * kRadixBins * copies;
  static constexpr size_t raw = cnt + sizeof(uint32_t) * kCntSlots;
  static constexpr size_t total = raw + sizeof(uint16_t) * (kCntSlots / kScanWaves);
};

struct DecodeLevel {
  const void *cls;
  const void *box;
  uint64_t key_off;      // first key of this level's span regions in the candidate pool
  uint64_t surv_off;     // first key of this level's survivor lists (parts * budget keys per segment)
  uint32_t cnt_off;      // first sub-list length of this level
  uint32_t n;            // A*C*H*W
  uint32_t spans;        // spans per image
  int32_t height, width;
  float stride;
  uint32_t channels_last;
  uint32_t pad_;
  const float *cls_bias; // [A*C] added to the cls head values (logits) before the sigmoid, or null
  const float *box_bias; // [A*NB] added to the gathered deltas, or null
  float anchors[ODTK_MAX_ANCHORS * 4];
};

struct DecodeArgs {
  DecodeLevel lv[ODTK_MAX_LEVELS];
  uint32_t part_begin[ODTK_MAX_LEVELS + 1];   // first workgroup of each level
  uint32_t parts[ODTK_MAX_LEVELS];            // workgroups provided per segment of that level (>= 1)
  SelSeg *sel;                                // [n_levels * batch], zeroed by the prefilter
  uint64_t *surv;                             // survivor lists (tournament route)
  const uint32_t *counts;                     // sub-list lengths written by the prefilter
  const uint64_t *cand;                       // candidate pool
  uint32_t budget;                            // keys a workgroup of the tournament route may pass on (>= top_n, <= sort capacity)
  uint32_t span_elems;                        // elements per span
  uint32_t aligned;                           // every image of every level starts on a 16-byte boundary (vector loads of raw spans)
  uint32_t coop_ticks;                        // cooperative route: 100 MHz ticks a workgroup waits for its segment's partners (0: route off)
  uint32_t rank_sort;                         // order the selected keys by COUNTING (histogram bases + in-bin ranks) and decode each where it lies; 0: the rank-merge sort (A/B)
  float raw_lo;                               // logits: conservative lower bound of a candidate's logit (as the prefilter's)
  FastDiv by_channels;                        // A*C
  float *out_scores;     // [batch, n_levels*top_n]
  float *out_boxes;      // [batch, n_levels*top_n, NB]
  float *out_classes;    // [batch, n_levels*top_n]
  int32_t *out_indices;  // optional
  uint32_t *run_valid;   // optional [batch, n_levels]: emitted entries with score > 0 of every (image, level) list (nms sorted-run mode)
  int n_levels, batch, num_anchors, num_classes, top_n;
  float thresh;
  unsigned long long *trace;   // debug (odtk_debug_set_trace): 8 words per segment, or null
};

// ---- key sources -------------------------------------------------------------------------
struct LdsSource {    // keys already gathered into LDS
  const uint64_t *keys;
  uint32_t count;
  template <typename F>
  __device__ __forceinline__ void for_each(F &&f) const {
    for (uint32_t i = threadIdx.x; i < count; i += kSelThreads) f(keys[i]);
  }
};

// A flat list of keys in global memory written by OTHER workgroups of this launch (the survivor list): agent-scope loads
// (`sc1`: past this XCD's L2 where it does not own the line; the writers stored write-through).  Sixteen loads in flight per
// lane: 16 384 keys per round trip.  Sources hand their keys over in BATCHES, f(keys[N], valid[N]) -- one call per load round,
// made by every lane of a wave together (ballots inside f are legal): a consumer that appends to a list then takes ONE LDS
// atomic per wave and round instead of one per key.  (Hand-written `global_load_dwordx4 ... sc1` in inline asm would halve the instruction count, but the compiler
// does not know that an asm statement's outputs arrive later: it copied -- and spilled -- them before the wait.)
struct FlatSource {
  const uint64_t *keys;
  uint32_t count;
  template <typename F>
  __device__ __forceinline__ void for_each(F &&f) const {
    constexpr int kLoads = 16;
    for (uint32_t i0 = 0; i0 < count; i0 += kLoads * kSelThreads) {
      uint64_t k[kLoads];
      bool v[kLoads];
#pragma unroll
      for (int u = 0; u < kLoads; ++u) {
        const uint32_t i = i0 + u * kSelThreads + threadIdx.x;
        v[u] = i < count;
        k[u] = v[u] ? __hip_atomic_load(keys + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
      }
      f(k, v);
    }
  }
};

// Keys in LDS
struct LdsFlat {
  const uint64_t *keys;
  uint32_t count;
  template <typename F>
  __device__ __forceinline__ void for_each(F &&f) const {
    for (uint32_t i0 = 0; i0 < count; i0 += 4 * kSelThreads) {             // (block-uniform trip count)
      uint64_t k[4];
      bool v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t i = i0 + u * kSelThreads + threadIdx.x;
        v[u] = i < count;
        k[u] = v[u] ? keys[i] : 0ull;
      }
      f(k, v);
    }
  }
};

// The spans s = part, part + G, part + 2G, ... of one segment: per span four sub-lists (one per prefilter wave) of up to
// kWaveStage keys, or -- a sub-list length of kListOverflow -- the span's raw scores.
//   lists     : a wave takes one span per load instruction -- 16 lanes per sub-list, a 16-byte load = 2 keys per lane, i.e.
//               the first 32 keys of each of the four sub-lists (at realistic densities: all of them) -- and eight spans
//               at a time, so that eight independent loads are in flight per lane; longer sub-lists follow in a second,
//               rolled loop that a wave enters only if one of its sub-lists needs it.
//   raw spans : (collected once per workgroup in `s_raw`) walked by the WHOLE workgroup, 16-byte vector loads, keys
//               rebuilt on the fly behind the prefilter's own conservative raw-domain test.
// f(keys[N], valid[N]): one call per load round, made by every lane of a wave together (ballots inside f are legal).
// for_each must be called by all threads of the workgroup.
template <typename T, bool kLogits>
struct SliceSource {
  const uint64_t *seg_keys;      // span 0 of this segment in the candidate pool
  const uint32_t *s_cnt;         // LDS: sub-list lengths, 4 per span
  const uint16_t *s_raw;         // LDS: this slice's raw spans (k indices)
  uint32_t n_raw;
  uint32_t part, G, ns;          // this workgroup's spans: part + k * G, k < ns
  uint32_t direct;               // s_cnt holds the whole segment (index by span) / only this slice (index by k)
  const void *image;             // raw scores of this image
  uint32_t n, hw, channels_last, span_elems, aligned;
  FastDiv by_channels;
  float thresh, raw_lo;
  const float *bias;             // per-channel head bias (logits only) or null

  __device__ __forceinline__ uint32_t cnt_index(uint32_t k) const { return (direct ? part + k * G : k) * kScanWaves; }

  // one raw element -> f(key, take)
  template <typename F>
  __device__ __forceinline__ void raw_element(float x, uint32_t r, bool inside, F &&f) const {
    bool take = inside;
    uint64_t key = 0;
    if (take) {
      uint32_t i = r;
      if (channels_last) {
        uint32_t ch;
        const uint32_t pix = fastdivmod(r, by_channels, &ch);
        i = ch * hw + pix;
        if (kLogits && bias) x += bias[ch];
      }
      take = kLogits ? x >= raw_lo : x >= thresh;            // (conservative for logits: the sigmoid only for the few that pass)
      if (take) {
        const float s = score_of<T, kLogits>(x);
        take = s >= thresh;
        key = make_key(s, i);
      }
    }
    const uint64_t k1[1] = {key};
    const bool v1[1] = {take};
    f(k1, v1);
  }

  template <typename F>
  __device__ __forceinline__ void raw_span(uint32_t span, F &&f) const {
    constexpr int kPer = T::kPerLoad;
    const uint32_t lo = span * span_elems;
    const uint32_t hi = n - lo < span_elems ? n : lo + span_elems;
    if (aligned) {                                           // every image starts on a 16-byte boundary, spans too
      const vuint4 *src = reinterpret_cast<const vuint4 *>(static_cast<const typename T::storage *>(image) + lo);
      const uint32_t n_vec = (hi - lo) / kPer;
      for (uint32_t q0 = 0; q0 < n_vec; q0 += kSelThreads) {            // (one vector per lane in flight: the rare route, registers matter more)
        const uint32_t q = q0 + threadIdx.x;
        const vuint4 v = q < n_vec ? src[q] : vuint4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
          float x;
          if constexpr (std::is_same_v<T, F32>) x = __uint_as_float(v[e]);
          else x = storage_to_float<T>(static_cast<uint16_t>((v[e >> 1] >> (16 * (e & 1))) & 0xffffu));
          raw_element(x, lo + q * kPer + e, q < n_vec, f);
        }
      }
    } else {
      for (uint32_t r0 = lo; r0 < hi; r0 += 4 * kSelThreads) {
        float raw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint32_t r = r0 + u * kSelThreads + threadIdx.x;
          raw[u] = r < hi ? load_raw<T>(image, r) : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint32_t r = r0 + u * kSelThreads + threadIdx.x;
          raw_element(raw[u], r, r < hi, f);
        }
      }
    }
  }

  template <typename F>
  __device__ __forceinline__ void for_each(F &&f) const {
    constexpr int kGroup = 4;                                            // spans per trip; 2 loads each: the first 64 keys of every sub-list
    const uint32_t wave = threadIdx.x >> 6, lane = static_cast<uint32_t>(lane_id());
    const uint32_t sub = lane >> 4, l16 = lane & 15u;
    bool more = false;                                                   // a sub-list of mine holds more than 64 keys
    for (uint32_t k0 = wave; k0 < ns; k0 += kSelWaves * kGroup) {        // (wave-uniform)
      vuint4 kv[kGroup][2];
      uint32_t cc[kGroup];
#pragma unroll
      for (int u = 0; u < kGroup; ++u) {
        const uint32_t k = k0 + kSelWaves * u;
        uint32_t c = k < ns ? s_cnt[cnt_index(k) + sub] : 0u;
        if (__ballot(c == kListOverflow)) c = 0;                         // one overflowed wave: the whole span is read raw (below)
        cc[u] = c;
        more = more || c > 64u;
        const uint64_t *list = seg_keys + static_cast<uint64_t>(part + k * G) * kSpanCap + sub * kWaveStage;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          kv[u][h] = vuint4{0u, 0u, 0u, 0u};
          if (32 * h + 2 * l16 < c) kv[u][h] = *reinterpret_cast<const vuint4 *>(list + 32 * h + 2 * l16);
        }
      }
      uint64_t key[4 * kGroup];
      bool val[4 * kGroup];
#pragma unroll
      for (int u = 0; u < kGroup; ++u) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint32_t i = 32 * h + 2 * l16;
          key[4 * u + 2 * h] = (static_cast<uint64_t>(kv[u][h][1]) << 32) | kv[u][h][0];
          key[4 * u + 2 * h + 1] = (static_cast<uint64_t>(kv[u][h][3]) << 32) | kv[u][h][2];
          val[4 * u + 2 * h] = i < cc[u];
          val[4 * u + 2 * h + 1] = i + 1 < cc[u];
        }
      }
      f(key, val);
    }
    if (__ballot(more)) {                                                // (wave-uniform) dense inputs: what the first 64 slots did not cover
#pragma unroll 1
      for (uint32_t k = wave; k < ns; k += kSelWaves) {
        uint32_t c = s_cnt[cnt_index(k) + sub];
        if (__ballot(c == kListOverflow)) continue;
        uint32_t cmax = c;
        cmax = max(cmax, static_cast<uint32_t>(__shfl_xor(cmax, 16, kWave)));
        cmax = max(cmax, static_cast<uint32_t>(__shfl_xor(cmax, 32, kWave)));
        cmax = __builtin_amdgcn_readfirstlane(cmax);
        const uint64_t *list = seg_keys + static_cast<uint64_t>(part + k * G) * kSpanCap + sub * kWaveStage;
        for (uint32_t base = 64; base < cmax; base += 64) {              // 2 x 2 keys per lane in flight
          vuint4 kk[2];
#pragma unroll
          for (int v = 0; v < 2; ++v) {
            const uint32_t i = base + 32 * v + 2 * l16;
            kk[v] = i < c ? *reinterpret_cast<const vuint4 *>(list + i) : vuint4{0u, 0u, 0u, 0u};
          }
          uint64_t key[4];
          bool val[4];
#pragma unroll
          for (int v = 0; v < 2; ++v) {
            const uint32_t i = base + 32 * v + 2 * l16;
            key[2 * v] = (static_cast<uint64_t>(kk[v][1]) << 32) | kk[v][0];
            key[2 * v + 1] = (static_cast<uint64_t>(kk[v][3]) << 32) | kk[v][2];
            val[2 * v] = i < c;
            val[2 * v + 1] = i + 1 < c;
          }
          f(key, val);
        }
      }
    }
    for (uint32_t q = 0; q < n_raw; ++q) raw_span(part + static_cast<uint32_t>(s_raw[q]) * G, f);   // (block-uniform)
  }
};

// ---- block-wide helpers --------------------------------------------------------------------
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int lane_mask) {
  const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), lane_mask, kWave);
  const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), lane_mask, kWave);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

// Bitonic sort, descending, of s_keys[0 .. 1024*E), 1024 threads, E keys per thread (element
// i = tid*E + e).  A compare-exchange with partner distance j needs
//   j <  E      : nothing but the thread's own registers,
//   j <  64*E   : one wave shuffle (partner lane = lane ^ j/E),
//   j >= 64*E   : another wave -> LDS + barrier.
// Of the 55 / 66 / 78 stages of a 1024 / 2048 / 4096-key network only 10 are of the last kind, so
// the keys live in registers and go through LDS only for those: ~20 barriers instead of 55-78
// (measured on MI355X: a 1024-key sort 13.6 us -> see DESIGN.md; every stage of the plain LDS
// version costs a full barrier round, ~0.25 us).
template <int E>
__device__ void bitonic_sort_desc_regs(uint64_t *s_keys) {
  constexpr uint32_t n = kSelThreads * E;
  const uint32_t tid = threadIdx.x;
  uint64_t v[E];
  auto load = [&] {
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = s_keys[tid * E + e];
  };
  auto store = [&] {
#pragma unroll
    for (int e = 0; e < E; ++e) s_keys[tid * E + e] = v[e];
  };
  // all stages j = j_start .. 1 of phase k, for j_start < 64*E: registers + wave shuffles only
  auto reg_stages = [&](uint32_t k, uint32_t j_start) {
    for (uint32_t j = j_start; j >= static_cast<uint32_t>(E); j >>= 1) {   // partner in another lane
      const int lane_mask = static_cast<int>(j / E);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const uint64_t p = shfl_xor_u64(v[e], lane_mask);
        const uint32_t i = tid * E + e;
        const bool take_max = ((i & j) == 0) == ((i & k) == 0);   // lower element of a descending pair
        v[e] = take_max ? (v[e] > p ? v[e] : p) : (v[e] < p ? v[e] : p);
      }
      if (j == 1) return;                                         // E == 1: j ran down to 1 here
    }
#pragma unroll
    for (int j = E / 2; j > 0; j >>= 1) {                        // partner in the same thread
      if (static_cast<uint32_t>(j) > j_start) continue;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if ((e & j) == 0) {
          const uint32_t i = tid * E + e;
          const bool desc = (i & k) == 0;
          const uint64_t x = v[e], y = v[e | j];
          if (desc ? (x < y) : (x > y)) { v[e] = y; v[e | j] = x; }
        }
      }
    }
  };
  load();
  for (uint32_t k = 2; k <= 64u * E; k <<= 1) reg_stages(k, k >> 1);           // no LDS, no barrier
  for (uint32_t k = 128u * E; k <= n; k <<= 1) {
    store();
    __syncthreads();
    for (uint32_t j = k >> 1; j >= 64u * E; j >>= 1) {                          // cross-wave stages
      for (uint32_t t = tid; t < (n >> 1); t += kSelThreads) {
        const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const uint32_t hi = lo | j;
        const uint64_t x = s_keys[lo], y = s_keys[hi];
        const bool desc = (lo & k) == 0;
        if (desc ? (x < y) : (x > y)) { s_keys[lo] = y; s_keys[hi] = x; }
      }
      __syncthreads();
    }
    load();
    reg_stages(k, 32u * E);
  }
  store();
  __syncthreads();
}

// The 4096-key network is the one piece of device code that stays out of line (a call from every select_decode and nms
// kernel, ~3 700 instructions each copy).  __noinline__ keeps it a call whichever kernels a source instantiates: the inliner
// absorbs it where only the six nms kernels call it.
__device__ __noinline__ void bitonic_sort_desc_4096(uint64_t *s_keys) { bitonic_sort_desc_regs<4>(s_keys); }

// Sorts s_keys[0..n_valid) descending; entries up to the padded size are zeroed (sort last).
// The buffer must hold max(1024, pow2(n_valid)) <= kSortCapBig keys.
template <int kMaxKeys = 4096>
__device__ __forceinline__ void sort_keys_desc(uint64_t *s_keys, uint32_t n_valid) {
  uint32_t n_pad = kSelThreads;
  while (n_pad < n_valid) n_pad <<= 1;
  for (uint32_t i = n_valid + threadIdx.x; i < n_pad; i += kSelThreads) s_keys[i] = 0;
  __syncthreads();
  if (n_pad == kSelThreads) bitonic_sort_desc_regs<1>(s_keys);
  else if (n_pad == 2 * kSelThreads) bitonic_sort_desc_regs<2>(s_keys);
  else if (n_pad == 4 * kSelThreads || kMaxKeys <= 4 * kSelThreads) bitonic_sort_desc_4096(s_keys);
  else if constexpr (kMaxKeys > 4 * kSelThreads) {           // only the top_n > 4096 variant carries the big networks
    if (n_pad == 8 * kSelThreads) bitonic_sort_desc_regs<8>(s_keys);
    else bitonic_sort_desc_regs<16>(s_keys);
  }
}

// Sort of up to 1024 keys (s_buf[0 .. n_valid), one per thread), descending, unique keys.  A wave sorts its 64 keys in
// registers (21 shuffle stages of the bitonic network); the sixteen runs are then MERGED BY RANK, four levels: a key's
// place in the union of its run and the partner run is its place in its own run plus the number of partner keys above
// it -- one binary search in LDS (keys are unique: no ties) -- instead of the 34 further compare-exchange stages of the
// network, ten of them through LDS with a barrier each.  Measured: 7.7 us for the full network, see DESIGN.md.
// s_buf must hold 2 * 1024 keys; returns where the sorted keys are (s_buf or s_buf + 1024): n_valid of them, what lies
// behind is unspecified.  The work follows n_valid, not the capacity: slots beyond n_valid exist only inside the wave that
// holds the last key (as values below every real key -- a real key's score word is never 0 -- for its network); waves
// behind it skip the network, no padding is ever merged, and a search looks at the real keys of the partner run only --
// the keys lie in [0, n_valid) before and after every level, so run r of length R holds clamp(n_valid - r R, 0, R) of
// them, at its front.  (The sort is VALU-issue-bound -- 16 waves share 4 SIMDs -- so the 1300 survivors of a P3 segment
// cost 1300 / 2048 of what the padded form did: 9.3 -> ~6.3 us.)
__device__ __forceinline__ uint32_t keys_in_run(uint32_t n_valid, uint32_t run, uint32_t R) {
  const uint32_t first = run * R;
  return n_valid <= first ? 0u : (n_valid - first < R ? n_valid - first : R);
}

__device__ __forceinline__ const uint64_t *merge_sort_1024(uint64_t *s_buf, uint32_t n_valid) {
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
  const bool real = tid < n_valid;
  uint64_t v = real ? s_buf[tid] : static_cast<uint64_t>(kSelThreads - tid);
  if ((tid & ~static_cast<uint32_t>(kWave - 1)) < n_valid) {   // (wave-uniform)
#pragma unroll
    for (uint32_t k = 2; k <= static_cast<uint32_t>(kWave); k <<= 1) {
#pragma unroll
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        const uint64_t p = shfl_xor_u64(v, static_cast<int>(j));
        const bool take_max = ((lane & j) == 0) == ((lane & k) == 0);   // lower element of a descending pair
        v = take_max ? (v > p ? v : p) : (v < p ? v : p);
      }
    }
  }
  __syncthreads();                                         // every thread has read its key
  uint64_t *src = s_buf, *dst = s_buf + kSelThreads;
  if (real) src[tid] = v;                                  // (after its wave's network slot `tid` holds a real key iff tid < n_valid)
  __syncthreads();
  uint32_t g = tid;                                        // where this thread's key sits
#pragma unroll
  for (uint32_t R = kWave; R < static_cast<uint32_t>(kSelThreads); R <<= 1) {
    if (real) {
      const uint32_t run = g / R, p = g - run * R;
      const uint64_t *other = src + (run ^ 1u) * R;        // the partner run, descending
      const uint32_t c = keys_in_run(n_valid, run ^ 1u, R);
      uint32_t above = 0;                                  // partner keys above mine
#pragma unroll
      for (uint32_t step = R >> 1; step > 0; step >>= 1)
        if (above + step <= c && other[above + step - 1] > v) above += step;
      above += (above < c && other[above] > v) ? 1u : 0u;
      g = (run >> 1) * 2 * R + p + above;
      dst[g] = v;
    }
    __syncthreads();
    uint64_t *t = src; src = dst; dst = t;
  }
  return src;
}

// The same for up to 2048 keys, two per thread (the two wave-local networks and the two binary searches of a level are
// independent chains: their shuffle / LDS latencies overlap).  s_buf must hold 2 * 2048 keys; five merge levels.
__device__ __forceinline__ const uint64_t *merge_sort_2048(uint64_t *s_buf, uint32_t n_valid) {
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
  uint64_t v[2];
  bool real[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t i = tid + h * kSelThreads;
    real[h] = i < n_valid;
    v[h] = real[h] ? s_buf[i] : static_cast<uint64_t>(2 * kSelThreads - i);
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if ((tid & ~static_cast<uint32_t>(kWave - 1)) + h * kSelThreads < n_valid) {   // (wave-uniform)
#pragma unroll
      for (uint32_t k = 2; k <= static_cast<uint32_t>(kWave); k <<= 1) {
#pragma unroll
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
          const bool take_max = ((lane & j) == 0) == ((lane & k) == 0);
          const uint64_t p = shfl_xor_u64(v[h], static_cast<int>(j));
          v[h] = take_max ? (v[h] > p ? v[h] : p) : (v[h] < p ? v[h] : p);
        }
      }
    }
  }
  __syncthreads();                                         // every thread has read its keys
  uint64_t *src = s_buf, *dst = s_buf + 2 * kSelThreads;
  uint32_t g[2] = {tid, tid + static_cast<uint32_t>(kSelThreads)};
#pragma unroll
  for (int h = 0; h < 2; ++h)
    if (real[h]) src[g[h]] = v[h];
  __syncthreads();
#pragma unroll
  for (uint32_t R = kWave; R < 2u * kSelThreads; R <<= 1) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (real[h]) {
        const uint32_t run = g[h] / R, p = g[h] - run * R;
        const uint64_t *other = src + (run ^ 1u) * R;
        const uint32_t c = keys_in_run(n_valid, run ^ 1u, R);
        uint32_t above = 0;
#pragma unroll
        for (uint32_t step = R >> 1; step > 0; step >>= 1)
          if (above + step <= c && other[above + step - 1] > v[h]) above += step;
        above += (above < c && other[above] > v[h]) ? 1u : 0u;
        g[h] = (run >> 1) * 2 * R + p + above;
        dst[g[h]] = v[h];
      }
    }
    __syncthreads();
    uint64_t *t = src; src = dst; dst = t;
  }
  return src;
}

// Given a histogram in s_hist (kRadixBins bins, REVERSED: bin 0 = largest digit) finds the bin in which the running
// count (from the largest digit down) crosses `remaining`.  All threads return the same (bin, count above it, count
// inside it).  s_misc: [0..15] wave totals, [16..18] result.  Ends with a barrier; s_hist may be reused afterwards.
__device__ __forceinline__ void scan_boundary(const uint32_t *s_hist, uint32_t remaining, uint32_t *s_misc, uint32_t *rbin,
                                              uint32_t *above, uint32_t *in_bin) {
  // inclusive scan over kRadixBins bins, 2 per thread
  const uint32_t h0 = s_hist[2 * threadIdx.x], h1 = s_hist[2 * threadIdx.x + 1];
  const uint32_t inc = wave_inclusive_sum(h0 + h1);
  const int w = threadIdx.x >> 6;
  if (lane_id() == kWave - 1) s_misc[w] = inc;
  __syncthreads();
  uint32_t woff = 0;
  for (int i = 0; i < w; ++i) woff += s_misc[i];
  const uint32_t excl = woff + inc - (h0 + h1);
  // the unique bin where the running count crosses `remaining`
  if (excl < remaining && remaining <= excl + h0) { s_misc[16] = 2 * threadIdx.x; s_misc[17] = excl; s_misc[18] = h0; }
  else if (excl + h0 < remaining && remaining <= excl + h0 + h1) { s_misc[16] = 2 * threadIdx.x + 1; s_misc[17] = excl + h0; s_misc[18] = h1; }
  __syncthreads();
  // (values read from LDS are VGPRs -- "divergent" to the compiler; callers steer loops with them, so pin them to SGPRs:
  // the descent loops then compile to scalar control flow instead of exec-masked waterfall loops)
  *rbin = __builtin_amdgcn_readfirstlane(s_misc[16]);
  *above = __builtin_amdgcn_readfirstlane(s_misc[17]);
  *in_bin = __builtin_amdgcn_readfirstlane(s_misc[18]);
  __syncthreads();
}

// MSD radix descent (11-bit digits, LDS histogram) on the bin that holds the `want`-th largest key.
// Returns a threshold T and *n_out = #{key >= T} with  want <= *n_out <= max_take : the descent
// stops as soon as everything above the boundary bin plus the bin itself fits `max_take`, so the
// caller sorts a few extra keys instead of paying for more passes.  Keys are unique; the source
// must hold at least `want` keys and max_take >= want.  s_misc: [0..15] wave totals, [16..18] result.
template <typename Source>
__device__ __forceinline__ uint64_t radix_threshold(const Source &src, uint32_t want, uint32_t max_take, uint32_t *s_hist,
                                    uint32_t *s_misc, uint32_t *n_out) {
  uint64_t prefix = 0, pmask = 0;
  uint32_t remaining = want, taken_above = 0, in_bin = 0;
  int hi_bit = 64;
  while (hi_bit > 0) {
    const int bits = hi_bit >= kRadixBits ? kRadixBits : hi_bit;
    const int shift = hi_bit - bits;
    const uint32_t nb = 1u << bits;
    for (uint32_t i = threadIdx.x; i < kRadixBins; i += kSelThreads) s_hist[i] = 0;
    __syncthreads();
    // histogram, bins reversed so that an ascending scan walks keys from the largest digit down
    src.for_each([&](uint64_t key) {
      if ((key & pmask) == prefix) atomicAdd(&s_hist[(nb - 1) - static_cast<uint32_t>((key >> shift) & (nb - 1))], 1u);
    });
    __syncthreads();
    uint32_t rbin, above;
    scan_boundary(s_hist, remaining, s_misc, &rbin, &above, &in_bin);
    const uint64_t digit = (nb - 1) - rbin;
    prefix |= digit << shift;
    pmask |= static_cast<uint64_t>(nb - 1) << shift;
    remaining -= above;
    taken_above += above;
    hi_bit = shift;
    if (taken_above + in_bin <= max_take) break;   // at the last digit in_bin == remaining == 1
  }
  *n_out = taken_above + in_bin;
  return prefix;                                    // undecided low bits are 0 = start of the boundary bin
}

__device__ __forceinline__ uint32_t sort_size_for(uint32_t top_n) {
  uint32_t sort_size = kSelThreads;
  while (sort_size < top_n) sort_size <<= 1;
  return sort_size;
}

__device__ __forceinline__ int range_shift(uint64_t lo, uint64_t hi) {   // (hi - lo) >> shift < 2048
  const uint64_t w = hi - lo;
  const int bl = w ? 64 - __clzll(static_cast<long long>(w)) : 0;
  return bl > kRadixBits ? bl - kRadixBits : 0;
}

// radix_threshold on a KNOWN key range [lo, hi] (both inclusive), 1024-thread workgroups: every pass cuts the range into
// 2048 equal bins instead of taking the next 11 key bits, so the first pass already lands on the bits in which the keys
// differ (fp32 scores of one image share their exponent bits: an 11-bit MSD digit separates almost nothing).  The source
// must hold at least `want` keys inside the range.  Returns T with  want <= #{key in [T, hi]} = *n_out <= max_take  (or
// the exact `want`-th key when ties in the digit cannot be split further).
template <typename Source>
__device__ uint64_t range_threshold(const Source &src, uint32_t want, uint32_t max_take, uint64_t lo, uint64_t hi, uint32_t *s_hist,
                                    uint32_t *s_misc, uint32_t *n_out) {
  uint32_t remaining = want, taken_above = 0, in_bin = 0;
  for (;;) {
    const int sh = range_shift(lo, hi);
    for (uint32_t i = threadIdx.x; i < kRadixBins; i += kSelThreads) s_hist[i] = 0;
    __syncthreads();
    src.for_each([&](uint64_t key) {
      if (key >= lo && key <= hi) {
        uint32_t digit = static_cast<uint32_t>((key - lo) >> sh);
        digit = digit > kRadixBins - 1 ? kRadixBins - 1 : digit;
        atomicAdd(&s_hist[(kRadixBins - 1) - digit], 1u);
      }
    });
    __syncthreads();
    uint32_t rbin, above;
    scan_boundary(s_hist, remaining, s_misc, &rbin, &above, &in_bin);
    const uint64_t digit = (kRadixBins - 1) - rbin;
    const uint64_t span = sh ? ((1ull << sh) - 1ull) : 0ull;
    const uint64_t nlo = lo + (digit << sh);
    uint64_t nhi = nlo > ~0ull - span ? ~0ull : nlo + span;
    nhi = nhi < hi ? nhi : hi;
    lo = nlo;
    hi = nhi;
    remaining -= above;
    taken_above += above;
    if (taken_above + in_bin <= max_take || sh == 0) break;
  }
  *n_out = taken_above + in_bin;
  return lo;
}

// scan_boundary that also returns the histogram's total; the histogram comes as kCopies interleaved sub-histograms
// (s_hist[bin * kCopies + c]).  s_misc: [0..15] wave totals, [16..18] result.
template <int kCopies>
__device__ __forceinline__ void scan_boundary_total(const uint32_t *s_hist, uint32_t remaining, uint32_t *s_misc, uint32_t *rbin,
                                                    uint32_t *above, uint32_t *in_bin, uint32_t *total) {
  uint32_t h0 = 0, h1 = 0;
#pragma unroll
  for (int c = 0; c < kCopies; ++c) {
    h0 += s_hist[(2 * threadIdx.x) * kCopies + c];
    h1 += s_hist[(2 * threadIdx.x + 1) * kCopies + c];
  }
  const uint32_t inc = wave_inclusive_sum_dpp(h0 + h1);
  const int w = threadIdx.x >> 6;
  if (lane_id() == kWave - 1) s_misc[w] = inc;
  if (threadIdx.x == 0) { s_misc[16] = 0; s_misc[17] = 0; s_misc[18] = 0; }
  __syncthreads();
  uint32_t woff = 0, all = 0;
  for (int i = 0; i < kSelWaves; ++i) {
    const uint32_t t = s_misc[i];
    if (i < w) woff += t;
    all += t;
  }
  const uint32_t excl = woff + inc - (h0 + h1);            // (the zeroing of [16..18] lies before the barrier above)
  if (excl < remaining && remaining <= excl + h0) { s_misc[16] = 2 * threadIdx.x; s_misc[17] = excl; s_misc[18] = h0; }
  else if (excl + h0 < remaining && remaining <= excl + h0 + h1) { s_misc[16] = 2 * threadIdx.x + 1; s_misc[17] = excl + h0; s_misc[18] = h1; }
  __syncthreads();
  *rbin = __builtin_amdgcn_readfirstlane(s_misc[16]);
  *above = __builtin_amdgcn_readfirstlane(s_misc[17]);
  *in_bin = __builtin_amdgcn_readfirstlane(s_misc[18]);
  *total = __builtin_amdgcn_readfirstlane(all);
  __syncthreads();
}

// State of a selection: the current key range [lo, hi] (both inclusive; T = lo is the threshold it stands for), `taken`
// keys above it -- all of them wanted --, `in_bin` inside it, of which the `remaining` largest are wanted.
struct SelState {
  uint64_t lo, hi;
  uint32_t remaining, taken, in_bin;
};

// Histogram of the keys of `src` inside [lo, hi] over 2048 equal bins (reversed: bin 0 = largest keys), kept as kCopies
// interleaved sub-histograms, lane l adding to copy l % kCopies: 16-bit scores put thousands of keys into a handful of bins, and
// lanes of a wave that add to ONE LDS word are served one after the other (measured: the pass over the 22 000 bf16-score
// keys of a P3 segment ~9 us with one histogram).  kTrack: also the smallest and the largest key inside the range (s_range).
// Per key ~10 instructions: ONE workgroup -- one CU, 64 lanes per clock -- pays every instruction once per key.
template <int kCopies>
__device__ __forceinline__ void hist_clear(uint32_t *s_hist, unsigned long long *s_range) {
  for (uint32_t i = threadIdx.x; i < kRadixBins * kCopies; i += kSelThreads) s_hist[i] = 0;
  if (threadIdx.x < 2) s_range[threadIdx.x] = 0;
}
template <int kCopies>
__device__ __forceinline__ void hist_add(uint32_t *s_hist, uint64_t key, uint64_t lo, int sh) {   // lo <= key <= hi
  atomicAdd(&s_hist[((kRadixBins - 1) - static_cast<uint32_t>((key - lo) >> sh)) * kCopies + (threadIdx.x & (kCopies - 1))], 1u);
}
template <int kCopies, bool kTrack, typename Source>
__device__ __forceinline__ void hist_pass(const Source &src, uint64_t lo, uint64_t hi, uint32_t *s_hist, unsigned long long *s_range) {
  hist_clear<kCopies>(s_hist, s_range);
  __syncthreads();
  const int sh = range_shift(lo, hi);
  uint64_t my_max = 0, my_min_inv = 0;
  src.for_each([&](const auto &key, const auto &valid) {
    constexpr int N = static_cast<int>(sizeof(valid) / sizeof(valid[0]));
#pragma unroll
    for (int u = 0; u < N; ++u) {
      if (valid[u] && key[u] >= lo && key[u] <= hi) {
        hist_add<kCopies>(s_hist, key[u], lo, sh);
        if (kTrack) {
          my_max = key[u] > my_max ? key[u] : my_max;
          my_min_inv = ~key[u] > my_min_inv ? ~key[u] : my_min_inv;
        }
      }
    }
  });
  if (kTrack) {
    my_max = wave_max_u64(my_max);
    my_min_inv = wave_max_u64(my_min_inv);
    if (lane_id() == 0 && my_max != 0) { atomicMax(&s_range[0], my_max); atomicMax(&s_range[1], my_min_inv); }
  }
  __syncthreads();
}

// Folds the histogram in s_hist -- of the keys inside [st.lo, st.hi] -- into the state: the bin where the running count,
// from the top, crosses st.remaining becomes the new range.  The new range is clipped (a) to [kmin, kmax], the smallest and
// largest key of the OLD range if known (0 / ~0 otherwise), and (b), when it lies inside ONE score word, to the index bits
// that can occur (an index is < n_index): keys that share all their score bits -- every 16-bit score is such a plateau -- are
// then split on their index bits by the very next pass.  Returns the histogram's total.  (block-uniform; ends with a barrier)
template <int kCopies>
__device__ __forceinline__ uint32_t advance_state(SelState &st, const uint32_t *s_hist, uint32_t *s_misc, uint32_t n_index, uint64_t kmin,
                                                  uint64_t kmax) {
  const int sh = range_shift(st.lo, st.hi);
  uint32_t rbin, above, in_bin, total;
  scan_boundary_total<kCopies>(s_hist, st.remaining, s_misc, &rbin, &above, &in_bin, &total);
  const uint64_t digit = (kRadixBins - 1) - rbin;
  const uint64_t span = sh ? ((1ull << sh) - 1ull) : 0ull;
  uint64_t lo = st.lo + (digit << sh);
  uint64_t hi = lo > ~0ull - span ? ~0ull : lo + span;
  hi = hi < st.hi ? hi : st.hi;
  lo = lo > kmin ? lo : kmin;
  hi = hi < kmax ? hi : kmax;
  if ((lo >> 32) == (hi >> 32)) {                                        // one score word: the low word is ~index, index < n_index
    const uint64_t floor_lo = (lo & 0xffffffff00000000ull) | static_cast<uint32_t>(0u - n_index);
    lo = lo > floor_lo ? lo : floor_lo;
  }
  st.lo = lo;
  st.hi = hi;
  st.remaining -= above;
  st.taken += above;
  st.in_bin = in_bin;
  return total;
}

// Threshold over the keys of `src`, all of which lie inside [lo, hi] (both inclusive): on return #{key >= st.lo} = st.taken +
// st.in_bin with  min(want, all) <= st.taken + st.in_bin <= max_take  (want <= take_all <= max_take); a source of no more
// than `take_all` keys is taken whole (st.lo = lo, in_bin = 0).  Every pass histograms the current range and descends into
// the boundary bin; it stops as soon as everything above that bin plus the bin itself fits max_take -- normally after ONE
// pass (a linear digit over the score range separates what an 11-bit MSD digit cannot: fp32 scores of one image share
// their exponent bits).  Source: for_each(f(key, valid)), uniform call count per wave.  s_misc: [0..18] scan scratch.
template <int kCopies, typename Source>
__device__ __forceinline__ SelState select_threshold(const Source &src, uint32_t want, uint32_t max_take, uint32_t take_all, uint64_t lo,
                                                     uint64_t hi, uint32_t n_index, uint32_t *s_hist, uint32_t *s_misc,
                                                     unsigned long long *s_range) {
  SelState st{lo, hi, want, 0u, 0u};
  hist_pass<kCopies, false>(src, st.lo, st.hi, s_hist, s_range);
  int sh = range_shift(st.lo, st.hi);
  const uint32_t total = advance_state<kCopies>(st, s_hist, s_misc, n_index, 0ull, ~0ull);
  if (total <= take_all) return SelState{lo, hi, 0u, total, 0u};          // few enough to take them all
  while (!(st.taken + st.in_bin <= max_take || sh == 0 || st.lo >= st.hi)) {
    hist_pass<kCopies, true>(src, st.lo, st.hi, s_hist, s_range);
    const uint64_t kmax = uniform_u64(s_range[0]), kmin = ~uniform_u64(s_range[1]);
    sh = range_shift(st.lo, st.hi);
    advance_state<kCopies>(st, s_hist, s_misc, n_index, kmin, kmax);       // (barriers inside: s_range may be reset after it)
  }
  return st;
}

// ---- the kernel ------------------------------------------------------------------------------
// NB: box parameters (4 axis-aligned, 6 rotated); T: element type of BOTH head tensors;
// kLogits: cls holds logits (sigmoid fused, see prefilter.hpp score_of).
// CAP: keys the LDS sort buffer holds -- kSortCap (static LDS) for top_n <= 4096, kSortCapBig (dynamic LDS, the launch
// passes CAP * 8 bytes) beyond.
template <int NB, typename T, bool kLogits, int CAP = kSortCap>
__global__ __launch_bounds__(kSelThreads) void select_decode_kernel(const DecodeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn_sel[];
  using Lds = SelLds<CAP>;
  uint64_t *s_keys = reinterpret_cast<uint64_t *>(s_dyn_sel + Lds::keys);
  uint32_t *s_hist = reinterpret_cast<uint32_t *>(s_dyn_sel + Lds::hist);
  uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_dyn_sel + Lds::cnt);
  uint16_t *s_raw = reinterpret_cast<uint16_t *>(s_dyn_sel + Lds::raw);
  __shared__ uint32_t s_misc[96];   // [0..18] scan scratch, [20] cursors, [22] positives, [25..28] tickets, [32..63] wave sums / flags, [64] route
  __shared__ unsigned long long s_range[2];

  int l = 0;
#pragma unroll
  for (int i = 1; i < ODTK_MAX_LEVELS; ++i)
    if (i < a.n_levels && blockIdx.x >= a.part_begin[i]) l = i;
  const uint32_t P = a.parts[l];
  const uint32_t jb = blockIdx.x - a.part_begin[l];
  const uint32_t b = jb / P, part = jb - b * P;
  const int seg = l * a.batch + static_cast<int>(b);
  const DecodeLevel &L = a.lv[l];
  const uint32_t top_n = a.top_n;
  const int H = L.height, W = L.width, A = a.num_anchors, C = a.num_classes;
  const uint32_t hw = static_cast<uint32_t>(H) * W;
  const uint32_t channels = static_cast<uint32_t>(A) * C;
  const typename T::storage *cls_image = static_cast<const typename T::storage *>(L.cls) + static_cast<uint64_t>(b) * L.n;
  const uint32_t tid = threadIdx.x;
  auto stamp = [&](int k) { if (a.trace && tid == 0) a.trace[seg * 8 + k] = wall_clock64(); };
  // finer phases (16 words per segment behind word 8192): [0..6] as workgroup 0 of the segment sees them, [8..12] the finisher
  auto stamp2 = [&](int k, bool mine) { if (a.trace && tid == 0 && mine) a.trace[8192 + seg * 16 + k] = wall_clock64(); };
  stamp2(0, part == 0);

  // ---- the segment's sub-list lengths: total, overflow; how many workgroups take part ----
  const uint32_t spans = L.spans, n_lists = spans * kScanWaves;
  const uint32_t *seg_counts = a.counts + L.cnt_off + static_cast<size_t>(b) * n_lists;
  const uint32_t direct = n_lists <= kCntSlots ? 1u : 0u;
  {
    uint32_t sum = 0;
    bool raw = false;
    for (uint32_t i = tid; i < n_lists; i += kSelThreads) {
      const uint32_t c = seg_counts[i];
      if (direct) s_cnt[i] = c;
      if (c == kListOverflow) raw = true;
      else sum += c;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, kWave);
    const uint64_t any_raw = __ballot(raw);
    if (lane_id() == 0) { s_misc[32 + (tid >> 6)] = sum; s_misc[48 + (tid >> 6)] = any_raw ? 1u : 0u; }
    if (tid == 0) s_misc[22] = 0;                                          // positive scores emitted (run_valid)
    __syncthreads();
  }
  uint32_t n_total = 0, has_raw = 0;
  for (int i = 0; i < kSelWaves; ++i) { n_total += s_misc[32 + i]; has_raw |= s_misc[48 + i]; }
  n_total = __builtin_amdgcn_readfirstlane(n_total);
  has_raw = __builtin_amdgcn_readfirstlane(has_raw);
  // workgroups that take part: one per kKeysPerPart candidates (a slice then fits the sort buffer whole), all of them when
  // raw spans have to be walked
  uint32_t G = (n_total + kKeysPerPart - 1) / kKeysPerPart;
  const uint32_t g_min = (n_lists + kCntSlots - 1) / kCntSlots;              // a slice's lengths must fit s_cnt
  G = G < g_min ? g_min : G;
  G = G < 1u ? 1u : G;
  if (has_raw || G > P) G = P;
  if (part >= G) return;                                                   // (block-uniform)
  stamp2(1, part == 0);
  if (part == G - 1) stamp(0);
  const uint32_t ns = part < spans ? (spans - part + G - 1) / G : 0u;
  if (!direct) {
    __syncthreads();
    for (uint32_t i = tid; i < ns * kScanWaves; i += kSelThreads)
      s_cnt[i] = seg_counts[(part + (i / kScanWaves) * G) * kScanWaves + (i % kScanWaves)];
    __syncthreads();
  }
  // this slice's raw spans (a sub-list overflowed), collected once: the whole workgroup walks them (SliceSource::raw_span)
  if (tid == 0) s_misc[28] = 0;
  __syncthreads();
  if (has_raw) {
    for (uint32_t k = tid; k < ns; k += kSelThreads) {
      const uint32_t *c = s_cnt + (direct ? part + k * G : k) * kScanWaves;
      if (c[0] == kListOverflow || c[1] == kListOverflow || c[2] == kListOverflow || c[3] == kListOverflow)
        s_raw[atomicAdd(&s_misc[28], 1u)] = static_cast<uint16_t>(k);
    }
    __syncthreads();
  }
  const uint32_t n_raw = __builtin_amdgcn_readfirstlane(s_misc[28]);
  const SliceSource<T, kLogits> slice{a.cand + L.key_off + static_cast<uint64_t>(b) * spans * kSpanCap, s_cnt, s_raw, n_raw, part, G, ns, direct,
                                      cls_image, L.n, hw, L.channels_last, a.span_elems, a.aligned, a.by_channels, a.thresh, a.raw_lo, L.cls_bias};
  // every candidate's key lies in [key(thresh, last index), key(1.0 | +inf, index 0)]; sigmoid outputs never exceed 1
  const uint64_t k_lo = make_key(a.thresh, 0xffffffffu);
  const uint64_t k_hi = kLogits ? make_key(1.0f, 0u) : ~0ull;

  // Gathers the keys >= T64 of `src` at the front of s_keys and -- in the same walk -- histograms them over [T64 | k_lo, k_hi]
  // (s_hist: the first digit of whatever selection follows).  Returns how many there ARE (block-uniform; more than CAP: the
  // buffer holds only the first CAP and the caller must narrow the source first).
  auto gather = [&](const auto &src, uint64_t T64) -> uint32_t {
    const uint64_t h_lo = T64 > k_lo ? T64 : k_lo;
    const int sh = range_shift(h_lo, k_hi);
    __syncthreads();
    hist_clear<Lds::copies>(s_hist, s_range);
    if (tid == 0) s_misc[20] = 0;
    __syncthreads();
    src.for_each([&](const auto &key, const auto &valid) {
      constexpr int N = static_cast<int>(sizeof(valid) / sizeof(valid[0]));
      // ONE LDS atomic per wave and batch (a returning atomic per key: ~150 clk each on the critical path)
      uint64_t m[N];
      uint32_t tot = 0;
#pragma unroll
      for (int u = 0; u < N; ++u) {
        m[u] = __ballot(valid[u] && key[u] >= T64);
        tot += static_cast<uint32_t>(__popcll(m[u]));
      }
      if (!tot) return;                                                   // (wave-uniform)
      uint32_t base = 0;
      if (lane_id() == 0) base = atomicAdd(&s_misc[20], tot);
      base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
      for (int u = 0; u < N; ++u) {
        if (valid[u] && key[u] >= T64) {
          hist_add<Lds::copies>(s_hist, key[u], h_lo, sh);
          const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m[u] >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m[u]), 0u));
          if (slot < static_cast<uint32_t>(CAP)) s_keys[slot] = key[u];
        }
        base += static_cast<uint32_t>(__popcll(m[u]));
      }
    });
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(s_misc[20]);
  };
  // The n_have keys at the front of s_keys -- all >= h_lo, their histogram over [h_lo, k_hi] in s_hist (gather's) -- cut down
  // IN LDS to the best `limit` or fewer (never fewer than top_n of them, if that many exist): further digits over keys that
  // are already here, then an in-place compaction.  *T_out: the threshold that was applied (h_lo if nothing was cut).
  // *first_bins: s_hist still holds the first digit and the keys kept are exactly those of its bins [0, *first_bins); 0: it
  // does not (further digits were needed).
  auto narrow_in_lds = [&](uint32_t n_have, uint32_t limit, uint64_t h_lo, uint32_t *first_bins) -> uint32_t {
    *first_bins = kRadixBins;
    if (n_have <= limit) return n_have;
    const LdsFlat in_lds{s_keys, n_have};
    SelState st{h_lo > k_lo ? h_lo : k_lo, k_hi, top_n, 0u, 0u};
    int sh = range_shift(st.lo, st.hi);
    advance_state<Lds::copies>(st, s_hist, s_misc, L.n, 0ull, ~0ull);
    *first_bins = (kRadixBins - 1) - static_cast<uint32_t>((st.lo - (h_lo > k_lo ? h_lo : k_lo)) >> sh) + 1;   // bins down to the boundary bin
    while (!(st.taken + st.in_bin <= limit || sh == 0 || st.lo >= st.hi)) {
      *first_bins = 0;
      hist_pass<Lds::copies, true>(in_lds, st.lo, st.hi, s_hist, s_range);
      const uint64_t kmax = uniform_u64(s_range[0]), kmin = ~uniform_u64(s_range[1]);
      sh = range_shift(st.lo, st.hi);
      advance_state<Lds::copies>(st, s_hist, s_misc, L.n, kmin, kmax);
    }
    // in-place compaction, 4096 keys per round: every lane reads its four keys, barrier, survivors go to the front (slots
    // below the round's first key: all of them read already)
    if (tid == 0) s_misc[20] = 0;
    for (uint32_t base = 0; base < n_have; base += 4 * kSelThreads) {
      uint64_t mine[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t i = base + u * kSelThreads + tid;
        mine[u] = i < n_have ? s_keys[i] : 0;
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool keep = mine[u] != 0 && mine[u] >= st.lo;
        const uint32_t slot = wave_append_slot(&s_misc[20], keep);
        if (keep) s_keys[slot] = mine[u];
      }
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(s_misc[20]);
  };
  // The best keys of `src` into s_keys (+ their histogram, as gather leaves it): those >= T_known if they fit the buffer,
  // otherwise those at or above a threshold found by histogram passes over the source itself.  *h_lo: the gather threshold.
  // direct = false: the source is known to hold more than the buffer (or raw spans, whose walk is not worth a trial).
  auto fetch = [&](const auto &src, uint64_t T_known, bool direct, uint64_t *h_lo) -> uint32_t {
    *h_lo = T_known;
    uint32_t got = 0;
    if (direct) {
      got = gather(src, T_known);
      if (got <= static_cast<uint32_t>(CAP)) return got;
    }
    const SelState st = select_threshold<Lds::copies>(src, top_n, CAP, CAP, k_lo, k_hi, L.n, s_hist, s_misc, s_range);
    *h_lo = st.lo;
    got = gather(src, st.lo);
    return got < static_cast<uint32_t>(CAP) ? got : static_cast<uint32_t>(CAP);
  };

  const uint32_t sort_size = sort_size_for(top_n);
  uint32_t n_sort;   // number of valid keys placed in s_keys
  uint64_t h_lo;     // ... all of them >= h_lo, their histogram over [max(h_lo, k_lo), k_hi] in s_hist
  bool coop_done = false;   // (debug trace) the segment went the cooperative route
  uint32_t coop_bins = 0;   // cooperative route: bins of the segment's histogram at or above the global threshold
  if (G == 1) {
    n_sort = fetch(slice, 0ull, !has_raw && n_total <= static_cast<uint32_t>(CAP), &h_lo);
    stamp2(4, true);
  } else {
    // Several workgroups share the segment.  Two routes, decided for the WHOLE segment by one compare-and-swap:
    //
    // cooperative (round 5; the normal case): every slice fits LDS whole.  Each workgroup adds its slice's histogram (first
    //   digit: 2048 bins of [k_lo, k_hi]) to the segment's and takes a ticket; a SEGMENT-LOCAL BARRIER -- a bounded spin on the
    //   ticket counter: the <= 64 partners have consecutive workgroup ids and are dispatched in order, nobody waits for a
    //   workgroup that waits for him -- makes the sum complete, and every workgroup derives the SAME threshold T from it (the
    //   boundary bin of top_n).  It then publishes only ITS keys >= T -- ~top_n / G of them instead of its local top_n, no
    //   narrowing pass of its own -- and takes a second ticket; the last one loads exactly the segment's ~1.3 x top_n keys >= T
    //   (one round trip: the first 2048 / G slots of every list are requested together with the lengths) into the sort
    //   buffer: no pass over ~G x top_n survivors.  (Publishing the lists SORTED and merging them by rank was built first: G
    //   binary searches per key are as many LDS steps as the merge sort's five levels -- 22 us for the ranking alone.)
    // tournament (rounds 3-4; the fall-back, taken when a slice could not be held whole, when the boundary bin holds more
    //   than the sort takes (2048 keys: plateaus), or when the barrier timed out -- other kernels may occupy the CUs a partner
    //   needs): each workgroup publishes its LOCAL top `publish` >= top_n keys (any key of the segment's top_n is in its
    //   slice's top_n); the last to arrive finds the threshold in the segment's histogram and fetches the survivors >= T.
    // Both routes are exact for any input and nobody waits without a bound.
    uint32_t n_mine = fetch(slice, 0ull, !has_raw, &h_lo);
    stamp2(2, part == 0);
    const bool whole = !has_raw && h_lo == 0ull;              // s_keys = EVERY key of the slice, s_hist = their first digit
    SelSeg &S = a.sel[seg];
    uint64_t *surv = a.surv + L.surv_off + static_cast<uint64_t>(b) * P * a.budget;
    if (!whole) {                                              // (rare) s_hist is a later digit / another range: redo the first digit
      const LdsFlat mine{s_keys, n_mine};
      hist_pass<Lds::copies, false>(mine, k_lo, k_hi, s_hist, s_range);
    }
    for (uint32_t i = tid; i < kRadixBins; i += kSelThreads) {
      uint32_t c = 0;
#pragma unroll
      for (int q = 0; q < Lds::copies; ++q) c += s_hist[i * Lds::copies + q];
      if (c) atomicAdd(&S.hist[i], c);
    }
    const bool coop_try = CAP == kSortCap && a.coop_ticks != 0 && !has_raw && sort_size <= 2u * kSelThreads;   // (block- AND segment-uniform)
    if (!whole && coop_try && tid == 0) atomicCAS(&S.route, 0u, kRouteTournament);   // no global threshold from a partial histogram
    // Ordering the protocol relies on: every access to SelSeg is an agent-scope ATOMIC (`sc1`: performed at the
    // device's coherence point, past this XCD's L2), relaxed in the C++ sense.  A wave's returning atomics are complete --
    // performed there, not merely issued -- once `s_waitcnt vmcnt(0)` retires; the workgroup barrier behind it makes that true
    // for all sixteen waves before thread 0 takes the ticket, and an atomic that a partner issues AFTER it has observed the ticket
    // (a sc1 load) is performed at the same point later.  So "ticket seen" implies "histogram contributions and the veto are
    // visible to sc1 loads" without a fence -- which on this part would write back and invalidate the XCD's whole L2 (40-90 us per
    // segment, measured in round 4).  The non-returning histogram atomics are covered by the same counter (vmcnt counts them
    // until the memory side acknowledges them on gfx9-family parts).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the histogram's atomics (and the veto) have been performed
    __syncthreads();
    if (tid == 0) {
      atomicAdd(&S.arrived, 1u);
      uint32_t route = kRouteTournament;
      if (coop_try) {
        const unsigned long long t0 = wall_clock64();
        bool all = false;
        for (int spin = 0; spin < (1 << 16); ++spin) {        // (bounded twice: by the clock and by the trip count)
          if (__hip_atomic_load(&S.arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= G) { all = true; break; }
          if (__hip_atomic_load(&S.route, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;   // somebody decided already
          if (wall_clock64() - t0 > a.coop_ticks) break;
          __builtin_amdgcn_s_sleep(2);
        }
        const uint32_t want = all ? kRouteCoop : kRouteTournament;
        const uint32_t prev = atomicCAS(&S.route, 0u, want);
        route = prev == 0u ? want : prev;                      // (kRouteCoop implies that all G histograms are in: its setter saw them)
      }
      s_misc[64] = route;
    }
    __syncthreads();
    stamp2(4, part == 0);
    uint32_t route = __builtin_amdgcn_readfirstlane(s_misc[64]);
    bool hist_clobbered = false;                               // s_hist no longer holds this slice's own first digit
    if (route == kRouteCoop) {
      hist_clobbered = true;
      // ---- the global threshold, the same in every workgroup of the segment ----
      for (uint32_t i = tid; i < kRadixBins; i += kSelThreads) {
        s_hist[i * Lds::copies] = __hip_atomic_load(&S.hist[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int q = 1; q < Lds::copies; ++q) s_hist[i * Lds::copies + q] = 0;
      }
      __syncthreads();
      SelState st{k_lo, k_hi, top_n, 0u, 0u};
      const uint32_t seg_total = advance_state<Lds::copies>(st, s_hist, s_misc, L.n, 0ull, ~0ull);
      const uint64_t T64 = seg_total <= top_n ? 0ull : st.lo;                 // fewer than top_n candidates: all of them
      // (bins [0, coop_bins) of the summed histogram -- still in s_hist when the keys are ordered -- count exactly the keys >= T64)
      coop_bins = seg_total <= top_n ? static_cast<uint32_t>(kRadixBins)
                                     : (kRadixBins - 1) - static_cast<uint32_t>((st.lo - k_lo) >> range_shift(k_lo, k_hi)) + 1;
      const uint32_t n_glob = seg_total <= top_n ? seg_total : st.taken + st.in_bin;   // #{keys of the segment >= T64}
      if (n_glob > 2u * kSelThreads) {
        route = kRouteTournament;                              // a plateau wider than the sort buffer's two keys per thread: every partner sees the same
      } else {
        // ---- my keys >= T, compacted in place and published as list `part` (unsorted: the finisher sorts the union) ----
        if (tid == 0) s_misc[20] = 0;
        for (uint32_t base = 0; base < n_mine; base += 4 * kSelThreads) {   // in-place compaction (narrow_in_lds's)
          uint64_t mine[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const uint32_t i = base + u * kSelThreads + tid;
            mine[u] = i < n_mine ? s_keys[i] : 0;
          }
          __syncthreads();
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const bool keep = mine[u] != 0 && mine[u] >= T64;
            const uint32_t slot = wave_append_slot(&s_misc[20], keep);
            if (keep) s_keys[slot] = mine[u];
          }
        }
        __syncthreads();
        const uint32_t n_g = __builtin_amdgcn_readfirstlane(s_misc[20]);   // (<= n_glob <= 2048)
        uint64_t *my_run = surv + static_cast<uint64_t>(part) * a.budget;
        for (uint32_t i = tid; i < n_g; i += kSelThreads) __hip_atomic_store(my_run + i, s_keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 0) __hip_atomic_store(&S.run_len[part], n_g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        stamp2(5, part == 0);
        if (tid == 0) s_misc[26] = atomicAdd(&S.arrived2, 1u);
        __syncthreads();
        stamp2(6, part == 0);
        if (s_misc[26] != G - 1) return;                       // (block-uniform) somebody else is last
        stamp2(8, true);
        // ---- the finisher: the G lists -- exactly the segment's keys >= T, n_glob <= 2048 of them -- into the sort buffer.
        // ONE round trip: slot p of list q is requested for every p below `spec` = 2048 / G together with the lengths (a list
        // longer than that -- a skewed segment -- takes a second, exact trip for its tail)
        uint32_t *s_len = s_cnt, *s_off = s_cnt + kMaxParts;   // (the sub-list lengths are no longer needed)
        const uint32_t spec = (2u * kSelThreads) / G;          // (G <= 64: >= 32)
        uint64_t early[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint32_t f = tid + h * kSelThreads, q = f / spec, p = f - q * spec;
          early[h] = q < G ? __hip_atomic_load(surv + static_cast<uint64_t>(q) * a.budget + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        }
        if (tid < G) s_len[tid] = __hip_atomic_load(&S.run_len[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (tid == 0) {
          uint32_t acc = 0;
          for (uint32_t q = 0; q < G; ++q) { s_off[q] = acc; acc += s_len[q]; }
          s_off[G] = acc;
        }
        __syncthreads();
        const uint32_t total = __builtin_amdgcn_readfirstlane(s_off[G]);      // (= n_glob)
        bool tails = false;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint32_t f = tid + h * kSelThreads, q = f / spec, p = f - q * spec;
          if (q < G) {
            const uint32_t len = s_len[q];
            if (p < len) s_keys[s_off[q] + p] = early[h];
            tails = tails || (p == 0 && len > spec);
          }
        }
        if (__syncthreads_or(tails ? 1 : 0)) {                 // (rare) the tails of the long lists
          for (uint32_t q = 0; q < G; ++q) {
            const uint32_t len = s_len[q];
            for (uint32_t p = spec + tid; p < len; p += kSelThreads)
              s_keys[s_off[q] + p] = __hip_atomic_load(surv + static_cast<uint64_t>(q) * a.budget + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          __syncthreads();
        }
        stamp2(9, true);
        stamp2(10, true);
        n_sort = total;                                        // (<= 2048: the standard sort below takes them as they are)
        coop_done = true;
      }
    }
    if (route != kRouteCoop) {
      const uint32_t publish = 2 * sort_size < a.budget ? 2 * sort_size : a.budget;   // >= top_n
      if (n_mine > publish && (hist_clobbered || !whole)) {   // narrow_in_lds reads s_hist as the first digit of s_keys over [h_lo | k_lo, k_hi]
        const LdsFlat mine{s_keys, n_mine};
        hist_pass<Lds::copies, false>(mine, h_lo > k_lo ? h_lo : k_lo, k_hi, s_hist, s_range);
      }
      uint32_t first_bins;
      n_mine = narrow_in_lds(n_mine, publish, h_lo, &first_bins);
      if (tid == 0) s_misc[25] = n_mine ? atomicAdd(&S.surv_count, n_mine) : 0u;
      __syncthreads();
      const uint32_t g0 = s_misc[25];
      // Publish: WRITE-THROUGH stores (agent-scope atomic stores: `sc1`), drained, then the ticket; the reader uses `sc1`
      // loads.  A release / acquire fence pair here (`__threadfence()`) writes back and invalidates the XCD's whole L2: measured
      // 40-90 us per segment with 2-8 workgroups taking part (profiles/r04_select_trace_fences.txt); MI355X_MICROARCH.md
      // "publish-large" prices the same choice at 8.2 vs 3.0 us.
      for (uint32_t i = tid; i < n_mine; i += kSelThreads)
        __hip_atomic_store(surv + g0 + i, s_keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      stamp2(5, part == 0);
      if (tid == 0) s_misc[26] = atomicAdd(&S.arrived2, 1u);
      __syncthreads();
      stamp2(6, part == 0);
      if (s_misc[26] != G - 1) return;                                     // (block-uniform) somebody else is last
      stamp2(8, true);
      // (the segment's histogram counts every key a slice held, not only the published ones: the threshold it gives has at
      //  least top_n keys at or above it, all of them among the top_n of their slices, i.e. published)
      if (tid == 0) s_misc[27] = __hip_atomic_load(&S.surv_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (uint32_t i = tid; i < kRadixBins; i += kSelThreads) {
        s_hist[i * Lds::copies] = __hip_atomic_load(&S.hist[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int q = 1; q < Lds::copies; ++q) s_hist[i * Lds::copies + q] = 0;
      }
      __syncthreads();
      const FlatSource all{surv, static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(s_misc[27]))};
      SelState st{k_lo, k_hi, top_n, 0u, 0u};
      advance_state<Lds::copies>(st, s_hist, s_misc, L.n, 0ull, ~0ull);
      stamp2(9, true);
      n_sort = fetch(all, all.count > sort_size ? st.lo : 0ull, true, &h_lo);
      stamp2(10, true);
    }
  }
  const uint32_t k_out = n_sort < top_n ? n_sort : top_n;                 // fewer than top_n candidates: all of them are here
  stamp(1);
  // Sorting is the expensive part, a histogram pass over keys that are already LDS-resident is cheap: cut the buffer down to
  // the smallest sortable size that still holds top_n (1024 for the default 1000) first.
  // (up to 2048 keys the rank-merge sort takes them as they are: two per thread)
  const uint32_t sort_limit = sort_size <= 2u * kSelThreads ? 2u * kSelThreads : sort_size;
  uint32_t hist_bins;   // s_hist still holds the first digit over [max(h_lo, k_lo), k_hi] and its bins [0, hist_bins) count exactly s_keys (0: not)
  n_sort = narrow_in_lds(n_sort, sort_limit, h_lo, &hist_bins);   // (cooperative route: <= 2048 keys, nothing to cut)
  if (coop_done) hist_bins = coop_bins;                  // (s_hist = the segment's summed histogram over [k_lo, k_hi]; h_lo is 0 there)
  stamp(2);
  if (a.trace && tid == 0) { a.trace[seg * 8 + 5] = n_total; a.trace[seg * 8 + 6] = n_sort; a.trace[seg * 8 + 7] = (static_cast<unsigned long long>(coop_done ? 1u : 0u) << 16) | (static_cast<unsigned long long>(G) << 1) | has_raw; }

  // ---- decode + write this segment's slice of the concatenated outputs ----
  const float stride = L.stride;
  const float lim_x = static_cast<float>(W) * stride - 1.0f;   // box.py:106  M = size*stride - 1
  const float lim_y = static_cast<float>(H) * stride - 1.0f;
  const typename T::storage *box_image = static_cast<const typename T::storage *>(L.box) + static_cast<uint64_t>(b) * A * NB * hw;
  const uint64_t out_row = static_cast<uint64_t>(b) * a.n_levels * top_n + static_cast<uint64_t>(l) * top_n;
  // slot t of the segment's list <- the candidate `key` (real) or the zero padding behind the last candidate
  auto emit = [&](uint64_t key, uint32_t t, bool real) {
    float score = 0.0f, cls = 0.0f;
    float bx[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) bx[k] = 0.0f;
    int32_t index = -1;
    if (real) {
      const uint32_t i = key_index(key);
      index = static_cast<int32_t>(i);
      const uint32_t pix = i % hw;
      const uint32_t x = pix % W, y = pix / W;
      const uint32_t c = (i / hw) % C;
      const uint32_t an = i / (hw * C);
      cls = static_cast<float>(c);
      if (!kLogits && sizeof(typename T::storage) == 4)
        // the key canonicalises -0.0 to +0.0 for ordering; emit the stored value itself
        score = load_raw<T>(cls_image, memory_offset(i, channels, hw, L.channels_last));
      else
        score = key_score(key);
      float d[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const uint64_t off = L.channels_last ? static_cast<uint64_t>(pix) * (A * NB) + an * NB + k
                                             : (static_cast<uint64_t>(an) * NB + k) * hw + pix;
        d[k] = load_raw<T>(box_image, off);
        if (L.box_bias) d[k] += L.box_bias[an * NB + k];                  // head bias folded in (fp32 add)
      }
      // box.py:302  grid = [x, y, x, y] * stride + anchors[a]
      const float *anc = L.anchors + 4 * an;
      const float fx = static_cast<float>(x) * stride, fy = static_cast<float>(y) * stride;
      const float ax1 = fx + anc[0], ay1 = fy + anc[1], ax2 = fx + anc[2], ay2 = fy + anc[3];
      // box.py:100-103
      const float w = ax2 - ax1 + 1.0f, h = ay2 - ay1 + 1.0f;
      const float cx = ax1 + 0.5f * w, cy = ay1 + 0.5f * h;
      const float pcx = d[0] * w + cx, pcy = d[1] * h + cy;
      const float pw = exp_cr(d[2]) * w, ph = exp_cr(d[3]) * h;
      // box.py:108-111
      bx[0] = clamp_like_torch(pcx - 0.5f * pw, lim_x);
      bx[1] = clamp_like_torch(pcy - 0.5f * ph, lim_y);
      bx[2] = clamp_like_torch(pcx + 0.5f * pw - 1.0f, lim_x);
      bx[3] = clamp_like_torch(pcy + 0.5f * ph - 1.0f, lim_y);
      if constexpr (NB == 6) { bx[4] = d[4]; bx[5] = d[5]; }   // sin, cos pass through (decode_rotate.cu:152-162)
    }
    a.out_scores[out_row + t] = score;
    a.out_classes[out_row + t] = cls;
#pragma unroll
    for (int k = 0; k < NB; ++k) a.out_boxes[(out_row + t) * NB + k] = bx[k];
    if (a.out_indices) a.out_indices[out_row + t] = index;
    return score;
  };

  // ---- order by COUNTING (round 6; VERDICT r05 #3: the sort was 8-10 us of every large segment, the decode behind it 4) ----
  // The keys' first digit -- 2048 equal bins over [max(h_lo, k_lo), k_hi] -- is still in s_hist from the selection.  A prefix
  // sum over the bins gives every bin its place in the list; a key's place inside its bin is the number of keys of the SAME bin
  // above it (keys are unique), a handful of LDS reads at realistic densities: no compare-exchange network, no merge levels.
  // And nobody needs the sorted array: the thread that holds a key knows its rank and decodes it straight into its slot.
  // Exact for any input: bins that hold more than kMaxInBin keys (plateaus of equal 16-bit scores are split on their index bits
  // only by later digits) or a histogram that does not describe the buffer any more (those later digits) take the rank-merge
  // sort below, as before.
  bool ranked = false;
  if constexpr (CAP == kSortCap) {
    if (a.rank_sort && hist_bins != 0 && n_sort != 0 && n_sort <= 2u * kSelThreads) {       // (block-uniform)
      const uint64_t r_lo = h_lo > k_lo ? h_lo : k_lo;
      const int sh = range_shift(r_lo, k_hi);
      uint32_t c0 = 0, c1 = 0;
#pragma unroll
      for (int q = 0; q < Lds::copies; ++q) {
        c0 += s_hist[(2 * tid) * Lds::copies + q];
        c1 += s_hist[(2 * tid + 1) * Lds::copies + q];
      }
      c0 = 2 * tid < hist_bins ? c0 : 0u;
      c1 = 2 * tid + 1 < hist_bins ? c1 : 0u;
      const uint32_t inc = wave_inclusive_sum_dpp(c0 + c1);
      uint32_t mx = c0 > c1 ? c0 : c1;
      uint32_t sq = (c0 > kMaxInBin ? kMaxInBinSquares : c0 * c0) + (c1 > kMaxInBin ? kMaxInBinSquares : c1 * c1);   // (no overflow)
#pragma unroll
      for (int dlt = 32; dlt > 0; dlt >>= 1) {
        const uint32_t o = __shfl_xor(mx, dlt, kWave);
        mx = o > mx ? o : mx;
        sq += __shfl_xor(sq, dlt, kWave);
        sq = sq > 4u * kMaxInBinSquares ? 4u * kMaxInBinSquares : sq;
      }
      const int wv = tid >> 6;
      if (lane_id() == kWave - 1) s_misc[wv] = inc;
      if (lane_id() == 0) { s_misc[32 + wv] = mx; s_misc[48 + wv] = sq; }
      __syncthreads();                                       // every thread has read its bins: s_hist may be rewritten
      uint32_t woff = 0, all = 0, worst = 0, squares = 0;
      for (int i = 0; i < kSelWaves; ++i) {
        const uint32_t tt = s_misc[i];
        woff += i < wv ? tt : 0u;
        all += tt;
        worst = s_misc[32 + i] > worst ? s_misc[32 + i] : worst;
        squares += s_misc[48 + i];
      }
      all = __builtin_amdgcn_readfirstlane(all);
      worst = __builtin_amdgcn_readfirstlane(worst);
      squares = __builtin_amdgcn_readfirstlane(squares);
      if (all == n_sort && worst <= kMaxInBin && squares <= kMaxInBinSquares) {   // (block-uniform) the histogram IS the buffer's, no wide plateau
        ranked = true;
        uint32_t *s_base = s_hist, *s_cur = s_hist + kRadixBins;          // bin -> first slot | keys placed so far (= its count, in the end)
        uint64_t *s_grp = s_keys + 2 * kSelThreads;                      // the keys grouped by bin (second half of the sort buffer)
        const uint32_t excl = woff + inc - (c0 + c1);
        s_base[2 * tid] = excl;
        s_base[2 * tid + 1] = excl + c0;
        s_cur[2 * tid] = 0;
        s_cur[2 * tid + 1] = 0;
        __syncthreads();
        uint64_t key[2];
        uint32_t bin[2];
        bool have[2];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          const uint32_t i = tid + hh * kSelThreads;
          have[hh] = i < n_sort;
          key[hh] = have[hh] ? s_keys[i] : 0ull;
          bin[hh] = 0;
          if (have[hh]) {
            uint32_t digit = static_cast<uint32_t>((key[hh] - r_lo) >> sh);
            digit = digit > kRadixBins - 1 ? kRadixBins - 1 : digit;
            bin[hh] = (kRadixBins - 1) - digit;
            s_grp[s_base[bin[hh]] + atomicAdd(&s_cur[bin[hh]], 1u)] = key[hh];
          }
        }
        __syncthreads();
        stamp(3);
        uint32_t positives = 0;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          bool pos = false;
          if (have[hh]) {
            const uint32_t base = s_base[bin[hh]], cnt = s_cur[bin[hh]];
            uint32_t rank = base;
            for (uint32_t j = 0; j < cnt; j += 8) {          // eight independent LDS reads per trip (a one-read trip pays the LDS latency per key of the bin)
              uint64_t o[8];
#pragma unroll
              for (int u = 0; u < 8; ++u) o[u] = s_grp[base + (j + u < cnt ? j + u : cnt - 1)];
#pragma unroll
              for (int u = 0; u < 8; ++u) rank += (j + u < cnt && o[u] > key[hh]) ? 1u : 0u;
            }
            if (rank < k_out) pos = emit(key[hh], rank, true) > 0.0f;
          }
          positives += static_cast<uint32_t>(__popcll(__ballot(pos)));
        }
        if (a.run_valid && positives && lane_id() == 0) atomicAdd(&s_misc[22], positives);
        for (uint32_t t = k_out + tid; t < top_n; t += kSelThreads) emit(0ull, t, false);   // the zero padding behind the last candidate
      }
    }
  }
  if (!ranked) {
    const uint64_t *sorted = s_keys;                                       // the first k_out are the answer
    if (n_sort <= static_cast<uint32_t>(kSelThreads)) sorted = merge_sort_1024(s_keys, n_sort);
    else if (n_sort <= 2u * kSelThreads) sorted = merge_sort_2048(s_keys, n_sort);
    else sort_keys_desc<CAP>(s_keys, n_sort);
    stamp(3);
    for (uint32_t t = tid; t < top_n; t += kSelThreads) {
      const float score = emit(t < k_out ? sorted[t] : 0ull, t, t < k_out);
      if (a.run_valid) {                                                   // (block-uniform; the list is sorted: positives are a prefix)
        const uint64_t positive = __ballot(score > 0.0f);
        if (positive && lane_id() == 0) atomicAdd(&s_misc[22], static_cast<uint32_t>(__popcll(positive)));
      }
    }
  }
  if (a.run_valid) {
    __syncthreads();
    if (tid == 0) a.run_valid[static_cast<size_t>(b) * a.n_levels + l] = s_misc[22];
  }
  stamp(4);
}

}  // namespace odtk
