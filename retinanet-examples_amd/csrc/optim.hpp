// optim.hpp -- the optimisation step of training on the device (odtk_optim_sgd_step, odtk_optim_grad_norm): SGD with momentum
// (dampening 0, no Nesterov) and weight decay, GradScaler's unscale and skip-on-overflow, the clip coefficient of a global gradient
// norm and the exponential moving average of the weights in ONE streaming pass over the parameters; the norm is one more pass over
// the gradients.  The definition -- the contract -- restated in torch in odtk/optim.py (FusedSGD._step_reference) and in numpy in
// tests/optim_ref.py, one float32 operation per rounding (the library is built with -ffp-contract=off):
//
//   skipped (nothing is written) when *found_inf != 0 or the norm state's skip word is set; otherwise, per element
//     g = grad;  g = g / *grad_scale (if given);  g = g * coef (if a norm state is given);  g = g + wd * p (if wd != 0)
//     buf = first ? g : (momentum * buf) + g;   p = p - (lr * buf);   e = e + one_minus_decay * (p - e) (if the tensor has an EMA)
//
// Launch shape: a tensor list of up to ODTK_MAX_OPTIM_TENSORS descriptors travels BY VALUE in the kernel arguments (2.9 KiB with
// the prefix table), nothing is uploaded, so the calls are hipGraph-capturable.  A workgroup of kOptimThreads lanes owns one chunk
// of ODTK_OPTIM_CHUNK consecutive elements of ONE tensor and finds it by a binary search of its own index in the prefix table
// (the index is wave-uniform: the table and the descriptor are read through scalar loads, never copied).  A lane owns four
// vectors of four elements, one workgroup-width apart; all of them are 16-byte accesses when every pointer of the tensor is
// 16-byte aligned (the host decides, one bit per tensor) and element accesses otherwise -- a view into a gradient bucket is only
// 4-byte aligned.  The arithmetic per element is the same code either way: the same bits.  No LDS in the step, no atomics, no
// scratch.
//
// The norm: per element g' = g / *grad_scale in float32 (the value the step will use), double(g') * double(g') is exact in double;
// the squares are added in double in one fixed order -- a lane's sixteen elements in index order, the wave's lanes by the xor
// tree, the waves of the workgroup in order -- into the workgroup's slot of the workspace.  The finish launch is one workgroup:
// lane t adds the slots t, t + kOptimFinishThreads, ... in index order, then the same tree; norm = float(sqrt(sum)),
// coef = min(1, max_norm / (norm + 1e-6f)) in float32 (torch's clip_grad_norm_; a NaN stays a NaN), skip = the norm is not finite.
// The same bits on every run.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/odtk_hip.h"
#include "loss.hpp"   // block_sum

namespace odtk {

constexpr int kOptimThreads = 256;
constexpr int kOptimVectors = ODTK_OPTIM_CHUNK / (4 * kOptimThreads);   // vectors of four elements per lane
constexpr int kOptimFinishThreads = 1024;
static_assert(kOptimVectors * 4 * kOptimThreads == ODTK_OPTIM_CHUNK, "a chunk is a whole number of vectors per lane");

struct OptimState {        // the device state of odtk_optim_grad_norm: 16 bytes
  float norm, coef;
  uint32_t skip, pad_;
};

struct OptimArgs {
  odtk_optim_tensor_t t[ODTK_MAX_OPTIM_TENSORS];
  uint32_t block_begin[ODTK_MAX_OPTIM_TENSORS + 1];   // the workgroups of tensor i are [block_begin[i], block_begin[i + 1])
  uint32_t n_tensors;
  uint64_t vec_mask;        // bit i: every pointer of tensor i is 16-byte aligned
  float lr, momentum, wd, one_minus_decay;
  int32_t first, pad_;
  const float *grad_scale;  // device scalars, each may be null
  const float *found_inf;
  const OptimState *norm_state;
  double *slots;            // the norm: one sum per workgroup, at slots[blockIdx.x]
};

// the tensor of this workgroup: the last i with block_begin[i] <= blockIdx.x (empty tensors have empty ranges and are never found)
__device__ __forceinline__ uint32_t optim_tensor_of(const OptimArgs &a) {
  uint32_t lo = 0, hi = a.n_tensors;                  // invariant: block_begin[lo] <= blockIdx.x < block_begin[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.block_begin[mid] <= blockIdx.x) lo = mid; else hi = mid;
  }
  return lo;
}

struct OptimScalars {
  float scale, coef, lr, momentum, wd, omd;
  bool unscale, clip, decay, first;
};

__device__ __forceinline__ void optim_element(const OptimScalars &s, float g, float &p, float &buf, float &e, bool has_ema) {
  if (s.unscale) g = g / s.scale;
  if (s.clip) g = g * s.coef;
  if (s.decay) g = g + s.wd * p;
  buf = s.first ? g : (s.momentum * buf) + g;
  p = p - (s.lr * buf);
  if (has_ema) e = e + s.omd * (p - e);
}

__global__ __launch_bounds__(kOptimThreads) void optim_sgd_step_kernel(const OptimArgs a) {
  if (a.found_inf && *a.found_inf != 0.0f) return;
  if (a.norm_state && a.norm_state->skip) return;
  const uint32_t ti = optim_tensor_of(a);
  const int64_t base = static_cast<int64_t>(blockIdx.x - a.block_begin[ti]) * ODTK_OPTIM_CHUNK;
  const int64_t left = a.t[ti].numel - base;
  const uint32_t n = left < ODTK_OPTIM_CHUNK ? static_cast<uint32_t>(left) : ODTK_OPTIM_CHUNK;
  float *const p = a.t[ti].param + base;
  const float *const g = a.t[ti].grad + base;
  float *const m = a.t[ti].momentum + base;
  float *const ema = a.t[ti].ema ? a.t[ti].ema + base : nullptr;
  const bool has_ema = ema != nullptr;
  OptimScalars s;
  s.unscale = a.grad_scale != nullptr;
  s.scale = s.unscale ? *a.grad_scale : 1.0f;
  s.clip = a.norm_state != nullptr;
  s.coef = s.clip ? a.norm_state->coef : 1.0f;
  s.decay = a.wd != 0.0f;
  s.lr = a.lr; s.momentum = a.momentum; s.wd = a.wd; s.omd = a.one_minus_decay;
  s.first = a.first != 0;
  const bool vec = (a.vec_mask >> ti) & 1ull;
  if (vec) {
    float4 vg[kOptimVectors], vp[kOptimVectors], vm[kOptimVectors], ve[kOptimVectors];
#pragma unroll
    for (int k = 0; k < kOptimVectors; ++k) {                       // every load of the lane first
      const uint32_t i = (k * kOptimThreads + threadIdx.x) * 4u;
      if (i + 4u <= n) {
        vg[k] = *reinterpret_cast<const float4 *>(g + i);
        vp[k] = *reinterpret_cast<const float4 *>(p + i);
        if (!s.first) vm[k] = *reinterpret_cast<const float4 *>(m + i);
        if (has_ema) ve[k] = *reinterpret_cast<const float4 *>(ema + i);
      }
    }
#pragma unroll
    for (int k = 0; k < kOptimVectors; ++k) {
      const uint32_t i = (k * kOptimThreads + threadIdx.x) * 4u;
      if (i + 4u <= n) {
        if (s.first) vm[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!has_ema) ve[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        optim_element(s, vg[k].x, vp[k].x, vm[k].x, ve[k].x, has_ema);
        optim_element(s, vg[k].y, vp[k].y, vm[k].y, ve[k].y, has_ema);
        optim_element(s, vg[k].z, vp[k].z, vm[k].z, ve[k].z, has_ema);
        optim_element(s, vg[k].w, vp[k].w, vm[k].w, ve[k].w, has_ema);
        *reinterpret_cast<float4 *>(p + i) = vp[k];
        *reinterpret_cast<float4 *>(m + i) = vm[k];
        if (has_ema) *reinterpret_cast<float4 *>(ema + i) = ve[k];
      } else if (i < n) {                                           // the chunk's last, partial vector: element by element
        for (uint32_t j = i; j < n; ++j) {
          float pj = p[j], mj = s.first ? 0.0f : m[j], ej = has_ema ? ema[j] : 0.0f;
          optim_element(s, g[j], pj, mj, ej, has_ema);
          p[j] = pj;
          m[j] = mj;
          if (has_ema) ema[j] = ej;
        }
      }
    }
  } else {
    // element accesses, coalesced: lane t takes the elements t, t + kOptimThreads, ...
#pragma unroll 4
    for (uint32_t j = threadIdx.x; j < n; j += kOptimThreads) {
      float pj = p[j], mj = s.first ? 0.0f : m[j], ej = has_ema ? ema[j] : 0.0f;
      optim_element(s, g[j], pj, mj, ej, has_ema);
      p[j] = pj;
      m[j] = mj;
      if (has_ema) ema[j] = ej;
    }
  }
}

// The norm's walk: the same chunks; only `grad` and `numel` of a descriptor are read.  A lane adds its elements in the order of the
// vector form (vector k = 0.., then the four elements) whichever form loads them, so the sum does not depend on the alignment.
__global__ __launch_bounds__(kOptimThreads) void optim_grad_norm_kernel(const OptimArgs a) {
  __shared__ double s_red[kOptimThreads / kWave];
  const uint32_t ti = optim_tensor_of(a);
  const int64_t base = static_cast<int64_t>(blockIdx.x - a.block_begin[ti]) * ODTK_OPTIM_CHUNK;
  const int64_t left = a.t[ti].numel - base;
  const uint32_t n = left < ODTK_OPTIM_CHUNK ? static_cast<uint32_t>(left) : ODTK_OPTIM_CHUNK;
  const float *const g = a.t[ti].grad + base;
  const bool unscale = a.grad_scale != nullptr;
  const float scale = unscale ? *a.grad_scale : 1.0f;
  const bool vec = (a.vec_mask >> ti) & 1ull;
  float4 vg[kOptimVectors];
#pragma unroll
  for (int k = 0; k < kOptimVectors; ++k) {
    const uint32_t i = (k * kOptimThreads + threadIdx.x) * 4u;
    vg[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);                    // an element beyond the chunk counts as +0: its square adds nothing
    if (vec && i + 4u <= n) {
      vg[k] = *reinterpret_cast<const float4 *>(g + i);
    } else if (i < n) {
      vg[k].x = g[i];
      if (i + 1u < n) vg[k].y = g[i + 1u];
      if (i + 2u < n) vg[k].z = g[i + 2u];
      if (i + 3u < n) vg[k].w = g[i + 3u];
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < kOptimVectors; ++k) {
    float x = vg[k].x, y = vg[k].y, z = vg[k].z, w = vg[k].w;
    if (unscale) { x = x / scale; y = y / scale; z = z / scale; w = w / scale; }
    acc += static_cast<double>(x) * static_cast<double>(x);
    acc += static_cast<double>(y) * static_cast<double>(y);
    acc += static_cast<double>(z) * static_cast<double>(z);
    acc += static_cast<double>(w) * static_cast<double>(w);
  }
  const double r = block_sum(acc, s_red);
  if (threadIdx.x == 0) a.slots[blockIdx.x] = r;
}

struct OptimFinishArgs {
  const double *slots;
  uint32_t n_slots, pad_;
  float max_norm;
  OptimState *state;
};

__global__ __launch_bounds__(kOptimFinishThreads) void optim_grad_norm_finish_kernel(const OptimFinishArgs a) {
  __shared__ double s_red[kOptimFinishThreads / kWave];
  double acc = 0.0;
  for (uint32_t i = threadIdx.x; i < a.n_slots; i += kOptimFinishThreads) acc += a.slots[i];
  const double sum = block_sum(acc, s_red);
  if (threadIdx.x == 0) {
    const float norm = static_cast<float>(sqrt(sum));
    const float c = a.max_norm / (norm + 1e-6f);
    a.state->norm = norm;
    a.state->coef = (c != c) ? c : (c < 1.0f ? c : 1.0f);
    a.state->skip = (__float_as_uint(norm) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;   // inf or NaN
    a.state->pad_ = 0u;
  }
}

}  // namespace odtk
