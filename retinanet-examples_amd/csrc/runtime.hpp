// runtime.hpp -- what more than one source of libodtk_hip.so uses on the host: the error state, the profiler (odtk_profile_*),
// the debug trace pointer, the opt-in to large dynamic LDS, workspace alignment and the dtype dispatch.  The state is DEFINED
// once, in core.hip; everything here has hidden visibility, so none of it joins the library's dynamic symbol table.
//
// Host side rules: validate, lay out the workspace, fill kernel-argument structs (level tables and
// anchors travel BY VALUE in the kernarg segment: nothing is uploaded, so calls are
// hipGraph-capturable), enqueue on the caller's stream, return.  No allocation, no host sync.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "../../include/odtk_hip.h"
#include "prefilter.hpp"   // element types F32 / BF16 / F16

#pragma GCC visibility push(hidden)

extern thread_local char g_last_error[256];
extern unsigned long long *g_trace;   // odtk_debug_set_trace

int hip_fail(hipError_t e, const char *what);
#define ODTK_HIP_TRY(expr)                                   \
  do {                                                       \
    hipError_t e_ = (expr);                                  \
    if (e_ != hipSuccess) return hip_fail(e_, #expr);        \
  } while (0)

// ---- measurement hooks (odtk_profile_*) ------------------------------------------------------
struct EventPair { hipEvent_t start, stop; };
struct Profiler {
  std::mutex mu;
  std::atomic<unsigned> on{0};   // bit k set: kernel id k is timed (read on every launch without the lock)
  std::vector<EventPair> pending[ODTK_KERNEL_COUNT];
  std::vector<EventPair> spare;
};
extern Profiler g_prof;
constexpr size_t kMaxPendingEvents = 1 << 16;

struct KernelTimer {   // RAII: records start now and stop at scope exit, on `stream`
  int id; hipStream_t stream; EventPair ev; bool active = false;
  KernelTimer(int id_, hipStream_t s) : id(id_), stream(s) {
    if (!((g_prof.on.load(std::memory_order_relaxed) >> id) & 1u)) return;
    std::lock_guard<std::mutex> lock(g_prof.mu);
    if (!((g_prof.on.load(std::memory_order_relaxed) >> id) & 1u) || g_prof.pending[id].size() >= kMaxPendingEvents) return;
    if (!g_prof.spare.empty()) { ev = g_prof.spare.back(); g_prof.spare.pop_back(); }
    else if (hipEventCreate(&ev.start) != hipSuccess || hipEventCreate(&ev.stop) != hipSuccess) return;
    active = hipEventRecord(ev.start, stream) == hipSuccess;
  }
  ~KernelTimer() {
    if (!active) return;
    (void)hipEventRecord(ev.stop, stream);
    std::lock_guard<std::mutex> lock(g_prof.mu);
    g_prof.pending[id].push_back(ev);
  }
};

// One kernel launch, timed when its id is enabled.  The event pair is handed to the launch itself
// (hipExtLaunchKernelGGL): start / stop then carry the timestamps of THIS dispatch's begin and end -- the same
// clock pair rocprofv3's kernel trace reports -- instead of two separate marker packets around it, which add the
// dispatch latency on both sides (measured: 57.9 vs 52.8 us for the same prefilter launches).
template <typename K, typename... Args>
void timed_launch(int id, K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args) {
  if ((g_prof.on.load(std::memory_order_relaxed) >> id) & 1u) {
    EventPair ev;
    bool ok = false;
    {
      std::lock_guard<std::mutex> lock(g_prof.mu);
      if (g_prof.pending[id].size() < kMaxPendingEvents) {
        if (!g_prof.spare.empty()) { ev = g_prof.spare.back(); g_prof.spare.pop_back(); ok = true; }
        else ok = hipEventCreate(&ev.start) == hipSuccess && hipEventCreate(&ev.stop) == hipSuccess;
      }
    }
    if (ok) {
      hipExtLaunchKernelGGL(kernel, grid, block, static_cast<uint32_t>(lds), stream, ev.start, ev.stop, 0, args...);
      std::lock_guard<std::mutex> lock(g_prof.mu);
      g_prof.pending[id].push_back(ev);
      return;
    }
  }
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
}

// Kernels that want more than 64 KiB of dynamic LDS opt in with hipFuncSetAttribute -- an attribute of the function ON
// THE CURRENT DEVICE, so it is set once per (kernel, device), not once per process (a process that drives several GPUs
// would otherwise launch on the second one without it).
int allow_dynamic_lds(const void *kernel, size_t bytes, const char *what);

constexpr size_t kAlign = 256;
inline size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

// f(odtk::F32{}), f(odtk::BF16{}) or f(odtk::F16{}) for a dtype the caller has validated.  An entry point that has no fp32
// form rejects ODTK_F32 first and branches on its two types itself: this helper would instantiate the third.
template <typename F>
auto dispatch_dtype(int dtype, F &&f) {
  if (dtype == ODTK_F32) return f(odtk::F32{});
  if (dtype == ODTK_BF16) return f(odtk::BF16{});
  return f(odtk::F16{});
}

#pragma GCC visibility pop
