// core.hip -- the one definition of the state runtime.hpp declares (error buffer, profiler, trace pointer, dynamic-LDS opt-ins)
// and the entry points over it: version, ABI sizes, last error, odtk_profile_*, odtk_debug_set_trace.
#include <cstdio>
#include <utility>

#include "runtime.hpp"

thread_local char g_last_error[256] = "";
unsigned long long *g_trace = nullptr;
Profiler g_prof;

int hip_fail(hipError_t e, const char *what) {
  std::snprintf(g_last_error, sizeof g_last_error, "%s: %s", what, hipGetErrorString(e));
  return ODTK_ERR_HIP;
}

int allow_dynamic_lds(const void *kernel, size_t bytes, const char *what) {
  static std::mutex mu;
  static std::vector<std::pair<const void *, int>> done;
  int device = 0;
  ODTK_HIP_TRY(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(mu);
  for (const auto &d : done)
    if (d.first == kernel && d.second == device) return ODTK_OK;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
  if (e != hipSuccess) return hip_fail(e, what);
  done.emplace_back(kernel, device);
  return ODTK_OK;
}

extern "C" {

const char *odtk_version(void) { return "odtk-hip 0.1 (gfx950)"; }

int odtk_abi_struct_size(int which) {
  switch (which) {
    case 0: return static_cast<int>(sizeof(odtk_level_t));
    case 1: return static_cast<int>(sizeof(odtk_snap_level_t));
    case 2: return static_cast<int>(sizeof(odtk_snap_rot_level_t));
    case 3: return static_cast<int>(sizeof(odtk_loss_level_t));
    case 5: return static_cast<int>(sizeof(odtk_image_t));
    case 6: return static_cast<int>(sizeof(odtk_augment_t));
    case 7: return static_cast<int>(sizeof(odtk_rotation_t));
    case 9: return static_cast<int>(sizeof(odtk_candidates_t));
    case 11: return static_cast<int>(sizeof(odtk_tile_t));
    case 14: return static_cast<int>(sizeof(odtk_mosaic_tile_t));
    case 15: return static_cast<int>(sizeof(odtk_mosaic_t));
    case 17: return static_cast<int>(sizeof(odtk_optim_tensor_t));
    default: return -1;
  }
}
const char *odtk_last_hip_error(void) { return g_last_error; }

int odtk_debug_set_trace(void *device_buffer) {
  g_trace = static_cast<unsigned long long *>(device_buffer);
  return ODTK_OK;
}

int odtk_profile_enable(int on) {
  std::lock_guard<std::mutex> lock(g_prof.mu);
  g_prof.on.store(on < 0 ? ~0u : static_cast<unsigned>(on), std::memory_order_relaxed);
  return ODTK_OK;
}

int odtk_profile_collect(double total_ms[ODTK_KERNEL_COUNT], int launches[ODTK_KERNEL_COUNT]) {
  if (!total_ms || !launches) return ODTK_ERR_INVALID;
  std::lock_guard<std::mutex> lock(g_prof.mu);
  for (int k = 0; k < ODTK_KERNEL_COUNT; ++k) {
    total_ms[k] = 0.0;
    launches[k] = 0;
    while (!g_prof.pending[k].empty()) {                    // an event pair leaves `pending` before anything can fail
      const EventPair ev = g_prof.pending[k].back();
      g_prof.pending[k].pop_back();
      g_prof.spare.push_back(ev);
      ODTK_HIP_TRY(hipEventSynchronize(ev.stop));
      float ms = 0.0f;
      ODTK_HIP_TRY(hipEventElapsedTime(&ms, ev.start, ev.stop));
      total_ms[k] += ms;
      ++launches[k];
    }
  }
  return ODTK_OK;
}

}  // extern "C"
