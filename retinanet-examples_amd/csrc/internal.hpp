// internal.hpp -- the few host functions one source of libodtk_hip.so calls in another (hidden: not part of the ABI).
#pragma once
#include "runtime.hpp"

namespace odtk {
struct ScanArgs;
struct DecodeArgs;
}  // namespace odtk

#pragma GCC visibility push(hidden)

// decode_launch.hip, compiled once per head dtype (the 24 select_decode instantiations are most of the library's device code):
// the prefilter + select_decode launches of one decode call
template <typename T, bool kLogits>
int launch_decode(bool rotated, bool aligned, uint32_t scan_blocks, uint32_t sel_blocks, uint32_t sort_cap, size_t scan_lds,
                  const odtk::ScanArgs &sa, const odtk::DecodeArgs &da, hipStream_t stream);

// nms.hip; odtk_detect (decode.hip) runs it over decode's own output
int nms_impl(int batch, const void *const *inputs, void *const *outputs, int n_outputs, size_t count,
             int ndet, float thresh, uint32_t flags, void *workspace, size_t workspace_size, hipStream_t stream,
             uint32_t sorted_run_len = 0, const uint32_t *run_valid = nullptr);

#pragma GCC visibility pop
