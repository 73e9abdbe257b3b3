// decode_launch.hip -- the prefilter + select_decode kernels of ONE head dtype: compiled three times,
// -DODTK_DECODE_T=F32 / BF16 / F16, so that the library's largest kernel family builds on three cores.
#include "internal.hpp"
#include "prefilter.hpp"
#include "select_decode.hpp"

template <typename T, bool kLogits>
int launch_decode(bool rotated, bool aligned, uint32_t scan_blocks, uint32_t sel_blocks, uint32_t sort_cap, size_t scan_lds,
                  const odtk::ScanArgs &sa, const odtk::DecodeArgs &da, hipStream_t stream) {
  if (aligned)
    timed_launch(ODTK_KERNEL_PREFILTER, odtk::prefilter_scan_kernel<T, kLogits, true>, dim3(scan_blocks), dim3(odtk::kScanThreads), scan_lds, stream, sa);
  else
    timed_launch(ODTK_KERNEL_PREFILTER, odtk::prefilter_scan_kernel<T, kLogits, false>, dim3(scan_blocks), dim3(odtk::kScanThreads), scan_lds, stream, sa);
  ODTK_HIP_TRY(hipGetLastError());
  // select_decode's LDS (sort buffer, sub-histograms, sub-list lengths) is one dynamic allocation above the 64 KiB a kernel
  // gets by default: every variant opts in, once per device.  top_n > 4096 (the reference has no cap): the variant with a
  // 128 KiB sort buffer.
#define ODTK_SELECT_LAUNCH(NB_, CAP_)                                                                                          \
  do {                                                                                                                         \
    const int rc_ = allow_dynamic_lds(reinterpret_cast<const void *>(&odtk::select_decode_kernel<NB_, T, kLogits, CAP_>),       \
                                      odtk::SelLds<CAP_>::total, "hipFuncSetAttribute(select_decode_kernel)");                 \
    if (rc_ != ODTK_OK) return rc_;                                                                                            \
    timed_launch(ODTK_KERNEL_SELECT, odtk::select_decode_kernel<NB_, T, kLogits, CAP_>, dim3(sel_blocks), dim3(odtk::kSelThreads), \
                 odtk::SelLds<CAP_>::total, stream, da);                                                                       \
  } while (0)
  if (sort_cap > static_cast<uint32_t>(odtk::kSortCap)) {
    if (rotated) ODTK_SELECT_LAUNCH(6, odtk::kSortCapBig); else ODTK_SELECT_LAUNCH(4, odtk::kSortCapBig);
  } else {
    if (rotated) ODTK_SELECT_LAUNCH(6, odtk::kSortCap); else ODTK_SELECT_LAUNCH(4, odtk::kSortCap);
  }
#undef ODTK_SELECT_LAUNCH
  ODTK_HIP_TRY(hipGetLastError());
  return ODTK_OK;
}

#define ODTK_DECODE_INSTANCE(LOGITS_)                                                                                   \
  template int launch_decode<odtk::ODTK_DECODE_T, LOGITS_>(bool, bool, uint32_t, uint32_t, uint32_t, size_t, const odtk::ScanArgs &, \
                                                           const odtk::DecodeArgs &, hipStream_t)
ODTK_DECODE_INSTANCE(true);
ODTK_DECODE_INSTANCE(false);
