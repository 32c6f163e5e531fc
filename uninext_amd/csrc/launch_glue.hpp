// Host code that every launcher of the library needs around its launch: the shared last-error slot, the status of the launch
// just made, the 16-byte alignment check of float4-accessed arguments, and grid / padding arithmetic.  Internal: host only,
// not part of the C ABI.  (The msda_fwd* / msda_bwd* kernels return raw HIP codes to msda_capi.hip's finish() instead.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

namespace msda {

// Writes `what` to the calling thread's last-error slot (msda_hip_last_error) and returns `code`.  Defined in msda_capi.hip.
int set_error(int code, const char* what);

// 0, or the HIP error `rc` with its text in the error slot
inline int launch_status(int rc) { return rc == 0 ? 0 : set_error(rc, hipGetErrorString((hipError_t)rc)); }
// the same for the thread's last HIP error (read and cleared): the status of the launches made since the last read
inline int launch_status() { return launch_status((int)hipGetLastError()); }

inline bool aligned16(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  return true;
}

template <typename T>
constexpr T ceil_div(T v, T m) { return (v + m - 1) / m; }
template <typename T>
constexpr T round_up(T v, T m) { return ceil_div(v, m) * m; }
// the parts of a workspace start 256 bytes apart
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace msda
