// mre_host.h -- what the two host units of the C ABI share (mre_api.cpp: the entry points that work on a handle;
// mre_stream_api.cpp: those that take a stream and no handle): error reporting, the device-pointer check and the
// overlap check of byte ranges.  Private to csrc/; no handle, no device model, no scheduler policy.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <utility>

#include "../../include/mre.h"

#define HIPCHK(x)                                                                       \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess)                                                               \
      return mre::fail(MRE_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));    \
  } while (0)

namespace mre {
int fail(int code, const std::string& msg);   // records msg for mre_last_error() (mre_api.cpp) and returns code
}  // namespace mre

inline bool is_device_ptr(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeDevice;
}

// A base (or null) and a length in bytes.  Whether a range of `outs` overlaps one of `ins`; a null or empty range
// overlaps nothing.  The callers' lengths cannot overflow: they state why.
typedef std::pair<const void*, size_t> ByteRange;
template <size_t I, size_t O>
static bool ranges_overlap(const ByteRange (&ins)[I], const ByteRange (&outs)[O]) {
  for (const auto& o : outs)
    for (const auto& i : ins) {
      if (!o.first || !i.first || !o.second || !i.second) continue;
      const uintptr_t o0 = (uintptr_t)o.first, i0 = (uintptr_t)i.first;
      if (o0 < i0 + i.second && i0 < o0 + o.second) return true;
    }
  return false;
}
