// device_pool.h -- the owner of a backend's device arrays (altro_handle::pool, WideBackend::pool).
// The arrays stay plain pointer members of the backend, so kernel argument lists read them as before; the pool remembers
// the ADDRESS of every member it has allocated for and frees, at release_all(), whatever each of them holds at that moment.
// A member is therefore allocated, reallocated and released here and nowhere else.  Host logic only: nothing synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

namespace altro {

struct DevicePool {
  std::vector<void**> slots;   // the registered members (of the heap object this pool is a member of)
  DevicePool() = default;
  DevicePool(const DevicePool&) = delete;              // (a copy would free the same members twice)
  DevicePool& operator=(const DevicePool&) = delete;

  template <class T>
  hipError_t release(T** slot) {
    void** s = reinterpret_cast<void**>(slot);
    const hipError_t e = *s ? hipFree(*s) : hipSuccess;
    if (e == hipSuccess) *s = nullptr;
    return e;
  }
  // *slot <- max(count, 1) elements, after what it held has been freed; zero-filled on stream `zero_on` unless the caller
  // overwrites the whole array at once (zero = false).  A failure leaves *slot null: every site that decides from a size
  // variable whether to come here also comes here when the pointer is null.
  template <class T>
  hipError_t alloc(T** slot, size_t count, hipStream_t zero_on, bool zero = true) {
    void** s = reinterpret_cast<void**>(slot);
    if (std::find(slots.begin(), slots.end(), s) == slots.end()) slots.push_back(s);   // before the hipMalloc: a bad_alloc leaks nothing
    hipError_t e = release(slot);
    if (e != hipSuccess) return e;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    if ((e = hipMalloc(s, bytes)) != hipSuccess) return e;
    return zero ? hipMemsetAsync(*s, 0, bytes, zero_on) : hipSuccess;
  }
  // grow-only buffers (staging, workspaces): at least `need` elements afterwards, contents not kept; *cap: what it holds
  template <class T>
  hipError_t reserve(T** slot, size_t* cap, size_t need) {
    if (need <= *cap && *slot) return hipSuccess;
    *cap = 0;
    const hipError_t e = alloc(slot, need, nullptr, false);
    if (e == hipSuccess) *cap = need;
    return e;
  }
  void release_all() {
    for (void** s : slots)
      if (*s) { hipFree(*s); *s = nullptr; }
  }
};

}  // namespace altro
