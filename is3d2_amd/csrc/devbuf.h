// devbuf.h -- DevBuf<T>: the one owner of a device allocation (hipMalloc / hipFree), move-only, freed by its
// destructor.  The engine's buffers are members of this type and its function-local scratch is a local, so an early
// return frees what it allocated.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

namespace is3d {

template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~DevBuf() { reset(); }

  // room for n elements on the current device: a buffer that has it is kept; otherwise it is freed and max(n, 1)
  // elements are allocated (the contents are never copied).  false: the allocation failed and the buffer is empty
  bool reserve(long n) {
    if (cap_ >= n && p_) return true;
    reset();
    void* p = nullptr;
    if (hipMalloc(&p, (size_t)std::max(n, 1L) * sizeof(T)) != hipSuccess) return false;
    p_ = (T*)p;
    cap_ = n;
    return true;
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  T* get() const { return p_; }
  T* data() const { return p_; }
  long capacity() const { return cap_; }   // the n of the reserve that allocated (0: empty)

 private:
  T* p_ = nullptr;
  long cap_ = 0;
};

}  // namespace is3d
