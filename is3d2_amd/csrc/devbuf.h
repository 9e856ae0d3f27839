// devbuf.h -- the one owner of each device resource in csrc, move-only, released by its destructor: DevBuf<T> of an
// allocation (hipMalloc / hipFree), DevStream of a stream and DevEvent of an event.  The buffers, streams and events of
// the engine, the device group, the sampler and the table sets are members of these types and function-local scratch
// is a local, so an early return releases what it made.
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

// a stream or an event: empty until create(flags) makes it on the current device (so a lazily made one stays lazy:
// `if (!s) s.create(...)`), destroyed by reset() or the destructor
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
class DevHandle {
 public:
  DevHandle() = default;
  DevHandle(DevHandle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  DevHandle& operator=(DevHandle&& o) noexcept {
    if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
    return *this;
  }
  ~DevHandle() { reset(); }

  hipError_t create(unsigned flags) {
    reset();
    return Create(&h_, flags);
  }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }
  H get() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }

 private:
  H h_ = nullptr;
};
using DevStream = DevHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;
using DevEvent = DevHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;   // flags hipEventDefault: a timing event

}  // namespace is3d
