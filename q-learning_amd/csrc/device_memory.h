// Owners of device and pinned host memory (internal).  Every allocation of the library lives in a DeviceBuffer or
// PinnedBuffer member or local; the four functions below (common.cpp) are the only callers of the HIP allocator.
#pragma once
#include <cstddef>

namespace qlx {

// Throw Error{QLX_E_OOM} (naming the byte count) when the device is out of memory, Error{QLX_E_HIP} on any other
// failure; either way the runtime's sticky error is cleared first, so the next launch check does not report it.
void* device_alloc(size_t bytes);
void device_free(void* p) noexcept;
void* pinned_alloc(size_t bytes);
void pinned_free(void* p) noexcept;

// `count` elements of device memory.  Move-only; converts to T* so launches and copies read as with a raw pointer
// (the deleted copy keeps a buffer from being passed into a kernel by value).
template <class T>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  explicit DeviceBuffer(size_t count) { alloc(count); }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~DeviceBuffer() { release(); }
  // requires an empty buffer (reset otherwise); count = 0 leaves it empty and calls nothing
  void alloc(size_t count) {
    if (count) p_ = static_cast<T*>(device_alloc(count * sizeof(T)));
    n_ = count;
  }
  // frees first, then allocates: peak memory stays one buffer, contents are lost, a failure leaves the buffer empty
  void reset(size_t count) { release(); alloc(count); }
  // grows only (by reset); does not synchronise: a caller whose stream may still use the old memory waits first
  void reserve(size_t count) { if (count > n_) reset(count); }
  void release() noexcept { if (p_) device_free(p_); p_ = nullptr; n_ = 0; }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  size_t bytes() const { return n_ * sizeof(T); }
  explicit operator bool() const { return p_ != nullptr; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// The same over pinned host memory.
template <class T>
class PinnedBuffer {
 public:
  PinnedBuffer() = default;
  explicit PinnedBuffer(size_t count) { alloc(count); }
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  PinnedBuffer(PinnedBuffer&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  PinnedBuffer& operator=(PinnedBuffer&& o) noexcept {
    if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~PinnedBuffer() { release(); }
  void alloc(size_t count) {
    if (count) p_ = static_cast<T*>(pinned_alloc(count * sizeof(T)));
    n_ = count;
  }
  void reset(size_t count) { release(); alloc(count); }
  void reserve(size_t count) { if (count > n_) reset(count); }
  void release() noexcept { if (p_) pinned_free(p_); p_ = nullptr; n_ = 0; }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  size_t bytes() const { return n_ * sizeof(T); }
  explicit operator bool() const { return p_ != nullptr; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

}  // namespace qlx
