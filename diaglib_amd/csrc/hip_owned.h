// Owners of the HIP engine's device buffers, pinned host buffers and events (hip_engine.hip only).
// reserve(count), in elements of T, is the only way to grow: nothing happens when count <= capacity(); otherwise the old block
// is released, the buffer is left EMPTY (null, capacity 0), the new block allocated and the capacity recorded after success
// -- a failed call can be repeated and nothing is released twice.  It does not synchronise: the caller waits for its stream
// first where queued work may use the old block.  The runtime calls come from `Api` (the unit test substitutes a fake).
#pragma once
#include <cstddef>
#include <utility>

struct HipApi;

template <class T, class Api = HipApi>
class DeviceBuffer {
  T* p_ = nullptr; size_t cap_ = 0;
public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept { swap(o); }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { DeviceBuffer t(std::move(o)); swap(t); return *this; }   // t takes the old block along
  ~DeviceBuffer() { reset(); }
  void swap(DeviceBuffer& o) { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
  void reset() { if (p_) (void)Api::free(p_); p_ = nullptr; cap_ = 0; }
  // flags = 0: plain device memory; otherwise the flags of an extended allocation (fine-grained, ...)
  typename Api::error_t reserve(size_t count, unsigned flags = 0)
  {
    if (count <= cap_) return Api::ok;
    reset();
    const typename Api::error_t e = Api::alloc((void**)&p_, sizeof(T) * count, flags);
    if (e != Api::ok) { p_ = nullptr; return e; }
    cap_ = count;
    return Api::ok;
  }
  size_t capacity() const { return cap_; }
  explicit operator bool() const { return p_ != nullptr; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }
};

// Pinned host memory, converts to the HOST pointer; mapped (the default), dev() is its device alias, re-derived at every regrow.
template <class T, class Api = HipApi>
class MappedHostBuffer {
  T* h_ = nullptr; T* d_ = nullptr; size_t cap_ = 0;
public:
  MappedHostBuffer() = default;
  MappedHostBuffer(MappedHostBuffer&& o) noexcept { swap(o); }
  MappedHostBuffer& operator=(MappedHostBuffer&& o) noexcept { MappedHostBuffer t(std::move(o)); swap(t); return *this; }
  ~MappedHostBuffer() { reset(); }
  void swap(MappedHostBuffer& o) { std::swap(h_, o.h_); std::swap(d_, o.d_); std::swap(cap_, o.cap_); }
  void reset() { if (h_) (void)Api::host_free(h_); h_ = nullptr; d_ = nullptr; cap_ = 0; }
  typename Api::error_t reserve(size_t count, bool mapped = true)
  {
    if (count <= cap_) return Api::ok;
    reset();
    typename Api::error_t e = Api::host_alloc((void**)&h_, sizeof(T) * count, mapped);
    if (e != Api::ok) { h_ = nullptr; return e; }
    if (mapped && (e = Api::host_alias((void**)&d_, h_)) != Api::ok) { reset(); return e; }
    cap_ = count;
    return Api::ok;
  }
  size_t capacity() const { return cap_; }
  T* dev() const { return d_; }
  explicit operator bool() const { return h_ != nullptr; }
  operator T*() const { return h_; }
  T* operator->() const { return h_; }
};

template <class Api = HipApi>
class BasicEvent {
  typename Api::event_t e_{};
public:
  BasicEvent() = default;
  BasicEvent(const BasicEvent&) = delete;
  BasicEvent& operator=(const BasicEvent&) = delete;
  ~BasicEvent() { if (e_) (void)Api::event_destroy(e_); }
  typename Api::error_t ensure(unsigned flags)     // create on first use
  {
    if (e_) return Api::ok;
    const typename Api::error_t e = Api::event_create(&e_, flags);
    if (e != Api::ok) e_ = typename Api::event_t{};
    return e;
  }
  explicit operator bool() const { return (bool)e_; }
  operator typename Api::event_t() const { return e_; }
};
using Event = BasicEvent<>;

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
struct HipApi {
  using error_t = hipError_t;
  using event_t = hipEvent_t;
  static constexpr hipError_t ok = hipSuccess;
  static hipError_t alloc(void** p, size_t bytes, unsigned flags) { return flags ? hipExtMallocWithFlags(p, bytes, flags) : hipMalloc(p, bytes); }
  static hipError_t free(void* p) { return hipFree(p); }
  static hipError_t host_alloc(void** p, size_t bytes, bool mapped) { return hipHostMalloc(p, bytes, mapped ? hipHostMallocMapped : hipHostMallocDefault); }
  static hipError_t host_free(void* p) { return hipHostFree(p); }
  static hipError_t host_alias(void** dev, void* host) { return hipHostGetDevicePointer(dev, host, 0); }
  static hipError_t event_create(hipEvent_t* e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
  static hipError_t event_destroy(hipEvent_t e) { return hipEventDestroy(e); }
};
#endif
