// bmpow_own.h -- move-only owners of the host library's device buffers, pinned buffers and events.
//
// Each records the device it was made for and releases there, so a tear-down never depends on what the
// shard set looks like by then.  The runtime's calls sit behind a traits parameter (an allocate and a free
// function), defaulted to the HIP one, so tests/native/own_sim.cpp instantiates the same template over a
// counting stand-in on the CPU.
//
// A wiping owner (WipeBuf; Owned<Api, true>) holds secrets: a private key, a nonce, a derived key, plaintext.
// It zeroes its whole capacity on its own device (the traits' zero function) right before every release --
// destruction, reset, a second alloc, a grow that reallocates, move-assignment over a live buffer -- so no
// list of buffers to wipe is kept by hand anywhere.
#pragma once
#include <atomic>
#include <cstddef>
#include <utility>

namespace bmown {

// No HIP call during static destruction: bmpow_atexit sets this on every one of its return paths, after
// its own shutdown, and it runs before the library's statics are destroyed (it is registered after they
// are constructed).  From then on an owner forgets its buffer instead of freeing it: the runtime's own
// exit handlers may already have run when a static owner's destructor does.
inline std::atomic<bool> g_exiting{false};

template <class Api, bool Wipe = false>
class Owned {
 public:
  using err_t = typename Api::err_t;
  Owned() = default;
  Owned(Owned&& o) noexcept { take(o); }
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      reset();
      take(o);
    }
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }
  // Frees on the owner's device (which becomes the thread's current one, as in the free lists this
  // replaces).  hipFree / hipHostFree wait for the whole device: never call this, or let an owner die,
  // under the engine's mutex -- move it into the shard's retired list instead (engine_launch).
  void reset() {
    if (p_ && !g_exiting.load(std::memory_order_relaxed)) {
      if constexpr (Wipe) Api::zero(dev_, p_, bytes_);
      Api::free(dev_, p_);
    }
    p_ = d_ = nullptr;
    n_ = bytes_ = 0;
    dev_ = -1;
  }
  size_t cap() const { return n_; }  // elements
  int dev() const { return dev_; }
  explicit operator bool() const { return p_ != nullptr; }

 protected:
  err_t alloc_bytes(int dev, size_t n, size_t bytes, unsigned flags) {
    reset();
    const err_t e = Api::alloc(dev, bytes, flags, &p_, &d_);
    if (e != Api::ok) {
      p_ = d_ = nullptr;
      return e;
    }
    n_ = n;
    bytes_ = bytes;
    dev_ = dev;
    return e;
  }
  void take(Owned& o) {
    p_ = std::exchange(o.p_, nullptr);
    d_ = std::exchange(o.d_, nullptr);
    n_ = std::exchange(o.n_, 0);
    bytes_ = std::exchange(o.bytes_, 0);
    dev_ = std::exchange(o.dev_, -1);
  }
  void* p_ = nullptr;  // what is freed
  void* d_ = nullptr;  // the device's address of it (a mapped pinned buffer; else p_)
  size_t n_ = 0, bytes_ = 0;
  int dev_ = -1;
};

template <class T, class Api, bool Wipe = false>
class Buf : public Owned<Api, Wipe> {
 public:
  using err_t = typename Api::err_t;
  err_t alloc(int dev, size_t n, unsigned flags = 0) { return this->alloc_bytes(dev, n, n * sizeof(T), flags); }
  // Hold at least n elements: nothing happens below the capacity; else the old buffer is released and n
  // allocated (the caller's growth policy chose n).  A failure leaves the owner empty, capacity 0.
  err_t grow(int dev, size_t n, unsigned flags = 0) { return this->p_ && n <= this->n_ ? Api::ok : alloc(dev, n, flags); }
  T* get() const { return static_cast<T*>(this->p_); }
  T* dptr() const { return static_cast<T*>(this->d_); }  // as the device addresses it
  T& operator[](size_t i) const { return get()[i]; }
};

template <class T, class Api>
using WipeBuf = Buf<T, Api, true>;

}  // namespace bmown

#ifdef __HIP__  // the HIP binding (the host units, compiled as HIP); the CPU test stops above
#include <hip/hip_runtime.h>

namespace bmown {

struct HipDev {  // hipMalloc
  using err_t = hipError_t;
  static constexpr err_t ok = hipSuccess;
  static err_t alloc(int dev, size_t bytes, unsigned, void** p, void** d) {
    err_t e = hipSetDevice(dev);
    if (e == ok) e = hipMalloc(p, bytes);
    *d = *p;
    return e;
  }
  static void free(int dev, void* p) { (void)hipSetDevice(dev), (void)hipFree(p); }
  static void zero(int dev, void* p, size_t bytes) {
    if (hipSetDevice(dev) == hipSuccess) (void)hipMemset(p, 0, bytes);
  }
};

struct HipPin {  // hipHostMalloc(flags); a mapped allocation also yields the device's address
  using err_t = hipError_t;
  static constexpr err_t ok = hipSuccess;
  static err_t alloc(int dev, size_t bytes, unsigned flags, void** p, void** d) {
    err_t e = hipSetDevice(dev);
    if (e == ok) e = hipHostMalloc(p, bytes, flags);
    if (e == ok && (flags & hipHostMallocMapped) && (e = hipHostGetDevicePointer(d, *p, 0)) != ok) (void)hipHostFree(*p);
    return e;
  }
  static void free(int dev, void* p) { (void)hipSetDevice(dev), (void)hipHostFree(p); }
};

struct HipEvent {  // hipEventCreateWithFlags(flags)
  using err_t = hipError_t;
  static constexpr err_t ok = hipSuccess;
  static err_t alloc(int dev, size_t, unsigned flags, void** p, void** d) {
    err_t e = hipSetDevice(dev);
    if (e == ok) e = hipEventCreateWithFlags(reinterpret_cast<hipEvent_t*>(p), flags);
    *d = *p;
    return e;
  }
  static void free(int dev, void* p) { (void)hipSetDevice(dev), (void)hipEventDestroy(static_cast<hipEvent_t>(p)); }
};

template <class T> using DevBuf = Buf<T, HipDev>;
template <class T> using WipeDevBuf = WipeBuf<T, HipDev>;  // zeroed on the device before it is released
template <class T> using PinBuf = Buf<T, HipPin>;
class Event : public Owned<HipEvent> {
 public:
  hipError_t alloc(int dev, unsigned flags = hipEventDefault) { return alloc_bytes(dev, 1, 0, flags); }
  hipEvent_t get() const { return static_cast<hipEvent_t>(p_); }
};

}  // namespace bmown
#endif
