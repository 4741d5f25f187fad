// Host-side owners of the handle's device and pinned memory, and of its side stream.  Four types and nothing else: no
// allocator, no pools.
// They know nothing of nlps_gpu or its error string: every acquiring call returns the hipError_t and the caller turns
// it into a message.  The views that kernels take by value (PView, NView, TileD ...) hold pointers BORROWED from these.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

// Move-only owner of one hipMalloc block of T.  Converts to the borrowed pointer, so launches and copies read as they
// did with raw members; what it cannot do is be copied, or forgotten when the handle is destroyed.
template <class T>
class DevBuf {
  T* p_ = nullptr;
  size_t n_ = 0;  // capacity in elements

 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) reset(), swap(o);
    return *this;
  }
  ~DevBuf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t size() const { return n_; }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr, n_ = 0;
  }
  void swap(DevBuf& o) noexcept { std::swap(p_, o.p_), std::swap(n_, o.n_); }

  // Grow-only, contents discarded when it grows: the old block goes first, and a failed allocation leaves {nullptr, 0}.
  // On an empty buffer this is a plain hipMalloc.
  hipError_t reserve(size_t n) {
    if (n <= n_) return hipSuccess;
    reset();
    const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    else n_ = n;
    return e;
  }
  // A fresh block of n zeroed elements (the buffer must be empty).
  hipError_t alloc_zeroed(size_t n) {
    const hipError_t e = reserve(n);
    // default stream, like the uploads that may follow: on the handle's stream a caller-provided NON-BLOCKING
    // stream (torch's are) could run this after them and wipe the upload
    return e != hipSuccess ? e : hipMemset(p_, 0, n * sizeof(T));
  }
};

// Owner of one hipHostMalloc block of n objects, with the address the device sees it at (nullptr if the runtime
// gives none).
template <class T>
class Pinned {
  T* p_ = nullptr;
  T* alias_ = nullptr;

 public:
  Pinned() = default;
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
  Pinned(Pinned&& o) noexcept { swap(o); }
  Pinned& operator=(Pinned&& o) noexcept {
    if (this != &o) reset(), swap(o);
    return *this;
  }
  ~Pinned() { reset(); }
  void reset() {
    if (p_) (void)hipHostFree(p_);
    p_ = alias_ = nullptr;
  }
  hipError_t alloc(size_t n = 1) {
    const hipError_t e = hipHostMalloc((void**)&p_, n * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) return p_ = nullptr, e;
    if (hipHostGetDevicePointer((void**)&alias_, p_, 0) != hipSuccess) {
      (void)hipGetLastError();
      alias_ = nullptr;
    }
    return hipSuccess;
  }
  void swap(Pinned& o) noexcept { std::swap(p_, o.p_), std::swap(alias_, o.alias_); }
  T* host() const { return p_; }
  T* alias() const { return alias_; }
};

// A pinned object that kernels write and the host reads after its own synchronise: through the device alias, or, where
// there is none, through a device copy that fetch() queues over before that synchronise.
template <class T>
class Mirrored {
  Pinned<T> pin_;
  DevBuf<T> dev_;  // the fallback, allocated only when the alias is missing
  size_t n_ = 0;

 public:
  hipError_t alloc(size_t n = 1) {
    const hipError_t e = pin_.alloc(n);
    if (e != hipSuccess) return e;
    n_ = n;
    if (pin_.alias()) return hipSuccess;
    const hipError_t ed = dev_.reserve(n);
    if (ed != hipSuccess) pin_.reset();  // (all or nothing: host() says whether there is a word to write)
    return ed;
  }
  T* host() const { return pin_.host(); }
  T* target() const { return pin_.alias() ? pin_.alias() : dev_.get(); }
  hipError_t fetch(hipStream_t s) const {  // never waits
    return pin_.alias() ? hipSuccess : hipMemcpyAsync(pin_.host(), dev_.get(), n_ * sizeof(T), hipMemcpyDeviceToHost, s);
  }
};

// Owner of one non-blocking stream and the two events (timing off) that fork work from another stream onto it and join
// it back: what is launched on stream() between fork(s) and join(s) runs behind everything queued on s before the
// fork and in front of everything queued on s after the join, and beside what s gets in between.
class SideStream {
  hipStream_t s_ = nullptr;
  hipEvent_t fork_ = nullptr, join_ = nullptr;

 public:
  SideStream() = default;
  SideStream(const SideStream&) = delete;
  SideStream& operator=(const SideStream&) = delete;
  SideStream(SideStream&& o) noexcept { swap(o); }
  SideStream& operator=(SideStream&& o) noexcept {  // (the reset waits for what the stream still runs)
    if (this != &o) reset(), swap(o);
    return *this;
  }
  ~SideStream() { reset(); }
  void reset() {
    if (s_) (void)hipStreamSynchronize(s_), (void)hipStreamDestroy(s_);
    if (fork_) (void)hipEventDestroy(fork_);
    if (join_) (void)hipEventDestroy(join_);
    s_ = nullptr, fork_ = join_ = nullptr;
  }
  hipError_t create() {
    hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&fork_, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&join_, hipEventDisableTiming);
    if (e != hipSuccess) reset();
    return e;
  }
  void swap(SideStream& o) noexcept { std::swap(s_, o.s_), std::swap(fork_, o.fork_), std::swap(join_, o.join_); }
  hipStream_t stream() const { return s_; }
  hipError_t fork(hipStream_t from) {
    const hipError_t e = hipEventRecord(fork_, from);
    return e != hipSuccess ? e : hipStreamWaitEvent(s_, fork_, 0);
  }
  hipError_t join(hipStream_t into) {
    const hipError_t e = hipEventRecord(join_, s_);
    return e != hipSuccess ? e : hipStreamWaitEvent(into, join_, 0);
  }
};
