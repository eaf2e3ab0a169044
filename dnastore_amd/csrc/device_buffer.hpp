// Who owns device memory: DevBuf (one allocation that may grow), DevPool (allocations freed together), the rules by which
// buffers grow, and the one macro that turns a HIP error into DNAS_E_DEVICE.  Nothing here is device code.
// The memory itself comes from a policy (types Error, Stream; static ok, alloc, free, copyPrefix, upload): DeviceMem and PinnedMem
// below, under hipcc only -- with a policy of its own a host program instantiates the same templates without HIP
// (tools/device_buffer_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "host/clusterer.hpp"

namespace dnas {

// ---- the growth rules: the elements to allocate when `need` are wanted and the buffer is too small ----------------------------
// buffers sized by a call's bases or symbols (the io copies of the host entry point, the both-strand bases and offsets, the
// winners' segment tables)
constexpr size_t growQuarter256(size_t need) { return need + need / 4 > 256 ? need + need / 4 : 256; }
// buffers with an entry per read (the io and both-strand per-read groups)
constexpr size_t growQuarter64(size_t need) { return need + need / 4 + 64; }
// everything sized by a plan that rarely changes: scheduling arrays, the pinned sync copies, the event log, segment tables, the
// forward-backward database and arenas, the consensus rounds
constexpr size_t growExact(size_t need) { return need; }
// the fourth rule, max(need, 2 x capacity), is the persistent clusterer's: clustererGrowTo (host/clusterer.hpp)

struct DeviceMem;

// what an allocating call answers: the policy's error and the bytes that were asked for
template <class Error>
struct AllocResult {
  Error error;
  size_t bytes;
};

// One allocation of `capacity()` elements (a byte at least), owned: freed with the object, on the device that is current then.
template <class T, class Mem = DeviceMem>
class DevBuf {
 public:
  using Result = AllocResult<typename Mem::Error>;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); }
    return *this;
  }
  ~DevBuf() { reset(); }                                 // (move-only: the moves above leave no implicit copies)
  T* get() const { return p_; }
  size_t capacity() const { return cap_; }
  void reset() { if (p_) Mem::free(p_); p_ = nullptr; cap_ = 0; }
  // Room for `need` elements: nothing happens when they fit an allocated buffer; otherwise what it held is freed and
  // `want` >= need elements are allocated.  After a failure the buffer is empty.
  Result reserve(size_t need, size_t want) {
    if (need <= cap_ && p_) return Result{typename Mem::Error{}, 0};
    reset();
    return allocate(&p_, &cap_, want);
  }
  // The same, but the first `keep` elements move to the new allocation before the old one is freed.  After a failure the
  // buffer is as it was.
  Result reserveKeep(size_t need, size_t want, size_t keep, typename Mem::Stream stream) {
    if (need <= cap_ && p_) return Result{typename Mem::Error{}, 0};
    DevBuf grown;
    Result r = allocate(&grown.p_, &grown.cap_, want);
    if (Mem::ok(r.error) && keep > 0 && p_) r.error = Mem::copyPrefix(grown.p_, p_, keep * sizeof(T), stream);
    if (Mem::ok(r.error)) *this = std::move(grown);
    return r;
  }
  // A buffer that is replaced whenever it is set up: free, then exactly max(n, 1) elements.
  Result assign(size_t n) {
    reset();
    return allocate(&p_, &cap_, std::max<size_t>(n, 1));
  }

 private:
  static Result allocate(T** p, size_t* cap, size_t want) {
    Result r{typename Mem::Error{}, std::max<size_t>(want, 1) * sizeof(T)};
    void* q = nullptr;
    r.error = Mem::alloc(&q, r.bytes);
    if (Mem::ok(r.error)) { *p = (T*)q; *cap = want; }
    return r;
  }
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// Allocations that live and die together (a model's tables, one run's buffers).
template <class Mem>
class DevPoolOf {
 public:
  using Result = AllocResult<typename Mem::Error>;
  DevPoolOf() = default;
  DevPoolOf(const DevPoolOf&) = delete;
  DevPoolOf& operator=(const DevPoolOf&) = delete;
  ~DevPoolOf() { reset(); }
  void reset() { for (void* q : mem_) Mem::free(q); mem_.clear(); }
  template <class T>
  Result alloc(size_t n, T** out) {                                    // max(n, 1) elements
    Result r{typename Mem::Error{}, std::max<size_t>(n, 1) * sizeof(T)};
    mem_.reserve(mem_.size() + 1);
    void* q = nullptr;
    r.error = Mem::alloc(&q, r.bytes);
    if (Mem::ok(r.error)) { mem_.push_back(q); *out = (T*)q; }
    return r;
  }
  template <class T>
  Result upload(const T* src, size_t n, T** out) {
    Result r = alloc(n, out);
    if (Mem::ok(r.error) && n) r.error = Mem::upload(*out, src, n * sizeof(T));
    return r;
  }

 private:
  std::vector<void*> mem_;
};

}  // namespace dnas

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#include <string>
#include "../../include/dnastore_amd.h"
#include "errors.hpp"

namespace dnas {

struct HipMemBase {
  using Error = hipError_t;          // alloc hands back the runtime's own error (the arena re-plans on hipErrorOutOfMemory)
  using Stream = hipStream_t;
  static bool ok(hipError_t e) { return e == hipSuccess; }
  static hipError_t copyPrefix(void* dst, const void* src, size_t bytes, hipStream_t stream) {
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream);
    return e == hipSuccess ? hipStreamSynchronize(stream) : e;
  }
  static hipError_t upload(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
};
struct DeviceMem : HipMemBase {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
};
struct PinnedMem : HipMemBase {     // host memory the device reads and writes: asynchronous copies stay asynchronous
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void* p) { (void)hipHostFree(p); }
};
using DevPool = DevPoolOf<DeviceMem>;

inline hipError_t hipErrorOf(hipError_t e) { return e; }
inline hipError_t hipErrorOf(const AllocResult<hipError_t>& r) { return r.error; }
inline std::string hipAskedFor(hipError_t) { return ""; }
inline std::string hipAskedFor(const AllocResult<hipError_t>& r) { return " (" + std::to_string(r.bytes) + " bytes)"; }

}  // namespace dnas

// A HIP call, or an allocating call of DevBuf / DevPool, inside a function that answers a DNAS_* status: on an error the
// function returns DNAS_E_DEVICE, the message naming the call (and the bytes an allocation asked for).  What the function has to
// undo then is undone by the destructors of its owners.
#define DNAS_HIP_TRY(expr)                                                                                                      \
  do {                                                                                                                          \
    const auto r_ = (expr);                                                                                                     \
    if (dnas::hipErrorOf(r_) != hipSuccess)                                                                                     \
      return dnas::fail(DNAS_E_DEVICE, std::string(#expr) + dnas::hipAskedFor(r_) + ": " + hipGetErrorString(dnas::hipErrorOf(r_))); \
  } while (0)
#endif
