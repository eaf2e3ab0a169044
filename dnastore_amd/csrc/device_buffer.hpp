// Who owns device memory: DevBuf (one allocation that may grow), DevPool (allocations freed together), the rules by which
// buffers grow, and the one macro that turns a HIP error into DNAS_E_DEVICE.  Nothing here is device code.
// The memory itself comes from a policy (types Error, Stream; static ok, alloc, free, copyPrefix, upload, fill, readBack): DeviceMem and PinnedMem
// below, under hipcc only -- with a policy of its own a host program instantiates the same templates without HIP
// (tools/device_buffer_host_check.cpp).  Both are GuardedMem over the policy that makes the HIP calls: with DNAS_DEBUG_ALLOC=<byte>
// in the environment an allocation is filled with that byte and followed by a guard band that its free checks (a testing aid).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
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

// ---- the debug allocation mode ------------------------------------------------------------------------------------------------
// DNAS_DEBUG_ALLOC=<byte> (decimal or 0x.., 0 to 255; read at each allocation): a block is kGuardBytes longer than asked for, every
// byte of it holds <byte> when alloc returns, and free compares the kGuardBytes behind the caller's bytes with <byte> before the
// block goes back.  A kernel that reads memory nobody wrote then reads poison and not the allocator's zeros; one that stores a
// little past the end of its buffer is counted (dnas_debug_alloc_stats).  LDS and a DevBuf that is reused without growing are not
// refilled.
constexpr size_t kGuardBytes = 256;

struct GuardedBlock {
  size_t bytes;                           // what the caller asked for
  unsigned char byte;                     // what the block was filled with
};
struct GuardState {                       // one per process, shared by every policy
  std::mutex mutex;                       // blocks and the counters
  std::unordered_map<void*, GuardedBlock> blocks;
  std::atomic<size_t> alive{0};           // blocks.size(): what a free looks at before it takes the mutex
  int64_t made = 0, checked = 0, violations = 0, firstBytes = 0, firstOffset = 0;
};
inline GuardState& guardState() {
  static GuardState* const s = new GuardState;     // never destroyed: buffers of static lifetime are freed after any static here
  return *s;
}
// the fill byte, or -1 when the mode is off (the variable unset, or not a number from 0 to 255)
inline int debugAllocByte() {
  const char* s = getenv("DNAS_DEBUG_ALLOC");
  if (!s || !*s) return -1;
  char* end = nullptr;
  const long v = strtol(s, &end, 0);
  return (*end == 0 && v >= 0 && v <= 255) ? (int)v : -1;
}
// out: guarded allocations made, guarded frees checked, guard violations, the bytes of the first violated allocation, the offset
// of its first changed guard byte (both 0 without a violation)
inline void debugAllocStats(int64_t out[5], bool reset) {
  GuardState& g = guardState();
  std::lock_guard<std::mutex> lock(g.mutex);
  out[0] = g.made, out[1] = g.checked, out[2] = g.violations, out[3] = g.firstBytes, out[4] = g.firstOffset;
  if (reset) g.made = g.checked = g.violations = g.firstBytes = g.firstOffset = 0;
}

// Base plus the mode.  Beyond alloc and free, Base has fill(p, byte, bytes): every byte set when it returns, and
// readBack(host, p, bytes): what the device has finished writing there.
template <class Base>
struct GuardedMem : Base {
  static typename Base::Error alloc(void** p, size_t bytes) {
    const int byte = debugAllocByte();
    if (byte < 0) return Base::alloc(p, bytes);
    void* q = nullptr;
    typename Base::Error e = Base::alloc(&q, bytes + kGuardBytes);
    if (!Base::ok(e)) return e;
    e = Base::fill(q, byte, bytes + kGuardBytes);
    if (!Base::ok(e)) { Base::free(q); return e; }
    GuardState& g = guardState();
    {
      std::lock_guard<std::mutex> lock(g.mutex);
      g.blocks[q] = GuardedBlock{bytes, (unsigned char)byte};
      g.alive.store(g.blocks.size(), std::memory_order_relaxed);
      ++g.made;
    }
    *p = q;
    return e;
  }
  static void free(void* p) {
    GuardState& g = guardState();
    if (g.alive.load(std::memory_order_relaxed) != 0) check(g, p);
    Base::free(p);
  }

 private:
  static void check(GuardState& g, void* p) {
    GuardedBlock block;
    {
      std::lock_guard<std::mutex> lock(g.mutex);
      const auto it = g.blocks.find(p);
      if (it == g.blocks.end()) return;                  // allocated with the mode off
      block = it->second;
      g.blocks.erase(it);
      g.alive.store(g.blocks.size(), std::memory_order_relaxed);
    }
    unsigned char guard[kGuardBytes];
    size_t bad = 0;                                      // the first changed byte; a band that cannot be read counts as changed at 0
    if (Base::ok(Base::readBack(guard, (const char*)p + block.bytes, kGuardBytes)))
      while (bad < kGuardBytes && guard[bad] == block.byte) ++bad;
    std::lock_guard<std::mutex> lock(g.mutex);
    ++g.checked;
    if (bad < kGuardBytes && g.violations++ == 0) {
      g.firstBytes = (int64_t)block.bytes, g.firstOffset = (int64_t)bad;
      fprintf(stderr, "DNAS_DEBUG_ALLOC: a store past the end of an allocation of %zu bytes, the first at byte %zu behind it\n", block.bytes, bad);
    }
  }
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
  // (the debug allocation mode) the library's streams are non-blocking: nothing orders them against the null stream but a
  // device-wide synchronise, after the fill and before the guard band is read
  static hipError_t readBack(void* host, const void* src, size_t bytes) {
    const hipError_t e = hipDeviceSynchronize();
    return e == hipSuccess ? hipMemcpy(host, src, bytes, hipMemcpyDefault) : e;
  }
};
struct HipDeviceMem : HipMemBase {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
  static hipError_t fill(void* p, int byte, size_t bytes) {
    const hipError_t e = hipMemset(p, byte, bytes);
    return e == hipSuccess ? hipDeviceSynchronize() : e;
  }
};
struct HipPinnedMem : HipMemBase {  // host memory the device reads and writes: asynchronous copies stay asynchronous
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void* p) { (void)hipHostFree(p); }
  static hipError_t fill(void* p, int byte, size_t bytes) { memset(p, byte, bytes); return hipSuccess; }
};
struct DeviceMem : GuardedMem<HipDeviceMem> {};
struct PinnedMem : GuardedMem<HipPinnedMem> {};
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
