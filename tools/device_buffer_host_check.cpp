// The owners of device memory (csrc/device_buffer.hpp) over a malloc-backed policy that counts, as a program of its own for a
// sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o device_buffer_host_check tools/device_buffer_host_check.cpp
// The growth rules against their formulas, reserve / reserveKeep / assign and the pool with and without a failing allocation,
// moves, and at the end: as many frees as allocations, no pointer freed twice.  The whole scenario runs over the debug allocation
// mode's wrapper (GuardedMem) with DNAS_DEBUG_ALLOC unset, its call counts held to those of the bare policy; then the mode itself:
// the fill, the guard band and what a free reports.  Exit status 0: all held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "../dnastore_amd/csrc/device_buffer.hpp"

namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

// malloc and free, counted; the failAt-th allocation from now (1: the next one) fails
struct CountingBase {
  using Error = int;             // 0: fine
  using Stream = int;
  static inline long allocs = 0, frees = 0, doubleFrees = 0, copies = 0, failAt = 0;
  static inline size_t lastBytes = 0;
  static inline std::set<void*> live;
  static bool ok(int e) { return e == 0; }
  static int alloc(void** p, size_t bytes) {
    lastBytes = bytes;
    if (failAt > 0 && --failAt == 0) return 2;
    *p = std::malloc(bytes);
    ++allocs;
    live.insert(*p);
    return 0;
  }
  static void free(void* p) {
    if (!live.erase(p)) { ++doubleFrees; return; }
    ++frees;
    std::free(p);
  }
  static int copyPrefix(void* dst, const void* src, size_t bytes, int) {
    ++copies;
    std::memcpy(dst, src, bytes);
    return 0;
  }
  static int upload(void* dst, const void* src, size_t bytes) {
    std::memcpy(dst, src, bytes);
    return 0;
  }
  static inline long fills = 0, readBacks = 0, failFill = 0;
  static int fill(void* p, int byte, size_t bytes) {
    ++fills;
    if (failFill > 0 && --failFill == 0) return 3;
    std::memset(p, byte, bytes);
    return 0;
  }
  static int readBack(void* host, const void* src, size_t bytes) {
    ++readBacks;
    std::memcpy(host, src, bytes);
    return 0;
  }
};
struct CountingMem : dnas::GuardedMem<CountingBase> {};
using Buf = dnas::DevBuf<int32_t, CountingMem>;

void fill(Buf& b, int32_t from) {
  for (size_t i = 0; i < b.capacity(); ++i) b.get()[i] = from + (int32_t)i;
}

void growthRules() {
  using namespace dnas;
  const size_t needs[] = {0, 1, 255, 256, 257, ((size_t)1 << 31) * 64};
  for (size_t need : needs) {
    EXPECT(growQuarter256(need) == std::max<size_t>(need + need / 4, 256));
    EXPECT(growQuarter64(need) == need + need / 4 + 64);
    EXPECT(growExact(need) == need);
    for (size_t cap : {(size_t)0, need / 2, need, 2 * need + 3})
      EXPECT((size_t)clustererGrowTo((int64_t)need, (int64_t)cap) == std::max(need, 2 * cap));
    EXPECT(growQuarter256(need) >= need && growQuarter64(need) >= need);
  }
  static_assert(growQuarter256(0) == 256 && growQuarter256(256) == 320 && growQuarter64(0) == 64 && growExact(7) == 7, "constexpr");
  EXPECT(growQuarter256(((size_t)1 << 31) * 64) == ((size_t)5 << 35));         // 2^37 + 2^35: no overflow
  EXPECT(growQuarter64(((size_t)1 << 31) * 64) == ((size_t)5 << 35) + 64);
}

void reserve() {
  Buf b;
  EXPECT(b.get() == nullptr && b.capacity() == 0);
  long a0 = CountingMem::allocs, f0 = CountingMem::frees;
  EXPECT(CountingMem::ok(b.reserve(10, dnas::growQuarter256(10)).error));       // empty: allocates
  EXPECT(b.get() && b.capacity() == 256 && CountingMem::lastBytes == 256 * sizeof(int32_t) && CountingMem::allocs == a0 + 1);
  fill(b, 0);
  int32_t* const was = b.get();
  auto r = b.reserve(256, dnas::growQuarter256(256));                           // large enough: nothing happens
  EXPECT(CountingMem::ok(r.error) && r.bytes == 0 && b.get() == was && b.capacity() == 256 && CountingMem::allocs == a0 + 1 && CountingMem::frees == f0);
  EXPECT(b.get()[255] == 255);
  EXPECT(CountingMem::ok(b.reserve(0, 0).error) && b.get() == was);
  r = b.reserve(257, dnas::growQuarter64(257));                                 // too small: frees, then allocates
  EXPECT(CountingMem::ok(r.error) && r.bytes == (257 + 64 + 64) * sizeof(int32_t) && b.capacity() == 257 + 64 + 64);
  EXPECT(CountingMem::allocs == a0 + 2 && CountingMem::frees == f0 + 1);
  fill(b, 0);
  // an empty buffer asked for nothing still allocates (a byte at least), as the hand-written owners did
  Buf e;
  EXPECT(CountingMem::ok(e.reserve(0, dnas::growExact(0)).error) && e.get() && e.capacity() == 0 && CountingMem::lastBytes == sizeof(int32_t));
  EXPECT(CountingMem::ok(e.reserve(0, 0).error) && CountingMem::allocs == a0 + 3);
  // a failed allocation: empty, and the next call succeeds
  CountingMem::failAt = 1;
  r = b.reserve(1000, dnas::growExact(1000));
  EXPECT(!CountingMem::ok(r.error) && r.bytes == 1000 * sizeof(int32_t) && b.get() == nullptr && b.capacity() == 0);
  EXPECT(CountingMem::ok(b.reserve(1000, dnas::growExact(1000)).error) && b.get() && b.capacity() == 1000);
  fill(b, 0);
  // assign: always a new allocation of exactly max(n, 1)
  a0 = CountingMem::allocs, f0 = CountingMem::frees;
  EXPECT(CountingMem::ok(b.assign(5).error) && b.capacity() == 5 && CountingMem::lastBytes == 5 * sizeof(int32_t));
  EXPECT(CountingMem::ok(b.assign(5).error) && CountingMem::allocs == a0 + 2 && CountingMem::frees == f0 + 2);
  EXPECT(CountingMem::ok(b.assign(0).error) && b.get() && b.capacity() == 1 && CountingMem::lastBytes == sizeof(int32_t));
  CountingMem::failAt = 1;
  EXPECT(!CountingMem::ok(b.assign(9).error) && b.get() == nullptr && b.capacity() == 0);
  EXPECT(CountingMem::ok(b.assign(9).error) && b.capacity() == 9);
  fill(b, 0);
  b.reset();
  EXPECT(b.get() == nullptr && b.capacity() == 0);
  b.reset();
}

void reserveKeep() {
  using dnas::clustererGrowTo;
  Buf b;
  const long c0 = CountingMem::copies;
  EXPECT(CountingMem::ok(b.reserveKeep(8, (size_t)clustererGrowTo(8, 0), 0, 0).error) && b.capacity() == 8);   // empty: nothing to keep
  EXPECT(CountingMem::copies == c0);
  fill(b, 100);
  int32_t* was = b.get();
  EXPECT(CountingMem::ok(b.reserveKeep(8, (size_t)clustererGrowTo(8, 8), 8, 0).error) && b.get() == was);        // large enough
  // keep = 0: a new allocation, nothing copied
  EXPECT(CountingMem::ok(b.reserveKeep(9, (size_t)clustererGrowTo(9, (int64_t)b.capacity()), 0, 0).error));
  EXPECT(b.capacity() == 16 && CountingMem::copies == c0);
  fill(b, 200);
  // keep = capacity: every element of the old one, and only those, in front of the new one
  EXPECT(CountingMem::ok(b.reserveKeep(40, (size_t)clustererGrowTo(40, (int64_t)b.capacity()), 16, 0).error));
  EXPECT(b.capacity() == 40 && CountingMem::copies == c0 + 1);
  for (int i = 0; i < 16; ++i) EXPECT(b.get()[i] == 200 + i);
  for (size_t i = 16; i < 40; ++i) b.get()[i] = -1;                            // (writable up to the new capacity)
  // a failed allocation leaves the buffer as it was: pointer, capacity and contents
  was = b.get();
  const long f0 = CountingMem::frees;
  CountingMem::failAt = 1;
  auto r = b.reserveKeep(41, (size_t)clustererGrowTo(41, 40), 40, 0);
  EXPECT(!CountingMem::ok(r.error) && r.bytes == 80 * sizeof(int32_t) && b.get() == was && b.capacity() == 40 && CountingMem::frees == f0);
  for (int i = 0; i < 16; ++i) EXPECT(b.get()[i] == 200 + i);
  EXPECT(CountingMem::ok(b.reserveKeep(41, (size_t)clustererGrowTo(41, 40), 40, 0).error) && b.capacity() == 80 && b.get()[15] == 215 && b.get()[39] == -1);
}

void moves() {
  Buf a;
  EXPECT(CountingMem::ok(a.assign(4).error));
  fill(a, 7);
  int32_t* const p = a.get();
  Buf b(std::move(a));
  EXPECT(a.get() == nullptr && a.capacity() == 0 && b.get() == p && b.capacity() == 4 && b.get()[3] == 10);
  Buf c;
  EXPECT(CountingMem::ok(c.assign(2).error));
  const long f0 = CountingMem::frees;
  c = std::move(b);                                                            // what c held is freed
  EXPECT(b.get() == nullptr && b.capacity() == 0 && c.get() == p && c.capacity() == 4 && CountingMem::frees == f0 + 1);
  Buf& self = c;
  c = std::move(self);
  EXPECT(c.get() == p && c.capacity() == 4);
  EXPECT(CountingMem::ok(a.reserve(3, 3).error) && a.capacity() == 3);         // a moved-from buffer serves again
}

void pool() {
  const long a0 = CountingMem::allocs, f0 = CountingMem::frees;
  {
    dnas::DevPoolOf<CountingMem> pool;
    double* d = nullptr;
    int32_t* u = nullptr;
    char* none = nullptr;
    EXPECT(CountingMem::ok(pool.alloc(3, &d).error) && d && CountingMem::lastBytes == 3 * sizeof(double));
    d[2] = 1.5;
    const int32_t src[4] = {4, 3, 2, 1};
    EXPECT(CountingMem::ok(pool.upload(src, 4, &u).error) && u && u[0] == 4 && u[3] == 1);
    EXPECT(CountingMem::ok(pool.upload((const char*)nullptr, 0, &none).error) && none && CountingMem::lastBytes == 1);   // one element at least
    CountingMem::failAt = 1;
    int32_t* bad = nullptr;
    auto r = pool.alloc(100, &bad);
    EXPECT(!CountingMem::ok(r.error) && r.bytes == 400 && bad == nullptr);
    EXPECT(CountingMem::ok(pool.alloc(100, &bad).error) && bad);
    EXPECT(CountingMem::allocs == a0 + 4 && CountingMem::frees == f0);
  }
  EXPECT(CountingMem::frees == f0 + 4);
}

struct Stats {
  int64_t made, checked, violations, firstBytes, firstOffset;
};
Stats stats(bool reset = false) {
  int64_t o[5];
  dnas::debugAllocStats(o, reset);
  return Stats{o[0], o[1], o[2], o[3], o[4]};
}
size_t mapSize() {
  std::lock_guard<std::mutex> lock(dnas::guardState().mutex);
  return dnas::guardState().blocks.size();
}
bool allBytes(const void* p, size_t n, unsigned char byte) {
  for (size_t i = 0; i < n; ++i)
    if (((const unsigned char*)p)[i] != byte) return false;
  return true;
}

// DNAS_DEBUG_ALLOC=<byte>: the fill, the guard band, what free reports
void debugMode() {
  using dnas::kGuardBytes;
  using Bytes = dnas::DevBuf<unsigned char, CountingMem>;
  // how the variable reads
  for (const char* off : {"", "256", "-1", "0x100", "85x", "x"}) {
    setenv("DNAS_DEBUG_ALLOC", off, 1);
    EXPECT(dnas::debugAllocByte() == -1);
  }
  setenv("DNAS_DEBUG_ALLOC", "0", 1);
  EXPECT(dnas::debugAllocByte() == 0);
  setenv("DNAS_DEBUG_ALLOC", "255", 1);
  EXPECT(dnas::debugAllocByte() == 255);
  setenv("DNAS_DEBUG_ALLOC", "0x55", 1);
  EXPECT(dnas::debugAllocByte() == 0x55);
  EXPECT(mapSize() == 0 && stats(true).made == 0);
  const long a0 = CountingMem::allocs, f0 = CountingMem::frees;
  {
    // every byte of a new block, guard included, holds the fill byte; the base was asked for the guard as well
    Bytes b;
    EXPECT(CountingMem::ok(b.assign(100).error) && CountingMem::lastBytes == 100 + kGuardBytes && b.capacity() == 100);
    EXPECT(allBytes(b.get(), 100 + kGuardBytes, 0x55) && mapSize() == 1 && stats().made == 1);
    // reserveKeep keeps its prefix and leaves the rest filled
    for (int i = 0; i < 100; ++i) b.get()[i] = (unsigned char)i;
    EXPECT(CountingMem::ok(b.reserveKeep(300, 300, 40, 0).error) && b.capacity() == 300);
    for (int i = 0; i < 40; ++i) EXPECT(b.get()[i] == i);
    EXPECT(allBytes(b.get() + 40, 260 + kGuardBytes, 0x55) && mapSize() == 1);
    Stats s = stats();
    EXPECT(s.made == 2 && s.checked == 1 && s.violations == 0 && s.firstBytes == 0 && s.firstOffset == 0);
    // a failed allocation, and a failed fill, leave no entry in the map (and the second no block)
    CountingMem::failAt = 1;
    Bytes c;
    EXPECT(!CountingMem::ok(c.assign(10).error) && c.get() == nullptr && mapSize() == 1);
    CountingMem::failFill = 1;
    EXPECT(c.assign(10).error == 3 && c.get() == nullptr && mapSize() == 1 && CountingMem::allocs == CountingMem::frees + 1);
    EXPECT(stats().made == 2);
    // a store at p[bytes - 1] is the caller's own
    b.get()[299] = 0;
    b.reset();
    s = stats();
    EXPECT(s.checked == 2 && s.violations == 0 && mapSize() == 0);
    // p[bytes + 255]: the last guard byte
    EXPECT(CountingMem::ok(b.assign(77).error));
    b.get()[77 + 255] = 0x54;
    b.reset();
    s = stats();
    EXPECT(s.checked == 3 && s.violations == 1 && s.firstBytes == 77 && s.firstOffset == 255);
    // the first violation is the one remembered; the count goes on
    EXPECT(CountingMem::ok(b.assign(5).error));
    b.get()[5] = 0;
    b.reset();
    s = stats(true);
    EXPECT(s.checked == 4 && s.violations == 2 && s.firstBytes == 77 && s.firstOffset == 255);
    // p[bytes]: size and offset 0, in the pool and with another byte
    setenv("DNAS_DEBUG_ALLOC", "255", 1);
    {
      dnas::DevPoolOf<CountingMem> pool;
      double* d = nullptr;
      int32_t* u = nullptr;
      EXPECT(CountingMem::ok(pool.alloc(3, &d).error) && allBytes(d, 24 + kGuardBytes, 0xFF));
      const int32_t src[2] = {7, 8};
      EXPECT(CountingMem::ok(pool.upload(src, 2, &u).error) && u[0] == 7 && u[1] == 8 && allBytes(u + 2, kGuardBytes, 0xFF));
      ((unsigned char*)d)[24] = 0;
      EXPECT(stats().violations == 0);                                          // found at the free, not before
    }
    s = stats(true);
    EXPECT(s.made == 2 && s.checked == 2 && s.violations == 1 && s.firstBytes == 24 && s.firstOffset == 0 && mapSize() == 0);
    // allocated with the mode on, freed with it off: still checked; and the other way round: never looked up in vain
    Bytes on, off;
    EXPECT(CountingMem::ok(on.assign(9).error));
    unsetenv("DNAS_DEBUG_ALLOC");
    EXPECT(CountingMem::ok(off.assign(9).error) && CountingMem::lastBytes == 9 && mapSize() == 1);
    on.get()[9 + 3] = 1;
    off.reset();
    EXPECT(stats().checked == 0 && mapSize() == 1);
    on.reset();
    s = stats(true);
    EXPECT(s.made == 1 && s.checked == 1 && s.violations == 1 && s.firstBytes == 9 && s.firstOffset == 3 && mapSize() == 0);
    // moves free once
    setenv("DNAS_DEBUG_ALLOC", "0x55", 1);
    Bytes m;
    EXPECT(CountingMem::ok(m.assign(4).error));
    Bytes n(std::move(m));
    Bytes o;
    o = std::move(n);
    EXPECT(mapSize() == 1 && stats().checked == 0);
    m.reset();
    n.reset();
    EXPECT(mapSize() == 1 && stats().checked == 0);
    o.reset();
    s = stats(true);
    EXPECT(s.made == 1 && s.checked == 1 && s.violations == 0 && mapSize() == 0);
    unsetenv("DNAS_DEBUG_ALLOC");
  }
  EXPECT(CountingMem::allocs - a0 == CountingMem::frees - f0 && mapSize() == 0);
  EXPECT(dnas::guardState().alive.load() == 0);
}

}  // namespace

int main() {
  // the mode off: the scenario's calls are those of the policy alone (the figures of the program before the wrapper existed)
  unsetenv("DNAS_DEBUG_ALLOC");
  growthRules();
  reserve();
  reserveKeep();
  moves();
  pool();
  EXPECT(CountingMem::allocs == 19 && CountingMem::frees == 19 && CountingMem::copies == 2);
  EXPECT(CountingMem::fills == 0 && CountingMem::readBacks == 0 && mapSize() == 0 && stats().made == 0 && stats().checked == 0);
  debugMode();
  EXPECT(CountingMem::allocs == CountingMem::frees && CountingMem::live.empty());
  EXPECT(CountingMem::doubleFrees == 0);
  EXPECT(CountingMem::allocs > 0);
  if (failures) {
    std::fprintf(stderr, "device buffer host check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("device buffer host check: ok (%ld allocations, %ld frees)\n", CountingMem::allocs, CountingMem::frees);
  return 0;
}
