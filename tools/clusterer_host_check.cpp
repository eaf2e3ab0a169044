// The persistent clusterer's bookkeeping (csrc/host/clusterer.hpp) on made-up counts, as a program of its own for a sanitizer
// build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o clusterer_host_check tools/clusterer_host_check.cpp
// It walks pools of many sizes and batch cuts through the grid, a filter on the host that mirrors the kernels' indexing into
// buffers of exactly the size the handle allocates (std::vector::at, and the sanitizer behind it), the prefix over (column,
// segment), and the band bisection, and checks that every band's list is the (j, i) order of the candidates.  Exit status 0: all
// held.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>

#include "../dnastore_amd/csrc/host/clusterer.hpp"

namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

// Is (i, j) a candidate of the made-up pool: a hash of the pair, so that columns are full, empty and anything between.
bool candidate(int64_t i, int64_t j, unsigned density) {
  uint64_t x = (uint64_t)i * 0x9E3779B97F4A7C15ull ^ (uint64_t)j * 0xBF58476D1CE4E5B9ull;
  x ^= x >> 29;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 32;
  return (j % 7 == 3) ? true : (j % 5 == 1) ? false : (x % 100) < density;
}

// One add: the count pass, the prefix, and every band's emit pass, as the kernels index them.
void oneAdd(int64_t n0, int64_t n1, int64_t cus, int64_t forced, int64_t capPairs, unsigned density) {
  using namespace dnas;
  const ClustererGrid g = clustererGrid(n0, n1, cus, forced);
  const int64_t nNew = n1 - n0, T = kClustererTile;
  EXPECT(g.colTiles == (nNew + T - 1) / T && g.rowTiles == (n1 - 1) / T + 1);
  EXPECT(g.segments >= 1 && g.segments <= kClustererMaxSegments && g.tilesPerSegment >= 1);
  EXPECT(g.segments * g.tilesPerSegment >= g.rowTiles);
  if (forced > 0) EXPECT(g.segments == std::min(forced, kClustererMaxSegments));
  else EXPECT((g.segments - 1) * g.tilesPerSegment < g.rowTiles);   // no segment is empty for every column

  std::vector<int64_t> count((size_t)(nNew * g.segments), -1);
  std::vector<std::pair<int64_t, int64_t>> want;         // the candidates in (j, i) order
  for (int64_t c = 0; c < g.colTiles; ++c)
    for (int64_t s = 0; s < g.segments; ++s) {
      int64_t first, end;
      g.rowTilesOf(c, s, &first, &end);
      EXPECT(0 <= first && first <= end && end <= g.rowTiles);
      for (int64_t lane = 0; lane < T; ++lane) {
        const int64_t j = n0 + c * T + lane;
        if (j >= n1) continue;
        int64_t cnt = 0;
        for (int64_t tile = first; tile < end; ++tile)
          for (int64_t r = 0; r < T; ++r) cnt += tile * T + r < j && candidate(tile * T + r, j, density);
        count.at((size_t)((j - n0) * g.segments + s)) = cnt;
      }
    }
  for (int64_t x : count) EXPECT(x >= 0);                // every slot was written
  for (int64_t j = n0; j < n1; ++j)
    for (int64_t i = 0; i < j; ++i)
      if (candidate(i, j, density)) want.emplace_back(i, j);
  const std::vector<int64_t> off = clustererPrefix(count);
  EXPECT(off.size() == count.size() + 1 && off.back() == (int64_t)want.size());
  const int64_t total = off.back();
  EXPECT(clustererAddPairs(n0, nNew) == n1 * (n1 - 1) / 2 - n0 * (n0 - 1) / 2);
  if (total == 0) return;

  capPairs = std::min(std::max<int64_t>(capPairs, 1), total);
  for (int64_t lo = 0; lo < total; lo += capPairs) {
    const int64_t hi = std::min(total, lo + capPairs);
    int64_t colFirst, colEnd;
    clustererBandColumns(off, g.segments, lo, hi, &colFirst, &colEnd);
    EXPECT(0 <= colFirst && colFirst < colEnd && colEnd <= nNew);
    // the columns outside [colFirst, colEnd) hold nothing of the band
    EXPECT(off.at((size_t)(colFirst * g.segments)) <= lo && off.at((size_t)(colEnd * g.segments)) >= hi);
    const int64_t tileFirst = colFirst / T, tiles = (colEnd - 1) / T - tileFirst + 1;
    EXPECT(tileFirst + tiles <= g.colTiles);
    std::vector<std::pair<int64_t, int64_t>> list((size_t)(hi - lo), {-1, -1});
    for (int64_t c = tileFirst; c < tileFirst + tiles; ++c)
      for (int64_t s = 0; s < g.segments; ++s) {
        int64_t first, end;
        g.rowTilesOf(c, s, &first, &end);
        for (int64_t lane = 0; lane < T; ++lane) {
          const int64_t j = n0 + c * T + lane;
          if (j >= n1) continue;
          const int64_t slot = (j - n0) * g.segments + s;
          int64_t pos = off.at((size_t)slot);
          for (int64_t tile = first; tile < end; ++tile)
            for (int64_t r = 0; r < T; ++r) {
              const int64_t i = tile * T + r;
              if (!(i < j && candidate(i, j, density))) continue;
              if (pos >= lo && pos < hi) list.at((size_t)(pos - lo)) = {i, j};
              ++pos;
            }
          EXPECT(pos == off.at((size_t)slot + 1));
        }
      }
    for (int64_t q = lo; q < hi; ++q) EXPECT(list[(size_t)(q - lo)] == want[(size_t)q]);
  }
}

}  // namespace

int main() {
  using namespace dnas;
  // growth: the capacity covers what is needed, doubles at least, and a run of adds reallocates O(log) times
  int64_t cap = 0, grown = 0;
  for (int64_t needed = 1; needed < (int64_t)1 << 40; needed += needed / 3 + 1)
    if (needed > cap) {
      const int64_t to = clustererGrowTo(needed, cap);
      EXPECT(to >= needed && to >= 2 * cap);
      cap = to, ++grown;
    }
  EXPECT(grown <= 42);
  EXPECT(clustererGrowTo(((int64_t)1 << 31) * 64, (int64_t)1 << 36) == (int64_t)1 << 37);   // 2^31 reads x 64 words: no overflow

  // the grid at the sizes of record, and at the largest pool
  {
    const ClustererGrid g = clustererGrid(20000, 22000, 256, 0);
    EXPECT(g.colTiles == 32 && g.rowTiles == 344 && g.segments * g.colTiles >= 512 && g.segments <= 344);
    const ClustererGrid big = clustererGrid(((int64_t)1 << 31) - 2, ((int64_t)1 << 31) - 1, 256, 0);
    EXPECT(big.colTiles == 1 && big.segments == 512 && big.segments * big.tilesPerSegment >= big.rowTiles);
    const ClustererGrid one = clustererGrid(0, 1, 256, 0);
    EXPECT(one.colTiles == 1 && one.rowTiles == 1 && one.segments == 1);
    const ClustererGrid huge = clustererGrid(0, 100, 256, 1000000);
    EXPECT(huge.segments == kClustererMaxSegments && huge.tilesPerSegment == 1);
  }

  // pools cut into batches, every segment count and band size
  std::mt19937 rng(12345);
  const int64_t cuts[][6] = {{1, 63, 1, 2, 0, 0}, {63, 1, 64, 65, 64, 0}, {257, 0, 0, 0, 0, 0}, {1, 1, 1, 1, 1, 1}, {130, 5, 70, 0, 0, 0}};
  for (const auto& cut : cuts)
    for (const int64_t forced : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)6, (int64_t)9})
      for (const int64_t capPairs : {(int64_t)1, (int64_t)37, (int64_t)1 << 21})
        for (const unsigned density : {0u, 3u, 60u}) {
          int64_t n0 = 0;
          for (const int64_t b : cut) {
            if (b == 0) continue;
            if (capPairs == 1 && n0 + b > 140) { n0 += b; continue; }   // (a band per pair: small pools only)
            oneAdd(n0, n0 + b, (int64_t)(rng() % 8 + 1), forced, capPairs, density);
            n0 += b;
          }
        }
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::puts("clusterer host check: ok");
  return 0;
}
