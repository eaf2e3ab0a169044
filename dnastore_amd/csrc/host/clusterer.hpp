// The bookkeeping of the persistent clusterer (include/dnastore_amd.h, dnas_clusterer_*; clusterer_kernels.hip): buffer growth,
// the cut of an add's row tiles into segments, the prefix over (column, segment) and the columns of a band.  Plain C++ over
// integers, so that a host program can run it under a sanitizer (tools/clusterer_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace dnas {

constexpr int64_t kClustererTile = 64;                   // rows and columns of a filter tile
constexpr int64_t kClustererMaxSegments = 65535;         // the grid's second dimension

// The capacity a buffer of capacity cap grows to when `needed` elements are wanted (needed > cap).
inline int64_t clustererGrowTo(int64_t needed, int64_t cap) { return std::max(needed, 2 * cap); }

// The pairs an add of nNew reads to a pool of n0 examines: every pair whose larger index is new.
inline int64_t clustererAddPairs(int64_t n0, int64_t nNew) { return nNew * n0 + nNew * (nNew - 1) / 2; }

// The filter grid of an add: column tile c holds the new reads n0 + 64 c ..; the row tiles of the pool (64 rows each, from read 0)
// pass by it up to the one that holds its last column, cut into `segments` runs of tilesPerSegment whole tiles.
struct ClustererGrid {
  int64_t n0 = 0, n1 = 0, colTiles = 0, rowTiles = 0, segments = 1, tilesPerSegment = 1;
  // the row tiles [first, end) of segment s of column tile c (empty when the column tile needs fewer)
  void rowTilesOf(int64_t c, int64_t s, int64_t* first, int64_t* end) const {
    const int64_t jLast = std::min(n0 + (c + 1) * kClustererTile, n1) - 1, need = jLast / kClustererTile + 1;
    *first = std::min(s * tilesPerSegment, need);
    *end = std::min(*first + tilesPerSegment, need);
  }
};

// n0 reads held, n1 after the add (n1 > n0).  The smallest segment count that makes the grid at least 2 x cus work-groups,
// at most one segment per row tile; forced > 0: that many segments (testing aid; may exceed the row tiles, the rest stay empty).
inline ClustererGrid clustererGrid(int64_t n0, int64_t n1, int64_t cus, int64_t forced) {
  ClustererGrid g;
  g.n0 = n0, g.n1 = n1;
  g.colTiles = (n1 - n0 + kClustererTile - 1) / kClustererTile;
  g.rowTiles = (n1 - 1) / kClustererTile + 1;
  int64_t s = (2 * std::max<int64_t>(cus, 1) + g.colTiles - 1) / g.colTiles;
  s = std::min(s, g.rowTiles);
  if (forced > 0) s = forced;
  g.tilesPerSegment = (g.rowTiles + s - 1) / s;
  if (forced <= 0) s = (g.rowTiles + g.tilesPerSegment - 1) / g.tilesPerSegment;   // no segment that is empty for every column
  g.segments = std::max<int64_t>(1, std::min(s, kClustererMaxSegments));
  g.tilesPerSegment = (g.rowTiles + g.segments - 1) / g.segments;
  return g;
}

// off[x] = count[0] + .. + count[x - 1], x <= count.size(): with count[jLocal * segments + s] the candidates of column jLocal in
// segment s, off is where each (column, segment) starts in the add's list, which is in (j, i) order.
inline std::vector<int64_t> clustererPrefix(const std::vector<int64_t>& count) {
  std::vector<int64_t> off(count.size() + 1, 0);
  for (size_t x = 0; x < count.size(); ++x) off[x + 1] = off[x] + count[x];
  return off;
}

// The columns (local indices) with candidates in the band [lo, hi) of the list, lo < hi <= off.back(): from the column of the
// last (column, segment) that starts at or before lo to the column of the last one that starts before hi, inclusive -> [first, end).
inline void clustererBandColumns(const std::vector<int64_t>& off, int64_t segments, int64_t lo, int64_t hi, int64_t* first, int64_t* end) {
  const int64_t xFirst = std::upper_bound(off.begin(), off.end(), lo) - off.begin() - 1;
  const int64_t xEnd = std::lower_bound(off.begin(), off.end(), hi) - off.begin();   // the first slot that starts at or after hi
  *first = xFirst / segments;
  *end = (xEnd - 1) / segments + 1;
}

}  // namespace dnas
